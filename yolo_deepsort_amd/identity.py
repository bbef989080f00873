"""Cross-camera identities: one global id per person over the trackers of many cameras, kept on the device (csrc/identity.hip).

``IdentityMap`` is bound to an ordered list of trackers (stream = index).  ``update()`` gives every Confirmed track that holds no
global id one: the id of the person's live track in another camera when the trackers' own appearance metric says so (a linear
assignment per camera, the reference's min_cost_matching on the cross-camera distances), else a fresh one.  The rules are spelled
out at yds_identity_update in include/ydsort.h.

Limits: only LIVE holders are matched against - once the last track holding an id has died (its max_age coasting frames included)
that id is never handed out again; an id is held by at most one track per camera; an update admits new tracks while their gallery
rows sum to at most ``max_rows`` and defers the rest to the next update (``ids()`` shows them with 0).

Call ``update()`` between steps, like the searches of search.py; inside a pipeline use ``MultiStreamPipeline.set_identities``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

__all__ = ["IdentityMap", "MAX_ROWS"]

MAX_ROWS = 4096          # default admission limit = the search's query limit (search.MAX_QUERIES)
_UNKNOWN = object()


def check_trackers(deepsorts, max_rows):
    """DeepSort objects or bare tracker handles -> the tracker handles.  Everything that can be refused without the device is
    refused here with ValueError: no trackers, a foreign object, a euclidean tracker, nn_budget=None, a tracker given twice,
    max_rows below the largest nn_budget."""
    trackers = [getattr(d, "tracker", d) for d in deepsorts]
    if not trackers:
        raise ValueError("identity map: no trackers given")
    largest = 0
    for s, t in enumerate(trackers):
        if getattr(t, "_h", None) is None:
            raise ValueError("identity map: entry %d is no tracker of this package" % s)
        if getattr(t, "metric", "cosine") != "cosine":
            raise ValueError("identity map: tracker %d uses the euclidean metric; its gallery rows are not normalised" % s)
        budget = getattr(t, "nn_budget", _UNKNOWN)
        if budget is None:
            raise ValueError("identity map: tracker %d has nn_budget=None; the map needs galleries of a bounded size" % s)
        if budget is not _UNKNOWN:
            largest = max(largest, int(budget))
    if len({id(t) for t in trackers}) != len(trackers):
        raise ValueError("identity map: a tracker is given for more than one stream")
    if int(max_rows) < max(largest, 1):
        raise ValueError("identity map: max_rows = %d is below the largest nn_budget %d; a track with a full gallery could never "
                         "be admitted" % (int(max_rows), largest))
    return trackers


def resolve_max_dist(trackers, max_dist):
    if max_dist is None:
        max_dist = getattr(trackers[0], "max_dist", None)
        if max_dist is None:
            raise ValueError("identity map: max_dist=None needs a tracker that knows its matching threshold")
    max_dist = float(max_dist)
    if not (max_dist >= 0.0) or not np.isfinite(max_dist):
        raise ValueError("identity map: max_dist must be a finite value >= 0, got %r" % max_dist)
    return max_dist


class IdentityMap:
    """``IdentityMap(deepsorts, max_dist=None, max_rows=4096)``: global ids over the given trackers (DeepSort objects or their
    ``.tracker`` handles; cosine metric, finite nn_budget).  max_dist=None: the first tracker's matching threshold."""

    def __init__(self, deepsorts, max_dist=None, max_rows=MAX_ROWS):
        self._h = None
        self.trackers = check_trackers(list(deepsorts), max_rows)      # (kept: the map reads their device state)
        self.max_dist, self.max_rows = resolve_max_dist(self.trackers, max_dist), int(max_rows)
        self.n_streams = len(self.trackers)
        handles = (C.c_void_p * self.n_streams)(*[t._h for t in self.trackers])
        self._h = _lib.check_ptr(_lib.load().yds_identity_create(handles, self.n_streams, self.max_dist, self.max_rows))

    @property
    def handle(self):
        return self._h

    def update(self):
        """One update over the trackers' state as it stands (between steps).  Returns (linked, fresh, deferred)."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().yds_identity_update(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def last_counts(self):
        """(linked, fresh, deferred) of the last update, also of one that ran inside a pipeline step."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().yds_identity_last_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def ids(self, stream):
        """dict track_id -> global_id of the live Confirmed tracks of ``stream`` after the last update, in track-list order;
        0 = deferred.  From the host copy: no device work."""
        stream = int(stream)
        if stream < 0 or stream >= self.n_streams:
            raise ValueError("identity map: stream %d outside [0, %d)" % (stream, self.n_streams))
        return _read_ids(lambda t, g, cap, n: _lib.load().yds_identity_get(self._h, stream, t, g, cap, n))

    def last_links(self):
        """The tracks the last update linked: a list of (stream, track_id, global_id, cost), cost as the fp32 the device compared."""
        lib = _lib.load()
        n = C.c_int(0)
        lib.yds_identity_last_links(self._h, None, None, None, None, 0, C.byref(n))     # (asks for the count)
        cap = max(n.value, 1)
        s, t, g = (np.zeros(cap, np.int32) for _ in range(3))
        c = np.zeros(cap, np.float32)
        _lib.check(lib.yds_identity_last_links(self._h, _lib.ptr(s), _lib.ptr(t), _lib.ptr(g), _lib.ptr(c), cap, C.byref(n)))
        return [(int(s[k]), int(t[k]), int(g[k]), c[k]) for k in range(n.value)]

    def reset(self):
        """Forget every identity; the counter keeps counting, so ids handed out before are never seen again."""
        _lib.check(_lib.load().yds_identity_reset(self._h))

    def set_timing(self, on=True):
        _lib.check(_lib.load().yds_identity_set_timing(self._h, 1 if on else 0))

    def last_us(self):
        """Device time of the last update's resolve sequence in us (set_timing first); None when that update launched none."""
        us = C.c_float(0)
        _lib.check(_lib.load().yds_identity_last_us(self._h, C.byref(us)))
        return None if us.value < 0 else float(us.value)

    def __del__(self):
        try:
            if self._h:
                _lib.load().yds_identity_destroy(self._h)
                self._h = None
        except Exception:
            pass


def _read_ids(call):
    """call(track_id*, global_id*, cap, n*) of yds_identity_get / yds_pipeline_last_identities -> dict in track-list order."""
    n = C.c_int(0)
    call(None, None, 0, C.byref(n))                                                     # (asks for the count)
    cap = max(n.value, 1)
    t, g = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    _lib.check(call(_lib.ptr(t), _lib.ptr(g), cap, C.byref(n)))
    return {int(t[k]): int(g[k]) for k in range(n.value)}
