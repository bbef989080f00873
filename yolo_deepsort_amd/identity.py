"""Cross-camera identities: one global id per person over the trackers of many cameras, kept on the device (csrc/identity.hip).

``IdentityMap`` is bound to an ordered list of trackers (stream = index).  ``update()`` gives every Confirmed track that holds no
global id one: the id of the person's live track in another camera when the trackers' own appearance metric says so (a linear
assignment per camera, the reference's min_cost_matching on the cross-camera distances), else a fresh one.  The rules are spelled
out at yds_identity_update in include/ydsort.h.

Limits: without a memory only LIVE holders are matched against - once the last track holding an id has died (its max_age coasting
frames included) that id is never handed out again; an id is held by at most one track per camera; an update admits new tracks while
their gallery rows sum to at most ``max_rows`` and defers the rest to the next update (``ids()`` shows them with 0).

The memory (``memory_ids > 0``) lifts the first limit: a bank of ``memory_ids`` entries of ``memory_rows`` appearance rows each, kept on
the device and refreshed at every update with each holder's newest gallery row.  A person who left every camera is a DEPARTED id; a new
track that resembles it takes the old id back (``last_relinked()``).  ``memory_ttl`` (in updates, None = never) drops departed ids that
stayed away longer; a full bank evicts the departed id that was held longest ago.  ``enrol`` adds identities from rows given by the
caller (a watch list); ``memory()``, ``memory_rows()`` and ``enrol`` together are enough to keep a bank across runs.

Call ``update()`` between steps, like the searches of search.py; inside a pipeline use ``MultiStreamPipeline.set_identities``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

__all__ = ["IdentityMap", "MAX_ROWS"]

MAX_ROWS = 4096          # default admission limit = the search's query limit (search.MAX_QUERIES)
EMB = 512
MEMORY_ROWS = (1, 2, 4, 8, 16, 32)      # rows per remembered id: whole entries tile a 32-row matrix tile
MEMORY_IDS_MAX = 65536
MEMORY_COUNTS = ("entries", "departed", "relinked", "remembered_rows", "expired", "evicted", "unremembered")
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


def check_memory(memory_ids, memory_rows, memory_ttl):
    """The memory's parameters -> (ids, rows, ttl as the library takes it: -1 = never).  Refused with ValueError: memory_ids outside
    [0, 65536], memory_rows outside {1, 2, 4, 8, 16, 32}, a negative memory_ttl."""
    ids, rows = int(memory_ids), int(memory_rows)
    if ids < 0 or ids > MEMORY_IDS_MAX:
        raise ValueError("identity map: memory_ids = %d outside [0, %d]" % (ids, MEMORY_IDS_MAX))
    if rows not in MEMORY_ROWS:
        raise ValueError("identity map: memory_rows = %d, must be one of %s" % (rows, ", ".join(map(str, MEMORY_ROWS))))
    if memory_ttl is not None and int(memory_ttl) < 0:
        raise ValueError("identity map: memory_ttl = %d, must be >= 0 updates or None (never expire)" % int(memory_ttl))
    return ids, rows, -1 if memory_ttl is None else int(memory_ttl)


def check_enrol(list_of_rows):
    """A list of [n, 512] arrays (n >= 1, any scale) -> (rows float32 [sum n, 512], counts int32).  Refused with ValueError: a wrong
    shape, an empty array, a row whose norm is zero or not finite."""
    arrays = []
    for k, a in enumerate(list_of_rows):
        a = np.asarray(a, np.float32)
        if a.ndim == 1 and a.size == EMB:
            a = a.reshape(1, EMB)
        if a.ndim != 2 or a.shape[1] != EMB or a.shape[0] < 1:
            raise ValueError("identity map: enrol takes arrays of shape [n >= 1, %d], entry %d has shape %s" % (EMB, k, a.shape))
        norms = np.sqrt((a.astype(np.float64) ** 2).sum(1))
        if not (np.isfinite(norms).all() and (norms > 0).all()):
            raise ValueError("identity map: enrol entry %d has a row of zero or non-finite norm" % k)
        arrays.append(a)
    rows = np.ascontiguousarray(np.concatenate(arrays, 0)) if arrays else np.zeros((0, EMB), np.float32)
    return rows, np.array([len(a) for a in arrays], np.int32)


class IdentityMap:
    """``IdentityMap(deepsorts, max_dist=None, max_rows=4096, memory_ids=0, memory_rows=8, memory_ttl=None)``: global ids over the
    given trackers (DeepSort objects or their ``.tracker`` handles; cosine metric, finite nn_budget).  max_dist=None: the first
    tracker's matching threshold.  memory_ids > 0: remember up to that many identities, ``memory_rows`` (1, 2, 4, 8, 16 or 32) rows
    each, and re-identify people who left every camera; memory_ttl: updates a departed id is kept, None = for ever."""

    def __init__(self, deepsorts, max_dist=None, max_rows=MAX_ROWS, memory_ids=0, memory_rows=8, memory_ttl=None):
        self._h = None
        self.trackers = check_trackers(list(deepsorts), max_rows)      # (kept: the map reads their device state)
        self.max_dist, self.max_rows = resolve_max_dist(self.trackers, max_dist), int(max_rows)
        self.memory_ids, self.rows_per_id, ttl = check_memory(memory_ids, memory_rows, memory_ttl)
        self.memory_ttl = memory_ttl
        self.n_streams = len(self.trackers)
        handles = (C.c_void_p * self.n_streams)(*[t._h for t in self.trackers])
        self._h = _lib.check_ptr(_lib.load().yds_identity_create(handles, self.n_streams, self.max_dist, self.max_rows))
        if self.memory_ids:
            _lib.check(_lib.load().yds_identity_set_memory(self._h, self.memory_ids, self.rows_per_id, ttl))

    def set_memory(self, memory_ids=0, memory_rows=8, memory_ttl=None):
        """(Re)create the memory, empty; memory_ids=0 frees it.  Inside a pipeline: refused (YdsError) while a look-ahead pass is in
        flight."""
        ids, rows, ttl = check_memory(memory_ids, memory_rows, memory_ttl)
        _lib.check(_lib.load().yds_identity_set_memory(self._h, ids, rows, ttl))
        self.memory_ids, self.rows_per_id, self.memory_ttl = ids, rows, memory_ttl

    def _need_memory(self, what):
        if not self.memory_ids:
            raise ValueError("identity map: %s needs a memory (memory_ids > 0)" % what)

    def enrol(self, list_of_rows):
        """The watch-list use: one remembered (departed) identity per [n, 512] array of appearance rows, of any scale; the last
        ``memory_rows`` rows of each are kept.  Returns the new global ids.  All or nothing: YdsError when the bank cannot take them
        (free entries first, then the departed ids held longest ago are evicted; an id with a live holder never is)."""
        self._need_memory("enrol")
        rows, counts = check_enrol(list_of_rows)
        ids = np.zeros(max(len(counts), 1), np.int32)
        _lib.check(_lib.load().yds_identity_enrol(self._h, _lib.ptr(rows), _lib.ptr(counts), len(counts), _lib.ptr(ids)))
        return [int(v) for v in ids[:len(counts)]]

    def memory(self):
        """[(global_id, n_rows, last_held)] of the remembered identities, ascending by id; last_held = the last update (counted from
        1 since the map was made) at which a live track held the id, or at which it was enrolled."""
        if not self.memory_ids:
            return []
        lib, n = _lib.load(), C.c_int(0)
        lib.yds_identity_get_memory(self._h, None, None, None, 0, C.byref(n))           # (asks for the count)
        cap = max(n.value, 1)
        g, r, l = (np.zeros(cap, np.int32) for _ in range(3))
        _lib.check(lib.yds_identity_get_memory(self._h, _lib.ptr(g), _lib.ptr(r), _lib.ptr(l), cap, C.byref(n)))
        return [(int(g[k]), int(r[k]), int(l[k])) for k in range(n.value)]

    def memory_rows(self, global_id):
        """float32 [n, 512]: the remembered rows of ``global_id``, oldest first, as stored (normalised)."""
        self._need_memory("memory_rows")
        out, n = np.zeros((self.rows_per_id, EMB), np.float32), C.c_int(0)
        _lib.check(_lib.load().yds_identity_get_memory_rows(self._h, int(global_id), _lib.ptr(out), self.rows_per_id, C.byref(n)))
        return out[:n.value].copy()

    def memory_distances(self, queries):
        """(dist float32 [Q, E], global_ids [E]): the cosine distance of every query (float32 [Q, 512] of any scale, or a
        (device_pointer, Q) pair) to every remembered identity - the minimum over its rows -, ids ascending.  The device's own
        kernel for the bank, on its own."""
        from .search import _queries
        self._need_memory("memory_distances")
        qp, on_device, Q, keep = _queries(queries)
        lib, n = _lib.load(), C.c_int(0)
        cap = max(len(self.memory()), 1)
        dist, gid = np.zeros((Q, cap), np.float32), np.zeros(cap, np.int32)
        _lib.check(lib.yds_identity_memory_distances(self._h, qp, on_device, Q, _lib.ptr(dist), _lib.ptr(gid), cap, C.byref(n)))
        return dist.reshape(-1)[:Q * n.value].reshape(Q, n.value).copy(), [int(v) for v in gid[:n.value]]

    def last_relinked(self):
        """The subset of ``last_links()`` that took the id of a departed identity from the memory."""
        return self._links(_lib.load().yds_identity_last_relinked)

    def last_memory_counts(self):
        """dict of the last update: entries, departed (both after it), relinked, remembered_rows, expired, evicted, unremembered."""
        c = np.zeros(7, np.int32)
        _lib.check(_lib.load().yds_identity_last_memory_counts(self._h, _lib.ptr(c)))
        return {k: int(v) for k, v in zip(MEMORY_COUNTS, c)}

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
        return self._links(_lib.load().yds_identity_last_links)

    def _links(self, call):
        n = C.c_int(0)
        call(self._h, None, None, None, None, 0, C.byref(n))                            # (asks for the count)
        cap = max(n.value, 1)
        s, t, g = (np.zeros(cap, np.int32) for _ in range(3))
        c = np.zeros(cap, np.float32)
        _lib.check(call(self._h, _lib.ptr(s), _lib.ptr(t), _lib.ptr(g), _lib.ptr(c), cap, C.byref(n)))
        return [(int(s[k]), int(t[k]), int(g[k]), c[k]) for k in range(n.value)]

    def reset(self):
        """Forget every identity, the remembered ones included; the counter keeps counting, so ids handed out before are never seen
        again."""
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
