"""Cross-camera search over the appearance galleries the trackers keep in HBM (csrc/gallery_search.hip).

``gallery_search`` answers "where is this person?" (a watch-list query against every camera's live tracks), ``link_track``
answers "is track 17 of camera 3 some track of another camera?" (a hand-over), ``gallery_distances`` returns the whole
distance matrix for callers with a policy of their own.  The distance is the trackers' own appearance metric
(deep_sort/sort/nn_matching.py:77-100): min over a track's stored rows of 1 - cosine.

Call them between steps: after ``DeepSort.update`` / a pipeline step has returned, never concurrently with one.  They read
tracker state and change none of it.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

__all__ = ["gallery_search", "gallery_distances", "link_track", "MAX_QUERIES"]

MAX_QUERIES = 4096
EMB = 512
TENTATIVE, CONFIRMED = 1, 2          # bits of the state mask (track states 1 and 2)


def _handles(deepsorts):
    """DeepSort objects or bare tracker handles -> the tracker handles; euclidean trackers and repeats raise ValueError."""
    trackers = [getattr(d, "tracker", d) for d in deepsorts]
    if not trackers:
        raise ValueError("gallery search: no trackers given")
    for s, t in enumerate(trackers):
        if getattr(t, "_h", None) is None:
            raise ValueError("gallery search: entry %d is no tracker of this package" % s)
        if getattr(t, "metric", "cosine") != "cosine":
            raise ValueError("gallery search: tracker %d uses the euclidean metric; its gallery rows are not normalised" % s)
    if len({id(t) for t in trackers}) != len(trackers):
        raise ValueError("gallery search: a tracker is given for more than one stream")
    return trackers


def _handle_array(trackers):
    return (C.c_void_p * len(trackers))(*[t._h for t in trackers])


def _queries(queries):
    """float32 [Q,512] array, or a (device_pointer, Q) pair -> (pointer, on_device, Q, keep-alive)."""
    if isinstance(queries, tuple) and len(queries) == 2 and not isinstance(queries[0], (np.ndarray, list, tuple)):
        p, q = queries
        q = int(q)
        if not p:
            raise ValueError("gallery search: the device pointer of the queries is NULL")
        if q < 1 or q > MAX_QUERIES:
            raise ValueError("gallery search: %d queries, the call takes 1..%d" % (q, MAX_QUERIES))
        return (p if isinstance(p, C.c_void_p) else C.c_void_p(int(p))), 1, q, None
    a = np.asarray(queries)
    if a.ndim == 1 and a.size == EMB:
        a = a.reshape(1, EMB)
    if a.ndim != 2 or a.shape[1] != EMB:
        raise ValueError("gallery search: queries must be a float32 [Q, %d] array or a (device_pointer, Q) pair, got shape %s" % (EMB, a.shape))
    if a.shape[0] < 1 or a.shape[0] > MAX_QUERIES:
        raise ValueError("gallery search: %d queries, the call takes 1..%d" % (a.shape[0], MAX_QUERIES))
    a = np.ascontiguousarray(a, dtype=np.float32)
    return _lib.ptr(a), 0, a.shape[0], a


def _select_args(trackers, top_k, max_dist, confirmed_only):
    top_k = int(top_k)
    if top_k < 1:
        raise ValueError("gallery search: top_k must be >= 1, got %d" % top_k)
    if max_dist is None:
        max_dist = getattr(trackers[0], "max_dist", None)
        if max_dist is None:
            raise ValueError("gallery search: max_dist=None needs a tracker that knows its matching threshold")
    total = sum(_lib.load().yds_tracker_num_tracks(t._h) for t in trackers)
    return min(top_k, max(total, 1)), float(max_dist), (CONFIRMED if confirmed_only else CONFIRMED | TENTATIVE)


def _hits(n_hits, stream, tid, dist, k):
    """The flat result arrays of the library -> per query a list of (stream, track_id, dist)."""
    return [[(int(stream[q * k + j]), int(tid[q * k + j]), float(dist[q * k + j])) for j in range(int(n_hits[q]))]
            for q in range(len(n_hits))]


def gallery_search(deepsorts, queries, top_k=5, max_dist=None, confirmed_only=True):
    """Per query the at most top_k nearest tracks of all given trackers with distance <= max_dist, as a list of
    (stream, track_id, dist) ordered by (dist, stream, position in the track list).  stream = index into ``deepsorts``.
    max_dist=None: the first tracker's matching threshold.  confirmed_only=False also returns Tentative tracks.
    queries: float32 [Q,512] (any scale: they are normalised on the device) or (device_pointer, Q), e.g.
    ``(extractor.features_dev(), n)`` after ``extractor.embed(frame, tlwh, to_host=False)``.  A zero or non-finite query
    matches nothing."""
    trackers = _handles(deepsorts)
    qp, on_dev, nq, _keep = _queries(queries)
    k, max_dist, mask = _select_args(trackers, top_k, max_dist, confirmed_only)
    n_hits = np.zeros(nq, np.int32)
    stream, tid = np.zeros(nq * k, np.int32), np.zeros(nq * k, np.int32)
    dist = np.zeros(nq * k, np.float32)
    _lib.check(_lib.load().yds_gallery_search(_handle_array(trackers), len(trackers), qp, on_dev, nq, mask, max_dist, k,
                                              _lib.ptr(n_hits), _lib.ptr(stream), _lib.ptr(tid), _lib.ptr(dist)))
    return _hits(n_hits, stream, tid, dist, k)


def gallery_distances(deepsorts, queries):
    """(dist [Q,T] float32, stream_of [T], track_id [T], state [T]): the distance of every query to every live track of
    every given tracker, tracks in (stream, track-list) order; state 1 = Tentative, 2 = Confirmed."""
    trackers = _handles(deepsorts)
    qp, on_dev, nq, _keep = _queries(queries)
    lib = _lib.load()
    cap = max(sum(lib.yds_tracker_num_tracks(t._h) for t in trackers), 1)
    dist = np.zeros(nq * cap, np.float32)
    stream, tid, state = (np.zeros(cap, np.int32) for _ in range(3))
    n = C.c_int(0)
    _lib.check(lib.yds_gallery_search_dense(_handle_array(trackers), len(trackers), qp, on_dev, nq, _lib.ptr(dist), _lib.ptr(stream),
                                            _lib.ptr(tid), _lib.ptr(state), cap, C.byref(n)))
    t = n.value
    return dist[:nq * t].reshape(nq, t).copy(), stream[:t].copy(), tid[:t].copy(), state[:t].copy()


def link_track(deepsorts, stream, track_id, exclude_stream=None, top_k=5, max_dist=None, confirmed_only=True):
    """Hand-over: the tracks nearest to live track ``track_id`` of stream ``stream``, as a list of (stream, track_id, dist);
    the distance is the minimum over the stored rows of both tracks.  The track itself is never returned, nor any track of
    ``exclude_stream`` (pass ``stream`` to look at the other cameras only).  Other arguments as gallery_search."""
    trackers = _handles(deepsorts)
    stream = int(stream)
    if stream < 0 or stream >= len(trackers):
        raise ValueError("gallery search: stream %d outside [0, %d)" % (stream, len(trackers)))
    ex = -1 if exclude_stream is None else int(exclude_stream)
    if ex < -1 or ex >= len(trackers):
        raise ValueError("gallery search: exclude_stream %d outside [0, %d)" % (ex, len(trackers)))
    k, max_dist, mask = _select_args(trackers, top_k, max_dist, confirmed_only)
    n_hits = np.zeros(1, np.int32)
    s, tid, dist = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.float32)
    _lib.check(_lib.load().yds_gallery_link(_handle_array(trackers), len(trackers), stream, int(track_id), ex, mask, max_dist, k,
                                            _lib.ptr(n_hits), _lib.ptr(s), _lib.ptr(tid), _lib.ptr(dist)))
    return _hits(n_hits, s, tid, dist, k)[0]
