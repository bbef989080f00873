"""Host side of the cross-camera search (yolo_deepsort_amd/search.py): argument validation and result formatting against a fake
library, no device needed; and the detector's search entries outside a running detect_streams generator."""
import ctypes as C

import numpy as np
import pytest

from yolo_deepsort_amd import _lib, search


class _FakeLib:
    """Records the search calls and fills the output arrays with a scripted answer."""

    def __init__(self, tracks_per_handle):
        self.tracks, self.calls = dict(tracks_per_handle), []

    def yds_tracker_num_tracks(self, h):
        return self.tracks[h]

    @staticmethod
    def _view(p, n, dtype):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(dtype)), shape=(n,))

    def yds_gallery_search(self, trks, n_streams, queries, on_dev, Q, mask, max_dist, top_k, n_hits, hs, hi, hd):
        self.calls.append(("search", [trks[i] for i in range(n_streams)], on_dev, Q, mask, max_dist, top_k))
        n = self._view(n_hits, Q, C.c_int32)
        s, i, d = self._view(hs, Q * top_k, C.c_int32), self._view(hi, Q * top_k, C.c_int32), self._view(hd, Q * top_k, C.c_float)
        for q in range(Q):
            n[q] = min(q, top_k)                          # query q gets q hits
            for k in range(n[q]):
                s[q * top_k + k], i[q * top_k + k], d[q * top_k + k] = k, 10 * q + k, 0.125 * k
        return 0

    def yds_gallery_search_dense(self, trks, n_streams, queries, on_dev, Q, dist, stream_of, track_id, state, cap, n_tracks):
        T = sum(self.tracks[trks[i]] for i in range(n_streams))
        self.calls.append(("dense", Q, cap))
        C.cast(n_tracks, C.POINTER(C.c_int))[0] = T
        self._view(dist, Q * T, C.c_float)[:] = np.arange(Q * T)
        self._view(stream_of, T, C.c_int32)[:] = np.arange(T) // 2
        self._view(track_id, T, C.c_int32)[:] = np.arange(T) + 1
        self._view(state, T, C.c_int32)[:] = 2
        return 0

    def yds_gallery_link(self, trks, n_streams, stream, track_id, exclude, mask, max_dist, top_k, n_hits, hs, hi, hd):
        self.calls.append(("link", stream, track_id, exclude, mask, max_dist, top_k))
        self._view(n_hits, 1, C.c_int32)[0] = 1
        self._view(hs, top_k, C.c_int32)[0], self._view(hi, top_k, C.c_int32)[0], self._view(hd, top_k, C.c_float)[0] = 1, 42, 0.25
        return 0


class _Trk:
    def __init__(self, h, max_dist=0.3, metric="cosine"):
        self._h, self.max_dist, self.metric = h, max_dist, metric


class _DS:
    def __init__(self, trk):
        self.tracker = trk


@pytest.fixture
def fake(monkeypatch):
    f = _FakeLib({11: 2, 12: 0, 13: 3})
    monkeypatch.setattr(_lib, "load", lambda: f)
    return f


def test_search_formats_hits_and_passes_its_arguments(fake):
    trks = [_Trk(11, max_dist=0.2), _DS(_Trk(12)), _Trk(13)]          # bare handles and DeepSort-like owners mix
    q = np.ones((3, 512), np.float64)
    hits = search.gallery_search(trks, q, top_k=9, confirmed_only=False)
    assert hits == [[], [(0, 10, 0.0)], [(0, 20, 0.0), (1, 21, 0.125)]]
    kind, handles, on_dev, Q, mask, max_dist, top_k = fake.calls[-1]
    assert (kind, handles, on_dev, Q, mask) == ("search", [11, 12, 13], 0, 3, 3)
    assert max_dist == pytest.approx(0.2) and top_k == 5              # max_dist=None: the first tracker's threshold; top_k capped at the 5 live tracks
    search.gallery_search(trks, q[0], top_k=2, max_dist=0.5)           # one [512] vector is one query; Confirmed only by default
    assert fake.calls[-1][3:] == (1, 2, 0.5, 2)
    search.gallery_search(trks, (0xdead00, 7), top_k=1)                # a device pointer and a count
    assert fake.calls[-1][2:4] == (1, 7)


def test_distances_and_link_format(fake):
    trks = [_Trk(11), _Trk(12), _Trk(13)]
    dist, stream_of, track_id, state = search.gallery_distances(trks, np.zeros((2, 512), np.float32))
    assert dist.shape == (2, 5) and dist[1, 4] == 9 and dist.dtype == np.float32
    assert stream_of.tolist() == [0, 0, 1, 1, 2] and track_id.tolist() == [1, 2, 3, 4, 5] and state.tolist() == [2] * 5
    assert fake.calls[-1] == ("dense", 2, 5)
    assert search.link_track(trks, 2, 17, exclude_stream=2, top_k=3, max_dist=0.4) == [(1, 42, 0.25)]
    assert fake.calls[-1] == ("link", 2, 17, 2, 2, pytest.approx(0.4), 3)
    search.link_track(trks, 0, 5, confirmed_only=False)
    assert fake.calls[-1] == ("link", 0, 5, -1, 3, pytest.approx(0.3), 5)


def test_arguments_are_refused_before_the_library_is_called(fake):
    trks = [_Trk(11), _Trk(13)]
    q = np.zeros((1, 512), np.float32)
    bad = [
        (lambda: search.gallery_search([], q), "no trackers"),
        (lambda: search.gallery_search([_Trk(11), _Trk(13, metric="euclidean")], q), "euclidean"),
        (lambda: search.gallery_search([trks[0], trks[0]], q), "more than one stream"),
        (lambda: search.gallery_search([trks[0], object()], q), "no tracker of this package"),
        (lambda: search.gallery_search(trks, np.zeros((0, 512), np.float32)), "1..4096"),
        (lambda: search.gallery_search(trks, np.zeros((4097, 512), np.float32)), "1..4096"),
        (lambda: search.gallery_search(trks, (0xdead00, 0)), "1..4096"),
        (lambda: search.gallery_search(trks, (None, 4)), "NULL"),
        (lambda: search.gallery_search(trks, np.zeros((2, 128), np.float32)), "512"),
        (lambda: search.gallery_search(trks, np.zeros((2, 2, 512), np.float32)), "512"),
        (lambda: search.gallery_search(trks, q, top_k=0), "top_k"),
        (lambda: search.gallery_search([_Trk(11, max_dist=None)], q), "max_dist"),
        (lambda: search.gallery_distances(trks, np.zeros(100, np.float32)), "512"),
        (lambda: search.link_track(trks, 2, 1), "stream 2"),
        (lambda: search.link_track(trks, -1, 1), "stream -1"),
        (lambda: search.link_track(trks, 0, 1, exclude_stream=5), "exclude_stream 5"),
        (lambda: search.link_track(trks, 0, 1, top_k=-3), "top_k"),
    ]
    for call, text in bad:
        with pytest.raises(ValueError, match=text):
            call()
    assert fake.calls == []


def test_library_errors_surface_as_yds_error(monkeypatch):
    class Failing(_FakeLib):
        def yds_gallery_search(self, *a):
            return -1

        def yds_last_error(self):
            return b"gallery_search: streams 0 and 1 share one tracker"
    monkeypatch.setattr(_lib, "load", lambda: Failing({1: 1, 2: 1}))
    with pytest.raises(_lib.YdsError, match="share one tracker"):
        search.gallery_search([_Trk(1), _Trk(2)], np.zeros((1, 512), np.float32))


def test_video_detector_search_needs_a_running_detect_streams():
    from yolo_deepsort_amd.detect import VideoDetector
    vd = VideoDetector.__new__(VideoDetector)                          # no model: only the guard is under test
    with pytest.raises(ValueError, match="detect_streams"):
        vd.search_streams(np.zeros((1, 512), np.float32))
    with pytest.raises(ValueError, match="detect_streams"):
        vd.link_stream_track(0, 1)

    class Pipe:
        def search(self, queries, **kw):
            return ("search", kw)

        def link(self, stream, track_id, **kw):
            return ("link", stream, track_id, kw)
    vd._streams_pipe = Pipe()
    assert vd.search_streams(None, top_k=2) == ("search", dict(top_k=2, max_dist=None, confirmed_only=True))
    assert vd.link_stream_track(1, 7, exclude_stream=1) == ("link", 1, 7, dict(exclude_stream=1, top_k=5, max_dist=None, confirmed_only=True))


def test_pipelines_hand_their_trackers_to_the_search(monkeypatch):
    from yolo_deepsort_amd import pipeline as pl
    seen = []
    monkeypatch.setattr(search, "gallery_search", lambda ds, q, **kw: seen.append(("search", ds, kw)) or [])
    monkeypatch.setattr(search, "link_track", lambda ds, s, t, **kw: seen.append(("link", ds, s, t, kw)) or [])
    multi = pl.MultiStreamPipeline.__new__(pl.MultiStreamPipeline)
    multi._h, multi.deepsorts, multi.ds = None, ["a", "b"], "a"
    single = pl.Pipeline.__new__(pl.Pipeline)
    single._h, single.ds = None, "solo"
    multi.search("q", top_k=2)
    single.link(0, 4, max_dist=0.5)
    assert seen[0] == ("search", ["a", "b"], dict(top_k=2, max_dist=None, confirmed_only=True))
    assert seen[1] == ("link", ["solo"], 0, 4, dict(exclude_stream=None, top_k=5, max_dist=0.5, confirmed_only=True))
