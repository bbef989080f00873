"""Host-side checks of the identity map: the oracle (identity_ref.py) on hand-made inputs, one rule at a time; the refusals that
need no device; the prototypes of the new entries.  The oracle takes rows of any width: four coordinates are enough to choose the
distances by hand (unit vectors: d = 1 - cosine)."""
import numpy as np
import pytest

import identity_ref as R

T, C = 1, 2          # Tentative, Confirmed


def _at(cos, axis=0, other=1):
    """a unit vector with cosine `cos` to basis vector `axis`"""
    v = np.zeros(4)
    v[axis], v[other] = cos, np.sqrt(1.0 - cos * cos)
    return v


E = np.eye(4)


def _cam(tracks):
    """tracks: list of (id, state, slot, rows)"""
    return R.Cam([t[0] for t in tracks], [t[1] for t in tracks], [t[2] for t in tracks], [np.atleast_2d(t[3]) for t in tracks])


def test_new_tracks_candidates_and_tentative_tracks():
    st = R.IdentityState(2)
    cams = [_cam([(1, C, 0, E[0]), (2, T, 1, E[1])]), _cam([(1, T, 0, E[0])])]
    r = R.update(st, cams, 0.3, 64)
    assert r["ids"] == [{1: 1}, {}] and (r["linked"], r["fresh"], r["deferred"]) == (0, 1, 0)
    # camera 1's track is confirmed: it is new, camera 0's holder is its candidate; the Tentative track 2 still takes no part
    cams[1] = _cam([(1, C, 0, _at(0.95))])
    r = R.update(st, cams, 0.3, 64)
    assert r["ids"] == [{1: 1}, {1: 1}] and r["linked"] == 1 and r["fresh"] == 0
    assert r["links"][0][:3] == (1, 1, 1) and abs(r["links"][0][3] - 0.05) < 1e-12
    # nothing new: nothing happens, the counter stands
    r = R.update(st, cams, 0.3, 64)
    assert (r["linked"], r["fresh"], r["deferred"]) == (0, 0, 0) and st.next_id == 2


def test_admission_is_a_prefix_and_nothing_is_skipped():
    st = R.IdentityState(1)
    rows = lambda n, k: np.tile(E[k], (n, 1))
    cams = [_cam([(1, C, 0, rows(40, 0)), (2, C, 1, rows(20, 1)), (3, C, 2, rows(30, 2)), (4, C, 3, rows(4, 3))])]
    r = R.update(st, cams, 0.3, 64)
    # 40 + 20 fit, 30 does not and ends admission: the 4-row track behind it would fit and is NOT taken
    assert r["ids"] == [{1: 1, 2: 2, 3: 0, 4: 0}] and (r["fresh"], r["deferred"]) == (2, 2)
    r = R.update(st, cams, 0.3, 64)
    assert r["ids"] == [{1: 1, 2: 2, 3: 3, 4: 4}] and (r["fresh"], r["deferred"]) == (2, 0)


def test_distance_is_the_minimum_over_the_rows_of_both_tracks():
    a = np.stack([_at(0.5), _at(0.9)])
    b = np.stack([E[0], _at(0.2, other=2)])
    assert abs(R.track_distance(a, b) - 0.1) < 1e-12          # row 1 of a against row 0 of b
    assert R.track_distance(a, np.zeros((0, 4))) == np.inf


def test_simultaneous_confirmation_fresh_in_the_lowest_stream_linked_in_the_others():
    st = R.IdentityState(3)
    cams = [_cam([(1, C, 0, E[0])]), _cam([(1, C, 0, _at(0.97))]), _cam([(1, C, 0, _at(0.96, other=2))])]
    r = R.update(st, cams, 0.3, 64)
    assert r["ids"] == [{1: 1}, {1: 1}, {1: 1}] and (r["linked"], r["fresh"]) == (2, 1)
    # camera 2 takes the minimum over BOTH holders (cameras 0 and 1)
    d0 = 1 - 0.96
    d1 = 1 - float(_at(0.96, other=2) @ _at(0.97))
    assert abs(r["links"][1][3] - min(d0, d1)) < 1e-12


def test_one_id_per_camera():
    st = R.IdentityState(2)
    cams = [_cam([(1, C, 0, E[0])]), _cam([])]
    R.update(st, cams, 0.3, 64)
    cams[1] = _cam([(1, C, 0, _at(0.90)), (2, C, 1, _at(0.95, other=2))])
    r = R.update(st, cams, 0.3, 64)
    assert r["ids"][1] == {1: 2, 2: 1} and (r["linked"], r["fresh"]) == (1, 1)       # the cheaper twin is linked
    cams[1] = _cam([(1, C, 0, _at(0.90)), (2, C, 1, _at(0.95, other=2)), (3, C, 2, _at(0.99, other=3))])
    r = R.update(st, cams, 0.3, 64)
    assert r["ids"][1] == {1: 2, 2: 1, 3: 3} and r["costs"][1].shape == (1, 0)      # id 1 is held in camera 1: not offered


def test_assignment_not_greedy():
    gram = np.array([[1, .8, .90, .89], [.8, 1, .88, .75], [.90, .88, 1, .85], [.89, .75, .85, 1]])
    assert np.linalg.eigvalsh(gram).min() > 0.07
    L = np.linalg.cholesky(gram)
    st = R.IdentityState(2)
    cams = [_cam([(1, C, 0, L[0]), (2, C, 1, L[1])]), _cam([])]
    R.update(st, cams, 0.3, 64)
    cams[1] = _cam([(1, C, 0, L[2]), (2, C, 1, L[3])])
    r = R.update(st, cams, 0.3, 64)
    np.testing.assert_allclose(r["costs"][1], [[.10, .12], [.11, .25]], atol=1e-12)
    assert r["ids"][1] == {1: 2, 2: 1}                       # total 0.23; the smallest entry first would give 0.35


def test_slot_reuse_does_not_inherit_and_dead_ids_are_not_offered():
    st = R.IdentityState(2)
    cams = [_cam([(1, C, 0, E[0])]), _cam([])]
    R.update(st, cams, 0.3, 64)
    # track 1 died, track 2 took slot 0 and looks the same: the pair names owner 1, so it holds nothing and is new
    cams[0] = _cam([(2, C, 0, E[0])])
    r = R.update(st, cams, 0.3, 64)
    assert r["ids"][0] == {2: 2} and r["fresh"] == 1
    # id 1 has no live holder: a look-alike in camera 1 is offered id 2 only
    cams[1] = _cam([(1, C, 0, _at(0.99))])
    r = R.update(st, cams, 0.3, 64)
    assert r["ids"][1] == {1: 2} and st.next_id == 3


def test_reset_forgets_pairs_and_keeps_the_counter():
    st = R.IdentityState(1)
    cams = [_cam([(1, C, 0, E[0])])]
    R.update(st, cams, 0.3, 64)
    st.reset()
    assert R.update(st, cams, 0.3, 64)["ids"] == [{1: 2}]


def test_marginal_scenarios_fail_in_the_oracle():
    with pytest.raises(AssertionError):                      # a cost within 1e-3 of max_dist
        R.min_cost_matching([[0.3005]], 0.3)
    with pytest.raises(AssertionError):                      # two outcomes 4e-4 apart
        R.min_cost_matching([[0.1000, 0.1002], [0.1002, 0.1000 + 8e-4]], 0.3)
    with pytest.raises(AssertionError):                      # every entry clamped: all assignments tie
        R.min_cost_matching([[0.9, 0.8], [0.7, 0.95]], 0.3)
    assert R.min_cost_matching([[0.1, 0.8], [0.7, 0.95]], 0.3) == {0: 0}
    assert R.min_cost_matching([[0.9]], 0.3) == {} and R.min_cost_matching([[0.1, 0.9]], 0.3) == {0: 0}
    # device costs switch the assertions off and decide at the bit
    c = np.float32(0.25)
    assert R.min_cost_matching([[float(c)]], float(c), check_margin=False) == {0: 0}
    assert R.min_cost_matching([[float(c)]], float(np.nextafter(c, np.float32(0))), check_margin=False) == {}


class _Fake:
    def __init__(self, metric="cosine", nn_budget=40, max_dist=0.3):
        self._h, self.metric, self.nn_budget, self.max_dist = 1, metric, nn_budget, max_dist


def test_refusals_that_need_no_device():
    from yolo_deepsort_amd import identity
    a, b = _Fake(), _Fake(nn_budget=100)
    assert identity.check_trackers([a, b], 100) == [a, b]
    for bad, rows, word in (([], 4096, "no trackers"), ([a, object()], 4096, "no tracker of this package"),
                            ([a, _Fake(metric="euclidean")], 4096, "euclidean"), ([a, _Fake(nn_budget=None)], 4096, "nn_budget=None"),
                            ([a, b, a], 4096, "more than one stream"), ([a, b], 99, "max_rows")):
        with pytest.raises(ValueError, match=word):
            identity.check_trackers(bad, rows)
    assert identity.resolve_max_dist([a], None) == 0.3 and identity.resolve_max_dist([a], 0.25) == 0.25
    with pytest.raises(ValueError):
        identity.resolve_max_dist([a], float("nan"))


def test_video_detector_stream_identities_outside_a_generator():
    from yolo_deepsort_amd.detect import VideoDetector
    vd = VideoDetector.__new__(VideoDetector)
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_identities()


def test_new_entries_are_prototyped_and_exported():
    from yolo_deepsort_amd import _lib, build
    build.build()                                               # (as tests/test_lib_abi.py: nothing to do when the library is current)
    names = ["yds_identity_create", "yds_identity_destroy", "yds_identity_reset", "yds_identity_update", "yds_identity_get",
             "yds_identity_last_links", "yds_identity_last_counts", "yds_identity_set_timing", "yds_identity_last_us",
             "yds_pipeline_set_identities", "yds_pipeline_last_identities"]
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
    assert _lib.MISSING == []
