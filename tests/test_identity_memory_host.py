"""The identity memory without a GPU: the restatement (tests/identity_memory_ref.py) against identity_ref with the memory off and
against its own rules on hand-made inputs, the Python layer's refusals, and the new symbols."""
import os
import re

import numpy as np
import pytest

import identity_memory_ref as M
import identity_ref as R

EMB = 512
MAXD = 0.3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _unit(seed):
    v = np.random.RandomState(9000 + seed).randn(EMB)
    return v / np.linalg.norm(v)


def _row(seed, k=0):
    """person `seed` as camera noise k shows it: distance ~1e-3 to the person's other rows, ~1 to everybody else"""
    v = _unit(seed) + 0.05 * np.random.RandomState(100 * seed + k + 1).randn(EMB) / np.sqrt(EMB)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _cam(tracks, budget=40):
    """tracks: [(track id, slot, person, hits)] of Confirmed tracks; the gallery holds the rows of hits 1 .. hits in ring order"""
    rows = []
    for tid, slot, person, hits in tracks:
        g = np.zeros((min(hits, budget), EMB), np.float32)
        for h in range(max(hits - budget, 0), hits):
            g[h % budget] = _row(person, 1000 * slot + h)
        rows.append(g)
    return M.Cam([t[0] for t in tracks], [R.CONFIRMED] * len(tracks), [t[1] for t in tracks], rows, [t[3] for t in tracks], budget)


# ------------------------------------------------------------------------------------------------ memory off = identity_ref
def test_memory_off_is_identity_ref_on_random_scenarios():
    """identity_ref asserts its margins on every matrix, and an all-clamped matrix with two columns is a tie: such a step must fail
    in the restatement too, and ends the trial"""
    rng = np.random.RandomState(1)
    compared = marginal = 0
    for trial in range(12):
        S = int(rng.randint(2, 5))
        a, b = R.IdentityState(S), M.MemoryState(S)
        next_tid = [1] * S
        alive = [[] for _ in range(S)]                          # (track id, slot, person, hits)
        for step in range(7):
            for s in range(S):
                alive[s] = [(t, sl, p, h + 1) for t, sl, p, h in alive[s] if rng.rand() > 0.2]
                here = {p for _, _, p, _ in alive[s]}
                for person in rng.permutation(4)[:int(rng.randint(0, 3))]:
                    free = sorted(set(range(8)) - {sl for _, sl, _, _ in alive[s]})
                    if int(person) not in here and free:
                        alive[s].append((next_tid[s], free[-1], int(person), 2))
                        next_tid[s] += 1
                        here.add(int(person))
            cams = [_cam(alive[s]) for s in range(S)]
            max_rows = int(rng.choice([4096, 6]))
            try:
                want = R.update(a, [R.Cam(c.ids, c.state, c.slots, c.rows) for c in cams], MAXD, max_rows)
            except AssertionError:
                with pytest.raises(AssertionError, match="assignment differ"):
                    M.update(b, cams, MAXD, max_rows)
                marginal += 1
                break
            got = M.update(b, cams, MAXD, max_rows)
            for key in ("ids", "links", "linked", "fresh", "deferred"):
                assert got[key] == want[key], (trial, step, key)
            assert all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(got["costs"], want["costs"]))
            assert a.pairs == b.pairs and a.next_id == b.next_id
            assert got["relinked"] == [] and got["memory"] == [] and got["counts"] == dict.fromkeys(M.COUNTS, 0)
            compared += 1
    print("compared %d updates, %d trials ended at a marginal step" % (compared, marginal))
    assert compared >= 30


# ------------------------------------------------------------------------------------------------ the rules on hand-made inputs
def _first(st, cams):
    """two updates: the identities are handed out, then remembered"""
    M.update(st, cams, MAXD, 4096)
    return M.update(st, cams, MAXD, 4096)


def test_touch_then_expire_at_ttl_and_one_later():
    for late in (0, 1):
        st = M.MemoryState(2, max_ids=4, rows_per_id=2, ttl=2)
        _first(st, [_cam([(1, 0, 1, 3)]), _cam([])])
        assert st.memory() == [(1, 1, 2)]
        for _ in range(1 + late):
            M.update(st, [_cam([]), _cam([])], MAXD, 4096)      # departed updates 3 (and 4): 3 - 2, 4 - 2 <= ttl
        out = M.update(st, [_cam([]), _cam([(1, 0, 1, 2)])], MAXD, 4096)
        if late:
            assert st.u - 2 == 3 and out["counts"]["expired"] == 1 and out["ids"] == [{}, {1: 2}] and out["memory"] == []
        else:
            assert st.u - 2 == 2 and out["counts"]["expired"] == 0 and out["ids"] == [{}, {1: 1}] and out["memory"] == [(1, 1, 4)]
            assert [l[:3] for l in out["relinked"]] == [(1, 1, 1)] and out["cols"] == [None, [1]]


def test_lru_eviction_by_last_held_then_id():
    """(a new track that matches nothing may face one column at most: two clamped columns are a tie the oracle refuses, so the
    identity that will need an entry is handed out while the others are still alive in its own camera)"""
    A, B = (1, 0, 1, 3), (2, 1, 2, 3)
    st = M.MemoryState(1, max_ids=2, rows_per_id=1)
    _first(st, [_cam([A, B])])
    out = M.update(st, [_cam([A, B, (3, 2, 3, 2)])], MAXD, 4096)                 # update 3: id 3 is handed out; ids 1, 2 are alive
    assert out["ids"] == [{1: 1, 2: 2, 3: 3}] and out["counts"]["unremembered"] == 0
    out = M.update(st, [_cam([(3, 2, 3, 3)])], MAXD, 4096)                       # both departed, held last at update 3: the lower id goes
    assert out["counts"]["evicted"] == 1 and out["memory"] == [(2, 1, 3), (3, 1, 4)]
    M.update(st, [_cam([(3, 2, 3, 4), (4, 3, 4, 2)])], MAXD, 4096)               # (one departed column: no tie)
    out = M.update(st, [_cam([(3, 2, 3, 5), (4, 3, 4, 3)])], MAXD, 4096)
    assert out["counts"]["evicted"] == 1 and [m[0] for m in out["memory"]] == [3, 4]
    # ---- the older one goes even when it is the higher id
    st = M.MemoryState(1, max_ids=2, rows_per_id=1)
    _first(st, [_cam([A, B])])
    M.update(st, [_cam([A, (3, 2, 3, 2)])], MAXD, 4096)                          # update 3: id 2 departed (held last at 2), id 3 handed out
    out = M.update(st, [_cam([(3, 2, 3, 3)])], MAXD, 4096)                       # id 1 departed too, held last at 3
    assert out["counts"]["evicted"] == 1 and out["memory"] == [(1, 1, 3), (3, 1, 4)]


def test_unremembered_is_retried():
    st = M.MemoryState(2, max_ids=1, rows_per_id=2)
    a = (1, 0, 1, 3)
    _first(st, [_cam([a]), _cam([])])
    out = _first(st, [_cam([a]), _cam([(1, 0, 2, 3)])])
    assert out["counts"]["unremembered"] == 1 and out["memory"] == [(1, 1, st.u)] and st.remembered[1][0] == (1, 0)
    out = M.update(st, [_cam([]), _cam([(1, 0, 2, 3)])], MAXD, 4096)
    assert out["counts"] == dict(entries=1, departed=0, relinked=0, remembered_rows=1, expired=0, evicted=1, unremembered=0)
    assert out["memory"] == [(2, 1, st.u)] and st.remembered[1][0] == (1, 3)


def test_ring_wrap_more_appenders_than_rows_and_idempotence():
    st = M.MemoryState(3, max_ids=2, rows_per_id=2)
    cams = lambda h: [_cam([(1, 0, 1, h)]), _cam([(1, 0, 1, h)]), _cam([(1, 0, 1, h)])]
    out = _first(st, cams(3))
    assert out["ids"] == [{1: 1}] * 3 and out["counts"]["remembered_rows"] == 3 and out["memory"] == [(1, 2, 2)]
    c = cams(3)
    assert np.array_equal(st.memory_rows(1), np.stack([c[1].newest(0), c[2].newest(0)]))     # the last two appenders survive
    out = M.update(st, cams(3), MAXD, 4096)                                                  # no tracker stepped
    assert out["counts"]["remembered_rows"] == 0 and np.array_equal(st.memory_rows(1), np.stack([c[1].newest(0), c[2].newest(0)]))
    one = M.MemoryState(1, max_ids=1, rows_per_id=2)
    _first(one, [_cam([(1, 0, 1, 3)], budget=3)])
    for h in (5, 6, 9):                                                                      # the tracker's own ring wraps: (hits - 1) % 3
        cam = _cam([(1, 0, 1, h)], budget=3)
        M.update(one, [cam], MAXD, 4096)
        assert np.array_equal(one.memory_rows(1)[-1], cam.rows[0][(h - 1) % 3]) and len(one.memory_rows(1)) == 2


def test_a_departed_id_relinked_in_stream_0_is_live_held_for_stream_1():
    st = M.MemoryState(3, max_ids=2, rows_per_id=2)
    _first(st, [_cam([]), _cam([]), _cam([(1, 0, 1, 3)])])
    M.update(st, [_cam([]), _cam([]), _cam([])], MAXD, 4096)
    out = M.update(st, [_cam([(1, 0, 1, 2)]), _cam([(1, 0, 1, 2)]), _cam([])], MAXD, 4096)
    assert out["ids"] == [{1: 1}, {1: 1}, {}] and [l[:3] for l in out["links"]] == [(0, 1, 1), (1, 1, 1)]
    assert [l[:3] for l in out["relinked"]] == [(0, 1, 1)] and out["counts"]["departed"] == 0 and out["counts"]["relinked"] == 1


def test_enrol_in_the_restatement():
    st = M.MemoryState(1, max_ids=2, rows_per_id=2)
    rows = [np.stack([_row(1, k) for k in range(3)]), _row(2)[None]]
    assert M.enrol(st, rows) == [1, 2] and st.memory() == [(1, 2, 0), (2, 1, 0)] and np.array_equal(st.memory_rows(1), rows[0][1:])
    assert M.enrol(st, [_row(3)[None]]) == [3] and [m[0] for m in st.memory()] == [2, 3]
    with pytest.raises(ValueError):
        M.enrol(st, [_row(4)[None]] * 3)
    out = M.update(st, [_cam([(1, 0, 2, 2)])], MAXD, 4096)
    assert out["ids"] == [{1: 2}] and len(out["relinked"]) == 1


def test_a_marginal_scenario_fails_inside_the_oracle():
    A, u = _unit(50), _unit(51)
    u = u - (u @ A) * A
    u /= np.linalg.norm(u)
    near = 0.7 * A + np.sqrt(1 - 0.49) * u                      # cosine distance 0.3 + 0 to A: inside the margin of max_dist
    st = M.MemoryState(1, max_ids=2, rows_per_id=1)
    M.enrol(st, [A[None].astype(np.float32)])
    cam = M.Cam([1], [R.CONFIRMED], [0], [near[None].astype(np.float32)], [2], 40)
    with pytest.raises(AssertionError, match="margin"):
        M.update(st, [cam], MAXD, 4096)


# ------------------------------------------------------------------------------------------------ the Python layer
class _FakeTracker:
    _h, metric, nn_budget, max_dist = 1, "cosine", 40, 0.3


def test_python_layer_refusals():
    from yolo_deepsort_amd import identity
    from yolo_deepsort_amd.detect import VideoDetector
    for kw, word in ((dict(memory_ids=4, memory_rows=3), "memory_rows"), (dict(memory_ids=-1), "memory_ids"), (dict(memory_ids=70000), "memory_ids"),
                     (dict(memory_ids=4, memory_ttl=-1), "memory_ttl")):
        with pytest.raises(ValueError, match=word):
            identity.IdentityMap([_FakeTracker()], **kw)         # (refused before the library is touched)
    assert identity.check_memory(0, 8, None) == (0, 8, -1) and identity.check_memory(65536, 32, 0) == (65536, 32, 0)
    good = np.ones((2, EMB), np.float32)
    rows, counts = identity.check_enrol([good, good[0]])
    assert rows.shape == (3, EMB) and counts.tolist() == [2, 1]
    zero = good.copy()
    zero[1] = 0
    for bad, word in ((zero, "norm"), (np.full((1, EMB), np.inf, np.float32), "norm"), (np.ones((2, 7), np.float32), "shape"),
                      (np.zeros((0, EMB), np.float32), "shape")):
        with pytest.raises(ValueError, match=word):
            identity.check_enrol([good, bad])
    im = identity.IdentityMap.__new__(identity.IdentityMap)
    im._h, im.memory_ids = None, 0
    with pytest.raises(ValueError, match="needs a memory"):
        im.enrol([good])
    assert im.memory() == []
    vd = VideoDetector.__new__(VideoDetector)
    with pytest.raises(ValueError, match="global_ids=True"):
        next(vd.detect_streams([[]], identity_memory=dict(ids=4)))
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_identity_map()


def test_new_symbols_are_declared_prototyped_and_exported():
    from yolo_deepsort_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ydsort.h")).read()
    declared = set(re.findall(r"\b(yds_[a-z0-9_]+)\s*\(", header))
    for name in ("yds_identity_set_memory", "yds_identity_enrol", "yds_identity_get_memory", "yds_identity_get_memory_rows",
                 "yds_identity_memory_distances", "yds_identity_last_relinked", "yds_identity_last_memory_counts", "yds_identity_memory_bench"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
