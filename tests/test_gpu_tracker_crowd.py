"""The fused association kernel (csrc/tracker.hip: trk_front / trk_assoc / trk_back) on the scripted crowd scenes of
tracker_crowd_cases.py, frame by frame against oracle.tracker.TrackerOracle: lists that span several 256-entry compaction chunks with
mixed predicates, 64/65 and 256/257 tracks, and every solver form lsap_form chooses in the fused kernel, in both stages.  The host test
test_tracker_crowd_cases_host.py shows that the reference decides every scene with margin.

Per frame: matches and unmatched detections bit-exact and in order, unmatched tracks as sorted lists, ids / state / time-since-update /
hits in track-list order, output rows through conftest.check_int_rows (off-by-one box columns < 2e-3 of all ints), state means at
test_gpu_assoc.py's RTOL / ATOL; the storage slots of the live tracks pairwise distinct and below the capacity, free + live = capacity;
the galleries of the tracks at list positions 0, 255, 256, 257 and last hold the last `budget` features (all of them when unbounded).

Measured on an MI355X, the reference included (it is computed once per process and shared): the unequal group 1.1 s, the two 3300-person
collapses 0.8 s each, the 600-person crowds 0.6 s each, every other trace 0.03 - 0.3 s, the form check 0.005 s behind them; 5.4 s for
the whole file.  Two value-only mutants of the kernel were run against it once: a freed-slot compaction that loses its chunk rank
fails the three collapse traces and the group, ranks running backwards inside every chunk but the first fail the 600-person crowds,
the collapses and the group.
"""
import ctypes as C

import numpy as np
import pytest

import tracker_crowd_cases as K
from conftest import check_int_rows

pytestmark = pytest.mark.gpu
F32 = np.float32
RTOL, ATOL = 1e-3, 1e-3          # test_gpu_assoc.py's


def _lib():
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    return _lib


def _tracker(params):
    from yolo_deepsort_amd.deep_sort import _TrackerHandle
    _lib()
    return _TrackerHandle(params["max_dist"], params["max_iou_distance"], params["max_age"], params["n_init"], params["nn_budget"],
                          params.get("metric", "cosine"))


def _sizes(trk):
    L = _lib()
    s = np.zeros(6, np.int32)
    L.check(L.load().yds_tracker_last_sizes(trk._h, L.ptr(s)))
    return [int(v) for v in s]


def _slots(trk, n):
    L = _lib()
    s = np.zeros(max(n, 1), np.int32)
    L.check(L.load().yds_tracker_get_slots(trk._h, L.ptr(s), max(n, 1)))
    return s[:n]


def _check_lists(trk, matches, rec, where):
    um_t, um_d = trk.last_unmatched()
    assert np.array_equal(matches, rec["matches"]), where                 # assignment indices: bit exact, in order
    assert np.array_equal(um_d, rec["um_d"]), where                       # in order
    assert np.array_equal(np.sort(um_t), np.sort(rec["um_t"])), where     # (the oracle's order comes from a set)


def _check_state(st, rec, where):
    for key in ("ids", "state", "tsu", "hits"):
        assert np.array_equal(st[key], rec[key]), (where, key)
    np.testing.assert_allclose(st["mean"], rec["mean"], rtol=RTOL, atol=ATOL, err_msg=str(where))


def _check_storage(trk, st, rec, params, where):
    """free list and galleries; returns how many of the galleries looked at had wrapped their ring"""
    tc, d, tb, db, capacity, n_free = _sizes(trk)
    n = len(st["ids"])
    slots = _slots(trk, n)
    assert len(np.unique(slots)) == n, where                              # no slot handed out twice
    assert n == 0 or (slots.min() >= 0 and slots.max() < capacity), where
    assert n_free + n == capacity, (where, n_free, n, capacity)           # no slot lost
    budget, exact = params["nn_budget"], params.get("metric", "cosine") == "euclidean"
    wrapped = 0
    for pos, want in rec["gallery"].items():
        got = trk.gallery(pos)
        hits = int(rec["hits"][pos])
        assert got.shape == want.shape and want.shape[0] == (hits if budget is None else min(hits, budget)), (where, pos)
        # `want` is in arrival order; the device keeps feature number j of a track (0-based) at ring position j % budget
        order = np.arange(hits - want.shape[0], hits) % (budget or hits)
        if exact:
            assert np.array_equal(got[order], want), (where, pos)
        else:   # rows are stored normalised: x / |x| in fp32, either side rounds the norm and the quotient once or twice (entries <= 0.2)
            np.testing.assert_allclose(got[order], want, rtol=1e-5, atol=1e-7, err_msg=str((where, pos)))
        wrapped += budget is not None and hits > budget
    return wrapped


SEEN = {}       # scene -> [(Tc, D, Tb, Db) per frame] as the kernel reported them


def _run_alone(name, check=True):
    """the scene through one tracker, frame by frame (yds_tracker_step_sel); returns (tracker, rows per frame)"""
    params = K.SCENES[name][2]
    ref = K.reference(name)
    trk = _tracker(params)
    stats, wrapped, dims, outs = [0, 0], 0, [], []
    for t, ((ids, tlwh, feats, payload), rec) in enumerate(zip(K.scene_frames(name), ref)):
        out, matches = trk.step(tlwh, feats, payload, want_debug=True)
        outs.append(out)
        sz = _sizes(trk)
        dims.append(tuple(sz[:4]))
        if not check:
            continue
        where = (name, t)
        _check_lists(trk, matches, rec, where)
        st = trk.state()
        _check_state(st, rec, where)
        assert out.shape == rec["out"].shape, where
        check_int_rows(out, rec["out"], st, stats)
        assert (sz[0], sz[1]) == rec["dims_a"], where
        assert (sz[2], sz[3]) == rec["dims_b"] if rec["dims_b"] is not None else sz[2] * sz[3] == 0, where
        wrapped += _check_storage(trk, st, rec, params, where)
    if check:
        print("%s: int32 box columns differing by one: %d of %d" % (name, stats[0], stats[1]))
        assert stats[1] > 0 and stats[0] / stats[1] < 2e-3, stats
        if params["nn_budget"] is not None:
            assert wrapped > 0, name
    SEEN[name] = dims
    return trk, outs


@pytest.mark.parametrize("name", K.TRACE_SCENES)
def test_crowd_trace_vs_oracle(name):
    _run_alone(name)


def test_every_fused_solver_form_ran_in_both_stages():
    """the sizes the kernel reported, through the library's own rule (yds_lsap_fused_form: the function the kernel switches over)"""
    lib = _lib().load()
    a, b = set(), set()
    for name in K.TRACE_SCENES:
        if name not in SEEN:
            _run_alone(name, check=False)
        for tc, d, tb, db in SEEN[name]:
            fa, fb = lib.yds_lsap_fused_form(tc, d), lib.yds_lsap_fused_form(tb, db)
            assert fa == K.fused_form(tc, d) and fb == K.fused_form(tb, db), (name, tc, d, tb, db, fa, fb)
            a.add(fa)
            b.add(fb)
    a.discard(0)
    b.discard(0)
    print("stage A forms:", sorted(K.FORM_NAMES[f] for f in a), " stage B forms:", sorted(K.FORM_NAMES[f] for f in b))
    assert a | b == K.REACHABLE_FORMS, (a, b)
    assert K.NEW_FORMS <= a and K.NEW_FORMS <= b, (a, b)
    for shape in ((64, 64), (65, 64), (200, 150), (200, 200), (256, 139), (256, 140), (257, 1), (300, 5), (300, 300), (3200, 1), (3201, 1),
                  (3300, 5), (5, 3300), (3300, 12), (0, 7), (7, 0)):
        assert lib.yds_lsap_fused_form(*shape) == K.fused_form(*shape), shape


# ------------------------------------------------------------------------------------------ one unequal group
GROUP = ("collapse3300x5", "crowd257_ring", "crowd65_ring", "crowd5_ring", None, "crowd30_ring")    # None: a stream without detections
GROUP_SKIP = (5, 3)            # stream 5 skips its frame 3
EMPTY_FRAMES = 4


def test_unequal_group_equals_each_tracker_alone():
    """One step_batch over trackers whose sizes differ by orders of magnitude and whose frame counts differ (rounds thin out): the
    grids come from the largest tracker of a round and the guards retire the rest.  Every stream's rows, last lists and full state -
    mean and covariance bits included - equal the same tracker stepped alone, which is held to the oracle frame by frame."""
    L = _lib()
    lib = L.load()
    empty = (np.zeros(0, np.int64), np.zeros((0, 4), F32), np.zeros((0, 512), F32), np.zeros(0, F32))
    frames = [K.scene_frames(n) if n else [empty] * EMPTY_FRAMES for n in GROUP]
    frames[GROUP_SKIP[0]] = [f if t != GROUP_SKIP[1] else empty for t, f in enumerate(frames[GROUP_SKIP[0]])]
    # ---- alone (the skipped frame is not stepped at all)
    alone, alone_rows = [], []
    for s, name in enumerate(GROUP):
        trk = _tracker(K.SCENES[name][2] if name else K.P_RING)
        rows = []
        ref = K.reference(name, skip=(GROUP_SKIP[1],) if s == GROUP_SKIP[0] else ()) if name else None
        stats = [0, 0]
        for t, (ids, tlwh, feats, payload) in enumerate(frames[s]):
            if (s, t) == GROUP_SKIP:
                rows.append(None)
                continue
            out, matches = trk.step(tlwh, feats, payload, want_debug=True)
            rows.append(out)
            if ref is not None:
                st = trk.state()
                _check_lists(trk, matches, ref[t], (name, t))
                _check_state(st, ref[t], (name, t))
                check_int_rows(out, ref[t]["out"], st, stats)
        assert ref is None or (stats[1] > 0 and stats[0] / stats[1] < 2e-3), (name, stats)
        alone.append(trk)
        alone_rows.append(rows)
    assert all(r.shape[0] == 0 for r in alone_rows[4]) and max(r.shape[0] for r in alone_rows[3] if r is not None) > 0
    # ---- the same frames in ONE step of a group, interleaved in time order
    group = [_tracker(K.SCENES[name][2] if name else K.P_RING) for name in GROUP]
    order = [(s, t) for t in range(max(len(f) for f in frames)) for s in range(len(GROUP)) if t < len(frames[s])]
    stream_of = np.array([s for s, _ in order], np.int32)
    first = np.concatenate([[0], np.cumsum([len(frames[s][t][1]) for s, t in order])]).astype(np.int32)
    tlwh = np.ascontiguousarray(np.concatenate([frames[s][t][1] for s, t in order], 0), dtype=F32)
    feats = np.ascontiguousarray(np.concatenate([frames[s][t][2] for s, t in order], 0), dtype=F32)
    payload = np.ascontiguousarray(np.concatenate([frames[s][t][3] for s, t in order], 0), dtype=F32)
    skip = np.array([1 if st == GROUP_SKIP else 0 for st in order], np.uint8)
    cap = 3400
    out6 = np.zeros((len(order), cap, 6), np.int32)
    counts = np.zeros(len(order), np.int32)
    handles = (C.c_void_p * len(group))(*[t._h for t in group])
    L.check(lib.yds_tracker_step_batch(handles, len(group), len(order), L.ptr(stream_of), L.ptr(tlwh), L.ptr(first), L.ptr(feats), L.ptr(payload),
                                       L.ptr(skip), L.ptr(out6), cap, L.ptr(counts)))
    for b, (s, t) in enumerate(order):
        want = alone_rows[s][t]
        if want is None:
            assert counts[b] == -1, (s, t)
            continue
        assert counts[b] == want.shape[0] and np.array_equal(out6[b, :counts[b]], want), (GROUP[s], t)
    for s, (a, g) in enumerate(zip(alone, group)):
        sa, sg = a.state(), g.state()
        for key in ("ids", "state", "tsu", "hits"):
            assert np.array_equal(sa[key], sg[key]), (GROUP[s], key)
        assert np.array_equal(sa["mean"].view(np.uint32), sg["mean"].view(np.uint32)), GROUP[s]
        assert np.array_equal(sa["cov"].view(np.uint32), sg["cov"].view(np.uint32)), GROUP[s]
        for x, y in zip(a.last_unmatched(), g.last_unmatched()):
            assert np.array_equal(x, y), GROUP[s]
        assert _sizes(a)[:4] == _sizes(g)[:4], GROUP[s]
        n = len(sg["ids"])
        slots = _slots(g, n)
        assert len(np.unique(slots)) == n and (n == 0 or slots.max() < _sizes(g)[4]), GROUP[s]
        assert _sizes(g)[5] + n == _sizes(g)[4], GROUP[s]
        for pos in (0, n - 1):
            if n:
                assert np.array_equal(a.gallery(pos), g.gallery(pos)), (GROUP[s], pos)
