"""The detector NMS (csrc/nms.hip: count, scan, emit, rank, mask, sweep, merge, publish) at its edges, bit for bit against the oracle.

The cases come from tests/nms_edge_cases.py; tests/test_nms_edges_host.py proves on the CPU that each one hits what it claims (an
IoU or a score exactly on its threshold, equal scores across the rank tile and the rank grid stride, counts carried over the
scan's seams, suppressed bits at both ends of a mask word, a cap below 300, the merge branch's limits, degenerate boxes, non-finite
scores) and that the oracle equals a second statement of the rule.  Centre-form cases run through yds_nms_pred against
oracle.nms.soft_non_max_suppression; their corner-form twins through yds_nms_merge_pred against soft_non_max_suppression_merge,
score and class columns bit for bit and the box columns - which the merge branch may have replaced by a weighted mean - at
rtol 1e-6, atol 1e-4.  Group h (non-finite scores) stays off the merge entries: an infinite weight makes every merged box NaN."""
import ctypes as C
import threading

import numpy as np
import pytest

import nms_edge_cases as E
from oracle import nms as onms
from yolo_deepsort_amd import _lib as L

pytestmark = pytest.mark.gpu
F32 = np.float32
EMPTY = np.zeros((0, 6), F32)


# ------------------------------------------------------------------------------------------------ entries
def _single(fn, pred, ct, it, cap=300):
    L.init()
    pred = np.ascontiguousarray(pred, dtype=F32)
    out = np.zeros((300, 6), F32)
    n = C.c_int(0)
    L.check(fn(L.ptr(pred), pred.shape[0], pred.shape[1], ct, it, L.ptr(out), cap, C.byref(n)))
    return out[:n.value].copy()


def _plain(pred, ct, it, cap=300):
    return _single(L.load().yds_nms_pred, pred, ct, it, cap)


def _merge(pred, ct, it, cap=300):
    return _single(L.load().yds_nms_merge_pred, pred, ct, it, cap)


def _batched(preds, ct, it):
    L.init()
    stack = np.ascontiguousarray(np.stack(preds, 0), dtype=F32)
    out = np.zeros((len(preds), 300, 6), F32)
    n = np.zeros(len(preds), np.int32)
    L.check(L.load().yds_nms_merge_pred_batched(L.ptr(stack), len(preds), stack.shape[1], stack.shape[2], ct, it, L.ptr(out), 300, L.ptr(n)))
    return [out[f, :n[f]].copy() for f in range(len(preds))]


def _ragged(frames, ct, it, lead=5):
    """frames: (pred, corner, merge); `lead` rows that belong to no frame stand in front of the block, so row0 starts above zero"""
    L.init()
    attrs = frames[0][0].shape[1]
    block = np.ascontiguousarray(np.concatenate([np.full((lead, attrs), 0.9, F32)] + [p for p, _, _ in frames], 0), dtype=F32)
    n_rows = np.array([p.shape[0] for p, _, _ in frames], np.int32)
    row0 = (lead + np.concatenate([[0], np.cumsum(n_rows)[:-1]])).astype(np.uint64)
    flags = np.array([[c, m] for _, c, m in frames], np.int32)
    scale = np.ones((len(frames), 2), F32)
    out = np.zeros((len(frames), 300, 6), F32)
    n = np.zeros(len(frames), np.int32)
    L.check(L.load().yds_nms_ragged_pred(L.ptr(block), block.shape[0], attrs, len(frames), L.ptr(row0), L.ptr(n_rows), L.ptr(flags),
                                         L.ptr(scale), ct, it, L.ptr(out), 300, L.ptr(n)))
    return [out[f, :n[f]].copy() for f in range(len(frames))]


# ------------------------------------------------------------------------------------------------ references, computed once
_WANT = {}


def _want(case, merge=False):
    name, pred, conf, iou, form = case
    key = (name, pred.shape, form, merge)
    if key not in _WANT:
        with np.errstate(all="ignore"):
            if merge:
                out = onms.soft_non_max_suppression_merge(pred[None], conf, iou, is_p1p2=form == "corner")[0]
            else:
                assert form == "centre"
                out = onms.soft_non_max_suppression(pred[None], conf, iou)[0]
        _WANT[key] = EMPTY if out is None else out
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _exact(tag, got, want, nan=False):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert got.dtype == want.dtype == F32 and np.array_equal(got, want, equal_nan=nan), (tag, got, want)


def _close(tag, got, want, nan=False):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(got[:, 4:], want[:, 4:]), tag
    np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=1e-6, atol=1e-4, equal_nan=nan, err_msg=str(tag))


def _both_entries(case, nan=False, merge=True):
    """The case through yds_nms_pred and its corner twin through yds_nms_merge_pred"""
    name, pred, conf, iou, form = case
    _exact(name, _plain(pred, conf, iou), _want(case), nan)
    if merge:
        twin = E.corner_twin(case)
        _close((name, "merge"), _merge(twin[1], conf, iou), _want(twin, True), nan)


# ------------------------------------------------------------------------------------------------ groups
@pytest.mark.parametrize("thr", E.THRESHOLDS)
def test_iou_on_the_threshold(thr):
    """a: a pair whose fp32 IoU is fl(thr), one float below, one above, and fl(thr) again behind the class offset 8192 - through
    every entry.  The threshold is a double all the way to the mask kernel: at 0.4 and 0.6, where fl(thr) > thr, the on-threshold
    pair is suppressed; a float-typed entry would keep both rows."""
    cases = E.threshold_pairs(thr)
    kept = []
    for case in cases:
        _both_entries(case)
        kept.append(len(_want(case)))
    on = 1 if float(F32(thr)) > thr else 2
    assert kept == [on, 2, 1, on], kept
    twins = [E.corner_twin(c) for c in cases]
    for tw, got in zip(twins, _batched([t[1] for t in twins], 0.5, thr)):
        _exact((tw[0], "batched"), got, _merge(tw[1], 0.5, thr))
        _close((tw[0], "batched"), got, _want(tw, True))
    frames = [(cases[0][1], 0, 0), (twins[1][1], 1, 1), (cases[2][1], 0, 1), (twins[3][1], 1, 0)]
    got = _ragged(frames, 0.5, thr)
    _exact("ragged 0", got[0], _want(cases[0]))
    _close("ragged 1", got[1], _want(twins[1], True))
    _close("ragged 2", got[2], _want(cases[2], True))
    _exact("ragged 3", got[3], _want(cases[3]))                             # corner form without the merge branch: the twin's plain rows


def test_dropin_signature_takes_the_python_float():
    """a and c through yolo_deepsort_amd.model_build.soft_non_max_suppression: it receives Python floats and must decide as the
    reference does with those floats"""
    from yolo_deepsort_amd.model_build import soft_non_max_suppression
    cases = [c for thr in E.THRESHOLDS for c in E.threshold_pairs(thr)] + [E.confidence_edges(0.5), E.confidence_edges(0.1)]
    for case in cases:
        name, pred, conf, iou, form = case
        got = soft_non_max_suppression(pred[None], conf_thres=conf, iou_thres=iou)
        assert len(got) == 1
        _exact((name, "drop-in"), EMPTY if got[0] is None else got[0], _want(case))
        twin = E.corner_twin(case)
        got = soft_non_max_suppression(twin[1][None], conf_thres=conf, iou_thres=iou, merge=True, is_p1p2=True)
        _close((name, "drop-in merge"), EMPTY if got[0] is None else got[0], _want(twin, True))


@pytest.mark.parametrize("n_classes", [1, 3])
def test_lattice_storm(n_classes):
    """b: 400 integer boxes with quantised scores - dozens of IoUs exactly on the threshold and of equal scores in one greedy pass"""
    for thr in (0.4, 0.5):
        _both_entries(E.lattice_storm(n_classes, thr))


def test_confidence_edges():
    """c: objectness and class products on fl(conf) and one ulp above, a row that passes with no class, a row with all 80: count and
    emit must agree on every one, or every later slot moves"""
    for conf in (0.5, 0.1):
        case = E.confidence_edges(conf)
        _both_entries(case)
        assert len(_want(case)) == sum(E.CONF_EDGE_SLOTS) - 1


def test_ties_across_seams():
    """d: equal scores over the rank kernel's 256-candidate tile and its grid stride of 4096, the mask's 64-bit words and the cap:
    candidate-index order, min(n, 300) rows"""
    for n in E.TIE_COUNTS:
        case = E.ties(n)
        _both_entries(case, merge=n in (301, 4097))                         # (k < n: the rows stay plain; k == n would average them)
        assert len(_want(case)) == min(n, 300)
    _both_entries(E.ties_multilabel())
    for phase in (0, 63):
        case = E.ties_dup(257, phase)
        _both_entries(case)
        assert len(_want(case)) == 253


def test_box_count_seams():
    """e: the scan's carries over 64 lanes, 1024 threads and its chunks, with real counts on both sides of every seam"""
    for n_boxes in E.SEAM_BOXES:
        _both_entries(E.box_seams(n_boxes))


def test_cap_below_300():
    """f: 301 disjoint candidates; a cap of 1, 7, 299, 300 returns the first `cap` rows in score order (the merge entry sweeps to
    300 whatever the cap is: k = 300 of n = 301 leaves the rows plain)"""
    case = E.cap_case()
    twin = E.corner_twin(case)
    want = _want(case)
    assert len(want) == 300
    _exact("merge 301", _want(twin, True), want)
    for cap in E.CAPS:
        _exact(("cap", cap), _plain(case[1], case[2], case[3], cap), want[:cap])
        _exact(("merge cap", cap), _merge(twin[1], case[2], case[3], cap), want[:cap])


def test_merge_branch_limits():
    """f: k == n == 300 (every row becomes the weighted mean), one survivor of n = 2999 (merged) and of n = 3000 (plain)"""
    case = E.merge_all_kept()
    twin = E.corner_twin(case)
    got = _merge(twin[1], case[2], case[3])
    _close("all kept", got, _want(twin, True))
    assert len(got) == 300 and (got[:, :4] == got[0, :4]).all() and not np.array_equal(got[:, :4], _want(case)[:, :4])
    _exact("all kept, plain", _plain(case[1], case[2], case[3]), _want(case))
    for n in (2999, 3000):
        case = E.merge_cluster(n)
        twin = E.corner_twin(case)
        got = _merge(twin[1], case[2], case[3])
        _close(("cluster", n), got, _want(twin, True))
        plain = _plain(case[1], case[2], case[3])
        _exact(("cluster plain", n), plain, _want(case))
        assert len(got) == 1 and (np.array_equal(got, plain) if n == 3000 else np.abs(got[0, :4] - plain[0, :4]).max() > 0.5)


def test_degenerate_geometry():
    """g: zero-area boxes (NaN IoU), negative sides, identical boxes, a width of +Inf, class 79 near 4000 (fp32 step 1/32 behind
    the offset); NaN == NaN in this group only"""
    for case in E.degenerate_cases():
        _both_entries(case, nan=True)


def test_nonfinite_scores():
    """h: NaN never passes `>`; +Inf passes and ranks first"""
    case = E.nonfinite_scores()
    _both_entries(case, merge=False)
    assert np.isinf(_want(case)[:4, 4]).all() and len(_want(case)) == 6


# ------------------------------------------------------------------------------------------------ several frames in one call
def _ragged_frames():
    """(case, corner, merge) at attrs 8, conf 0.5, iou 0.4, sizes in no order: 2, 4097, 8, 65, 400, 2049, 257, 2 rows"""
    empty = ("no_candidate", E.centre_rows(E._grid(8), np.full(8, 0.3), np.full((8, 3), 0.9)), 0.5, 0.4, "centre")
    on, below, _, on2 = E.threshold_pairs(0.4)
    return [(on, 1, 1), (E.ties(4097, attrs=8), 0, 0), (empty, 0, 1), (E.ties(65, attrs=8), 1, 0), (E.lattice_storm(3, 0.4), 0, 0),
            (E.box_seams(2049), 1, 1), (E.ties_dup(257, 63, attrs=8), 0, 1), (on2, 0, 0)]


def _run_ragged():
    frames = _ragged_frames()
    return _ragged([((E.corner_twin(c) if corner else c)[1], corner, merge) for c, corner, merge in frames], 0.5, 0.4)


def _run_batched_4097():
    return _batched([E.corner_twin(E.ties(4097))[1], E.corner_twin(E.ties_dup(4097, 0))[1]], 0.5, 0.4)


def _in_fresh_thread(fn):
    """fn() on a thread of its own: the entries' workspaces are thread_local, so it starts from the 4096-candidate workspace"""
    box = {}

    def work():
        try:
            box["out"] = fn()
        except BaseException as e:                                          # handed to the caller, not lost with the thread
            box["err"] = e
    t = threading.Thread(target=work)
    t.start()
    t.join()
    if "err" in box:
        raise box["err"]
    return box["out"]


def test_ragged_call_equals_each_case_alone():
    """yds_nms_ragged_pred: frames of different lengths that do not start at row 0, both forms, with and without the merge branch,
    one frame without a candidate, the 4097-candidate frame that outgrows the 4096-candidate workspace.  Every frame equals its
    case alone - no leak from an empty neighbour or a grown workspace - and a fresh thread, whose workspace grows during the call,
    returns the same."""
    frames = _ragged_frames()
    got = _run_ragged()
    assert [len(g) for g in got] == [1, 300, 0, 65, len(_want(frames[4][0])), len(_want(frames[5][0])), 253, 1]
    for f, ((case, corner, merge), g) in enumerate(zip(frames, got)):
        name, pred, conf, iou, form = case
        twin = E.corner_twin(case)
        if merge:
            _close((f, name), g, _want(twin if corner else case, True))
            if corner:
                _exact((f, name, "alone"), g, _merge(twin[1], conf, iou))
        else:
            _exact((f, name), g, _want(case))
            _exact((f, name, "alone"), g, _plain(pred, conf, iou))
    for f, (a, b) in enumerate(zip(_in_fresh_thread(_run_ragged), got)):
        _exact((f, "thread"), a, b)


def test_batched_call_equals_each_case_alone():
    """yds_nms_merge_pred_batched: cases of equal n_boxes as frames of one call (two of 4097 candidates, one with a duplicate at
    bit 0 of every mask word), from the main thread and from a fresh one"""
    got = _run_batched_4097()
    cases = [E.ties(4097), E.ties_dup(4097, 0)]
    assert [len(g) for g in got] == [300, 300]
    for case, g in zip(cases, got):
        twin = E.corner_twin(case)
        _exact((case[0], "batched"), g, _want(case))                        # n > 3000: the merge branch stays out
        _exact((case[0], "alone"), g, _merge(twin[1], 0.5, 0.4))
    for f, (a, b) in enumerate(zip(_in_fresh_thread(_run_batched_4097), got)):
        _exact((f, "thread"), a, b)
    seams = [E.corner_twin(E.box_seams(257)), E.corner_twin(E.ties_dup(257, 0, attrs=8)), E.corner_twin(E.ties_dup(257, 63, attrs=8))]
    for tw, g in zip(seams, _batched([t[1] for t in seams], 0.5, 0.4)):
        _close((tw[0], "batched"), g, _want(tw, True))
        _exact((tw[0], "alone"), g, _merge(tw[1], 0.5, 0.4))


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_refusals_keep_their_messages():
    lib = L.load()
    L.init()
    out = np.zeros((4, 300, 6), F32)
    n = np.zeros(4, np.int32)
    p5 = np.full((4, 5), 0.9, F32)
    p6 = np.full((8, 6), 0.9, F32)
    one = C.c_int(0)

    def refused(rc, text):
        assert rc != 0 and text in L.last_error(), L.last_error()
    refused(lib.yds_nms_pred(L.ptr(p5), 4, 5, 0.5, 0.4, L.ptr(out), 300, C.byref(one)), "nms: predictions need at least one class")
    refused(lib.yds_nms_merge_pred(L.ptr(p5), 4, 5, 0.5, 0.4, L.ptr(out), 300, C.byref(one)), "nms: predictions need at least one class")
    refused(lib.yds_nms_merge_pred_batched(L.ptr(p5), 2, 2, 5, 0.5, 0.4, L.ptr(out), 300, L.ptr(n)), "nms: predictions need at least one class")
    refused(lib.yds_nms_merge_pred_batched(L.ptr(p6), 0, 8, 6, 0.5, 0.4, L.ptr(out), 300, L.ptr(n)), "nms: 0 frames of 8 boxes")
    refused(lib.yds_nms_merge_pred_batched(L.ptr(p6), 2, 0, 6, 0.5, 0.4, L.ptr(out), 300, L.ptr(n)), "nms: 2 frames of 0 boxes")
    row0 = np.array([0, 4], np.uint64)
    flags = np.zeros((2, 2), np.int32)
    scale = np.ones((2, 2), F32)

    def ragged(pred, n_frames, n_rows):
        return lib.yds_nms_ragged_pred(L.ptr(pred), pred.shape[0], pred.shape[1], n_frames, L.ptr(row0), L.ptr(np.array(n_rows, np.int32)),
                                       L.ptr(flags), L.ptr(scale), 0.5, 0.4, L.ptr(out), 300, L.ptr(n))
    refused(ragged(p6, 0, [4, 4]), "nms: 0 frames")
    refused(ragged(p6, 2, [4, 5]), "nms: frame 1 holds rows [4, +5) of 8")
    refused(ragged(p6, 2, [0, 4]), "nms: frame 0 holds rows [0, +0) of 8")
    refused(ragged(np.full((8, 5), 0.9, F32), 2, [4, 4]), "nms: predictions need at least one class")
    _exact("after the refusals", _plain(E.ties(63)[1], 0.5, 0.4), _want(E.ties(63)))          # the entries still work
