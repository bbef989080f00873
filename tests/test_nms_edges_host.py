"""The detector-NMS edge cases (tests/nms_edge_cases.py) on the CPU: every case hits what it claims, and the oracle
(oracle/nms.py) equals, bit for bit, a second statement of the rule that shares no code with it (nms_naive: Python loops over
np.float32 scalars, an explicit stable sort, float(ovr) > float(thr)).  tests/test_gpu_nms_edges.py runs the same cases on the
device."""
import numpy as np
import pytest

import nms_edge_cases as E
from oracle import nms as onms

F32 = np.float32


def _oracle(case):
    name, pred, conf, iou, form = case
    assert form == "centre"
    with np.errstate(all="ignore"):
        out = onms.soft_non_max_suppression(pred[None], conf, iou)[0]
    return np.zeros((0, 6), F32) if out is None else out


def _oracle_merge(case):
    name, pred, conf, iou, form = case
    with np.errstate(all="ignore"):
        out = onms.soft_non_max_suppression_merge(pred[None], conf, iou, is_p1p2=form == "corner")[0]
    return np.zeros((0, 6), F32) if out is None else out


def _same(case, nan=False):
    """naive == oracle on the centre form; on the corner twin the naive rows equal the merge oracle's in score and class, and in the
    boxes too where its merge branch leaves them alone.  Returns the rows."""
    name, pred, conf, iou, form = case
    want = _oracle(case)
    got = E.nms_naive(pred, conf, iou, form)
    assert got.dtype == F32 and got.shape == want.shape, (name, got.shape, want.shape)
    assert np.array_equal(got, want, equal_nan=nan), name
    twin = E.corner_twin(case)
    n = len(E.candidates_naive(twin[1], conf, "corner")[0])
    merged = _oracle_merge(twin)
    got2 = E.nms_naive(twin[1], conf, iou, "corner")
    assert np.array_equal(got2, got, equal_nan=nan), name                   # the twin holds the same candidates
    fires = 1 < n < 3000 and len(got) in (1, n)
    assert merged.shape == got.shape and np.array_equal(merged[:, 4:], got[:, 4:]), name
    if not fires:
        assert np.array_equal(merged, got, equal_nan=nan), name
    return got


def _pair_ovr(case):
    rows, _ = E.candidates_naive(case[1], case[2], case[4])
    assert len(rows) == 2
    a, b = E.offset_boxes(rows)
    with np.errstate(all="ignore"):
        return E.pair_ovr(a, b)


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("thr", E.THRESHOLDS)
def test_threshold_pairs_sit_where_they_claim(thr):
    on, below, above, on2 = E.threshold_pairs(thr)
    t = F32(thr)
    assert _pair_ovr(on) == t and _pair_ovr(on2) == t                      # class 2: the offset 8192 leaves the IoU where it was
    assert _pair_ovr(below) == np.nextafter(t, F32(0)) and _pair_ovr(above) == np.nextafter(t, F32(1))
    assert E.offset_boxes(E.candidates_naive(on2[1], 0.5, "centre")[0])[0][0] == F32(8192)
    kept = [len(_same(c)) for c in (on, below, above, on2)]
    on_kept = 1 if float(t) > thr else 2                                    # fl(thr) > thr: the on-threshold pair is suppressed
    assert kept == [on_kept, 2, 1, on_kept], kept
    for c in (on, on2):
        rounded = onms.soft_non_max_suppression(c[1][None], 0.5, float(t))[0]
        assert len(rounded) == 2                                            # (double)fl(thr) as the threshold never suppresses it
    if thr in (0.4, 0.6):
        assert float(t) > thr and kept[0] == 1                              # ... which is what a float-typed entry computes: 2 rows for 1


def test_threshold_pair_table_is_what_the_search_finds():
    for (thr, kind), sizes in E.NEIGHBOUR_SIZES.items():
        assert E.find_pair(E.neighbour_target(thr, kind), E.NEIGHBOUR_LIMIT.get((thr, kind), 2048)) == sizes, (thr, kind)


# ------------------------------------------------------------------------------------------------ b
def _storm_counts(case):
    """(same-class candidate pairs whose fp32 IoU is fl(thr), score values shared by two or more candidates)"""
    name, pred, conf, iou, form = case
    rows = np.array(E.candidates_naive(pred, conf, form)[0], F32)
    b = np.array(E.offset_boxes([list(r) for r in rows]), F32)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = np.maximum(F32(0), np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]))
    h = np.maximum(F32(0), np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]))
    inter = w * h
    ovr = inter / ((area[:, None] + area[None, :]) - inter)
    assert ovr.dtype == F32
    on = np.triu(ovr == F32(iou), 1) & (rows[:, None, 5] == rows[None, :, 5])
    values, counts = np.unique(rows[:, 4], return_counts=True)
    return int(on.sum()), int((counts > 1).sum()), len(rows)


@pytest.mark.parametrize("n_classes", [1, 3])
@pytest.mark.parametrize("thr", [0.4, 0.5])
def test_lattice_storm_has_on_threshold_pairs_and_ties(n_classes, thr):
    case = E.lattice_storm(n_classes, thr)
    pairs, groups, n = _storm_counts(case)
    print(case[0], "candidates", n, "pairs on the threshold", pairs, "groups of equal scores", groups)
    assert pairs >= 20 and groups >= 50
    assert np.array_equal(case[1][:, :4] % 0.5, np.zeros((400, 4)))         # integer corners: centres in halves
    kept = _same(case)
    rounded = onms.soft_non_max_suppression(case[1][None], case[2], float(F32(thr)))[0]
    if thr == 0.4:
        assert kept.shape != rounded.shape or not np.array_equal(kept, rounded)     # the storm, too, tells the two thresholds apart


# ------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("conf", [0.5, 0.1])
def test_confidence_edges_slots(conf):
    case = E.confidence_edges(conf)
    pred, ct = case[1], F32(conf)
    obj3, c_on, c_above = E._product_edge(conf)
    assert pred[1, 4] == ct and pred[2, 4] == np.nextafter(ct, F32(1)) and obj3 > ct
    assert obj3 * c_on == ct and obj3 * c_above == np.nextafter(ct, F32(1))
    rows, per_box = E.candidates_naive(pred, conf, "centre")
    assert per_box == E.CONF_EDGE_SLOTS and pred.shape[1] == 85
    kept = _same(case)
    assert len(kept) == sum(per_box) - 1                                    # every candidate but the duplicate in the last row
    assert kept[-1, 4] == np.nextafter(ct, F32(1))                          # the lowest score is one ulp above the threshold
    assert (kept[:, 5] == 3).sum() == 2                                     # class 3: row 0 and the row of 80, not row 7


# ------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("n", E.TIE_COUNTS)
def test_ties_keep_candidate_order(n):
    case = E.ties(n)
    rows, per_box = E.candidates_naive(case[1], case[2], "centre")
    assert len(rows) == n and len({float(r[4]) for r in rows}) == 1
    kept = _same(case)
    assert np.array_equal(kept, np.array(rows[:min(n, 300)], F32))


def test_ties_multilabel_and_duplicates():
    case = E.ties_multilabel()
    kept = _same(case)
    assert kept[:, 5].tolist() == [0, 0, 2, 0, 1] and len(set(kept[:, 4].tolist())) == 1
    assert np.array_equal(kept[1, :4], kept[2, :4])
    for phase in (0, 63):
        case = E.ties_dup(257, phase)
        trace = []
        want = E.nms_naive(case[1], case[2], case[3], "centre", trace=trace)
        assert len(trace) == 4 and {j % 64 for j in trace} == {phase}          # the suppressed bits sit at one end of a mask word
        assert np.array_equal(_same(case), want) and len(want) == 253


# ------------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("n_boxes", E.SEAM_BOXES)
def test_box_seams_carry_counts(n_boxes):
    case = E.box_seams(n_boxes)
    rows, per_box = E.candidates_naive(case[1], case[2], "centre")
    assert len(per_box) == n_boxes and set(per_box) == {0, 1, 3} and per_box[-1] == 1
    assert 200 < len(rows) <= 300 and len({float(r[4]) for r in rows}) == len(rows)
    for seam in range(64, n_boxes, 64):
        assert sum(per_box[:seam]) > 0                                      # a real count is carried over every seam
    for seam in range(256, n_boxes, 256):
        assert per_box[seam - 1] and per_box[seam]
    no_slot = [i for i, c in enumerate(per_box) if c == 0]
    assert any(case[1][i, 4] > 0.5 for i in no_slot) and any(case[1][i, 4] < 0.5 for i in no_slot)
    kept = _same(case)
    assert len(kept) == len(rows) - 3                                       # every candidate but one box's three shows in the result


# ------------------------------------------------------------------------------------------------ f
def test_cap_and_merge_cases():
    case = E.cap_case()
    rows, _ = E.candidates_naive(case[1], case[2], "centre")
    assert len(rows) == 301 and len({float(r[4]) for r in rows}) == 301
    kept = _same(case)
    assert len(kept) == 300 and (np.diff(kept[:, 4]) < 0).all()
    for cap in E.CAPS:
        assert np.array_equal(E.nms_naive(case[1], case[2], case[3], "centre", max_det=cap), kept[:cap])
    case = E.merge_all_kept()
    kept = _same(case)
    merged = _oracle_merge(E.corner_twin(case))
    assert len(kept) == 300 and len(merged) == 300
    w = kept[:, 4].astype(np.float64)
    mean = (w[:, None] * kept[:, :4]).sum(0) / w.sum()
    assert np.array_equal(merged[:, :4], np.tile(mean.astype(F32), (300, 1)))          # exact sums: the mean in any order
    for n in (2999, 3000):
        case = E.merge_cluster(n)
        rows, _ = E.candidates_naive(case[1], case[2], "centre")
        kept = _same(case)
        merged = _oracle_merge(E.corner_twin(case))
        assert len(rows) == n and len(kept) == 1 and len(merged) == 1
        best = [r for r in rows if r[4] == 1][0]
        assert np.array_equal(kept[0], np.array(best, F32))
        if n == 3000:
            assert np.array_equal(merged, kept)
        else:
            allr = np.array(rows, np.float64)
            mean = (allr[:, 4:5] * allr[:, :4]).sum(0) / allr[:, 4].sum()
            assert np.array_equal(merged[0, :4], mean.astype(F32)) and np.abs(merged[0, :4] - kept[0, :4]).max() > 0.5


# ------------------------------------------------------------------------------------------------ g, h
def test_degenerate_geometry_and_nonfinite_scores():
    kept = {c[0]: _same(c, nan=True) for c in E.degenerate_cases()}
    assert set(kept) == {"zero_area", "negative_sides", "identical", "inf_width", "class79_near_4000"}
    assert len(kept["zero_area"]) == 5                                      # the two identical zero-area boxes both stay (NaN IoU)
    assert np.array_equal(kept["zero_area"][0], kept["zero_area"][1] + np.array([0, 0, 0, 0, kept["zero_area"][0, 4] - kept["zero_area"][1, 4], 0], F32))
    assert kept["identical"][:, 5].tolist() == [0, 1]
    assert np.isinf(kept["inf_width"][:, :4]).any() and not np.isnan(kept["inf_width"]).any()
    c79 = [c for c in E.degenerate_cases() if c[0] == "class79_near_4000"][0]
    rows, _ = E.candidates_naive(c79[1], 0.5, "centre")
    off = np.array(E.offset_boxes(rows), F32)
    raw = np.array(rows, F32)
    hi = raw[:, 5] == 79
    assert hi.any() and np.array_equal(off[hi] * 32 % 1, np.zeros_like(off[hi]))       # offset corners sit on the 1/32 grid ...
    assert ((raw[hi, :4] * 32 % 1) != 0).any()                                          # ... which the corners themselves do not
    case = E.nonfinite_scores()
    rows, per_box = E.candidates_naive(case[1], case[2], "centre")
    assert per_box == E.NONFINITE_SLOTS
    kept = _same(case)
    assert np.isinf(kept[:4, 4]).all() and np.isfinite(kept[4:, 4]).all() and len(kept) == 6
    assert np.array_equal(kept[:4], np.array([r for r in rows if np.isinf(r[4])], F32))  # the Inf scores first, in index order
