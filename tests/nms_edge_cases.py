"""Shared pieces of the detector-NMS edge tests (tests/test_nms_edges_host.py, tests/test_gpu_nms_edges.py): the case builders and a
naive statement of the rule.

A case is (name, pred [N, 5 + C] float32, conf_thres, iou_thres, form); form "centre": rows hold cx, cy, w, h (yds_nms_pred,
oracle.nms.soft_non_max_suppression), "corner": x1, y1, x2, y2 (yds_nms_merge_pred, soft_non_max_suppression_merge).  Every
builder makes the centre form; corner_twin() gives the corner form that holds the same candidates bit for bit.

Groups: a threshold_pairs, b lattice_storm, c confidence_edges, d ties / ties_multilabel / ties_dup, e box_seams, f cap_case and
merge_all_kept / merge_cluster, g degenerate_cases, h nonfinite_scores.

NaN COORDINATES ARE EXCLUDED: fmaxf, np.maximum and std::max disagree on a NaN operand, and the network cannot produce a NaN box
without an earlier Inf.  nms_naive asserts that no NaN reaches a max or a min, so the exclusion is checked for every case.
"""
import numpy as np

F32 = np.float32
MAX_WH, MAX_DET = 4096, 300
THRESHOLDS = (0.4, 0.6, 0.45, 0.5, 0.25, 0.75)


# ------------------------------------------------------------------------------------------------ forms
def centre_rows(corners, obj, cls):
    """[N, 5 + C] centre-form rows whose fp32 corners (x -+ w/2, as the emit stage computes them) are exactly `corners`"""
    corners = np.asarray(corners, np.float64).reshape(-1, 4)
    cls = np.asarray(cls, F32).reshape(len(corners), -1)
    p = np.zeros((len(corners), 5 + cls.shape[1]), F32)
    p[:, 0] = (corners[:, 0] + corners[:, 2]) / 2
    p[:, 1] = (corners[:, 1] + corners[:, 3]) / 2
    p[:, 2] = corners[:, 2] - corners[:, 0]
    p[:, 3] = corners[:, 3] - corners[:, 1]
    p[:, 4] = obj
    p[:, 5:] = cls
    assert np.array_equal(corners_of(p), corners.astype(F32)), "corners are not exact in centre form"
    return p


def corners_of(pred):
    """fp32 corners of centre-form rows: x -+ w/2, one division, one subtraction / addition (model_build.py:317-323)"""
    with np.errstate(all="ignore"):
        half = (pred[:, 2:4] / F32(2)).astype(F32)
        return np.concatenate([(pred[:, :2] - half).astype(F32), (pred[:, :2] + half).astype(F32)], 1)


def corner_twin(case):
    """The corner-form case with the same candidates, bit for bit"""
    name, pred, conf, iou, form = case
    if form == "corner":
        return case
    twin = pred.copy()
    twin[:, :4] = corners_of(pred)
    return (name, twin, conf, iou, "corner")


def _grid(n, pitch=10, side=8, cols=64):
    """n pairwise disjoint integer boxes"""
    i = np.arange(n)
    x, y = (i % cols) * pitch, (i // cols) * pitch
    return np.stack([x, y, x + side, y + side], 1)


# ------------------------------------------------------------------------------------------------ the naive reference
def _stable_order(score):
    """Indices by score descending, equal scores in index order: an explicit merge sort (left run first on a tie)"""
    def sort(idx):
        if len(idx) < 2:
            return idx
        a, b = sort(idx[:len(idx) // 2]), sort(idx[len(idx) // 2:])
        out, i, j = [], 0, 0
        while i < len(a) and j < len(b):
            if score[b[j]] > score[a[i]]:
                out.append(b[j]); j += 1
            else:
                out.append(a[i]); i += 1
        return out + a[i:] + b[j:]
    return sort(list(range(len(score))))


def candidates_naive(pred, conf, form):
    """([x1, y1, x2, y2, score, cls] per candidate in box-major, class-minor order, candidates per box): obj > fl(conf), then every
    class with fl(cls * obj) > fl(conf)"""
    ct = F32(conf)
    rows, per_box = [], []
    with np.errstate(all="ignore"):
        for p in pred:
            cnt = 0
            if p[4] > ct:
                if form == "corner":
                    box = [p[0], p[1], p[2], p[3]]
                else:
                    hw, hh = p[2] / F32(2), p[3] / F32(2)
                    box = [p[0] - hw, p[1] - hh, p[0] + hw, p[1] + hh]
                for j in range(5, len(p)):
                    sc = p[j] * p[4]
                    if sc > ct:
                        rows.append(box + [sc, F32(j - 5)])
                        cnt += 1
            per_box.append(cnt)
    assert all(type(v) is F32 for r in rows for v in r)
    return rows, per_box


def _max(a, b):
    assert a == a and b == b, "NaN operand of max"
    return a if a > b else b


def _min(a, b):
    assert a == a and b == b, "NaN operand of min"
    return a if a < b else b


def pair_ovr(bi, bj):
    """fp32 IoU of two class-offset boxes, operation by operation as torchvision's CPU kernel (0 / 0 and Inf - Inf are part of
    the cases: call it under np.errstate(all="ignore"))"""
    ai = (bi[2] - bi[0]) * (bi[3] - bi[1])
    aj = (bj[2] - bj[0]) * (bj[3] - bj[1])
    w = _max(F32(0), _min(bi[2], bj[2]) - _max(bi[0], bj[0]))
    h = _max(F32(0), _min(bi[3], bj[3]) - _max(bi[1], bj[1]))
    inter = w * h
    ovr = inter / ((ai + aj) - inter)
    assert type(ovr) is F32
    return ovr


def offset_boxes(rows):
    with np.errstate(all="ignore"):
        return [[r[k] + r[5] * F32(MAX_WH) for k in range(4)] for r in rows]


def nms_naive(pred, conf, iou, form, max_det=MAX_DET, trace=None):
    """[k, 6] float32: candidates, class offset, stable sort, greedy suppression with float(ovr) > float(thr), first max_det kept.
    The loop stops at max_det kept rows: a later row cannot change an earlier decision, and the reference cuts the list there.
    trace (a list) receives the sorted positions that were suppressed."""
    rows, _ = candidates_naive(pred, conf, form)
    order = _stable_order([r[4] for r in rows])
    rows = [rows[i] for i in order]
    boxes = offset_boxes(rows)
    thr = float(iou)
    dead = [False] * len(rows)
    keep = []
    with np.errstate(all="ignore"):
        for i in range(len(rows)):
            if dead[i]:
                continue
            keep.append(i)
            if len(keep) == max_det:
                break
            for j in range(i + 1, len(rows)):
                if not dead[j] and float(pair_ovr(boxes[i], boxes[j])) > thr:
                    dead[j] = True
                    if trace is not None:
                        trace.append(j)
    return np.array([rows[i] for i in keep], F32).reshape(-1, 6)


# ------------------------------------------------------------------------------------------------ a. IoU on the threshold
# A = (0, 0, wa, ha), B = (0, 0, wb, hb).  "on": the integer pairs whose intersection / union is the threshold itself, so the fp32
# quotient is fl(thr).  "below" / "above": the first hit of find_pair() for the neighbouring float - their areas pass 2**24, the
# fp32 sums round, and the quotient of the rounded values is what lands on the neighbour (the host test recomputes it).
ON_PAIRS = {0.4: ((0, 0, 7, 10), (3, 0, 10, 10)), 0.6: ((0, 0, 4, 10), (1, 0, 5, 10)), 0.45: ((0, 0, 29, 10), (11, 0, 40, 10)),
            0.5: ((0, 0, 3, 10), (1, 0, 4, 10)), 0.25: ((0, 0, 5, 10), (3, 0, 8, 10)), 0.75: ((0, 0, 7, 10), (1, 0, 8, 10))}

def find_pair(target, lim, seed=0, n=2_000_000):
    """Integer sizes (wa, ha, wb, hb), wb < wa and hb >= ha, whose fp32 IoU - computed as the mask kernel does - is `target`:
    a draw of n size triples below `lim`, hb solved for the ratio, the first hit"""
    rs = np.random.RandomState(seed)
    wa = rs.randint(lim // 2, lim, n).astype(np.int64)
    ha = rs.randint(lim // 2, lim, n).astype(np.int64)
    wb = rs.randint(lim // 4, wa)
    hb = ha + np.rint((wb * ha / float(target) - wa * ha) / wb).astype(np.int64)
    f = [v.astype(F32) for v in (wa, ha, wb, hb)]
    inter = f[2] * f[1]
    ovr = inter / ((f[0] * f[1] + f[2] * f[3]) - inter)
    hit = np.flatnonzero((hb >= ha) & (hb < 2 * lim) & (ovr == target))
    return tuple(int(v[hit[0]]) for v in (wa, ha, wb, hb)) if len(hit) else None


NEIGHBOUR_LIMIT = {(0.5, "below"): 4096, (0.25, "below"): 4096}          # every other target is met below 2048
NEIGHBOUR_SIZES = {          # (thr, "below" | "above") -> (wa, ha, wb, hb)
    (0.4, "below"): (1891, 1227, 1693, 2924), (0.4, "above"): (1671, 1657, 1055, 3175),
    (0.6, "below"): (1319, 1981, 928, 2467), (0.6, "above"): (1986, 2021, 1820, 3184),
    (0.45, "below"): (1978, 1959, 1456, 3651), (0.45, "above"): (1632, 1496, 1625, 3318),
    (0.5, "below"): (3844, 2771, 2771, 4469), (0.5, "above"): (1875, 1811, 1586, 3292),
    (0.25, "below"): (3847, 2151, 2806, 7806), (0.25, "above"): (1933, 1027, 1496, 3808),
    (0.75, "below"): (1326, 1988, 1177, 2399), (0.75, "above"): (1765, 1739, 1538, 2062),
}


def neighbour_target(thr, kind):
    return np.nextafter(F32(thr), F32(0 if kind == "below" else 1))


def _pair_case(name, a, b, thr, cls, conf=0.5):
    """Two boxes of class `cls` (attrs 8), the first with the higher score"""
    c = np.zeros((2, 3), F32)
    c[:, cls] = 1.0
    return (name, centre_rows([a, b], [0.9, 0.8], c), conf, thr, "centre")


def threshold_pairs(thr):
    """on / below / above at class 0 and the on-threshold pair at class 2 (offset 8192 added before the IoU)"""
    out = [_pair_case(f"iou{thr}_on", *ON_PAIRS[thr], thr, 0)]
    for kind in ("below", "above"):
        wa, ha, wb, hb = NEIGHBOUR_SIZES[thr, kind]
        out.append(_pair_case(f"iou{thr}_{kind}", (0, 0, wa, ha), (0, 0, wb, hb), thr, 0))
    out.append(_pair_case(f"iou{thr}_on_class2", *ON_PAIRS[thr], thr, 2))
    return out


# ------------------------------------------------------------------------------------------------ b. lattice storm
STORM_SEED = 8          # the first seed whose storms, with one class and with three, meet the host test's pair and tie counts at 0.4 and 0.5


def lattice_storm(n_classes, thr, conf=0.5):
    """400 boxes, corners on a 40 x 40 lattice, sides 2..12, objectness 1, class scores conf + k / 16 with k in 1..80 (scores above
    1: the kernels do not care, and 80 values among 400+ candidates give many groups of equal scores); with three classes a class
    passes with probability 0.6"""
    rs = np.random.RandomState(STORM_SEED)
    xy = rs.randint(0, 40, (400, 2))
    wh = rs.randint(2, 13, (400, 2))
    cls = conf + rs.randint(1, 81, (400, n_classes)) / 16.0
    if n_classes > 1:
        cls = np.where(rs.rand(400, n_classes) < 0.6, cls, 0.25)
    return (f"storm_c{n_classes}_iou{thr}", centre_rows(np.concatenate([xy, xy + wh], 1), np.ones(400), cls), conf, thr, "centre")


# ------------------------------------------------------------------------------------------------ c. confidence edges
def _product_edge(conf):
    """(obj, cls_on, cls_above): obj > fl(conf), fl(obj * cls_on) == fl(conf), fl(obj * cls_above) == nextafter(fl(conf), 1)"""
    ct = F32(conf)
    up = np.nextafter(ct, F32(1))
    for obj in (F32(0.8125), F32(0.9375), F32(0.7), F32(0.6)):
        c = F32(ct / obj)
        near = [c]
        for _ in range(8):
            near = [np.nextafter(near[0], F32(0))] + near + [np.nextafter(near[-1], F32(1))]
        on = [v for v in near if v * obj == ct]
        above = [v for v in near if v * obj == up]
        if on and above:
            return obj, on[0], above[0]
    raise AssertionError("no product edge")


def confidence_edges(conf):
    """attrs 85, disjoint boxes.  Rows: 0 plain; 1 obj == fl(conf): out; 2 obj one ulp above with class score 1: in; 3 obj * cls
    rounds to fl(conf): out; 4 the product one ulp above: in; 5 obj passes, none of the 80 products does: no slot; 6 all 80 pass:
    80 slots; 7 the box and class of row 0 at a lower score: a slot, and suppressed, so that k < n keeps the merge branch (whose
    fp32 sums the oracle takes in another order) out of the corner twin.  The expected candidates per row are CONF_EDGE_SLOTS."""
    ct = F32(conf)
    up = np.nextafter(ct, F32(1))
    obj3, c_on, c_above = _product_edge(conf)
    obj = np.array([0.9, ct, up, obj3, obj3, up, 1.0, 0.95], F32)
    cls = np.zeros((8, 80), F32)
    cls[0, 3] = 0.9
    cls[1, :] = 1.0
    cls[2, 5] = 1.0
    cls[3, 7] = c_on
    cls[4, 7] = c_above
    cls[5, :] = 0.99
    cls[6, :] = conf + (1 - conf) * (np.arange(80) + 1) / 81.0
    cls[7, 3] = 0.9
    boxes = _grid(8, pitch=20, side=10)
    boxes[7] = boxes[0]
    return (f"conf_edges_{conf}", centre_rows(boxes, obj, cls), conf, 0.4, "centre")


CONF_EDGE_SLOTS = [1, 0, 1, 0, 1, 0, 80, 1]


# ------------------------------------------------------------------------------------------------ d. ties across seams
TIE_COUNTS = (63, 64, 65, 128, 129, 255, 256, 257, 300, 301, 1025, 4097)


def ties(n, attrs=6, conf=0.5, iou=0.4):
    """n pairwise disjoint boxes of class 0, every score fl(0.9 * 0.9)"""
    cls = np.zeros((n, attrs - 5), F32)
    cls[:, 0] = 0.9
    return (f"ties_{n}", centre_rows(_grid(n), np.full(n, 0.9), cls), conf, iou, "centre")


def ties_multilabel():
    """Four disjoint boxes of equal scores; box 1 passes with classes 0 and 2: five candidates in index order"""
    cls = np.zeros((4, 3), F32)
    cls[:, 0] = 0.9
    cls[1, 2] = 0.9
    cls[3] = (0.0, 0.9, 0.0)
    return ("ties_multilabel", centre_rows(_grid(4), np.full(4, 0.9), cls), 0.5, 0.4, "centre")


def ties_dup(n, phase, attrs=6):
    """ties(n) where every candidate i > 0 with i % 64 == phase holds the box of candidate i - 1: with equal scores the sorted order
    is the index order, so the suppressed bits are bit `phase` of every mask word (0 and 63 are the word's two ends)"""
    name, pred, conf, iou, form = ties(n, attrs)
    dup = [i for i in range(1, n) if i % 64 == phase]
    pred[dup, :4] = pred[[i - 1 for i in dup], :4]
    return (f"ties_{n}_dup{phase}", pred, conf, iou, form)


# ------------------------------------------------------------------------------------------------ e. box-count seams
SEAM_BOXES = (255, 256, 257, 1023, 1024, 1025, 2049)


def box_seams(n_boxes, conf=0.5, iou=0.4):
    """n_boxes disjoint boxes, three classes, candidates per box drawn from {0, 1, 3}; the boxes on both sides of every 64-lane,
    256-thread and 1024-thread seam and the final row pass; at most 300 candidates with distinct scores in all, so every one of
    them but three is in the result and a slot that moved shows: one box of three candidates holds the box of another, so
    that k = n - 3 keeps the merge branch (whose fp32 sums the oracle takes in another order) out of the corner twin.  Of the boxes
    without a candidate, half fail on the objectness and half pass it with no class above the threshold."""
    rs = np.random.RandomState(n_boxes)
    cnt = np.zeros(n_boxes, np.int64)
    seams = sorted({i for s in range(64, n_boxes, 64) for i in (s - 1, s)} | {n_boxes - 1})
    seams = [i for i in seams if i % 256 in (255, 0) or i % 64 == 63 and rs.rand() < 0.5 or i == n_boxes - 1]
    cnt[seams] = rs.choice([1, 3], len(seams))
    cnt[n_boxes - 1] = 1
    rest = rs.permutation(np.flatnonzero(cnt == 0))
    for i in rest:
        c = rs.choice([1, 3])
        if cnt.sum() + c > 290:
            break
        cnt[i] = c
    n_cand = int(cnt.sum())
    score = rs.permutation(np.arange(1, 401))[:n_cand] / 1024.0 + 0.55          # distinct, above conf, exact in fp32
    obj = np.ones(n_boxes, F32)
    cls = np.full((n_boxes, 3), 0.25, F32)
    s = 0
    for i in range(n_boxes):
        if cnt[i] == 0:
            if i % 2:
                obj[i], cls[i] = 0.3, 0.9
            continue
        which = [0, 1, 2] if cnt[i] == 3 else [rs.randint(3)]
        for j in which:
            cls[i, j] = score[s]
            s += 1
    boxes = _grid(n_boxes, pitch=12)
    three = np.flatnonzero(cnt == 3)
    boxes[three[1]] = boxes[three[0]]
    return (f"seams_{n_boxes}", centre_rows(boxes, obj, cls), conf, iou, "centre")


# ------------------------------------------------------------------------------------------------ f. cap and merge edges
CAPS = (1, 7, 299, 300)


def cap_case(attrs=6):
    """301 disjoint candidates of class 0 with distinct scores in shuffled order"""
    rs = np.random.RandomState(301)
    cls = np.zeros((301, attrs - 5), F32)
    cls[:, 0] = rs.permutation(np.arange(1, 302)) / 1024.0 + 0.55
    return ("cap_301", centre_rows(_grid(301), np.ones(301), cls), 0.5, 0.4, "centre")


def merge_all_kept():
    """n = k = 300: disjoint 2 x 2 boxes with corners below 64, scores k / 512 descending in candidate order (conf 0.25).  Kept row j
    is paired with candidate j, so every weight is the score and every row becomes the weighted mean of all 300 boxes.  The products
    score * coordinate and their sums are below 2**24 units of 1 / 512: the mean is exact in any summation order."""
    i = np.arange(300)
    x, y = (i % 20) * 3, (i // 20) * 3
    cls = ((512 - i) / 512.0)[:, None]
    return ("merge_300_all_kept", centre_rows(np.stack([x, y, x + 2, y + 2], 1), np.ones(300), cls), 0.25, 0.4, "centre")


def merge_cluster(n):
    """n near-identical boxes of one class: corners (100, 100, 220, 220) moved by multiples of 1/4 within +-3, scores 0.75 or 1.
    One survivor (the first of the 1s).  Coordinates below 256 in quarters times weights in quarters, summed over < 3000 rows, stay
    below 2**24 units of 1/16: the weighted mean is exact in any summation order."""
    rs = np.random.RandomState(n)
    j = rs.randint(-12, 13, (n, 4)) / 4.0
    cls = np.where(rs.rand(n) < 0.5, 0.75, 1.0)[:, None]
    cls[0] = 0.75
    return (f"merge_cluster_{n}", centre_rows(np.array([100, 100, 220, 220]) + j, np.ones(n), cls), 0.5, 0.4, "centre")


# ------------------------------------------------------------------------------------------------ g. degenerate geometry
def degenerate_cases():
    one = lambda n: np.ones((n, 1), F32)
    score = lambda n: np.linspace(0.95, 0.6, n)
    out = []
    # two identical zero-area boxes (0 / 0: NaN, never above the threshold), a zero-width and a zero-height box inside a real one
    p = np.array([[50, 50, 0, 0], [50, 50, 0, 0], [100, 100, 40, 40], [100, 100, 0, 20], [100, 100, 20, 0], [100, 100, 40, 40]], F32)
    out.append(("zero_area", np.concatenate([p, score(6)[:, None].astype(F32), one(6)], 1), 0.5, 0.4, "centre"))
    # negative width and / or height: x1 > x2; the areas change sign, the clamped intersection is 0 or positive
    p = np.array([[100, 100, -40, 40], [102, 100, -40, 40], [100, 100, 40, 40], [100, 100, -40, -40], [101, 101, -38, -38],
                  [100, 100, 40, -40]], F32)
    out.append(("negative_sides", np.concatenate([p, score(6)[:, None].astype(F32), one(6)], 1), 0.5, 0.4, "centre"))
    # identical boxes: IoU exactly 1; distinct and equal scores, and one of another class that stays
    p = np.array([[100, 100, 40, 30]] * 5, F32)
    c = np.zeros((5, 2), F32)
    c[:4, 0] = 1.0
    c[4, 1] = 1.0
    out.append(("identical", np.concatenate([p, np.array([[0.9], [0.8], [0.8], [0.95], [0.7]], F32), c], 1), 0.5, 0.4, "centre"))
    # width +inf (exp overflow in the decode): corners -inf / +inf, area inf; two of them give inf / NaN; height 0 gives a NaN area
    inf = np.inf
    p = np.array([[100, 100, inf, 40], [100, 110, inf, 40], [100, 100, 40, 40], [300, 300, inf, 0], [100, 100, inf, inf],
                  [500, 500, 20, 20]], F32)
    out.append(("inf_width", np.concatenate([p, score(6)[:, None].astype(F32), one(6)], 1), 0.5, 0.4, "centre"))
    # class 79: offset 79 * 4096 = 323584, where fp32 steps by 1/32; corners in 1/64ths near 4000 round before the IoU
    rs = np.random.RandomState(79)
    base = 3990 + rs.randint(0, 4 * 64, (24, 2)) / 64.0
    wh = 2 + rs.randint(0, 3 * 64, (24, 2)) / 64.0
    c = np.zeros((24, 80), F32)
    c[:, 79] = 1.0
    c[::5, 78] = 1.0
    p = np.concatenate([base + wh / 2, wh], 1).astype(F32)
    out.append(("class79_near_4000", np.concatenate([p, np.linspace(0.99, 0.6, 24)[:, None].astype(F32), c], 1), 0.5, 0.4, "centre"))
    return out


# ------------------------------------------------------------------------------------------------ h. non-finite scores
NONFINITE_SLOTS = [1, 0, 1, 0, 0, 0, 1, 0, 1, 2]


def nonfinite_scores():
    """attrs 8, disjoint boxes.  NaN never passes `>`; +Inf passes and ranks first (two of them in index order); Inf * 0 is NaN."""
    nan, inf = np.nan, np.inf
    obj = np.array([0.9, nan, inf, inf, -inf, 0.9, 0.9, 0.9, 0.8, inf], F32)
    cls = np.array([[0.9, 0, 0], [1, 1, 1], [0.5, 0, -0.5], [0, 0, 0], [1, 1, 1], [nan, nan, 0.1], [0, inf, -inf], [-inf, nan, 0],
                    [0, 0, 0.9], [0, 0.7, 0.6]], F32)
    return ("nonfinite_scores", centre_rows(_grid(10, pitch=20, side=10), obj, cls), 0.5, 0.4, "centre")
