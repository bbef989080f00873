"""Stand-alone association kernels (through the C ABI) against float64 numpy at the shapes and values where they can go wrong
without a trace noticing: gallery lengths around the 16-row chunk, detection counts around the 16-column slab, zero-padded feature
dimensions, row norms over six decades; Kalman states of boxes 4..4000 px tall over 300 predict / update cycles and after 70
frames of coasting; gating distances on the chi-square thresholds; IOU and tracker-side NMS on their geometric edges.

Tolerances.  Appearance cost and IOU: the project's own for these kernels (rtol 1e-4 / atol 2e-6 and rtol 1e-5 / atol 1e-6).  Kalman
and gating are not fixed in advance: each run measures, against ONE float64 step from the kernel's own fp32 inputs, the error of
the kernel and the error of the oracle's fp32 restatement (oracle.tracker, pinned to the reference) and allows the kernel 4x the
oracle's worst value per quantity - both are fp32 LU solves that differ in operation order only, while a dropped or transposed term
is O(1e-2) on the same scale.  Mean errors are scaled by sqrt(P_ii), covariance errors by sqrt(P_ii P_jj) of the predicted
covariance; gating errors are relative, with d^2 < 1 taken as 1.

Measured on an MI355X (worst one-step error over the sweep, oracle / kernel):
    predict mean 8.58e-3 / 8.58e-3    predict cov 1.54e-7 / 1.54e-7    (bit-identical outputs)
    update mean  6.58e-3 / 6.58e-3    update cov  1.44e-7 / 1.44e-7
    gating, 2 dof 2.22e-7 / 2.82e-7   gating, 4 dof 2.78e-7 / 2.78e-7
The mean figures are the rounding of the mean itself: half an ulp of an aspect ratio of 2 is 1.2e-7, against a posterior deviation
of ~1.4e-5 once the aspect has been measured 300 times.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
HEIGHTS = (4, 8, 16, 64, 256, 1024, 4000)
ASPECTS = (0.1, 0.5, 2.0)
GALLERY_ROWS = (1, 15, 16, 17, 32, 33, 64, 100)
CHI2 = {2: 5.9915, 4: 9.4877}


def _lib():
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    return _lib


def _c(a, dtype=F32):
    return np.ascontiguousarray(a, dtype=dtype)


# ------------------------------------------------------------------------------------------------------- appearance cost
def _min_cost(gal, seg, feats, euclid):
    L = _lib()
    fn = L.load().yds_euclidean_min_cost if euclid else L.load().yds_cosine_min_cost
    gal, feats, seg = _c(gal), _c(feats), _c(seg, np.int32)
    out = np.full((len(seg) - 1, len(feats)), np.nan, F32)
    L.check(fn(L.ptr(gal), L.ptr(seg), len(seg) - 1, L.ptr(feats), len(feats), gal.shape[1], L.ptr(out)))
    return out


def _min_cost_f64(gal, seg, feats, euclid):
    """1 - <g/|g|, f/|f|> or sum((g - f)^2) clamped at 0, minimised per gallery segment; also the row that attains the minimum."""
    g, f = gal.astype(F64), feats.astype(F64)
    if euclid:
        d = np.maximum(((g[:, None, :] - f[None, :, :]) ** 2).sum(-1), 0)
    else:
        d = 1 - (g / np.linalg.norm(g, axis=1, keepdims=True)) @ (f / np.linalg.norm(f, axis=1, keepdims=True)).T
    want = np.stack([d[seg[k]:seg[k + 1]].min(0) for k in range(len(seg) - 1)], 0)
    arg = np.stack([d[seg[k]:seg[k + 1]].argmin(0) for k in range(len(seg) - 1)], 0)
    return want, arg


def _planted(D, dim, last, seed):
    """T = 8 galleries of GALLERY_ROWS rows; row norms 1e-3..1e3; track t's best match for detection t % D sits in the last row of
    its gallery (or in row 0), every other row of that gallery points the opposite way."""
    rng = np.random.RandomState(seed)
    seg = np.concatenate([[0], np.cumsum(GALLERY_ROWS)]).astype(np.int32)
    unit = rng.randn(D, dim)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    feats = unit * 10.0 ** rng.uniform(-3, 3, (D, 1))
    gal = np.zeros((seg[-1], dim))
    for t, rows in enumerate(GALLERY_ROWS):
        d = t % D
        noise = rng.randn(rows, dim) / np.sqrt(dim)
        g = -unit[d] + 0.3 * noise
        hit = rows - 1 if last else 0
        g[hit] = unit[d] + 0.05 * noise[hit]
        gal[seg[t]:seg[t + 1]] = g / np.linalg.norm(g, axis=1, keepdims=True) * 10.0 ** rng.uniform(-3, 3, (rows, 1))
    return gal.astype(F32), seg, feats.astype(F32)


@pytest.mark.parametrize("dim", [512, 128, 7])
@pytest.mark.parametrize("D", [1, 16, 17, 47])
def test_appearance_cost_chunk_edges_padding_and_norms(D, dim):
    for last in (True, False):
        gal, seg, feats = _planted(D, dim, last, seed=100 * D + dim + last)
        for euclid in (0, 1):
            if euclid:                                   # the same directions, every row of the track's gallery near the norm of
                for t in range(len(GALLERY_ROWS)):      # its detection: the planted row is the nearest in squared distance too
                    nf = np.linalg.norm(feats[t % D].astype(F64))
                    g = gal[seg[t]:seg[t + 1]].astype(F64)
                    gal[seg[t]:seg[t + 1]] = (g / np.linalg.norm(g, axis=1, keepdims=True) * nf).astype(F32)
            want, arg = _min_cost_f64(gal, seg, feats, euclid)
            for t, rows in enumerate(GALLERY_ROWS):      # the planting holds in float64: the minimum is where it was put, by O(1)
                assert arg[t, t % D] == (rows - 1 if last else 0)
            got = _min_cost(gal, seg, feats, euclid)
            if euclid:
                g2, f2 = (gal.astype(F64) ** 2).sum(1), (feats.astype(F64) ** 2).sum(1)
                atol = 2e-6 * (np.array([g2[seg[k]:seg[k + 1]].max() for k in range(len(seg) - 1)])[:, None] + f2[None, :])
            else:
                atol = 2e-6
            err = np.abs(got - want)
            assert np.isfinite(got).all()
            assert (err <= atol + 1e-4 * np.abs(want)).all(), (D, dim, last, euclid, float((err - 1e-4 * np.abs(want)).max()))


@pytest.mark.parametrize("dim", [512, 128, 16])
def test_appearance_cost_exact_cases(dim):
    """identical row -> euclidean 0.0 exactly, cosine 0 within the tolerance; antipodal row -> cosine 2; two +-1 rows that agree on
    12 of their 16 entries -> cosine exactly 0.5 (norm 4, products +-1/16: every partial sum is exact in fp32)."""
    rng = np.random.RandomState(dim)
    rows = (17, 16, 33)
    seg = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    feats = rng.randn(3, dim).astype(F32)
    feats[2] = 0
    feats[2, :16] = 1
    gal = np.zeros((seg[-1], dim), F32)
    gal[:17] = 40 * rng.randn(17, dim).astype(F32)                   # far from everything in squared distance
    gal[16] = feats[0]
    gal[seg[1]:seg[2]] = -feats[1][None, :] * (F32(10) ** np.linspace(-3, 3, 16, dtype=F32))[:, None]    # all antipodal: the min is 2
    for r in range(32):                                              # +-1 rows orthogonal to feats[2] (cosine cost exactly 1)
        gal[seg[2] + r, :16] = [1 if bin(k & (r % 15 + 1)).count("1") % 2 == 0 else -1 for k in range(16)]
    gal[seg[3] - 1, :16] = [1] * 12 + [-1] * 4
    cos, euc = _min_cost(gal, seg, feats, 0), _min_cost(gal, seg, feats, 1)
    assert euc[0, 0] == 0.0 and abs(cos[0, 0]) <= 2e-6
    assert abs(cos[1, 1] - 2) <= 2e-6 + 2e-4
    assert cos[2, 2].tobytes() == F32(0.5).tobytes()
    np.testing.assert_allclose(cos, _min_cost_f64(gal, seg, feats, 0)[0], rtol=1e-4, atol=2e-6)


# ---------------------------------------------------------------------------------------------------------------- Kalman
_STD_POS, _STD_VEL = F64(F32(1. / 20)), F64(F32(1. / 160))
_F = np.eye(8)
_F[:4, 4:] = np.eye(4)


def _predict64(mean, cov):
    """kalman_filter.py:89-123 in float64 from fp32 inputs (the fp32 constants are inputs too)."""
    m, P = mean.astype(F64), cov.astype(F64)
    h = m[:, 3]
    sp, sv = h * _STD_POS, h * _STD_VEL
    q = np.stack([sp, sp, 0 * h + F64(F32(1e-2)), sp, sv, sv, 0 * h + F64(F32(1e-5)), sv], 1) ** 2
    P = _F @ P @ _F.T
    P[:, np.arange(8), np.arange(8)] += q
    return m @ _F.T, P


def _project64(mean, cov):
    m, P = mean.astype(F64), cov.astype(F64)
    sp = m[:, 3] * _STD_POS
    S = P[:, :4, :4].copy()
    S[:, np.arange(4), np.arange(4)] += np.stack([sp, sp, 0 * sp + F64(F32(1e-1)), sp], 1) ** 2
    return m[:, :4], S


def _update64(mean, cov, z):
    m, P = mean.astype(F64), cov.astype(F64)
    pm, S = _project64(mean, cov)
    K = np.linalg.solve(S, P.transpose(0, 2, 1)[:, :4, :]).transpose(0, 2, 1)      # S K^T = (P H^T)^T
    new_m = m + np.einsum("tij,tj->ti", K, z.astype(F64) - pm)
    return new_m, P - K @ S @ K.transpose(0, 2, 1)


def _k_initiate(xyah):
    L = _lib()
    xyah = _c(xyah)
    m, c = np.zeros((len(xyah), 8), F32), np.zeros((len(xyah), 8, 8), F32)
    L.check(L.load().yds_kalman_initiate(L.ptr(xyah), len(xyah), L.ptr(m), L.ptr(c)))
    return m, c


def _k_predict(mean, cov):
    L = _lib()
    m, c = mean.copy(), cov.copy()
    L.check(L.load().yds_kalman_predict(L.ptr(m), L.ptr(c), len(m)))
    return m, c


def _k_update(mean, cov, z):
    L = _lib()
    m, c, z = mean.copy(), cov.copy(), _c(z)
    L.check(L.load().yds_kalman_update(L.ptr(m), L.ptr(c), L.ptr(z), len(m)))
    return m, c


def _k_project(mean, cov):
    L = _lib()
    m4, c16 = np.zeros((len(mean), 4), F32), np.zeros((len(mean), 4, 4), F32)
    L.check(L.load().yds_kalman_project(L.ptr(_c(mean)), L.ptr(_c(cov)), len(mean), L.ptr(m4), L.ptr(c16)))
    return m4, c16


def _scaled(mean, cov, mean64, cov64, pred_cov):
    """worst one-step error of (mean, cov) against the float64 step, on the scale of the predicted covariance"""
    sd = np.sqrt(np.diagonal(pred_cov.astype(F64), axis1=1, axis2=2))
    return (float((np.abs(mean - mean64) / sd).max()), float((np.abs(cov - cov64) / (sd[:, :, None] * sd[:, None, :])).max()))


class _Sweep:
    """worst scaled one-step errors, oracle and kernel side by side, per quantity"""

    def __init__(self):
        self.worst = {}

    def add(self, name, oracle, kernel):
        o, k = self.worst.get(name, (0.0, 0.0))
        self.worst[name] = (max(o, oracle), max(k, kernel))


def _states(heights, aspects, rng):
    h = np.array([hh for hh in heights for _ in aspects], F64)
    a = np.array([aa for _ in heights for aa in aspects], F64)
    return np.stack([rng.uniform(0, 1900, len(h)), rng.uniform(0, 1000, len(h)), a, h], 1).astype(F32)


def _chain(sw, xyah, cycles, skip, rng, snap_at=()):
    """initiate -> skip x predict -> cycles x (predict, update); every kernel output is checked against the float64 step and the
    oracle's step from the kernel's own previous output.  Returns {cycle: posterior (mean, cov)} for snap_at and, with skip > 0,
    {"coasted": the predicted state in front of the first update}."""
    from oracle import tracker as otrk
    m, P = _k_initiate(xyah)
    om, oP = zip(*[otrk.kf_initiate(x) for x in xyah])
    assert np.array_equal(m, np.concatenate(om)) and np.array_equal(P, np.concatenate(oP))         # single fp32 products
    snaps = {}
    for step in range(skip + cycles):
        pm, pP = _k_predict(m, P)
        om, oP = otrk.kf_predict(m, P)
        assert np.array_equal(pm, om) and np.array_equal(pP, oP), step                              # predict: two-term sums, bit exact
        m64, P64 = _predict64(m, P)
        e = _scaled(pm, pP, m64, P64, pP)
        sw.add("predict mean", e[0], e[0])
        sw.add("predict cov", e[1], e[1])
        assert (np.diagonal(pP, axis1=1, axis2=2) > 0).all(), step
        m, P = pm, pP
        if step < skip:
            continue
        if skip and step == skip:
            snaps["coasted"] = (pm.copy(), pP.copy())
        h = pm[:, 3:4]
        z = (pm[:, :4] + rng.randn(len(pm), 4) * np.concatenate([h / 20, h / 20, 0 * h + 0.01, h / 20], 1)).astype(F32)
        um, uP = _k_update(pm, pP, z)
        om, oP = otrk.kf_update(pm, pP, z)
        m64, P64 = _update64(pm, pP, z)
        eo, ek = _scaled(om, oP, m64, P64, pP), _scaled(um, uP, m64, P64, pP)
        sw.add("update mean", eo[0], ek[0])
        sw.add("update cov", eo[1], ek[1])
        assert (np.diagonal(uP, axis1=1, axis2=2) > 0).all(), step
        s4m, s4P = _k_project(um, uP)
        o4m, o4P = otrk.kf_project(um, uP)
        assert np.array_equal(s4m, o4m) and np.array_equal(s4P, o4P), step                          # project: one fp32 add
        m, P = um, uP
        if step - skip + 1 in snap_at:
            snaps[step - skip + 1] = (m.copy(), P.copy())
    return snaps


@functools.lru_cache(maxsize=None)
def _kalman_sweep():
    rng = np.random.RandomState(7)
    sw = _Sweep()
    xyah = _states(HEIGHTS, ASPECTS, rng)                                          # T = 21: every height x aspect in one call
    snaps = _chain(sw, xyah, 300, 0, rng, snap_at=(1, 30, 300))
    snaps.update(_chain(sw, xyah, 1, 69, rng))                                     # 70 predicts (the largest max_age in use), one update
    for T in (1, 63, 64, 65, 200):                                                 # the launchers use 64-thread blocks
        _chain(sw, _states(HEIGHTS, ASPECTS, rng)[np.arange(T) % 21], 2, 0, rng)
    return sw, snaps


def test_kalman_steps_4_to_4000_px_vs_float64():
    sw, _ = _kalman_sweep()
    for name, (o, k) in sw.worst.items():
        print("kalman one-step error, %-12s: oracle %.3g  kernel %.3g" % (name, o, k))
    for name, (o, k) in sw.worst.items():
        assert k <= 4 * o, (name, o, k)
        # the yardstick itself is sane.  Covariances: orders of magnitude under a wrong term.  Means: the rounding of the mean itself
        # (half an ulp of an aspect ratio of 2 is 1.2e-7, against a posterior deviation of ~1.4e-5 after 300 updates) bounds it.
        assert o < (2e-2 if name.endswith("mean") else 1e-5), (name, o)


# ---------------------------------------------------------------------------------------------------------------- gating
def _gate64(mean, cov, z, n):
    pm, S = _project64(mean, cov)
    d = z.astype(F64)[None, :, :n] - pm[:, None, :n]
    return np.einsum("tdi,tij,tdj->td", d, np.linalg.inv(S[:, :n, :n]), d)


def _k_gate(mean, cov, z, n):
    L = _lib()
    z = _c(z)
    out = np.full((len(mean), len(z)), np.nan, F32)
    L.check(L.load().yds_kalman_gating_ex(L.ptr(_c(mean)), L.ptr(_c(cov)), len(mean), L.ptr(z), len(z), 1 if n == 2 else 0, L.ptr(out)))
    return out


def _measurements(mean, cov, D, n, rng):
    """[D, 4] xyah for 3 tracks: per track its own mean, then points at d^2 = chi2inv95[2], chi2inv95[4] and 1e6 (float64
    construction through the Cholesky factor of the projected covariance), the rest between 0 and 20."""
    pm, S = _project64(mean, cov)
    z = np.zeros((D, 4))
    kinds = []
    for d in range(D):
        t, k = d % 3, d // 3
        target = 0.0 if k == 0 else (5.9915, 9.4877, 1e6)[k % 3] if k < 19 else rng.uniform(0, 20)
        u = rng.randn(n)
        step = np.linalg.cholesky(S[t, :n, :n]) @ (u / np.linalg.norm(u)) * np.sqrt(target)
        z[d] = pm[t]
        z[d, :n] += step
        kinds.append((t, target))
    return z.astype(F32), kinds


def test_gating_on_the_thresholds_small_and_coasted_states():
    from oracle import tracker as otrk
    _, snaps = _kalman_sweep()
    rng = np.random.RandomState(11)
    worst = {2: [0.0, 0.0], 4: [0.0, 0.0]}
    for name, (mean, cov) in snaps.items():
        for g in range(7):                                                         # 3 tracks of one height per call
            m, P = mean[3 * g:3 * g + 3], cov[3 * g:3 * g + 3]
            if name != "coasted":                                                  # the gate sees predicted states (tracker.py:95-113)
                m, P = _k_predict(m, P)
            for n in (2, 4):
                D = 85 + (g + n // 2) % 2                                         # T * D = 255 / 258: around the 256-thread block
                z, kinds = _measurements(m, P, D, n, rng)
                want = _gate64(m, P, z, n)
                got, ora = _k_gate(m, P, z, n), otrk.kf_gating_distance(m, P, z, n == 2)
                for d, (t, target) in enumerate(kinds):
                    if target == 0.0:
                        assert got[t, d] == 0.0, (name, g, n)                      # exactly the mean
                    elif target < 10:                                              # really on the threshold (fp32 rounding of z aside)
                        assert abs(want[t, d] / target - 1) < 2e-2, (name, g, n, want[t, d], target)
                scale = np.maximum(want, 1)
                worst[n][0] = max(worst[n][0], float((np.abs(ora - want) / scale).max()))
                worst[n][1] = max(worst[n][1], float((np.abs(got - want) / scale).max()))
    for n, (o, k) in worst.items():
        print("gating error, %d dof: oracle %.3g  kernel %.3g" % (n, o, k))
    for n, (o, k) in worst.items():
        assert k <= 4 * o, (n, o, k)
        assert 100 * o < 1e-3, (n, o)                 # the gate scenes of assoc_thresholds.npz keep a 1e-3 margin: > 100x this


# ------------------------------------------------------------------------------------------------------------- IOU cost
def _iou_cost64(tb, db):
    """1 - IOU with the +1 in the intersection only (iou_matching.py:5-41), in float64 from what the kernel is given: the fp32
    (x, y, a, h) rows the C entry makes of the track boxes, and the fp32 detections."""
    mean = np.stack([tb[:, 0] + tb[:, 2] / F32(2), tb[:, 1] + tb[:, 3] / F32(2), tb[:, 2] / tb[:, 3], tb[:, 3]], 1).astype(F64)
    bw, bh = mean[:, 2] * mean[:, 3], mean[:, 3]
    bx, by = mean[:, 0] - bw / 2, mean[:, 1] - bh / 2
    d = db.astype(F64)
    iw = np.maximum(np.minimum((bx + bw)[:, None], (d[:, 0] + d[:, 2])[None]) - np.maximum(bx[:, None], d[None, :, 0]) + 1, 0)
    ih = np.maximum(np.minimum((by + bh)[:, None], (d[:, 1] + d[:, 3])[None]) - np.maximum(by[:, None], d[None, :, 1]) + 1, 0)
    inter = iw * ih
    a_t, a_d = (bw * bh)[:, None], (d[:, 2] * d[:, 3])[None]
    union = a_t + a_d - inter
    return 1 - inter / union, np.maximum(a_t, a_d) / np.abs(union)


def _k_iou(tb, db):
    L = _lib()
    tb, db = _c(tb), _c(db)
    out = np.full((len(tb), len(db)), np.nan, F32)
    L.check(L.load().yds_iou_cost(L.ptr(tb), len(tb), L.ptr(db), len(db), L.ptr(out)))
    return out


_IOU_PAIRS = [   # (track tlwh, detection tlwh, expected cost or None): track w / h is a power of two, so a * h is exact in fp32
    ((100, 100, 32, 64), (100, 100, 32, 64), 1 - 33 * 65 / (4096 - 33 * 65)),              # identical: IOU > 1, cost negative
    ((100, 100, 32, 64), (132, 100, 32, 64), 1 - 65 / (4096 - 65)),                        # edges touch: the +1 makes a 1 px overlap
    ((100, 100, 32, 64), (133, 100, 32, 64), 1.0),                                         # 1 px gap
    ((100, 100, 32, 64), (100, 165, 32, 64), 1.0),                                         # 1 px gap, vertical
    ((100, 100, 32, 64), (108, 116, 8, 16), 1 - 9 * 17 / (2048 + 128 - 9 * 17)),           # nested
    ((3.25, 5.5, 0.25, 0.5), (3.25, 5.5, 0.25, 0.5), 1 - 1.25 * 1.5 / (0.25 - 1.25 * 1.5)),  # sub-pixel, identical: union < 0
    ((3.25, 5.5, 0.25, 0.5), (3.375, 5.625, 0.125, 0.25), None),                           # sub-pixel, nested
    ((3.25, 5.5, 0.25, 0.5), (4.5, 5.5, 0.5, 0.5), 1.0),                                   # sub-pixel, exactly 1 px apart
    ((10000, 9984, 64, 128), (10016, 10000, 64, 128), None),                               # coordinates around 1e4
    ((10000, 9984, 64, 128), (10065, 9984, 64, 128), 1.0),
    ((-200, -300, 32, 64), (-190, -280, 32, 64), None),                                    # negative coordinates
    ((-16, -32, 32, 64), (-8, -8, 16, 16), None),                                          # straddles the origin
    ((0, 0, 2000, 4000), (1000, 1000, 500, 700), None),                                    # the tallest tested box
    ((50, 50, 1, 4), (50, 50, 1, 4), None),                                                # the smallest
]


@pytest.mark.parametrize("T,D", [(15, 17), (16, 16), (257, 1)])            # T * D = 255, 256, 257: around the 256-thread block
def test_iou_cost_geometric_edges_vs_float64(T, D):
    """Boxes on dyadic coordinates with power-of-two track aspect ratios: the geometry is exact in fp32, so what is compared is
    the kernel's arithmetic (the order of the union, the +1, the clamps), not the conditioning of fp32 boxes."""
    rng = np.random.RandomState(T * 1000 + D)
    tb = np.zeros((T, 4))
    tb[:, 3] = rng.choice(HEIGHTS, T)
    tb[:, 2] = tb[:, 3] * rng.choice([0.125, 0.5, 2.0], T)
    tb[:, :2] = rng.randint(-500, 10000, (T, 2))
    db = np.zeros((D, 4))
    for d in range(D):                                                  # each detection near some track: integer offsets and sizes
        t = d % T
        db[d, 2:] = np.maximum(1, np.round(tb[t, 2:] * rng.uniform(0.5, 1.5, 2)))
        db[d, :2] = tb[t, :2] + np.round(rng.uniform(-1.2, 1.2, 2) * tb[t, 2:])
    pairs = _IOU_PAIRS[:min(T, D)]                                      # the scripted pairs sit on the diagonal, as many as fit
    for k, (a, b, _) in enumerate(pairs):
        tb[k], db[k] = a, b
    tb, db = tb.astype(F32), db.astype(F32)
    got = _k_iou(tb, db)
    want, cancel = _iou_cost64(tb, db)
    for k, (a, b, c) in enumerate(pairs):
        assert c is None or abs(want[k, k] - c) < 1e-12, k
    assert len(pairs) < len(_IOU_PAIRS) or ((want[0, 0] < 0) and (want == 1).any() and ((want > 0) & (want < 1)).any())
    err = np.abs(got - want)
    assert (err <= 1e-6 * np.maximum(1, cancel) + 1e-5 * np.abs(want)).all(), float(err.max())
    assert (got[want == 1] == 1).all()                                  # no overlap: exactly 1


# ------------------------------------------------------------------------------------------------------- tracker-side NMS
def _k_nms(boxes, order, thr):
    L = _lib()
    boxes, order = _c(boxes), _c(order, np.int32)
    pick, n = np.zeros(len(boxes), np.int32), C.c_int(0)
    L.check(L.load().yds_tracker_nms(L.ptr(boxes), L.ptr(order), len(boxes), float(thr), L.ptr(pick), C.byref(n)))
    return pick[:n.value].tolist()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 600])
def test_tracker_nms_block_edges_vs_oracle(n):
    from oracle import tracker as otrk
    rng = np.random.RandomState(n)
    centres = rng.randint(0, 1500, (max(n // 6, 1), 2))
    boxes = np.concatenate([centres[rng.randint(0, len(centres), n)] + rng.randint(-6, 7, (n, 2)), rng.randint(8, 40, (n, 2))], 1).astype(F32)
    for thr in (0.5, 0.3, 0.9):
        order = rng.permutation(n).astype(np.int32)
        want = otrk.tracker_nms(boxes, thr, order)
        assert _k_nms(boxes, order, thr) == want, (n, thr)
        assert n < 255 or 1 < len(want) < n                                            # clusters: some suppressed, some kept


def test_tracker_nms_overlap_exactly_on_the_threshold():
    """inter / area = 5 * 10 / (10 * 10) under the +1 convention: kept by `> 0.5`, suppressed by `> nextafter(0.5, 0)`."""
    from oracle import tracker as otrk
    pair = np.array([[0, 0, 9, 9], [5, 0, 9, 9]], F32)
    order = np.array([0, 1], np.int32)
    below = float(np.nextafter(F32(0.5), F32(0)))
    assert _k_nms(pair, order, 0.5) == otrk.tracker_nms(pair, 0.5, order) == [1, 0]
    assert _k_nms(pair, order, below) == otrk.tracker_nms(pair, below, order) == [1]
    assert _k_nms(pair, order, float(np.nextafter(0.5, 0))) == [1]                      # one float64 ulp: the comparison is in double
