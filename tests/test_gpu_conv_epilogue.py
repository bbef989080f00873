"""The two sweeps of the f16x3 epilogue (csrc/conv_common.h): the full-tile sweep (conv_epilogue_full: no predicates, eight channels
per thread of an H16 output, scaled domain) and the ragged sweep, on the window kernels and the LDS-DMA tiles with the 16x16x32
MFMA body, variant forced per family through yds_conv_run / yds_conv_run_view, against the float64 reference at mut / 16
(conv_ref.mutant_bound).  Shapes are the smallest that hold a full tile AND a ragged one of the tile shape they are meant for; every
activation / residual pair the kernels are instantiated for; every pairing of an H16 or fp32 residual with an H16 or fp32 output; a
merged launch whose boundary falls inside a tile (ragged sweep) and on a tile border (full sweep on both sides); and one case whose
float32 result is known exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

import conv_ref as R
from conv_ref import ACT, F32

pytestmark = pytest.mark.gpu

WIN = ("conv3x3_f16x3_win<256,128,4x2>", "conv3x3_f16x3_win<256,64,8x1>", "conv3x3_f16x3_win<128,64,4x1>")
DMA16 = ("conv_igemm_f16x3_dma<128,128,2x2,2>", "conv_igemm_f16x3_dma<256,128,4x2,3>", "conv_igemm_f16x3_dma<128,256,2x4,3>",
         "conv_igemm_f16x3_dma<128,64,2x2,2>", "conv_igemm_f16x3_dma<64,128,2x2,2>")       # the tiles of dma_body16 (csrc/conv_f16x3.hip)
ACT_RES = (("linear", 0), ("leaky", 0), ("leaky", 1), ("mish", 0), ("mish", 1), ("relu", 0), ("relu", 2))   # dispatch_act_res
SHAPES = [  # n, h, w, cin, cout, k, s
    (1, 16, 17, 32, 160, 3, 1),      # M = 272, Cout = 160: tile 0 full both ways, last pixel tile and second filter tile ragged (256-row tiles)
    (1, 12, 11, 64, 64, 3, 1),       # M = 132: one full and one ragged tile of the 128x64 shape
    (1, 13, 13, 64, 255, 1, 1),      # head: fp32 output, Cout % 4 != 0
    (1, 13, 13, 64, 18, 1, 1),       # fp32 output, Cout < 32
]
SENTINEL = -77.0


class _F16x3:
    def __enter__(self):
        from yolo_deepsort_amd import _lib as L
        L.init(0)
        self.lib = lib = L.load()
        lib.yds_conv_variant_name.restype = C.c_char_p
        self.prev = lib.yds_get_conv_math()
        L.check(lib.yds_set_conv_math(1))
        by = {lib.yds_conv_variant_name(v).decode(): v for v in range(lib.yds_conv_num_variants())}
        assert all(nme in by for nme in WIN + DMA16), sorted(by)
        return L, by

    def __exit__(self, *exc):
        self.lib.yds_set_conv_math(self.prev)


def _run(L, variant, r):
    n, h, wd, cin = r.x.shape
    cout = r.w.shape[0]
    ho, wo = R.out_hw(h, wd, r.k, r.s)
    y = np.empty((n, cout, ho, wo), F32)
    L.check(L.load().yds_conv_run(variant, n, h, wd, cin, cout, r.k, r.s, r.act, r.res_mode, L.ptr(r.x), L.ptr(r.w), L.ptr(r.bias),
                                  L.ptr(r.res) if r.res is not None else None, L.ptr(y)))
    return y


def _hold(name, what, r, got):
    err = r.err(got)
    assert err < 1e-3 * r.scale, (name, what, err / r.scale)
    assert err <= r.mut / 16, (name, what, f"err {err:.3e} = mut / {r.mut / max(err, 1e-30):.1f}: above mut / 16")


def _refused_by_its_limit(name, shape, msg):
    """a variant that does not take a shape says so in the words of its documented limit"""
    k, cout = shape[5], shape[4]
    if "_win<" in name:
        assert "window-resident" in msg, (name, shape, msg)
        assert k != 3 or ("win<128,64" in name and cout > 64), (name, shape, msg)
    else:
        raise AssertionError((name, shape, msg))                   # the LDS-DMA tiles take every shape of this file


def _takes(shape, res_mode):
    """a residual row is 16-byte aligned: the heads with Cout % 4 != 0 (dense rows of Cout floats) run without one"""
    return not res_mode or shape[4] % 4 == 0


@functools.lru_cache(maxsize=None)
def _refs():
    rng = np.random.RandomState(61)
    return tuple(R.Ref(sh + (act, res_mode), *R.make_case(rng, *sh, res_mode)) for sh in SHAPES for act, res_mode in ACT_RES if _takes(sh, res_mode))


def test_both_sweeps_every_activation_and_residual_mode():
    with _F16x3() as (L, by):
        ran = {}
        for r in _refs():
            for name in WIN + DMA16:
                try:
                    got = _run(L, by[name], r)
                except L.YdsError as e:
                    _refused_by_its_limit(name, r.case, str(e))
                    continue
                _hold(name, r.case, r, got)
                ran.setdefault(name, set()).add(r.case)
        for name in WIN + DMA16:
            cases = ran.get(name, set())
            want = [SHAPES[1]] if "win<128,64" in name else SHAPES[:2] if "_win<" in name else SHAPES
            for sh in want:
                for act, res_mode in ACT_RES:
                    if not _takes(sh, res_mode):
                        continue
                    assert sh + (act, res_mode) in cases, (name, sh, act, res_mode, "did not run")


# ---- formats, views, merged launches ---------------------------------------------------------------------------------------------
# 1x1 64 -> 128 on 16 x 16 pixels (M = 256: a full tile of every shape).  A view is pre-split (H16) where its row length and offset
# are multiples of 32 channels, else fp32: ld 132 makes a tensor fp32.  (cout, ld, off) of the output, (res_mode, ld, off) of the
# residual, (n_split, ld, off) of a second output.
VIEW_BASE = (1, 16, 16, (64, 64, 0))
VIEW_CASES = [(out, (res_mode,) + rv, act) for out in ((128, 192, 32), (128, 132, 4)) for rv in ((128, 0), (132, 4))   # H16 / fp32 output (ldy > Cout) x H16 / fp32 residual
              for act, res_mode in (("leaky", 1), ("relu", 2), ("mish", 1))]
MERGED_CASES = [  # cout, (n_split, ...): the boundary inside every tile / on a border of the 64- and 128-filter tiles (inside a 256-filter tile)
    ((128, 128, 0), (32, 96, 0), "leaky"), ((128, 160, 32), (32, 128, 32), "mish"),
    ((256, 128, 0), (128, 128, 0), "leaky"), ((256, 192, 64), (128, 160, 32), "linear"),
]


def _run_view(L, variant, vc, x, w, bias, res):
    n, h, wd, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), (n_split, y2_ld, y2_off) = vc
    view = np.array([x_ld, x_off, y_ld, y_off, r_ld, r_off, n_split, y2_ld, y2_off], np.int32)
    y = np.empty((n, y_ld, h, wd), F32)
    y2 = np.empty((n, y2_ld, h, wd), F32) if n_split else None
    L.check(L.load().yds_conv_run_view(variant, n, h, wd, cin, cout, k, s, ACT[act], res_mode, L.ptr(view), L.ptr(x), L.ptr(w), L.ptr(bias),
                                       L.ptr(res), SENTINEL, L.ptr(y), L.ptr(y2)))
    return y, y2


@functools.lru_cache(maxsize=None)
def _view_refs():
    rng = np.random.RandomState(67)
    out = []
    cases = [VIEW_BASE + (o, 1, 1, act, r, (0, 0, 0)) for o, r, act in VIEW_CASES]
    cases += [VIEW_BASE + ((cout, ld, off), 1, 1, act, (0, 0, 0), split) for (cout, ld, off), split, act in MERGED_CASES]
    for vc in cases:
        n, h, wd, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), _ = vc
        x = rng.standard_normal((n, h, wd, x_ld)).astype(F32)
        w = (rng.standard_normal((cout, cin)) / np.sqrt(cin)).astype(F32)
        bias = rng.standard_normal(cout).astype(F32)
        res = rng.standard_normal((n, h, wd, r_ld)).astype(F32) if res_mode else None
        r = R.Ref((n, h, wd, cin, cout, k, s, act, res_mode), x, w, bias, np.ascontiguousarray(res[..., r_off:r_off + cout]) if res_mode else None)
        out.append((vc, x, res, r))
    return tuple(out)


def test_formats_views_and_merged_boundaries():
    """every pairing of an H16 / fp32 residual with an H16 / fp32 output, outputs into slices (ldy > Cout), merged launches split
    inside a tile and on a tile border: the slices meet the bound, every channel outside them keeps the sentinel bit for bit"""
    with _F16x3() as (L, by):
        sent = np.float32(SENTINEL).view(np.uint32)
        ran = {}
        for vc, x, res, r in _view_refs():
            (cout, y_ld, y_off), (n_split, y2_ld, y2_off) = vc[4], vc[9]
            c1 = n_split if n_split else cout
            for name in DMA16:
                y, y2 = _run_view(L, by[name], vc, x, r.w, r.bias, res)      # every LDS-DMA tile is a candidate of these layers
                got = np.concatenate([y[:, y_off:y_off + c1], y2[:, y2_off:y2_off + cout - c1]], 1) if n_split else y[:, y_off:y_off + c1]
                _hold(name, vc, r, got)
                outside = np.ones(y_ld, bool)
                outside[y_off:y_off + c1] = False
                assert (y[:, outside].view(np.uint32) == sent).all(), (name, vc, "wrote outside its output slice")
                if n_split:
                    outside = np.ones(y2_ld, bool)
                    outside[y2_off:y2_off + cout - c1] = False
                    assert (y2[:, outside].view(np.uint32) == sent).all(), (name, vc, "wrote outside its second output slice")
                ran.setdefault(name, 0)
                ran[name] += 1
        assert set(ran) == set(DMA16) and all(v == len(VIEW_CASES) + len(MERGED_CASES) for v in ran.values()), ran


# ---- one exact case ----------------------------------------------------------------------------------------------------------------
def _h16_roundtrip(o):
    """an fp32 value stored as an H16 record (round to nearest even twice) and decoded again, all in float32"""
    xs = (o * F32(1 / 256)).astype(F32)
    hi = xs.astype(np.float16)
    lo = ((xs - hi.astype(F32)) * F32(2048)).astype(np.float16)
    return ((hi.astype(F32) + lo.astype(F32) * F32(1 / 2048)) * F32(256)).astype(F32)


def test_unit_weights_give_exact_bits():
    """3x3 conv whose only nonzero weights are a 1 at the centre tap of one input channel per filter, zero bias, LeakyReLU: filter o
    returns leaky(x[.., c(o)]).  The inputs are multiples of 1/8 up to 8 in both signs (exact hi halves, zero lo halves), zeros of
    both signs among them, so every product and sum of the K loop is exact and the result is float32(x) for x > 0, +0 for +-0 (the
    accumulator starts at +0) and the float32 product x * 0.1f below - bit for bit in an fp32 output, and after the H16 round trip
    of that very value in a pre-split output.  272 pixels: a full tile and a ragged one of every shape."""
    n, h, wd, cin = 1, 16, 17, 64
    rng = np.random.RandomState(71)
    x = (rng.randint(-64, 65, (n, h, wd, cin)) / 8).astype(F32)
    x[rng.random_sample(x.shape) < 0.05] = -0.0
    x[rng.random_sample(x.shape) < 0.05] = 0.0
    with _F16x3() as (L, by):
        ran = set()
        for cout in (128, 64, 72):                                  # H16 output (128, 64 filters), fp32 output (72 % 32 != 0)
            src = rng.randint(0, cin, cout)
            w = np.zeros((cout, 9 * cin), F32)
            w[np.arange(cout), 4 * cin + src] = 1
            picked = x[..., src]                                    # NHWC
            want = np.where(picked > 0, picked, picked * F32(0.1)).astype(F32)
            want[picked == 0] = 0.0                                 # -0 * 1 + (+0) = +0
            if cout % 32 == 0:
                want = _h16_roundtrip(want)
            want = np.ascontiguousarray(want.transpose(0, 3, 1, 2))
            for name in WIN + DMA16:
                y = np.empty((n, cout, h, wd), F32)
                try:
                    L.check(L.load().yds_conv_run(by[name], n, h, wd, cin, cout, 3, 1, ACT["leaky"], 0, L.ptr(x), L.ptr(w), L.ptr(np.zeros(cout, F32)),
                                                  None, L.ptr(y)))
                except L.YdsError as e:
                    _refused_by_its_limit(name, (n, h, wd, cin, cout, 3, 1), str(e))
                    continue
                assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (name, cout, float(np.abs(y - want).max()))
                ran.add(name)
        assert ran == set(WIN + DMA16), ran
