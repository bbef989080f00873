"""Every implicit-GEMM conv kernel variant (through the C ABI entries yds_conv_run / yds_conv_run_view) vs a float64 numpy convolution.

The detector tests only exercise the variant the autotuner picks per layer; this file pins each tile shape / staging
scheme on its own: 3x3 s1, 3x3 s2, 1x1 (s1 and s2), ragged M and Cout edges, images of one or two pixels, every activation, both
residual modes; every tile order; channel-slice views and the merged launch of two convolutions.
Two bounds: 1e-3 of the output scale (north_star), and mut / 16, where mut is the error of a kernel that drops one cross term of the
split-fp16 product, evaluated in float64 by the reference (conv_ref.py; test_conv_ref.py shows on the CPU that the reference
arithmetic itself sits below mut / 64 on every case)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import conv_ref as R
from conv_ref import ACT, CASES, F32
from conv_ref import conv_ref as _conv_ref

pytestmark = pytest.mark.gpu

FAMILIES = (("fp32 MFMA", "conv_igemm_f32<"), ("split-K", "+splitK"), ("LDS-DMA", "_dma<"), ("staged", "conv_igemm_f16x3<"),
            ("win2", "_win2<"), ("win", "_win<"))


def _family(name):
    return next(f for f, key in FAMILIES if key in name)


def _run(L, variant, x, w, bias, k, s, act, res, res_mode):
    n, h, wd, cin = x.shape
    cout = w.shape[0]
    ho, wo = R.out_hw(h, wd, k, s)
    y = np.empty((n, cout, ho, wo), F32)
    L.check(L.load().yds_conv_run(variant, n, h, wd, cin, cout, k, s, act, res_mode, L.ptr(x), L.ptr(w), L.ptr(bias),
                                  L.ptr(res) if res is not None else None, L.ptr(y)))
    return y


class _Math:
    """the library in conv math `math`: (lib, variant names, ids of that math's implicit-GEMM variants); restores the mode on exit"""

    def __init__(self, math):
        self.math = math

    def __enter__(self):
        from yolo_deepsort_amd import _lib as L
        L.init(0)
        self.lib = lib = L.load()
        lib.yds_conv_variant_name.restype = C.c_char_p
        self.prev = lib.yds_get_conv_math()
        L.check(lib.yds_set_conv_math(self.math))
        names = [lib.yds_conv_variant_name(v).decode() for v in range(lib.yds_conv_num_variants())]
        mine = [v for v, nme in enumerate(names) if ("f16x3" in nme) == bool(self.math) and "direct" not in nme]
        assert len(mine) >= 4
        return L, names, mine

    def __exit__(self, *exc):
        self.lib.yds_set_conv_math(self.prev)


class _Worst:
    """worst err / scale, err / mut and err / err_fp32 per variant; checks both bounds as it records"""

    def __init__(self):
        self.rows = {}

    def hold(self, name, what, err, r):
        row = self.rows.setdefault(name, [0.0, 0.0, 0.0])
        for i, v in enumerate((err / r.scale, err / r.mut, err / r.err_fp32)):
            row[i] = max(row[i], v)
        assert err < 1e-3 * r.scale, (name, what, err / r.scale)
        # a kernel that drops a cross term of the split product is at mut or above (conv_ref.mutant_bound)
        assert err <= r.mut / 16, (name, what, f"err {err:.3e} = mut / {r.mut / max(err, 1e-30):.1f}: above mut / 16")

    def report(self, title):
        print(f"\n{title}: worst err/scale, err/mut, err/err_fp32 per variant")
        for name, (a, b, c) in self.rows.items():
            print(f"  {name:46s} {a:.1e}  mut/{1 / max(b, 1e-30):7.0f}  {c:6.2f} x fp32" + ("   <-- between mut/64 and mut/16" if b > 1 / 64 else ""))
        fam = {}
        for name, (a, b, c) in self.rows.items():
            fam[_family(name)] = max(fam.get(_family(name), 0.0), b)
        print("  per family, worst err/mut: " + ", ".join(f"{f} mut/{1 / max(b, 1e-30):.0f}" for f, b in fam.items()))


def _check_refusal(names, v, case, e):
    """A variant that does not take a layer says why, in the words of its documented limit, instead of computing garbage."""
    n, h, wd, cin, cout, k, s = case[:7]
    name, msg = names[v], str(e)
    if cin % 32 and "_dma<" in name:                 # the LDS-DMA kernels (split-K is one) fetch pre-split tensors: Cin % 32 == 0
        assert "needs a pre-split" in msg, (name, msg)
        return
    if "splitK" in name:                             # split-K refuses layers that already have enough tiles / too few K steps
        assert "split-K does not apply" in msg, (name, msg)
        return
    # the window-resident kernels only take 3x3 stride-1 layers with a pre-split input (the two-workgroup form: W <= 127 as well)
    assert "window-resident" in msg, (name, msg)
    small = "win<128,64" in name and (cout > 64 or wd > 43)      # the 128x64 tile: 64-filter layers, W <= 43
    assert not (k == 3 and s == 1) or ("win2" in name and wd > 127) or small, (name, msg)


@pytest.mark.parametrize("math", [1, 0])
def test_every_conv_variant_vs_float64(math):
    with _Math(math) as (L, names, mine):
        worst = _Worst()
        for r in R.case_refs():
            for v in mine:
                try:
                    got = _run(L, v, r.x, r.w, r.bias, r.k, r.s, r.act, r.res, r.res_mode)
                except L.YdsError as e:
                    _check_refusal(names, v, r.case, e)
                    continue
                worst.hold(names[v], r.case, r.err(got), r)
        worst.report(f"conv math {math}")
        ran = worst.rows.keys()
        assert len(ran) == len(mine), set(names[v] for v in mine) - set(ran)        # every variant took some case
        if math:
            assert any("splitK" in k for k in ran) and any("win2" in k for k in ran) and any("win<128,64" in k for k in ran), ran   # these kernels really ran


# ---- tile order ------------------------------------------------------------------------------------------------------------------
TILE_ORDER_CASES = [  # n, h, w, cin, cout, k, s, act, res_mode: 608 / 1248 filters = rectangles of 5 (3, 10) filter tiles per XCD
    (2, 40, 40, 32, 608, 3, 1, "leaky", 0),
    (2, 40, 40, 64, 608, 1, 1, "leaky", 0),
    (2, 28, 28, 32, 1248, 1, 1, "leaky", 0),
]


def _tile_of(name):
    bm, bn = re.search(r"<(\d+),(\d+)", name).groups()
    return int(bm), int(bn)


@functools.lru_cache(maxsize=None)
def _tile_order_refs():
    rng = np.random.RandomState(29)
    return tuple(R.Ref(c, *R.make_case(rng, *c[:7], c[8])) for c in TILE_ORDER_CASES)


@pytest.mark.parametrize("math", [1, 0])
def test_tile_order_is_a_placement_never_a_different_sum(math):
    """The order in which an XCD walks its rectangle of tiles (tile_of_block, gn = 2 or 4 filter tiles together; bits 8.. of the
    variant argument) is picked by a stopwatch, so no network test runs it deterministically.  Every variant that takes a case
    returns THE SAME BITS column by column, in groups of 2 and in groups of 4.  The host restatement of plan_tile_map keeps the
    shapes honest: every rectangle is rn >= 3 filter tiles wide (both orders are real groupings, gn = 4 is clipped to rn = 3 on the
    128x256 tile) and at least one of the two orders ends in a narrower last group (rn = 5 and 3: both; the 128x32 and 256x64 tiles
    have rn = 10, where only gn = 4 does)."""
    with _Math(math) as (L, names, mine):
        grouped = set()
        for r in _tile_order_refs():
            case = r.case
            n, h, wd, cin, cout, k, s, act, res_mode = case
            for v in mine:
                try:
                    base = _run(L, v, r.x, r.w, r.bias, k, s, r.act, None, 0)
                except L.YdsError as e:
                    _check_refusal(names, v, case, e)
                    continue
                tiles_m, tiles_n, xm, rm, rn = R.plan_tile_map(n * h * wd, cout, *_tile_of(names[v]))
                assert rn >= 3 and rm >= 2, (names[v], case, rm, rn)               # min(gn, rn) > 1: never the column-by-column walk
                assert any(rn % gn != 0 or gn > rn for gn in (2, 4)), (names[v], case, rn)
                err = r.err(base)
                assert err < 1e-3 * r.scale and err <= r.mut / 16, (names[v], case, err, r.mut)
                for gn in (2, 4):
                    got = _run(L, v | gn << 8, r.x, r.w, r.bias, k, s, r.act, None, 0)
                    assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (names[v], case, gn, float(np.abs(got - base).max()))
                grouped.add(names[v])
        print("ran with gn = 2 and 4:", sorted(grouped))
        fams = {_family(nme) for nme in grouped}
        assert fams >= ({"staged", "LDS-DMA", "win", "win2"} if math else {"fp32 MFMA"}), fams      # these kernels really ran with gn > 1
        assert len(grouped) >= (14 if math else 7), grouped


# ---- strided views and the merged launch -----------------------------------------------------------------------------------------
SENTINEL = -77.0              # exact in fp32 and in the H16 split: an untouched channel decodes to these very bits
VIEW_CASES = [  # n, h, w, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), (n_split, y2_ld, y2_off)
    (2, 19, 19, (64, 192, 64), (128, 384, 128), 3, 1, "leaky", (1, 256, 64), (0, 0, 0)),
    (3, 13, 13, (128, 128, 0), (255, 256, 0), 1, 1, "linear", (0, 0, 0), (0, 0, 0)),           # head: fp32 output, one spare channel
    (2, 16, 16, (64, 64, 0), (128, 128, 64), 1, 1, "mish", (0, 0, 0), (64, 64, 0)),            # merged: 64 -> slice, 64 -> own tensor
    (2, 16, 16, (64, 64, 0), (64, 64, 32), 1, 1, "leaky", (0, 0, 0), (32, 32, 0)),             # merged 32 + 32: the yolov4 CSP pattern
    (1, 10, 10, (128, 256, 128), (64, 128, 32), 3, 1, "leaky", (1, 96, 32), (0, 0, 0)),        # few tiles, 36 K steps: split-K by rule
]


def _run_view(L, variant, vc, x, w, bias, res):
    n, h, wd, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), (n_split, y2_ld, y2_off) = vc
    ho, wo = R.out_hw(h, wd, k, s)
    view = np.array([x_ld, x_off, y_ld, y_off, r_ld, r_off, n_split, y2_ld, y2_off], np.int32)
    y = np.empty((n, y_ld, ho, wo), F32)
    y2 = np.empty((n, y2_ld, ho, wo), F32) if n_split else None
    L.check(L.load().yds_conv_run_view(variant, n, h, wd, cin, cout, k, s, ACT[act], res_mode, L.ptr(view), L.ptr(x), L.ptr(w), L.ptr(bias),
                                       L.ptr(res), SENTINEL, L.ptr(y), L.ptr(y2)))
    return y, y2


@functools.lru_cache(maxsize=None)
def _view_refs():
    """(view case, whole input, whole residual, Ref on the sliced operands) of every entry of VIEW_CASES"""
    rng = np.random.RandomState(41)
    out = []
    for vc in VIEW_CASES:
        n, h, wd, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), _ = vc
        ho, wo = R.out_hw(h, wd, k, s)
        x = rng.standard_normal((n, h, wd, x_ld)).astype(F32)
        w = (rng.standard_normal((cout, k * k * cin)) / np.sqrt(k * k * cin)).astype(F32)
        bias = rng.standard_normal(cout).astype(F32)
        res = rng.standard_normal((n, ho, wo, r_ld)).astype(F32) if res_mode else None
        r = R.Ref((n, h, wd, cin, cout, k, s, act, res_mode), np.ascontiguousarray(x[..., x_off:x_off + cin]), w, bias,
                  np.ascontiguousarray(res[..., r_off:r_off + cout]) if res_mode else None)
        out.append((vc, x, res, r))
    return tuple(out)


@pytest.mark.parametrize("math", [1, 0])
def test_strided_views_and_merged_launch(math):
    """Input as a channel slice (ldx > Cin), output into a slice of a concatenation buffer (ldy > Cout), a residual with its own
    ldr, and the merged launch (filters [n_split, Cout) to a second view): the slice meets both bounds against the float64
    reference on the sliced operands, every channel outside it keeps the sentinel bit for bit.  yds_conv_run_view refuses a variant
    the planner would never launch on the case, so the variants that run are those a network can meet in that layout."""
    with _Math(math) as (L, names, mine):
        worst = _Worst()
        sent = np.float32(SENTINEL).view(np.uint32)
        ran = {"slice": set(), "merged": set()}
        for vc, x, res, r in _view_refs():
            n, h, wd, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), (n_split, y2_ld, y2_off) = vc
            case, w, bias = r.case, r.w, r.bias
            c1 = n_split if n_split else cout
            for v in mine:
                try:
                    y, y2 = _run_view(L, v, vc, x, w, bias, res)
                except L.YdsError as e:
                    msg = str(e)
                    if "planner never launches" not in msg:
                        _check_refusal(names, v, case, e)
                    else:       # not a candidate: split-K outside its rule, window tiles outside their filter counts, the 128x32 tile
                        assert "splitK" in names[v] or "win" in names[v] or ("f32<128,32" in names[v] and cout > 64), (names[v], vc, msg)
                    continue
                got = np.concatenate([y[:, y_off:y_off + c1], y2[:, y2_off:y2_off + cout - c1]], 1) if n_split else y[:, y_off:y_off + c1]
                worst.hold(names[v], vc, r.err(got), r)
                outside = np.ones(y_ld, bool)
                outside[y_off:y_off + c1] = False
                assert (y[:, outside].view(np.uint32) == sent).all(), (names[v], vc, "wrote outside its output slice")
                if n_split:
                    outside = np.ones(y2_ld, bool)
                    outside[y2_off:y2_off + cout - c1] = False
                    assert (y2[:, outside].view(np.uint32) == sent).all(), (names[v], vc, "wrote outside its second output slice")
                ran["merged" if n_split else "slice"].add(names[v])
        worst.report(f"views, conv math {math}")
        print({k: sorted(v) for k, v in ran.items()})
        sliced, merged = ({_family(nme) for nme in ran[k]} for k in ("slice", "merged"))
        if math:
            assert sliced >= {"staged", "LDS-DMA", "win", "win2", "split-K"}, sliced
            assert merged >= {"staged", "LDS-DMA"} and not merged & {"split-K"}, merged
        else:
            assert sliced == {"fp32 MFMA"} and merged == {"fp32 MFMA"}, (sliced, merged)
            assert len(ran["slice"]) >= 6 and len(ran["merged"]) >= 6, ran


def test_view_entry_refuses_what_the_planner_never_launches():
    """yds_conv_run_view says no, with a message, to a variant outside the layer's candidates, to split-K and the direct kernel on a
    merged launch, and to slices that do not fit their buffers."""
    with _Math(1) as (L, names, mine):
        rng = np.random.RandomState(43)
        x = rng.standard_normal((1, 8, 8, 64)).astype(F32)
        w = (rng.standard_normal((64, 64)) / 8).astype(F32)
        bias = np.zeros(64, F32)
        dense = (1, 8, 8, (64, 64, 0), (64, 64, 0), 1, 1, "leaky", (0, 0, 0), (0, 0, 0))
        merged = (1, 8, 8, (64, 64, 0), (64, 64, 32), 1, 1, "leaky", (0, 0, 0), (32, 32, 0))
        by = {nme: v for v, nme in enumerate(names)}
        for vc, nme in ((dense, "conv_igemm_f32<128,128,2,2,32>"),                   # the other arithmetic
                        (dense, "conv3x3_f16x3_win<256,128,4x2>"),                   # a 1x1 layer
                        (dense, "conv_igemm_f16x3_dma<64,128,2x2,2>+splitK"),        # two K steps: the rule does not pick split-K
                        (merged, "conv_igemm_f16x3_dma<64,128,2x2,2>+splitK"), (merged, "conv_igemm_f16x3_dma<128,128,2x2,2>+splitK"),
                        (merged, "conv3x3_rgb_direct")):
            with pytest.raises(L.YdsError, match="planner never launches"):
                _run_view(L, by[nme], vc, x, w, bias, None)
        staged = by["conv_igemm_f16x3<64,64>"]
        for bad in ((1, 8, 8, (64, 64, 32), (64, 64, 0), 1, 1, "leaky", (0, 0, 0), (0, 0, 0)),      # input slice past its tensor
                    (1, 8, 8, (64, 64, 0), (64, 96, 64), 1, 1, "leaky", (0, 0, 0), (0, 0, 0)),      # output slice past its buffer
                    (1, 8, 8, (64, 64, 0), (64, 66, 0), 1, 1, "leaky", (0, 0, 0), (0, 0, 0)),       # ld no multiple of 4
                    (1, 8, 8, (64, 64, 0), (64, 64, 32), 1, 1, "leaky", (0, 0, 0), (32, 32, 4))):   # second slice past its buffer
            with pytest.raises(L.YdsError, match="does not fit"):
                _run_view(L, staged, bad, x, w, bias, None)
        y, _ = _run_view(L, staged, dense, x, w, bias, None)                         # and takes what the planner does launch
        assert np.abs(y - _conv_ref(x, w, bias, 1, 1, ACT["leaky"], None, 0)).max() < 1e-4


def test_direct_rgb_kernel_vs_float64():
    from yolo_deepsort_amd import _lib as L
    L.init(0)
    lib = L.load()
    lib.yds_conv_variant_name.restype = C.c_char_p
    direct = [v for v in range(lib.yds_conv_num_variants()) if b"direct" in lib.yds_conv_variant_name(v)]
    assert len(direct) == 1
    rng = np.random.RandomState(3)
    for cout, act in ((32, "leaky"), (64, "relu"), (32, "mish")):
        x = np.zeros((2, 33, 47, 4), F32)
        x[..., :3] = rng.uniform(0, 1, (2, 33, 47, 3))
        w = (rng.standard_normal((cout, 9 * 4)) / 5).astype(F32)
        bias = rng.standard_normal(cout).astype(F32)
        want = _conv_ref(x, w, bias, 3, 1, ACT[act], None, 0)
        got = _run(L, direct[0], x, w, bias, 3, 1, ACT[act], None, 0)
        assert float(np.abs(got - want).max()) / float(np.abs(want).max()) < 1e-5


def test_h16_range_saturates():
    """The H16 activation format holds |x| <= 65504 * 256 = 1.677e7 (csrc/h16.h).  Beyond it an encoded value SATURATES (every
    encoding kernel sets MODE.FP16_OVFL) instead of turning into inf / NaN: outputs of a layer whose pre-images exceed the range
    are finite, clamped to +-(65504 .. 65536) * 256 with the right sign, and every in-range output keeps its accuracy - for each
    f16x3 variant that takes the layer, and for an out-of-range INPUT tensor as well (the packing kernel clamps it)."""
    from yolo_deepsort_amd import _lib as L
    L.init(0)
    lib = L.load()
    lib.yds_conv_variant_name.restype = C.c_char_p
    prev = lib.yds_get_conv_math()
    L.check(lib.yds_set_conv_math(1))
    LIM, TOP = 65504.0 * 256, 65536.0 * 256
    try:
        names = [lib.yds_conv_variant_name(v).decode() for v in range(lib.yds_conv_num_variants())]
        mine = [v for v, nme in enumerate(names) if "f16x3" in nme and "direct" not in nme]
        rng = np.random.RandomState(23)
        ran = 0
        for n, h, wd, cin, cout, k in ((2, 19, 19, 64, 128, 3), (1, 26, 26, 128, 64, 1)):
            x = (rng.standard_normal((n, h, wd, cin)) * 1e4).astype(F32)
            w = (rng.standard_normal((cout, k * k * cin)) / np.sqrt(k * k * cin) * 1e3).astype(F32)
            bias = np.zeros(cout, F32)
            want = _conv_ref(x, w, bias, k, 1, 0, None, 0)
            over, inside = np.abs(want) > 1.01 * TOP, np.abs(want) < 0.99 * LIM
            assert over.mean() > 0.02 and inside.mean() > 0.5
            for v in mine:
                try:
                    got = _run(L, v, x, w, bias, k, 1, 0, None, 0)
                except L.YdsError:
                    continue
                ran += 1
                assert np.isfinite(got).all(), names[v]
                assert np.abs(got[inside] - want[inside]).max() < 1e-3 * LIM, names[v]
                assert (np.abs(got[over]) >= LIM).all() and (np.abs(got[over]) <= TOP).all(), names[v]
                assert np.array_equal(np.sign(got[over]), np.sign(want[over])), names[v]
        assert ran >= 6
        # an input beyond the range: clamped by the packing kernel, the layer's result stays finite
        x = np.full((1, 8, 8, 32), 3e7, F32)
        w = np.zeros((32, 32), F32)
        w[np.arange(32), np.arange(32)] = 1
        got = _run(L, mine[0], x, w, np.zeros(32, F32), 1, 1, 0, None, 0)
        assert np.isfinite(got).all() and (got >= LIM).all() and (got <= TOP).all()
    finally:
        lib.yds_set_conv_math(prev)
