"""Half mode (Darknet.half()) kernel by kernel: every conv variant with single-term fp16 operands (ConvArgs::terms == 1) and the 2-byte
F16 activation format, through the C ABI entry yds_conv_run_half, vs the float64 reference of the ROUNDED operands (conv_ref.HalfRef);
and the other layer kernels on F16 tensors, which are exact operations.

Bounds.  fp32 / H16 output: |got - want| <= mut / 16.  F16 output: |got - want| <= ulp16(want) / 2 + mut / 16 element by element, and every
value is representable in the format.  mut is the smaller float64 error of the two kernels that read an operand's lo half as well
(test_conv_ref.py shows on the CPU that fp32 arithmetic sits below mut / 64 and that a truncating store breaks the F16 bound).

Which reference.  The register-staged kernels (family "staged", conv_igemm_f16x3<..>) never look at `terms`: they stage hi AND lo halves
and issue all three MFMAs in half mode too (conv_f16x3.hip), so they are held to the default three-term arithmetic (HalfRef.full: Ref's
want and mut on the same tensors, an F16 residual as stored) with the same F16 output rule.  Every other family - LDS-DMA, win, win2 -
instantiates TERMS = 1 / 4 and is held to the single-term reference (HalfRef.half).  The family NAME decides, never the distance."""
import functools

import numpy as np
import pytest

import conv_ref as R
from conv_ref import ACT, F32, FMT_AUTO, FMT_F16
from test_gpu_conv_variants import SENTINEL, _family, _Math, _tile_of, _Worst

pytestmark = pytest.mark.gpu

FMT_NAME = {FMT_AUTO: "auto", FMT_F16: "F16"}


def _run_half(L, variant, fx, fy, x, w, bias, k, s, act, res, res_mode, view=None):
    """-> (y, y2): dense [n, cout, ho, wo] without a view, else the WHOLE buffers [n, y_ld, ho, wo] (and the second output's)"""
    n, h, wd, x_ld = x.shape
    cout = w.shape[0]
    cin = w.shape[1] // (k * k)
    ho, wo = R.out_hw(h, wd, k, s)
    y2 = None
    if view is None:
        y = np.empty((n, cout, ho, wo), F32)
    else:
        y = np.empty((n, view[2], ho, wo), F32)
        y2 = np.empty((n, view[7], ho, wo), F32) if view[6] else None
        view = np.asarray(view, np.int32)
    L.check(L.load().yds_conv_run_half(variant, n, h, wd, cin, cout, k, s, act, res_mode, L.ptr(view), fx, fy, L.ptr(x), L.ptr(w), L.ptr(bias),
                                       L.ptr(res) if res is not None else None, SENTINEL, L.ptr(y), L.ptr(y2)))
    return y, y2


def _takes(name, case, fx):
    """The documented limits, restated: does the half-mode planner time `name` on this layer?  (conv.hip's variant table)
    staged: every layer whose input is not F16.  LDS-DMA: a pre-split input (H16: Cin % 32 == 0, F16: Cin % 64 == 0).  split-K: never in
    half mode (its rule excludes terms == 1 and it is never timed).  win<128,64>: default arithmetic only.  win<256,..>: 3x3 stride 1,
    pre-split, W <= 95 (W <= 318 when the input is one channel group: 32 channels, or 64 with the 64-channel K steps); the 64-wide tile
    on layers of <= 64 filters.  win2: the same layers with an H16 input (it does not read F16), W <= 127, >= 128 filters."""
    n, h, wd, cin, cout, k, s = case[:7]
    presplit = cin % 64 == 0 if fx == FMT_F16 else cin % 32 == 0
    if "splitK" in name or "win<128,64" in name:
        return False
    if "conv_igemm_f16x3<" in name:
        return fx != FMT_F16
    if "_dma<" in name:
        return presplit
    win = k == 3 and s == 1 and presplit
    if "_win2<" in name:
        return win and fx != FMT_F16 and wd <= 127 and cout >= 128
    one_group = cin == (64 if cin % 64 == 0 else 32)
    fits = wd <= (318 if one_group else 95)
    if "win<256,128" in name:
        return win and fits
    assert "win<256,64" in name, name
    return win and fits and cout <= 64


def _arith(hr, name, fy):
    """the reference a variant is held to: by family name (module docstring)"""
    return hr.full(fy) if _family(name) == "staged" else hr.half(fy)


def _hold(worst, name, what, got, r, fy):
    """records and checks one result; an F16 output is held beyond half a spacing of its format and must be representable"""
    if fy == FMT_F16:
        assert np.array_equal(R.x_hat(got), got), (name, what, "an F16 output holds values outside the format")
        worst.hold(name, what, r.err_f16(got), r)
    else:
        worst.hold(name, what, r.err(got), r)


@pytest.mark.parametrize("fx,fy", [(FMT_AUTO, FMT_AUTO), (FMT_F16, FMT_AUTO), (FMT_AUTO, FMT_F16), (FMT_F16, FMT_F16)], ids=lambda f: FMT_NAME[f])
def test_every_conv_variant_in_half_mode_vs_float64(fx, fy):
    """CASES + HALF_CASES in one format pair ((F16, .) where Cin % 64 == 0, (., F16) where Cout % 64 == 0): every f16x3 variant that the
    half-mode planner times on the layer meets the bound of its reference, every other one refuses ("the planner never launches") - and
    which is which follows from the documented limits (_takes), so a variant cannot dodge a case.  The kernels that only half mode runs
    are asserted to have run: the LDS-DMA kernel with 32-channel K steps (TERMS = 1) and with 64-channel ones (TERMS = 4) on the input
    format of this run, both conv_win.hip tiles, win2 (H16 input), and an F16 output with an F16 residual in each residual mode."""
    with _Math(1) as (L, names, mine):
        worst = _Worst()
        ran = {}                                                   # variant name -> cases it ran
        for hr in R.half_refs():
            if (fx, fy) not in R.half_formats(hr.case):
                continue
            for v in mine:
                try:
                    got, _ = _run_half(L, v, fx, fy, hr.x, hr.w, hr.bias, hr.k, hr.s, hr.act, hr.res, hr.res_mode)
                except L.YdsError as e:
                    assert "planner never launches" in str(e), (names[v], hr.case, str(e))
                    assert not _takes(names[v], hr.case, fx), (names[v], hr.case, "refused a layer inside its documented limits", str(e))
                    continue
                assert _takes(names[v], hr.case, fx), (names[v], hr.case, "ran a layer outside its documented limits")
                _hold(worst, names[v], (hr.case, fx, fy), got, _arith(hr, names[v], fy), fy)
                ran.setdefault(names[v], []).append(hr.case)
        worst.report(f"half mode, input {FMT_NAME[fx]}, output {FMT_NAME[fy]}")
        dma = [c for nme, cs in ran.items() if _family(nme) == "LDS-DMA" for c in cs]
        assert any(c[3] % 64 == 0 for c in dma), "the LDS-DMA kernel with 64-channel K steps did not run"
        assert any(c[5] == 3 for c in dma if c[3] % 64 == 0) and any(c[5] == 1 for c in dma if c[3] % 64 == 0)
        for tile in ("win<256,128", "win<256,64"):
            assert any(tile in nme for nme in ran), (tile, sorted(ran))
        if fx == FMT_AUTO:
            assert any(c[3] in (32, 96) for c in dma), "the LDS-DMA kernel with 32-channel K steps did not run"
            assert any("win2" in nme for nme in ran), sorted(ran)
            assert any(_family(nme) == "staged" for nme in ran), sorted(ran)
        else:
            assert not any("win2" in nme or _family(nme) == "staged" for nme in ran), sorted(ran)
        if fy == FMT_F16:
            for mode in (1, 2):
                assert sum(1 for cs in ran.values() for c in cs if c[8] == mode) >= 6, (mode, "F16 residual")
        assert not any("splitK" in nme or "win<128,64" in nme for nme in ran), sorted(ran)


# ---- strided views and the merged launch in F16 -------------------------------------------------------------------------------------
HALF_VIEW_CASES = [  # n, h, w, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), (n_split, y2_ld, y2_off): channels, 64-granular
    (2, 19, 19, (64, 192, 64), (128, 384, 128), 3, 1, "leaky", (1, 256, 64), (0, 0, 0)),          # slice -> slice, residual with its own ld
    (1, 10, 10, (128, 256, 128), (64, 192, 64), 3, 1, "relu", (2, 128, 64), (0, 0, 0)),           # ... residual before the activation
    (2, 16, 16, (64, 64, 0), (128, 128, 64), 1, 1, "mish", (0, 0, 0), (64, 64, 0)),               # merged: 64 -> slice, 64 -> own tensor
    (2, 13, 13, (128, 192, 64), (192, 256, 64), 1, 1, "leaky", (0, 0, 0), (128, 192, 64)),        # merged 128 + 64, both into slices
    (1, 12, 12, (64, 128, 64), (256, 384, 0), 3, 1, "leaky", (0, 0, 0), (128, 256, 128)),         # merged 128 + 128 on a 3x3 layer
]


@functools.lru_cache(maxsize=None)
def _half_view_refs():
    """(view case, whole input, whole residual, HalfRef on the sliced operands) of every entry of HALF_VIEW_CASES"""
    rng = np.random.RandomState(59)
    out = []
    for vc in HALF_VIEW_CASES:
        n, h, wd, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), _ = vc
        ho, wo = R.out_hw(h, wd, k, s)
        x = rng.standard_normal((n, h, wd, x_ld)).astype(F32)
        w = (rng.standard_normal((cout, k * k * cin)) / np.sqrt(k * k * cin)).astype(F32)
        bias = rng.standard_normal(cout).astype(F32)
        res = rng.standard_normal((n, ho, wo, r_ld)).astype(F32) if res_mode else None
        hr = R.HalfRef((n, h, wd, cin, cout, k, s, act, res_mode), np.ascontiguousarray(x[..., x_off:x_off + cin]), w, bias,
                       np.ascontiguousarray(res[..., r_off:r_off + cout]) if res_mode else None)
        out.append((vc, x, res, hr))
    return tuple(out)


def test_half_views_and_merged_launch_in_f16():
    """An input slice, an output slice of a wider concatenation buffer, a residual with its own ld and the merged launch with two
    outputs, all at 64-channel granularity, in the four format pairs (the F16 ones are what yolov4's CSP blocks run in half mode): the
    slice meets its bound, every channel outside it keeps the sentinel bit for bit (-77 is exact in F16, H16 and fp32)."""
    with _Math(1) as (L, names, mine):
        worst = _Worst()
        sent = np.float32(SENTINEL).view(np.uint32)
        ran = {"slice": set(), "merged": set()}
        for vc, x, res, hr in _half_view_refs():
            n, h, wd, (cin, x_ld, x_off), (cout, y_ld, y_off), k, s, act, (res_mode, r_ld, r_off), (n_split, y2_ld, y2_off) = vc
            view = [x_ld, x_off, y_ld, y_off, r_ld, r_off, n_split, y2_ld, y2_off]
            c1 = n_split if n_split else cout
            for fx, fy in ((FMT_F16, FMT_F16), (FMT_AUTO, FMT_F16), (FMT_F16, FMT_AUTO), (FMT_AUTO, FMT_AUTO)):
                for v in mine:
                    try:
                        y, y2 = _run_half(L, v, fx, fy, x, hr.w, hr.bias, k, s, ACT[act], res, res_mode, view)
                    except L.YdsError as e:
                        assert "planner never launches" in str(e), (names[v], vc, str(e))
                        assert not _takes(names[v], hr.case, fx), (names[v], vc, str(e))
                        continue
                    assert _takes(names[v], hr.case, fx), (names[v], vc)
                    got = np.concatenate([y[:, y_off:y_off + c1], y2[:, y2_off:y2_off + cout - c1]], 1) if n_split else y[:, y_off:y_off + c1]
                    _hold(worst, names[v], (vc, fx, fy), got, _arith(hr, names[v], fy), fy)
                    outside = np.ones(y_ld, bool)
                    outside[y_off:y_off + c1] = False
                    assert (y[:, outside].view(np.uint32) == sent).all(), (names[v], vc, fx, fy, "wrote outside its output slice")
                    if n_split:
                        outside = np.ones(y2_ld, bool)
                        outside[y2_off:y2_off + cout - c1] = False
                        assert (y2[:, outside].view(np.uint32) == sent).all(), (names[v], vc, fx, fy, "wrote outside its second output slice")
                    if fx == FMT_F16 and fy == FMT_F16:
                        ran["merged" if n_split else "slice"].add(names[v])
        worst.report("half mode, views")
        print({k: sorted(v) for k, v in ran.items()})
        sliced, merged = ({_family(nme) for nme in ran[k]} for k in ("slice", "merged"))
        assert sliced >= {"LDS-DMA", "win"} and merged >= {"LDS-DMA", "win"}, (sliced, merged)       # F16 in and out: no staged kernel, no win2
        assert any("win<256,64" in nme for nme in ran["slice"]) and any("win<256,128" in nme for nme in ran["merged"]), ran


def test_half_entry_refuses_bad_formats_and_slices():
    """yds_conv_run_half says no, with a message: outside conv math f16x3, to a format that is neither 0 nor 2, to F16 slices off the
    64-channel granularity, to split-K and the default-arithmetic window tile; make_conv_args' own gate is the only other one."""
    rng = np.random.RandomState(61)
    x = rng.standard_normal((1, 8, 8, 64)).astype(F32)
    w = (rng.standard_normal((64, 64)) / 8).astype(F32)
    w96 = (rng.standard_normal((96, 64)) / 8).astype(F32)
    bias = np.zeros(96, F32)
    with _Math(0) as (L, names, _):
        with pytest.raises(L.YdsError, match="needs conv math f16x3"):
            _run_half(L, 0, 0, 0, x, w, bias, 1, 1, 1, None, 0)
    with _Math(1) as (L, names, mine):
        by = {nme: v for v, nme in enumerate(names)}
        dma = by["conv_igemm_f16x3_dma<128,128,2x2,2>"]
        with pytest.raises(L.YdsError, match="fmt_x / fmt_y"):
            _run_half(L, dma, 1, 0, x, w, bias, 1, 1, 1, None, 0)
        with pytest.raises(L.YdsError, match="does not fit"):                                   # 96 filters: no F16 output
            _run_half(L, dma, 0, FMT_F16, x, w96, bias, 1, 1, 1, None, 0)
        for bad in ([64, 32, 64, 0, 0, 0, 0, 0, 0],                                             # input slice past its tensor
                    [64, 0, 128, 32, 0, 0, 0, 0, 0],                                            # output offset 32: not 64-granular
                    [64, 0, 96, 0, 0, 0, 0, 0, 0]):                                             # ld 96
            with pytest.raises(L.YdsError, match="does not fit"):
                _run_half(L, dma, FMT_F16, FMT_F16, x, w, bias, 1, 1, 1, None, 0, bad)
        for nme in ("conv_igemm_f16x3_dma<64,128,2x2,2>+splitK", "conv3x3_f16x3_win<128,64,4x1>", "conv3x3_f16x3_win<256,128,4x2>",
                    "conv_igemm_f32<128,128,2,2,32>"):
            with pytest.raises(L.YdsError, match="planner never launches"):
                _run_half(L, by[nme], 0, 0, x, w, bias, 1, 1, 1, None, 0)
        with pytest.raises(L.YdsError, match="planner never launches"):                         # the staged kernel does not read F16
            _run_half(L, by["conv_igemm_f16x3<64,64>"], FMT_F16, 0, x, w, bias, 1, 1, 1, None, 0)
        y, _ = _run_half(L, dma, FMT_F16, FMT_F16, x, w, bias, 1, 1, 1, None, 0)               # and takes what the planner does launch
        want = R.conv_ref(R.x_hat(x), R.w_hat(w), bias[:64], 1, 1, 1, None, 0)
        assert np.abs(y - want).max() < 1e-2 and np.array_equal(R.x_hat(y), y)


# ---- tile order ---------------------------------------------------------------------------------------------------------------------
# TILE_ORDER_CASES has 608 / 1248 filters, no multiples of 64, so no F16 output: its first two cases with 640 filters instead - the
# same 5 (3, 10) filter tiles per XCD rectangle at every tile width, so plan_tile_map's shapes are those of the default-mode test.
HALF_TILE_ORDER_CASES = [  # (case, fmt_x)
    ((2, 40, 40, 32, 640, 3, 1, "leaky", 0), FMT_AUTO),       # 32-channel K steps, the window kernels
    ((2, 40, 40, 64, 640, 1, 1, "leaky", 0), FMT_F16),        # 64-channel K steps on an F16 input
]


def test_half_tile_order_is_a_placement():
    """gn = 2 and 4 (bits 8.. of the variant) return the same bits as the column-by-column walk, in half mode with an F16 output."""
    with _Math(1) as (L, names, mine):
        rng = np.random.RandomState(67)
        grouped = set()
        for case, fx in HALF_TILE_ORDER_CASES:
            n, h, wd, cin, cout, k, s, act, res_mode = case
            assert cout % 64 == 0
            x, w, bias, _ = R.make_case(rng, *case[:7], 0)
            hr = R.HalfRef(case, x, w, bias, None)
            for v in mine:
                try:
                    base, _ = _run_half(L, v, fx, FMT_F16, x, w, bias, k, s, ACT[act], None, 0)
                except L.YdsError as e:
                    assert "planner never launches" in str(e) and not _takes(names[v], case, fx), (names[v], case, str(e))
                    continue
                tiles_m, tiles_n, xm, rm, rn = R.plan_tile_map(n * h * wd, cout, *_tile_of(names[v]))
                assert rn >= 3 and rm >= 2, (names[v], case, rm, rn)
                assert any(rn % gn != 0 or gn > rn for gn in (2, 4)), (names[v], case, rn)
                r = _arith(hr, names[v], FMT_F16)
                assert np.array_equal(R.x_hat(base), base) and r.err_f16(base) <= r.mut / 16, (names[v], case, r.err_f16(base), r.mut)
                for gn in (2, 4):
                    got, _ = _run_half(L, v | gn << 8, fx, FMT_F16, x, w, bias, k, s, ACT[act], None, 0)
                    assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (names[v], case, gn, float(np.abs(got - base).max()))
                grouped.add(names[v])
        print("half mode, ran with gn = 2 and 4:", sorted(grouped))
        fams = {_family(nme) for nme in grouped}
        assert fams >= {"staged", "LDS-DMA", "win", "win2"}, fams
        assert sum(1 for nme in grouped if _family(nme) == "LDS-DMA") >= 6, grouped


# ---- saturation ---------------------------------------------------------------------------------------------------------------------
def test_half_f16_output_saturates():
    """The first layer of test_h16_range_saturates with an F16 output (H16 and F16 input): pre-images beyond the format's range come
    out finite, with the right sign, in [65504, 65536] * 256 (the F16 store clamps at 65504); every in-range output keeps its bound."""
    LIM, TOP = 65504.0 * 256, 65536.0 * 256
    with _Math(1) as (L, names, mine):
        rng = np.random.RandomState(23)
        n, h, wd, cin, cout, k = 2, 19, 19, 64, 128, 3
        x = (rng.standard_normal((n, h, wd, cin)) * 1e4).astype(F32)
        w = (rng.standard_normal((cout, k * k * cin)) / np.sqrt(k * k * cin) * 1e3).astype(F32)
        bias = np.zeros(cout, F32)
        hr = R.HalfRef((n, h, wd, cin, cout, k, 1, "linear", 0), x, w, bias, None)
        ran = 0
        for fx in (FMT_AUTO, FMT_F16):
            for v in mine:
                try:
                    got, _ = _run_half(L, v, fx, FMT_F16, x, w, bias, k, 1, 0, None, 0)
                except L.YdsError as e:
                    assert "planner never launches" in str(e) and not _takes(names[v], hr.case, fx), (names[v], str(e))
                    continue
                r = _arith(hr, names[v], FMT_F16)
                over, inside = np.abs(r.want) > 1.01 * TOP, np.abs(r.want) < 0.99 * LIM
                assert over.mean() > 0.02 and inside.mean() > 0.5
                ran += 1
                assert np.isfinite(got).all(), names[v]
                assert (np.abs(got[over]) >= LIM).all() and (np.abs(got[over]) <= TOP).all(), names[v]
                assert np.array_equal(np.sign(got[over]), np.sign(r.want[over])), names[v]
                excess = np.abs(got[inside] - r.want[inside]) - R.ulp16(r.want[inside]) / 2
                assert excess.max() <= r.mut / 16, (names[v], fx, float(excess.max()), r.mut)
                assert np.array_equal(R.x_hat(got[inside]), got[inside]), names[v]
        assert ran >= 12, ran


# ---- the other layer kernels on F16 tensors: exact ---------------------------------------------------------------------------------------
def _pool_ref(x, k, s):
    """oracle/darknet.py's padding: size 2 stride 1 pads one row / column of ZEROS below / right, everything else (k - 1) // 2 of -inf"""
    from oracle.darknet import maxpool_nchw
    if k == 2 and s == 1:
        b, c, h, w = x.shape
        xz = np.zeros((b, c, h + 1, w + 1), F32)
        xz[:, :, :h, :w] = x
        return maxpool_nchw(xz, 2, 1, 0)
    return maxpool_nchw(x, k, s, (k - 1) // 2)


def _h16_round(v):
    """a float64 value as an H16 record keeps it: hi + lo, both fp16 (conv_ref.split_x)"""
    hi, lo = R.split_x(v)
    return hi + lo


@pytest.mark.parametrize("name", ["yolov4", "yolov3-tiny", "yolov4-tiny"])
def test_half_layer_kernels_are_exact_on_f16_tensors(name):
    """Max-pool, nearest upsample, route copy / concatenation (grouped routes too) are exact operations on fp16 values and an unfused
    shortcut is ONE rounding of an exact sum: in half mode, batch 2, at 160 x 96 (5 x 3 maps at stride 32: the SPP windows of 5, 9
    and 13 are larger than the image), layer_output(i) of every such layer whose own or source tensor is F16 equals the numpy operation
    on layer_output of its sources bit for bit (padding as in oracle/darknet.py; shortcut: x_hat(a + b) in float64; a pool that reads
    a 4-byte tensor and writes an F16 one - yolov4-tiny's first - is x_hat of the maximum).  Layers that raise
    "fused" are skipped; the layers each network is here for are asserted to have been compared."""
    from yolo_deepsort_amd import cfgs, synth
    from yolo_deepsort_amd.models import Darknet
    cfg = cfgs.cfg_text(name, 160, 96)
    net = Darknet(None, img_size=(96, 160), batch_max=2, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 4, -2.0))
    x = np.random.RandomState(13).uniform(0, 1, (2, 3, 96, 160)).astype(F32)
    net.half()
    out = np.asarray(net(x))
    assert np.isfinite(out).all()
    defs = net.module_defs
    fmt = [net.layer_format(i) for i in range(len(defs))]
    cache = {}

    def layer(i):
        if i not in cache:
            try:
                cache[i] = net.layer_output(i, batch=2)
            except Exception as e:                      # conv fused with the following shortcut / never materialised
                assert "fused" in str(e), (i, str(e))
                cache[i] = None
        return cache[i]

    checked = []
    for i, d in enumerate(defs):
        t = d["type"]
        if t not in ("maxpool", "upsample", "route", "shortcut"):
            continue
        if t == "route":
            src = [int(v) for v in d["layers"].split(",")]
        elif t == "shortcut":
            src = [-1, int(d["from"])]
        else:
            src = [-1]
        src = [l if l >= 0 else i + l for l in src]
        if fmt[i] != 2 and not any(fmt[l] == 2 for l in src):
            continue
        got, ins = layer(i), [layer(l) for l in src]
        if got is None or any(a is None for a in ins):
            continue
        if t == "maxpool":
            want, what = _pool_ref(ins[0], int(d["size"]), int(d["stride"])), f"maxpool k{d['size']} s{d['stride']}"
            if fmt[i] == 2 and fmt[src[0]] != 2:            # an H16 / fp32 source pooled into an F16 tensor: the maximum, rounded once
                want = R.x_hat(want).astype(F32)
        elif t == "upsample":
            sc = int(d["stride"])
            want, what = ins[0].repeat(sc, axis=2).repeat(sc, axis=3), "upsample"
        elif t == "route":
            want, what = np.concatenate(ins, 1), "route" if len(ins) == 1 else f"concat of {len(ins)}"
            if "groups" in d:
                g, gid = int(d["groups"]), int(d["group_id"])
                c = want.shape[1] // g
                want, what = want[:, gid * c:(gid + 1) * c], "grouped route"
        else:
            total = ins[0].astype(np.float64) + ins[1].astype(np.float64)
            want = R.x_hat(total) if fmt[i] == 2 else _h16_round(total) if fmt[i] == 1 else total
            want, what = want.astype(F32), "shortcut"
        assert got.shape == want.shape, (i, what, got.shape, want.shape)
        want = np.ascontiguousarray(want, F32)
        same = got.view(np.uint32) == want.view(np.uint32)
        if t == "maxpool":                                  # the maximum of +0 and -0 has no defined sign (IEEE 754 maxNum): either zero is the maximum
            same |= (got == 0) & (want == 0)
        bad = np.argwhere(~same)[:4]
        assert same.all(), (name, i, what, fmt[i], [fmt[l] for l in src], int((~same).sum()),
                            [(tuple(b), float(got[tuple(b)]), float(want[tuple(b)])) for b in bad])
        assert np.abs(got).max() > 0
        checked.append((i, what, fmt[i], tuple(fmt[l] for l in src)))
    print(f"{name} half mode, exact layers checked (layer, kind, own format, source formats):")
    for row in checked:
        print("   ", row)
    kinds = [w for _, w, _, _ in checked]
    if name == "yolov4":
        assert {"maxpool k5 s1", "maxpool k9 s1", "maxpool k13 s1"} <= set(kinds), kinds
        assert kinds.count("upsample") >= 2, kinds
        assert any(w.startswith("concat") and fi == 2 and set(fs) == {2} for _, w, fi, fs in checked), checked
    elif name == "yolov3-tiny":
        assert "maxpool k2 s1" in kinds and "maxpool k2 s2" in kinds, kinds
    else:
        assert "grouped route" in kinds, kinds
