"""The kernels that run first in every pass, each on its own vs a float64 reference of the whole composition (conv_ref.FusedRef):
conv_stem2_f16x3 (detector layers 0 + 1) and conv_block1_f16x3 (first residual block), which exist only as fused launches and are
reached through the C ABI entry yds_conv_run_fused; conv3x3_rgb_pool_mfma / conv3x3_rgb_pool (ReID stem conv + max-pool, f16x3 and exact
fp32 math) through the same entry; conv3x3_rgb_direct<32 / 64> through yds_conv_run.  The entry calls the fused launcher itself, so no
other kernel can stand in for one of these.

Bounds, as in test_gpu_conv_variants.py: 1e-3 of the output scale, and mut / 16, where mut is the smallest float64 error of the mutants
that round ONE operand of ONE stage to its hi half - the input, either filter set, the LDS intermediate, the shortcut, the H16 output
(conv_ref.FUSED_MUTANTS).  test_conv_ref.py shows on the CPU that the three-term arithmetic and a plain fp32 composition sit at or
below mut / 64 on every case here, and that `_hold` fails on every one of the mutants.

Half mode.  The HALF instantiations of the two fused kernels round the LDS intermediate to its hi half, and that rounding is
discontinuous: fp32 noise in stage one flips a few intermediates that sit next to a rounding midpoint to the neighbouring fp16 value,
and one flip moves an output by mut / 3 or so (small intermediates after leaky fall into the subnormal range of fp16(h / 256), where
the spacing is coarse).  No UNIFORM bound of mut / 16 survives that, so the half-mode instantiations are held twice:
  * test_fused_half_mode_with_an_exact_first_stage makes stage one EXACT in every arithmetic (conv_ref.FusedHalfRef: dyadic inputs and
    filters, a bias that keeps every intermediate positive and on a grid fp16 holds), which leaves stage two as a plain half-mode
    convolution with one mutant, the kernel that reads the lo half of the second filter set;
  * test_fused_half_mode_on_generic_operands runs all four HALF instantiations (leaky and mish, stem and block, H16 and F16 tensors) on
    make_fused_case's operands - nothing dyadic, nothing kept positive, an fp32 bias that fp16 does not hold - against a PER-OUTPUT
    bound (conv_ref.FusedHalfGenericRef): the reference marks the intermediates within the fp32 error of a rounding midpoint as
    ambiguous, and an output's bound is mut / 16 plus what flipping the ambiguous intermediates under its taps can move it - nothing for
    an output whose taps see none.  mut is the smallest error of six mutants (an unrounded x, wa or wb, an intermediate that keeps its
    lo half or is truncated, and for the stem an fp32 layer-0 bias).  test_conv_ref.py shows on the CPU that an fp32 emulation of the
    kernel passes, that every mutant fails at every case, and that the widening stays rare (at most 10 % of the outputs above mut / 2)."""
import os

import numpy as np
import pytest

import conv_ref as R
from conv_ref import F32, FMT_AUTO, FMT_F16
from test_gpu_conv_variants import _Math, _Worst, _run

pytestmark = pytest.mark.gpu

ACT_NAME = {v: k for k, v in R.ACT.items()}


class _FusedWorst(_Worst):
    """_Worst for kernels outside the implicit-GEMM families: one row per kernel instantiation"""

    def report(self, title):
        print(f"\n{title}: worst err/scale, err/mut, err/err_fp32 per kernel")
        for name, (a, b, c) in self.rows.items():
            print(f"  {name:46s} {a:.1e}  mut/{1 / max(b, 1e-30):7.0f}  {c:6.2f} x fp32" + ("   <-- between mut/64 and mut/16" if b > 1 / 64 else ""))


def _hold(worst, name, what, got, r, f16=False):
    """records and checks one result against r (FusedRef or _Arith): err < 1e-3 * scale and err <= mut / 16; an F16 output is held
    beyond half a spacing of its format and must be representable in it"""
    assert got.shape == r.want.shape, (name, what, got.shape, r.want.shape)
    assert np.isfinite(got).all(), (name, what, "non-finite output")
    if f16:
        assert np.array_equal(R.x_hat(got), got), (name, what, "an F16 output holds values outside the format")
        worst.hold(name, what, r.err_f16(got), r)
    else:
        worst.hold(name, what, r.err(got), r)


class _BoundWorst:
    """per kernel: worst err / bound, worst err / mut over the outputs whose widening is under mut / 64 (the bound is as sharp there as the
    other conv tests'), worst err / err of the fp32 emulation"""

    def __init__(self):
        self.rows = {}

    def record(self, name, got, a):
        row = self.rows.setdefault(name, [0.0, 0.0, 0.0])
        for i, v in enumerate((a.ratio(got), a.err_sharp(got) / a.mut, a.err(got) / max(a.err_fp32, 1e-30))):
            row[i] = max(row[i], v)

    def report(self, title):
        print(f"\n{title}: worst err/bound, err/mut where the widening is under mut/64, err/err_emulation per kernel")
        for name, (a, b, c) in self.rows.items():
            print(f"  {name:46s} {a:5.2f} of the bound  " + (f"mut/{1 / b:7.0f}" if b > 0 else "      none") + f"  {c:6.2f} x emulation")


def _hold_bound(worst, name, what, got, a):
    """records and checks one result against a (conv_ref._BoundArith): finite, an F16 output representable in its format, err < 1e-3 *
    scale, and EVERY output within its own bound"""
    assert got.shape == a.want.shape, (name, what, got.shape, a.want.shape)
    assert np.isfinite(got).all(), (name, what, "non-finite output")
    if a.f16:
        assert np.array_equal(R.x_hat(got), got), (name, what, "an F16 output holds values outside the format")
    worst.record(name, got, a)
    print(f"  {name} {what}: err/bound {a.ratio(got):.2f}, err/scale {a.err(got) / a.scale:.1e}, {a.violations(got):.2%} of the outputs beyond their bound")
    assert a.err(got) < 1e-3 * a.scale, (name, what, a.err(got) / a.scale)
    assert a.violations(got) == 0, (name, what, f"{a.violations(got):.2%} of the outputs above their bound, the worst at {a.ratio(got):.2f} of it")


def _out_shape(kind, n, h, w):
    return (n, 64, h, w) if kind == "block1" else (n, 64, (h - 1) // 2 + 1, (w - 1) // 2 + 1)


def _run_fused(L, kind, x, wa, ba, wb, bb, act, half=0, fmt=0):
    n, h, w, _ = x.shape
    y = np.empty(_out_shape(kind, n, h, w), F32)
    L.check(L.load().yds_conv_run_fused(R.FUSED_KINDS[kind], n, h, w, act, half, fmt, L.ptr(x), L.ptr(wa), L.ptr(ba), L.ptr(wb), L.ptr(bb), L.ptr(y)))
    return y


@pytest.mark.parametrize("kind", ["stem2", "block1"])
def test_fused_stem_and_block_vs_float64(kind):
    """conv_stem2_f16x3<act, act, false> / conv_block1_f16x3<act, false>, leaky and mish: one patch, ragged patches with odd extents,
    images smaller than a patch, and more patches than the persistent grid across several images (conv_ref.FUSED_CASES)."""
    with _Math(1) as (L, names, _):
        worst = _FusedWorst()
        for r in R.fused_refs(kind):
            got = _run_fused(L, kind, r.x, r.wa, r.ba, r.wb, r.bb, r.act)
            _hold(worst, f"conv_{kind}_f16x3<{ACT_NAME[r.act]}>", r.case, got, r)
        worst.report(f"fused {kind}")
        assert len(worst.rows) == 2, worst.rows.keys()


@pytest.mark.parametrize("math", [1, 0])
def test_stem_conv_pool_vs_float64(math):
    """The ReID stem, conv + ReLU / leaky + MaxPool(3, 2, 1): conv3x3_rgb_pool_mfma in f16x3 math (H16 output), conv3x3_rgb_pool (the
    fp32 fma chain, fp32 output) in exact-fp32 math; the crop shape, odd extents, images smaller than a patch, 528 patches."""
    assert "YDS_POOL_VALU" not in os.environ, "the switch would replace the matrix-core kernel this test names"
    with _Math(math) as (L, names, _):
        worst = _FusedWorst()
        for r in R.fused_refs("pool"):
            got = _run_fused(L, "pool", r.x, r.wa, r.ba, None, None, r.act)
            _hold(worst, f"conv3x3_rgb_pool{'_mfma' if math else ''}<{ACT_NAME[r.act]}>", r.case, got, r)
        worst.report(f"stem conv + pool, conv math {math}")
        assert len(worst.rows) == 2, worst.rows.keys()


@pytest.mark.parametrize("math", [1, 0])
def test_direct_first_layer_vs_float64(math):
    """conv3x3_rgb_direct<32 / 64> (the fp32 fma chain in both math modes; H16 output with its own encode in f16x3 math, fp32 output
    otherwise): every activation, one tile, ragged tiles, one pixel, and 2210 tiles against the grid of 2048 persistent workgroups."""
    with _Math(math) as (L, names, _):
        direct = [v for v, nme in enumerate(names) if "direct" in nme]
        assert len(direct) == 1, names
        worst = _FusedWorst()
        for r in R.fused_refs("direct"):
            got = _run(L, direct[0], r.x, r.wa, r.ba, 3, 1, r.act, None, 0)
            _hold(worst, f"conv3x3_rgb_direct<{r.case[4]},{ACT_NAME[r.act]}>", r.case, got, r)
        worst.report(f"direct first layer, conv math {math}")
        assert len(worst.rows) == 8, worst.rows.keys()


def test_fused_half_mode_with_an_exact_first_stage():
    """conv_stem2_f16x3<leaky, leaky, true> and conv_block1_f16x3<leaky, true> on operands whose intermediate is exact in every
    arithmetic (module docstring): H16 outputs at or below mut / 16 of the float64 result on w_hat(wb), F16 outputs (and, for the block,
    F16 input and shortcut) within half a spacing of the format plus mut / 16."""
    with _Math(1) as (L, names, _):
        worst = _FusedWorst()
        for hr in R.fused_half_refs():
            for fmt in (FMT_AUTO, FMT_F16):
                got = _run_fused(L, hr.kind, hr.x, hr.wa, hr.ba, hr.wb, hr.bb, hr.act, half=1, fmt=fmt)
                _hold(worst, f"conv_{hr.kind}_f16x3<leaky,HALF> {'F16' if fmt else 'H16'}", hr.case, got, hr.half(fmt), f16=fmt == FMT_F16)
        worst.report("fused kernels, half mode")
        assert len(worst.rows) == 4, worst.rows.keys()


def test_fused_half_mode_on_generic_operands():
    """conv_stem2_f16x3<leaky, leaky, true>, <mish, mish, true>, conv_block1_f16x3<leaky, true> and <mish, true> on generic operands,
    H16 and F16 tensors, every output within its own bound of the float64 half-mode composition (module docstring): one patch, ragged
    patches with odd extents, images smaller than a patch, and 300 / 330 tiles against the 256 persistent workgroups, where the
    grid-stride loop and the next-tile prefetch run (conv_ref.FUSED_GENERIC_CASES).
    Measured on MI355X, worst err / bound per kernel (H16 tensors, F16 tensors): stem leaky 0.81, 0.94; stem mish 0.82, 0.95; block
    leaky 0.71, 0.94; block mish 0.64, 0.97 - the CPU emulation sits at 0.81 / 0.84 / 0.71 / 0.75 and 0.94 .. 0.97 (an F16 store alone
    takes up to half a spacing, which is most of its bound); where the widening is under mut / 64 the H16 outputs sit at mut / 272
    (stem) and mut / 545 (block) or better and no F16 output leaves its half spacing (reported as "none").  The kernel is on the
    reference's side of every mutant, the stem's fp32 bias included: its H16 output lies 0.97 mut or more from each mutant tensor (1.09 mut or more
    from the stem with an fp32 bias)."""
    with _Math(1) as (L, names, _):
        worst = _BoundWorst()
        for kind in ("stem2", "block1"):
            for r in R.fused_generic_refs(kind):
                for fmt in (FMT_AUTO, FMT_F16):
                    got = _run_fused(L, kind, r.x, r.wa, r.ba, r.wb, r.bb, r.act, half=1, fmt=fmt)
                    _hold_bound(worst, f"conv_{kind}_f16x3<{ACT_NAME[r.act]},HALF> {'F16' if fmt else 'H16'}", r.case, got, r.half(fmt))
        worst.report("fused kernels, half mode, generic operands")
        assert len(worst.rows) == 8, worst.rows.keys()


def test_fused_entry_refuses_what_the_launchers_refuse():
    """yds_conv_run_fused says no with a message - its own for arguments that name no launch, the launcher's where the launch does not
    apply - and never runs another kernel instead."""
    rng = np.random.RandomState(97)
    x4 = np.zeros((1, 4, 6, 4), F32)
    x4[..., :3] = rng.uniform(0, 1, (1, 4, 6, 3))
    x64 = rng.standard_normal((1, 4, 6, 64)).astype(F32)
    w0, w1 = (rng.standard_normal((32, 36)) / 6).astype(F32), (rng.standard_normal((64, 288)) / 17).astype(F32)
    w2, wp = (rng.standard_normal((32, 64)) / 8).astype(F32), (rng.standard_normal((64, 36)) / 6).astype(F32)
    b32, b64 = np.zeros(32, F32), np.zeros(64, F32)
    leaky, mish, relu = R.ACT["leaky"], R.ACT["mish"], R.ACT["relu"]
    with _Math(0) as (L, names, _):
        for kind, x, wa in (("stem2", x4, w0), ("block1", x64, w2)):
            with pytest.raises(L.YdsError, match="conv math f16x3 required"):
                _run_fused(L, kind, x, wa, b32, w1, b64, leaky)
    with _Math(1) as (L, names, _):
        lib = L.load()
        y = np.empty((1, 64, 4, 6), F32)
        for kind_id, msg in ((3, "kind is 0"), (-1, "kind is 0")):
            assert lib.yds_conv_run_fused(kind_id, 1, 4, 6, leaky, 0, 0, L.ptr(x4), L.ptr(w0), L.ptr(b32), L.ptr(w1), L.ptr(b64), L.ptr(y)) != 0
            assert msg in L.last_error()
        with pytest.raises(L.YdsError, match="fmt is 0"):
            _run_fused(L, "stem2", x4, w0, b32, w1, b64, leaky, half=1, fmt=1)
        with pytest.raises(L.YdsError, match="half mode only"):
            _run_fused(L, "block1", x64, w2, b32, w1, b64, leaky, half=0, fmt=FMT_F16)
        with pytest.raises(L.YdsError, match="takes two convolutions"):
            _run_fused(L, "stem2", x4, w0, b32, None, None, leaky)
        with pytest.raises(L.YdsError, match="no half mode"):
            _run_fused(L, "pool", x4, wp, b64, None, None, relu, half=1)
        with pytest.raises(L.YdsError, match="the fused stem takes"):                   # the launchers' own refusals
            _run_fused(L, "stem2", x4, w0, b32, w1, b64, relu)
        with pytest.raises(L.YdsError, match="the fused residual block takes"):
            _run_fused(L, "block1", x64, w2, b32, w1, b64, relu)
        with pytest.raises(L.YdsError, match="conv\\+pool: unsupported activation"):
            _run_fused(L, "pool", x4, wp, b64, None, None, mish)
        got = _run_fused(L, "stem2", x4, w0, b32, w1, b64, leaky)                       # and takes what the launcher does
        want = R.fused_eval("stem2", x4, w0, b32, w1, b64, leaky)
        assert np.abs(got - want).max() < 1e-4
