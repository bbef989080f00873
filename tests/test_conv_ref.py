"""The conv kernel tests' bound, checked on the CPU: for every case of conv_ref.CASES (and FUSED_CASES, the fused stem kernels' cases) the
reference arithmetic alone separates from the mutants that tests/test_gpu_conv_variants.py (test_gpu_conv_fused.py) has to catch.  A case whose data makes mut / 16 meaningless fails here, not on the GPU."""
import numpy as np
import pytest

import conv_ref as R


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=lambda i: "x".join(str(v) for v in R.CASES[i]))
def test_reference_arithmetic_separates_from_the_mutants(i):
    """The three-term split-fp16 sum (exact accumulation, rounded to fp32) and a plain fp32 CPU convolution both sit at or below
    mut / 64, where mut is the smaller error of the two mutants that drop one cross term (conv_ref.mutant_bound)."""
    r = R.case_refs()[i]
    emu = r.err(R.emulated_f16x3(r.x, r.w, r.bias, r.k, r.s, r.act, r.res, r.res_mode))
    print(f"{r.case}: scale {r.scale:.2f} mut {r.mut:.2e} mut/scale {r.mut / r.scale:.1e} | f16x3 emulation mut/{r.mut / emu:.0f} "
          f"fp32 conv mut/{r.mut / r.err_fp32:.0f}")
    assert r.mut > 0 and np.isfinite(r.mut)
    assert r.mut < 1e-3 * r.scale          # the mutants pass the suite's older bar: only mut / 16 can catch them
    assert emu <= r.mut / 64, (r.case, emu, r.mut)
    assert r.err_fp32 <= r.mut / 64, (r.case, r.err_fp32, r.mut)


def test_mutant_operands_are_the_hi_halves():
    """x_hat / w_hat are what a kernel reads when it drops the lo half: fp16 values (scaled by 256 for activations), and hi + lo
    restores the operand to the 22 bits the H16 format keeps."""
    rng = np.random.RandomState(5)
    x = rng.standard_normal(4096).astype(R.F32) * 3
    hi, lo = R.split_x(x)
    assert np.array_equal((hi / 256).astype(np.float16).astype(np.float64) * 256, hi)
    assert np.abs(hi - x).max() > 2.0 ** -12 * 0.5 and np.abs(hi - x).max() <= 2.0 ** -11 * np.abs(x).max()
    assert np.abs(hi + lo - x).max() <= 2.0 ** -21 * np.abs(x).max()
    w = rng.standard_normal(4096).astype(R.F32) / 24
    wh, wl = R.split_w(w)
    assert np.array_equal(wh, w.astype(np.float16).astype(np.float64))
    assert np.abs(wh + wl - w).max() <= 2.0 ** -21 * np.abs(w).max()


def test_plan_tile_map_restatement():
    """the host port of plan_tile_map on the tile-order shapes: the plans the tile-order test relies on"""
    for (BM, BN), (rm, rn) in {(128, 128): (4, 5), (128, 64): (7, 5), (64, 64): (13, 5), (64, 128): (7, 5), (256, 128): (2, 5),
                               (128, 256): (4, 3), (128, 32): (7, 10), (256, 64): (2, 10)}.items():
        assert R.plan_tile_map(2 * 40 * 40, 608, BM, BN)[3:] == (rm, rn), (BM, BN)
    assert R.plan_tile_map(2 * 28 * 28, 1248, 128, 128)[3:] == (4, 5)
    assert R.plan_tile_map(2 * 28 * 28, 1248, 128, 256)[4] == 3


# ---- half mode ------------------------------------------------------------------------------------------------------------------------
_HALF = list(R.CASES) + list(R.HALF_CASES)


@pytest.mark.parametrize("i", range(len(_HALF)), ids=lambda i: "x".join(str(v) for v in _HALF[i]))
def test_half_reference_arithmetic_separates_from_the_mutants(i):
    """Half mode (conv_ref.HalfRef), both output formats: a plain fp32 CPU convolution of the ROUNDED operands sits at or below
    mut / 64 of the float64 result, and rounded to nearest into the F16 format it exceeds half a spacing by no more than mut / 64 -
    a factor 4 inside the mut / 16 of tests/test_gpu_conv_half.py.  The bound bites: the same fp32 result rounded TOWARD ZERO breaks
    the F16 bound on every case whose |want| reaches 1 (a truncating store is one fp16 ulp, which no network test sees)."""
    hr = R.half_refs()[i]
    assert hr.case == _HALF[i]
    cout = hr.case[4]
    for fy in (R.FMT_AUTO, R.FMT_F16) if cout % 64 == 0 else (R.FMT_AUTO,):
        r = hr.half(fy)
        assert r.mut > 0 and np.isfinite(r.mut)
        assert r.mut < 1e-3 * r.scale
        stored = R.x_hat(r.fp32)                                  # the F16 store: fp16(v / 256) * 256, to nearest even
        over = r.err_f16(stored)
        print(f"{hr.case} fmt_y {fy}: scale {r.scale:.2f} mut {r.mut:.2e} | fp32 conv mut/{r.mut / max(r.err_fp32, 1e-30):.0f}, "
              f"as F16 beyond half an ulp mut/{r.mut / max(over, 1e-30):.0f}")
        assert r.err_fp32 <= r.mut / 64, (hr.case, fy, r.err_fp32, r.mut)
        assert over <= r.mut / 64, (hr.case, fy, over, r.mut)
        assert np.array_equal(R.x_hat(stored), stored)
        if fy == R.FMT_F16 and r.scale >= 1:
            cut = R.trunc16(r.fp32)
            assert np.array_equal(R.x_hat(cut), cut) and (np.abs(cut) <= np.abs(r.fp32)).all()
            assert r.err_f16(cut) > r.mut / 16, (hr.case, "a truncating store passes the bound", r.err_f16(cut), r.mut)
        # the three-term arithmetic on the same tensors (the kernels that ignore `terms`): Ref's quantities, residual as stored
        f = hr.full(fy)
        assert 0 < f.mut < 1e-3 * f.scale and f.err_fp32 <= f.mut / 64, (hr.case, fy, f.err_fp32, f.mut)


def test_half_operands_and_ulp16():
    """ulp16 is the spacing of fp16(v / 256) * 256 (subnormals included), trunc16 rounds toward zero onto that grid, and the half
    reference of a case without a residual does not depend on the output format."""
    v = np.array([0.0, 1e-9, 2.0 ** -6, 2.0 ** -6 * 1.5, 0.999, 1.0, 1.5, 255.9, 256.0, 3e3, -7.3, 60000.0 * 256])
    h = (np.abs(v) / 256).astype(np.float16)
    assert np.array_equal(R.ulp16(v), np.spacing(h).astype(np.float64) * 256)
    rng = np.random.RandomState(7)
    x = rng.standard_normal(4096) * 5
    t, n = R.trunc16(x), R.x_hat(x)
    assert (np.abs(t) <= np.abs(x)).all() and (np.abs(x - t) < R.ulp16(x)).all() and np.array_equal(R.x_hat(t), t)
    assert (np.abs(x - n) <= R.ulp16(x) / 2).all() and (t != n).mean() > 0.3
    hr = R.half_refs()[0]
    assert hr.res_mode == 0 and hr.half(R.FMT_F16) is hr.half(R.FMT_AUTO)
    assert R.half_formats((1, 1, 1, 64, 64, 3, 1, "relu", 2)) == [(0, 0), (0, 2), (2, 0), (2, 2)]
    assert R.half_formats((1, 1, 1, 96, 160, 3, 2, "mish", 0)) == [(0, 0)] and R.half_formats((1, 1, 1, 32, 64, 3, 1, "mish", 0)) == [(0, 0), (0, 2)]


# ---- the fused stem kernels (tests/test_gpu_conv_fused.py) ----------------------------------------------------------------------------
_FUSED = [(kind, i) for kind in ("stem2", "block1", "pool", "direct") for i in range(len(R.FUSED_CASES[kind]))]


@pytest.mark.parametrize("kind,i", _FUSED, ids=[kind + "-" + "x".join(str(c) for c in R.FUSED_CASES[kind][i] if c != "" and c != 0) for kind, i in _FUSED])
def test_fused_reference_arithmetic_separates_from_the_mutants(kind, i):
    """Every case of conv_ref.FUSED_CASES: the three-term composition (exact accumulation, the intermediate re-split to hi + lo
    between the stages, shortcut and result as H16 holds them) and the plain fp32 CPU composition both sit at or below mut / 64, where
    mut is the smallest float64 error of the mutants that round one operand of one stage (FUSED_MUTANTS)."""
    r = R.fused_refs(kind)[i]
    assert r.case == R.FUSED_CASES[kind][i] and set(r.mutant_err) == set(R.FUSED_MUTANTS[kind])
    emu = r.err(r.emulated())
    print(f"{kind} {r.case}: scale {r.scale:.2f} mut {r.mut:.2e} mut/scale {r.mut / r.scale:.1e} | f16x3 emulation mut/{r.mut / max(emu, 1e-30):.0f} "
          f"fp32 mut/{r.mut / max(r.err_fp32, 1e-30):.0f} | mutants / scale " + ", ".join(f"{k} {v / r.scale:.1e}" for k, v in r.mutant_err.items()))
    assert r.mut > 0 and np.isfinite(r.mut)
    assert r.mut < 1e-3 * r.scale          # every mutant's smallest error passes the older bar: only mut / 16 can catch it
    assert emu <= r.mut / 64, (kind, r.case, emu, r.mut)
    assert r.err_fp32 <= r.mut / 64, (kind, r.case, r.err_fp32, r.mut)
    if r.case[5] == "u8":
        assert np.array_equal(np.round(r.x * 255), r.x * np.float32(255)) and r.x[..., :3].max() > 0.9
    if kind != "block1":
        assert not r.x[..., 3].any() and 0 <= r.x.min() and r.x.max() <= 1


@pytest.mark.parametrize("kind", ["stem2", "block1", "pool", "direct"])
def test_fused_hold_fails_on_every_mutant(kind):
    """What tests/test_gpu_conv_fused.py does with a kernel's output (`_hold`) fails on every mutant tensor of every case - a kernel
    that loses the lo half of any one operand cannot pass - and accepts both reference arithmetics."""
    import test_gpu_conv_fused as G
    for r in R.fused_refs(kind):
        worst = G._FusedWorst()
        G._hold(worst, kind, r.case, r.emulated(), r)
        G._hold(worst, kind, r.case, r.fp32(), r)
        for name in R.FUSED_MUTANTS[kind]:
            with pytest.raises(AssertionError, match="above mut / 16"):
                G._hold(worst, kind, (r.case, name), r.mutant(name), r)


def test_fused_half_construction_is_exact():
    """conv_ref.FusedHalfRef: the intermediate is positive (leaky is the identity), equals its own hi half, and the fp32 pipeline
    reproduces it bit for bit, so half mode's rounding of the LDS patch changes nothing; stage two in fp32 on the rounded operands sits
    at or below mut / 64, also beyond half a spacing once stored as F16; `_hold` fails on the mutant."""
    import test_gpu_conv_fused as G
    for hr in R.fused_half_refs():
        assert hr.h.min() > 0 and hr.h.max() < (24 if hr.kind == "stem2" else 64)
        assert np.array_equal(R.x_hat(hr.h), hr.h) and np.array_equal(R.x_hat(hr.x), hr.x)
        assert np.array_equal(hr.stage_one(R.fp32_pre), hr.h)
        assert np.array_equal(hr.stage_one(R.emu_pre), hr.h)
        for fmt in (R.FMT_AUTO, R.FMT_F16):
            a = hr.half(fmt)
            stored = R.x_hat(a.fp32)
            print(f"{hr.case} fmt {fmt}: scale {a.scale:.2f} mut/scale {a.mut / a.scale:.1e} | fp32 mut/{a.mut / max(a.err_fp32, 1e-30):.0f}, "
                  f"as F16 beyond half an ulp mut/{a.mut / max(a.err_f16(stored), 1e-30):.0f}")
            assert 0 < a.mut < 1e-3 * a.scale
            assert a.err_fp32 <= a.mut / 64 and a.err_f16(stored) <= a.mut / 64, (hr.case, fmt, a.err_fp32, a.mut)
            mutant = hr._stage_two(R.conv_pre, hr.wb, fmt)
            for f16 in (False, True):
                with pytest.raises(AssertionError, match="above mut / 16"):
                    G._hold(G._FusedWorst(), hr.kind, hr.case, R.x_hat(mutant) if f16 else mutant, a, f16=f16)


# ---- the fused kernels in half mode on generic operands (test_fused_half_mode_on_generic_operands) -------------------------------------
_GENERIC = [(kind, i) for kind in ("stem2", "block1") for i in range(len(R.FUSED_GENERIC_CASES[kind]))]


@pytest.mark.parametrize("kind,i", _GENERIC, ids=[kind + "-" + "x".join(str(c) for c in R.FUSED_GENERIC_CASES[kind][i][:4]) for kind, i in _GENERIC])
def test_fused_generic_bound_admits_the_kernel_and_no_mutant(kind, i):
    """conv_ref.FusedHalfGenericRef, every case, both tensor formats.
    (a) The emulated kernel - stage one by the fp32 CPU convolution, activation, rounded to fp32 and then to the hi half; stage two in
        float64 on the rounded operands, rounded to fp32 and, for F16, into that format - passes `_hold_bound`, and every intermediate
        it rounds to the other neighbour is one the reference calls ambiguous.
    (b) Every mutant fails `_hold_bound` on its bound: as the float64 tensor against the H16 bound, stored as F16 against the F16 one.
    (c) The widening stays rare, which is what keeps it from hiding a failure: at most 10 % of the outputs have a bound above mut / 2
        (an F16 output's own half spacing aside), at most 25 % of the intermediates are ambiguous.  Conditions on the inputs, no tolerances.
    (d) Stem: fp16 holds the layer-0 bias in at most 2 of 32 channels, and the kernel that adds the fp32 bias is one of the mutants."""
    import test_gpu_conv_fused as G
    r = R.fused_generic_refs(kind)[i]
    assert r.case == R.FUSED_GENERIC_CASES[kind][i]
    flips, outside = r.flips()
    over = float((r.mut / 16 + r.widen > r.mut / 2).mean())
    print(f"{kind} {r.case}: mut {r.mut:.2e}, {r.amb.mean():.1%} ambiguous, {over:.1%} of the outputs bounded above mut/2, the emulation flips {flips} "
          f"intermediates ({outside} outside the ambiguous set) | mutants / mut " + ", ".join(f"{k} {v / r.mut:.1f}" for k, v in r.mutant_err.items()))
    assert r.mut > 0 and np.isfinite(r.mut)
    assert outside == 0, (kind, r.case, outside)                                                       # (a)
    assert over <= 0.10 and r.amb.mean() <= 0.25, (kind, r.case, over, r.amb.mean())                   # (c)
    assert set(r.mutant_err) == set(r.mutants) and ("ba fp32" in r.mutants) == (kind == "stem2")       # (d)
    if kind == "stem2":
        assert (R._f16(r.ba) != r.ba).sum() >= 30 and not np.array_equal(r.bias1, r.ba)
    else:
        assert np.array_equal(r.bias1, r.ba)
    cores = {name: r.mutant_core(name) for name in r.mutants}
    for fmt in (R.FMT_AUTO, R.FMT_F16):
        a = r.half(fmt)
        assert r.mut < 1e-3 * a.scale                                   # every mutant's smallest error passes the older bar
        worst = G._BoundWorst()
        G._hold_bound(worst, kind, r.case, a.fp32, a)                                                  # (a)
        print(f"  fmt {fmt}: the emulation at {worst.rows[kind][0]:.2f} of the bound; mutants' violations / worst ratio " +
              ", ".join(f"{k} {a.violations(v + r.shortcut(fmt)):.0%} / {a.ratio(v + r.shortcut(fmt)):.1f}" for k, v in cores.items()))
        for name, core in cores.items():                                                               # (b)
            m = core + r.shortcut(fmt)
            with pytest.raises(AssertionError, match="above their bound"):
                G._hold_bound(G._BoundWorst(), kind, (r.case, name), R.x_hat(m) if fmt == R.FMT_F16 else m, a)
