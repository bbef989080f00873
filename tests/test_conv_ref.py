"""The conv kernel tests' bound, checked on the CPU: for every case of conv_ref.CASES the reference arithmetic alone separates from
the mutants that tests/test_gpu_conv_variants.py has to catch.  A case whose data makes mut / 16 meaningless fails here, not on the GPU."""
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
