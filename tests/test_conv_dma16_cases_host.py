"""The bound of tests/test_gpu_conv_dma16.py, checked on the CPU: on exactly its cases (conv_dma16_cases) the reference arithmetic alone
separates from the mutants the GPU test has to catch, so mut / 16 there has the margin that test_conv_ref.py documents for the suite's
older cases.  A case whose data makes mut / 16 meaningless fails here, not on the GPU."""
import numpy as np
import pytest

import conv_dma16_cases as D
import conv_ref as R

_ALL = D.all_cases()


@pytest.mark.parametrize("i", range(len(_ALL)), ids=lambda i: "x".join(str(v) for v in _ALL[i]))
def test_reference_arithmetic_separates_from_the_mutants(i):
    """The three-term split-fp16 sum (exact accumulation, rounded to fp32) and a plain fp32 CPU convolution both sit at or below
    mut / 64, where mut is the smaller error of the two mutants that drop one cross term (conv_ref.mutant_bound)."""
    r = D.refs()[i]
    assert r.case == _ALL[i]
    emu = r.err(R.emulated_f16x3(r.x, r.w, r.bias, r.k, r.s, r.act, r.res, r.res_mode))
    print(f"{r.case}: scale {r.scale:.2f} mut {r.mut:.2e} mut/scale {r.mut / r.scale:.1e} | f16x3 emulation mut/{r.mut / max(emu, 1e-30):.0f} "
          f"fp32 conv mut/{r.mut / max(r.err_fp32, 1e-30):.0f}")
    assert r.mut > 0 and np.isfinite(r.mut)
    assert r.mut < 1e-3 * r.scale          # the mutants pass the suite's older bar: only mut / 16 can catch them
    assert emu <= r.mut / 64, (r.case, emu, r.mut)
    assert r.err_fp32 <= r.mut / 64, (r.case, r.err_fp32, r.mut)


def test_cases_reach_the_edges_they_name():
    """the case list holds what the GPU test's docstring promises: K steps 1..4 and 9, M and Cout around the 16-row blocks, odd strided
    extents over several images, both residual modes with mish, and a split-K layer of nine K steps"""
    steps = {c[3] * c[5] * c[5] // 32 for c in D.CASES}
    assert {1, 2, 3, 4, 9} <= steps, steps
    m = {c[0] * R.out_hw(c[1], c[2], c[5], c[6])[0] * R.out_hw(c[1], c[2], c[5], c[6])[1] for c in D.CASES}
    assert {15, 16, 17, 33} <= m, m
    assert {15, 16, 17, 33, 255} <= {c[4] for c in D.CASES}
    strided = [c for c in D.CASES if c[5] == 3 and c[6] == 2 and c[0] == 3]
    assert {(c[1], c[2]) for c in strided} == {(7, 5), (9, 11)}
    for k in (1, 3):
        modes = {(c[7], c[8]) for c in D.CASES if c[5] == k and c[8]}
        assert modes == {("mish", 1), ("relu", 2)}, (k, modes)
    n, h, w, cin, cout, k, s = D.SPLITK_CASE[:7]
    assert k * k * cin // 32 == 9 and cin % 32 == 0
    assert D.MERGED_CASE[-1][0] > 0
