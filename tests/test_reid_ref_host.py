"""The ReID network tests' bound, checked on the CPU: for each profile that tests/test_gpu_reid_net.py runs, on that test's own inputs
(reid_ref.case), the float64 reference alone meets the conditions that make mut / 16 a usable bound for the whole network.  A seed or
an input scale that breaks one of them fails here, not on the GPU.

Why the GPU test runs both profiles: on the "unit" weights (running_var in 0.8 .. 1.25) a BatchNorm folded without its eps moves the
embedding by 0.4 .. 2.8 bound - no test at this bound or any wider one can see a wrong fold there.  On the "wide" weights (running_var
down to 1e-3) the same defect in ANY of the 20 layers moves it by 42 .. 1656 bound."""
import numpy as np
import pytest

import reid_ref as R


@pytest.mark.parametrize("front", [False, True], ids=["crops", "front"])
@pytest.mark.parametrize("profile", R.PROFILES)
def test_reference_separates_from_the_mutants(profile, front):
    """the random crops of test_embedding_vs_float64, and the three image crops of test_embed_front_end_vs_float64"""
    from oracle import reid as oreid
    c = R.front_case(profile) if front else R.case(profile)
    weakest = min(c.mut, key=c.mut.get)
    ora = c.err(oreid.reid_forward(c.x, c.sd))
    emu = c.err(R.emulated(c.x, c.sd))
    f32 = c.err(R.folded_fp32(c.x, c.sd))
    print("%s %s: bound %.3g = %s %.3g / 16 | fp32 oracle %.3g (bound / %.1f)  folded fp32 network %.3g (bound / %.1f)  three-term emulation "
          "%.3g (bound / %.1f)" % (profile, "front" if front else "crops", c.bound, weakest, c.mut[weakest], ora, c.bound / ora, f32, c.bound / f32,
                                   emu, c.bound / emu))
    assert len(c.mut) == 40 and c.bound > 0 and np.isfinite(c.bound)
    np.testing.assert_allclose(np.linalg.norm(c.emb, axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.abs(c.emb).max() < 0.5 and (c.stages[-1] > 0).mean() > 0.2      # a live network: no collapsed embedding
    assert ora <= c.bound / 2, (profile, ora, c.bound)
    # fp32 arithmetic on the network as the device holds it (BatchNorm folded into fp32 weights), in another order than the oracle's:
    # where THAT misses half the bound, the inputs make the bound a yardstick of summation orders, not of kernels
    assert f32 <= c.bound / 2, (profile, f32, c.bound)
    assert emu <= c.bound / 4, (profile, emu, c.bound)


@pytest.mark.parametrize("profile", R.PROFILES)
def test_structural_mutants_lie_far_outside_the_bound(profile):
    c = R.case(profile)
    errs = c.errors(R.STRUCT_MUTANTS)
    print(profile, {m: "%.2g" % e for m, e in errs.items()})
    assert len(errs) == 8 + 3 + 1
    for m, e in errs.items():
        assert e > 16 * c.bound, (profile, m, e, c.bound)


def test_bn_eps_shows_on_the_wide_profile_only():
    wide, unit = R.case("wide"), R.case("unit")
    ew, eu = wide.errors(R.EPS_MUTANTS), unit.errors(R.EPS_MUTANTS)
    print("wide / bound", {m[1]: "%.0f" % (e / wide.bound) for m, e in ew.items()})
    print("unit / bound", {m[1]: "%.1f" % (e / unit.bound) for m, e in eu.items()})
    for m, e in ew.items():
        assert e > 16 * wide.bound, (m, e, wide.bound)
    assert max(eu.values()) < 16 * unit.bound


def test_stage_reuse_and_the_inputs_pairs():
    """a mutant resumed from the reference's stages equals the same mutant computed from the input; rows do not depend on the batch;
    the near-duplicate and the scaled pair are what crops() says"""
    c = R.case("unit")
    x = c.x[:2]
    ref = R.forward64(x, c.sd)
    assert np.abs(ref[0] - c.emb[:2]).max() < 1e-13                   # (another batch may add in another order: float64 roundings)
    assert len(ref[1]) == 9 and ref[1][0].shape == (2, 64, 64, 32) and ref[1][-1].shape == (2, 512, 8, 4)
    for m in (("xlo", 9), ("wlo", 17), ("res_after", 3), ("no_down", 4), ("eps", 12)):
        a, b = R.forward64(x, c.sd, m, ref[1])[0], R.forward64(x, c.sd, m)[0]
        assert np.abs(a - b).max() < 1e-13, m
        assert np.abs(a - ref[0]).max() > 1e-9, m
    # a bound taken on some of the crops is never wider than the bound of all of them (test_tuned_choice_reused_at_both_ends)
    assert 0 < R.bound(x, c.sd, ref) <= c.bound * (1 + 1e-6)
    big = R.crops(11)
    assert np.array_equal(big[:8], c.x) and big.shape[0] == 11
    assert 0 < np.abs(c.x[2] - c.x[0]).max() < 0.3 and np.array_equal(c.x[3], np.float32(0.9) * c.x[1])
