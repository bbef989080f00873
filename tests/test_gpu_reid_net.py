"""The appearance network (csrc/reid.cpp ReidNet::forward: 20 convs with BatchNorm folded on the host, 8 residual blocks, the pool +
L2-norm tail) against the float64 network of tests/reid_ref.py, as max abs per embedding entry, at reid_ref's bound: the smallest
error that a dropped x_lo or w_lo term in ANY one of the 20 convs causes, divided by 16 (1.6e-7 on the "unit" weights, 2.4e-7 on the
"wide" ones; test_reid_ref_host.py holds the reference to it on the CPU).  Before, the network was compared with the fp32 oracle at
rtol 1e-3 / atol 1e-5 only, a window that every one of those 40 mutants fits into.  A cosine distance is not used: it moves 10 to 100
times less than the rows do and cannot separate the mutants.

Both profiles run because a BatchNorm folded without its eps is invisible on the "unit" weights (test_reid_ref_host.py).  Math 1 walks
the f16x3 kernels, the H16 activations and the tail's H16 read path; math 0 the fp32 MFMA kernels and the tail's fp32 branch.

Measured (max abs per entry against forward64; the fp32 oracle's own error in brackets), each held to its bound:
    test_embedding_vs_float64 (worst of D = 1, 3, 8)   unit: bound 1.58e-7 [4.0e-8]  math 1 4.6e-8   math 0 6.4e-8
                                                       wide: bound 2.43e-7 [6.6e-8]  math 1 8.2e-8   math 0 1.74e-7
    test_embed_front_end_vs_float64                    unit: bound 1.49e-7 [3.8e-8]  math 1 4.3e-8   math 0 5.4e-8
                                                       wide: bound 2.11e-7 [6.5e-8]  math 1 5.6e-8   math 0 9.5e-8
    test_tuned_choice_reused_at_both_ends              unit: bound 1.58e-7           worst call 5.6e-8, the same row between two calls 6.0e-8
Math 0 on the wide weights sits highest (0.72 bound, all in crop 0).  docs/LAB_NOTEBOOK.md "ReID network" has the table and how the
front end's frame was chosen.
"""
import functools

import numpy as np
import pytest

import reid_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
MATHS = pytest.mark.parametrize("math", [1, 0], ids=["f16x3", "f32"])
PROFILES = pytest.mark.parametrize("profile", R.PROFILES)


def _with_math(mode, fn):
    from yolo_deepsort_amd import _lib
    _lib.init()
    lib = _lib.load()
    prev = lib.yds_get_conv_math()
    _lib.check(lib.yds_set_conv_math(mode))
    try:
        return fn()
    finally:
        lib.yds_set_conv_math(prev)


def _oracle_err(c):
    from oracle import reid as oreid
    return c.err(oreid.reid_forward(c.x, c.sd))


@MATHS
@PROFILES
def test_embedding_vs_float64(math, profile):
    """Extractor.forward on 1, 3 and 8 crops (a near-duplicate pair and a scaled copy among them): one crop leaves the last stages
    with 32 rows, less than any tile; each count tunes its own variants"""
    from yolo_deepsort_amd.deep_sort import Extractor
    c = R.case(profile)

    def run():
        ex = Extractor(c.sd, max_crops=8)
        return {d: ex.forward(c.x[:d]) for d in (1, 3, 8)}
    got = _with_math(math, run)
    errs = {d: c.err(g, slice(0, d)) for d, g in got.items()}
    print("reid embedding, math %d, %s: bound %.3g  oracle %.3g  kernel %s" % (math, profile, c.bound, _oracle_err(c),
                                                                             "  ".join("D=%d %.3g" % de for de in errs.items())))
    for d, g in got.items():
        assert g.dtype == F32 and g.shape == (d, 512) and np.isfinite(g).all()
        assert errs[d] <= c.bound, (math, profile, d, errs[d], c.bound)
    # the pairs stay apart by what the reference says, not by less
    for a, b in ((0, 2), (1, 3)):
        want = c.emb[a] - c.emb[b]
        assert np.abs(want).max() > 100 * c.bound
        assert np.abs(got[8][a].astype(np.float64) - got[8][b] - want).max() <= 2 * c.bound


@MATHS
@PROFILES
def test_embed_front_end_vs_float64(math, profile):
    """Extractor.embed on a 270x480 uint8 frame with three boxes, one clipped by two borders: the fused crop + stem + pool kernel in
    math 1, the crop kernel and the conv + pool kernel in math 0.  The reference is forward64 of the crop tensor, which
    Extractor.preprocess reproduces bit for bit."""
    from yolo_deepsort_amd.deep_sort import Extractor
    c = R.front_case(profile)
    frame = R.front_frame()

    def run():
        ex = Extractor(c.sd, max_crops=4)
        got = ex.embed(frame, R.FRONT_TLWH)
        return got, ex.front_fused(), ex.preprocess(frame, R.FRONT_TLWH)
    got, fused, pre = _with_math(math, run)
    assert np.array_equal(pre, c.x)
    assert fused == (math == 1)
    err = c.err(got)
    print("reid front end, math %d, %s: bound %.3g  oracle %.3g  kernel %.3g" % (math, profile, c.bound, _oracle_err(c), err))
    assert err <= c.bound, (math, profile, err, c.bound)


# crop counts of one Extractor's life: the first call tunes every layer, the second reuses each choice at exactly twice that count -
# where a split-K chosen by rule (conv_splitk_preferred: at most 128 tiles of 64x128) lands on the last factor launch_splitk accepts,
# ceil(512 / 256) = 2: layer2.1 from 16 crops, layer3 from 32, layer4 from 64 - the third at half of it, the last one retunes
SEQUENCES = [(16, 32, 8), (32, 64, 16), (64, 128, 32), (5, 10, 3, 1)]


@functools.lru_cache(maxsize=None)
def _ref128():
    """the float64 rows of 128 crops, once: a row does not depend on the batch it is computed in"""
    c = R.case("unit")
    x = R.crops(128)
    emb = R.forward64(x, c.sd)[0]
    assert np.abs(emb[:R.N_CROPS] - c.emb).max() < 1e-13
    emb.setflags(write=False)
    return x, emb


@pytest.mark.parametrize("seq", SEQUENCES, ids=lambda s: "-".join(map(str, s)))
def test_tuned_choice_reused_at_both_ends(seq):
    """ReidNet::forward reuses a layer's tuned variant for every D with D0 / 2 <= D <= 2 D0.  A fresh Extractor(max_crops=2) per
    sequence, so the buffers grow between the calls as well.  The bound is that of the first 8 of the 128 crops (reid_ref.case): a
    maximum over fewer rows, so never wider than the bound of all of them."""
    from yolo_deepsort_amd.deep_sort import Extractor
    c = R.case("unit")
    x, want = _ref128()

    def run():
        ex = Extractor(c.sd, max_crops=2)
        return [ex.forward(x[:d]) for d in seq]
    got = _with_math(1, run)
    errs = [float(np.abs(g - want[:d]).max()) for d, g in zip(seq, got)]
    drift = []
    for i in range(len(seq)):
        for j in range(i + 1, len(seq)):
            n = min(seq[i], seq[j])
            drift.append(float(np.abs(got[i][:n].astype(np.float64) - got[j][:n]).max()))
    print("reid reuse %s: bound %.3g  kernel %s  between calls %.3g" % (seq, c.bound, "  ".join("%.3g" % e for e in errs), max(drift)))
    for d, g, e in zip(seq, got, errs):
        assert g.shape == (d, 512) and np.isfinite(g).all()
        assert e <= c.bound, (seq, d, e, c.bound)
    assert max(drift) <= 2 * c.bound, (seq, drift, c.bound)
