"""The fused ReID front end (csrc/reid_stem.hip: frames + crop list -> pooled stem tensor in one kernel) against the pair of
kernels it replaces (crop kernel + stem conv/pool, selected with YDS_REID_FRONT_UNFUSED) - bit for bit - and against the oracle.

Both passes of a test run on ONE Extractor with the same crop count, so the per-layer tile choices the extractor caches are the
same for both and any difference comes from the front end."""
import os

import numpy as np
import pytest

from yolo_deepsort_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
RTOL = 1e-3
SWITCH = "YDS_REID_FRONT_UNFUSED"


def _both(ex, call):
    """call() with the fused front end, then with the fallback pair; the extractor says which front end each pass began with"""
    for k in (SWITCH, "YDS_REID_UNFUSED", "YDS_POOL_VALU"):       # any of them selects the fallback
        assert k not in os.environ, k
    fused = call()
    assert ex.front_fused()
    os.environ[SWITCH] = "1"
    try:
        unfused = call()
        assert not ex.front_fused()
    finally:
        del os.environ[SWITCH]
    return fused, unfused


def _check(ex, sd, frame, tlwh, oracle_rows=None):
    from oracle import reid as oreid
    fused, unfused = _both(ex, lambda: ex.embed(frame, tlwh))
    assert fused.shape == (len(tlwh), 512)
    assert np.array_equal(fused, unfused)
    rows = np.arange(len(tlwh)) if oracle_rows is None else np.asarray(oracle_rows)
    want = oreid.reid_forward(oreid.preprocess_crops(frame, tlwh[rows]), sd)
    np.testing.assert_allclose(fused[rows], want, rtol=RTOL, atol=1e-5)
    np.testing.assert_allclose(unfused[rows], want, rtol=RTOL, atol=1e-5)


def _extractor(max_crops):
    from yolo_deepsort_amd.deep_sort import Extractor
    sd = synth.reid_state_dict(0)
    return Extractor(sd, max_crops=max_crops), sd


# the boxes of test_reid_crop_resize_paths_bit_exact_and_growth: generic up- and down-scaling, the exact-2x 128x256 crop, the 64x128
# copy, crops that truncate to 1 pixel of width and 2 of height, clipped boxes
NINE = np.array([[100, 50, 128, 256], [300, 200, 64, 128], [10, 10, 1.5, 300], [500, 100, 37, 91], [-20, -30, 90, 200],
                 [900, 400, 200, 300], [400, 300, 300, 2.2], [7.9, 8.9, 63.2, 127.2], [600, 20, 20, 40]], F32)


def _frame(seed, h=540, w=960):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def test_every_resize_branch_bit_exact_and_growth():
    ex, sd = _extractor(4)                               # 9 crops: the buffers grow during the first call
    _check(ex, sd, _frame(12), NINE)


def _boxes(n, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(0, 900, n), rng.uniform(0, 400, n), rng.uniform(8, 120, n), rng.uniform(16, 250, n)], 1).astype(F32)


@pytest.mark.parametrize("d", [1, 3, "grid + 1"])
def test_crop_counts_at_the_seams(d):
    """A workgroup of the fused kernel takes one quarter of a crop (16 pooled rows), so no workgroup or wave is shared between
    crops: the seam of the decomposition is its persistent grid, 3 workgroups per CU.  yds_reid_front_grid_crops() crops fill the
    grid exactly (192 on 256 CUs); with one more, four workgroups take a second quarter - of the last crop - through the
    grid-stride loop and the box prefetch, while the others take one.  The host oracle was measured at 1.8 s for 16 crops, which
    is 20 s for 193, so at that count it checks the first two crops and the last two (the last is the one the second trips
    compute); fused against fallback covers all of them."""
    from yolo_deepsort_amd import _lib
    ex, sd = _extractor(256)
    if d == "grid + 1":
        d = _lib.load().yds_reid_front_grid_crops() + 1
        assert d > 1
    tlwh = _boxes(d, 100 + d)
    _check(ex, sd, _frame(13), tlwh, None if d <= 3 else [0, 1, d - 2, d - 1])


def test_bgr_and_frame_table():
    frames = [_frame(14, 360, 640), _frame(15, 540, 960)]
    # (frame, box): inside, at each frame's four borders (clipped), and the copy / exact-2x routes in the smaller frame
    tlwh = np.array([[50, 40, 60, 130], [-5, -8, 70, 150], [600, 300, 80, 100], [200, 100, 64, 128], [300, 60, 128, 256],
                     [100, 80, 45, 200], [-10, 500, 90, 80], [900, -20, 100, 180], [880, 470, 120, 120], [640, 360, 150, 170]], F32)
    frame_of = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1, 1], np.int32)
    ex, _ = _extractor(16)
    rgb, rgb_unfused = _both(ex, lambda: ex.embed_mixed(frames, tlwh, frame_of))
    assert np.array_equal(rgb, rgb_unfused)
    bgr, bgr_unfused = _both(ex, lambda: ex.embed_mixed(frames, tlwh, frame_of, bgr=True))
    assert np.array_equal(bgr, bgr_unfused)
    assert not np.array_equal(bgr, rgb)
    reversed_frames = [np.ascontiguousarray(f[:, :, ::-1]) for f in frames]
    assert np.array_equal(bgr, ex.embed_mixed(reversed_frames, tlwh, frame_of))


def test_fallback_selection():
    from oracle import reid as oreid
    from yolo_deepsort_amd import _lib
    lib = _lib.load()
    ex, sd = _extractor(16)
    frame = _frame(12)
    pre_want = oreid.preprocess_crops(frame, NINE)
    want = oreid.reid_forward(pre_want, sd)
    np.testing.assert_allclose(ex.embed(frame, NINE), want, rtol=RTOL, atol=1e-5)       # fused: the crop tensor does not exist yet
    assert ex.front_fused()
    assert np.array_equal(ex.preprocess(frame, NINE), pre_want)
    prev = lib.yds_get_conv_math()
    _lib.check(lib.yds_set_conv_math(0))                 # exact fp32: the fused kernel does not apply
    try:
        np.testing.assert_allclose(ex.embed(frame, NINE), want, rtol=RTOL, atol=1e-5)
        assert not ex.front_fused()
        assert np.array_equal(ex.preprocess(frame, NINE), pre_want)
    finally:
        lib.yds_set_conv_math(prev)
