"""The detector's launch plan: which convolution launches a pass costs, and that the plan follows every state change."""
import os

import numpy as np
import pytest

from yolo_deepsort_amd import cfgs, synth
from test_gpu_detector import _csp_cfg, _close

pytestmark = pytest.mark.gpu
F32 = np.float32

# name -> (cfg text, (h, w), batch)
NETS = {
    "yolov3": (lambda: cfgs.cfg_text("yolov3", 160, 96), (160, 96), 2),
    "yolov4": (lambda: cfgs.cfg_text("yolov4", 160, 96), (160, 96), 2),
    "csp64mish": (lambda: _csp_cfg(64, "mish"), (64, 64), 3),
    "csp32leaky": (lambda: _csp_cfg(32, "leaky"), (64, 64), 3),
    "csp24mish": (lambda: _csp_cfg(24, "mish"), (64, 64), 3),
    "yolov4-tiny": (lambda: cfgs.cfg_text("yolov4-tiny", 96, 96), (96, 96), 2),
}

# Conv launches of one pass per tile variant under YDS_NO_AUTOTUNE (the built-in variant choice), recorded on the parent of the
# commit that introduced the step list.  A fused stem is booked under direct_rgb, a fused first block under win_256x128.
# (name, half) -> (total, {variant: launches}); the account of each total is
#     convolutions in the cfg - those computed inside a fused stem / first-block launch - CSP partners.
IGEMM, DMA, WIN, RGB = "conv_igemm_f16x3<64,64>", "conv_igemm_f16x3_dma<128,128,2x2,2>", "conv3x3_f16x3_win<256,128,4x2>", "conv3x3_rgb_direct"
EXPECTED = {
    # 75 convolutions - layer 0 (inside the fused stem) - the 1x1 of the first residual block (inside the fused block)
    ("yolov3", False): (73, {IGEMM: 71, WIN: 1, RGB: 1}),
    ("yolov3", True): (73, {DMA: 71, WIN: 1, RGB: 1}),
    # 110 convolutions - layer 0 - the 1x1 of the first residual block - 5 CSP partners
    ("yolov4", False): (103, {IGEMM: 101, WIN: 1, RGB: 1}),
    ("yolov4", True): (103, {DMA: 101, WIN: 1, RGB: 1}),
    # 9 convolutions - 1 CSP partner (layer 1 has 128 filters: no fused stem; no 64 -> 32 -> 64 block)
    ("csp64mish", False): (8, {IGEMM: 8}),
    ("csp64mish", True): (8, {IGEMM: 3, DMA: 5}),
    # 9 convolutions - layer 0 (fused stem: 32 then 64 filters) - 1 CSP partner
    ("csp32leaky", False): (7, {IGEMM: 6, RGB: 1}),
    ("csp32leaky", True): (7, {IGEMM: 4, DMA: 2, RGB: 1}),
    # 9 convolutions - 1 CSP partner (fp32 tensors: 24 channels)
    ("csp24mish", False): (8, {IGEMM: 8}),
    ("csp24mish", True): (8, {IGEMM: 8}),
    # 21 convolutions, nothing fused (the stem has stride 2), no CSP pair of 1x1 convolutions
    ("yolov4-tiny", False): (21, {IGEMM: 21}),
    ("yolov4-tiny", True): (21, {IGEMM: 5, DMA: 16}),
}
# merged CSP pairs of the yolov4-family nets: YDS_NO_CSP_MERGE at creation adds exactly one launch per pair
MERGED_PAIRS = {"yolov4": 5, "csp64mish": 1, "csp32leaky": 1, "csp24mish": 1, "yolov4-tiny": 0}


def _make(name, seed=2, batch_max=None, no_merge=False):
    from yolo_deepsort_amd.models import Darknet
    cfg, size, batch = NETS[name]
    cfg = cfg()
    if no_merge:
        os.environ["YDS_NO_CSP_MERGE"] = "1"
    try:
        net = Darknet(None, img_size=size, batch_max=batch_max or batch, cfg_text=cfg)
    finally:
        os.environ.pop("YDS_NO_CSP_MERGE", None)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, seed, -1.0))
    return net


def _census(name, half, no_merge=False):
    from yolo_deepsort_amd import pipeline
    _, size, batch = NETS[name]
    net = _make(name, no_merge=no_merge)
    if half:
        net.half()
    x = np.random.RandomState(4).uniform(0, 1, (batch, 3) + size).astype(F32)
    net(x)                                                   # (first pass: the per-layer variant choice is made here)
    pipeline.conv_timing(net, 1)
    net(x)
    return {r["name"]: int(r["launches"]) for r in pipeline.conv_timing(net, 2) if r["launches"]}


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", list(NETS))
def test_launch_census(monkeypatch, name, half):
    """The test that fails when a fusion quietly stops engaging: results would stay right, only the launch count moves."""
    monkeypatch.setenv("YDS_NO_AUTOTUNE", "1")
    got = _census(name, half)
    total, per_variant = EXPECTED[name, half]
    print(name, "half" if half else "default", sum(got.values()), got)
    assert got == per_variant
    assert sum(got.values()) == total
    if name in MERGED_PAIRS:
        unmerged = _census(name, half, no_merge=True)
        print(name, "unmerged", sum(unmerged.values()), unmerged)
        assert sum(unmerged.values()) == total + MERGED_PAIRS[name]


def test_replanning_follows_batch_half_and_weights(monkeypatch):
    """One long-lived yolov4 walked through batch growth, half mode on / off, reloads and a cut-off load: after every step its output
    equals, bit for bit, that of a net created straight into that state."""
    monkeypatch.setenv("YDS_NO_AUTOTUNE", "1")
    from oracle.darknet import DarknetOracle
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.models import Darknet
    size = (96, 64)
    cfg = cfgs.cfg_text("yolov4", size[0], size[1])
    blobs = {s: synth.darknet_weights_blob(cfg, s, -1.0) for s in (2, 7)}
    x = np.random.RandomState(9).uniform(0, 1, (3, 3) + size).astype(F32)
    wants = {}                                               # (batch, half, seed) -> output of the net created for that state

    def load(net, seed, cut=-1):
        if cut < 0:
            net.load_darknet_weights(None, blob=blobs[seed])
        else:                                                # (the wrapper derives its cutoff from the file name: go below it)
            _lib.check(_lib.load().yds_darknet_load_weights(net._h, blobs[seed], len(blobs[seed]), cut))

    def fresh(batch, half, seed, cut=-1):
        net = Darknet(None, img_size=size, batch_max=batch, cfg_text=cfg)
        load(net, seed, cut)
        if half:
            net.half()
        return net

    def same(net, batch, half, seed, what):
        got = np.asarray(net(x[:batch]))
        if (batch, half, seed) not in wants:
            wants[batch, half, seed] = np.asarray(fresh(batch, half, seed)(x[:batch])).copy()
        assert np.array_equal(got, wants[batch, half, seed]), what

    net = fresh(1, False, 2)
    same(net, 1, False, 2, "1: batch 1")
    net.set_batch_max(3)
    same(net, 3, False, 2, "2: batch 3 after set_batch_max")
    net.half()
    same(net, 3, True, 2, "3: half mode on")
    net.float()
    same(net, 1, False, 2, "4: half mode off, batch 1")
    load(net, 7)
    same(net, 1, False, 7, "5: other weights")
    load(net, 7, len(net.module_defs) - 10)                  # short of the last layers: they have no weights any more
    with pytest.raises(RuntimeError, match="has no weights"):
        net(x[:1])
    load(net, 2)
    same(net, 1, False, 2, "7: full reload")
    # the layers the fused stem and first block never write are still produced on demand
    ref = DarknetOracle(cfg, size, is_text=True)
    ref.load_weights_array(np.frombuffer(blobs[2], dtype=F32, offset=20))
    ref.forward(x[:1], keep_layers=True)
    first_shortcut = next(i for i, d in enumerate(ref.module_defs) if d["type"] == "shortcut")
    for i in (0, first_shortcut - 2):                        # the stem's first conv; the 1x1 of the first residual block
        assert ref.module_defs[i]["type"] == "convolutional"
        _close(net.layer_output(i, 1), ref.layer_outputs[i], 1e-3, 1e-3, f"layer {i}")
