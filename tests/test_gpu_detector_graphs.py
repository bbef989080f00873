"""The detector's planner (csrc/darknet.cpp) on small random and directed graphs (tests/cfg_graphs.py), layer by layer: every
tensor is read back and held to the oracle's operator applied to the device's own read-back sources, so nothing compounds and a
wiring error (a wrong slice, offset, view, format or fused partner) shows at the layer that makes it."""
import functools
import json
import os

import numpy as np
import pytest

import cfg_graphs as G
import conv_ref
from test_gpu_detector import _close
from yolo_deepsort_amd import cfgs

pytestmark = pytest.mark.gpu
F32 = np.float32
BATCH = 3
GRAPHS = G.fixed_set()
NAMES = list(GRAPHS)
PER_ITEM = 4
GROUPS = [NAMES[k:k + PER_ITEM] for k in range(0, len(NAMES), PER_ITEM)]
GLUE = ("maxpool", "upsample", "route", "shortcut")


@functools.lru_cache(maxsize=None)
def _oracle(name):
    cfg, hw, _ = GRAPHS[name]
    ref, blob, _ = G.make_oracle(cfg, hw)
    x = G.graph_input(hw, BATCH)
    x.setflags(write=False)
    return ref, blob, x


def _net(name, batch_max=BATCH):
    from yolo_deepsort_amd.models import Darknet
    cfg, hw, _ = GRAPHS[name]
    net = Darknet(None, img_size=hw, batch_max=batch_max, cfg_text=cfg)
    net.load_darknet_weights(None, blob=_oracle(name)[1])
    return net


def _fmt_round(v, fmt):
    """what a tensor of storage format `fmt` keeps of the fp32 values v (float64): fp32 itself, the split-fp16 record hi + lo,
    or fp16 of x / 256 (round to nearest)"""
    v = np.asarray(v, np.float64)
    if fmt == 0:
        return v
    if fmt == 1:
        return conv_ref.h16_round(v)
    assert fmt == 2, fmt
    return (v / 256).astype(np.float16).astype(np.float64) * 256


def _read_back(net, layers):
    """layer -> read-back tensor; convolutions fused into their shortcut cannot be read and are returned as a set"""
    from yolo_deepsort_amd._lib import YdsError
    got, fused = {}, set()
    for i, l in enumerate(layers):
        if l["type"] == "yolo":
            continue
        try:
            got[i] = net.layer_output(i, BATCH)
        except YdsError as e:                       # conv fused with the following shortcut
            assert "fused" in str(e) and l["type"] == "convolutional" and layers[i + 1]["type"] == "shortcut", (i, str(e))
            fused.add(i)
    return got, fused


def _check_layers(name, net, ref, x, layers, convs):
    """Glue layers exactly, conv layers (if `convs`) within 1e-3 * max|ref|, each from the device's read-back sources."""
    got, fused = _read_back(net, layers)
    got[-1] = x
    n_glue = n_conv = 0
    for i, l in enumerate(layers):
        t = l["type"]
        what = f"{name} layer {i} {t} format {net.layer_format(i)}"
        if t == "yolo" or i in fused:
            continue
        assert got[i].shape == (BATCH, l["c"], l["h"], l["w"]), what
        if t == "convolutional" or (t == "shortcut" and i - 1 in fused):
            if not convs:
                continue
            if t == "shortcut":                     # the conv + residual launch: conv from its read-back input, then the add
                pre = G.one_step(ref, i - 1, {i - 2: got[i - 2]})
                want = G.one_step(ref, i, {i - 1: pre, l["refs"][1]: got[l["refs"][1]]})
            else:
                want = G.one_step(ref, i, {i - 1: got[i - 1]})
            err, scale = np.abs(got[i].astype(np.float64) - want).max(), np.abs(want).max()
            assert np.isfinite(got[i]).all() and err <= 1e-3 * scale, (what, err, scale)
            n_conv += 1
        else:
            assert t in GLUE
            want = _fmt_round(G.one_step(ref, i, {j: got[j] for j in G.sources(layers, i)}), net.layer_format(i))
            bad = got[i].astype(np.float64) != want
            assert not bad.any(), (what, int(bad.sum()), np.abs(got[i] - want).max())
            n_glue += 1
    return got, n_glue, n_conv


def _decode64(head, anchors, img_hw):
    """YOLOLayer's inference branch in float64 on the fp32 constants both implementations use (scale, anchors / scale)"""
    B, _, H, W = head.shape
    A = len(anchors)
    p = head.astype(np.float64).reshape(B, A, -1, H, W).transpose(0, 1, 3, 4, 2)
    s0, s1 = float(F32(img_hw[0] / H)), float(F32(img_hw[1] / W))
    aw = np.array([float(F32(a[0]) / F32(s0)) for a in anchors]).reshape(1, A, 1, 1)
    ah = np.array([float(F32(a[1]) / F32(s1)) for a in anchors]).reshape(1, A, 1, 1)
    gy, gx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sig = 1.0 / (1.0 + np.exp(-p))
    out = np.empty_like(p)
    out[..., 0] = (sig[..., 0] + gx) * s0
    out[..., 1] = (sig[..., 1] + gy) * s1
    out[..., 2] = np.exp(p[..., 2]) * aw * s0
    out[..., 3] = np.exp(p[..., 3]) * ah * s1
    out[..., 4:] = sig[..., 4:]
    return out.reshape(B, A * H * W, -1)


DECODE_GROUPS = (("centre", slice(0, 2), False), ("size", slice(2, 4), True), ("prob", slice(4, None), False))


def _decode_errors(got, want64, rows=slice(None)):
    """per column group: (worst error, worst error / allowed floor): centres and probabilities absolute, sizes relative"""
    out = {}
    for gname, cols, relative in DECODE_GROUPS:
        w = want64[:, rows, cols]
        e = np.abs(got[:, rows, cols].astype(np.float64) - w)
        ulp = np.spacing(np.abs(w).astype(F32)).astype(np.float64)
        if relative:
            e, ulp = e / np.abs(w), ulp / np.abs(w)
        out[gname] = (e, ulp)
    return out


def _check_decode(name, mode, out, got, layers, ref, hw):
    """The network output against a float64 decode of the READ-BACK head tensors.  The kernel may be at most 4 x the worst error
    of the oracle's fp32 numpy decode of the same tensor against that float64 decode (per column group), with a floor of one
    fp32 ulp of the value: both run the same chain of correctly rounded +, *, / and differ only in their exp."""
    from oracle.darknet import yolo_decode
    off = 0
    for i, l in enumerate(layers):
        if l["type"] != "yolo":
            continue
        p = ref.params[i]
        head = got[i - 1]
        want64 = _decode64(head, p["anchors"], hw)
        n = want64.shape[1]
        dev = np.asarray(out)[:, off:off + n]
        off += n
        assert np.isfinite(want64).all() and np.isfinite(dev).all(), (name, i)
        ora = _decode_errors(yolo_decode(head, p["anchors"], p["classes"], hw), want64)
        cells = l["h"] * l["w"]
        tails = [("all", slice(None))]
        if cells > 8192:                            # the rows only the kernel's grid-stride loop reaches
            late = np.nonzero(np.arange(n) % cells >= 8192)[0]
            assert late.size == 3 * (cells - 8192)
            tails.append(("cells >= 8192", late))
        for label, rows in tails:
            ker = _decode_errors(dev, want64, rows)
            for gname, _, _ in DECODE_GROUPS:
                e_o, (e_k, ulp) = ora[gname][0].max(), ker[gname]
                print("DECODE %-20s math %d head %2d %-13s %-6s oracle %.3e kernel %.3e" % (name, mode, i, label, gname, e_o, e_k.max()))
                assert (e_k <= np.maximum(4 * e_o, ulp)).all(), (name, i, label, gname, e_o, e_k.max())
    assert off == np.asarray(out).shape[1]


def _check_graph(name, mode):
    from yolo_deepsort_amd._lib import YdsError
    cfg, hw, layers = GRAPHS[name]
    ref, _, x = _oracle(name)
    if name == "refused":                           # a 6-channel tensor reaches a max pool: refused by name, never numbers
        with pytest.raises(YdsError, match=r"multiples? of 4"):
            _net(name)(x)
        return
    net = _net(name)
    out = np.asarray(net(x)).copy()                 # construction and forward succeed: no refusals allowed
    assert out.shape[0] == BATCH and np.isfinite(out).all(), name
    fmt = [net.layer_format(i) for i in range(len(layers))]
    assert set(fmt) <= ({0, 1, -1} if mode == 1 else {0, -1}), (name, fmt)
    got, n_glue, n_conv = _check_layers(name, net, ref, x, layers, convs=True)
    _check_decode(name, mode, out, got, layers, ref, hw)
    for b in range(BATCH):                          # image b of the batch == the batch-of-one run of that image
        _close(out[b:b + 1], np.asarray(net(x[b:b + 1])), 1e-4, 1e-4, f"{name} image {b}")
    if mode != 1:
        return
    net.half()
    half = np.asarray(net(x))
    assert np.isfinite(half).all(), name            # (the default mode's output is finite everywhere)
    fmt_half = [net.layer_format(i) for i in range(len(layers))]
    assert all(h == f or (f == 1 and h == 2) for f, h in zip(fmt, fmt_half)), (name, fmt, fmt_half)
    _check_layers(name, net, ref, x, layers, convs=False)
    net.float()
    assert [net.layer_format(i) for i in range(len(layers))] == fmt
    assert np.array_equal(np.asarray(net(x)), out), name


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("group", range(len(GROUPS)), ids=lambda g: "+".join(GROUPS[g]))
def test_graphs_layer_by_layer(group, mode):
    """Every graph of the fixed set, batch 3, both conv maths; in math 1 also half mode and back (the bars are in the helpers).
    Measured decode errors against the float64 decode of the read-back head, worst over the 42 heads of the set, oracle's fp32
    numpy decode | kernel (allowed: 4 x the oracle's, floor one fp32 ulp): centres 3.87e-6 | 3.87e-6 px absolute, sizes
    2.23e-7 | 1.28e-7 relative, probabilities 9.07e-8 | 8.28e-8 absolute; worst kernel / oracle of a single head 1.16.  On the
    rows of `big_head` whose cell index is 8192 or above: 3.87e-6 | 3.85e-6, 2.15e-7 | 1.17e-7, 8.23e-8 | 6.96e-8.
    Before the planner tied an upsample to its source, up_h16_to_f32, up_f32_to_h16 and seeds 0, 1, 8, 12, 14, 22 were refused in
    math 1 ("upsample: source and destination formats differ"); linear_shortcut in both maths while a shortcut was fused into
    a linear conv ("conv: unsupported activation/residual combination (0, 1)")."""
    from yolo_deepsort_amd import _lib
    lib = _lib.load()
    default = lib.yds_get_conv_math()
    try:
        lib.yds_set_conv_math(mode)
        for name in GROUPS[group]:
            _check_graph(name, mode)
    finally:
        lib.yds_set_conv_math(default)


@pytest.mark.parametrize("name", ["up_h16_to_f32", "up_f32_to_h16", "dup_route", "route_of_routes", "shortcut_into_slice", "seed0", "seed12"])
def test_lane_split_offsets_into_slices(monkeypatch, name):
    """Batch 9 as two lanes (5 + 4 images, run_graph): the second lane's views start 5 images into redirected slices, grouped
    views and copy destinations.  Same tolerances as test_lane_split_matches_single_stream."""
    _, hw, _ = GRAPHS[name]
    x = G.graph_input(hw, 9, seed=8)
    net = _net(name, batch_max=9)
    monkeypatch.setenv("YDS_DET_LANES", "2")
    two = np.asarray(net(x)).copy()
    monkeypatch.setenv("YDS_DET_LANES", "1")
    one = np.asarray(net(x)).copy()
    _close(two, one, 1e-4, 1e-4, f"{name} lanes")
    for b in (0, 4, 5, 8):
        _close(two[b:b + 1], np.asarray(net(x[b:b + 1])), 1e-4, 1e-4, f"{name} image {b}")


def test_stock_networks_keep_their_tensor_formats():
    """The planner's format ties must not move the stock networks: their layer_format lists, default and half mode, are the ones
    recorded from the library before upsamples were tied to their sources (tests/golden/stock_layer_formats.json)."""
    from yolo_deepsort_amd.models import Darknet
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stock_layer_formats.json")) as f:
        want = json.load(f)
    assert set(want) == set(cfgs.CFG_BUILDERS)
    for name in cfgs.CFG_BUILDERS:
        net = Darknet(None, img_size=(96, 96), batch_max=1, cfg_text=cfgs.cfg_text(name, 96, 96))
        n = len(net.module_defs)
        assert [net.layer_format(i) for i in range(n)] == want[name]["default"], name
        net.half()
        assert [net.layer_format(i) for i in range(n)] == want[name]["half"], name
        assert 1 in want[name]["default"] and 2 in want[name]["half"]
