"""A window setting per stream in one multi-stream step (csrc/pipeline.cpp yds_pipeline_set_stream_windows): every camera is cut by
its own ImageDetector(win_size, overlap), a step that holds a windowed frame runs as one slotted pass - a network slot per window and
per plain frame (csrc/layers.hip slot_resize_kernel / slot_boxes_kernel), one ragged NMS launch over all frames (csrc/nms.hip
launch with a frame table).  The yardstick per stream is the stream run alone at its own size and setting: the frame-by-frame path
(VideoDetector.process with an ImageDetector(win_size=...)), or the single-stream Pipeline where the same device arithmetic is
compared exactly.  Row criterion as tests/test_gpu_window_pipeline.py: track ids and classes bit exact, None frames agree, boxes
within one pixel.  yolov3-tiny at 416, overlap 0.15 throughout.

Camera set: A 480 x 640 (416, 416) 4 slots; B 360 x 480 (416, 416) 2 slots; C 300 x 400 (416, 416) plain, both sides under the window;
D 480 x 640 no setting; E 480 x 640 (320, 240) 4 slots."""
import atexit
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

from conftest import golden
from yolo_deepsort_amd import cfgs, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
WIN, WIN_E, OVERLAP, SIZE = (416, 416), (320, 240), 0.15, 416
EMPTY = np.zeros((0, 9), F32)
BOXES = 2535                                           # yolov3-tiny at 416: (13 * 13 + 26 * 26) * 3
# camera -> (frame h, w), window setting, the windows of img_detect.py:101-121 as (x, y, tile_h, tile_w); None: the plain branch
CAMERAS = {
    "A": ((480, 640), WIN, [(0, 0, 478, 478), (0, 416, 64, 478), (416, 0, 478, 224), (416, 416, 64, 224)]),
    "B": ((360, 480), WIN, [(0, 0, 360, 478), (416, 0, 360, 64)]),
    "C": ((300, 400), WIN, None),
    "D": ((480, 640), None, None),
    "E": ((480, 640), WIN_E, [(0, 0, 276, 368), (0, 240, 240, 368), (320, 0, 276, 320), (320, 240, 240, 320)]),
}


def _check_camera_set():
    """The window lists above against the oracle's restatement of the reference's loop (CPU only)."""
    from oracle import tiled
    for name, ((h, w), win, want) in CAMERAS.items():
        plain = win is None or (w < win[0] and h < win[1])                     # img_detect.py:68
        assert (want is None) == plain, name
        if want is not None:
            assert tiled.windows(h, w, win, OVERLAP) == want, name
    assert sum(len(c[2]) if c[2] else 1 for c in CAMERAS.values()) == 12


# ------------------------------------------------------------------------------------------------ helpers
def _cfg():
    return cfgs.cfg_text("yolov3-tiny", SIZE, SIZE)


def _net(blob, batch_max):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    net = Darknet(None, img_size=(SIZE, SIZE), batch_max=batch_max, cfg_text=_cfg())
    net.load_darknet_weights(None, blob=blob)
    return net


_shared = {}


def _random_net(batch_max):
    """One detector with random weights (objectness bias -1.3) per batch_max for the whole module."""
    key = ("net", batch_max)
    if key not in _shared:
        _shared[key] = _net(synth.darknet_weights_blob(_cfg(), 0, -1.3), batch_max)
    return _shared[key]


def _extractor():
    from yolo_deepsort_amd.deep_sort import DeepSort
    if "ex" not in _shared:
        _shared["ex"] = DeepSort(synth.reid_state_dict(0), use_cuda=True, **DS).extractor
    return _shared["ex"]


def _deepsort():
    from yolo_deepsort_amd.deep_sort import DeepSort
    return DeepSort(_extractor(), use_cuda=True, **DS)


def _names():
    if "names" not in _shared:
        with tempfile.NamedTemporaryFile("w", suffix=".names", delete=False) as f:
            f.write(cfgs.coco_names_text())
        _shared["names"] = f.name
        atexit.register(os.unlink, f.name)
    return _shared["names"]


def _video_detector(net, tracker, class_mask=None, win_size=None, thres=0.5, **kw):
    from yolo_deepsort_amd.detect import VideoDetector
    return VideoDetector(net, _names(), thres=thres, nms_thres=0.4, tracker=tracker, class_mask=class_mask, win_size=win_size,
                         overlap=OVERLAP, **kw)


def _rows(o):
    return None if o is None else np.array(o, np.int32).reshape(-1, 6)


def _frame_by_frame(net, frames, inj, win_size, class_mask=None):
    """The yardstick of one stream: every frame through ImageDetector(win_size).detect + DeepSort.update (VideoDetector.process), one
    frame at a time; inj[t] = one injection table per network slot of frame t (its windows, or the whole frame)."""
    vd = _video_detector(net, _deepsort(), class_mask, win_size=win_size, batch_frames=1)
    out = []
    for t, frame in enumerate(frames):
        for slot in range(net.batch_max):
            net.set_injection(slot, inj[t][slot] if slot < len(inj[t]) else EMPTY)
        out.append(_rows(vd.process(frame)))
    return out


def _compare(got, want, exact=False):
    """Row criterion; returns the number of rows compared."""
    assert len(got) == len(want)
    rows = 0
    for t, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, t
            continue
        assert g is not None and g.shape == w.shape, (t, g, w)
        assert np.array_equal(g[:, 4:], w[:, 4:]), (t, g, w)              # track ids and classes: bit exact
        if exact:
            assert np.array_equal(g, w), (t, g, w)
        assert np.abs(g[:, :4] - w[:, :4]).max(initial=0) <= 1, (t, g, w)
        rows += len(w)
    return rows


def _slot_tables(tlwh, cls, hw, windows, heads):
    """Injection tables of one frame, one per network slot.  A windowed frame: a person goes into every window that holds its whole
    box, in window coordinates (the window is what the network sees).  A plain frame: one table in frame coordinates."""
    tables = []
    for x0, y0, th, tw in (windows or [(0, 0) + tuple(hw)]):
        inside = [i for i, (x, y, w, h) in enumerate(tlwh) if x >= x0 and y >= y0 and x + w <= x0 + tw and y + h <= y0 + th]
        if not inside:
            tables.append(EMPTY)
            continue
        local = np.array([[tlwh[i][0] - x0, tlwh[i][1] - y0, tlwh[i][2], tlwh[i][3]] for i in inside], F32)
        rows = synth.head_injection(local, (th, tw), (SIZE, SIZE), heads)
        rows[:, 8] = [cls[i] for i in inside]
        tables.append(rows)
    return tables


def _scene_frame(seed, tlwh, hw):
    """A frame with a texture patch per person on a blocky background (the ReID crops must differ between persons)."""
    h, w = hw
    rng = np.random.RandomState(100 + seed)
    img = np.repeat(np.repeat(rng.randint(0, 256, ((h + 7) // 8, (w + 7) // 8, 3)), 8, 0), 8, 1)[:h, :w].astype(np.uint8)
    for x, y, bw, bh in tlwh:
        patch = np.random.RandomState(7 + int(bw) * 31 + int(bh)).randint(0, 256, (8, 4, 3)).astype(np.uint8)
        yy = (np.arange(int(bh)) * 8 // int(bh)).clip(0, 7)
        xx = (np.arange(int(bw)) * 4 // int(bw)).clip(0, 3)
        img[int(y):int(y) + int(bh), int(x):int(x) + int(bw)] = patch[yy][:, xx]
    return np.ascontiguousarray(img)


# persons (tlwh, class) of frame t of each scripted stream.  A: the scene of tests/test_gpu_window_pipeline.py - person 2 walks inside
# the 62-pixel overlap of the two window columns (seen by windows 0 and 2), person 4 inside the overlap of the rows.
PERSONS = {
    "A": lambda t: [((50 + 3 * t, 100 + 2 * t, 50, 120), 0), ((300 - 2 * t, 250 + t, 60, 150), 2), ((425 + t, 150 + 2 * t, 35, 100), 0),
                    ((520 + 3 * t, 60 + t, 60, 140), 2), ((100 + 2 * t, 424, 30, 45), 0)],
    "C": lambda t: [((30 + 2 * t, 40 + t, 40, 100), 0), ((260 - 2 * t, 120, 50, 110), 2)],
    "D": lambda t: [((60 + 2 * t, 80 + t, 55, 130), 0), ((330 - 3 * t, 200, 60, 150), 2), ((500 + t, 300 - 2 * t, 45, 110), 0)],
}


def _scripted_stream(cam, n, heads, only=None):
    """n frames of camera `cam`: (frames, injection tables per slot, persons per frame); only[t]: the persons of frame t, by index."""
    hw, _, windows = CAMERAS[cam]
    frames, inj, count = [], [], []
    for t in range(n):
        persons = PERSONS[cam](t)
        if only and t in only:
            persons = [persons[i] for i in only[t]]
        tlwh, cls = [p for p, _ in persons], [c for _, c in persons]
        frames.append(_scene_frame(t + 17 * ord(cam), tlwh, hw))
        inj.append(_slot_tables(tlwh, cls, hw, windows, heads))
        count.append(len(tlwh))
    return frames, inj, count


def _pack(frames):
    from yolo_deepsort_amd.pipeline import pack_frames
    return pack_frames(frames)


def _random_frame(cam, seed):
    return np.random.RandomState(seed).randint(0, 256, CAMERAS[cam][0] + (3,)).astype(np.uint8)


def _alone(cam, frame, n, win="camera"):
    """What a stream of n <= 6 times `frame` gives alone through the single-stream Pipeline at the camera's setting (computed once)."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    win = CAMERAS[cam][1] if win == "camera" else win
    key = ("alone", cam, win, frame.tobytes())
    if key not in _shared:
        pipe = pl.Pipeline(_random_net(5), _deepsort(), 0.5, 0.4, win_size=win, overlap=OVERLAP)
        dev = _lib.DeviceBuffer.from_array(frame[None])
        _shared[key] = [pipe.step(dev.ptr, frame.shape[0], frame.shape[1], 1)[0] for _ in range(6)]
    assert n <= 6
    return _shared[key][:n]


def _slot_pred(pipe, attrs):
    from yolo_deepsort_amd import _lib as L
    n = C.c_size_t(0)
    L.check(L.load().yds_pipeline_slot_pred(pipe._h, None, 0, C.byref(n)))
    out = np.zeros((n.value, attrs), F32)
    L.check(L.load().yds_pipeline_slot_pred(pipe._h, L.ptr(out), n.value, C.byref(n)))
    return out


# ------------------------------------------------------------------------------------------------ 1. front end, bit exact
def test_slotted_front_end_bit_exact():
    """One slotted pass over A, a 333 x 501 frame (an odd number of bytes: every frame behind it starts at an odd offset), B, C, D, E
    in a mixed layout, 13 slots in one forward.  Every network-input slot equals the oracle's cv2-exact resize of its window or
    its whole frame; every row of the prediction block equals img_detect.py:132-138 restated in fp32 on the network's raw rows for a
    window slot - corner form, resize_boxes to the window, shift by its origin - and the raw centre-form row for a plain slot."""
    from oracle.resize import resize_bilinear_u8
    from yolo_deepsort_amd import _lib, pipeline as pl
    _check_camera_set()
    net = _random_net(13)
    cams = ["A", None, "B", "C", "D", "E"]
    rng = np.random.RandomState(11)
    frames = [rng.randint(0, 256, (CAMERAS[c][0] if c else (333, 501)) + (3,)).astype(np.uint8) for c in cams]
    block, off, hw = _pack(frames)
    assert (333 * 501 * 3) % 2 and all(int(o) % 2 for o in off[2:])
    base = _deepsort()
    pipe = pl.MultiStreamPipeline(net, [base.clone() for _ in cams], 0.5, 0.4,
                                  stream_win_sizes=[CAMERAS[c][1] if c else None for c in cams], overlap=OVERLAP)
    dev = _lib.DeviceBuffer.from_array(block)
    assert len(pipe.step_mixed(dev.ptr, off, hw, list(range(len(cams))), block.nbytes)) == len(cams)
    slots = []                                                             # (frame, window or None)
    for f, c in enumerate(cams):
        windows = CAMERAS[c][2] if c else None
        slots += [(f, win) for win in windows] if windows else [(f, None)]
    assert len(slots) == 13
    got_in = net.get_input(13)
    want_in = np.stack([resize_bilinear_u8(frames[f] if win is None else frames[f][win[1]:win[1] + win[2], win[0]:win[0] + win[3]],
                                           (SIZE, SIZE)).astype(F32).transpose(2, 0, 1) / F32(255.) for f, win in slots], 0)
    for n, (f, win) in enumerate(slots):
        assert np.array_equal(got_in[n], want_in[n]), (n, f, win)
    got = _slot_pred(pipe, net.num_attrs).reshape(13, BOXES, net.num_attrs)
    raw = net.forward(want_in)                                             # the same 13 images through the same detector
    assert raw.shape == got.shape
    for n, (f, win) in enumerate(slots):
        want = raw[n].copy()
        if win is not None:
            x0, y0, th, tw = win
            half = raw[n][:, 2:4] / F32(2)
            corner = np.concatenate([raw[n][:, :2] - half, raw[n][:, :2] + half], 1)
            scale = np.array([F32(tw / SIZE), F32(th / SIZE)] * 2, F32)    # resize_boxes: python-double ratio, fp32 multiply
            want[:, :4] = corner * scale + np.array([x0, y0, x0, y0], F32)
        assert want.dtype == F32 and np.array_equal(got[n], want), (n, f, win)


# ------------------------------------------------------------------------------------------------ 2. ragged NMS
def _nms_plain(pred, ct, it, scale):
    from yolo_deepsort_amd import _lib as L
    pred = np.ascontiguousarray(pred, dtype=F32)
    out = np.zeros((300, 6), F32)
    n = C.c_int(0)
    L.check(L.load().yds_nms_pred(L.ptr(pred), pred.shape[0], pred.shape[1], ct, it, L.ptr(out), 300, C.byref(n)))
    out = out[:n.value].copy()
    out[:, :4] *= np.array(scale * 2, F32)                                 # as the sweep does: one fp32 multiply per coordinate
    return out


def _nms_merge(pred, ct, it):
    from yolo_deepsort_amd import _lib as L
    pred = np.ascontiguousarray(pred, dtype=F32)
    out = np.zeros((300, 6), F32)
    n = C.c_int(0)
    L.check(L.load().yds_nms_merge_pred(L.ptr(pred), pred.shape[0], pred.shape[1], ct, it, L.ptr(out), 300, C.byref(n)))
    return out[:n.value].copy()


def _nms_ragged(frames, ct, it):
    """frames: list of (pred [n_i, attrs], merge?, (sx, sy)) -> kept rows per frame from ONE ragged launch"""
    from yolo_deepsort_amd import _lib as L
    block = np.ascontiguousarray(np.concatenate([p for p, _, _ in frames], 0), dtype=F32)
    n_rows = np.array([p.shape[0] for p, _, _ in frames], np.int32)
    row0 = np.zeros(len(frames), np.uint64)
    row0[1:] = np.cumsum(n_rows)[:-1]
    flags = np.array([[m, m] for _, m, _ in frames], np.int32)
    scale = np.array([s for _, _, s in frames], F32)
    out = np.zeros((len(frames), 300, 6), F32)
    n = np.zeros(len(frames), np.int32)
    L.check(L.load().yds_nms_ragged_pred(L.ptr(block), block.shape[0], block.shape[1], len(frames), L.ptr(row0), L.ptr(n_rows), L.ptr(flags),
                                         L.ptr(scale), ct, it, L.ptr(out), 300, L.ptr(n)))
    return [out[f, :n[f]].copy() for f in range(len(frames))]


def _synthetic_frame(rng, n_rows, attrs, n_obj, corner, cluster=False):
    """n_rows rows of which n_obj pass the threshold: spread boxes, or one tight cluster (a single survivor: the merge branch)"""
    p = np.zeros((n_rows, attrs), F32)
    p[:, :4] = rng.uniform(1, 50, (n_rows, 4))
    p[:, 4] = rng.uniform(0, 0.3, n_rows)                                  # below the threshold
    p[:, 5:] = rng.uniform(0, 1, (n_rows, attrs - 5))
    idx = rng.choice(n_rows, n_obj, replace=False)
    if cluster:
        xy = 300 + rng.uniform(-3, 3, (n_obj, 2))
        wh = 120 + rng.uniform(-3, 3, (n_obj, 2))
    else:
        xy = rng.uniform(0, 1500, (n_obj, 2))
        wh = rng.uniform(5, 60, (n_obj, 2))
    p[idx, :4] = np.concatenate([xy, xy + wh] if corner else [xy + wh / 2, wh], 1)
    p[idx, 4] = rng.uniform(0.6, 1, n_obj)
    p[idx, 5:] = rng.uniform(0, 0.4, (n_obj, attrs - 5))
    p[idx, 5 + (0 if cluster else rng.randint(0, attrs - 5, n_obj))] = rng.uniform(0.9, 1, n_obj)
    return p


def _same_rows(got, want, tag):
    assert got.shape == want.shape, (tag, got, want)
    assert np.array_equal(got, want, equal_nan=True), (tag, got, want)     # bit for bit; the merge branch's 0 / 0 rows agree as NaN


@pytest.mark.parametrize("attrs", [7, 8])
def test_ragged_nms_equals_each_frame_alone(attrs):
    """One ragged launch over frames of 1 x 507, 4 x 507, 2 x 507 rows and 1 row, corner + merge frames among centre + scale
    frames, a frame without any candidate between two that have some: every frame's kept rows equal, bit for bit, the frame alone
    through yds_nms_pred (scaled on the host as the sweep does) or yds_nms_merge_pred."""
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    rng = np.random.RandomState(attrs)
    frames = [
        (_synthetic_frame(rng, 507, attrs, 12, False), 0, (1.5384616, 1.1538461)),
        (_synthetic_frame(rng, 4 * 507, attrs, 9, True), 1, (1.0, 1.0)),              # plain result (1 < k < n) or all kept
        (_synthetic_frame(rng, 507, attrs, 0, False), 0, (0.9615385, 0.7211539)),     # no candidate
        (_synthetic_frame(rng, 2 * 507, attrs, 5, True, cluster=True), 1, (1.0, 1.0)),  # one survivor: merged
        (_synthetic_frame(rng, 1, attrs, 1, False), 0, (1.5384616, 1.1538461)),
        (_synthetic_frame(rng, 2 * 507, attrs, 2, True), 1, (1.0, 1.0)),              # two apart: all kept, merged
    ]
    got = _nms_ragged(frames, 0.5, 0.4)
    kept = []
    for f, ((pred, merge, scale), g) in enumerate(zip(frames, got)):
        want = _nms_merge(pred, 0.5, 0.4) if merge else _nms_plain(pred, 0.5, 0.4, scale)
        _same_rows(g, want, f)
        kept.append(len(g))
    assert kept[2] == 0 and kept[3] == 1 and kept[4] == 1 and kept[5] == 2 and kept[0] > 1 and kept[1] > 1, kept
    plain3 = _nms_plain(np.concatenate([(frames[3][0][:, :2] + frames[3][0][:, 2:4]) / 2, frames[3][0][:, 2:4] - frames[3][0][:, :2],
                                        frames[3][0][:, 4:]], 1), 0.5, 0.4, (1.0, 1.0))
    assert not np.allclose(got[3][:, :4], plain3[:, :4], atol=1e-3)         # the merge branch did fire on the device


def test_ragged_nms_golden_merge_cases():
    """The four cases of tests/golden/tiled_detect.npz (all kept, one kept, plain, single) as merge frames of one ragged launch,
    centre-form frames between them: the reference's golden outputs, and bit for bit the uniform form of yds_nms_merge_pred."""
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    g = golden("tiled_detect")
    names = ("all_kept", "one_kept", "plain", "single")
    rng = np.random.RandomState(3)
    frames = []
    for nme in names:
        frames.append((g[nme + "_pred"][0], 1, (1.0, 1.0)))
        frames.append((_synthetic_frame(rng, 61, 85, 4, False), 0, (1.25, 0.75)))
    got = _nms_ragged(frames, 0.5, 0.4)
    for k, nme in enumerate(names):
        want = g[nme + "_out"]
        assert got[2 * k].shape == want.shape, nme
        assert np.array_equal(got[2 * k][:, 4:], want[:, 4:]) and np.array_equal(np.isnan(got[2 * k]), np.isnan(want)), nme
        np.testing.assert_allclose(got[2 * k][:, :4], want[:, :4], rtol=1e-6, atol=1e-4, equal_nan=True, err_msg=nme)
        _same_rows(got[2 * k], _nms_merge(frames[2 * k][0], 0.5, 0.4), nme)
        _same_rows(got[2 * k + 1], _nms_plain(frames[2 * k + 1][0], 0.5, 0.4, (1.25, 0.75)), (nme, "plain"))


def _nms_merge_batched(preds, ct, it):
    """preds: list of [n_boxes, attrs] of one length -> kept rows per frame from ONE uniform launch with the merge branch"""
    from yolo_deepsort_amd import _lib as L
    stack = np.ascontiguousarray(np.stack(preds, 0), dtype=F32)
    out = np.zeros((len(preds), 300, 6), F32)
    n = np.zeros(len(preds), np.int32)
    L.check(L.load().yds_nms_merge_pred_batched(L.ptr(stack), len(preds), stack.shape[1], stack.shape[2], ct, it, L.ptr(out), 300, L.ptr(n)))
    return [out[f, :n[f]].copy() for f in range(len(preds))]


def test_uniform_multi_frame_nms_equals_the_table_form():
    """The two descriptions of a launch's frames, several frames each: four corner-form frames of 507 rows (spread boxes, one tight
    cluster, no candidate, two boxes far apart) with the merge branch through yds_nms_merge_pred_batched (uniform record in the
    kernel arguments) and through yds_nms_ragged_pred (table read on the device), bit for bit."""
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    rng = np.random.RandomState(11)
    preds = [_synthetic_frame(rng, 507, 7, 12, True), _synthetic_frame(rng, 507, 7, 5, True, cluster=True),
             _synthetic_frame(rng, 507, 7, 0, True), _synthetic_frame(rng, 507, 7, 2, True)]
    uniform = _nms_merge_batched(preds, 0.5, 0.4)
    table = _nms_ragged([(p, 1, (1.0, 1.0)) for p in preds], 0.5, 0.4)
    for f, (u, t) in enumerate(zip(uniform, table)):
        _same_rows(u, t, f)
    kept = [len(u) for u in uniform]
    assert kept[0] > 1 and kept[1:] == [1, 0, 2], kept


def _tight_cluster(n):
    """n candidates of class 0, attrs = 7: corners 300 + U(-3, 3) to + 120 + U(-3, 3), objectness U(0.6, 1), class score U(0.9, 1).
    Returned in centre form and in corner form; the corners are the centre form's x -+ w/2 in fp32, as the emit stage computes them,
    so that both forms hold the same candidates bit for bit (they differ from the drawn corners by an fp32 rounding)."""
    rng = np.random.RandomState(n)
    p1 = 300 + rng.uniform(-3, 3, (n, 2))
    p2 = p1 + 120 + rng.uniform(-3, 3, (n, 2))
    centre = np.zeros((n, 7), F32)
    centre[:, :2] = (p1 + p2) / 2
    centre[:, 2:4] = p2 - p1
    centre[:, 4] = rng.uniform(0.6, 1, n)
    centre[:, 5] = rng.uniform(0.9, 1, n)
    corner = centre.copy()
    half = centre[:, 2:4] / F32(2)
    corner[:, :2] = centre[:, :2] - half
    corner[:, 2:4] = centre[:, :2] + half
    assert corner.dtype == F32
    return centre, corner


def test_merge_limit_is_3000_candidates():
    """The merge branch fires for 1 < n < 3000 candidates (model_build.py:122): a tight cluster of n = 2999 and of n = 3000 through
    yds_nms_merge_pred.  Both keep one row.  At 3000 it is the best candidate unmerged: bit for bit the row of yds_nms_pred on the
    same candidates in centre form.  At 2999 its box is the score-weighted mean of ALL candidates: within rtol (n + 2) * 2**-24 of
    that mean in float64 - the branch's only fp32 accumulation is the sequential sum of the n weights (error <= (n - 1) * 2**-24
    relative, all terms positive), the product sums are float64, one rounding of the sum to fp32 and one division follow - and more
    than half a pixel away from the best candidate's own box."""
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    for n in (2999, 3000):
        centre, corner = _tight_cluster(n)
        score = centre[:, 5] * centre[:, 4]                                   # fp32 product, as the emit stage
        assert score.dtype == F32 and (score > 0.5).all()
        best = int(np.argmax(score))                                          # (first of equals: the stable ranking)
        got = _nms_merge(corner, 0.5, 0.4)
        print("merge limit: n", n, "rows", len(got), "box", got[0, :4] if len(got) else None)
        assert got.shape == (1, 6), n
        assert got[0, 4] == score[best] and got[0, 5] == 0, n
        if n == 3000:
            _same_rows(got, _nms_plain(centre, 0.5, 0.4, (1.0, 1.0)), n)
            assert np.array_equal(got[0, :4], corner[best, :4])
        else:
            w = score.astype(np.float64)
            mean = (w[:, None] * corner[:, :4].astype(np.float64)).sum(0) / w.sum()
            print("merge limit: relative distance from the float64 mean", np.abs(got[0, :4] - mean) / np.abs(mean), "bound", (n + 2) * 2.0 ** -24)
            np.testing.assert_allclose(got[0, :4].astype(np.float64), mean, rtol=(n + 2) * 2.0 ** -24, atol=0)
            assert np.abs(got[0, :4] - corner[best, :4]).max() > 0.5


def test_ragged_nms_grows_its_workspace_and_reuses_it():
    """The grow-and-retry step from the table side: two centre-form frames, 2050 rows of which every row passes with both classes -
    4100 candidates against the 4096 of yds_nms_ragged_pred's own workspace - and 61 rows, each with a scale of its own.  Every
    frame's rows equal, bit for bit, the frame alone through yds_nms_pred (whose workspace of 16384 does not grow), scaled on the
    host as the sweep does; a second call runs in the grown workspace and returns the same."""
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    rng = np.random.RandomState(5)
    big = np.zeros((2050, 7), F32)
    wh = rng.uniform(5, 60, (2050, 2))
    big[:, :2] = rng.uniform(0, 1500, (2050, 2)) + wh / 2
    big[:, 2:4] = wh
    big[:, 4] = rng.uniform(0.8, 1, 2050)
    big[:, 5:] = rng.uniform(0.7, 1, (2050, 2))
    assert int(((big[:, 5:] * big[:, 4:5] > 0.5) & (big[:, 4:5] > 0.5)).sum()) == 4100
    frames = [(big, 0, (1.5384616, 1.1538461)), (_synthetic_frame(rng, 61, 7, 4, False), 0, (1.25, 0.75))]
    want = [_nms_plain(p, 0.5, 0.4, scale) for p, _, scale in frames]
    assert len(want[0]) > 1 and len(want[1]) > 1
    for call in range(2):
        for f, (g, w) in enumerate(zip(_nms_ragged(frames, 0.5, 0.4), want)):
            _same_rows(g, w, (call, f))


# ------------------------------------------------------------------------------------------------ 3. scripted scene
def test_scripted_scene_equals_each_stream_alone():
    """Streams A (4 windows), C (a setting, but plain: the frame is smaller than the window) and D (no setting) in one
    MultiStreamPipeline(stream_win_sizes=...): 4 steps with look-ahead, 2 frames per stream per step = 12 slots in one forward,
    injection tables per slot.  Frame 4 of A holds one person inside the overlap of the window columns - two candidates, one kept:
    the merge branch fires on the device while plain frames sit in the same NMS launch; frame 5 of C holds nothing (None).  Per
    stream the rows are those of the frame-by-frame path at that stream's setting."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    _check_camera_set()
    cams, F, steps = ["A", "C", "D"], 2, 4
    blob = synth.darknet_weights_blob(_cfg(), 0, -30.0)
    net = _net(blob, 12)
    heads = net.yolo_heads()
    only = {"A": {4: [2]}, "C": {5: []}, "D": None}
    scene = {c: _scripted_stream(c, F * steps, heads, only[c]) for c in cams}
    assert [len(r) for r in scene["A"][1][4]] == [1, 0, 1, 0] and scene["C"][2][5] == 0
    assert scene["A"][2][0] == 5 and sum(len(r) for r in scene["A"][1][0]) == 7          # two persons seen by two windows
    order = [[(c, s * F + k) for c in cams for k in range(F)] for s in range(steps)]
    sets = [[tab for c, t in st for tab in scene[c][1][t]] for st in order]
    assert all(len(s) == 12 for s in sets)
    pl.load_injection_sets(net, sets)
    pl.select_injection_set(net, 0)
    packs = [_pack([scene[c][0][t] for c, t in st]) for st in order]
    devs = [_lib.DeviceBuffer.from_array(p[0]) for p in packs]
    base = _deepsort()
    pipe = pl.MultiStreamPipeline(net, [base.clone() for _ in cams], 0.5, 0.4, class_mask=[0, 2, 4],
                                  stream_win_sizes=[CAMERAS[c][1] for c in cams], overlap=OVERLAP)
    ids = [cams.index(c) for c, _ in order[0]]
    got = {c: [] for c in cams}
    for s in range(steps):
        nxt = s + 1 < steps
        outs = pipe.step_mixed(devs[s].ptr, packs[s][1], packs[s][2], ids, packs[s][0].nbytes, devs[s + 1].ptr if nxt else None,
                               select_next=s + 1 if nxt else None)
        for (c, _), o in zip(order[s], outs):
            got[c].append(o)
    rows = 0
    for c in cams:
        want = _frame_by_frame(_net(blob, 4), scene[c][0], scene[c][1], CAMERAS[c][1], class_mask=[0, 2, 4])
        rows += _compare(got[c], want)
        assert sum(w is not None and len(w) > 0 for w in want) >= 4, c
    assert got["C"][5] is None
    assert rows >= 30, rows


# ------------------------------------------------------------------------------------------------ 4. chunks straddle frames
@pytest.mark.parametrize("entry", ["step_mixed", "step_host_mixed_bgr", "step"])
def test_chunks_straddle_frames(entry):
    """Random weights with objectness bias -1.3, batch_max = 5, one repeated random frame per stream for six steps.  A, B and C as a
    mixed layout (frames in HBM, and host frames in BGR order): the 7 slots run as 5 + 2.  A, D and E through the uniform step: the
    9 slots run as 5 + 4.  Per stream the rows are exactly those of the stream alone through Pipeline(win_size=...) / Pipeline()."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    _check_camera_set()
    cams = ["A", "D", "E"] if entry == "step" else ["A", "B", "C"]
    frames = [_random_frame(c, 20 + ord(c)) for c in cams]
    n, ids = 6, list(range(len(cams)))
    base = _deepsort()
    pipe = pl.MultiStreamPipeline(_random_net(5), [base.clone() for _ in cams], 0.5, 0.4, stream_win_sizes=[CAMERAS[c][1] for c in cams],
                                  overlap=OVERLAP)
    got = []
    if entry == "step":
        stack = np.stack(frames, 0)
        devs = [_lib.DeviceBuffer.from_array(stack) for _ in range(2)]
        for s in range(n):
            got.append(pipe.step(devs[s % 2].ptr, 480, 640, ids, devs[(s + 1) % 2].ptr if s + 1 < n else None))
    elif entry == "step_mixed":
        block, off, hw = _pack(frames)
        devs = [_lib.DeviceBuffer.from_array(block) for _ in range(2)]
        for s in range(n):
            got.append(pipe.step_mixed(devs[s % 2].ptr, off, hw, ids, block.nbytes, devs[(s + 1) % 2].ptr if s + 1 < n else None))
    else:
        pipe.set_frame_order(True)                                        # the frames as a decoder delivers them (B, G, R), read in place
        packs = [_pack([np.ascontiguousarray(f[:, :, ::-1]) for f in frames]) for _ in range(2)]
        for s in range(n):
            got.append(pipe.step_host_mixed(packs[s % 2], ids, packs[(s + 1) % 2] if s + 1 < n else None))
    rows = 0
    for k, c in enumerate(cams):
        want = _alone(c, frames[k], n)
        assert all(w is not None for w in want), c
        rows += _compare([g[k] for g in got], want, exact=True)
    assert rows > 0


# ------------------------------------------------------------------------------------------------ 5. the plan follows the streams
def test_plan_follows_the_streams():
    """Stream 0 is windowed, stream 1 is not, both 480 x 640.  Step 1 hands over its next frames; the next call names the streams the
    other way round - the same sizes, another plan: the look-ahead pass (planned with step 1's streams) is not reused, and the rows
    are still each stream's own.  Later, with nothing in flight, set_stream_windows takes effect on the next step."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    fa, fd = _random_frame("A", 20 + ord("A")), _random_frame("D", 20 + ord("D"))
    ad, da = _lib.DeviceBuffer.from_array(np.stack([fa, fd], 0)), _lib.DeviceBuffer.from_array(np.stack([fd, fa], 0))
    base = _deepsort()
    pipe = pl.MultiStreamPipeline(_random_net(5), [base.clone(), base.clone()], 0.5, 0.4, stream_win_sizes=[WIN, None], overlap=OVERLAP)
    got = {0: [], 1: []}

    def step(buf, ids, nxt=None):
        for s, o in zip(ids, pipe.step(buf.ptr, 480, 640, ids, nxt.ptr if nxt is not None else None)):
            got[s].append(o)

    step(ad, [0, 1], nxt=da)                                              # look-ahead over `da` planned as [windowed, plain]
    with pytest.raises(_lib.YdsError, match="in flight"):
        pipe.set_stream_windows(1, WIN, OVERLAP)
    step(da, [1, 0], nxt=ad)                                              # ... but `da` holds [plain, windowed]: redone
    step(ad, [0, 1], nxt=da)                                              # planned with [1, 0] for `ad`, asked with [0, 1]: redone again
    step(da, [1, 0], nxt=da)
    step(da, [1, 0])                                                      # the same streams: this pass is the look-ahead pass
    pipe.set_stream_windows(1, WIN, OVERLAP)                              # nothing in flight: stream 1 is windowed from now on
    assert pipe.stream_win_sizes == [WIN, WIN]
    step(ad, [0, 1])
    # the yardsticks: stream 0 alone with windows; stream 1 alone without for five frames, then with
    want0 = _alone("A", fa, 6)
    alone = pl.Pipeline(_random_net(5), _deepsort(), 0.5, 0.4)
    dev = _lib.DeviceBuffer.from_array(fd[None])
    want1 = [alone.step(dev.ptr, 480, 640, 1)[0] for _ in range(5)]
    alone.set_windows(WIN, OVERLAP)
    want1.append(alone.step(dev.ptr, 480, 640, 1)[0])
    assert _compare(got[0], want0, exact=True) > 0 and _compare(got[1], want1, exact=True) > 0
    # a reused pass would have cut the wrong frame: what stream 1 gives plain differs from what it gives windowed
    windowed1 = _alone("D", fd, 6, win=WIN)
    assert not all(np.array_equal(a, b) for a, b in zip(want1[:5], windowed1[:5]))


# ------------------------------------------------------------------------------------------------ 6. no setting = today's pipeline
def test_no_stream_setting_and_one_setting_for_all_equal_the_existing_modes():
    """stream_win_sizes=[None, None] gives exactly the rows of MultiStreamPipeline() on a mixed layout; [(416, 416)] * 2 on 480 x 640
    frames gives exactly the rows of MultiStreamPipeline(win_size=(416, 416))."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    net = _random_net(5)
    base = _deepsort()

    def run(frames, mixed, **kw):
        pipe = pl.MultiStreamPipeline(net, [base.clone(), base.clone()], 0.5, 0.4, overlap=OVERLAP, **kw)
        out = []
        if mixed:
            block, off, hw = _pack(frames)
            devs = [_lib.DeviceBuffer.from_array(block) for _ in range(2)]
            for s in range(4):
                out += pipe.step_mixed(devs[s % 2].ptr, off, hw, [0, 1], block.nbytes, devs[(s + 1) % 2].ptr if s < 3 else None)
        else:
            devs = [_lib.DeviceBuffer.from_array(np.stack(frames, 0)) for _ in range(2)]
            for s in range(4):
                out += pipe.step(devs[s % 2].ptr, 480, 640, [0, 1], devs[(s + 1) % 2].ptr if s < 3 else None)
        return out

    mixed = [_random_frame("A", 1), _random_frame("C", 2)]
    assert _compare(run(mixed, True, stream_win_sizes=[None, None]), run(mixed, True), exact=True) > 0
    same = [_random_frame("A", 1), _random_frame("D", 3)]
    assert _compare(run(same, False, stream_win_sizes=[WIN, WIN]), run(same, False, win_size=WIN), exact=True) > 0


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_pipeline_usable():
    """Every refusal of yds_pipeline_set_stream_windows, and of set_windows while a stream holds a setting, raises and changes
    nothing: the pipeline steps with the rows it gave before.  Refused during an in-flight look-ahead, the next step still
    consumes that pass."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    net = _random_net(5)
    fa, fd = _random_frame("A", 20 + ord("A")), _random_frame("D", 20 + ord("D"))
    devs = [_lib.DeviceBuffer.from_array(np.stack([fa, fd], 0)) for _ in range(2)]
    base = _deepsort()
    with pytest.raises(ValueError, match="exclude"):
        pl.MultiStreamPipeline(net, [base.clone(), base.clone()], win_size=WIN, stream_win_sizes=[WIN, None])
    with pytest.raises(ValueError, match="one entry per stream"):
        pl.MultiStreamPipeline(net, [base.clone(), base.clone()], stream_win_sizes=[WIN])
    pipe = pl.MultiStreamPipeline(net, [base.clone(), base.clone()], 0.5, 0.4, stream_win_sizes=[WIN, None], overlap=OVERLAP)
    got = {0: [], 1: []}

    def step(k, nxt=False):
        for s, o in enumerate(pipe.step(devs[k].ptr, 480, 640, [0, 1], devs[k ^ 1].ptr if nxt else None)):
            got[s].append(o)

    step(0)
    with pytest.raises(_lib.YdsError, match="stream 2"):                  # stream outside [0, n_streams)
        pipe.set_stream_windows(2, WIN, OVERLAP)
    with pytest.raises(_lib.YdsError, match="stream -1"):
        _lib.check(_lib.load().yds_pipeline_set_stream_windows(pipe._h, -1, 416, 416, OVERLAP))
    with pytest.raises(_lib.YdsError, match="416 x 0"):                   # win_w > 0 with win_h <= 0
        pipe.set_stream_windows(1, (416, 0), OVERLAP)
    for bad in (-0.1, float("nan")):                                      # an overlap that is not >= 0
        with pytest.raises(_lib.YdsError, match="overlap"):
            pipe.set_stream_windows(1, WIN, bad)
    with pytest.raises(_lib.YdsError, match="set_stream_windows"):        # the two modes are exclusive, this way round ...
        pipe.set_windows(WIN, OVERLAP)
    assert pipe.stream_win_sizes == [WIN, None] and pipe.win_size is None
    step(1, nxt=True)
    with pytest.raises(_lib.YdsError, match="in flight"):                 # a look-ahead pass in flight
        pipe.set_stream_windows(1, WIN, OVERLAP)
    with pytest.raises(_lib.YdsError, match="in flight"):
        pipe.set_stream_windows(0, None)
    step(0)                                                               # consumes that pass
    single = pl.Pipeline(net, _deepsort(), 0.5, 0.4)                      # a single-stream pipeline has no streams to set
    with pytest.raises(_lib.YdsError, match="no streams"):
        _lib.check(_lib.load().yds_pipeline_set_stream_windows(single._h, 0, 416, 416, OVERLAP))
    assert single.step(devs[0].ptr, 480, 640, 1)[0] is not None
    other = pl.MultiStreamPipeline(net, [base.clone(), base.clone()], 0.5, 0.4, win_size=WIN, overlap=OVERLAP)
    with pytest.raises(_lib.YdsError, match="yds_pipeline_set_windows"):  # ... and that way round
        other.set_stream_windows(0, WIN, OVERLAP)
    assert other.stream_win_sizes == [None, None]
    assert len(other.step(devs[0].ptr, 480, 640, [0, 1])) == 2
    other.set_windows(None)
    other.set_stream_windows(0, WIN, OVERLAP)                             # window mode off: accepted
    step(1)
    assert _compare(got[0], _alone("A", fa, 4), exact=True) > 0 and _compare(got[1], _alone("D", fd, 4), exact=True) > 0


# ------------------------------------------------------------------------------------------------ 8. VideoDetector.detect_streams
def test_detect_streams_with_stream_win_sizes(tmp_path):
    """detect_streams(stream_win_sizes=[(416, 416), None], mixed_sizes=True) on two short .npy clips (BGR, as a decoder delivers
    them), 480 x 640 and 300 x 400: per stream the rows and the rendered images are those of detect() on that clip alone - with
    win_size=(416, 416), frame by frame, for the first, without windows for the second."""
    from yolo_deepsort_amd.deep_sort import DeepSort
    net = _net(synth.darknet_weights_blob(_cfg(), 0, -1.3), 4)            # (its own: detect() sizes the detector's batch by the clip)
    base = DeepSort(_extractor(), use_cuda=True, **DS)
    clips = []
    for k, (cam, n) in enumerate((("A", 5), ("C", 4))):
        f = _random_frame(cam, 40 + k)
        path = str(tmp_path / ("clip%d.npy" % k))
        np.save(path, np.stack([np.roll(f, 3 * t, axis=1)[:, :, ::-1] for t in range(n)], 0))
        clips.append((path, n, f.shape))
    vd = _video_detector(net, base)
    per = [[], []]
    for items in vd.detect_streams([c[0] for c in clips], frames_per_stream=1, show_fps=False, mixed_sizes=True, stream_win_sizes=[WIN, None]):
        for s, img, rows, acts in items:
            assert acts == []
            per[s].append((img, _rows(rows)))
    rows = 0
    for s, (path, n, shape) in enumerate(clips):
        alone = _video_detector(net, base.clone(), win_size=WIN if s == 0 else None, batch_windows=False)
        want = [(img, _rows(d)) for img, d, _ in alone.detect(path, show_fps=False)]
        assert len(per[s]) == len(want) == n and all(img.shape == shape for img, _ in per[s])
        rows += _compare([d for _, d in per[s]], [d for _, d in want])
        for (img, d), (wimg, wd) in zip(per[s], want):
            if d is None or np.array_equal(d, wd):                        # the overlay draws the integer rows
                assert np.array_equal(img, wimg), s
    assert rows > 0
    with pytest.raises(ValueError, match="win_size"):                     # a detector with its own win_size: one or the other
        list(_video_detector(net, base, win_size=WIN).detect_streams([c[0] for c in clips], show_fps=False, stream_win_sizes=[WIN, None]))
