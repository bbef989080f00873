"""Sliding-window detection in the batched pipelines (csrc/pipeline.cpp window mode, yds_pipeline_set_windows): the windows of all
frames of a step are cut on the device, run through the detector in chunks of batch_max and merged per frame by one NMS launch
(merge branch included, csrc/nms.hip launch with a frame table).  The yardstick is the frame-by-frame path - VideoDetector.process with an
ImageDetector(win_size=...) (yds_detect_tiled, host merge branch) + DeepSort.update - which tests/test_gpu_assoc.py pins to the
reference's golden vectors.  Row criterion as tests/test_gpu_pipeline.py: track ids and classes bit exact, boxes within one pixel,
None frames agree.  yolov3-tiny at 416, win_size = (416, 416), overlap 0.15 throughout."""
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
WIN, OVERLAP, SIZE = (416, 416), 0.15, 416
EMPTY = np.zeros((0, 9), F32)
# img_detect.py:103-121 for a 480 x 640 frame: x, y, tile_h, tile_w, x-major then y
WINDOWS_480x640 = [(0, 0, 478, 478), (0, 416, 64, 478), (416, 0, 478, 224), (416, 416, 64, 224)]


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


def _extractor():
    """One ReID extractor for the whole module (DeepSort(extractor, ...) shares it: deep_sort.py:41-44)."""
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


def _video_detector(net, tracker, class_mask=None, win_size=WIN, thres=0.5, **kw):
    from yolo_deepsort_amd.detect import VideoDetector
    return VideoDetector(net, _names(), thres=thres, nms_thres=0.4, tracker=tracker, class_mask=class_mask, win_size=win_size,
                         overlap=OVERLAP, **kw)


def _rows(o):
    return None if o is None else np.array(o, np.int32).reshape(-1, 6)


def _frame_by_frame(net, frames, inj=None, class_mask=None, thres=0.5):
    """The yardstick: every frame through ImageDetector(win_size).detect + DeepSort.update (VideoDetector.process), one frame at a
    time; inj[t] = one injection table per window of frame t.  Asserts that the detector's rows hold no NaN."""
    vd = _video_detector(net, _deepsort(), class_mask, thres=thres, batch_frames=1)
    out = []
    for t, frame in enumerate(frames):
        if inj is not None:
            for slot, rows in enumerate(inj[t]):
                net.set_injection(slot, rows)
        det = vd.image_detector.detect(frame)
        if det is not None:
            det = det.numpy() if hasattr(det, "numpy") else det
            assert not np.isnan(det).any(), t
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


def _window_tables(tlwh, cls, windows, heads):
    """Injection tables of one frame, one per window: a person goes into every window that holds its whole box, in window
    coordinates (the window is what the network sees, stretched to the model size)."""
    tables = []
    for x0, y0, th, tw in windows:
        inside = [i for i, (x, y, w, h) in enumerate(tlwh) if x >= x0 and y >= y0 and x + w <= x0 + tw and y + h <= y0 + th]
        if not inside:
            tables.append(EMPTY)
            continue
        local = np.array([[tlwh[i][0] - x0, tlwh[i][1] - y0, tlwh[i][2], tlwh[i][3]] for i in inside], F32)
        rows = synth.head_injection(local, (th, tw), (SIZE, SIZE), heads)
        rows[:, 8] = [cls[i] for i in inside]
        tables.append(rows)
    return tables


def _scripted_frame(t, only=None):
    """Persons (tlwh, class) of frame t of the scripted 480 x 640 scene.  Person 2 walks inside the 62-pixel overlap of the two
    window columns (seen by windows 0 and 2), person 4 inside the overlap of the rows (windows 0 and 1), the others in one window."""
    persons = [((50 + 3 * t, 100 + 2 * t, 50, 120), 0), ((300 - 2 * t, 250 + t, 60, 150), 2), ((425 + t, 150 + 2 * t, 35, 100), 0),
               ((520 + 3 * t, 60 + t, 60, 140), 2), ((100 + 2 * t, 424, 30, 45), 0)]
    if only is not None:
        persons = [persons[i] for i in only]
    return [p for p, _ in persons], [c for _, c in persons]


def _scene_frame(t, tlwh):
    """A frame with a texture patch per person on a blocky background (the ReID crops must differ between persons)."""
    rng = np.random.RandomState(100 + t)
    img = np.repeat(np.repeat(rng.randint(0, 256, (60, 80, 3)), 8, 0), 8, 1).astype(np.uint8)
    for i, (x, y, w, h) in enumerate(tlwh):
        patch = np.random.RandomState(7 + int(w) * 31 + int(h)).randint(0, 256, (8, 4, 3)).astype(np.uint8)
        yy = (np.arange(int(h)) * 8 // int(h)).clip(0, 7)
        xx = (np.arange(int(w)) * 4 // int(w)).clip(0, 3)
        img[int(y):int(y) + int(h), int(x):int(x) + int(w)] = patch[yy][:, xx]
    return img


def _scripted_stream(n, heads, merge_at=(), empty_at=()):
    frames, inj, persons = [], [], []
    for t in range(n):
        tlwh, cls = _scripted_frame(t, only=[] if t in empty_at else ([2] if t in merge_at else None))
        frames.append(_scene_frame(t, tlwh))
        inj.append(_window_tables(tlwh, cls, WINDOWS_480x640, heads))
        persons.append(len(tlwh))
    return np.stack(frames, 0), inj, persons


# ------------------------------------------------------------------------------------------------ 1. scripted scene, one forward
def test_scripted_scene_one_forward_with_lookahead():
    """480 x 640 frames = 4 windows; 3 frames per step = 12 slots in ONE forward (batch_max = 12), 4 steps with look-ahead, injection
    tables per window slot.  Frame 4 holds one person inside the overlap of the window columns: two candidates, one kept - the merge
    branch fires (on the device here, on the host in the yardstick); the other frames hold five persons, two of them seen by two
    windows (plain branch, duplicates suppressed); frame 7 holds nothing (None)."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    B, T, steps = 3, 4, 4
    blob = synth.darknet_weights_blob(_cfg(), 0, -30.0)
    net = _net(blob, B * T)
    heads = net.yolo_heads()
    frames, inj, persons = _scripted_stream(B * steps, heads, merge_at=(4,), empty_at=(7,))
    assert [len(r) for r in inj[4]] == [1, 0, 1, 0] and persons[7] == 0        # n = 2 candidates for one person; a frame with nothing
    assert persons[0] == 5 and sum(len(r) for r in inj[0]) == 7                 # five persons, two of them seen by two windows
    pl.load_injection_sets(net, [[inj[s * B + b][t] for b in range(B) for t in range(T)] for s in range(steps)])
    pl.select_injection_set(net, 0)
    pipe = pl.Pipeline(net, _deepsort(), 0.5, 0.4, class_mask=[0, 2, 4], win_size=WIN, overlap=OVERLAP)
    dev = _lib.DeviceBuffer.from_array(frames)
    got = []
    for s in range(steps):
        nxt = dev.offset((s + 1) * B * frames[0].nbytes) if s + 1 < steps else None
        got += pipe.step(dev.offset(s * B * frames[0].nbytes), 480, 640, B, nxt, select_next=(s + 1 if nxt is not None else None))
    want = _frame_by_frame(_net(blob, T), frames, inj, class_mask=[0, 2, 4])
    rows = _compare(got, want)
    assert got[7] is None and want[7] is None
    assert rows >= 20, rows
    assert pipe.stage_us()["detector_dev"] > 0


# ------------------------------------------------------------------------------------------------ 1b. front end, bit exact
def _slot_pred(pipe, attrs):
    from yolo_deepsort_amd import _lib as L
    n = C.c_size_t(0)
    L.check(L.load().yds_pipeline_slot_pred(pipe._h, None, 0, C.byref(n)))
    out = np.zeros((n.value, attrs), F32)
    L.check(L.load().yds_pipeline_slot_pred(pipe._h, L.ptr(out), n.value, C.byref(n)))
    return out


def test_window_mode_front_end_bit_exact(monkeypatch):
    """Window mode itself, one step of two random 480 x 640 frames = 8 slots (slot = frame * 4 + window).  batch_max = 8, one chunk:
    every network-input slot equals the oracle's cv2-exact resize of its window; every row of the prediction block equals
    img_detect.py:132-138 restated in fp32 on the network's raw rows - corner form, resize_boxes to the window, shift by its origin.
    batch_max = 5 (chunks of 5 + 3 straddle the frames), and the same frames handed over in BGR order: the same block bit for bit.
    The detector's built-in tile choice is pinned (YDS_NO_AUTOTUNE): a measured choice is made per batch size, and two conv tiles may
    round a sum differently (seen between the chunks of 5 / 3 and of 8: 1e-7 relative), which is the detector's and not the route's."""
    monkeypatch.setenv("YDS_NO_AUTOTUNE", "1")
    from oracle.resize import resize_bilinear_u8
    from yolo_deepsort_amd import _lib, pipeline as pl
    blob = synth.darknet_weights_blob(_cfg(), 0, -1.3)
    frames = np.random.RandomState(12).randint(0, 256, (2, 480, 640, 3)).astype(np.uint8)
    slots = [(f, win) for f in range(2) for win in WINDOWS_480x640]

    def block(batch_max, bgr):
        net = _net(blob, batch_max)
        pipe = pl.Pipeline(net, _deepsort(), 0.5, 0.4, win_size=WIN, overlap=OVERLAP)
        pipe.set_frame_order(bgr)
        dev = _lib.DeviceBuffer.from_array(np.ascontiguousarray(frames[..., ::-1]) if bgr else frames)
        assert len(pipe.step(dev.ptr, 480, 640, 2)) == 2
        return net, _slot_pred(pipe, net.num_attrs)

    net, got = block(8, False)
    boxes = net.num_boxes
    got = got.reshape(8, boxes, net.num_attrs)
    want_in = np.stack([resize_bilinear_u8(frames[f][y0:y0 + th, x0:x0 + tw], (SIZE, SIZE)).astype(F32).transpose(2, 0, 1) / F32(255.)
                        for f, (x0, y0, th, tw) in slots], 0)
    got_in = net.get_input(8)
    for n, slot in enumerate(slots):
        assert np.array_equal(got_in[n], want_in[n]), (n, slot)
    raw = net.forward(want_in)                                             # the same 8 images through the same detector
    assert raw.shape == got.shape
    for n, (f, (x0, y0, th, tw)) in enumerate(slots):
        half = raw[n][:, 2:4] / F32(2)
        corner = np.concatenate([raw[n][:, :2] - half, raw[n][:, :2] + half], 1)
        scale = np.array([F32(tw / SIZE), F32(th / SIZE)] * 2, F32)        # resize_boxes: python-double ratio, fp32 multiply
        want = raw[n].copy()
        want[:, :4] = corner * scale + np.array([x0, y0, x0, y0], F32)
        assert want.dtype == F32 and np.array_equal(got[n], want), (n, f)
    for batch_max, bgr in ((5, False), (8, True), (5, True)):
        other = block(batch_max, bgr)[1]
        print("batch_max", batch_max, "bgr", bgr, "rows", other.shape[0], "elements that differ", int((other.reshape(got.shape) != got).sum()))
        assert other.shape == (8 * boxes, net.num_attrs) and np.array_equal(other.reshape(got.shape), got), (batch_max, bgr)


# ------------------------------------------------------------------------------------------------ 2. chunks straddling frames
def _random_weights_case(frame, n_frames, B, batch_max, host_bgr):
    from yolo_deepsort_amd import _lib, pipeline as pl
    blob = synth.darknet_weights_blob(_cfg(), 0, -1.3)
    h, w = frame.shape[:2]
    frames = np.stack([frame] * n_frames, 0)
    key = ("yard", h, w)
    if key not in _shared:                              # the yardstick of a frame size is computed once
        _shared[key] = _frame_by_frame(_net(blob, 4), frames)
    want = _shared[key]
    pipe = pl.Pipeline(_net(blob, batch_max), _deepsort(), 0.5, 0.4, win_size=WIN, overlap=OVERLAP)
    got = []
    steps = n_frames // B
    if host_bgr:
        # the frames as a decoder delivers them (B, G, R), read in place: the same results as the frame-by-frame path on the reversed frames
        pipe.set_frame_order(True)
        bufs = [np.ascontiguousarray(frames[s * B:(s + 1) * B, :, :, ::-1]) for s in range(steps)]
        for s in range(steps):
            got += pipe.step_host(bufs[s], bufs[s + 1] if s + 1 < steps else None)
    else:
        dev = _lib.DeviceBuffer.from_array(frames)
        for s in range(steps):
            nxt = dev.offset((s + 1) * B * frame.nbytes) if s + 1 < steps else None
            got += pipe.step(dev.offset(s * B * frame.nbytes), h, w, B, nxt)
    return got, want


@pytest.mark.parametrize("shape,seed,host_bgr", [((480, 640), 0, False), ((480, 640), 0, True), ((531, 977), 4, False)])
def test_chunks_straddle_frames(shape, seed, host_bgr):
    """No injection: random weights with objectness bias -1.3 on one random frame repeated six times (tracks confirm on the third).
    batch_max = 5 and 3 frames per step: the 12 windows of a 480 x 640 step run as 5 + 5 + 2, the 18 ragged windows of a 531 x 977
    step as 5 + 5 + 5 + 3 - chunks straddle frames.  Frames resident in HBM, and host frames in BGR order (step_host)."""
    frame = np.random.RandomState(seed).randint(0, 256, shape + (3,)).astype(np.uint8)
    got, want = _random_weights_case(frame, 6, 3, 5, host_bgr)
    rows = _compare(got, want)
    assert all(w is not None for w in want) and rows > 0, rows


def test_nms_workspace_overflow_redoes_the_window_pass():
    """A threshold so low that one WINDOW alone has more candidates than the pipeline's NMS workspace holds (4096): the workspace
    grows and the window pass of that step is redone - while the look-ahead pass of the next step is already in flight."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    blob = synth.darknet_weights_blob(_cfg(), 0, -1.0)
    conf = 0.3
    frame = np.random.RandomState(4).randint(0, 256, (480, 640, 3)).astype(np.uint8)
    frames = np.stack([frame] * 4, 0)
    yard = _net(blob, 4)
    pred = yard.forward_u8(np.ascontiguousarray(frame[:478, :478]))[0]                # window 0 as the window path sees it
    n_cand = int(((pred[:, 5:] * pred[:, 4:5] > conf) & (pred[:, 4:5] > conf)).sum())
    assert n_cand > 4096, n_cand                                                     # the case this test is about
    want = _frame_by_frame(yard, frames, thres=conf)
    pipe = pl.Pipeline(_net(blob, 5), _deepsort(), conf, 0.4, win_size=WIN, overlap=OVERLAP)   # 2 frames = 8 windows = 5 + 3
    dev = _lib.DeviceBuffer.from_array(frames)
    got = pipe.step(dev.offset(0), 480, 640, 2, dev.offset(2 * frame.nbytes)) + pipe.step(dev.offset(2 * frame.nbytes), 480, 640, 2)
    assert _compare(got, want) > 0


# ------------------------------------------------------------------------------------------------ 3. merge branch: a frame in a batch against the frame alone
def _merge_alone(pred, ct, it):
    from yolo_deepsort_amd import _lib as L
    pred = np.ascontiguousarray(pred, dtype=F32)
    out = np.zeros((300, 6), F32)
    n = C.c_int(0)
    L.check(L.load().yds_nms_merge_pred(L.ptr(pred), pred.shape[0], pred.shape[1], ct, it, L.ptr(out), 300, C.byref(n)))
    return out[:n.value].copy()


def _merge_batched(preds, ct, it):
    """preds: list of [n_i, attrs]; stacked as frames, padded to a common n with zero-confidence rows."""
    from yolo_deepsort_amd import _lib as L
    n_boxes = max(p.shape[0] for p in preds)
    stack = np.zeros((len(preds), n_boxes, preds[0].shape[1]), F32)
    for f, p in enumerate(preds):
        stack[f, :p.shape[0]] = p
    out = np.zeros((len(preds), 300, 6), F32)
    n = np.zeros(len(preds), np.int32)
    L.check(L.load().yds_nms_merge_pred_batched(L.ptr(stack), len(preds), n_boxes, stack.shape[2], ct, it, L.ptr(out), 300, L.ptr(n)))
    return [out[f, :n[f]].copy() for f in range(len(preds))]


def _same_detections(got, want, tag, atol=1e-4):
    assert got.shape == want.shape, tag
    assert np.array_equal(got[:, 4:], want[:, 4:]), tag                       # scores and classes: bit exact
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    np.testing.assert_allclose(got[:, :4], want[:, :4], rtol=1e-6, atol=atol, equal_nan=True, err_msg=str(tag))


def _same_rows(got, want, tag):
    assert got.shape == want.shape, tag
    assert np.array_equal(got, want, equal_nan=True), (tag, got, want)        # bit for bit; 0 / 0 rows agree as NaN


def test_merge_frame_in_a_uniform_batch_equals_the_frame_alone():
    """yds_nms_merge_pred_batched (several frames in one uniform launch, the merge branch for each) against yds_nms_merge_pred (the
    same launch with one frame): a frame inside a multi-frame launch equals the frame alone, bit for bit.  Both against the
    reference's golden outputs: the four cases of tiled_detect.npz as four frames.  Then the 40 random trials of
    test_gpu_assoc.py::test_nms_merge_branch_golden_and_oracle in groups of ten, each also against the oracle
    (soft_non_max_suppression_merge) at that test's tolerances: scores, classes and NaN pattern bit-exact, boxes rtol 1e-6, atol 1e-3."""
    from yolo_deepsort_amd import _lib
    from oracle import nms as onms
    _lib.init(0)
    g = golden("tiled_detect")
    names = ("all_kept", "one_kept", "plain", "single")
    preds = [g[nme + "_pred"][0] for nme in names]
    preds[1] = np.concatenate([preds[1], np.zeros((7, preds[1].shape[1]), F32)], 0)      # (frames of different length: padding inside the call too)
    for nme, p, got in zip(names, preds, _merge_batched(preds, 0.5, 0.4)):
        _same_detections(got, g[nme + "_out"], nme)
        _same_rows(got, _merge_alone(p, 0.5, 0.4), nme)
    rng = np.random.RandomState(8)
    trials = []
    for trial in range(40):
        n = int(rng.choice([2, 3, 5, 40]))
        p = np.zeros((1, n, 85), F32)
        if trial % 2:                                   # one tight cluster -> a single survivor
            p[0, :, :2] = 300 + rng.uniform(-3, 3, (n, 2))
            p[0, :, 2:4] = p[0, :, :2] + 120 + rng.uniform(-3, 3, (n, 2))
        else:
            p[0, :, :2] = rng.uniform(0, 1500, (n, 2))
            p[0, :, 2:4] = p[0, :, :2] + rng.uniform(5, 60, (n, 2))
        p[0, :, 4] = rng.uniform(0.3, 1, n)
        p[0, np.arange(n), 5 + (0 if trial % 2 else rng.randint(0, 3, n))] = rng.uniform(0.6, 1, n)
        trials.append(p)
    seen = set()
    for g0 in range(0, 40, 10):
        group = trials[g0:g0 + 10]
        for i, (p, got) in enumerate(zip(group, _merge_batched([p[0] for p in group], 0.5, 0.4))):
            _same_rows(got, _merge_alone(p[0], 0.5, 0.4), g0 + i)
            want = onms.soft_non_max_suppression_merge(p, 0.5, 0.4)[0]         # independent of the code under test
            if want is None:
                assert got.shape[0] == 0, g0 + i
                continue
            _same_detections(got, want, g0 + i, atol=1e-3)
            b = p[..., :4].astype(np.float64)
            centre = np.stack([(b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2, b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]], -1)
            plain = onms.soft_non_max_suppression(np.concatenate([centre.astype(F32), p[..., 4:]], -1), 0.5, 0.4)[0]
            seen.add("merged" if not np.allclose(np.nan_to_num(got[:, :4]), plain[:, :4], atol=1e-3) else "plain")
    assert seen == {"merged", "plain"}


# ------------------------------------------------------------------------------------------------ 4. multi-stream
def test_two_staggered_streams_equal_each_stream_alone():
    """Two streams in one MultiStreamPipeline(win_size=...): stream 1 starts a step after stream 0 and plays the scene from another
    frame offset; per stream the rows are those of the stream alone through Pipeline(win_size=...), bit for bit."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    T, bm = 4, 12
    blob = synth.darknet_weights_blob(_cfg(), 0, -30.0)
    net = _net(blob, bm)
    heads = net.yolo_heads()
    frames, inj, _ = _scripted_stream(9, heads, merge_at=(5,))
    offset = (0, 2)                                                    # stream s plays scene frames offset[s] + k
    steps = [[(0, 0), (0, 1)], [(0, 2), (1, 0), (1, 1)], [(0, 3), (1, 2), (1, 3)], [(0, 4), (1, 4)], [(0, 5), (1, 5), (1, 6)], [(0, 6)]]

    def play(pipe, steps, multi):
        sets = []
        for st in steps:
            tabs = [inj[offset[s] + k][t] for s, k in st for t in range(T)]
            sets.append(tabs + [EMPTY] * (bm - len(tabs)))
        pl.load_injection_sets(net, sets)
        devs = [_lib.DeviceBuffer.from_array(np.stack([frames[offset[s] + k] for s, k in st], 0)) for st in steps]
        res, sel = [], None
        for i, st in enumerate(steps):
            if sel != i:
                pl.select_injection_set(net, i)
            ahead = i + 1 < len(steps) and len(steps[i + 1]) == len(st)
            nxt, sn = (devs[i + 1].ptr if ahead else None), (i + 1 if ahead else None)
            if multi:
                res.append(pipe.step(devs[i].ptr, 480, 640, [s for s, _ in st], nxt, select_next=sn))
            else:
                res.append(pipe.step(devs[i].ptr, 480, 640, len(st), nxt, select_next=sn))
            sel = sn
        return res

    trackers = [_deepsort(), _deepsort()]
    multi = pl.MultiStreamPipeline(net, trackers, 0.5, 0.4, class_mask=[0, 2, 4], win_size=WIN, overlap=OVERLAP)
    out = play(multi, steps, True)
    per_stream = {0: [], 1: []}
    for st, outs in zip(steps, out):
        for (s, k), o in zip(st, outs):
            per_stream[s].append(o)
    rows = 0
    for s in (0, 1):
        alone_steps = [[(s, k) for ss, k in st if ss == s] for st in steps]
        alone_steps = [st for st in alone_steps if st]
        alone = pl.Pipeline(net, _deepsort(), 0.5, 0.4, class_mask=[0, 2, 4], win_size=WIN, overlap=OVERLAP)
        want = [o for outs in play(alone, alone_steps, False) for o in outs]
        rows += _compare(per_stream[s], want, exact=True)
    assert rows >= 20, rows


# ------------------------------------------------------------------------------------------------ 5. surface
def test_video_detector_batch_windows_and_detect_streams(tmp_path):
    """VideoDetector(win_size=..., batch_windows=True).detect runs the batched pipeline in window mode: the rows of a 7-frame .npy clip
    (BGR, as a decoder delivers it) equal those of the same detector with batch_windows=False (frame by frame); detect_streams
    accepts a detector with win_size and gives every stream those rows too."""
    blob = synth.darknet_weights_blob(_cfg(), 0, -1.3)
    frame = np.random.RandomState(0).randint(0, 256, (480, 640, 3)).astype(np.uint8)
    clip = str(tmp_path / "clip.npy")
    np.save(clip, np.stack([frame[:, :, ::-1]] * 7, 0))
    runs = {}
    for bw in (False, True):
        vd = _video_detector(_net(blob, 4), _deepsort(), batch_frames=4, batch_windows=bw)
        assert not vd._batchable()                                   # (pinned by tests/test_host_logic.py: win_size alone stays frame by frame)
        runs[bw] = [(img.shape, _rows(d)) for img, d, _ in vd.detect(clip, show_fps=False)]
        assert (vd._pipe is not None) == bw                          # the batched pipeline ran exactly when asked for
    assert len(runs[True]) == len(runs[False]) == 7 and all(s == (480, 640, 3) for s, _ in runs[True])
    assert _compare([d for _, d in runs[True]], [d for _, d in runs[False]]) > 0
    vd = _video_detector(_net(blob, 4), _deepsort())
    per_stream = {0: [], 1: []}
    for items in vd.detect_streams([[frame] * 4, [frame] * 3], frames_per_stream=2, show_fps=False):
        for s, img, rows, acts in items:
            assert img.shape == (480, 640, 3)
            per_stream[s].append(_rows(rows))
    assert len(per_stream[0]) == 4 and len(per_stream[1]) == 3
    want = [d for _, d in runs[False]]
    assert _compare(per_stream[0], want[:4]) + _compare(per_stream[1], want[:3]) > 0


def test_small_frames_take_the_plain_path_and_set_windows_is_refused_in_flight():
    """A frame with w < win_w and h < win_h takes the plain path (img_detect.py:68): the rows of Pipeline(win_size=...) are exactly
    those of Pipeline().  yds_pipeline_set_windows is refused while a look-ahead pass is in flight and the pipeline goes on working."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    blob = synth.darknet_weights_blob(_cfg(), 0, -1.3)
    frame = np.random.RandomState(2).randint(0, 256, (300, 400, 3)).astype(np.uint8)
    frames = np.stack([frame] * 6, 0)
    net = _net(blob, 3)
    dev = _lib.DeviceBuffer.from_array(frames)
    nxt = dev.offset(3 * frame.nbytes)
    runs = {}
    for win in (None, WIN):
        pipe = pl.Pipeline(net, _deepsort(), 0.5, 0.4, win_size=win, overlap=OVERLAP)
        got = pipe.step(dev.offset(0), 300, 400, 3, nxt)
        for new in (None, (208, 208)):
            with pytest.raises(_lib.YdsError, match="in flight"):
                pipe.set_windows(new, OVERLAP)
        assert pipe.win_size == win
        got += pipe.step(nxt, 300, 400, 3)
        pipe.set_windows(win, OVERLAP)                                # nothing in flight any more: accepted
        runs[win] = got
    assert _compare(runs[WIN], runs[None], exact=True) > 0
