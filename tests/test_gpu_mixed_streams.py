"""Cameras of different frame sizes in one multi-stream step (csrc/pipeline.cpp yds_pipeline_step_multi_mixed): every frame carries its
own offset and size through the resize front end, the NMS scale and the ReID crops.  The front ends are checked bit for bit against the
oracle's cv2-exact resize, a uniform layout through the mixed entry against the uniform entry, and a mixed step against each stream
run alone through the single-stream Pipeline at its own size."""
import functools

import numpy as np
import pytest

from yolo_deepsort_amd import cfgs, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
EMPTY = np.zeros((0, 9), np.float32)
IMG = (416, 416)


@functools.lru_cache(maxsize=None)
def _net(obj_bias=-4.0, batch_max=8):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", *IMG)
    net = Darknet(None, img_size=IMG, batch_max=batch_max, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, obj_bias))
    return net


@functools.lru_cache(maxsize=None)
def _extractor():
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import Extractor
    _lib.init(0)
    return Extractor(synth.reid_state_dict(0), max_crops=256)


def _deepsort():
    from yolo_deepsort_amd.deep_sort import DeepSort
    return DeepSort(_extractor(), use_cuda=True, **DS)


def _layout(frames):
    from yolo_deepsort_amd.pipeline import pack_frames
    return pack_frames(frames)


# ------------------------------------------------------------------------------------------------ 1. resize front end, exact
def test_mixed_resize_front_end_bit_exact():
    """Six frames of six sizes in ONE detector call: the same-size copy, the exact-2x area mean, bilinear down and up, a tiny source.
    The 333 x 501 frame holds an odd number of bytes, so every frame behind it starts at an odd offset.  Each slot of the network
    input equals the oracle's cv2-exact resize of its own frame."""
    from oracle.resize import resize_bilinear_u8
    net = _net()
    rng = np.random.RandomState(5)
    sizes = ((416, 416), (832, 832), (333, 501), (480, 640), (100, 90), (2, 3))
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    _, off, _ = _layout(frames)
    assert (333 * 501 * 3) % 4 and all(int(o) % 2 for o in off[3:])
    net.forward_u8_mixed(frames)
    got = net.get_input(len(frames))
    for n, f in enumerate(frames):
        want = resize_bilinear_u8(f, IMG).astype(F32).transpose(2, 0, 1) / F32(255.)
        assert np.array_equal(got[n], want), sizes[n]


# ------------------------------------------------------------------------------------------------ 2. crops, exact
def test_mixed_crops_bit_exact():
    """The crop front end over three device frames of different sizes: each box is clamped to ITS frame (the overhanging box of the
    64 x 128 frame ends at column 127 / row 63, not at a neighbour's border) and cut from it; copy, exact-2x and bilinear crops."""
    from oracle import reid as oreid
    rng = np.random.RandomState(9)
    sizes = ((64, 128), (96, 128), (480, 640))
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    boxes = [  # (frame, tlwh)
        (0, (10, 5, 40, 50)), (1, (20, 10, 50, 70)), (2, (100, 50, 80, 200)),        # interior, one per frame
        (0, (100, 30, 60, 60)),                                                      # overhangs the right and bottom edge of frame 0
        (1, (-5.5, -3.2, 40, 50)),                                                   # negative origin
        (2, (200, 100, 64, 128)),                                                    # exactly 64 x 128: copy
        (2, (300, 150, 128, 256)),                                                   # exactly 128 x 256: area mean
    ]
    frame_of = np.array([f for f, _ in boxes], np.int32)
    tlwh = np.array([b for _, b in boxes], F32)
    want = []
    for f, b in zip(frame_of, tlwh):                                 # on the CPU first: the oracle accepts every box
        x1, y1, x2, y2 = oreid.crop_boxes(b[None], *sizes[f])[0]
        assert x2 > x1 and y2 > y1, (f, b)
        want.append(oreid.preprocess_crops(frames[f], b[None])[0])
    assert tuple(oreid.crop_boxes(tlwh[3:4], *sizes[0])[0]) == (100, 30, 127, 63)
    assert tuple(oreid.crop_boxes(tlwh[5:6], *sizes[2])[0][2:] - oreid.crop_boxes(tlwh[5:6], *sizes[2])[0][:2]) == (64, 128)
    assert tuple(oreid.crop_boxes(tlwh[6:7], *sizes[2])[0][2:] - oreid.crop_boxes(tlwh[6:7], *sizes[2])[0][:2]) == (128, 256)
    got = _extractor().preprocess_mixed(frames, tlwh, frame_of)
    for d in range(len(boxes)):
        assert np.array_equal(got[d], want[d]), boxes[d]


# ------------------------------------------------------------------------------------------------ helpers of 3 and 4
def _scripted(heads, hw, tlwh0, vel, n):
    """n frames of scripted detections: boxes tlwh0 [k,4] moving by vel [k,2] pixels per frame -> head rows per frame"""
    out = []
    for t in range(n):
        b = np.array(tlwh0, np.float64)
        b[:, :2] += np.array(vel, np.float64) * t
        out.append(synth.head_injection(b.astype(F32), hw, IMG, heads))
    return out


def _steps(pipe, net, n_steps, sets, call, ahead=True):
    """Runs n_steps steps with injection set i selected for step i (the look-ahead pass takes set i + 1): call(i, has_next, select_next)"""
    from yolo_deepsort_amd import pipeline as pl
    pl.load_injection_sets(net, sets)
    sel, res = None, []
    for i in range(n_steps):
        if sel != i:
            pl.select_injection_set(net, i)
        nxt = ahead and i + 1 < n_steps
        res.append(call(i, nxt, i + 1 if nxt else None))
        sel = i + 1 if nxt else None
    return res


# ------------------------------------------------------------------------------------------------ 3. uniform layout, both entries
def test_uniform_layout_through_the_mixed_entry_equals_step():
    """6 steps of 4 frames (2 streams, 2 frames each) of one size: the uniform entry on the stack, the mixed entry on the same bytes with
    off = n * h * w * 3, two tracker sets cloned from one DeepSort, next frames handed over early in both.  Rows and counts are equal."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    net = _net()
    heads = net.yolo_heads()
    h, w, T = 480, 640, 12
    scenes = [synth.PersonScene(6, frame_hw=(h, w), seed=31 + s, occlude_frac=0.1) for s in range(2)]
    order = [[(s, 2 * i + k) for s in range(2) for k in range(2)] for i in range(T // 2)]
    stacks = [np.stack([scenes[s].frame(t) for s, t in st]) for st in order]
    sets = [[synth.head_injection(scenes[s].boxes(t)[1], (h, w), IMG, heads) for s, t in st] + [EMPTY] * (net.batch_max - 4) for st in order]
    devs = [_lib.DeviceBuffer.from_array(a) for a in stacks]
    ids = [s for s, _ in order[0]]
    off = np.arange(4, dtype=np.uint64) * np.uint64(h * w * 3)
    hw = np.array([[h, w]] * 4, np.int32)
    base = _deepsort()
    uni = pl.MultiStreamPipeline(net, [base.clone(), base.clone()], 0.5, 0.4)
    a = _steps(uni, net, len(order), sets, lambda i, nxt, sn: uni.step(devs[i].ptr, h, w, ids, devs[i + 1].ptr if nxt else None, select_next=sn))
    mix = pl.MultiStreamPipeline(net, [base.clone(), base.clone()], 0.5, 0.4)
    b = _steps(mix, net, len(order), sets, lambda i, nxt, sn: mix.step_mixed(devs[i].ptr, off, hw, ids, stacks[i].nbytes,
                                                                            devs[i + 1].ptr if nxt else None, select_next=sn))
    rows = 0
    for i, (oa, ob) in enumerate(zip(a, b)):
        for k, (ra, rb) in enumerate(zip(oa, ob)):
            assert (ra is None) == (rb is None), (i, k)
            if ra is not None:
                assert ra.dtype == rb.dtype == np.int32 and ra.shape == rb.shape and np.array_equal(ra, rb), (i, k)
                rows += len(ra)
    assert rows > 40


# ------------------------------------------------------------------------------------------------ 4. mixed step vs each stream alone
SIZES4 = ((480, 640), (270, 480), (416, 416))
N4 = 8
# scripted boxes per stream (tlwh in that stream's own pixels) and their motion; the last box of the smallest stream hangs over its
# right and bottom border (x2 = 500 > 479, y2 = 290 > 269) and stays there
BOXES4 = (
    ([(40, 60, 60, 150), (250, 200, 70, 180), (470, 90, 55, 140)], [(2, 1), (-2, 1), (1, -1)]),
    ([(30, 40, 50, 120), (200, 100, 45, 110), (430, 150, 70, 140)], [(2, 1), (-1, 0.5), (0, 0)]),
    ([(50, 50, 60, 160), (220, 180, 80, 190)], [(1, 2), (-2, -1)]),
)


@functools.lru_cache(maxsize=None)
def _case4():
    """Clips built like tests/test_gpu_multi_stream.py _clips() at three sizes, the scripted head rows, and - computed ONCE - what each
    stream gives alone through the single-stream Pipeline (batch 1, a fresh clone) at its own size."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    net = _net()
    heads = net.yolo_heads()
    clips, injs = [], []
    for s, (h, w) in enumerate(SIZES4):
        base = np.random.RandomState(41 + s).randint(0, 256, (h, w, 3)).astype(np.uint8)
        clips.append([np.roll(base, 3 * t, axis=1) for t in range(N4)])
        injs.append(_scripted(heads, (h, w), BOXES4[s][0], BOXES4[s][1], N4))
    alone = []
    for s, (h, w) in enumerate(SIZES4):
        pl.load_injection_sets(net, [[r] + [EMPTY] * (net.batch_max - 1) for r in injs[s]])
        pipe = pl.Pipeline(net, _deepsort(), 0.5, 0.4)
        out = []
        for t, f in enumerate(clips[s]):
            pl.select_injection_set(net, t)
            dev = _lib.DeviceBuffer.from_array(np.ascontiguousarray(f[None]))
            out.append(pipe.step(dev.ptr, h, w, 1)[0])
        alone.append(out)
    # the reference alone is not empty: every stream yields tracked rows, and a box of the smallest stream reaches its border
    for s, out in enumerate(alone):
        assert sum(0 if o is None else len(o) for o in out) >= 4, s
    h, w = SIZES4[1]
    assert any(o is not None and len(o) and ((o[:, 2] >= w - 1) | (o[:, 3] >= h - 1)).any() for o in alone[1])
    return clips, injs, alone


@pytest.mark.parametrize("variant", ["device", "device_lookahead", "host_lookahead", "device_bgr"])
def test_mixed_step_equals_each_stream_alone(variant):
    """Three cameras (480 x 640, 270 x 480, 416 x 416), one frame of each per step for 8 steps through ONE mixed step: per stream the
    rows are those of the stream alone at its own size - ids and classes exact, boxes within 1 (the allowance
    test_detect_streams_equals_detect_per_clip makes for another batch composition)."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    net = _net()
    clips, injs, alone = _case4()
    bgr = variant == "device_bgr"
    host = variant.startswith("host")
    ahead = variant.endswith("lookahead")
    packs = [_layout([np.ascontiguousarray(clips[s][t][:, :, ::-1]) if bgr else clips[s][t] for s in range(3)]) for t in range(N4)]
    sets = [[injs[s][t] for s in range(3)] + [EMPTY] * (net.batch_max - 3) for t in range(N4)]
    base = _deepsort()
    pipe = pl.MultiStreamPipeline(net, [base.clone() for _ in range(3)], 0.5, 0.4)
    pipe.set_frame_order(bgr)
    if host:
        pins = [_lib.PinnedArray.from_array(p[0]) for p in packs]
        run = lambda i, nxt, sn: pipe.step_host_mixed((pins[i].array, packs[i][1], packs[i][2]), [0, 1, 2],      # noqa: E731
                                                      (pins[i + 1].array, packs[i + 1][1], packs[i + 1][2]) if nxt else None, select_next=sn)
    else:
        devs = [_lib.DeviceBuffer.from_array(p[0]) for p in packs]
        run = lambda i, nxt, sn: pipe.step_mixed(devs[i].ptr, packs[i][1], packs[i][2], [0, 1, 2], packs[i][0].nbytes,      # noqa: E731
                                                 devs[i + 1].ptr if nxt else None, select_next=sn)
    got = _steps(pipe, net, N4, sets, run, ahead=ahead)
    rows = [0, 0, 0]
    for t in range(N4):
        for s in range(3):
            o, want = got[t][s], alone[s][t]
            assert (o is None) == (want is None), (variant, s, t)
            if o is None:
                continue
            assert o.shape == want.shape and np.array_equal(o[:, 4:], want[:, 4:]), (variant, s, t)
            assert np.abs(o[:, :4] - want[:, :4]).max(initial=0) <= 1, (variant, s, t)
            rows[s] += len(o)
    assert min(rows) >= 4, rows
    h, w = SIZES4[1]
    assert any(got[t][1] is not None and len(got[t][1]) and ((got[t][1][:, 2] >= w - 1) | (got[t][1][:, 3] >= h - 1)).any() for t in range(N4))


# ------------------------------------------------------------------------------------------------ 5. VideoDetector.detect_streams
def _video_detector(tmp_path, net, tracker, **kw):
    from yolo_deepsort_amd.detect import VideoDetector
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())
    return VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=tracker, **kw)


def _clips5():
    clips = []
    for seed, n, (h, w) in ((21, 15, (480, 640)), (22, 5, (270, 480)), (23, 11, (416, 416))):
        base = np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
        clips.append([np.roll(base, 3 * t, axis=1) for t in range(n)])
    return clips


def test_detect_streams_mixed_sizes_equals_detect_per_clip(tmp_path):
    """Three in-memory clips of three sizes and lengths through detect_streams(mixed_sizes=True), skip_frames=2 and a class mask: per
    stream the (image, rows, actions) items equal what detect() yields on that clip alone with a fresh clone (the comparison of
    tests/test_gpu_multi_stream.py test 5); the short clip drops out while the others go on."""
    from yolo_deepsort_amd.deep_sort import DeepSort
    net = _net(-1.45, 4)                                              # a handful of (random) detections per frame
    base = DeepSort(synth.reid_state_dict(0), use_cuda=True, **DS)
    clips = _clips5()
    kw = dict(skip_frames=2, class_mask=list(range(0, 80, 2)))
    vd = _video_detector(tmp_path, net, base, **kw)
    steps = list(vd.detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True))
    alone = []
    for clip in clips:
        vd = _video_detector(tmp_path, net, base.clone(), **kw)
        alone.append(list(vd.detect(clip, show_fps=False)))
    per = [[] for _ in clips]
    for step in steps:
        assert [s for s, *_ in step] == sorted(s for s, *_ in step)
        for s, img, det, act in step:
            per[s].append((img, det, act))
    assert {s for s, *_ in steps[-1]} == {0} and any({s for s, *_ in st} == {0, 1, 2} for st in steps)
    assert any({s for s, *_ in st} == {0, 2} for st in steps)         # clip 1 has ended, the two others go on
    rows = 0
    for s, clip in enumerate(clips):
        assert len(per[s]) == len(alone[s]) == len(clip)
        for k, ((img, det, act), (wimg, wdet, wact)) in enumerate(zip(per[s], alone[s])):
            assert act == wact == [], (s, k)
            assert img.shape == clip[k].shape and (det is None) == (wdet is None), (s, k)
            if det is None:
                continue
            d, wd = np.array(det, np.int32).reshape(-1, 6), np.array(wdet, np.int32).reshape(-1, 6)
            assert d.shape == wd.shape and np.array_equal(d[:, 4:], wd[:, 4:]), (s, k)
            assert np.abs(d[:, :4] - wd[:, :4]).max(initial=0) <= 1, (s, k)
            if np.array_equal(d, wd):
                assert np.array_equal(img, wimg), (s, k)
            rows += len(d)
    assert rows > 0


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_mixed_refusals_leave_the_pipeline_usable(tmp_path):
    """Every wrong layout is stopped on the host (ValueError or YdsError) before anything is enqueued; the pipeline steps afterwards."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    net = _net(-4.0, 2)
    base = _deepsort()
    pipe = pl.MultiStreamPipeline(net, [base.clone(), base.clone()])
    frames = [np.zeros((96, 128, 3), np.uint8), np.zeros((64, 100, 3), np.uint8)]
    block, off, hw = _layout(frames)
    dev = _lib.DeviceBuffer.from_array(block)

    def ok():
        assert len(pipe.step_mixed(dev.ptr, off, hw, [0, 1], block.nbytes)) == 2

    ok()
    with pytest.raises(_lib.YdsError, match="ends past"):             # the last frame runs past the buffer
        pipe.step_mixed(dev.ptr, off, hw, [0, 1], block.nbytes - 1)
    ok()
    with pytest.raises(_lib.YdsError, match="ends past"):
        pipe.step_mixed(dev.ptr, off + np.uint64(1), hw, [0, 1], block.nbytes)
    ok()
    with pytest.raises(_lib.YdsError, match="0 x 100"):               # h = 0
        pipe.step_mixed(dev.ptr, off, np.array([[96, 128], [0, 100]], np.int32), [0, 1], block.nbytes)
    ok()
    with pytest.raises(ValueError, match="batch_max"):                # more frames than the detector takes
        pipe.step_mixed(dev.ptr, [0, 0, 0], [[64, 100]] * 3, [0, 1, 1], block.nbytes)
    with pytest.raises(ValueError, match="sizes"):                    # a frame_hw of the wrong length
        pipe.step_mixed(dev.ptr, off, hw[:1], [0, 1], block.nbytes)
    with pytest.raises(ValueError, match="sizes"):
        pipe.step_mixed(dev.ptr, off[:1], hw, [0, 1], block.nbytes)
    ok()
    pipe.set_windows((64, 64), 0.15)                                  # window mode cuts frames of one size
    with pytest.raises(_lib.YdsError, match="window mode"):
        pipe.step_mixed(dev.ptr, off, hw, [0, 1], block.nbytes)
    with pytest.raises(_lib.YdsError, match="window mode"):
        pipe.step_host_mixed(frames, [0, 1])
    pipe.set_windows(None)
    ok()
    assert len(pipe.step_host_mixed(frames, [1, 0])) == 2
    vd = _video_detector(tmp_path, net, base)
    a, b = np.zeros((96, 128, 3), np.uint8), np.zeros((64, 128, 3), np.uint8)
    with pytest.raises(ValueError, match="stream 1"):                 # a stream that changes its size midway
        list(vd.detect_streams([[a, a, a], [b, b, a]], frames_per_stream=1, show_fps=False, mixed_sizes=True))
    with pytest.raises(ValueError, match="win_size"):
        list(_video_detector(tmp_path, net, base, win_size=(64, 64)).detect_streams([[a], [b]], show_fps=False, mixed_sizes=True))
    ok()
