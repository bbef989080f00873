"""Anonymised output on the device (csrc/anonymize.hip; the masked overlay entries, yds_anonymize_frames,
yds_pipeline_last_detections) against the host form of yolo_deepsort_amd/privacy.py, BIT FOR BIT: both entries of
DeviceOverlay.render(privacy=...) against VideoDetector._render_host, DeviceAnonymizer.apply against privacy.anonymize, the
detections a step hands out, and VideoDetector.detect(anonymize=...) with the output stage on the device against the one on the host."""
import atexit
import os
import tempfile

import numpy as np
import pytest

from yolo_deepsort_amd import cfgs, synth
from yolo_deepsort_amd.privacy import Anonymize, DeviceAnonymizer, anonymize, mask_rects

pytestmark = pytest.mark.gpu
F32 = np.float32
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
_shared = {}


def _classes():
    return cfgs.coco_names_text().split("\n")[:-1]


def _host_renderer(drawer, anon):
    from yolo_deepsort_amd.detect import VideoDetector
    vd = VideoDetector.__new__(VideoDetector)
    vd.label_drawer, vd.tracker, vd.anonymize = drawer, object(), anon
    return vd


# ---------------------------------------------------------------------------------------------- 1. the masked overlay entries
def _frame_rows(kind, h, w, m, rng):
    """(tracker rows int32 [r, 6] | None | [], detections float32 [d, 5] | None) of one output frame."""
    if kind == "none":
        return None, None
    if kind == "empty":
        return [], np.zeros((0, 5), F32)
    if kind == "whole":
        return np.array([[0, 0, w - 1, h - 1, 1, 0]], np.int32), None
    if kind == "many":                                    # 300 rectangles (more than one LDS chunk of 256), all from detections
        x, y = rng.randint(-5, w, 300), rng.randint(-5, h, 300)
        d = np.stack([x + rng.rand(300), y + rng.rand(300), rng.randint(1, max(w // 6, 3), 300) + rng.rand(300),
                      rng.randint(1, max(h // 6, 3), 300) + rng.rand(300), np.zeros(300)], 1).astype(F32)
        return np.array([[w // 4, h // 4, w // 2, h // 2, 9, 0]], np.int32), d
    assert kind == "mixed"
    rows = [[-50, -40, -3, -2, 1, 0],                     # entirely outside the frame
            [w + 2, 3, w + 30, 9, 2, 0],
            [3 * m + 1, 1, 3 * m + 1, 1, 3, 0],           # degenerate: one pixel
            [5 * m + 2, 2 * m + 2, 4 * m + 3, m + 3, 4, 0],    # inverted corners
            [m + 1, m + 1, m + 2, m + 2, 5, 0],           # smaller than a cell
            [0, 2 * m, m - 1, 3 * m - 1, 6, 0],           # ends exactly on a cell boundary ...
            [2 * m, 2 * m, 3 * m, 3 * m, 7, 0],           # ... and one pixel past it
            [6 * m + 1, m, 6 * m + 1 + m // 3, m + m // 3, 8, 0],      # three boxes sharing one cell
            [6 * m + m // 2, m + m // 4, 7 * m - 2, 2 * m - 2, 9, 0],
            [6 * m, m + m // 2, 6 * m + m // 2, 2 * m - 1, 10, 0],
            [w - 2 * m - 3, h - m - 2, w + 5, h + 5, 11, 0],           # clipped by the bottom-right corner
            [w // 2, h // 2, w // 2 + 3 * m, h // 2 + 2 * m, 12, 2]]   # another class: drawn, not masked
    d = np.array([[w / 3 + 0.25, h / 3 + 0.75, 2.5 * m, 1.5 * m + 0.5, 0],       # a person the tracker does not show yet
                  [4.0 * m, 4.0 * m, m, m, 0],                                  # integral corners: m + 1 pixels a side after ceil
                  [1.5, h - 2.5, 3.0, 9.0, 2]], F32)                             # another class
    return np.array(rows, np.int32), d


CASES = [  # h, w, m, frame kinds
    (5, 7, 16, ("mixed", "whole", "none", "many", "empty")),
    (5, 7, 2, ("mixed", "whole", "none", "many", "empty")),
    (33, 50, 16, ("mixed", "whole", "none", "many", "empty")),
    (33, 50, 3, ("mixed", "whole", "none", "many", "empty")),
    (33, 50, 64, ("mixed", "whole", "none", "many", "empty")),
    (64, 64, 16, ("mixed", "whole", "none", "many", "empty")),
    (333, 517, 16, ("mixed", "whole", "none", "many", "empty")),
    (1080, 1920, 16, ("mixed", "many", "none")),
    (1080, 1920, 2, ("whole", "mixed")),                  # two frames of 518 400 cells each
]


@pytest.mark.parametrize("h, w, m, kinds", CASES, ids=["%dx%d-m%d" % c[:3] for c in CASES])
def test_masked_overlay_equals_host_render(h, w, m, kinds):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    rng = np.random.RandomState(h + 7 * m)
    drawer = LabelDrawer(_classes(), None, 10, 2, (608, 608))
    ov = DeviceOverlay(drawer)
    n = len(kinds)
    frames = rng.randint(0, 256, (n + 1, h, w, 3)).astype(np.uint8)         # RGB; one staged frame more than is shown
    made = [_frame_rows(k, h, w, m, rng) for k in kinds]
    holds, dets = [r for r, _ in made], [d for _, d in made]
    fps = [("FPS: %d" % (10 + i) if i % 2 == 0 else None) for i in range(n)]
    slots_bgr = (list(range(1, n + 1, 2)) + list(range(0, n + 1, 2)))[:n]    # out of order, distinct: odd slots first
    assert len(set(slots_bgr)) == n
    slots_rgb = list(slots_bgr)
    slots_rgb[-1] = slots_rgb[0]                                             # the copy path may show one staged frame twice
    big = h * w > 10 ** 6
    settings = [Anonymize(block=m), Anonymize(mode="fill", color=(200, 30, 5), region="head", margin=5)]
    if not big:
        settings += [Anonymize(block=m, region="head", head_frac=(2, 3), margin=5, classes=None), Anonymize(mode="fill", color=(1, 2, 3), classes=None)]
    for anon in settings:
        host = _host_renderer(drawer, anon)
        want = {s: {} for s in range(n + 1)}

        def check(got, slots, tag):
            for i in range(n):
                key = (slots[i], i)
                if key not in want[slots[i]]:
                    want[slots[i]][key] = host._render_host(frames[slots[i]], holds[i], fps[i], dets[i])
                ref = want[slots[i]][key]
                assert got[i].shape == ref.shape and got[i].dtype == np.uint8
                assert np.array_equal(got[i], ref), (tag, anon.mode, anon.region, h, w, m, i, kinds[i], int((got[i] != ref).any(-1).sum()))
        # RGB frames: reversed device copy, mask on the copy, draw
        dev = _lib.DeviceBuffer.from_array(frames)
        check(ov.render(dev.offset(0), slots_rgb, h, w, holds, fps, privacy=anon, detections=dets, n_frames=n + 1), slots_rgb, "rgb")
        # BGR frames (a decoder's order): mask and draw in place on distinct slots
        dev = _lib.DeviceBuffer.from_array(np.ascontiguousarray(frames[..., ::-1]))
        check(ov.render(dev.offset(0), slots_bgr, h, w, holds, fps, bgr_frames=n + 1, privacy=anon, detections=dets), slots_bgr, "bgr")
        # in place means in place: the staged slots that were shown hold the results, the one that was not is untouched
        back = np.zeros_like(frames)
        _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(back), dev.ptr, back.nbytes))
        spare = (set(range(n + 1)) - set(slots_bgr)).pop()
        assert np.array_equal(back[spare], frames[spare][..., ::-1])
    # something was masked at all (a label plate may hide all of a 5 x 7 frame, so this looks at the mask alone)
    i = kinds.index("mixed")
    rects = mask_rects(Anonymize(block=m), h, w, holds[i], dets[i])
    assert rects and not np.array_equal(anonymize(frames[slots_bgr[i]], rects, Anonymize(block=m)), frames[slots_bgr[i]])


def test_masked_entries_refuse_bad_tables():
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    ov = DeviceOverlay(LabelDrawer(_classes(), None, 10, 2, (608, 608)))
    frames = np.zeros((2, 8, 8, 3), np.uint8)
    dev = _lib.DeviceBuffer.from_array(frames)
    rows = [np.array([[1, 1, 5, 5, 1, 0]], np.int32)]
    with pytest.raises(_lib.YdsError, match="slot 2 of 2"):                  # the masked RGB entry knows the staged count
        ov.render(dev.offset(0), [2], 8, 8, rows, privacy=Anonymize(), n_frames=2)
    with pytest.raises(_lib.YdsError, match="slot"):
        DeviceAnonymizer(Anonymize()).apply(dev.offset(0), [0, 0], 8, 8, [[(0, 0, 3, 3)], [(0, 0, 3, 3)]], n_frames=2)
    with pytest.raises(_lib.YdsError, match="slot"):
        DeviceAnonymizer(Anonymize()).apply(dev.offset(0), [2], 8, 8, [[(0, 0, 3, 3)]], n_frames=2)
    out = ov.render(dev.offset(0), [1], 8, 8, rows, privacy=Anonymize(), n_frames=2)   # ... and the handle stays usable
    assert out[0].shape == (8, 8, 3)


# ---------------------------------------------------------------------------------------------- 2. privacy=None is today's path
def test_privacy_none_equals_plain_render():
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    h, w = 120, 90
    rng = np.random.RandomState(2)
    ov = DeviceOverlay(LabelDrawer(_classes(), None, 10, 2, (608, 608)))
    frames = rng.randint(0, 256, (3, h, w, 3)).astype(np.uint8)
    holds = [np.array([[10, 20, 60, 100, 3, 0], [40, 5, 80, 50, 4, 2]], np.int32), None, []]
    fps = ["FPS: 9", None, "FPS: 10"]
    for bgr in (0, 3):
        outs = []
        for kw in (dict(), dict(privacy=None, detections=None), dict(privacy=Anonymize(classes=(7,)), detections=[None] * 3, n_frames=3)):
            dev = _lib.DeviceBuffer.from_array(frames)
            outs.append([o.copy() for o in ov.render(dev.offset(0), [2, 0, 1], h, w, holds, fps, bgr_frames=bgr, **kw)])
        for a, b, c in zip(*outs):
            assert np.array_equal(a, b) and np.array_equal(a, c)             # (a mask that names no class masks nothing)


# ---------------------------------------------------------------------------------------------- 3. the mask alone, in place
@pytest.mark.parametrize("h, w, m", [(33, 50, 16), (33, 50, 3), (64, 64, 16), (64, 64, 4), (120, 92, 20)])
def test_device_anonymizer_equals_host_form(h, w, m):
    from yolo_deepsort_amd import _lib
    _lib.init()
    rng = np.random.RandomState(m)
    frames = rng.randint(0, 256, (4, h, w, 3)).astype(np.uint8)
    rects = [[(3, 2, w // 2, h // 2), (w // 3, h // 3, w - 3, h - 2), (w - 1, 0, w + 9, 0), (-4, h - 1, 0, h + 4)],
             [(0, 0, w - 1, h - 1)], [(m, m, 2 * m - 1, 2 * m - 1), (m, m, 2 * m, 2 * m)] * 150]
    slots = [3, 0, 2]                                                        # slot 1 must stay as it is
    for anon in (Anonymize(block=m), Anonymize(mode="fill", color=(250, 128, 3))):
        for bgr in (False, True):
            dev = _lib.DeviceBuffer.from_array(frames)
            DeviceAnonymizer(anon).apply(dev.offset(0), slots, h, w, rects, n_frames=4, bgr=bgr)
            back = np.zeros_like(frames)
            _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(back), dev.ptr, back.nbytes))
            assert np.array_equal(back[1], frames[1])
            for s, r in zip(slots, rects):
                want = anonymize(frames[s], r, anon, bgr=bgr)
                assert np.array_equal(back[s], want), (h, w, m, anon.mode, bgr, s, int((back[s] != want).any(-1).sum()))
            assert not np.array_equal(back[0], frames[0])
    # frames that start at an odd address: rows of W % 4 == 0 pixels are 4-aligned only relative to the base, so the byte path must run
    raw = _lib.DeviceBuffer(frames.nbytes + 4)
    _lib.check(_lib.load().yds_memcpy_h2d(raw.offset(1), _lib.ptr(frames), frames.nbytes))
    DeviceAnonymizer(Anonymize(block=m)).apply(raw.offset(1), slots, h, w, rects, n_frames=4)
    back = np.zeros_like(frames)
    _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(back), raw.offset(1), back.nbytes))
    for s, r in zip(slots, rects):
        assert np.array_equal(back[s], anonymize(frames[s], r, Anonymize(block=m))), (h, w, m, s)
    # no rectangle, rectangles outside the frame, None: nothing moves
    dev = _lib.DeviceBuffer.from_array(frames)
    DeviceAnonymizer(Anonymize(block=m)).apply(dev.offset(0), [0, 1, 2], h, w, [None, [], [(w, h, w + 9, h + 9), (-9, -9, -1, -1)]])
    back = np.zeros_like(frames)
    _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(back), dev.ptr, back.nbytes))
    assert np.array_equal(back, frames)


# ---------------------------------------------------------------------------------------------- 4. the detections of a step
SIZE, WIN, OVERLAP = 416, (416, 416), 0.15
EMPTY = np.zeros((0, 9), F32)
WINDOWS_480x640 = [(0, 0, 478, 478), (0, 416, 64, 478), (416, 0, 478, 224), (416, 416, 64, 224)]    # img_detect.py:103-121 for 480 x 640


def _cfg():
    return cfgs.cfg_text("yolov3-tiny", SIZE, SIZE)


def _net(blob, batch_max):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    net = Darknet(None, img_size=(SIZE, SIZE), batch_max=batch_max, cfg_text=_cfg())
    net.load_darknet_weights(None, blob=blob)
    return net


def _deepsort():
    from yolo_deepsort_amd.deep_sort import DeepSort
    if "ex" not in _shared:
        _shared["ex"] = DeepSort(synth.reid_state_dict(0), use_cuda=True, **DS).extractor
    return DeepSort(_shared["ex"], use_cuda=True, **DS)


def _scripted_frame(t, empty):
    """Persons (tlwh, class) of frame t of a scripted 480 x 640 scene (the one of tests/test_gpu_window_pipeline.py)."""
    if empty:
        return [], []
    persons = [((50 + 3 * t, 100 + 2 * t, 50, 120), 0), ((300 - 2 * t, 250 + t, 60, 150), 2), ((425 + t, 150 + 2 * t, 35, 100), 0),
               ((520 + 3 * t, 60 + t, 60, 140), 2), ((100 + 2 * t, 424, 30, 45), 0)]
    return [p for p, _ in persons], [c for _, c in persons]


def _scene_frame(t, tlwh):
    rng = np.random.RandomState(100 + t)
    img = np.repeat(np.repeat(rng.randint(0, 256, (60, 80, 3)), 8, 0), 8, 1).astype(np.uint8)
    for x, y, w, h in tlwh:
        patch = np.random.RandomState(7 + int(w) * 31 + int(h)).randint(0, 256, (8, 4, 3)).astype(np.uint8)
        yy = (np.arange(int(h)) * 8 // int(h)).clip(0, 7)
        xx = (np.arange(int(w)) * 4 // int(w)).clip(0, 3)
        img[int(y):int(y) + int(h), int(x):int(x) + int(w)] = patch[yy][:, xx]
    return img


def _window_tables(tlwh, cls, heads):
    tables = []
    for x0, y0, th, tw in WINDOWS_480x640:
        inside = [i for i, (x, y, w, h) in enumerate(tlwh) if x >= x0 and y >= y0 and x + w <= x0 + tw and y + h <= y0 + th]
        if not inside:
            tables.append(EMPTY)
            continue
        local = np.array([[tlwh[i][0] - x0, tlwh[i][1] - y0, tlwh[i][2], tlwh[i][3]] for i in inside], F32)
        rows = synth.head_injection(local, (th, tw), (SIZE, SIZE), heads)
        rows[:, 8] = [cls[i] for i in inside]
        tables.append(rows)
    return tables


def _overlaps(row, det):
    return min(row[2], det[0] + det[2]) > max(row[0], det[0]) and min(row[3], det[1] + det[3]) > max(row[1], det[1])


def test_last_detections_of_plain_and_window_steps():
    """Per frame of a step: the post-NMS, class-masked detections the tracker was handed.  Plain steps and window-mode steps of the
    same scripted frames return the same persons: the scripted boxes, to within half a pixel (the decode is fp32 arithmetic on
    boxes of some hundred pixels: errors of 1e-3 pixels; a wrong window shift or frame scale would be tens of pixels)."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    B, T, steps, mask = 3, 4, 2, [0, 4]
    blob = synth.darknet_weights_blob(_cfg(), 0, -30.0)
    scripted = [_scripted_frame(t, empty=(t == 4)) for t in range(B * steps)]
    frames = np.stack([_scene_frame(t, tlwh) for t, (tlwh, _) in enumerate(scripted)], 0)
    per_mode = []
    for windows in (False, True):
        net = _net(blob, B * T if windows else B)
        heads = net.yolo_heads()
        if windows:
            sets = [[tab for b in range(B) for tab in _window_tables(*scripted[s * B + b], heads)] for s in range(steps)]
        else:
            sets = []
            for s in range(steps):
                sets.append([])
                for tlwh, cls in scripted[s * B:(s + 1) * B]:
                    rows = synth.head_injection(np.array(tlwh, F32).reshape(-1, 4), (480, 640), (SIZE, SIZE), heads) if tlwh else EMPTY
                    if len(rows):
                        rows[:, 8] = cls
                    sets[-1].append(rows)
        pl.load_injection_sets(net, sets)
        pl.select_injection_set(net, 0)
        pipe = pl.Pipeline(net, _deepsort(), 0.5, 0.4, class_mask=mask, win_size=WIN if windows else None, overlap=OVERLAP)
        assert pipe.last_detections() is None                                # no step has run
        dev = _lib.DeviceBuffer.from_array(frames)
        outs, dets = [], []
        for s in range(steps):
            nxt = dev.offset((s + 1) * B * frames[0].nbytes) if s + 1 < steps else None
            outs += pipe.step(dev.offset(s * B * frames[0].nbytes), 480, 640, B, nxt, select_next=(s + 1 if nxt is not None else None))
            d = pipe.last_detections()
            assert len(d) == B and all(x.dtype == np.float32 and x.ndim == 2 and x.shape[1] == 5 for x in d)
            dets += d
        for t, (o, d) in enumerate(zip(outs, dets)):
            tlwh, cls = scripted[t]
            want = sorted([list(b) + [c] for b, c in zip(tlwh, cls) if c in mask])
            assert (o is None) == (len(want) == 0) == (len(d) == 0), (windows, t, o, d)      # the step's None / rows pattern
            got = sorted(d.astype(np.float64).tolist())
            assert len(got) == len(want), (windows, t, got, want)                          # class 2 is masked out, duplicates of two windows merged
            assert np.abs(np.array(got).reshape(-1, 5) - np.array(want, np.float64).reshape(-1, 5)).max(initial=0) < 0.5, (windows, t, got, want)
            for row in (o if o is not None else []):                                        # every tracker row overlaps a detection of its frame
                assert any(_overlaps(row, x) for x in d), (windows, t, row, d)
        assert sum(len(o) for o in outs if o is not None) >= 3                              # tracks were confirmed and shown
        per_mode.append(dets)
    for a, b in zip(*per_mode):
        assert a.shape == b.shape
        assert np.abs(np.sort(a, 0) - np.sort(b, 0)).max(initial=0) < 0.5


# ---------------------------------------------------------------------------------------------- 5. the generator
class Capture:
    """cv2.VideoCapture protocol over an in-memory BGR clip (the one of tests/test_gpu_video_detect.py)."""

    def __init__(self, frames_bgr, fps):
        self.frames, self.fps, self.pos = frames_bgr, fps, 0

    def isOpened(self):
        return True

    def get(self, prop):
        n, h, w = self.frames.shape[:3]
        return {5: self.fps, 6: 0.0, 3: float(w), 4: float(h), 7: float(n), 1: float(self.pos)}[prop]

    def set(self, prop, value):
        self.pos = int(value)

    def read(self):
        if self.pos >= len(self.frames):
            return False, None
        f = np.array(self.frames[self.pos])
        self.pos += 1
        return True, f

    def release(self):
        pass


class CountingActions:
    def __init__(self):
        self.calls = 0

    def update(self, rows):
        self.calls += 1
        return [[self.calls, len(rows)]]


def _names():
    if "names" not in _shared:
        with tempfile.NamedTemporaryFile("w", suffix=".names", delete=False) as f:
            f.write(cfgs.coco_names_text())
        _shared["names"] = f.name
        atexit.register(os.unlink, f.name)
    return _shared["names"]


def _run_clip(frames, boxes, classes, anon, device_overlay):
    """VideoDetector.detect over the clip: 4 processed frames per step, every second frame processed."""
    from yolo_deepsort_amd import pipeline as pl
    from yolo_deepsort_amd.detect import VideoDetector
    B, hw = 4, frames.shape[1:3]
    net = _net(synth.darknet_weights_blob(_cfg(), seed=0), B)
    heads = net.yolo_heads()
    inj = []
    for b, k in zip(boxes, classes):
        rows = synth.head_injection(b, hw, (SIZE, SIZE), heads)
        rows[:, 8] = k
        inj.append(rows)
    tracker = _deepsort()
    vd = VideoDetector(net, _names(), thres=0.5, nms_thres=0.4, skip_frames=2, class_mask=[0, 2], tracker=tracker, action_id=CountingActions(),
                       batch_frames=B, device_overlay=device_overlay, anonymize=anon)
    index = {hash(f.tobytes()): t for t, f in enumerate(frames)}
    groups = [[index[hash(np.ascontiguousarray(f).tobytes())] for f, proc in grp if proc]
              for grp in vd._processed_batches(Capture(frames[..., ::-1], 25.0), 0)]
    pl.load_injection_sets(net, [[inj[t] for t in grp] + [EMPTY] * (B - len(grp)) for grp in groups])

    class InjectingPipeline(pl.Pipeline):
        i, sel = 0, None

        def step(self, frames_dev, h, w, batch, next_frames_dev=None, select_next=None):
            if self.sel != self.i:
                pl.select_injection_set(net, self.i)
            nxt = self.i + 1 if next_frames_dev is not None else None
            out = super().step(frames_dev, h, w, batch, next_frames_dev, select_next=nxt)
            self.sel, self.i = nxt, self.i + 1
            return out
    vd._pipe = InjectingPipeline(net, tracker, 0.5, 0.4, class_mask=[0, 2])
    yields = [(img.copy(), hold, acts) for img, hold, acts in vd.detect(Capture(frames[..., ::-1], 25.0), show_fps=False)]
    assert vd._pipe.i == len(groups) == 2 and len(yields) == len(frames)
    return yields


def _clip(T=12, hw=(360, 640)):
    scene = synth.PersonScene(8, frame_hw=hw, seed=5, occlude_frac=0.0)
    frames = np.stack([scene.frame(t) for t in range(T)], 0)
    boxes, classes = [], []
    for t in range(T):
        ids, tlwh = scene.boxes(t)
        if t == 6:                                                           # a processed frame on which the detector returns nothing
            ids, tlwh = ids[:0], tlwh[:0]
        boxes.append(np.asarray(tlwh, np.float64).reshape(-1, 4))
        classes.append((np.asarray(ids) % 3).astype(F32))
    return frames, boxes, classes


def test_frame_by_frame_path_masks_with_the_detections_the_tracker_was_handed():
    """batch_frames=1: the host form, with the rows x, y, w, h, class that process() handed the tracker on the last PROCESSED frame -
    held over a skipped frame like the tracker rows."""
    from yolo_deepsort_amd.detect import VideoDetector
    frames, boxes, classes = _clip()
    hw = frames.shape[1:3]
    net = _net(synth.darknet_weights_blob(_cfg(), seed=0), 1)
    heads = net.yolo_heads()
    anon = Anonymize(mode="fill", color=(255, 0, 255), margin=2)
    vd = VideoDetector(net, _names(), thres=0.5, nms_thres=0.4, skip_frames=2, class_mask=[0, 2], tracker=_deepsort(), batch_frames=1, anonymize=anon)
    index = {hash(f.tobytes()): t for t, f in enumerate(frames)}
    handed, orig_detect, orig_process = [], vd.image_detector.detect, vd.process

    def detect(frame):
        t = index[hash(np.ascontiguousarray(frame).tobytes())]
        rows = synth.head_injection(boxes[t], hw, (SIZE, SIZE), heads)
        rows[:, 8] = classes[t]
        net.set_injection(0, rows)
        return orig_detect(frame)

    def process(frame):
        out = orig_process(frame)
        handed.append((index[hash(np.ascontiguousarray(frame).tobytes())], vd._last_dets))
        return out
    vd.image_detector.detect, vd.process = detect, process
    yields = list(vd.detect(Capture(frames[..., ::-1], 25.0), show_fps=False))
    assert [t for t, _ in handed] == [0, 2, 4, 6, 8, 10] and len(yields) == len(frames)
    by_frame = dict(handed)
    assert by_frame[6] is None and by_frame[0].dtype == np.float32 and by_frame[0].shape[1] == 5
    assert set(by_frame[0][:, 4].tolist()) <= {0.0, 2.0} and (by_frame[0][:, 4] == 0).any()   # class-masked: what the tracker got
    plain = VideoDetector.__new__(VideoDetector)
    plain.label_drawer, plain.tracker, plain.anonymize = vd.label_drawer, vd.tracker, None
    masked = 0
    for t, (image, hold, _) in enumerate(yields):
        dets = by_frame[t - t % 2]
        assert np.array_equal(image, vd._render_host(frames[t], hold, None, dets)), t
        masked += int(not np.array_equal(image, plain._render_host(frames[t], hold, None)))
    assert masked >= 8 and np.array_equal(yields[7][0][..., ::-1], frames[7])                # frames 6, 7: the detector returned nothing
    assert not (yields[0][1] is not None and len(yields[0][1])) and not np.array_equal(yields[0][0][..., ::-1], frames[0])   # detection-only


def test_video_detector_anonymize_device_equals_host_and_rows_are_unchanged():
    T, hw = 12, (360, 640)
    frames, boxes, classes = _clip(T, hw)
    anon = Anonymize()
    dev = _run_clip(frames, boxes, classes, anon, True)
    host = _run_clip(frames, boxes, classes, anon, False)
    off = _run_clip(frames, boxes, classes, None, True)
    masked_with_rows = detection_only = 0
    for t in range(T):
        assert np.array_equal(dev[t][0], host[t][0]), (t, int((dev[t][0] != host[t][0]).any(-1).sum()))
        for a, b in ((dev[t], off[t]), (host[t], off[t])):                   # rows and actions do not depend on the option
            assert (a[1] is None) == (b[1] is None) and a[2] == b[2], t
            if a[1] is not None:
                assert np.array_equal(np.asarray(a[1], np.int32).reshape(-1, 6), np.asarray(b[1], np.int32).reshape(-1, 6)), t
        hold = dev[t][1]
        differs = not np.array_equal(dev[t][0], off[t][0])
        if hold is not None and len(hold) and differs:
            masked_with_rows += 1
        # masked although no tracker row of a masked class names anyone yet: the detections did it
        if differs and not mask_rects(anon, hw[0], hw[1], hold, None):
            detection_only += 1
    assert masked_with_rows >= 1
    assert detection_only >= 1, "the clip produced no frame that is masked by a detection alone (n_init = 3: the first processed frames)"
    assert dev[6][1] is None and np.array_equal(dev[6][0], off[6][0])        # the detector returned nothing: not masked
    assert np.array_equal(dev[7][0][..., ::-1], frames[7])                    # ... nor is the skipped frame that holds its (no) rows
