"""The output stage for frames of DIFFERENT sizes in one device buffer (csrc/overlay.hip, csrc/anonymize.hip: yds_overlay_tracks_mixed,
yds_overlay_tracks_bgr_mixed, yds_anonymize_frames_mixed) against the per-frame host definition - privacy.anonymize, then label_draw,
then the channel reversal, then put_text - BIT FOR BIT, each frame at its own size.

One block holds 5 x 7, 33 x 50, 64 x 64, 36 x 48, 1300 x 16, 720 x 1280 and 1080 x 1920 frames twice over: packed back to back (the
5 x 7 frame's 105 bytes leave every later frame at an odd address: only byte accesses are legal) and at 256-byte-aligned offsets
(where the 16-byte copy and the dword mask paths engage): both must give the same bits."""
import numpy as np
import pytest

from yolo_deepsort_amd import cfgs
from yolo_deepsort_amd.label_draw import put_text
from yolo_deepsort_amd.privacy import Anonymize, DeviceAnonymizer, anonymize, mask_rects

pytestmark = pytest.mark.gpu
SIZES = [(5, 7), (33, 50), (64, 64), (36, 48), (1300, 16), (720, 1280), (1080, 1920)]
HEAD, GUARD = 512, 4096            # bytes in front of the first frame / behind the end of a buffer: never written
_shared = {}


def _classes():
    return cfgs.coco_names_text().split("\n")[:-1]


def _frames():
    if "frames" not in _shared:
        rng = np.random.RandomState(11)
        _shared["frames"] = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
        for f in _shared["frames"]:
            f.setflags(write=False)
    return _shared["frames"]


def _layout(kind, sizes=SIZES):
    """Byte offsets of the frames inside one buffer, and the buffer's size: 'packed' = back to back from HEAD + 0 (HEAD is a
    multiple of 256, so the first frame is aligned and every frame behind the 105 bytes of 5 x 7 is not), 'aligned' = every frame
    at the next multiple of 256."""
    off, at = [], HEAD
    for h, w in sizes:
        if kind == "aligned":
            at = (at + 255) // 256 * 256
        off.append(at)
        at += 3 * h * w
    return np.array(off, np.uint64), at + GUARD


def _block(frames, off, nbytes, fill=0xA5):
    block = np.full(nbytes, fill, np.uint8)
    for f, o in zip(frames, off.tolist()):
        block[o:o + f.size] = f.reshape(-1)
    return block


def _rows(h, w):
    """Tracker rows of one h x w frame: partly outside, wholly outside, a box valid for the 1080p frame (placed in every frame),
    label plates clipped at the top and at the right, and two overlapping boxes of different colours, the later over the earlier."""
    return np.array([[-3, -2, w // 2, h // 2, 1, 0],
                     [w + 5, h + 5, w + 50, h + 40, 2, 1],
                     [900, 500, 1500, 1000, 3, 2],
                     [1, 2, w // 3 + 1, h // 3 + 2, 4, 0],
                     [w - 5, h // 2, w + 10, h - 1, 5, 3],
                     [w // 4, h // 4, 3 * w // 4, 3 * h // 4, 6, 0],
                     [w // 3, h // 3, 2 * w // 3, 2 * h // 3, 7, 5]], np.int32)


def _dets(h, w, m):
    """Post-NMS detections x, y, w, h, class: on tile seams (x = 64, y = 64), on the frame's edges, fractional corners."""
    return np.array([[62.5, 61.25, 4.0, 5.5, 0], [w - 3.5, h - 2.5, 9.0, 9.0, 0], [-4.0, -4.0, 6.0, 6.0, 0],
                     [w / 3 + 0.25, h / 3 + 0.75, 2.5 * m, 1.5 * m + 0.5, 0], [1.5, 2.5, 3.0, 2.0, 2]], np.float32)


def _host(drawer, frame_rgb, hold, det, anon, fps, only_rect=False):
    """The definition: mask, draw, reverse, FPS text - on ONE frame of its own size."""
    img = frame_rgb.copy()
    if anon is not None:
        rects = mask_rects(anon, img.shape[0], img.shape[1], hold, det)
        if rects:
            img = anonymize(img, rects, anon)
    if hold is not None and len(hold):
        drawer.draw_labels_by_trackers(img, hold, only_rect)
    out = np.ascontiguousarray(img[:, :, ::-1])
    if fps:
        put_text(out, fps, (3, 15), 2, (255, 0, 0))
    return out


def _back(dev, nbytes):
    from yolo_deepsort_amd import _lib
    back = np.zeros(nbytes, np.uint8)
    _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(back), dev.ptr, nbytes))
    return back


def _guarded_out(ov, out_bytes):
    """An output buffer that reports out_bytes and owns GUARD bytes more, preset to a pattern the call must leave alone."""
    from yolo_deepsort_amd import _lib
    buf = _lib.DeviceBuffer.from_array(np.full(out_bytes + GUARD, 0x3C, np.uint8))
    buf.nbytes = out_bytes
    ov._out_dev = buf
    return buf


def _same_outside(back, block, off, sizes, touched):
    """Every byte of the buffer outside the frames named in `touched` is what was uploaded: head, gaps, guard, unnamed frames."""
    keep = np.ones(block.size, bool)
    for j in touched:
        keep[int(off[j]):int(off[j]) + 3 * sizes[j][0] * sizes[j][1]] = False
    return np.array_equal(back[keep], block[keep])


ORDER = [6, 0, 3, 5, 1, 4, 2]                  # an output order that permutes the slots
FPS = ["FPS: 31", None, "FPS: 7", None, None, "FPS: 120", None]


@pytest.mark.parametrize("thickness, only_rect", [(1, False), (2, False), (3, False), (-1, False), (2, True)])
def test_draw_and_copy_equal_host_on_both_layouts(thickness, only_rect):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    frames = _frames()
    drawer = LabelDrawer(_classes(), None, 10, thickness, (608, 608))
    ov = DeviceOverlay(drawer)
    holds = [_rows(*SIZES[s]) for s in ORDER]
    holds[2] = None                              # a frame with nothing drawn ...
    holds[4] = []                                # ... and one whose tracker returned no row
    key = ("want", thickness, only_rect)
    if key not in _shared:
        _shared[key] = [_host(drawer, frames[s], holds[i], None, None, FPS[i], only_rect) for i, s in enumerate(ORDER)]
    want = _shared[key]
    rgb_order = ORDER + [5]                      # the reversed copy may show one staged frame twice, with other rows
    rgb_holds, rgb_fps = holds + [_rows(*SIZES[5])[:2]], FPS + ["FPS: 2"]
    want_twice = _host(drawer, frames[5], rgb_holds[-1], None, None, "FPS: 2", only_rect)
    hw = np.array(SIZES, np.int32)
    for kind in ("packed", "aligned"):
        off, nbytes = _layout(kind)
        block = _block(frames, off, nbytes)
        # RGB staged frames -> reversed copies, packed in output order
        dev = _lib.DeviceBuffer.from_array(block)
        out_bytes = sum(w.size for w in want) + want_twice.size
        guard = _guarded_out(ov, out_bytes)
        got = ov.render_mixed(dev.offset(0), nbytes, off, hw, rgb_order, rgb_holds, rgb_fps, only_rect=only_rect)
        for i, (g, w) in enumerate(zip(got, want + [want_twice])):
            assert g.shape == w.shape and g.dtype == np.uint8
            assert np.array_equal(g, w), ("rgb", kind, thickness, i, rgb_order[i], int((g != w).any(-1).sum()))
        assert np.array_equal(_back(dev, nbytes), block)                               # the staged frames are only read
        guard.nbytes = out_bytes + GUARD
        assert (_back(guard, out_bytes + GUARD)[out_bytes:] == 0x3C).all()              # nothing past the end of out_dev
        # BGR staged frames: drawn on in place, results leave in output order
        bgr_block = _block([np.ascontiguousarray(f[..., ::-1]) for f in frames], off, nbytes)
        dev = _lib.DeviceBuffer.from_array(bgr_block)
        got = ov.render_mixed(dev.offset(0), nbytes, off, hw, ORDER[:5], holds[:5], FPS[:5], only_rect=only_rect, bgr=True)
        for i, (g, w) in enumerate(zip(got, want[:5])):
            assert np.array_equal(g, w), ("bgr", kind, thickness, i, ORDER[i], int((g != w).any(-1).sum()))
        back = _back(dev, nbytes)
        assert _same_outside(back, bgr_block, off, SIZES, ORDER[:5])                   # head, gaps, guard, frames 4 and 2
        for i, s in enumerate(ORDER[:5]):                                              # in place means in place
            assert np.array_equal(back[int(off[s]):int(off[s]) + want[i].size], want[i].reshape(-1))


def test_copy_takes_the_dword_path_behind_a_twelve_byte_output():
    """The outputs are packed, so a 2 x 2 frame (12 bytes) in front leaves every later output at a 4-aligned address that is not
    16-aligned: with 256-aligned sources those copies walk the dword path - 33 x 50 (4950 bytes) with a tail of two pixels."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    sizes = [(2, 2), (36, 48), (33, 50), (64, 64)]
    rng = np.random.RandomState(8)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    off, nbytes = _layout("aligned", sizes)
    assert (off % 256 == 0).all()
    drawer = LabelDrawer(_classes(), None, 10, 2, (608, 608))
    ov = DeviceOverlay(drawer)
    dev = _lib.DeviceBuffer.from_array(_block(frames, off, nbytes))
    holds = [None, _rows(36, 48), None, _rows(64, 64)[:1]]
    t = ov.mixed_tables(sizes, [0, 1, 2, 3], holds)
    assert [int(o) % 16 for o in t["out_off"][1:]] == [12, 12, 2] and [int(o) % 4 for o in t["out_off"][1:]] == [0, 0, 2]
    out_bytes = t["out_bytes"]
    guard = _guarded_out(ov, out_bytes)
    assert guard.ptr % 16 == 0
    got = ov.render_mixed(dev.offset(0), nbytes, off, np.array(sizes, np.int32), [0, 1, 2, 3], holds)
    for i, g in enumerate(got):
        w = _host(drawer, frames[i], holds[i], None, None, None)
        assert np.array_equal(g, w), (i, int((g != w).any(-1).sum()))
    guard.nbytes = out_bytes + GUARD
    assert (_back(guard, out_bytes + GUARD)[out_bytes:] == 0x3C).all()


MASKS = [Anonymize(block=2), Anonymize(block=3), Anonymize(block=16), Anonymize(block=64),
         Anonymize(mode="fill", color=(200, 30, 5), margin=3)]


@pytest.mark.parametrize("anon", MASKS, ids=["m2", "m3", "m16", "m64", "fill"])
def test_masked_entries_equal_host_on_both_layouts(anon):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    frames = _frames()
    drawer = LabelDrawer(_classes(), None, 10, 2, (608, 608))
    ov = DeviceOverlay(drawer)
    rng = np.random.RandomState(anon.block)
    order = [5, 1, 2, 3, 4, 0] if anon.block in (2, 3) else ORDER      # (the 1080p frame at 2 x 2 cells is test_gpu_privacy's)
    holds = [_rows(*SIZES[s]) for s in order]
    dets = [_dets(SIZES[s][0], SIZES[s][1], anon.block) for s in order]
    # more than 256 rectangles in one frame (the 720p one), all from detections
    big = order.index(5)
    h1, w1 = SIZES[5]
    dets[big] = np.stack([rng.randint(-5, w1, 300) + rng.rand(300), rng.randint(-5, h1, 300) + rng.rand(300),
                        rng.randint(1, 9, 300) + rng.rand(300), rng.randint(1, 9, 300) + rng.rand(300), np.zeros(300)], 1).astype(np.float32)
    holds[2], dets[2] = np.array([[1, 1, 9, 9, 3, 2]], np.int32), None                # a frame with no rectangle: class 2 is not masked
    fps = FPS[:len(order)]
    want = [_host(drawer, frames[s], holds[i], dets[i], anon, fps[i]) for i, s in enumerate(order)]
    hw = np.array(SIZES, np.int32)
    for kind in ("packed", "aligned"):
        off, nbytes = _layout(kind)
        dev = _lib.DeviceBuffer.from_array(_block(frames, off, nbytes))
        got = ov.render_mixed(dev.offset(0), nbytes, off, hw, order, holds, fps, privacy=anon, detections=dets)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), ("rgb", kind, anon.mode, anon.block, i, order[i], int((g != w).any(-1).sum()))
        bgr_block = _block([np.ascontiguousarray(f[..., ::-1]) for f in frames], off, nbytes)
        dev = _lib.DeviceBuffer.from_array(bgr_block)
        got = ov.render_mixed(dev.offset(0), nbytes, off, hw, order, holds, fps, bgr=True, privacy=anon, detections=dets)
        for i, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), ("bgr", kind, anon.mode, anon.block, i, order[i], int((g != w).any(-1).sum()))
        assert _same_outside(_back(dev, nbytes), bgr_block, off, SIZES, order)
    # the mask did something on the frame of 300 rectangles
    assert not np.array_equal(want[big], _host(drawer, frames[5], holds[big], None, None, fps[big]))


@pytest.mark.parametrize("anon", [Anonymize(block=16), Anonymize(block=3), Anonymize(mode="fill", color=(250, 128, 3))], ids=["m16", "m3", "fill"])
def test_mask_alone_in_place(anon):
    from yolo_deepsort_amd import _lib
    _lib.init()
    frames = _frames()
    hw = np.array(SIZES, np.int32)
    slots = [6, 3, 0, 4, 1]                                                            # frames 2 and 5 are not named
    rects = []
    for s in slots:
        h, w = SIZES[s]
        rects.append([(3, 2, w // 2, h // 2), (w // 3, h // 3, w - 3, h - 2), (w - 1, 0, w + 9, 0), (-4, h - 1, 0, h + 4),
                      (60, 60, 68, 68), (63, 0, 64, h - 1)])                           # the last two sit on tile seams
    rects[1] = None                                                                    # a named frame with no rectangle
    for kind in ("packed", "aligned"):
        off, nbytes = _layout(kind)
        for bgr in (False, True):
            block = _block(frames, off, nbytes)
            dev = _lib.DeviceBuffer.from_array(block)
            DeviceAnonymizer(anon).apply_mixed(dev.offset(0), nbytes, off, hw, slots, rects, bgr=bgr)
            back = _back(dev, nbytes)
            assert _same_outside(back, block, off, SIZES, [s for s, r in zip(slots, rects) if r])
            for s, r in zip(slots, rects):
                want = anonymize(frames[s], r or [], anon, bgr=bgr)
                got = back[int(off[s]):int(off[s]) + want.size].reshape(want.shape)
                assert np.array_equal(got, want), (kind, anon.mode, anon.block, bgr, s, int((got != want).any(-1).sum()))
            assert not np.array_equal(back, block)
        # no rectangle at all: nothing is launched, nothing moves
        block = _block(frames, off, nbytes)
        dev = _lib.DeviceBuffer.from_array(block)
        DeviceAnonymizer(anon).apply_mixed(dev.offset(0), nbytes, off, hw, [0, 1, 2], [None, [], [(64, 64, 70, 70), (-9, -9, -1, -1)]])      # (both outside the 64 x 64 frame)
        assert np.array_equal(_back(dev, nbytes), block)


def test_equal_sizes_give_the_uniform_entries_bytes():
    """A layout of equal sizes at offsets i * h * w * 3 is the uniform entry's layout: the same tables give the same bytes."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    h, w, n = 120, 92, 4
    rng = np.random.RandomState(5)
    frames = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    ov = DeviceOverlay(LabelDrawer(_classes(), None, 10, 2, (608, 608)))
    holds = [_rows(h, w), None, _rows(h, w)[::-1].copy()]
    dets = [_dets(h, w, 16), _dets(h, w, 16)[:2], None]
    fps = ["FPS: 9", None, "FPS: 10"]
    off, hw = np.arange(n, dtype=np.uint64) * np.uint64(h * w * 3), np.array([(h, w)] * n, np.int32)
    for anon in (None, Anonymize(block=16), Anonymize(mode="fill", color=(9, 8, 7))):
        for bgr in (False, True):
            slots = [3, 0, 2] if bgr else [3, 0, 3]
            dev = _lib.DeviceBuffer.from_array(frames)
            a = [o.copy() for o in ov.render(dev.offset(0), slots, h, w, holds, fps, bgr_frames=n if bgr else 0, privacy=anon, detections=dets,
                                             n_frames=n)]
            back_a = _back(dev, frames.nbytes)
            dev = _lib.DeviceBuffer.from_array(frames)
            b = ov.render_mixed(dev.offset(0), frames.nbytes, off, hw, slots, holds, fps, bgr=bgr, privacy=anon, detections=dets)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (anon and anon.mode, bgr)
            assert np.array_equal(back_a, _back(dev, frames.nbytes))


def test_refusals_leave_buffers_untouched_and_the_library_usable():
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    sizes = [(5, 7), (33, 50), (36, 48)]
    rng = np.random.RandomState(3)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    off, nbytes = _layout("packed", sizes)
    block = _block(frames, off, nbytes)
    dev = _lib.DeviceBuffer.from_array(block)
    ov = DeviceOverlay(LabelDrawer(_classes(), None, 10, 2, (608, 608)))
    hw = np.array(sizes, np.int32)
    rows = [np.array([[1, 1, 5, 5, 1, 0]], np.int32)]
    anon = DeviceAnonymizer(Anonymize())
    R = [[(0, 0, 3, 3)]]

    def refused(match, call):
        with pytest.raises(_lib.YdsError, match=match):
            call()
        assert np.array_equal(_back(dev, nbytes), block)

    end = int(off[2]) + 3 * 36 * 48
    for bgr in (False, True):
        refused("past the buffer", lambda: ov.render_mixed(dev.offset(0), end - 1, off, hw, [0], rows, bgr=bgr))
        bad = hw.copy()
        bad[1, 0] = 0
        refused("0 x 50", lambda: ov.render_mixed(dev.offset(0), nbytes, off, bad, [0], rows, bgr=bgr))
        for bad_slot in (3, -1):                 # (render_mixed needs the slot's size for its tables and stops this one itself)
            with pytest.raises(ValueError, match="slots must lie in"):
                ov.render_mixed(dev.offset(0), nbytes, off, hw, [bad_slot], rows, bgr=bgr)
    lap = off.copy()
    lap[1] = off[0] + np.uint64(104)                                                   # frame 1 starts on frame 0's last byte
    refused("overlap", lambda: ov.render_mixed(dev.offset(0), nbytes, lap, hw, [0], rows, bgr=True))
    refused("overlap", lambda: anon.apply_mixed(dev.offset(0), nbytes, lap, hw, [0], R))
    refused("named twice", lambda: ov.render_mixed(dev.offset(0), nbytes, off, hw, [1, 1], rows * 2, bgr=True))
    refused("named twice", lambda: anon.apply_mixed(dev.offset(0), nbytes, off, hw, [1, 1], R * 2))
    refused("past the buffer", lambda: anon.apply_mixed(dev.offset(0), end - 1, off, hw, [0], R))
    refused("slot 3 of 3", lambda: anon.apply_mixed(dev.offset(0), nbytes, off, hw, [3], R))
    # a short out_bytes: the outputs need 3 * (33 * 50 + 5 * 7) bytes
    out_bytes = 3 * (33 * 50 + 5 * 7)
    guard = _guarded_out(ov, out_bytes)
    t = ov.mixed_tables(hw, [1, 0], rows * 2)
    assert t["out_bytes"] == out_bytes and t["out_off"].tolist() == [0, 3 * 33 * 50] and t["scales"] == [1, 1]
    host_out = np.zeros(out_bytes, np.uint8)

    def entry(slots, told, in_place=False):      # the C entries themselves (render_mixed sizes out_dev and checks the slots first)
        slots = np.array(slots, np.int32)
        head = (dev.offset(0), nbytes, 3, _lib.ptr(off), _lib.ptr(hw), _lib.ptr(slots), 2, _lib.ptr(t["boxes"]), _lib.ptr(t["box_ptr"]),
                _lib.ptr(t["text"]), t["n_text"], _lib.ptr(t["fps"]), _lib.ptr(ov.font), len(ov.font), 2, None, None, 0, 16, 0)
        if in_place:
            _lib.check(_lib.load().yds_overlay_tracks_bgr_mixed(*head, _lib.ptr(host_out)))
        else:
            _lib.check(_lib.load().yds_overlay_tracks_mixed(*head, guard.ptr, told, _lib.ptr(host_out)))
    refused("out_dev holds", lambda: entry([1, 0], out_bytes - 1))
    refused("slot 3 of 3", lambda: entry([1, 3], out_bytes))
    refused("slot -1 of 3", lambda: entry([-1, 0], out_bytes))
    refused("slot 3 of 3", lambda: entry([1, 3], 0, True))
    refused("named twice", lambda: entry([1, 1], 0, True))
    assert not host_out.any()
    guard.nbytes = out_bytes + GUARD
    assert (_back(guard, out_bytes + GUARD) == 0x3C).all()
    # ... and every entry still works
    ov._out_dev = None
    got = ov.render_mixed(dev.offset(0), nbytes, off, hw, [1, 0], rows * 2)
    assert [g.shape for g in got] == [(33, 50, 3), (5, 7, 3)]
    assert np.array_equal(got[1], _host(ov.drawer, frames[0], rows[0], None, None, None))
    anon.apply_mixed(dev.offset(0), nbytes, off, hw, [1], R)
    assert not np.array_equal(_back(dev, nbytes), block)
