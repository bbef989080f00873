"""privacy.py on the host: argument checks, the mask rectangles of a frame, the numpy host form of pixelate / fill (the DEFINITION the
device form is held to, tests/test_gpu_privacy.py) and the order of the output stage (mask, then outlines / plates / text)."""
import numpy as np
import pytest

from yolo_deepsort_amd import privacy
from yolo_deepsort_amd.privacy import Anonymize, anonymize, mask_rects


# ---- arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, value", [
    ("mode", "blur"), ("mode", None), ("block", 1), ("block", 65), ("block", 8.0), ("block", True), ("color", (0, 0)), ("color", (0, 0, 256)),
    ("color", (0, -1, 0)), ("color", 7), ("color", (0.5, 0, 0)), ("region", "face"), ("head_frac", (0, 4)), ("head_frac", (5, 4)),
    ("head_frac", (1, 0)), ("head_frac", 0.25), ("head_frac", (1.0, 4)), ("margin", -1), ("margin", 1.5), ("classes", 0), ("classes", ("person",)),
    ("exempt_ids", 3), ("exempt_ids", ("a",)), ("exempt_ids", "12"), ("include_detections", 1), ("include_detections", None)])
def test_bad_arguments_raise_value_error_naming_the_argument(name, value):
    with pytest.raises(ValueError, match=name):
        Anonymize(**{name: value})


def test_defaults_and_accepted_arguments():
    a = Anonymize()
    assert (a.mode, a.block, a.color, a.region, a.head_frac, a.margin, a.include_detections) == ("pixelate", 16, (0, 0, 0), "box", (1, 4), 0, True)
    assert a.classes == {0} and a.exempt_ids == set()
    for m in (2, 64):
        assert Anonymize(block=m).block == m
    assert Anonymize(mode="fill", color=np.array([1, 2, 255])).color == (1, 2, 255)
    assert Anonymize(classes=None).classes is None and Anonymize(head_frac=(4, 4)).head_frac == (4, 4)
    watch = {7}
    a = Anonymize(exempt_ids=watch)
    assert a.exempt_ids is watch                     # the caller's own set: ids added later count


# ---- rectangles -----------------------------------------------------------------------------------------------------------------
H, W = 200, 300


def test_rects_of_tracker_rows():
    rows = np.array([[10, 20, 50, 90, 1, 0],          # plain
                     [80, 70, 60, 30, 2, 0],          # both corners inverted
                     [5, 5, 9, 9, 3, 2],              # another class
                     [100, 100, 120, 140, 4, 0]], np.int32)
    assert mask_rects(Anonymize(), H, W, rows) == [(10, 20, 50, 90), (60, 30, 80, 70), (100, 100, 120, 140)]
    assert mask_rects(Anonymize(classes=None), H, W, rows)[2] == (5, 5, 9, 9)
    assert mask_rects(Anonymize(classes=(2,)), H, W, rows) == [(5, 5, 9, 9)]
    assert mask_rects(Anonymize(margin=7), H, W, rows)[:2] == [(3, 13, 57, 97), (53, 23, 87, 77)]
    # head: yb = ya + ((yb - ya) * num) // den on the rectangle WITH its margin; (90 - 20) * 1 = 70 is no multiple of 4 -> 17
    assert mask_rects(Anonymize(region="head"), H, W, rows)[0] == (10, 20, 50, 37)
    assert mask_rects(Anonymize(region="head", head_frac=(2, 3), margin=1), H, W, rows)[0] == (9, 19, 51, 19 + (72 * 2) // 3)
    assert mask_rects(Anonymize(region="head", head_frac=(3, 3)), H, W, rows)[0] == (10, 20, 50, 90)
    # exempt ids: tracker rows only, and the set is read at every call
    a = Anonymize(exempt_ids={2})
    assert mask_rects(a, H, W, rows) == [(10, 20, 50, 90), (100, 100, 120, 140)]
    a.exempt_ids.add(1)
    assert mask_rects(a, H, W, rows) == [(100, 100, 120, 140)]
    for empty in (None, [], np.zeros((0, 6), np.int32)):
        assert mask_rects(Anonymize(), H, W, empty) == []
    # Python ints, as lists too; rectangles that cover no pixel of the frame are left out
    out = mask_rects(Anonymize(), H, W, [[-30, -30, -1, 50, 1, 0], [W, 0, W + 5, 5, 2, 0], [-5, -5, 0, 0, 3, 0], [W - 1, H - 1, W + 9, H + 9, 4, 0]])
    assert out == [(-5, -5, 0, 0), (W - 1, H - 1, W + 9, H + 9)] and all(type(v) is int for r in out for v in r)


def test_rects_of_detections_round_outwards():
    a = Anonymize()
    d = np.array([[3.0, 4.0, 5.0, 6.0, 0]], np.float32)                      # exactly on integers: floor(3) = 3, ceil(8) = 8
    assert mask_rects(a, H, W, None, d) == [(3, 4, 8, 10)]
    d = np.array([[2.999, 4.5, 5.002, 6.25, 0]], np.float32)                 # floor(2.999) = 2; ceil(2.999 + 5.002) = 9; ceil(10.75) = 11
    assert mask_rects(a, H, W, None, d) == [(2, 4, 9, 11)]
    d = np.array([[3.0, 4.0, 5.0, 6.0, 1], [30.5, 40.5, 1.0, 1.0, 0]], np.float32)
    assert mask_rects(a, H, W, None, d) == [(30, 40, 32, 42)]                # class filter
    assert mask_rects(Anonymize(include_detections=False), H, W, None, d) == []
    assert mask_rects(Anonymize(margin=2, region="head", head_frac=(1, 2)), H, W, None, d) == [(28, 38, 34, 38 + 6 // 2)]
    # exempt ids do not exempt a detection; tracker rows come first, detections behind them
    rows = np.array([[10, 20, 50, 90, 1, 0]], np.int32)
    assert mask_rects(Anonymize(exempt_ids={1}), H, W, rows, d) == [(30, 40, 32, 42)]
    assert mask_rects(a, H, W, rows, d) == [(10, 20, 50, 90), (30, 40, 32, 42)]
    # raw detector rows (no tracker: float x1, y1, x2, y2, conf, class) are treated as detections
    raw = np.array([[2.999, 4.0, 8.0, 10.001, 0.9, 0], [1, 1, 2, 2, 0.9, 5]], np.float32)
    assert mask_rects(a, H, W, raw) == [(2, 4, 8, 11)]
    raw7 = np.array([[50.5, 60.5, 40.25, 30.0, 0.9, 0.8, 0]], np.float32)     # [n, 7] rows, corners inverted
    assert mask_rects(a, H, W, raw7) == [(40, 30, 51, 61)]
    assert mask_rects(a, H, W, None, np.array([[np.nan, 0, 5, 5, 0]], np.float32)) == []


# ---- the host form ----------------------------------------------------------------------------------------------------------------
def _cell_value(img, cy, cx, m):
    """The rounded mean of one cell with Python ints only."""
    h, w = img.shape[:2]
    ys, xs = range(cy * m, min((cy + 1) * m, h)), range(cx * m, min((cx + 1) * m, w))
    cnt = len(ys) * len(xs)
    return [(2 * sum(int(img[y, x, c]) for y in ys for x in xs) + cnt) // (2 * cnt) for c in range(3)], cnt


def _union(h, w, rects):
    u = np.zeros((h, w), bool)
    for xa, ya, xb, yb in rects:
        u[max(ya, 0):max(min(yb + 1, h), 0), max(xa, 0):max(min(xb + 1, w), 0)] = True
    return u


def _rects_for(h, w):
    return [(1, 1, w // 2, h // 2),                       # partly inside cells
            (w // 3, h // 3, w - 2, h - 2),               # overlaps the first
            (w - 1, 0, w + 40, 0),                        # one pixel, top-right corner, clipped
            (-9, h - 1, 0, h + 3),                        # one pixel, bottom-left corner
            (w // 2, h // 2, w // 2, h // 2)]             # a single pixel in the middle


@pytest.mark.parametrize("h, w", [(5, 7), (33, 50), (120, 90)])
@pytest.mark.parametrize("m", [2, 3, 16, 64])
def test_pixelate_host_form(h, w, m):
    rng = np.random.RandomState(h * 100 + m)
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    keep = img.copy()
    a = Anonymize(block=m)
    rects = _rects_for(h, w)
    out = anonymize(img, rects, a)
    assert np.array_equal(img, keep) and out is not img               # on a copy
    u = _union(h, w, rects)
    assert np.array_equal(out[~u], img[~u])                           # outside U: untouched
    # every pixel of U holds its cell's rounded mean of the ORIGINAL values (partial edge cells divide by their own count)
    counts = set()
    for cy in range((h + m - 1) // m):
        for cx in range((w + m - 1) // m):
            cell_u = u[cy * m:(cy + 1) * m, cx * m:(cx + 1) * m]
            if not cell_u.any():
                continue
            v, cnt = _cell_value(img, cy, cx, m)
            counts.add(cnt)
            got = out[cy * m:(cy + 1) * m, cx * m:(cx + 1) * m][cell_u]
            assert (got == np.array(v, np.uint8)).all(), (cy, cx, v, got[:2])
    if h % m or w % m:
        assert len(counts) > 1 or min(h, w) < m                       # a partial edge cell was among them
    # the whole frame: every cell uniform
    full = anonymize(img, [(0, 0, w - 1, h - 1)], a)
    for cy in range((h + m - 1) // m):
        for cx in range((w + m - 1) // m):
            cell = full[cy * m:(cy + 1) * m, cx * m:(cx + 1) * m].reshape(-1, 3)
            assert (cell == cell[0]).all() and cell[0].tolist() == _cell_value(img, cy, cx, m)[0]
    # order, duplicates, in place, channel order
    perm = [rects[i] for i in (3, 0, 4, 2, 1)]
    assert np.array_equal(anonymize(img, perm, a), out) and np.array_equal(anonymize(img, rects + rects[:2], a), out)
    work = img.copy()
    assert anonymize(work, rects, a, inplace=True) is work and np.array_equal(work, out)
    bgr = np.ascontiguousarray(img[..., ::-1])
    assert np.array_equal(anonymize(bgr, rects, a, bgr=True), out[..., ::-1])
    # a constant image does not change; no rectangle: an equal copy
    const = np.full((h, w, 3), (17, 200, 255), np.uint8)
    assert np.array_equal(anonymize(const, rects, a), const)
    assert np.array_equal(anonymize(img, [], a), img) and np.array_equal(anonymize(img, [(w, h, w + 5, h + 5)], a), img)


@pytest.mark.parametrize("h, w", [(5, 7), (33, 50)])
def test_fill_host_form(h, w):
    img = np.random.RandomState(3).randint(0, 256, (h, w, 3)).astype(np.uint8)
    a = Anonymize(mode="fill", color=(10, 20, 30))
    rects = _rects_for(h, w)
    out = anonymize(img, rects, a)
    u = _union(h, w, rects)
    assert np.array_equal(out[~u], img[~u]) and (out[u] == np.array([10, 20, 30], np.uint8)).all()
    assert np.array_equal(anonymize(img, rects[::-1] + rects, a), out)
    bgr = np.ascontiguousarray(img[..., ::-1])
    assert np.array_equal(anonymize(bgr, rects, a, bgr=True), out[..., ::-1])          # the colour names the RGB image's channels
    with pytest.raises(ValueError):
        anonymize(img.astype(np.float32), rects, a)


def test_rounding_is_half_up_on_integers():
    img = np.zeros((2, 2, 3), np.uint8)
    img[0, 0] = (1, 2, 3)
    img[0, 1] = (1, 0, 3)                                             # sums 2, 2, 6 over 4 pixels: 0.5 -> 1, 0.5 -> 1, 1.5 -> 2
    out = anonymize(img, [(0, 0, 1, 1)], Anonymize(block=2))
    assert out.reshape(-1, 3).tolist() == [[1, 1, 2]] * 4


def test_pack_rects_and_device_args():
    table, ptr = privacy.pack_rects([[(1, 2, 3, 4)], None, [], [(-2 ** 40, 0, 2 ** 40, 5), (0, 0, 0, 0)]])
    assert table.dtype == np.int32 and ptr.tolist() == [0, 1, 1, 1, 3]
    assert table.tolist() == [[1, 2, 3, 4], [-2 ** 30, 0, 2 ** 30, 5], [0, 0, 0, 0]]
    table, ptr = privacy.pack_rects([None, None])
    assert table.shape == (1, 4) and ptr.tolist() == [0, 0, 0]
    assert privacy.device_args(Anonymize(mode="fill", color=(1, 2, 3)), False) == (2, 16, 1 | 2 << 8 | 3 << 16)
    assert privacy.device_args(Anonymize(block=5, color=(1, 2, 3)), True) == (1, 5, 3 | 2 << 8 | 1 << 16)


# ---- the output stage -------------------------------------------------------------------------------------------------------------
def _video_detector(anon, tracker=True):
    from yolo_deepsort_amd import cfgs
    from yolo_deepsort_amd.detect import VideoDetector
    from yolo_deepsort_amd.label_draw import LabelDrawer
    vd = VideoDetector.__new__(VideoDetector)
    vd.label_drawer = LabelDrawer(cfgs.coco_names_text().split("\n")[:-1], None, 10, 2, (608, 608))
    vd.tracker = object() if tracker else None
    vd.anonymize = anon
    return vd


def test_render_host_masks_first_then_draws():
    h, w = 120, 160
    frame = np.random.RandomState(4).randint(0, 256, (h, w, 3)).astype(np.uint8)
    keep = frame.copy()
    rows = np.array([[40, 50, 100, 110, 12, 0]], np.int32)
    dets = np.array([[120.5, 10.5, 20.0, 30.0, 0]], np.float32)       # a person the tracker has not confirmed yet
    anon = Anonymize(mode="fill", color=(9, 8, 7))
    plain = _video_detector(None)._render_host(frame, rows, "FPS: 12")
    got = _video_detector(anon)._render_host(frame, rows, "FPS: 12", dets)
    assert np.array_equal(frame, keep)                                # the caller's frame array is not modified
    # what it must equal: mask on a copy, then the drawer, then BGR, then the FPS text
    from yolo_deepsort_amd.label_draw import put_text
    want = anonymize(frame, mask_rects(anon, h, w, rows, dets), anon)
    _video_detector(None).label_drawer.draw_labels_by_trackers(want, rows, only_rect=False)
    want = put_text(np.ascontiguousarray(want[..., ::-1]), "FPS: 12", (3, 15), 2, (255, 0, 0))
    assert np.array_equal(got, want)
    # text and outlines lie OVER the mask: wherever the plain render differs from the bare frame (something was drawn), the masked
    # render shows the same drawn pixel; inside the boxes everything else is the fill colour (BGR order in the result)
    drawn = (plain != frame[..., ::-1]).any(-1)
    assert drawn.any() and np.array_equal(got[drawn], plain[drawn])
    inside = np.zeros((h, w), bool)
    inside[50:111, 40:101] = True
    inside[10:42, 120:142] = True
    assert (got[inside & ~drawn] == np.array([7, 8, 9], np.uint8)).all() and (inside & ~drawn).sum() > 3000
    assert np.array_equal(got[~inside & ~drawn], frame[..., ::-1][~inside & ~drawn])
    # nothing to mask, nothing held: the frame itself, reversed
    none = _video_detector(anon)._render_host(frame, None, None)
    assert np.array_equal(none, frame[..., ::-1])
    # only a detection (rows None: the detector's frame gave the tracker nothing to show) is masked all the same
    only = _video_detector(Anonymize())._render_host(frame, [], None, dets)
    assert not np.array_equal(only, frame[..., ::-1]) and np.array_equal(only, anonymize(frame, [(120, 10, 141, 41)], Anonymize())[..., ::-1])


def test_render_host_without_a_tracker_masks_the_raw_rows():
    h, w = 90, 120
    frame = np.random.RandomState(5).randint(0, 256, (h, w, 3)).astype(np.uint8)
    raw = np.array([[10.2, 20.7, 60.1, 70.0, 0.9, 0], [70, 5, 110, 40, 0.8, 2]], np.float32)
    anon = Anonymize(block=8)
    got = _video_detector(anon, tracker=False)._render_host(frame, raw, None)
    want = anonymize(frame, [(10, 20, 61, 70)], anon)
    _video_detector(None).label_drawer.draw_labels(want, raw, only_rect=False)
    assert np.array_equal(got, want[..., ::-1])
