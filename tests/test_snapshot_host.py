"""Host-side checks of the snapshot stage (yolo_deepsort_amd.snapshot): the restated 8-bit resize against the oracle's, hand-computed
scores, the decision, closing and ring rules one at a time, the host join, the refusals that need no device, the prototypes of the new
entries, and the statistics that the GPU scenes (snapshot_common.py) rely on."""
import numpy as np
import pytest

import snapshot_common as sc
from oracle.resize import resize_bilinear_u8
from yolo_deepsort_amd import snapshot as S

INTERIOR = 126 * 62


def _board(h, w, a, b, block=1):
    y, x = np.mgrid[0:h, 0:w]
    v = np.where(((y // block) + (x // block)) % 2 == 0, a, b).astype(np.uint8)
    return np.repeat(v[:, :, None], 3, axis=2)


# ------------------------------------------------------------------------------------------------ the resize
def _crop_shapes():
    shapes = {(128, 64), (256, 128), (1, 1), (1, 9), (9, 1), (128, 1), (1, 64), (2, 3), (127, 65), (129, 63), (300, 200)}
    images, cases = sc.geometry_scene()
    for k, box in cases:
        h, w = images[k].shape[:2]
        _, _, vw, vh, _, full = S.clip_box(box, h, w)
        if vw >= 1 and vh >= 1 and full > 0:
            shapes.add((vh, vw))
    for images, call in (sc.order_scene(), (sc.crowd_scene()[0], sc.crowd_scene()[1][3])):
        for _, rows, _, k in call:
            for r in rows:
                _, _, vw, vh, _, full = S.clip_box(r, *images[k].shape[:2])
                if vw >= 1 and vh >= 1 and full > 0:
                    shapes.add((vh, vw))
    return sorted(shapes)


def test_resize_equals_the_oracle_on_every_crop_shape_the_gpu_tests_use():
    shapes = _crop_shapes()
    assert len(shapes) > 200 and (128, 64) in shapes and (256, 128) in shapes and any(w == 1 for _, w in shapes)
    rs = np.random.RandomState(0)
    for h, w in shapes:
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        got = S.resize_u8(img)
        assert got.dtype == np.uint8 and got.shape == (128, 64, 3)
        assert np.array_equal(got, resize_bilinear_u8(img, (64, 128))), (h, w)
    img = rs.randint(0, 256, (128, 64, 3)).astype(np.uint8)
    assert np.array_equal(S.resize_u8(img), img)                               # COPY
    big = rs.randint(0, 256, (256, 128, 3)).astype(np.int64)
    mean = (big[0::2, 0::2] + big[0::2, 1::2] + big[1::2, 0::2] + big[1::2, 1::2] + 2) >> 2
    assert np.array_equal(S.resize_u8(big.astype(np.uint8)), mean)             # AREA2


# ------------------------------------------------------------------------------------------------ three scores by hand
def test_a_flat_crop_scores_zero():
    frame = np.full((90, 70, 3), 131, np.uint8)
    thumb, score = S.snapshot_of(frame, [5, 5, 60, 80, 1, 0], S.SnapSpec())
    assert score == 0 and (thumb == 131).all()


def test_a_one_pixel_checkerboard_has_a_closed_form():
    # grey pixels: Y = (256 v + 128) >> 8 = v; every interior pixel differs from its four neighbours by |a - b|
    frame = _board(128, 64, 200, 50)
    thumb, score = S.snapshot_of(frame, [0, 0, 64, 128, 1, 0], S.SnapSpec())
    assert np.array_equal(thumb, frame) and score == INTERIOR * 4 * 150 == 4687200
    assert S.sharpness(thumb) <= 8.1e6 and S.sharpness(_board(128, 64, 255, 0)) == INTERIOR * 4 * 255 < 8.1e6


def test_a_half_visible_box_is_halved():
    # 2 x 2 blocks at exactly twice the size: the 2 x 2 mean gives the one-pixel checkerboard back; half of the box is left of the frame
    frame = _board(256, 128, 200, 50, block=2)
    thumb, score = S.snapshot_of(frame, [-128, 0, 128, 256, 1, 0], S.SnapSpec())
    assert np.array_equal(thumb, _board(128, 64, 200, 50)) and score == (INTERIOR * 4 * 150) // 2
    assert S.snapshot_of(frame, [0, 0, 128, 256, 1, 0], S.SnapSpec())[1] == INTERIOR * 4 * 150
    # channels are stored as RGB whatever the frame's order, and the luma weights are not symmetric
    rs = np.random.RandomState(1)
    f = rs.randint(0, 256, (128, 64, 3)).astype(np.uint8)
    t_rgb, _ = S.snapshot_of(f, [0, 0, 64, 128, 1, 0], S.SnapSpec())
    t_bgr, _ = S.snapshot_of(f, [0, 0, 64, 128, 1, 0], S.SnapSpec(), bgr=True)
    assert np.array_equal(t_bgr, t_rgb[:, :, ::-1]) and int(S.luma(t_rgb)[0, 0]) == (77 * int(f[0, 0, 0]) + 150 * int(f[0, 0, 1]) + 29 * int(f[0, 0, 2]) + 128) >> 8


# ------------------------------------------------------------------------------------------------ decision, closing, ring
def _frames():
    rs = np.random.RandomState(5)
    lively = rs.randint(0, 256, (64, 48, 3)).astype(np.uint8)
    dull = (128 + (lively.astype(np.int64) - 128) // 4).astype(np.uint8)
    return lively, dull


def test_strictly_greater_replaces_and_a_tie_keeps_the_earlier_sighting():
    lively, dull = _frames()
    book = S.SnapshotBook(S.SnapSpec(), max_age=3)
    box = [4, 4, 30, 60, 7, 2]
    ev = book.update(0, [box], 0.0, dull, tag=5)
    s_dull = S.snapshot_of(dull, box, S.SnapSpec())[1]
    assert ev.tolist() == [[5, 7, 2, S.BEST, s_dull, 1]] and ev.dtype == np.int32
    assert book.update(0, [box], 1.0, dull, tag=6).shape == (0, 6) and book.stats["ties"] == 1            # a tie: nothing changes
    rec = book.snapshot(0, 7)
    assert (rec["t_best"], rec["tag_best"], rec["t_last"], rec["n_seen"], rec["t_first"]) == (0.0, 5, 1.0, 2, 0.0)
    ev = book.update(0, [box], 2.0, lively, tag=7)
    s_live = S.snapshot_of(lively, box, S.SnapSpec())[1]
    assert s_live > s_dull and ev.tolist() == [[7, 7, 2, S.BEST, s_live, 3]]
    assert book.update(0, [box], 3.0, dull, tag=8).shape == (0, 6)                                          # a worse one: nothing changes
    rec = book.snapshot(0, 7)
    assert rec["score"] == s_live and rec["box"] == (4, 4, 30, 60) and rec["t_best"] == 2.0 and rec["n_seen"] == 4
    assert np.array_equal(rec["thumb"], S.resize_u8(lively[4:60, 4:30]))
    # a row that is no candidate is a sighting all the same: an entry without a picture, its age reset
    book.update(0, [[0, 0, 5, 50, 9, 0]], 4.0, lively)
    rec = book.snapshot(0, 9)
    assert rec["score"] == -1 and not rec["thumb"].any() and rec["n_seen"] == 1 and book.stats["non_candidates"] == 1
    assert book.snapshot(0, 12345) is None and book.update(0, None, 9.0, lively) is None
    with pytest.raises(ValueError, match="twice"):
        book.update(0, [box, box], 5.0, lively)


def test_closing_ring_wrap_and_no_archive():
    lively, dull = _frames()
    book = S.SnapshotBook(S.SnapSpec(archive=2), max_age=1)
    rows = [[2, 2, 20, 40, 1, 0], [10, 10, 40, 60, 2, 0], [0, 0, 12, 30, 3, 0], [0, 0, 4, 4, 4, 0]]
    book.update(0, rows, 0.0, lively, tag=0)
    assert book.update(0, [], 1.0, lively, tag=1).shape == (0, 6)              # age 1: nobody leaves
    ev = book.update(0, [], 2.0, lively, tag=2)
    scores = [S.snapshot_of(lively, r, S.SnapSpec())[1] for r in rows]
    # entry order; ring positions 0, 1, then 0 again (a wrap); the entry without a picture is dropped
    assert ev.tolist() == [[2, 1, 0, S.CLOSED, scores[0], 0], [2, 2, 0, S.CLOSED, scores[1], 1], [2, 3, 0, S.CLOSED, scores[2], 0],
                           [2, 4, 0, S.CLOSED, -1, -1]]
    arch = book.archive(0)
    assert [a["id"] for a in arch] == [2, 3] and arch[0]["t_closed"] == 2.0 and book.stats["ring_wraps"] == 1 and book.tracks(0) == []
    assert np.array_equal(book.snapshot(0, 3)["thumb"], S.resize_u8(lively[0:30, 0:12])) and book.snapshot(0, 1) is None
    # an id that returns is a new entry; the archived one stays
    book.update(0, [rows[1]], 3.0, dull, tag=3)
    assert book.snapshot(0, 2)["t_first"] == 3.0 and [a["id"] for a in book.archive(0)] == [2, 3]
    none = S.SnapshotBook(S.SnapSpec(archive=0), max_age=1)
    none.update(0, rows[:1], 0.0, lively)
    none.update(0, [], 1.0, lively)
    assert none.update(0, [], 2.0, lively, tag=4).tolist() == [[4, 1, 0, S.CLOSED, scores[0], -1]] and none.archive(0) == []
    assert none.stats["dropped"] == 1


def test_class_filter_skipped_stream_and_specs():
    lively, _ = _frames()
    book = S.SnapshotBook([S.SnapSpec(class_id=1), None], max_age=1)
    rows = [[2, 2, 20, 40, 1, 0], [10, 10, 40, 60, 2, 1]]
    assert book.update(0, rows, 0.0, lively)[:, 1].tolist() == [2] and [r["id"] for r in book.tracks(0)] == [2]
    assert book.update(1, rows, 0.0, lively).shape == (0, 6) and book.tracks(1) == []
    # rows of another class have no age effect either: id 2 ages although a row of class 0 carries its id
    book.update(0, [[10, 10, 40, 60, 2, 0]], 1.0, lively)
    assert book.update(0, [[10, 10, 40, 60, 2, 0]], 2.0, lively)[:, 3].tolist() == [S.CLOSED]
    for bad in (dict(min_w=0), dict(min_h=0), dict(archive=-1), dict(archive=S.MAX_ARCHIVE + 1), dict(class_id=-2), dict(min_w=2.5)):
        with pytest.raises(ValueError, match="snapshots"):
            S.SnapSpec(**bad)
    with pytest.raises(ValueError, match="snapshots"):
        S.SnapshotBook([None, None])
    with pytest.raises(ValueError, match="share archive"):
        S.SnapshotBook([S.SnapSpec(archive=1), S.SnapSpec(archive=2)])
    with pytest.raises(ValueError, match="max_age"):
        S.SnapshotBook(S.SnapSpec(), max_age=0)
    with pytest.raises(ValueError, match="snapshots"):
        S.DeviceSnapshotBook([S.SnapSpec()] * 2, n_streams=3)
    dev = S.DeviceSnapshotBook([S.SnapSpec(), None], max_age=4)                # (no handle until it is used)
    assert dev.host().max_age == 4 and dev.fresh(1).n_streams == 1
    with pytest.raises(ValueError, match="snapshots"):
        S.as_device_snapshots(dev, 3)
    with pytest.raises(ValueError, match="last_us"):
        dev.last_us("update")


def test_by_global_id_takes_the_best_picture_over_all_cameras():
    rec = lambda i, s: dict(id=i, score=s, thumb=None)      # noqa: E731
    books = [[rec(1, 50), rec(2, 70), rec(3, -1)], None, [rec(1, 90), rec(8, 50), rec(9, 10)]]
    ids = [[(1, 4), (2, 5), (3, 6)], [], {1: 5, 8: 4, 9: 0}]
    got = S.by_global_id(books, ids)
    assert list(got) == [4, 5] and got[4]["stream"] == 0 and got[4]["record"]["id"] == 1                   # a tie: the earlier stream
    assert got[5]["stream"] == 2 and got[5]["record"]["score"] == 90


def test_pixel_layout():
    off, hw, span = S.pixel_layout((4, 5), 3)
    assert off.tolist() == [0, 60, 120] and hw.tolist() == [[4, 5]] * 3 and span == 180 and off.dtype == np.uint64 and hw.dtype == np.int32
    off, hw, span = S.pixel_layout([(4, 5), (2, 2)], 2, [7, 100])
    assert off.tolist() == [7, 100] and span == 112
    with pytest.raises(ValueError, match="snapshots"):
        S.pixel_layout([(4, 5)], 2)


def test_video_detector_stream_snapshots_outside_a_generator():
    from yolo_deepsort_amd.detect import VideoDetector
    vd = VideoDetector.__new__(VideoDetector)
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_snapshots()
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_snapshot_events()


def test_new_entries_are_declared_prototyped_and_exported():
    import os
    from yolo_deepsort_amd import _lib, build
    build.build()                                               # (nothing to do when the library is current)
    names = ["yds_snap_create", "yds_snap_destroy", "yds_snap_set_stream", "yds_snap_reset", "yds_snap_update", "yds_snap_get_tracks",
             "yds_snap_get_archive", "yds_snap_get_pool", "yds_snap_set_timing", "yds_snap_last_us", "yds_pipeline_set_snapshots", "yds_pipeline_last_snapshots"]
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "ydsort.h")).read()
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n) and n + "(" in header, n
    assert _lib.MISSING == []
    assert "#define YDS_SNAP_H %d" % S.THUMB_H in header and "#define YDS_SNAP_W %d" % S.THUMB_W in header
    assert "#define YDS_SNAP_MAX_ARCHIVE %d" % S.MAX_ARCHIVE in header


# ------------------------------------------------------------------------------------------------ what the GPU scenes exercise
def test_the_geometry_scene_holds_every_case():
    images, cases = sc.geometry_scene()
    book = S.SnapshotBook(S.SnapSpec(**sc.GEOMETRY_SPEC), max_age=1000)
    ev = sc.run_host(book, sc.geometry_call(), images)
    st = book.stats
    assert len(cases) == len(ev) == 115 and st["clipped"] >= 33 and st["non_candidates"] >= 60 and st["copies"] >= 12 and st["area2"] >= 8, st
    assert sum(len(e) for e in ev) == len(cases) - st["non_candidates"] and st["max_table"] == len(cases)


def test_the_order_scene_holds_every_case():
    book, ev = sc.host_order()
    st = book.stats
    assert st["ties"] >= 6 and st["clipped"] >= 3 and st["non_candidates"] >= 6 and st["closes"] >= 12 and st["ring_wraps"] >= 6, st
    assert st["slot_reuses"] >= 3 and st["replacements"] >= 18, st
    images, call = sc.order_scene()
    for s in range(3):                                                         # id 2: wins in frame 0, beaten in frame 3, closed in frame 5
        mine = [e[e[:, 1] == 2] for f, e in enumerate(ev) if call[f][0] == s]
        assert [m[:, 3].tolist() for m in mine][0] == [S.BEST] and mine[3][:, 3].tolist() == [S.BEST] and mine[5][:, 3].tolist() == [S.CLOSED]
        assert mine[3][0, 4] > mine[0][0, 4] and mine[5][0, 4] == mine[3][0, 4] and mine[5][0, 5] >= 0
        assert np.array_equal(images[call[s][3]], images[call[3 + s][3]]) and not np.array_equal(images[call[s][3]], images[call[6 + s][3]])


def test_the_waves_scene_closes_more_pictures_than_the_ring_holds_over_a_full_ring():
    book, ev = sc.host_waves()
    st = book.stats
    assert st["overruns"] >= 3 and st["ring_wraps"] >= 29 and st["closes"] >= 106 and st["max_table"] >= 79, st
    assert [a["id"] for a in book.archive(0)] == [1067, 1068, 1069] and book.tracks(0) == []


@pytest.mark.parametrize("archive", [32, 0])
def test_the_crowd_scene_holds_every_case(archive):
    book, ev = sc.host_crowd(archive)
    st = book.stats
    assert st["max_table"] == 700 and st["closes"] == 700 and st["clipped"] >= 100 and st["non_candidates"] >= 100 and st["replacements"] == 0, st
    closed = ev[-1][1]
    assert len(ev[-1][0]) == 0 and len(closed) == 700 and (closed[:, 3] == S.CLOSED).all() and closed[:, 1].tolist() == list(range(1, 701))
    pictured = int((closed[:, 4] >= 0).sum())
    if archive:
        assert st["ring_wraps"] == pictured - 32 > 400 and len(book.archive(0)) == 32 and set(closed[:, 5].tolist()) == set(range(-1, 32))
    else:
        assert st["dropped"] == pictured > 400 and book.archive(0) == [] and (closed[:, 5] == -1).all()
