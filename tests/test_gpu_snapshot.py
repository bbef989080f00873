"""Track snapshots on the device (csrc/snapshot.hip): per stream a table of tracks with the best 128 x 64 thumbnail of each, its score,
box and times, and an archive ring of the snapshots of tracks that left.  The comparator is the host definition
(yolo_deepsort_amd.snapshot.SnapshotBook) fed the same rows, times and frames; everything is integer after an 8-bit resize that is
restated bit for bit, so items, tables, rings and pictures are compared with exact equality.  What the scenes exercise is asserted on
the host's statistics in test_snapshot_host.py and again where a scene is used here."""
import functools

import numpy as np
import pytest

import snapshot_common as sc
from yolo_deepsort_amd import action as A, cfgs, ground as G, heatmap as H, snapshot as S, synth, zones as Z

pytestmark = pytest.mark.gpu
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)


def _same_items(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), k
        if w is not None:
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (k, g[:4], w[:4])


def _same_state(dev, host):
    """Tables, rings and pictures equal the host's, and the device's picture pool keeps count: every slot is free, a live entry's
    picture or a ring occupant's."""
    for s in range(host.n_streams):
        live, ring = dev.tracks(s), dev.archive(s)
        assert S.same_records(live, host.tracks(s)), s
        assert S.same_records(ring, host.archive(s)), s
        free, slots = dev.pool(s)
        assert free + sum(r["score"] >= 0 for r in live) + len(ring) == slots, (s, free, slots, len(live), len(ring))


def _upload(images, call):
    """The images of a call in one buffer at odd byte offsets: (device buffer, per frame of the call its offset and size, bytes)."""
    from yolo_deepsort_amd import _lib
    block, offs, sizes = sc.pack(images)
    assert all(o % 2 == 1 for o in offs)
    return _lib.DeviceBuffer.from_array(block), [offs[k] for _, _, _, k in call], [sizes[k] for _, _, _, k in call], block.nbytes


def _call(dev, buf, call, offs, sizes, nbytes, bgr=False):
    return dev.update_batch([r for _, r, _, _ in call], [s for s, _, _, _ in call], [t for _, _, t, _ in call], buf.ptr, sizes, offs, nbytes, bgr=bgr)


# ------------------------------------------------------------------------------------------------ 1. geometry
@pytest.mark.parametrize("bgr", [False, True])
def test_geometry_equals_the_host(bgr):
    """One call, one row per frame over frames of 5 x 7, 37 x 53, 128 x 64, 256 x 128 and 300 x 200 at odd byte offsets of one mixed
    buffer: boxes inside, cut by each edge and by a corner, wholly outside, of zero and negative extent, exactly at min_w / min_h and
    one below, and the COPY and AREA2 shapes; both channel orders."""
    from yolo_deepsort_amd import _lib
    images, cases = sc.geometry_scene()
    call = sc.geometry_call()
    dev = S.DeviceSnapshotBook(S.SnapSpec(**sc.GEOMETRY_SPEC), max_age=1000)
    host = dev.host()
    buf, offs, sizes, nbytes = _upload(images, call)
    _same_items(_call(dev, buf, call, offs, sizes, nbytes, bgr), sc.run_host(host, call, images, bgr))
    _same_state(dev, host)
    st = host.stats
    assert len(cases) == 115 and st["clipped"] >= 33 and st["non_candidates"] >= 60 and st["copies"] >= 12 and st["area2"] >= 8, st
    assert cases[21] == (1, (0, 0, 53, 37))
    rec = dev.snapshot(0, 22)                                                    # the whole 37 x 53 frame
    want = S.resize_u8(images[1])
    assert np.array_equal(rec["thumb"], want[:, :, ::-1] if bgr else want)
    assert dev.snapshot(0, 10 ** 6) is None
    # a frame that ends past the buffer is refused before anything runs
    with pytest.raises(_lib.YdsError, match="ends past"):
        _call(dev, buf, call, offs, sizes, max(o + h * w * 3 for o, (h, w) in zip(offs, sizes)) - 1)
    _same_state(dev, host)
    buf.free()
    dev.close()


# ------------------------------------------------------------------------------------------------ 2. time order within a call
def test_time_order_within_a_call_and_the_same_scene_in_two_calls():
    """Three streams x 6 frames in ONE call: ties on identical frames, a track that wins in frame 0, is beaten in frame 3 and closes in
    frame 5 (max_age 1), a ring of two so that a slot is freed and taken again inside the call.  The same scene split into two calls
    gives the same items and the same state."""
    images, call = sc.order_scene()
    host, want = sc.host_order()
    st = host.stats
    assert st["ties"] >= 6 and st["clipped"] >= 3 and st["non_candidates"] >= 6 and st["closes"] >= 12 and st["ring_wraps"] >= 6, st
    assert st["slot_reuses"] >= 3 and st["replacements"] >= 18, st
    buf, offs, sizes, nbytes = _upload(images, call)
    one = S.DeviceSnapshotBook(S.SnapSpec(**sc.ORDER_SPEC), max_age=1, n_streams=3)
    one.set_timing(True)
    _same_items(_call(one, buf, call, offs, sizes, nbytes), want)
    _same_state(one, host)
    assert all(0 < one.last_us(w) < 1e6 for w in S.DeviceSnapshotBook.TIMED)
    two = S.DeviceSnapshotBook(S.SnapSpec(**sc.ORDER_SPEC), max_age=1, n_streams=3)
    got = _call(two, buf, call[:9], offs[:9], sizes[:9], nbytes)
    late = _call(two, buf, call[9:], offs[9:], sizes[9:], nbytes)
    for e in late:
        e[:, 0] += 9                                                             # (tags are the frame's index in its call)
    _same_items(got + late, want)
    for s in range(3):
        for a, b in ((two.tracks(s), host.tracks(s)), (two.archive(s), host.archive(s))):
            for r in a:
                r["tag_best"] += 9 if r["t_best"] >= call[9][2] else 0
            assert S.same_records(a, b), s
    buf.free()
    one.close()
    two.close()


def test_mass_closes_over_a_full_ring_lose_no_slot():
    """Four waves of eight pictured tracks close together into a ring of three, in two calls: from the second wave on more pictures
    close in one frame than the ring holds while it is full of earlier occupants.  Items and state equal the host after each call,
    and no slot of the pool goes missing; the last wave's frame also grows the table while the ring is full."""
    images, calls = sc.waves_scene()
    host, want = sc.host_waves()
    st = host.stats
    assert st["overruns"] >= 3 and st["ring_wraps"] >= 29 and st["closes"] >= 106 and st["max_table"] >= 79, st
    dev = S.DeviceSnapshotBook(S.SnapSpec(**sc.WAVES_SPEC), max_age=1)
    mirror = dev.host()
    for c, call in enumerate(calls):
        buf, offs, sizes, nbytes = _upload(images, call)
        _same_items(_call(dev, buf, call, offs, sizes, nbytes), want[c])
        sc.run_host(mirror, call, images)
        _same_state(dev, mirror)
        buf.free()
    free, slots = dev.pool(0)
    assert slots == 128 + 3 and free == slots - 3 - sum(r["score"] >= 0 for r in dev.tracks(0))
    dev.close()


# ------------------------------------------------------------------------------------------------ 3. the scale of the table frame
@pytest.mark.parametrize("archive", [32, 0])
def test_a_crowd_of_700_grows_the_table_and_vanishes(archive):
    """One stream: frames of 50, 200, 400 and 700 rows in four calls (the table grows through 64, 256 and 512 to 1024 and takes its
    pictures along; 700 entries are three strides of 256 threads), then two frames without rows: all 700 close in one frame, into a
    ring of 32 or into nothing."""
    images, calls = sc.crowd_scene()
    host, want = sc.host_crowd(archive)
    st = host.stats
    assert st["max_table"] == 700 and st["closes"] == 700 and st["clipped"] >= 100 and st["non_candidates"] >= 100, st
    assert (st["ring_wraps"] > 400) if archive else (st["dropped"] > 400), st
    dev = S.DeviceSnapshotBook(S.SnapSpec(archive=archive), max_age=1)
    mirror = dev.host()
    for c, call in enumerate(calls):
        buf, offs, sizes, nbytes = _upload(images, call)
        _same_items(_call(dev, buf, call, offs, sizes, nbytes), want[c])
        sc.run_host(mirror, call, images)
        _same_state(dev, mirror)
        buf.free()
    assert dev.tracks(0) == [] and len(dev.archive(0)) == (32 if archive else 0)
    dev.close()


# ------------------------------------------------------------------------------------------------ 4. skipped streams, class filter, reset
def test_a_stream_without_a_spec_is_skipped_the_class_filter_and_reset_per_stream():
    images, call = sc.order_scene()
    specs = [S.SnapSpec(class_id=0, **sc.ORDER_SPEC), None, S.SnapSpec(class_id=None, **sc.ORDER_SPEC)]
    dev = S.DeviceSnapshotBook(specs, max_age=2)
    host = dev.host()
    buf, offs, sizes, nbytes = _upload(images, call)
    got = _call(dev, buf, call[:12], offs[:12], sizes[:12], nbytes)
    _same_items(got, sc.run_host(host, call[:12], images))
    assert all(g.shape == (0, 6) for (s, _, _, _), g in zip(call[:12], got) if s == 1) and dev.tracks(1) == [] and dev.archive(1) == []
    assert host.stats["ignored_rows"] == 4 and {r["cls"] for r in dev.tracks(2)} == {0, 1} and {r["cls"] for r in dev.tracks(0)} == {0}
    _same_state(dev, host)
    kept = dev.tracks(0)
    dev.reset(2)
    host.reset(2)
    assert dev.tracks(2) == [] and dev.archive(2) == [] and S.same_records(dev.tracks(0), kept)
    more = call[12:]
    _same_items(_call(dev, buf, more, offs[12:], sizes[12:], nbytes), sc.run_host(host, more, images))
    _same_state(dev, host)
    assert len(dev.archive(0)) > 0
    dev.reset()
    assert not any(dev.tracks(s) or dev.archive(s) for s in range(3))
    buf.free()
    dev.close()


# ------------------------------------------------------------------------------------------------ 5. inside the step
@functools.lru_cache(maxsize=None)
def _net(batch_max, bias=-1.45):
    from yolo_deepsort_amd.models import Darknet
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=batch_max, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, bias))        # a handful of (random) detections per frame
    return net


def _clip(seed, hw, n, roll=3):
    img = np.random.RandomState(seed).randint(0, 256, hw + (3,)).astype(np.uint8)
    return [np.roll(img, roll * t, axis=1) for t in range(n)]


@pytest.mark.parametrize("mode", ["multi", "mixed", "windows"])
def test_step_snapshots_equal_the_host_and_leave_everything_else_alone(mode):
    """yolov3-tiny 416 with random weights over three cameras for 6 steps with actions, zones, heat maps, the ground plane and
    identities all on: a plain multi-stream step (480 x 640, look-ahead), a mixed-size step and a step whose first stream is cut
    into windows.  The items, tables, rings and pictures of every step equal the host SnapshotBook fed the step's rows, frame times
    and frames; a second pipeline without the stage returns the same rows and the same reports of every other stage.  set_snapshots
    is refused while a look-ahead pass is in flight and with a handle of too few streams."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    _lib.init(0)
    sizes = [(480, 640), (270, 480), (416, 416)] if mode == "mixed" else [(480, 640)] * 3
    n_steps, net = 6, _net(8)
    clips = [_clip(40 + s, sizes[s], n_steps) for s in range(3)]
    if mode == "windows":                            # the detector and the still frames of test_gpu_stream_windows.py's cameras A and D
        net, clips = _net(5, -1.3), [_clip(seed, (480, 640), n_steps, roll=0) for seed in (85, 88, 88)]
    spec = S.SnapSpec(min_w=8, min_h=16, archive=4)
    turn = np.eye(3)
    import ground_common as gc
    ground_specs = [G.GroundSpec(turn @ gc.pinhole_H(height=3.0 + s, tilt_deg=20.0 + 5 * s, f=0.9 * w, cx=w / 2, cy=h / 2), class_id=-1, **gc.PLAN)
                    for s, (h, w) in enumerate(sizes)]
    heat_specs = [H.HeatSpec(h, w, 32, -1) for h, w in sizes]
    packs = [pl.pack_frames([clips[s][i] for s in range(3)]) for i in range(n_steps)]
    devs = [_lib.DeviceBuffer.from_array(p[0]) for p in packs]
    ex = Extractor(synth.reid_state_dict(0), max_crops=256)
    ident = A.ActionIdentify([A.Glide(0, (0, 3)), A.FastCrossing(0, 0.01)], max_age=2, max_size=3)
    zones = ([Z.Zone([(0, 0), (240, 0), (240, 270), (0, 270)], name="left")], [Z.Line((200, 0), (200, 400))])
    time_of = lambda s, i: 0.04 * i + 0.001 * s          # noqa: E731
    ahead = mode == "multi"

    def run(with_snap):
        trackers = [DeepSort(ex, use_cuda=True, **DS) for _ in range(3)]
        pipe = pl.MultiStreamPipeline(net, trackers, 0.5, 0.4, stream_win_sizes=[(416, 416), None, None] if mode == "windows" else None)
        pipe.set_actions(ident)
        pipe.set_zones(zones, max_age=2)
        pipe.set_heatmap(heat_specs, max_age=2)
        pipe.set_ground(ground_specs, max_age=2)
        pipe.set_identities(True)
        assert pipe.last_snapshot_events() is None and pipe.snapshots() is None
        snap = None
        if with_snap:
            with pytest.raises(ValueError, match="snapshots"):
                pipe.set_snapshots([spec, spec])
            small = S.DeviceSnapshotBook(spec, n_streams=2)                  # (kept alive: its handle dies with it)
            with pytest.raises(_lib.YdsError, match="a snapshots handle of 2 streams"):
                _lib.check(_lib.load().yds_pipeline_set_snapshots(pipe._h, small.handle))
            small.close()
            snap = pipe.set_snapshots(spec, max_age=2)
            snap.set_timing(True)
        rows, other, items = [], [], []
        for i in range(n_steps):
            pipe.set_frame_times([time_of(s, i) for s in range(3)])
            nxt = ahead and i + 1 < n_steps
            if mode == "mixed":
                outs = pipe.step_mixed(devs[i].ptr, packs[i][1], packs[i][2], [0, 1, 2], packs[i][0].nbytes)
            else:
                outs = pipe.step(devs[i].ptr, 480, 640, [0, 1, 2], devs[i + 1].ptr if nxt else None)
            if with_snap and nxt and i == 2:
                with pytest.raises(_lib.YdsError, match="set_snapshots while a look-ahead"):
                    pipe.set_snapshots(None)
            rows.append(outs)
            other.append((pipe.last_actions(), pipe.last_zone_events(), pipe.last_identities(), [h.tolist() for h in pipe.heatmap()],
                          [None if g is None else g.tolist() for g in pipe.last_ground()]))
            if with_snap:
                items.append((pipe.last_snapshot_events(), pipe.last_snapshot_events(2), pipe.snapshots(), pipe.snapshots(archive=True)))
        return pipe, snap, rows, other, items
    pipe, snap, rows, other, items = run(True)
    host = S.SnapshotBook(spec, max_age=2, n_streams=3)
    best = 0
    for i in range(n_steps):
        want = [host.update(s, rows[i][s], time_of(s, i), clips[s][i], tag=s) for s in range(3)]
        _same_items(items[i][0], want)
        assert np.array_equal(items[i][1], want[2] if want[2] is not None else np.zeros((0, 6), np.int32))
        assert all(S.same_records(items[i][2][s], host.tracks(s)) and S.same_records(items[i][3][s], host.archive(s)) for s in range(3)), i
        best += sum(int((w[:, 3] == S.BEST).sum()) for w in want if w is not None)
    assert best >= 3 and sum(len(host.tracks(s)) for s in range(3)) >= 3, host.stats
    assert all(0 < snap.last_us(w) < 1e6 for w in ("score", "decide", "commit"))
    # without the stage: the same everything else
    _, _, plain_rows, plain_other, _ = run(False)
    for i in range(n_steps):
        assert other[i] == plain_other[i], i
        for a, p in zip(rows[i], plain_rows[i]):
            assert (a is None) == (p is None) and (a is None or (a.shape == p.shape and np.array_equal(a, p))), i
    # switched off again: the step launches nothing of the stage and the tables stand
    pipe.set_snapshots(None)
    assert pipe.last_snapshot_events() is None
    snap.set_timing(True)
    before = [snap.tracks(s) for s in range(3)]
    if mode == "mixed":
        pipe.step_mixed(devs[0].ptr, packs[0][1], packs[0][2], [0, 1, 2], packs[0][0].nbytes)
    else:
        pipe.step(devs[0].ptr, 480, 640, [0, 1, 2])
    with pytest.raises(_lib.YdsError, match="no timed launch"):
        snap.last_us("decide")
    assert all(S.same_records(snap.tracks(s), before[s]) for s in range(3))
    snap.close()


# ------------------------------------------------------------------------------------------------ 6. detect_streams
def test_detect_streams_takes_snapshots_and_anonymize_does_not_mask_them(tmp_path):
    """detect_streams(snapshots=...) over two in-memory clips of different sizes, the second camera without a spec, with the
    anonymise option on: between the yields stream_snapshots() and stream_snapshot_events() equal a host SnapshotBook fed the yielded
    rows and the SOURCE frames - the pictures are taken before the output stage and stay unmasked - and the yielded rows are those of
    a run without the option."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import DeepSort
    from yolo_deepsort_amd.detect import VideoDetector
    from yolo_deepsort_amd.privacy import Anonymize
    _lib.init(0)
    net = _net(8)
    base = DeepSort(synth.reid_state_dict(0), use_cuda=True, **DS)
    clips = [_clip(21, (480, 640), 21), _clip(22, (270, 480), 7)]
    specs = [S.SnapSpec(archive=4), None]
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())

    def detector():
        return VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=base, skip_frames=2, class_mask=list(range(0, 80, 2)),
                             anonymize=Anonymize())
    plain = [[(s, det) for s, _, det, _ in step] for step in detector().detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True)]
    vd = detector()
    host = S.SnapshotBook(specs, max_age=3)
    seen, items, best = [0, 0], [], 0
    for step in vd.detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True, snapshots=specs, snapshot_max_age=3):
        want, b = [[], []], 0
        for s, _, det, _ in step:
            if seen[s] % 2 == 0:                                      # a processed frame: frame b of the step
                want[s].append(host.update(s, det, seen[s] / 25.0, clips[s][seen[s]], tag=b))
                b += 1
            seen[s] += 1
        got = vd.stream_snapshot_events()
        for s in range(2):
            _same_items(got[s], want[s])
            best += sum(int((w[:, 3] == S.BEST).sum()) for w in want[s] if w is not None)
        recs = vd.stream_snapshots()
        assert S.same_records(recs[0], host.tracks(0)) and recs[1] == [] and S.same_records(vd.stream_snapshots(0, archive=True), host.archive(0))
        items.append([(s, det) for s, _, det, _ in step])
    assert seen == [21, 7] and best >= 2 and any(r["thumb"].any() for r in host.tracks(0) + host.archive(0))
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_snapshots()
    assert len(items) == len(plain)
    for a, b in zip(items, plain):
        assert [s for s, _ in a] == [s for s, _ in b]
        assert all((x is None) == (y is None) and (x is None or np.array_equal(x, y)) for (_, x), (_, y) in zip(a, b))
    with pytest.raises(ValueError, match="snapshots"):
        next(detector().detect_streams(clips, mixed_sizes=True, snapshots=[specs[0]]))
    with pytest.raises(ValueError, match="snapshots="):
        vd2 = detector()
        for _ in vd2.detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True):
            vd2.stream_snapshots()
