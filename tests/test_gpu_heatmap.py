"""Heat maps on the device (csrc/heatmap.hip): per stream five int64 layers and a table of tracks in HBM, one launch per call, and the
render that blends a layer into frames resident in HBM.  The comparator is the host definition (yolo_deepsort_amd.heatmap: HeatMap,
render) fed the same rows, times and frames; everything is integer arithmetic but one double subtraction and product per dwell
credit, so layers, maxima, tables and pixels are compared with exact equality.  What a scene exercises is asserted on the HOST
output (HeatMap.stats, explicit counts), so no comparison can pass vacuously."""
import ctypes as C
import functools

import numpy as np
import pytest

from yolo_deepsort_amd import action as A, cfgs, heatmap as H, synth, zones as Z

pytestmark = pytest.mark.gpu
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)


def foot(x, y, tid, cls=0):
    """A row whose foot point is (x, y)."""
    return [x - 3, y - 20, x + 3, y, tid, cls]


def _same_state(dev, hosts):
    for s, host in enumerate(hosts):
        if host is None:
            continue
        got = dev.layers(s)
        assert got.dtype == np.int64 and np.array_equal(got, host.layers()), s
        for name in H.LAYERS:
            assert dev.max(s, name) == host.max(name), (s, name)
        assert dev.tracks(s) == host.tracks(), s


def _feed(dev, hosts, frames):
    """frames: [(stream, rows or None, t), ...] in ONE device call against the hosts frame by frame."""
    got = dev.update_batch([r for _, r, _ in frames], [s for s, _, _ in frames], [t for _, _, t in frames])
    want = [hosts[s].update(r, t) for s, r, t in frames]
    assert got == want
    _same_state(dev, hosts)


def crowd_scene(seed, n_ids, n_frames, h, w):
    """[(rows int32 [m, 6], t), ...]: n_ids people at integer foot points in [-24, w + 24) x [-24, h + 24) (some outside the grid),
    velocity components in [-7, 7] redrawn every 6 frames, reflected at those borders; a person is missed with probability 0.12 and
    now and then hides for 2..6 frames; the visible rows shuffled; class i % 3; frame t at time 0.04 * t."""
    rs = np.random.RandomState(seed)
    lo, hi = np.array([-24, -24]), np.array([w + 24, h + 24])
    pos = rs.randint(0, 1 << 30, (n_ids, 2)) % (hi - lo) + lo
    hidden = np.zeros(n_ids, np.int64)
    ids, cls = np.arange(1, n_ids + 1), np.arange(n_ids) % 3
    vel = np.zeros((n_ids, 2), np.int64)
    frames = []
    for t in range(n_frames):
        if t % 6 == 0:
            vel = rs.randint(-7, 8, (n_ids, 2))
        pos = pos + vel
        low, high = pos < lo, pos >= hi
        pos = np.where(low, 2 * lo - pos, np.where(high, 2 * hi - 2 - pos, pos))
        vel = np.where(low | high, -vel, vel)
        hidden = np.where((hidden == 0) & (rs.rand(n_ids) < 0.04), rs.randint(2, 7, n_ids), np.maximum(hidden - 1, 0))
        seen = np.flatnonzero((hidden == 0) & (rs.rand(n_ids) < 0.88))
        rs.shuffle(seen)
        rows = np.stack([pos[seen, 0] - 4, pos[seen, 1] - 30, pos[seen, 0] + 4, pos[seen, 1], ids[seen], cls[seen]], 1).astype(np.int32)
        frames.append((rows, 0.04 * t))
    return frames


# ------------------------------------------------------------------------------------------------ 1. randomised
@pytest.mark.parametrize("max_age", [1, 3])
def test_random_scene_equals_the_host_map(max_age):
    """900 ids of three classes over 60 frames of 200 x 150 at cell 16, class 0 counted, in three calls of 20 frames: the table grows
    past 256 entries between calls.  After every call layers, maxima and table equal the host."""
    dev = H.DeviceHeatMap(H.HeatSpec(150, 200, cell=16, class_id=0), max_age=max_age)
    host = dev.host()
    frames = [(0, r, t) for r, t in crowd_scene(7, 900, 60, 150, 200)]
    for k in range(0, 60, 20):
        _feed(dev, [host], frames[k:k + 20])
    st = host.stats
    assert st["multi_hit_cells"] >= 500 and st["outside_rows"] >= 500 and st["returned"] >= 50 and st["gap_sightings"] >= 300, st
    assert st["cell_changes"] >= 1000 and st["stays"] >= 1000 and st["from_outside"] >= 50 and st["ignored_rows"] >= 10000, st
    assert st["max_table"] > 256 and host.max("dwell_us") > 0 and host.layer("flow_x").min() < 0 < host.layer("flow_x").max(), st
    dev.close()


# ------------------------------------------------------------------------------------------------ 2. burst
def test_more_than_a_workgroup_of_rows_on_one_cell_then_all_gone():
    """700 rows of one frame (300 of them of another class) land on one interior cell, stay one frame, then all vanish."""
    dev = H.DeviceHeatMap(H.HeatSpec(64, 64, cell=16, class_id=1), max_age=1)
    host = dev.host()
    crowd = [foot(20 + i % 9, 20 + i % 7, i + 1, 1 if i % 7 < 4 else 0) for i in range(700)]
    n_in = sum(1 for r in crowd if r[5] == 1)
    _feed(dev, [host], [(0, crowd, 0.0), (0, crowd[::-1], 0.5), (0, [], 1.0), (0, [], 1.5), (0, crowd[:3], 2.0)])
    assert n_in == 400 and host.layer("presence")[1, 1] == 2 * n_in + 3 and host.layer("visits")[1, 1] == n_in + 3
    assert host.layer("dwell_us")[1, 1] == n_in * 500000 and host.stats["max_table"] == n_in and len(host.tracks()) == 3
    assert host.layer("presence").sum() == 2 * n_in + 3 and host.stats["returned"] == 3
    dev.close()


# ------------------------------------------------------------------------------------------------ 3. several streams
def test_streams_of_different_specs_interleaved_in_one_call():
    """Four streams with different (h, w, cell, class_id), their frames interleaved in one call, one stream absent from the second
    call; each equals its own host map, and a reset of one stream leaves the others alone."""
    specs = [H.HeatSpec(150, 200, 16, 0), H.HeatSpec(90, 70, 4, -1), H.HeatSpec(300, 500, 64, 2), H.HeatSpec(33, 50, 8, 1)]
    dev = H.DeviceHeatMap(specs, max_age=2, n_streams=4)
    hosts = [dev.host(s) for s in range(4)]
    scenes = [crowd_scene(11 + s, 60, 12, sp.h, sp.w) for s, sp in enumerate(specs)]
    frames = [(s, scenes[s][t][0], scenes[s][t][1]) for t in range(6) for s in (2, 0, 3, 1)]
    frames.insert(5, (1, None, 9.0))                                   # a frame the tracker was not called for
    _feed(dev, hosts, frames)
    _feed(dev, hosts, [(s, scenes[s][t][0], scenes[s][t][1]) for t in range(6, 12) for s in (3, 0, 1)])
    assert all(h.layer("presence").sum() > 50 and h.layer("dwell_us").sum() > 0 for h in hosts)
    assert [h.stats["ignored_rows"] > 0 for h in hosts] == [True, False, True, True]
    dev.reset(1)
    hosts[1].reset()
    _same_state(dev, hosts)
    assert not dev.layers(1).any() and dev.tracks(1) == [] and dev.layers(0).any()
    _feed(dev, hosts, [(1, scenes[1][0][0], 20.0), (2, scenes[2][0][0], 20.0)])
    dev.reset()
    assert not any(dev.layers(s).any() or dev.tracks(s) for s in range(4))
    dev.close()


# ------------------------------------------------------------------------------------------------ 4. the largest grid
def test_largest_grid_corners_and_the_partial_column():
    """1024 x 1021 at cell 4: 256 x 256 = 65536 cells, the last column partial (one pixel wide); rows in the four corner cells, on the
    partial column's far edge beyond the frame, and just outside."""
    spec = H.HeatSpec(1024, 1021, cell=4, class_id=-1)
    assert spec.gw * spec.gh == 65536 and spec.gw == 256
    dev = H.DeviceHeatMap(spec, max_age=2)
    host = dev.host()
    rows = [foot(0, 0, 1), foot(1020, 0, 2), foot(0, 1023, 3), foot(1023, 1023, 4), foot(1023, 512, 5), foot(1024, 5, 6), foot(5, 1024, 7)]
    _feed(dev, [host], [(0, rows, 0.0), (0, rows, 1.0)])
    p = host.layer("presence")
    assert p[0, 0] == p[0, 255] == p[255, 0] == p[255, 255] == p[128, 255] == 2 and p.sum() == 10 and host.stats["outside_rows"] == 4
    assert host.max("dwell_us") == 1000000
    dev.close()


# ------------------------------------------------------------------------------------------------ 5. render
def _painted(spec, seed, streams=1):
    """A DeviceHeatMap whose layers hold a few hot spots (every layer different), with its host maps."""
    dev = H.DeviceHeatMap(spec, max_age=2, n_streams=streams)
    hosts = [dev.host(s) for s in range(streams)]
    rs = np.random.RandomState(seed)
    for s in range(streams):
        n = 12 + 5 * s
        x, y = rs.randint(0, spec.w, n), rs.randint(0, spec.h, n)
        for t in range(5):
            keep = rs.rand(n) < 0.8
            rows = [foot(int(x[i]), int(y[i]), i + 1, spec.class_id) for i in range(n) if keep[i]]
            _feed(dev, hosts, [(s, rows, 0.3 * t)])
            step = rs.randint(-spec.cell, spec.cell + 1, (2, n)) * (rs.rand(n) < 0.5)
            x, y = np.clip(x + step[0], 0, spec.w - 1), np.clip(y + step[1], 0, spec.h - 1)
    return dev, hosts


@pytest.mark.parametrize("h,w,cell", [(33, 50, 4), (33, 50, 16), (64, 64, 16), (120, 92, 32), (17, 9, 128)])
def test_render_equals_the_host_render(h, w, cell):
    """Four frames in HBM, slots [3, 0, 2] rendered from two streams (slot 1 must come back untouched): all three renderable
    layers, vmax 0 and an explicit vmax below the maximum, alpha 1 / 128 / 256, a custom LUT and its reverse (the other channel
    order), the frames at an aligned and at an odd base address, and an all-zero grid."""
    from yolo_deepsort_amd import _lib
    spec = H.HeatSpec(h, w, cell=cell, class_id=0)
    dev, hosts = _painted(spec, 5 + cell, streams=2)
    rs = np.random.RandomState(h * w)
    frames = rs.randint(0, 256, (4, h, w, 3)).astype(np.uint8)
    lut = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    slots, sof = [3, 0, 2], [1, 0, 1]
    touched = 0
    for shift in (0, 1):
        buf = _lib.DeviceBuffer(frames.nbytes + 4)
        base = buf.offset(shift)
        assert (base.value % 2 == 1) == (shift == 1)
        for layer in H.RENDERABLE:
            top = max(hosts[s].max(layer) for s in (0, 1))
            assert top >= 2, layer
            for vmax in (0, max(top // 2, 1)):
                for alpha, table in ((128, lut), (1, None), (256, lut[:, ::-1])):
                    _lib.check(_lib.load().yds_memcpy_h2d(base, _lib.ptr(frames), frames.nbytes))
                    dev.render(base, slots, sof, h, w, layer=layer, vmax=vmax, alpha=alpha, lut=table, n_frames=4)
                    got = np.zeros_like(frames)
                    _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(got), base, frames.nbytes))
                    want = frames.copy()
                    for slot, s in zip(slots, sof):
                        want[slot] = H.render(frames[slot], hosts[s].layer(layer), cell, vmax=vmax, lut=table, alpha=alpha)
                    assert np.array_equal(got, want), (shift, layer, vmax, alpha)
                    assert np.array_equal(got[1], frames[1])
                    touched += int((want != frames).any(axis=3).sum())
        buf.free()
    assert touched > 0
    # an all-zero grid leaves every byte as it was
    dev.reset(1)
    buf = _lib.DeviceBuffer.from_array(frames)
    dev.render(buf.ptr, [0, 1, 2, 3], [1, 1, 1, 1], h, w, alpha=256)
    got = np.zeros_like(frames)
    _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(got), buf.ptr, frames.nbytes))
    assert np.array_equal(got, frames)
    dev.close()


def test_render_one_1080p_frame_bit_for_bit():
    """1080 x 1920 at cell 16: 67.5 cells high, the wide path."""
    from yolo_deepsort_amd import _lib
    spec = H.HeatSpec(1080, 1920, cell=16, class_id=0)
    assert (spec.gh, spec.gw) == (68, 120)
    dev, hosts = _painted(spec, 3)
    _feed(dev, hosts, [(0, [foot(1900, 1079, 99), foot(3, 2, 98), foot(960, 1070, 97)], 9.0)])
    frame = np.random.RandomState(8).randint(0, 256, (1, 1080, 1920, 3)).astype(np.uint8)
    buf = _lib.DeviceBuffer.from_array(frame)
    dev.render(buf.ptr, [0], [0], 1080, 1920, layer="presence", alpha=160)
    got = np.zeros_like(frame)
    _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(got), buf.ptr, frame.nbytes))
    want = H.render(frame[0], hosts[0].layer("presence"), 16, alpha=160)
    changed = (want != frame[0]).any(axis=2)
    assert np.array_equal(got[0], want) and 1000 < changed.sum() < changed.size and changed[1079].any() and changed[0].any()
    dev.close()


# ------------------------------------------------------------------------------------------------ 6. inside the step
@functools.lru_cache(maxsize=None)
def _net(batch_max, bias=-1.45):
    from yolo_deepsort_amd.models import Darknet
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=batch_max, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, bias))       # a handful of (random) detections per frame
    return net


def _clip(seed, hw, n, roll=3):
    img = np.random.RandomState(seed).randint(0, 256, hw + (3,)).astype(np.uint8)
    return [np.roll(img, roll * t, axis=1) for t in range(n)]


@pytest.mark.parametrize("mode", ["multi", "mixed", "windows"])
def test_step_heatmaps_equal_host_maps_and_leave_everything_else_alone(mode):
    """yolov3-tiny 416 with random weights over three cameras for 8 steps, actions, zones and identities all on: a multi-stream step
    (480 x 640, look-ahead), a mixed-size step (three sizes) and a per-stream-window step (the cameras A, D, E of
    test_gpu_stream_windows.py: 416 x 416 windows, none, 320 x 240 windows; one frame per camera, repeated; batch_max 5, so that the
    9 slots run as 5 + 4).
    heatmap() after the steps equals host HeatMaps fed the returned rows and the frame times; a second pipeline without the stage
    returns the same rows, actions, zone events and identities.  set_heatmap(None) takes the launch away again, and set_heatmap
    is refused while a look-ahead pass is in flight."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    _lib.init(0)
    sizes = [(480, 640), (270, 480), (416, 416)] if mode == "mixed" else [(480, 640)] * 3
    n_steps, net = 8, (_net(5, -1.3) if mode == "windows" else _net(8))
    clips = [_clip(20 + ord("ADE"[s]), sizes[s], n_steps, 0) if mode == "windows" else _clip(40 + s, sizes[s], n_steps) for s in range(3)]
    specs = [H.HeatSpec(sizes[0][0], sizes[0][1], 32, -1), H.HeatSpec(sizes[1][0], sizes[1][1], 16, -1), H.HeatSpec(sizes[2][0], sizes[2][1], 64, -1)]
    packs = [pl.pack_frames([clips[s][i] for s in range(3)]) for i in range(n_steps)]
    devs = [_lib.DeviceBuffer.from_array(p[0]) for p in packs]
    ex = Extractor(synth.reid_state_dict(0), max_crops=256)
    ident = A.ActionIdentify([A.Glide(0, (0, 3)), A.FastCrossing(0, 0.01)], max_age=2, max_size=3)
    zones = ([Z.Zone([(0, 0), (240, 0), (240, 270), (0, 270)], name="left")], [Z.Line((200, 0), (200, 400))])
    time_of = lambda s, i: 0.04 * i + 0.001 * s          # noqa: E731
    ahead = mode == "multi"

    def run(with_heat):
        trackers = [DeepSort(ex, use_cuda=True, **DS) for _ in range(3)]
        kw = dict(stream_win_sizes=[(416, 416), None, (320, 240)], overlap=0.15) if mode == "windows" else {}
        pipe = pl.MultiStreamPipeline(net, trackers, 0.5, 0.4, **kw)
        pipe.set_actions(ident)
        pipe.set_zones(zones, max_age=2)
        pipe.set_identities(True)
        assert pipe.heatmap() is None
        heat = None
        if with_heat:
            with pytest.raises(ValueError, match="heatmap"):
                pipe.set_heatmap(specs[:2])
            heat = pipe.set_heatmap(specs, max_age=2)
            heat.set_timing(True)
        rows, other = [], []
        for i in range(n_steps):
            pipe.set_frame_times([time_of(s, i) for s in range(3)])
            nxt = ahead and i + 1 < n_steps
            if mode == "mixed":
                outs = pipe.step_mixed(devs[i].ptr, packs[i][1], packs[i][2], [0, 1, 2], packs[i][0].nbytes)
            else:
                outs = pipe.step(devs[i].ptr, 480, 640, [0, 1, 2], devs[i + 1].ptr if nxt else None)
            if with_heat and nxt and i == 2:
                with pytest.raises(_lib.YdsError, match="look-ahead"):
                    pipe.set_heatmap(None)
            rows.append(outs)
            other.append((pipe.last_actions(), pipe.last_zone_events(), pipe.last_identities()))
        return pipe, heat, rows, other
    pipe, heat, rows, other = run(True)
    hosts = [H.HeatMap(specs[s], max_age=2) for s in range(3)]
    counted = 0
    for i in range(n_steps):
        for s in range(3):
            counted += hosts[s].update(rows[i][s], time_of(s, i)) or 0
    got = pipe.heatmap()
    for s in range(3):
        assert np.array_equal(got[s], hosts[s].layers()), s
        assert np.array_equal(pipe.heatmap(s, "dwell_us"), hosts[s].layer("dwell_us")) and heat.tracks(s) == hosts[s].tracks()
    assert counted >= 6 and sum(h.layer("presence").sum() for h in hosts) >= 6 and sum(h.stats["dwell_credits"] for h in hosts) >= 3
    assert 0 < heat.last_us("update") < 1e6
    # without the stage: the same everything else
    _, _, plain_rows, plain_other = run(False)
    for i in range(n_steps):
        assert other[i] == plain_other[i], i
        for a, p in zip(rows[i], plain_rows[i]):
            assert (a is None) == (p is None) and (a is None or (a.shape == p.shape and np.array_equal(a, p))), i
    assert any(r is not None and len(r) for st in rows for r in st)
    # switched off again: the step launches nothing of the stage (no timed launch since the timer was re-armed) and the layers stand
    pipe.set_heatmap(None)
    assert pipe.heatmap() is None
    heat.set_timing(True)
    before = [heat.layers(s) for s in range(3)]
    if mode == "mixed":
        pipe.step_mixed(devs[0].ptr, packs[0][1], packs[0][2], [0, 1, 2], packs[0][0].nbytes)
    else:
        pipe.step(devs[0].ptr, 480, 640, [0, 1, 2])
    with pytest.raises(_lib.YdsError, match="no timed launch"):
        heat.last_us("update")
    assert all(np.array_equal(heat.layers(s), before[s]) for s in range(3))
    heat.close()


def test_single_stream_pipeline_takes_a_host_map():
    """Pipeline.set_heatmap(HeatMap): its spec and max_age go to the device; frame k of the stream carries k / 25."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    _lib.init(0)
    net = _net(8)
    ds = DeepSort(Extractor(synth.reid_state_dict(0), max_crops=64), use_cuda=True, **DS)
    clip = _clip(50, (480, 640), 12)
    host = H.HeatMap(H.HeatSpec(480, 640, 32, -1), max_age=4)
    pipe = pl.Pipeline(net, ds, 0.5, 0.4)
    dev = pipe.set_heatmap(host)
    assert dev.max_age == 4 and dev.specs == [host.spec]
    counted = 0
    for i in range(6):
        buf = _lib.DeviceBuffer.from_array(np.stack(clip[2 * i:2 * i + 2]))
        outs = pipe.step(buf.ptr, 480, 640, 2)
        for b in range(2):
            counted += host.update(outs[b], (2 * i + b) / 25.0) or 0
    assert counted >= 2 and np.array_equal(pipe.heatmap(), host.layers()) and np.array_equal(pipe.heatmap(0, "visits"), host.layer("visits"))
    with pytest.raises(ValueError, match="heatmap"):
        pipe.set_heatmap(object())
    pipe.set_heatmap(None)
    assert pipe.heatmap() is None


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_through_the_c_entries():
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    lib = _lib.load()
    err = _lib.last_error
    assert not lib.yds_heatmap_create(1, 0) and "max_age" in err()
    assert not lib.yds_heatmap_create(0, 3) and "streams" in err()
    h = _lib.check_ptr(lib.yds_heatmap_create(3, 2))
    for args, word in [((0, 100, 100, 5, 0), "cell 5"), ((0, 100, 100, 2, 0), "cell 2"), ((0, 100, 100, 256, 0), "cell 256"),
                       ((0, 100, 100, 0, 0), "cell 0"), ((0, 1028, 1024, 4, 0), "exceeds 65536"), ((3, 100, 100, 16, 0), "stream 3"),
                       ((-1, 100, 100, 16, 0), "stream -1"), ((0, 0, 100, 16, 0), "frame of"), ((0, 100, 100, 16, -2), "class_id")]:
        assert lib.yds_heatmap_set_stream(h, *args) != 0 and word in err(), (args, err())
    assert lib.yds_heatmap_set_stream(h, 0, 48, 64, 16, 0) == 0 and lib.yds_heatmap_set_stream(h, 1, 48, 64, 8, -1) == 0
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)          # noqa: E731
    a = foot(10, 10, 1)
    tm = np.zeros(1)

    def update(rows, stream):
        rows = i32(rows)
        return lib.yds_heatmap_update(h, _lib.ptr(rows), _lib.ptr(i32([0, len(rows)])), _lib.ptr(i32([stream])), _lib.ptr(tm), 1, None)
    assert update([a, a], 0) != 0 and "twice" in err()
    assert update([a], 5) != 0 and "stream 5" in err()
    assert update([a], 2) != 0 and "no spec" in err()                # a stream without a spec
    assert update([a], 0) == 0
    out, n, v = np.zeros((5, 3, 4), np.int64), C.c_int(0), C.c_int64(0)
    assert lib.yds_heatmap_get_layers(h, 0, _lib.ptr(out), 59) != 0 and "capacity" in err()
    assert lib.yds_heatmap_get_layers(h, 0, _lib.ptr(out), 60) == 0 and out[0, 0, 0] == 1 and out.sum() == 2
    assert lib.yds_heatmap_get_layers(h, 2, _lib.ptr(out), 60) != 0 and "no spec" in err()
    assert lib.yds_heatmap_get_layers(h, 3, _lib.ptr(out), 60) != 0 and "stream" in err()
    assert lib.yds_heatmap_get_max(h, 0, 5, C.byref(v)) != 0 and "layer" in err()
    assert lib.yds_heatmap_get_max(h, 2, 0, C.byref(v)) != 0 and "no spec" in err()
    assert lib.yds_heatmap_get_max(h, 0, 1, C.byref(v)) == 0 and v.value == 1
    assert lib.yds_heatmap_get_tracks(h, 3, None, None, None, None, None, 0, C.byref(n)) != 0 and "stream" in err()
    assert lib.yds_heatmap_get_tracks(h, 0, None, None, None, None, None, 0, C.byref(n)) != 0 and "1 tracks" in err() and n.value == 1
    assert lib.yds_heatmap_reset(h, 3) != 0 and "stream" in err()
    us = C.c_float(0)
    for what in (0, 1):
        assert lib.yds_heatmap_last_us(h, what, C.byref(us)) != 0 and "timed" in err()
    assert lib.yds_heatmap_last_us(h, 2, C.byref(us)) != 0 and "last_us" in err()
    # render: every bad argument is refused before anything launches - the frames stay as they were
    frames = np.random.RandomState(0).randint(0, 256, (3, 48, 64, 3)).astype(np.uint8)
    buf = _lib.DeviceBuffer.from_array(frames)
    lut = H.lut_heat()

    def render(slots, sof, hh=48, ww=64, layer=0, vmax=0, alpha=128, n_src=3):
        return lib.yds_heatmap_render(h, buf.ptr, n_src, _lib.ptr(i32(slots)), _lib.ptr(i32(sof)), len(slots), hh, ww, layer, vmax, alpha,
                                      _lib.ptr(lut))
    for kw, word in [(dict(slots=[0, 3], sof=[0, 0]), "slot 3"), (dict(slots=[0, -1], sof=[0, 0]), "slot -1"),
                     (dict(slots=[1, 2, 1], sof=[0, 0, 0]), "same slot 1"), (dict(slots=[0], sof=[3]), "stream 3"),
                     (dict(slots=[0], sof=[2]), "no spec"), (dict(slots=[0], sof=[0], hh=64, ww=48), "spec is 48 x 64"),
                     (dict(slots=[0], sof=[0], layer=3), "not renderable"), (dict(slots=[0], sof=[0], layer=-1), "not renderable"),
                     (dict(slots=[0], sof=[0], vmax=-1), "vmax"), (dict(slots=[0], sof=[0], vmax=(1 << 47) + 1), "vmax"),
                     (dict(slots=[0], sof=[0], alpha=0), "alpha"), (dict(slots=[0], sof=[0], alpha=257), "alpha"),
                     (dict(slots=[0], sof=[0], n_src=0), "NULL")]:
        assert render(**kw) != 0 and word in err(), (kw, err())
    assert render([2], [0], vmax=1 << 47) == 0 and render([0, 1], [1, 1]) == 0          # (stream 1 is empty: nothing changes)
    got = np.zeros_like(frames)
    _lib.check(lib.yds_memcpy_d2h(_lib.ptr(got), buf.ptr, frames.nbytes))
    assert np.array_equal(got[:2], frames[:2]) and np.array_equal(got[2], H.render(frames[2], out[0], 16, vmax=1 << 47))
    lib.yds_heatmap_destroy(h)
    # vmax = 0 whose reduced maximum exceeds 2^47: refused, no frame touched (a day of dwell per frame for 1630 frames)
    dev = H.DeviceHeatMap(H.HeatSpec(48, 64, 16, 0), max_age=2)
    host = dev.host()
    _feed(dev, [host], [(0, [a], 86400.0 * k) for k in range(1631)])
    assert host.max("dwell_us") == 1630 * 86400 * 10 ** 6 > 1 << 47
    _lib.check(lib.yds_memcpy_h2d(buf.ptr, _lib.ptr(frames), frames.nbytes))
    with pytest.raises(_lib.YdsError, match="exceeds 2\\^47"):
        dev.render(buf.ptr, [0], [0], 48, 64, layer="dwell_us")
    with pytest.raises(ValueError, match="2\\^47"):
        H.render(frames[0], host.layer("dwell_us"), 16)
    _lib.check(lib.yds_memcpy_d2h(_lib.ptr(got), buf.ptr, frames.nbytes))
    assert np.array_equal(got, frames)
    dev.render(buf.ptr, [0], [0], 48, 64, layer="dwell_us", vmax=1 << 47)
    _lib.check(lib.yds_memcpy_d2h(_lib.ptr(got), buf.ptr, frames.nbytes))
    assert np.array_equal(got[0], H.render(frames[0], host.layer("dwell_us"), 16, vmax=1 << 47)) and not np.array_equal(got[0], frames[0])
    with pytest.raises(ValueError, match="layer"):
        dev.render(buf.ptr, [0], [0], 48, 64, layer="speed")
    with pytest.raises(_lib.YdsError, match="not renderable"):
        dev.render(buf.ptr, [0], [0], 48, 64, layer="flow_x")
    dev.set_timing(True)
    dev.update(0, [a], 1.0)
    dev.render(buf.ptr, [1], [0], 48, 64)
    assert 0 < dev.last_us("update") < 1e6 and 0 < dev.last_us("render") < 1e6
    dev.close()
