"""Ground plane on the device (csrc/ground.hip): every camera's rows through its homography onto one floor plan - records, one site
grid of five int64 layers for all streams, per-stream tables with a ring of plan positions - and the two renders.  The comparator is
the host definition (yolo_deepsort_amd.ground: GroundMap, render_view) fed the same rows, times and frames; one floating-point step
per point and integers after it, so records, layers, maxima, tables and pixels are compared with exact equality.  What the scenes
exercise is asserted on the host's statistics in test_ground_host.py and again where a scene is used here."""
import functools

import numpy as np
import pytest

import ground_common as gc
from yolo_deepsort_amd import action as A, cfgs, ground as G, heatmap as H, synth, zones as Z

pytestmark = pytest.mark.gpu
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)


def _same_state(dev, host):
    got = dev.layers()
    assert got.dtype == np.int64 and np.array_equal(got, host.layers())
    for name in H.LAYERS:
        assert dev.max(name) == host.max(name), name
    for s in range(host.n_streams):
        assert dev.tracks(s) == host.tracks(s), s


def _same_records(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), k
        if w is not None:
            assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), (k, g[:4], w[:4])


def _call(dev, frames):
    return dev.update_batch([r for _, r, _ in frames], [s for s, _, _ in frames], [t for _, _, t in frames])


# ------------------------------------------------------------------------------------------------ 1. the division pin
def test_device_quotients_equal_numpy():
    """4096 (H, point) pairs, one row per frame, through the stand-alone entry in one call: (qx, qy, cell) - the whole record - equals
    the host, W near 0, W < 0, infinities and |p * scale| on and one ulp either side of 2^29 included."""
    specs, cases = gc.division_cases()
    dev = G.DeviceGroundMap(specs, max_age=30, speed_window=8)
    host = dev.host()
    frames = [(h, [row], 0.01 * k) for k, (h, row, _) in enumerate(cases)]
    got = _call(dev, frames)
    want = [host.update(s, r, t) for s, r, t in frames]
    _same_records(got, want)
    on = np.array([w[0, 7] != G.OFF_PLANE for w in want])
    assert len(want) == 4096 and all(w is None or w == o for (_, _, w), o in zip(cases, on)) and 1000 < on.sum() < 3800
    assert want[0][0, 2] == 1 << 29 and want[4][0, 2] == -(1 << 29) and host.stats["outside_rows"] > 100
    _same_state(dev, host)
    dev.close()


# ------------------------------------------------------------------------------------------------ 2. randomised
def test_random_scene_equals_the_host_map():
    """Three cameras with different H on one 40 x 30 plan, 300 ids of three classes over 40 frames, in two calls: records, the five
    layers, maxima and tables equal the host after each call."""
    frames = gc.plan_scene()
    host, (mid_layers, mid_tracks), recs = gc.host_scene()
    dev = G.DeviceGroundMap(gc.scene_specs(), **gc.SCENE_KW)
    half = len(frames) // 2
    _same_records(_call(dev, frames[:half]), recs[:half])
    assert np.array_equal(dev.layers(), mid_layers) and [dev.tracks(s) for s in range(3)] == mid_tracks
    _same_records(_call(dev, frames[half:]), recs[half:])
    _same_state(dev, host)
    st = host.stats
    assert st["off_plane_rows"] >= 50 and st["outside_rows"] >= 200 and st["multi_camera_cells"] >= 100 and st["gap_sightings"] >= 100, st
    assert st["ring_wraps"] >= 100 and st["max_table"] > 256, st
    dev.close()


# ------------------------------------------------------------------------------------------------ 3. burst
def test_two_cameras_burst_on_one_cell_then_all_gone():
    """700 rows from two cameras land on one cell of the site grid in one call (the atomics of two workgroups meet), stay a frame,
    then all vanish."""
    specs, frames = gc.burst_scene()
    host, recs = gc.host_burst()
    dev = G.DeviceGroundMap(specs, max_age=1, speed_window=8)
    _same_records(_call(dev, frames), recs)
    _same_state(dev, host)
    assert host.layer("presence")[10, 20] == 1403 and host.layer("dwell_us")[10, 20] == 700 * 500000 and len(host.tracks(0)) == 3
    dev.close()


# ------------------------------------------------------------------------------------------------ 4. skipped streams, reset
def test_a_stream_without_a_spec_is_skipped_and_reset_is_per_stream():
    sp = gc.scene_specs()
    dev = G.DeviceGroundMap([sp[2], None, sp[0]], max_age=2, speed_window=3)
    host = dev.host()
    frames = [(s, r, t) for s, r, t in gc.plan_scene()[:30]]
    frames = [({2: 0, 0: 2, 1: 1}[s], r, t) for s, r, t in frames]               # (camera 1's rows go to the stream without a spec)
    got = _call(dev, frames)
    _same_records(got, [host.update(s, r, t) for s, r, t in frames])
    assert all(g.shape == (0, 8) for (s, _, _), g in zip(frames, got) if s == 1) and dev.tracks(1) == []
    assert sum(len(r) for s, r, _ in frames if s == 1) > 500 and len(dev.tracks(0)) > 20 and len(dev.tracks(2)) > 100
    _same_state(dev, host)
    grid = dev.layers()
    dev.reset(2)
    host.reset(2)
    assert dev.tracks(2) == [] and len(dev.tracks(0)) > 20 and np.array_equal(dev.layers(), grid)
    more = [(2, gc.plan_scene()[30][1], 5.0), (0, gc.plan_scene()[32][1], 5.0)]
    _same_records(_call(dev, more), [host.update(s, r, t) for s, r, t in more])
    _same_state(dev, host)
    dev.reset()
    assert not dev.layers().any() and not any(dev.tracks(s) for s in range(3))
    dev.close()


# ------------------------------------------------------------------------------------------------ 5. inside the step
@functools.lru_cache(maxsize=None)
def _net(batch_max):
    from yolo_deepsort_amd.models import Darknet
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=batch_max, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, -1.45))       # a handful of (random) detections per frame
    return net


def _clip(seed, hw, n, roll=3):
    img = np.random.RandomState(seed).randint(0, 256, hw + (3,)).astype(np.uint8)
    return [np.roll(img, roll * t, axis=1) for t in range(n)]


def _camera_specs(sizes):
    """A pinhole per camera looking at the one plan from its own place (stream 1: none, when asked for)."""
    turn = np.array([[0.0, -1.0, 9.0], [1.0, 0.0, 5.0], [0.0, 0.0, 1.0]])
    out = []
    for s, (h, w) in enumerate(sizes):
        Hs = gc.pinhole_H(height=3.0 + s, tilt_deg=20.0 + 5 * s, f=0.9 * w, cx=w / 2, cy=h / 2)
        out.append(G.GroundSpec(turn @ Hs if s == 2 else Hs, class_id=-1, **gc.PLAN))
    return out


@pytest.mark.parametrize("mode", ["multi", "mixed"])
def test_step_ground_equals_the_host_and_leaves_everything_else_alone(mode):
    """yolov3-tiny 416 with random weights over three cameras for 6 steps with actions, zones, heat maps and identities all on: a
    plain multi-stream step (480 x 640, look-ahead) and a mixed-size step.  last_ground() of every step equals the host GroundMap fed
    the step's rows and frame times, ground_layers() its site grid; a second pipeline without the stage returns the same rows,
    actions, zone events, heat maps and identities.  set_ground is refused while a look-ahead pass is in flight."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    _lib.init(0)
    sizes = [(480, 640), (270, 480), (416, 416)] if mode == "mixed" else [(480, 640)] * 3
    n_steps, net = 6, _net(8)
    clips = [_clip(40 + s, sizes[s], n_steps) for s in range(3)]
    specs = _camera_specs(sizes)
    heat_specs = [H.HeatSpec(h, w, 32, -1) for h, w in sizes]
    packs = [pl.pack_frames([clips[s][i] for s in range(3)]) for i in range(n_steps)]
    devs = [_lib.DeviceBuffer.from_array(p[0]) for p in packs]
    ex = Extractor(synth.reid_state_dict(0), max_crops=256)
    ident = A.ActionIdentify([A.Glide(0, (0, 3)), A.FastCrossing(0, 0.01)], max_age=2, max_size=3)
    zones = ([Z.Zone([(0, 0), (240, 0), (240, 270), (0, 270)], name="left")], [Z.Line((200, 0), (200, 400))])
    time_of = lambda s, i: 0.04 * i + 0.001 * s          # noqa: E731
    ahead = mode == "multi"

    def run(with_ground):
        trackers = [DeepSort(ex, use_cuda=True, **DS) for _ in range(3)]
        pipe = pl.MultiStreamPipeline(net, trackers, 0.5, 0.4)
        pipe.set_actions(ident)
        pipe.set_zones(zones, max_age=2)
        pipe.set_heatmap(heat_specs, max_age=2)
        pipe.set_identities(True)
        assert pipe.last_ground() is None and pipe.ground_layers() is None
        ground = None
        if with_ground:
            with pytest.raises(ValueError, match="ground"):
                pipe.set_ground(specs[:2])
            ground = pipe.set_ground(specs, max_age=2)
            ground.set_timing(True)
        rows, other, recs = [], [], []
        for i in range(n_steps):
            pipe.set_frame_times([time_of(s, i) for s in range(3)])
            nxt = ahead and i + 1 < n_steps
            if mode == "mixed":
                outs = pipe.step_mixed(devs[i].ptr, packs[i][1], packs[i][2], [0, 1, 2], packs[i][0].nbytes)
            else:
                outs = pipe.step(devs[i].ptr, 480, 640, [0, 1, 2], devs[i + 1].ptr if nxt else None)
            if with_ground and nxt and i == 2:
                with pytest.raises(_lib.YdsError, match="look-ahead"):
                    pipe.set_ground(None)
            rows.append(outs)
            other.append((pipe.last_actions(), pipe.last_zone_events(), pipe.last_identities(), [h.tolist() for h in pipe.heatmap()]))
            if with_ground:
                recs.append((pipe.last_ground(), pipe.last_ground(2)))
        return pipe, ground, rows, other, recs
    pipe, ground, rows, other, recs = run(True)
    host = G.GroundMap(specs, max_age=2)
    counted = 0
    for i in range(n_steps):
        want = [host.update(s, rows[i][s], time_of(s, i)) for s in range(3)]
        _same_records(recs[i][0], want)
        assert np.array_equal(recs[i][1], want[2] if want[2] is not None else np.zeros((0, 8), np.int32))
        counted += sum(len(w) for w in want if w is not None)
    assert np.array_equal(pipe.ground_layers(), host.layers()) and np.array_equal(pipe.ground_layers("dwell_us"), host.layer("dwell_us"))
    assert all(ground.tracks(s) == host.tracks(s) for s in range(3))
    assert counted >= 6 and host.stats["consecutive"] >= 3 and 0 < ground.last_us("update") < 1e6, host.stats
    # without the stage: the same everything else
    _, _, plain_rows, plain_other, _ = run(False)
    for i in range(n_steps):
        assert other[i] == plain_other[i], i
        for a, p in zip(rows[i], plain_rows[i]):
            assert (a is None) == (p is None) and (a is None or (a.shape == p.shape and np.array_equal(a, p))), i
    # switched off again: the step launches nothing of the stage and the grid stands
    pipe.set_ground(None)
    assert pipe.last_ground() is None
    ground.set_timing(True)
    before = ground.layers()
    if mode == "mixed":
        pipe.step_mixed(devs[0].ptr, packs[0][1], packs[0][2], [0, 1, 2], packs[0][0].nbytes)
    else:
        pipe.step(devs[0].ptr, 480, 640, [0, 1, 2])
    with pytest.raises(_lib.YdsError, match="no timed launch"):
        ground.last_us("update")
    assert np.array_equal(ground.layers(), before)
    ground.close()


def test_detect_streams_takes_the_ground_plane(tmp_path):
    """detect_streams(ground=...) over two in-memory clips of different sizes, the second camera without a spec: between the yields
    stream_ground() holds the step's records and site_map() the site grid of a host GroundMap fed the yielded rows; the yielded rows
    are those of a run without the option; outside the generator stream_ground() raises ValueError."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import DeepSort
    from yolo_deepsort_amd.detect import VideoDetector
    _lib.init(0)
    net = _net(8)
    base = DeepSort(synth.reid_state_dict(0), use_cuda=True, **DS)
    clips = [_clip(21, (480, 640), 21), _clip(22, (270, 480), 7)]
    specs = [_camera_specs([(480, 640)])[0], None]
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())

    def detector():
        return VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=base, skip_frames=2, class_mask=list(range(0, 80, 2)))
    plain = [[(s, det) for s, _, det, _ in step] for step in detector().detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True)]
    vd = detector()
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_ground()
    host = G.GroundMap(specs, max_age=3)
    seen, items, counted = [0, 0], [], 0
    for step in vd.detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True, ground=specs, ground_max_age=3):
        want = [[], []]
        for s, _, det, _ in step:
            if seen[s] % 2 == 0:                                      # a processed frame
                want[s].append(host.update(s, det, seen[s] / 25.0))
            seen[s] += 1
        got = vd.stream_ground()
        for s in range(2):
            _same_records(got[s], want[s])
            counted += sum(len(w) for w in want[s] if w is not None)
        _same_records(vd.stream_ground(0), want[0])
        assert np.array_equal(vd.site_map(), host.layer("presence")) and np.array_equal(vd.site_map(None), host.layers())
        items.append([(s, det) for s, _, det, _ in step])
    assert seen == [21, 7] and counted >= 3
    with pytest.raises(ValueError, match="between the yields"):
        vd.site_map()
    assert len(items) == len(plain)
    for a, b in zip(items, plain):
        assert [s for s, _ in a] == [s for s, _ in b]
        assert all((x is None) == (y is None) and (x is None or np.array_equal(x, y)) for (_, x), (_, y) in zip(a, b))
    with pytest.raises(ValueError, match="ground"):
        next(detector().detect_streams(clips, mixed_sizes=True, ground=[specs[0]]))
    with pytest.raises(ValueError, match="ground="):
        vd2 = detector()
        for _ in vd2.detect_streams(clips, frames_per_stream=1, show_fps=False, mixed_sizes=True):
            vd2.stream_ground()


# ------------------------------------------------------------------------------------------------ 6. render_view
def _painted():
    """A site grid with hot spots seen by the reference camera (stream 0), a lower and steeper one (stream 1) and a stream without
    a spec: the plan scene's walkers through the scene's cameras fill every layer."""
    ref = gc.reference_spec(class_id=-1)
    low = G.GroundSpec(gc.pinhole_H(height=2.0, tilt_deg=30.0, f=60.0, cx=40.0, cy=20.0), class_id=-1, **gc.PLAN)
    dev = G.DeviceGroundMap([ref, low, None], max_age=2, speed_window=4)
    host = dev.host()
    rs = np.random.RandomState(4)
    for t in range(6):
        for s in (0, 1):
            n = 40
            u, v = rs.randint(0, 96, n), rs.randint(12, 64, n)
            rows = [[int(u[i]) - 2, int(v[i]) - 9, int(u[i]) + 2, int(v[i]), i + 1, 0] for i in range(n)]
            _same_records(_call(dev, [(s, rows, 0.2 * t)]), [host.update(s, rows, 0.2 * t)])
    return dev, host


@pytest.mark.parametrize("h,w", [(33, 50), (24, 36), (64, 96)])
def test_render_view_equals_the_host_render(h, w):
    """Four frames in HBM, slots [3, 0, 2] rendered as pictures of cameras [1, 0, 1] (two H in one call; slot 1 must come back
    untouched): all three renderable layers, vmax 0 and an explicit one, alpha 1 / 128 / 256, a custom LUT, the frames at an aligned
    base (33 x 50: the byte path, 24 x 36: dwords, 64 x 96: the 16-byte path) and at a base off by one byte (the byte path)."""
    from yolo_deepsort_amd import _lib
    dev, host = _painted()
    rs = np.random.RandomState(h * w)
    frames = rs.randint(0, 256, (4, h, w, 3)).astype(np.uint8)
    lut = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    slots, sof = [3, 0, 2], [1, 0, 1]
    touched, kept = 0, 0
    for shift in (0, 1):
        buf = _lib.DeviceBuffer(frames.nbytes + 4)
        base = buf.offset(shift)
        assert base.value % 16 == shift
        for layer in H.RENDERABLE:
            top = host.max(layer)
            assert top >= 2, layer
            for vmax, alpha, table in ((0, 128, lut), (max(top // 2, 1), 1, None), (0, 256, lut[:, ::-1])):
                _lib.check(_lib.load().yds_memcpy_h2d(base, _lib.ptr(frames), frames.nbytes))
                dev.render_view(base, slots, sof, h, w, layer=layer, vmax=vmax, alpha=alpha, lut=table, n_frames=4)
                got = np.zeros_like(frames)
                _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(got), base, frames.nbytes))
                want = frames.copy()
                for slot, s in zip(slots, sof):
                    want[slot] = G.render_view(frames[slot], dev.specs[s], host.layer(layer), vmax=vmax, lut=table, alpha=alpha)
                assert np.array_equal(got, want), (shift, layer, vmax, alpha)
                assert np.array_equal(got[1], frames[1])
                if alpha > 1:
                    touched += int((want != frames).any(axis=3).sum())
                    kept += int((want == frames).all(axis=3)[[0, 2, 3]].sum())
        buf.free()
    assert touched > 300 and kept > 300
    assert not np.array_equal(G.view_field(dev.specs[0], h, w, H.levels(host.layer("presence")))[0],
                              G.view_field(dev.specs[1], h, w, H.levels(host.layer("presence")))[0])
    with pytest.raises(_lib.YdsError, match="no spec"):
        dev.render_view(_lib.DeviceBuffer.from_array(frames).ptr, [0], [2], h, w)
    with pytest.raises(_lib.YdsError, match="same slot"):
        dev.render_view(_lib.DeviceBuffer.from_array(frames).ptr, [1, 1], [0, 0], h, w)
    dev.set_timing(True)
    buf = _lib.DeviceBuffer.from_array(frames)
    dev.render_view(buf.ptr, [0], [0], h, w)
    assert 0 < dev.last_us("render") < 1e6
    dev.close()


# ------------------------------------------------------------------------------------------------ 7. render_plan
@pytest.mark.parametrize("cell_px", [4, 16])
def test_render_plan_equals_the_heat_map_render(cell_px):
    """The site layer on a plan canvas of cell_px pixels per cell equals heatmap.render of the same grid: a site grid is a heat grid."""
    from yolo_deepsort_amd import _lib
    dev, host = _painted()
    rs = np.random.RandomState(cell_px)
    canvas = rs.randint(0, 256, (30 * cell_px, 40 * cell_px, 3)).astype(np.uint8)
    for layer, vmax, alpha in (("presence", 0, 256), ("dwell_us", 0, 100), ("visits", 2, 128)):
        buf = _lib.DeviceBuffer.from_array(canvas)
        dev.render_plan(buf.ptr, cell_px, layer=layer, vmax=vmax, alpha=alpha)
        got = np.zeros_like(canvas)
        _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(got), buf.ptr, canvas.nbytes))
        want = H.render(canvas, host.layer(layer), cell_px, vmax=vmax, alpha=alpha)
        assert np.array_equal(got, want) and (want != canvas).any(), layer
        assert np.array_equal(want, G.render_plan(host.layer(layer), cell_px, vmax=vmax, alpha=alpha, canvas=canvas))
        buf.free()
    with pytest.raises(_lib.YdsError, match="cell_px"):
        dev.render_plan(_lib.DeviceBuffer.from_array(canvas).ptr, 5)
    dev.close()
