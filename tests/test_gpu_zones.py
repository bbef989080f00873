"""Zones and counting lines on the device (csrc/zones.hip): per stream a table of tracks in HBM, one launch per call.  The comparator
is the host restatement (yolo_deepsort_amd.zones.ZoneMonitor) fed the same rows and times; the geometry is integer arithmetic and a
dwell is one double subtraction, so events, counters and tables are compared with exact equality."""
import ctypes as C
import math

import numpy as np
import pytest

from yolo_deepsort_amd import action as A, cfgs, synth, zones as Z

from zones_common import box_at, fast_scene, kind_counts, standard_geometry

pytestmark = pytest.mark.gpu
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
EMPTY = np.zeros((0, 9), np.float32)
SQUARE = [(100, 100), (200, 100), (200, 200), (100, 200)]


def _same_state(dev, hosts):
    for s, host in enumerate(hosts):
        if host is not None:
            assert dev.counts(s) == host.counts(), s
            assert dev.tracks(s) == host.tracks(), s


def _feed(dev, hosts, frames):
    """frames: [(stream, rows or None, t), ...] in ONE device call against the hosts frame by frame; returns the events."""
    got = dev.update_batch([r for _, r, _ in frames], [s for s, _, _ in frames], [t for _, _, t in frames])
    want = [hosts[s].update(r, t) for s, r, t in frames]
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f, frames[f][0])
    _same_state(dev, hosts)
    return want


# ------------------------------------------------------------------------------------------------ 1. randomised
@pytest.mark.parametrize("max_age,n_ids", [(3, 300), (1, 400), (2, 300)])
def test_random_scene_equals_the_host_monitor(max_age, n_ids):
    """60 frames of the fast scene against the standard geometry, in three calls of 20 frames so that the table grows between
    calls.  What the scene exercises is asserted on the HOST output, so the comparison cannot pass vacuously."""
    dev = Z.DeviceZoneMonitor(standard_geometry(), max_age=max_age)
    host = dev.host()
    frames = [(0, r, t) for r, t in fast_scene(0, n_ids, 60)]
    events = []
    for k in range(0, 60, 20):
        events += _feed(dev, [host], frames[k:k + 20])
    n = kind_counts(events)
    assert n[Z.ENTER] >= 100 and n[Z.EXIT] >= 100 and n[Z.CROSS_FWD] >= 100 and n[Z.CROSS_BACK] >= 100 and n[Z.LOST] >= 20, n
    assert host.stats["abandoned"] >= 50 and host.stats["zero_orientations"] >= 20 and host.stats["max_table"] > 256, host.stats
    dev.close()


# ------------------------------------------------------------------------------------------------ 2. bursts and full masks
def test_bursts_of_more_than_a_workgroup_of_events_in_one_frame():
    """300 tracks cross a line into one zone in the same frame (600 events in it), then all vanish: 300 LOST events in one frame."""
    dev = Z.DeviceZoneMonitor(([Z.Zone(SQUARE)], [Z.Line((150, 0), (150, 300))]), max_age=2)
    host = dev.host()
    out = [box_at(500 + 2 * (i % 7), 110 + i % 80, tid=i + 1, cls=i % 3) for i in range(300)]
    inn = [box_at(210 + (i % 90), 110 + i % 80, tid=i + 1, cls=i % 3) for i in range(300)]
    ev = _feed(dev, [host], [(0, out, 0.0), (0, inn[::-1], 1.0), (0, [], 2.0), (0, [], 3.5), (0, out[:5], 4.0)])
    assert [len(e) for e in ev] == [0, 600, 0, 300, 0]
    assert kind_counts([ev[1]]) == [300, 0, 0, 300, 0] and kind_counts([ev[3]]) == [0, 0, 300, 0, 0]
    assert {e[5] for e in ev[3]} == {0.0} and host.counts() == ([[0, 300, 0, 300]], [[300, 0]]) and len(host.tracks()) == 5
    dev.close()


def test_full_masks_32_zones_of_16_vertices_and_32_lines():
    """Zone k is a 16-gon of radius 100 + 5 k around (500, 500), line k is x = 300 + 10 k drawn upwards (a move to the right is
    FORWARD): one track inside all 32 zones (bit 31 of its mask set), one inside zone 31 only, one that crosses all 32 lines and
    one that crosses line 31 only."""
    gon = lambda r: [(500 + round(r * math.cos(math.pi * i / 8)), 500 + round(r * math.sin(math.pi * i / 8))) for i in range(16)]  # noqa: E731
    zones = [Z.Zone(gon(100 + 5 * k), min_sightings=1 + k % 2) for k in range(32)]
    lines = [Z.Line((300 + 10 * k, 1000), (300 + 10 * k, 0)) for k in range(32)]
    dev = Z.DeviceZoneMonitor((zones, lines), max_age=1)
    host = dev.host()
    f0 = [box_at(1000, 500, 1), box_at(1504, 500, 2), box_at(200, 900, 3), box_at(1210, 900, 4)]
    f1 = [box_at(1000, 500, 1), box_at(1504, 500, 2), box_at(1800, 900, 3), box_at(1230, 900, 4)]
    ev = _feed(dev, [host], [(0, f0, 0.0), (0, f1, 1.0), (0, f1[:1], 2.0)])
    assert host.tracks() == [(1, 0, 0xFFFFFFFF)]
    assert [(e[0], e[3]) for e in ev[1] if e[2] == Z.CROSS_FWD] == [(3, k) for k in range(32)] + [(4, 31)]
    assert [(e[0], e[2], e[3]) for e in ev[0] + ev[1] if e[0] == 2] == [(2, Z.ENTER, 31)]
    assert [(e[0], e[2], e[3]) for e in ev[2]] == [(2, Z.LOST, 31)]
    dev.close()


# ------------------------------------------------------------------------------------------------ 3. decision boundaries
def test_decision_boundaries_on_the_device():
    """Rows on the edges and vertices of the square and half a pixel beside them; moves between points on a line, at A, at B and
    half a pixel beyond; zones and lines of the other class.  One track per case, all in the same two frames."""
    zones = [Z.Zone(SQUARE), Z.Zone(SQUARE[::-1], class_id=2), Z.Zone(SQUARE, class_id=0, min_sightings=2)]
    lines = [Z.Line((100, 200), (300, 200)), Z.Line((300, 200), (100, 200), class_id=0), Z.Line((100, 100), (200, 200), class_id=2)]
    dev = Z.DeviceZoneMonitor((zones, lines), max_age=3)
    host = dev.host()
    pts = [(x2, y) for x2 in (199, 200, 201, 300, 399, 400, 401, 599, 600, 601) for y in (99, 100, 101, 150, 199, 200, 201)]
    f0, f1, tid = [], [], 0
    for p in pts:
        for c in pts:
            if (p[1] in (199, 200, 201) and c[1] in (199, 200, 201)) or p == (300, 150):
                tid += 1
                f0.append(box_at(p[0], p[1], tid, (tid % 2) * 2))
                f1.append(box_at(c[0], c[1], tid, (tid % 2) * 2))
    assert 900 <= tid <= 1100
    ev = _feed(dev, [host], [(0, f0, 0.0), (0, f1, 1.0), (0, f1, 2.0)])
    n = kind_counts(ev)
    assert min(n[Z.ENTER], n[Z.EXIT], n[Z.CROSS_FWD], n[Z.CROSS_BACK]) >= 40, n
    inside_any = {(e[0]) for e in ev[0] if e[2] == Z.ENTER and e[3] == 0}
    on = {t: (r[0] + r[2], r[3]) for t, r in ((r[4], r) for r in f0)}
    assert {on[t] for t in inside_any} == {(x, y) for x, y in on.values() if 200 <= x < 400 and 100 <= y < 200}
    assert host.stats["zero_orientations"] >= 200
    dev.close()


# ------------------------------------------------------------------------------------------------ 4. streams and lifecycle
def test_streams_interleaved_in_one_call_equal_each_stream_alone():
    zones, lines = standard_geometry()
    geo = [(zones, lines), (zones[:2], lines[2:]), ([], []), (zones[1:], [])]
    dev = Z.DeviceZoneMonitor(geo, max_age=2, n_streams=4)
    hosts = [dev.host(s) for s in range(4)]
    scenes = [fast_scene(10 + s, 40, 12) for s in range(3)]
    _feed(dev, hosts, [(3, scenes[0][0][0], 0.0), (3, scenes[0][1][0], 0.5)])
    before = (dev.tracks(3), dev.counts(3))
    assert len(before[0]) >= 30
    frames = [(s, scenes[s][k][0], scenes[s][k][1] + s) for k in range(12) for s in (2, 0, 1)]
    frames.insert(7, (1, None, 99.0))                                 # a frame whose rows are None is not seen
    ev = _feed(dev, hosts, frames)
    assert ev[7] is None and sum(len(e) for e in ev if e) >= 50 and all(e == [] for (s, _, _), e in zip(frames, ev) if s == 2 and e is not None)
    assert (dev.tracks(3), dev.counts(3)) == before                   # a stream without frames is untouched
    alone = Z.DeviceZoneMonitor(geo[1], max_age=2)
    got = [alone.update(0, r, t) for s, r, t in frames if s == 1]
    assert got == [e for (s, _, _), e in zip(frames, ev) if s == 1] and alone.tracks() == dev.tracks(1) and alone.counts() == dev.counts(1)
    alone.close()
    dev.close()


def test_a_call_that_names_some_streams_out_of_order_keeps_every_table_apart():
    """The host's bookkeeping per call: three calls over a handle of 3 streams - all three streams; then streams 2 and 0 in that
    order (two workgroups, for streams 0 and 2, and a frame order that is not the bucket order) with a frame of no rows and an entry
    that reaches max_age = 1 and leaves; then stream 1 alone (workgroup 0 is stream 1).  Every stream's ids and places differ, and
    after every call all three tables and counters are compared, the streams without frames included."""
    dev = Z.DeviceZoneMonitor(([Z.Zone(SQUARE)], [Z.Line((150, 0), (150, 300))]), max_age=1, n_streams=3)
    hosts = [dev.host(s) for s in range(3)]
    at = lambda s, k, x2: box_at(x2, 110 + 10 * k + s, tid=10 * s + k, cls=k % 2)      # noqa: E731 - doubled x: the zone is [200, 400), the line 300
    ev = _feed(dev, hosts, [(s, [at(s, k, 260 if k % 2 else 450) for k in range(3 + s)], 0.0) for s in range(3)])
    assert [len(e) for e in ev] == [1, 2, 2] and [len(h.tracks()) for h in hosts] == [3, 4, 5]
    ev = _feed(dev, hosts, [(2, [at(2, 0, 340), at(2, 1, 340), at(2, 2, 450), at(2, 4, 150), at(2, 7, 260)], 1.0), (0, [], 1.0),
                            (0, [at(0, 5, 260), at(0, 1, 450)], 2.0)])
    assert [len(e) for e in ev] == [5, 1, 1] and kind_counts(ev) == [3, 0, 2, 1, 1]
    assert [e[0] for e in ev[0] + ev[1] if e[2] == Z.LOST] == [23, 1]                 # 23 was not seen; the empty frame retires 0, 1, 2
    assert [[t[0] for t in h.tracks()] for h in hosts] == [[5, 1], [10, 11, 12, 13], [20, 21, 22, 24, 27]]
    ev = _feed(dev, hosts, [(1, [at(1, 1, 450), at(1, 2, 450), at(1, 0, 260), at(1, 6, 340)], 3.0)])
    assert kind_counts(ev) == [2, 1, 1, 1, 1] and [t[0] for t in hosts[1].tracks()] == [10, 11, 12, 16]
    assert [h.counts() for h in hosts] == [([[1, 2, 0, 1]], [[0, 0]]), ([[2, 4, 1, 1]], [[1, 1]]), ([[3, 4, 0, 1]], [[1, 1]])]
    dev.close()


def test_lifecycle_ageing_returns_and_resets():
    geo = ([Z.Zone(SQUARE, name="hall")], [Z.Line((150, 0), (150, 300))])
    dev = Z.DeviceZoneMonitor(geo, max_age=3, n_streams=2)
    hosts = [dev.host(0), dev.host(1)]
    a, b = box_at(300, 150, 1), box_at(320, 160, 2)
    ev = _feed(dev, hosts, [(0, [a, b], 0.0), (0, [b], 1.0), (0, None, 1.5), (0, [], 2.0), (0, [a, b], 3.0)])
    assert ev[0] == [(1, 0, Z.ENTER, "hall", 0.0, 0.0), (2, 0, Z.ENTER, "hall", 0.0, 0.0)] and ev[1:] == [[], None, [], []]
    assert dev.tracks(0) == [(1, 0, 1), (2, 0, 1)]                    # back before max_age: the bit is kept, no ENTER
    ev = _feed(dev, hosts, [(0, [b], 4.0), (0, [b], 5.0), (0, [b], 6.0), (0, [b, a], 7.0)])
    assert ev[2] == [(1, 0, Z.LOST, "hall", 6.0, 3.0)] and ev[3] == [(1, 0, Z.ENTER, "hall", 7.0, 0.0)]      # dropped, then re-enters
    assert dev.tracks(0) == [(2, 0, 1), (1, 0, 1)] and dev.counts(0) == ([[2, 3, 0, 1]], [[0, 0]])
    _feed(dev, hosts, [(1, [a], 0.0), (1, [b], 1.0)])
    dev.reset(0)
    hosts[0].reset()
    _same_state(dev, hosts)
    assert dev.tracks(0) == [] and dev.counts(0) == ([[0, 0, 0, 0]], [[0, 0]]) and len(dev.tracks(1)) == 2
    _feed(dev, hosts, [(0, [a], 8.0), (1, [a], 8.0)])
    from yolo_deepsort_amd import _lib
    g = dev.packed[1]
    _lib.check(_lib.load().yds_zones_set_stream(dev.handle, 1, _lib.ptr(g[0]), _lib.ptr(g[1]), _lib.ptr(g[2]), _lib.ptr(g[3]), 1, _lib.ptr(g[4]),
                                                _lib.ptr(g[5]), 1))
    hosts[1].reset()                                                  # set_stream resets the stream
    _same_state(dev, hosts)
    assert dev.tracks(1) == [] and len(dev.tracks(0)) == 1
    dev.reset()
    assert dev.tracks(0) == [] and dev.counts(0) == ([[0, 0, 0, 0]], [[0, 0]])
    dev.close()


def test_refusals_and_the_capacity_error():
    from yolo_deepsort_amd import _lib
    _lib.init(0)
    lib = _lib.load()
    assert not lib.yds_zones_create(1, 0) and "max_age" in _lib.last_error()
    assert not lib.yds_zones_create(0, 3) and "streams" in _lib.last_error()
    dev = Z.DeviceZoneMonitor(([Z.Zone(SQUARE)], [Z.Line((150, 0), (150, 300))]), max_age=3, n_streams=2)
    h = dev.handle
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)          # noqa: E731

    def set_stream(stream, ptr, xy, zc, zm, lxy, lc):
        ptr, xy, zc, zm, lxy, lc = (i32(v) for v in (ptr, xy, zc, zm, lxy, lc))
        rc = lib.yds_zones_set_stream(h, stream, _lib.ptr(ptr), _lib.ptr(xy), _lib.ptr(zc), _lib.ptr(zm), len(zc), _lib.ptr(lxy), _lib.ptr(lc), len(lc))
        return rc, _lib.last_error()
    tri, lim = [0, 0, 9, 0, 0, 9], 1 << 20
    ok = ([0, 3], tri, [-1], [1], [0, 0, 1, 1], [-1])
    assert set_stream(1, *ok)[0] == 0 and set_stream(-1, *ok)[0] == 0
    for stream, args, word in [
            (2, ok, "stream"), (-2, ok, "stream"),
            (0, ([0] + [3] * 33, tri * 11, [-1] * 33, [1] * 33, [], []), "33 zones"),
            (0, ([0], [], [], [], [0, 0, 1, 1] * 33, [-1] * 33), "33 lines"),
            (0, ([0, 2], tri[:4], [-1], [1], [], []), "vertices"), (0, ([0, 17], [0, 0] * 17, [-1], [1], [], []), "vertices"),
            (0, ([0, 3], [0, 0, lim + 1, 0, 0, 9], [-1], [1], [], []), "coordinate"), (0, ([0, 3], [0, -lim - 1, 9, 0, 0, 9], [-1], [1], [], []), "coordinate"),
            (0, ([0, 3], tri, [-1], [0], [], []), "min_sightings"), (0, ([0, 3], tri, [-1], [256], [], []), "min_sightings"),
            (0, ([0, 3], tri, [-2], [1], [], []), "class_id"),
            (0, ([0], [], [], [], [5, 5, 5, 5], [-1]), "A == B"), (0, ([0], [], [], [], [0, 0, lim + 1, 0], [-1]), "coordinate"),
            (0, ([0], [], [], [], [0, 0, 1, 1], [-2]), "class_id")]:
        rc, msg = set_stream(stream, *args)
        assert rc != 0 and word in msg, (word, msg)
    assert set_stream(0, [0, 3], [0, 0, lim, 0, 0, -lim], [-1], [255], [-lim, 0, lim, 0], [7])[0] == 0
    dev.close()
    dev = Z.DeviceZoneMonitor(([Z.Zone(SQUARE)], [Z.Line((150, 0), (150, 300))]), max_age=3, n_streams=2)
    a = box_at(300, 150, 1)
    with pytest.raises(_lib.YdsError, match="twice"):
        dev.update(0, [a, a], 0.0)
    with pytest.raises(ValueError, match="stream"):
        dev.update(2, [a], 0.0)
    rows, first, sof, tm = i32([a]), i32([0, 1]), i32([5]), np.zeros(1)
    ev6, evt2, m = np.zeros((8, 6), np.int32), np.zeros((8, 2)), C.c_int(0)
    assert lib.yds_zones_update(dev.handle, _lib.ptr(rows), _lib.ptr(first), _lib.ptr(sof), _lib.ptr(tm), 1, _lib.ptr(ev6), _lib.ptr(evt2), 8,
                                C.byref(m)) != 0 and "stream 5" in _lib.last_error()
    for s in (2, -1):
        assert lib.yds_zones_get_counts(dev.handle, s, None, None) != 0 and "stream" in _lib.last_error()
        assert lib.yds_zones_get_tracks(dev.handle, s, None, None, None, 0, C.byref(m)) != 0 and "stream" in _lib.last_error()
    assert lib.yds_zones_reset(dev.handle, 2) != 0 and "stream" in _lib.last_error()
    us = C.c_float(0)
    assert lib.yds_zones_last_us(dev.handle, C.byref(us)) != 0 and "timed" in _lib.last_error()
    # three tracks enter at once, the caller has room for two events: the error names the count, the table has advanced
    rows, first, sof = i32([box_at(300, 150, t) for t in (1, 2, 3)]), i32([0, 3]), i32([0])
    assert lib.yds_zones_update(dev.handle, _lib.ptr(rows), _lib.ptr(first), _lib.ptr(sof), _lib.ptr(tm), 1, _lib.ptr(ev6), _lib.ptr(evt2), 2,
                                C.byref(m)) != 0
    assert "3 events" in _lib.last_error() and m.value == 3
    assert dev.tracks(0) == [(1, 0, 1), (2, 0, 1), (3, 0, 1)] and dev.counts(0) == ([[3, 3, 0, 0]], [[0, 0]])
    dev.set_timing(True)
    dev.update(0, [a], 1.0)
    assert 0 < dev.last_us() < 1e6
    dev.close()


# ------------------------------------------------------------------------------------------------ 5. inside the pipeline
def _tracker_full(ds):
    from yolo_deepsort_amd import _lib
    lib = _lib.load()
    st = ds.tracker.state()
    n = len(st["ids"])
    pay, age = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
    _lib.check(lib.yds_tracker_get_payload(ds.tracker._h, _lib.ptr(pay), max(n, 1)))
    _lib.check(lib.yds_tracker_get_age(ds.tracker._h, _lib.ptr(age), max(n, 1)))
    st["payload"], st["age"] = pay[:n], age[:n]
    st["um_t"], st["um_d"] = ds.tracker.last_unmatched()
    return st


def _play(pipe, net, steps, frame_of, inj_of, hw, host, before_step, on_step):
    """tests/test_gpu_actions.py _play: per step a list of (stream, frame index), a hook ahead of every step; the next step's
    frames are handed over (look-ahead) when it has as many frames."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    bm = net.batch_max
    pl.load_injection_sets(net, [[inj_of(s, k) for s, k in st] + [EMPTY] * (bm - len(st)) for st in steps])
    h, w = hw
    bufs = {}

    def frames(i):
        if i not in bufs:
            a = _lib.PinnedArray((len(steps[i]), h, w, 3), np.uint8)
            for b, (s, k) in enumerate(steps[i]):
                a.array[b] = frame_of(s, k)
            bufs[i] = (a, None if host else _lib.DeviceBuffer.from_array(a.array))
        return bufs[i]
    sel, n_ahead = None, 0
    for i, st in enumerate(steps):
        if sel != i:
            pl.select_injection_set(net, i)
        ahead = i + 1 < len(steps) and len(steps[i + 1]) == len(st)
        n_ahead += ahead
        cur = frames(i)
        nxt = frames(i + 1) if ahead else None
        ids = [s for s, _ in st]
        before_step(i)
        if host:
            outs = pipe.step_host(cur[0].array, ids, nxt[0].array if ahead else None, select_next=(i + 1 if ahead else None))
        else:
            outs = pipe.step(cur[1].ptr, 480, 640, ids, nxt[1].ptr if ahead else None, select_next=(i + 1 if ahead else None))
        sel = i + 1 if ahead else None
        bufs.pop(i)
        on_step(i, outs)
    return n_ahead


def _frame_geometry():
    """Zones and lines for 640 x 480 frames of slow walkers: halves, a centre box, the whole frame for class 2, a grid of lines."""
    zones = [Z.Zone([(0, 0), (320, 0), (320, 480), (0, 480)], name="left"),
             Z.Zone([(320, 0), (640, 0), (640, 480), (320, 480)], class_id=0, min_sightings=2, name="right"),
             Z.Zone([(0, 0), (640, 0), (640, 480), (0, 480)], class_id=2),
             Z.Zone([(160, 200), (480, 180), (500, 420), (320, 380), (140, 440)], min_sightings=1, name="centre")]
    lines = [Z.Line((x, 0), (x, 480), class_id=(-1 if x % 160 else 0)) for x in range(80, 640, 80)]
    lines += [Z.Line((0, y), (640, y), name="y%d" % y) for y in range(160, 480, 60)]
    return zones, lines


@pytest.mark.parametrize("host_frames", [False, True])
def test_pipeline_zones_equal_host_clones_and_leave_everything_else_alone(host_frames):
    """yolov3-tiny 416 on 480x640 frames, three trackers, injected PersonScene detections, the step schedule of
    test_pipeline_actions_equal_host_clones_and_leave_tracking_alone (steps where a stream has no frame or several, a detector-None
    frame per stream, a mask-emptied frame, look-ahead steps), with zones, actions and identities all on.  last_zone_events() per
    frame equals host ZoneMonitor clones fed the returned rows and the same times, None where the rows are None; a second pipeline
    with zones off returns the same rows, tracker state, actions and identities."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=8, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0))
    ex = Extractor(synth.reid_state_dict(0), max_crops=256)
    settings = [dict(DS), dict(DS, max_dist=0.25, nn_budget=20), dict(DS, n_init=2, max_age=4)]
    counts = [(1, 2, 0), (3, 1, 1), (0, 0, 2), (2, 2, 2), (1, 0, 3), (2, 3, 1), (0, 2, 0), (3, 1, 2), (1, 1, 1), (2, 0, 2),
              (1, 2, 1), (2, 1, 1)]
    n_of = [sum(c[s] for c in counts) for s in range(3)]
    frames, injs = [], []
    for s in range(3):
        scene = synth.PersonScene(10, frame_hw=(480, 640), seed=3 + s, occlude_frac=0.2)
        heads = net.yolo_heads()
        fr, ij = [], []
        for t in range(n_of[s]):
            ids, tlwh = scene.boxes(t)
            rows = synth.head_injection(tlwh, (480, 640), (416, 416), heads)
            rows[:, 8] = np.where(ids % 3 == 0, 2, 0)
            rows[ids == 4, 8] = 5                                   # a class the mask drops
            if t == 4 + s:
                rows = rows[:0]                                     # the detector returns None: tracker and zone stage not called
            if t == 7 and s == 1:
                rows[:, 8] = 5                                      # every detection masked: D = 0, every entry of the stream ages
            fr.append(scene.frame(t))
            ij.append(rows)
        frames.append(fr)
        injs.append(ij)
    steps, nxt = [], [0, 0, 0]
    for c in counts:
        st = []
        for s in range(3):
            st += [(s, nxt[s] + k) for k in range(c[s])]
            nxt[s] += c[s]
        steps.append(st)
    mask = [0, 2, 4]
    ident = A.ActionIdentify([A.Glide(0, (0, 3)), A.FastCrossing(0, 0.01), A.BreakInto(0, 1), A.BreakInto(2, 0)], max_age=2, max_size=3)
    zones, lines = _frame_geometry()
    geo = [(zones, lines), (zones[::-1], lines[::2]), (zones[:3], lines)]
    time_of = lambda s, k: 0.04 * k + 0.001 * s          # noqa: E731
    small = Z.DeviceZoneMonitor(geo[:2], max_age=2, n_streams=2)

    def run(with_zones):
        trackers = [DeepSort(ex, use_cuda=True, **p) for p in settings]
        pipe = pl.MultiStreamPipeline(net, trackers, 0.5, 0.4, class_mask=mask)
        pipe.set_actions(ident)
        pipe.set_identities(True)
        assert pipe.last_zone_events() is None and pipe.zone_counts() is None
        mon = None
        if with_zones:
            with pytest.raises(ValueError, match="zones"):
                pipe.set_zones(small)
            assert _lib.load().yds_pipeline_set_zones(pipe._h, small.handle) != 0 and "2 streams" in _lib.last_error()
            mon = pipe.set_zones(Z.DeviceZoneMonitor(geo, max_age=2, n_streams=3))
        rows, got, states, refused = [], [], [], []

        def before(i):
            pipe.set_frame_times([time_of(s, k) for s, k in steps[i]])
            if with_zones and i and len(steps[i]) == len(steps[i - 1]):       # the previous step handed this one's frames over
                with pytest.raises(_lib.YdsError, match="look-ahead"):
                    pipe.set_zones(None)
                refused.append(i)

        def after(i, outs):
            rows.append(outs)
            got.append((pipe.last_zone_events(), pipe.last_actions(), pipe.last_identities()))
            states.append({s: _tracker_full(trackers[s]) for s in {s for s, _ in steps[i]}})
        n_ahead = _play(pipe, net, steps, lambda s, k: frames[s][k], lambda s, k: injs[s][k], (480, 640), host_frames, before, after)
        assert n_ahead >= 2 and (len(refused) == n_ahead or not with_zones)
        return rows, got, states, (None if mon is None else ([mon.tracks(s) for s in range(3)], pipe.zone_counts(), pipe.zone_counts(1)))
    rows, got, states, final = run(True)
    clones = [Z.ZoneMonitor(*geo[s], max_age=2) for s in range(3)]
    n_none, kinds = 0, [0] * 5
    for i, st in enumerate(steps):
        assert len(got[i][0]) == len(st)
        for b, (s, k) in enumerate(st):
            if rows[i][b] is None:
                assert got[i][0][b] is None, (i, b)
                n_none += 1
                continue
            want = clones[s].update(rows[i][b], time_of(s, k))
            assert got[i][0][b] == want, (i, b, s, k)
            kinds = [a + b_ for a, b_ in zip(kinds, kind_counts([want]))]
    assert n_none == 3 and sum(kinds) >= 20 and kinds[Z.ENTER] >= 10, kinds
    assert final == ([c.tracks() for c in clones], [c.counts() for c in clones], clones[1].counts())
    plain_rows, plain_got, plain_states, _ = run(False)
    for i, st in enumerate(steps):
        assert plain_got[i][0] is None and got[i][1] == plain_got[i][1] and got[i][2] == plain_got[i][2], i
        for b in range(len(st)):
            a, p = rows[i][b], plain_rows[i][b]
            assert (a is None) == (p is None) and (a is None or (a.shape == p.shape and np.array_equal(a, p))), (i, b)
        for s, full in states[i].items():
            for key in ("ids", "state", "tsu", "hits", "mean", "cov", "payload", "age", "um_t", "um_d"):
                assert np.array_equal(full[key], plain_states[i][s][key]), (i, s, key)
    assert any(g[1] and any(g[1]) for g in got) and any(any(d.values()) for g in got for d in g[2])
    small.close()


def test_pipeline_zone_times_default_to_the_frame_count_over_25():
    """Without set_frame_times a stream's k-th frame since the pipeline was made carries k / 25: the single-stream Pipeline over
    6 steps of 2 frames, zones alone (no action stage), against a host clone fed the returned rows with those times."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=2, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0))
    ds = DeepSort(Extractor(synth.reid_state_dict(0), max_crops=64), use_cuda=True, **DS)
    scene = synth.PersonScene(8, frame_hw=(480, 640), seed=5, occlude_frac=0.1)
    heads = net.yolo_heads()
    T = 12
    inj = [synth.head_injection(scene.boxes(t)[1], (480, 640), (416, 416), heads, cls=0) for t in range(T)]
    pl.load_injection_sets(net, [[inj[t], inj[t + 1]] for t in range(0, T, 2)])
    host = Z.ZoneMonitor(*_frame_geometry(), max_age=2)
    pipe = pl.Pipeline(net, ds, 0.5, 0.4, class_mask=[0])
    pipe.set_zones(host)                                   # (a ZoneMonitor: its geometry and max_age, fresh tables on the device)
    n = 0
    for i in range(T // 2):
        pl.select_injection_set(net, i)
        dev = _lib.DeviceBuffer.from_array(np.stack([scene.frame(2 * i), scene.frame(2 * i + 1)]))
        outs = pipe.step(dev.ptr, 480, 640, 2)
        got = pipe.last_zone_events()
        for b in range(2):
            assert outs[b] is not None
            want = host.update(outs[b], (2 * i + b) / 25.0)
            assert got[b] == want, (i, b)
            n += len(want)
    assert n >= 5 and pipe.zone_counts() == host.counts() and pipe.zone_counts(0) == host.counts()
    assert {e[4] for e in want} <= {(T - 1) / 25.0}
    with pytest.raises(ValueError, match="zones"):
        pipe.set_zones(object())
    pipe.set_zones(None)
    assert pipe.last_zone_events() is None and pipe.zone_counts() is None


# ------------------------------------------------------------------------------------------------ 6. VideoDetector.detect_streams
def test_detect_streams_carries_each_streams_zone_events(tmp_path):
    """Three in-memory clips, skip_frames=2, zones for all streams: between the yields stream_zone_events() holds, per stream,
    the events of every frame the step processed, equal to a host clone fed that stream's processed, non-None rows with times
    frame index / 25, and stream_zone_counts() the clone's counters; the yielded items are those of a run without zones."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import DeepSort
    from yolo_deepsort_amd.detect import VideoDetector
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=4, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, -1.45))      # a handful of (random) detections per frame
    base = DeepSort(synth.reid_state_dict(0), use_cuda=True, **DS)
    clips = []
    for seed, n in ((21, 15), (22, 5), (23, 11)):
        img = np.random.RandomState(seed).randint(0, 256, (480, 640, 3)).astype(np.uint8)
        clips.append([np.roll(img, 3 * t, axis=1) for t in range(n)])
    zones, lines = _frame_geometry()
    zones = [Z.Zone(z.polygon, -1, z.min_sightings, z.name) for z in zones]              # (the detections carry random classes)
    lines = [Z.Line(ln.a, ln.b, -1, ln.name) for ln in lines]
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())

    def detector():
        return VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=base, skip_frames=2, class_mask=list(range(0, 80, 2)))
    plain = [[(s, det) for s, _, det, _ in step] for step in detector().detect_streams(clips, frames_per_stream=1, show_fps=False)]
    total = 0
    for fps in (1, None):
        vd = detector()
        with pytest.raises(ValueError, match="between the yields"):
            vd.stream_zone_events()
        clones = [Z.ZoneMonitor(zones, lines, max_age=3) for _ in clips]
        seen, items = [0] * 3, []
        for step in vd.detect_streams(clips, frames_per_stream=fps, show_fps=False, zones=(zones, lines), zone_max_age=3):
            got = vd.stream_zone_events()
            want = [[] for _ in clips]
            for s, _, det, _ in step:
                if seen[s] % 2 == 0:                                      # a processed frame
                    want[s].append(None if det is None else clones[s].update(det, seen[s] / 25.0))
                seen[s] += 1
            assert got == want and vd.stream_zone_events(2) == want[2]
            assert vd.stream_zone_counts() == [c.counts() for c in clones] and vd.stream_zone_counts(1) == clones[1].counts()
            total += sum(len(e) for w in want for e in w if e)
            items.append([(s, det) for s, _, det, _ in step])
        if fps == 1:
            assert len(items) == len(plain)
            for a, b in zip(items, plain):
                assert [s for s, _ in a] == [s for s, _ in b]
                assert all((x is None) == (y is None) and (x is None or np.array_equal(x, y)) for (_, x), (_, y) in zip(a, b))
    assert seen == [15, 5, 11] and total >= 4
    with pytest.raises(ValueError, match="zones"):
        next(detector().detect_streams(clips, zones=([Z.Zone(SQUARE[:2])], [])))
    with pytest.raises(ValueError, match="zones="):
        vd2 = detector()
        for _ in vd2.detect_streams(clips, frames_per_stream=1, show_fps=False):
            vd2.stream_zone_counts()
