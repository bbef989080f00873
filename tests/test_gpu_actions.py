"""Action identification on the device (csrc/actions.hip): the orbit caches of ActionIdentify for many streams in HBM, one launch per
call.  The comparator is the host module (yolo_deepsort_amd.action) fed the same rows and the same explicit times; the device computes
in double in the Python expressions' operation order, so every comparison is exact equality of the row lists."""
import collections
import ctypes as C

import numpy as np
import pytest

from oracle.gen_golden import action_scene
from yolo_deepsort_amd import action as A, cfgs, synth

from actions_common import RANDOM_ACTIONS, as_tuples, fixture_row_times, random_scene, trace_actions, trace_want

pytestmark = pytest.mark.gpu
DS = dict(max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
EMPTY = np.zeros((0, 9), np.float32)


def _host_orbits(host):
    return [(int(tid), int(o.age), len(o.deque)) for tid, o in host.cache.items()]


# ------------------------------------------------------------------------------------------------ 1. the reference trace
def test_reference_trace_frame_by_frame_and_in_one_call():
    frames, want = action_scene(), trace_want()
    times = fixture_row_times(frames)
    host = A.ActionIdentify(trace_actions(), max_age=3, max_size=4)
    for det, ts in zip(frames, times):
        host.update(det, ts)
    one = A.DeviceActionIdentify(trace_actions(), max_age=3, max_size=4)
    for t, det in enumerate(frames):
        assert one.update(0, det, times[t]) == want[t], t
    assert one.orbits(0) == _host_orbits(host)
    assert one.update(0, None, 0.0) is None and one.orbits(0) == _host_orbits(host)
    whole = A.DeviceActionIdentify(trace_actions(), max_age=3, max_size=4)
    got = whole.update_batch(frames, [0] * len(frames), times)
    for t in range(len(frames)):
        assert got[t] == want[t], t
    assert whole.orbits(0) == _host_orbits(host)
    assert sum(map(len, want)) > 0 and any(r != sorted(r) for r in want)       # rows are in cache order, not id order


# ------------------------------------------------------------------------------------------------ 2. streams in one call
def test_streams_interleaved_in_one_call_equal_each_stream_alone():
    scene, want = action_scene(), trace_want()
    t0 = fixture_row_times(scene)
    other = [f.copy() for f in scene[3:] + scene[:3]]
    for f in other:
        f[:, 4] += 100
    t1 = [0.04 * k for k in range(len(other))]
    dev = A.DeviceActionIdentify(trace_actions(), max_age=3, max_size=4, n_streams=3)
    got = [[], []]
    for k in range(0, len(scene), 2):                    # 4 frames per call: two of each stream, interleaved
        out = dev.update_batch([scene[k], other[k], scene[k + 1], other[k + 1]], [0, 1, 0, 1], [t0[k], t1[k], t0[k + 1], t1[k + 1]])
        got[0] += [out[0], out[2]]
        got[1] += [out[1], out[3]]
    host1 = A.ActionIdentify(trace_actions(), max_age=3, max_size=4)
    alone1 = A.DeviceActionIdentify(trace_actions(), max_age=3, max_size=4)
    for k in range(len(scene)):
        assert got[0][k] == want[k], k
        w = as_tuples(host1.update(other[k], t1[k]))
        assert got[1][k] == w and alone1.update(0, other[k], t1[k]) == w, k
    assert sum(map(len, got[1])) > 0
    assert dev.orbits(1) == _host_orbits(host1) == alone1.orbits(0)
    assert dev.orbits(2) == [] and len(dev.orbits(0)) > 0


def test_a_call_that_names_some_streams_out_of_order_keeps_every_cache_apart():
    """The host's bookkeeping per call: a handle of 3 streams; a call with all three; one with streams 2 and 0 in that order (two
    workgroups, for streams 0 and 2, and a frame order that is not the bucket order), with a frame of no rows and an id that reaches
    max_age = 1 and leaves; stream 1 alone (workgroup 0 is stream 1); streams 1 and 2.  Every stream has its own ids and box
    widths, and after every call the rows per frame and all three caches equal three host clones, the streams without frames
    included."""
    acts = [A.BreakInto(0, 0), A.Glide(1, (2, 2)), A.BreakInto(1, 1)]
    dev = A.DeviceActionIdentify(acts, max_age=1, max_size=3, n_streams=3)
    hosts = [A.ActionIdentify(acts, max_age=1, max_size=3) for _ in range(3)]
    row = lambda s, k, x: [x, 0, x + 10 + s, 40 + k, 10 * s + k, k % 2]      # noqa: E731

    def feed(frames):
        rows = [np.array(r, np.int32).reshape(-1, 6) for _, r, _ in frames]
        got = dev.update_batch(rows, [s for s, _, _ in frames], [t for _, _, t in frames])
        want = [as_tuples(hosts[s].update(r, t)) for (s, _, t), r in zip(frames, rows)]
        assert got == want
        for s in range(3):
            assert dev.orbits(s) == _host_orbits(hosts[s]), s
        return want
    assert feed([(s, [row(s, k, 100 * k) for k in range(3 + s)], 0.5) for s in range(3)]) == [[], [], []]
    w = feed([(2, [row(2, 0, 5), row(2, 1, 108), row(2, 2, 200), row(2, 4, 430), row(2, 7, 0)], 1.0), (0, [], 1.0),
              (0, [row(0, 5, 7), row(0, 1, 9)], 1.5)])
    assert [r[0] for r in w[0]] == [20, 22, 24] and w[1:] == [[], []]
    assert [[o[0] for o in _host_orbits(h)] for h in hosts] == [[5, 1], [10, 11, 12, 13], [20, 21, 22, 24, 27]]      # 23, then 0, 1, 2 left
    w = feed([(1, [row(1, 1, 104), row(1, 2, 230), row(1, 0, 0), row(1, 6, 60)], 2.0)])
    assert [r[0] for r in w[0]] == [10, 12] and [o[0] for o in _host_orbits(hosts[1])] == [10, 11, 12, 16]
    w = feed([(1, [row(1, 1, 110), row(1, 6, 66)], 2.5), (2, [row(2, 1, 116)], 2.5)])
    assert w == [[(11, 1, "glide"), (11, 1, "break_into"), (16, 0, "break_into")], [(21, 1, "glide"), (21, 1, "break_into")]]


# ------------------------------------------------------------------------------------------------ 3. randomised against the host module
@pytest.mark.parametrize("max_age,max_size,n_ids", [(3, 4, 300), (1, 2, 400), (2, 16, 300), (3, 1, 300)])
def test_random_scene_equals_the_host_module(max_age, max_size, n_ids):
    """60 frames of n_ids tracks (actions_common.random_scene), 7 actions.  The conditions on the HOST output keep the comparison
    from passing vacuously: every action name fires >= 100 times, each stepwise action is also refused for >= 100 class-matching
    entries of >= 2 points, and the table passes 256 entries (the 256-thread chunk of the ordered compaction; 400 ids where
    max_age = 1 keeps fewer alive).  With max_size = 1 no orbit holds two points: only BreakInto(0, 0) fires."""
    frames, times = random_scene(0, n_ids, 60)
    acts = RANDOM_ACTIONS()
    host = A.ActionIdentify(acts, max_age, max_size)
    want, fired, refused, biggest = [], collections.Counter(), collections.Counter(), 0
    for det, t in zip(frames, times):
        want.append(as_tuples(host.update(det, t)))
        fired.update(r[2] for r in want[-1])
        biggest = max(biggest, len(host.cache))
        for o in host.cache.values():
            if o.age == 0 and len(o.deque) >= 2:
                refused.update(a.name for a in acts[:4] if a.class_id == o.class_id and not a.confirm(o))
    assert biggest > 256
    if max_size > 1:
        for name in ("takeoff", "landing", "glide", "fast_crossing", "break_into"):
            assert fired[name] >= 100, (name, fired)
        for name in ("takeoff", "landing", "glide", "fast_crossing"):
            assert refused[name] >= 100, (name, refused)
    else:
        assert set(fired) == {"break_into"} and fired["break_into"] >= 100
        assert all(r[1] == 0 for w in want for r in w)
    dev = A.DeviceActionIdentify(acts, max_age, max_size)
    got = []
    for k in range(0, 60, 20):                           # three calls of 20 frames: the table grows between calls
        got += dev.update_batch(frames[k:k + 20], [0] * 20, times[k:k + 20])
    for t in range(60):
        assert got[t] == want[t], t
    assert dev.orbits(0) == _host_orbits(host)


# ------------------------------------------------------------------------------------------------ 4. decision thresholds
def test_decision_thresholds():
    """Hand-built tracks whose every step sits exactly on a threshold (> and < are strict: no), one grid step beside it - 0.5 px in
    x (the foot point is x1 + w / 2), 1 px in y - (yes), a three-step track with a failing middle step, class mismatches.
    FastCrossing: dx = 5 px in dt = 0.0625 s is 0.08 px/ms exactly: not > 0.08, but > the double below 0.08."""
    acts = [A.TakeOff(0, (1, 2)), A.Landing(0, (1, 2)), A.Glide(0, (2, 2)), A.FastCrossing(2, 0.08),
            A.FastCrossing(2, float(np.nextafter(0.08, 0)))]
    # id: (class, per-step (x1 step, width step, y step)); foot dx = x1 step + width step / 2
    tracks = {
        1: (0, [(1, 0, -3)] * 3), 2: (0, [(1, 1, -2)] * 3), 3: (0, [(1, 1, -3)] * 3),                 # takeoff: dx on, dy on, beside
        4: (0, [(1, 0, 3)] * 3), 5: (0, [(1, 1, 2)] * 3), 6: (0, [(1, 1, 3)] * 3),                    # landing
        7: (0, [(2, 0, 1)] * 3), 8: (0, [(2, 1, 2)] * 3), 9: (0, [(2, 1, 1)] * 3),                    # glide
        10: (0, [(1, 1, -3), (1, 1, -2), (1, 1, -3)]),                                                  # a failing middle step
        11: (2, [(1, 1, -3)] * 3),                                                                      # takeoff's motion, another class
        12: (2, [(5, 0, 0)] * 3), 13: (2, [(5, 1, 0)] * 3),                                             # fast crossing: on, beside
        14: (0, [(5, 0, 0)] * 3),                                                                       # fast motion, another class
    }
    expect = {1: [], 2: [], 3: ["takeoff"], 4: [], 5: [], 6: ["landing"], 7: [], 8: [], 9: ["glide"], 10: [], 11: [],
              12: ["fast_crossing"], 13: ["fast_crossing", "fast_crossing"], 14: ["glide"]}
    state = {i: [100 * i, 10, 500] for i in tracks}      # x1, width, y2
    frames = []
    for t in range(5):                                   # frame 0 registers, frames 1-4 hold 4 points: 3 steps
        rows = []
        for i, (cls, steps) in tracks.items():
            if t >= 2:
                dx, dw, dy = steps[t - 2]
                state[i] = [state[i][0] + dx, state[i][1] + dw, state[i][2] + dy]
            x1, w, y2 = state[i]
            rows.append([x1, y2 - 40, x1 + w, y2, i, cls])
        frames.append(np.array(rows, np.int32))
    times = [t * 0.0625 for t in range(5)]
    assert 5 / (0.0625 * 1000) == 0.08
    host = A.ActionIdentify(acts, max_age=3, max_size=4)
    dev = A.DeviceActionIdentify(acts, max_age=3, max_size=4)
    got = dev.update_batch(frames, [0] * 5, times)
    for t in range(5):
        assert got[t] == as_tuples(host.update(frames[t], times[t])), t
    last = collections.defaultdict(list)
    for tid, cls, name in got[4]:
        assert cls == tracks[tid][0]
        last[tid].append(name)
    assert {i: last[i] for i in tracks} == expect
    # the raw rows: track 12 fires the SECOND fast-crossing entry (action index 4) only
    rows6 = np.ascontiguousarray(np.concatenate(frames), np.int32)
    first = np.arange(0, 15 * 6, 14, dtype=np.int32)[:6]
    raw = A.DeviceActionIdentify(acts, max_age=3, max_size=4)
    out, m = np.zeros((200, 4), np.int32), C.c_int(0)
    from yolo_deepsort_amd import _lib
    _lib.check(_lib.load().yds_actions_update(raw.handle, _lib.ptr(rows6), _lib.ptr(first), _lib.ptr(np.zeros(5, np.int32)),
                                              _lib.ptr(np.repeat(times, 14).astype(np.float64)), 5, _lib.ptr(out), 200, C.byref(m)))
    assert [r.tolist() for r in out[:m.value] if r[0] == 4 and r[1] == 12] == [[4, 12, 2, 4]]
    assert [r.tolist() for r in out[:m.value] if r[0] == 4 and r[1] == 13] == [[4, 13, 2, 3], [4, 13, 2, 4]]


# ------------------------------------------------------------------------------------------------ 5. lifecycle
def test_lifecycle_ageing_reset_and_capacity():
    from yolo_deepsort_amd import _lib
    acts = [A.BreakInto(0, 0)]
    dev = A.DeviceActionIdentify(acts, max_age=3, max_size=4, n_streams=2)
    host = A.ActionIdentify(acts, max_age=3, max_size=4)
    row = lambda i, x: [x, 0, x + 10, 40, i, 0]          # noqa: E731
    t = [0.0]

    def step(ids):
        t[0] += 0.04
        rows = np.array([row(i, int(100 * t[0]) + i) for i in ids], np.int32).reshape(-1, 6)
        got = dev.update(0, rows, t[0])
        assert got == as_tuples(host.update(rows, t[0])) and dev.orbits(0) == _host_orbits(host)
        return got
    assert step([1, 2]) == []
    assert step([1, 2]) == [(1, 0, "break_into"), (2, 0, "break_into")]
    step([2]); step([2])                                 # noqa: E702 - id 1 unseen for max_age - 1 frames
    assert dev.orbits(0)[0] == (1, 2, 1)
    assert (1, 0, "break_into") in step([1, 2]) and dev.orbits(0)[0] == (1, 0, 2)       # it kept its point and fires on return
    step([2]); step([2])                                 # noqa: E702
    assert [o[0] for o in dev.orbits(0)] == [1, 2]
    step([2])                                            # unseen for max_age frames: gone
    assert [o[0] for o in dev.orbits(0)] == [2]
    assert step([2, 1]) == [(2, 0, "break_into")]        # re-registered at the end of the table, nothing on that frame
    assert [o[:1] + o[2:] for o in dev.orbits(0)][1] == (1, 0)
    assert step([]) == [] and [o[1] for o in dev.orbits(0)] == [1, 1]                   # an empty frame ages everything
    before = dev.orbits(0)
    assert dev.update(1, np.array([row(7, 5), row(1, 9)], np.int32), 0.5) == []
    assert dev.orbits(0) == before and [o[0] for o in dev.orbits(1)] == [7, 1]           # stream 1's frame does not age stream 0
    dev.reset(0)
    assert dev.orbits(0) == [] and [o[0] for o in dev.orbits(1)] == [7, 1]
    dev.reset()
    assert dev.orbits(1) == []
    # ---- the C entry's refusals
    lib = _lib.load()
    two = np.array([row(1, 0), row(2, 0)], np.int32)
    dev.update(0, two, 0.0)
    out, m = np.zeros((1, 4), np.int32), C.c_int(0)
    args = (_lib.ptr(two), _lib.ptr(np.array([0, 2], np.int32)), _lib.ptr(np.zeros(1, np.int32)), _lib.ptr(np.full(2, 0.04)), 1)
    with pytest.raises(_lib.YdsError, match=r"\b2 action rows"):
        _lib.check(lib.yds_actions_update(dev.handle, *args, _lib.ptr(out), 1, C.byref(m)))
    assert m.value == 2
    dup = np.array([row(5, 0), row(5, 3)], np.int32)
    with pytest.raises(_lib.YdsError, match="twice"):
        dev.update(0, dup, 1.0)
    with pytest.raises(_lib.YdsError, match="stream"):
        dev.update(2, two, 1.0)
    k, c, p = np.array([4], np.int32), np.array([0], np.int32), np.zeros((1, 2))
    assert not lib.yds_actions_create(1, _lib.ptr(k), _lib.ptr(c), _lib.ptr(p), 1, 3, 17) and "max_size" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ 6. inside the pipeline
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
    """tests/test_gpu_multi_stream.py _play with a hook ahead of every step: per step a list of (stream, frame index); the next
    step's frames are handed over (look-ahead) when it has as many frames."""
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


@pytest.mark.parametrize("host_frames", [False, True])
def test_pipeline_actions_equal_host_clones_and_leave_tracking_alone(host_frames):
    """yolov3-tiny 416 on 480x640 frames, three trackers, injected PersonScene detections, the step schedule of
    test_three_tracker_settings_equal_the_single_stream_path_bit_for_bit (steps where a stream has no frame or several, a
    detector-None frame per stream, a mask-emptied frame) plus two steps of the last step's size so that look-ahead passes run.
    last_actions() per frame equals host ActionIdentify clones fed the returned rows and the same times, None where the rows
    are None (the clone is not called there); a second pipeline without actions returns the same rows and tracker state."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=8, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0))
    ex = Extractor(synth.reid_state_dict(0), max_crops=256)
    settings = [dict(DS), dict(DS, metric="euclidean", max_dist=0.5), dict(DS, nn_budget=None, max_age=4)]
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
                rows = rows[:0]                                     # the detector returns None: tracker and action stage not called
            if t == 7 and s == 1:
                rows[:, 8] = 5                                      # every detection masked: D = 0, every orbit of the stream ages
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
    acts = [A.TakeOff(0, (0, 0)), A.Landing(0, (0, 0)), A.Glide(0, (0, 3)), A.FastCrossing(0, 0.01), A.BreakInto(0, 1), A.BreakInto(2, 0),
            A.Glide(2, (0, 3))]
    ident = A.ActionIdentify(acts, max_age=2, max_size=3)
    time_of = lambda s, k: 0.04 * k + 0.001 * s          # noqa: E731

    def run(with_actions):
        trackers = [DeepSort(ex, use_cuda=True, **p) for p in settings]
        pipe = pl.MultiStreamPipeline(net, trackers, 0.5, 0.4, class_mask=mask)
        if with_actions:
            pipe.set_actions(ident)
        else:
            assert pipe.last_actions() is None
        rows, acts_got, states = [], [], []

        def before(i):
            if with_actions:
                pipe.set_frame_times([time_of(s, k) for s, k in steps[i]])

        def after(i, outs):
            rows.append(outs)
            acts_got.append(pipe.last_actions())
            states.append({s: _tracker_full(trackers[s]) for s in {s for s, _ in steps[i]}})
        n_ahead = _play(pipe, net, steps, lambda s, k: frames[s][k], lambda s, k: injs[s][k], (480, 640), host_frames, before, after)
        assert n_ahead >= 2
        return rows, acts_got, states
    rows, acts_got, states = run(True)
    clones = [ident.clone() for _ in range(3)]
    n_rows = n_none = 0
    for i, st in enumerate(steps):
        assert len(acts_got[i]) == len(st)
        for b, (s, k) in enumerate(st):
            if rows[i][b] is None:
                assert acts_got[i][b] is None, (i, b)
                n_none += 1
                continue
            want = as_tuples(clones[s].update(rows[i][b], time_of(s, k)))
            assert acts_got[i][b] == want, (i, b, s, k)
            n_rows += len(want)
    assert n_rows >= 20 and n_none == 3
    plain_rows, plain_acts, plain_states = run(False)
    assert all(a is None for a in plain_acts)
    for i, st in enumerate(steps):
        for b in range(len(st)):
            a, p = rows[i][b], plain_rows[i][b]
            assert (a is None) == (p is None) and (a is None or (a.shape == p.shape and np.array_equal(a, p))), (i, b)
        for s, full in states[i].items():
            for key in ("ids", "state", "tsu", "hits", "mean", "cov", "payload", "age", "um_t", "um_d"):
                assert np.array_equal(full[key], plain_states[i][s][key]), (i, s, key)


def test_pipeline_frame_times_default_to_the_frame_count_over_25():
    """Without set_frame_times a stream's k-th frame since the pipeline was made carries k / 25: the single-stream Pipeline over
    6 steps of 2 frames against a host clone fed the returned rows with those times."""
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
    acts = [A.FastCrossing(0, 0.02), A.BreakInto(0, 1), A.Glide(0, (0, 3))]
    ident = A.ActionIdentify(acts, max_age=2, max_size=3)
    pipe = pl.Pipeline(net, ds, 0.5, 0.4, class_mask=[0])
    pipe.set_actions(ident)
    clone, n = ident.clone(), 0
    for i in range(T // 2):
        pl.select_injection_set(net, i)
        dev = _lib.DeviceBuffer.from_array(np.stack([scene.frame(2 * i), scene.frame(2 * i + 1)]))
        outs = pipe.step(dev.ptr, 480, 640, 2)
        got = pipe.last_actions()
        for b in range(2):
            assert outs[b] is not None
            want = as_tuples(clone.update(outs[b], (2 * i + b) / 25.0))
            assert got[b] == want, (i, b)
            n += len(want)
    assert n >= 10
    with pytest.raises(_lib.YdsError, match="frame times"):
        pipe.set_frame_times([0.0, 1.0, 2.0])
        pipe.step(dev.ptr, 480, 640, 2)
    with pytest.raises(ValueError, match="action_id"):
        pipe.set_actions(object())
    pipe.set_actions(None)
    assert pipe.last_actions() is None


# ------------------------------------------------------------------------------------------------ 7. VideoDetector.detect_streams
def test_detect_streams_carries_each_streams_actions(tmp_path):
    """Three in-memory clips, skip_frames=2, an ActionIdentify of the five built-ins: per stream the fourth item equals a host clone
    fed that stream's processed, non-None rows with times frame index / 25 - [] on skipped frames, the previous value on
    detector-None frames; frames_per_stream=1 and the default give the same items."""
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
    acts = [A.TakeOff(0, (0, 0)), A.Landing(0, (0, 0)), A.Glide(0, (0, 5)), A.FastCrossing(0, 0.001)]
    acts += [A.BreakInto(c, 0) for c in range(0, 56, 2)]
    ident = A.ActionIdentify(acts, max_age=3, max_size=4)
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())
    per = {}
    for fps in (1, None):
        vd = VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=base, skip_frames=2, class_mask=list(range(0, 80, 2)),
                           action_id=ident)
        per[fps] = [[] for _ in clips]
        for step in vd.detect_streams(clips, frames_per_stream=fps, show_fps=False):
            for s, _, det, act in step:
                per[fps][s].append((det, act))
    assert ident.cache == {}                                           # the caller's own cache is not touched
    for fps in (1, None):
        for s, clip in enumerate(clips):
            assert len(per[fps][s]) == len(clip)
            clone, prev = ident.clone(), []
            for k, (det, act) in enumerate(per[fps][s]):
                if k % 2:
                    prev = []                                           # a skipped frame
                elif det is not None:
                    prev = as_tuples(clone.update(det, k / 25.0))
                assert act == prev, (fps, s, k)
    assert any(det is not None and len(det) for s in range(3) for det, _ in per[1][s])
    assert sum(len(act) for s in range(3) for _, act in per[1][s]) > 0
    for s in range(3):
        for k, (a, b) in enumerate(zip(per[1][s], per[None][s])):
            assert a[1] == b[1], ("fps 1 vs default", s, k)
