"""The shared host pieces of VideoDetector.detect / detect_streams (yolo_deepsort_amd/staging.py), without a GPU: a single video
grouped as a stream group of one against a restatement of the loop detect() used to run, the layout detect()'s reader stages by,
the per-frame bookkeeping against the rules of video_detect.py:134-159, and detect_streams end to end - both forms - over a
stand-in pipeline."""
import queue
import threading
import time

import numpy as np
import pytest

from yolo_deepsort_amd import cfgs
from yolo_deepsort_amd import detect as D
from yolo_deepsort_amd.staging import Bookkeeper, stage_steps


def _frames(n, h=4, w=6):
    return [np.full((h, w, 3), t, np.uint8) for t in range(n)]


def _video_detector(skip_frames, batch_frames):
    """A VideoDetector as far as its grouping goes (no model, no tracker)."""
    vd = object.__new__(D.VideoDetector)
    vd.skip_frames, vd.batch_frames, vd._batch_now = skip_frames, batch_frames, None
    return vd


def _yesterdays_batches(frames, bf, skip_frames):
    """detect()'s own grouping loop as it stood before a single video became a stream group of one, restated."""
    groups, group, n_proc, since = [], [], 0, 0
    for frame in frames:
        proc = since % skip_frames == 0
        if proc:
            since = 0
        since += 1
        group.append((frame, proc))
        n_proc += proc
        if n_proc == bf:
            groups.append(group)
            group, n_proc = [], 0
    if group:
        groups.append(group)
    return groups


@pytest.mark.parametrize("skip_frames", [-1, 1, 2, 3, 5])
@pytest.mark.parametrize("bf", [1, 2, 3, 4, 7])
def test_a_single_video_is_grouped_as_before(skip_frames, bf):
    for n in range(14):                                   # zero frames, fewer than one batch, several batches
        frames = _frames(n)
        want = _yesterdays_batches(frames, bf, skip_frames)
        got = list(_video_detector(skip_frames, bf)._video_steps(frames))
        assert len(got) == len(want), (skip_frames, bf, n)
        for g, w in zip(got, want):
            assert [(s, bool(p)) for s, _, p, _ in g] == [(0, bool(p)) for _, p in w]
            assert all(a[1] is b[0] for a, b in zip(g, w))                        # the very frames, in the very order
        pairs = list(_video_detector(skip_frames, bf)._processed_batches(frames))  # the adapter tests and tools preload tables by
        assert [[(id(f), bool(p)) for f, p in g] for g in pairs] == [[(id(f), bool(p)) for f, p in g] for g in want]


def test_a_last_group_of_skipped_frames_only_is_still_a_group():
    got = list(_video_detector(3, 2)._video_steps(_frames(7)))             # P s s P | s s P + end -> the second group ends with the clip
    assert [[bool(p) for _, _, p, _ in g] for g in got] == [[True, False, False, True], [False, False, True]]
    got = list(_video_detector(3, 2)._video_steps(_frames(6)))
    assert [[bool(p) for _, _, p, _ in g] for g in got] == [[True, False, False, True], [False, False]]
    assert list(_video_detector(3, 2)._video_steps([])) == []
    with pytest.raises(ValueError, match=r"^VideoDetector: frames of one video must share one uint8 \[h, w, 3\] shape$"):
        list(_video_detector(-1, 4)._video_steps(_frames(2) + [np.zeros((5, 6, 3), np.uint8)]))


def test_the_reader_of_detect_stages_processed_frames_first_one_frame_apart():
    """What detect()'s reader thread hands to the upload: skip 3, four processed frames a group - P s s P s s P s s P."""
    h, w = 5, 7
    frames = _frames(12, h, w)
    staged, out_q, free_q = [], queue.Queue(), queue.Queue()
    for _ in range(4):
        free_q.put(dict(dev=None, pin=None))

    def upload(blk, plan, group_frames):
        staged.append((plan, group_frames))
    stage_steps(_video_detector(3, 4)._video_steps(frames), False, upload, out_q, free_q, threading.Event())
    records = [out_q.get_nowait() for _ in range(3)]
    assert records[2] is None and out_q.empty() and len(staged) == 2
    plan, group_frames = staged[0]
    assert records[0]["plan"] is plan and [f[0, 0, 0] for f in group_frames] == list(range(10))
    assert records[0]["items"] == [(0, t % 3 == 0, t / 25.0) for t in range(10)]          # the items without their frames
    assert plan["order"] == [0, 3, 6, 9, 1, 2, 4, 5, 7, 8] and plan["n_proc"] == 4 and not plan["mixed"]
    assert plan["off"].tolist() == [k * h * w * 3 for k in range(10)] and plan["nbytes"] == 10 * h * w * 3
    assert plan["proc_bytes"] == 4 * h * w * 3 and plan["streams"] == [0, 0, 0, 0]
    assert [plan["order"][plan["slot_of"][i]] for i in range(10)] == list(range(10))      # slot_of maps every group index back
    assert plan["hw"].tolist() == [[h, w]] * 10
    assert staged[1][0]["order"] == [0, 1] and staged[1][0]["n_proc"] == 0 and staged[1][0]["proc_bytes"] == 0   # frames 10, 11: s s


# ------------------------------------------------------------------------------------------------------- the bookkeeper
def _tag(hold):
    return ["host", int(hold[0][0]) if len(hold) else "nobody"]


def _rules(frames, device):
    """video_detect.py:134-159 for one stream, restated: frames of (processed, rows or None, detections, actions)."""
    hold, dets, actions, out = None, None, [], []
    for proc, rows, det, acts in frames:
        if proc:
            dets = det
            if rows is not None:
                hold = rows if len(rows) else []
                actions = acts if device else _tag(hold)
            else:
                hold = None                                # (the previous actions stay)
        else:
            actions = []
        out.append((hold, dets, actions))
    return out


@pytest.mark.parametrize("device", [True, False])
def test_bookkeeper_follows_the_reference_rules_per_stream(device):
    rows = lambda v: np.full((2, 6), v, np.int32)
    empty = np.zeros((0, 6), np.int32)
    # per stream: rows, then a skipped frame, a detector-None frame and an empty-rows frame in that order, then rows and None again
    script = {0: [(True, rows(1), "d0", ["a0"]), (False, None, None, None), (True, None, "d1", None), (True, empty, "d2", []),
                  (True, rows(2), "d3", ["a1"]), (True, None, "d4", None)],
              1: [(True, rows(7), "e0", ["b0"]), (True, rows(8), "e1", ["b1"]), (False, None, None, None), (True, None, "e2", None),
                  (True, empty, "e3", []), (True, rows(9), "e4", ["b2"])]}
    want = {s: _rules(fr, device) for s, fr in script.items()}
    calls = []

    def host_actions(hold):
        calls.append(hold)
        return _tag(hold)
    book, got, expected_calls = Bookkeeper(2), {0: [], 1: []}, []
    for a in range(0, 6, 2):                                                       # three steps, two frames of each stream in each
        step = [(s, t) for s in (0, 1) for t in (a, a + 1)]
        procs = [(s, t) for s, t in step if script[s][t][0]]
        outs = [script[s][t][1] for s, t in procs]
        holds, dets, acts = book.update([(s, script[s][t][0], t / 25.0) for s, t in step], outs,
                                        step_acts=[script[s][t][3] for s, t in procs] if device else None,
                                        step_dets=[script[s][t][2] for s, t in procs], host_actions=None if device else host_actions)
        assert len(holds) == len(dets) == len(acts) == len(step)
        for (s, t), h, d, ac in zip(step, holds, dets, acts):
            got[s].append((h, d, ac))
        expected_calls += [want[s][t][0] for s, t in procs if script[s][t][1] is not None]
    for s in (0, 1):
        for t, ((h, d, ac), (wh, wd, wa)) in enumerate(zip(got[s], want[s])):
            assert d == wd and ac == wa, (s, t, d, wd, ac, wa)
            if wh is None or len(wh) == 0:
                assert h is None if wh is None else isinstance(h, list) and h == [], (s, t, h)
            else:
                assert h is wh, (s, t)
    # the host callable: only for processed frames whose detector returned rows, in frame order, with the hold that is yielded
    assert len(calls) == (0 if device else 7) and len(expected_calls) == 7
    assert [_tag(c) for c in calls] == [_tag(w) for w in expected_calls][:len(calls)]


# ------------------------------------------------------------------------------------- detect_streams over a stand-in pipeline
class _Model:
    img_size, batch_max = (64, 64), 4

    def eval(self):
        return self

    def parameters(self):
        yield type("P", (), {"device": "cpu"})()

    def set_batch_max(self, n):
        self.batch_max = n


class _Tracker:
    nms_max_overlap = 1.0

    def clone(self):
        return _Tracker()


class _Buf:
    def offset(self, o):
        return self


class _StreamsPipe:
    """pipeline.MultiStreamPipeline as far as detect_streams calls it: scripted rows per stream - a stream's k-th processed frame
    gives rows naming (stream, k), None when k % 3 == 1, empty rows when k % 3 == 2."""
    made = []

    def __init__(self, model, trackers, thres, nms_thres, **kw):
        self.count, self.aheads, self.identities = [0] * len(trackers), [], None
        _StreamsPipe.made.append(self)

    def set_frame_order(self, bgr):
        assert not bgr

    def set_identities(self, on, **memory):
        self.identities = on

    def step(self, frames_dev, h, w, streams, ahead=None, select_next=None):
        self.aheads.append(ahead)
        outs = []
        for s in streams:
            k = self.count[s]
            self.count[s] += 1
            outs.append(None if k % 3 == 1 else np.zeros((0, 6), np.int32) if k % 3 == 2 else np.array([[1, 2, 30, 40, s + 1, k]], np.int32))
        return outs


@pytest.fixture
def streams_detector(tmp_path, monkeypatch):
    from yolo_deepsort_amd import pipeline
    monkeypatch.setattr(pipeline, "MultiStreamPipeline", _StreamsPipe)
    monkeypatch.delenv("YDS_HOST_OVERLAY", raising=False)
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())
    _StreamsPipe.made = []

    def make(device_overlay, **kw):
        vd = D.VideoDetector(_Model(), str(names), tracker=_Tracker(), device_overlay=device_overlay, **kw)
        vd._batchable = lambda: True                              # the stand-in tracker plays the package's DeepSort
        # stand-ins for the two device hooks: the staged step stays on the host, the output stage is the host form
        vd._upload_step = lambda blk, plan, fr: blk.update(dev=_Buf(), host=list(fr))
        vd._render_step = lambda cur, holds, dets, fps, bgr: [vd._render_host(cur["blk"]["host"][i], holds[i], None) for i in range(len(holds))]
        return vd
    return make


def _clip(n, tag):
    return [np.full((48, 64, 3), (tag * 40 + t) % 256, np.uint8) for t in range(n)]


def _threads_back_to(before):
    deadline = time.time() + 3
    while threading.active_count() > before and time.time() < deadline:
        time.sleep(0.02)
    return threading.active_count() == before


def test_both_forms_of_detect_streams_yield_the_same_steps(streams_detector):
    clips = [_clip(11, 0), _clip(3, 1), _clip(9, 2)]                                 # stream 1 ends early
    before = threading.active_count()
    runs = {}
    for device in (False, True):
        vd = streams_detector(device, skip_frames=2)
        runs[device] = list(vd.detect_streams([list(c) for c in clips], frames_per_stream=2, show_fps=False))
        assert vd._streams_pipe is None
    assert _threads_back_to(before)
    host, dev = runs[False], runs[True]
    assert len(host) == len(dev) == 3 and sum(len(st) for st in host) == 23
    seen = set()
    for a, b in zip(host, dev):
        assert len(a) == len(b)
        for (s, img, hold, acts), (s2, img2, hold2, acts2) in zip(a, b):
            assert s == s2 and np.array_equal(img, img2) and acts == acts2 == []
            assert (hold is None) == (hold2 is None) and (hold is None or np.array_equal(np.asarray(hold).reshape(-1, 6), np.asarray(hold2).reshape(-1, 6)))
            seen.add("none" if hold is None else "empty" if len(hold) == 0 else "rows")
    assert seen == {"none", "empty", "rows"}
    assert [s for s, *_ in host[0]] == [0, 0, 0, 1, 1, 1, 2, 2, 2]                  # P s P of every stream
    host_pipe, dev_pipe = _StreamsPipe.made
    assert host_pipe.count == dev_pipe.count and not any(a is not None for a in host_pipe.aheads)


def test_closing_detect_streams_joins_its_reader(streams_detector):
    before = threading.active_count()
    vd = streams_detector(True)
    gen = vd.detect_streams([(np.zeros((48, 64, 3), np.uint8) for _ in range(10000)) for _ in range(3)], frames_per_stream=2, show_fps=False)
    assert len(next(gen)) == 6 and vd._streams_reader.is_alive()
    gen.close()
    vd._streams_reader.join(timeout=3)
    assert not vd._streams_reader.is_alive() and vd._streams_pipe is None
    assert _threads_back_to(before)


@pytest.mark.parametrize("device", [False, True])
def test_a_raising_source_surfaces_after_the_steps_staged_before_it(streams_detector, device):
    class Broken(Exception):
        pass

    def source():
        yield from _clip(3, 1)
        raise Broken("camera 1 fell over")
    before = threading.active_count()
    vd, got = streams_detector(device), []
    with pytest.raises(Broken, match="camera 1"):
        for step in vd.detect_streams([_clip(9, 0), source()], frames_per_stream=1, show_fps=False):
            got.append([s for s, *_ in step])
    assert got == [[0, 1]] * 3 and vd._streams_pipe is None
    assert _threads_back_to(before)


def test_global_ids_never_hand_the_pipeline_a_look_ahead_buffer(streams_detector):
    for global_ids in (False, True):
        vd = streams_detector(True)
        steps = list(vd.detect_streams([_clip(5, 0), _clip(5, 1)], frames_per_stream=1, show_fps=False, global_ids=global_ids))
        pipe = _StreamsPipe.made[-1]
        assert len(steps) == 5 and len(pipe.aheads) == 5 and pipe.identities == (True if global_ids else None)
        if global_ids:
            assert pipe.aheads == [None] * 5 and vd.streams_lookahead == [0, 5]
        else:                                                 # uniform sources that are not live: every step but the last
            assert [a is not None for a in pipe.aheads] == [True] * 4 + [False] and vd.streams_lookahead == [4, 5]
