"""The host half of detect_streams' device form, without a GPU: the grouping of the steps (detect.stream_groups) against a direct
restatement of the loop detect_streams has always run, the staging plan (detect.stage_plan: slot order, offsets), the look-ahead
decision (detect.same_composition), and the tables DeviceOverlay.render_mixed hands to the device (label_draw.mixed_tables) fed
through the numpy renderer of those tables and compared with the host overlay."""
import numpy as np
import pytest

from yolo_deepsort_amd import cfgs
from yolo_deepsort_amd.detect import STAGE_ALIGN, same_composition, stage_plan, stream_groups
from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer, draw_tables_host, frame_scale, put_text
from yolo_deepsort_amd.privacy import Anonymize, anonymize, mask_rects


def _clip(n, h, w, tag):
    return [np.full((h, w, 3), (tag * 16 + t) % 256, np.uint8) for t in range(n)]


def _todays_loop(clips, F, skip_frames):
    """detect_streams' own loop, restated: per step, per stream up to F processed frames, the skip gate, time = index / 25."""
    S = len(clips)
    its = [iter(c) for c in clips]
    since, alive, n_read = [0] * S, [True] * S, [0] * S
    steps = []
    while any(alive):
        items = []
        for s in range(S):
            n_proc = 0
            while alive[s] and n_proc < F:
                frame = next(its[s], None)
                if frame is None:
                    alive[s] = False
                    break
                t = n_read[s] / 25.0
                n_read[s] += 1
                proc = since[s] % skip_frames == 0
                if proc:
                    since[s] = 0
                since[s] += 1
                n_proc += proc
                items.append((s, frame, proc, t))
        if items:
            steps.append(items)
    return steps


@pytest.mark.parametrize("skip_frames", [-1, 1, 2, 3])
@pytest.mark.parametrize("F", [1, 2, 3])
def test_groups_are_those_of_the_host_loop(skip_frames, F):
    clips = [_clip(11, 6, 8, 0), _clip(4, 6, 8, 1), _clip(7, 6, 8, 2)]           # stream 1 ends mid-run, stream 2 later
    want = _todays_loop(clips, F, skip_frames)
    got = list(stream_groups([iter(c) for c in clips], F, skip_frames))
    assert len(got) == len(want) and sum(len(g) for g in got) == 22
    for g, w in zip(got, want):
        assert [(s, p, t) for s, _, p, t in g] == [(s, p, t) for s, _, p, t in w]
        assert all(a[1] is b[1] for a, b in zip(g, w))                            # the very frames, in the very order
    assert {s for s, *_ in got[0]} == {0, 1, 2} and 1 not in {s for s, *_ in got[-1]}


def test_frame_times_follow_the_source():
    ticks = iter(range(100, 200))
    rates = iter([30.0, None])                                                    # asked once per stream, after its first frame
    got = list(stream_groups([iter(_clip(3, 4, 4, 0)), iter(_clip(3, 4, 4, 1)), iter(_clip(2, 4, 4, 2))], 1, -1, live=[False, False, True],
                             source_fps=lambda: next(rates, None), clock=lambda: next(ticks)))
    times = {s: [t for g in got for ss, _, _, t in g if ss == s] for s in range(3)}
    assert times[0] == [0 / 30.0, 1 / 30.0, 2 / 30.0] and times[1] == [0.0, 1 / 25.0, 2 / 25.0] and times[2] == [100, 101]


def test_shape_changes_are_refused_with_the_stream_named():
    a, b = np.zeros((6, 8, 3), np.uint8), np.zeros((4, 5, 3), np.uint8)
    with pytest.raises(ValueError, match=r"stream 1 must keep one uint8 \[h, w, 3\] shape"):
        list(stream_groups([iter([a, a, a]), iter([b, b, a])], 1, -1, mixed_sizes=True))
    with pytest.raises(ValueError, match="in stream 1"):
        list(stream_groups([iter([a, a]), iter([a, b])], 1, -1))
    with pytest.raises(ValueError, match="stream 0"):
        list(stream_groups([iter([a.astype(np.float32)])], 1, -1, mixed_sizes=True))
    assert len(list(stream_groups([iter([a, a]), iter([b, b])], 1, -1, mixed_sizes=True))) == 2


def test_stage_plan_puts_processed_frames_first_at_aligned_offsets():
    clips = [_clip(9, 5, 7, 0), _clip(9, 33, 50, 1), _clip(9, 36, 48, 2)]
    for skip in (1, 2, 3):
        for F in (1, 2):
            for items in stream_groups([iter(c) for c in clips], F, skip, mixed_sizes=True):
                p = stage_plan(items, True)
                n = len(items)
                assert sorted(p["slot_of"]) == list(range(n)) and [p["slot_of"][i] for i in p["order"]] == list(range(n))
                proc = [i for i, it in enumerate(items) if it[2]]
                assert p["order"][:len(proc)] == proc and p["n_proc"] == len(proc)                  # processed first, in step order
                assert p["order"][len(proc):] == [i for i, it in enumerate(items) if not it[2]]
                assert p["streams"] == [items[i][0] for i in proc]
                assert (p["off"] % STAGE_ALIGN == 0).all() and STAGE_ALIGN == 256
                ends = [int(p["off"][k]) + 3 * int(p["hw"][k][0]) * int(p["hw"][k][1]) for k in range(n)]
                assert all(ends[k] <= int(p["off"][k + 1]) < ends[k] + STAGE_ALIGN for k in range(n - 1))   # no overlap, no waste
                assert p["nbytes"] == ends[-1] and p["proc_bytes"] == (ends[len(proc) - 1] if proc else 0)
                assert [tuple(p["hw"][p["slot_of"][i]]) for i in range(n)] == [it[1].shape[:2] for it in items]
    # a uniform step is packed h * w * 3 apart: the layout of the uniform entries
    items = next(stream_groups([iter(_clip(2, 5, 7, s)) for s in range(3)], 1, -1))
    p = stage_plan(items, False)
    assert p["off"].tolist() == [0, 105, 210] and p["nbytes"] == 315 and not p["mixed"]


def test_look_ahead_only_for_the_same_composition():
    def plans(clips, F, skip, mixed=True):
        return [stage_plan(items, mixed) for items in stream_groups([iter(c) for c in clips], F, skip, mixed_sizes=mixed)]
    p = plans([_clip(6, 5, 7, 0), _clip(3, 33, 50, 1)], 1, -1)
    assert [same_composition(a, b) for a, b in zip(p, p[1:] + [None])] == [True, True, False, True, True, False]     # stream 1 ends
    p = plans([_clip(6, 5, 7, 0), _clip(6, 5, 7, 1)], 1, 2, mixed=False)
    # skip 2: step 0 holds two processed frames, every later one a skipped and a processed frame per stream, the last only skipped
    assert [q["n_proc"] for q in p] == [2, 2, 2, 0]
    assert [same_composition(a, b) for a, b in zip(p, p[1:] + [None])] == [True, True, False, False]
    a = stage_plan([(0, np.zeros((5, 7, 3), np.uint8), True, 0.0), (1, np.zeros((5, 7, 3), np.uint8), True, 0.0)], True)
    b = stage_plan([(0, np.zeros((5, 7, 3), np.uint8), True, 0.0), (1, np.zeros((6, 7, 3), np.uint8), True, 0.0)], True)
    c = stage_plan([(1, np.zeros((5, 7, 3), np.uint8), True, 0.0), (0, np.zeros((5, 7, 3), np.uint8), True, 0.0)], True)
    d = stage_plan([(0, np.zeros((5, 7, 3), np.uint8), True, 0.0), (1, np.zeros((5, 7, 3), np.uint8), True, 0.0)], False)
    assert same_composition(a, a) and not same_composition(a, b) and not same_composition(a, c) and not same_composition(a, d)
    assert not same_composition(a, None) and not same_composition(None, a)


# ---------------------------------------------------------------------------------------------- render_mixed's tables
def _classes():
    return cfgs.coco_names_text().split("\n")[:-1]


@pytest.mark.parametrize("only_rect", [False, True])
@pytest.mark.parametrize("thickness", [1, 2, -1])
def test_mixed_tables_through_the_numpy_renderer_equal_the_host_overlay(thickness, only_rect):
    sizes = [(5, 7), (33, 50), (1300, 16), (270, 480), (750, 40), (1080, 64)]
    assert [frame_scale(h) for h, _ in sizes] == [1, 1, 3, 1, 2, 2]                 # 750 -> round(1.5) = 2: ties to even, as Python rounds
    rng = np.random.RandomState(4)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in sizes]
    drawer = LabelDrawer(_classes(), None, 10, thickness, (608, 608))
    drawer.id2label = {"7": "someone"}
    ov = DeviceOverlay(drawer)
    slots = [3, 0, 5, 2, 1, 3, 4]                                                   # a permutation, one slot twice
    holds = []
    for s in slots:
        h, w = sizes[s]
        holds.append(np.array([[-3, -2, w // 2, h // 2, 1, 0], [200, 100, 400, 250, 7, 2], [w - 5, 2, w + 9, h - 1, 3, 5],
                               [w // 4, h // 4, 3 * w // 4, 3 * h // 4, 4, 0]], np.int32))
    holds[1], holds[4] = None, []
    dets = [np.array([[1.5, 2.25, w / 2.0, h / 3.0, 0], [w - 2.5, h - 1.5, 9, 9, 0]], np.float32) for h, w in (sizes[s] for s in slots)]
    fps = ["FPS: 12", None, "FPS: 3", None, "FPS: 4", None, None]
    for anon in (None, Anonymize(block=3), Anonymize(mode="fill", color=(9, 200, 30), margin=2)):
        t = ov.mixed_tables(sizes, slots, holds, fps, only_rect, anon, dets if anon is not None else None)
        assert t["sizes"] == [sizes[s] for s in slots] and t["scales"] == [frame_scale(sizes[s][0]) for s in slots]
        assert t["out_off"].tolist() == np.concatenate([[0], np.cumsum([3 * h * w for h, w in t["sizes"]])[:-1]]).tolist()
        assert t["out_bytes"] == sum(3 * h * w for h, w in t["sizes"]) and t["box_ptr"].tolist() == [0, 4, 4, 8, 12, 12, 16, 20]
        for i, s in enumerate(slots):
            h, w = sizes[s]
            # the definition, on the frame at its own size
            img = frames[s].copy()
            if anon is not None:
                rects = mask_rects(anon, h, w, holds[i], dets[i])
                img = anonymize(img, rects, anon) if rects else img
            if holds[i] is not None and len(holds[i]):
                drawer.draw_labels_by_trackers(img, holds[i], only_rect)
            want = np.ascontiguousarray(img[:, :, ::-1])
            if fps[i]:
                put_text(want, fps[i], (3, 15), 2, (255, 0, 0))
            # the tables: this frame's rectangles (each frame's own clip), then its boxes at its own scale
            got = frames[s].copy()
            if anon is not None:
                table, ptr = t["mask"][0], t["mask"][1]
                mine = [tuple(r) for r in table[ptr[i]:ptr[i + 1]].tolist()]
                assert mine == [tuple(r) for r in mask_rects(anon, h, w, holds[i], dets[i])]
                got = anonymize(got, mine, anon)
            got = np.ascontiguousarray(got[:, :, ::-1])
            draw_tables_host(got, t["boxes"][t["box_ptr"][i]:t["box_ptr"][i + 1]], t["text"], t["fps"][i], thickness, t["scales"][i])
            assert np.array_equal(got, want), (thickness, only_rect, anon and anon.mode, i, s)
    # a rectangle that the large frame keeps is clipped away in the small one
    anon = Anonymize(classes=None)
    row = np.array([[100, 100, 200, 200, 1, 0]], np.int32)
    t = ov.mixed_tables(sizes, [0, 3], [row, row], privacy=anon)
    assert t["mask"][1].tolist() == [0, 0, 1]
    with pytest.raises(ValueError, match="slots"):
        ov.mixed_tables(sizes, [6], [row])
    with pytest.raises(ValueError, match="2 slots for 1 frames"):
        ov.mixed_tables(sizes, [0, 1], [row])
