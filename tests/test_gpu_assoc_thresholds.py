"""The association's decisions ON their thresholds: tests/golden/assoc_thresholds.npz (oracle/gen_golden.py gen_assoc_thresholds)
holds scripted scenes the real reference ran on either side of one threshold each - max_dist, max_iou_distance, the chi-square
gate, the eviction of the oldest gallery row, the tracker-side NMS.  The device tracker must take the reference's side in every run.
The loader and the fixture conditions are shared with the oracle replay in test_oracle_reid_tracker.py."""
import numpy as np
import pytest

from conftest import check_int_rows, golden

pytestmark = pytest.mark.gpu
F32 = np.float32
CHI2_2DOF = 5.9915
SCENES = ("max_dist", "max_iou_distance", "gate", "ring", "nms")


def threshold_runs():
    """{(scene, run): dict(params={name: value}, frames=[{field: array}])} from the flat store of the fixture: row i of `index` =
    (run, frame, field, kind, offset, rows, cols) names a slice of `ints` (kind 0) or `floats` (kind 1); cols 0 = one-dimensional."""
    g = golden("assoc_thresholds")
    assert all(g[k].dtype != object for k in g.files)                       # arrays only
    fields, pnames, stores = [str(s) for s in g["fields"]], [str(s) for s in g["param_names"]], (g["ints"], g["floats"])
    runs = {}
    for name, prow in zip(g["runs"], g["params"]):
        params = {k: float(v) for k, v in zip(pnames, prow) if not np.isnan(v)}
        for k in ("nn_budget", "n_init", "max_age"):
            params[k] = int(params[k])
        runs[tuple(str(name).split("."))] = dict(params=params, frames=[])
    keys = list(runs)
    for ri, t, fi, kind, off, rows, cols in g["index"]:
        frames = runs[keys[ri]]["frames"]
        while len(frames) <= t:
            frames.append({})
        v = stores[kind][off:off + rows * max(cols, 1)]
        frames[t][fields[fi]] = v.reshape(rows, cols) if cols else v
    return runs


def feats_of(frame):
    f = np.zeros((len(frame["sign16"]), 512), F32)
    f[:, :16] = frame["sign16"]
    return f


def id_set(run):
    return frozenset(int(i) for fr in run["frames"] for i in fr["ids"])


def check_fixture_conditions(runs):
    """What gen_assoc_thresholds asserted when it wrote the fixture: the reference's outcome differs across every threshold, and
    the costs it computed are the constructed values, bit for bit (the gate: at the stated margin)."""
    assert {s for s, _ in runs} == set(SCENES)
    for scene in SCENES:
        assert len({id_set(r) for (s, _), r in runs.items() if s == scene}) >= 2, scene
    half = F32(0.5)
    for tag, thr in (("under", np.nextafter(half, F32(0))), ("on", half), ("over", np.nextafter(half, F32(1)))):
        r = runs["max_dist", tag]
        assert F32(r["params"]["max_dist"]) == thr and r["params"]["max_dist"] == float(thr)
        assert r["frames"][3]["cos"].tobytes() == half.tobytes()                # exactly 0.5
        assert r["frames"][3]["gate"][0, 0] < 3.0                               # well inside the gate
        assert len(r["frames"][3]["matches"]) == (0 if tag == "under" else 1)
    assert (runs["max_dist", "under"]["frames"][3]["iou"] == 1.0).all()         # IOU 0 to the prediction: no rescue
    assert id_set(runs["max_dist", "under"]) == {1, 2} and id_set(runs["max_dist", "on"]) == id_set(runs["max_dist", "over"]) == {1}
    c = F32(1) - F32(1225) / F32(2871)                                          # 25 x 49 px intersection of two 32 x 64 boxes
    for tag, thr in (("under", np.nextafter(c, F32(0))), ("on", c), ("over", np.nextafter(c, F32(1)))):
        r = runs["max_iou_distance", tag]
        assert r["params"]["max_iou_distance"] == float(thr)
        assert r["frames"][1]["iou"].tobytes() == c.tobytes()
        assert len(r["frames"][1]["matches"]) == (0 if tag == "under" else 1)
    for tag, sign in (("inside", -1), ("outside", 1)):
        d2 = float(runs["gate", tag]["frames"][3]["gate"][0, 0])
        assert sign * (d2 / CHI2_2DOF - 1) >= 1e-3, (tag, d2)                   # > 100x the oracle's gating error (A.3)
        assert abs(d2 / CHI2_2DOF - 1) < 3e-3
        assert runs["gate", tag]["frames"][3]["cos"][0, 0] == 0.0
        assert len(runs["gate", tag]["frames"][3]["matches"]) == (1 if tag == "inside" else 0)
    for tag, cost in (("kept", 0.0), ("evicted", 1.0)):
        r = runs["ring", tag]
        assert r["params"]["nn_budget"] == 5 and len(r["frames"]) == 8
        assert r["frames"][7]["cos"].tobytes() == F32(cost).tobytes()
        assert len(r["frames"][7]["matches"]) == (1 if tag == "kept" else 0)
    assert runs["nms", "under"]["params"]["nms_max_overlap"] == float(np.nextafter(half, F32(0)))
    assert runs["nms", "on"]["params"]["nms_max_overlap"] == 0.5
    assert len(runs["nms", "under"]["frames"][0]["ids"]) == 1 and len(runs["nms", "on"]["frames"][0]["ids"]) == 2


def check_frame(fr, matches, um_t, um_d, st, where):
    assert np.array_equal(np.asarray(matches, np.int32).reshape(-1, 2), fr["matches"]), where
    assert np.array_equal(np.asarray(um_t, np.int32), fr["um_t"]), where
    assert np.array_equal(np.asarray(um_d, np.int32), fr["um_d"]), where
    for k in ("ids", "state", "tsu", "hits"):
        assert np.array_equal(np.asarray(st[k], np.int32), fr[k]), (where, k)


RUNS = sorted(k for k in threshold_runs())


def test_fixture_covers_every_threshold():
    check_fixture_conditions(threshold_runs())


@pytest.mark.parametrize("scene,run", [k for k in RUNS if k[0] != "nms"])
def test_tracker_takes_the_references_side(scene, run):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import _TrackerHandle
    _lib.init(0)
    r = threshold_runs()[scene, run]
    p = r["params"]
    trk = _TrackerHandle(p["max_dist"], p["max_iou_distance"], p["max_age"], p["n_init"], p["nn_budget"])
    for t, fr in enumerate(r["frames"]):
        payload = (np.arange(len(fr["tlwh"])) % 3 * 2).astype(F32)
        out, matches = trk.step(np.ascontiguousarray(fr["tlwh"]), feats_of(fr), payload, want_debug=True)
        um_t, um_d = trk.last_unmatched()
        st = trk.state()
        check_frame(fr, matches, um_t, um_d, st, (scene, run, t))
        check_int_rows(out, fr["out"], st, [0, 0])


@pytest.mark.parametrize("run", [k[1] for k in RUNS if k[0] == "nms"])
def test_tracker_side_nms_on_its_threshold(run):
    """DeepSort.update(nms_max_overlap): a pair whose inter / area is exactly 0.5 survives `> 0.5` and not `> prev(0.5)`."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import DeepSort
    from test_gpu_assoc import _keep_with_order
    _lib.init(0)
    r = threshold_runs()["nms", run]
    p = r["params"]
    state = {}
    ds = DeepSort(lambda crops: state["feats"], use_cuda=True, **p)
    frame = np.zeros((1080, 1920, 3), np.uint8)
    step = ds.tracker.step

    def step_with_matches(*a, **k):                            # DeepSort.update does not hand the debug match list on
        rows, state["matches"] = step(*a, **dict(k, want_debug=True))
        return rows
    ds.tracker.step = step_with_matches
    for t, fr in enumerate(r["frames"]):
        state["feats"] = feats_of(fr)
        ds._nms_keep = (lambda boxes, _o=fr["nms_order"]: _keep_with_order(ds, boxes, _o))
        n = len(fr["tlwh"])
        out = ds.update(np.ascontiguousarray(fr["tlwh"]), np.ones(n), frame, (np.arange(n) % 3 * 2).astype(F32))
        out = np.array(out, np.int32).reshape(-1, 6)
        um_t, um_d = ds.tracker.last_unmatched()
        st = ds.tracker.state()
        check_frame(fr, state["matches"], um_t, um_d, st, (run, t))
        check_int_rows(out, fr["out"], st, [0, 0])
