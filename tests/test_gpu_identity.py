"""Cross-camera identities on the device (csrc/identity.hip, yolo_deepsort_amd/identity.py) against tests/identity_ref.py.

Trackers are scripted without a detector, like tests/test_gpu_gallery_search.py: static, well separated boxes, one seeded unit vector
per person plus a gaussian vector of expected norm 0.05, so same-person distances are about 3e-3 and different-person distances
about 1 against max_dist = 0.3.  After EVERY update the device map must equal the oracle's map (identity_ref.update over the
exported state, slots and gallery rows and the previous map), and every linked cost must lie within BOUND of the oracle's float64
cost.  BOUND = 3.2e-5 is the search tests' derived bound (unit vectors, a 512-term fp32 fma chain: gamma_512 = 512 * 2^-24 ~ 3.05e-5
on sum |a b| <= 1); the rows on both sides are the stored rows, so no normalisation term is added.  The oracle itself asserts that
no decision of a scenario is marginal (1e-3)."""
import ctypes as C

import numpy as np
import pytest

import identity_ref as R
from yolo_deepsort_amd import cfgs, synth

pytestmark = pytest.mark.gpu
BOUND = 3.2e-5
EMB = 512
MAXD = 0.3


# ------------------------------------------------------------------------------------------------ helpers
def _centre(seed):
    v = np.random.RandomState(5000 + seed).randn(EMB)
    return v / np.linalg.norm(v)


def _box(i):
    return np.array([40 + 220 * (i % 8), 40 + 300 * (i // 8), 64, 128], np.float32)


def _tracker(**kw):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import _TrackerHandle
    _lib.init(0)
    p = dict(max_dist=MAXD, max_iou_distance=0.7, max_age=30, n_init=3, nn_budget=40)
    p.update(kw)
    return _TrackerHandle(**p)


class _Cam:
    """A tracker fed by a script: step({box index: centre}) shows each centre (plus this camera's own noise) at its box."""

    def __init__(self, seed, noise=0.05, **kw):
        self.trk, self.rng, self.noise = _tracker(**kw), np.random.RandomState(seed), noise
        self.tracker = self.trk                                  # (IdentityMap takes DeepSort-like objects or handles)

    def step(self, shown=None):
        shown = shown or {}
        ks = sorted(shown)
        feats = np.stack([(3.0 * (np.asarray(shown[k]) + self.noise * self.rng.randn(EMB) / np.sqrt(EMB))).astype(np.float32) for k in ks]) \
            if ks else np.zeros((0, EMB), np.float32)
        boxes = np.stack([_box(k) for k in ks]) if ks else np.zeros((0, 4), np.float32)
        return self.trk.step(boxes, feats, np.zeros(len(ks), np.float32))


def _twice(*shows):
    """n_init = 1: a track is Tentative in the frame that starts it and Confirmed at its next hit, so every look takes two frames"""
    for _ in range(2):
        for cam, shown in shows:
            cam.step(shown)


def _slots(trk):
    from yolo_deepsort_amd import _lib
    n = len(trk.state()["ids"])
    s = np.zeros(max(n, 1), np.int32)
    _lib.check(_lib.load().yds_tracker_get_slots(trk._h, _lib.ptr(s), max(n, 1)))
    return s[:n].tolist()


def _export(trackers):
    out = []
    for t in trackers:
        st = t.state()
        out.append(R.Cam(st["ids"], st["state"], _slots(t), [t.gallery(i) for i in range(len(st["ids"]))]))
    return out


class _Pair:
    """The device map and the oracle's, advanced together and compared after every update."""

    def __init__(self, cams, max_dist=None, max_rows=4096, device_costs=False):
        from yolo_deepsort_amd.identity import IdentityMap
        self.trackers = [getattr(c, "trk", c) for c in cams]
        self.im = IdentityMap(self.trackers, max_dist=max_dist, max_rows=max_rows)
        self.st = R.IdentityState(len(cams))
        self.max_dist, self.max_rows, self.device_costs = self.im.max_dist, max_rows, device_costs

    def compare(self, got_counts, ids, links):
        """the oracle over the exported state against what the device reported"""
        dc = {(s, t, g): c for s, t, g, c in links} if self.device_costs else None
        want = R.update(self.st, _export(self.trackers), self.max_dist, self.max_rows, device_costs=dc)
        assert ids == want["ids"], (ids, want["ids"])
        assert got_counts == (want["linked"], want["fresh"], want["deferred"]), (got_counts, want)
        assert [l[:3] for l in links] == [l[:3] for l in want["links"]]
        for g, w in zip(links, want["links"]):
            print("link", g, "oracle cost %.9g" % w[3])
            assert abs(float(g[3]) - w[3]) <= BOUND, (g, w)
        return want

    def update(self):
        got = self.im.update()
        assert got == self.im.last_counts()
        ids = [self.im.ids(s) for s in range(len(self.trackers))]
        return ids, self.compare(got, ids, self.im.last_links())


# ------------------------------------------------------------------------------------------------ 1. hand-over
def test_hand_over_and_an_unrelated_person():
    A, B = _centre(1), _centre(2)
    c0, c1 = _Cam(11), _Cam(12)
    p = _Pair([c0, c1])
    seen = []
    for t in range(10):
        c0.step({0: A})
        c1.step({1: B, **({0: A} if t >= 5 else {})})
        ids, want = p.update()
        seen.append(ids)
        states = [dict(zip(c.trk.state()["ids"].tolist(), c.trk.state()["state"].tolist())) for c in (c0, c1)]
        for s in range(2):                                      # Tentative tracks never appear in the map
            assert set(ids[s]) == {i for i, st in states[s].items() if st == 2}
    assert seen[1] == [{}, {}] and seen[2] == [{1: 1}, {1: 2}]                  # confirmed at the third hit: A fresh, B fresh
    assert seen[6] == [{1: 1}, {1: 2}]                                         # A is Tentative in camera 1: not in the map
    assert seen[7] == [{1: 1}, {1: 2, 2: 1}] and seen[9] == seen[7]             # confirmed: it takes camera 0's id
    assert p.im.last_links() == []                                              # (the last update had nothing to do)


# ------------------------------------------------------------------------------------------------ 2. simultaneous confirmation
def test_simultaneous_confirmation_in_three_cameras():
    A = _centre(3)
    cams = [_Cam(21), _Cam(22), _Cam(23)]
    p = _Pair(cams)
    for t in range(3):
        for c in cams:
            c.step({0: A})
    ids, want = p.update()
    assert ids == [{1: 1}, {1: 1}, {1: 1}] and (want["linked"], want["fresh"]) == (2, 1)
    assert [l[:3] for l in p.im.last_links()] == [(1, 1, 1), (2, 1, 1)]


# ------------------------------------------------------------------------------------------------ 3. one id per camera
def test_twins_one_id_per_camera():
    A = _centre(4)
    u = _centre(40)
    twin = (A + 0.3 * u) / np.linalg.norm(A + 0.3 * u)          # d ~ 0.04 to A: resembles the holder, clearly dearer than A itself
    c0, c1 = _Cam(31, n_init=1), _Cam(32, n_init=1)
    p = _Pair([c0, c1])
    _twice((c0, {0: A}))
    assert p.update()[0] == [{1: 1}, {}]
    _twice((c0, {0: A}), (c1, {0: twin, 1: A}))
    ids, want = p.update()
    assert want["costs"][1].shape == (2, 1) and want["costs"][1][1, 0] < want["costs"][1][0, 0] < MAXD
    assert ids == [{1: 1}, {1: 2, 2: 1}]                        # the cheaper one is linked, the other takes a fresh id
    _twice((c0, {0: A}), (c1, {0: twin, 1: A, 2: A}))
    ids, want = p.update()
    assert want["costs"][1].shape == (1, 0)                     # id 1 is held in camera 1, id 2 only there: nothing is offered
    assert ids == [{1: 1}, {1: 2, 2: 1, 3: 3}]


# ------------------------------------------------------------------------------------------------ 4. LSAP, not greedy
def test_assignment_is_the_lsap_not_greedy():
    gram = np.array([[1, .8, .90, .89], [.8, 1, .88, .75], [.90, .88, 1, .85], [.89, .75, .85, 1]])
    L = np.zeros((4, EMB))
    L[:, :4] = np.linalg.cholesky(gram)
    c0, c1 = _Cam(41, noise=0.0, n_init=1), _Cam(42, noise=0.0, n_init=1)
    p = _Pair([c0, c1])
    _twice((c0, {0: L[0], 1: L[1]}))
    assert p.update()[0] == [{1: 1, 2: 2}, {}]
    _twice((c1, {0: L[2], 1: L[3]}))
    ids, want = p.update()
    np.testing.assert_allclose(want["costs"][1], [[.10, .12], [.11, .25]], atol=1e-6)
    assert ids[1] == {1: 2, 2: 1}                               # total 0.23; the smallest entry first would give 0.35
    assert sorted(round(float(l[3]), 4) for l in p.im.last_links()) == [0.11, 0.12]


# ------------------------------------------------------------------------------------------------ 5. several holders
def test_cost_is_the_minimum_over_the_holders():
    A = _centre(5)
    cams = [_Cam(51, n_init=1), _Cam(52, n_init=1), _Cam(53, n_init=1)]
    p = _Pair(cams)
    for _ in range(4):
        cams[0].step({0: A})
        cams[1].step({0: A})
    assert p.update()[0] == [{1: 1}, {1: 1}, {}]
    _twice((cams[2], {0: A}))
    ids, want = p.update()
    assert ids == [{1: 1}, {1: 1}, {1: 1}]
    ex = _export(p.trackers)
    d0, d1 = (R.track_distance(ex[2].rows[0], ex[s].rows[0]) for s in (0, 1))
    assert abs(d0 - d1) > 1e-6                                  # (different noise: the minimum means something)
    (s, t, g, c), = p.im.last_links()
    assert (s, t, g) == (2, 1, 1) and abs(float(c) - min(d0, d1)) <= BOUND


# ------------------------------------------------------------------------------------------------ 6. threshold
def _threshold_run(max_dist):
    A = _centre(6)
    c0, c1 = _Cam(61, n_init=1), _Cam(62, n_init=1)
    p = _Pair([c0, c1], max_dist=max_dist, device_costs=max_dist is not None)
    _twice((c0, {0: A}))
    p.update()
    _twice((c1, {0: A}))
    ids, _ = p.update()
    return ids, p.im.last_links()


def test_link_threshold_at_the_bit():
    """As tests/test_gpu_assoc_thresholds.py: the device's own fp32 cost c as the threshold links (cost > max_dist is false), the
    next fp32 below c does not.  The oracle is fed the device's cost for that entry (the one exception to its margins)."""
    ids, links = _threshold_run(None)
    assert ids == [{1: 1}, {1: 1}]
    c = np.float32(links[0][3])
    assert 0 < c < 0.05
    ids, links = _threshold_run(float(c))
    assert ids == [{1: 1}, {1: 1}] and np.float32(links[0][3]) == c
    below = np.nextafter(c, np.float32(0))
    A = _centre(6)
    c0, c1 = _Cam(61, n_init=1), _Cam(62, n_init=1)
    p = _Pair([c0, c1], max_dist=float(below))
    _twice((c0, {0: A}))
    p.im.update()
    _twice((c1, {0: A}))
    assert p.im.update() == (0, 1, 0) and [p.im.ids(0), p.im.ids(1)] == [{1: 1}, {1: 2}] and p.im.last_links() == []
    # (the oracle with the device's cost at that entry decides the same)
    assert R.min_cost_matching([[float(c)]], float(below), check_margin=False) == {}


# ------------------------------------------------------------------------------------------------ 7. slot reuse and expiry
def test_slot_reuse_does_not_inherit_and_dead_ids_are_never_offered():
    A, B = _centre(7), _centre(8)
    c0, c1 = _Cam(71, n_init=1, max_age=2), _Cam(72, n_init=1, max_age=2)
    p = _Pair([c0, c1])
    c0.step({0: A})
    c0.step({0: A})
    assert p.update()[0] == [{1: 1}, {}]
    old_slot = _slots(c0.trk)[0]
    for _ in range(3):                                          # three misses with max_age = 2: the holder dies
        c0.step({})
        p.update()
    assert len(c0.trk.state()["ids"]) == 0
    c0.step({1: B})
    assert c0.trk.state()["ids"].tolist() == [2] and _slots(c0.trk) == [old_slot]      # a later track took the slot
    assert p.update()[0] == [{}, {}]                            # (Tentative)
    c0.step({1: B})
    c1.step({0: A})                                             # A again, in camera 1, after its last holder's death
    ids, _ = p.update()
    assert ids == [{2: 2}, {}]                                  # ... and did not inherit id 1
    c0.step({1: B})
    c1.step({0: A})
    ids, want = p.update()
    assert ids == [{2: 2}, {1: 3}] and want["linked"] == 0     # id 1 is never handed out again; fresh ids keep increasing
    p.im.reset()
    p.st.reset()
    ids, _ = p.update()
    assert ids == [{2: 4}, {1: 5}]                              # reset forgets the pairs, the counter keeps counting


# ------------------------------------------------------------------------------------------------ 8. deferral
def test_deferral_by_max_rows():
    A, B = _centre(9), _centre(10)
    c0, c1 = _Cam(81, n_init=1, nn_budget=40), _Cam(82, n_init=1, nn_budget=40)
    p = _Pair([c0, c1], max_rows=64)
    for t in range(45):
        c0.step({0: A, **({1: B} if t >= 25 else {})})
        c1.step({0: A} if t >= 15 else {})
    assert [[len(r) for r in cam.rows] for cam in _export(p.trackers)] == [[40, 20], [30]]
    ids, want = p.update()
    assert ids == [{1: 1, 2: 2}, {1: 0}] and (want["linked"], want["fresh"], want["deferred"]) == (0, 2, 1)
    ids, want = p.update()                                      # the deferred track is resolved against the ids of the first
    assert ids == [{1: 1, 2: 2}, {1: 1}] and (want["linked"], want["fresh"], want["deferred"]) == (1, 0, 0)


# ------------------------------------------------------------------------------------------------ 9. empty edges
def test_empty_edges():
    A = _centre(11)
    cams = [_Cam(91, n_init=1), _Cam(92, n_init=1), _Cam(93, n_init=1)]
    p = _Pair(cams)
    p.im.set_timing(True)
    ids, want = p.update()                                      # no tracker has tracks
    assert ids == [{}, {}, {}] and p.im.last_counts() == (0, 0, 0) and p.im.last_us() is None
    _twice((cams[0], {0: A}), (cams[2], {0: A}))                # a tracker without tracks between two that have some
    ids, want = p.update()
    assert ids == [{1: 1}, {}, {1: 1}] and want["linked"] == 1
    us = p.im.last_us()
    print("resolve sequence, 2 new tracks: %.1f us" % us)
    assert us is not None and us > 0
    ids, want = p.update()                                      # nothing new: no resolve launch
    assert ids == [{1: 1}, {}, {1: 1}] and p.im.last_counts() == (0, 0, 0) and p.im.last_us() is None


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals():
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.identity import IdentityMap
    lib = _lib.load()
    a, b = _tracker(), _tracker(nn_budget=100)
    eu, nb = _tracker(metric="euclidean"), _tracker(nn_budget=None)
    for trks, rows, word in (([a, eu], 4096, "euclidean"), ([a, nb], 4096, "nn_budget=None"), ([a, b, a], 4096, "more than one stream"),
                             ([a, b], 99, "max_rows")):
        with pytest.raises(ValueError, match=word):
            IdentityMap(trks, max_rows=rows)
    # the library refuses the same by itself, before any launch
    for trks, rows, word in (([a, eu], 4096, "euclidean"), ([a, nb], 4096, "nn_budget=None"), ([a, b, a], 4096, "share one tracker"),
                             ([a, b], 99, "max_rows"), ([], 4096, "no trackers")):
        arr = (C.c_void_p * max(len(trks), 1))(*[t._h for t in trks])
        assert not lib.yds_identity_create(arr, len(trks), 0.3, rows)
        assert word in _lib.last_error(), _lib.last_error()
    im = IdentityMap([a, b])
    assert im.max_dist == MAXD                                  # None = the first tracker's threshold
    t, g, n = np.zeros(1, np.int32), np.zeros(1, np.int32), C.c_int(0)
    assert lib.yds_identity_get(im.handle, 2, _lib.ptr(t), _lib.ptr(g), 1, C.byref(n)) != 0 and "stream 2" in _lib.last_error()
    cam = _Cam(95, n_init=1)
    _twice((cam, {0: _centre(12), 1: _centre(13)}))
    im2 = IdentityMap([cam])
    assert im2.update() == (0, 2, 0)
    assert lib.yds_identity_get(im2.handle, 0, _lib.ptr(t), _lib.ptr(g), 1, C.byref(n)) != 0 and n.value == 2 and "cap = 1" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ 11. inside the pipeline
PIPE_MAXD = 0.3


def test_identities_inside_the_pipeline():
    """yolov3-tiny 416 on 480x640 frames, three streams that all watch the same synthetic scene (so the cameras share persons),
    injected detections, steps in which a stream has no frame, one or several.  After each step the device map equals the oracle
    applied to the previous map and the exported state; the tracker rows and state of every step are bit-equal to the same run
    without identities; search / link return the same with the stage on; a map over other trackers is refused."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.deep_sort import DeepSort, Extractor
    from yolo_deepsort_amd.identity import IdentityMap
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=8, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0))
    ex = Extractor(synth.reid_state_dict(0), max_crops=256)
    ds_kw = dict(max_dist=PIPE_MAXD, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
    counts = [(1, 2, 0), (2, 1, 1), (1, 0, 2), (1, 2, 2), (2, 1, 1), (1, 1, 1), (2, 2, 2), (1, 1, 1)]
    scene = synth.PersonScene(5, frame_hw=(480, 640), seed=3, occlude_frac=0.0)
    heads = net.yolo_heads()
    n_frames = max(sum(c[s] for c in counts) for s in range(3))
    frames = [scene.frame(t) for t in range(n_frames)]
    injs = [synth.head_injection(scene.boxes(t)[1], (480, 640), (416, 416), heads) for t in range(n_frames)]
    steps, nxt = [], [0, 0, 0]
    for c in counts:
        st = []
        for s in range(3):
            st += [(s, nxt[s] + k) for k in range(c[s])]
            nxt[s] += c[s]
        steps.append(st)
    bm = net.batch_max
    empty = np.zeros((0, 9), np.float32)
    pl.load_injection_sets(net, [[injs[k] for _, k in st] + [empty] * (bm - len(st)) for st in steps])

    def run(with_ids):
        trackers = [DeepSort(ex, use_cuda=True, **ds_kw) for _ in range(3)]
        pipe = pl.MultiStreamPipeline(net, trackers, 0.5, 0.4)
        pair = None
        if with_ids:
            other = IdentityMap([DeepSort(ex, use_cuda=True, **ds_kw) for _ in range(3)])
            with pytest.raises(_lib.YdsError, match="not created over this pipeline"):
                pipe.set_identities(other)
            with pytest.raises(_lib.YdsError, match="not created over this pipeline"):
                pipe.set_identities(IdentityMap(trackers[::-1]))
            pair = _Pair([d.tracker for d in trackers])
            assert pipe.set_identities(pair.im) is pair.im
        else:
            assert pipe.last_identities() is None
        rows, states, found = [], [], []
        n_linked = 0
        for i, st in enumerate(steps):
            pl.select_injection_set(net, i)
            batch = np.ascontiguousarray(np.stack([frames[k] for _, k in st], 0))
            dev = _lib.DeviceBuffer.from_array(batch)
            outs = pipe.step(dev.ptr, 480, 640, [s for s, _ in st])
            rows.append(outs)
            states.append([d.tracker.state() for d in trackers])
            if with_ids:
                ids = pipe.last_identities()
                assert ids == [pair.im.ids(s) for s in range(3)] and ids[1] == pipe.last_identities(1)
                want = pair.compare(pair.im.last_counts(), ids, pair.im.last_links())
                n_linked += want["linked"]
            q = trackers[0].tracker.gallery(0)[:1] if len(states[-1][0]["ids"]) else None
            found.append((None if q is None else pipe.search(q, top_k=4),
                          pipe.link(0, int(states[-1][0]["ids"][0]), exclude_stream=0) if q is not None else None))
        if with_ids:
            assert n_linked >= 2
            final = pipe.last_identities()
            assert all(len(m) == 5 and 0 not in m.values() for m in final)
            assert sorted(final[0].values()) == sorted(final[1].values()) == sorted(final[2].values())     # five persons, five ids
            pipe.set_identities(None)
            assert pipe.last_identities() is None
        return rows, states, found
    rows, states, found = run(True)
    plain_rows, plain_states, plain_found = run(False)
    for i, st in enumerate(steps):
        for b in range(len(st)):
            a, p = rows[i][b], plain_rows[i][b]
            assert (a is None) == (p is None) and (a is None or (a.shape == p.shape and np.array_equal(a, p))), (i, b)
        for s in range(3):
            for key in ("ids", "state", "tsu", "hits", "mean", "cov"):
                assert np.array_equal(states[i][s][key], plain_states[i][s][key]), (i, s, key)
        assert found[i] == plain_found[i], i


# ------------------------------------------------------------------------------------------------ 12. VideoDetector.detect_streams
def test_detect_streams_global_ids(tmp_path):
    """Three cameras that show the SAME in-memory clip (a handful of random detections per frame), so every person is in all three:
    the yielded items are those of a run without global_ids; stream_identities() between the yields covers every track the rows
    show, defers nothing at this size, gives the three cameras the same map (camera 0 takes fresh ids - whatever holds an id
    elsewhere holds it there too - and cameras 1 and 2 are linked at distance ~0), never one id twice in a camera, and a track
    keeps its id for life.  Outside a running generator, and for one started without global_ids, it raises ValueError."""
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import DeepSort
    from yolo_deepsort_amd.detect import VideoDetector
    from yolo_deepsort_amd.models import Darknet
    _lib.init(0)
    cfg = cfgs.cfg_text("yolov3-tiny", 416, 416)
    net = Darknet(None, img_size=(416, 416), batch_max=4, cfg_text=cfg)
    net.load_darknet_weights(None, blob=synth.darknet_weights_blob(cfg, 0, -1.45))
    base = DeepSort(synth.reid_state_dict(0), use_cuda=True, max_dist=0.3, nn_budget=30, n_init=3, max_iou_distance=0.7, max_age=30)
    img = np.random.RandomState(21).randint(0, 256, (480, 640, 3)).astype(np.uint8)
    clip = [np.roll(img, 3 * t, axis=1) for t in range(12)]
    names = tmp_path / "coco.names"
    names.write_text(cfgs.coco_names_text())
    vd = VideoDetector(net, str(names), thres=0.5, nms_thres=0.4, tracker=base)
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_identities()
    plain = []
    for step in vd.detect_streams([clip] * 3, frames_per_stream=1, show_fps=False):
        with pytest.raises(ValueError, match="global_ids=True"):
            vd.stream_identities()
        plain.append(step)
    life, n_shown = [dict(), dict(), dict()], 0
    for k, step in enumerate(vd.detect_streams([clip] * 3, frames_per_stream=1, show_fps=False, global_ids=True)):
        ids = vd.stream_identities()
        assert ids == [vd.stream_identities(s) for s in range(3)]
        assert len(step) == len(plain[k]) == 3
        for (s, image, det, act), (ps, pimage, pdet, pact) in zip(step, plain[k]):
            assert s == ps and np.array_equal(image, pimage) and act == pact
            assert (det is None) == (pdet is None) and (det is None or np.array_equal(np.asarray(det), np.asarray(pdet)))
            shown = [] if det is None else [int(r[4]) for r in det]
            n_shown += len(shown)
            assert set(shown) <= set(ids[s]) and 0 not in ids[s].values()
            assert len(set(ids[s].values())) == len(ids[s])                                # one id per camera
            for t, g in ids[s].items():
                assert life[s].setdefault(t, g) == g                                        # for the track's life
        assert ids[0] == ids[1] == ids[2]
    assert n_shown > 0 and len(life[0]) > 0
    with pytest.raises(ValueError, match="between the yields"):
        vd.stream_identities()
