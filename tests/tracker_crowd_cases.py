"""Scripted crowd scenes for tests/test_gpu_tracker_crowd.py and their reference, oracle.tracker.TrackerOracle, shared with the host
check tests/test_tracker_crowd_cases_host.py.  Plain helpers, no fixtures.

The fused association kernel (csrc/tracker.hip, trk_assoc_kernel) builds every list with ordered compactions of 256 entries per chunk
and picks the form of both assignment solves on the device (csrc/tracker_lsap_dev.h, lsap_form).  The scenes put track and detection
counts at 64/65 and 256/257, above one chunk, and at the sizes that select every solver form, while misses, deletions, new tracks and
stage-A leftovers happen in the same frames.

Geometry: persons stand on a grid whose spacing exceeds the box, so the IoU of different persons is 0, and every person has the same
box and the same non-integer offset and velocity.  The Kalman filter is then the same for everybody up to a whole-pixel translation, so
the fractional parts of the output corners take only a few values per frame (one per visibility history), and the offsets are chosen
so that none of them sits next to an integer: int32 truncation cannot flip (test_tracker_crowd_cases_host.py measures the share)."""
import contextlib
import functools

import numpy as np

F32 = np.float32
BOX_W, BOX_H = 30.0, 60.0
STEP_X, STEP_Y = 72, 66                      # grid spacing > box: no overlap, also under the IoU's +1 pixel convention; wide enough that
                                             # the growing covariance of a track coasting to the last frame keeps its neighbours outside the gate
OFFSET = (0.37, 0.41)
VELOCITY = (2.3, 1.1)
N_CROWD_FRAMES = 10

P_RING = dict(max_dist=0.3, nn_budget=2, n_init=3, max_iou_distance=0.7, max_age=2)          # the ring wraps, tracks expire
P_UNBOUNDED = dict(max_dist=0.3, nn_budget=None, n_init=3, max_iou_distance=0.7, max_age=30)
P_EUCLID = dict(P_RING, max_dist=1.0, metric="euclidean")    # same person ~0.41 (two noisy copies), different persons ~2.4

# name -> (script, script arguments, tracker parameters)
SCENES = {
    "crowd64_ring": ("crowd", (64,), P_RING),
    "crowd65_ring": ("crowd", (65,), P_RING),
    "crowd65_unbounded": ("crowd", (65,), P_UNBOUNDED),
    "crowd200_ring": ("crowd", (200,), P_RING),
    "crowd200_unbounded": ("crowd", (200,), P_UNBOUNDED),
    "crowd256_ring": ("crowd", (256,), P_RING),
    "crowd257_ring": ("crowd", (257,), P_RING),
    "crowd257_unbounded": ("crowd", (257,), P_UNBOUNDED),
    "crowd257_euclid": ("crowd", (257,), P_EUCLID),
    "crowd600_ring": ("crowd", (600,), P_RING),
    "crowd600_unbounded": ("crowd", (600,), P_UNBOUNDED),
    "collapse300x5": ("collapse", (300, 5), P_RING),
    "collapse3300x5": ("collapse", (3300, 5), P_RING),
    "collapse3300x12": ("collapse", (3300, 12), P_RING),
    # small streams of the unequal group
    "crowd5_ring": ("crowd", (5,), P_RING),
    "crowd30_ring": ("crowd", (30,), P_RING),
}
TRACE_SCENES = tuple(n for n in SCENES if n not in ("crowd5_ring", "crowd30_ring"))


def _grid(n):
    cols = max(1, int(np.ceil(np.sqrt(n * 1.2))))
    p = np.arange(n)
    return 40.0 + STEP_X * (p % cols), 50.0 + STEP_Y * (p // cols)


def _frames(n, visible_of, n_frames, seed):
    """[(person ids, tlwh [D,4], features [D,512], payload [D])] per frame; detections in person order."""
    rng = np.random.RandomState(seed)
    gx, gy = _grid(n)
    base = rng.randn(n, 512)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    out = []
    for t in range(n_frames):
        feats = (base + 0.02 * rng.randn(n, 512)).astype(F32)
        p = np.asarray(visible_of(t), dtype=np.int64)
        tlwh = np.stack([gx[p] + OFFSET[0] + VELOCITY[0] * t, gy[p] + OFFSET[1] + VELOCITY[1] * t,
                         np.full(len(p), BOX_W), np.full(len(p), BOX_H)], 1).astype(F32).reshape(-1, 4)
        out.append((p, tlwh, np.ascontiguousarray(feats[p]).reshape(-1, 512), (p % 3 * 2).astype(F32)))
    return out


def crowd_frames(n, seed=11):
    """Ten frames.  Odd persons are absent when (p + t) % 5 == 0 (misses while tentative: deleted and re-created; coasting confirmed
    tracks; re-acquisition by appearance); persons with p % 11 == 3 arrive at frame 4 (new tracks in the frames of the misses); persons
    with p % 13 == 5 leave for good at frame 5 (they expire under max_age=2)."""
    p = np.arange(n)

    def visible(t):
        v = ~((p % 2 == 1) & ((p + t) % 5 == 0))
        v &= ~((p % 11 == 3) & (t < 4))
        v &= ~((p % 13 == 5) & (t >= 5))
        return p[v]
    return _frames(n, visible, N_CROWD_FRAMES, seed + n)


def collapse_frames(n, k, seed=23):
    """Frame 0: n detections; frames 1-4: the same k of them (spread over the list, so the survivors of the mass deletion come from
    several chunks) - they become confirmed; frames 5 and 6: n again, so stage A is k confirmed x n and stage B is wide."""
    keep = (np.arange(k) * n) // k + 7
    return _frames(n, lambda t: np.arange(n) if t in (0, 5, 6) else keep, 7, seed + n + k)


def scene_frames(name):
    script, args, _ = SCENES[name]
    return crowd_frames(*args) if script == "crowd" else collapse_frames(*args)


# ------------------------------------------------------------------------------------------ the form rule, restated
LDS_BYTES = 150 * 1024            # dynamic LDS of the fused kernel
FORM_NAMES = {0: "empty", 1: "wave/lds", 2: "wave/global", 3: "reg/lds", 4: "reg/global", 5: "lds-state/lds", 6: "lds-state/global",
              7: "global-state/lds", 8: "global-state/global"}
REACHABLE_FORMS = frozenset((1, 3, 4, 5, 6, 7, 8))     # (a 64 x 64 cost matrix always fits beside the wave form's state: 2 never runs)
NEW_FORMS = frozenset((4, 5, 7, 8))                    # not run in the fused kernel by any earlier test


def fused_form(nr, nc):
    """Python restatement of the table the fused kernel chooses its solver form by (the numbers yds_lsap_fused_form returns)."""
    if nr <= 0 or nc <= 0:
        return 0
    n = max(nr, nc)
    if n <= 64:
        return 1 if 64 * 44 + 4 * nr * nc <= LDS_BYTES else 2
    if n <= 256:
        return 3 if nr * nc <= 35584 else 4
    if n <= 3200:
        return 5 if 48 * n + 4 * nr * nc <= LDS_BYTES else 6
    return 7 if nr * nc <= 38400 else 8


# ------------------------------------------------------------------------------------------ the reference
GALLERY_POSITIONS = (0, 255, 256, 257, -1)


def _normalised(f):
    f = np.asarray(f, dtype=F32)
    return (f / np.sqrt((f * f).sum(-1, keepdims=True, dtype=F32))).astype(F32)


@contextlib.contextmanager
def perturbed_matching(seed):
    """min_cost_matching's input multiplied entrywise by 1 + k * 2^-23, k uniform in [-4, 4] (seed None: unchanged)."""
    from oracle import tracker as otrk
    if seed is None:
        yield
        return
    rng = np.random.RandomState(seed)
    orig = otrk.min_cost_matching

    def wrapped(cost, max_distance, track_indices, detection_indices):
        k = rng.uniform(-4.0, 4.0, cost.shape)
        return orig((cost.astype(np.float64) * (1.0 + k * 2.0 ** -23)).astype(F32), max_distance, track_indices, detection_indices)
    otrk.min_cost_matching = wrapped
    try:
        yield
    finally:
        otrk.min_cost_matching = orig


def _min_abs(a, thr):
    a = np.asarray(a, dtype=np.float64)
    return float(np.abs(a - thr).min()) if a.size else float("inf")


def oracle_run(name, perturb_seed=None, skip=()):
    """The scene through TrackerOracle: one record per frame with everything the tests compare (None for a frame in `skip`: the
    tracker is not called for it)."""
    from oracle import tracker as otrk
    _, _, params = SCENES[name]
    ora = otrk.TrackerOracle(**params)
    budget, cosine = params["nn_budget"], params.get("metric", "cosine") == "cosine"
    recs = []
    with perturbed_matching(perturb_seed):
        for frame, (ids, tlwh, feats, payload) in enumerate(scene_frames(name)):
            if frame in skip:
                recs.append(None)
                continue
            tc = sum(1 for t in ora.tracks if t.state == otrk.CONFIRMED)
            want = np.array(ora.update(tlwh, feats, payload), dtype=np.int32).reshape(-1, 6)
            dbg, st = ora.debug, ora.state()
            rec = dict(out=want, matches=np.array(dbg["matches"], np.int32).reshape(-1, 2),
                       um_t=np.array(dbg["unmatched_tracks"], np.int32), um_d=np.array(dbg["unmatched_detections"], np.int32),
                       ids=np.array(st["ids"], np.int32), state=np.array(st["state"], np.int32), tsu=np.array(st["tsu"], np.int32),
                       hits=np.array(st["hits"], np.int32), mean=st["mean"], cov=st["cov"],
                       dims_a=(tc, len(ids)), dims_b=dbg["cost_b_raw"].shape if "cost_b_raw" in dbg else None)
            assert "cost_a_raw" not in dbg or dbg["cost_a_raw"].shape == rec["dims_a"]
            rec["margin_a"] = _min_abs(dbg.get("cost_a_raw", ()), float(F32(params["max_dist"])))
            rec["margin_gate"] = _min_abs(np.asarray(dbg.get("gate", ()), np.float64) / otrk.CHI2_2DOF, 1.0)
            rec["margin_b"] = _min_abs(dbg.get("cost_b_raw", ()), float(F32(params["max_iou_distance"])))
            # output corners before the int32 truncation (deep_sort.py:73-87), in the oracle's fp32 order
            shown = [t for t in ora.tracks if t.state == otrk.CONFIRMED and t.tsu <= 1]
            fl = np.zeros((len(shown), 4), F32)
            for i, t in enumerate(shown):
                b = t.mean[0, :4].copy()
                b[2] *= b[3]
                b[:2] -= b[2:] / F32(2)
                b[2:] += b[:2]
                b[:2] = np.maximum(b[:2], F32(0))
                fl[i] = b
            rec["out_float"] = fl
            # what the galleries of a few tracks must hold: the features in arrival order, the last `budget` of them
            gal = {}
            n = len(ora.tracks)
            for pos in GALLERY_POSITIONS:
                pos = n - 1 if pos < 0 else pos
                if 0 <= pos < n:
                    t = ora.tracks[pos]
                    held = list(ora.samples.get(t.track_id, [])) + list(t.features)
                    if budget is not None:
                        held = held[-budget:]
                    rows = np.stack(held, 0).astype(F32)
                    gal[pos] = _normalised(rows) if cosine else rows
            rec["gallery"] = gal
            recs.append(rec)
    return recs


@functools.lru_cache(maxsize=None)
def reference(name, skip=()):
    """oracle_run(name, skip=skip), unperturbed; computed once per process, read-only"""
    return tuple(oracle_run(name, skip=skip))


def forms_of(recs, form=fused_form):
    """({forms of stage A}, {forms of stage B}) over the frames of a run"""
    a = {form(*r["dims_a"]) for r in recs}
    b = {form(*r["dims_b"]) for r in recs if r["dims_b"] is not None}
    return a - {0}, b - {0}
