"""Scenes of the ground plane tests, shared by the host tests (test_ground_host.py asserts what each scene exercises on the host
definition's own statistics) and the device tests (test_gpu_ground.py compares csrc/ground.hip against that definition)."""
import functools
import math

import numpy as np

from yolo_deepsort_amd import ground as G

PLAN = dict(origin=(-10.0, 0.0), cell=0.5, gw=40, gh=30, scale=1000)


def pinhole_H(height=3.0, tilt_deg=15.0, f=80.0, cx=48.0, cy=32.0):
    """Image to plan for a pinhole `height` units above the plan at the plan's origin, looking along +Y, tilted down by tilt_deg:
    a ray through pixel (u, v) meets the plan at X / W, Y / W with the rows below (the horizon is v = cy - f tan(tilt))."""
    t = math.radians(tilt_deg)
    return np.array([[height, 0.0, -height * cx],
                     [0.0, -height * math.sin(t), height * (f * math.cos(t) + cy * math.sin(t))],
                     [0.0, math.cos(t), f * math.sin(t) - cy * math.cos(t)]])


def reference_spec(class_id=0):
    """The reference camera of the issue: 3 units up, tilted 15 degrees, f = 80 px, principal point (48, 32), frames of 64 x 96; a
    40 x 30 grid of 0.5-unit cells at origin (-10, 0), scale 1000."""
    return G.GroundSpec(pinhole_H(), class_id=class_id, **PLAN)


def scene_specs():
    """Three cameras with different H on the one 40 x 30 plan: a fine pinhole that counts every class, the same optics turned by 90
    degrees about (0, 7) and moved (class 0), and a top-down scale-and-shift camera (class 1)."""
    H0 = pinhole_H(f=800.0, cx=480.0, cy=320.0)
    turn = np.array([[0.0, -1.0, 9.0], [1.0, 0.0, 5.0], [0.0, 0.0, 1.0]])     # plan to plan
    H1 = turn @ pinhole_H(height=4.0, tilt_deg=25.0, f=600.0, cx=400.0, cy=300.0)
    H2 = np.array([[0.02, 0.0, -11.0], [0.0, 0.02, -1.0], [0.0, 0.0, 1.0]])
    return [G.GroundSpec(H0, class_id=-1, **PLAN), G.GroundSpec(H1, class_id=0, **PLAN), G.GroundSpec(H2, class_id=1, **PLAN)]


@functools.lru_cache(maxsize=None)
def plan_scene(seed=3, n_ids=300, n_frames=40):
    """[(stream, rows int32 [m, 6], t), ...], frame-major, for the cameras of scene_specs(): n_ids people of class i % 3 walk on the
    plan in [-12, 12) x [-2, 17) (some outside the grid), velocity redrawn every 6 frames and reflected at those borders; per camera
    a person is missed with probability 0.12 and now and then hides for 2..6 frames; a visible person's plan point goes through the
    camera's inverse H to integer pixels (dropped where it lies behind the camera), 4 % of the pinhole cameras' rows are lifted above
    the horizon instead (off plane); the rows are shuffled; camera s sees frame k at 0.04 k + 0.001 s."""
    rs = np.random.RandomState(seed)
    specs = scene_specs()
    inv = [np.linalg.inv(sp.H) for sp in specs]
    lo, hi = np.array([-12.0, -2.0]), np.array([12.0, 17.0])
    pos = lo + rs.rand(n_ids, 2) * (hi - lo)
    vel = np.zeros((n_ids, 2))
    hidden = np.zeros((3, n_ids), np.int64)
    ids, cls = np.arange(1, n_ids + 1), np.arange(n_ids) % 3
    frames = []
    for k in range(n_frames):
        if k % 6 == 0:
            vel = rs.uniform(-0.15, 0.15, (n_ids, 2))
        pos = pos + vel
        low, high = pos < lo, pos >= hi
        pos = np.where(low, 2 * lo - pos, np.where(high, 2 * hi - pos - 1e-9, pos))
        vel = np.where(low | high, -vel, vel)
        for s in range(3):
            hidden[s] = np.where((hidden[s] == 0) & (rs.rand(n_ids) < 0.04), rs.randint(2, 7, n_ids), np.maximum(hidden[s] - 1, 0))
            seen = np.flatnonzero((hidden[s] == 0) & (rs.rand(n_ids) < 0.88))
            rs.shuffle(seen)
            p = (inv[s] @ np.c_[pos[seen], np.ones(len(seen))].T).T
            ok = p[:, 2] > 1e-6
            seen, p = seen[ok], p[ok]
            u, v = np.rint(p[:, 0] / p[:, 2]).astype(np.int64), np.rint(p[:, 1] / p[:, 2]).astype(np.int64)
            if s < 2:                                                  # above the horizon: no plan point
                sky = rs.rand(len(seen)) < 0.04
                v = np.where(sky, -5 - rs.randint(0, 40, len(seen)), v)
            rows = np.stack([u - 4, v - 30, u + 4 + ids[seen] % 2, v, ids[seen], cls[seen]], 1).astype(np.int32)
            frames.append((s, rows, 0.04 * k + 0.001 * s))
    return frames


def burst_scene():
    """700 rows from two top-down cameras (different scale-and-shift H) on ONE cell in one call - 400 from camera 0, 300 from camera 1,
    every id a frame apart twice - then all gone: (specs, frames)."""
    Ha = np.array([[0.01, 0.0, -0.2], [0.0, 0.01, 5.0], [0.0, 0.0, 1.0]])
    Hb = np.array([[0.0, 0.02, -0.45], [-0.02, 0.0, 5.45], [0.0, 0.0, 1.0]])
    specs = [G.GroundSpec(Ha, class_id=-1, **PLAN), G.GroundSpec(Hb, class_id=-1, **PLAN)]
    a = [[20 + i % 9 - 3, 0, 20 + i % 9 + 3, 20 + i % 7, i + 1, 0] for i in range(400)]            # plan (0.0 .. 0.1, 5.2 .. 5.3)
    b = [[10 + i % 4 - 3, 0, 10 + i % 4 + 3, 23 + i % 5, i + 1, 1] for i in range(300)]            # plan (0.01 .. 0.1, 5.19 .. 5.25)
    frames = [(0, a, 0.0), (1, b, 0.0), (0, a[::-1], 0.5), (1, b[::-1], 0.5), (0, [], 1.0), (1, [], 1.0), (0, [], 1.5), (1, [], 1.5),
              (0, a[:3], 2.0)]
    return specs, frames


def division_cases(seed=11, n_h=64, per_h=64):
    """The division pin: n_h matrices with per_h foot points each on a plan of scale 1024 - (specs, [(stream, row, expected on-plane
    or None: not stated)]), every frame one row.  The first streams carry one hand-made edge each (|p * scale| exactly 2^29 and one ulp
    either side, W == 0, W < 0, W tiny, an overflow to infinity in X and in W); the others are seeded perspective matrices, and every
    stream is filled up with seeded points on both sides of its horizon."""
    plan = dict(origin=(0.0, 0.0), cell=0.5, gw=40, gh=30, scale=1024)
    rs = np.random.RandomState(seed)
    up, down = float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0))
    eye = np.eye(3)

    def with_(**kw):
        H = eye.copy()
        for k, v in kw.items():
            H[int(k[1]), int(k[2])] = v
        return H
    edges = [(eye, 1 << 19, 10, True), (with_(h00=up), 1 << 19, 10, False), (with_(h00=down), 1 << 19, 10, True),
             (with_(h11=up), 10, 1 << 19, False), (with_(h00=-1.0), 1 << 19, 10, True), (with_(h00=-up), 1 << 19, 10, False),
             (with_(h21=0.001, h22=-0.2), 50, 200, None), (with_(h21=0.001, h22=-0.2), 50, 199, False),
             (with_(h21=0.001, h22=-0.2), 50, 201, None), (with_(h22=-1.0), 7, 9, False), (with_(h22=0.0), 7, 9, False),
             (with_(h22=1e-300), 7, 9, False), (with_(h00=1e308), 1000, 9, False), (with_(h21=1e308, h22=1e308), 7, 100, False),
             (with_(h22=4.0), 2001, 3, True), (with_(h22=3.0), 1, 1, True)]
    specs, cases = [], []
    for h, (H, u, v, want) in enumerate(edges):
        specs.append(G.GroundSpec(H, class_id=-1, **plan))
        cases.append((h, [u - 3, v - 20, u + 3, v, 1, 0], want))
    while len(specs) < n_h:
        H = np.array([[rs.uniform(0.005, 0.05), rs.uniform(-0.01, 0.01), rs.uniform(-5, 5)],
                      [rs.uniform(-0.01, 0.01), rs.uniform(0.005, 0.05), rs.uniform(-5, 5)],
                      [rs.uniform(-2e-3, 2e-3), rs.uniform(-2e-3, 2e-3), rs.uniform(-0.5, 1.0)]])
        specs.append(G.GroundSpec(H, class_id=-1, **plan))
    for h in range(n_h):
        k = sum(1 for c in cases if c[0] == h)
        for i in range(per_h - k):
            u, v = int(rs.randint(-200, 1200)), int(rs.randint(-200, 900))
            cases.append((h, [u - rs.randint(1, 9), v - 20, u + rs.randint(1, 9), v, 2 + i, 0], None))
    return specs, cases


SCENE_KW = dict(max_age=3, speed_window=4)


@functools.lru_cache(maxsize=None)
def host_scene():
    """plan_scene() through the host definition, once: (the map after the last frame, its layers and tables after the first half of
    the frames - the first of the two device calls -, the records of every frame).  Nobody changes what this returns."""
    frames = plan_scene()
    host = G.GroundMap(scene_specs(), **SCENE_KW)
    recs, mid = [], None
    for k, (s, rows, t) in enumerate(frames):
        recs.append(host.update(s, rows, t))
        if k + 1 == len(frames) // 2:
            mid = (host.layers(), [host.tracks(c) for c in range(3)])
    return host, mid, recs


@functools.lru_cache(maxsize=None)
def host_burst():
    specs, frames = burst_scene()
    host = G.GroundMap(specs, max_age=1, speed_window=8)
    return host, [host.update(s, rows, t) for s, rows, t in frames]
