"""The host definition of the ground plane (yolo_deepsort_amd.ground): hand-computed rows, the homography fit, the ring, the
refusals, the view render's properties, the reference camera, and what the scenes of the device tests (ground_common.py) exercise -
asserted here on the host's own statistics so that no device comparison can pass vacuously."""
import math

import numpy as np
import pytest

import ground_common as gc
from yolo_deepsort_amd import ground as G, heatmap as H

# image (u, v) -> plan (u / 128 - 1, v / 64 + 0.5): every product below is exact in binary
SHIFT = np.array([[1 / 128, 0.0, -1.0], [0.0, 1 / 64, 0.5], [0.0, 0.0, 1.0]])


def small(class_id=0, **kw):
    return G.GroundMap(G.GroundSpec(SHIFT, origin=(0.0, 0.0), cell=0.5, gw=4, gh=4, scale=1000, class_id=class_id), **kw)


def foot(u, v, tid, cls=0):
    return [u - 6, v - 40, u + 6, v, tid, cls]


def test_hand_computed_rows_under_a_scale_and_shift():
    m = small(max_age=2, speed_window=8)
    # (256, 64) -> plan (1.0, 1.5) -> quanta (1000, 1500) -> cell (3, 2); a row of another class is ignored; (1024, 64) is outside
    r = m.update(0, [foot(256, 64, 7), foot(300, 64, 8, cls=2), foot(1024, 64, 9)], 0.0)
    assert r.dtype == np.int32 and r.tolist() == [[7, 0, 1000, 1500, 0, 0, -1, 14], [9, 0, 7000, 1500, 0, 0, -1, -1]]
    # half a second later (320, 64) -> (1500, 1500): 500 quanta in 500000 us = 1000 quanta / s along x; cell (3, 3)
    r = m.update(0, [foot(320, 64, 7)], 0.5)
    assert r.tolist() == [[7, 0, 1500, 1500, 1000, 0, 1000, 15]]
    # an odd x1 + x2 is a half pixel: u = 320.5 -> 1503.90625 -> 1504; a step of (4, -250) against the oldest point (1000, 1500) of 1 s
    # ago: vx = 504, vy = -250, speed = isqrt(504^2 + 250^2) = 562
    r = m.update(0, [[314, 0, 327, 48, 7, 0]], 1.0)
    assert r.tolist() == [[7, 0, 1504, 1250, 504, -250, 562, 11]]
    assert m.layer("presence").ravel().tolist() == [0] * 11 + [1, 0, 0, 1, 1] and m.layer("visits").sum() == 3
    assert m.layer("dwell_us")[3, 2] == 500000 and m.layer("dwell_us")[3, 3] == 500000 and m.layer("dwell_us").sum() == 10 ** 6
    assert m.layer("flow_x")[3, 3] == 500 and m.layer("flow_x")[2, 3] == 4 and m.layer("flow_y")[2, 3] == -250
    (tid, age, cell, travelled, t_last, ring), other = m.tracks(0)
    assert (tid, age, cell, travelled, t_last) == (7, 0, 11, 500 + math.isqrt(16 + 250 * 250), 1.0) and len(ring) == 3
    assert other[:4] == (9, 2, -1, 0) and m.stats["ignored_rows"] == 1 and m.stats["outside_rows"] == 1
    m.update(0, [], 1.5)
    assert [t[0] for t in m.tracks(0)] == [7]                                        # id 9 was unseen for more than max_age frames
    assert m.update(0, None, 2.0) is None and m.tracks(0)[0][1] == 1


def test_negative_velocities_floor_and_saturate():
    m = small(speed_window=2)
    m.update(0, [foot(320, 64, 1)], 0.0)
    assert m.update(0, [foot(256, 128, 1)], 0.3).tolist() == [[1, 0, 1000, 2500, -1667, 3333, 3726, -1]]      # floor(-500e6 / 300000) = -1667
    m.update(0, [foot(128 * 400000, 64, 2)], 1.0)
    assert m.update(0, [foot(0, 64, 2)], 1.000001).tolist() == [[2, 0, -1000, 1500, -G.SAT, 0, G.SAT, -1]]


def test_homography_from_points_recovers_a_perspective_matrix():
    H0 = gc.pinhole_H()
    img = np.array([[5.0, 14.0], [90.0, 13.0], [47.0, 30.0], [10.0, 60.0], [85.0, 55.0], [60.0, 40.0]])
    p = (H0 @ np.c_[img, np.ones(6)].T).T
    plan = p[:, :2] / p[:, 2:]
    got = G.homography_from_points(img, plan)
    a, b = got / np.linalg.norm(got), H0 / np.linalg.norm(H0)
    assert np.linalg.norm(a - b) <= 1e-9 * np.linalg.norm(b)
    assert ((got[2, 0] * img[:, 0] + got[2, 1] * img[:, 1] + got[2, 2]) > 0).all()
    # a point above the horizon (v = 5 < 10.56) with the plan point the same matrix gives it: W changes sign over the set
    sky = np.array([40.0, 5.0])
    ps = H0 @ np.array([40.0, 5.0, 1.0])
    assert ps[2] < 0
    with pytest.raises(ValueError, match="sign"):
        G.homography_from_points(np.vstack([img, sky]), np.vstack([plan, ps[:2] / ps[2]]))
    with pytest.raises(ValueError, match="n >= 4"):
        G.homography_from_points(img[:3], plan[:3])
    with pytest.raises(ValueError, match="degenerate"):
        G.homography_from_points([[0, 0], [1, 1], [2, 2], [3, 3]], [[0, 0], [1, 1], [2, 2], [3, 3]])


def test_ring_wraps_at_the_window():
    m = small(speed_window=3)
    recs = [m.update(0, [foot(256 + 64 * k, 64, 1)], 0.25 * k)[0].tolist() for k in range(5)]       # 500 quanta every 0.25 s
    assert [r[2] for r in recs] == [1000, 1500, 2000, 2500, 3000]
    assert [r[6] for r in recs] == [-1, 2000, 2000, 2000, 2000] and m.stats["ring_wraps"] == 2
    (_, _, _, travelled, _, ring), = m.tracks(0)
    assert travelled == 2000 and ring == ((2000, 1500, 0.5), (2500, 1500, 0.75), (3000, 1500, 1.0))
    # the speed spans the ring: a jump back to the start against the oldest point (2500, 0.75 s): -1500 quanta in 0.5 s
    assert m.update(0, [foot(256, 64, 1)], 1.25)[0].tolist() == [1, 0, 1000, 1500, -3000, 0, 3000, 14]
    one = small(speed_window=1)
    assert [one.update(0, [foot(256 + 64 * k, 64, 1)], 0.25 * k)[0, 6] for k in range(3)] == [-1, -1, -1]


def test_time_that_does_not_advance_gives_no_speed():
    m = small(speed_window=8)
    m.update(0, [foot(256, 64, 1)], 5.0)
    assert m.update(0, [foot(320, 64, 1)], 5.0)[0].tolist() == [1, 0, 1500, 1500, 0, 0, -1, 15]
    assert m.update(0, [foot(384, 64, 1)], 4.0)[0].tolist() == [1, 0, 2000, 1500, 0, 0, -1, -1]
    assert m.tracks(0)[0][3] == 1000 and m.layer("dwell_us").sum() == 0 and m.stats["no_speed"] == 3


def test_a_gap_restarts_the_ring_and_leaves_travelled_alone():
    m = small(max_age=5, speed_window=8)
    m.update(0, [foot(256, 64, 1)], 0.0)
    m.update(0, [foot(320, 64, 1)], 0.1)
    m.update(0, [], 0.2)
    before = m.layers()
    r = m.update(0, [foot(384, 96, 1)], 0.3)
    assert r[0].tolist() == [1, 0, 2000, 2000, 0, 0, -1, -1] and m.stats["gap_sightings"] == 1 and m.stats["restarts"] == 1
    (_, age, _, travelled, _, ring), = m.tracks(0)
    assert age == 0 and travelled == 500 and ring == ((2000, 2000, 0.3),)
    assert np.array_equal(m.layers(), before)                                        # neither dwell nor flow across the gap
    assert m.update(0, [foot(384, 64, 1)], 0.4)[0].tolist() == [1, 0, 2000, 1500, 0, -5000, 5000, -1] and m.tracks(0)[0][3] == 1000


def test_refused_specs():
    ok = dict(origin=(0.0, 0.0), cell=0.5, gw=4, gh=4, scale=1000)
    for kw, word in [(dict(cell=1 / 3), "cell"), (dict(origin=(0.0001, 0.0)), "origin x"), (dict(origin=(0.0, 0.12345)), "origin y"),
                     (dict(gw=257, gh=256), "exceeds 65536"), (dict(gw=0), "grid"), (dict(cell=5000.0), "2\\^22"), (dict(scale=0), "scale"),
                     (dict(class_id=-2), "class_id"), (dict(gw=2.5), "gw"), (dict(origin=(2e6, 0.0)), "origin")]:
        with pytest.raises(ValueError, match="ground: .*" + word):
            G.GroundSpec(SHIFT, **dict(ok, **kw))
    for bad in (np.eye(2), np.full((3, 3), np.nan), [[1, 0, 0], [0, 1, 0], [0, 0, np.inf]]):
        with pytest.raises(ValueError, match="ground: H"):
            G.GroundSpec(bad, **ok)
    a, b = G.GroundSpec(SHIFT, **ok), G.GroundSpec(SHIFT, **dict(ok, cell=0.25))
    with pytest.raises(ValueError, match="one plan"):
        G.GroundMap([a, b])
    with pytest.raises(ValueError, match="no stream"):
        G.GroundMap([None, None])
    with pytest.raises(ValueError, match="one GroundSpec"):
        G.GroundMap([a, "b"])
    for k in (0, 17, 2.5):
        with pytest.raises(ValueError, match="speed_window"):
            G.GroundMap(a, speed_window=k)
    with pytest.raises(ValueError, match="max_age"):
        G.GroundMap(a, max_age=0)
    with pytest.raises(ValueError, match="twice"):
        G.GroundMap(a).update(0, [foot(1, 1, 3), foot(2, 2, 3)], 0.0)
    skipped = G.GroundMap([a, None])
    assert skipped.update(1, [foot(256, 64, 1)], 0.0).shape == (0, 8) and not skipped.layers().any() and skipped.tracks(1) == []


def test_a_pixel_on_a_cell_centre_takes_that_cells_level():
    """Pixel (x, y) of a camera with H = diag(0.5, 0.5, 1) looks at the centre of cell (y, x) of a 0.5-unit grid: k is that cell's
    level // 257, whatever the neighbours hold; pixels more than half a cell beyond the grid keep the picture."""
    sp = G.GroundSpec(np.diag([0.5, 0.5, 1.0]), origin=(0.0, 0.0), cell=0.5, gw=6, gh=5, scale=1000)
    rs = np.random.RandomState(1)
    grid = rs.randint(0, 1000, (5, 6)).astype(np.int64)
    lv = H.levels(grid)
    k, on, near, qx, qy = G.view_field(sp, 7, 8, lv)
    assert on.all()
    assert np.array_equal(near, (np.arange(7)[:, None] < 5) & (np.arange(8)[None, :] < 6))
    assert np.array_equal(k[:5, :6], lv // 257) and not k[5:].any() and not k[:, 6:].any() and (k > 0).sum() >= 20
    img = rs.randint(0, 256, (7, 8, 3)).astype(np.uint8)
    out = G.render_view(img, sp, grid, alpha=256)
    assert np.array_equal(out[5:], img[5:]) and np.array_equal(out[:, 6:], img[:, 6:])
    assert np.array_equal(out[:5, :6][k[:5, :6] > 0], H.lut_heat()[k[:5, :6][k[:5, :6] > 0]])
    # half a cell outside still blends (the edge cell continued outwards), a full cell outside does not
    edge = G.GroundSpec(np.array([[0.5, 0, -0.5], [0, 0.5, -0.5], [0, 0, 1.0]]), origin=(0.0, 0.0), cell=0.5, gw=6, gh=5, scale=1000)
    k2, _, near2, _, _ = G.view_field(edge, 7, 8, np.full((5, 6), 65535))
    assert near2[0, 0] and k2[0, 0] == 255 and near2[5, 6] and not near2[6].any() and not near2[:, 7].any()
    far = G.GroundSpec(np.array([[0.5, 0, -1.0], [0, 0.5, -1.0], [0, 0, 1.0]]), origin=(0.0, 0.0), cell=0.5, gw=6, gh=5, scale=1000)
    k3, _, near3, _, _ = G.view_field(far, 7, 8, np.full((5, 6), 65535))
    assert not near3[0].any() and not near3[:, 0].any() and near3[1, 1] and not k3[0].any()


def test_reference_camera_counts():
    """The pinhole of the issue: 11 whole rows above the horizon, 5088 floor pixels, 3552 of them inside the grid over 446 cells, no
    point beyond the clamp; and the view render leaves the sky alone."""
    sp = gc.reference_spec()
    rs = np.random.RandomState(2)
    grid = rs.randint(0, 50, (30, 40)).astype(np.int64)
    k, on, near, qx, qy = G.view_field(sp, 64, 96, H.levels(grid))
    assert (~on).all(axis=1).sum() == 11 and not on[:11].any() and on[11:].all() and on.sum() == 5088
    cx, cy = (qx - sp.ox_q) // sp.cell_q, (qy - sp.oy_q) // sp.cell_q
    inside = on & (cx >= 0) & (cx < 40) & (cy >= 0) & (cy < 30)
    assert inside.sum() == 3552 and len(set((cy * 40 + cx)[inside].tolist())) == 446
    assert max(np.abs(qx[on]).max(), np.abs(qy[on]).max()) < G.Q_LIMIT
    assert inside.sum() <= near.sum() < on.sum()
    img = rs.randint(0, 256, (64, 96, 3)).astype(np.uint8)
    out = G.render_view(img, sp, grid)
    changed = (out != img).any(axis=2)
    assert not changed[:11].any() and not changed[~near].any() and changed.sum() > 2000


def test_what_the_device_scenes_exercise():
    host, (mid_layers, mid_tracks), recs = gc.host_scene()
    st = host.stats
    assert st["off_plane_rows"] >= 50 and st["outside_rows"] >= 200 and st["multi_camera_cells"] >= 100, st
    assert st["gap_sightings"] >= 100 and st["ring_wraps"] >= 100 and st["max_table"] > 256 and st["ignored_rows"] >= 1000, st
    assert st["consecutive"] >= 5000 and st["restarts"] >= 100 and mid_layers.any() and all(len(t) > 50 for t in mid_tracks), st
    assert host.max("dwell_us") > 0 and host.layer("flow_x").min() < 0 < host.layer("flow_x").max()
    assert sum(len(r) for r in recs) >= 10000 and max(int(r[:, 6].max()) for r in recs if len(r)) > 0
    burst, brecs = gc.host_burst()
    cell = burst.cell_of(50, 5250)
    assert cell == 10 * 40 + 20 and [len(r) for r in brecs] == [400, 300, 400, 300, 0, 0, 0, 0, 3]
    assert burst.layer("presence")[10, 20] == 1403 and burst.layer("presence").sum() == 1403 and burst.layer("visits")[10, 20] == 703
    assert burst.layer("dwell_us")[10, 20] == 700 * 500000 and burst.stats["max_table"] == 400 and burst.stats["multi_camera_cells"] == 1
    assert len(burst.tracks(0)) == 3 and burst.tracks(1) == []
    specs, cases = gc.division_cases()
    assert len(specs) == 64 and len(cases) == 4096
    on = [bool(G.project(specs[h].H, 0.5 * (r[0] + r[2]), float(r[3]), 1024)[0]) for h, r, _ in cases]
    assert all(w is None or w == o for (_, _, w), o in zip(cases, on)) and 1000 < sum(on) < 3800
    qx = G.project(np.eye(3), float(1 << 19), 10.0, 1024)[1]
    assert int(qx) == 1 << 29


def test_site_people_joins_cameras_by_global_id():
    rows = [np.array([[5, 0, 1000, 2000, 10, 0, 10, 3], [6, 0, 0, 0, 0, 0, 0, -2]], np.int32), None,
            np.array([[9, 0, 1003, 2001, 0, 0, -1, 3], [4, 0, -7, 5, 1, 1, 1, -1]], np.int32)]
    ids = [{5: 1, 6: 2}, {}, [(9, 1), (4, 0)]]
    people = G.site_people(rows, ids)
    assert list(people) == [1] and people[1] == dict(qx=1001, qy=2000, speed=10, streams=[0, 2], tracks=[(0, 5), (2, 9)])
