"""Zones and counting lines on the host (yolo_deepsort_amd.zones): the rules of include/ydsort.h restated in Python ints - the
comparator of every device test - checked against the boundary truths the rules promise, a scripted track, the packing of the
geometry and the visitor log.  No GPU."""
import numpy as np
import pytest

from yolo_deepsort_amd import zones as Z

from zones_common import box_at, fast_scene, kind_counts, standard_geometry

SQUARE = [(100, 100), (200, 100), (200, 200), (100, 200)]


def _is_inside(poly, x2, y, **kw):
    """Inside through ZoneMonitor: a track first seen at the doubled foot point (x2, 2 y) enters a min_sightings=1 zone at once."""
    m = Z.ZoneMonitor([Z.Zone(poly)], [], **kw)
    ev = m.update([box_at(x2, y)], 0.0)
    assert m.tracks() == [(1, 0, 1 if ev else 0)]
    return bool(ev)


@pytest.mark.parametrize("poly", [SQUARE, SQUARE[::-1]])
def test_inside_boundary_truths_of_the_square(poly):
    """Left edge, top edge and top-left vertex inside; right edge, bottom edge and the other three vertices outside; half a pixel
    inside the right or bottom edge inside; the vertex order changes nothing."""
    assert _is_inside(poly, 200, 150) and _is_inside(poly, 300, 100) and _is_inside(poly, 200, 100)
    assert not _is_inside(poly, 400, 150) and not _is_inside(poly, 300, 200)
    assert not _is_inside(poly, 400, 100) and not _is_inside(poly, 400, 200) and not _is_inside(poly, 200, 200)
    assert _is_inside(poly, 399, 150) and not _is_inside(poly, 401, 150)
    assert _is_inside(poly, 199 + 1, 150) and not _is_inside(poly, 199, 150)
    poly2 = [(2 * x, 2 * y) for x, y in poly]
    assert Z.inside((300, 399), poly2) and not Z.inside((300, 400), poly2)      # (a row's doubled y is even: the function itself)
    assert Z.inside((300, 200), poly2) and not Z.inside((300, 199), poly2)
    assert _is_inside(poly, 300, 199)


def _crossing(line, p, c, cls=0, line_cls=-1):
    """Cross through ZoneMonitor: a track seen at doubled points p then c; +1 / -1 / 0."""
    m = Z.ZoneMonitor([], [Z.Line(*line, class_id=line_cls)])
    assert m.update([box_at(p[0], p[1], cls=cls)], 0.0) == []
    ev = m.update([box_at(c[0], c[1], cls=cls)], 1.0)
    assert len(ev) <= 1
    fwd, back = m.counts()[1][0]
    assert (fwd, back) == ((1, 0) if ev and ev[0][2] == Z.CROSS_FWD else (0, 1) if ev else (0, 0))
    return 0 if not ev else 1 if ev[0][2] == Z.CROSS_FWD else -1


def test_cross_boundary_truths():
    """A horizontal line drawn left to right, A = (100, 200), B = (300, 200): below it in the image is the >= 0 side (FORWARD),
    a point on the line belongs to that side, the segment contains A and not B, a move along the line or of zero length is no
    crossing, and the reverse move is always the opposite crossing.  Points are (doubled x, y)."""
    line = ((100, 200), (300, 200))
    assert _crossing(line, (400, 190), (400, 210)) == 1 and _crossing(line, (400, 210), (400, 190)) == -1
    assert _crossing(line, (400, 190), (400, 200)) == 1                  # onto the line: the >= 0 side
    assert _crossing(line, (400, 200), (400, 210)) == 0                  # from the line further down: the same side
    assert _crossing(line, (400, 200), (400, 190)) == -1
    assert _crossing(line, (200, 190), (200, 210)) == 1                  # through A
    assert _crossing(line, (600, 190), (600, 210)) == 0                  # through B
    assert _crossing(line, (599, 190), (599, 210)) == 1                  # half a pixel before B
    assert _crossing(line, (601, 190), (601, 210)) == 0 and _crossing(line, (199, 190), (199, 210)) == 0
    assert _crossing(line, (300, 200), (500, 200)) == 0                  # along the line
    assert _crossing(line, (400, 190), (400, 190)) == 0                  # zero length
    assert _crossing(line, (400, 190), (400, 210), cls=2, line_cls=0) == 0 and _crossing(line, (400, 190), (400, 210), cls=2, line_cls=2) == 1
    rs = np.random.RandomState(0)
    n = 0
    for _ in range(4000):
        a, b, p, c = (tuple(int(v) for v in rs.randint(-6, 7, 2)) for _ in range(4))
        if a == b:
            continue
        d = Z.cross(p, c, a, b)
        assert d == -Z.cross(c, p, a, b), (a, b, p, c)
        n += d != 0
    assert n >= 300


def test_scripted_track_enter_debounce_exit_lost_and_dwell():
    """Two tracks against a min_sightings=2 zone of class 0 (the square) and a min_sightings=1 zone of class 7, max_age=2."""
    m = Z.ZoneMonitor([Z.Zone(SQUARE, class_id=0, min_sightings=2, name="hall"), Z.Zone(SQUARE, class_id=7)], [Z.Line((150, 0), (150, 300), name="door")],
                      max_age=2)
    inside, outside = box_at(300, 150, tid=5), box_at(500, 150, tid=5)
    assert m.update([outside], 0.0) == []
    assert m.update(None, 0.5) is None and m.tracks() == [(5, 0, 0)]
    assert m.update([inside], 1.0) == [(5, 0, Z.CROSS_FWD, "door", 1.0, 0.0)]          # first sighting inside: streak 1 of 2
    assert m.update([outside], 2.0) == [(5, 0, Z.CROSS_BACK, "door", 2.0, 0.0)] and m.stats["abandoned"] == 1
    assert m.update([inside], 3.0) == [(5, 0, Z.CROSS_FWD, "door", 3.0, 0.0)]
    assert m.update([inside], 4.0) == [(5, 0, Z.ENTER, "hall", 4.0, 0.0)]
    assert m.counts() == ([[1, 1, 0, 0], [0, 0, 0, 0]], [[2, 1]]) and m.tracks() == [(5, 0, 1)]
    assert m.update([], 5.0) == [] and m.tracks() == [(5, 1, 1)]                       # a miss below max_age keeps the bit
    assert m.update([inside], 6.0) == []
    assert m.update([outside], 7.0) == [(5, 0, Z.CROSS_BACK, "door", 7.0, 0.0)]       # streak 1 of 2: still inside
    assert m.update([outside], 8.5) == [(5, 0, Z.EXIT, "hall", 8.5, 4.5)]
    assert m.counts()[0][0] == [0, 1, 1, 0]
    m.update([inside], 9.0)
    assert m.update([inside, box_at(300, 150, tid=6, cls=7)], 10.0) == [(5, 0, Z.ENTER, "hall", 10.0, 0.0), (6, 7, Z.ENTER, 1, 10.0, 0.0)]
    assert m.update([box_at(300, 150, tid=6, cls=7)], 11.0) == []
    assert m.update([], 12.0) == [(5, 0, Z.LOST, "hall", 12.0, 0.0)]                   # last seen 10.0, entered 10.0
    assert m.update([], 13.0) == [(6, 7, Z.LOST, 1, 13.0, 1.0)]                        # last seen 11.0, entered 10.0
    assert m.tracks() == [] and m.counts()[0] == [[0, 2, 1, 1], [0, 1, 0, 1]]
    with pytest.raises(ValueError, match="twice"):
        m.update([inside, inside], 14.0)
    c = m.clone()
    assert c.counts() == ([[0, 0, 0, 0], [0, 0, 0, 0]], [[0, 0]]) and c.max_age == 2 and c.tracks() == []


def test_anchor_is_clamped():
    assert Z.anchor([2 ** 30, 0, 2 ** 30, -2 ** 30, 1, 0]) == (2 ** 24, -2 ** 24) and Z.anchor([3, 0, 4, 9, 1, 0]) == (7, 18)


def test_random_recipe_exercises_every_rule():
    """The scene of the device tests' randomised case, on the host alone: every kind of event, abandoned streaks, orientation
    values of exactly zero and a table beyond one workgroup's width occur."""
    m = Z.ZoneMonitor(*standard_geometry(), max_age=3)
    n = kind_counts([m.update(r, t) for r, t in fast_scene(0, 300, 60)])
    assert min(n[Z.ENTER], n[Z.EXIT], n[Z.CROSS_FWD], n[Z.CROSS_BACK]) >= 100 and n[Z.LOST] >= 20
    assert m.stats["abandoned"] >= 50 and m.stats["zero_orientations"] >= 20 and m.stats["max_table"] > 256
    z4, l2 = m.counts()
    assert [r[1] for r in z4] and sum(r[1] for r in z4) == n[Z.ENTER] and sum(r[0] for r in z4) == n[Z.ENTER] - n[Z.EXIT] - n[Z.LOST]
    assert sum(r[0] for r in l2) == n[Z.CROSS_FWD] and sum(r[1] for r in l2) == n[Z.CROSS_BACK]
    assert all(r[0] == sum(1 for _, _, mask in m.tracks() if mask >> z & 1) for z, r in enumerate(z4))


def test_pack_geometry_and_its_refusals():
    zones, lines = standard_geometry()
    ptr, xy, zc, zm, lxy, lc, zn, ln = Z.pack_geometry(zones, lines)
    assert ptr.tolist() == [0, 4, 9, 13, 17] and xy.shape == (17, 2) and xy.dtype == np.int32 and xy[4].tolist() == [300, 300]
    assert zc.tolist() == [-1, 0, 2, -1] and zm.tolist() == [1, 2, 1, 3] and lc.tolist() == [-1, 0, 2, -1]
    assert lxy[3].tolist() == [400, 400, 600, 400] and zn == [0, 1, 2, 3] and ln == [0, 1, 2, 3]
    assert Z.pack_geometry([Z.Zone(SQUARE, name="a")], [Z.Line((0, 0), (1, 1), name="b")])[6:] == (["a"], ["b"])
    empty = Z.pack_geometry([], [])
    assert empty[0].tolist() == [0] and empty[1].shape == (0, 2) and empty[4].shape == (0, 4)
    lim = 2 ** 20
    Z.pack_geometry([Z.Zone([(-lim, -lim), (lim, -lim), (lim, lim)], min_sightings=255)] * 32, [Z.Line((-lim, 0), (lim, 0))] * 32)
    Z.pack_geometry([Z.Zone([(k, k * k) for k in range(16)])], [])
    bad = [
        ([Z.Zone(SQUARE)] * 33, []), ([], [Z.Line((0, 0), (1, 1))] * 33),
        ([Z.Zone(SQUARE[:2])], []), ([Z.Zone([(k, k * k) for k in range(17)])], []),
        ([Z.Zone([(0, 0), (lim + 1, 0), (0, 5)])], []), ([Z.Zone([(0, 0), (1.5, 0), (0, 5)])], []), ([Z.Zone([(0, 0), (1, 0), (0,)])], []),
        ([Z.Zone(SQUARE, min_sightings=0)], []), ([Z.Zone(SQUARE, min_sightings=256)], []), ([Z.Zone(SQUARE, class_id=-2)], []),
        ([Z.Zone(SQUARE, class_id="person")], []),
        ([], [Z.Line((5, 5), (5, 5))]), ([], [Z.Line((0, 0), (0, -lim - 1))]), ([], [Z.Line((0, 0), (1, 1), class_id=0.5)]),
        ([SQUARE], []), ([], [((0, 0), (1, 1))]), (None, []),
    ]
    for zs, ls in bad:
        with pytest.raises(ValueError, match="zones"):
            Z.pack_geometry(zs, ls)
    for kw in (dict(max_age=0), dict(max_age=1.5)):
        with pytest.raises(ValueError, match="zones"):
            Z.ZoneMonitor(zones, lines, **kw)
        with pytest.raises(ValueError, match="zones"):
            Z.DeviceZoneMonitor((zones, lines), **kw)
    with pytest.raises(ValueError, match="zones"):
        Z.DeviceZoneMonitor([(zones, lines)] * 2, n_streams=3)
    with pytest.raises(ValueError, match="zones"):
        Z.as_device_zones(Z.DeviceZoneMonitor((zones, lines), n_streams=2), 3)
    with pytest.raises(ValueError, match="zones"):
        Z.as_device_zones(object(), 1)
    d = Z.as_device_zones(Z.ZoneMonitor(zones, lines, max_age=7), 3)                     # (no handle, no GPU, until it is used)
    assert d.n_streams == 3 and d.max_age == 7 and len(d.packed) == 3 and d.host(2).max_age == 7


def test_visitor_log_two_cameras_one_person_deferred_id_and_lost():
    """Camera 0 sees track 4, camera 1 sees track 9: the same person under global id 3, deferred (0) on camera 1 for one step.  A
    second person is only ever seen by camera 1 and is closed by LOST."""
    log = Z.VisitorLog({"doors": [(0, "door"), (1, "door")], "shop": [(1, 1)]})
    E = lambda tid, kind, zone, t, dwell=0.0: (tid, 0, kind, zone, t, dwell)          # noqa: E731
    log.feed([[E(4, Z.ENTER, "door", 1.0), E(4, Z.CROSS_FWD, "door", 1.0)], None], [{4: 3}, {}])
    assert log.distinct("doors") == {3} and [v["dwell"] for v in log.visits("doors")] == [None]
    log.feed([[], [E(9, Z.ENTER, "door", 2.0), E(11, Z.ENTER, 1, 2.0)]], [{4: 3}, {9: 0, 11: 0}])
    assert log.distinct("doors") == {3} and len(log.visits("doors")) == 2 and log.distinct("shop") == set()
    log.feed([[E(4, Z.EXIT, "door", 3.0, 2.0)], []], [{4: 3}, {9: 3, 11: 5}])          # the deferred ids resolve one step later
    assert log.distinct("doors") == {3} and log.distinct("shop") == {5}
    doors = log.visits("doors")
    assert [(v["stream"], v["track_id"], v["global_id"], v["dwell"], v["closed_by"]) for v in doors] == [(0, 4, 3, 2.0, "exit"), (1, 9, 3, None, None)]
    log.feed([None, [E(11, Z.LOST, 1, 9.0, 4.5), E(9, Z.EXIT, "door", 9.0, 7.0)]], [{}, {}])     # (the tracks are gone from the map)
    shop = log.visits("shop")
    assert [(v["global_id"], v["enter"], v["exit"], v["dwell"], v["closed_by"]) for v in shop] == [(5, 2.0, 9.0, 4.5, "lost")]
    assert sum(v["dwell"] for v in log.visits("doors")) == 9.0 and log.open == {}
    log.feed([[E(4, Z.ENTER, "door", 10.0)]], [{}, {4: 8}], stream_of=[1])
    assert log.distinct("doors") == {3, 8} and log.visits("doors")[-1]["stream"] == 1
