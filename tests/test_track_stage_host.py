"""The Python front the four table stages share (yolo_deepsort_amd/track_stage.py): the frame table of a call, ``fresh`` and the
``as_device_*`` rule, over DeviceActionIdentify, DeviceZoneMonitor, DeviceHeatMap and DeviceGroundMap alike.  No case makes a
handle: nothing here needs a GPU."""
import numpy as np
import pytest

from yolo_deepsort_amd import action as A, ground as G, heatmap as H, zones as Z

SQUARE = [(0, 0), (10, 0), (10, 10), (0, 10)]
GEO = [([Z.Zone(SQUARE, name="z%d" % s)], [Z.Line((0, s), (9, s + 1))]) for s in range(3)]
HEAT = [H.HeatSpec(32, 48 + 16 * s, cell=16, class_id=s) for s in range(3)]
PLAN = dict(origin=(0.0, 0.0), cell=1.0, gw=8, gh=6, scale=100)
GROUND = [G.GroundSpec(np.diag([1.0, 1.0 + s, 1.0]), class_id=s, **PLAN) for s in range(3)]
ACTS = [A.Glide(0, (0, 3)), A.BreakInto(2, 1)]

# name, the class, its as_device_*, a stage of three streams, what tells its streams apart (None: they share everything), its settings
STAGES = [
    ("action_id", A.DeviceActionIdentify, A.as_device_actions, lambda: A.DeviceActionIdentify(ACTS, max_age=5, max_size=3, n_streams=3),
     None, lambda d: (d.actions, d.max_age, d.max_size)),
    ("zones", Z.DeviceZoneMonitor, Z.as_device_zones, lambda: Z.DeviceZoneMonitor(GEO, max_age=5, n_streams=3),
     lambda d: [[z.name for z in zs] + [ln.a + ln.b for ln in ls] for zs, ls in d.geometry], lambda d: (d.max_age,)),
    ("heatmap", H.DeviceHeatMap, H.as_device_heatmap, lambda: H.DeviceHeatMap(HEAT, max_age=5, n_streams=3),
     lambda d: d.specs, lambda d: (d.max_age,)),
    ("ground", G.DeviceGroundMap, G.as_device_ground, lambda: G.DeviceGroundMap(GROUND, max_age=5, speed_window=4),
     lambda d: d.specs, lambda d: (d.max_age, d.K)),
]
IDS = [s[0] for s in STAGES]


def row(tid, x, cls=0):
    return [x, 0, x + 2, 9, tid, cls]


@pytest.mark.parametrize("name,cls,as_device,make,specs,settings", STAGES, ids=IDS)
def test_the_packer(name, cls, as_device, make, specs, settings):
    """Frames [rows, None, empty, rows] over two streams: the table is the hand-written one; what does not fit 32 bits is refused
    by name, and so is a stream outside the range by the three stages that check it on the host."""
    dev = make()
    a, b = [row(7, 1), row(8, 5, 2)], np.array([row(9, 3), row(7, 4), row(1, 6)], np.int64)
    live, rows6, first, sof, tm = dev.pack([a, None, [], b], [2, 0, 0, 1], [0.5, 0.75, 1.0, 1.25])
    assert live == [0, 2, 3]
    assert rows6.dtype == np.int32 and rows6.flags["C_CONTIGUOUS"] and rows6.tolist() == a + b.tolist()
    assert first.dtype == np.int32 and first.tolist() == [0, 2, 2, 5]
    assert sof.dtype == np.int32 and sof.tolist() == [2, 0, 1]
    assert tm.dtype == np.float64 and tm.tolist() == [0.5, 1.0, 1.25]
    # a time per row (the action stage's form): a number stands for every row of its frame
    tm = dev.pack([a, None, [], b], [2, 0, 0, 1], [[0.5, 0.6], 0.75, 1.0, 1.25], per_row=True)[4]
    assert tm.dtype == np.float64 and tm.tolist() == [0.5, 0.6, 1.25, 1.25, 1.25]
    live, rows6, first, sof, tm = dev.pack([None, None], [0, 1], [0.0, 0.0])
    assert live == [] and rows6.shape == (0, 6) and first.tolist() == [0] and len(sof) == 0 and len(tm) == 0
    assert dev.update_batch([None, None], [0, 1], [0.0, 0.0]) == [None, None] and dev.update(0, None, 0.0) is None
    with pytest.raises(ValueError, match=name + ".*32 bits"):
        dev.pack([a, [[0, 0, 2, 9, 1, 2 ** 31]]], [0, 1], [0.0, 0.0])
    assert dev.pack([[row(1, 2 ** 31 - 3)]], [0], [0.0])[1].tolist() == [row(1, 2 ** 31 - 3)]
    for s in (3, -1):
        if name == "action_id":                          # (its stream range is the library's to refuse, as YdsError)
            assert dev.pack([a], [s], [0.0], per_row=True, check_streams=False)[3].tolist() == [s]
        else:
            with pytest.raises(ValueError, match=name + ".*stream"):
                dev.update_batch([a], [s], [0.0])
        with pytest.raises(ValueError, match=name + ".*stream"):
            dev.pack([a], [s], [0.0])
    assert dev._h is None


@pytest.mark.parametrize("name,cls,as_device,make,specs,settings", STAGES, ids=IDS)
def test_fresh_is_another_object_of_the_first_specs(name, cls, as_device, make, specs, settings):
    dev = make()
    for n in (1, 2, 3):
        new = dev.fresh(n)
        assert type(new) is cls and new is not dev and new.n_streams == n and new._h is None
        assert settings(new) == settings(dev)
        if specs is not None:
            assert specs(new) == specs(dev)[:n]
    assert dev.fresh(0).n_streams == 1                   # (a run without sources still names a stage of one stream)
    if specs is None:                                    # the streams share the actions: a run may have more of them
        assert dev.fresh(4).n_streams == 4 and settings(dev.fresh(4)) == settings(dev)
    else:
        what = "a map" if name == "ground" else "a " + cls.__name__
        with pytest.raises(ValueError, match="%s: %s of 3 streams for 4 sources" % (name, what)):
            dev.fresh(4)
    assert dev._h is None and dev.n_streams == 3


@pytest.mark.parametrize("name,cls,as_device,make,specs,settings", STAGES, ids=IDS)
def test_as_device_keeps_a_stage_that_is_large_enough(name, cls, as_device, make, specs, settings):
    dev = make()
    assert as_device(dev, 3) is dev and as_device(dev, 1) is dev
    with pytest.raises(ValueError, match="%s: a %s of 3 streams for 4 streams" % (name, cls.__name__)):
        as_device(dev, 4)
    with pytest.raises(ValueError, match=name):
        as_device(object(), 1)
    assert dev._h is None


def test_as_device_takes_a_host_comparators_settings():
    d = A.as_device_actions(A.ActionIdentify(ACTS, max_age=7, max_size=3), 2)
    assert (d.n_streams, d.max_age, d.max_size, d.names) == (2, 7, 3, ["glide", "break_into"]) and d._h is None
    d = Z.as_device_zones(Z.ZoneMonitor(*GEO[1], max_age=7), 2)
    assert (d.n_streams, d.max_age) == (2, 7) and d.packed[1][6] == ["z1"] and d._h is None
    d = H.as_device_heatmap(H.HeatMap(HEAT[1], max_age=7), 2, max_age=3)
    assert (d.n_streams, d.max_age, d.specs) == (2, 7, [HEAT[1]] * 2) and d._h is None
    d = G.as_device_ground(G.GroundMap(GROUND[:2], max_age=7, speed_window=5), 2)
    assert (d.n_streams, d.max_age, d.K, d.specs) == (2, 7, 5, GROUND[:2]) and d._h is None
    d = H.as_device_heatmap(HEAT[:2], 2, max_age=3)
    assert (d.n_streams, d.max_age, d.specs) == (2, 3, HEAT[:2]) and d._h is None
