"""Host side of the action stage: explicit timestamps in yolo_deepsort_amd.action (the comparator of the device tests) and the
descriptor DeviceActionIdentify packs for the device - no GPU needed."""
import numpy as np
import pytest

from oracle.gen_golden import action_scene
from yolo_deepsort_amd import action as A

from actions_common import as_tuples, fixture_row_times, trace_actions, trace_want


def test_explicit_timestamps_reproduce_the_reference_trace():
    """The 40 action_scene() frames with per-row times by the fixture's clock rule (1000.0, + 0.04 for every row whose id is
    already cached) equal action_trace.json - recorded from the reference with the stepped wall clock - frame by frame."""
    frames, want = action_scene(), trace_want()
    times = fixture_row_times(frames)
    host = A.ActionIdentify(trace_actions(), max_age=3, max_size=4)
    assert len(frames) == len(want) == 40
    names = set()
    for t, det in enumerate(frames):
        got = as_tuples(host.update(det, times[t]))
        assert got == want[t], t
        names |= {r[2] for r in got}
    assert names == {"takeoff", "landing", "glide", "fast_crossing", "break_into"}
    assert host.update(None, 5.0) is None


def test_scalar_timestamp_is_every_rows_time_and_none_keeps_the_clock(monkeypatch):
    import time
    host = A.ActionIdentify([A.FastCrossing(0, 0.05)], max_age=3, max_size=4)
    row = lambda x: np.array([[x, 0, x + 10, 40, 7, 0]], np.int32)      # noqa: E731
    assert host.update(row(0), 1.0) == [] and len(host.cache[7].timestamps) == 0     # a first sighting stores no time
    host.update(row(10), 2.0)
    host.update(row(20), 2.0625)
    assert list(host.cache[7].timestamps) == [2.0, 2.0625]
    monkeypatch.setattr(time, "time", lambda: 123.5)
    host.update(row(30))
    assert list(host.cache[7].timestamps) == [2.0, 2.0625, 123.5]
    o = A.Orbit(4, 1, 0)
    o.update([0, 0, 10, 40, 1, 0], 9.25)
    o.update([0, 0, 10, 40, 1, 0])
    assert list(o.timestamps) == [9.25, 123.5] and list(o.deque) == [(5.0, 40), (5.0, 40)]


def test_descriptor_packing():
    acts = [A.TakeOff(0, (1, 2)), A.Landing(3, (1.5, 2)), A.Glide(np.int64(2), (2, 4)), A.FastCrossing(2.0, 0.05), A.BreakInto(0, 2)]
    dev = A.DeviceActionIdentify(acts, max_age=3, max_size=16, n_streams=5)       # packs without touching the GPU
    assert dev.kind.dtype == np.int32 and dev.kind.tolist() == [0, 1, 2, 3, 4]
    assert dev.class_ids.dtype == np.int32 and dev.class_ids.tolist() == [0, 3, 2, 2, 0]
    assert dev.param.dtype == np.float64 and dev.param.tolist() == [[1, 2], [1.5, 2], [2, 4], [0.05, 0], [2, 0]]
    assert dev.names == ["takeoff", "landing", "glide", "fast_crossing", "break_into"]
    assert (dev.max_age, dev.max_size, dev.n_streams) == (3, 16, 5) and dev._h is None
    same = A.ActionIdentify(acts, max_age=3, max_size=16).to_device(5)
    assert same.kind.tolist() == dev.kind.tolist() and same.param.tolist() == dev.param.tolist() and same.n_streams == 5


def test_device_refusals_name_action_id():
    class Mine(A.TakeOff):
        def _step(self, prev, cur, dt):
            return True

    class Own(A.Action):
        def confirm(self, orbit):
            return True
    for bad in ([Mine(0, (1, 2))], [A.BreakInto(0, 2), Own("own")], [A.Glide(0.5, (1, 2))], [A.BreakInto("person", 2)]):
        with pytest.raises(ValueError, match="action_id"):
            A.DeviceActionIdentify(bad)
    with pytest.raises(ValueError, match="action_id"):
        A.DeviceActionIdentify([A.BreakInto(0, 2)], max_size=A.MAX_SIZE_DEVICE + 1)
    with pytest.raises(ValueError, match="action_id"):
        A.ActionIdentify([A.BreakInto(0, 2)], max_size=17).to_device(2)
    with pytest.raises(ValueError, match="action_id"):
        A.as_device_actions(object(), 3)
    with pytest.raises(ValueError, match="action_id"):
        A.as_device_actions(A.DeviceActionIdentify([A.BreakInto(0, 2)], n_streams=2), 3)
    assert A.MAX_SIZE_DEVICE >= 16
