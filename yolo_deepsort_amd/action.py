"""Track-trajectory "action" heuristics that consume the tracker's int32 rows.

Host-side consumer of the hot path's output (reference action/action_Identify.py:4-47,
action/orbit.py:5-25, action/actions.py:24-150).  Pure Python, stateful and
wall-clock dependent like the reference; kept so that ``video_deepsort.py`` imports and runs.  Explicit timestamps
(``update(..., timestamps)``) replace the clock where the caller knows the frames' times, and ``DeviceActionIdentify`` runs the
same stage for many streams with the orbit caches in HBM (csrc/actions.hip), equal to this module fed the same rows and times.

Every motion action below answers one question about a track's recent foot points: did EVERY
consecutive step satisfy a predicate (the reference's flag loop reduces to exactly that: the
flag is raised by step 1 and any failing step clears it for good).
"""

from __future__ import annotations

import time
from collections import deque

from .track_stage import TrackStage


class Orbit:
    """Recent foot points ((x1+x2)/2, y2) and their timestamps for one track id."""

    def __init__(self, max_age, track_id, class_id):
        self.max_age, self.track_id, self.class_id = max_age, track_id, class_id
        self.deque = deque(maxlen=max_age)
        self.timestamps = deque(maxlen=max_age)
        self.age = 0

    @staticmethod
    def _center_point(bbox):
        return bbox[0] + (bbox[2] - bbox[0]) / 2, bbox[3]

    def update(self, detection, timestamp=None):
        """``timestamp=None`` reads the wall clock like the reference; a number is the sighting's time instead."""
        self.age = 0
        self.deque.append(self._center_point(detection[:4]))
        self.timestamps.append(time.time() if timestamp is None else timestamp)


class Action:
    def __init__(self, name):
        self.name = name

    def confirm(self, orbit):
        raise NotImplementedError


class _Stepwise(Action):
    """True when the orbit has >= 2 points of the right class and every step passes ``_step``."""

    def __init__(self, name, class_id):
        super().__init__(name)
        self.class_id = class_id

    def _step(self, prev, cur, dt):
        raise NotImplementedError

    def confirm(self, orbit):
        pts, ts = orbit.deque, orbit.timestamps
        if len(pts) < 2 or orbit.class_id != self.class_id:
            return False
        return all(self._step(pts[i - 1], pts[i], ts[i] - ts[i - 1]) for i in range(1, len(pts)))


class TakeOff(_Stepwise):
    def __init__(self, class_id, delta):
        super().__init__("takeoff", class_id)
        self.delta = delta

    def _step(self, prev, cur, dt):
        return prev[1] - cur[1] > self.delta[1] and abs(prev[0] - cur[0]) > self.delta[0]


class Landing(_Stepwise):
    def __init__(self, class_id, delta):
        super().__init__("landing", class_id)
        self.delta = delta

    def _step(self, prev, cur, dt):
        return cur[1] - prev[1] > self.delta[1] and abs(prev[0] - cur[0]) > self.delta[0]


class Glide(_Stepwise):
    def __init__(self, class_id, delta):
        super().__init__("glide", class_id)
        self.delta = delta

    def _step(self, prev, cur, dt):
        return abs(cur[1] - prev[1]) < self.delta[1] and abs(cur[0] - prev[0]) > self.delta[0]


class FastCrossing(_Stepwise):
    def __init__(self, class_id, speed):
        super().__init__("fast_crossing", class_id)
        self.speed = speed

    def _step(self, prev, cur, dt):
        return abs(cur[0] - prev[0]) / (dt * 1000) > self.speed


class BreakInto(Action):
    def __init__(self, class_id, timeout):
        super().__init__("break_into")
        self.class_id, self.timeout = class_id, timeout

    def confirm(self, orbit):
        return orbit.class_id == self.class_id and len(orbit.deque) > self.timeout


class ActionIdentify:
    def __init__(self, actions, max_age=30, max_size=4):
        self.cache = {}
        self.max_age, self.max_size, self.actions = max_age, max_size, actions

    def clone(self):
        return ActionIdentify(self.actions, self.max_age, self.max_size)

    def to_device(self, n_streams=1):
        """The same actions and settings with the orbit caches of ``n_streams`` streams in HBM (``DeviceActionIdentify``)."""
        return DeviceActionIdentify(self.actions, self.max_age, self.max_size, n_streams)

    def update(self, detections, timestamps=None):
        """``timestamps``: None (the wall clock at every ``Orbit.update``, like the reference), one number for the frame, or a
        sequence with one number per row; used for rows whose id is already cached (a first sighting stores no time)."""
        if detections is None:
            return None
        per_row = timestamps is not None and hasattr(timestamps, "__len__")
        seen = set()
        for k, det in enumerate(detections):
            tid = det[4]
            seen.add(tid)
            if tid in self.cache:
                self.cache[tid].update(det, timestamps[k] if per_row else timestamps)
            else:                                   # first sighting only registers the track
                self.cache[tid] = Orbit(self.max_size, tid, det[-1])
        for tid in [t for t in self.cache if t not in seen]:
            self.cache[tid].age += 1
            if self.cache[tid].age >= self.max_age:
                del self.cache[tid]
        return [(tid, o.class_id, a.name) for tid, o in self.cache.items() if o.age == 0
                for a in self.actions if a.confirm(o)]


# ---- the same stage with the orbit caches in HBM (csrc/actions.hip) ---------------------------------------------------------------
_KINDS = ((TakeOff, 0), (Landing, 1), (Glide, 2), (FastCrossing, 3), (BreakInto, 4))     # YDS_ACT_* of include/ydsort.h
MAX_SIZE_DEVICE = 16            # YDS_ACT_MAX_SIZE
MAX_ACTIONS_DEVICE = 32         # YDS_ACT_MAX_ACTIONS


def pack_actions(actions, max_age=30, max_size=4):
    """(kind int32 [A], class_id int32 [A], param float64 [A, 2], names) of a list of built-in actions as yds_actions_create takes
    them.  Raises ValueError naming ``action_id`` for anything the device cannot run: an action that is not exactly one of the five
    built-in classes (a subclass may override ``confirm``), a class id that is no integer, max_size outside [1, 16]."""
    import numpy as np
    try:
        actions = list(actions)
    except TypeError:
        raise ValueError(f"action_id: actions must be a list of built-in actions, got {type(actions).__name__}") from None
    if int(max_size) != max_size or not 1 <= max_size <= MAX_SIZE_DEVICE:
        raise ValueError(f"action_id: max_size {max_size!r} outside [1, {MAX_SIZE_DEVICE}] (the device's orbit ring)")
    if int(max_age) != max_age:
        raise ValueError(f"action_id: max_age {max_age!r} is not an integer")
    if len(actions) > MAX_ACTIONS_DEVICE:
        raise ValueError(f"action_id: {len(actions)} actions, the device runs at most {MAX_ACTIONS_DEVICE}")
    kind = np.zeros(len(actions), np.int32)
    cls = np.zeros(len(actions), np.int32)
    param = np.zeros((len(actions), 2), np.float64)
    names = []
    for k, a in enumerate(actions):
        code = dict(_KINDS).get(type(a))
        if code is None:
            raise ValueError(f"action_id: action {k} ({type(a).__name__}) is not one of the built-in actions "
                             "TakeOff, Landing, Glide, FastCrossing, BreakInto; the device runs only those")
        try:
            integral = int(a.class_id) == a.class_id and abs(int(a.class_id)) < 2 ** 31
        except (TypeError, ValueError):
            integral = False
        if not integral:
            raise ValueError(f"action_id: action {k} ({a.name}) has class_id {a.class_id!r}, not an integer")
        kind[k], cls[k] = code, int(a.class_id)
        try:
            if code <= 2:
                param[k] = float(a.delta[0]), float(a.delta[1])
            else:
                param[k, 0] = float(a.speed if code == 3 else a.timeout)
        except (TypeError, ValueError, IndexError):
            raise ValueError(f"action_id: action {k} ({a.name}) has parameters the device cannot take") from None
        names.append(a.name)
    return kind, cls, param, names


class DeviceActionIdentify(TrackStage):
    """``ActionIdentify`` for ``n_streams`` video streams with every orbit cache in HBM: one launch advances the caches of all
    streams over the frames of a call, and the rows equal the host module's fed the same rows and times (double arithmetic in the
    same operation order).  One difference: two sightings with the same time make FastCrossing divide by zero - Python raises,
    the device follows IEEE (x / 0 = inf passes, 0 / 0 fails)."""
    NAME, LIB = "action_id", "actions"
    PER_STREAM = False              # (the streams share the actions: fresh(n) may make more caches than this object has)
    _check_max_age = staticmethod(int)      # (pack_actions has refused what is no integer; the host module sets no lower bound)

    def __init__(self, actions, max_age=30, max_size=4, n_streams=1):
        self.kind, self.class_ids, self.param, self.names = pack_actions(actions, max_age, max_size)
        self.actions, self.max_size = list(actions), int(max_size)
        super().__init__(n_streams, max_age)

    def _settings(self, n_streams):
        return self.actions, self.max_age, self.max_size, n_streams

    def clone(self, n_streams=None):
        return self.fresh(self.n_streams if n_streams is None else n_streams)

    def _create(self, lib):
        from . import _lib
        return lib.yds_actions_create(self.n_streams, _lib.ptr(self.kind), _lib.ptr(self.class_ids), _lib.ptr(self.param), len(self.names),
                                      self.max_age, self.max_size)

    def name_rows(self, rows4):
        return [(int(r[1]), int(r[2]), self.names[int(r[3])]) for r in rows4]

    def update_batch(self, frames_rows, stream_of, times):
        """Frames in the order given (a stream's frames in time order), frame f of stream ``stream_of[f]``; ``times[f]`` is a number
        for the frame or a sequence with one number per row.  Returns one ``[(track_id, class_id, name), ...]`` per frame (None
        for a frame whose rows are None: it is not seen).  A stream outside the handle's is refused by the library (YdsError)."""
        import ctypes as C
        import numpy as np
        from . import _lib
        live, rows6, first, sof, row_time = self.pack(frames_rows, stream_of, times, per_row=True, check_streams=False)
        per = [None] * len(frames_rows)
        if not live:
            return per
        cap = max(len(rows6) * len(self.names), 1)
        out = np.zeros((cap, 4), np.int32)
        m = C.c_int(0)
        _lib.check(_lib.load().yds_actions_update(self.handle, _lib.ptr(rows6), _lib.ptr(first), _lib.ptr(sof), _lib.ptr(row_time), len(live),
                                                  _lib.ptr(out), cap, C.byref(m)))
        for f in live:
            per[f] = []
        for r in out[:m.value]:
            per[live[int(r[0])]] += self.name_rows([r])
        return per

    def orbits(self, stream=0):
        """[(track_id, age, points held), ...] of one stream's cache in insertion order."""
        import numpy as np
        ids, ages, lens = self._read_table("orbits", stream, [(np.int32, ())] * 3)
        return list(zip(ids.tolist(), ages.tolist(), lens.tolist()))

    @classmethod
    def _from_host(cls, x, n_streams, max_age):
        if not isinstance(x, ActionIdentify):
            raise ValueError(f"action_id must be an ActionIdentify or a DeviceActionIdentify, got {type(x).__name__}")
        return x.to_device(n_streams)


as_device_actions = DeviceActionIdentify.as_device      # (the name Pipeline.set_actions and callers import; track_stage.TrackStage.as_device is the rule)
