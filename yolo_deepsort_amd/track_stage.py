"""The Python front the per-stream table stages share: ``DeviceActionIdentify`` (action.py), ``DeviceZoneMonitor`` (zones.py),
``DeviceHeatMap`` (heatmap.py) and ``DeviceGroundMap`` (ground.py).

It mirrors csrc/track_stage.h, the frame their device halves share: a stage keeps one table of tracks per video stream in HBM
behind a ``yds_<LIB>`` handle, one launch advances all tables over the frames of a call, and a step runs the stage in its slot
(csrc/engine.h StageSlot, ``Pipeline.set_actions`` / ``set_zones`` / ``set_heatmap`` / ``set_ground``).  ``TrackStage`` holds what
does not depend on what a table holds - the settings' checks, the handle, the frame table of a call, the two-call table read,
reset / timing / close, and the two rules by which a caller's object becomes a stage (``as_device``, ``fresh``); ``GridStage`` adds
what the two stages with int64 layers share.  A stage adds its specs, ``_create`` / ``_setup``, its update call and its report.
"""

from __future__ import annotations

import ctypes as C

import numpy as np


def as_int(name, v, what):
    try:
        ok = not isinstance(v, str) and int(v) == v
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{name}: {what} {v!r} is no integer")
    return int(v)


def check_max_age(name, max_age):
    if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 1:
        raise ValueError(f"{name}: max_age {max_age!r} is no integer >= 1")
    return int(max_age)


def per_stream(x, n_streams, is_one, message, or_none=False):
    """``x`` - one item for all streams (``is_one(x)``) or a list with one item (``or_none``: or None) per stream - as a list of
    n_streams items; ValueError(message % n_streams) otherwise."""
    if is_one(x):
        return [x] * n_streams
    try:
        per = list(x)
    except TypeError:
        per = None
    if per is None or len(per) != n_streams or not all(is_one(s) or (or_none and s is None) for s in per):
        raise ValueError(message % n_streams)
    return per


class TrackStage:
    NAME = None                 # the prefix of the stage's error texts
    LIB = None                  # its C entries are yds_<LIB>_create, _destroy, _reset, _set_timing, _last_us, _get_<table>
    HOST = None                 # the host comparator whose max_age as_device takes over
    TIMED = ("update",)         # what last_us can be asked for, in the library's order
    PER_STREAM = True           # the streams have specs of their own: fresh(n) cannot make more of them

    def __init__(self, n_streams, max_age):
        self.n_streams = int(n_streams)
        if self.n_streams < 1:
            raise ValueError(f"{self.NAME}: {n_streams} streams")
        self.max_age = self._check_max_age(max_age)
        self._h = None

    def _check_max_age(self, max_age):
        return check_max_age(self.NAME, max_age)

    # ---- the handle
    def _entry(self, what):
        from . import _lib
        return getattr(_lib.load(), f"yds_{self.LIB}_{what}")

    def _create(self, lib):
        """The yds_<LIB>_create call of these settings."""
        raise NotImplementedError

    def _setup(self, lib, h):
        """What a new handle needs before its first call (the per-stream specs)."""

    @property
    def handle(self):
        """The yds_<LIB> handle, created (and its per-stream set-up done) on first use."""
        if self._h is None:
            from . import _lib
            _lib.init()
            lib = _lib.load()
            h = _lib.check_ptr(self._create(lib))
            try:
                self._setup(lib, h)
            except Exception:
                self._entry("destroy")(h)
                raise
            self._h = h
        return self._h

    def _stream(self, stream):
        s = int(stream)
        if s < 0 or s >= self.n_streams:
            raise ValueError(f"{self.NAME}: stream {s} outside [0, {self.n_streams})")
        return s

    # ---- a call
    def pack(self, frames_rows, stream_of, times, per_row=False, check_streams=True):
        """The frame table of an update call.  Frames in the order given (a stream's frames in time order), frame f of stream
        ``stream_of[f]`` at time ``times[f]``; a frame whose rows are None is not seen.  Returns (live, rows6, first, sof, tm):
        the indices of the frames that are seen, their rows back to back as int32 [m, 6], frame k = rows [first[k], first[k + 1]),
        its stream and its time.  per_row: ``times[f]`` is a number or one number per row, tm holds one per row.  check_streams:
        a stream outside [0, n_streams) is refused here, else it is left to the library."""
        live = [f for f in range(len(frames_rows)) if frames_rows[f] is not None]
        rows = [np.asarray(frames_rows[f], dtype=np.int64).reshape(-1, 6) if len(frames_rows[f]) else np.zeros((0, 6), np.int64) for f in live]
        if any(r.size and np.abs(r).max() >= 2 ** 31 for r in rows):
            raise ValueError(f"{self.NAME}: a row value does not fit 32 bits")
        first = np.zeros(len(live) + 1, np.int32)
        first[1:] = np.cumsum([len(r) for r in rows])
        rows6 = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 6)), dtype=np.int32)
        sof = np.ascontiguousarray([self._stream(stream_of[f]) if check_streams else stream_of[f] for f in live], dtype=np.int32)
        if per_row:
            tm = np.zeros(int(first[-1]), np.float64)
            for k, f in enumerate(live):
                tm[first[k]:first[k + 1]] = np.asarray(times[f], np.float64)
        else:
            tm = np.ascontiguousarray([times[f] for f in live], dtype=np.float64)
        return live, rows6, first, sof, tm

    def update(self, stream, rows, t):
        """One frame of one stream: the host comparator's ``update`` (None in, None out, nothing touched)."""
        return self.update_batch([rows], [stream], [t])[0]

    # ---- reading a table
    def _table_count(self, what, stream, n_columns):
        from . import _lib
        n = C.c_int(0)
        _lib.check(self._entry("get_" + what)(self.handle, self._stream(stream), *[None] * n_columns, 1 << 30, C.byref(n)))
        return n.value

    def _read_table(self, what, stream, columns):
        """The two-call read of yds_<LIB>_get_<what>: ask the count, then copy.  columns: (dtype, trailing shape) of every column,
        in the entry's order; returns the columns, one row per entry of the stream's table."""
        from . import _lib
        n, m = C.c_int(0), max(self._table_count(what, stream, len(columns)), 1)
        cols = [np.zeros((m,) + tuple(shape), dtype) for dtype, shape in columns]
        _lib.check(self._entry("get_" + what)(self.handle, int(stream), *[_lib.ptr(c) for c in cols], m, C.byref(n)))
        return [c[:n.value] for c in cols]

    # ---- between calls
    def reset(self, stream=None):
        """Empty tables (and what the stage counts per stream) for one stream, or all of them."""
        from . import _lib
        if self._h is not None:
            _lib.check(self._entry("reset")(self._h, -1 if stream is None else int(stream)))

    def set_timing(self, on=True):
        from . import _lib
        _lib.check(self._entry("set_timing")(self.handle, 1 if on else 0))

    def last_us(self, what="update"):
        """Device time of the last timed launch of ``what`` in microseconds (set_timing first)."""
        from . import _lib
        if what not in self.TIMED:
            raise ValueError(f"{self.NAME}: last_us of " + " or ".join(repr(t) for t in self.TIMED))
        us = C.c_float(0)
        which = (self.TIMED.index(what),) if len(self.TIMED) > 1 else ()
        _lib.check(self._entry("last_us")(self.handle, *which, C.byref(us)))
        return us.value

    def close(self):
        if self._h is not None:
            self._entry("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- a caller's object as a stage
    @classmethod
    def _from_host(cls, x, n_streams, max_age):
        return cls(x, x.max_age if isinstance(x, cls.HOST) else max_age, n_streams=n_streams)

    @classmethod
    def as_device(cls, x, n_streams, max_age=30):
        """``x`` as a stage of at least n_streams streams: a stage object itself (its tables are used as they are), else a new one
        from the host comparator (its settings) or from specs; ValueError naming the stage for anything else."""
        if isinstance(x, cls):
            if x.n_streams < n_streams:
                raise ValueError(f"{cls.NAME}: a {cls.__name__} of {x.n_streams} streams for {n_streams} streams")
            return x
        return cls._from_host(x, n_streams, max_age)

    def _settings(self, n_streams):
        """The constructor's arguments for the first n_streams streams of this object."""
        raise NotImplementedError

    def _what(self):
        return "a " + type(self).__name__

    def fresh(self, n_streams):
        """Another object of the first n_streams specs (at least one) and the same settings, without a handle: empty tables for a
        run of its own, never this object's."""
        if self.PER_STREAM and self.n_streams < n_streams:
            raise ValueError(f"{self.NAME}: {self._what()} of {self.n_streams} streams for {n_streams} sources")
        return type(self)(*self._settings(max(int(n_streams), 1)))


class GridStage(TrackStage):
    """A stage with int64 layers per cell that ``render`` blends into frames resident in HBM."""
    LAYERS = ()
    TIMED = ("update", "render")

    def _layer(self, name):
        if name not in self.LAYERS:
            raise ValueError(f"{self.NAME}: layer {name!r} is not one of {self.LAYERS}")
        return self.LAYERS.index(name)

    def _read_max(self, name, *stream):
        from . import _lib
        v = C.c_int64(0)
        _lib.check(self._entry("get_max")(self.handle, *stream, self._layer(name), C.byref(v)))
        return int(v.value)

    def _render(self, what, frames_dev, slots, stream_of, h, w, layer, vmax, alpha, lut, n_frames):
        """yds_<LIB>_<what>: frame slots[i] of frames_dev (uint8 frames h*w*3 bytes apart) takes ``layer`` as stream stream_of[i]
        sees it.  Slots must be distinct and inside [0, n_frames) (default: max slot + 1).  Synchronous."""
        from . import _lib
        from .heatmap import check_lut
        slots_a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        sof = np.ascontiguousarray(stream_of, dtype=np.int32).reshape(-1)
        if len(slots_a) != len(sof):
            raise ValueError("%s: %d slots for %d streams" % (self.NAME, len(slots_a), len(sof)))
        k = self._layer(layer)
        if len(slots_a) == 0:
            return
        n_src = int(slots_a.max()) + 1 if n_frames is None else int(n_frames)
        _lib.check(self._entry(what)(self.handle, frames_dev, n_src, _lib.ptr(slots_a), _lib.ptr(sof), len(slots_a), int(h), int(w), k,
                                     as_int(self.NAME, vmax, "vmax"), as_int(self.NAME, alpha, "alpha"), _lib.ptr(check_lut(lut))))
