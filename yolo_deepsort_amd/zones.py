"""Zones and counting lines over the tracker's int32 rows: who is inside an area, who entered, how long they stayed, who crossed a
doorway in which direction.

There is no reference counterpart (the reference tracks one camera and has no geometry): the rules in include/ydsort.h (the zones
block) are the specification, ``ZoneMonitor`` restates them in Python ints, and ``DeviceZoneMonitor`` runs the same stage for many
streams with every table in HBM (csrc/zones.hip), equal to ``ZoneMonitor`` fed the same rows and times - events, counters and
tables, exactly: the geometry is integer arithmetic.

Geometry is in the stream's frame pixels.  A row ``(x1, y1, x2, y2, id, class)`` is reduced to its DOUBLED foot point
``(x1 + x2, 2 * y2)`` - twice the orbit's foot point (action.Orbit), as an integer - and every vertex is doubled before use.
"""

from __future__ import annotations

from functools import partial

from .track_stage import TrackStage, as_int, per_stream

_as_int = partial(as_int, "zones")

ENTER, EXIT, LOST, CROSS_FWD, CROSS_BACK = 0, 1, 2, 3, 4          # YDS_ZONE_* of include/ydsort.h
KIND_NAMES = ("enter", "exit", "lost", "cross_fwd", "cross_back")
MAX_ZONES = 32                  # YDS_ZONE_MAX_ZONES
MAX_LINES = 32                  # YDS_ZONE_MAX_LINES
MAX_VERTICES = 16               # YDS_ZONE_MAX_VERTICES
COORD_LIMIT = 1 << 20           # YDS_ZONE_COORD_LIMIT: |vertex coordinate| <= this
ANCHOR_LIMIT = 1 << 24          # each component of the doubled foot point is clamped to [-this, this]


class Zone:
    """A polygon of 3..16 integer vertices; class_id -1 = any class; a track's inside bit flips after ``min_sightings`` consecutive
    sightings on the other side."""

    def __init__(self, polygon, class_id=-1, min_sightings=1, name=None):
        self.polygon = [tuple(p) for p in polygon]
        self.class_id, self.min_sightings, self.name = class_id, min_sightings, name


class Line:
    """The segment a -> b (it contains a and not b); class_id -1 = any class.  FORWARD is a move onto the side of the line where
    the orientation of (a, b, point) is >= 0: for a line drawn left to right, the side below it in the image."""

    def __init__(self, a, b, class_id=-1, name=None):
        self.a, self.b = tuple(a), tuple(b)
        self.class_id, self.name = class_id, name


def _as_point(p, what):
    try:
        x, y = p
    except (TypeError, ValueError):
        raise ValueError(f"zones: {what} is {p!r}, not an (x, y) pair") from None
    x, y = _as_int(x, what), _as_int(y, what)
    if abs(x) > COORD_LIMIT or abs(y) > COORD_LIMIT:
        raise ValueError(f"zones: {what} = ({x}, {y}) lies outside [-2^20, 2^20]")
    return x, y


def pack_geometry(zones, lines):
    """(zone_ptr int32 [Z + 1], zone_xy int32 [V, 2], zone_class int32 [Z], zone_min_sightings int32 [Z], line_xy int32 [L, 4],
    line_class int32 [L], zone_names, line_names) as yds_zones_set_stream takes them; a name is the object's ``name`` or, without
    one, its index.  Raises ValueError naming ``zones`` for anything the device refuses: more than 32 zones or lines, a polygon
    of fewer than 3 or more than 16 vertices, a coordinate that is no integer or lies outside [-2^20, 2^20], min_sightings
    outside [1, 255], a line with a == b, a class id that is no 32-bit integer."""
    import numpy as np
    try:
        zones, lines = list(zones), list(lines)
    except TypeError:
        raise ValueError("zones: geometry is a (zones, lines) pair of lists") from None
    if len(zones) > MAX_ZONES:
        raise ValueError(f"zones: {len(zones)} zones, a stream holds at most {MAX_ZONES}")
    if len(lines) > MAX_LINES:
        raise ValueError(f"zones: {len(lines)} lines, a stream holds at most {MAX_LINES}")
    ptr, xy, zcls, zmin, znames = [0], [], [], [], []
    for k, z in enumerate(zones):
        if not isinstance(z, Zone):
            raise ValueError(f"zones: zone {k} is a {type(z).__name__}, not a Zone")
        if not 3 <= len(z.polygon) <= MAX_VERTICES:
            raise ValueError(f"zones: zone {k} has {len(z.polygon)} vertices, outside [3, {MAX_VERTICES}]")
        xy += [_as_point(p, f"vertex {i} of zone {k}") for i, p in enumerate(z.polygon)]
        ptr.append(len(xy))
        c = _as_int(z.class_id, f"class_id of zone {k}")
        m = _as_int(z.min_sightings, f"min_sightings of zone {k}")
        if not -1 <= c < 2 ** 31:
            raise ValueError(f"zones: class_id of zone {k} is {c}, outside [-1, 2^31)")
        if not 1 <= m <= 255:
            raise ValueError(f"zones: min_sightings of zone {k} is {m}, outside [1, 255]")
        zcls.append(c)
        zmin.append(m)
        znames.append(k if z.name is None else z.name)
    lxy, lcls, lnames = [], [], []
    for k, ln in enumerate(lines):
        if not isinstance(ln, Line):
            raise ValueError(f"zones: line {k} is a {type(ln).__name__}, not a Line")
        a, b = _as_point(ln.a, f"point a of line {k}"), _as_point(ln.b, f"point b of line {k}")
        if a == b:
            raise ValueError(f"zones: line {k} has a == b = {a}")
        c = _as_int(ln.class_id, f"class_id of line {k}")
        if not -1 <= c < 2 ** 31:
            raise ValueError(f"zones: class_id of line {k} is {c}, outside [-1, 2^31)")
        lxy.append(a + b)
        lcls.append(c)
        lnames.append(k if ln.name is None else ln.name)
    return (np.array(ptr, np.int32), np.array(xy, np.int32).reshape(-1, 2), np.array(zcls, np.int32), np.array(zmin, np.int32),
            np.array(lxy, np.int32).reshape(-1, 4), np.array(lcls, np.int32), znames, lnames)


def anchor(row):
    """The doubled foot point of a row, each component clamped to [-2^24, 2^24]."""
    x, y = int(row[0]) + int(row[2]), 2 * int(row[3])
    return max(-ANCHOR_LIMIT, min(ANCHOR_LIMIT, x)), max(-ANCHOR_LIMIT, min(ANCHOR_LIMIT, y))


def inside(p, poly2):
    """Even-odd rule over the edges of ``poly2`` (DOUBLED vertices) for the doubled point p: the left and top edges of an
    axis-parallel square belong to it, the right and bottom ones do not."""
    x, y = p
    n, hit = len(poly2), False
    for i in range(n):
        xi, yi = poly2[i]
        xj, yj = poly2[(i + 1) % n]
        if (yi > y) != (yj > y):
            s = (xj - xi) * (y - yi) - (x - xi) * (yj - yi)
            if s > 0 if yj > yi else s < 0:
                hit = not hit
    return hit


def orient(u, v, w):
    return (v[0] - u[0]) * (w[1] - u[1]) - (v[1] - u[1]) * (w[0] - u[0])


def cross(p, c, a, b, zeros=None):
    """The move p -> c against the segment a -> b (all doubled): +1 FORWARD, -1 BACKWARD, 0 no crossing.  A point on the line
    belongs to the >= 0 side; the segment contains a and not b; cross(p, c) == -cross(c, p) always.  ``zeros``: a one-element
    list that counts the orientation values that were exactly zero (tests)."""
    vals = [orient(a, b, p), orient(a, b, c)]
    sp, sc = vals[0] >= 0, vals[1] >= 0
    out = 0
    if sp != sc:
        n, q = (p, c) if sc else (c, p)
        vals += [orient(n, q, a), orient(n, q, b)]
        if (vals[2] >= 0) != (vals[3] >= 0):
            out = 1 if sc else -1
    if zeros is not None:
        zeros[0] += sum(1 for v in vals if v == 0)
    return out


class _Entry:
    __slots__ = ("cls", "age", "point", "t", "bit", "streak", "enter")

    def __init__(self, cls, n_zones):
        self.cls, self.age, self.point, self.t = cls, 0, None, 0.0
        self.bit, self.streak, self.enter = [False] * n_zones, [0] * n_zones, [0.0] * n_zones


class ZoneMonitor:
    """The zones and lines of ONE stream on the host, in Python ints.  ``update(rows, t)`` advances the table by one frame and
    returns its events ``[(track_id, class_id, kind, zone or line name (index without one), t, dwell), ...]``, entry-major, per
    entry lines before zones; ``rows=None`` (the tracker was not called) returns None and touches nothing, zero rows age every
    entry.  An id twice in one frame raises ValueError."""

    def __init__(self, zones, lines, max_age=30):
        self.zones, self.lines = list(zones), list(lines)
        g = pack_geometry(self.zones, self.lines)
        if int(max_age) != max_age or max_age < 1:
            raise ValueError(f"zones: max_age {max_age!r} is no integer >= 1")
        self.max_age = int(max_age)
        ptr, xy = g[0].tolist(), g[1].tolist()
        self._poly2 = [[(2 * x, 2 * y) for x, y in xy[ptr[k]:ptr[k + 1]]] for k in range(len(self.zones))]
        self._zcls, self._zmin = g[2].tolist(), g[3].tolist()
        self._line2 = [((2 * r[0], 2 * r[1]), (2 * r[2], 2 * r[3])) for r in g[4].tolist()]
        self._lcls = g[5].tolist()
        self.zone_names, self.line_names = g[6], g[7]
        self.table = {}                              # track id -> _Entry, in insertion order
        self._zone4 = [[0, 0, 0, 0] for _ in self.zones]
        self._line2n = [[0, 0] for _ in self.lines]
        # what the tests assert about their own scenes: debounce streaks abandoned before a flip, orientation values exactly
        # zero, the largest table
        self.stats = dict(abandoned=0, zero_orientations=0, max_table=0)

    def clone(self):
        """A fresh monitor of the same geometry and max_age."""
        return ZoneMonitor(self.zones, self.lines, self.max_age)

    @property
    def geometry(self):
        return self.zones, self.lines

    def reset(self):
        self.table.clear()
        self._zone4 = [[0, 0, 0, 0] for _ in self.zones]
        self._line2n = [[0, 0] for _ in self.lines]

    def counts(self):
        """(per zone [occupancy, entries, exits, lost], per line [forward, backward]), cumulative since creation or reset."""
        return [list(r) for r in self._zone4], [list(r) for r in self._line2n]

    def tracks(self):
        """[(track_id, age, inside mask), ...] in table order; bit z of the mask: inside zone z."""
        return [(tid, e.age, sum(1 << z for z, b in enumerate(e.bit) if b)) for tid, e in self.table.items()]

    def update(self, rows, t):
        if rows is None:
            return None
        t = float(t)
        by_id, new = {}, set()
        for r in rows:
            tid = int(r[4])
            if tid in by_id:
                raise ValueError(f"zones: track id {tid} appears twice in one frame")
            by_id[tid] = r
        for tid, r in by_id.items():                 # (dicts keep row order)
            if tid not in self.table:
                self.table[tid] = _Entry(int(r[5]), len(self.zones))
                new.add(tid)
        self.stats["max_table"] = max(self.stats["max_table"], len(self.table))
        events, dead, zeros = [], [], [0]
        for tid, e in self.table.items():
            r = by_id.get(tid)
            if r is None:
                e.age += 1
                if e.age >= self.max_age:
                    for z in range(len(self.zones)):
                        if e.bit[z]:
                            events.append((tid, e.cls, LOST, self.zone_names[z], t, e.t - e.enter[z]))
                            self._zone4[z][0] -= 1
                            self._zone4[z][3] += 1
                    dead.append(tid)
                continue
            c = anchor(r)
            if tid not in new:
                for k, (a, b) in enumerate(self._line2):
                    if self._lcls[k] not in (-1, e.cls):
                        continue
                    d = cross(e.point, c, a, b, zeros)
                    if d:
                        events.append((tid, e.cls, CROSS_FWD if d > 0 else CROSS_BACK, self.line_names[k], t, 0.0))
                        self._line2n[k][0 if d > 0 else 1] += 1
            for z, poly in enumerate(self._poly2):
                if self._zcls[z] not in (-1, e.cls):
                    continue
                now = inside(c, poly)
                if now == e.bit[z]:
                    self.stats["abandoned"] += e.streak[z] > 0
                    e.streak[z] = 0
                    continue
                e.streak[z] += 1
                if e.streak[z] < self._zmin[z]:
                    continue
                e.bit[z], e.streak[z] = now, 0
                if now:
                    e.enter[z] = t
                    events.append((tid, e.cls, ENTER, self.zone_names[z], t, 0.0))
                    self._zone4[z][0] += 1
                    self._zone4[z][1] += 1
                else:
                    events.append((tid, e.cls, EXIT, self.zone_names[z], t, t - e.enter[z]))
                    self._zone4[z][0] -= 1
                    self._zone4[z][2] += 1
            e.point, e.t, e.age = c, t, 0
        for tid in dead:
            del self.table[tid]
        self.stats["zero_orientations"] += zeros[0]
        return events


def _is_pair(g):
    """g is one (zones, lines) pair: two sequences holding only Zone / only Line objects."""
    try:
        zs, ls = g
        zs, ls = list(zs), list(ls)
    except (TypeError, ValueError):
        return False
    return all(isinstance(z, Zone) for z in zs) and all(isinstance(ln, Line) for ln in ls)


def stream_geometries(geometry, n_streams):
    """``geometry`` - one (zones, lines) pair for all streams, a ZoneMonitor (its geometry), or a list with one pair per stream -
    as a list of n_streams pairs; ValueError naming ``zones`` otherwise."""
    if isinstance(geometry, ZoneMonitor):
        geometry = geometry.geometry
    per = per_stream(geometry, n_streams, _is_pair, "zones: geometry is one (zones, lines) pair or a list of %d pairs, one per stream")
    return [(list(g[0]), list(g[1])) for g in per]


class DeviceZoneMonitor(TrackStage):
    """``ZoneMonitor`` for ``n_streams`` video streams with every table and counter in HBM: one launch advances the tables of all
    streams over the frames of a call.  ``geometry``: one (zones, lines) pair for all streams, or a list with one pair per
    stream; it travels to the device once, when the handle is made."""
    NAME = LIB = "zones"
    HOST = ZoneMonitor

    def __init__(self, geometry, max_age=30, n_streams=1):
        super().__init__(n_streams, max_age)
        self.geometry = stream_geometries(geometry, self.n_streams)
        self.packed = [pack_geometry(z, ln) for z, ln in self.geometry]

    def _settings(self, n_streams):
        return self.geometry[:n_streams], self.max_age, n_streams

    def host(self, stream=0):
        """A fresh ZoneMonitor of one stream's geometry and this max_age: the comparator."""
        z, ln = self.geometry[stream]
        return ZoneMonitor(z, ln, self.max_age)

    def _create(self, lib):
        return lib.yds_zones_create(self.n_streams, self.max_age)

    def _setup(self, lib, h):
        from . import _lib
        for s, g in enumerate(self.packed):
            _lib.check(lib.yds_zones_set_stream(h, s, _lib.ptr(g[0]), _lib.ptr(g[1]), _lib.ptr(g[2]), _lib.ptr(g[3]), len(g[2]),
                                                _lib.ptr(g[4]), _lib.ptr(g[5]), len(g[5])))

    def name_events(self, stream, ev6, evt2):
        """Event rows of one stream's frame as ZoneMonitor.update returns them."""
        zn, ln = self.packed[stream][6], self.packed[stream][7]
        return [(int(r[1]), int(r[2]), int(r[3]), (zn if r[3] <= LOST else ln)[int(r[4])], float(t[0]), float(t[1]))
                for r, t in zip(ev6, evt2)]

    def update_batch(self, frames_rows, stream_of, times):
        """Frames in the order given (a stream's frames in time order), frame f of stream ``stream_of[f]`` at time ``times[f]``;
        a frame whose rows are None is not seen.  Returns one event list per frame (None for a None frame)."""
        import ctypes as C
        import numpy as np
        from . import _lib
        live, rows6, first, sof, tm = self.pack(frames_rows, stream_of, times)
        out = [None] * len(frames_rows)
        if not live:
            return out
        # the most events the call can emit: every entry a frame can meet (the table before the call + the rows so far), at each
        # of its stream's zones and lines
        n, held, cap = len(live), {}, 1
        for k in range(n):
            s = int(sof[k])
            if s not in held:
                held[s] = self._table_count("tracks", s, 3)
            held[s] += int(first[k + 1] - first[k])
            cap += held[s] * (len(self.packed[s][2]) + len(self.packed[s][5]))
        ev6, evt2, m = np.zeros((cap, 6), np.int32), np.zeros((cap, 2), np.float64), C.c_int(0)
        _lib.check(_lib.load().yds_zones_update(self.handle, _lib.ptr(rows6), _lib.ptr(first), _lib.ptr(sof), _lib.ptr(tm), n, _lib.ptr(ev6),
                                                _lib.ptr(evt2), cap, C.byref(m)))
        per = [([], []) for _ in range(n)]
        for r, t in zip(ev6[:m.value], evt2[:m.value]):
            per[int(r[0])][0].append(r)
            per[int(r[0])][1].append(t)
        for k, f in enumerate(live):
            out[f] = self.name_events(int(sof[k]), *per[k])
        return out

    def counts(self, stream=0):
        """ZoneMonitor.counts() of one stream, read from the device."""
        import numpy as np
        from . import _lib
        g = self.packed[int(stream)]
        z4, l2 = np.zeros((max(len(g[2]), 1), 4), np.int32), np.zeros((max(len(g[5]), 1), 2), np.int32)
        _lib.check(_lib.load().yds_zones_get_counts(self.handle, int(stream), _lib.ptr(z4), _lib.ptr(l2)))
        return z4[:len(g[2])].tolist(), l2[:len(g[5])].tolist()

    def tracks(self, stream=0):
        """ZoneMonitor.tracks() of one stream, read from the device."""
        import numpy as np
        ids, ages, mask = self._read_table("tracks", stream, [(np.int32, ())] * 3)
        return list(zip(ids.tolist(), ages.tolist(), mask.view(np.uint32).tolist()))


as_device_zones = DeviceZoneMonitor.as_device      # (the name Pipeline.set_zones and callers import; track_stage.TrackStage.as_device is the rule)


class VisitorLog:
    """Host-side join of zone events with global ids: "distinct people through all the doors".

    ``groups``: dict group name -> list of (stream, zone name) pairs (a zone without a name goes by its index).  Per step,
    ``feed(events, identities)`` takes the zone events of every frame of the step (``last_zone_events()``) and the identity maps
    (``last_identities()``: per stream a dict track id -> global id, 0 = deferred).  A visit, keyed (stream, track id, zone),
    opens at ENTER and closes at EXIT or LOST; it carries the global id the track held, and an id of 0 is asked for again at
    every later feed while the visit is open."""

    def __init__(self, groups):
        self.groups = {g: [(int(s), z) for s, z in pairs] for g, pairs in groups.items()}
        self.open = {}                  # (stream, track id, zone) -> visit
        self.closed = []

    def feed(self, events, identities, stream_of=None):
        """events[f]: the event list of frame f (None: not seen) of stream stream_of[f] (default: frame f is stream f)."""
        for f, evs in enumerate(events):
            s = f if stream_of is None else int(stream_of[f])
            for tid, cls, kind, name, t, dwell in evs or []:
                if kind > LOST:
                    continue
                key = (s, tid, name)
                if kind == ENTER:
                    self.open[key] = dict(stream=s, track_id=tid, class_id=cls, zone=name, global_id=0, enter=t, exit=None, dwell=None,
                                          closed_by=None)
                elif key in self.open:
                    v = self.open[key]
                    self._resolve(v, identities)
                    v.update(exit=t, dwell=dwell, closed_by=KIND_NAMES[kind])
                    self.closed.append(self.open.pop(key))
        for v in self.open.values():
            self._resolve(v, identities)

    @staticmethod
    def _resolve(v, identities):
        if v["global_id"] == 0 and identities is not None and v["stream"] < len(identities):
            v["global_id"] = int((identities[v["stream"]] or {}).get(v["track_id"], 0))

    def visits(self, group):
        """The visits of a group, closed ones first in closing order, then the open ones (dwell None)."""
        pairs = set(self.groups[group])
        return [dict(v) for v in self.closed + list(self.open.values()) if (v["stream"], v["zone"]) in pairs]

    def distinct(self, group):
        """The set of distinct global ids seen in a group's zones (deferred ids that never resolved are left out)."""
        return {v["global_id"] for v in self.visits(group) if v["global_id"] > 0}
