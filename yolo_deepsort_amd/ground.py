"""Ground plane: floor-plan positions, speeds and a site-wide map.

Every camera gets a homography H from its image pixels to ONE floor plan; the tracker's rows then give, per person, a plan position
in quanta (``scale`` quanta per plan unit), a velocity, a speed and a distance travelled, and all cameras add to one site grid of the
heat map's five int64 layers.  The rules are written down in include/ydsort.h (the ground plane block); ``project``, ``GroundMap``
and ``render_view`` restate them in Python ints / numpy float64 and are the definition every device test (csrc/ground.hip,
``DeviceGroundMap``) compares against with exact equality: one floating-point step per point (``project``), integers after it.

Limits: the site grid counts per camera and track, so two cameras seeing one person credit twice (``site_people`` joins a step's
rows by global id instead); the foot point is the box's bottom centre, so an occluded foot lands too near; there is no lens
distortion model; the layers only ever grow (no decay).
"""

from __future__ import annotations

import math
from functools import partial

import numpy as np

from .heatmap import LAYERS, MAX_CELLS, check_alpha, check_lut, levels, render as _heat_render
from .track_stage import GridStage, as_int, check_max_age, per_stream

Q_LIMIT = 1 << 29                   # |px * scale| beyond this is off plane
MAX_WINDOW = 16                     # YDS_GROUND_MAX_WINDOW
MAX_EXTENT_Q = 1 << 22              # YDS_GROUND_MAX_EXTENT_Q: (max(gw, gh) + 2) * cell_q <= this
SAT = (1 << 31) - 1                 # vx, vy, speed saturate to +-SAT
OUTSIDE, OFF_PLANE = -1, -2


_as_int = partial(as_int, "ground")
_check_max_age = partial(check_max_age, "ground")


def _quanta(v, scale, what):
    q = float(v) * scale
    if not math.isfinite(q) or q != round(q):
        raise ValueError(f"ground: {what} {v!r} * scale {scale!r} is no integer")
    return int(round(q))


class GroundSpec:
    """One camera on the plan: ``H`` 3x3 float64 from image pixels to plan units, the plan's ``origin`` and ``cell`` edge in plan
    units, its grid of ``gw`` x ``gh`` cells, ``scale`` quanta per plan unit and the class counted (-1 = any).  origin * scale and
    cell * scale must be integers.  ValueError naming ground for what the device refuses."""

    def __init__(self, H, origin=(0.0, 0.0), cell=1.0, gw=1, gh=1, scale=1000, class_id=0):
        H = np.array(H, dtype=np.float64)
        if H.shape != (3, 3) or not np.isfinite(H).all():
            raise ValueError("ground: H must be a finite 3x3 matrix")
        self.H = H
        self.scale = float(scale)
        if not (0 < self.scale <= 1e9):
            raise ValueError(f"ground: scale {scale!r} outside (0, 1e9]")
        self.gw, self.gh, self.class_id = _as_int(gw, "gw"), _as_int(gh, "gh"), _as_int(class_id, "class_id")
        self.origin, self.cell = (float(origin[0]), float(origin[1])), float(cell)
        self.ox_q, self.oy_q = _quanta(origin[0], self.scale, "origin x"), _quanta(origin[1], self.scale, "origin y")
        self.cell_q = _quanta(cell, self.scale, "cell")
        if self.gw < 1 or self.gh < 1 or self.gw * self.gh > MAX_CELLS:
            raise ValueError(f"ground: a grid of {self.gh} x {self.gw} cells exceeds {MAX_CELLS}")
        if self.cell_q < 1 or (max(self.gw, self.gh) + 2) * self.cell_q > MAX_EXTENT_Q:
            raise ValueError(f"ground: cell_q {self.cell_q}: (max(gw, gh) + 2) * cell_q must lie in [1, 2^22]")
        if max(abs(self.ox_q), abs(self.oy_q)) > 1 << 30:
            raise ValueError("ground: origin outside +-2^30 quanta")
        if self.class_id < -1:
            raise ValueError(f"ground: class_id {self.class_id} (-1 = any class)")

    def plan(self):
        """What all streams of one map share."""
        return self.ox_q, self.oy_q, self.cell_q, self.gw, self.gh, self.scale

    def __repr__(self):
        return "GroundSpec(origin=%r, cell=%r, gw=%d, gh=%d, scale=%r, class_id=%d)" % (self.origin, self.cell, self.gw, self.gh, self.scale,
                                                                                         self.class_id)


def homography_from_points(image_pts, plan_pts):
    """H (3x3 float64, image to plan) from four or more correspondences by the normalised DLT, signed so that W > 0 at every given
    image point; ValueError when no sign does that (points on both sides of the horizon) or the set is degenerate.  Host only."""
    a, b = np.asarray(image_pts, dtype=np.float64), np.asarray(plan_pts, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape != b.shape or len(a) < 4 or not (np.isfinite(a).all() and np.isfinite(b).all()):
        raise ValueError("ground: homography_from_points needs two finite [n][2] arrays of n >= 4 points")

    def normalise(p):
        c = p.mean(axis=0)
        d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
        if not d > 0:
            raise ValueError("ground: homography_from_points: the points coincide")
        s = math.sqrt(2.0) / d
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])
    Ta, Tb = normalise(a), normalise(b)
    an = (Ta @ np.c_[a, np.ones(len(a))].T).T
    bn = (Tb @ np.c_[b, np.ones(len(b))].T).T
    A = np.zeros((2 * len(a), 9))
    for i, ((x, y, _), (X, Y, _)) in enumerate(zip(an, bn)):
        A[2 * i] = [-x, -y, -1, 0, 0, 0, X * x, X * y, X]
        A[2 * i + 1] = [0, 0, 0, -x, -y, -1, Y * x, Y * y, Y]
    _, sv, Vt = np.linalg.svd(A)
    if sv[-2] <= 1e-12 * sv[0]:
        raise ValueError("ground: homography_from_points: the points are degenerate (three on a line?)")
    H = np.linalg.inv(Tb) @ Vt[-1].reshape(3, 3) @ Ta
    H = H / np.sqrt((H ** 2).sum())
    W = H[2, 0] * a[:, 0] + H[2, 1] * a[:, 1] + H[2, 2]
    if (W < 0).all():
        H, W = -H, -W
    if not (W > 0).all():
        raise ValueError("ground: homography_from_points: W changes sign over the image points (they straddle the horizon)")
    return H


def project(H, u, v, scale):
    """Rule 2, the one floating-point step, for arrays of image points: (on, qx, qy) with ``on`` False off plane (qx = qy = 0
    there), qx / qy int64."""
    H = np.asarray(H, dtype=np.float64)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    s = np.float64(scale)
    with np.errstate(all="ignore"):
        X = (H[0, 0] * u + H[0, 1] * v) + H[0, 2]
        Y = (H[1, 0] * u + H[1, 1] * v) + H[1, 2]
        W = (H[2, 0] * u + H[2, 1] * v) + H[2, 2]
        px, py = X / W, Y / W
        sx, sy = px * s, py * s
        on = (W > 0) & np.isfinite(X) & np.isfinite(Y) & np.isfinite(W) & np.isfinite(px) & np.isfinite(py) & np.isfinite(sx) & np.isfinite(sy)
        on = on & (np.abs(sx) <= Q_LIMIT) & (np.abs(sy) <= Q_LIMIT)
        qx = np.where(on, np.rint(np.where(on, sx, 0.0)), 0.0).astype(np.int64)
        qy = np.where(on, np.rint(np.where(on, sy, 0.0)), 0.0).astype(np.int64)
    return on, qx, qy


def _sat(v):
    return max(-SAT, min(SAT, v))


def _us(dt):
    return int(np.rint(np.float64(dt) * 1e6))        # half to even, as llrint


def stream_specs(specs, n_streams):
    """``specs`` - one GroundSpec for all streams or a list with one GroundSpec or None (no spec: skipped) per stream - as a list of
    n_streams; all specs must share one plan.  ValueError naming ground otherwise."""
    if isinstance(specs, GroundMap):
        specs = specs.specs
    per = per_stream(specs, n_streams, lambda s: isinstance(s, GroundSpec),
                     "ground: specs is one GroundSpec or a list of %d, one (or None) per stream", or_none=True)
    given = [s for s in per if s is not None]
    if not given:
        raise ValueError("ground: no stream has a spec")
    if any(s.plan() != given[0].plan() for s in given):
        raise ValueError("ground: the specs of one map must share origin, cell, grid size and scale (one plan)")
    return per


def _check_window(k):
    if isinstance(k, bool) or int(k) != k or not 1 <= k <= MAX_WINDOW:
        raise ValueError(f"ground: speed_window {k!r} is no integer in [1, {MAX_WINDOW}]")
    return int(k)


class GroundMap:
    """The ground plane of ``len(specs)`` streams on the host: one site grid, one table per stream.  ``update(stream, rows, t)``
    takes one processed frame (rows [n][6] = x1, y1, x2, y2, track id, class; None: the tracker was not called, nothing is touched;
    zero rows age every entry) and returns the records int32 [m][8] = id, class, qx, qy, vx, vy, speed, cell of its counted rows
    (a stream without a spec: always [0][8])."""

    def __init__(self, specs, max_age=30, speed_window=8, n_streams=None):
        if isinstance(specs, GroundMap):
            specs = specs.specs
        if isinstance(specs, GroundSpec) and n_streams is None:
            n_streams = 1
        self.specs = stream_specs(specs, len(specs) if n_streams is None else int(n_streams))
        self.n_streams = len(self.specs)
        self.max_age, self.K = _check_max_age(max_age), _check_window(speed_window)
        self.ox_q, self.oy_q, self.cell_q, self.gw, self.gh, self.scale = next(s for s in self.specs if s is not None).plan()
        # what the tests assert about their own scenes
        self.stats = dict(off_plane_rows=0, outside_rows=0, gap_sightings=0, ring_wraps=0, ignored_rows=0, max_table=0, restarts=0,
                          multi_camera_cells=0, consecutive=0, no_speed=0)
        self._cell_streams = {}
        self.reset()

    def reset(self, stream=None):
        """stream: an empty table for it (the site grid is every stream's and stands); None: all tables and a zero grid."""
        if stream is None:
            self._layers = [[0] * (self.gw * self.gh) for _ in LAYERS]
            self.tables = [{} for _ in range(self.n_streams)]
        else:
            self.tables[int(stream)] = {}

    def cell_of(self, qx, qy):
        cx, cy = (qx - self.ox_q) // self.cell_q, (qy - self.oy_q) // self.cell_q
        return cy * self.gw + cx if 0 <= cx < self.gw and 0 <= cy < self.gh else OUTSIDE

    def update(self, stream, rows, t):
        if rows is None:
            return None
        sp, table = self.specs[stream], self.tables[stream]
        out = []
        if sp is None:
            return np.zeros((0, 8), np.int32)
        t = float(t)
        presence, visits, dwell, flow_x, flow_y = self._layers
        seen, ids = {}, set()
        for r in rows:
            tid = int(r[4])
            if tid in ids:
                raise ValueError(f"ground: track id {tid} appears twice in one frame")
            ids.add(tid)
            if sp.class_id not in (-1, int(r[5])):
                self.stats["ignored_rows"] += 1
                continue
            seen[tid] = r
        if seen:
            rr = np.array([[int(r[0]), int(r[2]), int(r[3])] for r in seen.values()], dtype=np.float64)
            on_a, qx_a, qy_a = project(sp.H, 0.5 * (rr[:, 0] + rr[:, 1]), rr[:, 2], self.scale)
        for k, (tid, r) in enumerate(seen.items()):      # (dicts keep row order: unknown ids register at the end in row order)
            on, qx, qy = bool(on_a[k]), int(qx_a[k]), int(qy_a[k])
            cell = self.cell_of(qx, qy) if on else OFF_PLANE
            self.stats["off_plane_rows"] += not on
            self.stats["outside_rows"] += cell == OUTSIDE
            e = table.get(tid)
            if e is None:
                e = table[tid] = dict(age=0, cell=OUTSIDE, t=t, travelled=0, ring=[])
            else:
                self.stats["gap_sightings"] += e["age"] > 0
            fresh, prev, ring = e["age"] == 0, e["cell"], e["ring"]
            vx = vy = speed = 0
            if fresh and prev >= 0:
                dwell[prev] += max(0, _us(t - e["t"]))
            if on:
                if fresh and ring:
                    dx, dy = qx - ring[-1][0], qy - ring[-1][1]
                    e["travelled"] += math.isqrt(dx * dx + dy * dy)
                    if cell >= 0:
                        flow_x[cell] += dx
                        flow_y[cell] += dy
                    self.stats["consecutive"] += 1
                else:
                    self.stats["restarts"] += bool(ring)
                    del ring[:]
                if len(ring) == self.K:
                    del ring[0]
                    self.stats["ring_wraps"] += 1
                ring.append((qx, qy, t))
                dx, dy, dt_us = qx - ring[0][0], qy - ring[0][1], _us(t - ring[0][2])
                if dt_us > 0:
                    vx, vy = _sat(dx * 1000000 // dt_us), _sat(dy * 1000000 // dt_us)
                    speed = _sat(math.isqrt(dx * dx + dy * dy) * 1000000 // dt_us)
                else:
                    speed = -1
                    self.stats["no_speed"] += 1
                if cell >= 0:
                    visits[cell] += cell != prev
                    presence[cell] += 1
                    self._cell_streams.setdefault(cell, set()).add(stream)
            else:
                del ring[:]
            e["age"], e["cell"], e["t"] = 0, cell, t
            out.append([tid, int(r[5]), qx, qy, vx, vy, speed, cell])
        self.stats["max_table"] = max(self.stats["max_table"], len(table))
        self.stats["multi_camera_cells"] = sum(1 for v in self._cell_streams.values() if len(v) >= 2)
        for tid in [k for k in table if k not in seen]:
            table[tid]["age"] += 1
            if table[tid]["age"] > self.max_age:
                del table[tid]
        return np.array(out, dtype=np.int32).reshape(-1, 8)

    def layer(self, name):
        """One site layer as int64 [gh, gw]."""
        if name not in LAYERS:
            raise ValueError(f"ground: layer {name!r} is not one of {LAYERS}")
        return np.array(self._layers[LAYERS.index(name)], dtype=np.int64).reshape(self.gh, self.gw)

    def layers(self):
        """All five site layers, int64 [5, gh, gw] in the order of LAYERS."""
        return np.array(self._layers, dtype=np.int64).reshape(5, self.gh, self.gw)

    def max(self, name):
        return int(self.layer(name).max())

    def tracks(self, stream=0):
        """[(track id, age, cell, travelled, t_last, ((qx, qy, t), ...) oldest first), ...] in table order."""
        return [(tid, e["age"], e["cell"], e["travelled"], e["t"], tuple(e["ring"])) for tid, e in self.tables[stream].items()]


def view_field(spec, h, w, level):
    """Rule 4 for every pixel of an h x w view of camera ``spec``: (k int64 [h, w] in 0..255, on bool [h, w] - the pixel's plan
    point exists -, near bool [h, w] - on and no more than half a cell outside the grid, qx, qy)."""
    L = np.asarray(level, dtype=np.int64)
    if L.shape != (spec.gh, spec.gw):
        raise ValueError("ground: a level grid of %s for a plan of %d x %d cells" % (L.shape, spec.gh, spec.gw))
    u, v = np.meshgrid(np.arange(w, dtype=np.float64) + 0.5, np.arange(h, dtype=np.float64) + 0.5)
    on, qx, qy = project(spec.H, u, v, spec.scale)
    a = ((qx - spec.ox_q) * 256) // spec.cell_q - 128
    b = ((qy - spec.oy_q) * 256) // spec.cell_q - 128
    i0, fx, j0, fy = a >> 8, a & 255, b >> 8, b & 255
    near = on & (i0 >= -1) & (i0 < spec.gw) & (j0 >= -1) & (j0 < spec.gh)
    ia, ib = np.clip(i0, 0, spec.gw - 1), np.clip(i0 + 1, 0, spec.gw - 1)
    ja, jb = np.clip(j0, 0, spec.gh - 1), np.clip(j0 + 1, 0, spec.gh - 1)
    num = (256 - fy) * ((256 - fx) * L[ja, ia] + fx * L[ja, ib]) + fy * ((256 - fx) * L[jb, ia] + fx * L[jb, ib])
    k = np.where(near, (num >> 16) // 257, 0)
    return k, on, near, qx, qy


def render_view(img, spec, grid, vmax=0, lut=None, alpha=128, inplace=False):
    """The host form, and the reference of the device form: ``img`` uint8 [H, W, 3] of camera ``spec`` with the colour map of
    ``grid`` (one site layer, int64 [gh, gw]) blended onto its floor; a copy unless inplace.  Pixels off plane, more than half a
    cell outside the grid or with k == 0 keep the picture; the others become (alpha * lut[k] + (256 - alpha) * src + 128) >> 8."""
    if not isinstance(img, np.ndarray) or img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError("ground: img must be uint8 [H, W, 3]")
    lut, alpha = check_lut(lut), check_alpha(alpha)
    k = view_field(spec, img.shape[0], img.shape[1], levels(grid, vmax))[0]
    out = img if inplace else img.copy()
    mix = (alpha * lut.astype(np.int64)[k] + (256 - alpha) * img.astype(np.int64) + 128) >> 8
    np.copyto(out, mix.astype(np.uint8), where=(k > 0)[:, :, None])
    return out


def render_plan(grid, cell_px=8, vmax=0, lut=None, alpha=256, canvas=None):
    """A site layer on a plan canvas of cell_px pixels per cell (black unless given): heatmap.render at cell = cell_px."""
    g = np.asarray(grid)
    if canvas is None:
        canvas = np.zeros((g.shape[0] * cell_px, g.shape[1] * cell_px, 3), np.uint8)
    return _heat_render(canvas, g, cell_px, vmax=vmax, lut=lut, alpha=alpha)


def site_people(rows_by_stream, ids_by_stream):
    """The host join of one step: ``rows_by_stream[s]`` the ground records int32 [m][8] of stream s (None: none),
    ``ids_by_stream[s]`` its (track id, global id) pairs (or a dict; global id 0 = not resolved yet).  One entry per global id, as
    zones.VisitorLog keeps one per person: {global id: dict(qx, qy, speed, streams, tracks)} with (qx, qy) the floor mean of its
    cameras' on-plane points - overlapping views do not count a person twice - and speed the floor mean of its cameras' known
    speeds (-1: none known)."""
    people = {}
    for s, rows in enumerate(rows_by_stream):
        if rows is None or not len(rows):
            continue
        ids = ids_by_stream[s]
        gid_of = dict(ids) if not isinstance(ids, dict) else ids
        for r in np.asarray(rows).reshape(-1, 8):
            gid = int(gid_of.get(int(r[0]), 0))
            if gid <= 0 or int(r[7]) == OFF_PLANE:
                continue
            p = people.setdefault(gid, dict(pts=[], speeds=[], streams=[], tracks=[]))
            p["pts"].append((int(r[2]), int(r[3])))
            p["streams"].append(s)
            p["tracks"].append((s, int(r[0])))
            if int(r[6]) >= 0:
                p["speeds"].append(int(r[6]))
    out = {}
    for gid, p in sorted(people.items()):
        n = len(p["pts"])
        out[gid] = dict(qx=sum(x for x, _ in p["pts"]) // n, qy=sum(y for _, y in p["pts"]) // n,
                        speed=sum(p["speeds"]) // len(p["speeds"]) if p["speeds"] else -1, streams=p["streams"], tracks=p["tracks"])
    return out


class DeviceGroundMap(GridStage):
    """``GroundMap`` with the site grid and every table in HBM: one launch advances all streams over the frames of a call,
    ``render_plan`` / ``render_view`` blend a site layer into a canvas / into camera frames resident in HBM.  ``specs``: one
    GroundSpec for all streams, or a list with one (or None) per stream."""
    NAME = LIB = "ground"
    HOST = GroundMap
    LAYERS = LAYERS

    def __init__(self, specs, max_age=30, speed_window=8, n_streams=None):
        if n_streams is None:
            n_streams = 1 if isinstance(specs, GroundSpec) else len(specs.specs if isinstance(specs, GroundMap) else specs)
        super().__init__(n_streams, max_age)
        self.K = _check_window(speed_window)
        self.specs = stream_specs(specs, self.n_streams)
        self.plan = next(s for s in self.specs if s is not None)
        self.gw, self.gh = self.plan.gw, self.plan.gh

    def _settings(self, n_streams):
        return self.specs[:n_streams], self.max_age, self.K, n_streams

    def _what(self):
        return "a map"

    def host(self):
        """A fresh GroundMap of these specs, max_age and speed_window: the comparator."""
        return GroundMap(self.specs, self.max_age, self.K)

    def _create(self, lib):
        p = self.plan
        return lib.yds_ground_create(self.n_streams, self.max_age, self.K, p.ox_q, p.oy_q, p.cell_q, p.gw, p.gh, p.scale)

    def _setup(self, lib, h):
        from . import _lib
        for s, sp in enumerate(self.specs):
            if sp is not None:
                _lib.check(lib.yds_ground_set_stream(h, s, _lib.ptr(np.ascontiguousarray(sp.H.reshape(9))), sp.class_id))

    def update_batch(self, frames_rows, stream_of, times):
        """Frames in the order given (a stream's frames in time order), frame f of stream ``stream_of[f]`` at time ``times[f]``;
        a frame whose rows are None is not seen.  Returns per frame its records int32 [m][8] (None for a None frame)."""
        import ctypes as C
        from . import _lib
        live, rows6, first, sof, tm = self.pack(frames_rows, stream_of, times)
        out = [None] * len(frames_rows)
        if not live:
            return out
        n = len(live)
        out8, first_out, m = np.zeros((max(len(rows6), 1), 8), np.int32), np.zeros(n + 1, np.int32), C.c_int(0)
        _lib.check(_lib.load().yds_ground_update(self.handle, _lib.ptr(rows6), _lib.ptr(first), _lib.ptr(sof), _lib.ptr(tm), n, _lib.ptr(out8),
                                                 _lib.ptr(first_out), len(out8), C.byref(m)))
        for k, f in enumerate(live):
            out[f] = out8[first_out[k]:first_out[k + 1]].copy()
        return out

    def layers(self):
        """GroundMap.layers(), read from the device."""
        from . import _lib
        out = np.zeros((5, self.gh, self.gw), np.int64)
        _lib.check(_lib.load().yds_ground_get_layers(self.handle, _lib.ptr(out), out.size))
        return out

    def layer(self, name):
        k = self._layer(name)
        return self.layers()[k]

    def max(self, name):
        """GroundMap.max(name), reduced on the device."""
        return self._read_max(name)

    def tracks(self, stream=0):
        """GroundMap.tracks(stream), read from the device."""
        i32, K = (np.int32, ()), self.K
        ids, ages, cells, lens, trav, tl, rxy, rt = self._read_table("tracks", stream, [i32, i32, i32, i32, (np.int64, ()), (np.float64, ()),
                                                                                        (np.int32, (K, 2)), (np.float64, (K,))])
        return [(int(ids[k]), int(ages[k]), int(cells[k]), int(trav[k]), float(tl[k]),
                 tuple((int(rxy[k, i, 0]), int(rxy[k, i, 1]), float(rt[k, i])) for i in range(int(lens[k])))) for k in range(len(ids))]

    def render_plan(self, canvas_dev, cell_px=8, layer="presence", vmax=0, alpha=256, lut=None):
        """canvas_dev: device pointer of a uint8 canvas of gh * cell_px x gw * cell_px x 3 bytes.  Bit-equal to
        heatmap.render(canvas, layer grid, cell_px, ...).  Synchronous."""
        from . import _lib
        _lib.check(_lib.load().yds_ground_render_plan(self.handle, canvas_dev, _as_int(cell_px, "cell_px"), self._layer(layer), _as_int(vmax, "vmax"),
                                                      _as_int(alpha, "alpha"), _lib.ptr(check_lut(lut))))

    def render_view(self, frames_dev, slots, stream_of, h, w, layer="presence", vmax=0, alpha=128, lut=None, n_frames=None):
        """frames_dev: device pointer of uint8 frames h*w*3 bytes apart; frame slots[i] is a picture of camera stream_of[i] and takes
        the site layer onto its floor.  Slots must be distinct and inside [0, n_frames) (default: max slot + 1).  Bit-equal to
        render_view() with that stream's spec.  Synchronous."""
        self._render("render_view", frames_dev, slots, stream_of, h, w, layer, vmax, alpha, lut, n_frames)

    @classmethod
    def _from_host(cls, x, n_streams, max_age):
        if isinstance(x, GroundMap):
            if x.n_streams != n_streams:
                raise ValueError(f"ground: a GroundMap of {x.n_streams} streams for {n_streams} streams")
            return cls(x.specs, x.max_age, x.K, n_streams)
        return cls(x, max_age, n_streams=n_streams)


as_device_ground = DeviceGroundMap.as_device      # (the name Pipeline.set_ground and callers import; track_stage.TrackStage.as_device is the rule)
