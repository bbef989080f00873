"""Heat maps: where people stand, walk and linger in a camera's view.

Per stream a grid of square cells over the frame and five int64 layers - presence (sightings), visits (arrivals in a cell),
dwell_us (microseconds spent), flow_x / flow_y (summed moves in doubled pixels) - fed by the tracker's rows, and a renderer that
blends a colour map of one layer into a frame as a bilinear field between cell centres.  The rules are written down in
include/ydsort.h (the heat maps block); ``HeatMap``, ``levels`` and ``render`` restate them in Python ints / numpy int64 and are
the definition every device test (csrc/heatmap.hip, ``DeviceHeatMap``) compares against with exact equality: everything is
integer arithmetic except one double subtraction and one double product per dwell credit.

Limits: the layers only ever grow (no decay: ``reset`` or a fresh map starts a new period); cells are squares of image pixels
(the floor-plan form is ground.py); ``VideoDetector.detect()`` has no heat map; ``detect_streams`` accumulates on the device but leaves rendering
to the caller (``render`` on the host) - the device render is for callers who keep their frames in HBM.
"""

from __future__ import annotations

import numpy as np

from .zones import anchor

CELLS = (4, 8, 16, 32, 64, 128)     # allowed cell edges in pixels
MAX_CELLS = 65536                   # YDS_HEATMAP_MAX_CELLS: gw * gh <= this
LAYERS = ("presence", "visits", "dwell_us", "flow_x", "flow_y")
RENDERABLE = LAYERS[:3]
VMAX_LIMIT = 1 << 47                # YDS_HEATMAP_VMAX_LIMIT: a level is (v * 65535) // vmax in int64


def _as_int(v, what):
    if isinstance(v, (bool, float)) and int(v) != v or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"heatmap: {what} {v!r} is no integer")
    return int(v)


class HeatSpec:
    """The grid of one stream: frames of h x w pixels, square cells of ``cell`` pixels (the last column / row may be partial),
    rows of class ``class_id`` counted (-1 = any class).  ValueError naming heatmap for what the device refuses."""

    def __init__(self, h, w, cell=16, class_id=0):
        self.h, self.w, self.cell, self.class_id = _as_int(h, "h"), _as_int(w, "w"), _as_int(cell, "cell"), _as_int(class_id, "class_id")
        if self.h < 1 or self.w < 1:
            raise ValueError(f"heatmap: a frame of {self.h} x {self.w}")
        if self.cell not in CELLS:
            raise ValueError(f"heatmap: cell {self.cell} is not one of {CELLS}")
        if self.class_id < -1:
            raise ValueError(f"heatmap: class_id {self.class_id} (-1 = any class)")
        self.gw, self.gh = -(-self.w // self.cell), -(-self.h // self.cell)
        if self.gw * self.gh > MAX_CELLS:
            raise ValueError(f"heatmap: a grid of {self.gh} x {self.gw} cells exceeds {MAX_CELLS}")

    def astuple(self):
        return self.h, self.w, self.cell, self.class_id

    def __eq__(self, other):
        return isinstance(other, HeatSpec) and self.astuple() == other.astuple()

    def __hash__(self):
        return hash(self.astuple())

    def __repr__(self):
        return "HeatSpec(h=%d, w=%d, cell=%d, class_id=%d)" % self.astuple()


def _check_max_age(max_age):
    if isinstance(max_age, bool) or int(max_age) != max_age or max_age < 1:
        raise ValueError(f"heatmap: max_age {max_age!r} is no integer >= 1")
    return int(max_age)


class HeatMap:
    """The heat map of ONE stream on the host.  ``update(rows, t)`` takes one processed frame (rows [n][6] = x1, y1, x2, y2, track
    id, class; ``rows=None``: the tracker was not called, nothing is touched; zero rows age every entry) and returns the number
    of rows it counted (rows of the spec's class).  An id twice in one frame raises ValueError."""

    def __init__(self, spec, max_age=30):
        if not isinstance(spec, HeatSpec):
            raise ValueError(f"heatmap: {spec!r} is no HeatSpec")
        self.spec, self.max_age = spec, _check_max_age(max_age)
        self.reset()
        # what the tests assert about their own scenes
        self.stats = dict(multi_hit_cells=0, outside_rows=0, returned=0, gap_sightings=0, cell_changes=0, stays=0, ignored_rows=0,
                          dwell_credits=0, from_outside=0, clamped_dwell=0, max_table=0)
        self._retired = set()

    def clone(self):
        """A fresh map of the same spec and max_age."""
        return HeatMap(self.spec, self.max_age)

    def reset(self):
        n = self.spec.gw * self.spec.gh
        self._layers = [[0] * n for _ in LAYERS]
        self.table = {}                              # track id -> [age, cell, t, (Fx, Fy)], in insertion order

    def cell_of(self, F):
        """The cell of a doubled foot point, -1 outside the grid."""
        c2 = 2 * self.spec.cell
        cx, cy = F[0] // c2, F[1] // c2
        return cy * self.spec.gw + cx if 0 <= cx < self.spec.gw and 0 <= cy < self.spec.gh else -1

    def update(self, rows, t):
        if rows is None:
            return None
        t = float(t)
        presence, visits, dwell, flow_x, flow_y = self._layers
        seen, ids, hits = {}, set(), {}
        for r in rows:
            tid = int(r[4])
            if tid in ids:
                raise ValueError(f"heatmap: track id {tid} appears twice in one frame")
            ids.add(tid)
            if self.spec.class_id not in (-1, int(r[5])):
                self.stats["ignored_rows"] += 1
                continue
            seen[tid] = anchor(r)
        for tid, F in seen.items():                  # (dicts keep row order: unknown ids register at the end in row order)
            cell = self.cell_of(F)
            self.stats["outside_rows"] += cell < 0
            e = self.table.get(tid)
            if e is not None:
                age, prev, t_last, F_prev = e
                if age == 0 and prev >= 0:
                    us = round((t - t_last) * 1e6)
                    self.stats["clamped_dwell"] += us < 0
                    self.stats["dwell_credits"] += 1
                    dwell[prev] += max(0, us)
                if age == 0 and cell >= 0:
                    flow_x[cell] += F[0] - F_prev[0]
                    flow_y[cell] += F[1] - F_prev[1]
                if cell >= 0 and cell != prev:
                    visits[cell] += 1
                    self.stats["cell_changes"] += 1
                    self.stats["from_outside"] += prev < 0
                self.stats["gap_sightings"] += age > 0
                self.stats["stays"] += age == 0 and cell >= 0 and cell == prev
            else:
                if cell >= 0:
                    visits[cell] += 1
                if tid in self._retired:
                    self.stats["returned"] += 1
                    self._retired.discard(tid)
            if cell >= 0:
                presence[cell] += 1
                hits[cell] = hits.get(cell, 0) + 1
            self.table[tid] = [0, cell, t, F]
        self.stats["multi_hit_cells"] += sum(1 for v in hits.values() if v >= 2)
        self.stats["max_table"] = max(self.stats["max_table"], len(self.table))
        for tid in [k for k in self.table if k not in seen]:
            self.table[tid][0] += 1
            if self.table[tid][0] > self.max_age:
                del self.table[tid]
                self._retired.add(tid)
        return len(seen)

    def layer(self, name):
        """One layer as int64 [gh, gw]."""
        if name not in LAYERS:
            raise ValueError(f"heatmap: layer {name!r} is not one of {LAYERS}")
        return np.array(self._layers[LAYERS.index(name)], dtype=np.int64).reshape(self.spec.gh, self.spec.gw)

    def layers(self):
        """All five layers, int64 [5, gh, gw] in the order of LAYERS."""
        return np.array(self._layers, dtype=np.int64).reshape(5, self.spec.gh, self.spec.gw)

    def max(self, name):
        return int(self.layer(name).max())

    def tracks(self):
        """[(track id, age, cell, Fx, Fy, t), ...] in table order."""
        return [(tid, e[0], e[1], e[3][0], e[3][1], e[2]) for tid, e in self.table.items()]


def levels(grid, vmax=0):
    """Per cell (min(max(v, 0), vmax) * 65535) // vmax as int64 in 0..65535; vmax = 0: the grid's maximum, 1 for a grid without
    a positive value.  vmax outside [1, 2^47] raises ValueError, and so does a reduced maximum above it."""
    g = np.asarray(grid, dtype=np.int64)
    vmax = _as_int(vmax, "vmax")
    if vmax == 0:
        vmax = max(int(g.max()), 1)
        if vmax > VMAX_LIMIT:
            raise ValueError(f"heatmap: the layer's maximum {vmax} exceeds vmax's limit 2^47")
    elif vmax < 1 or vmax > VMAX_LIMIT:
        raise ValueError(f"heatmap: vmax {vmax} outside [1, 2^47] (0 = the layer's maximum)")
    return (np.clip(g, 0, vmax) * 65535) // vmax


def lut_heat():
    """The built-in colour map, uint8 [256][3] as R, G, B: black over red and yellow to white, from an integer formula."""
    k = np.arange(256, dtype=np.int64)
    return np.stack([np.clip(3 * k, 0, 255), np.clip(3 * k - 255, 0, 255), np.clip(3 * k - 510, 0, 255)], axis=1).astype(np.uint8)


def check_lut(lut):
    lut = lut_heat() if lut is None else np.asarray(lut)
    if lut.shape != (256, 3) or lut.dtype != np.uint8:
        raise ValueError("heatmap: lut must be uint8 [256][3], got %s %s" % (lut.dtype, lut.shape))
    return np.ascontiguousarray(lut)


def check_alpha(alpha):
    alpha = _as_int(alpha, "alpha")
    if alpha < 1 or alpha > 256:
        raise ValueError(f"heatmap: alpha {alpha} outside [1, 256]")
    return alpha


def field(level, h, w, cell):
    """k [h, w] in 0..255 of a level grid: the bilinear field between cell centres, edge cells continued outwards."""
    L = np.asarray(level, dtype=np.int64)
    gh, gw = L.shape
    c = int(cell)

    def axis(n, g):
        U = 2 * np.arange(n, dtype=np.int64) + 1 - c
        i0 = U // (2 * c)
        return np.clip(i0, 0, g - 1), np.clip(i0 + 1, 0, g - 1), U - 2 * c * i0
    ia, ib, fx = axis(w, gw)
    ja, jb, fy = axis(h, gh)
    fx, fy = fx[None, :], fy[:, None]
    num = ((2 * c - fx) * (2 * c - fy) * L[ja][:, ia] + fx * (2 * c - fy) * L[ja][:, ib]
           + (2 * c - fx) * fy * L[jb][:, ia] + fx * fy * L[jb][:, ib])
    return num // (4 * c * c * 257)


def render(img, grid, cell, vmax=0, lut=None, alpha=128, inplace=False):
    """The host form, and the reference of the device form: ``img`` uint8 [H, W, 3] with the colour map of ``grid`` (one layer,
    int64 [ceil(H / cell), ceil(W / cell)]) blended in; a copy unless inplace.  Pixels whose field value k is 0 keep the picture;
    the others become (alpha * lut[k] + (256 - alpha) * src + 128) >> 8 per byte (the LUT's bytes as they land in memory: reverse
    its columns for B, G, R frames)."""
    if not isinstance(img, np.ndarray) or img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError("heatmap: img must be uint8 [H, W, 3]")
    h, w = img.shape[:2]
    cell = _as_int(cell, "cell")
    if cell not in CELLS:
        raise ValueError(f"heatmap: cell {cell} is not one of {CELLS}")
    g = np.asarray(grid)
    if g.shape != (-(-h // cell), -(-w // cell)):
        raise ValueError("heatmap: a grid of %s for a frame of %d x %d at cell %d" % (g.shape, h, w, cell))
    lut, alpha = check_lut(lut), check_alpha(alpha)
    k = field(levels(g, vmax), h, w, cell)
    out = img if inplace else img.copy()
    mix = (alpha * lut.astype(np.int64)[k] + (256 - alpha) * img.astype(np.int64) + 128) >> 8
    np.copyto(out, mix.astype(np.uint8), where=(k > 0)[:, :, None])
    return out


def stream_specs(specs, n_streams):
    """``specs`` - one HeatSpec for all streams, a HeatMap (its spec) or a list with one HeatSpec per stream - as a list of
    n_streams specs; ValueError naming heatmap otherwise."""
    if isinstance(specs, HeatMap):
        specs = specs.spec
    if isinstance(specs, HeatSpec):
        return [specs] * n_streams
    try:
        per = list(specs)
    except TypeError:
        per = None
    if per is None or len(per) != n_streams or not all(isinstance(s, HeatSpec) for s in per):
        raise ValueError(f"heatmap: specs is one HeatSpec or a list of {n_streams}, one per stream")
    return per


class DeviceHeatMap:
    """``HeatMap`` for ``n_streams`` video streams with every layer and table in HBM: one launch advances the maps of all streams
    over the frames of a call, and ``render`` blends a layer into frames that are resident in HBM.  ``specs``: one HeatSpec for
    all streams, or a list with one per stream."""

    def __init__(self, specs, max_age=30, n_streams=1):
        self.n_streams = int(n_streams)
        if self.n_streams < 1:
            raise ValueError(f"heatmap: {n_streams} streams")
        self.max_age = _check_max_age(max_age)
        self.specs = stream_specs(specs, self.n_streams)
        self._h = None

    def host(self, stream=0):
        """A fresh HeatMap of one stream's spec and this max_age: the comparator."""
        return HeatMap(self.specs[stream], self.max_age)

    @property
    def handle(self):
        """The yds_heatmap handle, created (and its grids allocated) on first use."""
        if self._h is None:
            from . import _lib
            _lib.init()
            lib = _lib.load()
            h = _lib.check_ptr(lib.yds_heatmap_create(self.n_streams, self.max_age))
            try:
                for s, sp in enumerate(self.specs):
                    _lib.check(lib.yds_heatmap_set_stream(h, s, sp.h, sp.w, sp.cell, sp.class_id))
            except Exception:
                lib.yds_heatmap_destroy(h)
                raise
            self._h = h
        return self._h

    def _stream(self, stream):
        s = int(stream)
        if s < 0 or s >= self.n_streams:
            raise ValueError(f"heatmap: stream {s} outside [0, {self.n_streams})")
        return s

    def update_batch(self, frames_rows, stream_of, times):
        """Frames in the order given (a stream's frames in time order), frame f of stream ``stream_of[f]`` at time ``times[f]``;
        a frame whose rows are None is not seen.  Returns per frame the number of rows counted (None for a None frame)."""
        from . import _lib
        live = [f for f in range(len(frames_rows)) if frames_rows[f] is not None]
        out = [None] * len(frames_rows)
        if not live:
            return out
        rows = [np.asarray(frames_rows[f], dtype=np.int64).reshape(-1, 6) if len(frames_rows[f]) else np.zeros((0, 6), np.int64) for f in live]
        if any(r.size and np.abs(r).max() >= 2 ** 31 for r in rows):
            raise ValueError("heatmap: a row value does not fit 32 bits")
        n = len(live)
        first = np.zeros(n + 1, np.int32)
        first[1:] = np.cumsum([len(r) for r in rows])
        rows6 = np.ascontiguousarray(np.concatenate(rows), dtype=np.int32)
        sof = np.ascontiguousarray([self._stream(stream_of[f]) for f in live], dtype=np.int32)
        tm = np.ascontiguousarray([times[f] for f in live], dtype=np.float64)
        counted = np.zeros(n, np.int32)
        _lib.check(_lib.load().yds_heatmap_update(self.handle, _lib.ptr(rows6), _lib.ptr(first), _lib.ptr(sof), _lib.ptr(tm), n,
                                                  _lib.ptr(counted)))
        for k, f in enumerate(live):
            out[f] = int(counted[k])
        return out

    def update(self, stream, rows, t):
        """One frame of one stream: ``HeatMap.update(rows, t)`` (None in, None out, nothing touched)."""
        return self.update_batch([rows], [stream], [t])[0]

    def layers(self, stream=0):
        """HeatMap.layers() of one stream, read from the device."""
        from . import _lib
        sp = self.specs[self._stream(stream)]
        out = np.zeros((5, sp.gh, sp.gw), np.int64)
        _lib.check(_lib.load().yds_heatmap_get_layers(self.handle, int(stream), _lib.ptr(out), out.size))
        return out

    def layer(self, stream, name):
        if name not in LAYERS:
            raise ValueError(f"heatmap: layer {name!r} is not one of {LAYERS}")
        return self.layers(stream)[LAYERS.index(name)]

    def max(self, stream, name):
        """HeatMap.max(name) of one stream, reduced on the device."""
        import ctypes as C
        from . import _lib
        if name not in LAYERS:
            raise ValueError(f"heatmap: layer {name!r} is not one of {LAYERS}")
        v = C.c_int64(0)
        _lib.check(_lib.load().yds_heatmap_get_max(self.handle, self._stream(stream), LAYERS.index(name), C.byref(v)))
        return int(v.value)

    def tracks(self, stream=0):
        """HeatMap.tracks() of one stream, read from the device."""
        import ctypes as C
        from . import _lib
        lib, n, s = _lib.load(), C.c_int(0), self._stream(stream)
        _lib.check(lib.yds_heatmap_get_tracks(self.handle, s, None, None, None, None, None, 1 << 30, C.byref(n)))
        m = max(n.value, 1)
        ids, ages, cells, xy, t = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 2), np.int32), np.zeros(m)
        _lib.check(lib.yds_heatmap_get_tracks(self.handle, s, _lib.ptr(ids), _lib.ptr(ages), _lib.ptr(cells), _lib.ptr(xy), _lib.ptr(t), m,
                                              C.byref(n)))
        return [(int(ids[k]), int(ages[k]), int(cells[k]), int(xy[k, 0]), int(xy[k, 1]), float(t[k])) for k in range(n.value)]

    def reset(self, stream=None):
        """Zero layers and an empty table for one stream, or all of them."""
        from . import _lib
        if self._h is not None:
            _lib.check(_lib.load().yds_heatmap_reset(self._h, -1 if stream is None else int(stream)))

    def render(self, frames_dev, slots, stream_of, h, w, layer="presence", vmax=0, alpha=128, lut=None, n_frames=None):
        """frames_dev: device pointer of uint8 frames h*w*3 bytes apart; frame slots[i] takes the grid of stream stream_of[i],
        whose spec must be of h x w.  Slots must be distinct and inside [0, n_frames) (default: max slot + 1).  Bit-equal to
        render() of the same layer; the LUT's bytes as they land in memory.  Synchronous."""
        from . import _lib
        slots_a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        sof = np.ascontiguousarray(stream_of, dtype=np.int32).reshape(-1)
        if len(slots_a) != len(sof):
            raise ValueError("heatmap: %d slots for %d streams" % (len(slots_a), len(sof)))
        if layer not in LAYERS:
            raise ValueError(f"heatmap: layer {layer!r} is not one of {LAYERS}")
        if len(slots_a) == 0:
            return
        n_src = int(slots_a.max()) + 1 if n_frames is None else int(n_frames)
        _lib.check(_lib.load().yds_heatmap_render(self.handle, frames_dev, n_src, _lib.ptr(slots_a), _lib.ptr(sof), len(slots_a), int(h), int(w),
                                                  LAYERS.index(layer), _as_int(vmax, "vmax"), _as_int(alpha, "alpha"), _lib.ptr(check_lut(lut))))

    def set_timing(self, on=True):
        from . import _lib
        _lib.check(_lib.load().yds_heatmap_set_timing(self.handle, 1 if on else 0))

    def last_us(self, what="update"):
        """Device time of the last timed update launch or render (levels + pixels) in microseconds (set_timing first)."""
        import ctypes as C
        from . import _lib
        if what not in ("update", "render"):
            raise ValueError("heatmap: last_us of 'update' or 'render'")
        us = C.c_float(0)
        _lib.check(_lib.load().yds_heatmap_last_us(self.handle, 0 if what == "update" else 1, C.byref(us)))
        return us.value

    def close(self):
        if self._h is not None:
            from . import _lib
            _lib.load().yds_heatmap_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def as_device_heatmap(x, n_streams, max_age=30):
    """``x`` (a DeviceHeatMap of at least n_streams streams, a HeatMap, one HeatSpec or a list of them) as a DeviceHeatMap;
    ValueError naming heatmap for anything else."""
    if isinstance(x, DeviceHeatMap):
        if x.n_streams < n_streams:
            raise ValueError(f"heatmap: a DeviceHeatMap of {x.n_streams} streams for {n_streams} streams")
        return x
    if isinstance(x, HeatMap):
        return DeviceHeatMap(x.spec, x.max_age, n_streams)
    return DeviceHeatMap(x, max_age, n_streams)
