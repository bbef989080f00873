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

from functools import partial

import numpy as np

from .track_stage import GridStage, as_int, check_max_age, per_stream
from .zones import anchor

CELLS = (4, 8, 16, 32, 64, 128)     # allowed cell edges in pixels
MAX_CELLS = 65536                   # YDS_HEATMAP_MAX_CELLS: gw * gh <= this
LAYERS = ("presence", "visits", "dwell_us", "flow_x", "flow_y")
RENDERABLE = LAYERS[:3]
VMAX_LIMIT = 1 << 47                # YDS_HEATMAP_VMAX_LIMIT: a level is (v * 65535) // vmax in int64


_as_int = partial(as_int, "heatmap")
_check_max_age = partial(check_max_age, "heatmap")


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
    return per_stream(specs, n_streams, lambda s: isinstance(s, HeatSpec), "heatmap: specs is one HeatSpec or a list of %d, one per stream")


class DeviceHeatMap(GridStage):
    """``HeatMap`` for ``n_streams`` video streams with every layer and table in HBM: one launch advances the maps of all streams
    over the frames of a call, and ``render`` blends a layer into frames that are resident in HBM.  ``specs``: one HeatSpec for
    all streams, or a list with one per stream."""
    NAME = LIB = "heatmap"
    HOST = HeatMap
    LAYERS = LAYERS

    def __init__(self, specs, max_age=30, n_streams=1):
        super().__init__(n_streams, max_age)
        self.specs = stream_specs(specs, self.n_streams)

    def _settings(self, n_streams):
        return self.specs[:n_streams], self.max_age, n_streams

    def host(self, stream=0):
        """A fresh HeatMap of one stream's spec and this max_age: the comparator."""
        return HeatMap(self.specs[stream], self.max_age)

    def _create(self, lib):
        return lib.yds_heatmap_create(self.n_streams, self.max_age)

    def _setup(self, lib, h):
        from . import _lib
        for s, sp in enumerate(self.specs):
            _lib.check(lib.yds_heatmap_set_stream(h, s, sp.h, sp.w, sp.cell, sp.class_id))

    def update_batch(self, frames_rows, stream_of, times):
        """Frames in the order given (a stream's frames in time order), frame f of stream ``stream_of[f]`` at time ``times[f]``;
        a frame whose rows are None is not seen.  Returns per frame the number of rows counted (None for a None frame)."""
        from . import _lib
        live, rows6, first, sof, tm = self.pack(frames_rows, stream_of, times)
        out = [None] * len(frames_rows)
        if not live:
            return out
        counted = np.zeros(len(live), np.int32)
        _lib.check(_lib.load().yds_heatmap_update(self.handle, _lib.ptr(rows6), _lib.ptr(first), _lib.ptr(sof), _lib.ptr(tm), len(live),
                                                  _lib.ptr(counted)))
        for k, f in enumerate(live):
            out[f] = int(counted[k])
        return out

    def layers(self, stream=0):
        """HeatMap.layers() of one stream, read from the device."""
        from . import _lib
        sp = self.specs[self._stream(stream)]
        out = np.zeros((5, sp.gh, sp.gw), np.int64)
        _lib.check(_lib.load().yds_heatmap_get_layers(self.handle, int(stream), _lib.ptr(out), out.size))
        return out

    def layer(self, stream, name):
        k = self._layer(name)
        return self.layers(stream)[k]

    def max(self, stream, name):
        """HeatMap.max(name) of one stream, reduced on the device."""
        return self._read_max(name, self._stream(stream))

    def tracks(self, stream=0):
        """HeatMap.tracks() of one stream, read from the device."""
        i32 = (np.int32, ())
        ids, ages, cells, xy, t = self._read_table("tracks", stream, [i32, i32, i32, (np.int32, (2,)), (np.float64, ())])
        return [(int(ids[k]), int(ages[k]), int(cells[k]), int(xy[k, 0]), int(xy[k, 1]), float(t[k])) for k in range(len(ids))]

    def render(self, frames_dev, slots, stream_of, h, w, layer="presence", vmax=0, alpha=128, lut=None, n_frames=None):
        """frames_dev: device pointer of uint8 frames h*w*3 bytes apart; frame slots[i] takes the grid of stream stream_of[i],
        whose spec must be of h x w.  Slots must be distinct and inside [0, n_frames) (default: max slot + 1).  Bit-equal to
        render() of the same layer; the LUT's bytes as they land in memory.  Synchronous."""
        self._render("render", frames_dev, slots, stream_of, h, w, layer, vmax, alpha, lut, n_frames)


as_device_heatmap = DeviceHeatMap.as_device      # (the name Pipeline.set_heatmap and callers import; track_stage.TrackStage.as_device is the rule)
