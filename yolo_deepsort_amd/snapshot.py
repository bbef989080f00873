"""Track snapshots: each track's best crop, kept and chosen on the device.

Per stream a table of tracks; every entry holds the best thumbnail seen of its track so far - uint8 RGB, 128 rows x 64 columns, the
ReID crop size - with its score, box and time.  A track that has not been seen for more than ``max_age`` of its stream's processed
frames closes into a per-stream archive ring, so the last picture of a person who has left stays readable.  The rules are written
down in include/ydsort.h (the snapshot block); ``resize_u8``, ``score_thumb`` and ``SnapshotBook`` restate them in numpy and Python
ints and are the definition every device test (csrc/snapshot.hip, ``DeviceSnapshotBook``) compares against with exact equality.

Limits: thumbnails are taken from the frames as they were handed over, BEFORE any output stage, so ``anonymize=`` does not mask them;
the box is the tracker's posterior box; ``VideoDetector.detect()`` has no snapshots; the score (sharpness of the resized crop,
discounted by the share of the box inside the frame) knows nothing about pose or occlusion.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from .track_stage import TrackStage, as_int, check_max_age, per_stream

THUMB_H, THUMB_W = 128, 64          # YDS_SNAP_H, YDS_SNAP_W
MAX_ARCHIVE = 4096                  # YDS_SNAP_MAX_ARCHIVE
BEST, CLOSED = 0, 1                 # YDS_SNAP_BEST, YDS_SNAP_CLOSED
F32 = np.float32


class SnapSpec:
    """What counts: ``class_id`` (None = every class; rows of another class are ignored entirely), the smallest visible box
    ``min_w`` x ``min_h`` that is a candidate, and ``archive``, the ring slots per stream (0: closed snapshots are dropped)."""

    def __init__(self, class_id=None, min_w=8, min_h=16, archive=32):
        self.class_id = None if class_id is None else as_int("snapshots", class_id, "class_id")
        self.min_w, self.min_h = as_int("snapshots", min_w, "min_w"), as_int("snapshots", min_h, "min_h")
        self.archive = as_int("snapshots", archive, "archive")
        if self.class_id is not None and self.class_id < 0:
            raise ValueError(f"snapshots: class_id {self.class_id} (None = every class)")
        if self.min_w < 1 or self.min_h < 1:
            raise ValueError(f"snapshots: min_w {self.min_w}, min_h {self.min_h} (both >= 1)")
        if not 0 <= self.archive <= MAX_ARCHIVE:
            raise ValueError(f"snapshots: archive {self.archive} outside [0, {MAX_ARCHIVE}]")

    def __repr__(self):
        return "SnapSpec(class_id=%r, min_w=%d, min_h=%d, archive=%d)" % (self.class_id, self.min_w, self.min_h, self.archive)


def stream_specs(specs, n_streams):
    """``specs`` - one SnapSpec for all streams or a list with one SnapSpec or None (off: skipped) per stream - as a list of
    n_streams; all specs share ``archive``.  ValueError naming snapshots otherwise."""
    if isinstance(specs, (SnapshotBook, DeviceSnapshotBook)):
        specs = specs.specs
    per = per_stream(specs, n_streams, lambda s: isinstance(s, SnapSpec),
                     "snapshots: specs is one SnapSpec or a list of %d, one (or None) per stream", or_none=True)
    given = [s for s in per if s is not None]
    if not given:
        raise ValueError("snapshots: no stream has a spec")
    if any(s.archive != given[0].archive for s in given):
        raise ValueError("snapshots: the specs of one book must share archive (the ring size of the handle)")
    return per


# ---------------------------------------------------------------------------------------------------------------- rules 2 - 4
def _taps(dst, src, x_axis):
    """csrc/resize_dev.h axis_tap for every destination index: (i0, i1, a0, a1)."""
    scale = np.float64(1.0) / (np.float64(dst) / np.float64(src))
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    fl = np.floor(f)
    s = fl.astype(np.int64)
    f = (f - fl).astype(F32)
    if x_axis:                                                       # the x axis zeroes the weight when it clamps ...
        lo, hi = s < 0, s >= src - 1
        s = np.where(lo, 0, np.where(hi, src - 1, s))
        f = np.where(lo | hi, F32(0), f).astype(F32)
    a0 = np.rint(((F32(1) - f).astype(F32) * F32(2048)).astype(F32)).astype(np.int64)
    a1 = np.rint((f * F32(2048)).astype(F32)).astype(np.int64)
    return np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1), a0, a1    # ... the y axis clips the two row indices and keeps its weights


def resize_u8(img, dst_h=THUMB_H, dst_w=THUMB_W):
    """csrc/resize_dev.h resize_px for every output pixel: uint8 [h, w, 3] to uint8 [dst_h, dst_w, 3] - the copy at equal sizes, the
    2 x 2 mean at exactly twice the size, else the 11-bit fixed-point bilinear form."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("snapshots: resize_u8 takes a uint8 [h, w, c] image")
    h, w = img.shape[:2]
    v = img.astype(np.int64)
    if (h, w) == (dst_h, dst_w):
        return img.copy()
    if (h, w) == (2 * dst_h, 2 * dst_w):
        return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, a0, a1 = _taps(dst_w, w, True)
    y0, y1, b0, b1 = _taps(dst_h, h, False)
    hz = v[:, x0] * a0[None, :, None] + v[:, x1] * a1[None, :, None]
    out = (((b0[:, None, None] * (hz[y0] >> 4)) >> 16) + ((b1[:, None, None] * (hz[y1] >> 4)) >> 16) + 2) >> 2
    return (out & 0xff).astype(np.uint8)


def clip_box(row, H, W):
    """Rule 2 in Python ints: (xa, ya, vw, vh, vis, full)."""
    x1, y1, x2, y2 = (int(v) for v in row[:4])
    xa, ya, xb, yb = max(x1, 0), max(y1, 0), min(x2, int(W)), min(y2, int(H))
    vw, vh = xb - xa, yb - ya
    return xa, ya, vw, vh, vw * vh, (x2 - x1) * (y2 - y1)


def luma(thumb):
    t = np.asarray(thumb).astype(np.int64)
    return (77 * t[..., 0] + 150 * t[..., 1] + 29 * t[..., 2] + 128) >> 8


def sharpness(thumb):
    """Rule 4: the Laplacian sum of the luma over the interior, a Python int."""
    Y = luma(thumb)
    return int(np.abs(4 * Y[1:-1, 1:-1] - Y[:-2, 1:-1] - Y[2:, 1:-1] - Y[1:-1, :-2] - Y[1:-1, 2:]).sum())


def snapshot_of(frame, row, spec, bgr=False):
    """Rules 2 - 4 for one row of one frame (uint8 [H, W, 3]): (thumbnail uint8 [128, 64, 3] RGB, score), or (None, -1) for a row
    that is no candidate."""
    H, W = frame.shape[:2]
    xa, ya, vw, vh, vis, full = clip_box(row, H, W)
    if vw < spec.min_w or vh < spec.min_h or full <= 0:
        return None, -1
    thumb = resize_u8(frame[ya:ya + vh, xa:xa + vw])
    if bgr:
        thumb = thumb[:, :, ::-1].copy()
    return thumb, (sharpness(thumb) * vis) // full


# ---------------------------------------------------------------------------------------------------------------- rules 5 - 7
class SnapshotBook:
    """The snapshots of ``n_streams`` streams on the host.  ``update(stream, rows, t, frame, tag=0, bgr=False)`` takes one processed
    frame (rows [n][6] = x1, y1, x2, y2, track id, class; None: the tracker was not called, nothing is touched; zero rows age every
    entry; frame: uint8 [H, W, 3]) and returns its items int32 [m][6] = tag, id, class, kind, score, aux (a stream without a spec:
    always [0][6])."""

    def __init__(self, specs, max_age=30, n_streams=None):
        if isinstance(specs, SnapSpec) and n_streams is None:
            n_streams = 1
        if isinstance(specs, (SnapshotBook, DeviceSnapshotBook)):
            specs = specs.specs
        self.specs = stream_specs(specs, len(specs) if n_streams is None else int(n_streams))
        self.n_streams = len(self.specs)
        self.max_age = check_max_age("snapshots", max_age)
        self.archive_slots = next(s for s in self.specs if s is not None).archive
        # what the tests assert about their own scenes
        self.stats = dict(ties=0, clipped=0, non_candidates=0, ignored_rows=0, replacements=0, closes=0, dropped=0, ring_wraps=0,
                          slot_reuses=0, max_table=0, copies=0, area2=0, overruns=0)
        self._freed = 0
        self.reset()

    def reset(self, stream=None):
        """An empty table, an empty ring and closed count 0 for one stream, or for all (None)."""
        if stream is None:
            self.tables, self.rings, self.closed = [{} for _ in self.specs], [{} for _ in self.specs], [0] * self.n_streams
        else:
            self.tables[int(stream)], self.rings[int(stream)], self.closed[int(stream)] = {}, {}, 0

    def begin_call(self):
        """A device call starts here: ``slot_reuses`` counts first pictures taken after a picture was given up in the same call
        (the device's free list hands that very slot out again)."""
        self._freed = 0

    def update(self, stream, rows, t, frame, tag=0, bgr=False):
        if rows is None:
            return None
        sp, table, ring, st = self.specs[stream], self.tables[stream], self.rings[stream], self.stats
        if sp is None:
            return np.zeros((0, 6), np.int32)
        t, A, out = float(t), self.archive_slots, []
        H, W = frame.shape[:2]
        seen = set()
        for r in rows:
            tid, cls = int(r[4]), int(r[5])
            if tid in seen:
                raise ValueError(f"snapshots: track id {tid} appears twice in one frame")
            if sp.class_id not in (None, cls):
                st["ignored_rows"] += 1
                continue
            seen.add(tid)
            e = table.get(tid)
            if e is None:
                e = table[tid] = dict(cls=cls, score=-1, n_seen=0, box=(0, 0, 0, 0), tag_best=-1, t_first=t, t_best=0.0, t_last=t, thumb=None,
                                      age=0)
            e["age"], e["t_last"], e["cls"] = 0, t, cls
            e["n_seen"] += 1
            thumb, score = snapshot_of(frame, r, sp, bgr)
            xa, ya, vw, vh, vis, full = clip_box(r, H, W)
            if thumb is None:
                st["non_candidates"] += 1
                continue
            st["clipped"] += vis != full
            st["copies"] += (vh, vw) == (THUMB_H, THUMB_W)
            st["area2"] += (vh, vw) == (2 * THUMB_H, 2 * THUMB_W)
            st["ties"] += score == e["score"]
            if score > e["score"]:                                   # strictly greater: on a tie the earlier sighting stays
                if e["thumb"] is None:
                    if self._freed:
                        st["slot_reuses"] += 1
                        self._freed -= 1
                else:
                    st["replacements"] += 1
                e.update(score=score, box=tuple(int(v) for v in r[:4]), tag_best=int(tag), t_best=t, thumb=thumb)
                out.append([int(tag), tid, cls, BEST, score, e["n_seen"]])
        st["max_table"] = max(st["max_table"], len(table))
        leaving = [k for k in table if k not in seen and table[k]["age"] + 1 > self.max_age and table[k]["thumb"] is not None]
        st["overruns"] += bool(0 < A < len(leaving) and ring)         # more pictures close in one frame than the ring holds, over occupants
        for tid in [k for k in table if k not in seen]:              # (dicts keep entry order)
            e = table[tid]
            e["age"] += 1
            if e["age"] <= self.max_age:
                continue
            del table[tid]
            st["closes"] += 1
            pos = -1
            if e["thumb"] is not None and A > 0:
                pos = self.closed[stream] % A
                if pos in ring:
                    st["ring_wraps"] += 1
                    self._freed += 1
                ring[pos] = dict(e, id=tid, t_closed=t)
                self.closed[stream] += 1
            elif e["thumb"] is not None:
                st["dropped"] += 1
                self._freed += 1
            out.append([int(tag), tid, e["cls"], CLOSED, e["score"], pos])
        return np.array(out, dtype=np.int32).reshape(-1, 6)

    def update_batch(self, frames_rows, stream_of, times, frames, bgr=False):
        """One device call's worth: frame f of stream ``stream_of[f]`` at ``times[f]`` with pixels ``frames[f]``, tagged f."""
        self.begin_call()
        return [self.update(stream_of[f], frames_rows[f], times[f], frames[f], tag=f, bgr=bgr) for f in range(len(frames_rows))]

    @staticmethod
    def _record(tid, e):
        thumb = np.zeros((THUMB_H, THUMB_W, 3), np.uint8) if e["thumb"] is None else e["thumb"]
        return dict(id=tid, cls=e["cls"], score=e["score"], n_seen=e["n_seen"], box=e["box"], tag_best=e["tag_best"], t_first=e["t_first"],
                    t_best=e["t_best"], t_last=e["t_last"], thumb=thumb)

    def tracks(self, stream=0):
        """The live entries of a stream in table order: dicts of id, cls, score, n_seen, box, tag_best, t_first, t_best, t_last and
        thumb (uint8 [128, 64, 3]; zeros while there is no picture)."""
        return [self._record(tid, e) for tid, e in self.tables[stream].items()]

    def archive(self, stream=0):
        """The archive ring of a stream, oldest first: the columns of ``tracks`` and t_closed."""
        A, n, ring = self.archive_slots, self.closed[stream], self.rings[stream]
        order = range(n) if n < A else [(n + k) % A for k in range(A)]
        return [dict(self._record(ring[p]["id"], ring[p]), t_closed=ring[p]["t_closed"]) for p in order]

    def snapshot(self, stream, track_id):
        """The record of ``track_id``: a live entry first, then the newest archived one; None when absent."""
        return _find(self.tracks(stream), self.archive(stream), track_id)


def _find(live, archived, track_id):
    for rec in live + archived[::-1]:
        if rec["id"] == int(track_id):
            return rec
    return None


def same_records(a, b):
    """Two lists of ``tracks()`` / ``archive()`` records are equal, pictures included."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.keys() != y.keys() or any(x[k] != y[k] for k in x if k != "thumb") or not np.array_equal(x["thumb"], y["thumb"]):
            return False
    return True


def by_global_id(books_tracks, identities):
    """The host join over all cameras: ``books_tracks[s]`` the records of stream s (``tracks(s)``, with ``archive(s)`` appended if
    wanted; None: none), ``identities[s]`` its (track id, global id) pairs or a dict (``last_identities()``; global id 0 = not
    resolved yet).  {global id: dict(stream, record)} with the best-scoring picture of every global id (the earlier stream wins a
    tie; records without a picture do not count)."""
    best = {}
    for s, recs in enumerate(books_tracks):
        if not recs:
            continue
        ids = identities[s]
        gid_of = ids if isinstance(ids, dict) else {int(a): int(b) for a, b in ids}
        for rec in recs:
            gid = int(gid_of.get(int(rec["id"]), 0))
            if gid <= 0 or rec["score"] < 0:
                continue
            if gid not in best or rec["score"] > best[gid]["record"]["score"]:
                best[gid] = dict(stream=s, record=rec)
    return dict(sorted(best.items()))


# ---------------------------------------------------------------------------------------------------------------- the device front
def pixel_layout(frame_hw, n, frame_off=None):
    """(off uint64 [n], hw int32 [n][2], the bytes they span) of n frames: ``frame_hw`` one (h, w) for all or one per frame, frames
    back to back unless ``frame_off`` names each frame's byte offset."""
    hw = np.asarray(frame_hw, dtype=np.int64)
    hw = np.tile(hw.reshape(1, 2), (n, 1)) if hw.ndim == 1 else hw.reshape(-1, 2)
    if len(hw) != n:
        raise ValueError("snapshots: %d frame sizes for %d frames" % (len(hw), n))
    size = hw[:, 0] * hw[:, 1] * 3
    off = np.concatenate([[0], np.cumsum(size)[:-1]]) if frame_off is None else np.asarray(frame_off, dtype=np.int64).reshape(-1)
    if len(off) != n or (n and (off.min() < 0 or hw.min() < 1)):
        raise ValueError("snapshots: a frame layout of %d offsets for %d frames, or a negative one" % (len(off), n))
    return off.astype(np.uint64), np.ascontiguousarray(hw, dtype=np.int32), int((off + size).max()) if n else 0


class DeviceSnapshotBook(TrackStage):
    """``SnapshotBook`` with every table, ring and picture in HBM: three launches (score, decide, commit) advance all streams over
    the frames of a call, whose pixels are read where they lie in HBM.  ``specs``: one SnapSpec for all streams, or a list with one
    (or None: that stream is skipped) per stream."""
    NAME = "snapshots"
    LIB = "snap"
    HOST = SnapshotBook
    TIMED = ("score", "decide", "commit")

    def __init__(self, specs, max_age=30, n_streams=None):
        if n_streams is None:
            n_streams = 1 if isinstance(specs, SnapSpec) else len(specs.specs if isinstance(specs, (SnapshotBook, DeviceSnapshotBook)) else specs)
        super().__init__(n_streams, max_age)
        self.specs = stream_specs(specs, self.n_streams)
        self.archive_slots = next(s for s in self.specs if s is not None).archive

    def _settings(self, n_streams):
        return self.specs[:n_streams], self.max_age, n_streams

    def _what(self):
        return "a book"

    def host(self):
        """A fresh SnapshotBook of these specs and max_age: the comparator."""
        return SnapshotBook(self.specs, self.max_age)

    def _create(self, lib):
        return lib.yds_snap_create(self.n_streams, self.max_age, self.archive_slots)

    def _setup(self, lib, h):
        from . import _lib
        for s, sp in enumerate(self.specs):
            if sp is not None:
                _lib.check(lib.yds_snap_set_stream(h, s, -1 if sp.class_id is None else sp.class_id, sp.min_w, sp.min_h))

    def update(self, stream, rows, t, frames_dev, frame_hw, bgr=False):
        """One frame of one stream, its pixels at ``frames_dev``: SnapshotBook.update (None in, None out)."""
        return self.update_batch([rows], [stream], [t], frames_dev, frame_hw, bgr=bgr)[0]

    def update_batch(self, frames_rows, stream_of, times, frames_dev, frame_hw, frame_off=None, frames_bytes=None, bgr=False):
        """Frames in the order given (a stream's frames in time order), frame f of stream ``stream_of[f]`` at time ``times[f]``, a
        frame whose rows are None is not seen.  ``frames_dev``: device pointer of the pixels - frame f is ``frame_hw[f]`` = (h, w)
        x 3 uint8 at byte ``frame_off[f]`` (``frame_hw`` one pair: all the same; no offsets: back to back) of a buffer of
        ``frames_bytes`` (default: what the layout spans), ``bgr``: the bytes are B, G, R.  Items carry the frame's index f as
        their tag.  Returns per frame its items int32 [m][6] (None for a None frame)."""
        from . import _lib
        live, rows6, first, sof, tm = self.pack(frames_rows, stream_of, times)
        out = [None] * len(frames_rows)
        if not live:
            return out
        off, hw, span = pixel_layout(frame_hw, len(frames_rows), frame_off)
        off, hw = np.ascontiguousarray(off[live]), np.ascontiguousarray(hw[live])
        n = len(live)
        total = int(first[-1])
        # (every row can report one BEST item, every entry - those there and those the rows bring - closes at most once)
        cap = 2 * total + sum(self._table_count("tracks", s, 10) for s in set(sof.tolist())) + 1
        out6, first_out, m = np.zeros((cap, 6), np.int32), np.zeros(n + 1, np.int32), C.c_int(0)
        _lib.check(_lib.load().yds_snap_update(self.handle, _lib.ptr(rows6), _lib.ptr(first), _lib.ptr(sof), _lib.ptr(tm), n, frames_dev,
                                               _lib.ptr(off), _lib.ptr(hw), span if frames_bytes is None else int(frames_bytes), 1 if bgr else 0,
                                               _lib.ptr(out6), _lib.ptr(first_out), cap, C.byref(m)))
        for k, f in enumerate(live):
            out[f] = out6[first_out[k]:first_out[k + 1]].copy()
            out[f][:, 0] = f                                         # (the library tags by live frame)
        return out

    _COLUMNS = [(np.int32, ())] * 4 + [(np.int32, (4,)), (np.int32, ())] + [(np.float64, ())] * 3

    @staticmethod
    def _records(cols, closed=None):
        ids, cls, score, seen, box, tag, tf, tb, tl = cols[:9]
        out = []
        for k in range(len(ids)):
            rec = dict(id=int(ids[k]), cls=int(cls[k]), score=int(score[k]), n_seen=int(seen[k]), box=tuple(int(v) for v in box[k]),
                       tag_best=int(tag[k]), t_first=float(tf[k]), t_best=float(tb[k]), t_last=float(tl[k]), thumb=cols[-1][k].copy())
            if closed is not None:
                rec["t_closed"] = float(closed[k])
            out.append(rec)
        return out

    def tracks(self, stream=0):
        """SnapshotBook.tracks(stream), read from the device."""
        return self._records(self._read_table("tracks", stream, self._COLUMNS + [(np.uint8, (THUMB_H, THUMB_W, 3))]))

    def archive(self, stream=0):
        """SnapshotBook.archive(stream), read from the device."""
        cols = self._read_table("archive", stream, self._COLUMNS + [(np.float64, ()), (np.uint8, (THUMB_H, THUMB_W, 3))])
        return self._records(cols, closed=cols[9])

    def snapshot(self, stream, track_id):
        """The record of ``track_id``: a live entry first, then the newest archived one; None when absent."""
        return _find(self.tracks(stream), self.archive(stream), track_id)

    def pool(self, stream=0):
        """(free slots, all slots) of the stream's picture pool: free + live entries with a picture + archived snapshots = all."""
        from . import _lib
        free, slots = C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().yds_snap_get_pool(self.handle, self._stream(stream), C.byref(free), C.byref(slots)))
        return free.value, slots.value

    @classmethod
    def _from_host(cls, x, n_streams, max_age):
        if isinstance(x, SnapshotBook):
            if x.n_streams != n_streams:
                raise ValueError(f"snapshots: a SnapshotBook of {x.n_streams} streams for {n_streams} streams")
            return cls(x.specs, x.max_age, n_streams)
        return cls(x, max_age, n_streams=n_streams)


as_device_snapshots = DeviceSnapshotBook.as_device      # (the name Pipeline.set_snapshots and callers import)
