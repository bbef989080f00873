"""Anonymised output: people are pixelated or filled over before anything is drawn on a frame.

``Anonymize`` holds the settings, ``mask_rects`` turns the rows of one frame into mask rectangles (Python ints, shared by the host
and the device form), ``anonymize`` is the numpy host form - the DEFINITION of the pixels - and ``DeviceAnonymizer`` runs the same
on frames resident in HBM (csrc/anonymize.hip, yds_anonymize_frames).  The output stage applies the mask first, then outlines,
plates and text, then the FPS text (label_draw.DeviceOverlay.render(privacy=...), detect.VideoDetector(anonymize=...)).

Semantics.  A rectangle (xa, ya, xb, yb) covers rows [max(ya,0), min(yb+1,H)) and columns [max(xa,0), min(xb+1,W)) - the filled
rectangle() of label_draw.py; U is the union over the frame's rectangles.
  pixelate: cells of ``block`` x ``block`` pixels anchored at the FRAME's origin (edge cells are partial); per channel
            v = (2*S + cnt) // (2*cnt) with S the sum of the ORIGINAL values of the whole cell and cnt its pixels; every pixel of
            cell & U takes v, every other pixel keeps its value.
  fill:     every pixel of U takes ``color``.
Both are independent of the order and overlap of the rectangles and of the channel order of the frame."""

from __future__ import annotations

import math

import numpy as np

MODES = ("pixelate", "fill")
REGIONS = ("box", "head")
_LIM = 1 << 30                     # rectangle corners handed to the device are clamped to +-2^30: far outside any frame


class Anonymize:
    """Settings of the mask.  mode "pixelate" | "fill"; block: cell edge in [2, 64] (pixelate); color: fill colour in the RGB
    image's channel order, like the class colours; region "box" | "head" (the top head_frac = (num, den) of the box);
    margin >= 0 pixels added on every side - the remedy for the lag of a skipped frame, which is masked with the rectangles of the
    last processed one; classes: class ids to mask (None: all); exempt_ids: a mutable set of track ids shown unmasked (it filters
    tracker rows only: with include_detections a person's detection still masks them - switch that off for a watch list);
    include_detections: the frame's post-NMS detections add rectangles of their own, so that a person is masked before their
    track is confirmed.  ValueError naming the argument for anything else."""

    def __init__(self, mode="pixelate", block=16, color=(0, 0, 0), region="box", head_frac=(1, 4), margin=0, classes=(0,),
                 exempt_ids=(), include_detections=True):
        if mode not in MODES:
            raise ValueError("Anonymize: mode must be one of %r, got %r" % (MODES, mode))
        if not _is_int(block) or not 2 <= int(block) <= 64:
            raise ValueError("Anonymize: block must be an integer in [2, 64], got %r" % (block,))
        try:
            col = tuple(color)
        except TypeError:
            col = ()
        if len(col) != 3 or not all(_is_int(c) and 0 <= int(c) <= 255 for c in col):
            raise ValueError("Anonymize: color must be three integers in [0, 255], got %r" % (color,))
        if region not in REGIONS:
            raise ValueError("Anonymize: region must be one of %r, got %r" % (REGIONS, region))
        try:
            hf = tuple(head_frac)
        except TypeError:
            hf = ()
        if len(hf) != 2 or not all(_is_int(v) for v in hf) or not 0 < int(hf[0]) <= int(hf[1]):
            raise ValueError("Anonymize: head_frac must be (num, den) integers with 0 < num <= den, got %r" % (head_frac,))
        if not _is_int(margin) or int(margin) < 0:
            raise ValueError("Anonymize: margin must be an integer >= 0, got %r" % (margin,))
        if classes is not None:
            try:
                cls = tuple(classes)
            except TypeError:
                cls = None
            if cls is None or not all(_is_int(c) for c in cls):
                raise ValueError("Anonymize: classes must be None or integer class ids, got %r" % (classes,))
        if isinstance(exempt_ids, (str, bytes)):
            raise ValueError("Anonymize: exempt_ids must be a set of integer track ids, got %r" % (exempt_ids,))
        try:
            ex = exempt_ids if isinstance(exempt_ids, set) else set(exempt_ids)
        except TypeError:
            ex = None
        if ex is None or not all(_is_int(t) for t in ex):
            raise ValueError("Anonymize: exempt_ids must be a set of integer track ids, got %r" % (exempt_ids,))
        if not isinstance(include_detections, (bool, np.bool_)):
            raise ValueError("Anonymize: include_detections must be a bool, got %r" % (include_detections,))
        self.mode, self.block, self.color = mode, int(block), tuple(int(c) for c in col)
        self.region, self.head_frac, self.margin = region, (int(hf[0]), int(hf[1])), int(margin)
        self.classes = None if classes is None else frozenset(int(c) for c in cls)
        self.exempt_ids = ex                             # the caller's own set when one was given: add and remove ids while running
        self.include_detections = bool(include_detections)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _rect(anon, xa, ya, xb, yb):
    """Margin and head rule on integer corners (xa <= xb, ya <= yb)."""
    m = anon.margin
    xa, xb, ya, yb = xa - m, xb + m, ya - m, yb + m
    if anon.region == "head":
        num, den = anon.head_frac
        yb = ya + ((yb - ya) * num) // den
    return (xa, ya, xb, yb)


def _masked(anon, cls):
    return anon.classes is None or cls in anon.classes


def mask_rects(anon, h, w, hold_rows, detections=None):
    """The mask rectangles of one h x w frame, [(xa, ya, xb, yb), ...] in Python ints, inclusive corners, not clipped;
    rectangles that cover no pixel of the frame are left out.
    hold_rows: the rows the frame is drawn with - tracker rows (integers [m, 6] = x1, y1, x2, y2, track id, class; filtered by
    class and exempt_ids), or the raw rows of a detector without a tracker (floats [m, 6 | 7] = x1, y1, x2, y2, ..., class;
    treated as detections: rounded outwards), or None / empty.
    detections: the frame's post-NMS detections, floats [n, 5] = x, y, w, h, class (Pipeline.last_detections()), used with
    include_detections: rounded outwards in float64 - floor(x), floor(y), ceil(x + w), ceil(y + h)."""
    out = []

    def add(r):
        if r[2] >= 0 and r[3] >= 0 and r[0] < w and r[1] < h and r[2] >= r[0] and r[3] >= r[1]:
            out.append(r)

    def add_float(x1, y1, x2, y2, cls):
        if not all(math.isfinite(v) for v in (x1, y1, x2, y2, cls)) or not _masked(anon, int(cls)):
            return
        add(_rect(anon, math.floor(min(x1, x2)), math.floor(min(y1, y2)), math.ceil(max(x1, x2)), math.ceil(max(y1, y2))))

    if hold_rows is not None and len(hold_rows):
        rows = hold_rows.detach().cpu().numpy() if hasattr(hold_rows, "detach") else np.asarray(hold_rows)
        if rows.dtype.kind in "iu":
            for r in rows.reshape(-1, 6).tolist():
                if _masked(anon, r[5]) and r[4] not in anon.exempt_ids:
                    add(_rect(anon, min(r[0], r[2]), min(r[1], r[3]), max(r[0], r[2]), max(r[1], r[3])))
        else:
            for r in rows.astype(np.float64).reshape(len(rows), -1).tolist():
                add_float(r[0], r[1], r[2], r[3], r[-1])
    if anon.include_detections and detections is not None and len(detections):
        for x, y, bw, bh, cls in np.asarray(detections, dtype=np.float64).reshape(-1, 5).tolist():
            add_float(x, y, x + bw, y + bh, cls)
    return out


def _clipped(rects, h, w):
    """Half-open pixel ranges (x0, y0, x1, y1) of the rectangles inside an h x w frame; empty ones dropped."""
    out = []
    for xa, ya, xb, yb in rects:
        x0, y0, x1, y1 = max(int(xa), 0), max(int(ya), 0), min(int(xb) + 1, w), min(int(yb) + 1, h)
        if x1 > x0 and y1 > y0:
            out.append((x0, y0, x1, y1))
    return out


def anonymize(img, rects, anon, inplace=False, bgr=False):
    """The host form, and the reference of the device form: ``img`` uint8 [H, W, 3] with the rectangles of mask_rects masked
    as ``anon`` says; a copy unless inplace.  bgr: the image holds B, G, R (only the fill colour depends on it).  Work is
    restricted to the cell-aligned surroundings of each rectangle."""
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError("anonymize: img must be uint8 [H, W, 3], got %s %s" % (img.dtype, img.shape))
    h, w = img.shape[:2]
    out = img if inplace else img.copy()
    rc = _clipped(rects, h, w)
    if not rc:
        return out
    if anon.mode == "fill":
        color = anon.color[::-1] if bgr else anon.color
        for x0, y0, x1, y1 in rc:
            out[y0:y1, x0:x1] = color
        return out
    m = anon.block
    src = img.copy() if inplace else img                         # every cell value comes from the ORIGINAL pixels
    for x0, y0, x1, y1 in rc:
        # the rectangle's cells, whole: rows [r0, r1), columns [c0, c1)
        r0, c0 = (y0 // m) * m, (x0 // m) * m
        r1, c1 = min(((y1 - 1) // m + 1) * m, h), min(((x1 - 1) // m + 1) * m, w)
        sub = src[r0:r1, c0:c1].astype(np.int64)
        ridx, cidx = np.arange(0, r1 - r0, m), np.arange(0, c1 - c0, m)
        s = np.add.reduceat(np.add.reduceat(sub, ridx, axis=0), cidx, axis=1)          # [cells y, cells x, 3]
        ch = np.diff(np.append(ridx, r1 - r0))
        cw = np.diff(np.append(cidx, c1 - c0))
        cnt = (ch[:, None] * cw[None, :])[:, :, None]
        v = ((2 * s + cnt) // (2 * cnt)).astype(np.uint8)
        full = np.repeat(np.repeat(v, ch, axis=0), cw, axis=1)
        out[y0:y1, x0:x1] = full[y0 - r0:y1 - r0, x0 - c0:x1 - c0]
    return out


def pack_rects(rects_per_frame):
    """The CSR table the device entries take: (int32 [max(total, 1), 4], int32 [n + 1]); a frame's entry may be None."""
    flat, ptr = [], [0]
    for rects in rects_per_frame:
        for r in (rects if rects is not None else ()):
            flat.append([max(-_LIM, min(_LIM, int(v))) for v in r])
        ptr.append(len(flat))
    table = np.array(flat, dtype=np.int32).reshape(-1, 4) if flat else np.zeros((1, 4), np.int32)
    return np.ascontiguousarray(table), np.ascontiguousarray(ptr, dtype=np.int32)


def device_args(anon, bgr):
    """(mode, block, colour) as the C entries take them; the colour as the three bytes that land in memory, byte 0 lowest."""
    c = anon.color[::-1] if bgr else anon.color
    return MODES.index(anon.mode) + 1, anon.block, c[0] | (c[1] << 8) | (c[2] << 16)


class DeviceAnonymizer:
    """The mask alone, in place on frames that are resident in HBM - no overlay, no copy (yds_anonymize_frames): for callers of
    Pipeline who keep their frames on the device.  Bit-equal to anonymize()."""

    def __init__(self, anon):
        self.anon = anon

    def apply(self, frames_dev, slots, h, w, rects_per_frame, n_frames=None, bgr=False):
        """frames_dev: device pointer of uint8 frames h*w*3 bytes apart; frame slots[i] is masked with rects_per_frame[i]
        (mask_rects lists; None or empty: untouched).  Slots must be distinct and inside [0, n_frames) (default: max slot + 1).
        bgr: the frames hold B, G, R.  Synchronous."""
        from . import _lib
        slots_a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        if len(slots_a) != len(rects_per_frame):
            raise ValueError("DeviceAnonymizer.apply: %d slots for %d rectangle lists" % (len(slots_a), len(rects_per_frame)))
        if len(slots_a) == 0:
            return
        n_src = int(slots_a.max()) + 1 if n_frames is None else int(n_frames)
        table, ptr = pack_rects(rects_per_frame)
        mode, block, color = device_args(self.anon, bgr)
        _lib.check(_lib.load().yds_anonymize_frames(frames_dev, n_src, _lib.ptr(slots_a), len(slots_a), int(h), int(w), _lib.ptr(table),
                                                    _lib.ptr(ptr), mode, block, color))

    def apply_mixed(self, frames_dev, frames_bytes, frame_off, frame_hw, slots, rects_per_frame, bgr=False):
        """apply() for frames of DIFFERENT sizes in one device buffer of frames_bytes bytes (yds_anonymize_frames_mixed): staged
        frame j is uint8 [frame_hw[j][0], frame_hw[j][1], 3] at frames_dev + frame_off[j], any byte offset; frame slots[i] is
        masked with rects_per_frame[i] - mask_rects lists made with THAT frame's h, w - its cells anchored at its own origin.
        Slots must be distinct, the frames must not overlap.  Synchronous."""
        from . import _lib
        slots_a = np.ascontiguousarray(slots, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(frame_off, dtype=np.uint64).reshape(-1)
        hw = np.ascontiguousarray(frame_hw, dtype=np.int32).reshape(-1, 2)
        if len(slots_a) != len(rects_per_frame):
            raise ValueError("DeviceAnonymizer.apply_mixed: %d slots for %d rectangle lists" % (len(slots_a), len(rects_per_frame)))
        if off.size != len(hw):
            raise ValueError("DeviceAnonymizer.apply_mixed: %d offsets for %d sizes" % (off.size, len(hw)))
        if len(slots_a) == 0:
            return
        table, ptr = pack_rects(rects_per_frame)
        mode, block, color = device_args(self.anon, bgr)
        _lib.check(_lib.load().yds_anonymize_frames_mixed(frames_dev, int(frames_bytes), len(hw), _lib.ptr(off), _lib.ptr(hw), _lib.ptr(slots_a),
                                                          len(slots_a), _lib.ptr(table), _lib.ptr(ptr), mode, block, color))
