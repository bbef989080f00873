#!/usr/bin/env python3
"""Timing of the cross-camera gallery search (csrc/gallery_search.hip) on resident galleries; writes profiles/gallery_search_bench.txt.

Set-up: 68 trackers x 30 tracks x 100 rows (nn_budget=100, every gallery full) and a crowd case of 150 tracks per tracker, galleries
filled through yds_tracker_step with synthetic features (static boxes, one feature cluster per identity).  Q = 1, 32, 256.
Per case: warm-up, then the median (and min / max) of repeated runs inside ONE invocation, device time per call from HIP events
around the launch sequence (yds_gallery_search_bench: normalise + table read + distances + select), and next to it the wall time of
the whole yds_gallery_search call (upload of the queries, launches, one synchronisation, one copy back).
Derived: gallery bytes / device time for Q <= 32 (every row is fetched once: rows x 2048 B) and FLOP/s for Q = 256 (2 x 512 x rows x
Q) against the 157.3 TFLOP/s fp32-MFMA peak.

usage: python tools/gallery_search_bench.py [--streams 68] [--rows 100] [--reps 50] [--out profiles/gallery_search_bench.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_deepsort_amd import _lib, search  # noqa: E402
from yolo_deepsort_amd.deep_sort import _TrackerHandle  # noqa: E402

EMB = 512
PEAK_F32_MFMA = 157.3e12
HBM_MEASURED = 6.29e12


def fill(n_streams, n_tracks, n_rows, seed):
    """n_streams trackers of n_tracks Confirmed tracks holding n_rows rows each."""
    rng = np.random.RandomState(seed)
    cols = 16
    tlwh = np.array([[20 + 100 * (i % cols), 20 + 160 * (i // cols), 48, 96] for i in range(n_tracks)], np.float32)
    payload = np.zeros(n_tracks, np.float32)
    trackers, centres = [], []
    for s in range(n_streams):
        t = _TrackerHandle(0.3, 0.7, 30, 1, n_rows)
        c = rng.randn(n_tracks, EMB).astype(np.float32)
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        for _ in range(n_rows):
            t.step(tlwh, c + (0.05 / np.sqrt(EMB)) * rng.randn(n_tracks, EMB).astype(np.float32), payload)
        trackers.append(t)
        centres.append(c)
    return trackers, np.concatenate(centres)


def measure(lib, trackers, queries, reps, warm, top_k=5):
    q = np.ascontiguousarray(queries, np.float32)
    dev = _lib.DeviceBuffer.from_array(q)
    arr = (C.c_void_p * len(trackers))(*[t._h for t in trackers])
    us = np.zeros(reps, np.float32)
    w = np.zeros(warm, np.float32)
    _lib.check(lib.yds_gallery_search_bench(arr, len(trackers), dev.ptr, len(q), 2, 0.3, top_k, warm, _lib.ptr(w)))
    _lib.check(lib.yds_gallery_search_bench(arr, len(trackers), dev.ptr, len(q), 2, 0.3, top_k, reps, _lib.ptr(us)))
    wall = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        hits = search.gallery_search(trackers, q, top_k=top_k)
        if i >= warm:
            wall.append((time.perf_counter() - t0) * 1e6)
    dev.free()
    return us, np.array(wall), hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gallery_search_bench.txt"))
    a = ap.parse_args()
    _lib.init()
    lib = _lib.load()
    lines = ["gallery search, measured on ONE MI355X box in ONE invocation of tools/gallery_search_bench.py "
             "(--streams %d --rows %d --reps %d --warmup %d)" % (a.streams, a.rows, a.reps, a.warmup),
             "device us: HIP events around the launch sequence, median [min, max] of %d repetitions after %d warm-up ones" % (a.reps, a.warmup),
             "wall us: host clock around the whole yds_gallery_search call (host queries), median of %d calls" % a.reps,
             "bounds quoted: 6.29 TB/s measured HBM copy rate, 157.3 TFLOP/s fp32-MFMA peak", ""]
    for name, n_tracks in (("30 tracks per tracker", 30), ("crowd: 150 tracks per tracker", 150)):
        t0 = time.perf_counter()
        trackers, centres = fill(a.streams, n_tracks, a.rows, seed=n_tracks)
        rows = a.streams * n_tracks * a.rows
        gbytes = rows * EMB * 4
        lines.append("%s: %d trackers x %d tracks x %d rows = %d rows, %.1f MB of galleries (filled in %.1f s)"
                     % (name, a.streams, n_tracks, a.rows, rows, gbytes / 1e6, time.perf_counter() - t0))
        rng = np.random.RandomState(1)
        for Q in (1, 32, 256):
            pick = rng.randint(0, len(centres), Q)
            queries = 2.0 * (centres[pick] + (0.05 / np.sqrt(EMB)) * rng.randn(Q, EMB).astype(np.float32))
            us, wall, hits = measure(lib, trackers, queries, a.reps, a.warmup)
            found = sum(1 for q in range(Q) if hits[q] and hits[q][0][:2] == (pick[q] // n_tracks, pick[q] % n_tracks + 1))
            med = float(np.median(us))
            line = "  Q = %3d: device %9.1f us [%.1f, %.1f]   wall %9.1f us   (%d / %d queries find their own track first)" % (
                Q, med, us.min(), us.max(), float(np.median(wall)), found, Q)
            if Q <= 32:
                rate = gbytes / (med * 1e-6)
                line += "   gallery bytes / device time = %.2f TB/s (%.0f %% of 6.29 TB/s)" % (rate / 1e12, 100 * rate / HBM_MEASURED)
            if Q == 256:
                fl = 2.0 * EMB * rows * Q / (med * 1e-6)
                line += "   %.1f TFLOP/s (%.0f %% of 157.3 TFLOP/s)" % (fl / 1e12, 100 * fl / PEAK_F32_MFMA)
            lines.append(line)
            print(line, flush=True)
        del trackers
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
