#!/usr/bin/env python3
"""What the identity stage costs a many-camera step; writes profiles/identity_stream_bench.txt.

Workload: cfg2 (yolov3 608 x 608 + DeepSORT), 68 streams x 1 frame per step, 30 persons per frame - the `multi` leg of
tools/multi_stream_bench.py, as in tools/action_stream_bench.py: every stream plays the workload's stream from its own offset,
frames resident in HBM, the next step's frames handed over (look-ahead), schedule fixed (serialized).  Legs, each on a fresh
MultiStreamPipeline with fresh trackers over the SAME steps:

  a     the step without identities
  b     the step with the identity stage (MultiStreamPipeline.set_identities before the first step, last_identities() read every
        step).  Every step carries the collect launch; a step that admits a new track also runs the resolve sequence (gather,
        distances, reduce, resolve) and synchronises once more.  Timed steps are split by that: the difference of their median
        wall times is what the extra synchronisation and the sequence cost a step that has one.
  cold  (once, after the rounds) W + N steps without identities, then identities switched on over the 68 x 30 live tracks: the
        steps that follow admit max_rows gallery rows each and defer the rest, until nothing is deferred.

One invocation runs --rounds rounds of (a, b), the order swapped in every other round so that no leg always runs first.  Per run:
W untimed warm-up steps (the tracks are confirmed, and get their ids, inside them), then N timed ones; the figure is the median
step wall time; the run-to-run spread is max - min over the runs of leg a.

  python tools/identity_stream_bench.py [--streams 68] [--steps 20] [--warmup 8] [--rounds 4]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yolo_deepsort_amd import _lib, pipeline as pl  # noqa: E402
from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, NMS_THRES, Workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--cold-steps", type=int, default=18)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identity_stream_bench.txt"))
    a = ap.parse_args()
    S, N, W = a.streams, a.steps, a.warmup
    total = W + N + a.cold_steps
    _lib.init()
    wl = Workload("cfg2", batch=S)
    L = len(wl.order)
    ring_index = lambda s, i: (s * (L // S) + i) % L     # noqa: E731
    stage = _lib.PinnedArray((S, wl.H, wl.W, 3), np.uint8)
    blocks = []
    for i in range(total):
        for s in range(S):
            stage.array[s] = wl.ring[ring_index(s, i)]
        blocks.append(_lib.DeviceBuffer.from_array(stage.array))
    pl.load_injection_sets(wl.net, [[wl.inj[wl.order[ring_index(s, i)]] for s in range(S)] for i in range(total)])
    stream_of = list(range(S))

    def pipeline():
        trackers = [wl.ds.clone() for _ in range(S)]
        mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
        mp.set_schedule(256)
        pl.select_injection_set(wl.net, 0)
        return mp, trackers

    def step(mp, i, last):
        """step i; `last`: nothing is handed over, so that no look-ahead pass is in flight afterwards"""
        nxt = None if last or i + 1 >= total else blocks[i + 1].ptr
        t0 = time.perf_counter()
        mp.step(blocks[i].ptr, wl.H, wl.W, stream_of, nxt, select_next=(i + 1 if nxt is not None else None))
        t1 = time.perf_counter()
        if nxt is None and i + 1 < total:
            pl.select_injection_set(wl.net, i + 1)         # (the next step's pass is not enqueued yet: it takes the set selected now)
        return t0 + (time.perf_counter() - t1)              # (the selection is no part of the step: the caller takes now - this)

    def leg(kind):
        mp, trackers = pipeline()
        if kind == "b":
            mp.set_identities(True).set_timing(True)
        plain, resolved, us, new, host = [], [], [], [], []
        for i in range(W + N):
            t0 = step(mp, i, i == W + N - 1)
            t1 = time.perf_counter()
            ids = mp.last_identities() if kind == "b" else None
            dt = time.perf_counter() - t0
            if i < W:
                continue
            host.append(time.perf_counter() - t1)
            u = mp.identities.last_us() if kind == "b" else None
            (plain if u is None else resolved).append(dt)
            if u is not None:
                c = mp.identities.last_counts()
                us.append(u)
                new.append(c[0] + c[1])
        n_ids = len({g for m in ids for g in m.values()}) if ids else 0
        n_tracks = sum(len(m) for m in ids) if ids else 0
        del mp, trackers
        return dict(step_ms=float(np.median(plain + resolved)) * 1e3, plain=plain, resolved=resolved, us=us, new=new,
                    host_ms=float(np.median(host)) * 1e3, n_ids=n_ids, n_tracks=n_tracks)

    runs, order_log = {"a": [], "b": []}, []
    for r in range(a.rounds):
        for kind in (("a", "b") if r % 2 == 0 else ("b", "a")):
            res = leg(kind)
            runs[kind].append(res)
            order_log.append("%s %.3f" % (kind, res["step_ms"]))
            print("round %d  %s median step %.3f ms  steps with a resolve sequence %d / %d" % (r, kind, res["step_ms"], len(res["resolved"]), N), flush=True)

    # ---- cold start: identities switched on over live tracks
    mp, trackers = pipeline()
    for i in range(W + N):
        step(mp, i, i == W + N - 1)
    t0 = time.perf_counter()
    ident = mp.set_identities(True)
    ident.set_timing(True)
    t_on = time.perf_counter() - t0
    cold = []
    for k in range(a.cold_steps):
        i = W + N + k
        t0 = step(mp, i, i == total - 1)
        dt = time.perf_counter() - t0
        c = ident.last_counts()
        cold.append((dt * 1e3, ident.last_us(), c))
        if c[2] == 0 and k > 0:
            break
    rows_per_track = int(np.median([len(t.tracker.gallery(0)) for t in trackers[:4]]))
    live = sum(len(m) for m in mp.last_identities())
    del mp, trackers

    a_ms = [x["step_ms"] for x in runs["a"]]
    b_ms = [x["step_ms"] for x in runs["b"]]
    a_med, b_med, spread = float(np.median(a_ms)), float(np.median(b_ms)), max(a_ms) - min(a_ms)
    inside = abs(b_med - a_med) <= spread
    plain = np.concatenate([x["plain"] for x in runs["b"]] or [[]]) * 1e3
    resolved = np.concatenate([x["resolved"] for x in runs["b"]] or [[]]) * 1e3
    us = np.concatenate([x["us"] for x in runs["b"]] or [[]])
    new = np.concatenate([x["new"] for x in runs["b"]] or [[]])
    lines = ["identity stage in a many-camera step, measured on ONE MI355X box in ONE invocation of tools/identity_stream_bench.py "
             "(--streams %d --steps %d --warmup %d --rounds %d)" % (S, N, W, a.rounds),
             "cfg2, %d streams x 1 frame per step, 30 persons per frame, frames resident in HBM, look-ahead, schedule fixed (serialized)" % S,
             "figure per run: median wall time of %d timed steps after %d warm-up steps; per leg: median [min, max] over its runs" % (N, W),
             "run order (leg, ms): " + ", ".join(order_log), "",
             "a   no identities              %8.3f ms [%.3f, %.3f] over %d runs; run-to-run spread (max - min) %.3f ms = %.2f %%"
             % (a_med, min(a_ms), max(a_ms), len(a_ms), spread, 100 * spread / a_med),
             "b   identity stage + last_identities() %8.3f ms [%.3f, %.3f] over %d runs   b - a = %+.3f ms (%+.2f %%): %s the spread of a"
             % (b_med, min(b_ms), max(b_ms), len(b_ms), b_med - a_med, 100 * (b_med - a_med) / a_med, "INSIDE" if inside else "OUTSIDE"),
             "    host time of last_identities() per step (68 streams, after step() returned): median of runs %.3f ms"
             % float(np.median([x["host_ms"] for x in runs["b"]])),
             "    at the end of a run: %d live Confirmed tracks hold %d distinct global ids" % (runs["b"][0]["n_tracks"], runs["b"][0]["n_ids"])]
    if len(resolved) and len(plain):
        lines += ["    timed steps of b without a resolve sequence (collect launch only, no extra synchronisation): %d, median %.3f ms" % (len(plain), float(np.median(plain))),
                  "    timed steps of b WITH one (new tracks admitted, one more synchronisation):                  %d, median %.3f ms" % (len(resolved), float(np.median(resolved))),
                  "    difference of the two medians = what the sequence and its synchronisation cost such a step: %+.3f ms" % float(np.median(resolved) - np.median(plain)),
                  "    device time of the resolve sequence in those steps (HIP events; %d steps, new tracks per step median %d [%d, %d]): median %.1f us [%.1f, %.1f]"
                  % (len(us), int(np.median(new)), int(new.min()), int(new.max()), float(np.median(us)), us.min(), us.max())]
    else:
        lines += ["    timed steps of b with a resolve sequence: %d, without: %d (one of the two classes is empty: no difference to report)" % (len(resolved), len(plain))]
    lines += ["", "cold start: %d steps without identities, then set_identities(True) (%.3f ms on the host) over %d live Confirmed tracks of about %d gallery rows each,"
              % (W + N, t_on * 1e3, live, rows_per_track),
              "max_rows = 4096 rows admitted per step, the rest deferred:",
              "    step  wall ms  resolve us  linked  fresh  deferred"]
    for k, (ms, u, c) in enumerate(cold):
        lines.append("    %4d  %7.3f  %10s  %6d  %5d  %8d" % (k, ms, "-" if u is None else "%.1f" % u, c[0], c[1], c[2]))
    cu = [u for _, u, _ in cold if u is not None]
    if cu:
        lines.append("    resolve sequence at the cold start: median %.1f us [%.1f, %.1f] over %d steps; a plain step of leg a: %.3f ms" % (float(np.median(cu)), min(cu), max(cu), len(cu), a_med))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
