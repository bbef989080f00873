#!/usr/bin/env python3
"""What the zone stage costs a many-camera step; writes profiles/zone_stream_bench.txt.

Workload: cfg2 (yolov3 608 x 608 + DeepSORT), 68 streams x 1 frame per step, 30 persons per frame - the workload of
tools/action_stream_bench.py: every stream plays the workload's stream from its own offset, frames resident in HBM, the next step's
frames handed over (look-ahead).  Every camera carries 4 zones and 4 lines in its own frame pixels.  Legs, each on a fresh
MultiStreamPipeline with fresh trackers over the SAME steps:

  a   the step without zones - run TWICE per round: the difference between its runs is the run-to-run spread
  b   the step with the zone stage on the device (MultiStreamPipeline.set_zones + last_zone_events() read every step)

One invocation runs --rounds rounds; a round is a, b, a and every other round b, a, a, so that no leg always runs first (clock and
temperature drift).  The schedule is fixed (set_schedule(256): serialized) so that no leg's schedule trial decides differently from
another's.  Per run: W untimed warm-up steps, then N timed ones; the figure is the median step wall time, and per leg the median over
its runs is compared with the spread of a.  Leg b also reports the device time of the zone launch alone (HIP events around it,
yds_zones_last_us), median / min / max over its timed steps, and the host time of last_zone_events().

  python tools/zone_stream_bench.py [--streams 68] [--steps 20] [--warmup 8] [--rounds 3]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yolo_deepsort_amd import _lib, pipeline as pl, zones as Z  # noqa: E402
from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, NMS_THRES, Workload  # noqa: E402


def camera_geometry(h, w):
    """4 zones and 4 lines of one camera: the left half, a concave area in the middle (debounced), the whole frame for persons, a
    box top right (debounced); two doorway lines for persons, a diagonal and a short segment."""
    zones = [Z.Zone([(0, 0), (w // 2, 0), (w // 2, h), (0, h)], name="left"),
             Z.Zone([(w // 4, h // 4), (3 * w // 4, h // 4), (w // 2, h // 2), (3 * w // 4, 3 * h // 4), (w // 4, 3 * h // 4)], class_id=0,
                    min_sightings=2, name="middle"),
             Z.Zone([(0, 0), (w, 0), (w, h), (0, h)], class_id=0, name="frame"),
             Z.Zone([(5 * w // 8, h // 8), (7 * w // 8, h // 8), (7 * w // 8, h // 2), (5 * w // 8, h // 2)], min_sightings=3, name="box")]
    lines = [Z.Line((w // 2, 0), (w // 2, h), class_id=0, name="door_x"), Z.Line((0, h // 2), (w, h // 2), class_id=0, name="door_y"),
             Z.Line((0, 0), (w, h), name="diagonal"), Z.Line((2 * w // 5, 2 * h // 5), (3 * w // 5, 2 * h // 5), name="gate")]
    return zones, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zone_stream_bench.txt"))
    a = ap.parse_args()
    S, N, W = a.streams, a.steps, a.warmup
    total = W + N
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
    geometry = camera_geometry(wl.H, wl.W)

    def leg(kind):
        """One run of a leg: dict(step_ms, host_ms, rows, events, kinds, launch_us)."""
        trackers = [wl.ds.clone() for _ in range(S)]
        mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
        mp.set_schedule(256)
        if kind == "b":
            mp.set_zones(Z.DeviceZoneMonitor(geometry, max_age=30, n_streams=S))
            mp.zones.set_timing(True)
        pl.select_injection_set(wl.net, 0)
        dts, launch, host, n_rows, kinds = [], [], [], 0, [0] * 5
        for i in range(total):
            nxt = blocks[i + 1].ptr if i + 1 < total else None
            t0 = time.perf_counter()
            outs = mp.step(blocks[i].ptr, wl.H, wl.W, stream_of, nxt, select_next=(i + 1 if nxt is not None else None))
            t1 = time.perf_counter()
            evs = mp.last_zone_events() if kind == "b" else []
            dt = time.perf_counter() - t0
            if i >= W:
                dts.append(dt)
                host.append(time.perf_counter() - t1)
                n_rows += sum(0 if o is None else len(o) for o in outs)
                for frame in evs:
                    for e in frame or []:
                        kinds[e[2]] += 1
                if kind == "b":
                    launch.append(mp.zones.last_us())
        del mp, trackers
        return dict(step_ms=float(np.median(dts)) * 1e3, host_ms=float(np.median(host)) * 1e3, rows=n_rows, events=sum(kinds), kinds=kinds,
                    launch_us=launch)

    runs, order_log = {}, []
    for r in range(a.rounds):
        for name in (("b", "a", "a") if r % 2 else ("a", "b", "a")):
            res = leg(name)
            runs.setdefault(name, []).append(res)
            order_log.append("%s %.3f" % (name, res["step_ms"]))
            print("round %d  %s median step %.3f ms  rows %d  zone events %d" % (r, name, res["step_ms"], res["rows"], res["events"]), flush=True)
    a_ms, b_ms = [x["step_ms"] for x in runs["a"]], [x["step_ms"] for x in runs["b"]]
    a_med, b_med, spread = float(np.median(a_ms)), float(np.median(b_ms)), max(a_ms) - min(a_ms)
    inside = abs(b_med - a_med) <= spread
    us = np.concatenate([x["launch_us"] for x in runs["b"]])
    first = runs["b"][0]
    lines = ["zone stage in a many-camera step, measured on ONE MI355X box in ONE invocation of tools/zone_stream_bench.py "
             "(--streams %d --steps %d --warmup %d --rounds %d)" % (S, N, W, a.rounds),
             "cfg2, %d streams x 1 frame per step, 30 persons per frame, 4 zones + 4 lines per camera, frames resident in HBM, look-ahead, "
             "schedule fixed (serialized)" % S,
             "figure per run: median wall time of %d timed steps after %d warm-up steps; per leg: median [min, max] over its runs" % (N, W),
             "run order (leg, ms): " + ", ".join(order_log), "",
             "a   no zones                              %8.3f ms [%.3f, %.3f] over %d runs; run-to-run spread (max - min) %.3f ms = %.2f %%"
             % (a_med, min(a_ms), max(a_ms), len(a_ms), spread, 100 * spread / a_med),
             "b   device stage + last_zone_events()     %8.3f ms [%.3f, %.3f] over %d runs; b - a = %+.3f ms (%+.2f %%): %s the spread of a"
             % (b_med, min(b_ms), max(b_ms), len(b_ms), b_med - a_med, 100 * (b_med - a_med) / a_med, "INSIDE" if inside else "OUTSIDE"),
             "    events of one run's %d timed steps: %d over %d tracker rows (enter %d, exit %d, lost %d, cross_fwd %d, cross_back %d)"
             % ((N, first["events"], first["rows"]) + tuple(first["kinds"])),
             "    host time per step after step() returned (last_zone_events()): median of runs %.3f ms"
             % float(np.median([x["host_ms"] for x in runs["b"]])),
             "    device time of the zone launch alone (HIP events, %d steps): median %.1f us [%.1f, %.1f]"
             % (len(us), float(np.median(us)), us.min(), us.max()), "",
             "measured: the difference b - a lies %s the run-to-run spread of a" % ("inside" if inside else "OUTSIDE")]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
