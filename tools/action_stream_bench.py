#!/usr/bin/env python3
"""What the action stage costs a many-camera step, on the device and on the host; writes profiles/action_stream_bench.txt.

Workload: cfg2 (yolov3 608 x 608 + DeepSORT), 68 streams x 1 frame per step, 30 persons per frame - the `multi` leg of
tools/multi_stream_bench.py: every stream plays the workload's stream from its own offset, frames resident in HBM, the next step's
frames handed over (look-ahead).  Legs, each on a fresh MultiStreamPipeline with fresh trackers over the SAME steps:

  a   the step without actions - run TWICE per round: the difference between its runs is the run-to-run spread
  b   the step with the action stage on the device (MultiStreamPipeline.set_actions + last_actions() read every step)
  c   step (a) plus the host loop: ActionIdentify.clone() per stream, .update(rows, time) on every frame's returned rows

The step wall time is what a caller sees; with look-ahead the device works on the next step's detector pass while the host is
between two step() calls, so host time spent there shows in the wall time only once it exceeds that cover.  The host time of the
stage itself (b: last_actions(), c: the update loop) is therefore reported next to it.

One invocation runs --rounds rounds; a round is a, b, c, a with b and c swapped in every other round, so that no leg always runs
first or last (clock and temperature drift).  Two action sets: `demo` is the list of the demo script (video_deepsort.py:28-34:
TakeOff / Landing / Glide / FastCrossing on class 4, BreakInto on class 0, max_age 30, max_size 8) as it stands - the workload's
persons are class 0, so four of its predicates return at the class test - and `demo_class0` is the same list with every class set
to 0, so that every predicate walks the orbit.  The schedule is fixed (set_schedule(256): serialized) so that no leg's schedule
trial decides differently from another's.  Per leg: W untimed warm-up steps, then N timed ones; the figure is the median step wall
time, and per leg the median over the rounds is compared.  Leg b also reports the device time of the action launch alone (HIP
events around it), median / min / max over its timed steps.

  python tools/action_stream_bench.py [--streams 68] [--steps 20] [--warmup 8] [--rounds 3]
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yolo_deepsort_amd import _lib, action as A, pipeline as pl  # noqa: E402
from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, NMS_THRES, Workload  # noqa: E402


def demo_actions(cls=None):
    c = (lambda k: k) if cls is None else (lambda k: cls)
    return A.ActionIdentify([A.TakeOff(c(4), delta=(0, 1)), A.Landing(c(4), delta=(2, 2)), A.Glide(c(4), delta=(1, 2)),
                             A.FastCrossing(c(4), speed=0.2), A.BreakInto(c(0), timeout=2)], max_age=30, max_size=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "action_stream_bench.txt"))
    a = ap.parse_args()
    S, N, W = a.streams, a.steps, a.warmup
    total = W + N
    _lib.init()
    lib = _lib.load()
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

    def leg(kind, ident):
        """One run of a leg: dict(step_ms, rows, action_rows, launch_us)."""
        trackers = [wl.ds.clone() for _ in range(S)]
        mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
        mp.set_schedule(256)
        clones = [ident.clone() for _ in range(S)] if kind == "c" else None
        if kind == "b":
            mp.set_actions(ident)
            _lib.check(lib.yds_actions_set_timing(mp.actions.handle, 1))
        pl.select_injection_set(wl.net, 0)
        dts, launch, host, n_rows, n_act = [], [], [], 0, 0
        us = C.c_float(0)
        for i in range(total):
            nxt = blocks[i + 1].ptr if i + 1 < total else None
            t0 = time.perf_counter()
            outs = mp.step(blocks[i].ptr, wl.H, wl.W, stream_of, nxt, select_next=(i + 1 if nxt is not None else None))
            t1 = time.perf_counter()
            if kind == "b":
                acts = mp.last_actions()
            elif kind == "c":
                acts = [clones[s].update(outs[s], i / 25.0) for s in range(S)]
            else:
                acts = []
            dt = time.perf_counter() - t0
            if i >= W:
                dts.append(dt)
                host.append(time.perf_counter() - t1)
                n_rows += sum(0 if o is None else len(o) for o in outs)
                n_act += sum(len(x) for x in acts if x)
                if kind == "b":
                    _lib.check(lib.yds_actions_last_us(mp.actions.handle, C.byref(us)))
                    launch.append(us.value)
        del mp, trackers
        return dict(step_ms=float(np.median(dts)) * 1e3, host_ms=float(np.median(host)) * 1e3, rows=n_rows, action_rows=n_act, launch_us=launch)

    sets = (("demo", demo_actions()), ("demo_class0", demo_actions(0)))
    runs = {}                                            # leg name -> list of run dicts, in the order they ran
    order_log = []
    for r in range(a.rounds):
        mid = [(k + "_" + name, k, ident) for name, ident in sets for k in ("b", "c")]
        if r % 2:
            mid.reverse()
        for name, kind, ident in [("a", "a", None)] + mid + [("a", "a", None)]:
            res = leg(kind, ident)
            runs.setdefault(name, []).append(res)
            order_log.append("%s %.3f" % (name, res["step_ms"]))
            print("round %d  %-14s median step %.3f ms  rows %d  action rows %d" % (r, name, res["step_ms"], res["rows"], res["action_rows"]),
                  flush=True)
    a_ms = [x["step_ms"] for x in runs["a"]]
    a_med, spread = float(np.median(a_ms)), max(a_ms) - min(a_ms)
    lines = ["action stage in a many-camera step, measured on ONE MI355X box in ONE invocation of tools/action_stream_bench.py "
             "(--streams %d --steps %d --warmup %d --rounds %d)" % (S, N, W, a.rounds),
             "cfg2, %d streams x 1 frame per step, 30 persons per frame, frames resident in HBM, look-ahead, schedule fixed (serialized)" % S,
             "figure per run: median wall time of %d timed steps after %d warm-up steps; per leg: median [min, max] over its runs" % (N, W),
             "run order (leg, ms): " + ", ".join(order_log), "",
             "a   no actions                 %8.3f ms [%.3f, %.3f] over %d runs; run-to-run spread (max - min) %.3f ms = %.2f %%"
             % (a_med, min(a_ms), max(a_ms), len(a_ms), spread, 100 * spread / a_med)]
    verdict = []
    for name, _ in sets:
        for k, what in (("b", "device stage + last_actions()"), ("c", "host ActionIdentify loop     ")):
            ms = [x["step_ms"] for x in runs[k + "_" + name]]
            med = float(np.median(ms))
            inside = abs(med - a_med) <= spread
            lines.append("%s   %-12s %s %8.3f ms [%.3f, %.3f]   %s - a = %+.3f ms (%+.2f %%): %s the spread of a;  %d action rows over %d tracker rows"
                         % (k, name, what, med, min(ms), max(ms), k, med - a_med, 100 * (med - a_med) / a_med, "INSIDE" if inside else "OUTSIDE",
                            runs[k + "_" + name][0]["action_rows"], runs[k + "_" + name][0]["rows"]))
            lines.append("    %-12s host time of that stage per step (after step() returned: %s): median of runs %.3f ms"
                         % (name, "last_actions()" if k == "b" else "68 clones' update()", float(np.median([x["host_ms"] for x in runs[k + "_" + name]]))))
            verdict.append((k, name, inside))
        us = np.concatenate([x["launch_us"] for x in runs["b_" + name]])
        lines.append("    %-12s device time of the action launch alone (HIP events, %d steps): median %.1f us [%.1f, %.1f]"
                     % (name, len(us), float(np.median(us)), us.min(), us.max()))
    lines += ["", "expectation: b - a inside the spread of a, c - a outside it.  measured: " +
              "; ".join("%s %s %s" % (k, name, "inside" if ins else "outside") for k, name, ins in verdict)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
