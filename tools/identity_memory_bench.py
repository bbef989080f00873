#!/usr/bin/env python3
"""What the identity map's memory costs a many-camera step, and the bank distance kernel alone; writes
profiles/identity_memory_bench.txt.

Workload: that of tools/identity_stream_bench.py - cfg2 (yolov3 608 x 608 + DeepSORT), 68 streams x 1 frame per step, 30 persons per
frame, every stream playing the workload's stream from its own offset, frames resident in HBM, look-ahead, schedule fixed.  Legs, each
a child process of ONE invocation (a fresh pipeline and fresh trackers over the same steps), under its own time limit:

  b   identities on, memory off - this tree's library
  p   the same leg on the PARENT commit's library (built with YDS_BUILD_TAG=<--parent-tag> from the parent's sources and put next to
      the product library; skipped, and said so, when that file is absent).  b and p must agree within the spread of the runs.
  m   identities on with a memory of --ids x --rows, pre-filled by enrol with --ids departed identities (random unit rows): every
      step carries the bookkeeping and row-copy launches, a step that admits a track also the bank distance kernel and --ids more
      columns in its assignment
  k   the bank distance kernel alone (yds_identity_memory_bench: HIP events around each launch) on that bank at Q = 32, 128, 1024
      and every strip length of --strips; GB/s = bank rows read once / time, against the streaming HBM figure DESIGN.md uses

Runs go in rounds, the order of the legs rotated every round so that no leg always runs first.  Per run: W untimed warm-up steps,
then N timed ones; the figure is the median step wall time; spread = max - min over the runs of leg b.

  python tools/identity_memory_bench.py [--streams 68] [--steps 20] [--warmup 8] [--rounds 3] [--parent-tag parent]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 6.29                                           # measured streaming HBM bandwidth


def child_step_leg(a, memory):
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, NMS_THRES, Workload
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
    trackers = [wl.ds.clone() for _ in range(S)]
    mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
    mp.set_schedule(256)
    pl.select_injection_set(wl.net, 0)
    im = mp.set_identities(True, memory_ids=a.ids if memory else 0, memory_rows=a.rows)
    im.set_timing(True)
    if memory:
        v = np.random.RandomState(0).randn(a.ids, a.rows, 512).astype(np.float32)
        im.enrol(list(v))
    plain, resolved, us, new = [], [], [], []
    for i in range(total):
        nxt = None if i + 1 >= total else blocks[i + 1].ptr
        t0 = time.perf_counter()
        mp.step(blocks[i].ptr, wl.H, wl.W, list(range(S)), nxt, select_next=(i + 1 if nxt is not None else None))
        mp.last_identities()
        dt = time.perf_counter() - t0
        if i < W:
            continue
        u = im.last_us()
        (plain if u is None else resolved).append(dt * 1e3)
        if u is not None:
            c = im.last_counts()
            us.append(u)
            new.append(c[0] + c[1])
    out = dict(step_ms=float(np.median(plain + resolved)), plain=plain, resolved=resolved, us=us, new=new)
    if memory:
        out["counts"] = im.last_memory_counts()
    print("RESULT " + json.dumps(out), flush=True)


def child_kernel_leg(a):
    import ctypes as C
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.deep_sort import _TrackerHandle
    from yolo_deepsort_amd.identity import IdentityMap
    _lib.init()
    im = IdentityMap([_TrackerHandle(0.3, 0.7, 30, 3, 40)], memory_ids=a.ids, memory_rows=a.rows)
    rng = np.random.RandomState(0)
    im.enrol(list(rng.randn(a.ids, a.rows, 512).astype(np.float32)))
    out = {}
    for Q in (32, 128, 1024):
        q = _lib.DeviceBuffer.from_array(np.ascontiguousarray(rng.randn(Q, 512).astype(np.float32)))
        for strip in a.strips:
            us = np.zeros(a.iters, np.float32)
            _lib.check(_lib.load().yds_identity_memory_bench(im.handle, C.c_void_p(q.ptr), Q, strip, a.iters, _lib.ptr(us)))
            out["%d/%d" % (Q, strip)] = [float(np.median(us[2:])), float(us[2:].min())]
    print("RESULT " + json.dumps(out), flush=True)


def run_child(a, leg, tag, limit):
    env = dict(os.environ)
    env.pop("YDS_BUILD_TAG", None)
    if tag:
        env["YDS_BUILD_TAG"] = tag
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--streams", str(a.streams), "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--ids", str(a.ids), "--rows", str(a.rows), "--iters", str(a.iters), "--strips", ",".join(map(str, a.strips))]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stdout.write(r.stdout[-3000:])
        raise SystemExit("leg %s ended with status %d: no further leg is started" % (leg, r.returncode))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ids", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--iters", type=int, default=22)
    ap.add_argument("--strips", type=lambda s: [int(v) for v in s.split(",")], default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--parent-tag", default="parent")
    ap.add_argument("--leg-limit", type=int, default=240)
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identity_memory_bench.txt"))
    a = ap.parse_args()
    if a.child == "k":
        return child_kernel_leg(a)
    if a.child:
        return child_step_leg(a, a.child == "m")
    have_parent = os.path.exists(os.path.join(ROOT, "yolo_deepsort_amd", "libydsort_%s.so" % a.parent_tag))
    legs = ["b", "p", "m"] if have_parent else ["b", "m"]
    runs, order_log = {k: [] for k in legs}, []
    for r in range(a.rounds):
        for leg in legs[r % len(legs):] + legs[:r % len(legs)]:
            res = run_child(a, "b" if leg == "p" else leg, a.parent_tag if leg == "p" else "", a.leg_limit)
            runs[leg].append(res)
            order_log.append("%s %.3f" % (leg, res["step_ms"]))
            print("round %d  %s median step %.3f ms  steps with a resolve sequence %d / %d" % (r, leg, res["step_ms"], len(res["resolved"]), a.steps), flush=True)
    kern = run_child(a, "k", "", a.leg_limit)

    med = {k: float(np.median([x["step_ms"] for x in v])) for k, v in runs.items()}
    lo = {k: min(x["step_ms"] for x in v) for k, v in runs.items()}
    hi = {k: max(x["step_ms"] for x in v) for k, v in runs.items()}
    spread = hi["b"] - lo["b"]
    cat = lambda leg, key: np.array([v for x in runs[leg] for v in x[key]], np.float64)      # noqa: E731
    S, N, W = a.streams, a.steps, a.warmup
    lines = ["identity memory in a many-camera step, measured on ONE MI355X box in ONE invocation of tools/identity_memory_bench.py "
             "(--streams %d --steps %d --warmup %d --rounds %d --ids %d --rows %d)" % (S, N, W, a.rounds, a.ids, a.rows),
             "cfg2, %d streams x 1 frame per step, 30 persons per frame, frames resident in HBM, look-ahead, schedule fixed (serialized)" % S,
             "every run is a process of its own; figure per run: median wall time (step + last_identities()) of %d timed steps after %d warm-up "
             "steps; per leg: median [min, max] over its runs" % (N, W),
             "run order (leg, ms): " + ", ".join(order_log), "",
             "(a) b   identities on, memory off, this tree   %8.3f ms [%.3f, %.3f] over %d runs; run-to-run spread (max - min) %.3f ms = %.2f %%"
             % (med["b"], lo["b"], hi["b"], len(runs["b"]), spread, 100 * spread / med["b"])]
    if have_parent:
        d = med["b"] - med["p"]
        lines.append("    p   the same leg, the parent commit's library %6.3f ms [%.3f, %.3f] over %d runs   b - p = %+.3f ms (%+.2f %%): %s the spread of b"
                     % (med["p"], lo["p"], hi["p"], len(runs["p"]), d, 100 * d / med["p"], "INSIDE" if abs(d) <= spread else "OUTSIDE"))
    else:
        lines.append("    p   the parent commit's library was not present (libydsort_%s.so): NOT MEASURED" % a.parent_tag)
    d = med["m"] - med["b"]
    lines.append("(b) m   memory %d x %d, %d departed ids enrolled  %8.3f ms [%.3f, %.3f] over %d runs   m - b = %+.3f ms per step (%+.2f %%): %s the spread of b"
                 % (a.ids, a.rows, a.ids, med["m"], lo["m"], hi["m"], len(runs["m"]), d, 100 * d / med["b"], "INSIDE" if abs(d) <= spread else "OUTSIDE"))
    lines.append("        memory counts after the last step of a run: %s" % json.dumps(runs["m"][0].get("counts")))
    for leg in ("b", "m"):
        pl_, rs = cat(leg, "plain"), cat(leg, "resolved")
        if len(pl_) and len(rs):
            lines.append("    %s   timed steps without a resolve sequence: %d, median %.3f ms; with one (a track was admitted): %d, median %.3f ms; difference %+.3f ms"
                         % (leg, len(pl_), float(np.median(pl_)), len(rs), float(np.median(rs)), float(np.median(rs) - np.median(pl_))))
        else:
            lines.append("    %s   timed steps without a resolve sequence: %d, with one: %d (one class is empty: no difference to report)" % (leg, len(pl_), len(rs)))
    lines.append("(c) device time of the resolve sequence (HIP events, gather .. resolve) in the timed steps that ran one:")
    for leg, what in (("b", "without the bank"), ("m", "with the bank: + bank distance kernel, + %d columns" % a.ids)):
        us, new = cat(leg, "us"), cat(leg, "new")
        if len(us):
            lines.append("    %s   %-52s %d steps, new tracks per step median %d [%d, %d]: median %.1f us [%.1f, %.1f]"
                         % (leg, what, len(us), int(np.median(new)), int(new.min()), int(new.max()), float(np.median(us)), us.min(), us.max()))
        else:
            lines.append("    %s   %-52s no timed step ran one: NOT MEASURED" % (leg, what))
    bank_bytes = a.ids * a.rows * 512 * 4
    lines += ["", "(d) ident_bank_dist_kernel alone on the %d x %d bank (%.1f MB of rows, every entry full), HIP events around each of %d launches (first 2 dropped):"
              % (a.ids, a.rows, bank_bytes / 1e6, a.iters),
              "    median us (GB/s of bank rows = rows read once / time; %% of the %.2f TB/s streaming figure of DESIGN.md) per strip length (bank tiles per workgroup)" % HBM_TBS,
              "    Q      " + "".join("strip %-2d             " % s for s in a.strips)]
    best = {}
    for Q in (32, 128, 1024):
        cells = []
        for s in a.strips:
            m = kern["%d/%d" % (Q, s)][0]
            gbs = bank_bytes / (m * 1e-6) / 1e9
            cells.append("%8.1f (%5.0f, %4.1f%%) " % (m, gbs, 100 * gbs / (HBM_TBS * 1e3)))
            best[Q] = min(best.get(Q, (1e30, 0)), (m, s))
        lines.append("    %-6d " % Q + "".join(cells))
    lines.append("    fastest strip length per Q: " + ", ".join("Q=%d: %d (%.1f us)" % (Q, s, m) for Q, (m, s) in best.items()))
    lines.append("    gallery_min_dist_kernel run over the same bank as one more GalleryDesc: NOT MEASURED (the 0.8 GB staging figure of the issue stays arithmetic)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
