#!/usr/bin/env python3
"""What the snapshot stage costs a many-camera step, and where its time goes; writes profiles/snapshot_bench.txt.

Workloads: cfg2 (yolov3 608 x 608 + DeepSORT, 30 persons per frame) and the crowd workload cfg5 (yolov4, 150 detections per frame),
68 streams x 1 frame per step as in tools/ground_bench.py: every stream plays the workload's stream from its own offset, frames
resident in HBM, the next step's frames handed over (look-ahead), schedule fixed (serialized).  Legs, each on a fresh
MultiStreamPipeline with fresh trackers over the SAME steps:

  a   the step without the stage - run TWICE per round: the difference between its runs is the run-to-run spread
  b   the step with the snapshot stage on the device (MultiStreamPipeline.set_snapshots)
  p   the step without the stage through ANOTHER build of the library (--parent-tag T: libydsort_T.so, built from the parent commit
      with YDS_BUILD_TAG=T) - left out, and said so, when that file is not there

A library is loaded once per process, so the legs run in two worker processes (this build: a and b; the other build: p) that the
driver starts once per workload and then commands in turn: one box, one invocation, the legs alternating - a round is a, b, p, a and
every other round p, b, a, a.  Per run: W untimed warm-up steps, then N timed ones; the figure is the median step wall time, and per
leg the median over its runs is compared with the spread of a.  Leg b also reports, per step, the device time of the three launches
(HIP events, yds_snap_last_us), the pictures committed (BEST items), and the bytes the score kernel reads - per candidate row its
clipped region of the frame once, counted on the host from the step's rows - over its time as a share of 6.29 TB/s, the project's
streaming figure.

  python tools/snapshot_bench.py [--configs cfg2,cfg5] [--streams 68] [--steps 20] [--warmup 8] [--rounds 3] [--parent-tag parent]
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

STREAM_TBS = 6.29          # the project's streaming figure in TB/s


def worker(a):
    """Sets the workload up once, then runs the leg named on every line of stdin and answers with one JSON line."""
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, NMS_THRES, Workload
    S, N, W = a.streams, a.steps, a.warmup
    total = W + N
    _lib.init()
    wl = Workload(a.worker, batch=S)
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

    def leg(kind):
        trackers = [wl.ds.clone() for _ in range(S)]
        mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
        mp.set_schedule(256)
        spec = None
        if kind == "b":
            from yolo_deepsort_amd import snapshot as SN
            spec = SN.SnapSpec()
            mp.set_snapshots(SN.DeviceSnapshotBook(spec, max_age=30, n_streams=S))
            mp.snap.set_timing(True)
        pl.select_injection_set(wl.net, 0)
        dts, us, n_rows, best, closed, read_bytes, cand = [], [], 0, [], 0, [], 0
        for i in range(total):
            nxt = blocks[i + 1].ptr if i + 1 < total else None
            t0 = time.perf_counter()
            outs = mp.step(blocks[i].ptr, wl.H, wl.W, stream_of, nxt, select_next=(i + 1 if nxt is not None else None))
            dt = time.perf_counter() - t0
            if i >= W:
                dts.append(dt)
                n_rows += sum(0 if o is None else len(o) for o in outs)
                if kind == "b":
                    us.append([mp.snap.last_us(w) for w in ("score", "decide", "commit")])
                    ev = [e for e in mp.last_snapshot_events() if e is not None]
                    best.append(sum(int((e[:, 3] == 0).sum()) for e in ev))
                    closed += sum(int((e[:, 3] == 1).sum()) for e in ev)
                    nbytes = 0
                    for o in outs:
                        if o is None:
                            continue
                        o = o.astype(np.int64)
                        vw = np.minimum(o[:, 2], wl.W) - np.maximum(o[:, 0], 0)
                        vh = np.minimum(o[:, 3], wl.H) - np.maximum(o[:, 1], 0)
                        ok = (vw >= spec.min_w) & (vh >= spec.min_h)
                        nbytes += int((vw * vh * 3)[ok].sum())
                        cand += int(ok.sum())
                    read_bytes.append(nbytes)
        pool = [mp.snap.pool(s) for s in range(S)] if kind == "b" else []
        del mp, trackers
        return dict(step_ms=float(np.median(dts)) * 1e3, rows=n_rows, us=us, best=best, closed=closed, read_bytes=read_bytes, candidates=cand,
                    held=sum(n - f for f, n in pool), slots=sum(n for _, n in pool))

    print(json.dumps(dict(ready=True, h=wl.H, w=wl.W)), flush=True)
    for line in sys.stdin:
        kind = line.strip()
        if kind == "quit":
            break
        print(json.dumps(leg(kind)), flush=True)


def measure(a, config):
    S, N, W = a.streams, a.steps, a.warmup
    have_parent = os.path.exists(os.path.join(ROOT, "yolo_deepsort_amd", "libydsort_%s.so" % a.parent_tag))

    def start(tag):
        env = dict(os.environ)
        env.pop("YDS_BUILD_TAG", None)
        if tag:
            env["YDS_BUILD_TAG"] = tag
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", config, "--streams", str(S), "--steps", str(N), "--warmup", str(W)]
        return subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)

    def answer(proc):
        while True:
            line = proc.stdout.readline()
            if not line:
                raise RuntimeError("a worker ended early")
            if line.startswith("{"):
                return json.loads(line)
    procs = {"a": start("")}
    procs["b"] = procs["a"]
    if have_parent:
        procs["p"] = start(a.parent_tag)
    ready = [answer(p) for p in set(procs.values())]
    h, w = ready[0]["h"], ready[0]["w"]
    runs, order_log = {}, []
    try:
        for r in range(a.rounds):
            for name in (("p", "b", "a", "a") if r % 2 else ("a", "b", "p", "a")):
                if name not in procs:
                    continue
                procs[name].stdin.write(name + "\n")
                procs[name].stdin.flush()
                res = answer(procs[name])
                runs.setdefault(name, []).append(res)
                order_log.append("%s %.3f" % (name, res["step_ms"]))
                print("%s round %d  %s median step %.3f ms  rows %d" % (config, r, name, res["step_ms"], res["rows"]), flush=True)
    finally:
        for p in set(procs.values()):
            try:
                p.stdin.write("quit\n")
                p.stdin.flush()
                p.wait(timeout=60)
            except Exception:                                # noqa: BLE001 - a worker that is gone already
                p.kill()
    a_ms, b_ms = [x["step_ms"] for x in runs["a"]], [x["step_ms"] for x in runs["b"]]
    a_med, b_med, spread = float(np.median(a_ms)), float(np.median(b_ms)), max(a_ms) - min(a_ms)
    inside = abs(b_med - a_med) <= spread
    us = np.concatenate([np.array(x["us"]).reshape(-1, 3) for x in runs["b"]])
    best = np.concatenate([x["best"] for x in runs["b"]])
    read = np.concatenate([x["read_bytes"] for x in runs["b"]]).astype(np.float64)
    first = runs["b"][0]
    med = np.median(us, axis=0)
    share = float(np.median(read / (us[:, 0] * 1e-6))) / (STREAM_TBS * 1e12)
    lines = ["%s, %d streams x 1 frame per step, frames of %d x %d resident in HBM, look-ahead, schedule fixed (serialized)" % (config, S, h, w),
             "figure per run: median wall time of %d timed steps after %d warm-up steps; per leg: median [min, max] over its runs" % (N, W),
             "run order (leg, ms): " + ", ".join(order_log), "",
             "a   no snapshots                          %8.3f ms [%.3f, %.3f] over %d runs; run-to-run spread (max - min) %.3f ms = %.2f %%"
             % (a_med, min(a_ms), max(a_ms), len(a_ms), spread, 100 * spread / a_med),
             "b   snapshot stage on the device          %8.3f ms [%.3f, %.3f] over %d runs; b - a = %+.3f ms (%+.2f %%): %s the spread of a"
             % (b_med, min(b_ms), max(b_ms), len(b_ms), b_med - a_med, 100 * (b_med - a_med) / a_med, "INSIDE" if inside else "OUTSIDE")]
    if have_parent:
        p_ms = [x["step_ms"] for x in runs["p"]]
        p_med = float(np.median(p_ms))
        lines.append("p   the parent commit's library, no stage %8.3f ms [%.3f, %.3f] over %d runs; a - p = %+.3f ms (%+.2f %%): %s the spread of a"
                     % (p_med, min(p_ms), max(p_ms), len(p_ms), a_med - p_med, 100 * (a_med - p_med) / p_med,
                        "INSIDE" if abs(a_med - p_med) <= spread else "OUTSIDE"))
    else:
        lines.append("p   the parent commit's library: NOT MEASURED (libydsort_%s.so is not there)" % a.parent_tag)
    lines += ["    one run's %d timed steps: %d tracker rows, %d of them candidates, %d BEST items (pictures committed), %d CLOSED items"
              % (N, first["rows"], first["candidates"], int(np.sum(first["best"])), first["closed"]),
              "    pictures held after the run (live entries and archive rings, all streams): %d of %d pool slots = %.1f MB of HBM"
              % (first["held"], first["slots"], first["slots"] * 24576 / 1e6),
              "    device time of the three launches (HIP events, %d steps), median [min, max] us: score %.1f [%.1f, %.1f], decide %.1f [%.1f, %.1f], "
              "commit %.1f [%.1f, %.1f]; together %.1f us" % (len(us), med[0], us[:, 0].min(), us[:, 0].max(), med[1], us[:, 1].min(), us[:, 1].max(),
                                                             med[2], us[:, 2].min(), us[:, 2].max(), float(med.sum())),
              "    score kernel: %.2f MB of frame pixels read per step (every candidate's clipped region once) over its time: %.2f %% of %.2f TB/s"
              %(float(np.median(read)) / 1e6, 100 * share, STREAM_TBS),
              "    pictures committed per step: median %d [%d, %d]; the last five timed steps of the first run: %s"
              % (int(np.median(best)), best.min(), best.max(), first["best"][-5:]),
              "measured: the difference b - a lies %s the run-to-run spread of a" % ("inside" if inside else "OUTSIDE"), ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg5")
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tag", default="parent")
    ap.add_argument("--worker", default=None, help="(internal) run as the worker process of this workload")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_bench.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    lines = ["track snapshots, measured on ONE MI355X box in ONE invocation of tools/snapshot_bench.py "
             "(--configs %s --streams %d --steps %d --warmup %d --rounds %d)" % (a.configs, a.streams, a.steps, a.warmup, a.rounds), ""]
    for config in a.configs.split(","):
        lines += measure(a, config)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
