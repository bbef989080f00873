#!/usr/bin/env python3
"""What the ground plane stage costs a many-camera step, and what render_view reaches; writes profiles/ground_bench.txt.

(a) The step.  Workload: cfg2 (yolov3 608 x 608 + DeepSORT), 68 streams x 1 frame per step, 30 persons per frame - the workload of
tools/heatmap_bench.py: every stream plays the workload's stream from its own offset, frames resident in HBM, the next step's frames
handed over (look-ahead), schedule fixed (serialized).  Every camera carries its own homography (a pinhole above the floor, a
different height, tilt and place per camera) onto ONE plan of 160 x 120 cells of 0.5 m.  Legs, each on a fresh
MultiStreamPipeline with fresh trackers over the SAME steps:

  a   the step without the stage - run TWICE per round: the difference between its runs is the run-to-run spread
  b   the step with the ground plane stage on the device (MultiStreamPipeline.set_ground)
  p   the step without the stage through ANOTHER build of the library (--parent-tag T: libydsort_T.so, built from the parent commit
      with YDS_BUILD_TAG=T) - left out, and said so, when that file is not there

A library is loaded once per process, so the legs run in two worker processes (this build: a and b; the other build: p) that the
driver starts once, lets set up the same workload, and then commands in turn: one box, one invocation, the legs alternating - a
round is a, b, p, a and every other round p, b, a, a.  Per run: W untimed warm-up steps, then N timed ones; the figure is the median
step wall time, and per leg the median over its runs is compared with the spread of a.  Leg b also reports the device time of the
update launch alone (HIP events around it, yds_ground_last_us).

(b) render_view alone.  68 frames of 1080 x 1920 resident in HBM, frame s a picture of camera s, the site grid as 200 steps of 30
walking persons per camera leave it.  Device time between HIP events around the two launches (levels + pixels), --render-iters
renders after 2 untimed ones.  Bytes = the pixels of every thread that changes one, read and written (a thread whose pixels all keep
the picture - sky, floor beyond the grid, k = 0 - neither loads nor stores); that is given as a share of 6.29 TB/s, the project's
streaming figure.  The kernel does two double divisions per pixel, so the time is also given per pixel.

  python tools/ground_bench.py [--streams 68] [--steps 20] [--warmup 8] [--rounds 3] [--render-iters 20] [--parent-tag parent]
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.29          # the project's streaming figure in TB/s
PLAN = dict(origin=(-40.0, 0.0), cell=0.5, gw=160, gh=120, scale=1000)


def camera_H(s, h, w):
    """Image to plan of camera s: a pinhole 3 .. 5 m up, tilted 20 .. 40 degrees, turned and moved about the plan."""
    t, height, f = math.radians(20 + (7 * s) % 21), 3.0 + (s % 5) * 0.5, 0.8 * w
    cx, cy = w / 2, h / 2
    P = np.array([[height, 0.0, -height * cx], [0.0, -height * math.sin(t), height * (f * math.cos(t) + cy * math.sin(t))],
                  [0.0, math.cos(t), f * math.sin(t) - cy * math.cos(t)]])
    a = math.radians((37 * s) % 90 - 45)
    T = np.array([[math.cos(a), -math.sin(a), -30.0 + (s % 8) * 8.0], [math.sin(a), math.cos(a), 5.0 + (s // 8) * 5.0], [0.0, 0.0, 1.0]])
    return T @ P


def specs_for(S, h, w):
    from yolo_deepsort_amd import ground as G
    return [G.GroundSpec(camera_H(s, h, w), class_id=0, **PLAN) for s in range(S)]


def walkers(seed, n, steps, h, w):
    """[rows int32 [n, 6], ...]: n persons walking a few pixels per step in the lower two thirds of the frame."""
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(0, w, n), rs.randint(h // 3, h, n)], 1)
    out = []
    for _ in range(steps):
        pos = np.clip(pos + rs.randint(-6, 7, (n, 2)), [0, h // 3], [w - 1, h - 1])
        out.append(np.stack([pos[:, 0] - 20, pos[:, 1] - 120, pos[:, 0] + 20, pos[:, 1], np.arange(1, n + 1), np.zeros(n, np.int64)], 1).astype(np.int32))
    return out


def worker(a):
    """Sets the workload up once, then runs the leg named on every line of stdin and answers with one JSON line."""
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
    stream_of = list(range(S))

    def leg(kind):
        trackers = [wl.ds.clone() for _ in range(S)]
        mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
        mp.set_schedule(256)
        if kind == "b":
            from yolo_deepsort_amd import ground as G
            mp.set_ground(G.DeviceGroundMap(specs_for(S, wl.H, wl.W), max_age=30, speed_window=8))
            mp.ground.set_timing(True)
        pl.select_injection_set(wl.net, 0)
        dts, launch, n_rows, n_rec, on_plan = [], [], 0, 0, 0
        for i in range(total):
            nxt = blocks[i + 1].ptr if i + 1 < total else None
            t0 = time.perf_counter()
            outs = mp.step(blocks[i].ptr, wl.H, wl.W, stream_of, nxt, select_next=(i + 1 if nxt is not None else None))
            dt = time.perf_counter() - t0
            if i >= W:
                dts.append(dt)
                n_rows += sum(0 if o is None else len(o) for o in outs)
                if kind == "b":
                    launch.append(mp.ground.last_us("update"))
                    recs = [r for r in mp.last_ground() if r is not None]
                    n_rec += sum(len(r) for r in recs)
                    on_plan += sum(int((r[:, 7] >= 0).sum()) for r in recs)
        presence = int(mp.ground_layers("presence").sum()) if kind == "b" else 0
        del mp, trackers
        return dict(step_ms=float(np.median(dts)) * 1e3, rows=n_rows, records=n_rec, in_grid=on_plan, presence=presence, launch_us=launch)

    print(json.dumps(dict(ready=True, h=wl.H, w=wl.W)), flush=True)
    for line in sys.stdin:
        kind = line.strip()
        if kind == "quit":
            break
        print(json.dumps(leg(kind)), flush=True)


def render_part(S, h, w, iters):
    """dict(us=[...], threads=fraction of the 16-pixel threads that change a pixel, changed=fraction of frame 0's pixels)."""
    from yolo_deepsort_amd import _lib, ground as G
    specs = specs_for(S, h, w)
    dev = G.DeviceGroundMap(specs, max_age=30, speed_window=8)
    walks = [walkers(100 + s, 30, 200, h, w) for s in range(S)]
    for t in range(200):
        dev.update_batch([walks[s][t] for s in range(S)], list(range(S)), [t / 25.0] * S)
    grid = dev.layer("presence")
    frames = np.random.RandomState(1).randint(0, 256, (S, h, w, 3)).astype(np.uint8)
    buf = _lib.DeviceBuffer.from_array(frames)
    from yolo_deepsort_amd.heatmap import levels
    threads, changed0 = [], 0.0
    for s in range(0, S, max(S // 4, 1)):                     # four cameras stand for all
        k = G.view_field(specs[s], h, w, levels(grid))[0]
        threads.append(float((k.reshape(h, w // 16, 16) > 0).any(axis=2).mean()))
        if s == 0:
            changed0 = float((k > 0).mean())
    slots, us = list(range(S)), []
    dev.set_timing(True)
    for it in range(iters + 2):
        dev.render_view(buf.ptr, slots, slots, h, w, layer="presence", alpha=128, n_frames=S)
        if it >= 2:                                          # two untimed renders first
            us.append(dev.last_us("render"))
    got = np.zeros_like(frames[:1])
    _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(got), buf.ptr, got.nbytes))
    assert changed0 == 0.0 or not np.array_equal(got[0], frames[0])       # (guards against measuring nothing)
    dev.close()
    return dict(us=us, threads=float(np.mean(threads)), changed=changed0, cells=int((grid > 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--render-iters", type=int, default=20)
    ap.add_argument("--parent-tag", default="parent")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground_bench.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    S, N, W = a.streams, a.steps, a.warmup
    parent_lib = os.path.join(ROOT, "yolo_deepsort_amd", "libydsort_%s.so" % a.parent_tag)
    have_parent = os.path.exists(parent_lib)

    def start(tag):
        env = dict(os.environ)
        env.pop("YDS_BUILD_TAG", None)
        if tag:
            env["YDS_BUILD_TAG"] = tag
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--streams", str(S), "--steps", str(N), "--warmup", str(W)]
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
                print("round %d  %s median step %.3f ms  rows %d  records %d" % (r, name, res["step_ms"], res["rows"], res["records"]), flush=True)
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
    us = np.concatenate([x["launch_us"] for x in runs["b"]])
    first = runs["b"][0]
    lines = ["ground plane, measured on ONE MI355X box in ONE invocation of tools/ground_bench.py "
             "(--streams %d --steps %d --warmup %d --rounds %d --render-iters %d)" % (S, N, W, a.rounds, a.render_iters), "",
             "(a) the stage in a many-camera step: cfg2, %d streams x 1 frame per step, 30 persons per frame, a homography per camera onto one "
             "plan of %d x %d cells, frames of %d x %d resident in HBM, look-ahead, schedule fixed (serialized)" % (S, PLAN["gw"], PLAN["gh"], h, w),
             "figure per run: median wall time of %d timed steps after %d warm-up steps; per leg: median [min, max] over its runs" % (N, W),
             "run order (leg, ms): " + ", ".join(order_log), "",
             "a   no ground plane                       %8.3f ms [%.3f, %.3f] over %d runs; run-to-run spread (max - min) %.3f ms = %.2f %%"
             % (a_med, min(a_ms), max(a_ms), len(a_ms), spread, 100 * spread / a_med),
             "b   ground plane stage on the device      %8.3f ms [%.3f, %.3f] over %d runs; b - a = %+.3f ms (%+.2f %%): %s the spread of a"
             % (b_med, min(b_ms), max(b_ms), len(b_ms), b_med - a_med, 100 * (b_med - a_med) / a_med, "INSIDE" if inside else "OUTSIDE")]
    if have_parent:
        p_ms = [x["step_ms"] for x in runs["p"]]
        p_med = float(np.median(p_ms))
        lines.append("p   the parent commit's library, no stage %8.3f ms [%.3f, %.3f] over %d runs; a - p = %+.3f ms (%+.2f %%): %s the spread of a"
                     % (p_med, min(p_ms), max(p_ms), len(p_ms), a_med - p_med, 100 * (a_med - p_med) / p_med,
                        "INSIDE" if abs(a_med - p_med) <= spread else "OUTSIDE"))
    else:
        lines.append("p   the parent commit's library: NOT MEASURED (libydsort_%s.so is not there)" % a.parent_tag)
    lines += ["    one run's %d timed steps: %d tracker rows, %d ground records, %d of them inside the grid; presence summed over the site "
              "grid after the run (warm-up included): %d" % (N, first["rows"], first["records"], first["in_grid"], first["presence"]),
              "    device time of the update launch alone (HIP events, %d steps): median %.1f us [%.1f, %.1f]"
              % (len(us), float(np.median(us)), us.min(), us.max()),
              "measured: the difference b - a lies %s the run-to-run spread of a" % ("inside" if inside else "OUTSIDE"), ""]
    from yolo_deepsort_amd import _lib
    _lib.init()
    rend = render_part(S, h, w, a.render_iters)
    t = np.array(rend["us"])
    px = S * h * w
    moved = px * 3 * 2 * rend["threads"]
    med = float(np.median(t))
    lines += ["(b) render_view alone: %d frames of %d x %d in HBM (%.0f MB), frame s a picture of camera s, layer presence (%d cells of the site "
              "grid positive), alpha 128, vmax 0; device time between HIP events around the two launches (levels + pixels), %d renders after 2 "
              "untimed ones" % (S, h, w, px * 3 / 1e6, rend["cells"], a.render_iters),
              "    median %8.1f us [%.1f, %.1f] = %.1f ps per pixel of %d pixels, each with two double divisions"
              % (med, t.min(), t.max(), med * 1e6 / px, px),
              "    threads of 16 pixels that change one (cameras 0, %d, ...: host count): %.1f %%; pixels of frame 0 changed: %.1f %%"
              % (max(S // 4, 1), 100 * rend["threads"], 100 * rend["changed"]),
              "    bytes = those threads' pixels read and written = %.0f MB: %.3f TB/s = %.1f %% of %.2f TB/s"
              % (moved / 1e6, moved / (med * 1e-6) / 1e12, 100 * moved / (med * 1e-6) / (STREAM_TBS * 1e12), STREAM_TBS),
              "    all %d frames' bytes once each way (%.0f MB) over the same time, for comparison with the heat map render: %.1f %% of %.2f TB/s"
              % (S, px * 6 / 1e6, 100 * px * 6 / (med * 1e-6) / (STREAM_TBS * 1e12), STREAM_TBS)]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
