#!/usr/bin/env python3
"""What the heat map stage costs a many-camera step, and what the device render reaches; writes profiles/heatmap_bench.txt.

(a) The step.  Workload: cfg2 (yolov3 608 x 608 + DeepSORT), 68 streams x 1 frame per step, 30 persons per frame - the workload of
tools/zone_stream_bench.py: every stream plays the workload's stream from its own offset, frames resident in HBM, the next step's
frames handed over (look-ahead).  Every camera carries a heat map at cell 16 over its own 1080 x 1920 frame.  Legs, each on a
fresh MultiStreamPipeline with fresh trackers over the SAME steps:

  a   the step without the stage - run TWICE per round: the difference between its runs is the run-to-run spread
  b   the step with the heat map stage on the device (MultiStreamPipeline.set_heatmap)

One invocation runs --rounds rounds; a round is a, b, a and every other round b, a, a, so that no leg always runs first (clock and
temperature drift).  The schedule is fixed (set_schedule(256): serialized).  Per run: W untimed warm-up steps, then N timed ones;
the figure is the median step wall time, and per leg the median over its runs is compared with the spread of a.  Leg b also
reports the device time of the update launch alone (HIP events around it, yds_heatmap_last_us).

(b) The render alone.  68 frames of 1080 x 1920 resident in HBM, one stream per frame.  Two grids: SPARSE - what 200 steps of 30
walking persons leave (most of the picture stays untouched: those pixels are read, not written) - and DENSE - every cell visited
(every pixel is read and written: 423 MB each way).  Cells 16 and 64, the legs alternating, --render-iters renders each; the figure
is the device time between HIP events around the two launches (levels + pixels).  Bytes over time are given as a fraction of
6.29 TB/s, the project's streaming figure, next to the anonymiser's 14 % (profiles/anonymize_bench.txt).

  python tools/heatmap_bench.py [--streams 68] [--steps 20] [--warmup 8] [--rounds 3] [--render-iters 20]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yolo_deepsort_amd import _lib, heatmap as H, pipeline as pl  # noqa: E402
from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, NMS_THRES, Workload  # noqa: E402

STREAM_TBS = 6.29          # the project's streaming figure in TB/s
ANONYMISER_PCT = 14        # what the anonymiser reached of it


def walkers(seed, n, steps, h, w):
    """[rows int32 [n, 6], ...]: n persons walking a few pixels per step inside the frame."""
    rs = np.random.RandomState(seed)
    pos = np.stack([rs.randint(0, w, n), rs.randint(0, h, n)], 1)
    out = []
    for _ in range(steps):
        pos = np.clip(pos + rs.randint(-6, 7, (n, 2)), 0, [w - 1, h - 1])
        out.append(np.stack([pos[:, 0] - 20, pos[:, 1] - 120, pos[:, 0] + 20, pos[:, 1], np.arange(1, n + 1), np.zeros(n, np.int64)], 1).astype(np.int32))
    return out


def render_part(S, h, w, iters):
    """{(grid, cell): dict(us=[...], written=fraction of the pixels that change)}, the legs alternating."""
    frames = np.random.RandomState(1).randint(0, 256, (S, h, w, 3)).astype(np.uint8)
    buf = _lib.DeviceBuffer.from_array(frames)
    maps = {}
    for cell in (16, 64):
        spec = H.HeatSpec(h, w, cell=cell, class_id=0)
        sparse = H.DeviceHeatMap(spec, max_age=30, n_streams=S)
        walks = [walkers(100 + s, 30, 200, h, w) for s in range(S)]
        for t in range(200):
            sparse.update_batch([walks[s][t] for s in range(S)], list(range(S)), [t / 25.0] * S)
        dense = H.DeviceHeatMap(spec, max_age=30, n_streams=S)
        rs = np.random.RandomState(cell)
        for t in range(3):                                   # every cell visited, with differing counts
            rows = [[x * cell + cell // 2 - 3, y * cell, x * cell + cell // 2 + 3, y * cell + cell // 2, 1 + y * spec.gw + x, 0]
                    for y in range(spec.gh) for x in range(spec.gw) if t == 0 or rs.rand() < 0.5]
            dense.update_batch([rows] * S, list(range(S)), [float(t)] * S)
        host = sparse.host(0)
        for t in range(200):
            host.update(walks[0][t], t / 25.0)
        want = H.render(frames[0], host.layer("presence"), cell)
        maps[("sparse", cell)] = (sparse, float((want != frames[0]).any(axis=2).mean()))
        maps[("dense", cell)] = (dense, 1.0)
        assert dense.layer(0, "presence").min() >= 1
    res = {k: dict(us=[], written=v[1]) for k, v in maps.items()}
    slots = list(range(S))
    for it in range(iters + 2):
        for key, (dev, _) in maps.items():
            dev.set_timing(True)
            dev.render(buf.ptr, slots, slots, h, w, layer="presence", alpha=128, n_frames=S)
            if it >= 2:                                      # two untimed rounds first
                res[key]["us"].append(dev.last_us("render"))
    # the first frame of the last sparse render against the host definition (the frames have been blended many times by now:
    # correctness is the tests' matter, this only guards the measurement against measuring nothing)
    got = np.zeros_like(frames[:1])
    _lib.check(_lib.load().yds_memcpy_d2h(_lib.ptr(got), buf.ptr, got.nbytes))
    assert not np.array_equal(got[0], frames[0])
    for dev, _ in maps.values():
        dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--render-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heatmap_bench.txt"))
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
    spec = H.HeatSpec(wl.H, wl.W, cell=16, class_id=0)

    def leg(kind):
        """One run of a leg: dict(step_ms, rows, presence, launch_us)."""
        trackers = [wl.ds.clone() for _ in range(S)]
        mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
        mp.set_schedule(256)
        if kind == "b":
            mp.set_heatmap(H.DeviceHeatMap(spec, max_age=30, n_streams=S))
            mp.heat.set_timing(True)
        pl.select_injection_set(wl.net, 0)
        dts, launch, n_rows = [], [], 0
        for i in range(total):
            nxt = blocks[i + 1].ptr if i + 1 < total else None
            t0 = time.perf_counter()
            outs = mp.step(blocks[i].ptr, wl.H, wl.W, stream_of, nxt, select_next=(i + 1 if nxt is not None else None))
            dt = time.perf_counter() - t0
            if i >= W:
                dts.append(dt)
                n_rows += sum(0 if o is None else len(o) for o in outs)
                if kind == "b":
                    launch.append(mp.heat.last_us("update"))
        presence = int(sum(mp.heatmap(s, "presence").sum() for s in range(S))) if kind == "b" else 0
        del mp, trackers
        return dict(step_ms=float(np.median(dts)) * 1e3, rows=n_rows, presence=presence, launch_us=launch)

    runs, order_log = {}, []
    for r in range(a.rounds):
        for name in (("b", "a", "a") if r % 2 else ("a", "b", "a")):
            res = leg(name)
            runs.setdefault(name, []).append(res)
            order_log.append("%s %.3f" % (name, res["step_ms"]))
            print("round %d  %s median step %.3f ms  rows %d  presence %d" % (r, name, res["step_ms"], res["rows"], res["presence"]), flush=True)
    a_ms, b_ms = [x["step_ms"] for x in runs["a"]], [x["step_ms"] for x in runs["b"]]
    a_med, b_med, spread = float(np.median(a_ms)), float(np.median(b_ms)), max(a_ms) - min(a_ms)
    inside = abs(b_med - a_med) <= spread
    us = np.concatenate([x["launch_us"] for x in runs["b"]])
    first = runs["b"][0]
    h, w = wl.H, wl.W
    blocks.clear()
    del wl
    rend = render_part(S, h, w, a.render_iters)
    px = S * h * w
    lines = ["heat maps, measured on ONE MI355X box in ONE invocation of tools/heatmap_bench.py "
             "(--streams %d --steps %d --warmup %d --rounds %d --render-iters %d)" % (S, N, W, a.rounds, a.render_iters), "",
             "(a) the stage in a many-camera step: cfg2, %d streams x 1 frame per step, 30 persons per frame, one %d x %d heat map at cell 16 "
             "per camera, frames resident in HBM, look-ahead, schedule fixed (serialized)" % (S, h, w),
             "figure per run: median wall time of %d timed steps after %d warm-up steps; per leg: median [min, max] over its runs" % (N, W),
             "run order (leg, ms): " + ", ".join(order_log), "",
             "a   no heat map                           %8.3f ms [%.3f, %.3f] over %d runs; run-to-run spread (max - min) %.3f ms = %.2f %%"
             % (a_med, min(a_ms), max(a_ms), len(a_ms), spread, 100 * spread / a_med),
             "b   heat map stage on the device          %8.3f ms [%.3f, %.3f] over %d runs; b - a = %+.3f ms (%+.2f %%): %s the spread of a"
             % (b_med, min(b_ms), max(b_ms), len(b_ms), b_med - a_med, 100 * (b_med - a_med) / a_med, "INSIDE" if inside else "OUTSIDE"),
             "    one run's %d timed steps: %d tracker rows; presence summed over the %d maps after the run (warm-up included): %d"
             % (N, first["rows"], S, first["presence"]),
             "    device time of the update launch alone (HIP events, %d steps): median %.1f us [%.1f, %.1f]"
             % (len(us), float(np.median(us)), us.min(), us.max()),
             "measured: the difference b - a lies %s the run-to-run spread of a" % ("inside" if inside else "OUTSIDE"), "",
             "(b) the render alone: %d frames of %d x %d in HBM (%.0f MB), layer presence, alpha 128, vmax 0; device time between HIP events "
             "around the two launches (levels + pixels), %d renders per leg after 2 untimed ones, legs alternating" % (S, h, w, px * 3 / 1e6, a.render_iters),
             "bytes = every pixel read + the changed pixels' threads written (a thread that changes nothing stores nothing); "
             "fraction of %.2f TB/s; the anonymiser reached %d %%" % (STREAM_TBS, ANONYMISER_PCT)]
    worst = 100.0
    for (grid, cell), r in sorted(rend.items()):
        t = np.array(r["us"])
        moved = px * 3 * (1 + r["written"])
        pct = 100 * moved / (float(np.median(t)) * 1e-6) / (STREAM_TBS * 1e12)
        worst = min(worst, pct)
        lines.append("    %-6s grid, cell %3d: median %8.1f us [%.1f, %.1f]; pixels changed %5.1f %%; >= %.0f MB moved: %5.2f TB/s = %4.1f %% of %.2f TB/s"
                     % (grid, cell, float(np.median(t)), t.min(), t.max(), 100 * r["written"], moved / 1e6, moved / (float(np.median(t)) * 1e-6) / 1e12,
                        pct, STREAM_TBS))
    lines.append("    (sparse: the changed fraction is that of frame 0 on the host and counts pixels, the device skips the store per thread of "
                 "16 pixels, so it writes somewhat more than counted: the figure is a lower bound)")
    lines.append("measured: the render's lowest leg reaches %.1f %% of the streaming figure, %s the anonymiser's %d %%"
                 % (worst, "ABOVE" if worst > ANONYMISER_PCT else "BELOW", ANONYMISER_PCT))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
