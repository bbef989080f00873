"""Sliding-window detection on 1080p video: the batched pipeline in window mode against the frame-by-frame loop, in ONE run on one box.

  window          Pipeline(win_size=(608, 608)): B frames per step, every frame cut into T = 8 windows on the device, the B * T windows
                  through the detector in one pass, one NMS launch (merge branch on the device), one ReID pass, the association -
                  frames resident in HBM, the next step's frames handed over early (csrc/pipeline.cpp window mode)
  frame_by_frame  ImageDetector(win_size=(608, 608)).detect + DeepSort.update per frame (VideoDetector.process: yds_detect_tiled
                  uploads the frame, runs its 8 windows, merges on the host) - the only way to run this workload without window mode

cfg2 (workload.py: yolov3 608 x 608, seeded weights, DeepSORT with the demo's parameters) on the synthetic 1080p stream.  The head
logits are injected per WINDOW: a person goes into every window that holds its whole box (persons astride a window border are seen
by the windows of the overlap or by none - the same for both legs).  Both legs see the same frames and tables in the same order.

Each leg is a child process under its own `timeout` (a leg that fails ends the run); the parent never opens the GPU.  Prints one
JSON line: frames/s and median time per step / frame of each leg and their ratio.

  python tools/window_pipeline_bench.py --frames-per-step 8 --steps 16 [--out profiles/window_pipeline_bench.txt]
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

WIN, OVERLAP = (608, 608), 0.15
EMPTY = np.zeros((0, 9), np.float32)


def windows(h, w):
    """img_detect.py:103-121: x, y, tile_h, tile_w on a win_size grid, x-major then y, extended by the overlap, clipped to the frame."""
    ox, oy = int(WIN[0] * OVERLAP), int(WIN[1] * OVERLAP)
    return [(x, y, min(y + WIN[1] + oy, h) - y, min(x + WIN[0] + ox, w) - x) for x in range(0, w, WIN[0]) for y in range(0, h, WIN[1])]


def window_tables(tlwh, wins, heads, img):
    from yolo_deepsort_amd import synth
    tables = []
    for x0, y0, th, tw in wins:
        inside = [b for b in tlwh if b[0] >= x0 and b[1] >= y0 and b[0] + b[2] <= x0 + tw and b[1] + b[3] <= y0 + th]
        if not inside:
            tables.append(EMPTY)
            continue
        local = np.array([[b[0] - x0, b[1] - y0, b[2], b[3]] for b in inside], np.float32)
        tables.append(synth.head_injection(local, (th, tw), (img, img), heads, cls=0))
    return tables


def leg(a):
    from yolo_deepsort_amd import _lib, cfgs, pipeline as pl
    from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, IMG, NMS_THRES, Workload
    _lib.init(0)
    B, N, W = a.frames_per_step, a.steps, a.warmup
    wins = windows(1080, 1920)
    T = len(wins)
    wl = Workload("cfg2", batch=B * T, n_distinct=max(4 * B, 32))       # net.batch_max = B * T: the windows of a step in ONE pass
    L = len(wl.order) // B * B                                          # frames in play order, whole steps
    heads = wl.net.yolo_heads()
    tabs = {t: window_tables(wl.scene.boxes(t)[1], wins, heads, IMG) for t in set(wl.order)}
    seen = float(np.mean([sum(len(r) for r in tabs[t]) for t in tabs]))
    out = dict(frames_per_step=B, windows_per_frame=T, steps=N, warmup=W, injected_boxes_per_frame=round(seen, 1))
    bm = wl.net.batch_max
    if a.leg == "window":
        n_sets = L // B
        pl.load_injection_sets(wl.net, [[tabs[wl.order[s * B + b]][t] for b in range(B) for t in range(T)] for s in range(n_sets)])
        pipe = pl.Pipeline(wl.net, wl.ds, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK, win_size=WIN, overlap=OVERLAP)
        dev = wl.to_device()
        pl.select_injection_set(wl.net, 0)
        rows, dts = 0, []
        for i in range(W + N):
            s, s_next = i % n_sets, (i + 1) % n_sets
            t0 = time.perf_counter()
            if i == W:
                t_start = t0
            res = pipe.step(dev.offset(s * B * wl.frame_bytes), wl.H, wl.W, B, dev.offset(s_next * B * wl.frame_bytes), select_next=s_next)
            if i >= W:
                dts.append(time.perf_counter() - t0)
                rows += sum(len(r) for r in res if r is not None)
        wall = time.perf_counter() - t_start
        out.update(fps=round(B * N / wall, 1), step_ms_median=round(float(np.median(dts)) * 1e3, 3), rows_per_frame=round(rows / (B * N), 1),
                   stage_us=pipe.stage_us(), schedule=pipe.last_schedule())
    else:
        import tempfile
        from yolo_deepsort_amd.detect import VideoDetector
        # one injection set per frame: its T window tables in the slots of the detector's one chunk
        pl.load_injection_sets(wl.net, [tabs[wl.order[f]] + [EMPTY] * (bm - T) for f in range(L)])
        with tempfile.NamedTemporaryFile("w", suffix=".names", delete=False) as f:
            f.write(cfgs.coco_names_text())
        vd = VideoDetector(wl.net, f.name, thres=CONF_THRES, nms_thres=NMS_THRES, tracker=wl.ds, class_mask=CLASS_MASK, win_size=WIN,
                           overlap=OVERLAP, batch_frames=1)
        os.unlink(f.name)
        rows, dts = 0, []
        for i in range((W + N) * B):
            k = i % L
            t0 = time.perf_counter()
            if i == W * B:
                t_start = t0
            pl.select_injection_set(wl.net, k)
            res = vd.process(wl.ring[k])
            if i >= W * B:
                dts.append(time.perf_counter() - t0)
                rows += 0 if res is None else len(res)
        wall = time.perf_counter() - t_start
        out.update(fps=round(B * N / wall, 1), frame_ms_median=round(float(np.median(dts)) * 1e3, 3), rows_per_frame=round(rows / (B * N), 1))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-per-step", type=int, default=8)
    ap.add_argument("--steps", type=int, default=16, help="timed steps of the window leg; the frame-by-frame leg times the same frames")
    ap.add_argument("--warmup", type=int, default=6, help="untimed steps per leg")
    ap.add_argument("--leg-timeout", type=int, default=240, help="seconds each leg may take (its own `timeout`)")
    ap.add_argument("--out", help="also append the result line to this file")
    ap.add_argument("--leg", choices=["window", "frame_by_frame"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    out = {}
    for name in ("window", "frame_by_frame"):
        cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name, "--frames-per-step",
               str(a.frames_per_step), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:                                           # nothing more is started on the GPU after a failed leg
            print(json.dumps(dict(failed_leg=name, returncode=r.returncode)), flush=True)
            return r.returncode
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    out["window_over_frame_by_frame"] = round(out["window"]["fps"] / out["frame_by_frame"]["fps"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
