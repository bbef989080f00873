"""A window setting per camera: wide 1080p cameras cut into 608 x 608 windows and 720p door cameras without windows, one frame of each
per step, in ONE slotted step against the alternative without yds_pipeline_set_stream_windows - in one run on one box.

  slotted  MultiStreamPipeline(stream_win_sizes=[(608, 608)] * wide + [None] * door).step_mixed: every window of the 1080p frames and
           every 720p frame is one network slot (8 * wide + door slots, one detector pass at the default 6 + 20 = 68 slots), one
           ragged NMS launch, one ReID pass, all trackers advanced together
  split    a MultiStreamPipeline(win_size=(608, 608)) over the 1080p cameras and a plain MultiStreamPipeline over the 720p cameras,
           stepped one after another (sharing the net and the extractor, each with its own look-ahead): two detector passes of 48 and
           20 slots, two NMS launches, two ReID passes

cfg2 (workload.py: yolov3 608 x 608, seeded weights, DeepSORT with the demo's parameters).  Camera s plays the workload's synthetic
1080p stream from its own offset; the 720p cameras see it sub-sampled (nearest pixel).  Head logits are injected per slot: per window
for a 1080p frame (a person goes into every window that holds its whole box), per frame for a 720p frame.  Frames resident in HBM,
the next step's frames handed over early.  Both legs see the same frames and tables.

Each leg runs twice, in the order slotted, split, split, slotted; each run is a child process under its own `timeout` (a run that
fails ends the whole measurement); the parent never opens the GPU.  Prints one JSON line: frames/s and median step time of every run,
the mean per leg and their ratio.

  python tools/stream_windows_bench.py [--wide 6 --door 20 --steps 16 --warmup 24] [--out profiles/stream_windows_bench.txt]
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
WIDE_HW, DOOR_HW = (1080, 1920), (720, 1280)
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
    from yolo_deepsort_amd import _lib, pipeline as pl
    from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, IMG, NMS_THRES, Workload
    _lib.init(0)
    nw, nd, N, W = a.wide, a.door, a.steps, a.warmup
    S, total = nw + nd, a.warmup + a.steps
    wins = windows(*WIDE_HW)
    T = len(wins)
    slots = nw * T + nd
    wl = Workload("cfg2", batch=slots)                                 # net.batch_max = all slots of a step: one pass in the slotted leg
    L = len(wl.order)
    heads = wl.net.yolo_heads()
    assert (wl.H, wl.W) == WIDE_HW

    def ring_index(s, i):                                              # camera s, step i: the workload's stream from the camera's own offset
        return (s * (L // S) + i) % L
    # ---- one block per step: the 1080p frames, then the 720p frames (sub-sampled), resident in HBM
    hw = np.array([WIDE_HW] * nw + [DOOR_HW] * nd, np.int32)
    sizes = hw[:, 0].astype(np.uint64) * hw[:, 1].astype(np.uint64) * np.uint64(3)
    off = np.zeros(S, np.uint64)
    off[1:] = np.cumsum(sizes)[:-1]
    nbytes = int(sizes.sum())
    ys, xs = (np.arange(DOOR_HW[0]) * WIDE_HW[0]) // DOOR_HW[0], (np.arange(DOOR_HW[1]) * WIDE_HW[1]) // DOOR_HW[1]
    stage = _lib.PinnedArray((nbytes,), np.uint8)
    blocks = []
    for i in range(total):
        for s in range(S):
            f = wl.ring[ring_index(s, i)]
            stage.array[int(off[s]):int(off[s] + sizes[s])] = (f if s < nw else f[ys][:, xs]).reshape(-1)
        blocks.append(_lib.DeviceBuffer.from_array(stage.array))
    wide_tabs = {t: window_tables(wl.scene.boxes(t)[1], wins, heads, IMG) for t in set(wl.order)}
    wide = lambda s, i: wide_tabs[wl.order[ring_index(s, i)]]          # noqa: E731  T tables
    door = lambda s, i: wl.inj[wl.order[ring_index(s, i)]]             # noqa: E731  (model-pixel boxes: the same at every size)
    out = dict(leg=a.leg, wide=nw, door=nd, windows_per_wide_frame=T, slots_per_step=slots, frames_per_step=S, steps=N, warmup=W)
    rows, dts = [0], []

    def timed(run_step):
        for i in range(total):
            t0 = time.perf_counter()
            if i == W:
                t_start = t0
            n = run_step(i)
            if i >= W:
                dts.append(time.perf_counter() - t0)
                rows[0] += n
        wall = time.perf_counter() - t_start
        out.update(fps=round(S * N / wall, 1), step_ms_median=round(float(np.median(dts)) * 1e3, 3), rows_per_frame=round(rows[0] / (S * N), 1))

    count = lambda res: sum(0 if r is None else len(r) for r in res)    # noqa: E731
    if a.leg == "slotted":
        pl.load_injection_sets(wl.net, [[tab for s in range(nw) for tab in wide(s, i)] + [door(s, i) for s in range(nw, S)] for i in range(total)])
        pipe = pl.MultiStreamPipeline(wl.net, [wl.ds.clone() for _ in range(S)], CONF_THRES, NMS_THRES, class_mask=CLASS_MASK,
                                      stream_win_sizes=[WIN] * nw + [None] * nd, overlap=OVERLAP)
        pl.select_injection_set(wl.net, 0)

        def step(i):
            nxt = blocks[i + 1].ptr if i + 1 < total else None
            return count(pipe.step_mixed(blocks[i].ptr, off, hw, list(range(S)), nbytes, nxt, select_next=(i + 1 if nxt is not None else None)))
        timed(step)
        out.update(stage_us=pipe.stage_us(), schedule=pipe.last_schedule())
    else:
        # injection set 2 i = the windowed pipeline's step i, 2 i + 1 = the plain pipeline's
        sets = []
        for i in range(total):
            sets.append([tab for s in range(nw) for tab in wide(s, i)] + [EMPTY] * nd)
            sets.append([door(s, i) for s in range(nw, S)] + [EMPTY] * (slots - nd))
        pl.load_injection_sets(wl.net, sets)
        pw = pl.MultiStreamPipeline(wl.net, [wl.ds.clone() for _ in range(nw)], CONF_THRES, NMS_THRES, class_mask=CLASS_MASK, win_size=WIN,
                                    overlap=OVERLAP)
        pd = pl.MultiStreamPipeline(wl.net, [wl.ds.clone() for _ in range(nd)], CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
        at = int(off[nw])

        def step(i):
            last = i + 1 >= total
            # the look-ahead pass of a pipeline's next step is enqueued inside its call, the other pipeline's pass runs in between: the set
            # of the pass enqueued NOW is selected before every call
            pl.select_injection_set(wl.net, 2 * i)
            n = count(pw.step(blocks[i].ptr, WIDE_HW[0], WIDE_HW[1], list(range(nw)), None if last else blocks[i + 1].ptr,
                              select_next=(None if last else 2 * (i + 1))))
            pl.select_injection_set(wl.net, 2 * i + 1)
            return n + count(pd.step(blocks[i].offset(at), DOOR_HW[0], DOOR_HW[1], list(range(nd)), None if last else blocks[i + 1].offset(at),
                                     select_next=(None if last else 2 * (i + 1) + 1)))
        timed(step)
        out.update(stage_us_windowed=pw.stage_us(), stage_us_plain=pd.stage_us())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", type=int, default=6, help="1080p cameras, cut into 608 x 608 windows (8 each)")
    ap.add_argument("--door", type=int, default=20, help="720p cameras, no windows")
    ap.add_argument("--steps", type=int, default=16, help="timed steps per run")
    ap.add_argument("--warmup", type=int, default=24, help="untimed steps per run (the schedule trial needs 20 steady-state steps)")
    ap.add_argument("--run-timeout", type=int, default=200, help="seconds each run may take (its own `timeout`)")
    ap.add_argument("--out", help="also append the result line to this file")
    ap.add_argument("--leg", choices=["slotted", "split"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    runs = []
    for name in ("slotted", "split", "split", "slotted"):
        cmd = ["timeout", "-k", "10", str(a.run_timeout), sys.executable, os.path.abspath(__file__), "--leg", name, "--wide", str(a.wide),
               "--door", str(a.door), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:                                           # nothing more is started on the GPU after a failed run
            print(json.dumps(dict(failed_run=name, returncode=r.returncode, runs=runs)), flush=True)
            return r.returncode
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    mean = {name: round(float(np.mean([r["fps"] for r in runs if r["leg"] == name])), 1) for name in ("slotted", "split")}
    line = json.dumps(dict(runs=runs, fps_mean=mean, slotted_over_split=round(mean["slotted"] / mean["split"], 3)))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
