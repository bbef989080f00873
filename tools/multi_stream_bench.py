"""Many streams on one GPU (MultiStreamPipeline) against the two ways to serve them without it, in ONE run on one box.

  multi           S streams x F frames per step through MultiStreamPipeline: one detector pass and one ReID pass over S*F frames,
                  the S trackers advanced in the same grouped launches (csrc/tracker.hip TrackerGroup)
  single_batch    (a) the single-stream Pipeline at batch S*F on one stream - what bench.py measures
  sequential_b1   (b) for S <= 16: S single-stream Pipelines at batch 1, one after another, sharing the net and the extractor (today's
                  way to serve S live cameras)

Each of the S streams plays the workload's stream (workload.py, head logits injected) from its own offset, F consecutive frames per
step.  Frames are resident in HBM; W untimed warm-up steps per leg (the pipeline's schedule trial runs in them), then N timed steps.
Prints one JSON line: aggregate frames/s, median step wall time and stage_us (pipeline.cpp stage_us) per leg, and the ratios.

  python tools/multi_stream_bench.py --config cfg2 --streams 68 --frames-per-stream 1 --steps 20

--sizes HxW:N,HxW:N,...  cameras of different frame sizes (N streams per size; --streams is their sum).  Two legs instead:

  mixed           all streams through ONE MultiStreamPipeline.step_mixed: one detector pass and one ReID pass over every frame
  per_size        the alternative without it: one MultiStreamPipeline per size, stepped one after another (sharing the net and the
                  extractor), each over its own streams

The workload's 1080p frames are sub-sampled to each size (nearest pixel); the injected boxes are the same in model pixels, so every
size tracks the same scripted persons at its own scale.

  python tools/multi_stream_bench.py --config cfg2 --sizes 1080x1920:34,720x1280:34 --steps 20
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yolo_deepsort_amd import _lib, pipeline as pl  # noqa: E402
from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, NMS_THRES, Workload  # noqa: E402

EMPTY = np.zeros((0, 9), np.float32)


def timed(run_step, W, N, frames_per_step):
    for i in range(W):
        run_step(i)
    dts = []
    t0 = time.perf_counter()
    for i in range(W, W + N):
        t = time.perf_counter()
        run_step(i)
        dts.append(time.perf_counter() - t)
    wall = time.perf_counter() - t0
    return dict(fps=round(frames_per_step * N / wall, 1), step_ms_median=round(float(np.median(dts)) * 1e3, 3))


def run_sizes(a, groups):
    """--sizes: groups = [(h, w, n_streams)]"""
    F, N, W = a.frames_per_stream, a.steps, a.warmup
    S = sum(n for _, _, n in groups)
    B = S * F
    _lib.init(0)
    wl = Workload(a.config, batch=B)
    L = len(wl.order)
    total = W + N
    size_of = [(h, w) for h, w, n in groups for _ in range(n)]

    def ring_index(s, i, k):
        return (s * (L // S) + i * F + k) % L

    def sized(frame, h, w):                      # nearest-pixel sub-sampling of a workload frame (identity at its own size)
        if frame.shape[:2] == (h, w):
            return frame
        return frame[(np.arange(h) * frame.shape[0]) // h][:, (np.arange(w) * frame.shape[1]) // w]
    # ---- one block per step: stream after stream (a size group's frames are contiguous), resident in HBM
    off = np.zeros(B, np.uint64)
    hw = np.array([size_of[s] for s in range(S) for _ in range(F)], np.int32)
    sizes = hw[:, 0].astype(np.uint64) * hw[:, 1].astype(np.uint64) * np.uint64(3)
    off[1:] = np.cumsum(sizes)[:-1]
    nbytes = int(sizes.sum())
    stage = _lib.PinnedArray((nbytes,), np.uint8)
    blocks = []
    for i in range(total):
        for s in range(S):
            for k in range(F):
                b = s * F + k
                h, w = size_of[s]
                stage.array[int(off[b]):int(off[b] + sizes[b])] = sized(wl.ring[ring_index(s, i, k)], h, w).reshape(-1)
        blocks.append(_lib.DeviceBuffer.from_array(stage.array))
    inj = lambda s, i, k: wl.inj[wl.order[ring_index(s, i, k)]]          # noqa: E731  (model-pixel boxes: the same at every size)
    stream_of = [s for s in range(S) for _ in range(F)]
    out = dict(config=a.config, sizes=[dict(h=h, w=w, streams=n) for h, w, n in groups], streams=S, frames_per_stream=F, steps=N, warmup=W,
               frames_per_step=B)

    # ---- mixed: every size in one step
    pl.load_injection_sets(wl.net, [[inj(s, i, k) for s in range(S) for k in range(F)] for i in range(total)])
    trackers = [wl.ds.clone() for _ in range(S)]
    mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
    pl.select_injection_set(wl.net, 0)
    rows = [0]

    def mixed_step(i):
        nxt = blocks[i + 1].ptr if i + 1 < total else None
        res = mp.step_mixed(blocks[i].ptr, off, hw, stream_of, nbytes, nxt, select_next=(i + 1 if nxt is not None else None))
        rows[0] += sum(0 if r is None else len(r) for r in res)
    out["mixed"] = timed(mixed_step, W, N, B)
    out["mixed"]["stage_us"] = mp.stage_us()
    out["mixed"]["schedule"] = mp.last_schedule()
    out["mixed"]["rows"] = rows[0]
    del mp, trackers

    # ---- per_size: one MultiStreamPipeline per size, one after another; injection set i * G + g = step i of group g
    G = len(groups)
    first = np.cumsum([0] + [n for _, _, n in groups])
    pl.load_injection_sets(wl.net, [[inj(s, i, k) for s in range(first[g], first[g + 1]) for k in range(F)] + [EMPTY] * (B - groups[g][2] * F)
                                    for i in range(total) for g in range(G)])
    pipes = [pl.MultiStreamPipeline(wl.net, [wl.ds.clone() for _ in range(n)], CONF_THRES, NMS_THRES, class_mask=CLASS_MASK) for _, _, n in groups]
    rows = [0]

    def per_size_step(i):
        for g, (h, w, n) in enumerate(groups):
            # the look-ahead pass of this group's next step is enqueued inside this call; the other groups' passes run in between, so the
            # set of the pass enqueued NOW is selected before every call
            pl.select_injection_set(wl.net, i * G + g)
            at = int(off[first[g] * F])
            nxt = blocks[i + 1].offset(at) if i + 1 < total else None
            res = pipes[g].step(blocks[i].offset(at), h, w, [s for s in range(n) for _ in range(F)], nxt,
                                select_next=((i + 1) * G + g if nxt is not None else None))
            rows[0] += sum(0 if r is None else len(r) for r in res)
    out["per_size"] = timed(per_size_step, W, N, B)
    out["per_size"]["stage_us_last_group"] = pipes[-1].stage_us()
    out["per_size"]["rows"] = rows[0]
    out["mixed_over_per_size"] = round(out["mixed"]["fps"] / out["per_size"]["fps"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=["cfg2", "cfg3", "cfg5"])
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--frames-per-stream", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=24, help="untimed steps per leg (the schedule trial needs 20 steady-state steps)")
    ap.add_argument("--sizes", default=None, help="HxW:N,HxW:N,... cameras of different frame sizes, N streams each (see the module text)")
    a = ap.parse_args()
    if a.sizes:
        groups = [(int(hw.split("x")[0]), int(hw.split("x")[1]), int(n)) for hw, n in (g.split(":") for g in a.sizes.split(","))]
        return run_sizes(a, groups)
    S, F, N, W = a.streams, a.frames_per_stream, a.steps, a.warmup
    B = S * F
    _lib.init(0)
    wl = Workload(a.config, batch=B)
    L = len(wl.order)
    H, Wd, fb = wl.H, wl.W, wl.frame_bytes
    total = W + N

    def ring_index(s, i, k):                       # stream s, step i, frame k: the workload's stream from the stream's own offset
        return (s * (L // S) + i * F + k) % L
    # ---- the frames of every step, stream after stream, resident in HBM (one block per step)
    stage = _lib.PinnedArray((B, H, Wd, 3), np.uint8)
    blocks = []
    for i in range(total):
        for s in range(S):
            for k in range(F):
                stage.array[s * F + k] = wl.ring[ring_index(s, i, k)]
        blocks.append(_lib.DeviceBuffer.from_array(stage.array))
    inj = lambda s, i, k: wl.inj[wl.order[ring_index(s, i, k)]]          # noqa: E731
    stream_of = [s for s in range(S) for _ in range(F)]
    out = dict(config=a.config, streams=S, frames_per_stream=F, steps=N, warmup=W, frames_per_step=B)

    # ---- multi: MultiStreamPipeline
    pl.load_injection_sets(wl.net, [[inj(s, i, k) for s in range(S) for k in range(F)] for i in range(total)])
    trackers = [wl.ds.clone() for _ in range(S)]
    mp = pl.MultiStreamPipeline(wl.net, trackers, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
    pl.select_injection_set(wl.net, 0)

    def multi_step(i):
        nxt = blocks[i + 1].ptr if i + 1 < total else None
        mp.step(blocks[i].ptr, H, Wd, stream_of, nxt, select_next=(i + 1 if nxt is not None else None))
    out["multi"] = timed(multi_step, W, N, B)
    out["multi"]["stage_us"] = mp.stage_us()
    out["multi"]["schedule"] = mp.last_schedule()
    del mp, trackers

    # ---- (a) the single-stream Pipeline at batch S*F (the Workload's own stream and injection sets, as bench.py runs it)
    pl.load_injection_sets(wl.net, [[wl.inj[wl.order[s * B + b]] for b in range(B)] for s in range(wl.n_sets)])
    wl._sel = None
    out["single_batch"] = timed(lambda i: wl.step(i, prefetch=True), W, N, B)
    out["single_batch"]["stage_us"] = wl.pipe.stage_us()
    out["single_batch"]["schedule"] = wl.pipe.last_schedule()

    # ---- (b) S single-stream pipelines at batch 1, one after another, sharing the net and the extractor
    if S <= 16:
        bm = wl.net.batch_max
        pl.load_injection_sets(wl.net, [[inj(s, i, k)] + [EMPTY] * (bm - 1) for i in range(total) for s in range(S) for k in range(F)])
        pipes = [pl.Pipeline(wl.net, wl.ds.clone(), CONF_THRES, NMS_THRES, class_mask=CLASS_MASK) for _ in range(S)]

        def seq_step(i):
            for s in range(S):
                for k in range(F):
                    pl.select_injection_set(wl.net, (i * S + s) * F + k)
                    pipes[s].step(blocks[i].offset((s * F + k) * fb), H, Wd, 1)
        out["sequential_b1"] = timed(seq_step, min(W, 4), N, B)
        out["sequential_b1"]["stage_us"] = pipes[-1].stage_us()
        del pipes
    else:
        out["sequential_b1"] = None
    out["multi_over_single_batch"] = round(out["multi"]["fps"] / out["single_batch"]["fps"], 3)
    out["assoc_us_multi_over_single_batch"] = round(out["multi"]["stage_us"]["assoc_host"] / max(out["single_batch"]["stage_us"]["assoc_host"], 1e-3), 3)
    if out["sequential_b1"]:
        out["multi_over_sequential_b1"] = round(out["multi"]["fps"] / out["sequential_b1"]["fps"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
