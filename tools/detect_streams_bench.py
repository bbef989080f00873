"""VideoDetector.detect_streams as a user calls it - the generator itself, frames/s over all yielded frames - in ONE run on one box.

Workload: the cfg of bench.py (--config cfg2) with S iterable sources x 1 frame per step, each source playing the workload's
stream from its own offset; one injection set is selected for the whole run (the detector sees the same scripted persons in every
pass: the generator offers no per-step injection), so every frame carries rows to draw.  Two workloads: `uniform` (all sources
1080 x 1920) and `mixed` (half 1080 x 1920, half 720 x 1280, mixed_sizes=True; the small frames are nearest-pixel sub-samples).

Legs, alternating, --runs of each (a run = one generator consumed to its end; the first --warmup yields are untimed):
  host        (a) device_overlay=False: the host loop - one upload per step on the caller's thread, step without look-ahead, host render per frame
  device      (b) device_overlay=True: reader thread + pinned staging, look-ahead, one DeviceOverlay.render / render_mixed per step
  device_anon (b) with anonymize=Anonymize()
  step        (c) the bare MultiStreamPipeline.step / step_mixed on the same frames resident in HBM, with look-ahead: the ceiling
  host_parent (a) again, on the PARENT commit: --parent-root DIR names a checkout of it with its library built; every host run is
              followed by a process that runs this file's host leg against that tree (YDS_BENCH_ROOT) - the confirmation that
              device_overlay=False still is the parent's detect_streams
Once per workload the rows of the first host run are compared with the first device run (`rows_equal`).
Per device leg: the render call's device time between two events on the overlay's stream (yds_overlay_set_timing: table uploads,
kernels and the D2H copy of the result), median over the timed steps, and the bytes it moves - read + write of every frame for the
reversed copy plus the read of the D2H copy = 3 x the frames' bytes - against the 6.29 TB/s streaming figure of the README.
Prints one JSON line per workload.

  python tools/detect_streams_bench.py --config cfg2 --streams 68 --runs 3
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

# YDS_BENCH_ROOT: the tree whose package is measured (the --parent-root legs run this file against another checkout)
sys.path.insert(0, os.environ.get("YDS_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from yolo_deepsort_amd import _lib, cfgs, pipeline as pl  # noqa: E402
from yolo_deepsort_amd.detect import VideoDetector  # noqa: E402
from yolo_deepsort_amd.privacy import Anonymize  # noqa: E402
from yolo_deepsort_amd.workload import CLASS_MASK, CONF_THRES, NMS_THRES, Workload  # noqa: E402

HBM_BPS = 6.29e12


def spread(v):
    return dict(median=round(float(np.median(v)), 1), min=round(float(min(v)), 1), max=round(float(max(v)), 1), runs=[round(float(x), 1) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=["cfg2", "cfg3", "cfg5"])
    ap.add_argument("--streams", type=int, default=68)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3, help="untimed yields at the start of every run")
    ap.add_argument("--host-steps", type=int, default=6, help="timed steps of a host run (it renders ~100 frames/s)")
    ap.add_argument("--device-steps", type=int, default=24, help="timed steps of a device run and of the bare step")
    ap.add_argument("--workloads", default="uniform,mixed")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: adds the host_parent leg")
    ap.add_argument("--host-leg-only", action="store_true", help="(used by --parent-root) one host run per workload, one JSON line each")
    a = ap.parse_args()
    S, W = a.streams, a.warmup
    _lib.init(0)
    lib = _lib.load()
    wl = Workload(a.config, batch=S, n_distinct=max(S, 32))
    L = len(wl.order)
    pl.load_injection_sets(wl.net, [[wl.inj[wl.order[b]] for b in range(S)]])
    pl.select_injection_set(wl.net, 0)
    names = os.path.join(tempfile.mkdtemp(), "coco.names")
    with open(names, "w") as f:
        f.write(cfgs.coco_names_text())
    H, Wd = wl.H, wl.W
    h2, w2 = 720, 1280
    small = None

    def frame(s, i, mixed):
        k = (s * (L // S) + i) % L
        return small[k] if mixed and s >= S // 2 else wl.ring[k]

    def detector(device, anon=None):
        return VideoDetector(wl.net, names, thres=CONF_THRES, nms_thres=NMS_THRES, tracker=wl.ds, class_mask=CLASS_MASK,
                             device_overlay=device, anonymize=anon)

    def run_generator(device, mixed, steps, anon=None, keep_rows=False):
        vd = detector(device, anon)
        sources = [(frame(s, i, mixed) for i in range(W + steps)) for s in range(S)]
        n, t0, us, rows = 0, None, [], []
        for k, out in enumerate(vd.detect_streams(sources, frames_per_stream=1, show_fps=True, mixed_sizes=mixed)):
            if k == W - 1:
                t0 = time.perf_counter()
            elif k >= W:
                n += len(out)
                if device:
                    v = np.zeros(1, np.float32)
                    _lib.check(lib.yds_overlay_last_us(_lib.ptr(v)))
                    us.append(float(v[0]))
            if keep_rows:
                rows.append([(s, None if det is None else np.array(det, np.int32).reshape(-1, 6)) for s, _, det, _ in out])
        wall = time.perf_counter() - t0
        return n / wall, us, rows, getattr(vd, "streams_lookahead", None)

    def run_step(mixed, steps):
        total = W + steps
        frames = [[frame(s, i, mixed) for s in range(S)] for i in range(2)]               # two blocks, alternating: the step reads, never writes
        block0, off, hw = pl.pack_frames(frames[0])
        blocks = [_lib.DeviceBuffer.from_array(block0), _lib.DeviceBuffer.from_array(pl.pack_frames(frames[1])[0])]
        mp = pl.MultiStreamPipeline(wl.net, [wl.ds.clone() for _ in range(S)], CONF_THRES, NMS_THRES, class_mask=CLASS_MASK)
        t0 = None
        for i in range(total):
            nxt = blocks[(i + 1) % 2].ptr if i + 1 < total else None
            if mixed:
                mp.step_mixed(blocks[i % 2].ptr, off, hw, list(range(S)), block0.nbytes, nxt)
            else:
                mp.step(blocks[i % 2].ptr, H, Wd, list(range(S)), nxt)
            if i == W - 1:
                t0 = time.perf_counter()
        return S * steps / (time.perf_counter() - t0)

    def parent_host_run(name):
        import subprocess
        env = dict(os.environ, YDS_BENCH_ROOT=os.path.abspath(a.parent_root))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-leg-only", "--config", a.config, "--streams", str(S),
                              "--warmup", str(W), "--host-steps", str(a.host_steps), "--workloads", name],
                             env=env, check=True, capture_output=True, text=True, timeout=300).stdout
        return json.loads(out.strip().splitlines()[-1])["fps"]

    if not a.host_leg_only:
        _lib.check(lib.yds_overlay_set_timing(1))
    for name in a.workloads.split(","):
        mixed = name == "mixed"
        if mixed and small is None:
            small = np.ascontiguousarray(wl.ring[:, (np.arange(h2) * H) // h2][:, :, (np.arange(w2) * Wd) // w2])
        if a.host_leg_only:
            print(json.dumps(dict(workload=name, fps=run_generator(False, mixed, a.host_steps)[0])), flush=True)
            continue
        res = dict(workload=name, config=a.config, streams=S, frames_per_stream=1, runs=a.runs, warmup=W, host_steps=a.host_steps,
                   device_steps=a.device_steps)
        fps = dict(host=[], device=[], device_anon=[], step=[])
        if a.parent_root:
            fps["host_parent"] = []
        render_us = dict(device=[], device_anon=[])
        rows = {}
        for r in range(a.runs):                                                          # alternating legs
            f, _, rw, _ = run_generator(False, mixed, a.host_steps, keep_rows=r == 0)
            fps["host"].append(f)
            if r == 0:
                rows["host"] = rw
            if a.parent_root:
                fps["host_parent"].append(parent_host_run(name))
            f, us, rw, ahead = run_generator(True, mixed, a.device_steps, keep_rows=r == 0)
            fps["device"].append(f)
            render_us["device"] += us
            res["lookahead_steps"] = ahead
            if r == 0:
                rows["device"] = rw
            f, us, _, _ = run_generator(True, mixed, a.device_steps, anon=Anonymize())
            fps["device_anon"].append(f)
            render_us["device_anon"] += us
            fps["step"].append(run_step(mixed, a.device_steps))
        k = min(len(rows["host"]), len(rows["device"]))
        res["rows_equal"] = bool(k > 0 and all(len(x) == len(y) and all(s == t and (d is None) == (e is None) and (d is None or np.array_equal(d, e))
                                                                         for (s, d), (t, e) in zip(x, y))
                                               for x, y in zip(rows["host"][:k], rows["device"][:k])))
        res["rows_compared_steps"] = k
        res["rows_drawn_per_step"] = int(np.mean([sum(0 if d is None else len(d) for _, d in st) for st in rows["device"][W:]] or [0]))
        res["fps"] = {leg: spread(v) for leg, v in fps.items()}
        frame_bytes = sum(3 * (h2 * w2 if mixed and s >= S // 2 else H * Wd) for s in range(S))
        res["render"] = {}
        for leg, us in render_us.items():
            med = float(np.median(us))
            res["render"][leg] = dict(device_us_median=round(med, 1), device_us_min=round(min(us), 1), device_us_max=round(max(us), 1),
                                      bytes_moved=3 * frame_bytes, gbps=round(3 * frame_bytes / med / 1e3, 1),
                                      fraction_of_hbm_stream=round(3 * frame_bytes / (med * 1e-6) / HBM_BPS, 4))
        res["device_over_host"] = round(res["fps"]["device"]["median"] / res["fps"]["host"]["median"], 2)
        res["device_beats_host_outside_spread"] = bool(res["fps"]["device"]["min"] > res["fps"]["host"]["max"])
        res["device_over_step"] = round(res["fps"]["device"]["median"] / res["fps"]["step"]["median"], 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
