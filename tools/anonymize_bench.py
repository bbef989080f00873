#!/usr/bin/env python3
"""What anonymised output costs (run on the GPU box): python tools/anonymize_bench.py [--rounds 5] [--runs 3] [--e2e-frames 2720]

1. One render of the output stage: 68 frames of 1080 x 1920 with the bench workload's 30 person boxes per frame
   (synth.PersonScene), through the BGR in-place entry (DeviceOverlay.render(bgr_frames=68)): privacy off, pixelate 16, pixelate 4,
   fill, region="head".  The legs alternate inside one process (the order rotates every round); `--runs` such processes alternate
   with processes that run the OFF leg on the PARENT commit's library (YDS_BUILD_TAG=parent: yolo_deepsort_amd/libydsort_parent.so,
   built from the parent's sources), so that "the off path did not change" is a comparison inside one invocation.
   render() is timed by the host clock around the call - it ends in a stream synchronise - and includes what Python does for it
   (box tables; with privacy: mask_rects and the CSR table).  The mask ALONE is timed through the C entry with prepacked tables
   (yds_anonymize_frames: host half + three small uploads + one launch + synchronise) next to the same call with one 1-pixel
   rectangle (the floor of such a call): the difference is the kernel and the tile list of the real table.
   Bytes: pixelate reads every cell a rectangle touches (whole) and writes the union U; fill reads nothing and writes U.
2. End to end: VideoDetector.detect frames/s on the value_video_detector workload of bench.py (reproduced here: the shim class,
   default arguments, a file-like BGR source, every result image consumed), anonymize off and on, alternating.
Everything is printed; nothing is asserted."""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, H, W, PERSONS = 68, 1080, 1920, 30
STREAM_TB_S = 6.29                       # the project's streaming figure (profiles/r01_ablation_dma.txt)


def _legs():
    from yolo_deepsort_amd.privacy import Anonymize
    return {"off": None, "pixelate16": Anonymize(block=16), "pixelate4": Anonymize(block=4), "fill": Anonymize(mode="fill", color=(0, 0, 0)),
            "head": Anonymize(block=16, region="head")}


def _scene():
    import numpy as np
    from yolo_deepsort_amd import synth
    scene = synth.PersonScene(PERSONS, seed=0)
    distinct = np.stack([scene.frame(t) for t in range(4)], 0)
    holds = []
    for t in range(N):
        ids, tlwh = scene.boxes(t)
        tlwh = np.asarray(tlwh, np.float64).reshape(-1, 4)
        holds.append(np.stack([tlwh[:, 0], tlwh[:, 1], tlwh[:, 0] + tlwh[:, 2], tlwh[:, 1] + tlwh[:, 3], np.asarray(ids) + 1, np.zeros(len(ids))],
                              1).astype(np.int32))
    return distinct, holds


def _traffic(anon, holds):
    """Bytes the mask of the whole batch reads and writes, from the rectangles."""
    import numpy as np
    from yolo_deepsort_amd import privacy
    rd = wr = rects_n = 0
    m = anon.block
    for hold in holds:
        rects = privacy.mask_rects(anon, H, W, hold, None)
        rects_n += len(rects)
        u = np.zeros((H, W), bool)
        cells = np.zeros(((H + m - 1) // m, (W + m - 1) // m), bool)
        for xa, ya, xb, yb in rects:
            x0, y0, x1, y1 = max(xa, 0), max(ya, 0), min(xb + 1, W), min(yb + 1, H)
            if x1 > x0 and y1 > y0:
                u[y0:y1, x0:x1] = True
                cells[y0 // m:(y1 - 1) // m + 1, x0 // m:(x1 - 1) // m + 1] = True
        wr += int(u.sum()) * 3
        if anon.mode == "pixelate":
            rd += int(np.repeat(np.repeat(cells, m, 0), m, 1)[:H, :W].sum()) * 3
    return rd, wr, rects_n


def child_render(names, rounds):
    import numpy as np
    from yolo_deepsort_amd import _lib, cfgs, privacy
    from yolo_deepsort_amd.label_draw import DeviceOverlay, LabelDrawer
    _lib.init()
    lib = _lib.load()
    distinct, holds = _scene()
    pin = _lib.PinnedArray((N, H, W, 3), np.uint8)
    for i in range(N):
        np.copyto(pin.array[i], distinct[i % len(distinct)][..., ::-1])                 # BGR, as a decoder delivers it
    dev = _lib.DeviceBuffer(pin.nbytes)
    ov = DeviceOverlay(LabelDrawer(cfgs.coco_names_text().split("\n")[:-1], None, 10, 2, (608, 608)))
    slots = list(range(N))
    fps = ["FPS: 1600"] * N
    legs = {k: v for k, v in _legs().items() if k in names}

    def stage():
        _lib.check(lib.yds_memcpy_h2d(dev.ptr, _lib.ptr(pin.array), pin.nbytes))        # (synchronous; the render consumes the frames)

    def render(anon):
        stage()
        t0 = time.perf_counter()
        if anon is None:
            out = ov.render(dev.offset(0), slots, H, W, holds, fps, bgr_frames=N)
        else:
            out = ov.render(dev.offset(0), slots, H, W, holds, fps, bgr_frames=N, privacy=anon, detections=None)
        dt = time.perf_counter() - t0
        del out
        return dt * 1e6

    tables = {}
    for k, anon in legs.items():
        if anon is not None:
            tables[k] = privacy.pack_rects([privacy.mask_rects(anon, H, W, h, None) for h in holds]) + privacy.device_args(anon, True)
    tiny = privacy.pack_rects([[(5, 5, 5, 5)]] * N) + (1, 16, 0)
    slot_a = np.ascontiguousarray(slots, dtype=np.int32)

    def alone(tab):
        stage()
        t0 = time.perf_counter()
        _lib.check(lib.yds_anonymize_frames(dev.ptr, N, _lib.ptr(slot_a), N, H, W, _lib.ptr(tab[0]), _lib.ptr(tab[1]), tab[2], tab[3], tab[4]))
        return (time.perf_counter() - t0) * 1e6

    order = list(legs)
    for k in order:                                                                     # warm every shape the timed rounds use
        render(legs[k])
        if k in tables:
            alone(tables[k])
    if tables:
        alone(tiny)
    res = {"render_us": {k: [] for k in order}, "alone_us": {k: [] for k in tables}, "alone_floor_us": []}
    for r in range(rounds):
        for k in order[r % len(order):] + order[:r % len(order)]:
            res["render_us"][k].append(render(legs[k]))
        for k in list(tables)[r % max(len(tables), 1):] + list(tables)[:r % max(len(tables), 1)]:
            res["alone_us"][k].append(alone(tables[k]))
        if tables:
            res["alone_floor_us"].append(alone(tiny))
    print("RESULT " + json.dumps(res))


class _ClipCapture:
    """cv2.VideoCapture protocol over frames held in memory (BGR), as in bench.py."""

    def __init__(self, frames_bgr, n, fps=25.0):
        self.frames, self.n, self.fps, self.pos = frames_bgr, n, fps, 0

    def isOpened(self):
        return True

    def get(self, prop):
        _, h, w = self.frames.shape[:3]
        return {5: self.fps, 6: 0.0, 3: float(w), 4: float(h), 7: float(self.n), 1: float(self.pos)}[prop]

    def set(self, prop, value):
        self.pos = int(value)

    def read(self):
        if self.pos >= self.n:
            return False, None
        f = self.frames[self.pos % len(self.frames)]
        self.pos += 1
        return True, f

    def release(self):
        pass


def _e2e_leg(anon, n_frames, config="cfg2", B=68):
    """bench.py video_detector_leg (a fresh Workload per leg, as there) with the anonymise option set as an attribute of the shim class."""
    import tempfile
    import numpy as np
    from yolo3.detect.video_detect import VideoDetector
    from yolo_deepsort_amd import cfgs, pipeline as pl
    from yolo_deepsort_amd.workload import Workload, CONF_THRES, NMS_THRES, CLASS_MASK
    wl = Workload(config, B, seed=0, n_distinct=4 * B)
    with tempfile.NamedTemporaryFile("w", suffix=".names", delete=False) as f:
        f.write(cfgs.coco_names_text())
    vd = VideoDetector(wl.net, f.name, thres=CONF_THRES, nms_thres=NMS_THRES, class_mask=CLASS_MASK, tracker=wl.ds, device_overlay=True)
    os.unlink(f.name)
    vd.AUTO_BATCH = B
    vd.anonymize = anon

    class InjectingPipeline(pl.Pipeline):
        i, sel = 0, None

        def step(self, frames_dev, h, w, batch, next_frames_dev=None, select_next=None):
            s_cur, s_next = self.i % wl.n_sets, (self.i + 1) % wl.n_sets
            if self.sel != s_cur:
                pl.select_injection_set(wl.net, s_cur)
            nxt = s_next if next_frames_dev is not None else None
            out = super().step(frames_dev, h, w, batch, next_frames_dev, select_next=nxt)
            self.sel, self.i = nxt, self.i + 1
            return out
    vd._pipe = InjectingPipeline(wl.net, wl.ds, CONF_THRES, NMS_THRES, class_mask=CLASS_MASK, cap=512)
    bgr = np.ascontiguousarray(wl.ring[..., ::-1])                                      # what a decoder delivers
    warm = 24 * B
    n, t0, t_last = 0, None, None
    for image, detections, actions in vd.detect(_ClipCapture(bgr, warm + n_frames), show_fps=True):
        n += 1
        if n == warm:
            t0 = time.perf_counter()
            vd.host_us.update({k: 0.0 for k in vd.host_us}, frames=0)
        elif n > warm:
            t_last = time.perf_counter()
    u = vd.host_us
    per = {k: round(u[k] / max(u["frames"], 1), 1) for k in ("wait_frames", "step", "wait_consumer", "wait_engine", "overlay")}
    del vd, wl
    gc.collect()
    return (n - warm) / (t_last - t0), per


def child_e2e(n_frames, pairs):
    from yolo_deepsort_amd import _lib
    from yolo_deepsort_amd.privacy import Anonymize
    _lib.init()
    res = {"off": [], "on": [], "us_per_frame": {}}
    for p in range(pairs):
        for name in (("off", "on") if p % 2 == 0 else ("on", "off")):
            fps, per = _e2e_leg(Anonymize() if name == "on" else None, n_frames)
            res[name].append(fps)
            res["us_per_frame"][name] = per
    print("RESULT " + json.dumps(res))


def _child(argv, tag=None):
    env = dict(os.environ)
    env.pop("YDS_BUILD_TAG", None)
    if tag:
        env["YDS_BUILD_TAG"] = tag
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, env=env, stdout=subprocess.PIPE, text=True, check=True).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def _med(v):
    return statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds of every leg inside one process")
    ap.add_argument("--runs", type=int, default=3, help="processes of this library, alternating with as many of the parent's (off leg)")
    ap.add_argument("--e2e-frames", type=int, default=2720, help="timed frames of an end-to-end leg (0: skip)")
    ap.add_argument("--e2e-pairs", type=int, default=3)
    ap.add_argument("--child", default=None)
    ap.add_argument("--legs", default="off,pixelate16,pixelate4,fill,head")
    args = ap.parse_args()
    if args.child == "render":
        return child_render(args.legs.split(","), args.rounds)
    if args.child == "e2e":
        return child_e2e(args.e2e_frames, args.e2e_pairs)
    parent_lib = os.path.join(ROOT, "yolo_deepsort_amd", "libydsort_parent.so")
    render, alone, floor, parent_off = {}, {}, [], []
    for r in range(args.runs):
        res = _child(["--child", "render", "--rounds", str(args.rounds), "--legs", args.legs])
        for k, v in res["render_us"].items():
            render.setdefault(k, []).extend(v)
        for k, v in res["alone_us"].items():
            alone.setdefault(k, []).extend(v)
        floor += res["alone_floor_us"]
        if os.path.exists(parent_lib):
            parent_off += _child(["--child", "render", "--rounds", str(args.rounds), "--legs", "off"], tag="parent")["render_us"]["off"]
    _, holds = _scene()
    print("anonymised output: %d frames of %d x %d, %d person boxes per frame, BGR in-place entry; %d runs x %d rounds per leg, alternating"
          % (N, H, W, PERSONS, args.runs, args.rounds))
    print("\n1a. DeviceOverlay.render(), host clock around the call (ends in a synchronise; includes Python's tables and the %d MB result copy)"
          % (N * H * W * 3 // 10 ** 6))
    off = render["off"]
    print("  %-12s median %9.0f us   min %9.0f   max %9.0f   (n = %d)" % ("off", _med(off), min(off), max(off), len(off)))
    if parent_off:
        print("  %-12s median %9.0f us   min %9.0f   max %9.0f   (n = %d)   parent commit's library, same script"
              % ("off/parent", _med(parent_off), min(parent_off), max(parent_off), len(parent_off)))
        d = _med(off) - _med(parent_off)
        print("  off - off/parent = %+.0f us; spread of the off leg (max - min) = %.0f us: the difference is %s the spread"
              % (d, max(off) - min(off), "INSIDE" if abs(d) <= max(off) - min(off) else "OUTSIDE"))
    else:
        print("  off/parent: not measured (no libydsort_parent.so)")
    for k in render:
        if k != "off":
            v = render[k]
            print("  %-12s median %9.0f us   min %9.0f   max %9.0f   added %+8.0f us" % (k, _med(v), min(v), max(v), _med(v) - _med(off)))
    print("\n1b. the mask alone: yds_anonymize_frames with prepacked tables (host half + uploads + one launch + synchronise)")
    print("  %-12s median %9.0f us   min %9.0f   max %9.0f   one 1-pixel rectangle per frame" % ("floor", _med(floor), min(floor), max(floor)))
    legs = _legs()
    for k, v in alone.items():
        rd, wr, n_rects = _traffic(legs[k], holds)
        add = _med(v) - _med(floor)
        rate = (rd + wr) / max(add, 1e-9) / 1e6                                         # bytes / us = MB/s ... / 1e6 = TB/s
        print("  %-12s median %9.0f us   min %9.0f   max %9.0f   over the floor %+7.0f us; %d rectangles, reads %.1f MB + writes %.1f MB "
              "=> %.3f TB/s = %.1f %% of %.2f TB/s" % (k, _med(v), min(v), max(v), add, n_rects, rd / 1e6, wr / 1e6, rate, 100 * rate / STREAM_TB_S,
                                                      STREAM_TB_S))
    if args.e2e_frames > 0:
        res = _child(["--child", "e2e", "--e2e-frames", str(args.e2e_frames), "--e2e-pairs", str(args.e2e_pairs)])
        a, b = res["off"], res["on"]
        print("\n2. VideoDetector.detect, bench.py's value_video_detector workload (cfg2, 68 frames per step, %d timed frames per leg), legs alternating"
              % args.e2e_frames)
        print("  anonymize=None        frames/s %s   median %.1f   spread %.1f" % ([round(v, 1) for v in a], _med(a), max(a) - min(a)))
        print("  anonymize=Anonymize() frames/s %s   median %.1f   spread %.1f" % ([round(v, 1) for v in b], _med(b), max(b) - min(b)))
        d, s = _med(b) - _med(a), max(max(a) - min(a), max(b) - min(b))
        print("  on - off = %+.1f frames/s (%+.2f %%): %s the spread of %.1f" % (d, 100 * d / _med(a), "INSIDE" if abs(d) <= s else "OUTSIDE", s))
        print("  us per frame by thread, off: %s" % json.dumps(res["us_per_frame"]["off"]))
        print("  us per frame by thread, on:  %s" % json.dumps(res["us_per_frame"]["on"]))


if __name__ == "__main__":
    main()
