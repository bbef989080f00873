"""Drop-in ``ImageDetector`` / ``VideoDetector`` (reference yolo3/detect/img_detect.py:36-153,
yolo3/detect/video_detect.py:39-208).  Only the per-frame hot glue is accelerated; video decode,
drawing and display stay host side and are optional (cv2 / imutils are not required to import this)."""

from __future__ import annotations

import logging
import os
import time
from functools import reduce

import numpy as np

from .action import as_device_actions
from .ground import as_device_ground
from .snapshot import as_device_snapshots
from .heatmap import as_device_heatmap
from .label_draw import LabelDrawer, put_text
from .loaders import load_classes
from .staging import (NOTHING, STAGE_ALIGN, Bookkeeper, give, same_composition, shut_down, skip_gate, stage_plan,  # noqa: F401 - part of this
                      stage_steps, stream_groups, take)                                                            # module's interface
from .track_stage import TrackStage
from .zones import as_device_zones


def p1p2Toxywh(x):
    """model_build.py:326-332"""
    y = np.empty_like(x)
    y[..., 0] = x[..., 0]
    y[..., 1] = x[..., 1]
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def _as_tensor(a):
    try:
        import torch
        return torch.from_numpy(a)
    except ImportError:
        return a


class ImageDetector:
    def __init__(self, model, class_path, thickness=2, thres=0.5, nms_thres=0.4, win_size=None, overlap=0.15,
                 half=False):
        self.model = model
        self.model.eval()
        self.device = next(self.model.parameters()).device
        if half:
            self.model.half()
        self.classes = load_classes(class_path)
        self.num_classes = len(self.classes)
        self.thickness = thickness
        self.thres = thres
        self.nms_thres = nms_thres
        self.half = half
        self.win_size = win_size
        self.overlap = overlap

    def detect(self, img):
        """img: RGB uint8 [H,W,3] -> Tensor[n,6] (x1,y1,x2,y2,conf,cls) in frame pixels, or None."""
        h, w, _ = img.shape
        prev_time = time.time()
        if self.win_size is not None:
            win_width, win_height = self.win_size
            if not (w < win_width and h < win_height):
                # img_detect.py:97-151: windows on a win_size grid, each extended by the overlap and clipped to the frame
                overlap_x, overlap_y = int(win_width * self.overlap), int(win_height * self.overlap)
                tiles = [(x, y, min(y + win_height + overlap_y, h) - y, min(x + win_width + overlap_x, w) - x)
                         for x in range(0, w, win_width) for y in range(0, h, win_height)]
                det = self.model.detect_tiled(img, tiles, self.thres, self.nms_thres)
                logging.info("\t Inference time: %.6f s" % (time.time() - prev_time))
                return _as_tensor(det) if det.shape[0] else None
        self.model.forward_u8(img, want_output=False)
        det = self.model.nms(0, self.thres, self.nms_thres, frame_hw=(h, w))
        logging.info("\t Inference time: %.6f s" % (time.time() - prev_time))
        if det.shape[0] == 0:
            return None
        return _as_tensor(det)


class FileVideoStream:
    """Threaded frame reader with a bounded queue and a per-frame transform - the role of ``imutils.video.FileVideoStream``
    in the reference (yolo3/detect/video_detect.py:12,86,112-126: ``FileVideoStream(path, _transform).start()``, ``more()``,
    ``read()``).  Sources: a video file / camera index through cv2.VideoCapture when cv2 is installed, or an ``.npy`` file
    holding uint8 [N,H,W,3] frames (what the tests and synthetic streams use), or any object with cv2.VideoCapture's
    ``isOpened / read / get / set / release`` (an already-open capture, an in-memory clip).  Frames are BGR like cv2's;
    ``transform`` is applied on the reader thread (the reference passes BGR->RGB)."""

    # cv2.CAP_PROP_* ordinals (stable across OpenCV 3.x / 4.x), so that capture-like sources work without cv2
    CAP_PROP_POS_FRAMES, CAP_PROP_FPS, CAP_PROP_FRAME_COUNT = 1, 5, 7

    def __init__(self, path, transform=None, queue_size=128):
        import queue
        self.transform = transform
        self.stopped = False
        self.Q = queue.Queue(maxsize=queue_size)
        self._frames = None
        self._cap = None
        if isinstance(path, str) and path.endswith(".npy"):
            self._frames = iter(np.load(path, mmap_mode="r"))
        elif all(hasattr(path, a) for a in ("isOpened", "read", "get", "set")):
            self._cap = path
            if not self._cap.isOpened():
                raise IOError("Couldn't open webcam or video")
        else:
            try:
                import cv2
            except ImportError:
                raise IOError("Couldn't open webcam or video")
            self._cap = cv2.VideoCapture(path)
            if not self._cap.isOpened():
                raise IOError("Couldn't open webcam or video")
        self._thread = None

    def start(self):
        import threading
        self._thread = threading.Thread(target=self._update, daemon=True)
        self._thread.start()
        return self

    def _next(self):
        if self._frames is not None:
            f = next(self._frames, None)
            return None if f is None else np.array(f)
        ok, f = self._cap.read()
        return f if ok else None

    def _update(self):
        import queue
        try:
            while not self.stopped:
                frame = self._next()
                if frame is None:
                    break
                if self.transform is not None:
                    frame = self.transform(frame)
                while not self.stopped:            # a full queue must not pin the thread once the consumer has gone
                    try:
                        self.Q.put(frame, timeout=0.05)
                        break
                    except queue.Full:
                        pass
        finally:
            self.stopped = True
            if self._cap is not None and hasattr(self._cap, "release"):   # released on the thread that reads it (never concurrently with read())
                self._cap.release()
            try:
                self.Q.put_nowait(None)            # end marker wakes a blocked reader
            except queue.Full:
                pass

    def more(self):
        return not (self.stopped and self.Q.empty())

    def read(self):
        import queue
        while True:
            try:
                return self.Q.get(timeout=0.05)
            except queue.Empty:
                if self.stopped and self.Q.empty():
                    return None

    def fps(self):
        """video_detect.py:92: int(CAP_PROP_FPS) of a capture - the reference truncates the rate before it uses it for the seek
        and for the writer (29.97 -> 29).  None for .npy sources (no rate stored with them)."""
        if self._cap is None:
            return None
        v = self._cap.get(self.CAP_PROP_FPS)
        return int(v) if v and v > 0 else None

    def seek_secs(self, skip_secs):
        """video_detect.py:97-101: skip_frames = int(skip_secs) * int(fps); the seek is refused (with the reference's message)
        when skip_secs exceeds the frame count; before start().  .npy sources count 25 frames per second."""
        if self._thread is not None:
            raise RuntimeError("seek_secs must be called before start()")
        if self._cap is not None:
            total = int(self._cap.get(self.CAP_PROP_FRAME_COUNT))
            if skip_secs > total:
                print("Can't skip over total video!")
            else:
                self._cap.set(self.CAP_PROP_POS_FRAMES, int(skip_secs) * (self.fps() or 0))
        else:
            for _ in range(int(skip_secs) * 25):
                if next(self._frames, None) is None:
                    break

    def stop(self):
        """Ends the reader thread (drains the queue so a blocked put() returns, joins) - safe when the consumer stops early."""
        import queue
        self.stopped = True
        t = self._thread
        if t is not None and t.is_alive():
            while t.is_alive():
                try:
                    while True:
                        self.Q.get_nowait()
                except queue.Empty:
                    pass
                t.join(timeout=0.05)
        elif t is None and self._cap is not None and hasattr(self._cap, "release"):
            self._cap.release()
        try:
            while True:
                self.Q.get_nowait()
        except queue.Empty:
            pass


def _transform(frame):
    """video_detect.py:33-36: BGR -> RGB"""
    return None if frame is None else np.ascontiguousarray(frame[:, :, ::-1])


def _is_frame_iterable(source):
    """An iterable of already-decoded RGB frames - not a path, not a capture."""
    return hasattr(source, "__iter__") and not isinstance(source, (str, bytes)) and not hasattr(source, "isOpened")


STAGE_FRONTS = dict(actions=as_device_actions, zones=as_device_zones, heatmap=as_device_heatmap, ground=as_device_ground,
                    snapshots=as_device_snapshots)


def fresh_stage(name, x, n_sources, *max_age):
    """``x`` as the table stage ``name`` of a detect_streams run over n_sources sources: converted as Pipeline.set_<name> converts
    it (a host comparator that names its streams keeps them), then ``fresh`` - the first n_sources specs and the settings in a new
    object, so that every stream starts with empty tables whatever the caller handed over."""
    if not isinstance(x, TrackStage):
        x = STAGE_FRONTS[name](x, getattr(x, "n_streams", max(n_sources, 1)), *max_age)
    return x.fresh(n_sources)


class VideoDetector:
    def __init__(self, model, class_path, thickness=2, font_path=None, font_size=10, thres=0.7, nms_thres=0.4,
                 skip_frames=-1, fourcc="mp4v", class_mask=None, win_size=None, overlap=0.15, tracker=None,
                 action_id=None, half=False, batch_frames=None, device_overlay=True, batch_windows=False, anonymize=None):
        # batch_frames (not in the reference): with a tracker, read that many frames ahead and run them through the batched device
        # pipeline (csrc/pipeline.cpp) - same results per frame, yielded in order, several times the frame rate of the frame-by-frame
        # path.  None (default, round 5) = by source: AUTO_BATCH frames for a file / an .npy / an iterable of frames - the reference
        # itself decodes up to 128 frames ahead of the detector for those (FileVideoStream queue, video_detect.py:86) - and 1 for a
        # live source (a camera index, a stream URL), where reading ahead would be waiting.  1 = the reference's latency (one frame
        # in, one result out).  device_overlay: the output stage (overlay, RGB -> BGR, FPS text) of the batched path on the device.
        # batch_windows (not in the reference): with win_size set, run the batched pipeline in window mode (pipeline.Pipeline(win_size=...):
        # windows cut, merged and tracked on the device) wherever a detector without win_size would take the batched path.  False
        # (default): a detector with win_size keeps the frame-by-frame loop, as before.
        # anonymize (not in the reference): a privacy.Anonymize - people are pixelated or filled over in every yielded image BEFORE
        # anything is drawn on it; the yielded rows and actions do not change.  None (default): off.
        self.batch_windows = bool(batch_windows)
        self.anonymize = anonymize
        self.batch_frames = None if batch_frames is None else max(1, int(batch_frames))
        self.device_overlay = bool(device_overlay) and not os.environ.get("YDS_HOST_OVERLAY")
        self._pipe = None
        self.thickness = thickness
        self.skip_frames = skip_frames
        self.class_names = load_classes(class_path)
        self.fourcc = fourcc
        self.class_mask = class_mask
        self.tracker = tracker
        self.action_id = action_id
        self._fps_prev, self._fps_acc, self._fps_cnt, self._fps_text = time.time(), 0.0, 0, "FPS: ??"
        self.label_drawer = LabelDrawer(self.class_names, font_path=font_path, font_size=font_size, thickness=thickness,
                                        img_size=getattr(model, "img_size", None))
        self.image_detector = ImageDetector(model, class_path, thickness=thickness, thres=thres, nms_thres=nms_thres,
                                            win_size=win_size, overlap=overlap, half=half)

    AUTO_BATCH = 68          # frames per step of the batched path when batch_frames is left to the source: bench.py's step size for the 608 x 608 nets
    #                          (workload.DEFAULT_BATCH says why 68; the reference itself reads 128 frames ahead); a shorter clip is read whole

    @staticmethod
    def _is_live(video_path):
        """A source that cannot be read ahead of real time: a camera index (cv2.VideoCapture(0), video_detect.py:86 passes the path
        through) or a network stream URL."""
        if isinstance(video_path, int):
            return True
        if hasattr(video_path, "isOpened"):                          # an already-open capture: live unless it knows its frame count
            try:
                return float(video_path.get(7)) <= 0                 # cv2.CAP_PROP_FRAME_COUNT (0 / -1 for cameras and streams)
            except Exception:
                return True
        return isinstance(video_path, str) and (video_path.isdigit() or "://" in video_path)

    def _batchable(self):
        """The batched device pipeline drives the package's own DeepSort (its Extractor and device tracker handles); a tracker that
        only offers update() - a DeepSort built around a user callable, any custom tracker - keeps the frame-by-frame loop."""
        from .deep_sort import DeepSort, Extractor
        t = self.tracker
        return (isinstance(t, DeepSort) and isinstance(getattr(t, "extractor", None), Extractor)
                and hasattr(t.extractor, "_h") and hasattr(getattr(t, "tracker", None), "_h")
                and self.image_detector.win_size is None and getattr(t, "nms_max_overlap", 1) == 1)

    def _batchable_windows(self):
        """_batchable() with the sliding-window condition lifted: every other condition holds and win_size is set (the batched
        pipeline then runs in window mode: detect() with batch_windows=True, detect_streams)."""
        det = self.image_detector
        if det.win_size is None:
            return False
        keep, det.win_size = det.win_size, None
        try:
            return self._batchable()
        finally:
            det.win_size = keep

    def _frames(self, video_path, skip_secs=0, transform=True):
        """RGB frames of the source (transform=False: a capture / file source's frames as decoded, BGR)."""
        self._source_fps = None
        if _is_frame_iterable(video_path):
            if skip_secs:
                raise ValueError("skip_secs needs a seekable source (a video file or an .npy path), not an iterable of frames")
            for f in video_path:           # already-decoded RGB frames
                yield f
            return
        fvs = FileVideoStream(video_path, _transform if transform else None)   # video_detect.py:86: decode thread + BGR -> RGB
        self._source_fps = fvs.fps()
        fvs.seek_secs(skip_secs)                                     # video_detect.py:99-101
        fvs.start()
        try:
            while fvs.more():
                frame = fvs.read()
                if frame is None:
                    return
                yield frame
        finally:
            fvs.stop()

    def process(self, frame):
        """The hot glue of video_detect.py:134-157 for one frame: returns hold_detections (self._tracked: the tracker branch
        :137-154 ran, i.e. the detector returned rows and a tracker is set)."""
        detections = self.image_detector.detect(frame)
        self._tracked = detections is not None and self.tracker is not None
        self._last_dets = None                                 # x, y, w, h, class of what the tracker is handed (the anonymise option)
        if self._tracked:
            det = detections.numpy() if hasattr(detections, "numpy") else detections
            boxs = p1p2Toxywh(det[:, :4])
            class_ids = det[:, -1]
            confidences = det[:, 4]
            if self.class_mask is not None:
                mask = reduce(lambda a, b: a | b, [class_ids == m for m in self.class_mask])
                boxs, confidences, class_ids = boxs[mask], confidences[mask], class_ids[mask]
            if getattr(self, "anonymize", None) is not None:
                self._last_dets = np.concatenate([np.asarray(boxs, np.float32).reshape(-1, 4), np.asarray(class_ids, np.float32).reshape(-1, 1)], 1)
            if hasattr(self.tracker, "extractor"):
                self.tracker.frame_source = self.image_detector.model       # lets update() crop from the detector's device copy
            detections = self.tracker.update(boxs.astype(np.float32), confidences, frame, class_ids)
        return detections

    def _video_steps(self, video_path, skip_secs=0, transform=True):
        """The steps of the batched detect(): a single video is a stream group of one - stream_groups' steps of (0, frame,
        processed, frame time), up to batch_frames frames that pass the skip_frames gate in each."""
        bf = getattr(self, "_batch_now", None) or self.batch_frames or 1
        return stream_groups([self._frames(video_path, skip_secs, transform)], bf, self.skip_frames,
                             refusal="VideoDetector: frames of one video must share one uint8 [h, w, 3] shape")

    def _processed_batches(self, video_path, skip_secs=0, transform=True):
        """_video_steps as lists of (frame, processed): which frames form each batch, for callers that prepare per-batch tables."""
        for items in self._video_steps(video_path, skip_secs, transform):
            yield [(frame, proc) for _, frame, proc, _ in items]

    def _render_host(self, frame, hold_detections, fps_text, detections=None):
        """video_detect.py:161-186 on the host: overlay (on a copy: callers may hand in their own frame arrays), RGB -> BGR, FPS text.
        With the anonymise option the mask comes first (privacy.anonymize on the copy; detections: the post-NMS rows x, y, w, h,
        class of the frame the held rows came from), then outlines, plates and text, then the FPS text."""
        image = frame
        anon = getattr(self, "anonymize", None)
        if anon is not None:
            from . import privacy
            rects = privacy.mask_rects(anon, frame.shape[0], frame.shape[1], hold_detections, detections)
            if rects:
                image = privacy.anonymize(frame, rects, anon)
        if hold_detections is not None and len(hold_detections):
            if image is frame:
                image = frame.copy()
            if self.tracker is not None:
                self.label_drawer.draw_labels_by_trackers(image, hold_detections, only_rect=False)
            else:
                self.label_drawer.draw_labels(image, hold_detections, only_rect=False)
        result = np.ascontiguousarray(image[:, :, ::-1])           # RGB -> BGR
        if fps_text:
            put_text(result, fps_text, (3, 15), 2, (255, 0, 0))
        return result

    def _render(self, frame, hold_detections, show_fps, detections=None):
        now = time.time()
        text = self._fps_tick(now - self._fps_prev)
        self._fps_prev = now
        return self._render_host(frame, hold_detections, text if show_fps else None, detections)

    def _fps_tick(self, dt):
        """The FPS counter of video_detect.py:176-182 advanced by one yielded frame that took `dt` seconds; returns the text to show."""
        self._fps_acc += dt
        self._fps_cnt += 1
        if self._fps_acc > 1:
            self._fps_acc -= 1
            self._fps_text = "FPS: " + str(self._fps_cnt)
            self._fps_cnt = 0
        return self._fps_text

    @staticmethod
    def _upload_step(blk, plan, frames):
        """The device part of the reader thread (stage_steps): the frames of one step (step order) -> the block's pinned staging
        array at the plan's offsets -> its HBM buffer in one copy (synchronous on the calling thread, the GIL released), in the
        source's own channel order: a BGR source stays BGR in HBM, the pipeline reads it in that order (set_frame_order) and the
        output stage draws on it.  blk["dev"] / blk["pin"] are (re)allocated only when the step outgrows them."""
        from . import _lib
        nbytes = plan["nbytes"]
        if blk["dev"] is None or blk["dev"].nbytes < nbytes:
            blk["dev"] = _lib.DeviceBuffer(nbytes)
            blk["pin"] = _lib.PinnedArray((nbytes,), np.uint8)
        stage = blk["pin"].array
        for slot, i in enumerate(plan["order"]):
            f, o = frames[i], int(plan["off"][slot])
            np.copyto(stage[o:o + f.size].reshape(f.shape), f)
        _lib.check(_lib.load().yds_memcpy_h2d(blk["dev"].ptr, _lib.ptr(stage[:nbytes]), nbytes))

    def _render_step(self, cur, holds, dets, fps_texts, bgr):
        """Output stage of one staged step (cur: stage_steps' record): a list of BGR frames in yield order, with the anonymise mask
        first (dets: per frame the detections its held rows came with).  Device form: csrc/overlay.hip over the frames in HBM,
        uniform or mixed as the step was planned; host form (device_overlay=False / YDS_HOST_OVERLAY in detect(): A/B runs and
        tests): label_draw.py on the staged copy."""
        plan, blk, n = cur["plan"], cur["blk"], len(holds)
        anon = getattr(self, "anonymize", None)
        dets = dets if anon is not None else None
        if self.device_overlay:
            if getattr(self, "_overlay", None) is None:
                from .label_draw import DeviceOverlay
                self._overlay = DeviceOverlay(self.label_drawer)
            if plan["mixed"]:
                return self._overlay.render_mixed(blk["dev"].offset(0), plan["nbytes"], plan["off"], plan["hw"], plan["slot_of"], holds,
                                                  fps_texts, bgr=bgr, privacy=anon, detections=dets)
            return self._overlay.render(blk["dev"].offset(0), plan["slot_of"], int(plan["hw"][0][0]), int(plan["hw"][0][1]), holds, fps_texts,
                                        bgr_frames=n if bgr else 0, privacy=anon, detections=dets, n_frames=n)
        stage, out = blk["pin"].array, []
        for i, slot in enumerate(plan["slot_of"]):
            o, h, w = int(plan["off"][slot]), int(plan["hw"][slot][0]), int(plan["hw"][slot][1])
            frame = stage[o:o + 3 * h * w].reshape(h, w, 3)
            out.append(self._render_host(np.ascontiguousarray(frame[..., ::-1] if bgr else frame), holds[i], fps_texts[i] if fps_texts else None,
                                         dets[i] if dets else None))
        return out

    def _detect_batched(self, video_path, show_fps=True, skip_secs=0, batch_frames=None):
        """detect() through the batched pipeline: identical per-frame results, frames are read batch_frames ahead (the reference itself
        decodes up to 128 frames ahead, video_detect.py:86).  Round 5: frames go reader thread -> pinned staging -> HBM once; the
        pipeline and the OUTPUT STAGE (overlay, RGB -> BGR, FPS text: csrc/overlay.hip) both read them there, the rendered batch comes
        back in one D2H copy.  A capture / file source is uploaded as the BGR the decoder delivers and channel-swapped on the device
        (the reference converts on the host, video_detect.py:33-36)."""
        import queue
        import threading
        det = self.image_detector
        bf = batch_frames or self.batch_frames or 1
        if self._pipe is None:
            from . import pipeline as pl
            if det.model.batch_max < bf:
                det.model.set_batch_max(bf)
            self._pipe = pl.Pipeline(det.model, self.tracker, det.thres, det.nms_thres, class_mask=self.class_mask,
                                     win_size=det.win_size, overlap=det.overlap)
        self._batch_now = bf
        iterable = _is_frame_iterable(video_path)
        if hasattr(self._pipe, "set_frame_order"):
            self._pipe.set_frame_order(not iterable)              # a capture / file source is staged as the decoder's BGR
        # Three threads, two hand-overs: reader (stage + upload) -> engine (pipeline steps, hold / action bookkeeping in frame order)
        # -> this generator's thread (output stage + yield).  The engine calls step(i + 1) while batch i is rendered and consumed:
        # with the output stage on the engine's thread the device idled for its 6 ms per batch (1193 against 1605 frames/s).
        out_q, done_q, free_q, stop = queue.Queue(maxsize=1), queue.Queue(maxsize=1), queue.Queue(), threading.Event()
        for _ in range(6):           # one being filled, one in out_q, two with the engine (this batch, the next), one in done_q, one being rendered
            free_q.put(dict(dev=None, pin=None))
        self.host_us = dict(wait_frames=0.0, step=0.0, wait_consumer=0.0, overlay=0.0, wait_engine=0.0, frames=0)
        reader = threading.Thread(target=stage_steps, daemon=True, args=(self._video_steps(video_path, skip_secs, transform=iterable), False,
                                                                          self._upload_step, out_q, free_q, stop))
        engine = threading.Thread(target=self._run_engine, args=(out_q, done_q, stop), daemon=True)
        reader.start()
        engine.start()
        t_prev = time.time()
        try:
            while True:
                t0 = time.perf_counter()
                item = done_q.get()
                if isinstance(item, BaseException):
                    raise item
                if item is None:
                    break
                cur, holds, dets, acts = item
                t1 = time.perf_counter()
                now = time.time()
                dt = (now - t_prev) / len(holds)
                t_prev = now
                fps = [self._fps_tick(dt) for _ in holds]
                results = self._render_step(cur, holds, dets, fps if show_fps else None, not iterable)
                free_q.put(cur["blk"])
                u = self.host_us
                u["wait_engine"] += (t1 - t0) * 1e6; u["overlay"] += (time.perf_counter() - t1) * 1e6; u["frames"] += len(holds)
                for i in range(len(holds)):
                    yield results[i], holds[i], acts[i]
        finally:
            shut_down(stop, free_q, (out_q, done_q), (engine, reader))

    def _run_engine(self, out_q, done_q, stop):
        """Engine thread of the batched path: one pipeline step per staged step (the next one handed over for its early detector
        pass), then the per-frame bookkeeping of video_detect.py:134-159 in frame order - held rows, the action module."""
        try:
            book = Bookkeeper()
            host_actions = self.action_id.update if self.action_id is not None else None
            masking = getattr(self, "anonymize", None) is not None     # the frame's detections travel with its held rows
            u = self.host_us

            def staged():
                item = take(out_q, stop)
                if isinstance(item, BaseException):
                    raise item
                return item
            t0 = time.perf_counter()
            cur = staged()
            u["wait_frames"] += (time.perf_counter() - t0) * 1e6
            while cur is not None and not stop.is_set():
                t0 = time.perf_counter()
                nxt = staged()
                t1 = time.perf_counter()
                outs, plan = [], cur["plan"]
                n = plan["n_proc"]
                if n:
                    # (one stream, uniform frames: same_composition is the same h, w and number of processed frames)
                    ahead = nxt["blk"]["dev"].offset(0) if nxt is not None and same_composition(plan, nxt["plan"]) else None
                    outs = self._pipe.step(cur["blk"]["dev"].offset(0), int(plan["hw"][0][0]), int(plan["hw"][0][1]), n, ahead)
                step_dets = self._pipe.last_detections() if masking and n else None
                u["wait_frames"] += (t1 - t0) * 1e6
                u["step"] += (time.perf_counter() - t1) * 1e6
                result = (cur,) + book.update(cur["items"], outs, step_dets=step_dets, host_actions=host_actions)
                t2 = time.perf_counter()
                give(done_q, result, stop)
                u["wait_consumer"] += (time.perf_counter() - t2) * 1e6
                cur = nxt
            give(done_q, None, stop)
        except BaseException as e:                             # noqa: BLE001 - re-raised on the consumer's thread
            give(done_q, e, stop)

    def detect(self, video_path, output_path=None, skip_secs=0, real_show=False, show_fps=True):
        """Generator of (bgr_image, hold_detections, actions) like video_detect.py:78-199.  output_path: every result is
        also written - through cv2.VideoWriter when cv2 is installed, as one uint8 [N,H,W,3] array for a path ending in
        ``.npy``; real_show needs cv2 (ignored without it); skip_secs seeks a capture to int(skip_secs) * int(fps) frames like
        video_detect.py:92-101 (an .npy source skips int(skip_secs) * 25 frames; an iterable of frames cannot seek and raises)."""
        writer, frames_out, cv2 = None, None, None
        try:
            import cv2 as _cv2
            cv2 = _cv2
        except ImportError:
            pass
        if output_path is not None:
            if str(output_path).endswith(".npy"):
                frames_out = []
            elif cv2 is None:
                raise IOError("writing %s needs cv2 (or use an .npy path)" % output_path)
        try:
            for result, det, actions in self._detect_impl(video_path, show_fps, skip_secs):
                if frames_out is not None:
                    frames_out.append(result.copy())
                elif output_path is not None:
                    if writer is None:
                        fourcc = cv2.VideoWriter_fourcc(*self.fourcc) if isinstance(self.fourcc, str) else self.fourcc
                        # video_detect.py:92,106: the writer takes int(SOURCE frame rate); 25 only where the source has none (.npy, iterables)
                        writer = cv2.VideoWriter(output_path, fourcc, self._source_fps or 25, (result.shape[1], result.shape[0]))
                    writer.write(result)
                if real_show and cv2 is not None:
                    cv2.imshow("result", result)
                yield result, det, actions
                if real_show and cv2 is not None and cv2.waitKey(1) & 0xFF == ord("q"):
                    break
        finally:
            if writer is not None:
                writer.release()
            if frames_out is not None:
                np.save(output_path, np.stack(frames_out, 0) if frames_out else np.zeros((0, 0, 0, 3), np.uint8))
            if real_show and cv2 is not None:
                cv2.destroyAllWindows()

    def detect_streams(self, sources, frames_per_stream=None, show_fps=True, mixed_sizes=False, stream_win_sizes=None, global_ids=False,
                       identity_memory=None, zones=None, zone_max_age=30, heatmap=None, heatmap_max_age=30, ground=None, ground_max_age=30,
                       snapshots=None, snapshot_max_age=30):
        """Many sources (cameras, files, iterables of RGB frames) on one GPU: a generator that yields, per step, a list of
        (stream_index, bgr_image, hold_detections, actions) for every frame read in that step, streams in the order given, each
        stream's frames in time order.  Each stream gets its own self.tracker.clone() (one tracker per stream, the Extractor shared:
        deep_sort.py:41-44), and its items are what detect(source) yields for that source alone with a fresh clone - skip_frames,
        class_mask, the overlay and the image included; the FPS text (show_fps) counts the frames of all streams.  One step takes up
        to frames_per_stream processed frames from every stream that is still running and runs them through ONE MultiStreamPipeline
        step: one detector pass, one ReID pass, all trackers advanced in the same launches.  A stream that ends drops out, the
        others go on.  frames_per_stream=None: 1 when any source is live (_is_live), else max(1, AUTO_BATCH // len(sources)).
        Limits: every frame of every source must have one uint8 [h, w, 3] shape (ValueError otherwise); the tracker must be this
        package's DeepSort around its Extractor, with nms_max_overlap=1.  A detector with win_size runs the pipeline in window mode
        (MultiStreamPipeline(win_size=...)).
        action_id (an action.ActionIdentify of the five built-in actions, or an action.DeviceActionIdentify) runs ON THE DEVICE
        inside the step (MultiStreamPipeline.set_actions): every stream gets a fresh orbit cache - the device form of
        action_id.clone() per stream - and the fourth item carries that stream's actions with the semantics of
        video_detect.py:134-159: [] on a skipped frame, the previous value on a frame whose detector returned None, else the
        frame's list.  Frame times are explicit, not the wall clock at the update: time.time() at read for a live source
        (_is_live), else the stream's frame index (skipped frames counted) over the source's frame rate (25 where it has none).
        An action_id the device cannot run (a custom Action subclass, a non-integral class id, max_size > 16) raises ValueError
        naming action_id.  detect() keeps calling the host module with the wall clock, as the reference does.
        mixed_sizes=True lifts the first limit: every stream has its own uint8 [h, w, 3] shape (1080p and 720p cameras in one step,
        MultiStreamPipeline.step_mixed) and keeps it - a stream that changes its shape midway raises ValueError naming the stream;
        window mode takes frames of one size, so win_size with mixed_sizes=True raises ValueError.
        stream_win_sizes: one (w, h) or None per source - that camera's ImageDetector(win_size, overlap), with this detector's overlap
        (MultiStreamPipeline(stream_win_sizes=...)): a wide camera is cut into windows, a door camera is not, in one step, with
        mixed_sizes False or True.  It needs a detector whose own win_size is None (ValueError otherwise); per stream the items are
        those of detect() with a detector of that win_size.
        global_ids=True keeps one identity per person ACROSS the streams (MultiStreamPipeline.set_identities with the tracker's
        own matching threshold): read it with stream_identities() between the yields.  The yielded items are the same either way:
        track ids stay per stream.  Limits (identity.py): the tracker needs the cosine metric and a finite nn_budget (ValueError
        otherwise); only live tracks hold an identity, unless identity_memory=dict(ids=..., rows=8, ttl=None) gives the map a memory
        of departed identities (identity.IdentityMap's memory_ids / memory_rows / memory_ttl; ValueError without global_ids=True):
        stream_identity_map() between the yields returns the map itself, for enrol(), memory() and last_relinked().
        zones: zones and counting lines ON THE DEVICE inside the step (MultiStreamPipeline.set_zones) - one (zones, lines) pair of
        zones.Zone / zones.Line lists for all streams, a list with one pair per stream, a zones.ZoneMonitor (its geometry and
        max_age) or a zones.DeviceZoneMonitor (its geometry and max_age; never its tables): every stream starts with an empty
        table, entries leave after zone_max_age unseen processed frames, geometry is in the stream's own frame pixels, frame times
        are those of the action stage.  Read stream_zone_events() and stream_zone_counts() between the yields; the yielded items
        do not change.  ValueError naming zones for geometry the device refuses.
        heatmap: heat maps ON THE DEVICE inside the step (MultiStreamPipeline.set_heatmap) - one heatmap.HeatSpec for all streams, a
        list with one per stream, a heatmap.HeatMap (its spec and max_age) or a heatmap.DeviceHeatMap (its specs and max_age; never
        its layers): every stream starts with zero layers and an empty table, entries leave after heatmap_max_age unseen processed
        frames, frame times are those of the action stage.  Read stream_heatmaps() between the yields; the yielded items and images
        do not change: blending a layer into a frame is the caller's (heatmap.render on the host; DeviceHeatMap.render is for
        frames kept in HBM).  ValueError naming heatmap for a spec the device refuses.
        ground: the ground plane ON THE DEVICE inside the step (MultiStreamPipeline.set_ground) - one ground.GroundSpec for all
        streams, a list with one (or None: that camera is skipped) per stream, a ground.GroundMap or a ground.DeviceGroundMap (their
        specs, max_age and speed_window; never their grid): one fresh site grid on one floor plan for all cameras, entries leave
        after ground_max_age unseen processed frames, frame times are those of the action stage.  Read stream_ground() (the step's
        records: plan position, velocity, speed, cell per person) and site_map(layer) between the yields; the yielded items and
        images do not change.  ValueError naming ground for a spec the device refuses.
        snapshots: each track's best crop ON THE DEVICE inside the step (MultiStreamPipeline.set_snapshots) - one snapshot.SnapSpec
        for all streams, a list with one (or None: that camera is skipped) per stream, a snapshot.SnapshotBook or a
        snapshot.DeviceSnapshotBook (their specs and max_age; never their tables): every stream starts with an empty table and an
        empty archive ring, entries close after snapshot_max_age unseen processed frames, frame times are those of the action
        stage.  Read stream_snapshots() (the records with their 128 x 64 RGB thumbnails) and stream_snapshot_events() between the
        yields; the yielded items and images do not change.  The thumbnails are taken from the frames as they were read, before the
        output stage: anonymize= does not mask them.  ValueError naming snapshots for a spec the device refuses.
        device_overlay (the constructor's flag, on by default; YDS_HOST_OVERLAY turns it off) runs the generator as a staged engine
        (_detect_streams_device): a reader thread forms the steps and uploads them from pinned staging blocks, the step runs on the
        caller's thread in lock-step with the yields and takes the next staged step along for its early detector pass, and the
        output stage - the anonymise mask, the overlay, RGB -> BGR, the FPS text - is one call on the device over the staged block
        (DeviceOverlay.render, render_mixed for mixed_sizes).  The yielded items and everything read between the yields are the
        same either way; the images are views of a pinned block and the FPS text advances by the step's time over its frames.
        With global_ids no step carries a look-ahead pass: stream_identity_map() hands out the map, and changing it between the
        yields (enrol, set_memory) is refused by the library while such a pass is in flight.  device_overlay=False keeps the host
        loop below."""
        from . import pipeline as pl
        from .identity import check_memory
        sources = list(sources)
        memory = {}
        if identity_memory is not None:
            if not global_ids:
                raise ValueError("VideoDetector.detect_streams: identity_memory needs global_ids=True")
            unknown = set(identity_memory) - {"ids", "rows", "ttl"}
            if unknown or "ids" not in identity_memory:
                raise ValueError("VideoDetector.detect_streams: identity_memory is dict(ids=..., rows=..., ttl=...), got %r" % (identity_memory,))
            memory = dict(memory_ids=identity_memory["ids"], memory_rows=identity_memory.get("rows", 8), memory_ttl=identity_memory.get("ttl"))
            check_memory(**memory)
        stream_win_sizes = pl.check_stream_win_sizes(len(sources), self.image_detector.win_size, stream_win_sizes, "VideoDetector.detect_streams")
        if self.tracker is None:
            raise ValueError("VideoDetector.detect_streams needs a tracker (each stream runs a clone of it)")
        # the table stages (track_stage.py): fresh tables for this run, one per stream, never the caller's own; ValueError naming the
        # stage for what the device refuses
        stages = {name: fresh_stage(name, x, len(sources), *age)
                  for name, x, *age in (("actions", self.action_id), ("zones", zones, zone_max_age), ("heatmap", heatmap, heatmap_max_age),
                                        ("ground", ground, ground_max_age), ("snapshots", snapshots, snapshot_max_age)) if x is not None}
        if not (self._batchable() or self._batchable_windows()):
            raise ValueError("VideoDetector.detect_streams needs this package's DeepSort with its Extractor and nms_max_overlap=1")
        if mixed_sizes and self.image_detector.win_size is not None:
            raise ValueError("VideoDetector.detect_streams: mixed_sizes=True cannot be combined with win_size (window mode cuts frames of one "
                             "size); give every stream its own setting with stream_win_sizes")
        S = len(sources)
        if S == 0:
            return
        F = int(frames_per_stream) if frames_per_stream else (1 if any(self._is_live(src) for src in sources) else max(1, self.AUTO_BATCH // S))
        det = self.image_detector
        if det.model.batch_max < S * F:
            det.model.set_batch_max(S * F)
        pipe = pl.MultiStreamPipeline(det.model, [self.tracker.clone() for _ in range(S)], det.thres, det.nms_thres, class_mask=self.class_mask,
                                      win_size=det.win_size, overlap=det.overlap, stream_win_sizes=stream_win_sizes)
        for name, dev in stages.items():
            getattr(pipe, "set_" + name)(dev)
        if global_ids:
            pipe.set_identities(True, **memory)
        self._stream_ground = [[] for _ in range(S)]
        self._stream_snap_events = [[] for _ in range(S)]
        self._stream_zone_events = [[] for _ in range(S)]
        self._streams_pipe = pipe                        # search_streams / link_stream_track reach the trackers between the yields
        on = dict({name: name in stages for name in STAGE_FRONTS}, timed=bool(stages))
        try:
            if self.device_overlay:                          # staged uploads, look-ahead, the output stage on the device
                yield from self._detect_streams_device(pipe, sources, F, show_fps, mixed_sizes, on, lookahead=not global_ids)
                return
            # the host loop (device_overlay=False / YDS_HOST_OVERLAY): every step's processed frames are planned and uploaded as a
            # step of their own, on this thread; the images are rendered on the host from the frames as they were read
            its = [iter(self._frames(src)) for src in sources]
            book, blk = Bookkeeper(S), dict(dev=None, pin=None)
            for items in stream_groups(its, F, self.skip_frames, mixed_sizes, [self._is_live(src) for src in sources],
                                       lambda: getattr(self, "_source_fps", None)):
                procs = [it for it in items if it[2]]
                plan = stage_plan(procs, mixed_sizes)
                if procs:
                    self._upload_step(blk, plan, [it[1] for it in procs])
                holds, dets, acts = book.update([(s, p) for s, _, p, _ in items], *self._streams_step(pipe, plan, [it[3] for it in procs], blk, None, on))
                yield [(s, self._render(frame, holds[i], show_fps, dets[i]), holds[i], acts[i]) for i, (s, frame, _, _) in enumerate(items)]
        finally:
            self._streams_pipe = None                    # the generator ended, was closed or raised

    def _streams_step(self, pipe, plan, times, blk, ahead, on):
        """One MultiStreamPipeline step over the processed frames of a planned step (uniform or mixed; times: their frame times;
        ahead: the next step's HBM buffer for its early detector pass, or None), and what the bookkeeping reads after it:
        (outs, actions per frame or None, detections per frame or None).  on: which device stages run (the stages' names, and
        timed: any of them)."""
        n, outs = plan["n_proc"], []
        if n:
            if on["timed"]:
                pipe.set_frame_times(times)
            if plan["mixed"]:
                outs = pipe.step_mixed(blk["dev"].offset(0), plan["off"][:n], plan["hw"][:n], plan["streams"], plan["proc_bytes"], ahead)
            else:
                outs = pipe.step(blk["dev"].offset(0), int(plan["hw"][0][0]), int(plan["hw"][0][1]), plan["streams"], ahead)
        step_acts = pipe.last_actions() if on["actions"] and n else None
        step_dets = pipe.last_detections() if getattr(self, "anonymize", None) is not None and n else None
        if on["zones"]:                                  # the events of this step's processed frames, per stream in time order
            self._stream_zone_events = [[] for _ in self._stream_zone_events]
            for s, evs in zip(plan["streams"], pipe.last_zone_events() if n else []):
                self._stream_zone_events[s].append(evs)
        if on["ground"]:                                 # the records of this step's processed frames, per stream in time order
            self._stream_ground = [[] for _ in self._stream_ground]
            for s, rows in zip(plan["streams"], pipe.last_ground() if n else []):
                self._stream_ground[s].append(rows)
        if on["snapshots"]:                              # the items of this step's processed frames, per stream in time order
            self._stream_snap_events = [[] for _ in self._stream_snap_events]
            for s, items in zip(plan["streams"], pipe.last_snapshot_events() if n else []):
                self._stream_snap_events[s].append(items)
        return outs, step_acts, step_dets

    def _detect_streams_device(self, pipe, sources, F, show_fps, mixed_sizes, on, lookahead=True):
        """detect_streams with the output stage on the device (device_overlay).  A reader thread forms, stages and uploads the
        steps (stage_steps: a ring of four blocks - one being filled, one queued, the two the step holds); THIS thread runs the
        step in lock-step with the yields, so that whatever is read between the yields (zone events and counts, identities, heat
        maps, search, link) is the state right after the yielded step.  Overlap comes from look-ahead: when the next step is
        already staged and has the same composition (same_composition), its HBM buffer goes along as next_frames_dev and the
        device runs its detector pass while the host renders and the consumer works; with a live source the next step is never
        waited for.  The output stage is ONE call over the staged block, processed and skipped frames alike (_render_step), with
        the mask first when the anonymise option is on.  Sources that are all captures or files are staged as the decoder's BGR
        (set_frame_order(True)) and drawn on in place; any iterable keeps RGB staging and the reversed copy.  lookahead=False
        (detect_streams with global_ids): no step carries a look-ahead pass - the identity map is the caller's to change
        between the yields (stream_identity_map().enrol, set_memory), which the library refuses while such a pass is in flight."""
        import queue
        import threading
        bgr = not any(_is_frame_iterable(src) for src in sources)
        pipe.set_frame_order(bgr)
        live = [self._is_live(src) for src in sources]
        its = [iter(self._frames(src, transform=not bgr)) for src in sources]
        groups = stream_groups(its, F, self.skip_frames, mixed_sizes, live, lambda: getattr(self, "_source_fps", None))
        out_q, free_q, stop = queue.Queue(maxsize=1), queue.Queue(), threading.Event()
        for _ in range(4):
            free_q.put(dict(dev=None, pin=None))
        reader = threading.Thread(target=stage_steps, args=(groups, mixed_sizes, self._upload_step, out_q, free_q, stop), daemon=True)
        self._streams_reader = reader
        reader.start()
        book = Bookkeeper(len(sources))
        wait_next = not any(live)                              # (a live source is never waited for)
        self.streams_lookahead = [0, 0]                        # steps that carried a look-ahead pass, steps run (tools/, tests)
        t_prev = time.time()
        try:
            cur, nxt = take(out_q, stop, reader), NOTHING
            while cur is not None:
                if isinstance(cur, BaseException):            # after everything staged before it was yielded, as on the host form
                    raise cur
                if nxt is NOTHING:
                    nxt = take(out_q, stop, reader, wait_next)
                plan, items, ahead = cur["plan"], cur["items"], None
                if plan["n_proc"]:
                    if lookahead and isinstance(nxt, dict) and same_composition(plan, nxt["plan"]):
                        ahead = nxt["blk"]["dev"].offset(0)
                    self.streams_lookahead[0] += ahead is not None
                    self.streams_lookahead[1] += 1
                holds, dets, acts = book.update(items, *self._streams_step(pipe, plan, [t for _, p, t in items if p], cur["blk"], ahead, on))
                now = time.time()
                dt = (now - t_prev) / len(items)
                t_prev = now
                fps = [self._fps_tick(dt) for _ in items]
                images = self._render_step(cur, holds, dets, fps if show_fps else None, bgr)
                free_q.put(cur["blk"])
                out = [(items[i][0], images[i], holds[i], acts[i]) for i in range(len(items))]
                del images
                yield out
                cur, nxt = (take(out_q, stop, reader), NOTHING) if nxt is NOTHING else (nxt, NOTHING)
        finally:
            shut_down(stop, free_q, (out_q,), (reader,))
            for it in its:                                   # ends the decoder threads of file / capture sources
                try:
                    it.close()
                except Exception:                            # noqa: BLE001 - a reader that did not stop in time still runs the iterator
                    pass

    def _live_streams_pipe(self, who):
        pipe = getattr(self, "_streams_pipe", None)
        if pipe is None:
            raise ValueError("VideoDetector.%s is valid between the yields of a running detect_streams generator only" % who)
        return pipe

    def search_streams(self, queries, top_k=5, max_dist=None, confirmed_only=True):
        """Watch-list query against the live tracks of every stream of the running detect_streams generator, between two of its
        yields (ValueError outside): per query a list of (stream_index, track_id, dist), MultiStreamPipeline.search."""
        return self._live_streams_pipe("search_streams").search(queries, top_k=top_k, max_dist=max_dist, confirmed_only=confirmed_only)

    def link_stream_track(self, stream, track_id, exclude_stream=None, top_k=5, max_dist=None, confirmed_only=True):
        """Hand-over between the streams of the running detect_streams generator, between two of its yields (ValueError outside):
        the tracks nearest to live track track_id of stream `stream`, MultiStreamPipeline.link."""
        return self._live_streams_pipe("link_stream_track").link(stream, track_id, exclude_stream=exclude_stream, top_k=top_k,
                                                                 max_dist=max_dist, confirmed_only=confirmed_only)

    def stream_identities(self, stream=None):
        """The global ids of the running detect_streams(global_ids=True) generator, between two of its yields (ValueError outside,
        and for a generator started without global_ids): dict track_id -> global_id of the live Confirmed tracks of ``stream``
        (0 = deferred to the next step), or a list of such dicts, one per stream; MultiStreamPipeline.last_identities."""
        pipe = self._live_streams_pipe("stream_identities")
        if getattr(pipe, "identities", None) is None:
            raise ValueError("VideoDetector.stream_identities needs detect_streams(..., global_ids=True)")
        return pipe.last_identities(stream)

    def _stage_pipe(self, who, name):
        """The pipe of the running generator for a reader of the stage ``name``: ValueError outside the generator, and for one
        started without the stage."""
        pipe = self._live_streams_pipe(who)
        if getattr(pipe, {"heatmap": "heat", "snapshots": "snap"}.get(name, name), None) is None:
            raise ValueError("VideoDetector.%s needs detect_streams(..., %s=...)" % (who, name))
        return pipe

    def _stage_report(self, who, name, kept, stream):
        """The last step's report of the stage as _streams_step kept it (attribute ``kept``: per stream an entry per processed
        frame): one stream's list or all."""
        self._stage_pipe(who, name)
        per = getattr(self, kept)
        if stream is None:
            return [list(e) for e in per]
        if int(stream) < 0 or int(stream) >= len(per):
            raise ValueError("VideoDetector.%s: stream %d outside [0, %d)" % (who, int(stream), len(per)))
        return list(per[int(stream)])

    def stream_zone_events(self, stream=None):
        """The zone events of the last step of the running detect_streams(zones=...) generator, between two of its yields
        (ValueError outside, and for a generator started without zones): for ``stream`` one entry per frame of it that the step
        processed, in time order - that frame's ``[(track_id, class_id, kind, zone or line name, t, dwell), ...]``, None where
        the detector returned None - or a list of such lists, one per stream; MultiStreamPipeline.last_zone_events."""
        return self._stage_report("stream_zone_events", "zones", "_stream_zone_events", stream)

    def stream_zone_counts(self, stream=None):
        """The zone and line counters of the running detect_streams(zones=...) generator, between two of its yields (ValueError
        outside, and for a generator started without zones): MultiStreamPipeline.zone_counts."""
        return self._stage_pipe("stream_zone_counts", "zones").zone_counts(stream)

    def stream_heatmaps(self, layer="presence", stream=None):
        """The heat maps of the running detect_streams(heatmap=...) generator, between two of its yields (ValueError outside, and
        for a generator started without heatmap): ``layer`` of ``stream`` as int64 [gh, gw], read from the device, or a list with
        one grid per stream; layer=None: all five layers [5, gh, gw]; MultiStreamPipeline.heatmap."""
        return self._stage_pipe("stream_heatmaps", "heatmap").heatmap(stream, layer)

    def stream_ground(self, stream=None):
        """The ground records of the last step of the running detect_streams(ground=...) generator, between two of its yields
        (ValueError outside, and for a generator started without ground): for ``stream`` one entry per frame of it that the step
        processed, in time order - int32 [m, 8] = track id, class, qx, qy, vx, vy, speed, cell, None where the detector returned
        None - or a list of such lists, one per stream; MultiStreamPipeline.last_ground."""
        return self._stage_report("stream_ground", "ground", "_stream_ground", stream)

    def site_map(self, layer="presence"):
        """The site grid of the running detect_streams(ground=...) generator, between two of its yields (ValueError outside, and
        for a generator started without ground): ``layer`` as int64 [gh, gw], read from the device; layer=None: all five layers
        [5, gh, gw]; MultiStreamPipeline.ground_layers."""
        return self._stage_pipe("site_map", "ground").ground_layers(layer)

    def stream_snapshots(self, stream=None, archive=False):
        """The snapshots of the running detect_streams(snapshots=...) generator, between two of its yields (ValueError outside, and
        for a generator started without snapshots): the records of ``stream`` - dicts of id, cls, score, n_seen, box, tag_best,
        t_first, t_best, t_last and thumb (uint8 [128, 64, 3] RGB) in table order, read from the device; archive=True: the archive
        ring, oldest first, with t_closed - or a list of such lists, one per stream; MultiStreamPipeline.snapshots."""
        return self._stage_pipe("stream_snapshots", "snapshots").snapshots(stream, archive)

    def stream_snapshot_events(self, stream=None):
        """The snapshot items of the last step of the running detect_streams(snapshots=...) generator, between two of its yields
        (ValueError outside, and for a generator started without snapshots): for ``stream`` one entry per frame of it that the
        step processed, in time order - int32 [m, 6] = frame of the step, track id, class, kind, score, aux, None where the
        detector returned None - or a list of such lists, one per stream; MultiStreamPipeline.last_snapshot_events."""
        return self._stage_report("stream_snapshot_events", "snapshots", "_stream_snap_events", stream)

    def stream_identity_map(self):
        """The IdentityMap of the running detect_streams(global_ids=True) generator, between two of its yields (ValueError outside,
        and for a generator started without global_ids): enrol(), memory(), last_relinked() and the other reads go through it."""
        pipe = self._live_streams_pipe("stream_identity_map")
        if getattr(pipe, "identities", None) is None:
            raise ValueError("VideoDetector.stream_identity_map needs detect_streams(..., global_ids=True)")
        return pipe.identities

    @staticmethod
    def _source_len(video_path):
        """Frames the source holds, when it can tell without being consumed (a sequence, an .npy file, an open capture); else None."""
        try:
            if hasattr(video_path, "isOpened"):
                n = int(video_path.get(7))                           # cv2.CAP_PROP_FRAME_COUNT
                return n if n > 0 else None
            if isinstance(video_path, str):
                return int(np.load(video_path, mmap_mode="r").shape[0]) if video_path.endswith(".npy") else None
            return len(video_path) if hasattr(video_path, "__len__") else None
        except Exception:                                             # noqa: BLE001 - a source that cannot tell simply gets the default
            return None

    def _detect_impl(self, video_path, show_fps=True, skip_secs=0):
        # (the tracker-side NMS option reorders detections on the host, so it keeps the frame-by-frame path)
        bf = self.batch_frames if self.batch_frames is not None else (1 if self._is_live(video_path) else self.AUTO_BATCH)
        if self.batch_frames is None and bf > 1:
            n = self._source_len(video_path)                          # a clip shorter than the default read-ahead: no buffers for frames
            if n is not None:                                         # that will never come (every capacity follows the batch size)
                bf = max(1, min(bf, n))
        if bf > 1 and (self._batchable() or (getattr(self, "batch_windows", False) and self._batchable_windows())):
            yield from self._detect_batched(video_path, show_fps, skip_secs, bf)
            return
        # the frame-by-frame loop: a step of one frame; the action module runs where the tracker branch did (process)
        book, since = Bookkeeper(rows_as_given=True), 0
        host_actions = None if self.tracker is None else (self.action_id.update if self.action_id is not None else (lambda hold: []))
        for frame in self._frames(video_path, skip_secs):
            if frame is None:
                break
            proc, since = skip_gate(since, self.skip_frames)
            outs = [self.process(frame)] if proc else []
            (hold,), (dets,), (actions,) = book.update([(0, proc)], outs, step_dets=[self._last_dets] if proc else None, host_actions=host_actions)
            yield self._render(frame, hold, show_fps, dets), hold, actions
