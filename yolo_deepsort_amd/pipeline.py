"""Whole-path driver used by bench.py and smoke(): frames resident in HBM -> detector over a batch ->
per frame NMS, class mask, ReID, tracker (csrc/pipeline.cpp; reference yolo3/detect/video_detect.py:134-157)."""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib


def _refuse_tracker_nms(deepsort, message):
    # the batched path hands the tracker handle to the C pipeline and never passes through DeepSort.update: the
    # tracker-side NMS (deep_sort.py:52-57, a host-ordered reordering of the detections) is not part of it
    if getattr(deepsort, "nms_max_overlap", 1) != 1:
        raise ValueError(message % (deepsort.nms_max_overlap,))


def _check_host_frames(frames, next_frames=None):
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.flags["C_CONTIGUOUS"]
    if next_frames is not None:
        assert next_frames.shape == frames.shape and next_frames.dtype == np.uint8 and next_frames.flags["C_CONTIGUOUS"]
    return frames.shape[:3]


def pack_frames(frames):
    """Frames of any sizes back to back in one block: (uint8 block, byte offsets uint64 [n], sizes int32 [n,2]) - the layout the
    mixed entries take (yds_pipeline_step_multi_mixed).  Each frame must be a uint8 [h, w, 3] array."""
    frames = [np.asarray(f) for f in frames]
    for i, f in enumerate(frames):
        if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
            raise ValueError("frame %d must be a uint8 [h, w, 3] array, got %s %s" % (i, f.dtype, f.shape))
    sizes = np.array([f.shape[0] * f.shape[1] * 3 for f in frames], np.uint64)
    off = np.zeros(len(frames), np.uint64)
    off[1:] = np.cumsum(sizes)[:-1]
    block = np.concatenate([f.reshape(-1) for f in frames]) if frames else np.zeros(0, np.uint8)
    hw = np.array([f.shape[:2] for f in frames], np.int32).reshape(-1, 2)
    return block, off, hw


def check_stream_win_sizes(n_streams, win_size, stream_win_sizes, who="MultiStreamPipeline"):
    """stream_win_sizes of n_streams streams as a list of (w, h) or None; raises ValueError for a list of another length, an entry
    that is no (w, h) pair, or win_size given as well (one window setting for all streams, or one per stream)."""
    if stream_win_sizes is None:
        return None
    if win_size is not None:
        raise ValueError("%s: win_size (one setting for all streams) and stream_win_sizes (one per stream) exclude each other" % who)
    sizes = list(stream_win_sizes)
    if len(sizes) != n_streams:
        raise ValueError("%s: stream_win_sizes needs one entry per stream (%d), got %d" % (who, n_streams, len(sizes)))
    out = []
    for s, ws in enumerate(sizes):
        if ws is not None and (len(ws) != 2 or int(ws[0]) < 1 or int(ws[1]) < 1):
            raise ValueError("%s: stream_win_sizes[%d] must be None or a positive (w, h), got %r" % (who, s, ws))
        out.append(None if ws is None else (int(ws[0]), int(ws[1])))
    return out


class Pipeline:
    def __init__(self, net, deepsort, conf_thres=0.5, nms_thres=0.4, class_mask=None, cap=512, win_size=None, overlap=0.15):
        self.net, self.ds, self.cap = net, deepsort, int(cap)
        self._h = None
        _refuse_tracker_nms(deepsort, "Pipeline: DeepSort(nms_max_overlap=%r) needs the frame-by-frame path (DeepSort.update / "
                                      "VideoDetector(batch_frames=1)); the batched pipeline has no tracker-side NMS")
        mask = np.ascontiguousarray(class_mask if class_mask is not None else [], dtype=np.int32)
        self._h = _lib.check_ptr(_lib.load().yds_pipeline_create(net._h, deepsort.extractor._h, deepsort.tracker._h,
                                                                 conf_thres, nms_thres,
                                                                 _lib.ptr(mask) if mask.size else None, int(mask.size)))
        self.set_windows(win_size, overlap)

    def set_windows(self, win_size=None, overlap=0.15):
        """Window mode, ImageDetector(win_size=(win_w, win_h), overlap) (img_detect.py:97-151) for every frame of a step: the frames
        are cut into windows on the device, all windows of the step run through the detector in chunks of net.batch_max, one NMS
        launch merges them per frame (yds_pipeline_set_windows).  None = off (the default).  Refused (YdsError) while a look-ahead
        pass is in flight, i.e. between a step that was given next frames and the step that consumes them."""
        ww, wh = (0, 0) if win_size is None else (int(win_size[0]), int(win_size[1]))
        _lib.check(_lib.load().yds_pipeline_set_windows(self._h, ww, wh, float(overlap)))
        self.win_size, self.overlap = (None if win_size is None else (ww, wh)), overlap

    def step(self, frames_dev, h, w, batch, next_frames_dev=None, select_next=None):
        """frames_dev: device pointer to uint8 [batch,h,w,3]; next_frames_dev (optional): the frames of the next
        call, whose detector pass is enqueued early.  Returns a list of int32 [m,6] (None when the detector found
        nothing and the tracker was not called)."""
        return self._run(batch, select_next, lambda out, counts: _lib.load().yds_pipeline_step(
            self._h, frames_dev, next_frames_dev, h, w, batch, out, self.cap, counts))

    def _run(self, n, select_next, call, streams=None):
        """One step of n frames: call(out, counts) is the library entry that fills int32 out [n,cap,6] and counts [n]; streams: the
        stream of every frame (a multi-stream step), kept for the per-stream readers of the stages' reports."""
        self._step_streams = None if streams is None else [int(v) for v in streams]
        out = np.zeros((n, self.cap, 6), np.int32)
        counts = np.zeros(n, np.int32)
        if select_next is not None:
            _lib.check(_lib.load().yds_pipeline_set_next_injection(self._h, int(select_next)))
        _lib.check(call(_lib.ptr(out), _lib.ptr(counts)))
        self._last_counts = counts
        return [None if counts[b] < 0 else out[b, :counts[b]].copy() for b in range(n)]

    def step_host(self, frames, next_frames=None, select_next=None):
        """frames / next_frames: uint8 [batch,h,w,3] HOST arrays (C-contiguous; views of a _lib.PinnedArray upload
        asynchronously).  The upload of next_frames overlaps this call's work; the next call must pass the same array
        object's memory as `frames`."""
        batch, h, w = _check_host_frames(frames, next_frames)
        return self._run(batch, select_next, lambda out, counts: _lib.load().yds_pipeline_step_host(
            self._h, _lib.ptr(frames), _lib.ptr(next_frames), h, w, batch, out, self.cap, counts))

    def _set_stage(self, name, as_device, x, *max_age):
        """One table stage of every following step (yds_pipeline_set_<name>): x as the stage's device object (track_stage.py
        as_device), None = off.  The object is kept as self.actions / .zones / .heat / .ground / .snap: the handle lives while the
        pipeline names it."""
        dev = None if x is None else as_device(x, getattr(self, "n_streams", 1), *max_age)
        _lib.check(getattr(_lib.load(), "yds_pipeline_set_" + name)(self._h, None if dev is None else dev.handle))
        setattr(self, {"heatmap": "heat", "snapshots": "snap"}.get(name, name), dev)
        return dev

    def _last_report(self, dev, entry, columns):
        """The two-call read of a stage's report of the last step (yds_pipeline_last_<entry>: ask the count, then copy).  columns:
        (dtype, width) each; returns (counts of the step, the columns cut to the items reported), or None when the stage is off
        or no step ran."""
        counts = getattr(self, "_last_counts", None)
        if dev is None or counts is None:
            return None
        n, call = C.c_int(0), getattr(_lib.load(), "yds_pipeline_last_" + entry)
        call(self._h, *[None] * len(columns), 0, C.byref(n))      # (asks for the count; refuses to copy when it is not 0)
        cols = [np.zeros((max(n.value, 1), w) if w > 1 else max(n.value, 1), t) for t, w in columns]
        _lib.check(call(self._h, *[_lib.ptr(c) for c in cols], len(cols[0]), C.byref(n)))
        return counts, [c[:n.value] for c in cols]

    def _per_stream(self, who, stream, one):
        """one(s) for ``stream``, or for every stream as a list (the single-stream Pipeline: its one value)."""
        n = getattr(self, "n_streams", 1)
        if stream is None:
            return [one(s) for s in range(n)] if hasattr(self, "n_streams") else one(0)
        if int(stream) < 0 or int(stream) >= n:
            raise ValueError("%s: stream %d outside [0, %d)" % (who, int(stream), n))
        return one(int(stream))

    def set_actions(self, action_id=None):
        """The action stage of every following step (video_detect.py:151-152 on the device): ``action_id`` is an
        action.ActionIdentify (its actions and settings go to the device, fresh orbit caches, one per stream) or an
        action.DeviceActionIdentify of at least as many streams as the pipeline (its caches are used as they are); None switches
        the stage off.  A step then adds one launch behind the association and ``last_actions()`` holds its rows; the step's own
        return value does not change.  ValueError naming action_id for anything the device cannot run; refused (YdsError) while
        a look-ahead pass is in flight."""
        from .action import as_device_actions
        self._set_stage("actions", as_device_actions, action_id)

    def set_frame_times(self, times):
        """Times (seconds) of the frames of the NEXT step, one per frame: every row of a frame carries its frame's time in the
        action stage.  Without it a stream's k-th frame since the pipeline was made carries k / 25."""
        t = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        _lib.check(_lib.load().yds_pipeline_set_frame_times(self._h, _lib.ptr(t), int(t.size)))

    def last_actions(self):
        """Per frame of the last step: ``[(track_id, class_id, name), ...]`` as ActionIdentify.update returns it, ``[]`` where
        nothing fired, None where the frame's rows were None (the stage did not see that frame).  Already on the host."""
        dev = getattr(self, "actions", None)
        got = self._last_report(dev, "actions", [(np.int32, 4)])
        if got is None:
            return None
        counts, (rows,) = got
        per = [None if counts[b] < 0 else [] for b in range(len(counts))]
        for r in rows:
            per[int(r[0])] += dev.name_rows([r])
        return per

    def last_detections(self):
        """Per frame of the last step (any step entry: plain, window, mixed, multi-stream): float32 [n, 5] = x, y, w, h, class of the
        post-NMS, class-masked detections in the frame's own pixels - what the tracker was handed ([0, 5] where the detector
        returned nothing).  The tracker shows only Confirmed tracks, so a person who has just appeared is in these rows before
        any tracker row names them (privacy.Anonymize(include_detections=True)).  Already on the host: no device work."""
        counts = getattr(self, "_last_counts", None)
        if counts is None:
            return None
        lib = _lib.load()
        per = np.zeros(len(counts), np.int32)
        total = lib.yds_pipeline_last_detections(self._h, None, 0, _lib.ptr(per))
        if total < 0:
            raise _lib.YdsError(_lib.last_error())
        rows = np.zeros((max(total, 1), 5), np.float32)
        if lib.yds_pipeline_last_detections(self._h, _lib.ptr(rows), len(rows), _lib.ptr(per)) < 0:
            raise _lib.YdsError(_lib.last_error())
        ends = np.cumsum(per)
        return [rows[e - c:e].copy() for c, e in zip(per.tolist(), ends.tolist())]

    def set_zones(self, zones=None, max_age=30):
        """The zone stage of every following step: ``zones`` is a zones.DeviceZoneMonitor of at least as many streams as the
        pipeline (its tables are used as they are), a zones.ZoneMonitor (its geometry and max_age go to the device, fresh tables,
        for every stream), one (zones, lines) pair for all streams or a list with one pair per stream; None switches the stage
        off.  Geometry is in each stream's own frame pixels.  A step then adds one launch behind the association and
        ``last_zone_events()`` holds its events; the step's own return value does not change.  ValueError naming zones for
        anything the device refuses; refused (YdsError) while a look-ahead pass is in flight."""
        from .zones import as_device_zones
        return self._set_stage("zones", as_device_zones, zones, max_age)

    def last_zone_events(self):
        """Per frame of the last step: ``[(track_id, class_id, kind, zone or line name (index without one), t, dwell), ...]`` as
        ZoneMonitor.update returns it, ``[]`` where nothing happened, None where the frame's rows were None (the stage did not
        see that frame).  Already on the host."""
        dev = getattr(self, "zones", None)
        got = self._last_report(dev, "zone_events", [(np.int32, 6), (np.float64, 2)])
        if got is None:
            return None
        counts, (ev6, evt2) = got
        streams = self._step_streams or [0] * len(counts)
        per = [None if counts[b] < 0 else [] for b in range(len(counts))]
        for r, t in zip(ev6, evt2):
            b = int(r[0])
            per[b] += dev.name_events(streams[b], [r], [t])
        return per

    def zone_counts(self, stream=None):
        """(per zone [occupancy, entries, exits, lost], per line [forward, backward]) of ``stream``, read from the device, or a
        list of such pairs for all streams; None when the stage is off."""
        dev = getattr(self, "zones", None)
        return None if dev is None else self._per_stream("zone_counts", stream, dev.counts)

    def set_heatmap(self, heatmap=None, max_age=30):
        """The heat map stage of every following step: ``heatmap`` is a heatmap.DeviceHeatMap of at least as many streams as the
        pipeline (its layers and tables are used as they are), a heatmap.HeatMap (its spec and max_age go to the device, fresh
        layers, for every stream), one heatmap.HeatSpec for all streams or a list with one per stream; None switches the stage
        off.  A step then adds one launch behind the association and ``heatmap()`` reads the layers; the step's own return value
        does not change.  ValueError naming heatmap for anything the device refuses; refused (YdsError) while a look-ahead pass is
        in flight."""
        from .heatmap import as_device_heatmap
        return self._set_stage("heatmap", as_device_heatmap, heatmap, max_age)

    def heatmap(self, stream=None, layer=None):
        """The layers of ``stream`` as the last step left them, read from the device: int64 [5, gh, gw], or [gh, gw] for a named
        ``layer``; stream=None: a list with one such array per stream (the single-stream Pipeline: its one array).  None when the
        stage is off."""
        dev = getattr(self, "heat", None)
        return None if dev is None else self._per_stream("heatmap", stream, dev.layers if layer is None else (lambda s: dev.layer(s, layer)))

    def set_ground(self, ground=None, max_age=30):
        """The ground plane stage of every following step: ``ground`` is a ground.DeviceGroundMap of at least as many streams as the
        pipeline (its site grid and tables are used as they are), a ground.GroundMap (its specs, max_age and speed_window go to the
        device, a fresh grid), one ground.GroundSpec for all streams or a list with one (or None: that stream is skipped) per stream;
        None switches the stage off.  A step then adds one launch behind the heat map launch, ``last_ground()`` holds its records
        and ``ground_layers()`` reads the site grid; the step's own return value does not change.  ValueError naming ground for
        anything the device refuses; refused (YdsError) while a look-ahead pass is in flight."""
        from .ground import as_device_ground
        return self._set_stage("ground", as_device_ground, ground, max_age)

    def last_ground(self, stream=None):
        """The ground records of the last step, int32 [m, 8] = track id, class, qx, qy, vx, vy, speed, cell (cell -1: outside the
        grid, -2: off plane): a list with one array per frame of the step (None where the frame's rows were None), or with
        ``stream`` the records of that stream's frames of the step in time order as one array.  Already on the host; None when the
        stage is off or no step ran."""
        got = self._last_report(getattr(self, "ground", None), "ground", [(np.int32, 8), (np.int32, 1)])
        if got is None:
            return None
        counts, (rows, frame) = got
        per = [None if counts[b] < 0 else rows[frame == b].copy() for b in range(len(counts))]
        if stream is None:
            return per
        streams = self._step_streams or [0] * len(counts)
        mine = [per[b] for b in range(len(counts)) if streams[b] == int(stream) and per[b] is not None]
        return np.concatenate(mine) if mine else np.zeros((0, 8), np.int32)

    def ground_layers(self, layer=None):
        """The site grid as the last step left it, read from the device: int64 [5, gh, gw], or [gh, gw] for a named ``layer``.  None
        when the stage is off."""
        dev = getattr(self, "ground", None)
        if dev is None:
            return None
        return dev.layers() if layer is None else dev.layer(layer)

    def set_snapshots(self, snapshots=None, max_age=30):
        """The snapshot stage of every following step: ``snapshots`` is a snapshot.DeviceSnapshotBook of at least as many streams as
        the pipeline (its tables, rings and pictures are used as they are), a snapshot.SnapshotBook (its specs and max_age go to the
        device, fresh tables), one snapshot.SnapSpec for all streams or a list with one (or None: that stream is skipped) per stream;
        None switches the stage off.  A step then adds three launches behind the ground launch, over the frames of the step where
        they lie in HBM (before any output stage: anonymisation does not mask the pictures); ``last_snapshot_events()`` holds its
        items and ``snapshots(stream)`` reads the pictures; the step's own return value does not change.  ValueError naming
        snapshots for anything the device refuses; refused (YdsError) while a look-ahead pass is in flight."""
        from .snapshot import as_device_snapshots
        return self._set_stage("snapshots", as_device_snapshots, snapshots, max_age)

    def last_snapshot_events(self, stream=None):
        """The snapshot items of the last step, int32 [m, 6] = frame of the step, track id, class, kind (snapshot.BEST: the picture
        changed, aux = n_seen; snapshot.CLOSED: aux = the ring position or -1), score, aux: a list with one array per frame of the
        step (None where the frame's rows were None), or with ``stream`` the items of that stream's frames of the step in time
        order as one array.  Already on the host; None when the stage is off or no step ran."""
        got = self._last_report(getattr(self, "snap", None), "snapshots", [(np.int32, 6), (np.int32, 1)])
        if got is None:
            return None
        counts, (rows, frame) = got
        per = [None if counts[b] < 0 else rows[frame == b].copy() for b in range(len(counts))]
        if stream is None:
            return per
        streams = self._step_streams or [0] * len(counts)
        mine = [per[b] for b in range(len(counts)) if streams[b] == int(stream) and per[b] is not None]
        return np.concatenate(mine) if mine else np.zeros((0, 6), np.int32)

    def snapshots(self, stream=None, archive=False):
        """The snapshot records of ``stream`` as the last step left them, read from the device (snapshot.DeviceSnapshotBook.tracks;
        archive=True: the archive ring instead), or a list of such lists for all streams; None when the stage is off."""
        dev = getattr(self, "snap", None)
        return None if dev is None else self._per_stream("snapshots", stream, dev.archive if archive else dev.tracks)

    def _search_trackers(self):
        return getattr(self, "deepsorts", None) or [self.ds]

    def search(self, queries, top_k=5, max_dist=None, confirmed_only=True):
        """search.gallery_search over this pipeline's trackers (stream = the stream index of the pipeline; 0 for a single-stream one):
        per query a list of (stream, track_id, dist).  Between steps only; queries: float32 [Q,512] or (device_pointer, Q)."""
        from . import search
        return search.gallery_search(self._search_trackers(), queries, top_k=top_k, max_dist=max_dist, confirmed_only=confirmed_only)

    def link(self, stream, track_id, exclude_stream=None, top_k=5, max_dist=None, confirmed_only=True):
        """search.link_track over this pipeline's trackers: the tracks nearest to live track track_id of stream `stream`."""
        from . import search
        return search.link_track(self._search_trackers(), stream, track_id, exclude_stream=exclude_stream, top_k=top_k, max_dist=max_dist,
                                 confirmed_only=confirmed_only)

    def set_frame_order(self, bgr):
        """bgr=True: the frames handed to step / step_host are B, G, R as a decoder delivers them (read in place, no reversed copy)."""
        _lib.check(_lib.load().yds_pipeline_set_frame_order(self._h, 1 if bgr else 0))

    def prefetch_host(self, frames):
        """Start uploading a batch that a LATER step_host call will receive (one per step; the array must stay alive and
        unchanged until the next step_host call returns)."""
        batch, h, w = _check_host_frames(frames)
        _lib.check(_lib.load().yds_pipeline_prefetch_host(self._h, _lib.ptr(frames), h, w, batch))

    def set_schedule(self, min_crops=None):
        """Crops per batch from which the ReID pass is serialized with the detector passes (own stream otherwise);
        -1 = always two streams, None = the library's policy (both schedules timed on the first steady-state steps, the
        faster one kept: schedule_trial()).  Results do not depend on it."""
        _lib.check(_lib.load().yds_pipeline_set_schedule(self._h, -2 if min_crops is None else int(min_crops)))

    def last_schedule(self):
        return "serialized" if _lib.load().yds_pipeline_last_schedule(self._h) else "two-stream"

    def schedule_trial(self, uploaded=False):
        """What the pipeline's schedule trial measured for an entry (frames resident in HBM / uploaded inside the step):
        dict(decided="serialized" | "two-stream" | None while measuring, serialized_s, two_stream_s: seconds of three measured steps, the better of each schedule's two groups, wall clock between returns of step())."""
        d, a, b = C.c_int(0), C.c_double(0), C.c_double(0)
        _lib.check(_lib.load().yds_pipeline_schedule_trial(self._h, 1 if uploaded else 0, C.byref(d), C.byref(a), C.byref(b)))
        return dict(decided={1: "serialized", -1: "two-stream"}.get(d.value), serialized_s=a.value, two_stream_s=b.value)

    def stage_us(self):
        us = np.zeros(5, np.float32)
        _lib.check(_lib.load().yds_pipeline_stage_us(self._h, _lib.ptr(us)))
        return dict(zip(("resize_dev", "detector_dev", "wait_nms_host", "reid_host", "assoc_host"), us.tolist()))

    def __del__(self):
        try:
            if self._h:
                _lib.load().yds_pipeline_destroy(self._h)
                self._h = None
        except Exception:
            pass


class MultiStreamPipeline(Pipeline):
    """Many video streams through one pipeline (csrc/pipeline.cpp yds_pipeline_create_multi): one DeepSort per stream - clones of
    one DeepSort (deep_sort.py:41-44), sharing its Extractor - and one detector.  A step takes frames of any of the streams (all of
    one size): the detector, NMS and ReID run once over all of them, the association advances every stream's tracker in the same
    launches (a stream's k-th frame of the step in round k).  Per stream the results are those of that stream run alone through
    Pipeline.  Schedule, frame order, prefetch and stage times: as Pipeline.  step_mixed / step_host_mixed take cameras of different
    frame sizes in one step (every frame with its own offset and size); window mode (win_size) takes frames of one size.
    stream_win_sizes: one (w, h) or None per stream - ImageDetector(win_size, overlap) per camera (set_stream_windows), in uniform
    and mixed steps alike; exclusive with win_size."""

    def __init__(self, net, deepsorts, conf_thres=0.5, nms_thres=0.4, class_mask=None, cap=512, win_size=None, overlap=0.15,
                 stream_win_sizes=None):
        from .deep_sort import Extractor
        self._h = None
        deepsorts = list(deepsorts)
        if not deepsorts:
            raise ValueError("MultiStreamPipeline: no streams")
        stream_win_sizes = check_stream_win_sizes(len(deepsorts), win_size, stream_win_sizes)
        ex = deepsorts[0].extractor
        if not isinstance(ex, Extractor) or any(d.extractor is not ex for d in deepsorts):
            raise ValueError("MultiStreamPipeline: the streams' DeepSort objects must share one Extractor (DeepSort.clone())")
        if len({id(d) for d in deepsorts}) != len(deepsorts) or len({id(d.tracker) for d in deepsorts}) != len(deepsorts):
            raise ValueError("MultiStreamPipeline: a DeepSort (or its tracker) is given for more than one stream; use DeepSort.clone()")
        for d in deepsorts:
            _refuse_tracker_nms(d, "MultiStreamPipeline: DeepSort(nms_max_overlap=%r) needs the frame-by-frame path; the batched pipeline "
                                   "has no tracker-side NMS")
        self.net, self.ds, self.deepsorts, self.cap = net, deepsorts[0], deepsorts, int(cap)
        self.n_streams = len(deepsorts)
        mask = np.ascontiguousarray(class_mask if class_mask is not None else [], dtype=np.int32)
        trks = (C.c_void_p * self.n_streams)(*[d.tracker._h for d in deepsorts])
        self._h = _lib.check_ptr(_lib.load().yds_pipeline_create_multi(net._h, ex._h, trks, self.n_streams, conf_thres, nms_thres,
                                                                       _lib.ptr(mask) if mask.size else None, int(mask.size)))
        self.set_windows(win_size, overlap)
        self.stream_win_sizes = [None] * self.n_streams
        for s, ws in enumerate(stream_win_sizes or []):
            if ws is not None:
                self.set_stream_windows(s, ws, overlap)

    def set_stream_windows(self, stream, win_size=None, overlap=0.15):
        """The window setting of ONE stream, ImageDetector(win_size=(win_w, win_h), overlap) of that camera: its frames are cut into
        their own windows whatever their size (None: the plain branch), in step / step_host and step_mixed / step_host_mixed
        (yds_pipeline_set_stream_windows).  Refused (YdsError) for a stream outside [0, n_streams), while a look-ahead pass is in
        flight, and while set_windows holds a setting for all streams."""
        ww, wh = (0, 0) if win_size is None else (int(win_size[0]), int(win_size[1]))
        _lib.check(_lib.load().yds_pipeline_set_stream_windows(self._h, int(stream), ww, wh, float(overlap)))
        self.stream_win_sizes[int(stream)] = None if win_size is None else (ww, wh)

    def set_identities(self, on=True, max_dist=None, max_rows=4096, memory_ids=0, memory_rows=8, memory_ttl=None):
        """Global ids across the streams (identity.IdentityMap over this pipeline's trackers), updated behind every following step:
        one small launch ahead of the step's synchronisation, and the resolve sequence with one more synchronisation only in the
        steps that admit a new track.  ``on`` may also be an IdentityMap made over exactly these trackers in stream order (its
        identities are kept); False / None switches the stage off.  max_dist=None: the first tracker's matching threshold;
        memory_ids > 0 gives the new map a memory of departed identities (identity.IdentityMap; 0, the default: none).  The
        step's own return value does not change: read ``last_identities()``.  Refused (YdsError) while a look-ahead pass is in
        flight and for a map over other trackers."""
        from .identity import IdentityMap
        ident = None
        if isinstance(on, IdentityMap):
            ident = on
        elif on:
            ident = IdentityMap(self.deepsorts, max_dist=max_dist, max_rows=max_rows, memory_ids=memory_ids, memory_rows=memory_rows,
                                memory_ttl=memory_ttl)
        _lib.check(_lib.load().yds_pipeline_set_identities(self._h, None if ident is None else ident.handle))
        self.identities = ident                             # (keeps the handle alive while the pipeline names it)
        return ident

    def last_identities(self, stream=None):
        """The identity map after the last step, from the host copy: dict track_id -> global_id (0 = deferred) of the live
        Confirmed tracks of ``stream``, or a list of such dicts for all streams; None when the stage is off."""
        ident = getattr(self, "identities", None)
        if ident is None:
            return None
        from .identity import _read_ids
        lib = _lib.load()

        return self._per_stream("MultiStreamPipeline", stream, lambda s: _read_ids(
            lambda t, g, cap, n: lib.yds_pipeline_last_identities(self._h, s, t, g, cap, n)))

    def _streams(self, stream_of_frame):
        s = np.ascontiguousarray(stream_of_frame, dtype=np.int32).reshape(-1)
        if s.size < 1 or s.size > self.net.batch_max:
            raise ValueError("MultiStreamPipeline: %d frames in a step, the detector takes 1..%d (Darknet batch_max)" % (s.size, self.net.batch_max))
        if s.min() < 0 or s.max() >= self.n_streams:
            raise ValueError("MultiStreamPipeline: stream ids must lie in [0, %d), got %s" % (self.n_streams, s.tolist()))
        return s

    def step(self, frames_dev, h, w, stream_of_frame, next_frames_dev=None, select_next=None):
        """frames_dev: device pointer to uint8 [n,h,w,3], frame i of stream stream_of_frame[i] (each stream's frames in time order);
        next_frames_dev (optional): the next call's n frames, whose detector pass is enqueued early.  Returns a list per frame of
        int32 [m,6] (None when the detector found nothing and that stream's tracker was not called)."""
        s = self._streams(stream_of_frame)
        return self._run(s.size, select_next, lambda out, counts: _lib.load().yds_pipeline_step_multi(
            self._h, frames_dev, next_frames_dev, h, w, s.size, _lib.ptr(s), out, self.cap, counts), s)

    def step_host(self, frames, stream_of_frame, next_frames=None, select_next=None):
        """frames / next_frames: uint8 [n,h,w,3] HOST arrays, as Pipeline.step_host; frame i of stream stream_of_frame[i]."""
        n, h, w = _check_host_frames(frames, next_frames)
        s = self._streams(stream_of_frame)
        if s.size != n:
            raise ValueError("MultiStreamPipeline: %d frames but %d stream ids" % (n, s.size))
        return self._run(n, select_next, lambda out, counts: _lib.load().yds_pipeline_step_multi_host(
            self._h, _lib.ptr(frames), _lib.ptr(next_frames), h, w, n, _lib.ptr(s), out, self.cap, counts), s)


    def _layout(self, n, frame_off, frame_hw):
        off = np.ascontiguousarray(frame_off, dtype=np.uint64).reshape(-1)
        hw = np.ascontiguousarray(frame_hw, dtype=np.int32)
        if off.size != n or hw.size != 2 * n:
            raise ValueError("MultiStreamPipeline: %d frames need %d offsets and [%d, 2] sizes, got %d and %s" % (n, n, n, off.size, hw.shape))
        return off, hw.reshape(n, 2)

    def step_mixed(self, frames_dev, frame_off, frame_hw, stream_of_frame, frames_bytes, next_frames_dev=None, select_next=None):
        """step() for frames of different sizes: frame i is uint8 [frame_hw[i][0], frame_hw[i][1], 3] at frames_dev + frame_off[i],
        inside a device buffer of frames_bytes bytes (a layout that leaves it raises YdsError before anything runs).
        next_frames_dev (optional): the next call's frames in a buffer of the SAME layout and at least frames_bytes bytes."""
        s = self._streams(stream_of_frame)
        off, hw = self._layout(s.size, frame_off, frame_hw)
        return self._run(s.size, select_next, lambda out, counts: _lib.load().yds_pipeline_step_multi_mixed(
            self._h, frames_dev, next_frames_dev, _lib.ptr(off), _lib.ptr(hw), int(frames_bytes), s.size, _lib.ptr(s), out, self.cap, counts), s)

    def step_host_mixed(self, frames, stream_of_frame, next_frames=None, select_next=None):
        """frames: a list of uint8 [h, w, 3] HOST arrays of any sizes, frame i of stream stream_of_frame[i], or the triple
        pack_frames() made of such a list (a caller that keeps pinned blocks packs once); they are packed back to back into one
        block and uploaded by the pipeline.  next_frames (optional): the next call's frames, given the same way - the same sizes
        in the same order; the next call must then pass the same triple (its block's memory) as `frames`."""
        block, off, hw = frames if isinstance(frames, tuple) else pack_frames(frames)
        s = self._streams(stream_of_frame)
        off, hw = self._layout(s.size, off, hw)
        nxt = None
        if next_frames is not None:
            nxt, noff, nhw = next_frames if isinstance(next_frames, tuple) else pack_frames(next_frames)
            if not (np.array_equal(noff, off) and np.array_equal(np.asarray(nhw).reshape(-1, 2), hw)):
                raise ValueError("MultiStreamPipeline: next_frames must have the layout of frames (the same sizes in the same order)")
            assert nxt.dtype == np.uint8 and nxt.flags["C_CONTIGUOUS"]
        assert block.dtype == np.uint8 and block.flags["C_CONTIGUOUS"]
        self._keep = (block, nxt)
        return self._run(s.size, select_next, lambda out, counts: _lib.load().yds_pipeline_step_multi_mixed_host(
            self._h, _lib.ptr(block), _lib.ptr(nxt), _lib.ptr(off), _lib.ptr(hw), block.nbytes, s.size, _lib.ptr(s), out, self.cap, counts), s)


def conv_timing(net, mode=0):
    """Per tile-variant (total_us, launches, flops, name) of the conv kernel; mode 1 resets+starts, 2 stops."""
    lib = _lib.load()
    nv = lib.yds_conv_num_variants()
    us, fl, by, at = ((C.c_double * nv)() for _ in range(4))
    n = (C.c_int64 * nv)()
    _lib.check(lib.yds_conv_timing_ex(net._h, mode, us, n, fl, by, at))
    return [dict(name=lib.yds_conv_variant_name(v).decode(), us=us[v], launches=n[v], flops=fl[v], bytes=by[v], attainable_us=at[v])
            for v in range(nv)]


def conv_clock(reset=True):
    """(GHz, sampled ms) of the in-kernel clock sampling of a -DYDS_CLOCK_PROBE build since the last reset; (0, 0) from the product
    library, whose kernels carry no sampling code (bench.py then reads the driver's sclk instead: SclkSampler)."""
    ghz, ms = C.c_double(0), C.c_double(0)
    _lib.check(_lib.load().yds_conv_clock(C.byref(ghz), C.byref(ms), 1 if reset else 0))
    return ghz.value, ms.value


class SclkSampler:
    """Samples the driver's shader clock of the bound device (sysfs /sys/bus/pci/devices/<bdf>/pp_dpm_sclk: the line marked '*') on a
    host thread while a workload runs: `with SclkSampler() as s: ...; s.ghz()`.  None when the file is absent or unreadable."""

    def __init__(self, period_s=0.01):
        import threading
        self.period, self.samples, self._stop = period_s, [], threading.Event()
        bdf = _lib.pci_bus_id()
        self.path = "/sys/bus/pci/devices/%s/pp_dpm_sclk" % bdf.lower() if bdf else None
        self._thread = threading.Thread(target=self._run, daemon=True)

    def _read(self):
        try:
            with open(self.path) as f:
                for line in f:
                    if line.rstrip().endswith("*"):
                        return float(line.split(":")[1].lower().split("mhz")[0])
        except Exception:                                   # noqa: BLE001 - no sysfs in this container, another driver version ...
            return None
        return None

    def _run(self):
        while not self._stop.is_set():
            v = self._read()
            if v is not None:
                self.samples.append(v)
            self._stop.wait(self.period)

    def __enter__(self):
        if self.path:
            self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        if self._thread.is_alive():
            self._thread.join(timeout=1)

    def ghz(self):
        busy = [v for v in self.samples if v > 300]          # (drop the idle / sleep state between legs)
        return round(sum(busy) / len(busy) / 1e3, 3) if busy else None


def load_injection_sets(net, sets, logit=6.0):
    """sets: list (per step) of lists (per batch slot) of [n,9] arrays."""
    bm = net.batch_max
    rows, offsets = [], [0]
    for s in sets:
        assert len(s) == bm, "every set needs one table per batch slot"
        for r in s:
            r = np.asarray(r, np.float32).reshape(-1, 9)
            rows.append(r)
            offsets.append(offsets[-1] + r.shape[0])
    rows = np.ascontiguousarray(np.concatenate(rows, 0) if rows else np.zeros((0, 9), np.float32))
    off = np.ascontiguousarray(offsets, dtype=np.int32)
    _lib.check(_lib.load().yds_darknet_load_injection_sets(net._h, _lib.ptr(rows), _lib.ptr(off), len(sets), logit))


def select_injection_set(net, i):
    _lib.check(_lib.load().yds_darknet_select_injection_set(net._h, int(i)))
