"""The source-independent half of VideoDetector.detect / detect_streams (detect.py), none of which needs a GPU: forming the steps
(stream_groups - a single video is a stream group of one), where a step's frames go in a staging block (stage_plan) and when two
steps may share a look-ahead pass (same_composition), the reader thread both generators run (stage_steps), the hand-over between
their threads (give / take / shut_down) and the per-frame bookkeeping of video_detect.py:134-159 (Bookkeeper)."""

from __future__ import annotations

import queue
import time

import numpy as np


def skip_gate(since, skip_frames):
    """The skip_frames gate of video_detect.py:134,157-159: (is this frame processed, frames since the last processed one with
    this one counted).  since: that count before the frame, 0 at the start."""
    proc = since % skip_frames == 0
    return proc, (1 if proc else since + 1)


def stream_groups(its, frames_per_stream, skip_frames, mixed_sizes=False, live=None, source_fps=None, clock=time.time, refusal=None):
    """The steps of detect_streams and of the batched detect(), the only place that reads the sources: a generator of lists of
    (stream, frame, processed, frame time) in yield order.  its: one frame iterator per stream; one step takes from every
    stream that is still running up to frames_per_stream frames that pass the skip_frames gate (the frames the gate skips
    come along, in time order); a stream that ends drops out; a step without frames is not yielded.  Frame times: clock() at
    read for a live stream (live[s]), else the stream's frame index over its rate - source_fps() right after the stream's first
    frame was read, 25 where that gives nothing.  Shapes: all frames one uint8 [h, w, 3] shape, or with mixed_sizes one per
    stream; ValueError otherwise, naming the stream - or saying `refusal`, the message of a caller with a single source."""
    S, F = len(its), int(frames_per_stream)
    live = [False] * S if live is None else list(live)
    shapes, shape = [None] * S, None
    since, alive, n_read, rate = [0] * S, [True] * S, [0] * S, [None] * S
    while any(alive):
        items = []
        for s in range(S):
            n_proc = 0
            while alive[s] and n_proc < F:
                frame = next(its[s], None)
                if frame is None:
                    alive[s] = False
                    break
                if rate[s] is None:
                    rate[s] = float((source_fps() if source_fps is not None else None) or 25.0)
                t_frame = clock() if live[s] else n_read[s] / rate[s]
                n_read[s] += 1
                frame = np.asarray(frame)
                if mixed_sizes:
                    if shapes[s] is None:
                        shapes[s] = frame.shape
                    if frame.shape != shapes[s] or frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
                        raise ValueError("VideoDetector.detect_streams: stream %d must keep one uint8 [h, w, 3] shape (%s, then %s %s)"
                                         % (s, shapes[s], frame.shape, frame.dtype))
                elif shape is None:
                    shape = frame.shape
                if not mixed_sizes and (frame.shape != shape or frame.dtype != np.uint8 or frame.ndim != 3 or shape[2] != 3):
                    raise ValueError(refusal or "VideoDetector.detect_streams: every frame of every source must share one uint8 [h, w, 3] "
                                     "shape (%s, then %s %s in stream %d)" % (shape, frame.shape, frame.dtype, s))
                proc, since[s] = skip_gate(since[s], skip_frames)
                n_proc += proc
                items.append((s, frame, proc, t_frame))
        if items:
            yield items


STAGE_ALIGN = 256          # a mixed step's frames start at multiples of this in the staging block (the mixed entries take any offset)


def stage_plan(items, mixed_sizes=False):
    """Where the frames of one step (stream_groups) go in a staging block: processed frames first, in step order - the
    pipeline wants them in front, and its look-ahead reads nothing behind them - the skipped ones behind.  A dict: slot_of
    (item index -> slot), order (slot -> item index), n_proc, streams (stream of every processed frame, in slot order), off
    (uint64 [n], byte offset of every slot), hw (int32 [n, 2]), nbytes (the end of the last frame), proc_bytes (the end of the
    last processed frame) and mixed.  A uniform step packs its frames h * w * 3 bytes apart, which is the layout the uniform
    entries take; a mixed step starts every frame at a multiple of STAGE_ALIGN."""
    order = [i for i, it in enumerate(items) if it[2]] + [i for i, it in enumerate(items) if not it[2]]
    n_proc = sum(1 for it in items if it[2])
    slot_of = [0] * len(items)
    for slot, i in enumerate(order):
        slot_of[i] = slot
    hw = np.array([items[i][1].shape[:2] for i in order], np.int32).reshape(-1, 2)
    off, at, proc_bytes = np.zeros(len(order), np.uint64), 0, 0
    for slot in range(len(order)):
        if mixed_sizes:
            at = (at + STAGE_ALIGN - 1) // STAGE_ALIGN * STAGE_ALIGN
        off[slot] = at
        at += 3 * int(hw[slot][0]) * int(hw[slot][1])
        if slot < n_proc:
            proc_bytes = at
    return dict(slot_of=slot_of, order=order, n_proc=n_proc, streams=[items[i][0] for i in order[:n_proc]], off=off, hw=hw, nbytes=at,
                proc_bytes=proc_bytes, mixed=bool(mixed_sizes))


def same_composition(cur, nxt):
    """The look-ahead decision of both generators: may the detector pass of the step planned as `nxt` be enqueued with the step
    planned as `cur` (stage_plan dicts)?  Only when both process the same number of frames of the same streams at the same
    offsets and sizes: a stream that ended, skip phases that differ or another layout give False, and the step passes None."""
    if cur is None or nxt is None:
        return False
    n = cur["n_proc"]
    return bool(n > 0 and nxt["n_proc"] == n and cur["mixed"] == nxt["mixed"] and cur["streams"] == nxt["streams"]
                and np.array_equal(cur["hw"][:n], nxt["hw"][:n]) and np.array_equal(cur["off"][:n], nxt["off"][:n]))


# ------------------------------------------------------------------------------------------------ threads and hand-overs
NOTHING = object()         # take(block=False): nothing is waiting


def give(q, item, stop):
    """Hands `item` over through q; never blocks past a stop request (the item is dropped then)."""
    while not stop.is_set():
        try:
            q.put(item, timeout=0.1)
            return
        except queue.Full:
            pass


def take(q, stop, producer=None, block=True):
    """The next item of q (an exception a producer handed over included: the caller raises it in its turn); None after a stop
    request or once the `producer` thread is dead and q is empty; block=False: NOTHING when no item is waiting."""
    while True:
        try:
            return q.get(timeout=0.1) if block else q.get_nowait()
        except queue.Empty:
            if not block:
                return NOTHING
            if stop.is_set() or (producer is not None and not producer.is_alive() and q.empty()):
                return None


def shut_down(stop, free_q, queues, threads):
    """The end of a generator, however it ended: stop request, the block pool poisoned, every hand-over drained (a producer
    waiting on a full one wakes up), the threads joined in the order given."""
    stop.set()
    free_q.put(None)
    for q in queues:
        try:
            while True:
                q.get_nowait()
        except queue.Empty:
            pass
    for t in threads:
        t.join(timeout=5)


def stage_steps(steps, mixed_sizes, upload, out_q, free_q, stop):
    """The reader thread of both generators: every step of `steps` (stream_groups) is planned (stage_plan), put into a block
    taken from free_q by upload(blk, plan, frames) - frames in step order; the device part: VideoDetector._upload_step - and
    handed over as dict(blk, plan, items), the items without their frames: (stream, processed, frame time).  The consumer hands
    the blocks back through free_q.  None follows the last step; an exception (of a source, of the upload) travels through
    out_q too and is raised again on the consumer's side."""
    try:
        for items in steps:
            if stop.is_set():
                return
            plan = stage_plan(items, mixed_sizes)
            blk = free_q.get()
            if blk is None or stop.is_set():
                return
            upload(blk, plan, [it[1] for it in items])
            give(out_q, dict(blk=blk, plan=plan, items=[(s, proc, t) for s, _, proc, t in items]), stop)
        give(out_q, None, stop)
    except BaseException as e:                             # noqa: BLE001 - re-raised on the consumer's side
        give(out_q, e, stop)


class Bookkeeper:
    """The per-frame bookkeeping of video_detect.py:134-159 for n_streams streams: the rows a stream holds (hold), the detections
    they came with (hold_dets, for the anonymise mask) and its last actions (acts).  rows_as_given: the frame-by-frame loop,
    whose tracker's return value is yielded as it is; otherwise empty rows of a pipeline become []."""

    def __init__(self, n_streams=1, rows_as_given=False):
        self.rows_as_given = rows_as_given
        self.hold, self.hold_dets, self.acts = [None] * n_streams, [None] * n_streams, [[] for _ in range(n_streams)]

    def update(self, items, outs, step_acts=None, step_dets=None, host_actions=None):
        """One step.  items: (stream, processed, ...) per frame in yield order; outs: the rows of every processed frame, None where
        the detector returned None; step_acts / step_dets: per processed frame the actions the device found (None on a
        detector-None frame) / the detections handed to the tracker; host_actions: hold -> actions, called in frame order and
        only for a processed frame whose detector did not return None.  Returns (holds, dets, acts), one entry per frame:
        actions are [] on a skipped frame (:158-159) and stay what they were after a detector-None frame (:137-154)."""
        holds, dets, acts, k = [], [], [], 0
        for s, proc, *_ in items:
            if proc:
                o = outs[k]
                self.hold[s] = o if o is None or self.rows_as_given or len(o) else []
                if step_dets is not None:
                    self.hold_dets[s] = step_dets[k]
                if step_acts is not None:
                    if step_acts[k] is not None:
                        self.acts[s] = step_acts[k]
                elif host_actions is not None and o is not None:
                    self.acts[s] = host_actions(self.hold[s])
                k += 1
            else:
                self.acts[s] = []
            holds.append(self.hold[s])
            dets.append(self.hold_dets[s])
            acts.append(self.acts[s])
        return holds, dets, acts
