// Per-frame hot glue: detect -> NMS -> class mask -> p1p2Toxywh -> ReID -> tracker, in frame order.
//
// Mirrors the loop body of VideoDetector.detect, reference yolo3/detect/video_detect.py:134-157:
//   * ImageDetector.detect (img_detect.py:61-95): resize + /255 + Darknet + NMS + resize_boxes;
//   * the tracker is NOT called when the detector returns None (video_detect.py:137), but IS called
//     with D = 0 when the class mask empties the list (:141-149);
//   * boxes go to the tracker as (x1, y1, x2-x1, y2-y1) fp32 (p1p2Toxywh, model_build.py:326-332),
//     payload = class id.
// Scheduling (results are identical to the frame-by-frame loop, only the order of independent work
// changes):  the detector is stateless, so it runs over a whole batch of frames; NMS for all frames of
// the batch is enqueued behind it; the ReID CNN embeds the crops of ALL frames of the batch in one
// launch sequence; only the association consumes frames strictly in order.  While ReID + association of
// batch i run on their streams, the detector of batch i+1 (if the caller already has those frames) is
// enqueued on the detector stream, so the small latency-bound tracker kernels and their host syncs hide
// under MFMA work.
#include "engine.h"

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <utility>

namespace yds {

// One NMS slot: workspace + pinned results, and the events of the detector pass that uses it.  Two slots alternate, so that the
// pass of batch i+1 can be enqueued before the host has waited for and read the results of batch i: the detector stream never
// drains between passes.
struct DetSlot {
    std::unique_ptr<NmsWorkspace> nms;
    hipEvent_t e0, e1, e2, e_nms;      // pass start, resize (+ head) done, network done, NMS done
    hipEvent_t e_r0, e_r1;             // around a ReID pass enqueued inside this slot's detector pass
    bool reid_in_pass = false;
    DetSlot() { for (hipEvent_t *e : {&e0, &e1, &e2, &e_nms, &e_r0, &e_r1}) YDS_HIP(hipEventCreate(e)); }
    ~DetSlot() {
        for (hipEvent_t e : {e0, e1, e2, e_nms, e_r0, e_r1}) (void)hipEventDestroy(e);
        if (plan_tab) (void)hipHostFree(plan_tab);
    }
    // The plan's two tables (per slot, per frame) as the pass reads them ON THE DEVICE - the resize and box kernels each slot's record, the
    // NMS each frame's descriptor - in pinned host memory the kernels read in place (like the extractor's crop list).  It lives with
    // the DetSlot because those kernels run long after the call that enqueued them has gone on: the look-ahead pass of the next batch
    // is in flight while the host works on this one, and keeps its own copy.  Before the table is rewritten the slot's last pass must
    // have read it: the head's resize (e1) and the NMS (e_nms) - both long over in the steady state, where a slot is reused two passes
    // later; an abandoned look-ahead pass that only got its head is what the wait on e1 is for.
    void *plan_tab = nullptr;
    size_t plan_bytes = 0, plan_slots_n = 0;
    const SlotRec *plan_slots() const { return static_cast<const SlotRec *>(plan_tab); }
    const NmsFrame *plan_frames() const { return reinterpret_cast<const NmsFrame *>(plan_slots() + plan_slots_n); }
    void write_plan(const SlotPlan &pl) {
        YDS_HIP(hipEventSynchronize(e1));
        YDS_HIP(hipEventSynchronize(e_nms));
        const size_t need = pl.slots.size() * sizeof(SlotRec) + pl.frames.size() * sizeof(NmsFrame);
        if (plan_bytes < need) {
            if (plan_tab) (void)hipHostFree(plan_tab);
            plan_tab = nullptr;
            plan_bytes = 0;
            YDS_HIP(hipHostMalloc(&plan_tab, std::max<size_t>(need, 4096), hipHostMallocDefault));
            plan_bytes = std::max<size_t>(need, 4096);
        }
        plan_slots_n = pl.slots.size();
        memcpy(plan_tab, pl.slots.data(), pl.slots.size() * sizeof(SlotRec));
        memcpy(const_cast<NmsFrame *>(plan_frames()), pl.frames.data(), pl.frames.size() * sizeof(NmsFrame));
    }
};

// Where the frames of a step lie.  Uniform (the plain entries): every frame h x w, frame n at byte n * h * w * 3.  Mixed: frame n
// is frames[n].h x frames[n].w at byte frames[n].off (h and w are 0).
struct Geometry {
    int h = 0, w = 0;
    std::vector<FrameGeom> frames;
    bool mixed() const { return !frames.empty(); }
    bool operator==(const Geometry &o) const {
        if (h != o.h || w != o.w || frames.size() != o.frames.size()) return false;
        for (size_t n = 0; n < frames.size(); ++n)
            if (frames[n].off != o.frames[n].off || frames[n].h != o.frames[n].h || frames[n].w != o.frames[n].w) return false;
        return true;
    }
};

// One detector pass (+ NMS) over a batch, as far as it has been enqueued.
struct Pass {
    const uint8_t *frames = nullptr;   // nullptr: no pass (slot still names the DetSlot used last)
    Geometry geo;                      // layout of the frames the pass was enqueued with
    SlotPlan plan;                     // empty: the plain uniform pass; direct: a mixed layout; else slotted (some frame is windowed)
    int batch = 0;
    int slot = 0;                      // DetSlot
    enum { NOTHING, HEAD, WHOLE } done = NOTHING;     // NOTHING with frames set: the head is still to be (re-)enqueued
    bool split = false;                // HEAD: the first layers went with the head, the tail runs the rest
    bool open() const { return frames && done != WHOLE; }
    bool is_whole(const uint8_t *f, int n, const Geometry &g, const SlotPlan &pl) const {
        return frames == f && batch == n && geo == g && plan == pl && done == WHOLE;
    }
};

// ---- frames handed over as HOST memory (img_detect.py:70-71 starts from a host frame) ------------------------------
// Three device staging buffers take turns; the copy runs on its own stream (SDMA engine), so uploads overlap the detector /
// ReID / association of earlier batches.  A batch is matched by its host pointer for a BOUNDED time: the slot is forgotten
// when the step that consumed it returns, and an announced batch that is never consumed is forgotten too (`next` must be the
// following call's `frames`, a prefetch_host batch must be consumed within two calls: Slot::ttl) - so a caller may reuse a
// host buffer for new frames and a later buffer at the same address can never match stale device frames.  A slot is only
// overwritten after the kernels that read it (the detector's resize, the extractor's crops) have passed: the copy stream
// waits on their events.  Pinned source memory (yds_host_alloc) makes the copy asynchronous and full speed.
// Depth: step_host(frames, next) starts the upload of `next` when it is called - but the detector stream runs a whole pass
// ahead of the host chain (NMS -> ReID -> association), so it wants `next` at that very moment and would idle for the
// 1.7 ms of a 100 MB copy (1352 vs 1447 frames/s).  prefetch_host(frames of the step after next) starts that copy one
// step earlier; step_host then finds both of its batches resident.
class FrameStager {
public:
    enum Reader { DET, REID };
    FrameStager(hipStream_t det_stream, hipStream_t reid_stream) : det_stream(det_stream), reid_stream(reid_stream) {
        YDS_HIP(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    }
    ~FrameStager() { (void)hipStreamDestroy(copy_stream); }
    // slot holding the batch uploaded from `host` / the slot whose device buffer is `dev`; -1: none
    int find(const uint8_t *host) const {
        for (int k = 0; k < N; ++k)
            if (host && slots[k].host == host) return k;
        return -1;
    }
    int slot_of(const uint8_t *dev) const {
        for (int k = 0; k < N; ++k)
            if (slots[k].dev.p && dev == slots[k].dev.p) return k;
        return -1;
    }
    const uint8_t *dev(int k) const { return slots[k].dev.p; }
    // ttl: step_host calls the batch survives unconsumed (1 = this step's frames, 2 = its `next`, 3 = a prefetch)
    int upload(const uint8_t *host, size_t bytes, int ttl, int keep_a = -1, int keep_b = -1) {
        int k = -1;
        for (int pass = 0; pass < 2 && k < 0; ++pass)               // next slot in turn: an empty one first, else any not in use
            for (int t = 1; t <= N; ++t) {
                const int c = (turn + t) % N;
                if (c == keep_a || c == keep_b || (pass == 0 && slots[c].host)) continue;
                k = c;
                break;
            }
        if (k < 0) fail("pipeline: no staging buffer free");
        turn = k;
        Slot &s = slots[k];
        // the previous tenant's readers (a prefetched detector pass, an early ReID pass) may still be running on their streams
        for (Read &r : s.rd)
            if (r.set) { YDS_HIP(hipStreamWaitEvent(copy_stream, r.ev, 0)); r.set = false; }
        if (s.dev.n < bytes) {                                      // (re)allocation frees the old buffer: its readers must be done
            YDS_HIP(hipStreamSynchronize(det_stream));
            YDS_HIP(hipStreamSynchronize(reid_stream));
        }
        s.dev.ensure(bytes);
        s.ttl = ttl;
        YDS_HIP(hipMemcpyAsync(s.dev.p, host, bytes, hipMemcpyHostToDevice, copy_stream));
        YDS_HIP(hipEventRecord(s.up_done, copy_stream));
        s.host = host;
        s.up_pending = true;
        return k;
    }
    // `dev` is a staging buffer whose copy is still running: `stream` waits for the copy engine (only then: see Pipeline::step)
    void wait_uploaded(const uint8_t *dev, hipStream_t stream) {
        if (const int k = slot_of(dev); k >= 0 && hipEventQuery(slots[k].up_done) != hipSuccess)
            YDS_HIP(hipStreamWaitEvent(stream, slots[k].up_done, 0));
    }
    // the last kernels of `who` that read staging buffer `dev` have just been enqueued on `stream`
    void mark_read(const uint8_t *dev, hipStream_t stream, Reader who) {
        if (const int k = slot_of(dev); k >= 0) { YDS_HIP(hipEventRecord(slots[k].rd[who].ev, stream)); slots[k].rd[who].set = true; }
    }
    // every host buffer handed over so far may be reused by the caller when the step returns; the consumed batch is forgotten
    void end_of_step(int consumed) {
        for (Slot &s : slots)
            if (s.up_pending) { YDS_HIP(hipEventSynchronize(s.up_done)); s.up_pending = false; }
        slots[consumed].host = nullptr;
        for (int k = 0; k < N; ++k)                                 // announced but never consumed: forget it (its address may be reused)
            if (k != consumed && slots[k].host && --slots[k].ttl <= 0) slots[k].host = nullptr;
        cur = -1;
    }
    int cur = -1, next = -1;           // slots of the running step's frames and of its `next` (the last step's, between steps)

private:
    static constexpr int N = 3;
    struct Read { hipEvent_t ev = nullptr; bool set = false; };       // recorded behind the last kernels that read a slot
    struct Slot {
        DevBuf<uint8_t> dev;           // device copy of the host frames
        const uint8_t *host = nullptr; // where they came from; nullptr: forgotten
        bool up_pending = false;
        int ttl = 0;
        hipEvent_t up_done = nullptr;
        Read rd[2];                    // by Reader
        Slot() { for (hipEvent_t *e : {&up_done, &rd[DET].ev, &rd[REID].ev}) YDS_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming)); }
        ~Slot() { for (hipEvent_t e : {up_done, rd[DET].ev, rd[REID].ev}) (void)hipEventDestroy(e); }
    };
    Slot slots[N];
    int turn = 0;
    hipStream_t copy_stream = nullptr, det_stream, reid_stream;
};

class Pipeline {
public:
    // trks: the tracker of every stream; multi: made by yds_pipeline_create_multi (a step names the stream of each frame)
    Pipeline(Darknet *net, ReidNet *reid, std::vector<TrackerIface *> trks, bool multi, float conf, double nms_iou, const int32_t *mask, int n_mask)
        : net(net), reid(reid), trks(std::move(trks)), group(make_tracker_group()), multi(multi), conf(conf), nms_thres(nms_iou),
          class_mask(mask, mask + n_mask), deep_min(getenv("YDS_PIPE_DEEP_MIN") ? atoi(getenv("YDS_PIPE_DEEP_MIN")) : 64),
          stager(net->stream, reid->stream) {
        for (DetSlot &s : det) s.nms.reset(new NmsWorkspace(4096, net->batch_max));
        YDS_HIP(hipEventCreateWithFlags(&ev_feat, hipEventDisableTiming));
        YDS_HIP(hipEventCreateWithFlags(&ev_reid_done, hipEventDisableTiming));
    }
    ~Pipeline() {
        *self = nullptr;
        (void)hipEventDestroy(ev_feat);
        (void)hipEventDestroy(ev_reid_done);
    }

    // frames handed over as host memory: see FrameStager
    void prefetch_host(const uint8_t *frames_host, int h, int w, int batch) {
        if (stager.find(frames_host) >= 0) return;
        stager.upload(frames_host, (size_t)batch * h * w * 3, 3, stager.cur, stager.next);      // survives this call's step and the next: consumed by the one after
    }
    // bytes: what is uploaded of each host block - batch * h * w * 3, or the span [0, max(off + size)) of a mixed layout
    void step_host(const uint8_t *frames_host, const uint8_t *next_host, const Geometry &geo, size_t bytes, int batch, int32_t *out6, int cap,
                   int32_t *counts) {
        check_step(geo, batch);                                     // (before anything is uploaded)
        // batches handed over earlier (as `next` of the previous call, or through prefetch_host) are already resident or on their way
        stager.cur = stager.find(frames_host);
        if (stager.cur < 0) stager.cur = stager.upload(frames_host, bytes, 1, stager.find(next_host));
        stager.next = next_host ? stager.find(next_host) : -1;
        if (next_host && stager.next < 0) stager.next = stager.upload(next_host, bytes, 2, stager.cur);      // survives this step: the next call's `frames`
        step(stager.dev(stager.cur), stager.next >= 0 ? stager.dev(stager.next) : nullptr, geo, batch, out6, cap, counts, true);
        stager.end_of_step(stager.cur);
    }

    // One detector pass over a batch AND its NMS, all asynchronous on the detector stream, in two pieces (serialized schedule, see
    // step()): head = upload wait + resize + the first layers (Darknet::head_layers), tail = the remaining layers + NMS.  split =
    // false (or a network that cannot be split) puts the whole network into the tail.  launch_detector enqueues what is missing.
    // Two pass forms.  No plan: the plain uniform pass - one stack of frames of one size, geometry and scale as kernel arguments.  A
    // slot plan (slot_plan.h), written into the DetSlot's table by the head: DIRECT (a mixed layout, no windowed frame) keeps that
    // shape, the head's resize reads one plain slot per frame and the ragged NMS reads the network's output in place, frame b = rows
    // [b * total_boxes, +total_boxes) in centre form with its own (sx, sy); SLOTTED (some frame is windowed) runs the whole pass in
    // the tail, see window mode below.
    void launch_detector(Pass &p, bool split = false) {
        if (p.done == Pass::NOTHING) launch_detector_head(p, split);
        if (p.done == Pass::HEAD) launch_detector_tail(p);
    }
    void launch_detector_head(Pass &p, bool split) {
        DetSlot &s = det[p.slot];
        s.reid_in_pass = false;                                     // (a head re-recorded for this slot: no ReID interval of an earlier pass belongs to it)
        stager.wait_uploaded(p.frames, net->stream);                // frames uploaded by step_host: wait for the copy engine
        YDS_HIP(hipEventRecord(s.e0, net->stream));
        p.done = Pass::HEAD;
        p.split = false;
        if (!p.plan.empty()) s.write_plan(p.plan);
        if (p.plan.windowed) {                                      // slotted pass: the whole pass (resize included) is the tail's
            YDS_HIP(hipEventRecord(s.e1, net->stream));
            return;
        }
        if (p.plan.direct()) launch_slot_resize(p.frames, s.plan_slots(), p.batch, net->input_view(p.batch), net->stream, frames_bgr);
        else launch_resize_u8(p.frames, p.batch, p.geo.h, p.geo.w, net->input_view(p.batch), net->stream, frames_bgr);
        YDS_HIP(hipEventRecord(s.e1, net->stream));
        stager.mark_read(p.frames, net->stream, FrameStager::DET);
        p.split = split && net->forward_resized_part(p.batch, 0);
    }
    void launch_detector_tail(Pass &p) {
        DetSlot &s = det[p.slot];
        const size_t per_slot = (size_t)net->total_boxes * net->attrs, n_slots = p.plan.slots.size();
        if (p.plan.windowed) {
            if (win_pred.n < n_slots * per_slot) {
                YDS_HIP(hipStreamSynchronize(net->stream));         // (an NMS of the previous pass may still read the old buffer)
                win_pred.alloc(n_slots * per_slot);
            }
            pred_rows = n_slots * net->total_boxes;
            net->forward_slots(p.frames, s.plan_slots(), (int)n_slots, win_pred.p, frames_bgr);
            stager.mark_read(p.frames, net->stream, FrameStager::DET);
        } else if (p.split) {
            (void)net->forward_resized_part(p.batch, 1);
        } else {
            net->forward_resized(p.batch);
        }
        YDS_HIP(hipEventRecord(s.e2, net->stream));
        if (p.plan.empty()) {
            const float sx = box_scale(p.geo.w, net->img_w), sy = box_scale(p.geo.h, net->img_h);
            s.nms->launch(net->out.p, NmsUniform{net->total_boxes, 0, 0, sx, sy}, p.batch, net->attrs, conf, nms_thres, 300, net->stream);
        } else {
            s.nms->launch(p.plan.windowed ? win_pred.p : net->out.p, s.plan_frames(), p.batch, p.plan.max_rows, n_slots * net->total_boxes,
                          net->attrs, conf, nms_thres, 300, net->stream);
        }
        YDS_HIP(hipEventRecord(s.e_nms, net->stream));
        p.done = Pass::WHOLE;
    }

    // ---- window mode (yds_pipeline_set_windows; ImageDetector(win_size, overlap), img_detect.py:97-151, for a batch of frames) ----
    // Every frame of a step is cut into the same T windows (build_slot_plan: the reference's grid); window t of frame b is slot
    // b * T + t.  The pass is SLOTTED: the slots run through the network in chunks of at most batch_max (Darknet::forward_slots) into
    // win_pred [batch * T * total_boxes, attrs], a frame's rows window-major then in box order - the concatenation of
    // img_detect.py:142, which the stable ranking and the merge branch depend on.  ONE ragged NMS launch per step, n_rows =
    // T * total_boxes per frame, merge branch as a kernel (nms.hip); no copy of candidates to the host and no synchronisation inside
    // the pass.  win_pred holds the FULL shifted predictions (no compaction per chunk): batch * T * total_boxes * attrs * 4 bytes -
    // yolov3-608 (22743 boxes x 85): 7.73 MB per window, 8 frames of 1080p (T = 8) 495 MB.  One buffer serves both NMS slots: the NMS
    // of a pass and the box kernels of the next are ordered by the detector's stream.  A frame smaller than the window (w < win_w and
    // h < win_h, img_detect.py:68) is not cut: the plan is empty and the plain uniform pass runs.
    // Bench-only logit injection addresses the slots of a CHUNK (tables [0, batch_max) of the selected set serve every chunk).
    void set_windows(int ww, int wh, double overlap) {
        if (pending.frames || ahead.reid_in_flight) fail("pipeline: set_windows while a look-ahead pass is in flight (consume it with a step first)");
        if (ww > 0 && wh <= 0) fail("pipeline: window %d x %d", ww, wh);
        if (ww > 0 && !(overlap >= 0)) fail("pipeline: window overlap %g", overlap);
        if (ww > 0 && any_stream_windows()) fail("pipeline: set_windows while a stream holds a window setting of its own (set_stream_windows): one or the other");
        win_w = ww > 0 ? ww : 0; win_h = ww > 0 ? wh : 0; win_overlap = overlap;
    }
    // ---- a window setting per stream (yds_pipeline_set_stream_windows; ImageDetector(win_size, overlap) per camera) ----
    // Frame b of a step belongs to stream stream_of[b]; that stream's setting decides whether the frame is cut into windows (as above,
    // for its own size) or takes the plain branch - no setting, or w < win_w and h < win_h.  A step with at least one windowed frame
    // is slotted like window mode, with frames that differ: every window and every plain frame is one network slot, a windowed frame's
    // rows in corner form in frame pixels, a plain frame's rows as the network gave them; the ragged NMS treats each frame by its
    // descriptor - merge branch and scale 1 for a windowed frame, centre form and the frame's own ratio for a plain one.  A step with
    // no windowed frame runs exactly the launches it runs without any setting.
    bool any_stream_windows() const {
        for (const WindowSetting &sw : stream_win)
            if (sw.w > 0) return true;
        return false;
    }
    void set_stream_windows(int stream, int ww, int wh, double overlap) {
        if (!multi) fail("pipeline: created by yds_pipeline_create: it has no streams (window mode: yds_pipeline_set_windows)");
        if (stream < 0 || stream >= (int)trks.size()) fail("pipeline: stream %d outside [0,%zu)", stream, trks.size());
        if (ww > 0 && wh <= 0) fail("pipeline: window %d x %d", ww, wh);
        if (ww > 0 && !(overlap >= 0)) fail("pipeline: window overlap %g", overlap);
        if (pending.frames || ahead.reid_in_flight)
            fail("pipeline: set_stream_windows while a look-ahead pass is in flight (consume it with a step first)");
        if (win_w > 0) fail("pipeline: set_stream_windows while window mode is on for all streams (yds_pipeline_set_windows): one or the other");
        stream_win.resize(trks.size());
        stream_win[stream] = ww > 0 ? WindowSetting{ww, wh, overlap} : WindowSetting();
    }
    // the plan of a step of `batch` frames laid out by `geo`, frame b of stream stream_of[b]: the setting of all streams, or each
    // frame's stream's own (the two exclude each other)
    SlotPlan make_plan(const Geometry &geo, int batch) const {
        std::vector<WindowSetting> win;
        if (win_w > 0) win.push_back(WindowSetting{win_w, win_h, win_overlap});
        else if (multi && any_stream_windows())
            for (int b = 0; b < batch; ++b) win.push_back(stream_win[stream_of[b]]);
        return build_slot_plan(batch, geo.h, geo.w, geo.mixed() ? geo.frames.data() : nullptr, win, net->img_h, net->img_w, net->total_boxes);
    }

    // detections of one batch after NMS + class mask + p1p2Toxywh, ready for the extractor and the tracker
    struct Dets {
        std::vector<float> tlwh, payload;
        std::vector<int> frame_of, first, n_det;
        const uint8_t *frames = nullptr;
        Geometry geo;                             // layout of `frames`: the crops read it
        SlotPlan plan;                            // plan of the pass the detections came from
        int batch = 0;
        bool reid_in_flight = false;
        hipStream_t reid_on = nullptr;            // stream the ReID pass of this batch was enqueued on
    };

    // wait for the detector pass + NMS `p` (whole), build the detection lists
    void finish_detector(Dets &d, const Pass &p) {
        DetSlot &s = det[p.slot];
        const int batch = p.batch;
        YDS_HIP(hipEventSynchronize(s.e_nms));
        if (s.nms->needed(batch) > s.nms->max_cand) {
            // More candidates than the workspace holds (the reference has no limit): grow it and redo this batch.  The
            // prefetched pass of the next batch may already have overwritten the predictions, so the detector runs again
            // after that pass has drained (its NMS results sit in the other slot's pinned buffers and stay valid).
            // Rare slow path; bench-only logit injection is not re-selected for it.
            YDS_HIP(hipStreamSynchronize(net->stream));
            s.nms->resize(s.nms->needed(batch), s.nms->frames);
            Pass redo{p.frames, p.geo, p.plan, batch, p.slot};
            launch_detector(redo);
            if (pending.done == Pass::HEAD) pending.done = Pass::NOTHING;      // a head enqueued for the next pass has been overwritten
            YDS_HIP(hipEventSynchronize(s.e_nms));
        }
        float ms01 = 0, ms12 = 0;
        YDS_HIP(hipEventElapsedTime(&ms01, s.e0, s.e1));
        YDS_HIP(hipEventElapsedTime(&ms12, s.e1, s.e2));
        if (s.reid_in_pass) {
            // serialized schedule: the ReID pass of the PREVIOUS batch ran on this stream between the head and the tail of this
            // pass (between e1 and e2); its own event pair takes it out of the detector's figure again, so that stage_us[1]
            // means the same under both schedules
            float msr = 0;
            YDS_HIP(hipEventElapsedTime(&msr, s.e_r0, s.e_r1));
            ms12 -= msr;
            s.reid_in_pass = false;
        }
        stage_us[0] = ms01 * 1e3f; stage_us[1] = ms12 * 1e3f;
        std::vector<float> det_rows(300 * 6);
        d.tlwh.clear(); d.payload.clear(); d.frame_of.clear();
        d.first.assign(batch + 1, 0); d.n_det.assign(batch, 0);
        d.frames = p.frames; d.geo = p.geo; d.plan = p.plan; d.batch = batch; d.reid_in_flight = false;
        for (int b = 0; b < batch; ++b) {
            d.n_det[b] = s.nms->collect(b, det_rows.data(), 300);
            for (int i = 0; i < d.n_det[b]; ++i) {
                const float *r = &det_rows[i * 6];
                bool keep = class_mask.empty();
                for (int m : class_mask) keep |= (r[5] == (float)m);
                if (!keep) continue;
                d.tlwh.push_back(r[0]); d.tlwh.push_back(r[1]); d.tlwh.push_back(r[2] - r[0]); d.tlwh.push_back(r[3] - r[1]);
                d.payload.push_back(r[5]);
                d.frame_of.push_back(b);
            }
            d.first[b + 1] = (int)d.payload.size();
        }
    }
    // one ReID pass over the crops of the whole batch, asynchronous on the extractor's stream
    // `on` = the detector's stream: the pass is SERIALIZED with the detector passes (stream order) instead of sharing the CUs
    // with them from the extractor's own stream
    // inside: the pass sits between the head and the tail of that detector pass (serialized schedule) and gets an event pair of
    // its own in the pass's DetSlot (see finish_detector).
    void launch_reid(Dets &d, hipStream_t on = nullptr, const Pass *inside = nullptr) {
        d.reid_on = on ? on : reid->stream;
        if (!d.payload.empty()) {
            struct Swap { hipStream_t &s; hipStream_t keep; ~Swap() { s = keep; } } swap{reid->stream, reid->stream};
            // Both streams' passes use the extractor's ONE set of buffers (input, activations, features, pinned crop list).  A pass
            // on another stream than the previous one (the schedule changed, or an announced batch was abandoned) is ordered
            // behind it explicitly; on the same stream the stream order does it.
            if (reid_last_on && reid_last_on != d.reid_on) YDS_HIP(hipStreamWaitEvent(d.reid_on, ev_reid_done, 0));
            reid->stream = d.reid_on;
            if (reid_last_on && reid_last_on != d.reid_on) reid->sync_before_regrow = reid_last_on;
            if (inside) YDS_HIP(hipEventRecord(det[inside->slot].e_r0, d.reid_on));
            reid->embed_multi_dev(d.frames, d.geo.h, d.geo.w, d.tlwh.data(), d.frame_of.data(), (int)d.payload.size(), frames_bgr,
                                  d.geo.mixed() ? d.geo.frames.data() : nullptr, (int)d.geo.frames.size());
            reid->sync_before_regrow = nullptr;
            if (inside) { YDS_HIP(hipEventRecord(det[inside->slot].e_r1, d.reid_on)); det[inside->slot].reid_in_pass = true; }
            YDS_HIP(hipEventRecord(ev_reid_done, d.reid_on));
            reid_last_on = d.reid_on;
            stager.mark_read(d.frames, d.reid_on, FrameStager::REID);
        }
        d.reid_in_flight = true;
    }

    // ---- stream schedule by measurement (round 5) ----------------------------------------------------------------------
    // Which schedule is faster is a property of the box (round 4: serialized +1.2 % on one, two-stream +1.3-3.1 % on four others),
    // so the pipeline times both on the caller's own steps, like conv_autotune times tile variants: steady-state steps (a next
    // batch handed over, >= 256 crops) run in groups of SKIP + STEPS - serialized, two-stream, serialized, two-stream; the first
    // steps of a group absorb the transition - the wall time of the three measured steps is taken between the returns of step(), and the
    // schedule whose better group is shorter is kept (20 steps in all; round 6: see step_done).
    // Results do not depend on the schedule (parity tests run both), so the trial is invisible to the caller.  One decision per
    // entry (frames resident in HBM / uploaded inside the step): their balance differs.
    struct Trial {
        static constexpr int STEPS = 3, GROUPS = 4;             // groups alternate serialized / two-stream: S T S T
        // unmeasured steps at the head of a group (round 6: two - with ONE the step after a switch still ran short on work the other
        // schedule had left in flight, and serialized measured 7 % faster in the trial where the steady rates were equal)
        static constexpr int SKIP = 2, LEN = SKIP + STEPS;
        int n = 0;                      // steady-state steps seen
        double t0 = 0, t_serial = 0, t_two = 0;   // t0: start of the running group; t_*: the better group of each schedule (3 measured steps)
        int decided = 0;                // 0 = measuring, 1 = serialized, -1 = two-stream
        // Schedule of the NEXT ReID pass while the trial runs.  A group = SKIP transition steps + STEPS measured steps;
        // the groups alternate (serialized first) and each schedule is measured twice, once earlier and once later in the run, so that
        // the clock / temperature drift of the first second under load (the first group ran 7 % faster than steady state on one box)
        // does not decide the comparison.
        bool wants_serial() const { return decided ? decided > 0 : (n / LEN) % 2 == 0; }
        // A group is timed by the wall clock between the RETURNS of step() - the steady-state period, which is what the schedules differ in
        // (round 6 first timed the seconds spent INSIDE step(): that is not the period - the serialized schedule returns earlier relative to
        // the device's work - and it preferred serialized by 8 % where the frame rates were equal; profiles/r06_bench_cfg3.json of that tree).
        // Per schedule the BETTER of its two groups counts (round 6): one hiccup of the caller inside a three-step group - a slow
        // decoder, a consumer rendering - no longer fixes the decision; a steadily slow caller stretches both schedules alike.
        void step_done() {
            if (decided) return;
            const double now = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
            const int group = n / LEN, k = n % LEN;
            if (k == SKIP - 1) t0 = now;                            // the group's transition steps have returned
            if (k == LEN - 1) {
                double &best = group % 2 == 0 ? t_serial : t_two;
                best = best > 0 ? std::min(best, now - t0) : now - t0;
            }
            ++n;
            if (n == GROUPS * LEN) decided = t_serial <= t_two ? 1 : -1;
        }
    };

    // what a step refuses, before anything is uploaded or enqueued
    void check_step(const Geometry &geo, int batch) {
        if (batch < 1 || batch > net->batch_max) fail("pipeline: batch %d outside [1,%d]", batch, net->batch_max);
        if (geo.mixed() && (int)geo.frames.size() != batch) fail("pipeline: a layout of %zu frames for a step of %d", geo.frames.size(), batch);
        if (geo.mixed() && win_w > 0)
            fail("pipeline: window mode takes frames of one size (yds_pipeline_step_multi); a mixed layout is refused while windows are set");
    }
    // geo: the layout of `frames_dev` AND of `next_frames_dev` (a steady camera set; pass no next frames when the layout changes)
    void step(const uint8_t *frames_dev, const uint8_t *next_frames_dev, const Geometry &geo, int batch, int32_t *out6, int cap, int32_t *counts,
              bool uploaded = false) {
        using clk = std::chrono::steady_clock;
        auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<float, std::micro>(b - a).count(); };
        check_step(geo, batch);
        auto t_begin = clk::now();
        const int inject_set = std::exchange(next_inject_set, -1); // bench-only: applies to the pass this step enqueues for `next`
        // The plan of this step, and of the look-ahead pass it enqueues: the next call's frames are planned with THIS step's streams; if
        // the next call names other streams (another plan) the pass is not reused - the rule of a changed layout.
        const SlotPlan plan = make_plan(geo, batch);
        const bool resumed = ahead.reid_in_flight && ahead.frames == frames_dev && ahead.batch == batch && ahead.geo == geo && ahead.plan == plan;
        // Serialized schedule (round 4).  The ReID pass of batch i and the detector pass of batch i+1 are both chip-filling
        // sequences of matrix-core kernels; from two streams they time-share the CUs, every launch stretched by the other
        // stream's work (1.3x on the detector's kernels at cfg2) for the same total.  With >= serial_min crops in the batch the
        // ReID pass is enqueued on the DETECTOR's stream instead, between the head of the next pass (resize + first layers,
        // already queued while the host waited for this batch's NMS and built the crop list: the stream never drains) and its
        // tail: every conv kernel then has the chip to itself, a launch takes its isolated time, and only the association's
        // small kernels (own high-priority stream) run beside them.  Smaller batches (the frame-by-frame API) keep the two-stream
        // form - a 30-crop ReID pass cannot fill the chip and gains from running beside the detector.
        // Measured on the final tree (tools/ab_serial.sh, tools/ab_upload.sh, profiles/r04_serial_schedule_ab.txt; alternating runs on
        // one box), two-stream -> serialized, 32 frames per step, frames resident in HBM:
        //   cfg2 yolov3 1597-1604 -> 1614-1626 frames/s (+1.2 %), window kernel 423 -> 303 us per launch in the pipeline (isolated: 316)
        //   cfg3 yolov4 1499-1501 -> 1515 (+1.0 %), cfg5 yolov4 crowd 682-693 -> 689-690 (equal), exact-fp32 cfg2 573-575 -> 565-566 (-1.5 %)
        // (before the association ran as three launches per frame - round 4 - its ~450 small launches per batch gained from the
        //  two-stream form on yolov4: 1456 -> 1415 then.)  With the frames uploaded inside the step (yds_pipeline_step_host) the
        // serialized form LOSES 4 % (1469-1508 -> 1426-1436: +1.3 ms per step on the detector's stream that neither the start time of
        // the copy nor the result read-back explains - open), so that entry keeps two streams.
        // A detector in half mode keeps two streams as well: its pass is half as long, the (default-arithmetic) ReID pass is 40 % of
        // the step, and its kernels are no longer power bound - running beside the ReID network's gains 3.5 % there (cfg2 --half,
        // alternating runs on one box: 2210-2214 serialized, 2287-2295 two-stream).
        // Policy (round 5): yds_pipeline_set_schedule / YDS_PIPE_SERIAL=<crops> force a threshold (-1 = never serialize); otherwise a
        // ReID pass of >= 256 crops takes the schedule the trial measured faster on THIS box (serialized while none has been
        // decided: see Trial), smaller passes keep two streams.
        const bool forced = schedule_min_crops != INT_MIN || getenv("YDS_PIPE_SERIAL");
        Trial &trial = trials[uploaded ? 1 : 0];
        const int serial_min = schedule_min_crops != INT_MIN ? schedule_min_crops
                               : getenv("YDS_PIPE_SERIAL")  ? atoi(getenv("YDS_PIPE_SERIAL"))
                               : (trial.wants_serial() ? 256 : -1);
        // detector (+ NMS) of the next batch goes in flight, in the DetSlot this batch's pass does not use
        auto launch_next = [&](int this_slot, bool head_only) {
            pending = next_frames_dev ? Pass{next_frames_dev, geo, plan, batch, this_slot ^ 1} : Pass{nullptr, Geometry(), SlotPlan(), 0, this_slot};
            if (!next_frames_dev) return;
            if (inject_set >= 0) net->select_injection_set(inject_set);
            if (head_only) launch_detector_head(pending, true);
            else launch_detector(pending);
        };
        auto copy_feats = [&]() {
            // the tracker reads its own copy so that the extractor can start on the next batch during the association
            if (cur.payload.empty()) return;
            feat_cur.ensure((size_t)reid->max_crops * 512);
            YDS_HIP(hipMemcpyAsync(feat_cur.p, reid->feat.p, cur.payload.size() * 512 * sizeof(float), hipMemcpyDeviceToDevice, cur.reid_on));
            YDS_HIP(hipEventRecord(ev_feat, cur.reid_on));
        };
        bool serial = false;
        if (resumed) {
            std::swap(cur, ahead);                                  // NMS done and ReID already running since the previous call
            ahead.reid_in_flight = false;
            serial = cur.reid_on == net->stream;
            copy_feats();                                           // (behind that ReID pass, ahead of the next detector pass)
            launch_next(pending.slot, false);
        } else {
            ahead.reid_in_flight = false;
            Pass now = pending.is_whole(frames_dev, batch, geo, plan) ? pending : Pass{frames_dev, geo, plan, batch, pending.slot ^ 1};
            launch_detector(now);
            launch_next(now.slot, serial_min >= 0);                 // enqueued BEFORE the host waits for this batch's NMS
            finish_detector(cur, now);
            serial = serial_min >= 0 && (int)cur.payload.size() >= std::max(serial_min, 1);
            if (serial) {
                launch_reid(cur, net->stream, pending.open() ? &pending : nullptr);
                copy_feats();
                if (pending.open()) launch_detector(pending, true);
            } else {
                if (pending.open()) launch_detector(pending, true); // (the head again first if a redone pass overwrote it)
                launch_reid(cur);
                copy_feats();
            }
        }
        last_serial = serial;
        auto t_nms = clk::now();
        const int D_all = (int)cur.payload.size();
        // One frame per step (the frame-by-frame API): the association is ordered behind the features ON THE DEVICE - its stream waits
        // for the event - instead of by a host wake-up between the two (round 6: one round trip less on the latency path; stage_us[3]
        // then holds the enqueue only and stage_us[4] the ReID pass + association).  Batches keep the host wait: it is what lets the
        // host start the next batch's work in the right order below.
        if (D_all) { if (batch == 1 && !next_frames_dev) group->wait_for(ev_feat); else YDS_HIP(hipEventSynchronize(ev_feat)); }
        auto t_reid = clk::now();
        // Crowded scenes (the association of a batch takes long and is all small latency-bound kernels and host syncs):
        // before associating, finish the next batch's detector + NMS and start its ReID pass, so that the matrix
        // cores stay busy underneath.  Sparse scenes keep the simpler order (the detector alone covers the association).
        if (next_frames_dev && D_all >= deep_min * batch) {
            finish_detector(ahead, pending);
            pending.frames = nullptr;                               // consumed: its detections are in `ahead`
            launch_reid(ahead, serial ? net->stream : nullptr);
        }
        // association of the whole batch on the group's stream, one host synchronisation: frame b advances tracker stream_of[b] (a
        // single stream: all zeros), every tracker in the same launches
        std::vector<char> skip(batch, 0);
        for (int b = 0; b < batch; ++b) skip[b] = cur.n_det[b] == 0;  // detector returned None: tracker not called (video_detect.py:137)
        if (!multi) stream_of.assign(batch, 0);
        // the table stages (set_stage): frame b carries the caller's time for it, else its stream's frame count / 25
        std::vector<double> times;
        if ((int)frames_seen.size() < (int)trks.size()) frames_seen.resize(trks.size(), 0);
        const std::vector<double> given = std::move(next_times);      // (they name this step's frames, whatever becomes of it)
        next_times.clear();
        if (std::any_of(stages, stages + N_STAGES, [](const TrackStageIface *sg) { return sg != nullptr; })) {
            if (!given.empty() && (int)given.size() != batch)
                fail("pipeline: %zu frame times for a step of %d frames (yds_pipeline_set_frame_times)", given.size(), batch);
            times.resize(batch);
            std::vector<int64_t> seen(frames_seen);
            for (int b = 0; b < batch; ++b) times[b] = given.empty() ? (double)seen[stream_of[b]]++ / 25.0 : given[b];
            group->set_stages(stages, times.data());
            if (SnapIface *snap = static_cast<SnapIface *>(stages[STAGE_SNAP])) {      // the one stage that reads pixels: this step's frames
                std::vector<FrameGeom> by_frame(cur.geo.frames);
                if (!cur.geo.mixed())
                    for (int b = 0; b < batch; ++b) by_frame.push_back(FrameGeom{(uint64_t)b * cur.geo.h * cur.geo.w * 3, cur.geo.h, cur.geo.w});
                snap->set_pixels(cur.frames, by_frame.data(), batch, frames_bgr);
            }
        }
        for (int b = 0; b < batch; ++b) ++frames_seen[stream_of[b]];
        for (StageReport &r : last) r = StageReport();
        if (identities) group->set_identities(identities);
        group->step_batch(trks.data(), (int)trks.size(), batch, stream_of.data(), cur.tlwh.data(), cur.first.data(), feat_cur.p,
                          cur.payload.data(), skip.data(), out6, cap, counts);
        for (int k = 0; k < N_STAGES; ++k)
            if (stages[k]) last[k] = stages[k]->report;   // (a copy: a stand-alone update on the handle between two steps leaves it alone)
        auto t_end = clk::now();
        stage_us[2] = us(t_begin, t_nms); stage_us[3] = us(t_nms, t_reid); stage_us[4] = us(t_reid, t_end);
        // a steady-state step of a chip-filling ReID pass counts towards the schedule trial of its entry
        if (!forced && next_frames_dev && D_all >= 256) trial.step_done();
    }

    // Several video streams through one pipeline (yds_pipeline_create_multi): one tracker per stream, advanced together by `group`;
    // stream_of[b] = stream of frame b of the step being run (set_streams before step / step_host)
    void set_streams(const int32_t *stream_of_frame, int n) {
        if (!multi) fail("pipeline: created by yds_pipeline_create: it has no streams (use yds_pipeline_step)");
        if (n < 1 || n > net->batch_max) fail("pipeline: batch %d outside [1,%d]", n, net->batch_max);
        for (int b = 0; b < n; ++b)
            if (stream_of_frame[b] < 0 || stream_of_frame[b] >= (int)trks.size())
                fail("pipeline: frame %d belongs to stream %d outside [0,%zu)", b, stream_of_frame[b], trks.size());
        stream_of.assign(stream_of_frame, stream_of_frame + n);
    }

    // ---- the table stages (yds_pipeline_set_actions / _set_zones / _set_heatmap / _set_ground / _set_snapshots; video_detect.py:151-152 for every
    //      stream of a step): a handle of at least as many streams as the pipeline, geometry in each stream's own frame pixels;
    //      nullptr switches the stage off ----
    void set_stage(StageSlot slot, TrackStageIface *sg) {
        static const char *const setter[N_STAGES] = {"set_actions", "set_zones", "set_heatmap", "set_ground", "set_snapshots"};
        static const char *const noun[N_STAGES] = {"an action", "a zones", "a heatmap", "a ground", "a snapshots"};
        if (pending.frames || ahead.reid_in_flight) fail("pipeline: %s while a look-ahead pass is in flight (consume it with a step first)", setter[slot]);
        if (sg) sg->check_for((int)trks.size(), noun[slot]);
        stages[slot] = sg;
        last[slot] = StageReport();
    }
    // m items of a stage's last report for a caller with room for cap: rows of `width` int32, then the tags / times the stage has
    void give_last(StageSlot slot, const char *noun, int width, int32_t *rows_out, int32_t *tags_out, double *times_out, int cap, int *n_out) const {
        const StageReport &r = last[slot];
        const int m = (int)(r.rows.size() / width);
        if (n_out) *n_out = m;
        if (m > cap) fail("pipeline: %d %s exceed the caller's capacity %d", m, noun, cap);
        if (!m) return;
        memcpy(rows_out, r.rows.data(), r.rows.size() * sizeof(int32_t));
        if (tags_out) memcpy(tags_out, r.tags.data(), r.tags.size() * sizeof(int32_t));
        if (times_out) memcpy(times_out, r.times.data(), r.times.size() * sizeof(double));
    }
    TrackStageIface *stages[N_STAGES] = {};       // the table stages of every following step, by slot
    StageReport last[N_STAGES];                   // what each reported in the last step, tagged with the frame of the step
    // ---- the identity stage (yds_pipeline_set_identities): global ids over the streams' trackers, updated behind every step ----
    void set_identities(IdentityIface *i) {
        if (pending.frames || ahead.reid_in_flight) fail("pipeline: set_identities while a look-ahead pass is in flight (consume it with a step first)");
        if (i && !i->bound_to(trks.data(), (int)trks.size()))
            fail("pipeline: the identity map was not created over this pipeline's %zu trackers in stream order", trks.size());
        if (identities) identities->user.reset();
        identities = i;
        if (i) {
            i->user = self;
            i->user_busy = [](void *p) { const Pipeline *me = static_cast<const Pipeline *>(p); return me->pending.frames || me->ahead.reid_in_flight; };
        }
    }
    IdentityIface *identities = nullptr;
    std::shared_ptr<void *> self = std::make_shared<void *>(this);      // what a map bound to this pipeline asks; cleared by ~Pipeline
    std::vector<double> next_times;               // set_frame_times: times of the next step's frames (empty: count / 25)
    std::vector<int64_t> frames_seen;             // frames every stream was handed since the pipeline was made

    Darknet *net;
    ReidNet *reid;
    std::vector<TrackerIface *> trks;             // tracker of each stream
    std::unique_ptr<TrackerGroupIface> group;     // the association driver of all of them
    const bool multi;                             // yds_pipeline_create_multi: the step_multi entries, else the plain ones
    std::vector<int32_t> stream_of;
    float conf;
    double nms_thres;                             // held as double down to the mask kernel, like the reference's threshold
    std::vector<int32_t> class_mask;
    const int deep_min;                           // crowded-scene order from this many detections per frame (YDS_PIPE_DEEP_MIN, read per pipeline)
    DetSlot det[2];
    Pass pending;                   // the pass enqueued for the next call (whole between steps); a fresh pass takes the other DetSlot
    FrameStager stager;             // device copies of host frames (step_host / prefetch_host)
    Dets cur, ahead;                // this batch; the next batch when its ReID pass was started early
    DevBuf<float> feat_cur;
    int next_inject_set = -1;      // bench-only: injection set of the next prefetched detector pass (step() takes it)
    hipEvent_t ev_feat = nullptr;      // this batch's embeddings have been copied for the tracker
    int schedule_min_crops = INT_MIN;  // yds_pipeline_set_schedule: crops per batch from which the ReID pass is serialized (INT_MIN: policy)
    Trial trials[2];                   // schedule trial per entry: [0] frames resident in HBM, [1] uploaded inside the step
    hipEvent_t ev_reid_done = nullptr; // behind the last ReID pass, on the stream it ran on
    hipStream_t reid_last_on = nullptr;
    bool last_serial = false;          // schedule of the last step
    bool frames_bgr = false;           // yds_pipeline_set_frame_order: the frames handed over hold B, G, R bytes (a decoder's order)
    float stage_us[5] = {0, 0, 0, 0, 0};
    int win_w = 0, win_h = 0;          // window mode (set_windows): the setting of all streams
    double win_overlap = 0;
    DevBuf<float> win_pred;            // the prediction block of a slotted pass: shifted corner-form rows of window slots, raw rows of plain ones
    std::vector<WindowSetting> stream_win;        // set_stream_windows: setting of every stream (empty: none was ever set)
    size_t pred_rows = 0;              // rows of the last slotted pass in win_pred (bench / test read-out)
};

}  // namespace yds

struct yds_pipe { yds::Pipeline *p; };

// the four step entries: multi_entry = one that names the stream of each frame; host = frames in host memory (uploaded by the pipeline)
static void pipeline_step(yds_pipe *p, bool multi_entry, bool host, const uint8_t *frames, const uint8_t *next_frames, int h, int w, int n,
                          const int32_t *stream_of_frame, int32_t *out6_host, int cap, int32_t *counts_host) {
    if (multi_entry) p->p->set_streams(stream_of_frame, n);
    else if (p->p->multi) yds::fail("pipeline: created by yds_pipeline_create_multi: use yds_pipeline_step_multi%s", host ? "_host" : "");
    const yds::Geometry geo{h, w, {}};
    if (host) p->p->step_host(frames, next_frames, geo, (size_t)n * h * w * 3, n, out6_host, cap, counts_host);
    else p->p->step(frames, next_frames, geo, n, out6_host, cap, counts_host);
}
// the two mixed entries: every frame with its own (offset, h, w) inside a block of frames_bytes bytes
static void pipeline_step_mixed(yds_pipe *p, bool host, const uint8_t *frames, const uint8_t *next_frames, const uint64_t *frame_off,
                                const int32_t *frame_hw, size_t frames_bytes, int n, const int32_t *stream_of_frame, int32_t *out6_host, int cap,
                                int32_t *counts_host) {
    if (!frames) yds::fail("pipeline: NULL frames");
    p->p->set_streams(stream_of_frame, n);                           // (refuses n outside [1, batch_max] and a single-stream pipeline)
    yds::Geometry geo;
    geo.frames = yds::checked_layout(frame_off, frame_hw, n, frames_bytes);
    if (!host) { p->p->step(frames, next_frames, geo, n, out6_host, cap, counts_host); return; }
    size_t span = 0;
    for (const yds::FrameGeom &g : geo.frames) span = std::max(span, (size_t)(g.off + (uint64_t)g.h * g.w * 3));
    p->p->step_host(frames, next_frames, geo, span, n, out6_host, cap, counts_host);
}

extern "C" {

yds_pipe *yds_pipeline_create(yds_net *n, yds_reid *r, yds_trk *t, float conf_thres, double nms_thres, const int32_t *class_mask, int n_mask) {
    YDS_API_BEGIN
    if (!n || !r || !t) yds::fail("pipeline: NULL handle");
    return new yds_pipe{new yds::Pipeline(n->d, r->r, {t->t}, false, conf_thres, nms_thres, class_mask, class_mask ? n_mask : 0)};
    YDS_API_END_PTR
}
yds_pipe *yds_pipeline_create_multi(yds_net *n, yds_reid *r, yds_trk *const *trks, int n_streams, float conf_thres, double nms_thres,
                                    const int32_t *class_mask, int n_mask) {
    YDS_API_BEGIN
    if (!n || !r || !trks) yds::fail("pipeline: NULL handle");
    if (n_streams < 1) yds::fail("pipeline: %d streams", n_streams);
    std::vector<yds::TrackerIface *> t(n_streams);
    for (int s = 0; s < n_streams; ++s) {
        if (!trks[s]) yds::fail("pipeline: NULL tracker handle of stream %d", s);
        t[s] = trks[s]->t;
        for (int q = 0; q < s; ++q)
            if (trks[q] == trks[s] || t[q] == t[s]) yds::fail("pipeline: streams %d and %d share one tracker (one tracker per stream: DeepSort.clone())", q, s);
    }
    return new yds_pipe{new yds::Pipeline(n->d, r->r, t, true, conf_thres, nms_thres, class_mask, class_mask ? n_mask : 0)};
    YDS_API_END_PTR
}
void yds_pipeline_destroy(yds_pipe *p) {
    if (p) { delete p->p; delete p; }
}
int yds_pipeline_step(yds_pipe *p, const uint8_t *frames_dev, const uint8_t *next_frames_dev, int h, int w, int batch, int32_t *out6_host,
                      int cap, int32_t *counts_host) {
    YDS_API_BEGIN
    pipeline_step(p, false, false, frames_dev, next_frames_dev, h, w, batch, nullptr, out6_host, cap, counts_host);
    YDS_API_END
}
int yds_pipeline_step_host(yds_pipe *p, const uint8_t *frames_host, const uint8_t *next_frames_host, int h, int w, int batch,
                           int32_t *out6_host, int cap, int32_t *counts_host) {
    YDS_API_BEGIN
    pipeline_step(p, false, true, frames_host, next_frames_host, h, w, batch, nullptr, out6_host, cap, counts_host);
    YDS_API_END
}
int yds_pipeline_step_multi(yds_pipe *p, const uint8_t *frames_dev, const uint8_t *next_frames_dev, int h, int w, int n_frames,
                            const int32_t *stream_of_frame, int32_t *out6_host, int cap, int32_t *counts_host) {
    YDS_API_BEGIN
    pipeline_step(p, true, false, frames_dev, next_frames_dev, h, w, n_frames, stream_of_frame, out6_host, cap, counts_host);
    YDS_API_END
}
int yds_pipeline_step_multi_host(yds_pipe *p, const uint8_t *frames_host, const uint8_t *next_frames_host, int h, int w, int n_frames,
                                 const int32_t *stream_of_frame, int32_t *out6_host, int cap, int32_t *counts_host) {
    YDS_API_BEGIN
    pipeline_step(p, true, true, frames_host, next_frames_host, h, w, n_frames, stream_of_frame, out6_host, cap, counts_host);
    YDS_API_END
}
int yds_pipeline_step_multi_mixed(yds_pipe *p, const uint8_t *frames_dev, const uint8_t *next_frames_dev, const uint64_t *frame_off,
                                  const int32_t *frame_hw, size_t frames_bytes, int n_frames, const int32_t *stream_of_frame, int32_t *out6_host,
                                  int cap, int32_t *counts_host) {
    YDS_API_BEGIN
    pipeline_step_mixed(p, false, frames_dev, next_frames_dev, frame_off, frame_hw, frames_bytes, n_frames, stream_of_frame, out6_host, cap,
                        counts_host);
    YDS_API_END
}
int yds_pipeline_step_multi_mixed_host(yds_pipe *p, const uint8_t *frames_host, const uint8_t *next_frames_host, const uint64_t *frame_off,
                                       const int32_t *frame_hw, size_t frames_bytes, int n_frames, const int32_t *stream_of_frame,
                                       int32_t *out6_host, int cap, int32_t *counts_host) {
    YDS_API_BEGIN
    pipeline_step_mixed(p, true, frames_host, next_frames_host, frame_off, frame_hw, frames_bytes, n_frames, stream_of_frame, out6_host, cap,
                        counts_host);
    YDS_API_END
}
int yds_pipeline_prefetch_host(yds_pipe *p, const uint8_t *frames_host, int h, int w, int batch) {
    YDS_API_BEGIN
    p->p->prefetch_host(frames_host, h, w, batch);
    YDS_API_END
}
int yds_pipeline_set_next_injection(yds_pipe *p, int set) {
    YDS_API_BEGIN
    p->p->next_inject_set = set;
    YDS_API_END
}
int yds_pipeline_set_frame_order(yds_pipe *p, int bgr) {
    YDS_API_BEGIN
    p->p->frames_bgr = bgr != 0;
    YDS_API_END
}
int yds_pipeline_set_windows(yds_pipe *p, int win_w, int win_h, double overlap) {
    YDS_API_BEGIN
    p->p->set_windows(win_w, win_h, overlap);
    YDS_API_END
}
int yds_pipeline_set_stream_windows(yds_pipe *p, int stream, int win_w, int win_h, double overlap) {
    YDS_API_BEGIN
    p->p->set_stream_windows(stream, win_w, win_h, overlap);
    YDS_API_END
}
int yds_pipeline_set_actions(yds_pipe *p, yds_act *a) {
    YDS_API_BEGIN
    p->p->set_stage(yds::STAGE_ACTIONS, a ? a->a : nullptr);
    YDS_API_END
}
int yds_pipeline_set_frame_times(yds_pipe *p, const double *t_host, int n) {
    YDS_API_BEGIN
    if (n < 0 || (n && !t_host)) yds::fail("pipeline: %d frame times", n);
    p->p->next_times.assign(t_host, t_host + n);
    YDS_API_END
}
int yds_pipeline_last_actions(yds_pipe *p, int32_t *out4_host, int cap, int *n_out) {
    YDS_API_BEGIN
    p->p->give_last(yds::STAGE_ACTIONS, "action rows", 4, out4_host, nullptr, nullptr, cap, n_out);
    YDS_API_END
}
int yds_pipeline_last_detections(yds_pipe *p, float *rows5_host, int cap, int32_t *counts_host) {
    try {
        if (!p || !counts_host) yds::fail("pipeline: NULL argument");
        const yds::Pipeline::Dets &d = p->p->cur;                 // (finish_detector filled it on the host; the step has returned)
        if (d.batch < 1) yds::fail("pipeline: no step has run");
        const int total = (int)d.payload.size();
        for (int b = 0; b < d.batch; ++b) counts_host[b] = d.first[b + 1] - d.first[b];
        if (rows5_host) {
            if (total > cap) yds::fail("pipeline: %d detections exceed the caller's capacity %d", total, cap);
            for (int i = 0; i < total; ++i) {
                memcpy(rows5_host + (size_t)i * 5, d.tlwh.data() + (size_t)i * 4, 4 * sizeof(float));
                rows5_host[(size_t)i * 5 + 4] = d.payload[i];
            }
        }
        return total;
    } catch (const std::exception &e) {
        yds::set_error(e.what());
        return -1;
    }
}
int yds_pipeline_set_zones(yds_pipe *p, yds_zones *z) {
    YDS_API_BEGIN
    p->p->set_stage(yds::STAGE_ZONES, z ? z->z : nullptr);
    YDS_API_END
}
int yds_pipeline_set_heatmap(yds_pipe *p, yds_heatmap *h) {
    YDS_API_BEGIN
    p->p->set_stage(yds::STAGE_HEAT, h ? h->h : nullptr);
    YDS_API_END
}
int yds_pipeline_set_ground(yds_pipe *p, yds_ground *g) {
    YDS_API_BEGIN
    p->p->set_stage(yds::STAGE_GROUND, g ? g->g : nullptr);
    YDS_API_END
}
int yds_pipeline_set_snapshots(yds_pipe *p, yds_snap *g) {
    YDS_API_BEGIN
    p->p->set_stage(yds::STAGE_SNAP, g ? g->s : nullptr);
    YDS_API_END
}
int yds_pipeline_last_snapshots(yds_pipe *p, int32_t *items6_host, int32_t *frame_host, int cap, int *n_out) {
    YDS_API_BEGIN
    p->p->give_last(yds::STAGE_SNAP, "snapshot items", 6, items6_host, frame_host, nullptr, cap, n_out);
    YDS_API_END
}
int yds_pipeline_last_ground(yds_pipe *p, int32_t *rows8_host, int32_t *frame_host, int cap, int *n_out) {
    YDS_API_BEGIN
    p->p->give_last(yds::STAGE_GROUND, "ground rows", 8, rows8_host, frame_host, nullptr, cap, n_out);
    YDS_API_END
}
int yds_pipeline_last_zone_events(yds_pipe *p, int32_t *ev6_host, double *evt2_host, int cap, int *n_out) {
    YDS_API_BEGIN
    p->p->give_last(yds::STAGE_ZONES, "zone events", 6, ev6_host, nullptr, evt2_host, cap, n_out);
    YDS_API_END
}
int yds_pipeline_set_identities(yds_pipe *p, yds_ident *i) {
    YDS_API_BEGIN
    p->p->set_identities(i ? i->i : nullptr);
    YDS_API_END
}
int yds_pipeline_last_identities(yds_pipe *p, int stream, int32_t *track_id, int32_t *global_id, int cap, int *n) {
    YDS_API_BEGIN
    if (!p->p->identities) yds::fail("pipeline: no identity map is set (yds_pipeline_set_identities)");
    p->p->identities->get(stream, track_id, global_id, cap, n);
    YDS_API_END
}
int yds_pipeline_slot_pred(yds_pipe *p, float *pred_host, size_t cap_rows, size_t *n_rows) {
    YDS_API_BEGIN
    yds::Pipeline *pp = p->p;
    YDS_HIP(hipStreamSynchronize(pp->net->stream));
    if (n_rows) *n_rows = pp->pred_rows;
    const size_t rows = std::min(cap_rows, pp->pred_rows);
    if (pred_host && rows) YDS_HIP(hipMemcpy(pred_host, pp->win_pred.p, rows * pp->net->attrs * sizeof(float), hipMemcpyDeviceToHost));
    YDS_API_END
}
int yds_pipeline_set_schedule(yds_pipe *p, int min_crops) {
    YDS_API_BEGIN
    p->p->schedule_min_crops = min_crops < -1 ? INT_MIN : min_crops;
    YDS_API_END
}
int yds_pipeline_last_schedule(yds_pipe *p) {
    return p && p->p->last_serial ? 1 : 0;
}
int yds_pipeline_schedule_trial(yds_pipe *p, int uploaded, int *decided, double *serialized_s, double *two_stream_s) {
    YDS_API_BEGIN
    const yds::Pipeline::Trial &t = p->p->trials[uploaded ? 1 : 0];
    if (decided) *decided = t.decided;
    if (serialized_s) *serialized_s = t.t_serial;
    if (two_stream_s) *two_stream_s = t.t_two;
    YDS_API_END
}
int yds_pipeline_stage_us(yds_pipe *p, float *us5) {
    YDS_API_BEGIN
    for (int i = 0; i < 5; ++i) us5[i] = p->p->stage_us[i];
    YDS_API_END
}

}  // extern "C"
