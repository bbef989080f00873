// Host-side engine classes of libydsort (detector, ReID, tracker, pipeline).
#pragma once
#include "common.h"
#include "conv_weights.h"

#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace yds {

struct CfgBlock {
    std::string type;
    std::map<std::string, std::string> kv;
};
std::vector<CfgBlock> parse_cfg(const std::string &text);

enum LayerType { L_CONV, L_MAXPOOL, L_UPSAMPLE, L_ROUTE, L_SHORTCUT, L_YOLO };     // (the cfg's section names end in the parser)

struct Layer {
    LayerType type = L_CONV;
    int c = 0, h = 0, w = 0;              // logical output shape
    int root = -1, coff = 0;              // storage owner + channel offset (views)
    int src = -1;                         // single data input (conv/pool/upsample/yolo)
    std::vector<int> refs;                // route sources / shortcut operands
    std::vector<std::pair<int, int>> copies;   // (source layer, channel offset) needing a copy kernel
    bool concat() const { return type == L_ROUTE && refs.size() > 1; }   // a route that owns the concatenated buffer
    // conv: geometry (fixed when the net is planned) and folded weights (load_weights) in cw
    int bn = 0, act = ACT_LINEAR;
    ConvWeights cw;
    int fused_res = -1;                   // residual layer absorbed from the following shortcut
    int variant = -1, tuned_batch = 0, tuned_math = -1;   // measured conv tile variant, the batch and math mode it was measured at
    // CSP split (yolov4: conv 1x1, route -2, conv 1x1 - two convolutions of the same tensor): the first one launches both
    // (merge_next = the second conv, merged_into = the first) from the concatenated filters in cw_merged, so the shared input is
    // read from HBM once.  The pairing is part of the static plan; the launch is merged while both have weights (cw_merged loaded).
    int merge_next = -1, merged_into = -1;
    ConvWeights cw_merged;
    // pool / upsample
    int ksize = 1, stride = 1, pad = 0;
    // shortcut / route / pool
    bool fused = false, zero_br = false;
    int groups = 0, group_id = 0;
    // yolo
    std::vector<float> anchors;
    int classes = 0, box_off = 0;
};

// One launch (or launch-shaped piece of work) of a detector pass.  Indices only: views are built when the step is enqueued, because
// they depend on the lane's first image and on buffers that set_batch_max replaces.
struct Step {
    enum Kind { CONV, CONV_MERGED, CONV_STEM2, CONV_BLOCK1, MAXPOOL, UPSAMPLE, COPY, ADD, YOLO };
    Kind kind;
    int layer;                            // cfg position the step runs at (forward_resized_part cuts by it); the layer it writes.
                                          // CONV_MERGED also writes layers[layer].merge_next; CONV_STEM2 / CONV_BLOCK1 compute layer - 1 inside
    int src = -1;                         // MAXPOOL: the tensor read (an earlier pool of the same tensor in an SPP cascade); COPY: source layer
    int arg = 0;                          // COPY: channel offset in the concatenation; YOLO: head index
    int ksize = 1, stride = 1, pad = 0;   // MAXPOOL, as launched (a cascaded pool is 5 / 1 / 2)
    bool zero_br = false;
};
// The steps of one pass in cfg order, for one (batch, conv math, plan epoch).  Everything that decides what layer i costs a launch
// is decided where this is built (Darknet::plan) and nowhere else.
struct LaunchPlan {
    std::vector<Step> steps;
    std::vector<int> produced_by;         // layer -> the step that writes it (a concatenation: its last copy); -1: a view, or a layer
                                          // that a fused launch computes without writing it
    int batch = -1, math = -1, epoch = -1;
};

struct Storage {
    DevBuf<float> buf;
    int ld = 0;
    int fmt = 0;                          // TensorFmt of the owned buffer (H16 only in f16x3 mode, 32-channel granularity)
    int fmt_half = 0;                     // ... while the network is in half mode: FMT_F16 where every user of the buffer can take it (plan_half_formats)
    bool owns = false;                    // this layer owns `buf` (sized by batch_max)
    bool redirected = false;              // producer writes into a slice of storage[into]
    int into = -1, coff = 0;
};

class Darknet {
public:
    Darknet(const std::string &cfg_text, int img_h, int img_w, int batch_max);
    ~Darknet();
    void load_weights(const void *blob, size_t nbytes, int cutoff);
    void set_batch_max(int b);               // re-sizes the activation buffers in place (weights, plan and handle stay)
    void forward_f32_host(const float *nchw, int batch, float *out_host);
    void forward_u8_host(const uint8_t *frames, int h, int w, int batch, float *out_host);
    void forward_u8_dev(const uint8_t *frames_dev, int h, int w, int batch);
    // frames of different sizes: frame n at frames_dev + geom[n].off, one plain slot each (the table is copied before the call returns)
    void forward_u8_frames_dev(const uint8_t *frames_dev, const std::vector<FrameGeom> &geom);
    void forward_resized(int batch) { run_graph(batch); }      // input buffer already filled
    // the same pass enqueued in two pieces (layers [0, head_layers()) and the rest): the pipeline puts another stream-ordered
    // job between them (pipeline.cpp, serialized schedule); false = this configuration runs in lanes and cannot be split
    bool forward_resized_part(int batch, int part);
    int head_layers() const;
    // sliding-window front end (img_detect.py:97-139): windows (x, y, th, tw) of one host frame -> corner-form, window-
    // shifted predictions [n_tiles * total_boxes, attrs] in tiled_pred (windows run in chunks of batch_max)
    void forward_tiles_host(const uint8_t *frame, int h, int w, const int *tiles_xyhw, int n_tiles);
    // slots [0, n_slots) of `slots` (slot_plan.h; device-readable until the pass has run) through the network in chunks of batch_max (a
    // chunk may straddle frames): resize -> network -> a window slot's boxes in corner form, resize_boxes to the window's own size,
    // shifted by the window origin, a plain slot's rows unchanged in centre form, to pred [n_slots * total_boxes, attrs].
    // Asynchronous on `stream`.
    void forward_slots(const uint8_t *frames_dev, const SlotRec *slots, int n_slots, float *pred, bool bgr);
    void layer_output_host(int layer, int batch, float *nchw);
    void get_input_host(int batch, float *nchw);
    void set_injection(int image, const float *rows, int n, float logit);
    void load_injection_sets(const float *rows, const int *offsets, int n_sets, float logit);
    void select_injection_set(int set);
    void enable_conv_timing(bool on);
    void autotune(int batch);                // measure the fastest conv tile per layer at this batch size
    int64_t flops_per_image() const;
    // `batch` images from image `first` of the buffers on (a lane of run_graph starts past 0)
    View view(int layer, int batch, int first = 0) const;
    View input_view(int batch, int first = 0) const;
    // merged: both convolutions of a CSP split in one launch (layer = the first of the pair)
    ConvArgs conv_args(int layer, int batch, int first = 0, bool merged = false) const;

    int img_h, img_w, batch_max, in_channels = 3;
    int math = 0;                            // conv arithmetic the plan (tensor formats) was built for
    bool half_mode = false;                  // Darknet.half(): single-term fp16 operands in the LDS-DMA / window kernels
    void set_half(bool on);                  // half mode on / off: re-plans the activation formats (2-byte tensors while it is on)
    void plan_half_formats();
    int owner_of(int layer, int &off) const; // layer -> the storage its view lives in and the channel offset of that view
    int total_boxes = 0, attrs = 0;
    std::vector<Layer> layers;
    std::vector<Storage> storage;
    std::vector<int> yolo_layers;
    DevBuf<float> input, out, stage_f32;
    DevBuf<uint8_t> stage_u8;
    DevBuf<SlotRec> slot_tab;                                // slots of the last forward_u8_frames_dev / forward_tiles_host
    int stage_h = 0, stage_w = 0, stage_n = 0;               // frames last uploaded by forward_u8_host (device copy in stage_u8)
    DevBuf<float> tiled_pred;
    hipStream_t stream = nullptr;
    // bench-only logit injection
    std::vector<DevBuf<float>> inject_rows;
    std::vector<int> inject_n;
    bool inject_active = false;
    DevBuf<float> inject_table;              // preloaded sets: rows of all (set, image) pairs
    std::vector<int> inject_offsets;         // n_sets * batch_max + 1 row offsets into inject_table
    DevBuf<int> inject_offsets_dev;
    int inject_max_rows = 0;
    int inject_set = -1;
    float inject_logit = 6.f;
    // conv timing: a HIP event pair around every conv launch on this stream, resolved when the counters are read (no host
    // synchronisation inside the pass)
    struct ConvTimeRec { hipEvent_t e0 = nullptr, e1 = nullptr; int variant = 0; double flops = 0, bytes = 0, attain_us = 0; };
    bool time_convs = false;
    std::vector<ConvTimeRec> conv_pending;
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t timing_event();
    void resolve_conv_timing();
    double conv_us[kConvVariants] = {}, conv_flops_acc[kConvVariants] = {}, conv_bytes_acc[kConvVariants] = {}, conv_attain_us[kConvVariants] = {};
    int64_t conv_launches[kConvVariants] = {};

private:
    void allocate_buffers();
    void check_pass(int batch) const;                         // batch within [1, batch_max], conv math the one planned for
    void run_graph(int batch);
    // layers [l0, l1) over images [first, first + batch) on one stream (l1 < 0: to the end)
    void run_lane(int first, int batch, hipStream_t st, int l0 = 0, int l1 = -1);
    void enqueue_conv(const Step &st, int first, int batch, hipStream_t s);
    const LaunchPlan &plan(int batch);                        // the cached step list, rebuilt when its key moved
    LaunchPlan plan_;
    int plan_epoch = 0;                                       // bumped by whatever the plan reads besides batch and conv math: half mode,
                                                              // the buffers (set_batch_max), the weights (load_weights)
    bool stem_fusable = false;                                // layers 0+1 can run as one kernel (conv_stem2.hip)
    int block1_at = -1;                                       // first conv of the fusable residual block (conv_block1.hip), -1: none
    std::vector<hipStream_t> lane_streams;
    std::vector<hipEvent_t> lane_done;
    hipEvent_t lane_fork = nullptr;
};

// --------------------------------------------------------------------------------------------- NMS
// Device multi-label NMS over decoded predictions [n_boxes, attrs] (nms.hip).
// The uniform description of a launch's frames, carried in the kernel arguments: frame f is rows [f * n_boxes, (f + 1) * n_boxes), every
// frame in the same form (corner: x1,y1,x2,y2 as with is_p1p2=True; merge: the reference's merge branch runs) with the same scale.
struct NmsUniform { int32_t n_boxes, corner, merge; float sx, sy; };
class NmsWorkspace {
public:
    explicit NmsWorkspace(int max_candidates = 16384, int frames = 1);
    ~NmsWorkspace();
    NmsWorkspace(const NmsWorkspace &) = delete;
    // asynchronous form: launch() enqueues the kernels, the last of which stores the results into pinned host memory; collect() reads
    // them after the caller synchronised the stream.  One kernel set and one launch sequence, the frames described in one of two ways:
    // uniformly (the plain pipeline pass: no table, no merge kernel unless u.merge) ...
    void launch(const float *pred_dev, const NmsUniform &u, int n_frames, int attrs, float conf_thres, double iou_thres, int cap, hipStream_t s);
    // ... or by a table `fr` [n_frames] (slot_plan.h) which the kernels read on the device, for frames that differ in row count and
    // form - per frame corner form or not, the merge branch or not, its own (sx, sy); max_rows: the largest n_rows, total_rows: the
    // largest row0 + n_rows (box_count is addressed like the prediction block)
    void launch(const float *pred_dev, const NmsFrame *fr, int n_frames, int max_rows, size_t total_rows, int attrs, float conf_thres,
                double iou_thres, int cap, hipStream_t s);
    int collect(int frame, float *out6_host, int cap);
    void resize(int max_candidates, int n_frames);       // (re)allocates; contents are lost
    int needed(int n_frames) const;                       // largest candidate count of the last launch (after the caller's sync)
    static constexpr int kMaxCandidates = 1 << 18;
    // returns number of rows written to out6_host (<= cap); rows sorted by score, boxes in model pixels
    // scaled by (sx, sy) when scale is requested (resize_boxes).
    int run(const float *pred_dev, int n_boxes, int attrs, float conf_thres, double iou_thres, float sx, float sy,
            float *out6_host, int cap, hipStream_t s);
    // merge=True / is_p1p2=True form used by the sliding-window detector: corner-form boxes, the reference's merge branch (the same
    // kernel behind the sweep that a windowed pipeline pass runs)
    int run_merge(const float *pred_dev, int n_boxes, int attrs, float conf_thres, double iou_thres, float *out6_host, int cap, hipStream_t s);
    int max_cand, frames;
    DevBuf<float> cand;          // [max_cand, 6]   x1,y1,x2,y2,score,cls in candidate order
    DevBuf<float> sorted;        // [max_cand, 6]   score order
    DevBuf<int> counts;          // [0] n candidates, [1] n kept
    DevBuf<int> box_count;       // per box candidate count / offsets
    DevBuf<unsigned long long> mask;   // [max_cand, max_cand/64] suppression bits
    DevBuf<float> kept;          // [300, 6]
    int *h_counts = nullptr;     // pinned
    float *h_kept = nullptr;     // pinned [300,6]
};

// --------------------------------------------------------------------------------------------- ReID
class ReidNet {
public:
    explicit ReidNet(int max_crops);
    ~ReidNet();
    void load_tensor(const std::string &name, const float *data, const int64_t *shape, int ndim);
    void finalize();
    void embed_dev(const uint8_t *frame_dev, int h, int w, const float *tlwh_host, int D, float *out_host);
    // crops of several frames in one batch: frame_of[d] selects frames_dev + frame_of[d]*h*w*3; asynchronous
    // geom (n_geom frames): the frames differ in size - frame_of[d] indexes geom instead, h and w are not used, every box is clamped
    // to its own frame; the table travels in the pinned crop list of the pass
    void embed_multi_dev(const uint8_t *frames_dev, int h, int w, const float *tlwh_host, const int *frame_of, int D, bool bgr = false,
                         const FrameGeom *geom = nullptr, int n_geom = 0);
    void preprocess_frames_dev(const uint8_t *frames_dev, const std::vector<FrameGeom> &geom, const float *tlwh_host, const int *frame_of, int D,
                               float *nchw_host);
    void embed_host(const uint8_t *frame_host, int h, int w, const float *tlwh_host, int D, float *out_host);
    void preprocess_host(const uint8_t *frame_host, int h, int w, const float *tlwh_host, int D, float *nchw_host);
    void forward_f32_host(const float *nchw, int D, float *out_host);
    // front == nullptr: input already in `in` (NHWC4).  Otherwise the pass starts from the frames: with the fused front end
    // (reid_stem.hip) where it applies - f16x3 arithmetic, none of YDS_POOL_VALU, YDS_REID_UNFUSED, YDS_REID_FRONT_UNFUSED set -
    // else with the crop kernel into `in`
    void forward(int D, const ReidFront *front = nullptr);
    void reserve(int D);                     // grows the activation buffers (and `feat`) to hold D crops
    float *in_buf();                         // `in`, allocated on first use (the fused front end never touches it), sized by max_crops
    void crop_into_in(const ReidFront &f, int D);            // the crop kernel of the unfused front end
    // crop list of a batched pass into the pinned list whose turn it is; the returned record points into it
    ReidFront stage_crops(const uint8_t *frames_dev, int h, int w, const float *tlwh_host, const int *frame_of, int D, bool bgr,
                          const FrameGeom *geom, int n_geom);
    void allocate_buffers();
    static int64_t flops_per_crop();

    int max_crops;
    std::map<std::string, std::vector<float>> raw;
    std::map<std::string, std::vector<int64_t>> raw_shape;
    bool ready = false;
    std::vector<ConvWeights> convs;                // in execution order
    std::vector<DevBuf<float>> bufs;         // [0], the full-resolution stem output of the unfused pair, is allocated on first use
    DevBuf<float> in, feat, stage_f32;
    DevBuf<uint8_t> stage_u8;
    DevBuf<int> boxes_dev;
    std::vector<int> boxes_host;
    // crop rectangles of the batched pass, in PINNED host memory the crop kernel reads in place (19 KB for 960 crops): no
    // host-to-device copy command on the stream - a pageable hipMemcpyAsync stalls the host behind everything queued on that
    // stream and shares the copy engine with the frame uploads.  Two buffers alternate (a pass may be enqueued while the crop
    // kernel of the previous one has not run yet).
    int *boxes_pin[2] = {nullptr, nullptr};
    size_t boxes_pin_cap[2] = {0, 0};
    int boxes_pin_turn = 0;
    hipStream_t sync_before_regrow = nullptr;   // set by the pipeline while a pass runs on another stream than the previous one
    std::map<int, std::pair<int, int>> tuned;   // conv index -> (D at measurement, measured tile variant)
    int tuned_math = -1;
    hipStream_t stream = nullptr;
    double conv_flops_last = 0;
    bool front_fused_last = false;              // the last forward() began with the fused front end
};

// --------------------------------------------------------------------------------------------- actions
// Implemented in actions.hip: the orbit caches of ActionIdentify (action/action_Identify.py:4-47) for S streams in HBM, advanced over
// the frames of a call by ONE launch (a workgroup per stream walks that stream's frames in order).
// One frame as the kernel reads it: rows6 [n][6] int32 = x1, y1, x2, y2, track id, class - device-readable (HBM, or pinned host
// memory such as a tracker result block).  n_rows_p: where the kernel finds the row count (a result header written earlier on the
// same stream), nullptr = n_rows is the count; with n_rows_p, n_rows is the host's upper bound.  Every row carries time t unless
// row_time (device-readable [n]) names one per row.  tag: what the frame's action rows carry in column 0.
struct ActFrame {
    const int32_t *rows6;
    const int32_t *n_rows_p;
    int n_rows, stream, tag;
    double t;
    const double *row_time;
};
// What the driver of a step needs of a per-stream table stage (actions, zones, heat maps, ground plane, snapshots; their shared frame is
// track_stage.h, their Python front yolo_deepsort_amd/track_stage.py).  The slots of a step, in launch order:
enum StageSlot { STAGE_ACTIONS, STAGE_ZONES, STAGE_HEAT, STAGE_GROUND, STAGE_SNAP, N_STAGES };
// What a call reported, frame k = items [first[k], first[k + 1]): `rows` holds `width` int32 per item (a stage names its width and
// columns below), `tags` one frame tag per item and `times` doubles per item where the stage has them.
struct StageReport {
    std::vector<int32_t> rows, tags;
    std::vector<double> times;
};
struct TrackStageIface {
    virtual ~TrackStageIface() {}
    virtual int streams() const = 0;
    // what a pipeline of n_streams streams asks of a handle before it accepts it; noun: the handle in its words ("a zones")
    virtual void check_for(int n_streams, const char *noun) const {
        if (streams() < n_streams) fail("pipeline: %s handle of %d streams for a pipeline of %d", noun, streams(), n_streams);
    }
    // asynchronous on s: grows the tables, one launch; what the stage reports lands in pinned host memory
    virtual void enqueue(const ActFrame *fr, int n, hipStream_t s) = 0;
    // after the caller synchronised s: the report of that call
    virtual void collect() = 0;
    std::vector<int32_t> first;
    StageReport report;
};
struct ActionsIface : TrackStageIface {};         // report.rows [m][4] tag, id, class, action

// --------------------------------------------------------------------------------------------- zones
// Implemented in zones.hip: per stream a table of tracks with, per zone, an inside bit, a debounce streak and an enter time, advanced
// over the frames of a call by ONE launch over the same frame descriptors as the action stage (row_time is not read: every row of a
// frame carries the frame's time t).
struct ZonesIface : TrackStageIface {};           // report.rows [m][6] tag, id, class, kind, zone or line, 0; report.times [m][2] t, dwell

// --------------------------------------------------------------------------------------------- heat maps
// Implemented in heatmap.hip: per stream a grid of int64 layers and a table of tracks with the cell, time and foot point of their last
// sighting, advanced over the frames of a call by ONE launch over the same frame descriptors as the zone stage.  It reports nothing
// per event: `counted` and `first` only say how many rows of each frame were of the stream's class.  Its check_for also refuses a
// stream without a spec (yds_heatmap_set_stream).
struct HeatmapIface : TrackStageIface {
    std::vector<int32_t> counted;                 // [n] rows counted per frame
};

// --------------------------------------------------------------------------------------------- ground plane
// Implemented in ground.hip: ONE site grid of int64 layers on a floor plan shared by all streams, per stream a homography and a table
// of tracks with a ring of their last plan positions, advanced over the frames of a call by ONE launch over the same frame
// descriptors as the zone stage.  It reports one int32[8] record per counted row: id, class, qx, qy, vx, vy, speed, cell.  A stream
// without a spec (yds_ground_set_stream) is skipped.
struct GroundIface : TrackStageIface {};          // report.rows [m][8]; report.tags [m] the tag of the frame every record belongs to

// --------------------------------------------------------------------------------------------- snapshots
// Implemented in snapshot.hip: per stream a table of tracks with the best thumbnail (uint8 RGB 128 x 64) seen of each, its score, box
// and time, and an archive ring of the snapshots of tracks that left, advanced over the frames of a call by THREE launches (score,
// decide, commit) over the same frame descriptors as the zone stage.  The one stage that reads pixels: ActFrame carries none, so the
// driver of a step hands them over before enqueue - frame tag k of the call is geom_by_tag[k].h x .w x 3 bytes at frames +
// geom_by_tag[k].off, bgr: the bytes are B, G, R.  The table is copied; the pixels must stay device-readable until the call has been
// collected, and serve that one call.  A stream without a spec (yds_snap_set_stream) is skipped.
struct SnapIface : TrackStageIface {              // report.rows [m][6] tag, id, class, kind, score, aux; report.tags [m] = column 0
    virtual void set_pixels(const uint8_t *frames, const FrameGeom *geom_by_tag, int n, bool bgr) = 0;
};

// --------------------------------------------------------------------------------------------- tracker
// Implemented in tracker.hip.  A tracker is state; the association driver (TrackerGroupIface) advances it.
// What a reader of a tracker's appearance galleries needs (gallery_search.hip): device pointers into the tracker's own state, valid
// until its next step (a step may reallocate them), and what the host knows without touching the device.  Track t of the list
// (t < n_tracks) holds n_feat[t] rows at gallery + (slot[t] * budget + r) * 512, r in [0, n_feat[t]).
struct GalleryView {
    const float *gallery;
    const int *slot, *id, *state, *n_feat;
    int budget, n_tracks, metric;
    double max_dist;
    // for a reader that runs inside a step, before its synchronisation (identity.hip): the live track count where the association
    // kernels keep it, the number of slots (the most tracks the step can leave) and whether nn_budget is None
    const int *n_tracks_dev;
    int capacity, unbounded;
    // for the identity memory: hits[t], so that a track's NEWEST row is ring position (hits[t] - 1) mod budget of its slot
    const int *hits;
};
struct TrackerIface {
    virtual ~TrackerIface() {}
    virtual GalleryView gallery_view() const = 0;
    // stand-alone call, one frame through a driver of the tracker's own.  feats: [D,512] on device when feats_on_device, else host.
    // Returns rows written to out6 (int32 [m,6]).
    virtual int step(const float *tlwh_host, const float *feats, bool feats_on_device, const float *payload_host, int D,
                     int32_t *out6_host, int cap) = 0;
    virtual int num_tracks() const = 0;
};
// The cross-camera identity map (identity.hip) as the association driver and the pipeline see it.
struct IdentityIface {
    virtual ~IdentityIface() {}
    // the map was made over exactly these trackers, in this order
    virtual bool bound_to(TrackerIface *const *trk, int S) const = 0;
    // asynchronous on s: ONE small launch over the trackers' state as the work queued on s leaves it; counts land in pinned host memory
    virtual void enqueue_collect(hipStream_t s) = 0;
    // after the caller synchronised s: takes the counts; only when a new track was admitted it launches the resolve sequence on s
    // and synchronises once more
    virtual void finish(hipStream_t s) = 0;
    // the map of the last update, from the host copy: live Confirmed tracks of a stream in track-list order (0 = deferred)
    virtual void get(int stream, int32_t *track_id, int32_t *global_id, int cap, int *n) const = 0;
    // the pipeline that runs the map as a stage (*user is null once that pipeline is gone) and its answer to "is a look-ahead pass
    // in flight": the map refuses to rebuild its memory then, as the pipeline refuses set_identities
    std::shared_ptr<void *> user;
    bool (*user_busy)(void *) = nullptr;
};

// The association driver (tracker.hip TrackerGroup): S trackers (one per video stream; the pipeline of a single stream has S = 1)
// advanced together through the frames of one batch with ONE host synchronisation.  Frame b belongs to tracker stream_of[b], each
// tracker's frames in time order; detections of frame b are rows [first[b], first[b+1]) of tlwh / feats_dev / payload; skip[b] != 0:
// its tracker is not called for that frame (counts[b] = -1).
struct TrackerGroupIface {
    virtual ~TrackerGroupIface() {}
    // the identity stage of the NEXT step_batch (nullptr: none): one small launch behind the action stage, ahead of the step's one
    // synchronisation, and the resolve sequence behind it in the steps that admit a new track.  Cleared by the step.
    virtual void set_identities(IdentityIface *ident) = 0;
    // the table stages of the NEXT step_batch by slot (nullptr: none), N_STAGES of them: one more launch each, in slot order, behind
    // the last round and ahead of the identity collect launch and of the step's one synchronisation; frame_times[b] = time of frame b
    // of that step, the same for every stage.  Cleared by the step.
    virtual void set_stages(TrackStageIface *const *by_slot, const double *frame_times) = 0;
    virtual void step_batch(TrackerIface *const *trk, int S, int n, const int *stream_of, const float *tlwh_host, const int *first,
                            const float *feats_dev, const float *payload_host, const char *skip, int32_t *out6_host, int cap, int32_t *counts) = 0;
    // the next step_batch starts behind `ev` on the driver's stream (features produced on another stream: no host wait)
    virtual void wait_for(hipEvent_t ev) = 0;
};
TrackerGroupIface *make_tracker_group();

}  // namespace yds

// C handles (shared by the translation units that implement the ABI)
struct yds_net { yds::Darknet *d; };
struct yds_reid { yds::ReidNet *r; };
struct yds_trk { yds::TrackerIface *t; };
struct yds_act { yds::ActionsIface *a; };
struct yds_ident { yds::IdentityIface *i; };
struct yds_zones { yds::ZonesIface *z; };
struct yds_heatmap { yds::HeatmapIface *h; };
struct yds_ground { yds::GroundIface *g; };
struct yds_snap { yds::SnapIface *s; };
