// DeepSORT appearance extractor on the HIP conv engine.
//
// Net(reid=True).forward, reference deep_sort/deep/model.py:48-95 (BasicBlock :5-37): stem
// conv3x3(3->64, bias)+BN+ReLU+MaxPool(3,2,1), four stages of two BasicBlocks (64,128,256,512;
// stride-2 first block with a 1x1 stride-2 conv+BN shortcut in stages 2-4), AvgPool(8,4), x/||x||.
// BN is folded into the conv at finalize(); ReLU and the residual add run in the conv epilogue, so a
// crop batch costs 20 conv launches + 1 maxpool + 1 pool/normalise launch.
// Crop boxes follow DeepSort._s_tlwh_to_xyxy (deep_sort/deep_sort.py:116-122): python int()
// truncation of fp32 sums, clipped to [0, W-1] / [0, H-1], end-exclusive slices.
#include "engine.h"
#include "h16.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace yds {

namespace {
struct StageDef { const char *name; int cin, cout; bool down; };
const StageDef kStages[4] = {{"layer1", 64, 64, false}, {"layer2", 64, 128, true}, {"layer3", 128, 256, true}, {"layer4", 256, 512, true}};
constexpr int CROP_H = 128, CROP_W = 64, EMB = 512;
}  // namespace

ReidNet::ReidNet(int max_crops) : max_crops(max_crops) {
    if (max_crops < 1) fail("reid: max_crops must be positive");
    stream = make_stream(false);
}
ReidNet::~ReidNet() {
    if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
    for (int *b : boxes_pin) if (b) (void)hipHostFree(b);
}

void ReidNet::load_tensor(const std::string &name, const float *data, const int64_t *shape, int ndim) {
    size_t n = 1;
    std::vector<int64_t> sh;
    for (int i = 0; i < ndim; ++i) { n *= (size_t)shape[i]; sh.push_back(shape[i]); }
    raw[name].assign(data, data + n);
    raw_shape[name] = sh;
    ready = false;
}

int64_t ReidNet::flops_per_crop() {
    int64_t f = 2ll * 128 * 64 * 64 * 27;                       // stem
    int h = 64, w = 32;
    for (const StageDef &s : kStages) {
        int ho = s.down ? h / 2 : h, wo = s.down ? w / 2 : w;
        f += 2ll * ho * wo * s.cout * 9 * s.cin;                // block0.conv1
        f += 2ll * ho * wo * s.cout * 9 * s.cout * 3;           // block0.conv2, block1.conv1, block1.conv2
        if (s.down) f += 2ll * ho * wo * s.cout * s.cin;        // 1x1 shortcut
        h = ho; w = wo;
    }
    return f;
}

void ReidNet::finalize() {
    auto need = [&](const std::string &k) -> const std::vector<float> & {
        auto it = raw.find(k);
        if (it == raw.end()) fail("reid: state dict lacks '%s'", k.c_str());
        return it->second;
    };
    convs.clear();
    auto add_conv = [&](const std::string &conv, const std::string &bn, int cin_file, int cout, int k, int stride, bool has_bias) {
        const auto &w = need(conv + ".weight");
        if (w.size() != (size_t)cout * cin_file * k * k) fail("reid: %s.weight has %zu elements, expected %d", conv.c_str(), w.size(), cout * cin_file * k * k);
        const auto &g = need(bn + ".weight"), &b = need(bn + ".bias"), &m = need(bn + ".running_mean"), &v = need(bn + ".running_var");
        const std::vector<float> *cb = has_bias ? &need(conv + ".bias") : nullptr;
        ConvWeights c;
        c.shape(cout, cin_file, (cin_file + 3) / 4 * 4, k, stride, k == 3 ? 1 : 0);
        std::vector<double> scale(cout);
        std::vector<float> bias(cout);
        for (int o = 0; o < cout; ++o) {
            scale[o] = (double)g[o] / sqrt((double)v[o] + 1e-5);         // nn.BatchNorm2d default eps
            double b0 = cb ? (double)(*cb)[o] : 0.0;
            bias[o] = (float)((b0 - (double)m[o]) * scale[o] + (double)b[o]);
        }
        c.upload(w.data(), scale.data(), bias.data(), stream);
        convs.push_back(std::move(c));
    };
    add_conv("conv.0", "conv.1", 3, 64, 3, 1, true);
    for (const StageDef &s : kStages) {
        for (int b = 0; b < 2; ++b) {
            std::string p = std::string(s.name) + "." + std::to_string(b);
            int ci = b == 0 ? s.cin : s.cout;
            bool down = b == 0 && s.down;
            add_conv(p + ".conv1", p + ".bn1", ci, s.cout, 3, down ? 2 : 1, false);
            add_conv(p + ".conv2", p + ".bn2", s.cout, s.cout, 3, 1, false);
            if (down) add_conv(p + ".downsample.0", p + ".downsample.1", ci, s.cout, 1, 2, false);
        }
    }
    allocate_buffers();
    ready = true;
}

// activation buffers: input, stem, pooled, then (y1, out, [shortcut]) per block - everything sized by max_crops
// `in` (131 KB per crop) and the stem output (2 MB per crop) serve the unfused front end, the fallback stem and the parity entries only:
// they are allocated where those run (in_buf(), forward) and, once they exist, grow there with max_crops
void ReidNet::allocate_buffers() {
    feat.alloc((size_t)max_crops * EMB);
    bufs.clear();
    bufs.emplace_back();                                                   // 0 stem (on first use)
    bufs.emplace_back((size_t)max_crops * 64 * 32 * 64);                   // 1 pooled
    int h = 64, w = 32;
    for (const StageDef &s : kStages) {
        if (s.down) { h /= 2; w /= 2; }
        for (int k = 0; k < 5; ++k) bufs.emplace_back((size_t)max_crops * h * w * s.cout);   // y1a, outa, sc, y1b, outb
    }
}

// The reference's extractor takes any number of crops (feature_extractor.py:53-58); the buffers grow on demand.
// Nothing of an earlier pass may still be in flight on this stream's buffers when they are replaced.
void ReidNet::reserve(int D) {
    if (D <= max_crops) return;
    YDS_HIP(hipStreamSynchronize(stream));
    int m = max_crops;
    while (m < D) m *= 2;
    max_crops = m;
    if (ready) allocate_buffers();
}

float *ReidNet::in_buf() {
    in.ensure((size_t)max_crops * CROP_H * CROP_W * 4);
    return in.p;
}

void ReidNet::crop_into_in(const ReidFront &f, int D) {
    View x0; x0.p = in_buf(); x0.n = D; x0.h = CROP_H; x0.w = CROP_W; x0.c = 4; x0.ld = 4;
    launch_crop_resize(f, D, x0, stream);
}

void ReidNet::forward(int D, const ReidFront *front) {
    if (!ready) fail("reid: weights not loaded (yds_reid_finalize)");
    if (D < 1) fail("reid: no crops");
    reserve(D);
    const bool f16 = conv_math() == MATH_F16X3;
    auto mk = [&](DevBuf<float> &b, int h, int w, int c) {
        View v; v.p = b.p; v.n = D; v.h = h; v.w = w; v.c = c; v.ld = c;
        v.fmt = (f16 && c % 32 == 0) ? FMT_H16 : FMT_F32;      // activations between the convs stay pre-split
        return v;
    };
    conv_flops_last = 0;
    auto run = [&](int ci, const View &x, const View &y, int act, const View *res, int res_mode) {
        ConvArgs a;
        a.x = x; a.y = y; a.act = act;
        convs[ci].fill(a);
        if (res) { a.res = *res; a.res_mode = res_mode; }
        // measured tile choice per layer; the crop count varies from call to call, so a measurement is reused
        // while D stays within a factor of two of the D it was taken at
        if (tuned_math != conv_math()) { tuned.clear(); tuned_math = conv_math(); }
        auto it = tuned.find(ci);
        if (it == tuned.end() || D > 2 * it->second.first || 2 * D < it->second.first) {
            int v = conv_autotune(a, stream, nullptr);
            tuned[ci] = std::make_pair(D, v);
            it = tuned.find(ci);
        }
        (void)launch_conv(a, stream, it->second.second);
        conv_flops_last += conv_flops(a);
    };
    View cur = mk(bufs[1], 64, 32, 64);
    // frames -> pooled tensor in one kernel: it takes the crop kernel's place as the first launch of the pass
    const bool fused_front = front && f16 && cur.fmt == FMT_H16 && !getenv("YDS_POOL_VALU") && !getenv("YDS_REID_UNFUSED") &&
                             !getenv("YDS_REID_FRONT_UNFUSED");
    front_fused_last = fused_front;
    if (fused_front) {
        const ConvWeights &c = convs[0];
        launch_reid_stem(*front, D, c.wt.p, c.kpad, c.bias.p, cur, stream);
        conv_flops_last += 2.0 * D * CROP_H * CROP_W * 64 * 9 * 4;
    } else {
        if (front) crop_into_in(*front, D);
        in_buf();
        View x0 = mk(in, CROP_H, CROP_W, 4);
        // stem conv + BN + ReLU + MaxPool2d(3, 2, 1) (model.py:52-60) as one kernel; the unfused pair stays as fallback
        ConvArgs a;
        a.x = x0; a.y = cur; a.act = ACT_RELU;
        convs[0].fill(a);
        if (!getenv("YDS_REID_UNFUSED") && launch_conv_maxpool3s2(a, stream)) {
            conv_flops_last += 2.0 * D * CROP_H * CROP_W * 64 * 9 * 4;
        } else {
            bufs[0].ensure((size_t)max_crops * CROP_H * CROP_W * 64);
            View stem = mk(bufs[0], CROP_H, CROP_W, 64);
            run(0, x0, stem, ACT_RELU, nullptr, RES_NONE);
            launch_maxpool(stem, cur, 3, 2, 1, false, stream);
        }
    }
    int ci = 1, bi = 2, h = 64, w = 32;
    for (const StageDef &s : kStages) {
        if (s.down) { h /= 2; w /= 2; }
        for (int b = 0; b < 2; ++b) {
            bool down = b == 0 && s.down;
            View y1 = mk(bufs[bi + (b == 0 ? 0 : 3)], h, w, s.cout);
            View out = mk(bufs[bi + (b == 0 ? 1 : 4)], h, w, s.cout);
            run(ci, cur, y1, ACT_RELU, nullptr, RES_NONE);                        // conv1+bn1+relu
            View res = cur;
            if (down) {
                res = mk(bufs[bi + 2], h, w, s.cout);
                run(ci + 2, cur, res, ACT_LINEAR, nullptr, RES_NONE);             // 1x1 s2 conv + bn
            }
            run(ci + 1, y1, out, ACT_RELU, &res, RES_BEFORE_ACT);                 // relu(x + bn2(conv2))
            ci += down ? 3 : 2;
            cur = out;
        }
        bi += 5;
    }
    launch_avgpool_l2norm(cur, feat.p, stream);
}

// geom: the box of detection d is clamped to frame frame_of[d]'s own size (H, W are not used)
static void crop_boxes_host(const float *tlwh, int D, int H, int W, std::vector<int> &out, const int *frame_of = nullptr,
                            const FrameGeom *geom = nullptr, int n_geom = 0) {
    out.resize((size_t)D * 5);
    for (int d = 0; d < D; ++d) {
        if (geom) {
            if (!frame_of || frame_of[d] < 0 || frame_of[d] >= n_geom) fail("reid: detection %d names frame %d outside [0,%d)", d, frame_of ? frame_of[d] : -1, n_geom);
            H = geom[frame_of[d]].h; W = geom[frame_of[d]].w;
        }
        float x = tlwh[d * 4], y = tlwh[d * 4 + 1], w = tlwh[d * 4 + 2], h = tlwh[d * 4 + 3];
        float xe = x + w, ye = y + h;                         // fp32 sums like the reference's tensor ops
        int x1 = (int)x > 0 ? (int)x : 0;
        int y1 = (int)y > 0 ? (int)y : 0;
        int x2 = (int)xe < W - 1 ? (int)xe : W - 1;
        int y2 = (int)ye < H - 1 ? (int)ye : H - 1;
        if ((x2 <= x1 || y2 <= y1) && geom)                       // frames of different sizes: say which one clamped the box
            fail("reid: detection %d yields an empty crop (%d,%d,%d,%d) in frame %d (%d x %d); cv2.resize raises in the reference", d, x1, y1, x2, y2,
                 frame_of[d], H, W);
        if (x2 <= x1 || y2 <= y1) fail("reid: detection %d yields an empty crop (%d,%d,%d,%d); cv2.resize raises in the reference", d, x1, y1, x2, y2);
        out[d * 5] = x1; out[d * 5 + 1] = y1; out[d * 5 + 2] = x2; out[d * 5 + 3] = y2; out[d * 5 + 4] = frame_of ? frame_of[d] : 0;
    }
}

void ReidNet::embed_dev(const uint8_t *frame_dev, int h, int w, const float *tlwh_host, int D, float *out_host) {
    if (D == 0) return;
    if (!ready) fail("reid: weights not loaded (yds_reid_finalize)");
    reserve(D);
    std::vector<int> boxes;
    crop_boxes_host(tlwh_host, D, h, w, boxes);
    boxes_dev.upload(boxes.data(), boxes.size(), stream);
    YDS_HIP(hipStreamSynchronize(stream));                      // `boxes` is a stack temporary
    ReidFront front;
    front.frames = frame_dev; front.h = h; front.w = w; front.boxes = boxes_dev.p;
    forward(D, &front);
    if (out_host) YDS_HIP(hipMemcpyAsync(out_host, feat.p, (size_t)D * EMB * sizeof(float), hipMemcpyDeviceToHost, stream));
    // always complete before returning: the caller hands `feat` to the tracker, which runs on its own non-blocking
    // stream and would otherwise read features of a pass that is still in flight
    YDS_HIP(hipStreamSynchronize(stream));
}

void ReidNet::embed_multi_dev(const uint8_t *frames_dev, int h, int w, const float *tlwh_host, const int *frame_of, int D, bool bgr,
                              const FrameGeom *geom, int n_geom) {
    if (D == 0) return;
    if (!ready) fail("reid: weights not loaded (yds_reid_finalize)");
    const ReidFront front = stage_crops(frames_dev, h, w, tlwh_host, frame_of, D, bgr, geom, n_geom);
    forward(D, &front);
}

ReidFront ReidNet::stage_crops(const uint8_t *frames_dev, int h, int w, const float *tlwh_host, const int *frame_of, int D, bool bgr,
                               const FrameGeom *geom, int n_geom) {
    reserve(D);
    crop_boxes_host(tlwh_host, D, h, w, boxes_host, frame_of, geom, n_geom);
    // the list of a pass with frames of different sizes starts with their table (n_geom entries of 16 bytes), the boxes follow
    static_assert(sizeof(FrameGeom) == 4 * sizeof(int), "the frame table is laid out in the int list");
    const size_t head = geom ? (size_t)n_geom * 4 : 0, need = head + boxes_host.size();
    const int t = boxes_pin_turn ^= 1;
    if (boxes_pin_cap[t] < need) {
        if (boxes_pin[t]) {
            // the previous tenants of this list may still be read by crop kernels: on this stream, and - when the pipeline moved
            // the pass to another stream since - on the one the earlier pass ran on
            YDS_HIP(hipStreamSynchronize(stream));
            if (sync_before_regrow) YDS_HIP(hipStreamSynchronize(sync_before_regrow));
            (void)hipHostFree(boxes_pin[t]);
            boxes_pin[t] = nullptr;
        }
        boxes_pin_cap[t] = std::max<size_t>(need * 2, 4096);
        YDS_HIP(hipHostMalloc((void **)&boxes_pin[t], boxes_pin_cap[t] * sizeof(int), hipHostMallocDefault));
    }
    if (geom) memcpy(boxes_pin[t], geom, head * sizeof(int));
    memcpy(boxes_pin[t] + head, boxes_host.data(), boxes_host.size() * sizeof(int));
    ReidFront front;
    front.frames = frames_dev; front.h = h; front.w = w; front.bgr = bgr ? 1 : 0;
    front.geom = geom ? reinterpret_cast<const FrameGeom *>(boxes_pin[t]) : nullptr;
    front.boxes = boxes_pin[t] + head;
    return front;
}

void ReidNet::preprocess_frames_dev(const uint8_t *frames_dev, const std::vector<FrameGeom> &geom, const float *tlwh_host, const int *frame_of,
                                    int D, float *nchw_host) {
    if (D == 0) return;
    crop_into_in(stage_crops(frames_dev, 0, 0, tlwh_host, frame_of, D, false, geom.data(), (int)geom.size()), D);
    View x3; x3.p = in.p; x3.n = D; x3.h = CROP_H; x3.w = CROP_W; x3.c = 3; x3.ld = 4;
    nhwc_to_host(x3, nchw_host, stream);
}

void ReidNet::embed_host(const uint8_t *frame_host, int h, int w, const float *tlwh_host, int D, float *out_host) {
    size_t n = (size_t)h * w * 3;
    stage_u8.ensure(n);
    YDS_HIP(hipMemcpyAsync(stage_u8.p, frame_host, n, hipMemcpyHostToDevice, stream));
    embed_dev(stage_u8.p, h, w, tlwh_host, D, out_host);
    YDS_HIP(hipStreamSynchronize(stream));
}

void ReidNet::preprocess_host(const uint8_t *frame_host, int h, int w, const float *tlwh_host, int D, float *nchw_host) {
    if (D == 0) return;
    reserve(D);
    size_t n = (size_t)h * w * 3;
    stage_u8.ensure(n);
    YDS_HIP(hipMemcpyAsync(stage_u8.p, frame_host, n, hipMemcpyHostToDevice, stream));
    std::vector<int> boxes;
    crop_boxes_host(tlwh_host, D, h, w, boxes);
    boxes_dev.upload(boxes.data(), boxes.size(), stream);
    YDS_HIP(hipStreamSynchronize(stream));
    ReidFront front;
    front.frames = stage_u8.p; front.h = h; front.w = w; front.boxes = boxes_dev.p;
    crop_into_in(front, D);
    View x3; x3.p = in.p; x3.n = D; x3.h = CROP_H; x3.w = CROP_W; x3.c = 3; x3.ld = 4;
    nhwc_to_host(x3, nchw_host, stream);
}

void ReidNet::forward_f32_host(const float *nchw, int D, float *out_host) {
    if (D == 0) return;
    if (!ready) fail("reid: weights not loaded (yds_reid_finalize)");
    reserve(D);
    size_t n = (size_t)D * 3 * CROP_H * CROP_W;
    stage_f32.ensure(n);
    YDS_HIP(hipMemcpyAsync(stage_f32.p, nchw, n * sizeof(float), hipMemcpyHostToDevice, stream));
    View x0; x0.p = in_buf(); x0.n = D; x0.h = CROP_H; x0.w = CROP_W; x0.c = 4; x0.ld = 4;
    launch_nchw_to_nhwc(stage_f32.p, x0, 3, stream);
    forward(D);
    YDS_HIP(hipMemcpyAsync(out_host, feat.p, (size_t)D * EMB * sizeof(float), hipMemcpyDeviceToHost, stream));
    YDS_HIP(hipStreamSynchronize(stream));
}

}  // namespace yds

// ============================================================================================ C ABI

extern "C" {

yds_reid *yds_reid_create(int max_crops) {
    YDS_API_BEGIN
    return new yds_reid{new yds::ReidNet(max_crops)};
    YDS_API_END_PTR
}
void yds_reid_destroy(yds_reid *r) {
    if (r) { delete r->r; delete r; }
}
int yds_reid_load_tensor(yds_reid *r, const char *name, const float *data_host, const int64_t *shape, int ndim) {
    YDS_API_BEGIN
    r->r->load_tensor(name, data_host, shape, ndim);
    YDS_API_END
}
int yds_reid_finalize(yds_reid *r) {
    YDS_API_BEGIN
    r->r->finalize();
    YDS_API_END
}
int64_t yds_reid_flops_per_crop(void) { return yds::ReidNet::flops_per_crop(); }
int yds_reid_embed(yds_reid *r, const uint8_t *frame, int h, int w, const float *tlwh, int D, float *out) {
    YDS_API_BEGIN
    r->r->embed_host(frame, h, w, tlwh, D, out);
    YDS_API_END
}
int yds_reid_embed_dev(yds_reid *r, const uint8_t *frame_dev, int h, int w, const float *tlwh, int D, float *out) {
    YDS_API_BEGIN
    r->r->embed_dev(frame_dev, h, w, tlwh, D, out);
    YDS_API_END
}
const float *yds_reid_features_dev(yds_reid *r) { return r->r->feat.p; }
int yds_reid_preprocess(yds_reid *r, const uint8_t *frame, int h, int w, const float *tlwh, int D, float *nchw) {
    YDS_API_BEGIN
    r->r->preprocess_host(frame, h, w, tlwh, D, nchw);
    YDS_API_END
}
int yds_reid_preprocess_mixed(yds_reid *r, const uint8_t *frames_dev, const uint64_t *frame_off, const int32_t *frame_hw, int n_frames,
                              size_t frames_bytes, const float *tlwh, const int32_t *frame_of, int D, float *nchw) {
    YDS_API_BEGIN
    if (!frames_dev) yds::fail("reid: NULL frames");
    r->r->preprocess_frames_dev(frames_dev, yds::checked_layout(frame_off, frame_hw, n_frames, frames_bytes), tlwh, frame_of, D, nchw);
    YDS_API_END
}
int yds_reid_embed_mixed(yds_reid *r, const uint8_t *frames_dev, const uint64_t *frame_off, const int32_t *frame_hw, int n_frames,
                         size_t frames_bytes, const float *tlwh, const int32_t *frame_of, int D, int bgr, float *out) {
    YDS_API_BEGIN
    if (!frames_dev) yds::fail("reid: NULL frames");
    if (D < 1) return 0;
    const std::vector<yds::FrameGeom> geom = yds::checked_layout(frame_off, frame_hw, n_frames, frames_bytes);
    yds::ReidNet &net = *r->r;
    net.embed_multi_dev(frames_dev, 0, 0, tlwh, frame_of, D, bgr != 0, geom.data(), (int)geom.size());
    YDS_HIP(hipMemcpyAsync(out, net.feat.p, (size_t)D * 512 * sizeof(float), hipMemcpyDeviceToHost, net.stream));
    YDS_HIP(hipStreamSynchronize(net.stream));
    YDS_API_END
}
int yds_reid_front_fused(yds_reid *r) { return r && r->r->front_fused_last ? 1 : 0; }
int yds_reid_front_grid_crops(void) {
    YDS_API_BEGIN
    return yds::reid_stem_grid() / yds::kReidStemUnitsPerCrop;
    YDS_API_END
}
int yds_reid_forward_f32(yds_reid *r, const float *nchw, int D, float *out) {
    YDS_API_BEGIN
    r->r->forward_f32_host(nchw, D, out);
    YDS_API_END
}

}  // extern "C"
