// Single convolutions through the C ABI: yds_conv_bench times one layer shape on synthetic data, yds_conv_run runs one tile variant
// on the caller's tensors (the kernel tests).  Both build the same case - input and residual (pre-split where the kernels take them
// that way), weights, output - and differ in what they do with the launch.  yds_conv_run_view is yds_conv_run on channel slices of
// wider buffers and on the merged launch of two convolutions; yds_conv_run_half is that entry in half mode (single-term fp16 operands,
// optionally 2-byte F16 tensors); yds_conv_run_fused launches the kernels that exist only as fused multi-layer launches.
#include "conv_common.h"
#include "conv_weights.h"
#include "h16.h"

#include <algorithm>
#include <math.h>
#include <stdlib.h>
#include <string.h>

namespace yds {
namespace {

// fp16(x * 2^-8) as f16_store4 encodes it: round to nearest even, an overflow saturates at +-65504 (infinities and NaNs pass)
uint16_t f16_bits_saturating(float x) {
    const float xs = x * H16_A_SCALE;
    _Float16 h = (_Float16)xs;                                     // round to nearest even
    if (isfinite(xs) && !isfinite((float)h)) h = (_Float16)(xs > 0.f ? 65504.f : -65504.f);
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}

// Where a case's tensors sit inside wider buffers (yds_conv_run_view): channel offsets and row lengths of the input, output and
// residual views, and the second output of a merged launch.  Without one the tensors are dense.
struct CaseViews {
    int x_ld, x_off, y_ld, y_off, r_ld, r_off, n_split, y2_ld, y2_off;
};

struct ConvCase {
    ConvArgs a;
    ConvWeights cw;
    DevBuf<float> x, y, y2, res, raw[4];
    View y_whole, y2_whole;                  // the buffers a.y / a.y2 are slices of

    // host fp32 NHWC (ld = c) -> the device tensor v.p in v's format.  An F16 tensor is packed on the host: 2 bytes per channel, so its
    // row is v.c / 2 float slots (v.ld is set to that); hipMalloc aligns the pointer far beyond the 128 bytes the kernels ask for.
    static void put(View &v, const float *host, DevBuf<float> &raw, DevBuf<float> &packed) {
        if (v.fmt == FMT_F16) {
            const size_t count = v.pixels() * v.c;
            std::vector<uint16_t> h(count);
            for (size_t i = 0; i < count; ++i) h[i] = f16_bits_saturating(host[i]);
            v.ld = fmt_slots(FMT_F16, v.c);
            packed.upload(reinterpret_cast<const float *>(h.data()), count / 2);
            YDS_HIP(hipDeviceSynchronize());                           // (the host vector dies with this call)
            v.p = packed.p;
            return;
        }
        raw.upload(host, v.pixels() * v.c);
        v.p = raw.p;
        if (v.fmt != FMT_H16) return;
        packed.alloc(raw.n);
        v.p = packed.p;
        launch_pack_h16(raw.p, v, nullptr);
    }
    // channels [off, off + c) of the tensor `whole` (F16: the offset in float slots is half the channel offset)
    static View slice(const View &whole, int off, int c) {
        View v = whole;
        v.p = whole.p + fmt_slots(whole.fmt, off);
        v.c = c;
        return v;
    }
    static bool h16_ok(int c, int ld, int off) { return c % 32 == 0 && ld % 32 == 0 && off % 32 == 0; }
    // x_nhwc [n, h, w, x_ld], w_okkc [cout][ksize * ksize * cin], bias [cout], res_nhwc [n, ho, wo, r_ld] (read when res_mode): host;
    // vw == nullptr: dense tensors (x_ld = cin, r_ld = cout), the output row padded to a multiple of 4.  With views the output
    // buffers start out filled with `sentinel`.  fmt_x / fmt_y (yds_conv_run_half): 0 = the format picked here (H16 where h16_ok, else
    // fp32), FMT_F16 = 2-byte activations; the residual and the second output of a merged launch follow fmt_y.  x_nhwc == nullptr: the
    // input is described (shape, format, ld) but has no storage - the second layer of a fused launch, whose input lives in LDS only.
    ConvCase(int n, int h, int w, int cin, int cout, int ksize, int stride, int act, const float *x_nhwc, const float *w_okkc, const float *bias,
             const float *res_nhwc, int res_mode, const CaseViews *vw = nullptr, float sentinel = 0.f, int fmt_x = 0, int fmt_y = 0) {
        const int pad = (ksize - 1) / 2, ho = (h + 2 * pad - ksize) / stride + 1, wo = (w + 2 * pad - ksize) / stride + 1;
        const CaseViews d = vw ? *vw : CaseViews{cin, 0, (cout + 3) / 4 * 4, 0, cout, 0, 0, 0, 0};
        const bool f16 = conv_math() == MATH_F16X3;
        const int c1 = d.n_split > 0 ? d.n_split : cout, c2 = cout - c1;      // filters of the first / second output
        cw.shape(cout, cin, cin, ksize, stride, pad);
        cw.upload_korder(w_okkc, bias, nullptr);
        cw.fill(a);
        a.act = act;
        View x_whole{nullptr, n, h, w, d.x_ld, d.x_ld, fmt_x == FMT_F16 ? FMT_F16 : (f16 && h16_ok(cin, d.x_ld, d.x_off)) ? FMT_H16 : FMT_F32};
        const int yfmt = fmt_y == FMT_F16 ? FMT_F16 : (f16 && h16_ok(c1, d.y_ld, d.y_off) && h16_ok(c2, d.y2_ld, d.y2_off)) ? FMT_H16 : FMT_F32;
        y_whole = View{nullptr, n, ho, wo, d.y_ld, d.y_ld, yfmt};
        if (x_nhwc) put(x_whole, x_nhwc, raw[0], x);
        else x_whole.ld = fmt_slots(x_whole.fmt, d.x_ld);
        a.x = slice(x_whole, d.x_off, cin);
        if (vw) {
            const std::vector<float> fill(y_whole.pixels() * (size_t)std::max(d.y_ld, d.y2_ld), sentinel);
            put(y_whole, fill.data(), raw[2], y);
            if (c2 > 0) {
                y2_whole = View{nullptr, n, ho, wo, d.y2_ld, d.y2_ld, yfmt};
                put(y2_whole, fill.data(), raw[3], y2);
                a.y2 = slice(y2_whole, d.y2_off, c2);
                a.n_split = c1;
            }
        } else {
            y_whole.ld = fmt_slots(yfmt, d.y_ld);
            y.alloc(y_whole.pixels() * y_whole.ld);
            y_whole.p = y.p;
        }
        a.y = slice(y_whole, d.y_off, cout);                     // (merged: both filter counts, the first output's pointer and stride)
        if (res_mode) {
            // the residual is pre-split where ITS view allows it (dense tensors: wherever the output is), so a view case can pair an
            // H16 shortcut with an fp32 output and the reverse
            const int rfmt = yfmt == FMT_F16 ? FMT_F16 : (f16 && h16_ok(cout, d.r_ld, d.r_off)) ? FMT_H16 : FMT_F32;
            View r_whole{nullptr, n, ho, wo, d.r_ld, d.r_ld, rfmt};
            put(r_whole, res_nhwc, raw[1], res);
            a.res = slice(r_whole, d.r_off, cout);
            a.res_mode = res_mode;
        }
        YDS_HIP(hipDeviceSynchronize());
    }
};

}  // namespace
}  // namespace yds

extern "C" {

int yds_conv_bench(int n, int h, int w, int cin, int cout, int ksize, int stride, int act, int with_residual, int iters, double *avg_us,
                   int *variant) {
    YDS_API_BEGIN
    using namespace yds;
    std::vector<float> hx((size_t)n * h * w * cin), hw((size_t)cout * ksize * ksize * cin), hb(cout);
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((s >> 8) & 0xffff) / 32768.f - 1.f; };
    // YDS_BENCH_DATA=zero | const: power experiment (the chip is power limited: operands that do not toggle run at a higher clock)
    const char *dk = getenv("YDS_BENCH_DATA");
    const int data_kind = !dk ? 0 : (!strcmp(dk, "zero") ? 1 : (!strcmp(dk, "const") ? 2 : 0));
    for (auto &v : hx) v = data_kind == 1 ? 0.f : data_kind == 2 ? 0.5f : rnd();
    for (auto &v : hw) v = data_kind == 1 ? 0.f : data_kind == 2 ? 0.03125f : rnd() * 0.05f;
    for (auto &v : hb) v = rnd();
    const int pad = (ksize - 1) / 2;
    const std::vector<float> hr(with_residual ? (size_t)n * ((h + 2 * pad - ksize) / stride + 1) * ((w + 2 * pad - ksize) / stride + 1) * cout : 0, 0.f);
    ConvCase c(n, h, w, cin, cout, ksize, stride, act, hx.data(), hw.data(), hb.data(), hr.data(), with_residual ? RES_AFTER_ACT : RES_NONE);
    if (const char *t = getenv("YDS_BENCH_TERMS")) c.a.terms = atoi(t) == 1 ? 1 : 3;      // tuning aid: the half-mode kernels on single layers
    hipStream_t st;
    YDS_HIP(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    YDS_HIP(hipEventCreate(&e0)); YDS_HIP(hipEventCreate(&e1));
    int tuned = conv_autotune(c.a, st, nullptr);
    for (int i = 0; i < 3; ++i) *variant = launch_conv(c.a, st, tuned);
    YDS_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) launch_conv(c.a, st, tuned);
    YDS_HIP(hipEventRecord(e1, st));
    YDS_HIP(hipEventSynchronize(e1));
    float ms = 0;
    YDS_HIP(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1e3 / iters;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(st);
    YDS_API_END
}

int yds_conv_run(int variant, int n, int h, int w, int cin, int cout, int ksize, int stride, int act, int res_mode, const float *x_nhwc,
                 const float *w_okkc, const float *bias, const float *res_nhwc, float *y_nchw) {
    YDS_API_BEGIN
    using namespace yds;
    if (cin % 4) fail("conv_run: input channels must be a multiple of 4");
    if (res_mode && !res_nhwc) fail("conv_run: residual mode %d without a residual tensor", res_mode);
    ConvCase c(n, h, w, cin, cout, ksize, stride, act, x_nhwc, w_okkc, bias, res_nhwc, res_mode);
    launch_conv(c.a, nullptr, variant);
    nhwc_to_host(c.a.y, y_nchw, nullptr);
    YDS_API_END
}

int yds_conv_run_view(int variant, int n, int h, int w, int cin, int cout, int ksize, int stride, int act, int res_mode, const int *view,
                      const float *x_nhwc, const float *w_okkc, const float *bias, const float *res_nhwc, float sentinel, float *y_nchw,
                      float *y2_nchw) {
    YDS_API_BEGIN
    using namespace yds;
    const CaseViews v{view[0], view[1], view[2], view[3], view[4], view[5], view[6], view[7], view[8]};
    const bool merged = v.n_split > 0;
    const int c1 = merged ? v.n_split : cout;
    if (n < 1 || h < 1 || w < 1 || cin < 4 || cout < 1 || cin % 4) fail("conv_run_view: bad shape (input channels must be a multiple of 4)");
    if (res_mode && !res_nhwc) fail("conv_run_view: residual mode %d without a residual tensor", res_mode);
    if (merged && (v.n_split >= cout || res_mode || !y2_nchw)) fail("conv_run_view: a merged launch needs 0 < n_split < cout, a second output and no residual");
    auto inside = [](int off, int c, int ld) { return off >= 0 && c > 0 && off % 4 == 0 && ld % 4 == 0 && off + c <= ld; };
    if (!inside(v.x_off, cin, v.x_ld)) fail("conv_run_view: input slice [%d, %d) does not fit %d channels (multiples of 4)", v.x_off, v.x_off + cin, v.x_ld);
    if (!inside(v.y_off, c1, v.y_ld)) fail("conv_run_view: output slice [%d, %d) does not fit %d channels (multiples of 4)", v.y_off, v.y_off + c1, v.y_ld);
    if (merged && !inside(v.y2_off, cout - c1, v.y2_ld)) fail("conv_run_view: second output slice [%d, %d) does not fit %d channels (multiples of 4)", v.y2_off, v.y2_off + cout - c1, v.y2_ld);
    if (res_mode && !inside(v.r_off, cout, v.r_ld)) fail("conv_run_view: residual slice [%d, %d) does not fit %d channels (multiples of 4)", v.r_off, v.r_off + cout, v.r_ld);
    ConvCase c(n, h, w, cin, cout, ksize, stride, act, x_nhwc, w_okkc, bias, res_nhwc, res_mode, &v, sentinel);
    // only what the planner launches on such a layer: a timing candidate, or split-K where its rule applies
    const int id = variant & kVariantMask;
    if (variant < 0 || id >= kConvVariants) fail("conv_run_view: no such variant %d", variant);
    const std::vector<int> cand = conv_candidates(c.a);
    bool planned = std::find(cand.begin(), cand.end(), id) != cand.end();
    if (id == VAR_SPLITK_64x128 && conv_math() == MATH_F16X3 && !merged && conv_presplit_input(c.a)) {
        const ConvKernelArgs k = make_conv_args(c.a);
        planned = conv_splitk_applicable(k, 0) && conv_splitk_preferred(k);
    }
    if (!planned) fail("conv_run_view: the planner never launches %s on this layer%s", conv_variant_name(id), merged ? " (merged launch)" : "");
    launch_conv(c.a, nullptr, variant);
    nhwc_to_host(c.y_whole, y_nchw, nullptr);
    if (merged) nhwc_to_host(c.y2_whole, y2_nchw, nullptr);
    YDS_API_END
}

int yds_conv_run_half(int variant, int n, int h, int w, int cin, int cout, int ksize, int stride, int act, int res_mode, const int *view,
                      int fmt_x, int fmt_y, const float *x_nhwc, const float *w_okkc, const float *bias, const float *res_nhwc, float sentinel,
                      float *y_nchw, float *y2_nchw) {
    YDS_API_BEGIN
    using namespace yds;
    if (conv_math() != MATH_F16X3) fail("conv_run_half: half mode needs conv math f16x3");
    if ((fmt_x != 0 && fmt_x != FMT_F16) || (fmt_y != 0 && fmt_y != FMT_F16)) fail("conv_run_half: fmt_x / fmt_y are 0 (the planner's format) or %d (F16)", (int)FMT_F16);
    if (n < 1 || h < 1 || w < 1 || cin < 4 || cout < 1 || cin % 4) fail("conv_run_half: bad shape (input channels must be a multiple of 4)");
    if (res_mode && !res_nhwc) fail("conv_run_half: residual mode %d without a residual tensor", res_mode);
    const CaseViews v = view ? CaseViews{view[0], view[1], view[2], view[3], view[4], view[5], view[6], view[7], view[8]}
                             : CaseViews{cin, 0, (cout + 3) / 4 * 4, 0, cout, 0, 0, 0, 0};
    const bool merged = v.n_split > 0;
    const int c1 = merged ? v.n_split : cout;
    if (merged && (v.n_split >= cout || res_mode || !y2_nchw)) fail("conv_run_half: a merged launch needs 0 < n_split < cout, a second output and no residual");
    // slices in CHANNELS: multiples of 4, of 64 in an F16 tensor (whose rows and offsets the kernels see in float slots, half of these)
    auto inside = [](int off, int c, int ld, int g) { return off >= 0 && c > 0 && off % g == 0 && ld % g == 0 && c % g == 0 && off + c <= ld; };
    const int gx = fmt_x == FMT_F16 ? 64 : 4, gy = fmt_y == FMT_F16 ? 64 : 4;
    if (!inside(v.x_off, cin, v.x_ld, gx)) fail("conv_run_half: input slice [%d, %d) does not fit %d channels (multiples of %d)", v.x_off, v.x_off + cin, v.x_ld, gx);
    if (view || fmt_y == FMT_F16) {
        if (!inside(v.y_off, c1, v.y_ld, gy)) fail("conv_run_half: output slice [%d, %d) does not fit %d channels (multiples of %d)", v.y_off, v.y_off + c1, v.y_ld, gy);
        if (merged && !inside(v.y2_off, cout - c1, v.y2_ld, gy)) fail("conv_run_half: second output slice [%d, %d) does not fit %d channels (multiples of %d)", v.y2_off, v.y2_off + cout - c1, v.y2_ld, gy);
        if (res_mode && !inside(v.r_off, cout, v.r_ld, gy)) fail("conv_run_half: residual slice [%d, %d) does not fit %d channels (multiples of %d)", v.r_off, v.r_off + cout, v.r_ld, gy);
    }
    ConvCase c(n, h, w, cin, cout, ksize, stride, act, x_nhwc, w_okkc, bias, res_nhwc, res_mode, view ? &v : nullptr, sentinel, fmt_x, fmt_y);
    c.a.terms = 1;
    // only what the planner launches on such a half-mode layer: a timing candidate (split-K is never one, and its rule excludes half mode)
    const int id = variant & kVariantMask;
    if (variant < 0 || id >= kConvVariants) fail("conv_run_half: no such variant %d", variant);
    const std::vector<int> cand = conv_candidates(c.a);
    if (std::find(cand.begin(), cand.end(), id) == cand.end())
        fail("conv_run_half: the planner never launches %s on this layer in half mode%s", conv_variant_name(id), merged ? " (merged launch)" : "");
    launch_conv(c.a, nullptr, variant);
    nhwc_to_host(view ? c.y_whole : c.a.y, y_nchw, nullptr);
    if (merged) nhwc_to_host(c.y2_whole, y2_nchw, nullptr);
    YDS_API_END
}

int yds_conv_run_fused(int kind, int n, int h, int w, int act, int half, int fmt, const float *x_nhwc, const float *w_a, const float *bias_a,
                       const float *w_b, const float *bias_b, float *y_nchw) {
    YDS_API_BEGIN
    using namespace yds;
    if (kind < 0 || kind > 2) fail("conv_run_fused: kind is 0 (stem2), 1 (block1) or 2 (stem conv + pool), got %d", kind);
    if (n < 1 || h < 1 || w < 1) fail("conv_run_fused: bad shape %d x %d x %d", n, h, w);
    if (fmt != 0 && fmt != FMT_F16) fail("conv_run_fused: fmt is 0 (the planner's format) or %d (F16)", (int)FMT_F16);
    if (kind == 2) {
        // the ReID stem: 3x3 RGB -> 64, activation, MaxPool(3, 2, 1); the case's output buffer has the convolution's size, the kernel
        // fills the pooled tensor at its start
        if (half || fmt) fail("conv_run_fused: the stem conv + pool has no half mode and writes no F16 tensor");
        ConvCase c(n, h, w, 4, 64, 3, 1, act, x_nhwc, w_a, bias_a, nullptr, RES_NONE);
        launch_conv_pool(make_conv_args(c.a), nullptr);
        View pooled = c.a.y;
        pooled.h = (h - 1) / 2 + 1;
        pooled.w = (w - 1) / 2 + 1;
        nhwc_to_host(pooled, y_nchw, nullptr);
        return 0;
    }
    if (conv_math() != MATH_F16X3) fail("conv_run_fused: the fused stem and the fused block are f16x3 kernels (conv math f16x3 required)");
    if (!w_b || !bias_b) fail("conv_run_fused: kind %d takes two convolutions", kind);
    if (fmt == FMT_F16 && !half) fail("conv_run_fused: F16 tensors exist in half mode only");
    const int terms = half ? 1 : 3;
    if (kind == 0) {
        // layers 0 + 1 of the detector: the RGB input is fp32, fmt is the output's format
        ConvCase c0(n, h, w, 4, 32, 3, 1, act, x_nhwc, w_a, bias_a, nullptr, RES_NONE);
        ConvCase c1(n, h, w, 32, 64, 3, 2, act, nullptr, w_b, bias_b, nullptr, RES_NONE, nullptr, 0.f, 0, fmt);
        c0.a.terms = c1.a.terms = terms;
        ConvKernelArgs k0 = make_conv_args(c0.a), k1 = make_conv_args(c1.a);
        k1.w = reinterpret_cast<const float *>(c1.a.w16);
        launch_conv_stem2(k0, k1, nullptr);
        nhwc_to_host(c1.a.y, y_nchw, nullptr);
    } else {
        // the first residual block: input, shortcut and output are one format (H16, or F16 in half mode); the shortcut IS the input
        ConvCase c2(n, h, w, 64, 32, 1, 1, act, x_nhwc, w_a, bias_a, nullptr, RES_NONE, nullptr, 0.f, fmt, 0);
        ConvCase c3(n, h, w, 32, 64, 3, 1, act, nullptr, w_b, bias_b, nullptr, RES_NONE, nullptr, 0.f, 0, fmt);
        c3.a.res = c2.a.x;
        c3.a.res_mode = RES_AFTER_ACT;
        c2.a.terms = c3.a.terms = terms;
        ConvKernelArgs k2 = make_conv_args(c2.a), k3 = make_conv_args(c3.a);
        k2.w = reinterpret_cast<const float *>(c2.a.w16);
        k3.w = reinterpret_cast<const float *>(c3.a.w16);
        launch_conv_block1(k2, k3, nullptr);
        nhwc_to_host(c3.a.y, y_nchw, nullptr);
    }
    YDS_API_END
}

}  // extern "C"
