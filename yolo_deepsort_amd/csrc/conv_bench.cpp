// Single convolutions through the C ABI: yds_conv_bench times one layer shape on synthetic data, yds_conv_run runs one tile variant
// on the caller's tensors (the kernel tests).  Both build the same case - input and residual (pre-split where the kernels take them
// that way), weights, output - and differ in what they do with the launch.
#include "conv_weights.h"
#include "h16.h"

#include <stdlib.h>
#include <string.h>

namespace yds {
namespace {

struct ConvCase {
    ConvArgs a;
    ConvWeights cw;
    DevBuf<float> x, y, res, raw[2];

    // host fp32 NHWC (ld = c) -> the device tensor v.p in v's format
    static void put(View &v, const float *host, DevBuf<float> &raw, DevBuf<float> &packed) {
        raw.upload(host, v.pixels() * v.c);
        v.p = raw.p;
        if (v.fmt != FMT_H16) return;
        packed.alloc(raw.n);
        v.p = packed.p;
        launch_pack_h16(raw.p, v, nullptr);
    }
    // x_nhwc [n, h, w, cin], w_okkc [cout][ksize * ksize * cin], bias [cout], res_nhwc [n, ho, wo, cout] (read when res_mode): host
    ConvCase(int n, int h, int w, int cin, int cout, int ksize, int stride, int act, const float *x_nhwc, const float *w_okkc, const float *bias,
             const float *res_nhwc, int res_mode) {
        const int pad = (ksize - 1) / 2, ho = (h + 2 * pad - ksize) / stride + 1, wo = (w + 2 * pad - ksize) / stride + 1, ldy = (cout + 3) / 4 * 4;
        const bool f16 = conv_math() == MATH_F16X3;
        cw.shape(cout, cin, cin, ksize, stride, pad);
        cw.upload_korder(w_okkc, bias, nullptr);
        cw.fill(a);
        a.act = act;
        y.alloc((size_t)n * ho * wo * ldy);
        a.x = View{nullptr, n, h, w, cin, cin, (f16 && cin % 32 == 0) ? FMT_H16 : FMT_F32};
        a.y = View{y.p, n, ho, wo, cout, ldy, (f16 && cout % 32 == 0) ? FMT_H16 : FMT_F32};
        put(a.x, x_nhwc, raw[0], x);
        if (res_mode) {
            a.res = View{nullptr, n, ho, wo, cout, cout, a.y.fmt};
            put(a.res, res_nhwc, raw[1], res);
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

}  // extern "C"
