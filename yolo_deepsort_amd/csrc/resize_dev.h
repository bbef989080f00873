// Bilinear resize of 8-bit images, one output pixel at a time - the device text shared by every kernel that resizes (layers.hip: the
// detector and window front ends and the crop kernel; reid_stem.hip: the fused ReID front end).  One text, so that all of them produce
// the same integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yds {

// cv2.resize(INTER_LINEAR) on 8-bit images, bit for bit (OpenCV modules/imgproc/src/resize.cpp; spec and citations in
// oracle/resize.py): sample position in double, one rounding to float, 11-bit fixed-point weights (round half to even),
// integer horizontal pass, vertical pass (((b0*(h0>>4))>>16) + ((b1*(h1>>4))>>16) + 2) >> 2; exact 2x down-scaling takes
// INTER_AREA's (a+b+c+d+2)>>2, equal sizes copy.
struct Tap { int i0, i1, a0, a1; };
__device__ __forceinline__ double cv_scale(int dst, int src) { return __ddiv_rn(1.0, __ddiv_rn((double)dst, (double)src)); }
template <bool X_AXIS> __device__ __forceinline__ Tap axis_tap(int d, double scale, int src) {
    float f = __double2float_rn(__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5));
    const float fl = floorf(f);
    int s = (int)fl;
    f = __fsub_rn(f, fl);
    if (X_AXIS) {                                               // the x axis zeroes the weight when it clamps ...
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
    }
    Tap t;
    t.a0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
    t.a1 = (int)rintf(__fmul_rn(f, 2048.f));
    t.i0 = min(max(s, 0), src - 1);                             // ... the y axis clips the two row indices and keeps its weights
    t.i1 = min(max(s + 1, 0), src - 1);
    return t;
}
enum { RESIZE_LINEAR = 0, RESIZE_AREA2 = 1, RESIZE_COPY = 2 };
__device__ __forceinline__ int resize_mode(int src_h, int src_w, int dst_h, int dst_w) {
    if (src_h == dst_h && src_w == dst_w) return RESIZE_COPY;
    if (src_h == 2 * dst_h && src_w == 2 * dst_w) return RESIZE_AREA2;
    return RESIZE_LINEAR;
}
// one output pixel (3 channels) of the region whose top-left source pixel is `base` (row stride `row_bytes`)
__device__ __forceinline__ void resize_px(const uint8_t *base, size_t row_bytes, int src_h, int src_w, int dst_h, int dst_w, int oy, int ox,
                                          float o[3]) {
    const int mode = resize_mode(src_h, src_w, dst_h, dst_w);
    if (mode == RESIZE_COPY) {
        const uint8_t *p = base + (size_t)oy * row_bytes + ox * 3;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        return;
    }
    if (mode == RESIZE_AREA2) {
        const uint8_t *p = base + (size_t)(2 * oy) * row_bytes + 2 * ox * 3, *q = p + row_bytes;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (float)(((int)p[c] + (int)p[3 + c] + (int)q[c] + (int)q[3 + c] + 2) >> 2);
        return;
    }
    const Tap tx = axis_tap<true>(ox, cv_scale(dst_w, src_w), src_w), ty = axis_tap<false>(oy, cv_scale(dst_h, src_h), src_h);
    const uint8_t *r0 = base + (size_t)ty.i0 * row_bytes, *r1 = base + (size_t)ty.i1 * row_bytes;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int h0 = (int)r0[tx.i0 * 3 + c] * tx.a0 + (int)r0[tx.i1 * 3 + c] * tx.a1;
        const int h1 = (int)r1[tx.i0 * 3 + c] * tx.a0 + (int)r1[tx.i1 * 3 + c] * tx.a1;
        o[c] = (float)(((((ty.a0 * (h0 >> 4)) >> 16) + ((ty.a1 * (h1 >> 4)) >> 16) + 2) >> 2) & 0xff);
    }
}

}  // namespace yds
