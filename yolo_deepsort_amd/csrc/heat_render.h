// What the renders of a grid of int64 cells share (heatmap.hip: a stream's layer into its frames; ground.hip: a site layer onto a plan
// canvas and onto the floor of camera frames): the job of the levels kernel, the byte blend, a thread's whole-pixel accesses, and the
// launch front of heat_levels_kernel / heat_render_kernel, which takes any layer pointer - a site grid is a heat grid.
#pragma once
#include "common.h"

#include <stdint.h>

namespace yds {

// one grid named in a render call (or asked for its maximum: level == nullptr)
struct HeatLevelJob {
    const long long *layer;                       // [gh * gw]
    uint16_t *level;                              // [gh * gw]
    long long vmax;                               // 0: the layer's maximum, 1 when nothing is positive
    int n, gw, gh, lc;                            // cells; lc = log2(cell)
};

struct HeatRenderArgs {
    uint8_t *frames;
    size_t frame_bytes;
    const int2 *fjobs;                            // per frame of the call: (slot, job)
    const HeatLevelJob *jobs;
    const uint32_t *lut;                          // [256] byte 0 | byte 1 << 8 | byte 2 << 16
    const int *bad;
    int h, w;
    uint32_t alpha;
};

// The launch front (heatmap.hip), asynchronous on s.  levels: a workgroup per job; res[job] = the layer's maximum, *bad = 1 when the
// vmax to use exceeds the limit (the caller zeroes *bad first).  render: n frames of a.h x a.w, the pixels per thread chosen by the
// base address and the width; refuses frames too large for one launch.
void heat_launch_levels(const HeatLevelJob *jobs_dev, int n_jobs, long long *res, int *bad, hipStream_t s);
void heat_launch_render(const HeatRenderArgs &a, int n, hipStream_t s);
// pixels of a row a thread owns for frames at `base` of width w: 16 (uint4 accesses), 4 (dwords) or 1 (bytes)
inline int heat_px_per_thread(const void *base, int w) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(base);
    return b % 16 == 0 && w % 16 == 0 ? 16 : b % 4 == 0 && w % 4 == 0 ? 4 : 1;
}
// the LUT as the kernels read it
inline void heat_pack_lut(uint32_t *lut32, const uint8_t *lut) {
    for (int k = 0; k < 256; ++k) lut32[k] = (uint32_t)lut[3 * k] | (uint32_t)lut[3 * k + 1] << 8 | (uint32_t)lut[3 * k + 2] << 16;
}

#ifdef __HIPCC__
// two bytes per multiply: the even bytes of s and l in the low halves of two 16-bit lanes (a * l + na * s + 128 <= 65408: no carry
// between the lanes), the odd bytes likewise after a shift
__device__ __forceinline__ uint32_t heat_blend(uint32_t s, uint32_t l, uint32_t a, uint32_t na) {
    const uint32_t M = 0x00ff00ffu, C = 0x00800080u;
    const uint32_t e = (s & M) * na + (l & M) * a + C;
    const uint32_t o = ((s >> 8) & M) * na + ((l >> 8) & M) * a + C;
    return ((e >> 8) & M) | (o & ~M);
}

// words a thread holds for its PX pixels
template <int PX> struct HeatWords { static constexpr int N = PX >= 4 ? PX * 3 / 4 : 1; };

// PX whole pixels at p into word[]: three 16-byte accesses, three dwords, or three bytes
template <int PX> __device__ __forceinline__ void heat_load_px(const uint8_t *p, uint32_t *word) {
    if constexpr (PX == 16) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) { const uint4 v = q[i]; word[4 * i] = v.x; word[4 * i + 1] = v.y; word[4 * i + 2] = v.z; word[4 * i + 3] = v.w; }
    } else if constexpr (PX == 4) {
        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) word[i] = q[i];
    } else {
        word[0] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    }
}

// col[i]: the LUT colour of pixel i with bits 24..31 set where the pixel takes part, 0 where it keeps the picture; blends and writes
// the PX pixels back
template <int PX> __device__ __forceinline__ void heat_blend_store_px(uint8_t *p, uint32_t *word, const uint32_t *col, uint32_t al, uint32_t na) {
    if constexpr (PX >= 4) {
#pragma unroll
        for (int g = 0; g < PX / 4; ++g) {                                        // pixels c d e f = bytes c0 c1 c2 d0 | d1 d2 e0 e1 | e2 f0 f1 f2
            const uint32_t l0 = col[4 * g], l1 = col[4 * g + 1], l2 = col[4 * g + 2], l3 = col[4 * g + 3];
            const uint32_t m0 = (uint32_t)((int32_t)l0 >> 31), m1 = (uint32_t)((int32_t)l1 >> 31), m2 = (uint32_t)((int32_t)l2 >> 31),
                           m3 = (uint32_t)((int32_t)l3 >> 31);
            const uint32_t lw[3] = {(l0 & 0xffffffu) | l1 << 24, ((l1 >> 8) & 0xffffu) | l2 << 16, ((l2 >> 16) & 0xffu) | l3 << 8};
            const uint32_t mw[3] = {(m0 & 0xffffffu) | (m1 & 0xff000000u), (m1 & 0xffffu) | (m2 & 0xffff0000u), (m2 & 0xffu) | (m3 & 0xffffff00u)};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const uint32_t s = word[3 * g + i];
                word[3 * g + i] = (heat_blend(s, lw[i], al, na) & mw[i]) | (s & ~mw[i]);
            }
        }
        if constexpr (PX == 16) {
            uint4 *q = reinterpret_cast<uint4 *>(p);
#pragma unroll
            for (int i = 0; i < 3; ++i) q[i] = make_uint4(word[4 * i], word[4 * i + 1], word[4 * i + 2], word[4 * i + 3]);
        } else {
            uint32_t *q = reinterpret_cast<uint32_t *>(p);
#pragma unroll
            for (int i = 0; i < 3; ++i) q[i] = word[i];
        }
    } else {
        const uint32_t v = heat_blend(word[0], col[0], al, na);
        p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16);
    }
}
#endif

}  // namespace yds
