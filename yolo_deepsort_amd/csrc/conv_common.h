// Pieces shared by the implicit-GEMM convolution kernels (conv.hip: fp32 MFMA, conv_f16x3.hip: split-fp16 MFMA).
#pragma once
#include "common.h"
#include "h16.h"

#include <algorithm>
#include <stdlib.h>
#include <type_traits>

namespace yds {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// split-fp16 ("f16x3") operand encoding shared by conv_f16x3.hip and conv_win.hip:
//   x * A_SCALE = hi + lo / LO_SCALE,  w = hi + lo / LO_SCALE   (hi, lo fp16; see conv_f16x3.hip)
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
constexpr float A_SCALE = 1.f / 256.f, LO_SCALE = 2048.f;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

struct ConvKernelArgs {
    const float *x, *w, *bias, *res;
    float *y;
    int H, W, Cin, ldx;
    int Ho, Wo, Cout, ldy, ldr;
    int ksize, stride, pad;
    int K, Kpad, M;
    int act, res_mode;
    int fmt_x, fmt_y, fmt_r;              // TensorFmt of input, output and residual views
    int terms;                            // 3: f16x3, 1: hi halves only (half mode; LDS-DMA and window kernels)
    int ksplit = 1;                       // LDS-DMA kernel: K ranges (grid.y); > 1 writes raw partial sums into slab blockIdx.y of y
    // two convolutions of the same input in one launch (CSP split, darknet.cpp): filters [n_split, Cout) write to y2
    float *y2 = nullptr;
    int ldy2 = 0, n_split = 0;
    // XCD-aware tile map: the 8 XCDs own an xm x xn grid of rectangles of rm x rn tiles (workgroup id % 8 = XCD)
    int tiles_m, tiles_n, xm, rm, rn;
    int gn = 1;                           // filter tiles walked together inside an XCD's rectangle (tile_of_block); set by plan_tile_map
    int gn_req = 0;                       // ... as requested by the caller (ConvArgs::tile_gn: 0 / 1 = column by column)
};

constexpr int KALIGN = 32;                // weight rows are zero padded to a multiple of this
constexpr int STAGGER = 24;              // s_sleep units of 64 clocks: start offset of every other resident workgroup (staged kernels)

template <int ACT> __device__ __forceinline__ float apply_act(float v) {
    if (ACT == ACT_LEAKY) return v > 0.f ? v : v * 0.1f;
    if (ACT == ACT_RELU) return v > 0.f ? v : 0.f;
    if (ACT == ACT_MISH) {
        // x * tanh(softplus(x)) with ONE exponential:  tanh(log(1+e)) = ((1+e)^2 - 1) / ((1+e)^2 + 1) = n / (n + 2),
        // n = e*(e+2), e = exp(x).  Same threshold as torch's softplus (x > 20 -> softplus(x) = x, tanh = 1).
        // Raw hardware exp2 / reciprocal (v_exp_f32, v_rcp_f32: ~1 ulp each), branch free: the result stays within ~3e-7
        // relative of the exact value.  (Round 3: `__frcp_rn` had been expanding to the IEEE division sequence - div_scale,
        // four fmas, div_fmas, div_fixup - behind an exec-mask branch: ten instructions per value, which made the Mish layers of
        // yolov4 VALU bound in their epilogues: 304x304 64->64 181 us against 149 us with a linear epilogue.)
        const float e = __builtin_amdgcn_exp2f(fminf(v, 20.f) * 1.44269504088896341f);
        const float n = e * (e + 2.f);
        const float m = v * (n * __builtin_amdgcn_rcpf(n + 2.f));
        return v > 20.f ? v : m;
    }
    return v;
}

// Workgroup -> tile map.  The dispatcher places workgroup b on XCD b % 8 and every XCD has a private 4 MiB L2,
// so each XCD gets a compact rm x rn rectangle of tiles (small A-rows + B-columns footprint per K step) instead
// of a stripe through the whole problem.  Placement only affects speed, never results.
// Order INSIDE an XCD's rectangle (round 6): the ~32 workgroups an XCD runs at a time are consecutive ids.  gn = 1 walks the
// rectangle column by column (32 different pixel tiles against ONE filter tile at a time); gn > 1 walks it in groups of gn filter
// tiles, filter tile fastest, so that the gn workgroups of one pixel tile run together and share its input window through the L2.
__device__ __forceinline__ bool tile_of_block(const ConvKernelArgs &p, int &tm, int &tn) {
    const int b = blockIdx.x, xcd = b & 7, idx = b >> 3;
    int lm, ln;
    if (p.gn <= 1) {
        lm = idx % p.rm;
        ln = idx / p.rm;
    } else {
        const int per = p.rm * p.gn, grp = idx / per, w = idx - grp * per;
        const int g = min(p.gn, p.rn - grp * p.gn);              // the last group of columns may be narrower
        lm = w / g;
        ln = grp * p.gn + (w - lm * g);
    }
    tm = (xcd % p.xm) * p.rm + lm;
    tn = (xcd / p.xm) * p.rn + ln;
    return tm < p.tiles_m && tn < p.tiles_n;
}

// host: choose the XCD grid (xm x xn = 8) with the smallest per-K-step footprint (rows*BM + cols*BN) per XCD;
// returns the grid size in workgroups
inline int plan_tile_map(ConvKernelArgs &k, int BM, int BN) {
    k.tiles_m = (k.M + BM - 1) / BM;
    k.tiles_n = (k.Cout + BN - 1) / BN;
    long best = -1;
    for (int xm = 1; xm <= 8; xm *= 2) {
        int xn = 8 / xm;
        int rm = (k.tiles_m + xm - 1) / xm, rn = (k.tiles_n + xn - 1) / xn;
        long waste = (long)rm * rn * 8 - (long)k.tiles_m * k.tiles_n;       // idle workgroup slots
        long cost = ((long)rm * BM + (long)rn * BN) * 64 + waste * (BM + BN);
        if (best < 0 || cost < best) { best = cost; k.xm = xm; k.rm = rm; k.rn = rn; }
    }
    k.gn = std::max(1, std::min(k.gn_req, k.rn));                 // measured per layer by conv_autotune (results do not depend on it)
    return 8 * k.rm * k.rn;
}

// Epilogue over 32x32 MFMA accumulator fragments (C/D layout: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)).
// The tile is transposed through LDS (the main loop's buffers are free by now) so that global traffic is 16-byte
// and row contiguous: bias, residual and output move as float4 along the channel axis.  One pass per row of waves
// keeps the staging area at (BM/WM) x (BN+4) floats, which fits inside every variant's main-loop allocation.
// ACT / RES are compile-time.
// RowMap: tile row -> flat output pixel index (or < 0 for "no such pixel"); FlatRows = consecutive pixels from m0
struct FlatRows {
    int m0;
    __device__ __forceinline__ int operator()(int row) const { return m0 + row; }
};
// The f16x3 accumulators come out of the K loop as o * 2^-8 (A_SCALE), and H16 tensors store x * 2^-8.  Linear, LeakyReLU and ReLU
// commute with a positive scale, so the kernels that opt in (FAST) hand over acc1 + acc2 / LO_SCALE as it is and the epilogue works
// on scaled values throughout: bias * 2^-8 once per thread, an H16 residual decoded without the unscale, the activation, then
// h16_encode4_scaled - or one multiply by 2^8 in front of an fp32 store.  Every dropped operation is a multiplication by a power of
// two, exact unless the scaled value is an fp32 subnormal, so the stored bits are those of the unscaled sequence (NaN, -0 and inf
// included; tests/test_conv_epilogue_host.py replays both sequences).  Mish is not homogeneous: its values arrive unscaled.
constexpr bool conv_epilogue_scaled(bool fast, int act) { return fast && act != ACT_MISH; }
// the activation on a value in the domain SC names; max(o, 0.1 o) is LeakyReLU's select in two instructions (same bits: both forms
// return o * 0.1 for o <= -0 and NaN, o above)
template <int ACT, bool SC> __device__ __forceinline__ float conv_epilogue_act(float o) {
    if (SC && ACT == ACT_LEAKY) return fmaxf(o, o * 0.1f);
    return apply_act<ACT>(o);                                      // ReLU and linear are the same function of a scaled value
}

// Sweep of a FULL tile (every row below M, every filter below Cout, all of them bound for one output; flat row map, whole-tile
// staging): no per-row predicate, no channel tail, no merged-launch test.  Addresses are one 64-bit base per tensor, uniform over the
// workgroup, plus a 32-bit byte offset per thread that advances by a constant per row step (a tile spans at most BM x ld x 4 bytes).
// A thread of an H16 output owns EIGHT consecutive channels of a pixel: two 16-byte LDS reads, one 16-byte store of the hi halves
// and one of the lo halves (the ragged sweep owns four and trades halves with its neighbour lane).  fp32 outputs keep four.
// (Bank check of the 8-channel read, ds_read_b128 lane groups of MI355X: threads sit 32 bytes apart in a row and rows BN * 4 + 16
// bytes apart; at BN = 128 the 16 lanes of a group fall on 16 distinct 16-byte slots, at BN = 64 two slots of a group are hit twice, at
// BN = 256 - one row per 32 lanes - every slot: two-way.  On paper; the <128,256> tile gained like the others.)
template <int BM, int BN, int WM, int WN, int ACT, int RES, int NT, bool SC, class Store>
__device__ __forceinline__ void conv_epilogue_full(const ConvKernelArgs &p, Store store, float *stage, int m0, int n0, int tid) {
    constexpr int ROWS = BM / WM, LD = BN + 4;
    const int wm = (tid >> 6) / WN;
    const bool second = p.n_split > 0 && n0 >= p.n_split;          // uniform: the tile lies on one side of the boundary
    const int y_ld = second ? p.ldy2 : p.ldy, ny0 = second ? n0 - p.n_split : n0;
    char *const y_tile = reinterpret_cast<char *>((second ? p.y2 : p.y) + (size_t)m0 * y_ld);
    const char *const r_tile = RES != RES_NONE ? reinterpret_cast<const char *>(p.res + (size_t)m0 * p.ldr) : nullptr;
    auto sweep = [&](auto yh_c, auto rh_c) {
        constexpr bool YH = decltype(yh_c)::value, RH = decltype(rh_c)::value;         // H16 (or fp32) output / residual
        constexpr int CH = YH ? 8 : 4, Q = CH / 4;                  // channels per thread, in quads
        constexpr int CT = BN / CH, RSTEP = NT / CT, NIT = BM / RSTEP;                 // threads per row, rows per sweep of the workgroup, sweeps
        static_assert(NT % CT == 0 && BM % RSTEP == 0, "tile width must divide the workgroup");
        const int c = tid % CT, rr = tid / CT;
        const int n = n0 + c * CH, ny = ny0 + c * CH;
        // byte offset of channel ch (a multiple of CH) in a pixel: H16 keeps [32 hi | 32 lo] halves per group of 32 channels
        auto chan_off = [](bool h16, int ch) { return h16 ? (unsigned)(ch & ~31) * 4u + (unsigned)(ch & 31) * 2u : (unsigned)ch * 4u; };
        const unsigned y_off = (unsigned)(rr * y_ld) * 4u + chan_off(YH, ny), y_step = (unsigned)(RSTEP * y_ld) * 4u;
        float bias[CH];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 b = *reinterpret_cast<const float4 *>(p.bias + n + q * 4);
            bias[q * 4] = b.x; bias[q * 4 + 1] = b.y; bias[q * 4 + 2] = b.z; bias[q * 4 + 3] = b.w;
        }
        if (SC) {
#pragma unroll
            for (int k = 0; k < CH; ++k) bias[k] *= A_SCALE;
        }
        // the residual rows of all sweeps are fetched up front (in flight while the tile goes through LDS); per row and thread
        // H16: CH hi halves then CH lo halves, fp32: CH floats - Q float4 either way
        union ResRow { float4 f[Q]; float2 d[2 * Q]; _Float16 h[2 * CH]; float v[CH]; };
        ResRow rraw[RES != RES_NONE ? NIT : 1];
        if (RES != RES_NONE) {
            const unsigned r_off = (unsigned)(rr * p.ldr) * 4u + chan_off(RH, n), r_step = (unsigned)(RSTEP * p.ldr) * 4u;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const char *g = r_tile + (r_off + (unsigned)it * r_step);
                if (RH && CH == 8) {
                    rraw[it].f[0] = *reinterpret_cast<const float4 *>(g);
                    rraw[it].f[Q - 1] = *reinterpret_cast<const float4 *>(g + 64);
                } else if (RH) {
                    rraw[it].d[0] = *reinterpret_cast<const float2 *>(g);
                    rraw[it].d[1] = *reinterpret_cast<const float2 *>(g + 64);
                } else {
#pragma unroll
                    for (int q = 0; q < Q; ++q) rraw[it].f[q] = *reinterpret_cast<const float4 *>(g + q * 16);
                }
            }
        }
        store(stage + wm * ROWS * LD);
        __syncthreads();
        const float *st = stage + rr * LD + c * CH;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            float o[CH];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float4 v = *reinterpret_cast<const float4 *>(st + it * RSTEP * LD + q * 4);
                o[q * 4] = v.x + bias[q * 4]; o[q * 4 + 1] = v.y + bias[q * 4 + 1]; o[q * 4 + 2] = v.z + bias[q * 4 + 2]; o[q * 4 + 3] = v.w + bias[q * 4 + 3];
            }
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                float rs = 0.f;
                if (RES != RES_NONE) {
                    const ResRow &t = rraw[RES != RES_NONE ? it : 0];
                    if (RH) {
                        rs = (float)t.h[k] + (float)t.h[CH + k] * (1.f / H16_LO_SCALE);
                        if (!SC) rs *= 1.f / H16_A_SCALE;
                    } else rs = SC ? t.v[k] * A_SCALE : t.v[k];
                }
                if (RES == RES_BEFORE_ACT) o[k] += rs;
                o[k] = conv_epilogue_act<ACT, SC>(o[k]);
                if (RES == RES_AFTER_ACT) o[k] += rs;
            }
            char *g = y_tile + (y_off + (unsigned)it * y_step);
            if (YH) {
                union { h16x4 h[2]; float4 f; } hi, lo;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if (SC) h16_encode4_scaled(o + q * 4, hi.h[q], lo.h[q]);
                    else h16_encode4(o + q * 4, hi.h[q], lo.h[q]);
                }
                *reinterpret_cast<float4 *>(g) = hi.f;
                *reinterpret_cast<float4 *>(g + 64) = lo.f;
            } else {
                if (SC) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] *= 1.f / A_SCALE;
                }
                *reinterpret_cast<float4 *>(g) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
    };
    // (an FMT_F16 output is a half-mode tensor: those kernels do not take this path)
    const bool yh = p.fmt_y == FMT_H16, rh = RES != RES_NONE && p.fmt_r == FMT_H16;
    if (yh) {
        if (rh) sweep(std::true_type{}, std::true_type{});
        else sweep(std::true_type{}, std::false_type{});
    } else {
        if (rh) sweep(std::false_type{}, std::true_type{});
        else sweep(std::false_type{}, std::false_type{});
    }
}

// ONE_PASS: the staging area holds the WHOLE tile (BM x (BN+4) floats instead of one row of waves): every wave stores its
// accumulators at once and the workgroup sweeps all rows after a single barrier (2 barriers instead of 2 x WM, no waves
// idling while one wave row is staged).  The caller sizes the LDS for it (conv_stage_bytes).
// Store: callable (float *st) that writes THIS wave's accumulator tile into its band of the staging area (row r, column c of
// the band at st[r * (BN + 4) + c]) - the only part that depends on the MFMA shape's C/D layout.
template <int BM, int BN, int WM, int WN, int ACT, int RES, int NT, class RowMap, bool ONE_PASS, bool FAST, class Store>
__device__ __forceinline__ void conv_epilogue_core(const ConvKernelArgs &p, Store store, float *stage, RowMap rows, int n0, int tid) {
    constexpr int ROWS = BM / WM, LD = BN + 4, C4 = BN / 4;        // staged rows, padded row length, float4 per row
    constexpr bool SC = conv_epilogue_scaled(FAST, ACT);           // the staged values are o * 2^-8 (see conv_epilogue_scaled)
    if constexpr (FAST) {
        // full tiles of a flat row map whose filters all go to one output take the sweep without predicates; ragged tiles and a
        // merged launch whose boundary falls inside the tile stay here.  Every operand of the test is uniform: one scalar branch.
        static_assert(ONE_PASS && std::is_same<RowMap, FlatRows>::value, "the full-tile sweep reads a whole staged tile of consecutive pixels");
        const int m0 = rows(0);
        const bool split_inside = p.n_split > n0 && p.n_split < n0 + BN;
        if (m0 + BM <= p.M && n0 + BN <= p.Cout && !split_inside && p.fmt_y != FMT_F16) {
            conv_epilogue_full<BM, BN, WM, WN, ACT, RES, NT, SC>(p, store, stage, m0, n0, tid);
            return;
        }
    }
    constexpr int RSTEP = NT / C4;                                   // rows covered by one sweep of the NT threads
    static_assert(NT % C4 == 0 && C4 % 2 == 0 && ROWS % RSTEP == 0, "tile width must divide the workgroup; lane pairs share a row");
    const int wave = tid >> 6, wm = wave / WN;
    const int c4 = tid % C4, rr = tid / C4;
    const int n = n0 + c4 * 4;
    const bool n_vec = n + 3 < p.Cout;
    // output destination of this thread's four channels (merged launches: the second convolution's filters go to y2)
    const bool second = p.n_split > 0 && n >= p.n_split;
    float *const y_base = second ? p.y2 : p.y;
    const int y_ld = second ? p.ldy2 : p.ldy, ny = second ? n - p.n_split : n;
    float4 bias4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n_vec) bias4 = *reinterpret_cast<const float4 *>(p.bias + n);
    else {
        if (n < p.Cout) bias4.x = p.bias[n];
        if (n + 1 < p.Cout) bias4.y = p.bias[n + 1];
        if (n + 2 < p.Cout) bias4.z = p.bias[n + 2];
    }
    if (SC) { bias4.x *= A_SCALE; bias4.y *= A_SCALE; bias4.z *= A_SCALE; bias4.w *= A_SCALE; }
    // The tensor formats are uniform run-time flags; the sweep is instantiated per (output H16?, residual H16?) and entered
    // through ONE uniform branch, so its loops carry no format tests (the generic form spent a third of its instructions on
    // exec-mask bookkeeping and re-tested the formats in every iteration).
    constexpr int PER_PASS = ROWS / RSTEP, NRES = RES != RES_NONE ? WM * PER_PASS : 1;
    auto sweep = [&](auto yf_c, auto rf_c) {
        constexpr int YF = decltype(yf_c)::value, RF = decltype(rf_c)::value;          // TensorFmt of the output / the residual
        constexpr bool YH = YF == FMT_H16, RH = RF == FMT_H16, YS = YF == FMT_F16, RS = RF == FMT_F16;
        // The residual rows of ALL passes are fetched up front: the loads are in flight while the tile goes through LDS,
        // instead of paying one exposed global-load latency per pass.
        float4 rraw[NRES];
        if (RES != RES_NONE) {
#pragma unroll
            for (int q = 0; q < NRES; ++q) {
                const int m = rows((q / PER_PASS) * ROWS + rr + (q % PER_PASS) * RSTEP);
                rraw[q] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (m >= 0 && m < p.M && n < p.Cout) {
                    const float *rp = p.res + (size_t)m * p.ldr;
                    if (RH) {                                                      // H16 tensors have Cout % 32 == 0: [hi 8 B | lo 8 B]
                        const char *g = reinterpret_cast<const char *>(rp + (n & ~31)) + (n & 31) * 2;
                        const float2 hi = *reinterpret_cast<const float2 *>(g), lo = *reinterpret_cast<const float2 *>(g + 64);
                        rraw[q] = make_float4(hi.x, hi.y, lo.x, lo.y);
                    } else if (RS) {                                               // FMT_F16: four channels = 8 bytes, ldr in float slots
                        const float2 h = *reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(rp) + n * 2);
                        rraw[q] = make_float4(h.x, h.y, 0.f, 0.f);
                    } else if (n_vec) {
                        rraw[q] = *reinterpret_cast<const float4 *>(rp + n);
                    } else {
                        rraw[q].x = rp[n];
                        if (n + 1 < p.Cout) rraw[q].y = rp[n + 1];
                        if (n + 2 < p.Cout) rraw[q].z = rp[n + 2];
                    }
                }
            }
        }
#pragma unroll
        for (int pass = 0; pass < WM; ++pass) {
            if (ONE_PASS ? pass == 0 : wm == pass) store(stage + (ONE_PASS ? wm * ROWS * LD : 0));
            if (!ONE_PASS || pass == 0) __syncthreads();
#pragma unroll
            for (int k2 = 0; k2 < PER_PASS; ++k2) {
                const int r = rr + k2 * RSTEP;
                const int m = rows(pass * ROWS + r);
                const bool live = m >= 0 && m < p.M && n < p.Cout;   // no early exit: lane pairs trade halves below
                float4 v = *reinterpret_cast<const float4 *>(stage + (ONE_PASS ? pass * ROWS * LD : 0) + r * LD + c4 * 4);
                float rs[4] = {0.f, 0.f, 0.f, 0.f};
                if (RES != RES_NONE) {
                    const float4 t = rraw[RES != RES_NONE ? pass * PER_PASS + k2 : 0];     // zeros where the row is not live
                    if (RH) {
                        union { float2 f; h16x4 h; } uh, ul;
                        uh.f = make_float2(t.x, t.y);
                        ul.f = make_float2(t.z, t.w);
                        if (SC) h16_decode4_scaled(uh.h, ul.h, rs);
                        else h16_decode4(uh.h, ul.h, rs);
                    } else if (RS) {
                        union { float2 f; h16x4 h; } uh;
                        uh.f = make_float2(t.x, t.y);
#pragma unroll
                        for (int k = 0; k < 4; ++k) rs[k] = SC ? (float)uh.h[k] : (float)uh.h[k] * (1.f / H16_A_SCALE);
                    } else {
                        rs[0] = t.x; rs[1] = t.y; rs[2] = t.z; rs[3] = t.w;
                        if (SC) { rs[0] *= A_SCALE; rs[1] *= A_SCALE; rs[2] *= A_SCALE; rs[3] *= A_SCALE; }
                    }
                }
                float o[4] = {v.x + bias4.x, v.y + bias4.y, v.z + bias4.z, v.w + bias4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (RES == RES_BEFORE_ACT) o[k] += rs[k];
                    o[k] = conv_epilogue_act<ACT, SC>(o[k]);
                    if (RES == RES_AFTER_ACT) o[k] += rs[k];
                }
                float *yp = y_base + (size_t)m * y_ld;
                if (YH) {
                    // neighbouring lanes hold neighbouring channel quads of the same pixel: they trade halves so that each lane
                    // issues ONE 16-byte store (even lane: 8 hi halves, odd lane: 8 lo halves) instead of two 8-byte ones.
                    // The trade is a DPP quad permute [1,0,3,2] on the vector ALU (__shfl_xor goes through the LDS crossbar).
                    h16x4 hi, lo;
                    if (SC) h16_encode4_scaled(o, hi, lo);
                    else h16_encode4(o, hi, lo);
                    const bool odd = c4 & 1;
                    union { h16x4 h; int i[2]; } send, recv;
                    send.h = odd ? hi : lo;
                    recv.i[0] = __builtin_amdgcn_update_dpp(send.i[0], send.i[0], 0xB1, 0xF, 0xF, false);
                    recv.i[1] = __builtin_amdgcn_update_dpp(send.i[1], send.i[1], 0xB1, 0xF, 0xF, false);
                    union { h16x4 h[2]; float4 f; } out;
                    out.h[0] = odd ? recv.h : hi;
                    out.h[1] = odd ? lo : recv.h;
                    const int nq = ny & ~7;                                         // first channel of the lane pair
                    char *g = reinterpret_cast<char *>(yp + (nq & ~31)) + (nq & 31) * 2 + (odd ? 64 : 0);
                    if (live) *reinterpret_cast<float4 *>(g) = out.f;
                } else if (YS) {
                    // FMT_F16: the even lane of a pair stores both lanes' channel quads, 8 consecutive fp16 = one 16-byte store
                    union { h16x4 h; int i[2]; } mine, other;
#pragma unroll
                    for (int k = 0; k < 4; ++k) mine.h[k] = SC ? (_Float16)o[k] : (_Float16)(o[k] * H16_A_SCALE);
                    other.i[0] = __builtin_amdgcn_update_dpp(mine.i[0], mine.i[0], 0xB1, 0xF, 0xF, false);
                    other.i[1] = __builtin_amdgcn_update_dpp(mine.i[1], mine.i[1], 0xB1, 0xF, 0xF, false);
                    union { h16x4 h[2]; float4 f; } out;
                    out.h[0] = mine.h;
                    out.h[1] = other.h;
                    if (live && !(c4 & 1)) *reinterpret_cast<float4 *>(reinterpret_cast<char *>(yp) + ny * 2) = out.f;
                } else if (live) {
                    if (SC) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) o[k] *= 1.f / A_SCALE;
                    }
                    if (n_vec) *reinterpret_cast<float4 *>(yp + ny) = make_float4(o[0], o[1], o[2], o[3]);
                    else { yp[ny] = o[0]; if (n + 1 < p.Cout) yp[ny + 1] = o[1]; if (n + 2 < p.Cout) yp[ny + 2] = o[2]; }
                }
            }
            if (!ONE_PASS && pass + 1 < WM) __syncthreads();
        }
    };
    // (FMT_F16 outputs exist in half mode only and take an FMT_F16 residual or none: the planner keeps both sides of a shortcut in
    //  one format, make_conv_args refuses anything else)
    using F32c = std::integral_constant<int, FMT_F32>;
    using H16c = std::integral_constant<int, FMT_H16>;
    using F16c = std::integral_constant<int, FMT_F16>;
    const bool yh = p.fmt_y == FMT_H16, rh = RES != RES_NONE && p.fmt_r == FMT_H16;
    if (p.fmt_y == FMT_F16) {
        sweep(F16c{}, F16c{});
    } else if (yh) {
        if (rh) sweep(H16c{}, H16c{});
        else sweep(H16c{}, F32c{});
    } else {
        if (rh) sweep(F32c{}, H16c{});
        else sweep(F32c{}, F32c{});
    }
}
constexpr size_t conv_stage_bytes(int BM, int BN) { return (size_t)BM * (BN + 4) * sizeof(float); }

// 32x32 accumulator fragments (v_mfma_f32_32x32x*): col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
template <int BM, int BN, int WM, int WN, int ACT, int RES, int TM, int TN, int NT = 256, class RowMap = FlatRows, bool ONE_PASS = false>
__device__ __forceinline__ void conv_epilogue_rows(const ConvKernelArgs &p, f32x16 (&acc)[TM][TN], float *stage, RowMap rows, int n0, int tid) {
    constexpr int LD = BN + 4;
    const int lane = tid & 63, wn = (tid >> 6) % WN;
    const int col = lane & 31, rsel = (lane >> 5) * 4;
    auto store = [&](float *st) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e)
                    st[(i * 32 + rsel + (e & 3) + 8 * (e >> 2)) * LD + wn * (BN / WN) + j * 32 + col] = acc[i][j][e];
    };
    conv_epilogue_core<BM, BN, WM, WN, ACT, RES, NT, RowMap, ONE_PASS, false>(p, store, stage, rows, n0, tid);
}

// 16x16 accumulator fragments (v_mfma_f32_16x16x32_f16): col = lane & 15, row = 4 * (lane >> 4) + e; TM / TN count 16-wide blocks.
// (Bank check: the four 16-lane groups of a store sit 4 rows = 4 * (BN + 4) floats apart = 16 banks mod 64: conflict free.)
// FAST (the f16x3 kernels on this instruction): the accumulators arrive as conv_epilogue_scaled(true, ACT) says, full tiles take
// conv_epilogue_full.
template <int BM, int BN, int WM, int WN, int ACT, int RES, int TM, int TN, int NT = 256, class RowMap = FlatRows, bool ONE_PASS = false, bool FAST = false>
__device__ __forceinline__ void conv_epilogue16_rows(const ConvKernelArgs &p, f32x4 (&acc)[TM][TN], float *stage, RowMap rows, int n0, int tid) {
    constexpr int LD = BN + 4;
    const int lane = tid & 63, wn = (tid >> 6) % WN;
    const int col = lane & 15, rsel = (lane >> 4) * 4;
    auto store = [&](float *st) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    st[(i * 16 + rsel + e) * LD + wn * (BN / WN) + j * 16 + col] = acc[i][j][e];
    };
    conv_epilogue_core<BM, BN, WM, WN, ACT, RES, NT, RowMap, ONE_PASS, FAST>(p, store, stage, rows, n0, tid);
}
template <int BM, int BN, int WM, int WN, int ACT, int RES, int TM, int TN, int NT = 256, bool ONE_PASS = false, bool FAST = false>
__device__ __forceinline__ void conv_epilogue16(const ConvKernelArgs &p, f32x4 (&acc)[TM][TN], float *stage, int m0, int n0, int tid) {
    conv_epilogue16_rows<BM, BN, WM, WN, ACT, RES, TM, TN, NT, FlatRows, ONE_PASS, FAST>(p, acc, stage, FlatRows{m0}, n0, tid);
}

template <int BM, int BN, int WM, int WN, int ACT, int RES, int TM, int TN, int NT = 256, bool ONE_PASS = false>
__device__ __forceinline__ void conv_epilogue(const ConvKernelArgs &p, f32x16 (&acc)[TM][TN], float *stage, int m0, int n0, int tid) {
    conv_epilogue_rows<BM, BN, WM, WN, ACT, RES, TM, TN, NT, FlatRows, ONE_PASS>(p, acc, stage, FlatRows{m0}, n0, tid);
}

ConvKernelArgs make_conv_args(const ConvArgs &a);
// fused detector stem (conv_stem2.hip): 3x3/s1 RGB conv (direct, vector ALU) + 3x3/s2 32->64 conv (f16x3 MFMA) in one kernel
bool conv_stem2_applicable(const ConvKernelArgs &k0, const ConvKernelArgs &k1);
void launch_conv_stem2(const ConvKernelArgs &k0, const ConvKernelArgs &k1, hipStream_t s);
// fused first residual block (conv_block1.hip): conv1x1 64->32 + conv3x3 32->64 + shortcut to the block input
bool conv_block1_applicable(const ConvKernelArgs &k2, const ConvKernelArgs &k3);
void launch_conv_block1(const ConvKernelArgs &k2, const ConvKernelArgs &k3, hipStream_t s);

// dispatch on (activation, residual mode): f(A, R) is called with the pair as std::integral_constant values, so that a generic
// lambda can name the compile-time epilogue instantiation:  dispatch_act_res(k, [&](auto A, auto R) { launch<..., A, R>(k, s); });
template <class F> void dispatch_act_res(const ConvKernelArgs &k, F f) {
    using Linear = std::integral_constant<int, ACT_LINEAR>;
    using Leaky = std::integral_constant<int, ACT_LEAKY>;
    using Mish = std::integral_constant<int, ACT_MISH>;
    using Relu = std::integral_constant<int, ACT_RELU>;
    using None = std::integral_constant<int, RES_NONE>;
    using After = std::integral_constant<int, RES_AFTER_ACT>;
    using Before = std::integral_constant<int, RES_BEFORE_ACT>;
    switch (k.act * 4 + k.res_mode) {
        case ACT_LINEAR * 4 + RES_NONE: f(Linear{}, None{}); break;
        case ACT_LEAKY * 4 + RES_NONE: f(Leaky{}, None{}); break;
        case ACT_LEAKY * 4 + RES_AFTER_ACT: f(Leaky{}, After{}); break;
        case ACT_MISH * 4 + RES_NONE: f(Mish{}, None{}); break;
        case ACT_MISH * 4 + RES_AFTER_ACT: f(Mish{}, After{}); break;
        case ACT_RELU * 4 + RES_NONE: f(Relu{}, None{}); break;
        case ACT_RELU * 4 + RES_BEFORE_ACT: f(Relu{}, Before{}); break;
        default: fail("conv: unsupported activation/residual combination (%d, %d)", k.act, k.res_mode);
    }
}

// Launch of one instantiation KERN(ConvKernelArgs, args...) of a dynamic-LDS convolution kernel over the BM x BN tiles of k (times
// grid_y K ranges): raises the kernel's dynamic-LDS limit when this launch needs more than every earlier one (grow-only, one
// high-water mark per instantiation), plans the tile map, launches, checks the launch.
template <auto KERN, class... Args>
void launch_conv_tiles(ConvKernelArgs k, int BM, int BN, int grid_y, int threads, size_t smem, hipStream_t s, Args... args) {
    static size_t attr_set = 0;
    if (smem > attr_set) {
        YDS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERN), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        attr_set = smem;
    }
    dim3 grid(plan_tile_map(k, BM, BN), grid_y);
    hipLaunchKernelGGL(KERN, grid, dim3(threads), smem, s, k, args...);
    YDS_HIP(hipGetLastError());
}

// direct first-layer kernel (conv_first.hip)
bool conv_direct_applicable(const ConvKernelArgs &k);
void launch_conv_direct(const ConvKernelArgs &k, hipStream_t s);
// ReID stem: the direct kernel fused with MaxPool2d(3, 2, 1); k.y is the pooled tensor
bool conv_pool_applicable(const ConvKernelArgs &k);
void launch_conv_pool(const ConvKernelArgs &k, hipStream_t s);

// split-fp16 path (conv_f16x3.hip): one launcher per kernel family, `tile` picks the instantiation (conv.hip's variant table)
void launch_conv_f16x3_staged(ConvKernelArgs k, int tile, hipStream_t s);   // 0: 128x128, 1: 64x128, 2: 128x64, 3: 64x64
void launch_conv_f16x3_dma(ConvKernelArgs k, int tile, hipStream_t s);      // 0: 128x128 NS2, 1: 256x128 NS3, 2: 128x256 NS3, 3: 128x128 NS3, 4: 128x64 NS2, 5: 64x128 NS2
void launch_conv_f16x3_win(ConvKernelArgs k, int tile, hipStream_t s);      // 0: 256x128, 1: 256x64, 2: 128x64 (default arithmetic only)
void launch_conv_f16x3_splitk(ConvKernelArgs k, int tile, hipStream_t s);   // 0: 64x128, 1: 128x128
bool conv_splitk_applicable(const ConvKernelArgs &k, int tile);   // a split of >= 2 K ranges exists
bool conv_splitk_preferred(const ConvKernelArgs &k);              // the deterministic rule that selects split-K tile 0 (never timed against the others)
// two-workgroup window kernel (conv_win2.hip): 128x128 tiles, 4 waves, 16-channel K steps
bool conv_win2_applicable(const ConvKernelArgs &k);
void launch_conv_win2(ConvKernelArgs k, hipStream_t s);
// window-resident 3x3 stride-1 kernel: launch_conv_f16x3_win runs half mode (terms == 1) on conv_win.hip, the default arithmetic on conv_win16.hip
bool conv_win_applicable(const ConvKernelArgs &k);
void launch_conv_win(ConvKernelArgs k, int shape, hipStream_t s);   // half mode; shape 0: 256x128 (4x2 waves), otherwise 256x64
// sampled (shader cycles, 100 MHz ticks) accumulated inside the window kernels since the last reset
void conv_win_clock(unsigned long long *cycles_ticks, bool reset);   // in-kernel sampling: -DYDS_CLOCK_PROBE builds only (zeros otherwise)
void conv_win16_clock(unsigned long long *cycles_ticks, bool reset);
bool conv_win16_small_applicable(const ConvKernelArgs &k);           // shape 2 below
void launch_conv_win16(ConvKernelArgs k, int shape, hipStream_t s);  // default arithmetic, v_mfma_f32_16x16x32_f16; shape 0: 256x128 (4x2 waves), 1: 256x64 (8x1), 2: 128x64 (4x1, two workgroups per CU)
void conv_win2_clock(unsigned long long *cycles_ticks, bool reset);

}  // namespace yds
