// ReID front end in one kernel: crop + cv2-exact resize to 128 x 64 + /255 + mean/std (crop_resize_kernel, layers.hip) and the stem
// conv3x3(3->64) + BN + ReLU + MaxPool2d(3, 2, 1) (conv3x3_rgb_pool_mfma, conv_first.hip), from the uint8 frames and the crop list to
// the pooled H16 tensor [D, 64, 32, 64].  The pair it replaces writes the normalised crop to HBM as fp32 NHWC4 (131 KB per crop) and
// reads it back, and stages every convolution output in LDS as fp32 to pool it from there; here neither exists.  The values are
// those of the pair: resize_px, the crop kernel's normalisation (as a table, below), the same split-fp16 MFMA products in the same
// order, the same recombination, activation and H16 encoding - the pooled tensor is bit-identical (tests/test_gpu_reid_front.py).
//
// Scheme.  A unit is 16 pooled rows of one crop over the full width (4 units per crop); a 256-thread persistent workgroup takes units
// in a grid-stride loop.  Per unit:
//   1. all threads resize the 35 x 64 input pixels the unit needs (input rows 2 py0 - 2 .. 2 py0 + 32; rows outside the crop and the
//      columns -1 and 64: zero, the convolution's padding) straight into LDS as the split tile: (hi r g b 0) and (lo r g b 0),
//      8 bytes each, in two planes.  A tile row keeps the odd columns (-1, 1, .., 63) in its first 33 entries and the even ones
//      (0, 2, .., 64) in the other 33.
//   2. wave (n, s) - n: channels 32 n .. 32 n + 31, s: pooled rows 8 s .. 8 s + 7 of the unit - sweeps down its 17 convolution rows.
//      A row is two MFMA fragments of 32 positions: lane j of the first holds column 2 j, of the second column 2 j + 1 (so every
//      operand read has a lane stride of 8 bytes within one column parity).  A pooled pixel j is the maximum over columns 2 j - 1,
//      2 j, 2 j + 1: the lane's own two values and the second fragment's value of lane j - 1, one DPP shift (column -1 is the pool's
//      padding: pooled column 0 takes its own value twice).  The vertical 3-maximum runs in registers: rows 2 P - 1, 2 P, 2 P + 1,
//      the last carried over as row 2 (P + 1) - 1; row -1 is -inf.  The maxima are taken over the recombined products; bias and
//      ReLU follow once per pooled value (conv_row below).  Every pooled row is encoded and stored as soon as it is complete -
//      half-wave pairs trade their 8-byte channel quads (v_permlane32_swap) so that a lane stores 16 bytes.
// Recompute: 17/16 of the convolution rows, 35/32 of the resized rows.  The crop's box (and its frame's geometry) is read by ONE
// thread per unit, a unit ahead, into LDS - the list lives in pinned host memory in the pipeline.
// Budget: LDS 35 * 66 * 16 + 3 072 + 48 = 40 080 bytes per workgroup; registers: 24 filter fragments + 12 operand offsets + 16 running
// maxima + 32 accumulators + 32 row values = 152 allocated, within the 168 of three workgroups (12 waves) per CU.
#include "conv_common.h"
#include "resize_dev.h"

#include <algorithm>

namespace yds {

namespace {
constexpr int RS_H = 128, RS_W = 64, RS_HP = 64, RS_WP = 32;        // crop and pooled size
constexpr int RS_PR = 16, RS_WR = 8;                                // pooled rows per unit and per wave
constexpr int RS_UNITS = RS_HP / RS_PR;                             // units per crop
static_assert(RS_UNITS == kReidStemUnitsPerCrop, "common.h tells the callers");
constexpr int RS_IR = 2 * RS_PR + 3;                                // input rows of a unit
constexpr int RS_PW = RS_W / 2 + 1, RS_ROW = 2 * RS_PW;             // entries per column parity, per tile row
constexpr int RS_NT = 256, RS_OCC = 3;
static_assert(RS_NT / 64 == 2 * (RS_PR / RS_WR), "one wave per channel half and 8 pooled rows");

struct CropSrc { unsigned long long off; int row_bytes, cw, ch, pad; };    // top-left source pixel of a crop, its row stride and size

// Maxima of values that are arithmetic results or -inf.  fmaxf would first quiet a signalling NaN in every operand the compiler cannot
// prove canonical (a v_max_f32 x, x each): that doubled the vector-ALU work of the sweep, which is what bounds it.  The bit-identity
// with the unfused pair is claimed for finite weights and biases (every sample is finite): with a NaN among them the two paths may
// pick different NaN payloads, and neither path's output means anything.
__device__ __forceinline__ float rs_max(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float rs_max3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// tile entry of input column c (-1 .. 64)
__device__ __forceinline__ int rs_entry(int c) { return (c & 1) ? (c + 1) >> 1 : RS_PW + (c >> 1); }
}  // namespace

__global__ __launch_bounds__(RS_NT, RS_OCC) void reid_stem_kernel(ReidFront f, const float *w, int kpad, const float *bias, float *y, int n_units) {
    fp16_saturate_on();
    __shared__ __attribute__((aligned(16))) h16x4 tile_hi[RS_IR * RS_ROW], tile_lo[RS_IR * RS_ROW];   // (r g b 0) halves of a pixel
    __shared__ CropSrc src[2];
    // A resized sample is one of 256 integers, so its normalised and split value is one of 3 x 256: crop_resize_kernel's
    // ((s / 255) - mean) / std in the same three correctly rounded steps, then h16_encode4, evaluated once per workgroup instead of
    // once per pixel (six IEEE divisions and the split).  [channel][sample] = hi | lo << 16
    __shared__ unsigned int norm[3 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kb = lane >> 5, j = lane & 31, n = wave & 1, sub = wave >> 1;
    // filter fragments of this wave's 32 channels (first MFMA operand: row = channel, k = 16 sb + 8 kb + e = tap 4 sb + 2 kb + (e >> 2),
    // channel e & 3), split on the fly - the layout of conv3x3_rgb_pool_mfma
    h8 wh[3], wl[3];
#pragma unroll
    for (int sb = 0; sb < 3; ++sb)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int t = 4 * sb + 2 * kb + (e >> 2), c = e & 3;
            const float x = (t < 9 && c < 3) ? w[(size_t)(n * 32 + j) * kpad + t * 4 + c] : 0.f;
            const _Float16 h = (_Float16)x;
            wh[sb][e] = h;
            wl[sb][e] = (_Float16)((x - (float)h) * 2048.f);
        }
    // operand offsets of this lane's taps relative to the tile row of tap row 0: [fragment][sb][h]; a padding tap (t >= 9) reads
    // entry 0 of that row, column -1, which is zero in every row
    int off[2][3][2];
#pragma unroll
    for (int fr = 0; fr < 2; ++fr)
#pragma unroll
        for (int sb = 0; sb < 3; ++sb)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int t = 4 * sb + 2 * kb + h;
                off[fr][sb][h] = t < 9 ? (t / 3) * RS_ROW + rs_entry(2 * j + fr - 1 + t % 3) : 0;
            }
    for (int i = tid; i < 3 * 256; i += RS_NT) {
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
        const int c = i >> 8;
        const float px[4] = {__fdiv_rn(__fsub_rn(__fdiv_rn((float)(i & 255), 255.f), mean[c]), stdv[c]), 0.f, 0.f, 0.f};
        union { h16x4 h; unsigned short u[4]; } hi, lo;
        h16_encode4(px, hi.h, lo.h);
        norm[i] = hi.u[0] | (unsigned int)lo.u[0] << 16;
    }
    auto load_src = [&](int u, int slot) {
        const int *b = f.boxes + (size_t)(u / RS_UNITS) * 5;
        const int x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3], fi = b[4];
        CropSrc c;
        if (f.geom) {
            const FrameGeom g = f.geom[fi];
            c.off = g.off + ((unsigned long long)y1 * g.w + x1) * 3;
            c.row_bytes = g.w * 3;
        } else {
            c.off = ((unsigned long long)fi * f.h * f.w + (unsigned long long)y1 * f.w + x1) * 3;
            c.row_bytes = f.w * 3;
        }
        c.cw = x2 - x1; c.ch = y2 - y1; c.pad = 0;
        src[slot] = c;
    };
    if (tid == 0) load_src(blockIdx.x, 0);
    int cur = 0;
    for (int u = blockIdx.x; u < n_units; u += gridDim.x, cur ^= 1) {         // trip count uniform per workgroup
        __syncthreads();                                                        // previous unit swept; src[cur] written
        if (tid == 0 && u + (int)gridDim.x < n_units) load_src(u + gridDim.x, cur ^ 1);
        const CropSrc cs = src[cur];
        const int d = u / RS_UNITS, py0 = (u - d * RS_UNITS) * RS_PR, iy0 = 2 * py0 - 2;
        const uint8_t *base = f.frames + cs.off;
        // thread -> (row r, column ix): ix is the same in every trip, so its horizontal tap is computed once per unit
        const int ix = tid & (RS_W - 1);
        for (int r = tid / RS_W; r < RS_IR; r += RS_NT / RS_W) {
            const int iy = iy0 + r;
            uint2 vh = make_uint2(0u, 0u), vl = make_uint2(0u, 0u);
            if ((unsigned)iy < (unsigned)RS_H) {
                float o[3];
                resize_px(base, (size_t)cs.row_bytes, cs.ch, cs.cw, RS_H, RS_W, iy, ix, o);
                if (f.bgr) { const float t = o[0]; o[0] = o[2]; o[2] = t; }     // (BGR frames: see resize_u8_kernel)
                const unsigned int e0 = norm[(int)o[0]], e1 = norm[256 + (int)o[1]], e2 = norm[512 + (int)o[2]];
                vh = make_uint2((e0 & 0xffffu) | e1 << 16, e2 & 0xffffu);
                vl = make_uint2(e0 >> 16 | (e1 & 0xffff0000u), e2 >> 16);
            }
            *reinterpret_cast<uint2 *>(&tile_hi[r * RS_ROW + rs_entry(ix)]) = vh;
            *reinterpret_cast<uint2 *>(&tile_lo[r * RS_ROW + rs_entry(ix)]) = vl;
        }
        if (tid < 2 * RS_IR) {                                                  // columns -1 and 64
            const int e = (tid >> 1) * RS_ROW + ((tid & 1) ? RS_ROW - 1 : 0);
            tile_hi[e] = h16x4{0, 0, 0, 0};
            tile_lo[e] = h16x4{0, 0, 0, 0};
        }
        __syncthreads();
        // convolution row r of the crop (r = -1: computed on the zero rows above the crop and discarded), as the recombined products
        // BEFORE bias and ReLU, already reduced to the horizontal 3-maximum of the pool: x -> relu(256 x + bias) does not decrease, so
        // it commutes with the maximum, bit for bit, and is applied once per pooled value instead of once per convolution output.
        // hm[4 g + c] = channel 32 n + 8 g + 4 kb + c of pooled column j
        auto conv_row = [&](int r, float hm[16]) {
            const int row = (r + 1 - 2 * py0) * RS_ROW;
            float t[2][16];
#pragma unroll
            for (int fr = 0; fr < 2; ++fr) {
                f32x16 c1, c2;
#pragma unroll
                for (int e = 0; e < 16; ++e) { c1[e] = 0.f; c2[e] = 0.f; }
#pragma unroll
                for (int sb = 0; sb < 3; ++sb) {
                    union { h16x4 q[2]; h8 v; } xh, xl;
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        xh.q[h] = tile_hi[row + off[fr][sb][h]];
                        xl.q[h] = tile_lo[row + off[fr][sb][h]];
                    }
                    c1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[sb], xh.v, c1, 0, 0, 0);
                    c2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[sb], xl.v, c2, 0, 0, 0);
                    c2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[sb], xh.v, c2, 0, 0, 0);
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) t[fr][e] = c1[e] + c2[e] * (1.f / 2048.f);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                // column 2 j - 1: the odd fragment's value of the lane below (DPP wave_shr:1).  Pooled column 0 has the padding there:
                // lanes 0 and 32 take their own value a second time instead
                const int own = __float_as_int(t[1][e]), left = __builtin_amdgcn_update_dpp(own, own, 0x138, 0xF, 0xF, false);
                hm[e] = rs_max3(t[0][e], t[1][e], __int_as_float(j == 0 ? own : left));
            }
        };
        // rows 2 p0 - 1 .. 2 p0 + 15: `run` holds the maximum over the rows of the open pooled row seen so far
        const int p0 = py0 + sub * RS_WR;                                       // this wave's first pooled row
        float run[16];
#pragma unroll 1
        for (int i = 0; i <= 2 * RS_WR; ++i) {
            const int r = 2 * p0 - 1 + i, Py = r >> 1;
            float hm[16];
            conv_row(r, hm);
            if (r & 1) {                                                        // row 2 P + 1 closes pooled row P and opens P + 1
                if (i == 0) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) run[e] = r < 0 ? -INFINITY : hm[e];
                    continue;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) run[e] = rs_max(run[e], hm[e]);
                continue;
            }
            union { h16x4 h; unsigned int i[2]; } hi[4], lo[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 b4 = *reinterpret_cast<const float4 *>(bias + n * 32 + 8 * g + 4 * kb);
                const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
                float m[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    m[c] = apply_act<ACT_RELU>(rs_max(run[g * 4 + c], hm[g * 4 + c]) * 256.f + bb[c]);
                    run[g * 4 + c] = hm[g * 4 + c];
                }
                h16_encode4(m, hi[g].h, lo[g].h);
            }
            // H16 pixel: per 32 channels 64 bytes of hi halves, then 64 of lo halves.  Lane (j, kb) holds the quads 8 g + 4 kb .. + 3;
            // after the half-wave trade the lower lane holds channels 16 p .. 16 p + 7 and the upper one 16 p + 8 .. 16 p + 15.
            char *pix = reinterpret_cast<char *>(y + ((size_t)(d * RS_HP + Py) * RS_WP + j) * 64) + n * 128 + kb * 16;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
#pragma unroll
                for (int l = 0; l < 2; ++l) {
                    unsigned int *ka = l ? lo[2 * p].i : hi[2 * p].i, *kn = l ? lo[2 * p + 1].i : hi[2 * p + 1].i;
                    const auto s0 = __builtin_amdgcn_permlane32_swap(ka[0], kn[0], false, false);
                    const auto s1 = __builtin_amdgcn_permlane32_swap(ka[1], kn[1], false, false);
                    uint4 o4;
                    o4.x = s0[0]; o4.y = s1[0]; o4.z = s0[1]; o4.w = s1[1];
                    *reinterpret_cast<uint4 *>(pix + l * 64 + p * 32) = o4;
                }
            }
        }
    }
}

// workgroups of the persistent grid: RS_OCC per CU of the current device
int reid_stem_grid() {
    static int grid = 0;
    if (!grid) {
        int dev = 0, cus = 0;
        YDS_HIP(hipGetDevice(&dev));
        YDS_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        grid = std::max(cus, 1) * RS_OCC;
    }
    return grid;
}

// pooled: the H16 tensor [D, 64, 32, 64]; w, bias: the stem's folded fp32 weights (rows of kpad floats, tap-major x 4 channels)
void launch_reid_stem(const ReidFront &f, int D, const float *w, int kpad, const float *bias, const View &pooled, hipStream_t s) {
    if (D < 1) return;
    if (pooled.fmt != FMT_H16 || pooled.h != RS_HP || pooled.w != RS_WP || pooled.c != 64 || pooled.ld != 64 || pooled.n < D)
        fail("reid stem: the pooled view must be H16 [D,%d,%d,64]", RS_HP, RS_WP);
    if (!f.frames || !f.boxes) fail("reid stem: no frames or no crop list");
    const int n_units = D * RS_UNITS;
    hipLaunchKernelGGL(reid_stem_kernel, dim3((unsigned)std::min(n_units, reid_stem_grid())), dim3(RS_NT), 0, s, f, w, kpad, bias, pooled.p, n_units);
    YDS_HIP(hipGetLastError());
}

}  // namespace yds
