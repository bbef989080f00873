// The frame the three window-resident 3x3 kernels share (conv_win.hip, conv_win16.hip, conv_win2.hip; conv_win.hip's header describes
// the data movement): ring geometry and LDS plan, tap validity, the nine-tap unroll and the in-kernel clock probe.  Each file keeps
// what really differs: its step schedule (the order of every memory operation inside an MFMA shadow is pinned by hand and measured),
// its fragment plan and its mfma order.  The DMA, tap_addr and prologue text stays per file as well, although much of it repeats:
// the compiler's inlining and register allocation in the K loops is sensitive to where that code lives (profiles/win_refactor_isa.txt).
#pragma once
#include "conv_common.h"

#include <utility>

namespace yds {
namespace {

// ---- ring geometry and LDS plan (host and device) ------------------------------------------------------------------------------
struct WinGeom {
    int row;                                   // bytes per LDS row: the channels one pixel / one filter contributes to a K step
    int nsb;                                   // filter-stage ring depth
    int apw;                                   // window DMA instructions per wave while one channel group is consumed (taps 0 .. apw-1 carry one each)
    constexpr int piece() const { return 1024 / row; }   // rows per DMA instruction (64 lanes x 16 bytes)
};
constexpr WinGeom WIN128 = {128, 3, 7};        // conv_win.hip, conv_win16.hip: one 32-channel group [32 hi | 32 lo] per row (half mode: 64 hi values)
constexpr WinGeom WIN64 = {64, 4, 6};          // conv_win2.hip: one 16-channel half group [16 hi | 16 lo] per row
constexpr int ROW = WIN128.row, NSB = WIN128.nsb, APW = WIN128.apw;

// several channel groups: two window buffers (the next group's window is fetched while this one is consumed); a single group needs one
constexpr int win_buffers(int Cin, int group_channels) { return Cin == group_channels ? 1 : 2; }

// LDS plan of a BM x BN tile on nw waves at image width W with nbuf window buffers
struct WinPlan {
    int wrows;                                 // window rows: the tile's pixels and W + 1 on either side, in whole DMA pieces
    size_t loop_bytes;                         // the windows + the filter ring + the zero row
    size_t launch_bytes;                       // ... or the epilogue's whole-tile staging in the same LDS where that is more (narrow images)
    bool prefetch_fits;                        // two buffers: the next window is fetched by at most apw instructions per wave
};
constexpr WinPlan win_plan(const WinGeom &g, int BM, int BN, int nw, int W, int nbuf) {
    const int wrows = (BM + 2 * W + 2 + g.piece() - 1) / g.piece() * g.piece();
    const size_t loop_bytes = (size_t)nbuf * wrows * g.row + (size_t)g.nsb * BN * g.row + g.row;
    return {wrows, loop_bytes, std::max(loop_bytes, conv_stage_bytes(BM, BN)), nbuf == 1 || wrows <= g.apw * nw * g.piece()};
}

// ---- taps -----------------------------------------------------------------------------------------------------------------------
// validity of the nine taps (bit t = tap (t / 3, t % 3)) of flat output pixel m: inside the image, and m inside the tensor
__device__ __forceinline__ unsigned tap_valid_bits(const ConvKernelArgs &p, int m) {
    unsigned bits = 0;
    if (m < p.M) {
        const int W = p.W, HW = p.H * W;
        const int rem = m % HW, y = rem / W, x = rem - y * W;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            bits |= ((unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)W ? 1u : 0u) << t;
        }
    }
    return bits;
}

// step(std::integral_constant<int, TAP>, args...) for TAP = 0 .. 8, in order: the nine K steps of one channel group, each with its tap
// at compile time
template <class Step, int... TAP, class... Args> __device__ __forceinline__ void each_tap(Step &step, std::integer_sequence<int, TAP...>, Args... args) {
    (step(std::integral_constant<int, TAP>{}, args...), ...);
}
template <class Step, class... Args> __device__ __forceinline__ void for_each_tap(Step &step, Args... args) {
    each_tap(step, std::make_integer_sequence<int, 9>{}, args...);
}

// ---- clock probe -----------------------------------------------------------------------------------------------------------------
// Sustained shader clock INSIDE the kernel (-DYDS_CLOCK_PROBE builds of tools/ only): one workgroup in 32 samples the shader-cycle
// counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) at its start and end; cycles / ticks is the clock the chip
// really ran at while every CU was busy with this kernel (it is power limited: ~1.55 GHz, not the 2.4 GHz the MFMA peak is quoted at).
// One pair of counters per translation unit, i.e. per window file.
#ifdef YDS_CLOCK_PROBE
__device__ unsigned long long yds_clk[2];
struct ClockProbe {
    bool sample;
    unsigned long long c0 = 0, w0 = 0;
    __device__ __forceinline__ explicit ClockProbe(int tid) : sample(tid == 0 && (blockIdx.x & 31) == 0) {
        if (sample) { c0 = __builtin_amdgcn_s_memtime(); w0 = wall_clock64(); }
    }
    __device__ __forceinline__ void end() const {
        if (sample) {
            atomicAdd(&yds_clk[0], __builtin_amdgcn_s_memtime() - c0);
            atomicAdd(&yds_clk[1], wall_clock64() - w0);
        }
    }
};
// host: (shader cycles, 100 MHz ticks) accumulated by this file's kernels since the last reset
inline void clock_probe_read(unsigned long long *cycles_ticks, bool reset) {
    YDS_HIP(hipMemcpyFromSymbol(cycles_ticks, HIP_SYMBOL(yds_clk), 2 * sizeof(unsigned long long)));
    if (reset) {
        unsigned long long z[2] = {};
        YDS_HIP(hipMemcpyToSymbol(HIP_SYMBOL(yds_clk), z, sizeof z));
    }
}
#else
struct ClockProbe {                            // product build: no sampling inside the kernel
    __device__ __forceinline__ explicit ClockProbe(int) {}
    __device__ __forceinline__ void end() const {}
};
inline void clock_probe_read(unsigned long long *cycles_ticks, bool) { cycles_ticks[0] = cycles_ticks[1] = 0; }
#endif

}  // namespace
}  // namespace yds
