// Window-resident 3x3 / stride-1 convolution on the fp16 matrix cores: the data movement all three window kernels share, and the
// half-mode tiers (the default f16x3 arithmetic, see conv_f16x3.hip, runs conv_win16.hip; two workgroups per CU: conv_win2.hip).
//
// The LDS-DMA implicit-GEMM kernel fetches the activation tile once per filter tap: nine times the same pixels,
// shifted.  Its K loop is bound by the number of global->LDS instructions a wave has to issue between its MFMAs
// (profiles/r01_ablation_dma.txt), so this kernel stops re-fetching: for a 3x3, stride 1, pad 1 layer the output pixel
// with flat index m (over batch, rows, columns) reads input pixel m + dy*W + dx, hence the 256 output pixels of a tile
// need the CONTIGUOUS run of input pixels [m0 - W - 1, m0 + 256 + W + 1).  That window (one 32-channel group = 128 B
// per pixel) is brought into LDS once per channel group and all nine taps read their A fragments from it at a row
// offset of (dy+1)*W + (dx+1); taps that fall outside the image (left/right column, top/bottom row, tile tail) are
// redirected per lane to a zero row.  Only the filter rows (BN x 128 B per tap) still stream through a 3-stage ring.
//   K order: channel group outer, tap inner (weights stay [Cout][kh][kw][Cin]: chunk index tap*G + g)
//   global->LDS instructions per wave and K step: 2 (filters) + <= 1 (next group's window), against 6-8 before
//   LDS: two window buffers (double buffered across channel groups) + 3 filter stages + the zero row <= 160 KB, one
//   512-thread workgroup per CU (8 waves, 4x2, 64x64 accumulator tiles), W <= 95 (single-group layers: one window
//   buffer, W <= 318)
// Same swizzle as the DMA kernel: row r keeps its 16-byte chunk c at position c ^ ((r >> 1) & 7), applied on the source
// address of the DMA and again by the fragment reads; 16 consecutive rows hit 16 distinct bank slots at any base.
#include "conv_win_common.h"

namespace yds {
namespace {

constexpr int BM = 256, NW = 8, NT = NW * 64;
constexpr int BN_MAX = 128;                    // the widest tile (shape 0): conv_win_applicable plans for it

// This file holds the HALF-MODE tiers of the window kernel (Darknet.half()), on v_mfma_f32_32x32x16_f16; the default f16x3 arithmetic
// runs conv_win16.hip.  BN x (WM x WN waves): 128 x (4x2) = 64x64 accumulator tiles per wave, 64 x (4x2) for 64-filter layers.
// TERMS: 1 = hi halves of both operands only: no lo fragment reads, one MFMA per product block;
// 4 = 64 channels per K step: the LDS rows (window and filter stages alike) are GATHERED by the DMA from the hi halves
// of two consecutive 32-channel groups (a DMA lane's global address is free), [hi of group 2q | hi of group 2q+1], so the "lo" fragment
// slots hold the second group's hi values and the step does A_hi x B_hi + A_lo x B_lo - the same DMA instructions, fragment reads and
// barrier per step as TERMS = 1 for twice the channels, i.e. half the steps (a K step is bound by those, not by its MFMAs, once two
// thirds of them are gone: profiles/r03_fp8_cross.txt #5).  Needs Cin % 64 == 0; the tensors in HBM stay H16.
template <int BN, int WM, int WN, int ACT, int RES, int TERMS>
__global__ __launch_bounds__(NT, 1) void conv3x3_f16x3_win(ConvKernelArgs p, int wrows, int nbuf) {
    fp16_saturate_on();
    static_assert(WM * WN == NW, "eight waves");
    static_assert(TERMS == 1 || TERMS == 4, "the default arithmetic (three fp16 terms) is conv_win16.hip's kernel");
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int B_STAGE = BN * ROW;
    constexpr int B_INST = BN / (8 * NW);      // filter DMA instructions per wave per stage (8 rows each)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int WB = wrows * ROW;                                  // bytes per window buffer
    char *bring = smem + nbuf * WB;                              // [NSB][BN][128]; nbuf = 2 window buffers, 1 for single-group layers
    const int zoff = nbuf * WB + NSB * B_STAGE;                  // zero row

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (SGPR): LDS-DMA destinations need no v_readfirstlane per piece
    const int wm = wave / WN, wn = wave % WN;
    int m0, n0;
    {
        int tm, tn;
        if (!tile_of_block(p, tm, tn)) return;
        m0 = tm * BM;
        n0 = tn * BN;
    }
    if (tid < 32) reinterpret_cast<float *>(smem + zoff)[tid] = 0.f;
    const ClockProbe clk(tid);

    const int W = p.W, G = TERMS == 4 ? p.Cin / 64 : p.Cin / 32;       // channel groups per K step
    constexpr int GROUP_BYTES = TERMS == 4 ? 256 : 128;
    // logical 16-byte chunk c of an LDS row -> chunk of the global record(s): TERMS = 4 takes chunks 0-3 (the hi halves) of two records
    auto gchunk = [&](int c) { return TERMS == 4 ? ((c >> 2) << 3) + (c & 3) : c; };
    // An FMT_F16 activation tensor (2-byte half-mode activations, TERMS = 4 only) already is the gathered row: 64 channels = 128
    // contiguous bytes with chunk c in place; the filters keep the split record.  Strides stay in float slots (h16.h).
    const bool xs = TERMS == 4 && p.fmt_x == FMT_F16;
    const int x_group_bytes = xs ? 128 : GROUP_BYTES;
    const int drow = lane >> 3, dpos = lane & 7;
    // window pieces: piece pc covers window rows pc*8 .. pc*8+7, wave w issues pieces w, w+8, ...; row j <-> flat input
    // pixel m0 - W - 1 + j (clamped into the tensor: rows outside it are never read unmasked); offsets in 16-byte units
    const int npieces = wrows / 8;
    unsigned w_off16[B_INST];
#pragma unroll
    for (int b = 0; b < B_INST; ++b) {
        const int row = (b * NW + wave) * 8 + drow;
        w_off16[b] = (unsigned)min(n0 + row, p.Cout - 1) * (unsigned)(p.Kpad / 4) + (unsigned)gchunk(dpos ^ ((row >> 1) & 7));
    }
    const char *x_bytes = reinterpret_cast<const char *>(p.x), *w_bytes = reinterpret_cast<const char *>(p.w);
    auto a_piece = [&](int g, int k) {                           // window of channel group g -> buffer g & 1
        const int pc = min(k * NW + wave, npieces - 1);        // surplus instructions repeat the last piece (same data, same place)
        const int j = pc * 8 + drow;
        const int f = min(max(m0 - W - 1 + j, 0), p.M - 1);
        const int c = dpos ^ ((j >> 1) & 7);
        const unsigned off16 = (unsigned)f * (unsigned)(p.ldx / 4) + (unsigned)(xs ? c : gchunk(c));
        const char *src = x_bytes + (size_t)g * x_group_bytes + ((size_t)off16 << 4);
        __builtin_amdgcn_global_load_lds((glb_void_t *)src, (lds_void_t *)(smem + (g & 1) * WB + pc * 8 * ROW), 16, 0, 0);
    };
    auto b_piece = [&](int g, int tap, int stage, int b) {       // filter rows of K chunk (tap, g)
        const char *src = w_bytes + (size_t)(tap * G + g) * GROUP_BYTES + ((size_t)w_off16[b] << 4);
        __builtin_amdgcn_global_load_lds((glb_void_t *)src, (lds_void_t *)(bring + stage * B_STAGE + (b * NW + wave) * 8 * ROW), 16, 0, 0);
    };

    // per-lane validity of the nine taps for the two A fragments of this wave (rows wm*64 + i*32 + (lane & 31))
    int r_row[TM];
    unsigned ok9[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        r_row[i] = wm * (BM / WM) + i * 32 + (lane & 31);
        ok9[i] = tap_valid_bits(p, m0 + r_row[i]);
    }

    f32x16 acc1[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc1[i][j][e] = 0.f;

    // filter fragment addressing (as in the DMA kernel)
    const int swz = (lane >> 1) & 7, kb = lane >> 5;
    const int b_frag = (wn * (BN / WN) + (lane & 31)) * ROW;
    int bpos_hi[2], bpos_lo[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) { bpos_hi[s] = ((2 * s + kb) ^ swz) * 16; bpos_lo[s] = ((4 + 2 * s + kb) ^ swz) * 16; }

    constexpr int NF = 2 * (TM + TN), NM = 3 * TM * TN;
    h8 fr[2][NF];                                               // [substep][A0h, A0l, A1h, A1l, B0h, B0l, B1h, B1l]
    int a_addr[TM], a_sw[TM];                                   // this tap: LDS byte address of the lane's window row (or the zero row), swizzle
    auto frag_read = [&](const char *bst, int s, int f) {
        const int which = f / 2, lo = f & 1;
        if (TERMS == 1 && lo) return;
        if (which < TM) {
            const int c = (lo ? 4 : 0) + 2 * s + kb;
            fr[s][f] = *reinterpret_cast<const h8 *>(smem + a_addr[which] + ((c ^ a_sw[which]) << 4));
        } else {
            fr[s][f] = *reinterpret_cast<const h8 *>(bst + b_frag + (which - TM) * 32 * ROW + (lo ? bpos_lo[s] : bpos_hi[s]));
        }
    };
    // slot m of a substep: product block m / 3, term m % 3 of the three-term slot plan the schedule below is laid out for; the half
    // tiers fill term 0 (hi x hi) and, TERMS = 4, term 1 (the "lo" slots hold the second channel group's hi values)
    auto mfma = [&](int s, int m) {
        const int ij = m / 3, term = m % 3, i = ij / TN, j = ij % TN;
        if (term == 0) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[s][2 * i], fr[s][2 * (TM + j)], acc1[i][j], 0, 0, 0);
        else if (TERMS == 4 && term == 1) acc1[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fr[s][2 * i + 1], fr[s][2 * (TM + j) + 1], acc1[i][j], 0, 0, 0);
    };
    // substep-1 fragment order: the operands of accumulator tile (0,0) first
    auto frag_order = [&](int k) {
        if (k < 2) return k;
        if (k < 4) return 2 * TM + (k - 2);
        const int r = k - 4, nb = 2 * (TN - 1);
        return r < nb ? 2 * TM + 2 + r : 2 + (r - nb);
    };

    // One K step = tap TAP of channel group g, software pipelined across steps (the wave issues in order and an MFMA
    // occupies the matrix pipe for 32 cycles, so every memory instruction sits in the shadow of one MFMA, order pinned):
    //   substep 0   12 MFMAs on fr[0] (read during the previous step)    slots: this step's substep-1 fragments -> fr[1]
    //   mid         s_waitcnt vmcnt(0) + s_barrier: the filter stage of step t+1 (and, before a new group, its window)
    //               has landed for every wave, and every wave is done with step t-1
    //   substep 1   12 MFMAs on fr[1]      slots: window piece of group g+1, filter pieces of step t+2 (into the stage
    //               step t-1 used), then the substep-0 fragments of step t+1 -> fr[0]
    // so the only exposed latency per step is the barrier itself.
    auto tap_addr = [&](int g, int tap) {                        // A-fragment row addresses for (g, tap)
        const int shift = (tap / 3) * W + (tap % 3);            // (dy+1)*W + (dx+1)
        const int wbase = (g & 1) * WB;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            asm volatile("" : "+v"(r_row[i]), "+v"(ok9[i]));      // keep the per-tap addresses out of loop-invariant hoisting (registers)
            const bool ok = (ok9[i] >> tap) & 1u;
            const int j = r_row[i] + shift;
            a_addr[i] = ok ? wbase + j * ROW : zoff;
            a_sw[i] = ok ? (j >> 1) & 7 : 0;
        }
    };
    auto step = [&](auto tap_c, int g, auto last_c) {
        constexpr int TAP = decltype(tap_c)::value;
        constexpr bool LAST = decltype(last_c)::value;          // last channel group: no window prefetch, filter refills stop
        constexpr int AHEAD = 2;             // prefetch distance of the filter stages, in steps
        constexpr bool REFILL = !(LAST && TAP + AHEAD > 8);     // a step t+AHEAD exists
        constexpr bool NEXT = !(LAST && TAP == 8);              // a step t+1 exists
        constexpr int TAP1 = (TAP + 1) % 9, TAP2 = (TAP + AHEAD) % 9;
        constexpr int OPS = (1 + B_INST + NF + NM - 1) / NM;    // memory operations per substep-1 slot
        static_assert(NF <= NM, "not enough MFMA slots in substep 0");
        const int g1 = TAP + 1 >= 9 ? g + 1 : g, g2 = TAP + AHEAD >= 9 ? g + 1 : g;
        const char *bst = bring + (TAP % NSB) * B_STAGE, *bst1 = bring + ((TAP + 1) % NSB) * B_STAGE;
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            mfma(0, m);
            __builtin_amdgcn_sched_barrier(0);
            if (m < NF) frag_read(bst, 1, frag_order(m));
            __builtin_amdgcn_sched_barrier(0);
        }
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        if (NEXT) tap_addr(g1, TAP1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            mfma(1, m);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int o = m * OPS; o < (m + 1) * OPS; ++o) {     // memory operations of this slot
                if (o == 0) { if (!LAST && TAP < APW) a_piece(g + 1, TAP); }
                else if (o - 1 < B_INST) { if (REFILL) b_piece(g2, TAP2, (TAP + AHEAD) % NSB, o - 1); }
                else if (o - 1 - B_INST < NF) { if (NEXT) frag_read(bst1, 0, o - 1 - B_INST); }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    auto group = [&](int g, auto last_c) { for_each_tap(step, g, last_c); };

    // prologue: window of group 0, filter stages of steps 0 and 1, fragments of step 0 / substep 0
    for (int k = 0; k < (npieces + NW - 1) / NW; ++k) a_piece(0, k);
#pragma unroll
    for (int b = 0; b < B_INST; ++b) b_piece(0, 0, 0, b);
#pragma unroll
    for (int b = 0; b < B_INST; ++b) b_piece(0, 1, 1, b);
    wait_vmcnt<B_INST>();              // later stages may still be in flight: the mid-step waits cover them
    __syncthreads();                                            // window 0, stage 0 and the zero row are in LDS
    tap_addr(0, 0);
#pragma unroll
    for (int f = 0; f < NF; ++f) frag_read(bring, 0, f);
    __builtin_amdgcn_sched_barrier(0);

    for (int g = 0; g + 1 < G; ++g) group(g, std::false_type{});
    group(G - 1, std::true_type{});

    __syncthreads();                                            // every wave is done with the window and the ring
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e)
                acc1[i][j][e] *= 1.f / A_SCALE;
    conv_epilogue<BM, BN, WM, WN, ACT, RES, TM, TN, NT, true>(p, acc1, reinterpret_cast<float *>(smem), m0, n0, tid);   // whole-tile staging
    clk.end();
}

// 64 channels per K step where Cin allows (TERMS = 4): a 64-channel layer is a single group there
constexpr int step_channels(const ConvKernelArgs &k) { return k.terms == 1 && k.Cin % 64 == 0 ? 64 : 32; }

template <int BN, int WM, int WN, int ACT, int RES, int TERMS> void launch_inst_win(ConvKernelArgs k, hipStream_t s) {
    const int nbuf = win_buffers(k.Cin, TERMS == 4 ? 64 : 32);
    const WinPlan plan = win_plan(WIN128, BM, BN, NW, k.W, nbuf);
    launch_conv_tiles<conv3x3_f16x3_win<BN, WM, WN, ACT, RES, TERMS>>(k, BM, BN, 1, NT, plan.launch_bytes, s, plan.wrows, nbuf);
}

}  // namespace

void conv_win_clock(unsigned long long *cycles_ticks, bool reset) { clock_probe_read(cycles_ticks, reset); }

// the 256-row tiles of this file and of conv_win16.hip (its shapes 0 / 1: same LDS plan), planned for the widest one
bool conv_win_applicable(const ConvKernelArgs &k) {
    const bool presplit = (k.fmt_x == FMT_H16 && k.Cin % 32 == 0) || (k.fmt_x == FMT_F16 && k.terms == 1 && k.Cin % 64 == 0);
    if (!(k.ksize == 3 && k.stride == 1 && k.pad == 1 && presplit && k.H == k.Ho && k.W == k.Wo)) return false;
    const WinPlan plan = win_plan(WIN128, BM, BN_MAX, NW, k.W, win_buffers(k.Cin, step_channels(k)));
    // several channel groups: the next group's window is fetched by at most APW instructions per wave while this one is
    // consumed (two buffers); a single group needs one buffer only, which admits much wider images
    // (the epilogue stages BM x (BN+4) floats in the same LDS: 135 KB at BN = 128)
    return plan.prefetch_fits && plan.launch_bytes <= 160 * 1024 && (size_t)k.M * (k.ldx / 4) < (1ull << 32);
}

// half mode (launch_conv_f16x3_win checks applicability): 256x128, or 256x64 for narrow layers; 64 channels per K step where Cin allows
void launch_conv_win(ConvKernelArgs k, int shape, hipStream_t s) {
    dispatch_act_res(k, [&](auto A, auto R) {
        if (k.Cin % 64 == 0) {
            if (shape == 0) launch_inst_win<128, 4, 2, A, R, 4>(k, s);
            else launch_inst_win<64, 4, 2, A, R, 4>(k, s);
        } else {
            if (shape == 0) launch_inst_win<128, 4, 2, A, R, 1>(k, s);
            else launch_inst_win<64, 4, 2, A, R, 1>(k, s);
        }
    });
}

}  // namespace yds
