// Heat maps on the device: per video stream a grid of square cells over the frame with five int64 layers in HBM - presence, visits,
// dwell_us, flow_x, flow_y - and a table of tracks - id, age, cell, last doubled foot point and its time - advanced by one launch
// per call beside the action and zone stages (actions.hip, zones.hip) and built on the same frame (track_stage.h); and a renderer
// that blends the colour map of one layer IN PLACE into packed 3-byte frames resident in HBM.
//
// There is no reference counterpart; the rules are written down in include/ydsort.h (the heat maps block) and restated in Python
// ints by yolo_deepsort_amd/heatmap.py (HeatMap, levels, render), which every device test compares against with exact equality.
//
// Accumulation.  One workgroup per stream that has frames in the call walks that stream's frames in time order.  Per frame it stages
// the rows once (they may sit in pinned host memory: a tracker result block), drops the rows of another class by an ordered
// compaction in place, registers unknown ids at the end of the table in row order, then handles the entries in table order, a thread
// per entry: a seen entry credits dwell to its previous cell, flow, a visit and presence to its new one, an unseen entry ages.
// Several rows of a frame can land in one cell, so every layer update is a 64-bit integer atomic: integer sums do not depend on
// the order of the threads.  Entries older than max_age then leave by an ordered compaction (track_stage.h retire).  The stage
// reports nothing per event: its result block carries the frames' counted-row counts and the tables' entry counts.
//
// Render, two launches.  heat_levels_kernel, a workgroup per stream named in the call: the layer's maximum (LDS tree), then per cell
// level = (min(max(v, 0), vmax) * 65535) / vmax as uint16 - the only 64-bit divisions, one per cell.  heat_render_kernel streams the
// frames named in the call: a thread owns PX consecutive pixels of a row, reads them whole, evaluates the bilinear field between
// cell centres in 32-bit integers (the weights of a pixel sum to 4 c^2 <= 2^16 and a level is < 2^16, so the numerator fits a
// uint32; 4 c^2 is a shift, / 257 a constant), looks the colours up in an LDS copy of the LUT, blends two bytes per multiply and
// writes the pixels back only when one of them changed.  The four levels a pixel reads change only where the pixel crosses a cell
// centre, so they are reloaded there and nowhere else.  PX = 16 (three 16-byte accesses per thread) when every address it forms is
// proved 16-aligned - the frames' base is and W % 16 == 0 (rows and frames are then multiples of 48 bytes); PX = 4 (three dwords)
// with a 4-aligned base and W % 4 == 0; a byte path otherwise (a 33 x 50 frame, an odd base).
#include "heat_render.h"
#include "track_stage.h"
#include "ydsort.h"

#include <algorithm>

namespace yds {

constexpr long long HEAT_VMAX_LIMIT = YDS_HEATMAP_VMAX_LIMIT;
constexpr int HEAT_ANCHOR_LIMIT = 1 << 24;        // the zones' clamp of a doubled foot point
constexpr int N_LAYERS = 5, N_RENDERABLE = 3;

// table of one stream: `cap` entries, every field twice (the second copy takes the survivors of a removal)
struct HeatTab {
    int *id, *age, *cell, *px, *py;               // [2][cap] each
    double *pt;                                   // [2][cap]        time of the last sighting
    int *count;                                   // live entries (device)
    int cap;
};
struct HeatWork {
    HeatTab tab;
    unsigned long long *layers;                   // [5][gh * gw] two's complement sums
    int gw, gh, shift, cls;                       // shift = log2(2 * cell): a doubled coordinate >> shift is its cell index
    int f0, f1;                                   // frames [f0, f1) of the call's frame list (sorted by stream, order kept)
    int *srows;                                   // staging [max rows of a frame][6]
    int res_count;                                // int index in the result block of this stream's entry count
};
struct HeatFrameDev {
    const int *rows;
    const int *n_p;
    double t;
    int n;
    int res_n;                                    // int index in the result block of this frame's counted-row count
};

__device__ __forceinline__ int heat_clamp(long long v) {
    return (int)(v < -HEAT_ANCHOR_LIMIT ? -HEAT_ANCHOR_LIMIT : v > HEAT_ANCHOR_LIMIT ? HEAT_ANCHOR_LIMIT : v);
}

__global__ __launch_bounds__(256) void heat_update_kernel(const HeatWork *works, const HeatFrameDev *frames, int max_age, int *res) {
    __shared__ int s_cnt[4];
    const HeatWork W = works[blockIdx.x];
    const HeatTab T = W.tab;
    const int tid = threadIdx.x, cap = T.cap;
    const size_t G = (size_t)W.gw * W.gh;
    unsigned long long *presence = W.layers, *visits = W.layers + G, *dwell = W.layers + 2 * G, *flow_x = W.layers + 3 * G,
                       *flow_y = W.layers + 4 * G;
    int n = *T.count;
    for (int f = W.f0; f < W.f1; ++f) {
        const HeatFrameDev F = frames[f];
        int R = stage_frame_rows(F.rows, F.n_p, F.n, W.srows);
        __syncthreads();
        // ---- rows of another class are ignored entirely: the others move up, order kept (a chunk of 256 rows is read into
        //      registers before the barrier inside compact_ordered, and a row never moves to a higher index)
        if (W.cls != -1) {
            int r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0;
            R = compact_ordered(R, s_cnt, [&](int j) {
                const int *r = W.srows + j * 6;
                r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3]; r4 = r[4]; r5 = r[5];
                return r5 == W.cls;
            }, [&](int, int k) {
                int *d = W.srows + k * 6;
                d[0] = r0; d[1] = r1; d[2] = r2; d[3] = r3; d[4] = r4; d[5] = r5;
            });
            __syncthreads();
        }
        // ---- rows whose id is unknown are registered at the end of the table in row order, outside every cell until handled below
        const int n_all = register_unknown(R, n, cap, s_cnt, T.id, W.srows, [&](int e, const int *r) { T.id[e] = r[4]; T.age[e] = 0; T.cell[e] = -1; });
        __syncthreads();
        // ---- entries in table order, a thread each
        int dead = 0;
        for (int base = 0; base < n_all; base += 256) {
            const int e = base + tid;
            bool gone = false;
            if (e < n_all) {
                const int j = find_row(W.srows, R, T.id[e]);
                if (j == R) {                                                     // unseen: ages
                    const int a = T.age[e] + 1;
                    T.age[e] = a;
                    gone = a > max_age;
                } else {
                    const int *r = W.srows + j * 6;
                    const int X = heat_clamp((long long)r[0] + (long long)r[2]), Y = heat_clamp(2ll * (long long)r[3]);
                    const int cx = X >> W.shift, cy = Y >> W.shift;               // floor division: the shift of a negative int is arithmetic
                    const int cell = cx >= 0 && cx < W.gw && cy >= 0 && cy < W.gh ? cy * W.gw + cx : -1;
                    if (e < n) {                                                  // a known id
                        const int prev = T.cell[e];
                        if (T.age[e] == 0) {                                      // seen in the previous processed frame: a gap credits nothing
                            if (prev >= 0) {
                                const double us = (F.t - T.pt[e]) * 1e6;
                                const long long q = llrint(us);                   // half to even
                                if (q > 0) atomicAdd(dwell + prev, (unsigned long long)q);
                            }
                            if (cell >= 0) {
                                atomicAdd(flow_x + cell, (unsigned long long)(long long)(X - T.px[e]));
                                atomicAdd(flow_y + cell, (unsigned long long)(long long)(Y - T.py[e]));
                            }
                        }
                        if (cell >= 0 && cell != prev) atomicAdd(visits + cell, 1ull);
                    } else if (cell >= 0) {
                        atomicAdd(visits + cell, 1ull);
                    }
                    if (cell >= 0) atomicAdd(presence + cell, 1ull);
                    T.age[e] = 0; T.cell[e] = cell; T.px[e] = X; T.py[e] = Y; T.pt[e] = F.t;
                }
            }
            dead += __syncthreads_count(gone);
        }
        if (tid == 0) res[F.res_n] = R;
        // ---- entries older than max_age leave, the rest keep their order
        int n_live = n_all;
        if (dead) {
            auto move = [&](int d, int e) {
                T.id[d] = T.id[e]; T.age[d] = T.age[e]; T.cell[d] = T.cell[e]; T.px[d] = T.px[e]; T.py[d] = T.py[e]; T.pt[d] = T.pt[e];
            };
            n_live = retire(n_all, cap, s_cnt, [&](int e) { return T.age[e] <= max_age; }, move, move);
        }
        n = n_live;
        __syncthreads();
    }
    if (tid == 0) { *T.count = n; res[W.res_count] = n; }
}

// ------------------------------------------------------------------------------------------------------------------ render
// (HeatLevelJob - one stream named in a render call, or asked for its maximum - the byte blend and a thread's whole-pixel accesses:
// heat_render.h, shared with the ground plane's renders)
// res[job] = the layer's maximum; *bad = 1 when the vmax to use exceeds the limit (the levels are then not written and the render
// kernel touches nothing)
__global__ __launch_bounds__(256) void heat_levels_kernel(const HeatLevelJob *jobs, long long *res, int *bad) {
    __shared__ long long s_m[256];
    const HeatLevelJob J = jobs[blockIdx.x];
    const int tid = threadIdx.x;
    long long m = LLONG_MIN;
    for (int k = tid; k < J.n; k += 256) m = max(m, J.layer[k]);
    s_m[tid] = m;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) s_m[tid] = max(s_m[tid], s_m[tid + d]);
        __syncthreads();
    }
    m = s_m[0];
    if (tid == 0) res[blockIdx.x] = m;
    if (!J.level) return;
    const long long vmax = J.vmax ? J.vmax : max(m, 1ll);
    if (vmax > HEAT_VMAX_LIMIT) {
        if (tid == 0) *bad = 1;
        return;
    }
    for (int k = tid; k < J.n; k += 256) {
        const long long v = min(max(J.layer[k], 0ll), vmax);
        J.level[k] = (uint16_t)((unsigned long long)v * 65535ull / (unsigned long long)vmax);
    }
}

// PX pixels of one row per thread: 16 (uint4 accesses), 4 (dwords) or 1 (bytes)
template <int PX> __global__ __launch_bounds__(256) void heat_render_kernel(HeatRenderArgs a) {
    __shared__ uint32_t s_lut[256];
    if (*a.bad) return;
    s_lut[threadIdx.x] = a.lut[threadIdx.x];
    __syncthreads();
    const int2 fj = a.fjobs[blockIdx.y];
    const HeatLevelJob J = a.jobs[fj.y];
    const unsigned per_row = (unsigned)a.w / PX, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= per_row * (unsigned)a.h) return;
    const int y = (int)(idx / per_row), x0 = (int)(idx - (unsigned)y * per_row) * PX;
    uint8_t *p = a.frames + (size_t)fj.x * a.frame_bytes + ((size_t)y * a.w + x0) * 3;
    uint32_t word[HeatWords<PX>::N];
    heat_load_px<PX>(p, word);
    // the field: k = num / (4 c^2 * 257), num = (2c - fx) * Va + fx * Vb, Va / Vb = the two level columns at this row's fy
    const int lc = J.lc, c = 1 << lc, c2 = 2 * c;
    const int V = 2 * y + 1 - c, j0 = V >> (lc + 1);
    const uint32_t fy = (uint32_t)(V & (c2 - 1));
    const uint16_t *La = J.level + (size_t)min(max(j0, 0), J.gh - 1) * J.gw, *Lb = J.level + (size_t)min(max(j0 + 1, 0), J.gh - 1) * J.gw;
    uint32_t Va = 0, Vb = 0, col[PX], any = 0;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        const int U = 2 * (x0 + i) + 1 - c;
        const uint32_t fx = (uint32_t)(U & (c2 - 1));
        if (i == 0 || fx == 1u) {                                                 // the first pixel past a cell centre: the next pair of columns
            const int i0 = U >> (lc + 1), ia = min(max(i0, 0), J.gw - 1), ib = min(max(i0 + 1, 0), J.gw - 1);
            Va = ((uint32_t)c2 - fy) * La[ia] + fy * Lb[ia];
            Vb = ((uint32_t)c2 - fy) * La[ib] + fy * Lb[ib];
        }
        const uint32_t num = ((uint32_t)c2 - fx) * Va + fx * Vb;
        const uint32_t k = (num >> (2 * lc + 2)) / 257u;
        col[i] = k ? s_lut[k] | 0xff000000u : 0u;                                 // bits 24..31: the pixel takes part
        any |= k;
    }
    if (!any) return;                                                             // empty areas keep the picture, and cost no store
    heat_blend_store_px<PX>(p, word, col, a.alpha, 256u - a.alpha);
}

void heat_launch_levels(const HeatLevelJob *jobs_dev, int n_jobs, long long *res, int *bad, hipStream_t s) {
    hipLaunchKernelGGL(heat_levels_kernel, dim3(n_jobs), dim3(256), 0, s, jobs_dev, res, bad);
}

void heat_launch_render(const HeatRenderArgs &a, int n, hipStream_t s) {
    const int px = heat_px_per_thread(a.frames, a.w);
    const size_t threads = (size_t)a.h * (a.w / px);
    if ((threads + 255) / 256 > 0x7fffffffull) fail("heatmap: frames of %d x %d are too large for one launch", a.h, a.w);
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)n);
    if (px == 16) hipLaunchKernelGGL(heat_render_kernel<16>, grid, dim3(256), 0, s, a);
    else if (px == 4) hipLaunchKernelGGL(heat_render_kernel<4>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(heat_render_kernel<1>, grid, dim3(256), 0, s, a);
}

class Heatmap : public TrackStage<HeatmapIface> {
public:
    Heatmap(int S, int max_age) : TrackStage("heatmap", S), max_age(max_age), tabs(S), grids(S) {
        if (max_age < 1) fail("heatmap: max_age %d < 1", max_age);
        bad.alloc(1);
    }

    struct Tab {
        DevBuf<int> ints;         // id | age | cell | px | py, [2][cap] each
        DevBuf<double> pt;
        int cap = 0;
    };
    struct Grid {                 // the spec of a stream and what hangs on it; cell == 0: no spec yet
        int h = 0, w = 0, cell = 0, cls = 0, gw = 0, gh = 0, lc = 0;
        DevBuf<long long> layers;
        DevBuf<uint16_t> level;
        size_t cells() const { return (size_t)gw * gh; }
    };
    HeatTab dev_tab(int s) {
        Tab &t = tabs[s];
        const size_t c2 = 2 * (size_t)t.cap;
        return HeatTab{t.ints.p, t.ints.p + c2, t.ints.p + 2 * c2, t.ints.p + 3 * c2, t.ints.p + 4 * c2, t.pt.p, counts.p + s, t.cap};
    }
    void grow(int s, int need) {
        const size_t n = count_host[s];
        grow_table(tabs[s], need, n, [&](Tab &nt) {
            nt.ints.alloc(10 * (size_t)nt.cap);
            nt.pt.alloc(2 * (size_t)nt.cap);
        }, [&](Tab &nt, const Tab &t) {
            copy_live(nt.ints, t.ints, n, 5, nt.cap, t.cap);
            copy_live(nt.pt, t.pt, n);
        });
    }
    void check_for(int n_streams, const char *noun) const override {
        HeatmapIface::check_for(n_streams, noun);
        for (int s = 0; s < n_streams; ++s)
            if (grids[s].cell == 0) fail("pipeline: stream %d of the heatmap handle has no spec (yds_heatmap_set_stream)", s);
    }
    const Grid &grid_of(int stream) const {
        check_stream(stream);
        if (!grids[stream].cell) fail("heatmap: stream %d has no spec (yds_heatmap_set_stream)", stream);
        return grids[stream];
    }

    void set_stream(int stream, int h, int w, int cell, int cls) {
        check_stream(stream);
        if (h < 1 || w < 1) fail("heatmap: a frame of %d x %d", h, w);
        int lc = 0;
        while ((1 << lc) < cell && lc < 8) ++lc;
        if (cell < 4 || cell > 128 || (1 << lc) != cell) fail("heatmap: cell %d is not one of 4, 8, 16, 32, 64, 128", cell);
        if (cls < -1) fail("heatmap: class_id %d (-1 = any class)", cls);
        const long long gw = ((long long)w + cell - 1) / cell, gh = ((long long)h + cell - 1) / cell;
        if (gw * gh > YDS_HEATMAP_MAX_CELLS) fail("heatmap: a grid of %lld x %lld cells exceeds %d", gh, gw, YDS_HEATMAP_MAX_CELLS);
        Grid g;
        g.h = h; g.w = w; g.cell = cell; g.cls = cls; g.gw = (int)gw; g.gh = (int)gh; g.lc = lc;
        g.layers.alloc(N_LAYERS * g.cells());
        g.level.alloc(g.cells());
        grids[stream] = std::move(g);
        reset(stream);
    }

    // zero layers and an empty table for one stream, or all (-1)
    void reset(int stream) {
        TrackStage::reset(stream);
        for (int s = 0; s < S; ++s) {
            if ((stream >= 0 && s != stream) || !grids[s].cell) continue;
            YDS_HIP(hipMemset(grids[s].layers.p, 0, N_LAYERS * grids[s].cells() * sizeof(long long)));
        }
    }

    void enqueue(const ActFrame *fr, int n, hipStream_t s) override { enqueue_ex(fr, n, s, nullptr, 0); }

    // rows_host (the stand-alone entry): a host array that travels to the device inside the call's input block (open_blocks)
    void enqueue_ex(const ActFrame *fr, int n, hipStream_t s, const int32_t *rows_host, size_t n_rows_host) {
        for (int i = 0; i < n; ++i)
            if (fr[i].stream >= 0 && fr[i].stream < S && !grids[fr[i].stream].cell)
                fail("heatmap: frame %d names stream %d, which has no spec (yds_heatmap_set_stream)", i, fr[i].stream);
        const StagePlan P = plan(fr, n, [&](int st, int need) { grow(st, need); });
        if (!P.n_wg) return;
        pending_cap.resize(n);
        for (int i = 0; i < n; ++i) pending_cap[i] = fr[i].n_rows;
        // ---- blocks: input = works | frames | rows; results = counted rows of every frame | entry counts
        const size_t works_b = (size_t)P.n_wg * sizeof(HeatWork);
        open_blocks(P, works_b + (size_t)n * sizeof(HeatFrameDev), rows_host, n_rows_host, (size_t)n + P.n_wg);
        HeatWork *w = reinterpret_cast<HeatWork *>(in_host.p);
        HeatFrameDev *fd = reinterpret_cast<HeatFrameDev *>(in_host.p + works_b);
        for (int k = 0; k < P.n_wg; ++k) {
            const int st = wg_stream[k];
            const Grid &g = grids[st];
            w[k] = HeatWork{dev_tab(st), reinterpret_cast<unsigned long long *>(g.layers.p), g.gw, g.gh, g.lc + 1, g.cls, P.start[st],
                            P.start[st] + P.n_of[st], wg_srows(k), n + k};
        }
        for (int e = 0; e < n; ++e) {
            const ActFrame &f = fr[P.order[e]];
            HeatFrameDev d;
            d.rows = dev_rows(f);
            d.n_p = f.n_rows_p;
            d.t = f.t; d.n = f.n_rows;
            d.res_n = P.order[e];
            fd[e] = d;
        }
        submit(s, [&] {
            hipLaunchKernelGGL(heat_update_kernel, dim3(P.n_wg), dim3(256), 0, s, reinterpret_cast<const HeatWork *>(in_dev.p),
                               reinterpret_cast<const HeatFrameDev *>(in_dev.p + works_b), max_age, res_host.p);
        });
    }

    void collect() override {
        counted.clear();
        collect_counts("counted rows", [&](int, int m) { counted.push_back(m); });
    }

    // the maximum of one layer of one stream, reduced on the device (the levels kernel without levels)
    long long layer_max(int stream, int layer) {
        const Grid &g = grid_of(stream);
        if (layer < 0 || layer >= N_LAYERS) fail("heatmap: layer %d outside [0,%d)", layer, N_LAYERS);
        open_render(1, 0);
        jobs_host()[0] = HeatLevelJob{g.layers.p + (size_t)layer * g.cells(), nullptr, 0, (int)g.cells(), g.gw, g.gh, g.lc};
        YDS_HIP(hipMemcpyAsync(r_in_dev.p, r_in_host.p, sizeof(HeatLevelJob), hipMemcpyHostToDevice, own_stream));
        heat_launch_levels(reinterpret_cast<const HeatLevelJob *>(r_in_dev.p), 1, r_res.p, bad.p, own_stream);
        YDS_HIP(hipGetLastError());
        YDS_HIP(hipStreamSynchronize(own_stream));
        return r_res.p[0];
    }

    // the input block of a render call: jobs | (slot, job) of every frame | LUT
    void open_render(int n_jobs, int n_frames) {
        r_jobs_b = (size_t)n_jobs * sizeof(HeatLevelJob);
        r_fj_b = (size_t)n_frames * sizeof(int2);
        const size_t total = r_jobs_b + r_fj_b + 256 * sizeof(uint32_t);
        if (total > r_in_host.n) { r_in_host.ensure(total * 2); r_in_dev.alloc(r_in_host.n); }
        r_res.ensure((size_t)std::max(n_jobs, 1));
    }
    HeatLevelJob *jobs_host() { return reinterpret_cast<HeatLevelJob *>(r_in_host.p); }

    void render(uint8_t *frames, int n_src, const int32_t *slot, const int32_t *stream_of, int n, int h, int w, int layer, long long vmax, int alpha,
                const uint8_t *lut) {
        if (n <= 0) return;
        if (!frames || !slot || !stream_of || !lut || n_src < 1) fail("heatmap: NULL argument");
        if (h < 1 || w < 1) fail("heatmap: frames of %d x %d", h, w);
        if (layer < 0 || layer >= N_RENDERABLE) fail("heatmap: layer %d is not renderable (0 presence, 1 visits, 2 dwell_us)", layer);
        if (vmax < 0 || vmax > HEAT_VMAX_LIMIT) fail("heatmap: vmax %lld outside [1, 2^47] (0 = the layer's maximum)", vmax);
        if (alpha < 1 || alpha > 256) fail("heatmap: alpha %d outside [1, 256]", alpha);
        std::vector<int> sorted(slot, slot + n), job_of(S, -1), job_stream;
        for (int i = 0; i < n; ++i)
            if (slot[i] < 0 || slot[i] >= n_src) fail("heatmap: frame %d names slot %d of %d frames", i, slot[i], n_src);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 1; i < n; ++i)
            if (sorted[i] == sorted[i - 1]) fail("heatmap: two frames name the same slot %d", sorted[i]);
        for (int i = 0; i < n; ++i) {
            const Grid &g = grid_of(stream_of[i]);
            if (g.h != h || g.w != w) fail("heatmap: frames of %d x %d for stream %d, whose spec is %d x %d", h, w, stream_of[i], g.h, g.w);
            if (job_of[stream_of[i]] < 0) { job_of[stream_of[i]] = (int)job_stream.size(); job_stream.push_back(stream_of[i]); }
        }
        const int n_jobs = (int)job_stream.size();
        open_render(n_jobs, n);
        HeatLevelJob *jobs = jobs_host();
        int2 *fj = reinterpret_cast<int2 *>(r_in_host.p + r_jobs_b);
        uint32_t *lut32 = reinterpret_cast<uint32_t *>(r_in_host.p + r_jobs_b + r_fj_b);
        for (int k = 0; k < n_jobs; ++k) {
            Grid &g = grids[job_stream[k]];
            jobs[k] = HeatLevelJob{g.layers.p + (size_t)layer * g.cells(), g.level.p, vmax, (int)g.cells(), g.gw, g.gh, g.lc};
        }
        for (int i = 0; i < n; ++i) fj[i] = make_int2(slot[i], job_of[stream_of[i]]);
        heat_pack_lut(lut32, lut);
        const hipStream_t s = own_stream;
        const size_t in_bytes = r_jobs_b + r_fj_b + 256 * sizeof(uint32_t);
        YDS_HIP(hipMemcpyAsync(r_in_dev.p, r_in_host.p, in_bytes, hipMemcpyHostToDevice, s));
        YDS_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), s));
        HeatRenderArgs a{frames, (size_t)h * w * 3, reinterpret_cast<const int2 *>(r_in_dev.p + r_jobs_b),
                         reinterpret_cast<const HeatLevelJob *>(r_in_dev.p), reinterpret_cast<const uint32_t *>(r_in_dev.p + r_jobs_b + r_fj_b),
                         bad.p, h, w, (uint32_t)alpha};
        render_timer.begin(s);
        heat_launch_levels(a.jobs, n_jobs, r_res.p, bad.p, s);
        heat_launch_render(a, n, s);
        YDS_HIP(hipGetLastError());
        render_timer.end(s);
        YDS_HIP(hipStreamSynchronize(s));
        if (!vmax)
            for (int k = 0; k < n_jobs; ++k)
                if (r_res.p[k] > HEAT_VMAX_LIMIT)
                    fail("heatmap: vmax 0 and the layer's maximum %lld of stream %d exceeds 2^47: nothing was rendered", r_res.p[k], job_stream[k]);
    }

    int max_age;
    std::vector<Tab> tabs;
    std::vector<Grid> grids;
    DevBuf<int> bad;
    DevBuf<char> r_in_dev;
    PinBuf<char> r_in_host;
    PinBuf<long long> r_res;
    size_t r_jobs_b = 0, r_fj_b = 0;
    LaunchTimer render_timer;
};

}  // namespace yds

static inline yds::Heatmap *impl(yds_heatmap *h) {
    if (!h) yds::fail("heatmap: NULL handle");
    return static_cast<yds::Heatmap *>(h->h);
}

extern "C" {

yds_heatmap *yds_heatmap_create(int n_streams, int max_age) {
    YDS_API_BEGIN
    return new yds_heatmap{new yds::Heatmap(n_streams, max_age)};
    YDS_API_END_PTR
}
void yds_heatmap_destroy(yds_heatmap *h) {
    if (h) { delete h->h; delete h; }
}
int yds_heatmap_set_stream(yds_heatmap *h, int stream, int height, int width, int cell, int class_id) {
    YDS_API_BEGIN
    impl(h)->set_stream(stream, height, width, cell, class_id);
    YDS_API_END
}
int yds_heatmap_reset(yds_heatmap *h, int stream) {
    YDS_API_BEGIN
    impl(h)->reset(stream);
    YDS_API_END
}
int yds_heatmap_update(yds_heatmap *h, const int32_t *rows6_host, const int32_t *first, const int32_t *stream_of, const double *frame_time,
                       int n_frames, int32_t *counted_out) {
    YDS_API_BEGIN
    yds::Heatmap *H = impl(h);
    const std::vector<yds::ActFrame> fr = yds::csr_frames("heatmap", rows6_host, first, stream_of, frame_time, false, n_frames, nullptr);
    if (fr.empty()) return 0;
    H->enqueue_ex(fr.data(), n_frames, H->own_stream, rows6_host, (size_t)first[n_frames]);
    H->finish_alone();
    if (counted_out) memcpy(counted_out, H->counted.data(), (size_t)n_frames * sizeof(int32_t));
    YDS_API_END
}
int yds_heatmap_get_layers(yds_heatmap *h, int stream, int64_t *out5, size_t cap) {
    YDS_API_BEGIN
    yds::Heatmap *H = impl(h);
    const yds::Heatmap::Grid &g = H->grid_of(stream);
    const size_t m = yds::N_LAYERS * g.cells();
    if (m > cap) yds::fail("heatmap: %zu layer values exceed the caller's capacity %zu", m, cap);
    if (!out5) yds::fail("heatmap: NULL argument");
    YDS_HIP(hipMemcpy(out5, g.layers.p, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    YDS_API_END
}
int yds_heatmap_get_max(yds_heatmap *h, int stream, int layer, int64_t *out) {
    YDS_API_BEGIN
    if (!out) yds::fail("heatmap: NULL argument");
    *out = impl(h)->layer_max(stream, layer);
    YDS_API_END
}
int yds_heatmap_get_tracks(yds_heatmap *h, int stream, int32_t *ids, int32_t *ages, int32_t *cells, int32_t *xy2, double *t, int cap, int *n) {
    YDS_API_BEGIN
    yds::Heatmap *H = impl(h);
    const int m = H->table_count(stream, "tracks", cap, n);
    const yds::HeatTab tb = H->dev_tab(stream);
    H->column_out(ids, tb.id, m);
    H->column_out(ages, tb.age, m);
    H->column_out(cells, tb.cell, m);
    if (xy2 && m) {
        std::vector<int32_t> x(m), y(m);
        H->column_out(x.data(), tb.px, m);
        H->column_out(y.data(), tb.py, m);
        for (int k = 0; k < m; ++k) { xy2[2 * k] = x[k]; xy2[2 * k + 1] = y[k]; }
    }
    if (t && m) YDS_HIP(hipMemcpy(t, tb.pt, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    YDS_API_END
}
int yds_heatmap_render(yds_heatmap *h, uint8_t *frames_dev, int n_src, const int32_t *slot_host, const int32_t *stream_of_host, int n, int height,
                       int width, int layer, int64_t vmax, int alpha, const uint8_t *lut_host) {
    YDS_API_BEGIN
    impl(h)->render(frames_dev, n_src, slot_host, stream_of_host, n, height, width, layer, vmax, alpha, lut_host);
    YDS_API_END
}
int yds_heatmap_set_timing(yds_heatmap *h, int on) {
    YDS_API_BEGIN
    impl(h)->timer.set(on != 0);
    impl(h)->render_timer.set(on != 0);
    YDS_API_END
}
int yds_heatmap_last_us(yds_heatmap *h, int what, float *us) {
    YDS_API_BEGIN
    if (what != 0 && what != 1) yds::fail("heatmap: last_us of %d (0 = the update launch, 1 = the render)", what);
    *us = what ? impl(h)->render_timer.us("heatmap") : impl(h)->timer.us("heatmap");
    YDS_API_END
}

}  // extern "C"
