// Ground plane on the device: every camera's tracker rows taken through that camera's homography onto ONE floor plan - plan positions,
// speeds and distances per track, one site-wide grid of five int64 layers in HBM for all streams, and two renders of a site layer:
// onto a plan canvas and, perspective-correct, onto the floor of camera frames resident in HBM.  Built on the frame the per-stream
// table stages share (track_stage.h) and modelled on heatmap.hip.
//
// There is no reference counterpart; the rules are written down in include/ydsort.h (the ground plane block) and restated in Python
// ints / numpy float64 by yolo_deepsort_amd/ground.py (GroundMap, render_view), which every device test compares against with exact
// equality.  The one floating-point step is ground_project: nine double multiplies and adds in a fixed order, two divisions, two
// products and two roundings half to even per point - the tree is built with -ffp-contract=off and without fast-math, so each is the
// correctly rounded IEEE operation numpy performs.  Every point evaluates the full expression (X(u + 1) != X(u) + H00 in floating
// point); everything after it is integer arithmetic.
//
// Update.  One workgroup per stream that has frames in the call walks that stream's frames in time order, as the heat map stage
// does: stage the rows, drop the rows of another class, register unknown ids, then a thread per entry.  An entry keeps age, cell, the
// time of its last sighting, the distance travelled and a ring of its last K on-plane sightings (qx, qy, t) - an array per entry like
// the orbit caches of actions.hip.  Workgroups of different streams add to the same cells of the one site grid, so every layer update
// is a 64-bit integer atomic: integer sums do not depend on the order.  Per counted row one int32[8] record goes straight into the
// pinned result block.
//
// Renders.  render_plan is the heat map's render of a foreign layer pointer (heat_render.h): levels, then heat_render_kernel on a
// canvas of cell_px pixels per cell.  render_view: levels per cell by the same levels kernel, then ground_view_kernel streams the named
// frames - a thread owns PX consecutive pixels of a row (16, 4 or 1 by base and width, as heat_render_kernel), projects each pixel
// centre by ground_project with the frame's own H (a per-frame table), interpolates the four surrounding levels with 8-bit weights in
// 32-bit integers, and reads and writes the pixels only where one of them changes: rows above the horizon cost no memory traffic.
#include "heat_render.h"
#include "track_stage.h"
#include "ydsort.h"

#include <algorithm>
#include <math.h>

namespace yds {

constexpr int GROUND_LAYERS = 5, GROUND_RENDERABLE = 3;
constexpr long long GROUND_VMAX_LIMIT = YDS_HEATMAP_VMAX_LIMIT;

// the plan all streams of a handle share
struct GroundPlanDev {
    unsigned long long *layers;                   // [5][gh * gw] two's complement sums
    double scale;                                 // quanta per plan unit
    int ox_q, oy_q, cell_q, gw, gh, K;            // origin and cell edge in quanta; K = speed_window
};
// table of one stream: `cap` entries, every field twice (the second copy takes the survivors of a removal)
struct GroundTab {
    int *id, *age, *cell, *len, *head;            // [2][cap] each
    int *rxy;                                     // [2][cap][K][2]  ring of plan positions in quanta
    double *rt;                                   // [2][cap][K]     ... and their times
    double *tl;                                   // [2][cap]        time of the last sighting (on or off the plane)
    long long *trav;                              // [2][cap]        quanta travelled
    int *count;                                   // live entries (device)
    int cap;
};
struct GroundWork {
    GroundTab tab;
    double H[9];                                  // image to plan units, row-major
    int cls, skip;                                // skip: the stream has no spec - its frames report nothing and touch nothing
    int f0, f1;                                   // frames [f0, f1) of the call's frame list (sorted by stream, order kept)
    int *srows;                                   // staging [max rows of a frame][6]
    int res_count;                                // int index in the result block of this stream's entry count
};
struct GroundFrameDev {
    const int *rows;
    const int *n_p;
    double t;
    int n;
    int res_n;                                    // int index in the result block of this frame's counted-row count
    int res_rows;                                 // ... of its records [n][8]
};

// Rule 2, the one floating-point step: false = off plane.
__device__ __forceinline__ bool ground_project(const double *H, double u, double v, double scale, int &qx, int &qy) {
    const double X = (H[0] * u + H[1] * v) + H[2];
    const double Y = (H[3] * u + H[4] * v) + H[5];
    const double W = (H[6] * u + H[7] * v) + H[8];
    if (!(W > 0.0) || !(W <= 1.7976931348623157e308)) return false;
    const double px = X / W, py = Y / W;
    const double sx = px * scale, sy = py * scale;
    // (a NaN or an infinity anywhere above ends in a NaN or an infinity here)
    if (!(fabs(sx) <= 536870912.0) || !(fabs(sy) <= 536870912.0)) return false;
    qx = (int)llrint(sx);                         // half to even
    qy = (int)llrint(sy);
    return true;
}

__device__ __forceinline__ long long ground_floor_div(long long a, long long b) {       // b > 0
    long long q = a / b;
    if (a % b < 0) --q;
    return q;
}
// exact integer square root of n < 2^63
__device__ __forceinline__ long long ground_isqrt(long long n) {
    long long r = (long long)sqrt((double)n);
    while (r * r > n) --r;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}
__device__ __forceinline__ int ground_sat(long long v) {
    return (int)(v < -(long long)INT_MAX ? -(long long)INT_MAX : v > (long long)INT_MAX ? (long long)INT_MAX : v);
}

__global__ __launch_bounds__(256) void ground_update_kernel(const GroundWork *works, const GroundFrameDev *frames, GroundPlanDev P, int max_age,
                                                            int *res) {
    __shared__ int s_cnt[4];
    __shared__ double s_H[9];
    const GroundWork &Wg = works[blockIdx.x];
    const GroundTab T = Wg.tab;
    const int tid = threadIdx.x, cap = T.cap, K = P.K;
    const int f0 = Wg.f0, f1 = Wg.f1, cls = Wg.cls, res_count = Wg.res_count;
    int *const srows = Wg.srows;
    if (Wg.skip) {
        if (tid == 0) {
            for (int f = f0; f < f1; ++f) res[frames[f].res_n] = 0;
            res[res_count] = 0;
        }
        return;
    }
    if (tid < 9) s_H[tid] = Wg.H[tid];
    const size_t G = (size_t)P.gw * P.gh;
    unsigned long long *presence = P.layers, *visits = P.layers + G, *dwell = P.layers + 2 * G, *flow_x = P.layers + 3 * G,
                       *flow_y = P.layers + 4 * G;
    int n = *T.count;
    __syncthreads();
    for (int f = f0; f < f1; ++f) {
        const GroundFrameDev F = frames[f];
        int R = stage_frame_rows(F.rows, F.n_p, F.n, srows);
        __syncthreads();
        // ---- rows of another class are ignored entirely: the others move up, order kept
        if (cls != -1) {
            int r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0;
            R = compact_ordered(R, s_cnt, [&](int j) {
                const int *r = srows + j * 6;
                r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3]; r4 = r[4]; r5 = r[5];
                return r5 == cls;
            }, [&](int, int k) {
                int *d = srows + k * 6;
                d[0] = r0; d[1] = r1; d[2] = r2; d[3] = r3; d[4] = r4; d[5] = r5;
            });
            __syncthreads();
        }
        // ---- unknown ids are registered at the end of the table in row order: no cell, an empty ring, nothing travelled
        const int n_all = register_unknown(R, n, cap, s_cnt, T.id, srows, [&](int e, const int *r) {
            T.id[e] = r[4]; T.age[e] = 0; T.cell[e] = -1; T.len[e] = 0; T.head[e] = 0; T.trav[e] = 0; T.tl[e] = F.t;
        });
        __syncthreads();
        // ---- entries in table order, a thread each
        int *out = res + F.res_rows;
        int dead = 0;
        for (int base = 0; base < n_all; base += 256) {
            const int e = base + tid;
            bool gone = false;
            if (e < n_all) {
                const int j = find_row(srows, R, T.id[e]);
                if (j == R) {                                                     // unseen: ages
                    const int a = T.age[e] + 1;
                    T.age[e] = a;
                    gone = a > max_age;
                } else {
                    const int *r = srows + j * 6;
                    const double u = 0.5 * ((double)r[0] + (double)r[2]), v = (double)r[3];
                    int qx = 0, qy = 0, cell = -2;
                    const bool on = ground_project(s_H, u, v, P.scale, qx, qy);
                    if (on) {
                        const long long cx = ground_floor_div((long long)qx - P.ox_q, P.cell_q), cy = ground_floor_div((long long)qy - P.oy_q, P.cell_q);
                        cell = cx >= 0 && cx < P.gw && cy >= 0 && cy < P.gh ? (int)(cy * P.gw + cx) : -1;
                    }
                    const bool fresh = T.age[e] == 0;                             // seen in the previous processed frame (or new: an empty ring)
                    const int prev = T.cell[e];
                    int len = T.len[e], head = T.head[e], vx = 0, vy = 0, speed = 0;
                    if (fresh && prev >= 0) {                                     // a gap credits nothing
                        const long long q = llrint((F.t - T.tl[e]) * 1e6);        // half to even
                        if (q > 0) atomicAdd(dwell + prev, (unsigned long long)q);
                    }
                    if (on) {
                        int *ring = T.rxy + (size_t)e * K * 2;
                        double *rt = T.rt + (size_t)e * K;
                        if (fresh && len > 0) {                                   // a sighting after a sighting: the step counts
                            int last = head + len - 1;
                            if (last >= K) last -= K;
                            const long long dx = (long long)qx - ring[2 * last], dy = (long long)qy - ring[2 * last + 1];
                            T.trav[e] += ground_isqrt(dx * dx + dy * dy);
                            if (cell >= 0) {
                                atomicAdd(flow_x + cell, (unsigned long long)dx);
                                atomicAdd(flow_y + cell, (unsigned long long)dy);
                            }
                        } else {                                                  // after a gap or an off-plane point: the ring restarts
                            len = 0; head = 0;
                        }
                        int pos;
                        if (len < K) { pos = head + len; if (pos >= K) pos -= K; ++len; }
                        else { pos = head; head = head + 1 == K ? 0 : head + 1; }
                        ring[2 * pos] = qx; ring[2 * pos + 1] = qy; rt[pos] = F.t;
                        const long long dx = (long long)qx - ring[2 * head], dy = (long long)qy - ring[2 * head + 1];
                        const long long dt_us = llrint((F.t - rt[head]) * 1e6);
                        if (dt_us > 0) {
                            vx = ground_sat(ground_floor_div(dx * 1000000ll, dt_us));
                            vy = ground_sat(ground_floor_div(dy * 1000000ll, dt_us));
                            speed = ground_sat(ground_isqrt(dx * dx + dy * dy) * 1000000ll / dt_us);
                        } else {
                            speed = -1;
                        }
                        if (cell >= 0) {
                            if (cell != prev) atomicAdd(visits + cell, 1ull);
                            atomicAdd(presence + cell, 1ull);
                        }
                    } else {
                        len = 0; head = 0;
                    }
                    T.age[e] = 0; T.cell[e] = cell; T.len[e] = len; T.head[e] = head; T.tl[e] = F.t;
                    int *o = out + (size_t)j * 8;
                    o[0] = r[4]; o[1] = r[5]; o[2] = qx; o[3] = qy; o[4] = vx; o[5] = vy; o[6] = speed; o[7] = cell;
                }
            }
            dead += __syncthreads_count(gone);
        }
        if (tid == 0) res[F.res_n] = R;
        // ---- entries older than max_age leave, the rest keep their order
        int n_live = n_all;
        if (dead) {
            auto move = [&](int d, int e) {
                T.id[d] = T.id[e]; T.age[d] = T.age[e]; T.cell[d] = T.cell[e]; T.len[d] = T.len[e]; T.head[d] = T.head[e]; T.tl[d] = T.tl[e];
                T.trav[d] = T.trav[e];
            };
            n_live = retire(n_all, cap, s_cnt, [&](int e) { return T.age[e] <= max_age; }, [&](int d, int e) {
                move(d, e);
                for (int k = 0; k < 2 * K; ++k) T.rxy[(size_t)d * K * 2 + k] = T.rxy[(size_t)e * K * 2 + k];
                for (int k = 0; k < K; ++k) T.rt[(size_t)d * K + k] = T.rt[(size_t)e * K + k];
            }, move);
            for (size_t k = tid; k < (size_t)n_live * K * 2; k += 256) T.rxy[k] = T.rxy[(size_t)cap * K * 2 + k];
            for (size_t k = tid; k < (size_t)n_live * K; k += 256) T.rt[k] = T.rt[(size_t)cap * K + k];
        }
        n = n_live;
        __syncthreads();
    }
    if (tid == 0) { *T.count = n; res[res_count] = n; }
}

// ------------------------------------------------------------------------------------------------------------------ render_view
struct GroundViewFrame {
    double H[9];
    long long slot;
};
struct GroundViewArgs {
    uint8_t *frames;
    size_t frame_bytes;
    const GroundViewFrame *vf;                    // per frame of the call
    const uint16_t *level;                        // [gh * gw]
    const uint32_t *lut;                          // [256] byte 0 | byte 1 << 8 | byte 2 << 16
    const int *bad;
    double scale;
    int h, w, ox_q, oy_q, cell_q, gw, gh;
    uint32_t alpha;
};

// One axis of rule 4: the lower cell index and the 8-bit weight of the upper one for plan coordinate q; false where the pixel keeps
// the picture (i0 < -1 or i0 >= g).  e = q - o + cell >= 0 shifts the floor division to unsigned 32-bit: the spec bounds
// (g + 2) * cell_q by 2^22, so e * 256 < 2^30.
__device__ __forceinline__ bool ground_axis(int q, int o_q, int cell_q, int g, int &i0, uint32_t &f) {
    const long long e = (long long)q - o_q + cell_q;
    if (e < 0 || e >= (long long)(g + 2) * cell_q) return false;
    const int a = (int)(((uint32_t)e * 256u) / (uint32_t)cell_q) - 384;           // = ((q - o) * 256) // cell_q - 128
    i0 = a >> 8;
    f = (uint32_t)(a & 255);
    return i0 >= -1 && i0 < g;
}

// (the occupancy hint: left alone the compiler interleaves the 16 projections of a thread into 252 VGPRs, one wave per SIMD, and the
// division chains then have nothing to hide behind; held to 8 waves it finds 64 VGPRs without scratch)
template <int PX> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void ground_view_kernel(GroundViewArgs a) {
    __shared__ uint32_t s_lut[256];
    __shared__ double s_H[9];
    if (*a.bad) return;
    const GroundViewFrame &VF = a.vf[blockIdx.y];
    s_lut[threadIdx.x] = a.lut[threadIdx.x];
    if (threadIdx.x < 9) s_H[threadIdx.x] = VF.H[threadIdx.x];
    const long long slot = VF.slot;
    __syncthreads();
    const unsigned per_row = (unsigned)a.w / PX, idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= per_row * (unsigned)a.h) return;
    const int y = (int)(idx / per_row), x0 = (int)(idx - (unsigned)y * per_row) * PX;
    const double v = (double)y + 0.5;
    uint32_t col[PX], any = 0;
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        col[i] = 0u;
        int qx, qy, i0, j0;
        uint32_t fx, fy;
        if (!ground_project(s_H, (double)(x0 + i) + 0.5, v, a.scale, qx, qy)) continue;
        if (!ground_axis(qx, a.ox_q, a.cell_q, a.gw, i0, fx) || !ground_axis(qy, a.oy_q, a.cell_q, a.gh, j0, fy)) continue;
        const int ia = max(i0, 0), ib = min(i0 + 1, a.gw - 1), ja = max(j0, 0), jb = min(j0 + 1, a.gh - 1);
        const uint16_t *La = a.level + (size_t)ja * a.gw, *Lb = a.level + (size_t)jb * a.gw;
        const uint32_t num = (256u - fy) * ((256u - fx) * La[ia] + fx * La[ib]) + fy * ((256u - fx) * Lb[ia] + fx * Lb[ib]);
        const uint32_t k = (num >> 16) / 257u;
        col[i] = k ? s_lut[k] | 0xff000000u : 0u;                                 // bits 24..31: the pixel takes part
        any |= k;
    }
    if (!any) return;                                                             // nothing changes: neither a load nor a store
    uint8_t *p = a.frames + (size_t)slot * a.frame_bytes + ((size_t)y * a.w + x0) * 3;
    uint32_t word[HeatWords<PX>::N];
    heat_load_px<PX>(p, word);
    heat_blend_store_px<PX>(p, word, col, a.alpha, 256u - a.alpha);
}

class Ground : public TrackStage<GroundIface> {
public:
    Ground(int S, int max_age, int K, long long ox_q, long long oy_q, long long cell_q, int gw, int gh, double scale)
        : TrackStage("ground", S), max_age(max_age), K(K), ox_q((int)ox_q), oy_q((int)oy_q), cell_q((int)cell_q), gw(gw), gh(gh), scale(scale), tabs(S),
          specs(S) {
        if (max_age < 1) fail("ground: max_age %d < 1", max_age);
        if (K < 1 || K > YDS_GROUND_MAX_WINDOW) fail("ground: speed_window %d outside [1,%d]", K, YDS_GROUND_MAX_WINDOW);
        if (!(scale > 0.0) || !(scale <= 1e9)) fail("ground: scale %g outside (0, 1e9]", scale);
        if (gw < 1 || gh < 1 || (long long)gw * gh > YDS_HEATMAP_MAX_CELLS) fail("ground: a grid of %d x %d cells exceeds %d", gh, gw, YDS_HEATMAP_MAX_CELLS);
        if (cell_q < 1 || (long long)(std::max(gw, gh) + 2) * cell_q > YDS_GROUND_MAX_EXTENT_Q)
            fail("ground: cell_q %lld with a grid of %d x %d cells: (max(gw, gh) + 2) * cell_q must lie in [1, 2^22]", cell_q, gh, gw);
        if (std::max(std::abs(ox_q), std::abs(oy_q)) > (1ll << 30)) fail("ground: origin (%lld, %lld) quanta outside +-2^30", ox_q, oy_q);
        layers.alloc(GROUND_LAYERS * cells());
        level.alloc(cells());
        bad.alloc(1);
        YDS_HIP(hipMemset(layers.p, 0, GROUND_LAYERS * cells() * sizeof(long long)));
    }

    struct Tab {
        DevBuf<int> ints, rxy;    // id | age | cell | len | head, [2][cap] each; the rings' positions
        DevBuf<double> rt, tl;
        DevBuf<long long> trav;
        int cap = 0;
    };
    struct Spec { double H[9]; int cls = 0; bool set = false; };
    size_t cells() const { return (size_t)gw * gh; }
    GroundTab dev_tab(int s) {
        Tab &t = tabs[s];
        const size_t c2 = 2 * (size_t)t.cap;
        return GroundTab{t.ints.p, t.ints.p + c2, t.ints.p + 2 * c2, t.ints.p + 3 * c2, t.ints.p + 4 * c2, t.rxy.p, t.rt.p, t.tl.p, t.trav.p, counts.p + s, t.cap};
    }
    GroundPlanDev dev_plan() const { return GroundPlanDev{reinterpret_cast<unsigned long long *>(layers.p), scale, ox_q, oy_q, cell_q, gw, gh, K}; }
    void grow(int s, int need) {
        if (!specs[s].set) return;
        const size_t n = count_host[s];
        grow_table(tabs[s], need, n, [&](Tab &nt) {
            nt.ints.alloc(10 * (size_t)nt.cap);
            nt.rxy.alloc(4 * (size_t)nt.cap * K);
            nt.rt.alloc(2 * (size_t)nt.cap * K);
            nt.tl.alloc(2 * (size_t)nt.cap);
            nt.trav.alloc(2 * (size_t)nt.cap);
        }, [&](Tab &nt, const Tab &t) {
            copy_live(nt.ints, t.ints, n, 5, nt.cap, t.cap);
            copy_live(nt.rxy, t.rxy, n * K * 2);
            copy_live(nt.rt, t.rt, n * K);
            copy_live(nt.tl, t.tl, n);
            copy_live(nt.trav, t.trav, n);
        });
    }
    const Spec &spec_of(int stream) const {
        check_stream(stream);
        if (!specs[stream].set) fail("ground: stream %d has no spec (yds_ground_set_stream)", stream);
        return specs[stream];
    }

    void set_stream(int stream, const double *H9, int cls) {
        check_stream(stream);
        if (!H9) fail("ground: NULL argument");
        if (cls < -1) fail("ground: class_id %d (-1 = any class)", cls);
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(H9[k])) fail("ground: H[%d] of stream %d is not finite", k, stream);
        Spec sp;
        std::copy(H9, H9 + 9, sp.H);
        sp.cls = cls; sp.set = true;
        specs[stream] = sp;
        TrackStage::reset(stream);
    }

    // one stream: an empty table for it (the site grid is every stream's and stands); all (-1): empty tables and a zero grid
    void reset(int stream) {
        TrackStage::reset(stream);
        if (stream < 0) YDS_HIP(hipMemset(layers.p, 0, GROUND_LAYERS * cells() * sizeof(long long)));
    }

    void enqueue(const ActFrame *fr, int n, hipStream_t s) override { enqueue_ex(fr, n, s, nullptr, 0); }

    // rows_host (the stand-alone entry): a host array that travels to the device inside the call's input block (open_blocks)
    void enqueue_ex(const ActFrame *fr, int n, hipStream_t s, const int32_t *rows_host, size_t n_rows_host) {
        const StagePlan P = plan(fr, n, [&](int st, int need) { grow(st, need); });
        if (!P.n_wg) return;
        // ---- blocks: input = works | frames | rows; results = counted rows of every frame | entry counts | records
        const size_t works_b = (size_t)P.n_wg * sizeof(GroundWork);
        size_t res_total = (size_t)n + P.n_wg;
        pending_rows.resize(n);
        pending_cap.resize(n);
        pending_tag.resize(n);
        for (int i = 0; i < n; ++i) {
            pending_rows[i] = res_total;
            pending_cap[i] = fr[i].n_rows;
            pending_tag[i] = fr[i].tag;
            res_total += (size_t)fr[i].n_rows * 8;
        }
        open_blocks(P, works_b + (size_t)n * sizeof(GroundFrameDev), rows_host, n_rows_host, res_total);
        GroundWork *w = reinterpret_cast<GroundWork *>(in_host.p);
        GroundFrameDev *fd = reinterpret_cast<GroundFrameDev *>(in_host.p + works_b);
        for (int k = 0; k < P.n_wg; ++k) {
            const int st = wg_stream[k];
            GroundWork g;
            g.tab = dev_tab(st);
            std::copy(specs[st].H, specs[st].H + 9, g.H);
            g.cls = specs[st].cls; g.skip = specs[st].set ? 0 : 1;
            g.f0 = P.start[st]; g.f1 = P.start[st] + P.n_of[st];
            g.srows = wg_srows(k);
            g.res_count = n + k;
            w[k] = g;
        }
        for (int e = 0; e < n; ++e) {
            const ActFrame &f = fr[P.order[e]];
            GroundFrameDev d;
            d.rows = dev_rows(f);
            d.n_p = f.n_rows_p;
            d.t = f.t; d.n = f.n_rows;
            d.res_n = P.order[e];
            d.res_rows = (int)pending_rows[P.order[e]];
            fd[e] = d;
        }
        const GroundPlanDev plan_dev = dev_plan();
        submit(s, [&] {
            hipLaunchKernelGGL(ground_update_kernel, dim3(P.n_wg), dim3(256), 0, s, reinterpret_cast<const GroundWork *>(in_dev.p),
                               reinterpret_cast<const GroundFrameDev *>(in_dev.p + works_b), plan_dev, max_age, res_host.p);
        });
    }

    void collect() override {
        report.rows.clear();
        report.tags.clear();
        collect_counts("ground rows", [&](int i, int m) {
            const int *r = res_host.p + pending_rows[i];
            report.rows.insert(report.rows.end(), r, r + (size_t)m * 8);
            report.tags.insert(report.tags.end(), (size_t)m, pending_tag[i]);
        });
    }

    // ---- the input block of a render call: one level job | one (slot, job) pair | LUT | the view frames
    static constexpr size_t R_FJ = sizeof(HeatLevelJob), R_LUT = R_FJ + sizeof(int2), R_VF = R_LUT + 256 * sizeof(uint32_t);
    void open_render(int n_view) {
        const size_t total = R_VF + (size_t)n_view * sizeof(GroundViewFrame);
        if (total > r_in_host.n) { r_in_host.ensure(total * 2); r_in_dev.alloc(r_in_host.n); }
        r_res.ensure(1);
        r_bytes = total;
    }
    void check_render(const void *dst, int layer, long long vmax, int alpha, const uint8_t *lut) const {
        if (!dst || !lut) fail("ground: NULL argument");
        if (layer < 0 || layer >= GROUND_RENDERABLE) fail("ground: layer %d is not renderable (0 presence, 1 visits, 2 dwell_us)", layer);
        if (vmax < 0 || vmax > GROUND_VMAX_LIMIT) fail("ground: vmax %lld outside [1, 2^47] (0 = the layer's maximum)", vmax);
        if (alpha < 1 || alpha > 256) fail("ground: alpha %d outside [1, 256]", alpha);
    }
    // job, pair and LUT into the block; the block goes up and the levels kernel runs behind it
    void start_render(int layer, long long vmax, int lc, const uint8_t *lut) {
        *reinterpret_cast<HeatLevelJob *>(r_in_host.p) = HeatLevelJob{layers.p + (size_t)layer * cells(), level.p, vmax, (int)cells(), gw, gh, lc};
        *reinterpret_cast<int2 *>(r_in_host.p + R_FJ) = make_int2(0, 0);
        heat_pack_lut(reinterpret_cast<uint32_t *>(r_in_host.p + R_LUT), lut);
        YDS_HIP(hipMemcpyAsync(r_in_dev.p, r_in_host.p, r_bytes, hipMemcpyHostToDevice, own_stream));
        YDS_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), own_stream));
        render_timer.begin(own_stream);
        heat_launch_levels(reinterpret_cast<const HeatLevelJob *>(r_in_dev.p), 1, r_res.p, bad.p, own_stream);
    }
    void end_render(long long vmax) {
        YDS_HIP(hipGetLastError());
        render_timer.end(own_stream);
        YDS_HIP(hipStreamSynchronize(own_stream));
        if (!vmax && r_res.p[0] > GROUND_VMAX_LIMIT)
            fail("ground: vmax 0 and the layer's maximum %lld exceeds 2^47: nothing was rendered", r_res.p[0]);
    }

    // a site layer onto a plan canvas of gh * cell_px x gw * cell_px pixels: the heat map's render of this grid
    void render_plan(uint8_t *canvas, int cell_px, int layer, long long vmax, int alpha, const uint8_t *lut) {
        check_render(canvas, layer, vmax, alpha, lut);
        int lc = 0;
        while ((1 << lc) < cell_px && lc < 8) ++lc;
        if (cell_px < 4 || cell_px > 128 || (1 << lc) != cell_px) fail("ground: cell_px %d is not one of 4, 8, 16, 32, 64, 128", cell_px);
        const int h = gh * cell_px, w = gw * cell_px;
        open_render(0);
        start_render(layer, vmax, lc, lut);
        const HeatRenderArgs a{canvas, (size_t)h * w * 3, reinterpret_cast<const int2 *>(r_in_dev.p + R_FJ), reinterpret_cast<const HeatLevelJob *>(r_in_dev.p),
                               reinterpret_cast<const uint32_t *>(r_in_dev.p + R_LUT), bad.p, h, w, (uint32_t)alpha};
        heat_launch_render(a, 1, own_stream);
        end_render(vmax);
    }

    // a site layer onto the floor of n camera frames of h x w: frame i sits in slot slot[i] of n_src and takes the H of stream_of[i]
    void render_view(uint8_t *frames, int n_src, const int32_t *slot, const int32_t *stream_of, int n, int h, int w, int layer, long long vmax,
                     int alpha, const uint8_t *lut) {
        if (n <= 0) return;
        check_render(frames, layer, vmax, alpha, lut);
        if (!slot || !stream_of || n_src < 1) fail("ground: NULL argument");
        if (h < 1 || w < 1) fail("ground: frames of %d x %d", h, w);
        std::vector<int> sorted(slot, slot + n);
        for (int i = 0; i < n; ++i)
            if (slot[i] < 0 || slot[i] >= n_src) fail("ground: frame %d names slot %d of %d frames", i, slot[i], n_src);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 1; i < n; ++i)
            if (sorted[i] == sorted[i - 1]) fail("ground: two frames name the same slot %d", sorted[i]);
        for (int i = 0; i < n; ++i) spec_of(stream_of[i]);
        const int px = heat_px_per_thread(frames, w);
        const size_t threads = (size_t)h * (w / px);
        if ((threads + 255) / 256 > 0x7fffffffull || n > 65535) fail("ground: %d frames of %d x %d are too large for one launch", n, h, w);
        open_render(n);
        GroundViewFrame *vf = reinterpret_cast<GroundViewFrame *>(r_in_host.p + R_VF);
        for (int i = 0; i < n; ++i) {
            std::copy(specs[stream_of[i]].H, specs[stream_of[i]].H + 9, vf[i].H);
            vf[i].slot = slot[i];
        }
        start_render(layer, vmax, 0, lut);
        const GroundViewArgs a{frames, (size_t)h * w * 3, reinterpret_cast<const GroundViewFrame *>(r_in_dev.p + R_VF), level.p,
                               reinterpret_cast<const uint32_t *>(r_in_dev.p + R_LUT), bad.p, scale, h, w, ox_q, oy_q, cell_q, gw, gh, (uint32_t)alpha};
        const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)n);
        if (px == 16) hipLaunchKernelGGL(ground_view_kernel<16>, grid, dim3(256), 0, own_stream, a);
        else if (px == 4) hipLaunchKernelGGL(ground_view_kernel<4>, grid, dim3(256), 0, own_stream, a);
        else hipLaunchKernelGGL(ground_view_kernel<1>, grid, dim3(256), 0, own_stream, a);
        end_render(vmax);
    }

    // the maximum of one site layer, reduced on the device (the levels kernel without levels)
    long long layer_max(int layer) {
        if (layer < 0 || layer >= GROUND_LAYERS) fail("ground: layer %d outside [0,%d)", layer, GROUND_LAYERS);
        open_render(0);
        *reinterpret_cast<HeatLevelJob *>(r_in_host.p) = HeatLevelJob{layers.p + (size_t)layer * cells(), nullptr, 0, (int)cells(), gw, gh, 0};
        YDS_HIP(hipMemcpyAsync(r_in_dev.p, r_in_host.p, sizeof(HeatLevelJob), hipMemcpyHostToDevice, own_stream));
        heat_launch_levels(reinterpret_cast<const HeatLevelJob *>(r_in_dev.p), 1, r_res.p, bad.p, own_stream);
        YDS_HIP(hipGetLastError());
        YDS_HIP(hipStreamSynchronize(own_stream));
        return r_res.p[0];
    }

    int max_age, K, ox_q, oy_q, cell_q, gw, gh;
    double scale;
    std::vector<Tab> tabs;
    std::vector<Spec> specs;
    DevBuf<long long> layers;                     // the site grid [5][gh * gw]
    DevBuf<uint16_t> level;
    DevBuf<int> bad;
    DevBuf<char> r_in_dev;
    PinBuf<char> r_in_host;
    PinBuf<long long> r_res;
    size_t r_bytes = 0;
    std::vector<size_t> pending_rows;             // of the call in flight: where every frame's records begin in the result block
    std::vector<int> pending_tag;
    LaunchTimer render_timer;
};

}  // namespace yds

static inline yds::Ground *impl(yds_ground *g) {
    if (!g) yds::fail("ground: NULL handle");
    return static_cast<yds::Ground *>(g->g);
}

extern "C" {

yds_ground *yds_ground_create(int n_streams, int max_age, int speed_window, int64_t ox_q, int64_t oy_q, int64_t cell_q, int gw, int gh, double scale) {
    YDS_API_BEGIN
    return new yds_ground{new yds::Ground(n_streams, max_age, speed_window, ox_q, oy_q, cell_q, gw, gh, scale)};
    YDS_API_END_PTR
}
void yds_ground_destroy(yds_ground *g) {
    if (g) { delete g->g; delete g; }
}
int yds_ground_set_stream(yds_ground *g, int stream, const double *H9, int class_id) {
    YDS_API_BEGIN
    impl(g)->set_stream(stream, H9, class_id);
    YDS_API_END
}
int yds_ground_reset(yds_ground *g, int stream) {
    YDS_API_BEGIN
    impl(g)->reset(stream);
    YDS_API_END
}
int yds_ground_update(yds_ground *g, const int32_t *rows6_host, const int32_t *first, const int32_t *stream_of, const double *frame_time, int n_frames,
                      int32_t *out8_host, int32_t *first_out, int cap, int *n_out) {
    YDS_API_BEGIN
    yds::Ground *G = impl(g);
    const std::vector<yds::ActFrame> fr = yds::csr_frames("ground", rows6_host, first, stream_of, frame_time, false, n_frames, n_out);
    if (fr.empty()) return 0;
    G->enqueue_ex(fr.data(), n_frames, G->own_stream, rows6_host, (size_t)first[n_frames]);
    G->finish_alone();
    const int m = G->give_count("ground rows", (int)(G->report.rows.size() / 8), cap, n_out);
    if (m) {
        if (!out8_host) yds::fail("ground: NULL argument");
        memcpy(out8_host, G->report.rows.data(), (size_t)m * 8 * sizeof(int32_t));
    }
    if (first_out) memcpy(first_out, G->first.data(), ((size_t)n_frames + 1) * sizeof(int32_t));
    YDS_API_END
}
int yds_ground_get_layers(yds_ground *g, int64_t *out5, size_t cap) {
    YDS_API_BEGIN
    yds::Ground *G = impl(g);
    const size_t m = yds::GROUND_LAYERS * G->cells();
    if (m > cap) yds::fail("ground: %zu layer values exceed the caller's capacity %zu", m, cap);
    if (!out5) yds::fail("ground: NULL argument");
    YDS_HIP(hipMemcpy(out5, G->layers.p, m * sizeof(int64_t), hipMemcpyDeviceToHost));
    YDS_API_END
}
int yds_ground_get_max(yds_ground *g, int layer, int64_t *out) {
    YDS_API_BEGIN
    if (!out) yds::fail("ground: NULL argument");
    *out = impl(g)->layer_max(layer);
    YDS_API_END
}
int yds_ground_get_tracks(yds_ground *g, int stream, int32_t *ids, int32_t *ages, int32_t *cells, int32_t *lens, int64_t *travelled, double *t_last,
                          int32_t *ring_xy, double *ring_t, int cap, int *n) {
    YDS_API_BEGIN
    yds::Ground *G = impl(g);
    const int m = G->table_count(stream, "tracks", cap, n);
    if (!m) return 0;
    const yds::GroundTab tb = G->dev_tab(stream);
    const int K = G->K;
    std::vector<int32_t> len(m), head(m);
    G->column_out(ids, tb.id, m);
    G->column_out(ages, tb.age, m);
    G->column_out(cells, tb.cell, m);
    G->column_out(len.data(), tb.len, m);
    G->column_out(head.data(), tb.head, m);
    if (lens) memcpy(lens, len.data(), (size_t)m * sizeof(int32_t));
    if (travelled) YDS_HIP(hipMemcpy(travelled, tb.trav, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (t_last) YDS_HIP(hipMemcpy(t_last, tb.tl, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (ring_xy || ring_t) {                      // oldest first, unused places zero
        std::vector<int32_t> xy((size_t)m * K * 2);
        std::vector<double> rt((size_t)m * K);
        YDS_HIP(hipMemcpy(xy.data(), tb.rxy, xy.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        YDS_HIP(hipMemcpy(rt.data(), tb.rt, rt.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int e = 0; e < m; ++e)
            for (int k = 0; k < K; ++k) {
                const size_t d = (size_t)e * K + k, s = (size_t)e * K + (head[e] + k) % K;
                const bool live = k < len[e];
                if (ring_xy) { ring_xy[2 * d] = live ? xy[2 * s] : 0; ring_xy[2 * d + 1] = live ? xy[2 * s + 1] : 0; }
                if (ring_t) ring_t[d] = live ? rt[s] : 0.0;
            }
    }
    YDS_API_END
}
int yds_ground_render_plan(yds_ground *g, uint8_t *canvas_dev, int cell_px, int layer, int64_t vmax, int alpha, const uint8_t *lut_host) {
    YDS_API_BEGIN
    impl(g)->render_plan(canvas_dev, cell_px, layer, vmax, alpha, lut_host);
    YDS_API_END
}
int yds_ground_render_view(yds_ground *g, uint8_t *frames_dev, int n_src, const int32_t *slot_host, const int32_t *stream_of_host, int n, int height,
                           int width, int layer, int64_t vmax, int alpha, const uint8_t *lut_host) {
    YDS_API_BEGIN
    impl(g)->render_view(frames_dev, n_src, slot_host, stream_of_host, n, height, width, layer, vmax, alpha, lut_host);
    YDS_API_END
}
int yds_ground_set_timing(yds_ground *g, int on) {
    YDS_API_BEGIN
    impl(g)->timer.set(on != 0);
    impl(g)->render_timer.set(on != 0);
    YDS_API_END
}
int yds_ground_last_us(yds_ground *g, int what, float *us) {
    YDS_API_BEGIN
    if (what != 0 && what != 1) yds::fail("ground: last_us of %d (0 = the update launch, 1 = the render)", what);
    *us = what ? impl(g)->render_timer.us("ground") : impl(g)->timer.us("ground");
    YDS_API_END
}

}  // extern "C"
