// Zones and counting lines on the device: per video stream a table of tracks in HBM - id, class, age, last doubled foot point and its
// time, and per zone an inside bit, a debounce streak and an enter time - advanced by one launch per call, beside the action stage
// (actions.hip) and built on the same frame (track_stage.h).
//
// There is no reference counterpart; the rules are written down in include/ydsort.h (the zones block) and restated in Python ints by
// yolo_deepsort_amd/zones.py ZoneMonitor, which every device test compares against with exact equality: all geometry is int64.
// One workgroup per stream that has frames in the call walks that stream's frames in time order.  Per frame it stages the rows once
// (they may sit in pinned host memory: a tracker result block), registers unknown ids at the end of the table in row order, then
// handles the entries in table order, one thread per entry: a seen entry tests every class-matching line against the move from its
// last point and every class-matching zone against its new point, an unseen entry ages.  What an entry emits is kept as five 32-bit
// masks in registers; the events go count, prefix, write - entry-major, lines before zones - straight into a pinned result block.
// Entries that reached max_age then leave by an ordered compaction (track_stage.h retire).  Counters are summed in LDS and
// added to the stream's counters in HBM once per call.
#include "track_stage.h"
#include "ydsort.h"

#include <memory>

namespace yds {

constexpr int ZMAX = YDS_ZONE_MAX_ZONES, LMAX = YDS_ZONE_MAX_LINES, VMAX = YDS_ZONE_MAX_VERTICES;
constexpr int N_CTR = ZMAX * 4 + LMAX * 2;        // per zone occupancy, entries, exits, lost; per line forward, backward
constexpr long long ANCHOR_LIMIT = 1ll << 24;

// geometry of one stream as the kernel reads it: every coordinate DOUBLED
struct ZoneGeo {
    int Z, L;
    int zptr[ZMAX + 1];
    int zcls[ZMAX], zmin[ZMAX], lcls[LMAX];
    int lxy[LMAX][4];
    int vxy[ZMAX * VMAX][2];
};
constexpr int GEO_INTS = sizeof(ZoneGeo) / sizeof(int);

// table of one stream: `cap` entries, every field twice (the second copy takes the survivors of a removal)
struct ZoneTab {
    int *id, *cls, *age, *px, *py;                // [2][cap] each
    uint32_t *mask;                               // [2][cap]        bit z: inside zone z
    double *pt;                                   // [2][cap]        time of the last point
    uint8_t *streak;                              // [2][cap][ZMAX]
    double *enter;                                // [2][cap][ZMAX]
    int *count;                                   // live entries (device)
    int *ctr;                                     // [N_CTR] counters of the stream
    int cap;
};
struct ZoneWork {
    ZoneTab tab;
    const ZoneGeo *geo;
    int f0, f1;                                   // frames [f0, f1) of the call's frame list (sorted by stream, order kept)
    int *srows;                                   // staging [max rows of a frame][6]
    int res_count;                                // int index in the result block of this stream's entry count
};
struct ZoneFrameDev {
    const int *rows;
    const int *n_p;
    double t;
    int n, tag;
    int res_n;                                    // int index in the result block of this frame's event count
    int ev_off, ev_cap;                           // its events [ev_off, ev_off + ev_cap) of the call's event area
};

__device__ __forceinline__ long long zone_orient(long long ux, long long uy, long long vx, long long vy, long long wx, long long wy) {
    return (vx - ux) * (wy - uy) - (vy - uy) * (wx - ux);
}
// the move P -> C against the segment A -> B: +1 forward, -1 backward, 0 none
__device__ __forceinline__ int zone_cross(long long px, long long py, long long cx, long long cy, const int *ab) {
    const long long ax = ab[0], ay = ab[1], bx = ab[2], by = ab[3];
    const bool sp = zone_orient(ax, ay, bx, by, px, py) >= 0, sc = zone_orient(ax, ay, bx, by, cx, cy) >= 0;
    if (sp == sc) return 0;
    const long long nx = sc ? px : cx, ny = sc ? py : cy, qx = sc ? cx : px, qy = sc ? cy : py;
    if ((zone_orient(nx, ny, qx, qy, ax, ay) >= 0) == (zone_orient(nx, ny, qx, qy, bx, by) >= 0)) return 0;
    return sc ? 1 : -1;
}
// even-odd rule over the edges (Vi, Vi+1 mod n)
__device__ __forceinline__ bool zone_inside(long long x, long long y, const int (*v)[2], int nv) {
    bool hit = false;
    long long xi = v[nv - 1][0], yi = v[nv - 1][1];
    for (int j = 0; j < nv; ++j) {                // edge (V[j - 1], V[j]), j = 0: the closing edge
        const long long xj = v[j][0], yj = v[j][1];
        if ((yi > y) != (yj > y)) {
            const long long s = (xj - xi) * (y - yi) - (x - xi) * (yj - yi);
            if (yj > yi ? s > 0 : s < 0) hit = !hit;
        }
        xi = xj; yi = yj;
    }
    return hit;
}
__device__ __forceinline__ int clamp_anchor(long long v) { return (int)(v < -ANCHOR_LIMIT ? -ANCHOR_LIMIT : v > ANCHOR_LIMIT ? ANCHOR_LIMIT : v); }

__global__ __launch_bounds__(256) void zone_update_kernel(const ZoneWork *works, const ZoneFrameDev *frames, int max_age, int *res, int ev_base,
                                                          double *res_t) {
    __shared__ int s_cnt[4];
    __shared__ int s_geo[GEO_INTS];
    __shared__ int s_ctr[N_CTR];
    const ZoneWork W = works[blockIdx.x];
    const ZoneTab T = W.tab;
    const int tid = threadIdx.x, cap = T.cap;
    for (int k = tid; k < GEO_INTS; k += 256) s_geo[k] = reinterpret_cast<const int *>(W.geo)[k];
    for (int k = tid; k < N_CTR; k += 256) s_ctr[k] = 0;
    int n = *T.count;
    __syncthreads();
    const ZoneGeo &G = *reinterpret_cast<const ZoneGeo *>(s_geo);
    for (int f = W.f0; f < W.f1; ++f) {
        const ZoneFrameDev F = frames[f];
        const int R = stage_frame_rows(F.rows, F.n_p, F.n, W.srows);
        __syncthreads();
        // ---- rows whose id is unknown are registered at the end of the table in row order: bit outside, no streak
        const int n_all = register_unknown(R, n, cap, s_cnt, T.id, W.srows, [&](int e, const int *r) {
            T.id[e] = r[4]; T.cls[e] = r[5]; T.age[e] = 0; T.mask[e] = 0u;
            for (int z = 0; z < ZMAX; ++z) T.streak[(size_t)e * ZMAX + z] = 0;
        });
        __syncthreads();
        // ---- entries in table order, a thread each; the events of a chunk of 256 entries go count, prefix, write
        int *out6 = res + ev_base + (size_t)F.ev_off * 6;
        double *out2 = res_t + (size_t)F.ev_off * 2;
        int total = 0, dead = 0;
        for (int base = 0; base < n_all; base += 256) {
            const int e = base + tid;
            uint32_t m_fwd = 0u, m_back = 0u, m_in = 0u, m_out = 0u, m_lost = 0u;
            bool gone = false;
            int id = 0, cls = 0;
            if (e < n_all) {
                id = T.id[e]; cls = T.cls[e];
                const int j = find_row(W.srows, R, id);
                if (j == R) {                                                     // unseen: ages, LOST from every zone it is inside
                    const int a = T.age[e] + 1;
                    T.age[e] = a;
                    if (a >= max_age) { gone = true; m_lost = T.mask[e]; }
                } else {
                    const int *r = W.srows + j * 6;
                    const int X = clamp_anchor((long long)r[0] + (long long)r[2]), Y = clamp_anchor(2ll * (long long)r[3]);
                    if (e < n) {                                                  // (a registering row is its first sighting: no line test)
                        const int PX = T.px[e], PY = T.py[e];
                        for (int k = 0; k < G.L; ++k) {
                            if (G.lcls[k] != -1 && G.lcls[k] != cls) continue;
                            const int d = zone_cross(PX, PY, X, Y, G.lxy[k]);
                            if (d > 0) m_fwd |= 1u << k; else if (d < 0) m_back |= 1u << k;
                        }
                    }
                    uint32_t bits = T.mask[e];
                    for (int z = 0; z < G.Z; ++z) {
                        if (G.zcls[z] != -1 && G.zcls[z] != cls) continue;
                        const bool now = zone_inside(X, Y, G.vxy + G.zptr[z], G.zptr[z + 1] - G.zptr[z]);
                        uint8_t *st = T.streak + (size_t)e * ZMAX + z;
                        if (now == (((bits >> z) & 1u) != 0u)) { *st = 0; continue; }
                        const int s = (int)*st + 1;
                        if (s < G.zmin[z]) { *st = (uint8_t)s; continue; }
                        *st = 0;
                        bits ^= 1u << z;
                        if (now) { T.enter[(size_t)e * ZMAX + z] = F.t; m_in |= 1u << z; } else m_out |= 1u << z;
                    }
                    T.mask[e] = bits; T.px[e] = X; T.py[e] = Y; T.pt[e] = F.t; T.age[e] = 0;
                }
            }
            const uint32_t m_line = m_fwd | m_back, m_zone = m_in | m_out;
            int chunk;
            int at = total + block_prefix(__popc(m_line) + __popc(m_zone) + __popc(m_lost), s_cnt, chunk);
            for (uint32_t m = m_line; m; m &= m - 1u, ++at) {
                const int k = __ffs(m) - 1;
                const bool fwd = (m_fwd >> k) & 1u;
                atomicAdd(&s_ctr[ZMAX * 4 + k * 2 + (fwd ? 0 : 1)], 1);
                if (at >= F.ev_cap) continue;
                int *o = out6 + (size_t)at * 6;
                o[0] = F.tag; o[1] = id; o[2] = cls; o[3] = fwd ? YDS_ZONE_CROSS_FWD : YDS_ZONE_CROSS_BACK; o[4] = k; o[5] = 0;
                out2[(size_t)at * 2] = F.t; out2[(size_t)at * 2 + 1] = 0.0;
            }
            for (uint32_t m = m_zone; m; m &= m - 1u, ++at) {
                const int z = __ffs(m) - 1;
                const bool in = (m_in >> z) & 1u;
                atomicAdd(&s_ctr[z * 4], in ? 1 : -1);
                atomicAdd(&s_ctr[z * 4 + (in ? 1 : 2)], 1);
                if (at >= F.ev_cap) continue;
                int *o = out6 + (size_t)at * 6;
                o[0] = F.tag; o[1] = id; o[2] = cls; o[3] = in ? YDS_ZONE_ENTER : YDS_ZONE_EXIT; o[4] = z; o[5] = 0;
                out2[(size_t)at * 2] = F.t; out2[(size_t)at * 2 + 1] = in ? 0.0 : F.t - T.enter[(size_t)e * ZMAX + z];
            }
            for (uint32_t m = m_lost; m; m &= m - 1u, ++at) {
                const int z = __ffs(m) - 1;
                atomicAdd(&s_ctr[z * 4], -1);
                atomicAdd(&s_ctr[z * 4 + 3], 1);
                if (at >= F.ev_cap) continue;
                int *o = out6 + (size_t)at * 6;
                o[0] = F.tag; o[1] = id; o[2] = cls; o[3] = YDS_ZONE_LOST; o[4] = z; o[5] = 0;
                out2[(size_t)at * 2] = F.t; out2[(size_t)at * 2 + 1] = T.pt[e] - T.enter[(size_t)e * ZMAX + z];
            }
            total += chunk;
            dead += __syncthreads_count(gone);
        }
        if (tid == 0) res[F.res_n] = total;
        // ---- entries that reached max_age leave, the rest keep their order (only an entry that just aged has age > 0)
        int n_live = n_all;
        if (dead) {
            auto move = [&](int d, int e) {
                T.id[d] = T.id[e]; T.cls[d] = T.cls[e]; T.age[d] = T.age[e]; T.px[d] = T.px[e]; T.py[d] = T.py[e]; T.mask[d] = T.mask[e];
                T.pt[d] = T.pt[e];
            };
            n_live = retire(n_all, cap, s_cnt, [&](int e) { const int a = T.age[e]; return !(a > 0 && a >= max_age); }, [&](int d, int e) {
                move(d, e);
                for (int z = 0; z < ZMAX; ++z) {
                    T.streak[(size_t)d * ZMAX + z] = T.streak[(size_t)e * ZMAX + z];
                    T.enter[(size_t)d * ZMAX + z] = T.enter[(size_t)e * ZMAX + z];
                }
            }, move);
            for (size_t k = tid; k < (size_t)n_live * ZMAX; k += 256) {
                T.streak[k] = T.streak[(size_t)cap * ZMAX + k];
                T.enter[k] = T.enter[(size_t)cap * ZMAX + k];
            }
        }
        n = n_live;
        __syncthreads();
    }
    for (int k = tid; k < N_CTR; k += 256) T.ctr[k] += s_ctr[k];
    if (tid == 0) { *T.count = n; res[W.res_count] = n; }
}

class Zones : public TrackStage<ZonesIface> {
public:
    Zones(int S, int max_age) : TrackStage("zones", S), max_age(max_age), tabs(S), nz(S, 0), nl(S, 0) {
        if (max_age < 1) fail("zones: max_age %d < 1", max_age);
        geo.alloc(S);
        YDS_HIP(hipMemset(geo.p, 0, S * sizeof(ZoneGeo)));                       // (no zones, no lines until set_stream)
        ctr.alloc((size_t)S * N_CTR);
        YDS_HIP(hipMemset(ctr.p, 0, (size_t)S * N_CTR * sizeof(int)));
    }

    struct Tab {
        DevBuf<int> ints;         // id | cls | age | px | py | mask, [2][cap] each
        DevBuf<double> pt, enter;
        DevBuf<uint8_t> streak;
        int cap = 0;
    };
    ZoneTab dev_tab(int s) {
        Tab &t = tabs[s];
        const size_t c2 = 2 * (size_t)t.cap;
        return ZoneTab{t.ints.p, t.ints.p + c2, t.ints.p + 2 * c2, t.ints.p + 3 * c2, t.ints.p + 4 * c2,
                       reinterpret_cast<uint32_t *>(t.ints.p + 5 * c2), t.pt.p, t.streak.p, t.enter.p, counts.p + s, ctr.p + (size_t)s * N_CTR, t.cap};
    }
    void grow(int s, int need) {
        const size_t n = count_host[s];
        grow_table(tabs[s], need, n, [&](Tab &nt) {
            nt.ints.alloc(12 * (size_t)nt.cap);
            nt.pt.alloc(2 * (size_t)nt.cap);
            nt.enter.alloc(2 * (size_t)nt.cap * ZMAX);
            nt.streak.alloc(2 * (size_t)nt.cap * ZMAX);
        }, [&](Tab &nt, const Tab &t) {
            copy_live(nt.ints, t.ints, n, 6, nt.cap, t.cap);
            copy_live(nt.pt, t.pt, n);
            copy_live(nt.enter, t.enter, n * ZMAX);
            copy_live(nt.streak, t.streak, n * ZMAX);
        });
    }

    void set_stream(int stream, const int32_t *zptr, const int32_t *zxy, const int32_t *zcls, const int32_t *zmin, int Z, const int32_t *lxy,
                    const int32_t *lcls, int L) {
        check_stream(stream, -1);
        if (Z < 0 || Z > ZMAX) fail("zones: %d zones outside [0,%d]", Z, ZMAX);
        if (L < 0 || L > LMAX) fail("zones: %d lines outside [0,%d]", L, LMAX);
        if (Z && (!zptr || !zxy || !zcls || !zmin)) fail("zones: NULL zone geometry");
        if (L && (!lxy || !lcls)) fail("zones: NULL line geometry");
        auto g = std::make_unique<ZoneGeo>();
        memset(g.get(), 0, sizeof(ZoneGeo));
        auto coord = [](int v, const char *what, int k) {
            if (v < -YDS_ZONE_COORD_LIMIT || v > YDS_ZONE_COORD_LIMIT) fail("zones: a coordinate of %s %d is %d, outside [-2^20, 2^20]", what, k, v);
            return 2 * v;
        };
        g->Z = Z; g->L = L;
        if (Z && zptr[0] != 0) fail("zones: zone_ptr[0] = %d", zptr[0]);
        for (int z = 0; z < Z; ++z) {
            const int nv = zptr[z + 1] - zptr[z];
            if (nv < 3 || nv > VMAX) fail("zones: zone %d has %d vertices, outside [3,%d]", z, nv, VMAX);
            if (zmin[z] < 1 || zmin[z] > 255) fail("zones: min_sightings of zone %d is %d, outside [1,255]", z, zmin[z]);
            if (zcls[z] < -1) fail("zones: class_id of zone %d is %d (-1 = any class)", z, zcls[z]);
            g->zptr[z + 1] = zptr[z + 1]; g->zcls[z] = zcls[z]; g->zmin[z] = zmin[z];
            for (int v = zptr[z]; v < zptr[z + 1]; ++v) {
                g->vxy[v][0] = coord(zxy[2 * v], "zone", z);
                g->vxy[v][1] = coord(zxy[2 * v + 1], "zone", z);
            }
        }
        for (int k = 0; k < L; ++k) {
            for (int c = 0; c < 4; ++c) g->lxy[k][c] = coord(lxy[4 * k + c], "line", k);
            if (lxy[4 * k] == lxy[4 * k + 2] && lxy[4 * k + 1] == lxy[4 * k + 3]) fail("zones: line %d has A == B", k);
            if (lcls[k] < -1) fail("zones: class_id of line %d is %d (-1 = any class)", k, lcls[k]);
            g->lcls[k] = lcls[k];
        }
        for (int s = 0; s < S; ++s) {
            if (stream >= 0 && s != stream) continue;
            YDS_HIP(hipMemcpy(geo.p + s, g.get(), sizeof(ZoneGeo), hipMemcpyHostToDevice));
            nz[s] = Z; nl[s] = L;
        }
        reset(stream);
    }

    void reset(int stream) {
        TrackStage::reset(stream);
        YDS_HIP(hipMemset(ctr.p + (size_t)std::max(stream, 0) * N_CTR, 0, (size_t)(stream < 0 ? S : 1) * N_CTR * sizeof(int)));
    }

    void enqueue(const ActFrame *fr, int n, hipStream_t s) override { enqueue_ex(fr, n, s, nullptr, 0); }

    // rows_host (the stand-alone entry): a host array that travels to the device inside the call's input block (open_blocks)
    void enqueue_ex(const ActFrame *fr, int n, hipStream_t s, const int32_t *rows_host, size_t n_rows_host) {
        const StagePlan P = plan(fr, n, [&](int st, int need) { grow(st, need); });
        if (!P.n_wg) return;
        // ---- the most events a frame can emit: every entry it can meet (the table before the call + the rows so far), at each zone
        //      and line of its stream
        pending_off.resize(n);
        pending_cap.resize(n);
        size_t ev_total = 0;
        {
            std::vector<size_t> held(count_host.begin(), count_host.end());
            for (int i = 0; i < n; ++i) {
                const int st = fr[i].stream;
                held[st] += fr[i].n_rows;
                const size_t c = held[st] * (size_t)(nz[st] + nl[st]);
                if (c > (size_t)INT_MAX) fail("zones: frame %d may emit %zu events", i, c);
                pending_off[i] = ev_total;
                pending_cap[i] = (int)c;
                ev_total += c;
            }
        }
        // ---- blocks: input = works | frames | rows; results = frame counts | entry counts | events [m][6] (int) and [m][2] (double)
        const size_t works_b = (size_t)P.n_wg * sizeof(ZoneWork);
        pending_base = (size_t)n + P.n_wg;
        open_blocks(P, works_b + (size_t)n * sizeof(ZoneFrameDev), rows_host, n_rows_host, pending_base + ev_total * 6);
        if (ev_total * 2 + 2 > res_t_host.n) res_t_host.ensure((ev_total * 2 + 2) * 2);
        ZoneWork *w = reinterpret_cast<ZoneWork *>(in_host.p);
        ZoneFrameDev *fd = reinterpret_cast<ZoneFrameDev *>(in_host.p + works_b);
        for (int k = 0; k < P.n_wg; ++k) {
            const int st = wg_stream[k];
            w[k] = ZoneWork{dev_tab(st), geo.p + st, P.start[st], P.start[st] + P.n_of[st], wg_srows(k), n + k};
        }
        for (int e = 0; e < n; ++e) {
            const ActFrame &f = fr[P.order[e]];
            ZoneFrameDev d;
            d.rows = dev_rows(f);
            d.n_p = f.n_rows_p;
            d.t = f.t; d.n = f.n_rows; d.tag = f.tag;
            d.res_n = P.order[e];
            d.ev_off = (int)pending_off[P.order[e]];
            d.ev_cap = pending_cap[P.order[e]];
            fd[e] = d;
        }
        submit(s, [&] {
            hipLaunchKernelGGL(zone_update_kernel, dim3(P.n_wg), dim3(256), 0, s, reinterpret_cast<const ZoneWork *>(in_dev.p),
                               reinterpret_cast<const ZoneFrameDev *>(in_dev.p + works_b), max_age, res_host.p, (int)pending_base, res_t_host.p);
        });
    }

    void collect() override {
        report.rows.clear();
        report.times.clear();
        collect_counts("events", [&](int i, int m) {
            const int *r = res_host.p + pending_base + pending_off[i] * 6;
            const double *t = res_t_host.p + pending_off[i] * 2;
            report.rows.insert(report.rows.end(), r, r + (size_t)m * 6);
            report.times.insert(report.times.end(), t, t + (size_t)m * 2);
        });
    }

    int max_age;
    std::vector<Tab> tabs;
    std::vector<int> nz, nl;                      // zones / lines of every stream
    DevBuf<ZoneGeo> geo;
    DevBuf<int> ctr;
    PinBuf<double> res_t_host;
    size_t pending_base = 0;                      // of the call in flight: where the events begin in the int result block ...
    std::vector<size_t> pending_off;              // ... and every frame's first event
};

}  // namespace yds

static inline yds::Zones *impl(yds_zones *h) {
    if (!h) yds::fail("zones: NULL handle");
    return static_cast<yds::Zones *>(h->z);
}

extern "C" {

yds_zones *yds_zones_create(int n_streams, int max_age) {
    YDS_API_BEGIN
    return new yds_zones{new yds::Zones(n_streams, max_age)};
    YDS_API_END_PTR
}
void yds_zones_destroy(yds_zones *z) {
    if (z) { delete z->z; delete z; }
}
int yds_zones_set_stream(yds_zones *z, int stream, const int32_t *zone_ptr, const int32_t *zone_xy, const int32_t *zone_class,
                         const int32_t *zone_min_sightings, int n_zones, const int32_t *line_xy, const int32_t *line_class, int n_lines) {
    YDS_API_BEGIN
    impl(z)->set_stream(stream, zone_ptr, zone_xy, zone_class, zone_min_sightings, n_zones, line_xy, line_class, n_lines);
    YDS_API_END
}
int yds_zones_reset(yds_zones *z, int stream) {
    YDS_API_BEGIN
    impl(z)->reset(stream);
    YDS_API_END
}
int yds_zones_update(yds_zones *z, const int32_t *rows6_host, const int32_t *first, const int32_t *stream_of, const double *frame_time,
                     int n_frames, int32_t *ev6_host, double *evt2_host, int cap, int *n_out) {
    YDS_API_BEGIN
    yds::Zones *Zn = impl(z);
    const std::vector<yds::ActFrame> fr = yds::csr_frames("zones", rows6_host, first, stream_of, frame_time, false, n_frames, n_out);
    if (fr.empty()) return 0;
    Zn->enqueue_ex(fr.data(), n_frames, Zn->own_stream, rows6_host, (size_t)first[n_frames]);
    Zn->finish_alone();
    const int m = Zn->give_count("events", (int)(Zn->report.rows.size() / 6), cap, n_out);
    if (m) {
        memcpy(ev6_host, Zn->report.rows.data(), (size_t)m * 6 * sizeof(int32_t));
        memcpy(evt2_host, Zn->report.times.data(), (size_t)m * 2 * sizeof(double));
    }
    YDS_API_END
}
int yds_zones_get_counts(yds_zones *z, int stream, int32_t *zone4, int32_t *line2) {
    YDS_API_BEGIN
    yds::Zones *Zn = impl(z);
    Zn->check_stream(stream);
    int c[yds::N_CTR];
    YDS_HIP(hipMemcpy(c, Zn->ctr.p + (size_t)stream * yds::N_CTR, sizeof c, hipMemcpyDeviceToHost));
    if (zone4) memcpy(zone4, c, (size_t)Zn->nz[stream] * 4 * sizeof(int32_t));
    if (line2) memcpy(line2, c + yds::ZMAX * 4, (size_t)Zn->nl[stream] * 2 * sizeof(int32_t));
    YDS_API_END
}
int yds_zones_get_tracks(yds_zones *z, int stream, int32_t *ids, int32_t *ages, int32_t *inside_mask, int cap, int *n) {
    YDS_API_BEGIN
    yds::Zones *Zn = impl(z);
    const int m = Zn->table_count(stream, "tracks", cap, n);
    const yds::ZoneTab t = Zn->dev_tab(stream);
    Zn->column_out(ids, t.id, m);
    Zn->column_out(ages, t.age, m);
    Zn->column_out(inside_mask, t.mask, m);
    YDS_API_END
}
int yds_zones_set_timing(yds_zones *z, int on) {
    YDS_API_BEGIN
    impl(z)->timer.set(on != 0);
    YDS_API_END
}
int yds_zones_last_us(yds_zones *z, float *us) {
    YDS_API_BEGIN
    *us = impl(z)->timer.us("zones");
    YDS_API_END
}

}  // extern "C"
