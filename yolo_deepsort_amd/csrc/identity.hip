// Cross-camera identities: one global id per person over the trackers of S cameras, kept where the galleries live (HBM).
//
// No reference counterpart: the reference tracks one camera.  The semantics are those of include/ydsort.h (yds_identity_update);
// tests/identity_ref.py restates them in numpy / scipy.  The map is a pair (owner track id, global id) per stream and gallery slot:
// a live track HOLDS global id g iff its slot's pair names the track's own id and g > 0, so a slot that changes hands never hands
// an identity on and no stage here writes tracker state.
//   ident_collect_kernel   one workgroup over all trackers: per track its stream / held id, the Confirmed tracks of every stream for
//                          the host copy, the new tracks (Confirmed, no id) in (stream, track-list) order, the admission prefix
//                          (gallery rows <= max_rows) and the counts - stored to pinned host memory, read with the caller's own
//                          synchronisation
//   ident_gather_kernel    the admitted tracks' gallery rows (stored normalised) -> a dense query block [Q][512]
//   gallery_min_dist_kernel (gallery_search.hip, unchanged)  dist[Q][T]: the search's exact-fp32 512-term chains
//   ident_reduce_kernel    segmented minimum over each new track's rows: D2[N][T], coalesced along T
//   ident_resolve_kernel   one workgroup, streams 0 .. S-1 in turn: columns = ids held in other streams and not in this one, cost =
//                          min over the holders, min_cost_matching's clamp, the device LSAP (tracker_lsap_dev.h), gate, pairs, counter
// A step in which no track needs an identity costs the collect launch alone and no synchronisation of its own; the other four run
// at their exact sizes behind it, with one more synchronisation, only when a track was admitted.
#include "gallery_dev.h"
#include "tracker_lsap_dev.h"

#include <limits.h>

namespace yds {

// One tracker as the collect and resolve kernels read it (pinned host memory, rewritten ahead of every collect: a step may move
// the tracker's buffers).  pair: [cap][2] ints of this map, indexed by the tracker's slot.
struct alignas(16) IdentSrc {
    const float *gallery;
    const int *slot, *id, *state, *n_feat, *n_tracks;
    int *pair;
    int budget, cap;
};
static_assert(sizeof(IdentSrc) % 16 == 0, "IdentSrc arrays are indexed at a stride of sizeof(IdentSrc)");

// counts of an update, in pinned host memory
enum IdentCount { IC_T = 0, IC_NCONF, IC_NNEW, IC_NADM, IC_Q, IC_NLINK, IC_NFRESH, IC_NEXT, IC_COUNT };

// Device arrays of the map, sized by the sum of the trackers' slot counts (no step can leave more tracks).  g = index of a track in
// (stream, track-list) order over all trackers; n = index of a new track in the same order.
struct IdentDev {
    int *g_stream, *g_gid, *g_conf, *g_hpos, *g_uk;     // stream, held id (0: none), Confirmed, place in the host list, index into U
    int *new_g, *new_rows, *new_q0;                     // new track n: its g, gallery rows, first row of its queries
    int *U, *flag_s, *flag_o, *colk, *colof;            // U: held ids ascending; per id: held in / outside the stream; columns
    int *link_col, *fresh_rank, *rows, *cols, *misc;    // per new track of the stream; LSAP pairs; misc[0] = LSAP pair count
    int *next_id;                                       // the one counter of all streams (next id to hand out)
};

// the inverse of ordered_bits (gallery_dev.h)
__device__ __forceinline__ float ident_from_ordered(unsigned b) {
    if (b == 0xffffffffu) return INFINITY;                                    // (the initial value: no holder seen)
    return __uint_as_float((b & 0x80000000u) ? (b & 0x7fffffffu) : ~b);
}

// hl: first [S + 1] | track id [cap_total] | global id [cap_total] of the Confirmed tracks, stream by stream in track-list order
__global__ __launch_bounds__(256) void ident_collect_kernel(const IdentSrc *src, int S, int max_rows, int cap_total, GalleryDesc *gdesc, IdentDev d,
                                                            int *counts, int *hl) {
    __shared__ int s_cnt[4];
    __shared__ int s_scan[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *hl_id = hl + S + 1, *hl_gid = hl_id + cap_total;
    int g0 = 0, n_conf = 0, n_new = 0;
    for (int s = 0; s < S; ++s) {
        const IdentSrc e = src[s];
        const int T = min(min(max(*e.n_tracks, 0), e.cap), cap_total - g0);
        if (tid == 0) {
            gdesc[s] = GalleryDesc{e.gallery, e.slot, e.id, e.state, e.n_feat, e.budget, g0, T, s};
            hl[s] = n_conf;
        }
        for (int t = tid; t < T; t += 256) {
            const int g = g0 + t, slot = e.slot[t];
            const int conf = e.state[t] == CONFIRMED ? 1 : 0;
            int gid = 0;
            if (conf && slot >= 0 && slot < e.cap) {
                const int owner = e.pair[2 * slot], held = e.pair[2 * slot + 1];
                if (owner == e.id[t] && held > 0) gid = held;
            }
            d.g_stream[g] = s; d.g_gid[g] = gid; d.g_conf[g] = conf; d.g_hpos[g] = -1; d.g_uk[g] = -1;
        }
        __syncthreads();
        const int c = compact_ordered(T, s_cnt, [&](int t) { return d.g_conf[g0 + t] != 0; },
                                      [&](int t, int r) { hl_id[n_conf + r] = e.id[t]; hl_gid[n_conf + r] = d.g_gid[g0 + t]; d.g_hpos[g0 + t] = n_conf + r; });
        const int m = compact_ordered(T, s_cnt, [&](int t) { return d.g_conf[g0 + t] != 0 && d.g_gid[g0 + t] == 0; },
                                      [&](int t, int r) { d.new_g[n_new + r] = g0 + t; d.new_rows[n_new + r] = min(max(e.n_feat[t], 0), e.budget); });
        n_conf += c; n_new += m; g0 += T;
    }
    __syncthreads();
    // admission: new tracks while their rows sum to at most max_rows; rows are >= 0, so "inclusive sum <= max_rows" IS a prefix
    int cum = 0, n_adm = 0;
    for (int base = 0; base < n_new; base += 256) {
        const int i = base + tid;
        const int rows = i < n_new ? d.new_rows[i] : 0;
        int x = rows;
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
        if (lane == 63) s_scan[wave] = x;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const int v = s_scan[w]; if (w < wave) woff += v; tot += v; }
        const int incl = cum + woff + x;
        const bool adm = i < n_new && incl <= max_rows;
        if (i < n_new) d.new_q0[i] = incl - rows;
        n_adm += __syncthreads_count(adm);
        cum += tot;
    }
    __syncthreads();
    if (tid == 0) {
        hl[S] = n_conf;
        counts[IC_T] = g0; counts[IC_NCONF] = n_conf; counts[IC_NNEW] = n_new; counts[IC_NADM] = n_adm;
        counts[IC_Q] = n_adm ? d.new_q0[n_adm - 1] + d.new_rows[n_adm - 1] : 0;
        counts[IC_NLINK] = 0; counts[IC_NFRESH] = 0; counts[IC_NEXT] = *d.next_id;
    }
}

// workgroup n: the rows of admitted track n, as stored, to rows [q0, q0 + rows) of the query block
__global__ __launch_bounds__(256) void ident_gather_kernel(const GalleryDesc *gdesc, IdentDev d, float *qn) {
    const int n = blockIdx.x, g = d.new_g[n];
    const GalleryDesc &e = gdesc[d.g_stream[g]];
    const int t = g - e.g0, rows = d.new_rows[n];
    const float4 *src = reinterpret_cast<const float4 *>(e.gallery + (size_t)e.slot[t] * e.budget * EMB);
    float4 *dst = reinterpret_cast<float4 *>(qn + (size_t)d.new_q0[n] * EMB);
    for (int i = threadIdx.x; i < rows * (EMB / 4); i += 256) dst[i] = src[i];
}

// D2[n][g] = min over the query rows of new track n; grid (ceil(T / 256), N)
__global__ __launch_bounds__(256) void ident_reduce_kernel(const float *dist, IdentDev d, int T, float *D2) {
    const int g = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (g >= T) return;
    const int q0 = d.new_q0[n], rows = d.new_rows[n];
    float m = INFINITY;
    for (int q = 0; q < rows; ++q) m = fminf(m, dist[(size_t)(q0 + q) * T + g]);
    D2[(size_t)n * T + g] = m;
}

// ascending bitonic sort of P (a power of two) ints by the workgroup; a: LDS or global
__device__ __forceinline__ void ident_sort(int *a, int P) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const int x = a[i], y = a[l];
                    if (((i & k) == 0) == (x > y)) { a[i] = y; a[l] = x; }
                }
            }
            __syncthreads();
        }
}

// One workgroup; N admitted new tracks, T tracks.  sort_global: where the held ids are sorted when their padded count P exceeds the
// dynamic LDS (else the LDS, which the LSAP takes over afterwards).  cost: [max new tracks of a stream][columns] scratch, first as
// ordered bits, then as floats.  lk: stream | track id | global id | cost bits, [cap_total] each, of the linked tracks.
__global__ __launch_bounds__(256) void ident_resolve_kernel(const IdentSrc *src, const GalleryDesc *gdesc, int S, int N, int T, int P, IdentDev d,
                                                            const float *D2, float max_dist, float flood, float *cost, int *sort_global,
                                                            char *lsap_state, int smem_bytes, int cap_total, int *counts, int *hl, int *lk) {
    extern __shared__ __attribute__((aligned(16))) char lsap_smem[];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    int *hl_gid = hl + S + 1 + cap_total;
    unsigned *cost_bits = reinterpret_cast<unsigned *>(cost);
    // ---- U: the ids held by a live track, ascending (fresh ids are appended as they are handed out: they only grow)
    int *sb = sort_global ? sort_global : reinterpret_cast<int *>(lsap_smem);
    for (int i = tid; i < P; i += 256) sb[i] = INT_MAX;
    __syncthreads();
    const int h = compact_ordered(T, s_cnt, [&](int g) { return d.g_gid[g] > 0; }, [&](int g, int r) { sb[r] = d.g_gid[g]; });
    __syncthreads();
    ident_sort(sb, P);
    int nU = compact_ordered(h, s_cnt, [&](int i) { return i == 0 || sb[i] != sb[i - 1]; }, [&](int i, int r) { d.U[r] = sb[i]; });
    __syncthreads();
    for (int g = tid; g < T; g += 256) {
        const int gid = d.g_gid[g];
        int k = -1;
        if (gid > 0) {
            int lo = 0, hi = nU;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (d.U[mid] < gid) lo = mid + 1; else hi = mid; }
            k = lo;
        }
        d.g_uk[g] = k;
    }
    __syncthreads();
    int next = *d.next_id, n0 = 0, n_link = 0, n_fresh = 0;
    for (int s = 0; s < S && n0 < N; ++s) {
        // the admitted new tracks of stream s: [n0, n0 + ns) (the list is in stream order)
        int ns = 0;
        for (int base = n0; base < N; base += 256) {
            const int n = base + tid;
            const int c = __syncthreads_count(n < N && d.g_stream[d.new_g[n]] == s);
            ns += c;
            if (c < min(256, N - base)) break;                                // (uniform: c is the same in every thread)
        }
        if (ns == 0) continue;
        // ---- columns: ids with a holder outside s and none in s, ascending
        for (int k = tid; k < nU; k += 256) { d.flag_s[k] = 0; d.flag_o[k] = 0; d.colof[k] = -1; }
        __syncthreads();
        for (int g = tid; g < T; g += 256) {
            const int k = d.g_uk[g];
            if (k >= 0) { if (d.g_stream[g] == s) d.flag_s[k] = 1; else d.flag_o[k] = 1; }
        }
        __syncthreads();
        const int nc = compact_ordered(nU, s_cnt, [&](int k) { return d.flag_o[k] && !d.flag_s[k]; }, [&](int k, int c) { d.colk[c] = k; d.colof[k] = c; });
        __syncthreads();
        // ---- cost[n][c] = min over the holders g of column c of D2[n][g] (every holder of a column sits outside s)
        for (int i = tid; i < ns * nc; i += 256) cost_bits[i] = 0xffffffffu;
        __syncthreads();
        if (nc > 0)
            for (size_t i = tid; i < (size_t)ns * T; i += 256) {
                const int n = (int)(i / T), g = (int)(i - (size_t)n * T);
                const int k = d.g_uk[g];
                const int c = k >= 0 ? d.colof[k] : -1;
                if (c >= 0) atomicMin(&cost_bits[(size_t)n * nc + c], ordered_bits(D2[(size_t)(n0 + n) * T + g]));
            }
        __syncthreads();
        for (int i = tid; i < ns * nc; i += 256) {
            const float v = ident_from_ordered(cost_bits[i]);
            cost[i] = v > max_dist ? flood : v;                               // linear_assignment.py:52
        }
        __syncthreads();
        // ---- min_cost_matching: scipy's assignment, pairs above the threshold dropped (linear_assignment.py:51-72)
        lsap_solve_block(cost, ns, nc, d.rows, d.cols, d.misc, lsap_state, smem_bytes);
        const int n_pairs = nc > 0 ? d.misc[0] : 0;
        for (int n = tid; n < ns; n += 256) d.link_col[n] = -1;
        __syncthreads();
        for (int p = tid; p < n_pairs; p += 256) {
            const int r = d.rows[p], c = d.cols[p];
            if (!(cost[(size_t)r * nc + c] > max_dist)) d.link_col[r] = c;
        }
        __syncthreads();
        const int nl = compact_ordered(ns, s_cnt, [&](int n) { return d.link_col[n] >= 0; }, [&](int n, int r) { d.fresh_rank[n] = -1 - (n_link + r); });
        const int nf = compact_ordered(ns, s_cnt, [&](int n) { return d.link_col[n] < 0; }, [&](int n, int r) { d.fresh_rank[n] = r; });
        __syncthreads();
        // ---- hand the ids out: a matched track takes the column's id, every other one the next fresh id in track-list order
        const IdentSrc e = src[s];
        const GalleryDesc ge = gdesc[s];
        for (int n = tid; n < ns; n += 256) {
            const int g = d.new_g[n0 + n], t = g - ge.g0, fr = d.fresh_rank[n];
            int gid, k;
            if (fr < 0) {
                const int c = d.link_col[n], at = -1 - fr;
                k = d.colk[c]; gid = d.U[k];
                lk[at] = s; lk[cap_total + at] = e.id[t]; lk[2 * cap_total + at] = gid;
                lk[3 * cap_total + at] = __float_as_int(cost[(size_t)n * nc + c]);
            } else {
                gid = next + fr; k = nU + fr;
                d.U[k] = gid;
            }
            d.g_uk[g] = k; d.g_gid[g] = gid;
            const int slot = e.slot[t];
            if (slot >= 0 && slot < e.cap) { e.pair[2 * slot] = e.id[t]; e.pair[2 * slot + 1] = gid; }
            const int hp = d.g_hpos[g];
            if (hp >= 0) hl_gid[hp] = gid;
        }
        nU += nf; next += nf; n_link += nl; n_fresh += nf; n0 += ns;
        __syncthreads();
    }
    if (tid == 0) {
        *d.next_id = next;
        counts[IC_NLINK] = n_link; counts[IC_NFRESH] = n_fresh; counts[IC_NEXT] = next;
    }
}

// ============================================================================================ host
namespace {

constexpr int kDevArrays = 18;                     // the int arrays of IdentDev, cap_total entries each

}  // namespace

class Identity : public IdentityIface {
public:
    struct Link { int stream, track_id, global_id; float cost; };

    Identity(yds_trk *const *handles, int n_streams, float max_dist_in, int max_rows)
        : max_rows(max_rows) {
        const char *who = "identity_create";
        if (!handles || n_streams < 1) fail("%s: no trackers given", who);
        int max_budget = 0;
        for (int a = 0; a < n_streams; ++a) {
            if (!handles[a] || !handles[a]->t) fail("%s: tracker %d is NULL", who, a);
            for (int b = 0; b < a; ++b)
                if (handles[a] == handles[b] || handles[a]->t == handles[b]->t) fail("%s: streams %d and %d share one tracker", who, b, a);
            const GalleryView v = handles[a]->t->gallery_view();
            if (v.metric != METRIC_COSINE)
                fail("%s: tracker %d uses the euclidean metric: its gallery rows are not normalised, identities are linked by cosine distance", who, a);
            if (v.unbounded)
                fail("%s: tracker %d has nn_budget=None: the map needs galleries of a bounded size (pass a finite nn_budget)", who, a);
            max_budget = std::max(max_budget, v.budget);
            trks.push_back(handles[a]->t);
        }
        if (max_rows < max_budget)
            fail("%s: max_rows = %d is below the largest nn_budget %d: a track with a full gallery could never be admitted", who, max_rows, max_budget);
        const double md = max_dist_in < 0.f ? trks[0]->gallery_view().max_dist : (double)max_dist_in;     // < 0: the first tracker's threshold
        max_dist = (float)md;
        flood = (float)(md + 1e-5);                                           // linear_assignment.py:52
        const int S = n_streams;
        pair.resize(S);
        pair_cap.assign(S, 0);
        src.ensure((size_t)S);
        counts.ensure(IC_COUNT);
        memset(counts.p, 0, IC_COUNT * sizeof(int));
        gdesc.alloc((size_t)S);
        next_id.alloc(1);
        const int one = 1;
        YDS_HIP(hipMemcpy(next_id.p, &one, 4, hipMemcpyHostToDevice));
        first.assign(S + 1, 0);
        stream = make_stream(true);
        YDS_HIP(hipEventCreate(&ev0));
        YDS_HIP(hipEventCreate(&ev1));
    }
    ~Identity() override {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }

    bool bound_to(TrackerIface *const *trk, int S) const override {
        if (S != (int)trks.size()) return false;
        for (int s = 0; s < S; ++s) if (trk[s] != trks[s]) return false;
        return true;
    }

    // forget every pair; the counter keeps counting
    void reset() {
        for (size_t s = 0; s < pair.size(); ++s)
            if (pair_cap[s]) YDS_HIP(hipMemset(pair[s].p, 0, (size_t)pair_cap[s] * 2 * sizeof(int)));
        first.assign(trks.size() + 1, 0);
        ids_track.clear(); ids_global.clear(); links.clear();
        n_linked = n_fresh = n_deferred = 0;
        resolve_ran = false;
    }

    void enqueue_collect(hipStream_t s) override {
        const int S = (int)trks.size();
        cap_total = 0;
        max_cap = 0;
        for (int a = 0; a < S; ++a) {
            const GalleryView v = trks[a]->gallery_view();
            if (v.capacity > pair_cap[a]) {                                   // the tracker grew: its slots keep their numbers
                DevBuf<int> p((size_t)v.capacity * 2);
                YDS_HIP(hipMemset(p.p, 0, (size_t)v.capacity * 2 * sizeof(int)));
                if (pair_cap[a]) YDS_HIP(hipMemcpy(p.p, pair[a].p, (size_t)pair_cap[a] * 2 * sizeof(int), hipMemcpyDeviceToDevice));
                pair[a] = std::move(p);
                pair_cap[a] = v.capacity;
            }
            src.p[a] = IdentSrc{v.gallery, v.slot, v.id, v.state, v.n_feat, v.n_tracks_dev, pair[a].p, v.budget, v.capacity};
            cap_total += v.capacity;
            max_cap = std::max(max_cap, v.capacity);
        }
        if ((size_t)cap_total * kDevArrays > arrays.n) arrays.alloc((size_t)cap_total * kDevArrays * 2);
        int *a = arrays.p;
        auto take = [&]() { int *r = a; a += cap_total; return r; };
        dev.g_stream = take(); dev.g_gid = take(); dev.g_conf = take(); dev.g_hpos = take(); dev.g_uk = take();
        dev.new_g = take(); dev.new_rows = take(); dev.new_q0 = take();
        dev.U = take(); dev.flag_s = take(); dev.flag_o = take(); dev.colk = take(); dev.colof = take();
        dev.link_col = take(); dev.fresh_rank = take(); dev.rows = take(); dev.cols = take(); dev.misc = take();
        dev.next_id = next_id.p;
        hl.ensure((size_t)S + 1 + 2 * (size_t)cap_total);
        lk.ensure(4 * (size_t)cap_total);
        hipLaunchKernelGGL(ident_collect_kernel, dim3(1), dim3(256), 0, s, src.p, S, max_rows, cap_total, gdesc.p, dev, counts.p, hl.p);
        YDS_HIP(hipGetLastError());
    }

    void finish(hipStream_t s) override {
        const int S = (int)trks.size();
        const int T = counts.p[IC_T], N = counts.p[IC_NADM], Q = counts.p[IC_Q];
        n_deferred = counts.p[IC_NNEW] - N;
        n_linked = n_fresh = 0;
        links.clear();
        resolve_ran = false;
        if (N > 0) {
            // ---- the resolve sequence at its exact sizes, one more synchronisation
            int P = 1;
            while (P < T) P <<= 1;
            const int R = std::min(N, max_cap);                               // the most new tracks one stream can bring
            const size_t lsap_need = (size_t)std::max(std::max(R, T), 1) * LSAP_STATE_BYTES;
            qn.ensure((size_t)Q * EMB);
            dist.ensure((size_t)Q * T);
            D2.ensure((size_t)N * T);
            cost.ensure((size_t)R * T);
            if ((size_t)P * sizeof(int) > LSAP_LDS_MAX) sort_global.ensure((size_t)P);
            if (lsap_need > LSAP_LDS_MAX) lsap_scratch.ensure(lsap_need);
            static bool attr_set = false;
            if (!attr_set) {
                YDS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ident_resolve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LSAP_LDS_MAX));
                attr_set = true;
            }
            if (timing) YDS_HIP(hipEventRecord(ev0, s));
            hipLaunchKernelGGL(ident_gather_kernel, dim3(N), dim3(256), 0, s, gdesc.p, dev, qn.p);
            hipLaunchKernelGGL(gallery_min_dist_kernel, dim3(T, (Q + GALLERY_SLAB - 1) / GALLERY_SLAB), dim3(256), 0, s, gdesc.p, S, qn.p, Q, dist.p, T);
            hipLaunchKernelGGL(ident_reduce_kernel, dim3((T + 255) / 256, N), dim3(256), 0, s, dist.p, dev, T, D2.p);
            hipLaunchKernelGGL(ident_resolve_kernel, dim3(1), dim3(256), LSAP_LDS_MAX, s, src.p, gdesc.p, S, N, T, P, dev, D2.p, max_dist, flood, cost.p,
                               (size_t)P * sizeof(int) > LSAP_LDS_MAX ? sort_global.p : nullptr, lsap_need > LSAP_LDS_MAX ? lsap_scratch.p : nullptr,
                               (int)LSAP_LDS_MAX, cap_total, counts.p, hl.p, lk.p);
            if (timing) YDS_HIP(hipEventRecord(ev1, s));
            YDS_HIP(hipGetLastError());
            YDS_HIP(hipStreamSynchronize(s));
            resolve_ran = true;
            if (timing) {
                float ms = 0.f;
                YDS_HIP(hipEventElapsedTime(&ms, ev0, ev1));
                last_us = ms * 1e3f;
            }
            n_linked = counts.p[IC_NLINK];
            n_fresh = counts.p[IC_NFRESH];
            for (int k = 0; k < n_linked; ++k) {
                float c;
                memcpy(&c, lk.p + 3 * (size_t)cap_total + k, 4);
                links.push_back(Link{lk.p[k], lk.p[cap_total + k], lk.p[2 * (size_t)cap_total + k], c});
            }
        }
        // ---- the host copy of the map
        const int n_conf = counts.p[IC_NCONF];
        first.assign(hl.p, hl.p + S + 1);
        ids_track.assign(hl.p + S + 1, hl.p + S + 1 + n_conf);
        ids_global.assign(hl.p + S + 1 + cap_total, hl.p + S + 1 + cap_total + n_conf);
    }

    void update() {
        enqueue_collect(stream);
        YDS_HIP(hipStreamSynchronize(stream));
        finish(stream);
    }

    void get(int s, int32_t *track_id, int32_t *global_id, int cap, int *n) const override {
        if (s < 0 || s >= (int)trks.size()) fail("identity_get: stream %d outside [0, %zu)", s, trks.size());
        if (!n) fail("identity_get: n is NULL");
        const int m = first[s + 1] - first[s];
        *n = m;
        if (m > cap) fail("identity_get: cap = %d too small for %d tracks (the needed size is in *n)", cap, m);
        if (m && (!track_id || !global_id)) fail("identity_get: an output array is NULL");
        for (int k = 0; k < m; ++k) { track_id[k] = ids_track[first[s] + k]; global_id[k] = ids_global[first[s] + k]; }
    }

    std::vector<TrackerIface *> trks;
    float max_dist = 0.f, flood = 0.f;
    int max_rows;
    hipStream_t stream = nullptr;                 // of the stand-alone update
    std::vector<DevBuf<int>> pair;                // per stream [slots][2]: owner track id, global id
    std::vector<int> pair_cap;
    PinBuf<IdentSrc> src;
    PinBuf<int> counts, hl, lk;
    DevBuf<GalleryDesc> gdesc;
    DevBuf<int> arrays, next_id, sort_global;
    DevBuf<float> qn, dist, D2, cost;
    DevBuf<char> lsap_scratch;
    IdentDev dev{};
    int cap_total = 0, max_cap = 0;
    // the last update, on the host
    std::vector<int> first, ids_track, ids_global;
    std::vector<Link> links;
    int n_linked = 0, n_fresh = 0, n_deferred = 0;
    bool resolve_ran = false, timing = false;
    float last_us = -1.f;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

}  // namespace yds

// ============================================================================================ C ABI
static inline yds::Identity *impl(yds_ident *h) {
    if (!h || !h->i) yds::fail("identity: NULL handle");
    return static_cast<yds::Identity *>(h->i);
}

extern "C" {

yds_ident *yds_identity_create(yds_trk *const *trks, int n_streams, float max_dist, int max_rows) {
    YDS_API_BEGIN
    return new yds_ident{new yds::Identity(trks, n_streams, max_dist, max_rows)};
    YDS_API_END_PTR
}
void yds_identity_destroy(yds_ident *h) {
    if (!h) return;
    delete h->i;
    delete h;
}
int yds_identity_reset(yds_ident *h) {
    YDS_API_BEGIN
    impl(h)->reset();
    YDS_API_END
}
int yds_identity_update(yds_ident *h, int *n_linked, int *n_fresh, int *n_deferred) {
    YDS_API_BEGIN
    yds::Identity *I = impl(h);
    I->update();
    if (n_linked) *n_linked = I->n_linked;
    if (n_fresh) *n_fresh = I->n_fresh;
    if (n_deferred) *n_deferred = I->n_deferred;
    YDS_API_END
}
int yds_identity_get(yds_ident *h, int stream, int32_t *track_id, int32_t *global_id, int cap, int *n) {
    YDS_API_BEGIN
    impl(h)->get(stream, track_id, global_id, cap, n);
    YDS_API_END
}
int yds_identity_last_links(yds_ident *h, int32_t *stream, int32_t *track_id, int32_t *global_id, float *cost, int cap, int *n) {
    YDS_API_BEGIN
    const yds::Identity *I = impl(h);
    if (!n) yds::fail("identity_last_links: n is NULL");
    const int m = (int)I->links.size();
    *n = m;
    if (m > cap) yds::fail("identity_last_links: cap = %d too small for %d links (the needed size is in *n)", cap, m);
    if (m && (!stream || !track_id || !global_id || !cost)) yds::fail("identity_last_links: an output array is NULL");
    for (int k = 0; k < m; ++k) {
        stream[k] = I->links[k].stream; track_id[k] = I->links[k].track_id; global_id[k] = I->links[k].global_id; cost[k] = I->links[k].cost;
    }
    YDS_API_END
}
int yds_identity_last_counts(yds_ident *h, int *n_linked, int *n_fresh, int *n_deferred) {
    YDS_API_BEGIN
    const yds::Identity *I = impl(h);
    if (n_linked) *n_linked = I->n_linked;
    if (n_fresh) *n_fresh = I->n_fresh;
    if (n_deferred) *n_deferred = I->n_deferred;
    YDS_API_END
}
int yds_identity_set_timing(yds_ident *h, int on) {
    YDS_API_BEGIN
    impl(h)->timing = on != 0;
    impl(h)->last_us = -1.f;
    YDS_API_END
}
int yds_identity_last_us(yds_ident *h, float *us) {
    YDS_API_BEGIN
    const yds::Identity *I = impl(h);
    if (!us) yds::fail("identity_last_us: us is NULL");
    *us = I->timing && I->resolve_ran ? I->last_us : -1.f;     // -1: the last update launched no resolve sequence (or timing is off)
    YDS_API_END
}

}  // extern "C"
