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
// With a memory (identity_memory_dev.h, off by default) two launches follow the collect ahead of that same synchronisation - the
// book kernel and the row copies - and the resolve sequence gains the bank distance kernel and E = max_ids more columns: D2 is
// [N][T + E], a departed entry (used, no live holder) is a column of every stream, its cost read straight from D2.
#include "identity_memory_dev.h"
#include "tracker_lsap_dev.h"

#include <limits.h>

namespace yds {

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

// One workgroup; N admitted new tracks, T tracks, D2 rows of ldd = T + m.max_ids values.  sort_global: where the held ids are sorted when their padded count P exceeds the
// dynamic LDS (else the LDS, which the LSAP takes over afterwards).  cost: [max new tracks of a stream][columns] scratch, first as
// ordered bits, then as floats.  lk: stream | track id | global id | cost bits, [cap_total] each, of the linked tracks.
__global__ __launch_bounds__(256) void ident_resolve_kernel(const IdentSrc *src, const GalleryDesc *gdesc, int S, int N, int T, int P, IdentDev d,
                                                            IdentMem m, const float *D2, float max_dist, float flood, float *cost, int *sort_global,
                                                            char *lsap_state, int smem_bytes, int cap_total, int *counts, int *hl, int *lk) {
    extern __shared__ __attribute__((aligned(16))) char lsap_smem[];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const int E = m.max_ids, ldd = T + E;
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
    int next = *d.next_id, n0 = 0, n_link = 0, n_fresh = 0, n_relinked = 0;
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
        const int nch = compact_ordered(nU, s_cnt, [&](int k) { return d.flag_o[k] && !d.flag_s[k]; }, [&](int k, int c) { d.colk[c] = k; d.colof[k] = c; });
        // ---- behind them the departed ids: used entries without a live holder (one relinked earlier in this resolve is live)
        const int nd = E ? compact_ordered(E, s_cnt, [&](int e) { return m.gid[e] > 0 && m.n[e] > 0 && !m.live[e]; }, [&](int e, int c) { m.dcol[c] = e; }) : 0;
        const int nc = nch + nd;
        __syncthreads();
        // ---- cost[n][c] = min over the holders g of column c of D2[n][g] (every holder of a column sits outside s)
        for (int i = tid; i < ns * nc; i += 256) cost_bits[i] = 0xffffffffu;
        __syncthreads();
        if (nch > 0)
            for (size_t i = tid; i < (size_t)ns * T; i += 256) {
                const int n = (int)(i / T), g = (int)(i - (size_t)n * T);
                const int k = d.g_uk[g];
                const int c = k >= 0 ? d.colof[k] : -1;
                if (c >= 0) atomicMin(&cost_bits[(size_t)n * nc + c], ordered_bits(D2[(size_t)(n0 + n) * ldd + g]));
            }
        __syncthreads();
        for (int i = tid; i < ns * nc; i += 256) {
            const int n = i / nc, c = i - n * nc;
            const float v = c < nch ? ident_from_ordered(cost_bits[i]) : D2[(size_t)(n0 + n) * ldd + T + m.dcol[c - nch]];
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
        const int nr = nd ? compact_ordered(ns, s_cnt, [&](int n) { return d.link_col[n] >= nch; }, [&](int n, int r) { m.g_rank[n] = r; }) : 0;
        __syncthreads();
        // ---- hand the ids out: a matched track takes the column's id, every other one the next fresh id in track-list order; an id
        //      taken from the bank has a live holder from here on and joins U behind the fresh ones (m.g_rank: its rank, scratch)
        const IdentSrc e = src[s];
        const GalleryDesc ge = gdesc[s];
        for (int n = tid; n < ns; n += 256) {
            const int g = d.new_g[n0 + n], t = g - ge.g0, fr = d.fresh_rank[n];
            int gid, k;
            if (fr < 0) {
                const int c = d.link_col[n], at = -1 - fr;
                if (c < nch) { k = d.colk[c]; gid = d.U[k]; }
                else {
                    const int en = m.dcol[c - nch];
                    gid = m.gid[en]; k = nU + nf + m.g_rank[n];
                    d.U[k] = gid;
                    m.live[en] = 1; m.last[en] = m.u;
                }
                lk[4 * cap_total + at] = c >= nch ? 1 : 0;
                lk[at] = s; lk[cap_total + at] = e.id[t]; lk[2 * cap_total + at] = gid;
                lk[3 * cap_total + at] = __float_as_int(cost[(size_t)n * nc + c]);
            } else {
                gid = next + fr; k = nU + fr;
                d.U[k] = gid;
            }
            d.g_uk[g] = k; d.g_gid[g] = gid;
            const int slot = e.slot[t];
            if (slot >= 0 && slot < e.cap) {
                e.pair[2 * slot] = e.id[t]; e.pair[2 * slot + 1] = gid;
                if (e.rem) e.rem[slot] = 0;                                   // (hits >= 1: the next update remembers its newest row)
            }
            const int hp = d.g_hpos[g];
            if (hp >= 0) hl_gid[hp] = gid;
        }
        nU += nf + nr; next += nf; n_link += nl; n_fresh += nf; n_relinked += nr; n0 += ns;
        __syncthreads();
    }
    if (tid == 0) {
        *d.next_id = next;
        counts[IC_NLINK] = n_link; counts[IC_NFRESH] = n_fresh; counts[IC_NEXT] = next;
        if (E) { counts[IC_M_RELINKED] = n_relinked; counts[IC_M_DEPARTED] -= n_relinked; }
    }
}

// ============================================================================================ host
namespace {

constexpr int kDevArrays = 18;                     // the int arrays of IdentDev, cap_total entries each
constexpr int kMemArrays = 5;                      // the per-track / per-id int arrays of IdentMem, cap_total entries each
constexpr int kMemEntryArrays = 8;                 // its per-entry int arrays, max_ids entries each
constexpr int kMaxMemoryIds = 65536;
constexpr int kBankStrip = 8;                      // bank tiles per workgroup of ident_bank_dist_kernel (profiles/identity_memory_bench.txt)

template <class... A> void launch_bank_dist(int R, dim3 grid, hipStream_t s, A... a) {
    switch (R) {
    case 1: hipLaunchKernelGGL(ident_bank_dist_kernel<1>, grid, dim3(256), 0, s, a...); break;
    case 2: hipLaunchKernelGGL(ident_bank_dist_kernel<2>, grid, dim3(256), 0, s, a...); break;
    case 4: hipLaunchKernelGGL(ident_bank_dist_kernel<4>, grid, dim3(256), 0, s, a...); break;
    case 8: hipLaunchKernelGGL(ident_bank_dist_kernel<8>, grid, dim3(256), 0, s, a...); break;
    case 16: hipLaunchKernelGGL(ident_bank_dist_kernel<16>, grid, dim3(256), 0, s, a...); break;
    case 32: hipLaunchKernelGGL(ident_bank_dist_kernel<32>, grid, dim3(256), 0, s, a...); break;
    default: fail("identity memory: rows_per_id = %d", R);
    }
}

}  // namespace

class Identity : public IdentityIface {
public:
    struct Link { int stream, track_id, global_id; float cost; int relinked; };
    struct Entry { int global_id, n_rows, last_held, index, head; };

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
        rem.resize(S);
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

    // forget every pair and every remembered identity; the id counter and the update counter keep counting
    void reset() {
        for (size_t s = 0; s < pair.size(); ++s)
            if (pair_cap[s]) YDS_HIP(hipMemset(pair[s].p, 0, (size_t)pair_cap[s] * 2 * sizeof(int)));
        clear_memory();
        memset(mcounts, 0, sizeof(mcounts));
        first.assign(trks.size() + 1, 0);
        ids_track.clear(); ids_global.clear(); links.clear();
        n_linked = n_fresh = n_deferred = 0;
        resolve_ran = false;
    }

    void enqueue_collect(hipStream_t s) override {
        const int S = (int)trks.size();
        ++n_updates;
        cap_total = 0;
        max_cap = 0;
        for (int a = 0; a < S; ++a) {
            const GalleryView v = trks[a]->gallery_view();
            if (v.capacity > pair_cap[a]) {                                   // the tracker grew: its slots keep their numbers
                DevBuf<int> p((size_t)v.capacity * 2);
                YDS_HIP(hipMemset(p.p, 0, (size_t)v.capacity * 2 * sizeof(int)));
                if (pair_cap[a]) YDS_HIP(hipMemcpy(p.p, pair[a].p, (size_t)pair_cap[a] * 2 * sizeof(int), hipMemcpyDeviceToDevice));
                pair[a] = std::move(p);
                if (mem.max_ids) grow_rem(a, pair_cap[a], v.capacity);
                pair_cap[a] = v.capacity;
            }
            src.p[a] = IdentSrc{v.gallery, v.slot, v.id, v.state, v.n_feat, v.n_tracks_dev, v.hits, pair[a].p, mem.max_ids ? rem[a].p : nullptr,
                                v.budget, v.capacity};
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
        lk.ensure(5 * (size_t)cap_total);
        hipLaunchKernelGGL(ident_collect_kernel, dim3(1), dim3(256), 0, s, src.p, S, max_rows, cap_total, gdesc.p, dev, counts.p, hl.p);
        if (mem.max_ids) {
            // ---- the memory's steps 2-4 behind the collect, ahead of the caller's synchronisation: bookkeeping, then the row copies
            int P = 1;
            while (P < cap_total) P <<= 1;
            if ((size_t)cap_total * kMemArrays + P > mem_arrays.n) mem_arrays.alloc(((size_t)cap_total * kMemArrays + P) * 2);
            int *b = mem_arrays.p;
            auto takem = [&]() { int *r = b; b += cap_total; return r; };
            mem.ent_of = takem(); mem.first_g = takem(); mem.g_ent = takem(); mem.g_rank = takem(); mem.g_pos = takem();
            mem.sortbuf = b;
            mem.u = n_updates;
            hipLaunchKernelGGL(ident_book_kernel, dim3(1), dim3(256), 0, s, src.p, gdesc.p, S, cap_total, dev, mem, counts.p);
            if (cap_total) hipLaunchKernelGGL(ident_remember_kernel, dim3(cap_total), dim3(128), 0, s, src.p, gdesc.p, dev, mem);
        }
        YDS_HIP(hipGetLastError());
    }

    void finish(hipStream_t s) override {
        const int S = (int)trks.size();
        const int T = counts.p[IC_T], N = counts.p[IC_NADM], Q = counts.p[IC_Q], E = mem.max_ids, ldd = T + E;
        n_deferred = counts.p[IC_NNEW] - N;
        n_linked = n_fresh = 0;
        links.clear();
        resolve_ran = false;
        if (N > 0) {
            // ---- the resolve sequence at its exact sizes, one more synchronisation
            int P = 1;
            while (P < T) P <<= 1;
            const int R = std::min(N, max_cap);                               // the most new tracks one stream can bring
            // (columns: at most one per held id and one per bank entry; the LSAP state is sized by the larger side)
            const size_t lsap_need = (size_t)std::max(std::max(R, ldd), 1) * LSAP_STATE_BYTES;
            qn.ensure((size_t)Q * EMB);
            dist.ensure((size_t)Q * ldd);
            D2.ensure((size_t)N * ldd);
            cost.ensure((size_t)R * ldd);
            if ((size_t)P * sizeof(int) > LSAP_LDS_MAX) sort_global.ensure((size_t)P);
            if (lsap_need > LSAP_LDS_MAX) lsap_scratch.ensure(lsap_need);
            static bool attr_set = false;
            if (!attr_set) {
                YDS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ident_resolve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LSAP_LDS_MAX));
                attr_set = true;
            }
            if (timing) YDS_HIP(hipEventRecord(ev0, s));
            hipLaunchKernelGGL(ident_gather_kernel, dim3(N), dim3(256), 0, s, gdesc.p, dev, qn.p);
            hipLaunchKernelGGL(gallery_min_dist_kernel, dim3(T, (Q + GALLERY_SLAB - 1) / GALLERY_SLAB), dim3(256), 0, s, gdesc.p, S, qn.p, Q, dist.p, ldd);
            if (E) launch_bank_dist(mem.R, bank_grid(Q, strip), s, (const float *)mem.rows, (const int *)mem.n, E, strip, (const float *)qn.p, Q, dist.p + T, ldd);
            hipLaunchKernelGGL(ident_reduce_kernel, dim3((ldd + 255) / 256, N), dim3(256), 0, s, dist.p, dev, ldd, D2.p);
            hipLaunchKernelGGL(ident_resolve_kernel, dim3(1), dim3(256), LSAP_LDS_MAX, s, src.p, gdesc.p, S, N, T, P, dev, mem, D2.p, max_dist, flood, cost.p,
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
                links.push_back(Link{lk.p[k], lk.p[cap_total + k], lk.p[2 * (size_t)cap_total + k], c, E ? lk.p[4 * (size_t)cap_total + k] : 0});
            }
        }
        if (E) for (int k = 0; k < 7; ++k) mcounts[k] = counts.p[IC_M_ENTRIES + k];
        // ---- the host copy of the map
        const int n_conf = counts.p[IC_NCONF];
        first.assign(hl.p, hl.p + S + 1);
        ids_track.assign(hl.p + S + 1, hl.p + S + 1 + n_conf);
        ids_global.assign(hl.p + S + 1 + cap_total, hl.p + S + 1 + cap_total + n_conf);
    }

    // ---------------------------------------------------------------------------------------- the memory (yds_identity_set_memory)
    dim3 bank_grid(int Q, int strip_len) const {
        const int n_tiles = (mem.max_ids * mem.R + 31) / 32;
        return dim3((n_tiles + strip_len - 1) / strip_len, (Q + GALLERY_SLAB - 1) / GALLERY_SLAB);
    }

    // rem of stream a for `cap` slots, the first `keep` kept (the tracker grew: its slots keep their numbers)
    void grow_rem(int a, int keep, int cap) {
        DevBuf<int> r((size_t)cap);
        YDS_HIP(hipMemset(r.p, 0, (size_t)cap * sizeof(int)));
        if (keep && rem[a].p) YDS_HIP(hipMemcpy(r.p, rem[a].p, (size_t)keep * sizeof(int), hipMemcpyDeviceToDevice));
        rem[a] = std::move(r);
    }

    // every entry free, every holder's `remembered` void
    void clear_memory() {
        if (!mem.max_ids) return;
        YDS_HIP(hipMemset(mem_entries.p, 0, (size_t)mem.max_ids * kMemEntryArrays * sizeof(int)));
        for (size_t s = 0; s < rem.size(); ++s)
            if (rem[s].p) YDS_HIP(hipMemset(rem[s].p, 0, rem[s].n * sizeof(int)));
    }

    void set_memory(int max_ids, int rows_per_id, int ttl) {
        const char *who = "identity_set_memory";
        if (max_ids < 0 || max_ids > kMaxMemoryIds) fail("%s: max_ids = %d outside [0, %d]", who, max_ids, kMaxMemoryIds);
        if (max_ids && !(rows_per_id == 1 || rows_per_id == 2 || rows_per_id == 4 || rows_per_id == 8 || rows_per_id == 16 || rows_per_id == 32))
            fail("%s: rows_per_id = %d, must be one of 1, 2, 4, 8, 16, 32 (whole entries tile a 32-row tile)", who, rows_per_id);
        if (user && *user && user_busy && user_busy(*user))
            fail("%s: the map's pipeline has a look-ahead pass in flight (consume it with a step first)", who);
        mem = IdentMem{};
        bank.release();
        mem_entries.release();
        mem_arrays.release();
        for (auto &r : rem) r.release();
        memset(mcounts, 0, sizeof(mcounts));
        if (!max_ids) return;
        try {
            bank.alloc((size_t)max_ids * rows_per_id * EMB);
            mem_entries.alloc((size_t)max_ids * kMemEntryArrays);
            for (size_t a = 0; a < rem.size(); ++a)
                if (pair_cap[a]) grow_rem((int)a, 0, pair_cap[a]);
        } catch (const std::exception &e) {
            bank.release();
            mem_entries.release();
            for (auto &r : rem) r.release();
            fail("%s: no memory for %d ids of %d rows: %s", who, max_ids, rows_per_id, e.what());
        }
        int *b = mem_entries.p;
        auto take = [&]() { int *r = b; b += max_ids; return r; };
        mem.rows = bank.p;
        mem.gid = take(); mem.n = take(); mem.head = take(); mem.last = take(); mem.live = take(); mem.cnt = take(); mem.pool = take(); mem.dcol = take();
        mem.max_ids = max_ids; mem.R = rows_per_id; mem.ttl = ttl < 0 ? -1 : ttl;
        clear_memory();
    }

    // gid | n | head | last | live of every entry, from the device (a call between steps: nothing of the map is in flight)
    std::vector<int> fetch_entries() const {
        std::vector<int> h((size_t)mem.max_ids * 5);
        if (mem.max_ids) YDS_HIP(hipMemcpy(h.data(), mem_entries.p, h.size() * sizeof(int), hipMemcpyDeviceToHost));
        return h;
    }

    // the used entries, ascending by id
    std::vector<Entry> entries() const {
        const std::vector<int> h = fetch_entries();
        const int E = mem.max_ids;
        std::vector<Entry> out;
        for (int e = 0; e < E; ++e)
            if (h[e] > 0) out.push_back(Entry{h[e], h[E + e], h[3 * (size_t)E + e], e, h[2 * (size_t)E + e]});
        std::sort(out.begin(), out.end(), [](const Entry &a, const Entry &b) { return a.global_id < b.global_id; });
        return out;
    }

    // rows of one id, oldest first
    void memory_rows(int global_id, float *rows_out, int cap, int *n_rows) const {
        const char *who = "identity_get_memory_rows";
        if (!mem.max_ids) fail("%s: the map has no memory (yds_identity_set_memory)", who);
        if (!n_rows) fail("%s: n_rows is NULL", who);
        for (const Entry &e : entries()) {
            if (e.global_id != global_id) continue;
            *n_rows = e.n_rows;
            if (e.n_rows > cap) fail("%s: cap = %d too small for %d rows (the needed size is in *n_rows)", who, cap, e.n_rows);
            if (e.n_rows && !rows_out) fail("%s: rows_out is NULL", who);
            const int R = mem.R, first = e.n_rows < R ? 0 : e.head;
            for (int k = 0; k < e.n_rows; ++k)
                YDS_HIP(hipMemcpy(rows_out + (size_t)k * EMB, bank.p + ((size_t)e.index * R + (first + k) % R) * EMB, EMB * sizeof(float), hipMemcpyDeviceToHost));
            return;
        }
        fail("%s: the memory holds no id %d", who, global_id);
    }

    // one departed entry per array under the next fresh ids; all or nothing
    void enrol(const float *rows_host, const int *n_rows, int n_arrays, int32_t *ids_out) {
        const char *who = "identity_enrol";
        if (!mem.max_ids) fail("%s: the map has no memory (yds_identity_set_memory)", who);
        if (n_arrays < 0 || (n_arrays && (!rows_host || !n_rows || !ids_out))) fail("%s: NULL argument", who);
        if (user && *user && user_busy && user_busy(*user)) fail("%s: the map's pipeline has a look-ahead pass in flight (consume it with a step first)", who);
        size_t total = 0;
        for (int a = 0; a < n_arrays; ++a) {
            if (n_rows[a] < 1) fail("%s: array %d has %d rows, at least one is needed", who, a, n_rows[a]);
            total += (size_t)n_rows[a];
        }
        for (size_t r = 0; r < total; ++r) {
            double ss = 0.0;
            for (int k = 0; k < EMB; ++k) ss += (double)rows_host[r * EMB + k] * rows_host[r * EMB + k];
            if (!(ss > 0.0) || !std::isfinite(ss) || !std::isfinite((float)std::sqrt(ss)))
                fail("%s: row %zu has a zero or non-finite norm", who, r);
        }
        if (!n_arrays) return;
        // ---- entries: the free ones in index order, then the departed ones by (last_held, id) - the update's own eviction rule
        std::vector<int> h = fetch_entries();
        const int E = mem.max_ids, R = mem.R;
        std::vector<int> pool, departed;
        for (int e = 0; e < E; ++e) {
            if (h[e] == 0) pool.push_back(e);
            else if (!h[4 * (size_t)E + e]) departed.push_back(e);
        }
        std::sort(departed.begin(), departed.end(), [&](int a, int b) {
            const int la = h[3 * (size_t)E + a], lb = h[3 * (size_t)E + b];
            return la != lb ? la < lb : h[a] < h[b];
        });
        pool.insert(pool.end(), departed.begin(), departed.end());
        if ((int)pool.size() < n_arrays)
            fail("%s: %d identities do not fit: the memory of %d ids has %zu entries free or departed, every other one has a live holder", who, n_arrays, E,
                 pool.size());
        // ---- rows: normalised on the device by the tracker's own kernel, the last R of each array to ring positions 0 .. n - 1
        enrol_stage.ensure(total * EMB);
        enrol_n.ensure(total * EMB);
        YDS_HIP(hipMemcpyAsync(enrol_stage.p, rows_host, total * EMB * sizeof(float), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(normalize_rows_kernel, dim3(((int)total + 3) / 4), dim3(256), 0, stream, (const float *)enrol_stage.p, (const int *)nullptr, enrol_n.p,
                           (int)total, 1);
        YDS_HIP(hipGetLastError());
        int next = 0;
        YDS_HIP(hipMemcpyAsync(&next, next_id.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        YDS_HIP(hipStreamSynchronize(stream));
        size_t r0 = 0;
        for (int a = 0; a < n_arrays; ++a) {
            const int e = pool[a], n = std::min(n_rows[a], R);
            YDS_HIP(hipMemcpyAsync(bank.p + (size_t)e * R * EMB, enrol_n.p + (r0 + n_rows[a] - n) * EMB, (size_t)n * EMB * sizeof(float), hipMemcpyDeviceToDevice,
                                   stream));
            h[e] = next + a; h[E + e] = n; h[2 * (size_t)E + e] = n % R; h[3 * (size_t)E + e] = n_updates; h[4 * (size_t)E + e] = 0;
            ids_out[a] = next + a;
            r0 += (size_t)n_rows[a];
        }
        next += n_arrays;
        YDS_HIP(hipMemcpyAsync(mem_entries.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, stream));
        YDS_HIP(hipMemcpyAsync(next_id.p, &next, sizeof(int), hipMemcpyHostToDevice, stream));
        YDS_HIP(hipStreamSynchronize(stream));
    }

    // the bank kernel on its own: dist [Q][entries] over the used entries ascending by id
    void memory_distances(const float *queries, int on_device, int Q, float *dist_out, int32_t *gid_out, int cap, int *n_entries, int strip_len = 0,
                          int iters = 0, float *us_out = nullptr) {
        const char *who = "identity_memory_distances";
        if (!mem.max_ids) fail("%s: the map has no memory (yds_identity_set_memory)", who);
        if (Q < 1 || Q > 4096) fail("%s: Q = %d outside [1, 4096]", who, Q);
        if (!queries || !n_entries) fail("%s: NULL argument", who);
        const std::vector<Entry> used = entries();
        *n_entries = (int)used.size();
        if ((int)used.size() > cap) fail("%s: cap = %d too small for %zu entries (the needed size is in *n_entries)", who, cap, used.size());
        if (used.size() && (!dist_out || !gid_out)) fail("%s: an output array is NULL", who);
        const int E = mem.max_ids;
        qn.ensure((size_t)Q * EMB);
        dist.ensure((size_t)Q * E);
        const float *src = queries;
        if (!on_device) {
            enrol_stage.ensure((size_t)Q * EMB);
            YDS_HIP(hipMemcpyAsync(enrol_stage.p, queries, (size_t)Q * EMB * sizeof(float), hipMemcpyHostToDevice, stream));
            src = enrol_stage.p;
        }
        hipLaunchKernelGGL(normalize_rows_kernel, dim3((Q + 3) / 4), dim3(256), 0, stream, src, (const int *)nullptr, qn.p, Q, 1);
        const int sl = strip_len > 0 ? strip_len : strip;
        const dim3 grid = bank_grid(Q, sl);
        launch_bank_dist(mem.R, grid, stream, (const float *)mem.rows, (const int *)mem.n, E, sl, (const float *)qn.p, Q, dist.p, E);
        for (int i = 0; i < iters; ++i) {                                     // (measurement aid: the kernel alone, HIP events around each)
            YDS_HIP(hipEventRecord(ev0, stream));
            launch_bank_dist(mem.R, grid, stream, (const float *)mem.rows, (const int *)mem.n, E, sl, (const float *)qn.p, Q, dist.p, E);
            YDS_HIP(hipEventRecord(ev1, stream));
            YDS_HIP(hipStreamSynchronize(stream));
            float ms = 0.f;
            YDS_HIP(hipEventElapsedTime(&ms, ev0, ev1));
            us_out[i] = ms * 1e3f;
        }
        YDS_HIP(hipGetLastError());
        std::vector<float> host((size_t)Q * E);
        YDS_HIP(hipMemcpyAsync(host.data(), dist.p, host.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
        YDS_HIP(hipStreamSynchronize(stream));
        for (size_t k = 0; k < used.size(); ++k) {
            gid_out[k] = used[k].global_id;
            for (int q = 0; q < Q; ++q) dist_out[(size_t)q * used.size() + k] = host[(size_t)q * E + used[k].index];
        }
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
    // the memory (mem.max_ids = 0: none, and none of these is allocated)
    std::vector<DevBuf<int>> rem;                 // per stream [slots]: the holder's hits at its last remembered row
    DevBuf<float> bank, enrol_stage, enrol_n;
    DevBuf<int> mem_entries, mem_arrays;
    IdentMem mem{};
    int n_updates = 0, strip = kBankStrip;
    int mcounts[7] = {0, 0, 0, 0, 0, 0, 0};       // entries, departed, relinked, remembered rows, expired, evicted, unremembered
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
int yds_identity_set_memory(yds_ident *h, int max_ids, int rows_per_id, int ttl) {
    YDS_API_BEGIN
    impl(h)->set_memory(max_ids, rows_per_id, ttl);
    YDS_API_END
}
int yds_identity_enrol(yds_ident *h, const float *rows, const int32_t *n_rows, int n_arrays, int32_t *global_id_out) {
    YDS_API_BEGIN
    impl(h)->enrol(rows, n_rows, n_arrays, global_id_out);
    YDS_API_END
}
int yds_identity_get_memory(yds_ident *h, int32_t *global_id, int32_t *n_rows, int32_t *last_held, int cap, int *n) {
    YDS_API_BEGIN
    const yds::Identity *I = impl(h);
    if (!n) yds::fail("identity_get_memory: n is NULL");
    const std::vector<yds::Identity::Entry> used = I->entries();
    const int m = (int)used.size();
    *n = m;
    if (m > cap) yds::fail("identity_get_memory: cap = %d too small for %d entries (the needed size is in *n)", cap, m);
    if (m && (!global_id || !n_rows || !last_held)) yds::fail("identity_get_memory: an output array is NULL");
    for (int k = 0; k < m; ++k) { global_id[k] = used[k].global_id; n_rows[k] = used[k].n_rows; last_held[k] = used[k].last_held; }
    YDS_API_END
}
int yds_identity_get_memory_rows(yds_ident *h, int global_id, float *rows_out, int cap, int *n_rows) {
    YDS_API_BEGIN
    impl(h)->memory_rows(global_id, rows_out, cap, n_rows);
    YDS_API_END
}
int yds_identity_memory_distances(yds_ident *h, const float *queries, int queries_on_device, int Q, float *dist_out, int32_t *global_id_out, int cap,
                                  int *n_entries) {
    YDS_API_BEGIN
    impl(h)->memory_distances(queries, queries_on_device, Q, dist_out, global_id_out, cap, n_entries);
    YDS_API_END
}
int yds_identity_memory_bench(yds_ident *h, const float *queries_dev, int Q, int strip_len, int iters, float *us_out) {
    YDS_API_BEGIN
    yds::Identity *I = impl(h);
    if (iters < 1 || !us_out || strip_len < 0) yds::fail("identity_memory_bench: iters = %d, strip_len = %d", iters, strip_len);
    const size_t E = (size_t)I->mem.max_ids;
    std::vector<float> d((size_t)Q * std::max<size_t>(E, 1));
    std::vector<int32_t> g(std::max<size_t>(E, 1));
    int n = 0;
    I->memory_distances(queries_dev, 1, Q, d.data(), g.data(), (int)E, &n, strip_len, iters, us_out);
    YDS_API_END
}
int yds_identity_last_relinked(yds_ident *h, int32_t *stream, int32_t *track_id, int32_t *global_id, float *cost, int cap, int *n) {
    YDS_API_BEGIN
    const yds::Identity *I = impl(h);
    if (!n) yds::fail("identity_last_relinked: n is NULL");
    int m = 0;
    for (const auto &l : I->links) m += l.relinked ? 1 : 0;
    *n = m;
    if (m > cap) yds::fail("identity_last_relinked: cap = %d too small for %d links (the needed size is in *n)", cap, m);
    if (m && (!stream || !track_id || !global_id || !cost)) yds::fail("identity_last_relinked: an output array is NULL");
    int k = 0;
    for (const auto &l : I->links)
        if (l.relinked) { stream[k] = l.stream; track_id[k] = l.track_id; global_id[k] = l.global_id; cost[k] = l.cost; ++k; }
    YDS_API_END
}
int yds_identity_last_memory_counts(yds_ident *h, int32_t *counts7) {
    YDS_API_BEGIN
    const yds::Identity *I = impl(h);
    if (!counts7) yds::fail("identity_last_memory_counts: counts7 is NULL");
    for (int k = 0; k < 7; ++k) counts7[k] = I->mcounts[k];
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
