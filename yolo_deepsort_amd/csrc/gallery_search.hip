// Cross-camera search: queries against the appearance galleries of MANY trackers, where the galleries live (HBM).
//
// No reference counterpart as a call: the reference keeps one NearestNeighborDistanceMetric per tracker and only ever asks it for
// the cost of that tracker's own detections (deep_sort/sort/nn_matching.py:158-187).  The arithmetic is that of
// _nn_cosine_distance (:77-100): min over a track's stored rows of 1 - <row, query / |query|>, rows stored normalised.
//   gallery_min_dist_kernel   dist[q][g] for every live track g of every given tracker, g in (stream, track-list) order
//   gallery_meta_kernel       (stream, track id, state) of every g
//   gallery_link_kernel       link mode: min over the query rows (the rows of one track), own track and excluded stream masked
//   gallery_select_kernel     per query the top_k smallest distances that pass the threshold and the state mask
// A call reads tracker state and writes none of it.  It runs on a stream of its own, between steps: a tracker's step returns after
// its own synchronisation, so nothing that writes a gallery is in flight.  One host synchronisation, one device-to-host copy.
#include "gallery_dev.h"

#include <limits.h>

namespace yds {

// the tracker that holds track g (n_desc is small: one entry per tracker with tracks); -1 never happens for g < total
__device__ __forceinline__ int desc_of(const GalleryDesc *desc, int n_desc, int g) {
    int s = 0;
    while (s + 1 < n_desc && g >= desc[s + 1].g0) ++s;
    return s;
}

constexpr int SLAB = GALLERY_SLAB;                // queries per workgroup = one MFMA tile edge
constexpr int PF = 16;                            // float4 chunks of a gallery row per register batch (EMB / 8 = 64 chunks per lane)
constexpr int LDQ = EMB + 4;                      // LDS row stride of the query slab: float4 reads of 32 rows spread over all banks

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Workgroup (g, slab): track g against queries [slab * 32, slab * 32 + 32).  The normalised query slab sits in LDS once; wave w takes
// the track's row tiles w, w + 4, ... (32 rows each) straight from HBM, every row fetched once per slab.  A tile is one 32 x 32
// accumulator of v_mfma_f32_32x32x2_f32 (exact fp32: per element a 512-term fma chain) with A = gallery rows, B = queries: lane
// (i = l & 31, h = l >> 5) loads the float4 at k = 8c + 4h of row i of either operand, so instruction j of chunk c multiplies the
// k pair {8c + j, 8c + 4 + j} - a fixed permutation of k, the same for both operands.  The accumulator holds, per lane, 16 gallery
// rows of ONE query: the segmented minimum is 16 in-lane maxima of the dot product plus one exchange with lane l ^ 32.  Rows
// >= n_feat of the last tile are not loaded and their accumulator entries are skipped (a reused slot keeps a dead track's rows there).
__global__ __launch_bounds__(256) void gallery_min_dist_kernel(const GalleryDesc *desc, int n_desc, const float *qn, int Q, float *dist, int ld) {
    __shared__ float qs[SLAB][LDQ];
    __shared__ float s_best[4][SLAB];
    __shared__ int s_valid[SLAB];
    const int g = blockIdx.x, q0 = blockIdx.y * SLAB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const GalleryDesc &e = desc[desc_of(desc, n_desc, g)];
    const int t = g - e.g0;
    const int rows = min(max(e.n_feat[t], 0), e.budget);
    const float *G = e.gallery + (size_t)e.slot[t] * e.budget * EMB;
    // ---- query slab: wave w stages rows 8w .. 8w + 7, and checks each: a normalised row has a squared norm of 1; a query whose norm
    //      was 0 or not finite arrives as NaN or zeros (normalize_rows_kernel divides) and matches nothing
#pragma unroll
    for (int r = 0; r < SLAB / 4; ++r) {
        const int row = wave * (SLAB / 4) + r, q = q0 + row;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (q < Q) {
            const float4 *src = reinterpret_cast<const float4 *>(qn + (size_t)q * EMB);
            a = src[lane]; b = src[64 + lane];
        }
        float ss = a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w + b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
        *reinterpret_cast<float4 *>(&qs[row][lane * 4]) = a;
        *reinterpret_cast<float4 *>(&qs[row][256 + lane * 4]) = b;
        if (lane == 0) s_valid[row] = (ss > 0.5f && ss < 2.f) ? 1 : 0;       // (NaN fails both)
    }
    __syncthreads();
    const int i = lane & 31, h = lane >> 5;
    float best = -INFINITY;                                                   // largest dot product = smallest distance
    for (int tile = wave; tile * 32 < rows; tile += 4) {
        const int r = tile * 32 + i;
        const bool live = r < rows;
        const float4 *gp = reinterpret_cast<const float4 *>(G + (size_t)(live ? r : 0) * EMB) + h;
        f32x16 acc;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.f;
        // the row streams through two register batches of PF chunks: batch n + 1 is in flight while batch n feeds the matrix core
        // (a rolled loop: unrolled, the compiler hoists every load of the row and spills)
        float4 cur[PF], nxt[PF];
#pragma unroll
        for (int j = 0; j < PF; ++j) cur[j] = live ? gp[2 * j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
        for (int n = 0; n < EMB / 8 / PF; ++n) {
            if (n + 1 < EMB / 8 / PF) {
#pragma unroll
                for (int j = 0; j < PF; ++j) nxt[j] = live ? gp[2 * ((n + 1) * PF + j)] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < PF; ++j) {
                const float4 b = *reinterpret_cast<const float4 *>(&qs[i][8 * (n * PF + j) + 4 * h]);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j].x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j].y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j].z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j].w, b.w, acc, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < PF; ++j) cur[j] = nxt[j];
        }
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int row = tile * 32 + (k & 3) + 8 * (k >> 2) + 4 * h;       // C/D map: lane holds column l & 31, these 16 rows
            if (row < rows) m = fmaxf(m, acc[k]);
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        best = fmaxf(best, m);
    }
    if (lane < SLAB) s_best[wave][lane] = best;
    __syncthreads();
    if (threadIdx.x < SLAB && q0 + (int)threadIdx.x < Q) {
        const int j = threadIdx.x;
        const float m = fmaxf(fmaxf(s_best[0][j], s_best[1][j]), fmaxf(s_best[2][j], s_best[3][j]));
        dist[(size_t)(q0 + j) * ld + g] = s_valid[j] ? 1.f - m : INFINITY;    // (a track without rows: 1 - (-inf) = +inf)
    }
}

// meta [3][T]: stream, track id, state of every track of the call
__global__ void gallery_meta_kernel(const GalleryDesc *desc, int n_desc, int T, int *meta) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= T) return;
    const GalleryDesc &e = desc[desc_of(desc, n_desc, g)];
    const int t = g - e.g0;
    meta[g] = e.stream; meta[T + g] = e.id[t]; meta[2 * T + g] = e.state[t];
}

// link mode: the queries were the rows of one track; link[g] = min over them, +inf for that track itself and for an excluded stream
__global__ void gallery_link_kernel(const float *dist, int n_q, int T, const int *meta, int self_g, int exclude_stream, float *link) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= T) return;
    float m = INFINITY;
    for (int q = 0; q < n_q; ++q) m = fminf(m, dist[(size_t)q * T + g]);
    link[g] = (g == self_g || meta[g] == exclude_stream) ? INFINITY : m;
}

// Workgroup q: the candidates of query q - finite distance <= max_dist, state bit set in state_mask (bit 0 Tentative, bit 1
// Confirmed) - compacted in g order, then min(top_k, candidates) rounds that each take the smallest (distance, g) key above the
// previous one: ties fall in (stream, track-list) order because g does.  res: n_hits [Q] | stream [Q][k_ld] | id [Q][k_ld] | dist [Q][k_ld].
__global__ __launch_bounds__(256) void gallery_select_kernel(const float *dist, int ld, int T, const int *meta, int state_mask, float max_dist,
                                                            int top_k, int k_ld, int Q, int *cand, int *res) {
    __shared__ int s_cnt[4];
    __shared__ unsigned long long s_key[4];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *row = dist + (size_t)q * ld;
    int *c = cand + (size_t)q * T;
    const int *state = meta + 2 * T;
    const int n = compact_ordered(T, s_cnt, [&](int g) {
        const float d = row[g];
        const int st = state[g];
        return d <= max_dist && d < INFINITY && st >= TENTATIVE && st <= CONFIRMED && ((state_mask >> (st - 1)) & 1);
    }, [&](int g, int r) { c[r] = g; });
    __syncthreads();
    const int n_out = min(n, top_k);
    int *o_stream = res + Q + (size_t)q * k_ld, *o_id = res + Q + (size_t)Q * k_ld + (size_t)q * k_ld;
    float *o_dist = reinterpret_cast<float *>(res + Q + 2 * (size_t)Q * k_ld + (size_t)q * k_ld);
    unsigned long long prev = 0;
    for (int k = 0; k < n_out; ++k) {
        unsigned long long local = ULLONG_MAX;
        for (int idx = tid; idx < n; idx += 256) {
            const int g = c[idx];
            const unsigned long long key = ((unsigned long long)ordered_bits(row[g]) << 32) | (unsigned)g;
            if ((k == 0 || key > prev) && key < local) local = key;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(local, o, 64);
            local = other < local ? other : local;
        }
        if (lane == 0) s_key[wave] = local;
        __syncthreads();
        unsigned long long bestk = s_key[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) bestk = s_key[w] < bestk ? s_key[w] : bestk;
        __syncthreads();
        if (tid == 0) {
            const int g = (int)(bestk & 0xffffffffull);
            o_stream[k] = meta[g]; o_id[k] = meta[T + g]; o_dist[k] = row[g];
        }
        prev = bestk;
    }
    if (tid == 0) res[q] = n_out;
}

// ============================================================================================ host
namespace {

constexpr int kMaxQueries = 4096;

// The buffers and the stream of the search calls of this process (the calls are not thread safe, like a handle).
struct SearchCtx {
    hipStream_t stream = nullptr;
    DevBuf<GalleryDesc> desc_dev;
    DevBuf<float> q_stage, qn;
    DevBuf<int> blk, cand;                         // blk: meta [3T] | dist [Q][T] | link [T] | select results
    PinBuf<GalleryDesc> desc_host;
    PinBuf<int> out_host;
    ~SearchCtx() { if (stream) (void)hipStreamDestroy(stream); }
};
SearchCtx &ctx() {
    static SearchCtx c;
    if (!c.stream) c.stream = make_stream(true);
    return c;
}

struct Plan {
    std::vector<GalleryView> views;                // per stream
    std::vector<int> g0;                           // per stream: its first g
    int T = 0, n_desc = 0;
};

// Everything a call can refuse without touching the device, then the descriptor array (host side)
Plan plan_call(yds_trk *const *trks, int n_streams, const char *who) {
    if (!trks || n_streams < 1) fail("%s: no trackers given", who);
    Plan p;
    for (int a = 0; a < n_streams; ++a) {
        if (!trks[a] || !trks[a]->t) fail("%s: tracker %d is NULL", who, a);
        for (int b = 0; b < a; ++b)
            if (trks[a] == trks[b] || trks[a]->t == trks[b]->t) fail("%s: streams %d and %d share one tracker", who, b, a);
    }
    SearchCtx &c = ctx();
    c.desc_host.ensure((size_t)n_streams);
    for (int s = 0; s < n_streams; ++s) {
        const GalleryView v = trks[s]->t->gallery_view();
        if (v.metric != METRIC_COSINE)
            fail("%s: tracker %d uses the euclidean metric: its gallery rows are not normalised, a cosine search cannot read them", who, s);
        p.views.push_back(v);
        p.g0.push_back(p.T);
        if (v.n_tracks > 0) {                      // a tracker without tracks contributes nothing
            c.desc_host.p[p.n_desc++] = GalleryDesc{v.gallery, v.slot, v.id, v.state, v.n_feat, v.budget, p.T, v.n_tracks, s};
            p.T += v.n_tracks;
        }
    }
    return p;
}

void check_queries(const char *who, const float *queries, int Q) {
    if (Q < 1 || Q > kMaxQueries) fail("%s: Q = %d outside [1, %d]", who, Q, kMaxQueries);
    if (!queries) fail("%s: queries is NULL", who);
}

// word offsets inside blk
struct Layout { size_t meta, dist, link, res, total; int k_ld; };
Layout layout_of(int T, int n_q, int n_sel, int top_k) {
    Layout l;
    l.k_ld = std::max(1, std::min(top_k, std::max(T, 1)));
    l.meta = 0; l.dist = 3 * (size_t)T; l.link = l.dist + (size_t)n_q * T; l.res = l.link + (size_t)T;
    l.total = l.res + (size_t)n_sel * (1 + 3 * (size_t)l.k_ld);
    return l;
}

// descriptors + meta + the distance matrix of n_q query rows (qn: normalised, on the device)
void enqueue_dist(SearchCtx &c, const Plan &p, const Layout &l, const float *qn, int n_q) {
    c.desc_dev.ensure((size_t)p.n_desc);
    YDS_HIP(hipMemcpyAsync(c.desc_dev.p, c.desc_host.p, (size_t)p.n_desc * sizeof(GalleryDesc), hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(gallery_meta_kernel, dim3((p.T + 255) / 256), dim3(256), 0, c.stream, c.desc_dev.p, p.n_desc, p.T, c.blk.p + l.meta);
    hipLaunchKernelGGL(gallery_min_dist_kernel, dim3(p.T, (n_q + SLAB - 1) / SLAB), dim3(256), 0, c.stream, c.desc_dev.p, p.n_desc, qn, n_q,
                       reinterpret_cast<float *>(c.blk.p + l.dist), p.T);
}

// queries (host or device, raw) -> c.qn, normalised by the tracker's own kernel
const float *enqueue_normalise(SearchCtx &c, const float *queries, int on_device, int Q) {
    c.qn.ensure((size_t)Q * EMB);
    const float *src = queries;
    if (!on_device) {
        c.q_stage.ensure((size_t)Q * EMB);
        YDS_HIP(hipMemcpyAsync(c.q_stage.p, queries, (size_t)Q * EMB * 4, hipMemcpyHostToDevice, c.stream));
        src = c.q_stage.p;
    }
    hipLaunchKernelGGL(normalize_rows_kernel, dim3((Q + 3) / 4), dim3(256), 0, c.stream, src, (const int *)nullptr, c.qn.p, Q, 1);
    return c.qn.p;
}

void enqueue_select(SearchCtx &c, const Layout &l, const float *dist, int T, int n_sel, int state_mask, float max_dist, int top_k) {
    c.cand.ensure((size_t)n_sel * T);
    hipLaunchKernelGGL(gallery_select_kernel, dim3(n_sel), dim3(256), 0, c.stream, dist, T, T, c.blk.p + l.meta, state_mask, max_dist,
                       std::min(top_k, l.k_ld), l.k_ld, n_sel, c.cand.p, c.blk.p + l.res);
}

// the one copy and the one synchronisation of a call: words [first, first + count) of blk
const int *fetch(SearchCtx &c, size_t first, size_t count) {
    YDS_HIP(hipGetLastError());
    c.out_host.ensure(count);
    YDS_HIP(hipMemcpyAsync(c.out_host.p, c.blk.p + first, count * 4, hipMemcpyDeviceToHost, c.stream));
    YDS_HIP(hipStreamSynchronize(c.stream));
    return c.out_host.p;
}

void scatter_hits(const int *res, int n_sel, int k_ld, int top_k, int32_t *n_hits, int32_t *hit_stream, int32_t *hit_id, float *hit_dist) {
    const int *rs = res + n_sel, *ri = rs + (size_t)n_sel * k_ld;
    const float *rd = reinterpret_cast<const float *>(ri + (size_t)n_sel * k_ld);
    for (int q = 0; q < n_sel; ++q) {
        n_hits[q] = res[q];
        for (int k = 0; k < res[q]; ++k) {
            hit_stream[(size_t)q * top_k + k] = rs[(size_t)q * k_ld + k];
            hit_id[(size_t)q * top_k + k] = ri[(size_t)q * k_ld + k];
            hit_dist[(size_t)q * top_k + k] = rd[(size_t)q * k_ld + k];
        }
    }
}

void check_select_args(const char *who, int top_k, const int32_t *n_hits, const int32_t *hit_stream, const int32_t *hit_id, const float *hit_dist) {
    if (top_k < 1) fail("%s: top_k = %d, must be >= 1", who, top_k);
    if (!n_hits || !hit_stream || !hit_id || !hit_dist) fail("%s: an output array is NULL", who);
}

}  // namespace
}  // namespace yds

// ============================================================================================ C ABI
extern "C" {

int yds_gallery_search(yds_trk *const *trks, int n_streams, const float *queries, int queries_on_device, int Q, int state_mask, float max_dist,
                       int top_k, int32_t *n_hits, int32_t *hit_stream, int32_t *hit_id, float *hit_dist) {
    YDS_API_BEGIN
    using namespace yds;
    const char *who = "gallery_search";
    check_queries(who, queries, Q);
    check_select_args(who, top_k, n_hits, hit_stream, hit_id, hit_dist);
    const Plan p = plan_call(trks, n_streams, who);
    for (int q = 0; q < Q; ++q) n_hits[q] = 0;
    if (p.T == 0) return 0;
    SearchCtx &c = ctx();
    const Layout l = layout_of(p.T, Q, Q, top_k);
    c.blk.ensure(l.total);
    const float *qn = enqueue_normalise(c, queries, queries_on_device, Q);
    enqueue_dist(c, p, l, qn, Q);
    enqueue_select(c, l, reinterpret_cast<const float *>(c.blk.p + l.dist), p.T, Q, state_mask, max_dist, top_k);
    scatter_hits(fetch(c, l.res, l.total - l.res), Q, l.k_ld, top_k, n_hits, hit_stream, hit_id, hit_dist);
    YDS_API_END
}

int yds_gallery_search_dense(yds_trk *const *trks, int n_streams, const float *queries, int queries_on_device, int Q, float *dist_out,
                             int32_t *stream_of, int32_t *track_id, int32_t *state, int cap, int *n_tracks) {
    YDS_API_BEGIN
    using namespace yds;
    const char *who = "gallery_search_dense";
    check_queries(who, queries, Q);
    if (!n_tracks) fail("%s: n_tracks is NULL", who);
    const Plan p = plan_call(trks, n_streams, who);
    *n_tracks = p.T;
    if (p.T > cap) fail("%s: cap = %d too small for %d tracks (the needed size is in *n_tracks)", who, cap, p.T);
    if (p.T == 0) return 0;
    if (!dist_out || !stream_of || !track_id || !state) fail("%s: an output array is NULL", who);
    SearchCtx &c = ctx();
    const Layout l = layout_of(p.T, Q, 0, 1);
    c.blk.ensure(l.total);
    const float *qn = enqueue_normalise(c, queries, queries_on_device, Q);
    enqueue_dist(c, p, l, qn, Q);
    const int *r = fetch(c, 0, l.link);
    memcpy(stream_of, r, (size_t)p.T * 4);
    memcpy(track_id, r + p.T, (size_t)p.T * 4);
    memcpy(state, r + 2 * (size_t)p.T, (size_t)p.T * 4);
    memcpy(dist_out, r + l.dist, (size_t)Q * p.T * 4);
    YDS_API_END
}

int yds_gallery_link(yds_trk *const *trks, int n_streams, int stream, int track_id, int exclude_stream, int state_mask, float max_dist, int top_k,
                     int32_t *n_hits, int32_t *hit_stream, int32_t *hit_id, float *hit_dist) {
    YDS_API_BEGIN
    using namespace yds;
    const char *who = "gallery_link";
    check_select_args(who, top_k, n_hits, hit_stream, hit_id, hit_dist);
    const Plan p = plan_call(trks, n_streams, who);
    if (stream < 0 || stream >= n_streams) fail("%s: stream %d outside [0, %d)", who, stream, n_streams);
    if (exclude_stream < -1 || exclude_stream >= n_streams) fail("%s: exclude_stream %d outside [-1, %d)", who, exclude_stream, n_streams);
    // the caller's track: the one table read of a link call, of the caller's tracker alone (columns slot .. n_feat are one block)
    const GalleryView &v = p.views[stream];
    int idx = -1, slot = 0, rows = 0;
    if (v.n_tracks > 0) {
        std::vector<int> tab((size_t)(v.n_feat - v.slot) + v.n_tracks);
        YDS_HIP(hipMemcpy(tab.data(), v.slot, tab.size() * 4, hipMemcpyDeviceToHost));
        const int *ids = tab.data() + (v.id - v.slot), *nf = tab.data() + (v.n_feat - v.slot);
        for (int t = 0; t < v.n_tracks && idx < 0; ++t)
            if (ids[t] == track_id) { idx = t; slot = tab[t]; rows = std::min(nf[t], v.budget); }
    }
    if (idx < 0) fail("%s: stream %d has no live track with id %d", who, stream, track_id);
    n_hits[0] = 0;
    if (rows < 1) return 0;
    SearchCtx &c = ctx();
    const Layout l = layout_of(p.T, rows, 1, top_k);
    c.blk.ensure(l.total);
    // its rows are the queries, normalised when they were stored
    enqueue_dist(c, p, l, v.gallery + (size_t)slot * v.budget * EMB, rows);
    float *link = reinterpret_cast<float *>(c.blk.p + l.link);
    hipLaunchKernelGGL(gallery_link_kernel, dim3((p.T + 255) / 256), dim3(256), 0, c.stream, reinterpret_cast<const float *>(c.blk.p + l.dist), rows,
                       p.T, c.blk.p + l.meta, p.g0[stream] + idx, exclude_stream, link);
    enqueue_select(c, l, link, p.T, 1, state_mask, max_dist, top_k);
    scatter_hits(fetch(c, l.res, l.total - l.res), 1, l.k_ld, top_k, n_hits, hit_stream, hit_id, hit_dist);
    YDS_API_END
}

int yds_tracker_get_gallery(yds_trk *trk, int track_index, float *rows_out, int cap, int *n_rows) {
    YDS_API_BEGIN
    using namespace yds;
    if (!trk || !trk->t || !n_rows) fail("tracker_get_gallery: NULL argument");
    const GalleryView v = trk->t->gallery_view();
    if (track_index < 0 || track_index >= v.n_tracks) fail("tracker_get_gallery: track index %d outside [0, %d)", track_index, v.n_tracks);
    int slot = 0, rows = 0;
    YDS_HIP(hipMemcpy(&slot, v.slot + track_index, 4, hipMemcpyDeviceToHost));
    YDS_HIP(hipMemcpy(&rows, v.n_feat + track_index, 4, hipMemcpyDeviceToHost));
    rows = std::min(rows, v.budget);
    *n_rows = rows;
    if (rows > cap) fail("tracker_get_gallery: cap = %d too small for %d rows (the needed size is in *n_rows)", cap, rows);
    if (rows && !rows_out) fail("tracker_get_gallery: rows_out is NULL");
    if (rows) YDS_HIP(hipMemcpy(rows_out, v.gallery + (size_t)slot * v.budget * EMB, (size_t)rows * EMB * 4, hipMemcpyDeviceToHost));
    YDS_API_END
}

// measurement aid (tools/gallery_search_bench.py): the launch sequence of yds_gallery_search - normalise, meta, distances, select -
// `iters` times back to back on device-resident queries, a HIP event between every two; us_out[i] = device time of repetition i
int yds_gallery_search_bench(yds_trk *const *trks, int n_streams, const float *queries_dev, int Q, int state_mask, float max_dist, int top_k,
                             int iters, float *us_out) {
    YDS_API_BEGIN
    using namespace yds;
    const char *who = "gallery_search_bench";
    check_queries(who, queries_dev, Q);
    if (top_k < 1 || iters < 1 || !us_out) fail("%s: top_k = %d, iters = %d", who, top_k, iters);
    const Plan p = plan_call(trks, n_streams, who);
    if (p.T == 0) fail("%s: the trackers hold no tracks", who);
    SearchCtx &c = ctx();
    const Layout l = layout_of(p.T, Q, Q, top_k);
    c.blk.ensure(l.total);
    c.qn.ensure((size_t)Q * EMB);
    c.cand.ensure((size_t)Q * p.T);
    c.desc_dev.ensure((size_t)p.n_desc);
    std::vector<hipEvent_t> ev((size_t)iters + 1);
    for (auto &e : ev) YDS_HIP(hipEventCreate(&e));
    YDS_HIP(hipEventRecord(ev[0], c.stream));
    for (int i = 0; i < iters; ++i) {
        const float *qn = enqueue_normalise(c, queries_dev, 1, Q);
        enqueue_dist(c, p, l, qn, Q);
        enqueue_select(c, l, reinterpret_cast<const float *>(c.blk.p + l.dist), p.T, Q, state_mask, max_dist, top_k);
        YDS_HIP(hipEventRecord(ev[i + 1], c.stream));
    }
    YDS_HIP(hipGetLastError());
    YDS_HIP(hipStreamSynchronize(c.stream));
    for (int i = 0; i < iters; ++i) {
        float ms = 0.f;
        YDS_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        us_out[i] = ms * 1e3f;
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    YDS_API_END
}

// the storage slot of every live track, in track-list order (parity tests: a slot that changes hands keeps the old rows behind n_feat)
int yds_tracker_get_slots(yds_trk *trk, int32_t *slots, int cap) {
    YDS_API_BEGIN
    using namespace yds;
    if (!trk || !trk->t) fail("tracker_get_slots: NULL argument");
    const GalleryView v = trk->t->gallery_view();
    if (v.n_tracks > cap) fail("tracker: %d tracks exceed cap %d", v.n_tracks, cap);
    if (v.n_tracks) YDS_HIP(hipMemcpy(slots, v.slot, (size_t)v.n_tracks * 4, hipMemcpyDeviceToHost));
    YDS_API_END
}

}  // extern "C"
