// The identity map's memory (identity.hip): a bank of appearance rows per global id in HBM, so that a person who left every camera
// is recognised when they come back.  Semantics: include/ydsort.h (yds_identity_set_memory); tests/identity_memory_ref.py restates them.
//   bank rows  [max_ids][R][512] fp32, R = rows_per_id in {1, 2, 4, 8, 16, 32}: whole entries tile a 32-row MFMA tile; an entry is a
//              ring: rows [0, n) are valid, `head` is where the next row goes, rows are bit copies of tracker gallery rows
//   per entry  gid (0: free), n, head, last (the last update at which a live track held the id), live (holder alive, as of the last
//              update and of the resolve in progress), cnt (appenders of this update)
//   ident_book_kernel      one workgroup behind ident_collect_kernel: touch, expire, entry of every holder (the held ids sorted, every
//                          entry looks its id up by binary search), allocation (free entries, then the departed entry with the smallest
//                          (last, gid)), rank and ring position of every appender; counts to the pinned block
//   ident_remember_kernel  workgroup g: the newest gallery row of holder g to its ring position; exits early when g appends nothing
//   ident_bank_dist_kernel dist[q][e] = min over the valid rows of entry e of 1 - <row, query q>, +inf for a free entry: a 32-query
//                          slab sits in LDS once per workgroup, which walks a strip of 32-row bank tiles
#pragma once
#include "gallery_dev.h"

#include <limits.h>

namespace yds {

// One tracker as the collect, book and resolve kernels read it (pinned host memory, rewritten ahead of every collect: a step may move
// the tracker's buffers).  pair: [cap][2] ints of this map, indexed by the tracker's slot; rem: [cap] the holder's hits at its last
// remembered row (nullptr without a memory), void like the pair when the slot changes hands.
struct alignas(16) IdentSrc {
    const float *gallery;
    const int *slot, *id, *state, *n_feat, *n_tracks, *hits;
    int *pair, *rem;
    int budget, cap;
};
static_assert(sizeof(IdentSrc) % 16 == 0, "IdentSrc arrays are indexed at a stride of sizeof(IdentSrc)");

// counts of an update, in pinned host memory
enum IdentCount {
    IC_T = 0, IC_NCONF, IC_NNEW, IC_NADM, IC_Q, IC_NLINK, IC_NFRESH, IC_NEXT,
    IC_M_ENTRIES, IC_M_DEPARTED, IC_M_RELINKED, IC_M_ROWS, IC_M_EXPIRED, IC_M_EVICTED, IC_M_UNREM, IC_COUNT
};

// Device arrays of the map, sized by the sum of the trackers' slot counts (no step can leave more tracks).  g = index of a track in
// (stream, track-list) order over all trackers; n = index of a new track in the same order.
struct IdentDev {
    int *g_stream, *g_gid, *g_conf, *g_hpos, *g_uk;     // stream, held id (0: none), Confirmed, place in the host list, index into U
    int *new_g, *new_rows, *new_q0;                     // new track n: its g, gallery rows, first row of its queries
    int *U, *flag_s, *flag_o, *colk, *colof;            // U: held ids ascending; per id: held in / outside the stream; columns
    int *link_col, *fresh_rank, *rows, *cols, *misc;    // per new track of the stream; LSAP pairs; misc[0] = LSAP pair count
    int *next_id;                                       // the one counter of all streams (next id to hand out)
};

// The memory as the kernels see it; max_ids = 0: the map has none (every pointer is null and no kernel here is launched)
struct IdentMem {
    float *rows;
    int *gid, *n, *head, *last, *live, *cnt;            // per entry
    int *pool, *dcol;                                   // per entry: free entries in index order; the departed columns of a stream
    int *ent_of, *first_g;                              // per held id (index into U): its entry, the first holder that needs one
    int *g_ent, *g_rank, *g_pos;                        // per track g: entry, rank among the entry's appenders, destination row (-1: none)
    int *sortbuf;                                       // a power of two >= the slot count
    int max_ids, R, ttl, u;                             // ttl < 0: never expire; u: the number of this update
};

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

// index of the first element >= v of the ascending array a[0, n)
__device__ __forceinline__ int ident_lower_bound(const int *a, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

// Steps 2-4 of an update with a memory (touch, expire, remember) up to the copy of the rows.  One workgroup.
__global__ __launch_bounds__(256) void ident_book_kernel(const IdentSrc *src, const GalleryDesc *gdesc, int S, int cap_total, IdentDev d, IdentMem m,
                                                         int *counts) {
    __shared__ int s_cnt[4];
    __shared__ unsigned long long s_key[4];
    __shared__ int s_ent[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = min(max(counts[IC_T], 0), cap_total), E = m.max_ids, R = m.R, u = m.u;
    int P = 1;
    while (P < T) P <<= 1;
    // ---- the held ids, ascending and unique (d.U, d.g_uk: the resolve kernel builds its own afterwards)
    int *sb = m.sortbuf;
    for (int i = tid; i < P; i += 256) sb[i] = INT_MAX;
    for (int g = tid; g < cap_total; g += 256) { m.g_pos[g] = -1; m.g_ent[g] = -1; m.g_rank[g] = -1; }
    __syncthreads();
    const int h = compact_ordered(T, s_cnt, [&](int g) { return d.g_gid[g] > 0; }, [&](int g, int r) { sb[r] = d.g_gid[g]; });
    __syncthreads();
    ident_sort(sb, P);
    const int nU = compact_ordered(h, s_cnt, [&](int i) { return i == 0 || sb[i] != sb[i - 1]; }, [&](int i, int r) { d.U[r] = sb[i]; });
    __syncthreads();
    for (int g = tid; g < T; g += 256) d.g_uk[g] = d.g_gid[g] > 0 ? ident_lower_bound(d.U, nU, d.g_gid[g]) : -1;
    for (int k = tid; k < nU; k += 256) { m.ent_of[k] = -1; m.first_g[k] = INT_MAX; }
    __syncthreads();
    // ---- touch and expire: every entry looks its id up among the held ones
    int n_expired = 0;
    for (int base = 0; base < E; base += 256) {
        const int e = base + tid;
        bool expired = false;
        if (e < E) {
            const int gid = m.gid[e];
            int live = 0;
            if (gid > 0) {
                const int k = ident_lower_bound(d.U, nU, gid);
                if (k < nU && d.U[k] == gid) { m.ent_of[k] = e; m.last[e] = u; live = 1; }
                else if (m.ttl >= 0 && u - m.last[e] > m.ttl) { m.gid[e] = 0; m.n[e] = 0; m.head[e] = 0; expired = true; }
            }
            m.live[e] = live; m.cnt[e] = 0;
        }
        n_expired += __syncthreads_count(expired);
    }
    __syncthreads();
    // ---- appenders: holders whose hits moved since their last remembered row; the first one (in g order) of an id without an entry
    //      asks for one
    auto table = [&](int g, int &hits, int **rem) {
        const int s = d.g_stream[g];
        const IdentSrc &e = src[s];
        const int t = g - gdesc[s].g0, slot = e.slot[t];
        hits = e.hits[t];
        *rem = (slot >= 0 && slot < e.cap) ? e.rem + slot : nullptr;
    };
    for (int g = tid; g < T; g += 256) {
        if (d.g_gid[g] <= 0) continue;
        int hits, *rem;
        table(g, hits, &rem);
        if (!rem || *rem == hits) continue;
        m.g_rank[g] = 0;
        const int k = d.g_uk[g];
        if (m.ent_of[k] < 0) atomicMin(&m.first_g[k], g);
    }
    __syncthreads();
    const int n_free = compact_ordered(E, s_cnt, [&](int e) { return m.gid[e] == 0; }, [&](int e, int r) { m.pool[r] = e; });
    const int n_need = compact_ordered(T, s_cnt, [&](int g) { return m.g_rank[g] == 0 && m.first_g[d.g_uk[g]] == g; }, [&](int g, int r) { d.colk[r] = g; });
    __syncthreads();
    auto take = [&](int e, int g) {
        m.gid[e] = d.g_gid[g]; m.n[e] = 0; m.head[e] = 0; m.last[e] = u; m.live[e] = 1;
        m.ent_of[d.g_uk[g]] = e;
    };
    for (int r = tid; r < min(n_need, n_free); r += 256) take(m.pool[r], d.colk[r]);
    __syncthreads();
    // ---- no free entry left: one round per asker takes the departed entry with the smallest (last, gid) (ids are unique, so keys are)
    int n_evicted = 0;
    for (int r = n_free; r < n_need; ++r) {
        unsigned long long best = ULLONG_MAX;
        int best_e = -1;
        for (int e = tid; e < E; e += 256) {
            if (m.gid[e] > 0 && !m.live[e]) {
                const unsigned long long key = ((unsigned long long)(unsigned)m.last[e] << 32) | (unsigned)m.gid[e];
                if (key < best) { best = key; best_e = e; }
            }
        }
        unsigned long long wbest = best;
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long other = __shfl_xor(wbest, o, 64); wbest = other < wbest ? other : wbest; }
        if (lane == 0) { s_key[wave] = wbest; s_ent[wave] = -1; }
        __syncthreads();                                                      // (nobody writes s_ent before every lane 0 cleared it)
        if (best == wbest && best_e >= 0) s_ent[wave] = best_e;
        __syncthreads();
        int win = 0;
#pragma unroll
        for (int w = 1; w < 4; ++w) if (s_key[w] < s_key[win]) win = w;
        const bool none = s_key[win] == ULLONG_MAX;
        const int e = s_ent[win];
        __syncthreads();
        if (none) break;                                                      // (uniform) every entry has a live holder
        if (tid == 0) take(e, d.colk[r]);
        ++n_evicted;
        __syncthreads();
    }
    // ---- every holder's entry; rank among the appenders of its entry: a camera holds an id at most once, so inside one stream the
    //      appenders write different counters, and the streams go in turn
    int n_unrem = 0;
    for (int base = 0; base < T; base += 256) {
        const int g = base + tid;
        bool un = false;
        if (g < T && d.g_gid[g] > 0) {
            const int e = m.ent_of[d.g_uk[g]];
            m.g_ent[g] = e;
            un = e < 0 && m.g_rank[g] == 0;
        }
        n_unrem += __syncthreads_count(un);
    }
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        const int g0 = gdesc[s].g0, n = gdesc[s].n;
        for (int g = g0 + tid; g < g0 + n; g += 256) {
            const int e = m.g_ent[g];
            if (m.g_rank[g] == 0 && e >= 0) { const int c = m.cnt[e]; m.g_rank[g] = c; m.cnt[e] = c + 1; }
            else m.g_rank[g] = -1;
        }
        __syncthreads();
    }
    // ---- ring positions: appender r of c goes to (head + r) mod R; when c > R only the last R are written
    int n_rows = 0;
    for (int base = 0; base < T; base += 256) {
        const int g = base + tid;
        bool app = false;
        if (g < T && m.g_rank[g] >= 0) {
            const int e = m.g_ent[g], c = m.cnt[e], r = m.g_rank[g];
            if (c - r <= R) m.g_pos[g] = e * R + (m.head[e] + r) % R;
            int hits, *rem;
            table(g, hits, &rem);
            *rem = hits;
            app = true;
        }
        n_rows += __syncthreads_count(app);
    }
    __syncthreads();
    for (int g = tid; g < T; g += 256) {
        if (m.g_rank[g] < 0) continue;
        const int e = m.g_ent[g], c = m.cnt[e];
        if (m.g_rank[g] == c - 1) { m.head[e] = (m.head[e] + c) % R; m.n[e] = min(m.n[e] + c, R); }
    }
    int n_ent = 0, n_dep = 0;
    for (int base = 0; base < E; base += 256) {
        const int e = base + tid;
        const bool used = e < E && m.gid[e] > 0;
        n_ent += __syncthreads_count(used);
        n_dep += __syncthreads_count(used && !m.live[e]);
    }
    if (tid == 0) {
        counts[IC_M_ENTRIES] = n_ent; counts[IC_M_DEPARTED] = n_dep; counts[IC_M_RELINKED] = 0; counts[IC_M_ROWS] = n_rows;
        counts[IC_M_EXPIRED] = n_expired; counts[IC_M_EVICTED] = n_evicted; counts[IC_M_UNREM] = n_unrem;
    }
}

// workgroup g (128 threads, one float4 each): the newest gallery row of holder g - ring position (hits - 1) mod budget of its slot -
// to the bank row the book kernel chose.  The grid covers every slot: the track count is not known on the host at enqueue time.
__global__ __launch_bounds__(128) void ident_remember_kernel(const IdentSrc *src, const GalleryDesc *gdesc, IdentDev d, IdentMem m) {
    const int g = blockIdx.x, pos = m.g_pos[g];
    if (pos < 0) return;
    const int s = d.g_stream[g];
    const IdentSrc &e = src[s];
    const int t = g - gdesc[s].g0, slot = e.slot[t];
    const int newest = (max(e.hits[t], 1) - 1) % e.budget;
    const float4 *from = reinterpret_cast<const float4 *>(e.gallery + ((size_t)slot * e.budget + newest) * EMB);
    float4 *to = reinterpret_cast<float4 *>(m.rows + (size_t)pos * EMB);
    to[threadIdx.x] = from[threadIdx.x];
}

constexpr int BANK_PF = 16;                       // float4 chunks of a bank row per register batch, as gallery_min_dist_kernel
constexpr int BANK_LDQ = EMB + 4;                 // LDS row stride of the query slab

typedef float bank_f32x16 __attribute__((ext_vector_type(16)));

// Workgroup (strip, slab): queries [slab * 32, slab * 32 + 32) against bank tiles [strip * strip_len, (strip + 1) * strip_len), a tile
// = bank rows [32 * tile, 32 * tile + 32) = 32 / R whole entries.  The query slab is staged once; wave w takes the strip's tiles w,
// w + 4, ...  Operand layout, k permutation and C/D map are those of gallery_min_dist_kernel (gallery_search.hip): lane (i = l & 31,
// h = l >> 5) holds, of query i, the dot products with tile rows (k & 3) + 8 (k >> 2) + 4 h, k < 16.  An entry's R rows are therefore
// R consecutive k for R <= 4, and for R >= 8 they spread over this lane and lane l ^ 32: in-lane maxima, then one exchange.  Rows at or
// beyond an entry's row count are not loaded and are masked out of the maximum (a reused entry keeps old rows there); a tile without
// a valid row costs no load at all.
template <int R>
__global__ __launch_bounds__(256) void ident_bank_dist_kernel(const float *bank, const int *b_n, int max_ids, int strip_len, const float *qn, int Q,
                                                              float *dist, int ld) {
    __shared__ float qs[GALLERY_SLAB][BANK_LDQ];
    __shared__ int s_valid[GALLERY_SLAB];
    const int q0 = blockIdx.y * GALLERY_SLAB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- query slab, checked like gallery_min_dist_kernel's: a query whose norm was 0 or not finite matches nothing
#pragma unroll
    for (int r = 0; r < GALLERY_SLAB / 4; ++r) {
        const int row = wave * (GALLERY_SLAB / 4) + r, q = q0 + row;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (q < Q) {
            const float4 *src = reinterpret_cast<const float4 *>(qn + (size_t)q * EMB);
            a = src[lane]; b = src[64 + lane];
        }
        float ss = a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w + b.x * b.x + b.y * b.y + b.z * b.z + b.w * b.w;
        for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
        *reinterpret_cast<float4 *>(&qs[row][lane * 4]) = a;
        *reinterpret_cast<float4 *>(&qs[row][256 + lane * 4]) = b;
        if (lane == 0) s_valid[row] = (ss > 0.5f && ss < 2.f) ? 1 : 0;
    }
    __syncthreads();
    const int i = lane & 31, h = lane >> 5;
    const int q = q0 + i;
    const bool q_ok = q < Q, q_valid = s_valid[i] != 0;
    float *out = dist + (size_t)(q_ok ? q : 0) * ld;
    auto put = [&](int e, float best) {                                       // best: the largest dot product, -inf without a valid row
        if (q_ok && e < max_ids) out[e] = q_valid ? 1.f - best : INFINITY;
    };
    const int n_tiles = (max_ids * R + 31) / 32;
    const int tile_end = min((int)(blockIdx.x + 1) * strip_len, n_tiles);
    for (int tile = blockIdx.x * strip_len + wave; tile < tile_end; tile += 4) {
        const int r = tile * 32 + i, ent = r / R;
        const bool live = ent < max_ids && (r % R) < min(b_n[ent < max_ids ? ent : 0], R);
        const unsigned mask = (unsigned)__ballot(live);                       // bit j: tile row j is valid (lanes j and j + 32 agree)
        bank_f32x16 acc;
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] = 0.f;
        if (mask != 0u) {                                                     // (uniform over the wave)
            const float4 *gp = reinterpret_cast<const float4 *>(bank + (size_t)(live ? r : 0) * EMB) + h;
            float4 cur[BANK_PF], nxt[BANK_PF];
#pragma unroll
            for (int j = 0; j < BANK_PF; ++j) cur[j] = live ? gp[2 * j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 1
            for (int n = 0; n < EMB / 8 / BANK_PF; ++n) {
                if (n + 1 < EMB / 8 / BANK_PF) {
#pragma unroll
                    for (int j = 0; j < BANK_PF; ++j) nxt[j] = live ? gp[2 * ((n + 1) * BANK_PF + j)] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int j = 0; j < BANK_PF; ++j) {
                    const float4 b = *reinterpret_cast<const float4 *>(&qs[i][8 * (n * BANK_PF + j) + 4 * h]);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j].x, b.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j].y, b.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j].z, b.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[j].w, b.w, acc, 0, 0, 0);
                }
#pragma unroll
                for (int j = 0; j < BANK_PF; ++j) cur[j] = nxt[j];
            }
        }
        // ---- segmented maximum per entry, inside the accumulator
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int row = (k & 3) + 8 * (k >> 2) + 4 * h;
            v[k] = ((mask >> row) & 1u) ? acc[k] : -INFINITY;
        }
        if constexpr (R == 1) {
#pragma unroll
            for (int k = 0; k < 16; ++k) put(tile * 32 + (k & 3) + 8 * (k >> 2) + 4 * h, v[k]);
        } else if constexpr (R == 2) {
#pragma unroll
            for (int k = 0; k < 16; k += 2) put(tile * 16 + ((k & 3) + 8 * (k >> 2) + 4 * h) / 2, fmaxf(v[k], v[k + 1]));
        } else {
            float v4[4];                                                      // rows 8 j + 4 h .. + 3
#pragma unroll
            for (int j = 0; j < 4; ++j) v4[j] = fmaxf(fmaxf(v[4 * j], v[4 * j + 1]), fmaxf(v[4 * j + 2], v[4 * j + 3]));
            if constexpr (R == 4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) put(tile * 8 + 2 * j + h, v4[j]);
            } else if constexpr (R == 8) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float x = fmaxf(v4[j], __shfl_xor(v4[j], 32, 64));
                    if ((j & 1) == h) put(tile * 4 + j, x);
                }
            } else if constexpr (R == 16) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    float x = fmaxf(v4[2 * j], v4[2 * j + 1]);
                    x = fmaxf(x, __shfl_xor(x, 32, 64));
                    if (j == h) put(tile * 2 + j, x);
                }
            } else {
                float x = fmaxf(fmaxf(v4[0], v4[1]), fmaxf(v4[2], v4[3]));
                x = fmaxf(x, __shfl_xor(x, 32, 64));
                if (h == 0) put(tile, x);
            }
        }
    }
}

}  // namespace yds
