// Track snapshots on the device: per stream a table of tracks that keeps, per track, the best thumbnail seen so far (uint8 RGB,
// 128 x 64, the ReID crop size) with its score, box and time, and an archive ring of the snapshots of tracks that left.  The fifth
// table stage (track_stage.h) and the first that reads PIXELS as well as rows: the frames of the step are handed over before enqueue
// (SnapIface::set_pixels).
//
// There is no reference counterpart; the rules are written down in include/ydsort.h (the snapshot block) and restated in numpy and
// Python ints by yolo_deepsort_amd/snapshot.py (SnapshotBook), which every device test compares against with exact equality.  The
// resize is resize_dev.h's resize_px, the text the ReID front end uses; everything after it is integer arithmetic.
//
// Three launches per call:
//   score   one workgroup per (frame, row slot): the row's clipped region resampled pixel by pixel straight to luma in LDS (8 KiB -
//           the thumbnail itself never leaves the workgroup), the Laplacian sum, a workgroup reduction, ONE int per row: the score, or
//           -1 for a row that is no candidate.
//   decide  the table-stage workgroup per stream: walks the stream's frames in time order, applies the decision and closing rules and
//           writes the report into the pinned block.  It moves no pixels: an entry holds a SLOT of a per-stream pool of cap + archive
//           thumbnails, closing hands the slot to the archive ring, the slot that falls off the ring returns to a free list, and a
//           per-slot `pending` names the row of this call that has to be written into the slot (a later winner overwrites it, freeing
//           the slot clears it).  At the end the slots with a pending row are listed.
//   commit  one workgroup per listed slot: the row resampled again by the same device function - the same bytes - into LDS and stored
//           with 16-byte accesses.  Pictures that did not change cost nothing.
#include "resize_dev.h"
#include "track_stage.h"
#include "ydsort.h"

#include <algorithm>

namespace yds {

constexpr int SNAP_H = YDS_SNAP_H, SNAP_W = YDS_SNAP_W, SNAP_PX = SNAP_H * SNAP_W, SNAP_BYTES = SNAP_PX * 3;
constexpr int SNAP_ICOLS = 11, SNAP_DCOLS = 3;    // table columns: id, age, slot, score, n_seen, tag_best, class, box[4]; t_first, t_best, t_last
constexpr int SNAP_AICOLS = 10, SNAP_ADCOLS = 4;  // ring columns:  id, class, score, n_seen, tag_best, box[4], slot; t_first, t_best, t_last, t_closed
enum { SC_ID, SC_AGE, SC_SLOT, SC_SCORE, SC_SEEN, SC_TAG, SC_CLS, SC_X1, SC_Y1, SC_X2, SC_Y2 };
enum { SA_ID, SA_CLS, SA_SCORE, SA_SEEN, SA_TAG, SA_X1, SA_Y1, SA_X2, SA_Y2, SA_SLOT };

// table of one stream: `cap` entries, every column twice (the second copy takes the survivors of a removal)
struct SnapTab {
    int *ic;                                      // [11][2][cap]
    double *dc;                                   // [3][2][cap]
    int *count;                                   // live entries (device)
    int cap;
    __device__ __forceinline__ int &i(int col, int e) const { return ic[(size_t)col * 2 * cap + e]; }
    __device__ __forceinline__ double &d(int col, int e) const { return dc[(size_t)col * 2 * cap + e]; }
};
// the pictures of one stream
struct SnapPool {
    uint8_t *thumbs;                              // [pool_cap][128][64][3]
    int *freelist, *n_free;                       // a stack of free slots
    int2 *pending;                                // per slot: (frame of the call's sorted list, row of that frame) to be written, x < 0: none
    int *commit_slot;                             // the slots listed for the commit launch, and what each takes
    int2 *commit_src;
    int *n_commit;
    int pool_cap;
};
struct SnapRing {
    int *ic;                                      // [10][A]
    double *dc;                                   // [4][A]
    long long *closed;                            // snapshots archived so far
};
struct SnapWork {
    SnapTab tab;
    SnapPool pool;
    SnapRing ring;
    int cls, skip;                                // skip: the stream has no spec - its frames report nothing and touch nothing
    int f0, f1;                                   // frames [f0, f1) of the call's frame list (sorted by stream, order kept)
    int *srows;                                   // staging [max rows of a frame][6]
    int *sx;                                      // ... [max rows of a frame][3]: the row's index in the frame, its score, n_seen if it won
    int res_count, res_free;                      // int indices in the result block of this stream's entry count and free slot count
};
struct SnapFrameDev {
    const int *rows;
    const int *n_p;
    double t;
    uint64_t off;                                 // the frame's pixels: h x w x 3 bytes at frames + off
    int h, w;
    int n, tag;
    int cls, min_w, min_h, skip;                  // of the frame's stream
    int res_n, res_ev, ev_cap;                    // int indices in the result block of the frame's item count and of its items [.][6]
};

// Rule 2: the clipped box of a row in a frame of H x W; false = no candidate.
struct SnapRegion { int xa, ya, vw, vh; unsigned long long vis, full; };
__device__ __forceinline__ bool snap_region(const int *r, int H, int W, int min_w, int min_h, SnapRegion &g) {
    const long long x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
    const long long xa = max(x1, 0ll), ya = max(y1, 0ll), xb = min(x2, (long long)W), yb = min(y2, (long long)H);
    const long long vw = xb - xa, vh = yb - ya;
    if (vw < min_w || vh < min_h || x2 <= x1 || y2 <= y1) return false;          // (min_w, min_h >= 1: both extents are positive, so full > 0)
    g.xa = (int)xa; g.ya = (int)ya; g.vw = (int)vw; g.vh = (int)vh;
    g.vis = (unsigned long long)vw * (unsigned long long)vh;
    g.full = (unsigned long long)(x2 - x1) * (unsigned long long)(y2 - y1);       // < 2^64 for any int32 corners
    return true;
}
// Rule 3: one pixel of the thumbnail, channels as R, G, B.
__device__ __forceinline__ void snap_px(const uint8_t *src, size_t row_bytes, const SnapRegion &g, int p, int bgr, int &R, int &G, int &B) {
    float o[3];
    resize_px(src, row_bytes, g.vh, g.vw, SNAP_H, SNAP_W, p / SNAP_W, p % SNAP_W, o);
    R = (int)o[bgr ? 2 : 0]; G = (int)o[1]; B = (int)o[bgr ? 0 : 2];
}

__global__ __launch_bounds__(256) void snap_score_kernel(const SnapFrameDev *frames, const uint8_t *base, int bgr, int max_rows, int *scores) {
    __shared__ uint8_t s_y[SNAP_PX];
    __shared__ int s_red[4];
    const SnapFrameDev &F = frames[blockIdx.y];
    const int j = blockIdx.x, tid = threadIdx.x;
    if (F.skip) return;
    const int R = F.n_p ? min(max(*F.n_p, 0), F.n) : F.n;
    if (j >= R) return;
    const int *r = F.rows + (size_t)j * 6;
    int *out = scores + (size_t)blockIdx.y * max_rows + j;
    SnapRegion g;
    if ((F.cls != -1 && r[5] != F.cls) || !snap_region(r, F.h, F.w, F.min_w, F.min_h, g)) {
        if (tid == 0) *out = -1;
        return;
    }
    const size_t row_bytes = (size_t)F.w * 3;
    const uint8_t *src = base + F.off + (size_t)g.ya * row_bytes + (size_t)g.xa * 3;
    for (int p = tid; p < SNAP_PX; p += 256) {
        int cr, cg, cb;
        snap_px(src, row_bytes, g, p, bgr, cr, cg, cb);
        s_y[p] = (uint8_t)((77 * cr + 150 * cg + 29 * cb + 128) >> 8);
    }
    __syncthreads();
    int sum = 0;
    for (int p = tid; p < SNAP_PX; p += 256) {
        const int y = p / SNAP_W, x = p % SNAP_W;
        if (y < 1 || y > SNAP_H - 2 || x < 1 || x > SNAP_W - 2) continue;
        sum += abs(4 * (int)s_y[p] - (int)s_y[p - SNAP_W] - (int)s_y[p + SNAP_W] - (int)s_y[p - 1] - (int)s_y[p + 1]);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if ((tid & 63) == 0) s_red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long sharp = (unsigned long long)(s_red[0] + s_red[1] + s_red[2] + s_red[3]);
        *out = (int)(sharp * g.vis / g.full);                                     // vis <= full: the result is at most sharp
    }
}

__global__ __launch_bounds__(256) void snap_decide_kernel(const SnapWork *works, const SnapFrameDev *frames, const int *scores, int max_rows,
                                                          int max_age, int A, int *res) {
    __shared__ int s_cnt[4];
    const SnapWork &Wg = works[blockIdx.x];
    const SnapTab T = Wg.tab;
    const SnapPool P = Wg.pool;
    const SnapRing Rg = Wg.ring;
    const int tid = threadIdx.x, cap = T.cap, cls = Wg.cls;
    int *const srows = Wg.srows, *const sx = Wg.sx;
    if (Wg.skip) {
        if (tid == 0) {
            for (int f = Wg.f0; f < Wg.f1; ++f) res[frames[f].res_n] = 0;
            res[Wg.res_count] = 0;
            res[Wg.res_free] = 0;
            *P.n_commit = 0;
        }
        return;
    }
    int n = *T.count, n_free = *P.n_free, broken = 0;                             // broken: the pool's invariant does not hold (the host refuses)
    long long closed = *Rg.closed;
    __syncthreads();
    for (int f = Wg.f0; f < Wg.f1; ++f) {
        const SnapFrameDev F = frames[f];
        int R = stage_frame_rows(F.rows, F.n_p, F.n, srows);
        for (int k = tid; k < R; k += 256) { sx[3 * k] = k; sx[3 * k + 1] = scores[(size_t)f * max_rows + k]; sx[3 * k + 2] = 0; }
        __syncthreads();
        // ---- rows of another class are ignored entirely: the others move up, order kept
        if (cls != -1) {
            int r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, x0 = 0, x1 = 0;
            R = compact_ordered(R, s_cnt, [&](int j) {
                const int *r = srows + j * 6;
                r0 = r[0]; r1 = r[1]; r2 = r[2]; r3 = r[3]; r4 = r[4]; r5 = r[5]; x0 = sx[3 * j]; x1 = sx[3 * j + 1];
                return r5 == cls;
            }, [&](int, int k) {
                int *d = srows + k * 6;
                d[0] = r0; d[1] = r1; d[2] = r2; d[3] = r3; d[4] = r4; d[5] = r5; sx[3 * k] = x0; sx[3 * k + 1] = x1;
            });
            __syncthreads();
        }
        // ---- unknown ids are registered at the end of the table in row order: no picture, score -1
        const int n_all = register_unknown(R, n, cap, s_cnt, &T.i(SC_ID, 0), srows, [&](int e, const int *r) {
            T.i(SC_ID, e) = r[4]; T.i(SC_AGE, e) = 0; T.i(SC_SLOT, e) = -1; T.i(SC_SCORE, e) = -1; T.i(SC_SEEN, e) = 0; T.i(SC_TAG, e) = -1;
            T.i(SC_CLS, e) = r[5]; T.i(SC_X1, e) = 0; T.i(SC_Y1, e) = 0; T.i(SC_X2, e) = 0; T.i(SC_Y2, e) = 0;
            T.d(0, e) = F.t; T.d(1, e) = 0.0; T.d(2, e) = F.t;
        });
        __syncthreads();
        // ---- entries in table order, a thread each: a sighting, perhaps a better picture; else the entry ages
        int dead = 0;
        for (int base = 0; base < n_all; base += 256) {
            const int e = base + tid;
            int j = R;
            bool win = false, need = false;
            if (e < n_all) {
                j = find_row(srows, R, T.i(SC_ID, e));
                if (j < R) {
                    win = sx[3 * j + 1] > T.i(SC_SCORE, e);                       // strictly greater: on a tie the earlier sighting stays
                    need = win && T.i(SC_SLOT, e) < 0;
                }
            }
            int taken = 0;
            const int rank = block_prefix(need ? 1 : 0, s_cnt, taken);
            bool gone = false;
            if (e < n_all) {
                if (j == R) {
                    const int a = T.i(SC_AGE, e) + 1;
                    T.i(SC_AGE, e) = a;
                    gone = a > max_age;
                } else {
                    const int *r = srows + j * 6;
                    const int seen = T.i(SC_SEEN, e) + 1;
                    T.i(SC_AGE, e) = 0; T.i(SC_SEEN, e) = seen; T.i(SC_CLS, e) = r[5]; T.d(2, e) = F.t;
                    if (win && need && n_free - 1 - rank < 0) win = false;        // keeps the read below in bounds; `broken` reports the damage
                    if (win) {
                        const int slot = need ? P.freelist[n_free - 1 - rank] : T.i(SC_SLOT, e);
                        T.i(SC_SLOT, e) = slot; T.i(SC_SCORE, e) = sx[3 * j + 1]; T.i(SC_TAG, e) = F.tag; T.d(1, e) = F.t;
                        T.i(SC_X1, e) = r[0]; T.i(SC_Y1, e) = r[1]; T.i(SC_X2, e) = r[2]; T.i(SC_Y2, e) = r[3];
                        P.pending[slot] = make_int2(f, sx[3 * j]);
                        sx[3 * j + 2] = seen;
                    }
                }
            }
            if (taken > n_free) broken = 1;
            n_free = max(n_free - taken, 0);
            dead += __syncthreads_count(gone);
        }
        // ---- BEST items in row order
        int *const ev = res + F.res_ev;
        const int nb = compact_ordered(R, s_cnt, [&](int j) { return sx[3 * j + 2] > 0; }, [&](int j, int k) {
            if (k >= F.ev_cap) return;
            int *o = ev + (size_t)k * 6;
            o[0] = F.tag; o[1] = srows[j * 6 + 4]; o[2] = srows[j * 6 + 5]; o[3] = YDS_SNAP_BEST; o[4] = sx[3 * j + 1]; o[5] = sx[3 * j + 2];
        });
        // ---- entries older than max_age close in entry order: a picture goes to ring position closed % A, the rest vanish
        int n_live = n_all, n_gone = 0;
        if (dead) {
            int Kc = 0;                                                           // closers with a picture in this frame
            if (A > 0)
                for (int base = 0; base < n_all; base += 256) {
                    const int e = base + tid;
                    Kc += __syncthreads_count(e < n_all && T.i(SC_AGE, e) > max_age && T.i(SC_SLOT, e) >= 0);
                }
            // every ring position this frame's closers reach gives up the occupant it had before the frame, once - whether the first
            // closer that reaches it stays there or a later one of the same frame does
            const int n_hit = min(Kc, A);
            for (int base = 0; base < n_hit; base += 256) {
                const int r = base + tid;
                const bool out = r < n_hit && closed + r >= A;
                int tot_o = 0;
                const int rank_o = block_prefix(out ? 1 : 0, s_cnt, tot_o);
                if (out && n_free + rank_o < P.pool_cap) {
                    const int old = Rg.ic[(size_t)SA_SLOT * A + (int)((closed + r) % A)];
                    P.freelist[n_free + rank_o] = old;
                    P.pending[old] = make_int2(-1, -1);
                }
                if (n_free + tot_o > P.pool_cap) broken = 1;
                n_free = min(n_free + tot_o, P.pool_cap);
            }
            __syncthreads();
            int pb = 0;
            for (int base = 0; base < n_all; base += 256) {
                const int e = base + tid;
                const bool gone = e < n_all && T.i(SC_AGE, e) > max_age;
                const bool pic = gone && A > 0 && T.i(SC_SLOT, e) >= 0;
                int tot_g = 0, tot_p = 0, tot_f = 0;
                const int rank_g = block_prefix(gone ? 1 : 0, s_cnt, tot_g);
                const int rank_p = block_prefix(pic ? 1 : 0, s_cnt, tot_p);
                int freed = -1, aux = -1;
                if (gone) {
                    const int slot = T.i(SC_SLOT, e);
                    if (pic) {
                        const int r = pb + rank_p;
                        const long long g = closed + r;
                        const int pos = (int)(g % A);
                        aux = pos;
                        if (r >= Kc - A) {                                        // the last closer of this frame at pos: it stays
                            int *ai = Rg.ic + pos;
                            ai[(size_t)SA_ID * A] = T.i(SC_ID, e); ai[(size_t)SA_CLS * A] = T.i(SC_CLS, e); ai[(size_t)SA_SCORE * A] = T.i(SC_SCORE, e);
                            ai[(size_t)SA_SEEN * A] = T.i(SC_SEEN, e); ai[(size_t)SA_TAG * A] = T.i(SC_TAG, e);
                            ai[(size_t)SA_X1 * A] = T.i(SC_X1, e); ai[(size_t)SA_Y1 * A] = T.i(SC_Y1, e);
                            ai[(size_t)SA_X2 * A] = T.i(SC_X2, e); ai[(size_t)SA_Y2 * A] = T.i(SC_Y2, e); ai[(size_t)SA_SLOT * A] = slot;
                            double *ad = Rg.dc + pos;
                            ad[0] = T.d(0, e); ad[A] = T.d(1, e); ad[2 * (size_t)A] = T.d(2, e); ad[3 * (size_t)A] = F.t;
                        } else {
                            freed = slot;                                         // overwritten within the frame
                        }
                    } else if (slot >= 0) {
                        freed = slot;                                             // no archive: dropped
                    }
                    const int k = nb + n_gone + rank_g;
                    if (k < F.ev_cap) {
                        int *o = ev + (size_t)k * 6;
                        o[0] = F.tag; o[1] = T.i(SC_ID, e); o[2] = T.i(SC_CLS, e); o[3] = YDS_SNAP_CLOSED; o[4] = T.i(SC_SCORE, e); o[5] = aux;
                    }
                }
                const int rank_f = block_prefix(freed >= 0 ? 1 : 0, s_cnt, tot_f);
                if (freed >= 0 && n_free + rank_f < P.pool_cap) {
                    P.freelist[n_free + rank_f] = freed;
                    P.pending[freed] = make_int2(-1, -1);
                }
                if (n_free + tot_f > P.pool_cap) broken = 1;
                n_free = min(n_free + tot_f, P.pool_cap);
                pb += tot_p;
                n_gone += tot_g;
            }
            closed += Kc;
            __syncthreads();
            auto move = [&](int d, int e) {
#pragma unroll
                for (int c = 0; c < SNAP_ICOLS; ++c) T.i(c, d) = T.i(c, e);
#pragma unroll
                for (int c = 0; c < SNAP_DCOLS; ++c) T.d(c, d) = T.d(c, e);
            };
            n_live = retire(n_all, cap, s_cnt, [&](int e) { return T.i(SC_AGE, e) <= max_age; }, move, move);
        }
        if (tid == 0) res[F.res_n] = min(nb + n_gone, F.ev_cap);
        n = n_live;
        __syncthreads();
    }
    // ---- the slots that take a row of this call, listed for the commit launch
    const int nc = compact_ordered(P.pool_cap, s_cnt, [&](int s) { return P.pending[s].x >= 0; }, [&](int s, int k) {
        P.commit_slot[k] = s;
        P.commit_src[k] = P.pending[s];
        P.pending[s] = make_int2(-1, -1);
    });
    if (tid == 0) {
        *T.count = n; *P.n_free = n_free; *Rg.closed = closed; *P.n_commit = nc;
        res[Wg.res_count] = n;
        res[Wg.res_free] = broken ? -1 : n_free;
    }
}

__global__ __launch_bounds__(256) void snap_commit_kernel(const SnapWork *works, const SnapFrameDev *frames, const uint8_t *base, int bgr) {
    __shared__ uint4 s_t4[SNAP_BYTES / 16];
    const SnapWork &Wg = works[blockIdx.y];
    const SnapPool P = Wg.pool;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (Wg.skip || k >= *P.n_commit) return;
    const int slot = P.commit_slot[k];
    const int2 from = P.commit_src[k];
    const SnapFrameDev &F = frames[from.x];
    SnapRegion g;
    if (slot < 0 || slot >= P.pool_cap || !snap_region(F.rows + (size_t)from.y * 6, F.h, F.w, F.min_w, F.min_h, g)) return;
    const size_t row_bytes = (size_t)F.w * 3;
    const uint8_t *src = base + F.off + (size_t)g.ya * row_bytes + (size_t)g.xa * 3;
    uint8_t *s_t = reinterpret_cast<uint8_t *>(s_t4);
    for (int p = tid; p < SNAP_PX; p += 256) {
        int cr, cg, cb;
        snap_px(src, row_bytes, g, p, bgr, cr, cg, cb);
        s_t[p * 3] = (uint8_t)cr; s_t[p * 3 + 1] = (uint8_t)cg; s_t[p * 3 + 2] = (uint8_t)cb;
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(P.thumbs + (size_t)slot * SNAP_BYTES);
    for (int q = tid; q < SNAP_BYTES / 16; q += 256) dst[q] = s_t4[q];
}

class Snap : public TrackStage<SnapIface> {
public:
    Snap(int S, int max_age, int archive) : TrackStage("snapshots", S), max_age(max_age), A(archive), tabs(S), specs(S), free_host(S, 0) {
        if (max_age < 1) fail("snapshots: max_age %d < 1", max_age);
        if (archive < 0 || archive > YDS_SNAP_MAX_ARCHIVE) fail("snapshots: archive %d outside [0,%d]", archive, YDS_SNAP_MAX_ARCHIVE);
        ring_i.alloc((size_t)S * SNAP_AICOLS * std::max(A, 1));
        ring_d.alloc((size_t)S * SNAP_ADCOLS * std::max(A, 1));
        closed.alloc(S);
        n_free.alloc(S);
        n_commit.alloc(S);
        YDS_HIP(hipMemset(closed.p, 0, S * sizeof(long long)));
        YDS_HIP(hipMemset(n_free.p, 0, S * sizeof(int)));
        YDS_HIP(hipMemset(n_commit.p, 0, S * sizeof(int)));
    }

    struct Tab {
        DevBuf<int> ints, freelist, commit_slot;
        DevBuf<double> dbl;
        DevBuf<uint8_t> thumbs;
        DevBuf<int2> pending, commit_src;
        int cap = 0;
        int pool_cap() const { return cap ? cap + archive : 0; }
        int archive = 0;
    };
    struct Spec { int cls = -1, min_w = 8, min_h = 16; bool set = false; };

    SnapTab dev_tab(int s) { return SnapTab{tabs[s].ints.p, tabs[s].dbl.p, counts.p + s, tabs[s].cap}; }
    SnapPool dev_pool(int s) {
        Tab &t = tabs[s];
        return SnapPool{t.thumbs.p, t.freelist.p, n_free.p + s, t.pending.p, t.commit_slot.p, t.commit_src.p, n_commit.p + s, t.pool_cap()};
    }
    SnapRing dev_ring(int s) {
        const size_t a = std::max(A, 1);
        return SnapRing{ring_i.p + (size_t)s * SNAP_AICOLS * a, ring_d.p + (size_t)s * SNAP_ADCOLS * a, closed.p + s};
    }
    // every slot of [first, pool_cap) onto the free stack behind its `have` entries; no pending rows there
    void push_free(Tab &t, int s, int have, int first) {
        std::vector<int> fl;
        for (int k = t.pool_cap() - 1; k >= first; --k) fl.push_back(k);
        if (!fl.empty()) YDS_HIP(hipMemcpy(t.freelist.p + have, fl.data(), fl.size() * sizeof(int), hipMemcpyHostToDevice));
        if (t.pool_cap() > first) YDS_HIP(hipMemset(t.pending.p + first, 0xff, (size_t)(t.pool_cap() - first) * sizeof(int2)));
        free_host[s] = have + (int)fl.size();
        YDS_HIP(hipMemcpy(n_free.p + s, &free_host[s], sizeof(int), hipMemcpyHostToDevice));
    }
    void grow(int s, int need) {
        if (!specs[s].set) return;
        const size_t n = count_host[s];
        const bool keep = n > 0 || free_host[s] < tabs[s].pool_cap();          // (archived pictures outlive an empty table)
        const int old_pool = tabs[s].pool_cap(), old_free = free_host[s];
        if (need <= tabs[s].cap) return;
        Tab nt;
        nt.archive = A;
        nt.cap = std::max(tabs[s].cap, 64);
        while (nt.cap < need) nt.cap *= 2;
        nt.ints.alloc((size_t)SNAP_ICOLS * 2 * nt.cap);
        nt.dbl.alloc((size_t)SNAP_DCOLS * 2 * nt.cap);
        nt.thumbs.alloc((size_t)nt.pool_cap() * SNAP_BYTES);
        nt.freelist.alloc(nt.pool_cap());
        nt.pending.alloc(nt.pool_cap());
        nt.commit_slot.alloc(nt.pool_cap());
        nt.commit_src.alloc(nt.pool_cap());
        const Tab &t = tabs[s];
        int have = 0, first = 0;
        if (keep && old_pool) {                   // slot indices stand: the old pool is the head of the new one
            if (n) {
                copy_live(nt.ints, t.ints, n, SNAP_ICOLS, nt.cap, t.cap);
                copy_live(nt.dbl, t.dbl, n, SNAP_DCOLS, nt.cap, t.cap);
            }
            YDS_HIP(hipMemcpy(nt.thumbs.p, t.thumbs.p, (size_t)old_pool * SNAP_BYTES, hipMemcpyDeviceToDevice));
            if (old_free) YDS_HIP(hipMemcpy(nt.freelist.p, t.freelist.p, (size_t)old_free * sizeof(int), hipMemcpyDeviceToDevice));
            YDS_HIP(hipMemset(nt.pending.p, 0xff, (size_t)old_pool * sizeof(int2)));
            have = old_free; first = old_pool;
        }
        tabs[s] = std::move(nt);
        push_free(tabs[s], s, have, first);
    }

    void set_stream(int stream, int cls, int min_w, int min_h) {
        check_stream(stream);
        if (cls < -1) fail("snapshots: class_id %d (-1 = any class)", cls);
        if (min_w < 1 || min_h < 1) fail("snapshots: min_w %d, min_h %d (both >= 1)", min_w, min_h);
        Spec sp;
        sp.cls = cls; sp.min_w = min_w; sp.min_h = min_h; sp.set = true;
        specs[stream] = sp;
        reset(stream);
    }
    // empty tables, empty rings and every picture free for one stream, or for all (-1)
    void reset(int stream) {
        TrackStage::reset(stream);
        for (int s = 0; s < S; ++s) {
            if (stream >= 0 && s != stream) continue;
            YDS_HIP(hipMemset(closed.p + s, 0, sizeof(long long)));
            push_free(tabs[s], s, 0, 0);
        }
    }

    void set_pixels(const uint8_t *frames, const FrameGeom *by_tag, int n, bool bgr) override {
        px_frames = frames;
        px_geom.assign(by_tag, by_tag + std::max(n, 0));
        px_bgr = bgr;
    }

    void enqueue(const ActFrame *fr, int n, hipStream_t s) override { enqueue_ex(fr, n, s, nullptr, 0); }

    // rows_host (the stand-alone entry): a host array that travels to the device inside the call's input block (open_blocks)
    void enqueue_ex(const ActFrame *fr, int n, hipStream_t s, const int32_t *rows_host, size_t n_rows_host) {
        const uint8_t *const frames = std::exchange(px_frames, nullptr);         // (the pixels of one call: the next one brings its own)
        // (what the call refuses comes before plan(): a refused call leaves nothing pending and grows nothing)
        if (n > 0 && !frames) fail("snapshots: no frames were handed over for this call (set_pixels)");
        if (n > 65535) fail("snapshots: %d frames are too many for one launch", n);
        for (int i = 0; i < n; ++i)
            if (fr[i].tag < 0 || fr[i].tag >= (int)px_geom.size()) fail("snapshots: frame %d carries tag %d, the call has the pixels of %zu frames", i, fr[i].tag, px_geom.size());
        std::vector<int> rows_of(S, 0);
        const StagePlan P = plan(fr, n, [&](int st, int need) { rows_of[st] = need - count_host[st]; grow(st, need); });
        if (!P.n_wg) return;
        // ---- blocks: input = works | frames | rows; results = items of every frame | entry counts | free slot counts | items
        const size_t works_b = (size_t)P.n_wg * sizeof(SnapWork);
        size_t res_total = (size_t)n + 2 * P.n_wg;
        pending_ev.resize(n);
        pending_cap.resize(n);
        std::vector<int> table(count_host);                                       // the most entries a stream's table can hold at each frame
        for (int i = 0; i < n; ++i) {
            table[fr[i].stream] += fr[i].n_rows;
            pending_ev[i] = res_total;
            pending_cap[i] = specs[fr[i].stream].set ? fr[i].n_rows + table[fr[i].stream] : 0;
            res_total += (size_t)pending_cap[i] * 6;
        }
        open_blocks(P, works_b + (size_t)n * sizeof(SnapFrameDev), rows_host, n_rows_host, res_total);
        if ((size_t)P.n_wg * P.max_rows * 3 > sx.n) sx.alloc((size_t)P.n_wg * P.max_rows * 3 * 2);
        if ((size_t)n * P.max_rows > scores.n) scores.alloc((size_t)n * P.max_rows * 2);
        SnapWork *w = reinterpret_cast<SnapWork *>(in_host.p);
        SnapFrameDev *fd = reinterpret_cast<SnapFrameDev *>(in_host.p + works_b);
        int commit_max = 0;
        bool any = false;
        for (int k = 0; k < P.n_wg; ++k) {
            const int st = wg_stream[k];
            SnapWork g;
            g.tab = dev_tab(st); g.pool = dev_pool(st); g.ring = dev_ring(st);
            g.cls = specs[st].cls; g.skip = specs[st].set ? 0 : 1;
            g.f0 = P.start[st]; g.f1 = P.start[st] + P.n_of[st];
            g.srows = wg_srows(k);
            g.sx = sx.p + (size_t)k * P.max_rows * 3;
            g.res_count = n + k; g.res_free = n + P.n_wg + k;
            w[k] = g;
            if (specs[st].set) { commit_max = std::max(commit_max, std::min(tabs[st].pool_cap(), rows_of[st])); any = true; }
        }
        for (int e = 0; e < n; ++e) {
            const int i = P.order[e];
            const ActFrame &f = fr[i];
            const FrameGeom &gm = px_geom[f.tag];
            const Spec &sp = specs[f.stream];
            SnapFrameDev d;
            d.rows = dev_rows(f);
            d.n_p = f.n_rows_p;
            d.t = f.t; d.off = gm.off; d.h = gm.h; d.w = gm.w;
            d.n = f.n_rows; d.tag = f.tag;
            d.cls = sp.cls; d.min_w = sp.min_w; d.min_h = sp.min_h; d.skip = sp.set ? 0 : 1;
            d.res_n = i; d.res_ev = (int)pending_ev[i]; d.ev_cap = pending_cap[i];
            fd[e] = d;
        }
        const SnapWork *works_dev = reinterpret_cast<const SnapWork *>(in_dev.p);
        const SnapFrameDev *frames_dev = reinterpret_cast<const SnapFrameDev *>(in_dev.p + works_b);
        const int bgr = px_bgr ? 1 : 0, max_rows = P.max_rows;
        submit(s, [&] {
            t_score.begin(s);
            if (any) hipLaunchKernelGGL(snap_score_kernel, dim3(max_rows, n), dim3(256), 0, s, frames_dev, frames, bgr, max_rows, scores.p);
            t_score.end(s);
            t_decide.begin(s);
            hipLaunchKernelGGL(snap_decide_kernel, dim3(P.n_wg), dim3(256), 0, s, works_dev, frames_dev, scores.p, max_rows, max_age, A, res_host.p);
            t_decide.end(s);
            t_commit.begin(s);
            if (commit_max) hipLaunchKernelGGL(snap_commit_kernel, dim3(commit_max, P.n_wg), dim3(256), 0, s, works_dev, frames_dev, frames, bgr);
            t_commit.end(s);
        });
    }

    void collect() override {
        report.rows.clear();
        report.tags.clear();
        const int n = pending_n, n_wg = (int)wg_stream.size();
        collect_counts("snapshot items", [&](int i, int m) {
            const int *r = res_host.p + pending_ev[i];
            report.rows.insert(report.rows.end(), r, r + (size_t)m * 6);
            for (int k = 0; k < m; ++k) report.tags.push_back(r[(size_t)k * 6]);
        });
        for (int k = 0; n > 0 && k < n_wg; ++k) {
            if (!specs[wg_stream[k]].set) continue;
            const int f = res_host.p[n + n_wg + k];
            if (f < 0) fail("snapshots: the picture pool of stream %d lost count of its slots (free + held != %d)", wg_stream[k], tabs[wg_stream[k]].pool_cap());
            free_host[wg_stream[k]] = f;
        }
    }

    // pictures of `m` slots (a slot < 0: zeros) to out [m][128][64][3]
    void thumbs_out(int stream, const std::vector<int32_t> &slot, uint8_t *out) {
        if (!out) return;
        for (size_t k = 0; k < slot.size(); ++k) {
            uint8_t *d = out + k * SNAP_BYTES;
            if (slot[k] < 0 || slot[k] >= tabs[stream].pool_cap()) memset(d, 0, SNAP_BYTES);
            else YDS_HIP(hipMemcpy(d, tabs[stream].thumbs.p + (size_t)slot[k] * SNAP_BYTES, SNAP_BYTES, hipMemcpyDeviceToHost));
        }
    }

    int max_age, A;
    std::vector<Tab> tabs;
    std::vector<Spec> specs;
    std::vector<int> free_host;                   // free slots of every stream after the last collected call
    DevBuf<int> ring_i, n_free, n_commit, sx, scores;
    DevBuf<double> ring_d;
    DevBuf<long long> closed;
    std::vector<size_t> pending_ev;               // of the call in flight: where every frame's items begin in the result block
    const uint8_t *px_frames = nullptr;           // the pixels of the next call (set_pixels)
    std::vector<FrameGeom> px_geom;
    bool px_bgr = false;
    LaunchTimer t_score, t_decide, t_commit;
};

}  // namespace yds

static inline yds::Snap *impl(yds_snap *g) {
    if (!g) yds::fail("snapshots: NULL handle");
    return static_cast<yds::Snap *>(g->s);
}

extern "C" {

yds_snap *yds_snap_create(int n_streams, int max_age, int archive) {
    YDS_API_BEGIN
    return new yds_snap{new yds::Snap(n_streams, max_age, archive)};
    YDS_API_END_PTR
}
void yds_snap_destroy(yds_snap *g) {
    if (g) { delete g->s; delete g; }
}
int yds_snap_set_stream(yds_snap *g, int stream, int class_id, int min_w, int min_h) {
    YDS_API_BEGIN
    impl(g)->set_stream(stream, class_id, min_w, min_h);
    YDS_API_END
}
int yds_snap_reset(yds_snap *g, int stream) {
    YDS_API_BEGIN
    impl(g)->check_stream(stream, -1);
    impl(g)->reset(stream);
    YDS_API_END
}
int yds_snap_update(yds_snap *g, const int32_t *rows6_host, const int32_t *first, const int32_t *stream_of, const double *frame_time, int n_frames,
                    const uint8_t *frames_dev, const uint64_t *frame_off, const int32_t *frame_hw, size_t frames_bytes, int bgr, int32_t *out6_host,
                    int32_t *first_out, int cap, int *n_out) {
    YDS_API_BEGIN
    yds::Snap *G = impl(g);
    const std::vector<yds::ActFrame> fr = yds::csr_frames("snapshots", rows6_host, first, stream_of, frame_time, false, n_frames, n_out);
    if (fr.empty()) return 0;
    if (!frames_dev) yds::fail("snapshots: NULL frames");
    const std::vector<yds::FrameGeom> geom = yds::checked_layout(frame_off, frame_hw, n_frames, frames_bytes);      // (before anything runs)
    G->set_pixels(frames_dev, geom.data(), n_frames, bgr != 0);
    G->enqueue_ex(fr.data(), n_frames, G->own_stream, rows6_host, (size_t)first[n_frames]);
    G->finish_alone();
    const int m = G->give_count("snapshot items", (int)(G->report.rows.size() / 6), cap, n_out);
    if (m) {
        if (!out6_host) yds::fail("snapshots: NULL argument");
        memcpy(out6_host, G->report.rows.data(), (size_t)m * 6 * sizeof(int32_t));
    }
    if (first_out) memcpy(first_out, G->first.data(), ((size_t)n_frames + 1) * sizeof(int32_t));
    YDS_API_END
}
int yds_snap_get_tracks(yds_snap *g, int stream, int32_t *ids, int32_t *classes, int32_t *scores, int32_t *n_seen, int32_t *box4, int32_t *tag_best,
                        double *t_first, double *t_best, double *t_last, uint8_t *thumbs, int cap, int *n) {
    YDS_API_BEGIN
    yds::Snap *G = impl(g);
    const int m = G->table_count(stream, "tracks", cap, n);
    if (!m) return 0;
    const yds::SnapTab tb = G->dev_tab(stream);
    const size_t c2 = 2 * (size_t)tb.cap;
    G->column_out(ids, tb.ic + yds::SC_ID * c2, m);
    G->column_out(classes, tb.ic + yds::SC_CLS * c2, m);
    G->column_out(scores, tb.ic + yds::SC_SCORE * c2, m);
    G->column_out(n_seen, tb.ic + yds::SC_SEEN * c2, m);
    G->column_out(tag_best, tb.ic + yds::SC_TAG * c2, m);
    if (box4) {
        std::vector<int32_t> col(m);
        for (int c = 0; c < 4; ++c) {
            G->column_out(col.data(), tb.ic + (yds::SC_X1 + c) * c2, m);
            for (int e = 0; e < m; ++e) box4[(size_t)e * 4 + c] = col[e];
        }
    }
    double *const dcol[3] = {t_first, t_best, t_last};
    for (int c = 0; c < 3; ++c)
        if (dcol[c]) YDS_HIP(hipMemcpy(dcol[c], tb.dc + c * c2, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (thumbs) {
        std::vector<int32_t> slot(m);
        G->column_out(slot.data(), tb.ic + yds::SC_SLOT * c2, m);
        G->thumbs_out(stream, slot, thumbs);
    }
    YDS_API_END
}
int yds_snap_get_archive(yds_snap *g, int stream, int32_t *ids, int32_t *classes, int32_t *scores, int32_t *n_seen, int32_t *box4, int32_t *tag_best,
                         double *t_first, double *t_best, double *t_last, double *t_closed, uint8_t *thumbs, int cap, int *n) {
    YDS_API_BEGIN
    yds::Snap *G = impl(g);
    G->check_stream(stream);
    long long closed = 0;
    YDS_HIP(hipMemcpy(&closed, G->closed.p + stream, sizeof(long long), hipMemcpyDeviceToHost));
    const int A = G->A;
    const int m = G->give_count("archived snapshots", (int)std::min<long long>(closed, A), cap, n);
    if (!m) return 0;
    const yds::SnapRing rg = G->dev_ring(stream);
    std::vector<int32_t> ic((size_t)yds::SNAP_AICOLS * A);
    std::vector<double> dc((size_t)yds::SNAP_ADCOLS * A);
    YDS_HIP(hipMemcpy(ic.data(), rg.ic, ic.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    YDS_HIP(hipMemcpy(dc.data(), rg.dc, dc.size() * sizeof(double), hipMemcpyDeviceToHost));
    const int start = closed >= A ? (int)(closed % A) : 0;                        // oldest first
    std::vector<int32_t> slot(m);
    double *const dcol[4] = {t_first, t_best, t_last, t_closed};
    for (int k = 0; k < m; ++k) {
        const int pos = (start + k) % A;
        auto col = [&](int c) { return ic[(size_t)c * A + pos]; };
        if (ids) ids[k] = col(yds::SA_ID);
        if (classes) classes[k] = col(yds::SA_CLS);
        if (scores) scores[k] = col(yds::SA_SCORE);
        if (n_seen) n_seen[k] = col(yds::SA_SEEN);
        if (tag_best) tag_best[k] = col(yds::SA_TAG);
        if (box4) for (int c = 0; c < 4; ++c) box4[(size_t)k * 4 + c] = col(yds::SA_X1 + c);
        for (int c = 0; c < 4; ++c) if (dcol[c]) dcol[c][k] = dc[(size_t)c * A + pos];
        slot[k] = col(yds::SA_SLOT);
    }
    G->thumbs_out(stream, slot, thumbs);
    YDS_API_END
}
int yds_snap_get_pool(yds_snap *g, int stream, int *n_free, int *n_slots) {
    YDS_API_BEGIN
    yds::Snap *G = impl(g);
    G->check_stream(stream);
    if (!n_free || !n_slots) yds::fail("snapshots: NULL argument");
    YDS_HIP(hipMemcpy(n_free, G->n_free.p + stream, sizeof(int), hipMemcpyDeviceToHost));
    if (*n_free != G->free_host[stream]) yds::fail("snapshots: stream %d has %d free slots on the device, %d came back with the last call", stream, *n_free, G->free_host[stream]);
    *n_slots = G->tabs[stream].pool_cap();
    YDS_API_END
}
int yds_snap_set_timing(yds_snap *g, int on) {
    YDS_API_BEGIN
    yds::Snap *G = impl(g);
    G->timer.set(on != 0); G->t_score.set(on != 0); G->t_decide.set(on != 0); G->t_commit.set(on != 0);
    YDS_API_END
}
int yds_snap_last_us(yds_snap *g, int what, float *us) {
    YDS_API_BEGIN
    yds::Snap *G = impl(g);
    if (what < 0 || what > 2) yds::fail("snapshots: last_us of %d (0 = the score launch, 1 = decide, 2 = commit)", what);
    *us = (what == 0 ? G->t_score : what == 1 ? G->t_decide : G->t_commit).us("snap");
    YDS_API_END
}

}  // extern "C"
