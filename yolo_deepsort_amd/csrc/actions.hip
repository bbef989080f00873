// Action identification on the device: the orbit caches of ActionIdentify for S video streams in HBM, advanced by one launch per call.
//
// Replaces the per-row, per-frame host loop of the reference:
//   ActionIdentify.update                       action/action_Identify.py:15-47
//   Orbit (foot point ring + timestamps)        action/orbit.py:5-25
//   TakeOff / Landing / Glide / FastCrossing / BreakInto .confirm   action/actions.py:24-150
// A stream's cache is a table in dict insertion order: id, class, age, ring length, ring head, and max_size (x, y, t) doubles per
// entry.  One workgroup per stream that has frames in the call walks that stream's frames in time order; per frame it stages the rows
// once (they may sit in pinned host memory: a tracker result block), updates / registers / ages / drops entries with ordered
// compactions (tracker_dev.h compact_ordered), and emits (frame, id, class, action) rows entry-major, action-minor - count, prefix,
// write - straight into a pinned result block.  All arithmetic is double in the operation order of the Python expressions (the tree
// is built with -ffp-contract=off), so the rows equal the host module's.  What the stage shares with the zone stage - the workgroup's
// table steps, the host's bookkeeping per call - is track_stage.h.
#include "track_stage.h"
#include "ydsort.h"

namespace yds {

struct ActDesc { int kind, class_id; double p0, p1; };

// table of one stream: `cap` entries, every field twice (the second copy takes the survivors of a removal)
struct ActTab {
    int *id, *cls, *age, *len, *head;            // [2][cap] each: [0, cap) live, [cap, 2 cap) the removal's target
    double *pts;                                  // [2][cap][max_size][3]  x, y, t
    int *count;                                   // live entries (device)
    int cap;
};
// one workgroup's job: its stream's table and frames [f0, f1) of the call's frame list (sorted by stream, order kept)
struct ActWork {
    ActTab tab;
    int f0, f1;
    int *srows;                                   // staging [max rows of a frame][6]
    double *stime;                                //         [max rows of a frame]
    int res_count;                                // int index in the result block of this stream's entry count
};
struct ActFrameDev {
    const int *rows;
    const int *n_p;
    const double *row_time;
    double t;
    int n, tag;
    int res_n;                                    // int index in the result block of this frame's row count
    int res_rows;                                 // ... of its rows [n * A][4]
};

__device__ __forceinline__ bool act_confirm(const ActDesc &a, const ActTab &T, int e, int ms) {
    if (T.cls[e] != a.class_id) return false;
    const int len = T.len[e];
    if (a.kind == YDS_ACT_BREAK_INTO) return (double)len > a.p0;             // actions.py:144-150
    if (len < 2) return false;
    const int head = T.head[e];
    const double *P = T.pts + (size_t)e * ms * 3;
    int k = head;
    double px = P[k * 3], py = P[k * 3 + 1], pt = P[k * 3 + 2];
    for (int i = 1; i < len; ++i) {
        k = k + 1 == ms ? 0 : k + 1;
        const double cx = P[k * 3], cy = P[k * 3 + 1], ct = P[k * 3 + 2];
        bool ok;
        switch (a.kind) {
        case YDS_ACT_TAKEOFF: ok = py - cy > a.p1 && fabs(px - cx) > a.p0; break;             // actions.py:32-50
        case YDS_ACT_LANDING: ok = cy - py > a.p1 && fabs(px - cx) > a.p0; break;             // actions.py:60-78
        case YDS_ACT_GLIDE: ok = fabs(cy - py) < a.p1 && fabs(cx - px) > a.p0; break;         // actions.py:88-105
        default: ok = fabs(cx - px) / ((ct - pt) * 1000.0) > a.p0; break;                     // actions.py:115-134
        }
        if (!ok) return false;
        px = cx; py = cy; pt = ct;
    }
    return true;
}

__global__ __launch_bounds__(256) void act_update_kernel(const ActWork *works, const ActFrameDev *frames, const ActDesc *acts, int A, int max_age,
                                                         int ms, int *res) {
    __shared__ int s_cnt[4];
    __shared__ ActDesc s_act[YDS_ACT_MAX_ACTIONS];
    const ActWork W = works[blockIdx.x];
    const ActTab T = W.tab;
    const int tid = threadIdx.x, cap = T.cap;
    if (tid < A) s_act[tid] = acts[tid];
    int n = *T.count;
    __syncthreads();
    for (int f = W.f0; f < W.f1; ++f) {
        const ActFrameDev F = frames[f];
        const int R = stage_frame_rows(F.rows, F.n_p, F.n, W.srows);
        for (int j = tid; j < R; j += 256) W.stime[j] = F.row_time ? F.row_time[j] : F.t;
        __syncthreads();
        // ---- cached ids: Orbit.update (orbit.py:22-25), else age += 1 (action_Identify.py:27-34)
        for (int e = tid; e < n; e += 256) {
            const int j = find_row(W.srows, R, T.id[e]);
            if (j == R) { T.age[e] += 1; continue; }
            const int *r = W.srows + j * 6;
            const int len = T.len[e], head = T.head[e];
            int pos;
            if (len < ms) { pos = head + len; if (pos >= ms) pos -= ms; T.len[e] = len + 1; }
            else { pos = head; T.head[e] = head + 1 == ms ? 0 : head + 1; }
            double *p = T.pts + ((size_t)e * ms + pos) * 3;
            p[0] = (double)r[0] + ((double)r[2] - (double)r[0]) / 2.0;           // orbit.py:16-20
            p[1] = (double)r[3];
            p[2] = W.stime[j];
            T.age[e] = 0;
        }
        // ---- unknown ids are registered in row order, no point yet (action_Identify.py:23-25)
        const int n_all = register_unknown(R, n, cap, s_cnt, T.id, W.srows, [&](int e, const int *r) {
            T.id[e] = r[4]; T.cls[e] = r[5]; T.age[e] = 0; T.len[e] = 0; T.head[e] = 0;
        });
        __syncthreads();
        // ---- entries that reached max_age leave, the rest keep their order (only an entry that just aged has age > 0 tested)
        auto keep = [&](int e) { const int a = T.age[e]; return !(a > 0 && a >= max_age); };
        int dead = 0;
        for (int base = 0; base < n; base += 256) dead += __syncthreads_count(base + tid < n && !keep(base + tid));
        int n_live = n_all;
        if (dead) {
            auto move = [&](int d, int e) { T.id[d] = T.id[e]; T.cls[d] = T.cls[e]; T.age[d] = T.age[e]; T.len[d] = T.len[e]; T.head[d] = T.head[e]; };
            n_live = retire(n_all, cap, s_cnt, keep, [&](int d, int e) {
                move(d, e);
                const double *src = T.pts + (size_t)e * ms * 3;
                double *dst = T.pts + (size_t)d * ms * 3;
                for (int k = 0; k < ms * 3; ++k) dst[k] = src[k];
            }, move);
            for (size_t k = tid; k < (size_t)n_live * ms * 3; k += 256) T.pts[k] = T.pts[(size_t)cap * ms * 3 + k];
            __syncthreads();
        }
        // ---- every entry seen in this frame, in cache order, by every action in list order (action_Identify.py:36-46)
        int *out = res + F.res_rows;
        const int out_cap = F.n * A;
        const int total = compact_ordered(n_live * A, s_cnt, [&](int i) {
            const int e = i / A;
            return T.age[e] == 0 && act_confirm(s_act[i - e * A], T, e, ms);
        }, [&](int i, int r) {
            if (r >= out_cap) return;
            const int e = i / A;
            int *o = out + (size_t)r * 4;
            o[0] = F.tag; o[1] = T.id[e]; o[2] = T.cls[e]; o[3] = i - e * A;
        });
        if (tid == 0) res[F.res_n] = total;
        n = n_live;
        __syncthreads();
    }
    if (tid == 0) { *T.count = n; res[W.res_count] = n; }
}

class Actions : public TrackStage<ActionsIface> {
public:
    Actions(int S, const int32_t *kind, const int32_t *class_id, const double *param, int A, int max_age, int max_size)
        : TrackStage("actions", S), A(A), max_age(max_age), ms(max_size), tabs(S) {
        if (A < 0 || A > YDS_ACT_MAX_ACTIONS) fail("actions: %d actions outside [0,%d]", A, YDS_ACT_MAX_ACTIONS);
        if (max_size < 1 || max_size > YDS_ACT_MAX_SIZE) fail("actions: max_size %d outside [1,%d]", max_size, YDS_ACT_MAX_SIZE);
        std::vector<ActDesc> d(std::max(A, 1));
        for (int a = 0; a < A; ++a) {
            if (kind[a] < YDS_ACT_TAKEOFF || kind[a] > YDS_ACT_BREAK_INTO) fail("actions: action %d has unknown kind %d", a, kind[a]);
            d[a] = ActDesc{kind[a], class_id[a], param[2 * a], param[2 * a + 1]};
        }
        acts.alloc(d.size());
        YDS_HIP(hipMemcpy(acts.p, d.data(), d.size() * sizeof(ActDesc), hipMemcpyHostToDevice));
    }

    struct Tab {
        DevBuf<int> ints;         // id | cls | age | len | head, [2][cap] each
        DevBuf<double> pts;
        int cap = 0;
    };
    ActTab dev_tab(int s) {
        Tab &t = tabs[s];
        const size_t c2 = 2 * (size_t)t.cap;
        return ActTab{t.ints.p, t.ints.p + c2, t.ints.p + 2 * c2, t.ints.p + 3 * c2, t.ints.p + 4 * c2, t.pts.p, counts.p + s, t.cap};
    }
    void grow(int s, int need) {
        const size_t n = count_host[s];
        grow_table(tabs[s], need, n, [&](Tab &nt) {
            nt.ints.alloc(10 * (size_t)nt.cap);
            nt.pts.alloc(2 * (size_t)nt.cap * ms * 3);
        }, [&](Tab &nt, const Tab &t) {
            copy_live(nt.ints, t.ints, n, 5, nt.cap, t.cap);
            copy_live(nt.pts, t.pts, n * ms * 3);
        });
    }

    void enqueue(const ActFrame *fr, int n, hipStream_t s) override { enqueue_ex(fr, n, s, nullptr, 0, nullptr, 0); }

    // rows_host / time_host (the stand-alone entry): host arrays that travel to the device inside the call's input block (open_blocks)
    void enqueue_ex(const ActFrame *fr, int n, hipStream_t s, const int32_t *rows_host, size_t n_rows_host, const double *time_host, size_t n_time_host) {
        const StagePlan P = plan(fr, n, [&](int st, int need) { grow(st, need); });
        if (!P.n_wg) return;
        // ---- blocks: input = works | frames | row times | rows, result = frame counts | entry counts | rows
        const size_t works_b = (size_t)P.n_wg * sizeof(ActWork), time_off = works_b + (size_t)n * sizeof(ActFrameDev);
        size_t res_total = (size_t)n + P.n_wg;
        pending_rows.resize(n);
        pending_cap.resize(n);
        for (int i = 0; i < n; ++i) {
            pending_rows[i] = res_total;
            pending_cap[i] = fr[i].n_rows * A;
            res_total += (size_t)fr[i].n_rows * A * 4;
        }
        open_blocks(P, time_off + n_time_host * sizeof(double), rows_host, n_rows_host, res_total);
        if ((size_t)P.n_wg * P.max_rows > stime.n) stime.alloc((size_t)P.n_wg * P.max_rows * 2);
        const double *time_dev = reinterpret_cast<const double *>(in_dev.p + time_off);
        ActWork *w = reinterpret_cast<ActWork *>(in_host.p);
        ActFrameDev *fd = reinterpret_cast<ActFrameDev *>(in_host.p + works_b);
        for (int k = 0; k < P.n_wg; ++k) {
            const int st = wg_stream[k];
            w[k] = ActWork{dev_tab(st), P.start[st], P.start[st] + P.n_of[st], wg_srows(k), stime.p + (size_t)k * P.max_rows, n + k};
        }
        for (int e = 0; e < n; ++e) {
            const ActFrame &f = fr[P.order[e]];
            ActFrameDev d;
            d.rows = dev_rows(f);
            d.n_p = f.n_rows_p;
            // (row_time of the stand-alone entry points into time_host, which travels in the block like the rows)
            d.row_time = f.row_time ? (time_host ? time_dev + (f.row_time - time_host) : f.row_time) : nullptr;
            d.t = f.t; d.n = f.n_rows; d.tag = f.tag;
            d.res_n = P.order[e];
            d.res_rows = (int)pending_rows[P.order[e]];
            fd[e] = d;
        }
        if (n_time_host) memcpy(in_host.p + time_off, time_host, n_time_host * sizeof(double));
        submit(s, [&] {
            hipLaunchKernelGGL(act_update_kernel, dim3(P.n_wg), dim3(256), 0, s, reinterpret_cast<const ActWork *>(in_dev.p),
                               reinterpret_cast<const ActFrameDev *>(in_dev.p + works_b), acts.p, A, max_age, ms, res_host.p);
        });
    }

    void collect() override {
        report.rows.clear();
        collect_counts("rows", [&](int i, int m) {
            const int *r = res_host.p + pending_rows[i];
            report.rows.insert(report.rows.end(), r, r + (size_t)m * 4);
        });
    }

    int A, max_age, ms;
    std::vector<Tab> tabs;
    DevBuf<ActDesc> acts;
    DevBuf<double> stime;                         // staging [n_wg][max rows of a frame]
    std::vector<size_t> pending_rows;             // of the call in flight: where every frame's rows begin in the result block
};

}  // namespace yds

static inline yds::Actions *impl(yds_act *h) {
    if (!h) yds::fail("actions: NULL handle");
    return static_cast<yds::Actions *>(h->a);
}

extern "C" {

yds_act *yds_actions_create(int n_streams, const int32_t *kind, const int32_t *class_id, const double *param, int n_actions, int max_age,
                            int max_size) {
    YDS_API_BEGIN
    if (n_actions > 0 && (!kind || !class_id || !param)) yds::fail("actions: NULL descriptor");
    return new yds_act{new yds::Actions(n_streams, kind, class_id, param, n_actions, max_age, max_size)};
    YDS_API_END_PTR
}
void yds_actions_destroy(yds_act *a) {
    if (a) { delete a->a; delete a; }
}
int yds_actions_reset(yds_act *a, int stream) {
    YDS_API_BEGIN
    impl(a)->reset(stream);
    YDS_API_END
}
int yds_actions_update(yds_act *a, const int32_t *rows6_host, const int32_t *first, const int32_t *stream_of, const double *row_time,
                       int n_frames, int32_t *out4_host, int cap, int *n_out) {
    YDS_API_BEGIN
    yds::Actions *A = impl(a);
    const std::vector<yds::ActFrame> fr = yds::csr_frames("actions", rows6_host, first, stream_of, row_time, true, n_frames, n_out);
    if (fr.empty()) return 0;
    const size_t n_rows = first[n_frames];
    A->enqueue_ex(fr.data(), n_frames, A->own_stream, rows6_host, n_rows, row_time, n_rows);
    A->finish_alone();
    const int m = A->give_count("action rows", (int)(A->report.rows.size() / 4), cap, n_out);
    if (m) memcpy(out4_host, A->report.rows.data(), (size_t)m * 4 * sizeof(int32_t));
    YDS_API_END
}
int yds_actions_get_orbits(yds_act *a, int stream, int32_t *ids, int32_t *ages, int32_t *lens, int cap, int *n) {
    YDS_API_BEGIN
    yds::Actions *A = impl(a);
    const int m = A->table_count(stream, "orbits", cap, n);
    const yds::ActTab t = A->dev_tab(stream);
    A->column_out(ids, t.id, m);
    A->column_out(ages, t.age, m);
    A->column_out(lens, t.len, m);
    YDS_API_END
}
int yds_actions_set_timing(yds_act *a, int on) {
    YDS_API_BEGIN
    impl(a)->timer.set(on != 0);
    YDS_API_END
}
int yds_actions_last_us(yds_act *a, float *us) {
    YDS_API_BEGIN
    *us = impl(a)->timer.us("actions");
    YDS_API_END
}

}  // extern "C"
