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
// is built with -ffp-contract=off), so the rows equal the host module's.
#include "tracker_dev.h"
#include "ydsort.h"

#include <limits.h>

#include <memory>

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
        const int R = F.n_p ? min(max(*F.n_p, 0), F.n) : F.n;
        for (int k = tid; k < R * 6; k += 256) W.srows[k] = F.rows[k];
        for (int j = tid; j < R; j += 256) W.stime[j] = F.row_time ? F.row_time[j] : F.t;
        __syncthreads();
        // ---- cached ids: Orbit.update (orbit.py:22-25), else age += 1 (action_Identify.py:27-34)
        for (int e = tid; e < n; e += 256) {
            const int id = T.id[e];
            int j = 0;
            while (j < R && W.srows[j * 6 + 4] != id) ++j;
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
        const int added = compact_ordered(R, s_cnt, [&](int j) {
            const int id = W.srows[j * 6 + 4];
            for (int e = 0; e < n; ++e) if (T.id[e] == id) return false;
            return true;
        }, [&](int j, int r) {
            const int e = n + r;
            if (e >= cap) return;                                                 // (the host sized the table for every row of the call)
            T.id[e] = W.srows[j * 6 + 4]; T.cls[e] = W.srows[j * 6 + 5]; T.age[e] = 0; T.len[e] = 0; T.head[e] = 0;
        });
        const int n_all = min(n + added, cap);
        __syncthreads();
        // ---- entries that reached max_age leave, the rest keep their order (only an entry that just aged has age > 0 tested)
        auto keep = [&](int e) { const int a = T.age[e]; return !(a > 0 && a >= max_age); };
        int dead = 0;
        for (int base = 0; base < n; base += 256) dead += __syncthreads_count(base + tid < n && !keep(base + tid));
        int n_live = n_all;
        if (dead) {
            n_live = compact_ordered(n_all, s_cnt, keep, [&](int e, int r) {
                const int d = cap + r;
                T.id[d] = T.id[e]; T.cls[d] = T.cls[e]; T.age[d] = T.age[e]; T.len[d] = T.len[e]; T.head[d] = T.head[e];
                const double *src = T.pts + (size_t)e * ms * 3;
                double *dst = T.pts + (size_t)d * ms * 3;
                for (int k = 0; k < ms * 3; ++k) dst[k] = src[k];
            });
            __syncthreads();
            for (int e = tid; e < n_live; e += 256) {
                const int d = cap + e;
                T.id[e] = T.id[d]; T.cls[e] = T.cls[d]; T.age[e] = T.age[d]; T.len[e] = T.len[d]; T.head[e] = T.head[d];
            }
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

class Actions : public ActionsIface {
public:
    Actions(int S, const int32_t *kind, const int32_t *class_id, const double *param, int A, int max_age, int max_size)
        : S(S), A(A), max_age(max_age), ms(max_size), tabs(S), count_host(S, 0) {
        if (S < 1) fail("actions: %d streams", S);
        if (A < 0 || A > YDS_ACT_MAX_ACTIONS) fail("actions: %d actions outside [0,%d]", A, YDS_ACT_MAX_ACTIONS);
        if (max_size < 1 || max_size > YDS_ACT_MAX_SIZE) fail("actions: max_size %d outside [1,%d]", max_size, YDS_ACT_MAX_SIZE);
        std::vector<ActDesc> d(std::max(A, 1));
        for (int a = 0; a < A; ++a) {
            if (kind[a] < YDS_ACT_TAKEOFF || kind[a] > YDS_ACT_BREAK_INTO) fail("actions: action %d has unknown kind %d", a, kind[a]);
            d[a] = ActDesc{kind[a], class_id[a], param[2 * a], param[2 * a + 1]};
        }
        acts.alloc(d.size());
        YDS_HIP(hipMemcpy(acts.p, d.data(), d.size() * sizeof(ActDesc), hipMemcpyHostToDevice));
        counts.alloc(S);
        YDS_HIP(hipMemset(counts.p, 0, S * sizeof(int)));
        own_stream = make_stream(true);
        YDS_HIP(hipEventCreate(&ev0));
        YDS_HIP(hipEventCreate(&ev1));
    }
    ~Actions() override {
        if (in_host) (void)hipHostFree(in_host);
        if (res_host) (void)hipHostFree(res_host);
        (void)hipEventDestroy(ev0);
        (void)hipEventDestroy(ev1);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
    int streams() const override { return S; }

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
    // room for `need` entries; nothing of this handle is in flight between calls (every call ends behind a synchronisation)
    void grow(int s, int need) {
        Tab &t = tabs[s];
        if (need <= t.cap) return;
        int c = std::max(t.cap, 64);
        while (c < need) c *= 2;
        Tab nt;
        nt.cap = c;
        nt.ints.alloc(10 * (size_t)c);
        nt.pts.alloc(2 * (size_t)c * ms * 3);
        const int n = count_host[s];
        if (n) {
            for (int fld = 0; fld < 5; ++fld)
                YDS_HIP(hipMemcpy(nt.ints.p + (size_t)fld * 2 * c, t.ints.p + (size_t)fld * 2 * t.cap, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice));
            YDS_HIP(hipMemcpy(nt.pts.p, t.pts.p, (size_t)n * ms * 3 * sizeof(double), hipMemcpyDeviceToDevice));
        }
        t = std::move(nt);
    }

    void enqueue(const ActFrame *fr, int n, hipStream_t s) override { enqueue_ex(fr, n, s, nullptr, 0, nullptr, 0); }

    // rows_host / time_host (the stand-alone entry): host arrays that travel to the device inside the call's input block; the frames'
    // rows6 / row_time then point INTO those host arrays and are translated to the block's device addresses

    void enqueue_ex(const ActFrame *fr, int n, hipStream_t s, const int32_t *rows_host, size_t n_rows_host, const double *time_host, size_t n_time_host) {
        pending_n = n;
        order.clear();
        if (n <= 0) return;
        // ---- frames by stream, order kept; a workgroup per stream with frames
        std::vector<int> n_of(S, 0), rows_of(S, 0);
        int max_rows = 1;
        for (int i = 0; i < n; ++i) {
            if (fr[i].stream < 0 || fr[i].stream >= S) fail("actions: frame %d names stream %d outside [0,%d)", i, fr[i].stream, S);
            if (fr[i].n_rows < 0) fail("actions: frame %d has %d rows", i, fr[i].n_rows);
            ++n_of[fr[i].stream];
            rows_of[fr[i].stream] += fr[i].n_rows;
            max_rows = std::max(max_rows, fr[i].n_rows);
        }
        std::vector<int> wg_of(S, -1), start(S, 0);
        int n_wg = 0, acc = 0;
        for (int st = 0; st < S; ++st) {
            if (!n_of[st]) continue;
            wg_of[st] = n_wg++;
            start[st] = acc;
            acc += n_of[st];
            grow(st, count_host[st] + rows_of[st]);
        }
        order.assign(n, 0);                       // order[slot in the sorted list] = frame of the call
        {
            std::vector<int> fill(start);
            for (int i = 0; i < n; ++i) order[fill[fr[i].stream]++] = i;
        }
        // ---- blocks: input = works | frames | payload (8-byte aligned pieces), result = frame counts | entry counts | rows
        const size_t works_b = (size_t)n_wg * sizeof(ActWork), frames_b = (size_t)n * sizeof(ActFrameDev);
        const size_t time_off = works_b + frames_b, rows_off = time_off + n_time_host * sizeof(double);
        const size_t in_total = rows_off + n_rows_host * 6 * sizeof(int32_t);
        size_t res_total = (size_t)n + n_wg;
        std::vector<size_t> res_rows(n);
        for (int i = 0; i < n; ++i) { res_rows[i] = res_total; res_total += (size_t)fr[i].n_rows * A * 4; }
        if (res_total > (size_t)INT_MAX) fail("actions: result block of %zu ints", res_total);
        if (in_total > in_cap) {
            if (in_host) (void)hipHostFree(in_host);
            in_host = nullptr;
            in_cap = in_total * 2;
            YDS_HIP(hipHostMalloc((void **)&in_host, in_cap));
            in_dev.alloc(in_cap);
        }
        if (res_total > res_cap) {
            if (res_host) (void)hipHostFree(res_host);
            res_host = nullptr;
            res_cap = res_total * 2;
            YDS_HIP(hipHostMalloc((void **)&res_host, res_cap * sizeof(int)));
        }
        if ((size_t)n_wg * max_rows * 6 > srows.n) { srows.alloc((size_t)n_wg * max_rows * 6 * 2); }
        if ((size_t)n_wg * max_rows > stime.n) { stime.alloc((size_t)n_wg * max_rows * 2); }
        const int32_t *rows_dev = reinterpret_cast<const int32_t *>(in_dev.p + rows_off);
        const double *time_dev = reinterpret_cast<const double *>(in_dev.p + time_off);
        ActWork *w = reinterpret_cast<ActWork *>(in_host);
        ActFrameDev *fd = reinterpret_cast<ActFrameDev *>(in_host + works_b);
        for (int st = 0; st < S; ++st) {
            if (wg_of[st] < 0) continue;
            const int k = wg_of[st];
            w[k] = ActWork{dev_tab(st), start[st], start[st] + n_of[st], srows.p + (size_t)k * max_rows * 6, stime.p + (size_t)k * max_rows, n + k};
        }
        for (int e = 0; e < n; ++e) {
            const ActFrame &f = fr[order[e]];
            ActFrameDev d;
            // rows6 / row_time of the stand-alone entry are offsets into the uploaded payload, marked by rows_host
            d.rows = rows_host ? rows_dev + (f.rows6 - rows_host) : f.rows6;
            d.n_p = f.n_rows_p;
            d.row_time = f.row_time ? (time_host ? time_dev + (f.row_time - time_host) : f.row_time) : nullptr;
            d.t = f.t; d.n = f.n_rows; d.tag = f.tag;
            d.res_n = order[e];
            d.res_rows = (int)res_rows[order[e]];
            fd[e] = d;
        }
        if (n_time_host) memcpy(in_host + time_off, time_host, n_time_host * sizeof(double));
        if (n_rows_host) memcpy(in_host + rows_off, rows_host, n_rows_host * 6 * sizeof(int32_t));
        wg_stream.assign(n_wg, 0);
        for (int st = 0; st < S; ++st) if (wg_of[st] >= 0) wg_stream[wg_of[st]] = st;
        pending_rows.assign(res_rows.begin(), res_rows.end());
        pending_cap.resize(n);
        for (int i = 0; i < n; ++i) pending_cap[i] = fr[i].n_rows * A;
        YDS_HIP(hipMemcpyAsync(in_dev.p, in_host, in_total, hipMemcpyHostToDevice, s));
        if (timing) YDS_HIP(hipEventRecord(ev0, s));
        hipLaunchKernelGGL(act_update_kernel, dim3(n_wg), dim3(256), 0, s, reinterpret_cast<const ActWork *>(in_dev.p),
                           reinterpret_cast<const ActFrameDev *>(in_dev.p + works_b), acts.p, A, max_age, ms, res_host);
        YDS_HIP(hipGetLastError());
        if (timing) { YDS_HIP(hipEventRecord(ev1, s)); timed = true; }
    }

    void collect() override {
        const int n = pending_n;
        rows4.clear();
        first.assign(std::max(n, 0) + 1, 0);
        if (n <= 0) return;
        for (int i = 0; i < n; ++i) {
            const int m = res_host[i];
            if (m < 0 || m > pending_cap[i]) fail("actions: frame %d reports %d rows, %d possible", i, m, pending_cap[i]);
            const int *r = res_host + pending_rows[i];
            rows4.insert(rows4.end(), r, r + (size_t)m * 4);
            first[i + 1] = first[i] + m;
        }
        for (size_t k = 0; k < wg_stream.size(); ++k) count_host[wg_stream[k]] = res_host[n + k];
        pending_n = 0;
    }

    void reset(int stream) {
        if (stream < -1 || stream >= S) fail("actions: stream %d outside [-1,%d)", stream, S);
        for (int s = 0; s < S; ++s) {
            if (stream >= 0 && s != stream) continue;
            YDS_HIP(hipMemset(counts.p + s, 0, sizeof(int)));
            count_host[s] = 0;
        }
    }

    int S, A, max_age, ms;
    std::vector<Tab> tabs;
    std::vector<int> count_host;                  // entries of every stream after the last collected call
    DevBuf<ActDesc> acts;
    DevBuf<int> counts, srows;
    DevBuf<double> stime;
    DevBuf<char> in_dev;
    char *in_host = nullptr;
    int *res_host = nullptr;
    size_t in_cap = 0, res_cap = 0;
    int pending_n = 0;
    std::vector<int> order, wg_stream, pending_cap;
    std::vector<size_t> pending_rows;
    hipStream_t own_stream = nullptr;             // the stand-alone entry's
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing = false, timed = false;
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
    if (n_frames < 0) yds::fail("actions: %d frames", n_frames);
    if (n_out) *n_out = 0;
    if (!n_frames) return 0;
    if (!first || !stream_of) yds::fail("actions: NULL frame table");
    if (first[0] != 0) yds::fail("actions: first[0] = %d", first[0]);
    const int n_rows = first[n_frames];
    if (n_rows && (!rows6_host || !row_time)) yds::fail("actions: NULL rows");
    std::vector<yds::ActFrame> fr(n_frames);
    std::vector<int32_t> ids;
    for (int f = 0; f < n_frames; ++f) {
        const int r0 = first[f], r1 = first[f + 1];
        if (r1 < r0) yds::fail("actions: frame %d has first %d > %d", f, r0, r1);
        ids.clear();
        for (int r = r0; r < r1; ++r) ids.push_back(rows6_host[(size_t)r * 6 + 4]);
        std::sort(ids.begin(), ids.end());
        for (size_t k = 1; k < ids.size(); ++k)
            if (ids[k] == ids[k - 1]) yds::fail("actions: track id %d appears twice in frame %d", ids[k], f);
        fr[f] = yds::ActFrame{rows6_host + (size_t)r0 * 6, nullptr, r1 - r0, stream_of[f], f, 0.0, row_time + r0};
    }
    A->enqueue_ex(fr.data(), n_frames, A->own_stream, rows6_host, (size_t)n_rows, row_time, (size_t)n_rows);
    YDS_HIP(hipStreamSynchronize(A->own_stream));
    A->collect();
    const int m = (int)(A->rows4.size() / 4);
    if (n_out) *n_out = m;
    if (m > cap) yds::fail("actions: %d action rows exceed the caller's capacity %d", m, cap);
    if (m) memcpy(out4_host, A->rows4.data(), (size_t)m * 4 * sizeof(int32_t));
    YDS_API_END
}
int yds_actions_get_orbits(yds_act *a, int stream, int32_t *ids, int32_t *ages, int32_t *lens, int cap, int *n) {
    YDS_API_BEGIN
    yds::Actions *A = impl(a);
    if (stream < 0 || stream >= A->S) yds::fail("actions: stream %d outside [0,%d)", stream, A->S);
    const int m = A->count_host[stream];
    if (n) *n = m;
    if (m > cap) yds::fail("actions: %d orbits exceed the caller's capacity %d", m, cap);
    if (m) {
        const yds::ActTab t = A->dev_tab(stream);
        if (ids) YDS_HIP(hipMemcpy(ids, t.id, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
        if (ages) YDS_HIP(hipMemcpy(ages, t.age, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
        if (lens) YDS_HIP(hipMemcpy(lens, t.len, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    }
    YDS_API_END
}
int yds_actions_set_timing(yds_act *a, int on) {
    YDS_API_BEGIN
    impl(a)->timing = on != 0;
    impl(a)->timed = false;
    YDS_API_END
}
int yds_actions_last_us(yds_act *a, float *us) {
    YDS_API_BEGIN
    yds::Actions *A = impl(a);
    if (!A->timed) yds::fail("actions: no timed launch (yds_actions_set_timing, then a call)");
    float ms = 0;
    YDS_HIP(hipEventSynchronize(A->ev1));
    YDS_HIP(hipEventElapsedTime(&ms, A->ev0, A->ev1));
    *us = ms * 1e3f;
    YDS_API_END
}

}  // extern "C"
