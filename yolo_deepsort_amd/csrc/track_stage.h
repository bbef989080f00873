// The frame the per-stream table stages share (actions.hip: orbit caches, zones.hip: zone and line state, heatmap.hip: last cells,
// ground.hip: plan positions).  Such a stage keeps one
// table of tracks per video stream in HBM, keyed by track id, every field twice (the second copy takes the survivors of a removal).
// One launch per call advances all tables: a 256-thread workgroup per stream that has frames in the call walks that stream's frames
// in time order, and what it reports goes straight into a pinned block that the host reads after the step's one synchronisation.
//   device half: what a workgroup does to a table whatever it holds - stage a frame's rows, find a row by id, register unknown ids,
//                retire entries - with the fields left to functors
//   host half:   TrackStage, the bookkeeping that does not depend on what a table holds - frames bucketed by stream, table growth,
//                the input / result blocks, the counts that come back - and the front of the stand-alone C entries
// A stage adds its device structs, its kernel, its table layout and its result layout.
// Above this frame a stage is a slot of a step (engine.h: StageSlot, TrackStageIface, StageReport; pipeline.cpp: set_stage) and, in
// Python, a subclass of the front that mirrors this header: yolo_deepsort_amd/track_stage.py (handle, frame table of a call, table
// read, reset / timing / close).
#pragma once
#include "tracker_dev.h"

#include <limits.h>

namespace yds {

// ---------------------------------------------------------------------------------------------------------------- device half
// (for a 256-thread workgroup; s_cnt: LDS int[4]; rows are [6] int32 = x1, y1, x2, y2, track id, class)

// exclusive prefix of v over the 256 threads of the workgroup; chunk = the sum (to every thread)
__device__ __forceinline__ int block_prefix(int v, int *s_cnt, int &chunk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_cnt[wave] = x;
    __syncthreads();
    int woff = 0;
    chunk = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int c = s_cnt[w]; if (w < wave) woff += c; chunk += c; }
    __syncthreads();
    return woff + x - v;
}

// Copies a frame's rows into the workgroup's staging area (they may sit in pinned host memory: a tracker result block) and returns
// how many there are: *n_p clamped to [0, n] where the count is on the device, else n.  The caller places the barrier.
__device__ __forceinline__ int stage_frame_rows(const int *rows, const int *n_p, int n, int *srows) {
    const int R = n_p ? min(max(*n_p, 0), n) : n;
    for (int k = threadIdx.x; k < R * 6; k += 256) srows[k] = rows[k];
    return R;
}

// the staged row that carries track id `id`; R when there is none
__device__ __forceinline__ int find_row(const int *srows, int R, int id) {
    int j = 0;
    while (j < R && srows[j * 6 + 4] != id) ++j;
    return j;
}

// Rows whose id is not among ids[0, n) become entries n, n + 1, ... in row order: init(e, row) fills entry e from its row.
// Returns the entry count afterwards.
template <class Init> __device__ __forceinline__ int register_unknown(int R, int n, int cap, int *s_cnt, const int *ids, const int *srows, Init init) {
    const int added = compact_ordered(R, s_cnt, [&](int j) {
        const int id = srows[j * 6 + 4];
        for (int e = 0; e < n; ++e) if (ids[e] == id) return false;
        return true;
    }, [&](int j, int r) {
        const int e = n + r;
        if (e >= cap) return;                                                     // (the host sized the table for every row of the call)
        init(e, srows + j * 6);
    });
    return min(n + added, cap);
}

// Entries of [0, n_all) that keep(e) holds stay, in their order: move(cap + rank, e) takes a whole entry to the table's second
// half, then back(e, cap + e) brings home the fields that are one value per entry, a thread per entry.  Returns the number of
// survivors.  Fields that are an array per entry come home by a strided bulk copy of the caller's, which then places the barrier.
template <class Keep, class Move, class Back> __device__ __forceinline__ int retire(int n_all, int cap, int *s_cnt, Keep keep, Move move, Back back) {
    const int n_live = compact_ordered(n_all, s_cnt, keep, [&](int e, int r) { move(cap + r, e); });
    __syncthreads();
    for (int e = threadIdx.x; e < n_live; e += 256) back(e, cap + e);
    return n_live;
}

// ------------------------------------------------------------------------------------------------------------------ host half
// device time of one launch, for the tools (yds_*_set_timing / yds_*_last_us)
struct LaunchTimer {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool on = false, timed = false;
    LaunchTimer() { YDS_HIP(hipEventCreate(&ev0)); YDS_HIP(hipEventCreate(&ev1)); }
    LaunchTimer(const LaunchTimer &) = delete;
    ~LaunchTimer() { (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1); }
    void set(bool v) { on = v; timed = false; }
    void begin(hipStream_t s) { if (on) YDS_HIP(hipEventRecord(ev0, s)); }
    void end(hipStream_t s) { if (on) { YDS_HIP(hipEventRecord(ev1, s)); timed = true; } }
    float us(const char *what) {
        if (!timed) fail("%s: no timed launch (yds_%s_set_timing, then a call)", what, what);
        float ms = 0;
        YDS_HIP(hipEventSynchronize(ev1));
        YDS_HIP(hipEventElapsedTime(&ms, ev0, ev1));
        return ms * 1e3f;
    }
};

// Room for `need` entries in table t (a struct of DevBufs with a `cap`), of which n are live: capacities double from 64; alloc(nt)
// allocates a table of nt.cap entries, copy(nt, t) takes the live entries over.  Nothing of a stage is in flight between calls
// (every call ends behind a synchronisation).
template <class Tab, class Alloc, class Copy> void grow_table(Tab &t, int need, int n, Alloc alloc, Copy copy) {
    if (need <= t.cap) return;
    Tab nt;
    nt.cap = std::max(t.cap, 64);
    while (nt.cap < need) nt.cap *= 2;
    alloc(nt);
    if (n) copy(nt, t);
    t = std::move(nt);
}
// the first n values of src to dst; of each column where the buffers hold `fields` columns [2][cap] (capacities c and c0)
template <class T> void copy_live(DevBuf<T> &dst, const DevBuf<T> &src, size_t n, int fields = 1, int c = 0, int c0 = 0) {
    for (int f = 0; f < fields; ++f)
        YDS_HIP(hipMemcpy(dst.p + (size_t)f * 2 * c, src.p + (size_t)f * 2 * c0, n * sizeof(T), hipMemcpyDeviceToDevice));
}

// The frames of a call by stream, order kept: workgroup k takes stream wg_stream[k], stream st's frames are slots
// [start[st], start[st] + n_of[st]) of the sorted list, order[slot] = frame of the call.
struct StagePlan {
    int n_wg = 0, max_rows = 1;
    std::vector<int> n_of, start, order;
};

// Iface: the stage's interface in engine.h (a TrackStageIface).  name: the prefix of its error texts.
template <class Iface> class TrackStage : public Iface {
public:
    TrackStage(const char *name, int S) : name(name), S(S), count_host(S, 0) {
        if (S < 1) fail("%s: %d streams", name, S);
        counts.alloc(S);
        YDS_HIP(hipMemset(counts.p, 0, S * sizeof(int)));
        own_stream = make_stream(true);
    }
    ~TrackStage() override { if (own_stream) (void)hipStreamDestroy(own_stream); }
    int streams() const override { return S; }

    void check_stream(int stream, int lo = 0) const {
        if (stream < lo || stream >= S) fail("%s: stream %d outside [%d,%d)", name, stream, lo, S);
    }
    // empties the table of one stream, or of all (-1)
    void reset(int stream) {
        check_stream(stream, -1);
        for (int s = 0; s < S; ++s) {
            if (stream >= 0 && s != stream) continue;
            YDS_HIP(hipMemset(counts.p + s, 0, sizeof(int)));
            count_host[s] = 0;
        }
    }

    // Opens a call: checks its frames and buckets them; grow(st, need) makes room in stream st's table for every row the call brings
    // it.  A call without frames has no workgroups: nothing to launch.
    template <class Grow> StagePlan plan(const ActFrame *fr, int n, Grow grow) {
        StagePlan p;
        pending_n = n;
        if (n <= 0) return p;
        std::vector<int> rows_of(S, 0);
        p.n_of.assign(S, 0);
        for (int i = 0; i < n; ++i) {
            if (fr[i].stream < 0 || fr[i].stream >= S) fail("%s: frame %d names stream %d outside [0,%d)", name, i, fr[i].stream, S);
            if (fr[i].n_rows < 0) fail("%s: frame %d has %d rows", name, i, fr[i].n_rows);
            ++p.n_of[fr[i].stream];
            rows_of[fr[i].stream] += fr[i].n_rows;
            p.max_rows = std::max(p.max_rows, fr[i].n_rows);
        }
        p.start.assign(S, 0);
        wg_stream.clear();
        int acc = 0;
        for (int st = 0; st < S; ++st) {
            if (!p.n_of[st]) continue;
            wg_stream.push_back(st);
            p.start[st] = acc;
            acc += p.n_of[st];
            grow(st, count_host[st] + rows_of[st]);
        }
        p.n_wg = (int)wg_stream.size();
        p.order.assign(n, 0);
        std::vector<int> fill(p.start);
        for (int i = 0; i < n; ++i) p.order[fill[fr[i].stream]++] = i;
        return p;
    }

    // Room for the blocks of a call.  Input: `head` bytes of the stage's own (works | frames | ..., 8-byte aligned pieces), then the
    // rows of the stand-alone entry: rows_host is a host array that travels to the device inside the block; the frames' rows6 then
    // point INTO that array and dev_rows translates them.  Result: res_total ints, of which [0, n) are the frames' counts and
    // [n, n + n_wg) the tables' entry counts.  Staging: max_rows rows per workgroup.
    void open_blocks(const StagePlan &p, size_t head, const int32_t *rows_host, size_t n_rows_host, size_t res_total) {
        if (res_total > (size_t)INT_MAX) fail("%s: result block of %zu ints", name, res_total);
        in_total = head + n_rows_host * 6 * sizeof(int32_t);
        if (in_total > in_host.n) { in_host.ensure(in_total * 2); in_dev.alloc(in_host.n); }
        if (res_total > res_host.n) res_host.ensure(res_total * 2);
        srows_ld = (size_t)p.max_rows * 6;
        if (p.n_wg * srows_ld > srows.n) srows.alloc(p.n_wg * srows_ld * 2);
        if (n_rows_host) memcpy(in_host.p + head, rows_host, n_rows_host * 6 * sizeof(int32_t));
        rows_src = rows_host;
        rows_dev = reinterpret_cast<const int32_t *>(in_dev.p + head);
    }
    const int32_t *dev_rows(const ActFrame &f) const { return rows_src ? rows_dev + (f.rows6 - rows_src) : f.rows6; }
    int *wg_srows(int k) const { return srows.p + k * srows_ld; }

    // the input block goes up and launch() issues the stage's one kernel behind it, timed when asked for
    template <class Launch> void submit(hipStream_t s, Launch launch) {
        YDS_HIP(hipMemcpyAsync(in_dev.p, in_host.p, in_total, hipMemcpyHostToDevice, s));
        timer.begin(s);
        launch();
        YDS_HIP(hipGetLastError());
        timer.end(s);
    }

    // After the synchronisation: frame i reported m of `noun` (rows, events): append(i, m) takes them; first[] and the tables' entry
    // counts follow.
    template <class Append> void collect_counts(const char *noun, Append append) {
        const int n = pending_n;
        this->first.assign(std::max(n, 0) + 1, 0);
        if (n <= 0) return;
        for (int i = 0; i < n; ++i) {
            const int m = res_host.p[i];
            if (m < 0 || m > pending_cap[i]) fail("%s: frame %d reports %d %s, %d possible", name, i, m, noun, pending_cap[i]);
            append(i, m);
            this->first[i + 1] = this->first[i] + m;
        }
        for (size_t k = 0; k < wg_stream.size(); ++k) count_host[wg_stream[k]] = res_host.p[n + k];
        pending_n = 0;
    }
    // the stand-alone entries: the call that was enqueued on own_stream, to its end
    void finish_alone() {
        YDS_HIP(hipStreamSynchronize(own_stream));
        this->collect();
    }
    // m of `noun` for a caller with room for cap: *n = m, refused when they do not fit
    int give_count(const char *noun, int m, int cap, int *n) const {
        if (n) *n = m;
        if (m > cap) fail("%s: %d %s exceed the caller's capacity %d", name, m, noun, cap);
        return m;
    }
    // the getters: the entry count of a stream's table, then its columns
    int table_count(int stream, const char *noun, int cap, int *n) const {
        check_stream(stream);
        return give_count(noun, count_host[stream], cap, n);
    }
    static void column_out(int32_t *dst, const void *col, int m) {
        if (dst && m) YDS_HIP(hipMemcpy(dst, col, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    }

    const char *name;
    int S;
    std::vector<int> count_host;                  // entries of every stream after the last collected call
    DevBuf<int> counts, srows;                    // live entries of every stream (device); staging [n_wg][max rows of a frame][6]
    DevBuf<char> in_dev;
    PinBuf<char> in_host;
    PinBuf<int> res_host;
    size_t in_total = 0, srows_ld = 0;
    const int32_t *rows_src = nullptr, *rows_dev = nullptr;
    int pending_n = 0;
    std::vector<int> wg_stream, pending_cap;      // of the call in flight: the stream of every workgroup, the most every frame can report
    hipStream_t own_stream = nullptr;             // the stand-alone entry's
    LaunchTimer timer;
};

// The front of the stand-alone update entries: checks the CSR frame table of a call (frame f = rows [first[f], first[f + 1]) of
// rows6, no track id twice in a frame) and returns its frames, tagged with their index.  time: per_row ? a time per row : a time per
// frame.  No frames: empty.
inline std::vector<ActFrame> csr_frames(const char *what, const int32_t *rows6, const int32_t *first, const int32_t *stream_of, const double *time,
                                        bool per_row, int n_frames, int *n_out) {
    if (n_frames < 0) fail("%s: %d frames", what, n_frames);
    if (n_out) *n_out = 0;
    std::vector<ActFrame> fr(n_frames);
    if (!n_frames) return fr;
    if (!first || !stream_of || (!per_row && !time)) fail("%s: NULL frame table", what);
    if (first[0] != 0) fail("%s: first[0] = %d", what, first[0]);
    if (first[n_frames] && (!rows6 || (per_row && !time))) fail("%s: NULL rows", what);
    std::vector<int32_t> ids;
    for (int f = 0; f < n_frames; ++f) {
        const int r0 = first[f], r1 = first[f + 1];
        if (r1 < r0) fail("%s: frame %d has first %d > %d", what, f, r0, r1);
        ids.clear();
        for (int r = r0; r < r1; ++r) ids.push_back(rows6[(size_t)r * 6 + 4]);
        std::sort(ids.begin(), ids.end());
        for (size_t k = 1; k < ids.size(); ++k)
            if (ids[k] == ids[k - 1]) fail("%s: track id %d appears twice in frame %d", what, ids[k], f);
        fr[f] = ActFrame{rows6 + (size_t)r0 * 6, nullptr, r1 - r0, stream_of[f], f, per_row ? 0.0 : time[f], per_row ? time + r0 : nullptr};
    }
    return fr;
}

}  // namespace yds
