// Anonymised output on the device: the mask rectangles of every frame of a batch (people, built by yolo_deepsort_amd/privacy.py
// mask_rects) are pixelated or filled over IN PLACE on packed 3-byte frames in HBM, before the overlay draws on them.  Pixel
// semantics are those of privacy.py anonymize(), bit for bit (tests/test_gpu_privacy.py compares the two):
//   pixelate: cells of m x m pixels anchored at the frame's origin (edge cells partial); per channel v = (2 S + cnt) / (2 cnt)
//             with S the sum of the ORIGINAL values of the whole cell; every pixel of (cell & union of rectangles) takes v
//   fill:     every pixel of the union takes the colour
// Both are independent of the order and overlap of the rectangles.
//
// Work follows the union.  The host clips the rectangles, marks the TILES they touch (a tile = k x k cells, k = max(1, 64 / m):
// at most 64 x 64 pixels, cell aligned) and hands the kernel the list of touched tiles: a frame without rectangles adds no tile and
// a call without tiles launches nothing.  One workgroup OWNS a tile, hence each of its cells: it collects the frame's rectangles
// that meet the tile in LDS (in chunks of 256: any count per frame), flags the cells they meet, reads every flagged cell
// COMPLETELY (an unflagged cell is not read), and only behind a barrier writes - which is what makes the in-place form safe when
// rectangles overlap.  Sums are integers (<= 64 * 64 * 255): row segments of <= 16 pixels per thread into LDS, then four lanes per
// cell add the segments and combine across lanes (__shfl_xor); no atomics touch a sum.
// Wide path (dword loads and stores): only when every address it forms is proved 4-aligned - the frame's base is, W % 4 == 0 (each
// row is then a multiple of 12 bytes) and m % 4 == 0 (each cell, segment and tile starts at a multiple of 4 pixels = 12 bytes).  A
// 33 x 50 frame, an odd slot of it, m = 2 or m = 3 take the byte path.
// Mixed layouts (frames of different sizes in one buffer, yds_anonymize_frames_mixed and the mixed overlay entries): a work item
// stays (frame, tile); the tile's geometry - tiles per row, edge tiles, the wide test - comes from that frame's row of the
// per-frame table (OutFrame), which the host fills from the frame's own H, W and address.
#include "anonymize_dev.h"

#include <algorithm>
#include <cmath>
#include <mutex>

#include "ydsort.h"

namespace yds {
namespace {

constexpr int kTile = 64;            // largest tile edge in pixels (k * m <= 64)
constexpr int kSeg = 16;             // pixels of one thread's row segment
constexpr int kCols = 32;            // segments per tile row: k * ceil(m / 16) <= 32 for every m in [2, 64]
constexpr int kCells = 32 * 32;      // cells per tile at m = 2
constexpr int kList = 256;           // rectangles per LDS chunk (= threads)

struct AnonArgs {
    uint8_t *frames;
    size_t frame_bytes;
    const int *slots;        // frame i lives in slot slots[i] (NULL: slot i)
    const int4 *rects;       // clipped: columns [x, z), rows [y, w)
    const int *rect_ptr;     // [n + 1]
    const int2 *work;        // (frame i, tile index ty * tiles_x + tx)
    int n_work, H, W, m, k, tiles_x, mode;
    uint32_t color;
    static constexpr bool kMixed = false;
};
// a mixed layout: frame i is geom[i] (its own offset, H, W, tiles_x, wide; frame_bytes, slots, H, W, tiles_x unused)
struct AnonArgsMixed : AnonArgs {
    const OutFrame *geom;
    static constexpr bool kMixed = true;
};

// One kernel text, two kernels: anonymize_kernel<AnonArgs> is the uniform kernel as it always was (one H, W, stride and tiles_x
// for every frame: nothing of the table exists in it); anonymize_kernel<AnonArgsMixed> reads the frame's row of the per-frame table.
template <class Args>
__global__ __launch_bounds__(256) void anonymize_kernel(Args a) {
    constexpr bool kMixed = Args::kMixed;
    __shared__ int4 list[kList];
    __shared__ int n_list;
    __shared__ uint8_t flag[kCells];              // per cell: 0 = meets no rectangle, 1 = partly covered, 2 = inside one rectangle
    __shared__ ushort4 part[kTile * kCols];       // per (tile row, segment): channel sums (<= 16 * 255)
    __shared__ uint32_t cellv[kCells];            // per cell: v0 | v1 << 8 | v2 << 16
    const int tid = threadIdx.x, m = a.m, k = a.k, T = m * k, Hu = a.H, Wu = a.W;
    const int nseg = (m + kSeg - 1) / kSeg;
    for (int wi = blockIdx.x; wi < a.n_work; wi += gridDim.x) {
        const int2 wk = a.work[wi];
        // the frame of this work item: one size and stride for all (a uniform call), or its own row of the table (a mixed layout)
        const OutFrame *g = nullptr;
        if constexpr (kMixed) g = a.geom + wk.x;
        const int H = kMixed ? g->H : Hu, W = kMixed ? g->W : Wu, tiles_x = kMixed ? g->tiles_x : a.tiles_x;
        const int f = wk.x, x0 = (wk.y % tiles_x) * T, y0 = (wk.y / tiles_x) * T;
        const int tw = min(T, W - x0), th = min(T, H - y0);                 // the tile's pixels (edge tiles are partial)
        const int kx = (tw + m - 1) / m, ky = (th + m - 1) / m;             // ... and cells
        uint8_t *img = kMixed ? a.frames + g->off : a.frames + (size_t)(a.slots ? a.slots[f] : f) * a.frame_bytes;
        const int r_lo = a.rect_ptr[f], r_hi = a.rect_ptr[f + 1];
        const bool one_chunk = r_hi - r_lo <= kList;
        const bool wide = m % 4 == 0 && (kMixed ? g->wide != 0 : W % 4 == 0 && (reinterpret_cast<uintptr_t>(img) & 3) == 0);
        // rectangles [c0, c0 + 256) of the frame that meet the tile -> list[0, n_list)
        auto gather = [&](int c0) {
            __syncthreads();                                                // everyone is done with the previous list
            if (tid == 0) n_list = 0;
            __syncthreads();
            if (c0 + tid < r_hi) {
                const int4 r = a.rects[c0 + tid];
                if (r.x < x0 + tw && r.z > x0 && r.y < y0 + th && r.w > y0) list[atomicAdd(&n_list, 1)] = r;     // (a slot counter, not a sum)
            }
            __syncthreads();
        };
        for (int c = tid; c < kCells; c += blockDim.x) flag[c] = 0;
        for (int c0 = r_lo; c0 < r_hi; c0 += kList) {
            gather(c0);
            const int nl = n_list;
            for (int c = tid; c < ky * kx; c += blockDim.x) {
                const int cy = c / kx, cx = c % kx;
                const int xa = x0 + cx * m, xb = min(xa + m, W), ya = y0 + cy * m, yb = min(ya + m, H);
                int fl = flag[cy * k + cx];
                for (int j = 0; j < nl; ++j) {
                    const int4 r = list[j];
                    if (r.x < xb && r.z > xa && r.y < yb && r.w > ya)
                        fl = max(fl, (r.x <= xa && r.z >= xb && r.y <= ya && r.w >= yb) ? 2 : 1);
                }
                flag[cy * k + cx] = (uint8_t)fl;
            }
        }
        __syncthreads();
        if (a.mode == MASK_PIXELATE) {
            // 1: one thread per (row, segment) of a flagged cell
            const int ncol = k * nseg;
            for (int it = tid; it < th * ncol; it += blockDim.x) {
                const int r = it / ncol, c = it % ncol, cx = c / nseg, cy = r / m;
                if (cx >= kx || !flag[cy * k + cx]) continue;
                const int xc = x0 + cx * m, xs = xc + (c % nseg) * kSeg, xe = min(min(xs + kSeg, xc + m), W);
                unsigned s0 = 0, s1 = 0, s2 = 0;
                if (xs < xe) {
                    const uint8_t *p = img + ((size_t)(y0 + r) * W + xs) * 3;
                    if (wide) {                                             // xs, xe multiples of 4 pixels: whole dwords, 4-aligned
                        const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
                        for (int j = 0; j < (xe - xs) / 4; ++j) {
                            const uint32_t w0 = q[3 * j], w1 = q[3 * j + 1], w2 = q[3 * j + 2];
                            // bytes: w0 = c0 c1 c2 d0 | w1 = d1 d2 e0 e1 | w2 = e2 f0 f1 f2   (pixels c d e f, channel 0..2)
                            s0 += (w0 & 0xff) + (w0 >> 24) + ((w1 >> 16) & 0xff) + ((w2 >> 8) & 0xff);
                            s1 += ((w0 >> 8) & 0xff) + (w1 & 0xff) + (w1 >> 24) + ((w2 >> 16) & 0xff);
                            s2 += ((w0 >> 16) & 0xff) + ((w1 >> 8) & 0xff) + (w2 & 0xff) + (w2 >> 24);
                        }
                    } else {
                        for (int x = xs; x < xe; ++x, p += 3) { s0 += p[0]; s1 += p[1]; s2 += p[2]; }
                    }
                }
                part[r * kCols + c] = make_ushort4((unsigned short)s0, (unsigned short)s1, (unsigned short)s2, 0);
            }
            __syncthreads();
            // 2: four adjacent lanes per cell add its rows' segments, then combine across lanes
            const int items = ky * kx * 4;
            for (int base = 0; base < items; base += blockDim.x) {
                const int it = base + tid, cell = it >> 2, cy = cell / kx, cx = cell % kx;
                const bool live = it < items && flag[cy * k + cx];
                const int ch = min(m, th - cy * m), cw = min(m, tw - cx * m);
                unsigned s0 = 0, s1 = 0, s2 = 0;
                if (live)
                    for (int r = it & 3; r < ch; r += 4)
                        for (int s = 0; s < nseg; ++s) {
                            const ushort4 v = part[(cy * m + r) * kCols + cx * nseg + s];
                            s0 += v.x; s1 += v.y; s2 += v.z;
                        }
                s0 += __shfl_xor(s0, 1); s1 += __shfl_xor(s1, 1); s2 += __shfl_xor(s2, 1);
                s0 += __shfl_xor(s0, 2); s1 += __shfl_xor(s1, 2); s2 += __shfl_xor(s2, 2);
                if (live && (it & 3) == 0) {
                    const unsigned cnt = (unsigned)(cw * ch);
                    cellv[cy * k + cx] = (2 * s0 + cnt) / (2 * cnt) | ((2 * s1 + cnt) / (2 * cnt)) << 8 | ((2 * s2 + cnt) / (2 * cnt)) << 16;
                }
            }
            __syncthreads();                                                // every flagged cell has been read: writes may start
        }
        // 3: write.  One chunk: the list of the flag pass still stands.  More: each chunk's rectangles in turn (a pixel covered by
        // two chunks is written twice with the same value); cells inside one rectangle are written once, with the first chunk.
        for (int c0 = r_lo; c0 < r_hi; c0 += kList) {
            if (!one_chunk) gather(c0);
            const int nl = n_list;
            const bool first = c0 == r_lo;
            if (wide) {                                                     // one thread per 4 pixels = 3 dwords (inside one cell: m % 4 == 0)
                const int qw = tw / 4;
                for (int it = tid; it < th * qw; it += blockDim.x) {
                    const int r = it / qw, q = it % qw, x = x0 + q * 4, y = y0 + r, cell = (r / m) * k + (q * 4) / m;
                    const int fl = flag[cell];
                    if (!fl) continue;
                    unsigned cov = 0;
                    if (fl == 2) cov = first ? 15u : 0u;
                    else
                        for (int j = 0; j < nl; ++j) {
                            const int4 rc = list[j];
                            if (y >= rc.y && y < rc.w)
                                for (int e = 0; e < 4; ++e) cov |= (unsigned)(x + e >= rc.x && x + e < rc.z) << e;
                        }
                    if (!cov) continue;
                    const uint32_t v = a.mode == MASK_FILL ? a.color : cellv[cell];
                    const uint32_t b0 = v & 0xff, b1 = (v >> 8) & 0xff, b2 = (v >> 16) & 0xff;
                    uint8_t *p = img + ((size_t)y * W + x) * 3;
                    if (cov == 15u) {
                        uint32_t *d = reinterpret_cast<uint32_t *>(p);
                        d[0] = b0 | b1 << 8 | b2 << 16 | b0 << 24;
                        d[1] = b1 | b2 << 8 | b0 << 16 | b1 << 24;
                        d[2] = b2 | b0 << 8 | b1 << 16 | b2 << 24;
                    } else {
                        for (int e = 0; e < 4; ++e)
                            if (cov >> e & 1) { p[3 * e] = (uint8_t)b0; p[3 * e + 1] = (uint8_t)b1; p[3 * e + 2] = (uint8_t)b2; }
                    }
                }
            } else {                                                        // one thread per pixel, three byte stores
                for (int it = tid; it < th * tw; it += blockDim.x) {
                    const int r = it / tw, c = it % tw, x = x0 + c, y = y0 + r, cell = (r / m) * k + c / m;
                    const int fl = flag[cell];
                    if (!fl) continue;
                    bool cov = false;
                    if (fl == 2) cov = first;
                    else
                        for (int j = 0; j < nl; ++j) {
                            const int4 rc = list[j];
                            cov |= x >= rc.x && x < rc.z && y >= rc.y && y < rc.w;
                        }
                    if (!cov) continue;
                    const uint32_t v = a.mode == MASK_FILL ? a.color : cellv[cell];
                    uint8_t *p = img + ((size_t)y * W + x) * 3;
                    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16);
                }
            }
        }
        __syncthreads();                                                    // the next tile resets the flags
    }
}

// the mask alone (yds_anonymize_frames): its own stream and scratch, one call at a time
struct AnonState {
    std::mutex mu;
    hipStream_t stream = nullptr;
    Anonymizer anon;
    DevBuf<int> slots;
    MixedLayout layout;                  // yds_anonymize_frames_mixed: the table of the call, host and device
    DevBuf<OutFrame> geom;
    AnonState() { YDS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)); }
};
AnonState &anon_state() {
    static AnonState s;
    return s;
}

}  // namespace

int Anonymizer::prepare(int n, int h, int w, const MaskSpec &mk, const int32_t *hw) {
    if (mk.mode != MASK_PIXELATE && mk.mode != MASK_FILL) fail("anonymize: mode %d (1 = pixelate, 2 = fill)", mk.mode);
    if (mk.mode == MASK_PIXELATE && (mk.block < 2 || mk.block > 64)) fail("anonymize: block %d outside [2, 64]", mk.block);
    if (n < 1 || (!hw && (h < 1 || w < 1))) fail("anonymize: bad geometry (n %d, h %d, w %d)", n, h, w);
    for (int i = 0; hw && i < n; ++i)
        if (hw[2 * i] < 1 || hw[2 * i + 1] < 1) fail("anonymize: bad geometry (frame %d: h %d, w %d)", i, hw[2 * i], hw[2 * i + 1]);
    if (!mk.rect_ptr_host) fail("anonymize: NULL rectangle table");
    if (mk.rect_ptr_host[0] < 0) fail("anonymize: bad rectangle table");
    for (int i = 0; i < n; ++i)
        if (mk.rect_ptr_host[i + 1] < mk.rect_ptr_host[i]) fail("anonymize: rect_ptr decreases at frame %d", i);
    if (mk.rect_ptr_host[n] > mk.rect_ptr_host[0] && !mk.rects_host) fail("anonymize: NULL rectangle table");
    // fill has no cells of its own: it takes the tiling (and the wide path) of m = 16
    m = mk.mode == MASK_FILL ? 16 : mk.block;
    k = std::max(1, kTile / m);
    mode = mk.mode; color = mk.color & 0xffffffu; H = hw ? 0 : h; W = hw ? 0 : w;
    const int T = m * k;
    tiles_x = hw ? 0 : (w + T - 1) / T;
    h_rects.clear(); h_work.clear(); h_tiles_x.clear();
    h_ptr.assign(1, 0);
    std::vector<char> touched;
    for (int i = 0; i < n; ++i) {
        const int fh = hw ? hw[2 * i] : h, fw = hw ? hw[2 * i + 1] : w;     // the frame's own size: its clip, its tiles
        const int ftx = (fw + T - 1) / T, fty = (fh + T - 1) / T;
        if (hw) h_tiles_x.push_back(ftx);
        bool any = false;
        for (int j = mk.rect_ptr_host[i]; j < mk.rect_ptr_host[i + 1]; ++j) {
            const int32_t *r = mk.rects_host + (size_t)j * 4;
            // the filled rectangle() of label_draw.py: rows [max(ya,0), min(yb+1,H)), columns [max(xa,0), min(xb+1,W))
            const int64_t x0 = std::max<int64_t>(r[0], 0), y0 = std::max<int64_t>(r[1], 0);
            const int64_t x1 = std::min<int64_t>((int64_t)r[2] + 1, fw), y1 = std::min<int64_t>((int64_t)r[3] + 1, fh);
            if (x1 <= x0 || y1 <= y0) continue;
            if (!any) { touched.assign((size_t)ftx * fty, 0); any = true; }
            h_rects.insert(h_rects.end(), {(int)x0, (int)y0, (int)x1, (int)y1});
            for (int ty = (int)y0 / T; ty <= (int)(y1 - 1) / T; ++ty)
                for (int tx = (int)x0 / T; tx <= (int)(x1 - 1) / T; ++tx) touched[(size_t)ty * ftx + tx] = 1;
        }
        h_ptr.push_back((int)(h_rects.size() / 4));
        if (any)
            for (int t = 0; t < ftx * fty; ++t)
                if (touched[t]) { h_work.push_back(i); h_work.push_back(t); }
    }
    return (int)(h_work.size() / 2);
}

void Anonymizer::launch(hipStream_t s, uint8_t *frames, size_t frame_bytes, const int *slots_dev, const OutFrame *geom_dev) {
    const int n_work = (int)(h_work.size() / 2);
    if (!n_work) return;
    rects.upload(h_rects.data(), h_rects.size(), s);
    rect_ptr.upload(h_ptr.data(), h_ptr.size(), s);
    work.upload(h_work.data(), h_work.size(), s);
    const AnonArgs a{frames, frame_bytes, slots_dev, reinterpret_cast<const int4 *>(rects.p), rect_ptr.p, reinterpret_cast<const int2 *>(work.p),
                     n_work, H, W, m, k, tiles_x, mode, color};
    if (geom_dev) {
        AnonArgsMixed am;
        static_cast<AnonArgs &>(am) = a;
        am.geom = geom_dev;
        anonymize_kernel<AnonArgsMixed><<<std::min(n_work, 1 << 16), 256, 0, s>>>(am);
    } else {
        anonymize_kernel<AnonArgs><<<std::min(n_work, 1 << 16), 256, 0, s>>>(a);      // (a workgroup walks the list in strides of the grid)
    }
    YDS_HIP(hipGetLastError());
}

void MixedLayout::build(const char *who, const void *work_base, size_t frames_bytes, int n_src, const uint64_t *frame_off, const int32_t *frame_hw,
                        const int32_t *slots, int n, bool in_place) {
    if (!frame_off || !frame_hw || !slots || n_src < 1) fail("%s: NULL layout (%d staged frames)", who, n_src);
    std::vector<uint64_t> bytes((size_t)n_src);
    for (int j = 0; j < n_src; ++j) {
        const int h = frame_hw[2 * j], w = frame_hw[2 * j + 1];
        if (h < 1 || w < 1) fail("%s: staged frame %d is %d x %d", who, j, h, w);
        bytes[j] = (uint64_t)h * (uint64_t)w * 3;                          // < 2^64 for any int h, w
        if (frame_off[j] > frames_bytes || bytes[j] > frames_bytes - frame_off[j])
            fail("%s: staged frame %d (%d x %d at byte %llu) ends past the buffer of %zu bytes", who, j, h, w, (unsigned long long)frame_off[j], frames_bytes);
    }
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= n_src) fail("%s: frame %d names slot %d of %d staged frames", who, i, slots[i], n_src);
    if (in_place) {
        std::vector<int> order((size_t)n_src);
        for (int j = 0; j < n_src; ++j) order[j] = j;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return frame_off[a] < frame_off[b]; });
        for (int j = 1; j < n_src; ++j)
            if (frame_off[order[j - 1]] + bytes[order[j - 1]] > frame_off[order[j]])
                fail("%s: staged frames %d and %d overlap", who, order[j - 1], order[j]);
        std::vector<char> named((size_t)n_src, 0);
        for (int i = 0; i < n; ++i) {
            if (named[slots[i]]) fail("%s: slot %d is named twice (frame %d)", who, slots[i], i);
            named[slots[i]] = 1;
        }
    }
    rows.assign((size_t)n, OutFrame{});
    hw.resize((size_t)n * 2);
    src_off.resize((size_t)n);
    packed_bytes = 0;
    for (int i = 0; i < n; ++i) {
        const int j = slots[i], h = frame_hw[2 * j], w = frame_hw[2 * j + 1];
        OutFrame &r = rows[i];
        r.off = in_place ? frame_off[j] : (uint64_t)packed_bytes;
        r.H = h; r.W = w;
        r.scale = std::max(1, (int)std::nearbyint(2 * (h / 1000.)));      // label_draw.py: max(1, int(round(2 * (h / 1000.)))), ties to even
        r.tiles_x = 0;
        r.wide = w % 4 == 0 && ((reinterpret_cast<uintptr_t>(work_base) + r.off) & 3) == 0;
        hw[2 * i] = h; hw[2 * i + 1] = w;
        src_off[i] = frame_off[j];
        packed_bytes += (size_t)bytes[j];
    }
}

}  // namespace yds

extern "C" {

int yds_anonymize_frames_mixed(uint8_t *frames_dev, size_t frames_bytes, int n_src, const uint64_t *frame_off_host, const int32_t *frame_hw_host,
                               const int32_t *slot_host, int n, const int32_t *rects_host, const int32_t *rect_ptr_host, int mode, int block,
                               uint32_t color) {
    YDS_API_BEGIN
    if (n <= 0) return 0;
    if (!frames_dev) yds::fail("anonymize: NULL argument");
    yds::AnonState &s = yds::anon_state();
    std::lock_guard<std::mutex> lock(s.mu);                                 // held until the stream has drained: the scratch is shared
    s.layout.build("anonymize", frames_dev, frames_bytes, n_src, frame_off_host, frame_hw_host, slot_host, n, true);
    yds::MaskSpec mk;
    mk.rects_host = rects_host; mk.rect_ptr_host = rect_ptr_host; mk.mode = mode; mk.block = block; mk.color = color;
    if (!s.anon.prepare(n, 0, 0, mk, s.layout.hw.data())) return 0;         // no rectangle touches a frame: nothing is enqueued
    s.layout.set_tiles(s.anon.h_tiles_x);
    s.geom.upload(s.layout.rows.data(), s.layout.rows.size(), s.stream);
    s.anon.launch(s.stream, frames_dev, 0, nullptr, s.geom.p);
    YDS_HIP(hipStreamSynchronize(s.stream));
    YDS_API_END
}

int yds_anonymize_frames(uint8_t *frames_dev, int n_src, const int32_t *slot_host, int n, int h, int w, const int32_t *rects_host,
                         const int32_t *rect_ptr_host, int mode, int block, uint32_t color) {
    YDS_API_BEGIN
    if (n <= 0) return 0;
    if (!frames_dev || !slot_host || n_src < 1) yds::fail("anonymize: NULL argument");
    for (int i = 0; i < n; ++i) {
        if (slot_host[i] < 0 || slot_host[i] >= n_src) yds::fail("anonymize: frame %d names slot %d of %d frames", i, slot_host[i], n_src);
        for (int j = 0; j < i; ++j)
            if (slot_host[i] == slot_host[j]) yds::fail("anonymize: frames %d and %d name the same slot %d", j, i, slot_host[i]);
    }
    yds::AnonState &s = yds::anon_state();
    std::lock_guard<std::mutex> lock(s.mu);                                 // held until the stream has drained: the scratch is shared
    yds::MaskSpec mk;
    mk.rects_host = rects_host; mk.rect_ptr_host = rect_ptr_host; mk.mode = mode; mk.block = block; mk.color = color;
    if (!s.anon.prepare(n, h, w, mk)) return 0;                             // no rectangle touches a frame: nothing is enqueued
    s.slots.upload(slot_host, (size_t)n, s.stream);
    s.anon.launch(s.stream, frames_dev, (size_t)h * w * 3, s.slots.p);
    YDS_HIP(hipStreamSynchronize(s.stream));
    YDS_API_END
}

}  // extern "C"
