// The anonymising pass of the output stage (anonymize.hip): mask tables of the C ABI -> one launch on the caller's stream.
#pragma once
#include "common.h"

namespace yds {

enum MaskMode { MASK_NONE = 0, MASK_PIXELATE = 1, MASK_FILL = 2 };

// what the C entries take: rects_host [total][4] = xa, ya, xb, yb (inclusive corners, unclipped), rect_ptr_host [n + 1] (CSR over
// the frames of the call), colour = the three bytes as they land in memory, byte 0 lowest
struct MaskSpec {
    const int32_t *rects_host = nullptr, *rect_ptr_host = nullptr;
    int mode = MASK_NONE, block = 16;
    uint32_t color = 0;
};

// One frame of a mixed layout as the output-stage kernels see it (overlay.hip's draw, anonymize.hip's mask): the frame a work
// item names lives at base + off with its own size; scale = the label font's pixels per dot; tiles_x and wide belong to the mask
// (tiles per row at the call's tile edge; base + off is 4-aligned and W % 4 == 0, so dword accesses are legal for cells of m % 4 == 0).
struct OutFrame {
    uint64_t off;
    int H, W, scale, tiles_x, wide, pad;
};

// Host half of a mixed layout (the *_mixed entries): checks what the caller handed in - fail() before anything is enqueued - and
// builds the table of the n frames the call works on, in the caller's order.
struct MixedLayout {
    std::vector<OutFrame> rows;        // per frame of the call; tiles_x is filled by set_tiles() once the mask is prepared
    std::vector<int32_t> hw;           // [n][2]: h, w of the frames of the call (Anonymizer::prepare takes it)
    std::vector<uint64_t> src_off;     // [n]: offset of the staged frame each one names
    size_t packed_bytes = 0;           // sum of 3 h w over the frames of the call
    // staged frame j = [frame_hw[j][0], frame_hw[j][1], 3] at frame_off[j] inside frames_bytes; frame i of the call names staged
    // frame slots[i].  in_place: rows[i] addresses the staged frame itself (work_base = the staged buffer; the staged frames must
    // not overlap and the slots must be distinct); else rows[i] addresses the packed copy i at work_base (= out_dev).
    void build(const char *who, const void *work_base, size_t frames_bytes, int n_src, const uint64_t *frame_off, const int32_t *frame_hw,
               const int32_t *slots, int n, bool in_place);
    void set_tiles(const std::vector<int> &tiles_x) { for (size_t i = 0; i < rows.size() && i < tiles_x.size(); ++i) rows[i].tiles_x = tiles_x[i]; }
};

// Scratch of one caller (a stream's worth): host and device copies of the clipped rectangles and of the tile work list.
struct Anonymizer {
    DevBuf<int> rects, rect_ptr, work;
    std::vector<int> h_rects, h_ptr, h_work;      // kept until the stream has drained (the uploads read them)
    std::vector<int> h_tiles_x;                   // mixed layouts: tiles per row of every frame of the call
    int m = 0, k = 0, tiles_x = 0, mode = 0, H = 0, W = 0;
    uint32_t color = 0;
    // Host half: checks the tables of n frames of h x w pixels (fail() on a bad one: no device work has been enqueued), clips the
    // rectangles and lists the tiles they touch.  Returns the number of tiles: 0 = no rectangle touches any frame.
    // hw != NULL: a mixed layout - frame i is hw[2 i] x hw[2 i + 1] pixels (h and w are ignored) and h_tiles_x[i] is filled.
    int prepare(int n, int h, int w, const MaskSpec &mk, const int32_t *hw = nullptr);
    // Device half: masks frame (slots_dev ? slots_dev[i] : i) of `frames` (frame_bytes apart, packed 3-byte pixels) with the
    // rectangles prepare() took for frame i, in place, asynchronously on `s`.  No tiles: nothing is uploaded or launched.
    // geom_dev != NULL: a mixed layout - frame i is geom_dev[i] (frame_bytes and slots_dev are ignored).
    void launch(hipStream_t s, uint8_t *frames, size_t frame_bytes, const int *slots_dev, const OutFrame *geom_dev = nullptr);
};

}  // namespace yds
