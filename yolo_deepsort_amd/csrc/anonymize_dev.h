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

// Scratch of one caller (a stream's worth): host and device copies of the clipped rectangles and of the tile work list.
struct Anonymizer {
    DevBuf<int> rects, rect_ptr, work;
    std::vector<int> h_rects, h_ptr, h_work;      // kept until the stream has drained (the uploads read them)
    int m = 0, k = 0, tiles_x = 0, mode = 0, H = 0, W = 0;
    uint32_t color = 0;
    // Host half: checks the tables of n frames of h x w pixels (fail() on a bad one: no device work has been enqueued), clips the
    // rectangles and lists the tiles they touch.  Returns the number of tiles: 0 = no rectangle touches any frame.
    int prepare(int n, int h, int w, const MaskSpec &mk);
    // Device half: masks frame (slots_dev ? slots_dev[i] : i) of `frames` (frame_bytes apart, packed 3-byte pixels) with the
    // rectangles prepare() took for frame i, in place, asynchronously on `s`.  No tiles: nothing is uploaded or launched.
    void launch(hipStream_t s, uint8_t *frames, size_t frame_bytes, const int *slots_dev);
};

}  // namespace yds
