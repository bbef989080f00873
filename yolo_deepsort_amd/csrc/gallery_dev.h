// What the readers of the trackers' appearance galleries share (gallery_search.hip: the search calls, identity.hip: the identity map):
// the descriptor of one tracker as the kernels see it, the distance kernel (defined in gallery_search.hip and launched from either
// unit through its host stub), and the order-preserving bits of a distance.
#pragma once
#include "tracker_dev.h"

namespace yds {

// One tracker as the kernels see it, in an array like TrkGroupDev: tracks [g0, g0 + n) of the call are its track list.
struct alignas(16) GalleryDesc {
    const float *gallery;                         // [slot][budget][EMB], rows normalised
    const int *slot, *id, *state, *n_feat;        // the tracker's table columns (track-list order)
    int budget, g0, n, stream;
};
static_assert(sizeof(GalleryDesc) % 16 == 0, "the host packs GalleryDesc arrays at a stride of sizeof(GalleryDesc)");

constexpr int GALLERY_SLAB = 32;                  // queries per workgroup of gallery_min_dist_kernel = one MFMA tile edge

// dist[q][g] for q < Q and every track g of the descriptors; grid (tracks, ceil(Q / GALLERY_SLAB)), 256 threads
__global__ __launch_bounds__(256) void gallery_min_dist_kernel(const GalleryDesc *desc, int n_desc, const float *qn, int Q, float *dist, int ld);

// fp32 -> unsigned with the same order (negative values included: 1 - dot may come out a few ulps below 0)
__device__ __forceinline__ unsigned ordered_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
}  // namespace yds
