// rm_common.h -- what the two stable compactions on the device share (opq_remove.hip: OPQ entries, flat_remove.hip: rows of a flat
// index): the geometry of the bitmap and the tiles, the position of a tile after the two-level scan, the layout helpers of the
// scratch.  The mark by entry id (launch_rm_mark_ids), the scan (launch_rm_scan) and launch_rm_fill_remap live in opq_remove.hip
// and take any RmPlan (kernels.h).
#pragma once
#include "kernels.h"

namespace cvtmi {

static_assert(kRmTile == 256, "a tile is 4 bitmap words: one per wave of its workgroup");
constexpr int kRmWords = kRmTile / 64;     // bitmap words of a tile
constexpr int kRmScanTiles = 2048;         // tiles one workgroup of the first scan level owns (8 per thread)
constexpr int kRmPivots = 1024;            // pivots of a removal table kept in LDS

__device__ __forceinline__ unsigned long long rm_valid_mask(int64_t row0, int64_t n)   // rows row0 .. row0 + 63 that exist
{
    if (row0 >= n) return 0ull;
    return n - row0 >= 64 ? ~0ull : ((1ull << (n - row0)) - 1ull);
}

// new insertion index of the first kept row of tile t (t == ntiles: the kept total)
__device__ __forceinline__ int64_t rm_tile_pos(const uint32_t *tile_off, const int64_t *boff, const int64_t *total, int64_t ntiles, int64_t t)
{
    return t < ntiles ? boff[t / kRmScanTiles] + tile_off[t] : total[0];
}

inline size_t rm_align(size_t b) { return (b + 255) & ~(size_t)255; }
template <class T> inline T *rm_at(void *scratch, size_t off) { return reinterpret_cast<T *>(static_cast<char *>(scratch) + off); }

}  // namespace cvtmi
