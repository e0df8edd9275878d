// range_common.h -- what the two range searches share (flat_range.hip: rows of a flat index under a distance radius, ivf_range.hip:
// entries of the probed lists under a score radius).  Both count before they place: a scan leaves per (query, part) the exact number
// of hits and the first C of them in the part's segment of a spill area, the offsets kernels turn the counts into lims and the
// parts' places, and a fill and a rescan write the result.  Here: the rank of a hit inside its part, the workgroup scan, and the
// layout of part_cnt / part_off / spill (RangeBufs, kernels.h) with the rule that keeps the spill area within a byte cap.  The
// offsets kernels live in ivf_range.hip behind launch_range_offsets (kernels.h); the scan, fill and rescan kernels stay with their
// payloads.
#pragma once
#include <algorithm>

#include "kernels.h"

namespace cvtmi {

// One 256-row tile of a part, QT queries at once: hit[q] is this lane's verdict for query q, run[q] the hits of the part so far
// (workgroup-uniform).  A hit's rank inside its part is the running count + the waves before + the lanes before: every wave ballots,
// the four wave counts meet in LDS -- no atomics, ascending rows, the same order on every run.  place(q, rank) is called for this
// lane's hits, then run[q] moves on by the hits of the tile.  Holds one barrier; wcnt has two count buffers, so the next tile's
// writes cannot pass this tile's reads.
template <int QT, class Place>
__device__ __forceinline__ void range_rank(uint32_t (*wcnt)[QT][4], int tile, const bool (&hit)[QT], uint32_t (&run)[QT], const Place &place)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long bal[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        bal[q] = __ballot(hit[q]);
        if (lane == 0) wcnt[tile & 1][q][wave] = (uint32_t)__popcll(bal[q]);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t c = wcnt[tile & 1][q][w];
            before += w < wave ? c : 0u;
            total += c;
        }
        if (hit[q]) place(q, run[q] + before + (uint32_t)__popcll(bal[q] & ((1ull << lane) - 1ull)));
        run[q] += total;
    }
}

// inclusive scan over the workgroup; s[kBlock - 1] holds the total until the caller's next barrier
template <class T>
__device__ __forceinline__ T range_block_scan(T v, T *s)
{
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < kBlock; o <<= 1) {
        const T t = tid >= o ? s[tid - o] : (T)0;
        __syncthreads();
        s[tid] += t;
        __syncthreads();
    }
    return s[tid];
}

// ---- host side ----
inline size_t range_up16(size_t b) { return (b + 15) / 16 * 16; }

// the spill records per (query, part) with which the spill area, nq x parts x records x 8 bytes, stays within `bytes`
inline int64_t range_spill_fit(size_t bytes, int64_t nq, int64_t parts)
{
    return (int64_t)(bytes / ((size_t)std::max<int64_t>(nq, 1) * parts * sizeof(unsigned long long)));
}

// part_cnt, part_off and the spill area of nq x parts cells, laid out from byte `off` of base on (base or b null: nothing is
// written).  Returns the offset behind them.
inline size_t range_carve(void *base, size_t off, int64_t nq, int64_t parts, int64_t spill, RangeBufs *b)
{
    const size_t cells = (size_t)nq * parts;
    const size_t o_cnt = off, o_off = o_cnt + range_up16(cells * sizeof(uint32_t)), o_spill = o_off + range_up16(cells * sizeof(uint32_t));
    if (base && b) {
        char *c = static_cast<char *>(base);
        b->part_cnt = reinterpret_cast<uint32_t *>(c + o_cnt);
        b->part_off = reinterpret_cast<uint32_t *>(c + o_off);
        b->spill = reinterpret_cast<unsigned long long *>(c + o_spill);
    }
    return o_spill + range_up16(cells * (size_t)spill * sizeof(unsigned long long));
}

}  // namespace cvtmi
