// video_rank.hip -- the end of the reference's own query (opq/src/multi_frame_index_test.cpp:51-84): the per-frame rows of
// IVFOPQ::Query are added up in frame order into score_total[img_num], one fp32 add per frame, and the best videos are taken from the
// totals.  cvtmi_opq_rank_videos runs that for several query videos (segments of the frame list) at once: the existing probe and
// query_video_kernel write a chunk of the dense [frames][img_num] score matrix, video_frame_sum_kernel folds the chunk into
// total[segment][img_num], and the existing selection (launch_topk_select) reads the totals.
//   * the fold is t = +0.0f; for f ascending: t = __fadd_rn(t, ms[f][v]) -- no fma, no tree; a chunk that ends inside a segment
//     leaves the running totals in `total`, the next chunk continues from them, so the order of the adds never changes;
//   * a pure stream: every score cell is read once, every total written once per chunk.  A thread owns video columns, neighbouring
//     lanes neighbouring videos (256 contiguous bytes per wave and load, or 1 KB in the 16-byte form), and keeps the loads of kRankFrames
//     frames in flight while the adds stay in order;
//   * rows are img_num floats apart: the 16-byte form is taken only where img_num % 4 == 0 and both bases are 16-byte aligned, the
//     dword form everywhere else.  Index arithmetic is int64 (frames x img_num passes 2^31).
#include <algorithm>
#include <cstdint>

#include "kernels.h"
#include "launch.h"

namespace cvtmi {

constexpr int kRankCols = 4;                      // video columns of a thread
constexpr int kRankTile = kBlock * kRankCols;     // ... of a workgroup
constexpr int kRankFrames = 4;                    // frames whose loads are in flight together
constexpr int kRankSegArgs = 256;                 // segment offsets one table launch carries in its arguments

struct RankSegArgs {
    int64_t v[kRankSegArgs];
};

// the host's segment offsets into the leased set without a copy the stream would have to wait for: the values travel as arguments
__global__ __launch_bounds__(kBlock) void video_seg_table_kernel(RankSegArgs a, int count, int64_t *__restrict__ out)
{
    const int i = threadIdx.x;
    if (i < count) out[i] = a.v[i];
}

// segments [s0, s0 + gridDim.y) without frames: their totals are +0.0 (the others leave at once, workgroup-uniform)
__global__ __launch_bounds__(kBlock) void video_total_zero_kernel(const int64_t *__restrict__ seg_off, int64_t s0, int img_num, float *__restrict__ total,
                                                                  int64_t total_s0)
{
    const int64_t s = s0 + blockIdx.y;
    if (seg_off[s] != seg_off[s + 1]) return;
    float *t = total + (s - total_s0) * img_num;
    const int64_t v0 = (int64_t)blockIdx.x * kRankTile + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kRankCols; ++j) {
        const int64_t v = v0 + (int64_t)j * kBlock;
        if (v < img_num) t[v] = 0.0f;
    }
}

// ms: the score rows of frames [c0, c1), row f at ms + (f - c0) * img_num.  Workgroup (x, y): videos of tile x, segment s0 + y; its
// frames of the chunk are [max(seg_off[s], c0), min(seg_off[s + 1], c1)) -- none: nothing to do.  total row of segment s at
// total + (s - total_s0) * img_num; it is read only where the segment began in an earlier chunk.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void video_frame_sum_kernel(const float *__restrict__ ms, int64_t c0, int64_t c1, const int64_t *__restrict__ seg_off,
                                                                 int64_t s0, int img_num, float *__restrict__ total, int64_t total_s0)
{
    const int64_t s = s0 + blockIdx.y;
    const int64_t sb = seg_off[s], se = seg_off[s + 1];
    const int64_t b = sb > c0 ? sb : c0, e = se < c1 ? se : c1;
    if (b >= e) return;   // workgroup-uniform
    const bool first = b == sb;
    const int64_t w = img_num;
    float *trow = total + (s - total_s0) * w;
    const float *row = ms + (b - c0) * w;
    const int64_t nf = e - b;
    float t[kRankCols];
    if (VEC) {
        const int64_t v = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kRankCols;
        if (v >= w) return;   // img_num % 4 == 0: a thread's four columns are inside or outside together
        if (first) {
#pragma unroll
            for (int j = 0; j < kRankCols; ++j) t[j] = 0.0f;
        } else {
            const float4 x = *reinterpret_cast<const float4 *>(trow + v);
            t[0] = x.x; t[1] = x.y; t[2] = x.z; t[3] = x.w;
        }
        int64_t f = 0;
        for (; f + kRankFrames <= nf; f += kRankFrames) {
            float4 x[kRankFrames];
#pragma unroll
            for (int u = 0; u < kRankFrames; ++u) x[u] = *reinterpret_cast<const float4 *>(row + (f + u) * w + v);
#pragma unroll
            for (int u = 0; u < kRankFrames; ++u) {
                t[0] = __fadd_rn(t[0], x[u].x); t[1] = __fadd_rn(t[1], x[u].y);
                t[2] = __fadd_rn(t[2], x[u].z); t[3] = __fadd_rn(t[3], x[u].w);
            }
        }
        for (; f < nf; ++f) {
            const float4 x = *reinterpret_cast<const float4 *>(row + f * w + v);
            t[0] = __fadd_rn(t[0], x.x); t[1] = __fadd_rn(t[1], x.y);
            t[2] = __fadd_rn(t[2], x.z); t[3] = __fadd_rn(t[3], x.w);
        }
        *reinterpret_cast<float4 *>(trow + v) = make_float4(t[0], t[1], t[2], t[3]);
    } else {
        const int64_t v0 = (int64_t)blockIdx.x * kRankTile + threadIdx.x;
        bool in[kRankCols];
#pragma unroll
        for (int j = 0; j < kRankCols; ++j) {
            in[j] = v0 + (int64_t)j * kBlock < w;
            t[j] = (first || !in[j]) ? 0.0f : trow[v0 + (int64_t)j * kBlock];
        }
        int64_t f = 0;
        for (; f + kRankFrames <= nf; f += kRankFrames) {
            float x[kRankFrames][kRankCols];
#pragma unroll
            for (int u = 0; u < kRankFrames; ++u)
#pragma unroll
                for (int j = 0; j < kRankCols; ++j) x[u][j] = in[j] ? row[(f + u) * w + v0 + (int64_t)j * kBlock] : 0.0f;
#pragma unroll
            for (int u = 0; u < kRankFrames; ++u)
#pragma unroll
                for (int j = 0; j < kRankCols; ++j) t[j] = __fadd_rn(t[j], x[u][j]);
        }
        for (; f < nf; ++f)
#pragma unroll
            for (int j = 0; j < kRankCols; ++j)
                if (in[j]) t[j] = __fadd_rn(t[j], row[f * w + v0 + (int64_t)j * kBlock]);
#pragma unroll
        for (int j = 0; j < kRankCols; ++j)
            if (in[j]) trow[v0 + (int64_t)j * kBlock] = t[j];
    }
}

int launch_video_seg_table(const int64_t *seg_off_host, int64_t count, int64_t *seg_off_dev, hipStream_t st)
{
    for (int64_t i = 0; i < count; i += kRankSegArgs) {
        RankSegArgs a;
        const int c = (int)std::min<int64_t>(kRankSegArgs, count - i);
        for (int j = 0; j < kRankSegArgs; ++j) a.v[j] = j < c ? seg_off_host[i + j] : 0;
        CVTMI_TRY(launch("video_seg_table_kernel", video_seg_table_kernel, 1, kBlock, 0, st, a, c, seg_off_dev + i));
    }
    return CVTMI_OK;
}

int launch_video_total_zero(const int64_t *seg_off_dev, int64_t s_lo, int64_t s_hi, int img_num, float *total, int64_t total_s0, hipStream_t st)
{
    if (img_num <= 0) return CVTMI_OK;
    const int64_t tiles = blocks_for(img_num, kRankTile);
    for (int64_t s = s_lo; s < s_hi; s += kGridMaxYZ) {
        const int64_t ny = std::min<int64_t>(kGridMaxYZ, s_hi - s);
        CVTMI_TRY(launch("video_total_zero_kernel", video_total_zero_kernel, Grid(tiles, ny), kBlock, 0, st, seg_off_dev, s, img_num, total, total_s0));
    }
    return CVTMI_OK;
}

int launch_video_frame_sum(const float *ms, int64_t c0, int64_t c1, const int64_t *seg_off_dev, int64_t s_lo, int64_t s_hi, int img_num, float *total,
                           int64_t total_s0, hipStream_t st)
{
    if (img_num <= 0 || c0 >= c1) return CVTMI_OK;
    const bool vec = img_num % 4 == 0 && (reinterpret_cast<uintptr_t>(ms) & 15) == 0 && (reinterpret_cast<uintptr_t>(total) & 15) == 0;
    const int64_t tiles = blocks_for(img_num, kRankTile);
    for (int64_t s = s_lo; s < s_hi; s += kGridMaxYZ) {
        const int64_t ny = std::min<int64_t>(kGridMaxYZ, s_hi - s);
        CVTMI_TRY(launch("video_frame_sum_kernel", vec ? video_frame_sum_kernel<true> : video_frame_sum_kernel<false>, Grid(tiles, ny), kBlock, 0, st, ms, c0, c1,
                         seg_off_dev, s, img_num, total, total_s0));
    }
    return CVTMI_OK;
}

}  // namespace cvtmi
