// ivf_table.h -- what the kernels that walk probed lists share (ivf_search.hip, ivf_range.hip): the [M][256] table of a
// (query, list) pair in LDS and the score of a row of the list-ordered copy.  The arithmetic is IVFOPQ::Query's
// (opq/src/IVFOPQ.cpp:273-306): residual q - coarse[l], separate subtract / multiply / add, the M cells summed m ascending.
#pragma once
#include "common.h"

namespace cvtmi {

typedef uint32_t ivf_u32x4 __attribute__((ext_vector_type(4)));

// res[D] = q - coarse[l], then lut[m][j] = |res_m - books[m][j]|^2 (j >= K: +inf), spread over the workgroup's kBlock threads;
// returns behind a barrier, so every thread may read the table
__device__ __forceinline__ void ivf_build_table(float *res, float *lut, const float *__restrict__ q, const float *__restrict__ centroid,
                                                const float *__restrict__ books, int D, int M, int K, int step, int tid)
{
    for (int d = tid; d < D; d += kBlock) res[d] = __fsub_rn(q[d], centroid[d]);
    __syncthreads();
    for (int t = tid; t < M * 256; t += kBlock) {
        const int m = t >> 8, j = t & 255;
        float acc = __uint_as_float(0x7f800000u);
        if (j < K) {
            const float *c = books + ((int64_t)m * K + j) * step;
            const float *rr = res + m * step;
            acc = 0.0f;
            if ((step & 3) == 0) {  // (16-byte aligned codewords: four dimensions per load, same operation order)
                for (int kk = 0; kk < step; kk += 4) {
                    const float4 cv = *reinterpret_cast<const float4 *>(c + kk);
                    const float4 rv = *reinterpret_cast<const float4 *>(rr + kk);
                    const float d0 = __fsub_rn(rv.x, cv.x), d1 = __fsub_rn(rv.y, cv.y), d2 = __fsub_rn(rv.z, cv.z), d3 = __fsub_rn(rv.w, cv.w);
                    acc = __fadd_rn(acc, __fmul_rn(d0, d0)); acc = __fadd_rn(acc, __fmul_rn(d1, d1));
                    acc = __fadd_rn(acc, __fmul_rn(d2, d2)); acc = __fadd_rn(acc, __fmul_rn(d3, d3));
                }
            } else {
                for (int kk = 0; kk < step; ++kk) {
                    const float d = __fsub_rn(rr[kk], c[kk]);
                    acc = __fadd_rn(acc, __fmul_rn(d, d));
                }
            }
        }
        lut[t] = acc;
    }
    __syncthreads();
}

// score of one row from its 16 code bytes (M = 16), m ascending
__device__ __forceinline__ float ivf_score16(const float *lut, const ivf_u32x4 v)
{
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
    float s = 0.0f;
#pragma unroll
    for (int m = 0; m < 16; ++m) s = __fadd_rn(s, lut[m * 256 + ((w[m >> 2] >> (8 * (m & 3))) & 0xffu)]);
    return s;
}

// any other M: the row's M bytes in one load where M is 8 or 4 (rows of the list-ordered copy are M-byte aligned), byte loads otherwise
__device__ __forceinline__ float ivf_score_row(const float *lut, const uint8_t *__restrict__ c, int M)
{
    float s = 0.0f;
    if (M == 8) {
        const uint2 v = *reinterpret_cast<const uint2 *>(c);
        const uint32_t w[2] = { v.x, v.y };
#pragma unroll
        for (int m = 0; m < 8; ++m) s = __fadd_rn(s, lut[m * 256 + ((w[m >> 2] >> (8 * (m & 3))) & 0xffu)]);
    } else if (M == 4) {
        const uint32_t w = *reinterpret_cast<const uint32_t *>(c);
#pragma unroll
        for (int m = 0; m < 4; ++m) s = __fadd_rn(s, lut[m * 256 + ((w >> (8 * m)) & 0xffu)]);
    } else {
        for (int m = 0; m < M; ++m) s = __fadd_rn(s, lut[m * 256 + c[m]]);
    }
    return s;
}

}  // namespace cvtmi
