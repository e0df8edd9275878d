// dist_f32.h -- fp32 distances in the summation order of the reference's own SIMD builds, so that results are
// bit-exact: inner product = 1 - sum in 4-lane SSE order (space_ip.hpp / space_ip.h: the AVX branches are not
// compiled), squared L2 in 8-lane AVX order when D % 16 == 0, 4-lane when D % 4 == 0 (space_l2.h:40-151), the
// scalar loop otherwise.  Shared by the flat search and the HNSW search.
#ifndef CVTMI_DIST_F32_H
#define CVTMI_DIST_F32_H
#include "common.h"

namespace cvtmi {

// LANES = 1 (scalar loop), 4 or 8;  IP = inner product, else squared L2
template <bool IP, int LANES, int QT>
__device__ __forceinline__ void dist_f32_row(const float *__restrict__ row, const float *qs, int D, float (&out)[QT])
{
    float acc[QT][LANES];
#pragma unroll
    for (int q = 0; q < QT; ++q)
#pragma unroll
        for (int l = 0; l < LANES; ++l) acc[q][l] = 0.0f;
    if constexpr (LANES == 1) {
        for (int i = 0; i < D; ++i) {
            const float xv = row[i];
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                if constexpr (IP) {
                    acc[q][0] = __fadd_rn(acc[q][0], __fmul_rn(qs[q * D + i], xv));
                } else {
                    const float t = __fsub_rn(qs[q * D + i], xv);
                    acc[q][0] = __fadd_rn(acc[q][0], __fmul_rn(t, t));
                }
            }
        }
    } else {
        for (int i = 0; i < D; i += LANES) {
            float xv[LANES];
#pragma unroll
            for (int l4 = 0; l4 < LANES / 4; ++l4) {
                const float4 v = *reinterpret_cast<const float4 *>(row + i + 4 * l4);
                xv[4 * l4 + 0] = v.x; xv[4 * l4 + 1] = v.y; xv[4 * l4 + 2] = v.z; xv[4 * l4 + 3] = v.w;
            }
#pragma unroll
            for (int q = 0; q < QT; ++q) {
#pragma unroll
                for (int l = 0; l < LANES; ++l) {
                    if constexpr (IP) {
                        acc[q][l] = __fadd_rn(acc[q][l], __fmul_rn(qs[q * D + i + l], xv[l]));
                    } else {
                        const float t = __fsub_rn(qs[q * D + i + l], xv[l]);
                        acc[q][l] = __fadd_rn(acc[q][l], __fmul_rn(t, t));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        float s = acc[q][0];
#pragma unroll
        for (int l = 1; l < LANES; ++l) s = __fadd_rn(s, acc[q][l]);
        out[q] = IP ? __fsub_rn(1.0f, s) : s;
    }
}

// The queries of a workgroup as dist_f32_row reads them: queries group * QT .. + QT - 1 of Q[nq][D] copied to qs[QT][D] in LDS.  A
// query past the batch is a copy of the last one (its result is never written).  The caller's next barrier makes qs visible.
// I: the caller's index type (int or int64_t)
template <int QT, class I>
__device__ __forceinline__ void dist_f32_stage(float *qs, const float *Q, I group, I nq, int D)
{
    for (int i = threadIdx.x; i < QT * D; i += kBlock) {
        const int q = i / D, d = i - q * D;
        I qi = group * QT + q;
        qi = qi < nq ? qi : nq - 1;
        qs[i] = Q[(int64_t)qi * D + d];
    }
}

// The same queries as dist_f32_blocked reads them: constant address space + uniform address = s_load_dword*, the values land in
// SGPRs.  Clamped as above.
typedef const __attribute__((address_space(4))) float dist_cfloat;
template <int QT, class I>
__device__ __forceinline__ void dist_f32_uniform(dist_cfloat *(&qp)[QT], const void *Q, I group, I nq, int D)
{
    dist_cfloat *Qc = (dist_cfloat *)(uintptr_t)Q;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        I qi = group * QT + q;
        qi = qi < nq ? qi : nq - 1;
        qp[q] = Qc + (int64_t)qi * D;   // wave-uniform
    }
}

// The same distances for R rows of the 64-row blocked layout (flat_block_kernel: float4 c of a row lies 64 float4 behind its
// float4 c - 1) with the queries behind uniform constant-address-space pointers, i.e. in SGPRs: every query value is the same for
// all 64 lanes, so the multiply / subtract take it as a scalar operand and the distance loop has no LDS traffic at all.  The loop is
// unrolled so that the scalar loads of 16 dimensions x QT queries are in flight together.
// Per lane and query the operations and their order are dist_f32_row's, hence the same bits.  LANES = 4 or 8, D % LANES == 0.
template <bool IP, int LANES, int QT, int R>
__device__ __forceinline__ void dist_f32_blocked(const float4 *const (&rowp)[R], dist_cfloat *const (&qp)[QT], int D, float (&out)[R][QT])
{
    static_assert(LANES == 4 || LANES == 8, "the blocked layout holds whole float4");
    float acc[R][QT][LANES];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < QT; ++q)
#pragma unroll
            for (int l = 0; l < LANES; ++l) acc[r][q][l] = 0.0f;
#pragma unroll 16 / LANES
    for (int i = 0; i < D; i += LANES) {
        float xv[R][LANES];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int l4 = 0; l4 < LANES / 4; ++l4) {
                const float4 v = rowp[r][(int64_t)((i >> 2) + l4) * 64];
                xv[r][4 * l4 + 0] = v.x; xv[r][4 * l4 + 1] = v.y; xv[r][4 * l4 + 2] = v.z; xv[r][4 * l4 + 3] = v.w;
            }
#pragma unroll
        for (int q = 0; q < QT; ++q) {
#pragma unroll
            for (int l = 0; l < LANES; ++l) {
                const float qv = qp[q][i + l];  // uniform address: scalar load
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if constexpr (IP) {
                        acc[r][q][l] = __fadd_rn(acc[r][q][l], __fmul_rn(qv, xv[r][l]));
                    } else {
                        const float t = __fsub_rn(qv, xv[r][l]);
                        acc[r][q][l] = __fadd_rn(acc[r][q][l], __fmul_rn(t, t));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            float s = acc[r][q][0];
#pragma unroll
            for (int l = 1; l < LANES; ++l) s = __fadd_rn(s, acc[r][q][l]);
            out[r][q] = IP ? __fsub_rn(1.0f, s) : s;
        }
}

}  // namespace cvtmi
#endif
