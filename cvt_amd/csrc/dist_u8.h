// dist_u8.h -- the exact squared L2 distance between uint8 rows, L2SqrI (space_l2.h:186-245), as |q|^2 + |x|^2 - 2<q,x> on v_dot4:
// all three terms are exact in 32-bit integers (D <= 4096), so the order of the sums is free.  Only the first D / 4 * 4 bytes of a
// row take part: the reference sums groups of four bytes and drops a dim % 4 tail (space_l2.h:198), and so does everything here --
// W = D >> 2 is the number of 32-bit words of a row that count.  One lane per row, QT queries packed in LDS share every row read.
// Shared by the flat search (flat.hip), the range search (flat_range.hip) and the masked search (flat_masked.hip: the query set-up;
// its row walk is a written-out copy of dist_u8_row's, see there).
#ifndef CVTMI_DIST_U8_H
#define CVTMI_DIST_U8_H
#include "common.h"

namespace cvtmi {

// How a row is read.  U8_BYTES: single bytes, any D and alignment.  U8_PIECES: 16-byte pieces (D % 16 == 0), |x|^2 summed on the way.
// U8_SIGNED: 16-byte pieces with |x - 128|^2 supplied by the caller: q' = q - 128, x' = x - 128 (one xor per word),
// |q'|^2 + |x'|^2 - 2<q',x'> on the signed dot4 -- the same integer, without the dot4 of the row with itself.
enum { U8_BYTES = 0, U8_PIECES = 1, U8_SIGNED = 2 };

// Queries group * QT .. + QT - 1 of Q[nq][D], packed, to qw[QT][W] in LDS (U8_SIGNED: every byte ^ 0x80).  A query past the batch
// is a copy of the last one (its result is never written).  The caller's next barrier makes qw visible.
// I: the caller's index type (int or int64_t)
template <int FORM, int QT, class I>
__device__ __forceinline__ void dist_u8_stage(uint32_t *qw, const uint8_t *Q, I group, I nq, int D)
{
    const int W = D >> 2;
    for (int i = threadIdx.x; i < QT * W; i += kBlock) {
        const int q = i / W, w = i - q * W;
        I qi = group * QT + q;
        qi = qi < nq ? qi : nq - 1;
        const uint8_t *p = Q + (int64_t)qi * D + 4 * w;
        const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        qw[i] = FORM == U8_SIGNED ? v ^ 0x80808080u : v;
    }
}

// qq[q] = |q|^2 (U8_SIGNED: |q - 128|^2) of the staged queries, one thread each; call between two barriers
template <int FORM, int QT>
__device__ __forceinline__ void dist_u8_qnorms(uint32_t *qq, const uint32_t *qw, int W)
{
    const int tid = threadIdx.x;
    if (tid < QT) {
        uint32_t s = 0;
        for (int w = 0; w < W; ++w) {
            const uint32_t v = qw[tid * W + w];
            s = FORM == U8_SIGNED ? (uint32_t)__builtin_amdgcn_sdot4((int)v, (int)v, (int)s, false) : __builtin_amdgcn_udot4(v, v, s, false);
        }
        qq[tid] = s;
    }
}

// d[q] = the distance of row xr to staged query q (qw, qq as the two functions above left them): |q|^2 + |x|^2 - 2<q,x>, exact
// modulo 2^32, and every distance is below 2^31.  norm: U8_SIGNED, where |x - 128|^2 of the row lies (read behind the loop); unused
// otherwise.
// U: 16-byte pieces of the row requested before the first is used.  With one load in flight per lane a walk over many queries waits
// for memory latency, not bandwidth; with U = 1 the compiler unrolls the plain loop and moves its loads ahead by itself.
template <int FORM, int QT, int U = 1>
__device__ __forceinline__ void dist_u8_row(const uint8_t *xr, const uint32_t *qw, const uint32_t *qq, int W, const int32_t *norm,
                                            uint32_t (&d)[QT])
{
    uint32_t xx = 0, qx[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) qx[q] = 0;
    if constexpr (FORM == U8_BYTES) {
        for (int w = 0; w < W; ++w) {
            // (the four bytes are spelled out here, not in a function of their own: behind a call the compiler merges them, and those of
            // the iterations it unrolls, into 4- and 16-byte loads at any alignment, a different kernel from the one that was measured)
            const uint8_t *p = xr + 4 * w;
            const uint32_t xv = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            xx = __builtin_amdgcn_udot4(xv, xv, xx, false);
#pragma unroll
            for (int q = 0; q < QT; ++q) qx[q] = __builtin_amdgcn_udot4(qw[q * W + w], xv, qx[q], false);
        }
    } else {
        for (int w0 = 0; w0 < W; w0 += 4 * U) {
            uint4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (w0 + 4 * u < W) v[u] = *reinterpret_cast<const uint4 *>(xr + 4 * (w0 + 4 * u));   // (uniform: W is)
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = w0 + 4 * u;
                if (w >= W) break;
                const uint32_t xv[4] = { v[u].x, v[u].y, v[u].z, v[u].w };
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (FORM == U8_SIGNED) {
                        const int xs = (int)(xv[e] ^ 0x80808080u);
#pragma unroll
                        for (int q = 0; q < QT; ++q) qx[q] = (uint32_t)__builtin_amdgcn_sdot4((int)qw[q * W + w + e], xs, (int)qx[q], false);
                    } else {
                        xx = __builtin_amdgcn_udot4(xv[e], xv[e], xx, false);
#pragma unroll
                        for (int q = 0; q < QT; ++q) qx[q] = __builtin_amdgcn_udot4(qw[q * W + w + e], xv[e], qx[q], false);
                    }
                }
            }
        }
        if constexpr (FORM == U8_SIGNED) xx = (uint32_t)*norm;
    }
#pragma unroll
    for (int q = 0; q < QT; ++q) d[q] = qq[q] + xx - 2u * qx[q];
}

}  // namespace cvtmi
#endif
