// flat_rerank.hip -- cvtmi_flat_rerank: the exact top k among the candidate rows a caller names, one fused launch.
//
// A workgroup owns one query (and loops while nq exceeds the grid).  Per query:
//   1. the query goes to LDS; the valid candidates (cand_base <= cand < cand_base + n) are compacted into the low words of the pair
//      array -- in any order: nothing below depends on it;
//   2. tiles of candidate rows are staged in LDS by the whole workgroup, rows padded against bank conflicts:
//        blocked fp32   a wave instruction fetches float4 c of 64 candidates, each from a 128-byte line of its own (16 useful bytes
//                       of 128: the 8x source);
//        row-major      whole rows in 16-byte (4-byte, 1-byte) units, consecutive lanes on consecutive units of a row;
//      then LANES lanes walk one candidate: lane l keeps accumulator l of dist_f32_row -- the same operations in the same order on
//      the same values -- and the LANES sums are added left to right through shuffles, as dist_f32_row adds them.  The three row
//      sources therefore give the same bits.  uint8: eight lanes share a row's 4-byte words, the sum is an exact integer;
//   3. the (key, row) pairs are sorted in LDS (bitonic, a power of two >= the valid count, the rest filled with all-ones);
//   4. equal neighbours -- a row named several times: same row, same distance -- are dropped by a workgroup scan, and the first k
//      distinct pairs are written with their labels; the list pads with (0x7f800000, -1).
// There is no [nq][R] array in HBM.  Keys: cvtmi_topk_select's float order (-0.0 on +0.0's key; NaN by its bits) without its clamp
// of the last NaN -- the "not a candidate" code here is the all-ones PAIR, which no row < 2^32 - 1 forms; uint8: the int32 itself.
#include <algorithm>

#include "kernels.h"
#include "launch.h"

namespace cvtmi {

namespace {

// rows in flight per workgroup and step (a 128-d fp32 tile: 30 rows).  Measured, 1 M x 128-d fp32, 1000 queries, R = 1000, from the
// row-major copy: 8 KB 0.202 ms, 16 KB 0.160, 32 KB 0.261 (fewer workgroups per CU); blocked rows 0.637 / 0.635 / 0.728; 10 M x 128-byte
// uint8 0.089 / 0.093 / 0.129
constexpr int RR_TILE_BYTES = 16384;
constexpr int RR_U8_LANES = 8;         // lanes that share a uint8 row

struct FlatRerankArgs {
    const void *data;        // rows: blocked fp32 (src 1), row-major otherwise
    const void *q;           // [nq][D] of the index's own type
    const int64_t *cand;     // [nq][R]
    const int64_t *labels;   // stored labels, or null: id_base + row
    uint32_t *out_d;         // [nq][k] 4-byte fields
    int64_t *out_l;          // [nq][k]
    int64_t n, nq, cand_base, id_base;
    int D, R, k, src, skip_m1;
    int row_bytes, vec;      // bytes of a row; unit of the row-major staging loop: 16, 4 or 1 bytes
    int rp, tr, stride_w;    // pairs the LDS array holds (a power of two >= R), rows per tile, 4-byte words between two rows of a tile
};

__device__ __forceinline__ uint32_t rr_key(float d)
{
    const uint32_t u = __float_as_uint(d);
    const uint32_t m = (uint32_t)((int32_t)u >> 31);
    return (u ^ (m | 0x80000000u)) - m;   // (topk_merge.hip: -0.0 lands on +0.0's key)
}
__device__ __forceinline__ uint32_t rr_key_bits(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : (0u - k); }

// MODE 0 = IP, 1 = L2F, 2 = L2U8; LANES as dist_f32_row's (uint8: unused)
template <int MODE, int LANES>
__global__ __launch_bounds__(kBlock) void flat_rerank_kernel(const FlatRerankArgs a)
{
    extern __shared__ __align__(16) unsigned char rr_lds[];
    __shared__ int cnt_s;
    __shared__ int wsum_s[kBlock / 64];
    unsigned long long *pair_s = reinterpret_cast<unsigned long long *>(rr_lds);
    uint32_t *tile_s = reinterpret_cast<uint32_t *>(rr_lds + (size_t)a.rp * 8);
    uint32_t *q_s = tile_s + (size_t)a.tr * a.stride_w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int L = MODE == 2 ? RR_U8_LANES : LANES;   // lanes per candidate in the walk

    for (int64_t f = blockIdx.x; f < a.nq; f += gridDim.x) {
        // ---- 1. query, valid candidates ----
        if (tid == 0) cnt_s = 0;
        if constexpr (MODE == 2) {
            const uint8_t *qb = reinterpret_cast<const uint8_t *>(a.q) + f * a.D;   // (a row of D bytes: no alignment to speak of)
            for (int w = tid; w < (a.D >> 2); w += kBlock)
                q_s[w] = (uint32_t)qb[4 * w] | ((uint32_t)qb[4 * w + 1] << 8) | ((uint32_t)qb[4 * w + 2] << 16) | ((uint32_t)qb[4 * w + 3] << 24);
        } else {
            const uint32_t *qw = reinterpret_cast<const uint32_t *>(a.q) + f * a.D;
            for (int i = tid; i < a.D; i += kBlock) q_s[i] = qw[i];
        }
        __syncthreads();
        for (int j0 = 0; j0 < a.R; j0 += kBlock) {   // (workgroup-uniform trip count)
            const int j = j0 + tid;
            bool ok = false;
            uint32_t row = 0;
            if (j < a.R) {
                const int64_t c = a.cand[f * a.R + j];
                const uint64_t u = (uint64_t)c - (uint64_t)a.cand_base;   // modulo 2^64: with c >= cand_base it is the true difference
                ok = c >= a.cand_base && u < (uint64_t)a.n && !(a.skip_m1 && c == -1);
                row = (uint32_t)u;
            }
            const unsigned long long b = __ballot(ok);
            int at = 0;
            if (lane == 0 && b) at = atomicAdd(&cnt_s, __popcll(b));
            at = __shfl(at, 0, 64);
            if (ok) pair_s[at + __popcll(b & ((1ull << lane) - 1ull))] = row;
        }
        __syncthreads();
        const int cnt = cnt_s;
        int sp = 2;
        while (sp < cnt) sp <<= 1;   // <= rp
        for (int i = cnt + tid; i < sp; i += kBlock) pair_s[i] = ~0ull;

        // ---- 2. score: stage a tile of rows, walk it ----
        for (int t0 = 0; t0 < cnt; t0 += a.tr) {
            const int tn = min(a.tr, cnt - t0);
            if (a.src == 1) {
                const int upr = a.D >> 2, total = tn * upr;
                const float4 *X = reinterpret_cast<const float4 *>(a.data);
#pragma unroll 4
                for (int u = tid; u < total; u += kBlock) {
                    const int c = u / tn, t = u - c * tn;   // candidates fastest: a wave instruction fetches one float4 column of 64 rows
                    const uint32_t r = (uint32_t)pair_s[t0 + t];
                    const float4 v = X[((int64_t)(r >> 6) * upr + c) * 64 + (r & 63)];
                    *reinterpret_cast<float4 *>(tile_s + (size_t)t * a.stride_w + 4 * c) = v;
                }
            } else if (a.vec == 16) {
                const int upr = a.row_bytes >> 4, total = tn * upr;
                const unsigned char *X = reinterpret_cast<const unsigned char *>(a.data);
#pragma unroll 4
                for (int u = tid; u < total; u += kBlock) {
                    const int t = u / upr, c = u - t * upr;   // units of a row fastest: whole lines
                    const uint32_t r = (uint32_t)pair_s[t0 + t];
                    const uint4 v = *reinterpret_cast<const uint4 *>(X + (int64_t)r * a.row_bytes + 16 * c);
                    *reinterpret_cast<uint4 *>(tile_s + (size_t)t * a.stride_w + 4 * c) = v;
                }
            } else if (a.vec == 4) {
                const int upr = a.row_bytes >> 2, total = tn * upr;
                const unsigned char *X = reinterpret_cast<const unsigned char *>(a.data);
#pragma unroll 4
                for (int u = tid; u < total; u += kBlock) {
                    const int t = u / upr, c = u - t * upr;
                    const uint32_t r = (uint32_t)pair_s[t0 + t];
                    tile_s[(size_t)t * a.stride_w + c] = *reinterpret_cast<const uint32_t *>(X + (int64_t)r * a.row_bytes + 4 * c);
                }
            } else {
                const int upr = a.row_bytes, total = tn * upr;
                const unsigned char *X = reinterpret_cast<const unsigned char *>(a.data);
                unsigned char *tb = reinterpret_cast<unsigned char *>(tile_s);
#pragma unroll 4
                for (int u = tid; u < total; u += kBlock) {
                    const int t = u / upr, c = u - t * upr;
                    const uint32_t r = (uint32_t)pair_s[t0 + t];
                    tb[(size_t)t * a.stride_w * 4 + c] = X[(int64_t)r * a.row_bytes + c];
                }
            }
            __syncthreads();
            const int l = tid % L, first = lane - l;
            for (int tb0 = 0; tb0 < tn; tb0 += kBlock / L) {   // (uniform: every lane of a candidate's group takes part in the shuffles)
                const int t = tb0 + tid / L;
                const bool live = t < tn;
                uint32_t key;
                if constexpr (MODE == 2) {
                    int acc = 0;
                    if (live) {
                        const uint32_t *x = tile_s + (size_t)t * a.stride_w;
                        for (int w = l; w < (a.D >> 2); w += L) {
                            const uint32_t xv = x[w], qv = q_s[w];
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const int d = (int)((xv >> (8 * b)) & 255u) - (int)((qv >> (8 * b)) & 255u);
                                acc += d * d;
                            }
                        }
                    }
#pragma unroll
                    for (int o = 1; o < L; o <<= 1) acc += __shfl_xor(acc, o, 64);
                    key = (uint32_t)acc;
                } else {
                    float acc = 0.0f;
                    if (live) {
                        const float *x = reinterpret_cast<const float *>(tile_s) + (size_t)t * a.stride_w;
                        const float *qf = reinterpret_cast<const float *>(q_s);
                        for (int i = l; i < a.D; i += L) {   // accumulator l of dist_f32_row: elements l, l + LANES, ...
                            if constexpr (MODE == 0) {
                                acc = __fadd_rn(acc, __fmul_rn(qf[i], x[i]));
                            } else {
                                const float d = __fsub_rn(qf[i], x[i]);
                                acc = __fadd_rn(acc, __fmul_rn(d, d));
                            }
                        }
                    }
                    float s = __shfl(acc, first, 64);
#pragma unroll
                    for (int j = 1; j < L; ++j) s = __fadd_rn(s, __shfl(acc, first + j, 64));
                    key = rr_key(MODE == 0 ? __fsub_rn(1.0f, s) : s);
                }
                if (live && l == 0) pair_s[t0 + t] = ((unsigned long long)key << 32) | (uint32_t)pair_s[t0 + t];
            }
            __syncthreads();
        }
        __syncthreads();   // (cnt == 0: the fill above)

        // ---- 3. sort ascending (key, row) ----
        for (int k2 = 2; k2 <= sp; k2 <<= 1)
            for (int j = k2 >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < sp; i += kBlock) {
                    const int o = i ^ j;
                    if (o > i) {
                        const unsigned long long x = pair_s[i], y = pair_s[o];
                        if ((x > y) == ((i & k2) == 0)) { pair_s[i] = y; pair_s[o] = x; }
                    }
                }
                __syncthreads();
            }

        // ---- 4. drop equal neighbours, write the first k ----
        const int per = sp > kBlock ? sp / kBlock : 1;
        const int i0 = tid * per, i1 = min(i0 + per, cnt);
        int mine = 0;
        for (int i = i0; i < i1; ++i) mine += (i == 0 || pair_s[i] != pair_s[i - 1]) ? 1 : 0;
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum_s[wave] = incl;
        __syncthreads();
        int before = incl - mine, distinct = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            if (w < wave) before += wsum_s[w];
            distinct += wsum_s[w];
        }
        uint32_t *od = a.out_d + f * a.k;
        int64_t *ol = a.out_l + f * a.k;
        for (int i = i0; i < i1 && before < a.k; ++i) {
            const unsigned long long p = pair_s[i];
            if (i == 0 || p != pair_s[i - 1]) {
                const uint32_t row = (uint32_t)p, key = (uint32_t)(p >> 32);
                od[before] = MODE == 2 ? key : rr_key_bits(key);
                ol[before] = a.labels ? a.labels[row] : a.id_base + (int64_t)row;
                ++before;
            }
        }
        for (int i = distinct + tid; i < a.k; i += kBlock) {
            od[i] = 0x7f800000u;
            ol[i] = -1;
        }
        __syncthreads();   // the next query reuses the arrays
    }
}

}  // namespace

int launch_flat_rerank(int metric, int D, const void *data, int src, int64_t n, const int64_t *labels, int64_t id_base, const void *q,
                       int64_t nq, const int64_t *cand, int R, int64_t cand_base, bool skip_minus_one, int k, void *dist, int64_t *out_labels,
                       int64_t info[4], hipStream_t st)
{
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (nq <= 0) return CVTMI_OK;
    if (k < 1 || k > kBigK || R < 1 || R > CVTMI_RERANK_MAX) return fail(CVTMI_EINVAL, "flat_rerank: k=%d R=%d out of range", k, R);
    if (D < 1 || D > 4096) return fail(CVTMI_EUNSUPPORTED, "flat_rerank: D=%d outside 1..4096", D);
    if (n < 0 || n >= ((int64_t)1 << 32)) return fail(CVTMI_EUNSUPPORTED, "flat_rerank: %lld rows: rows travel as 32-bit words", (long long)n);
    const bool u8 = metric == CVTMI_METRIC_L2U8, ip = metric == CVTMI_METRIC_IP;
    if (!u8 && !ip && metric != CVTMI_METRIC_L2F) return fail(CVTMI_EINVAL, "flat_rerank: unknown metric %d", metric);
    if ((src == 1 || src == 2) != (!u8 && D % 4 == 0) || src < 0 || src > 2) return fail(CVTMI_EINVAL, "flat_rerank: row source %d does not fit the layout", src);
    const int lanes = u8 ? 0 : ((D % 4 != 0) ? 1 : (ip ? 4 : (D % 16 == 0 ? 8 : 4)));   // as launch_flat_search and launch_hnsw_rerank pick them
    FlatRerankArgs a;
    a.data = data; a.q = q; a.cand = cand; a.labels = labels; a.out_d = static_cast<uint32_t *>(dist); a.out_l = out_labels;
    a.n = n; a.nq = nq; a.cand_base = cand_base; a.id_base = id_base;
    a.D = D; a.R = R; a.k = k; a.src = src; a.skip_m1 = skip_minus_one ? 1 : 0;
    a.row_bytes = u8 ? D : D * 4;
    a.vec = a.row_bytes % 16 == 0 ? 16 : (a.row_bytes % 4 == 0 ? 4 : 1);
    a.rp = std::max(2, next_pow2(R));
    // words between two rows of a tile: the groups of lanes that walk neighbouring rows start LANES banks apart (ds_read_b32: 32
    // banks per half wave), one lane per row an odd number of words
    const int words = (a.row_bytes + 3) / 4, step = u8 ? RR_U8_LANES : lanes;
    a.stride_w = step == 1 ? (words | 1) : words + ((step - words % 32) + 32) % 32;
    a.tr = std::max(1, std::min(kBlock, RR_TILE_BYTES / (a.stride_w * 4)));
    const size_t lds = (size_t)a.rp * 8 + (size_t)a.tr * a.stride_w * 4 + (size_t)words * 4;
    const int64_t groups = std::min<int64_t>(nq, (int64_t)8 * device_cus());
    if (info) { info[0] = src; info[1] = lanes; info[2] = groups; info[3] = (int64_t)lds; }
    static LdsOnce once[6];
    constexpr size_t kLimit = 96 << 10;   // pairs 32 KB + a tile of 16 KB (one row of 4096-d with its padding: 16.5 KB) + the query 16 KB
    if (lds > kLimit) return fail(CVTMI_EUNSUPPORTED, "flat_rerank: %zu bytes of LDS", lds);
#define RR_LAUNCH(slot, MODE, LN) \
    return launch_lds_once("flat_rerank_kernel", flat_rerank_kernel<MODE, LN>, once[slot], kLimit, groups, kBlock, lds, st, a)
    if (u8) RR_LAUNCH(0, 2, 1);
    if (ip) {
        if (lanes == 4) RR_LAUNCH(1, 0, 4);
        RR_LAUNCH(2, 0, 1);
    }
    if (lanes == 8) RR_LAUNCH(3, 1, 8);
    if (lanes == 4) RR_LAUNCH(4, 1, 4);
    RR_LAUNCH(5, 1, 1);
#undef RR_LAUNCH
}

}  // namespace cvtmi
