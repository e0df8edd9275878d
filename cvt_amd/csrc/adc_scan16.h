// adc_scan16.h -- pieces shared by the M = 16 skewed scan kernels (adc_scan.hip: adc_scan16q / adc_scan16a, adc_scan_p.hip:
// adc_scan16p, adc_scan_h.hip: adc_scan16h and its table kernel): kernel arguments, the rule of the 15-bit lower-bound tables
// (scan16_query_params, scan16_quantise: stated here ONCE, every form calls them) and their build in LDS, the conflict-free
// look-up loop of one row, the exact re-sum of candidates, the lazy (integer-key) selection, the seed, and the workgroup frame
// of the checkpointed forms (block decoding, first thresholds, chunk hand-out, candidate push, checkpoint compaction, list
// epilogue).  A kernel keeps what is its own: its shared-memory layout, its look-up loop and its control words.  See
// adc_scan.hip for the reference arithmetic (opq/src/IVFOPQ.cpp:273-306) and the derivations.
// Shape of the helpers: they take structures by reference and read them where the value is used, and keep what they update in
// locals; a helper that takes a value the caller has loaded already, or updates a caller's variable through a reference inside a
// loop, moves loads and branches and with them the kernel's schedule (check a change with tools/device_asm_diff.sh).
#pragma once
#include "block_topk.h"
#include "kernels.h"

namespace cvtmi {

struct ScanArgs {
    const uint8_t *codes;
    int64_t n_rows;
    int64_t id_base;
    const float *q_rot;
    int nq;
    const float *books;
    const float *centroid;  // coarse[0]
    int D, step, K, k;
    int splits;
    int64_t rows_per_split;
    int groups;
    int groups_a, splits_b, stride;  // two-region plan (kernels.h), adc_scan16q only; stride = partial slots per query
    int64_t rows_per_split_b;
    float *part_d;
    int64_t *part_id;
    float *out_d;      // adc_scan16q, two-region plan whose first region has ONE row split: that region's groups write their (final) lists
    int64_t *out_id;   // straight to [nq][k] here and the merge only visits the other queries (scan_in_place_queries); null: everything to part_*
    const float *lut_g;  // [nq][M][256] fp32 tables in HBM, +inf past K (adc_scan16q only)
    const uint8_t *codes_rot;  // adc_scan16q: copy of the code rows with row r rotated left by r & 15 bytes (or null)
    uint32_t *gthr;            // adc_scan16q: [nq] filter thresholds (table units) shared by the row splits of a query, or null
    int lazy;                  // adc_scan16q: 1 = intermediate compactions select on the integer lower bounds (exact sums only at the end)
    int seed;                  // adc_scan16q / 16a: 1 = first thresholds from a histogram of the split's first rows (scan16q_seed)
    const uint32_t *only = nullptr;  // answer query g only when only[g] != 0; null: every query.  Read by adc_scan_kernel with one query per
                                     // workgroup (the big-k filter pipeline's fall-back, adc_scan_h.hip) and by adc_scan16q_kernel (the
                                     // matrix-core route's, adc_mfma.hip); the launches of adc_scan16a / adc_scan16p refuse it
};

#ifdef CVTMI_SCAN_TIMING
static __device__ unsigned long long g_scan_dbg[8];   // (one copy per translation unit: each has its own debug accessor)
static __device__ unsigned long long g_scan_dbg2[8];  // adc_scan16a slow path, lane 0 of every wave: calls, cycles, compactions, compaction cycles, cycles waiting for stores, retry rounds
static __device__ unsigned long long g_scan_trace[4 * 16384];  // per workgroup: wall start, wall end (100 MHz), shader clocks, HW_ID | XCC_ID << 32
#define SQ_T(i) do { if (threadIdx.x == 0) { const unsigned long long now__ = clock64(); t_acc__[i] += now__ - t_last__; t_last__ = now__; } } while (0)
#define SQ_T0() unsigned long long t_last__ = clock64(); unsigned long long t_acc__[5] = { 0, 0, 0, 0, 0 }; \
    const unsigned long long t_first__ = t_last__, w_first__ = wall_clock64()
#define SQ_TEND() do { if (threadIdx.x == 0) { for (int i__ = 0; i__ < 5; ++i__) atomicAdd(&g_scan_dbg[i__], t_acc__[i__]); \
    if (blockIdx.x < 16384) { unsigned long long *tr__ = g_scan_trace + 4 * blockIdx.x; tr__[0] = w_first__; tr__[1] = wall_clock64(); \
        tr__[2] = clock64() - t_first__; \
        tr__[3] = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32); } } } while (0)
#define SQA_ADD(i, v) do { if ((threadIdx.x & 63) == 0) atomicAdd(&ck.dbg[i], (unsigned long long)(v)); } while (0)  // LDS; flushed once per workgroup
#define SQA_SET(i, v) do { if ((threadIdx.x & 63) == 0) ck.dbg[i] += (unsigned long long)(v); } while (0)
#define SQA_NOW() clock64()
#else
#define SQA_SET(i, v) do { } while (0)
#define SQA_ADD(i, v) do { } while (0)
#define SQA_NOW() 0ll
#define SQ_T(i) do { } while (0)
#define SQ_T0() do { } while (0)
#define SQ_TEND() do { } while (0)
#endif
constexpr int SQ_QT = 8;
constexpr int SQ_CAP = 238;   // two workgroups per CU: (81920 - 65536 table - ~1 KB control) / 8 queries / 8 bytes
constexpr int SQ_TRIG = 192;
constexpr int SQ_MAXSUM = 32766;

struct QuantParams {
    union {
        float mn[SQ_QT][16];          // per (query, sub-quantiser) minimum finite table entry
        uint32_t mn_bits[SQ_QT][16];  // same words while the minimum is being reduced (non-negative floats)
    };
    float inv_scale[SQ_QT];
    double scale_eff[SQ_QT];  // 1 / inv_scale, the scale the integers are really in
    double bias[SQ_QT];       // sum_m mn[m]
    uint32_t slack[SQ_QT];    // lazy selection: a row whose integer sum is >= (k-th smallest integer sum) + slack is out (0 = not usable)
};

struct QuantThr {
    const QuantParams *qp;
    __device__ __forceinline__ uint32_t operator()(int q, uint32_t t) const
    {
        if (t >= 0x7f800000u) return 32767u;  // no finite threshold yet: every sum (<= 32766) passes
        const double x = ((double)__uint_as_float(t) * (1.0 + 1e-6) - qp->bias[q]) / qp->scale_eff[q];
        if (!(x > 0.0)) return 2u;
        const double f = floor(x) + 2.0;
        return f > 32767.0 ? 32767u : (uint32_t)f;
    }
};

// ---- the table rule: every later stage trusts this arithmetic (why the sums are lower bounds: adc_scan.hip ahead of adc_scan16q_kernel;
// the band of the lazy selection: scan_compact_lazy_q below) -----------------------------------------------------------------------
// Query q's parameters from the collected ranges of its MP real tables (qp.mn_bits / mx_bits hold the minimum / maximum finite entry of
// each table as float bits): per-table minimum, one scale over the sum of the ranges such that sum_m max_j qv <= SQ_MAXSUM, the bias,
// and the band of the lazy selection (scan_compact_lazy_q; derived for sixteen entries of two units each, MP entries need less) --
// usable when every entry is finite and the band stays narrow.  One thread per query; returns whether the query may select lazily
// (the same as qp.slack != 0).
template <int MP>
__device__ __forceinline__ bool scan16_query_params(QuantParams &qp, const uint32_t (*mx_bits)[16], int q, int lazy_on, const int *nonfinite)
{
    float range = 0.0f;
    double bias = 0.0;
    for (int m = 0; m < MP; ++m) {
        uint32_t lo = qp.mn_bits[q][m], hi = mx_bits[q][m];
        if (lo > hi) { lo = 0u; hi = 0u; }  // no finite entry at all
        const float fl = __uint_as_float(lo), fh = __uint_as_float(hi);
        qp.mn[q][m] = fl;
        range += fh - fl;
        bias += (double)fl;
    }
    float scale = range > 0.0f ? range / (float)SQ_MAXSUM * 1.001f : 1.0f;
    if (!(scale > 1e-37f)) scale = 1e-37f;
    const float inv = 1.0f / scale;
    qp.inv_scale[q] = inv;
    qp.scale_eff[q] = 1.0 / (double)inv;
    qp.bias[q] = bias;
    const double sl = 34.0 + ceil(4e-6 * (32767.0 + bias * (double)inv));
    const bool lazy_ok = lazy_on && !nonfinite[q] && sl < 1024.0 && bias >= 0.0;
    qp.slack[q] = lazy_ok ? (uint32_t)sl : 0u;
    return lazy_ok;
}
// One entry: qv = clamp(floor((v - min_m) * inv) - 1, 0, SQ_MAXSUM), a lower bound of (v - min_m) in table units; a non-finite
// entry -> 0 (a lower bound of anything).  (qp by reference: its two LDS reads stay inside the finite-entry branch.)
__device__ __forceinline__ uint32_t scan16_quantise(float v, const QuantParams &qp, int q, int m)
{
    int iv = 0;
    if (__float_as_uint(v) < 0x7f800000u) {
        const float f = __fmul_rn(__fsub_rn(v, qp.mn[q][m]), qp.inv_scale[q]);
        iv = (int)floorf(f) - 1;
        iv = iv < 0 ? 0 : (iv > SQ_MAXSUM ? SQ_MAXSUM : iv);
    }
    return (uint32_t)iv;
}

// The QT queries' tables of `group`, quantised into LDS: lut[code j][slot][q] u16, with the per-query scale / bias /
// lazy-selection parameters in qp.  MP = the model's real tables (range and bias run over these only); the sixteen 16-byte slots of a
// code value hold 16 / MP copies of them, copy c of sub-space m at slot m + MP c (adc_scan16p's packed rows; MP = 16: slot = m).
// mx_bits = QT x 16 words of scratch; nonfinite / lazy = QT flags each.  Called by the whole workgroup; ends with a barrier.
template <int NT, int MP = 16>
__device__ __forceinline__ void scan16q_build_tables(const ScanArgs &a, int group, uint32_t *lut, QuantParams &qp, uint32_t (*mx_bits)[16],
                                                     int *nonfinite, int *lazy)
{
    constexpr int QT = SQ_QT;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < QT * 16) {
        qp.mn_bits[tid >> 4][tid & 15] = 0x7f7fffffu;  // FLT_MAX
        mx_bits[tid >> 4][tid & 15] = 0u;
    }
    if (tid < QT) nonfinite[tid] = 0;
    __syncthreads();
    // fp32 table entries of (m, j) for the QT queries, from the per-query tables a.lut_g
    // (lut_kernel: IVFOPQ.cpp:279-291); lanes walk consecutive j -> coalesced
    int qis[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        const int qi = group * QT + q;
        qis[q] = qi < a.nq ? qi : a.nq - 1;
    }
    auto entry = [&](int m, int j, float (&acc)[QT]) {
#pragma unroll
        for (int q = 0; q < QT; ++q)
            acc[q] = a.lut_g[((int64_t)qis[q] * 16 + m) * 256 + j];  // padded with +inf past K
    };
    // pass A: per (query, m) range of the finite entries (a wave covers 64 consecutive j of one m)
    for (int e = tid; e < MP * 256; e += NT) {
        const int m = e >> 8, j = e & 255;
        float acc[QT];
        entry(m, j, acc);
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            const uint32_t bits = __float_as_uint(acc[q]);
            uint32_t lo = bits < 0x7f800000u ? bits : 0x7f7fffffu;  // non-finite: ignored
            uint32_t hi = bits < 0x7f800000u ? bits : 0u;
            if (__ballot(bits >= 0x7f800000u) != 0 && lane == 0) nonfinite[q] = 1;  // (the +inf padding past K counts: a code >= K reaches it)
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const uint32_t l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
            if (lane == 0) {
                atomicMin(&qp.mn_bits[q][m], lo);
                atomicMax(&mx_bits[q][m], hi);
            }
        }
    }
    __syncthreads();
    if (tid < QT) lazy[tid] = scan16_query_params<MP>(qp, mx_bits, tid, a.lazy, nonfinite) ? 1 : 0;
    __syncthreads();
    // pass B: quantise every slot
    for (int e = tid; e < 16 * 256; e += NT) {
        const int slot = e >> 8, j = e & 255, m = slot & (MP - 1);
        float acc[QT];
        entry(m, j, acc);
        uint32_t qv[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) qv[q] = scan16_quantise(acc[q], qp, q, m);
        *reinterpret_cast<uint4 *>(&lut[(j * 16 + slot) * (QT / 2)]) =
            make_uint4(qv[0] | (qv[1] << 16), qv[2] | (qv[3] << 16), qv[4] | (qv[5] << 16), qv[6] | (qv[7] << 16));
    }
    __syncthreads();  // tables ready; the scratch words are dead from here on
}

// exact reference-order distance of (row, query): sum over m ascending of the fp32 table entries
// (IVFOPQ.cpp:302-306) gathered from the per-query tables in HBM -- 16 independent loads.
struct ExactFromLut {
    static constexpr bool enabled = true;
    const uint4 *rows;
    const float *lut_g;
    int K, nq, group;
    __device__ __forceinline__ unsigned long long operator()(int q, unsigned long long e) const
    {
        const uint32_t row = (uint32_t)e;
        const uint4 c = rows[row];
        const uint32_t w[4] = { c.x, c.y, c.z, c.w };
        int qi = group * SQ_QT + q;
        qi = qi < nq ? qi : nq - 1;
        const float *t = lut_g + (int64_t)qi * 16 * 256;
        float v[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const int j = (int)((w[m >> 2] >> (8 * (m & 3))) & 0xffu);
            v[m] = t[m * 256 + j];  // padded with +inf past K
        }
        float s = 0.0f;
#pragma unroll
        for (int m = 0; m < 16; ++m) s = __fadd_rn(s, v[m]);
        return ((unsigned long long)__float_as_uint(s) << 32) | row;
    }
};

// ascending bitonic sort of n (a power of two) 64-bit keys in LDS by the whole workgroup of NT threads
template <int NT>
__device__ __forceinline__ void block_bitonic_u64(unsigned long long *e, int n)
{
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n / 2; i += NT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;   // lo = (i / stride) * 2 stride + i % stride
                const bool up = (lo & size) == 0;
                const unsigned long long a0 = e[lo], a1 = e[hi];
                if ((a0 > a1) == up) { e[lo] = a1; e[hi] = a0; }
            }
        }
    }
    __syncthreads();
}

// batched form for the register compaction: up to 4 entries per lane, all row loads first, then all
// 4 MP table gathers, then the in-order sums -- two dependent memory round trips per batch instead of 2 x 4.
// Rows of MP code bytes (16: one 16-byte load); tables [nq][16][256] fp32 of which the first MP belong to the model.
template <int MP = 16>
struct ExactFromLutBatch {
    const void *rows;
    const float *lut_g;
    int K, nq, group;
    __device__ __forceinline__ void operator()(int q, unsigned long long (&e)[4], const bool (&need)[4]) const
    {
        int qi = group * SQ_QT + q;
        qi = qi < nq ? qi : nq - 1;
        const float *t = lut_g + (int64_t)qi * 16 * 256;
        uint32_t c[4][MP / 4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t row = need[r] ? (uint32_t)e[r] : 0u;
            if constexpr (MP == 16) {
                const uint4 c4 = static_cast<const uint4 *>(rows)[row];
                c[r][0] = c4.x; c[r][1] = c4.y; c[r][2] = c4.z; c[r][3] = c4.w;
            } else {
                const uint32_t *p = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(rows) + (size_t)row * MP);
#pragma unroll
                for (int w = 0; w < MP / 4; ++w) c[r][w] = p[w];
            }
        }
#pragma unroll
        for (int h = 0; h < 4; h += 2) {  // two entries at a time: 2 MP gathers in flight
            if (__ballot(need[h] || need[h + 1]) == 0) continue;  // wave-uniform: nothing to fix in this pair
            float v[2][MP];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int m = 0; m < MP; ++m) {
                    const int j = (int)((c[h + r][m >> 2] >> (8 * (m & 3))) & 0xffu);
                    // (a predicated gather made hipcc wait vmcnt(0) after every one of the 64 loads:
                    //  64 serialized memory round trips, 14 us per compaction)
                    v[r][m] = t[m * 256 + j];  // scratch tables are padded to 256 entries (+inf past K): no predicate
                }
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float s = 0.0f;
#pragma unroll
                for (int m = 0; m < MP; ++m) s = __fadd_rn(s, v[r][m]);
                if (need[h + r]) e[h + r] = ((unsigned long long)__float_as_uint(s) << 32) | (uint32_t)e[h + r];
            }
        }
    }
};

typedef unsigned short cvt_us2 __attribute__((ext_vector_type(2)));
typedef short cvt_s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_add_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (cvt_us2)(__builtin_bit_cast(cvt_us2, a) + __builtin_bit_cast(cvt_us2, b)));
}
__device__ __forceinline__ uint32_t pk_sub_i16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, (cvt_s2)(__builtin_bit_cast(cvt_s2, a) - __builtin_bit_cast(cvt_s2, b)));
}

// ---- lazy selection (intermediate compactions of adc_scan16q) -----------------------------------------------------------
// The integer sum S of a row is a two-sided bound of its real table sum D in table units u = (D - bias) / scale_eff:
//     S <= u < S + 32.01        (each entry: qv = max(0, floor(f) - 1), f = fl((v - mn) * inv) within 2^-22 of (v - mn) / scale_eff)
// and the reference's fp32 sum d_ref is within 15 rounding steps (9e-7 relative) of D.  Let S_k be the k-th smallest S seen
// so far.  A row with S >= S_k + slack, slack = 34 + ceil(4e-6 * (32767 + bias / scale_eff)), has
//     D >= bias + scale (S_k + slack)  >  (bias + scale (S_k + 32.01)) (1 + 2e-6)  >  D_i (1 + 2e-6)   for each of the k rows i with S_i <= S_k,
// hence d_ref > d_ref,i for k rows: it is not among the k smallest (distance, id) pairs, ties included.  So between checkpoints
// the buffer only needs the integer keys: keep every entry with S < T = S_k + slack (k plus the few rows within `slack` units
// of the k-th), push under the same T, and compute exact reference-order sums ONCE, in the final compaction (entries keep
// exact_n = 0, so the final pass re-sums all of them).  The two dependent memory round trips of the exact re-sum leave every
// intermediate compaction.  If the band [S_k, S_k + slack) is crowded (more than `keep_max` entries stay), the query switches to
// the exact-key protocol for the rest of the scan: its entries are re-summed now and from then on it is compacted by
// topk_compact_wave_q.  Queries whose tables hold non-finite entries never start lazy (slack = 0): S is no upper bound there.
template <int QT, int CAP, class FixB, class ThrX>
__device__ __attribute__((noinline)) int scan_compact_lazy_q(TopKShared<QT, CAP> &s, int q, int k, const FixB &fixb, const ThrX &thrx,
                                                            uint32_t slack, int keep_max, int *lazy_flag, int n_in = -1)
{
    static_assert(CAP <= 256, "register selection holds 256 entries per wave");
    constexpr int NR = CAP <= 64 ? 1 : (CAP <= 128 ? 2 : 4);
    const int lane = threadIdx.x & 63;
    unsigned long long *b = s.buf[q];
    int n = n_in >= 0 ? n_in : s.cnt[q];
    n = n < CAP ? n : CAP;
    unsigned long long e[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int p = r * 64 + lane;
        e[r] = p < n ? b[p] : ~0ull;
    }
    if (n < k) {  // fewer than k rows seen: everything stays where it is, every sum passes
        if (lane == 0) { s.exact_n[q] = 0; s.thr[q] = KEY_MAX; s.thr_x[q] = 32767u; }
        return n;
    }
    const uint32_t T = wave_select_field<NR, 15>(e, k) + slack;  // the k-th smallest integer sum (sums are below 2^15) + the band
    int total = 0;
    unsigned long long in_m[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        in_m[r] = __ballot((uint32_t)(e[r] >> 32) < T);  // empty slots carry 0xffffffff: never in
        total += __popcll(in_m[r]);
    }
    if (total <= keep_max) {  // wave-uniform
        int base = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const bool in = (in_m[r] >> lane) & 1ull;
            const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(in_m[r] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)in_m[r], 0u));
            if (in) b[pos] = e[r];
            base += __popcll(in_m[r]);
        }
        if (lane == 0) { s.exact_n[q] = 0; s.thr[q] = KEY_MAX; s.thr_x[q] = T < 32767u ? T : 32767u; }
        return total;
    }
    // crowded band: this query leaves the lazy protocol -- exact keys for everything it holds, then the ordinary selection
    bool need[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) need[r] = r * 64 + lane < n;
    fixb(q, e, need);
    const unsigned long long kx = wave_select<NR>(e, k);
    int base = 0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const bool in = e[r] <= kx;
        const unsigned long long m = __ballot(in);
        const int pos = base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (in && pos < k) b[pos] = e[r];
        base += __popcll(m);
    }
    if (lane == 0) {
        *lazy_flag = 0;
        s.exact_n[q] = k;
        s.thr[q] = (uint32_t)(kx >> 32);
        s.thr_x[q] = thrx(q, (uint32_t)(kx >> 32));
    }
    return k;
}

// the 16 look-ups of one row: packed 15-bit sums of the SQ_QT queries, two per word -- they can never carry across the 16-bit
// halves, so they are accumulated with plain 32-bit adds, two look-ups per v_add3_u32 (half the VALU of v_pk_add_u16).  Integer
// sums, any order.  NG look-ups are in flight at a time: 16 in adc_scan16q; adc_scan16a takes groups of four -- there the scheduler
// would otherwise form all 16 addresses first, more registers than its waves have left.
// BIASED: the sums start from s0 .. s3 as passed in instead of zero (adc_scan16q: 0x8000 - T per 16-bit field, so that "sum < T" is a
// CLEAR bit 15 and the test of a row is an AND over the four words instead of four packed subtractions; sum + 0x8000 - T < 2^16: still no carry)
template <bool PREROT, int NG = 4, bool BIASED = false>
__device__ __forceinline__ void scan16q_row_sums(const uint4 &row, const uint32_t (&moffp)[4], uint32_t cr8, uint32_t cq, const char *lut_b,
                                                 uint32_t &s0, uint32_t &s1, uint32_t &s2, uint32_t &s3)
{
    uint32_t d0 = row.x, d1 = row.y, d2 = row.z, d3 = row.w;
    if constexpr (!PREROT) {
        d0 = __builtin_amdgcn_alignbit(row.y, row.x, cr8);
        d1 = __builtin_amdgcn_alignbit(row.z, row.y, cr8);
        d2 = __builtin_amdgcn_alignbit(row.w, row.z, cr8);
        d3 = __builtin_amdgcn_alignbit(row.x, row.w, cr8);
        const bool b0 = cq & 1;
        const uint32_t e0 = b0 ? d1 : d0, e1 = b0 ? d2 : d1, e2 = b0 ? d3 : d2, e3 = b0 ? d0 : d3;
        const bool b1 = cq & 2;
        d0 = b1 ? e2 : e0; d1 = b1 ? e3 : e1; d2 = b1 ? e0 : e2; d3 = b1 ? e1 : e3;
    }
    const uint32_t rot[4] = { d0, d1, d2, d3 };
    if constexpr (!BIASED) { s0 = 0; s1 = 0; s2 = 0; s3 = 0; }
#pragma unroll
    for (int h = 0; h < 16 / NG; ++h) {
        uint4 v[NG];
#pragma unroll
        for (int t = 0; t < NG; ++t) {
            const int tt = NG * h + t;
            const uint32_t sel = 0x0c0c0000u | ((4u + (tt & 3)) << 8) | (uint32_t)(tt & 3);
            const uint32_t addr = __builtin_amdgcn_perm(rot[tt >> 2], moffp[tt >> 2], sel);  // code*256 + m*16
            v[t] = *reinterpret_cast<const uint4 *>(lut_b + addr);
        }
#pragma unroll
        for (int t = 0; t < NG; t += 2) {
            s0 = s0 + v[t].x + v[t + 1].x; s1 = s1 + v[t].y + v[t + 1].y;
            s2 = s2 + v[t].z + v[t + 1].z; s3 = s3 + v[t].w + v[t + 1].w;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The threshold half of a seed: wave q turns query q's histogram (256 bins of 128 table units) into a first threshold.  The first bin b
// at which the cumulative count reaches k proves k rows with sum < (b + 1) << 7; queries that cannot select lazily keep what they have.
__device__ __forceinline__ void scan16_seed_threshold(int k, const uint32_t *hist, const QuantParams &qp, const int *lazy, uint32_t *thr_x, uint32_t *thr_pk)
{
    constexpr int QT = SQ_QT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < QT && lazy[wave]) {
        const int q = wave;
        uint32_t c4[4], mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { c4[j] = hist[q * 256 + lane * 4 + j]; mine += c4[j]; }
        uint32_t incl = mine;  // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        const unsigned long long reach = __ballot(incl >= (uint32_t)k);
        if (reach) {  // wave-uniform
            const int l0 = __ffsll((long long)reach) - 1;
            if (lane == l0) {
                uint32_t cum = incl - mine;
                int b = lane * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    cum += c4[j];
                    if (cum >= (uint32_t)k) { b = lane * 4 + j; break; }
                }
                uint32_t t = ((uint32_t)(b + 1) << 7) + qp.slack[q];
                t = t < 32767u ? t : 32767u;
                const uint32_t have = thr_x[q];  // what the other row splits have established already
                t = have < t ? have : t;
                thr_x[q] = t;
                reinterpret_cast<uint16_t *>(thr_pk)[q] = (uint16_t)t;
            }
        }
    }
}

// Seed: a first filter threshold per query from a histogram of the split's first SQ_SEED_CHUNKS x 64 rows.
// Without it a scan starts with "every row passes": a thousand rows in flight against SQ_CAP slots, and four to five rounds of
// the whole workgroup waiting for compactions before the pass rate has fallen.  bin = sum >> 7; the first bin b at which the
// cumulative count reaches k proves k rows with sum < (b + 1) << 7 =: S, hence S_k <= S, and T = S + slack is a valid (looser)
// lazy-selection threshold (scan_compact_lazy_q).  Queries that cannot select lazily keep "pass all".  The seed rows are
// scanned again by the main loop.  hist = SQ_QT x 256 words (the still unused selection buffers).  Whole workgroup; ends with a barrier.
constexpr uint32_t SQ_SEED_CHUNKS = 32;
template <int NT, bool PREROT, class LoadRow>
__device__ __forceinline__ void scan16q_seed(int k, const LoadRow &load64, const uint32_t (&moffp)[4], uint32_t cr8, uint32_t cq, const char *lut_b,
                                             uint32_t *hist, const QuantParams &qp, const int *lazy, uint32_t *thr_x, uint32_t *thr_pk)
{
    constexpr int QT = SQ_QT, NW = NT / 64;
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < QT * 256; i += NT) hist[i] = 0;
    __syncthreads();
    for (uint32_t ch = wave; ch < SQ_SEED_CHUNKS; ch += NW) {
        const uint4 row = load64(ch);
        uint32_t sm[4];
        scan16q_row_sums<PREROT>(row, moffp, cr8, cq, lut_b, sm[0], sm[1], sm[2], sm[3]);
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            const uint32_t sq = (sm[q >> 1] >> (16 * (q & 1))) & 0xffffu;
            atomicAdd(&hist[q * 256 + (sq >> 7)], 1u);
        }
    }
    __syncthreads();
    scan16_seed_threshold(k, hist, qp, lazy, thr_x, thr_pk);
    __syncthreads();
}

// ---- the workgroup frame of adc_scan16q / adc_scan16p / adc_scan16a: everything around their look-up loops ------------------------------
using ScanTopK = TopKShared<SQ_QT, SQ_CAP>;

// block -> (query group, row split) of the two-region plan (kernels.h).  A region whose split count is a multiple of 8 keeps a row
// split on one XCD (block b runs on XCD b % 8), so each XCD's L2 only ever caches 1/8 of the code matrix.
struct ScanBlock {
    int group, split, my_splits;
    int64_t my_rps;  // rows per split of this block's region
};
__device__ __forceinline__ ScanBlock scan16_block(const ScanArgs &a)
{
    int group, split, my_splits = a.splits;
    int64_t my_rps = a.rows_per_split;
    int b = blockIdx.x, g0 = 0;
    if (b >= a.groups_a * a.splits) {  // region B: the tail groups, split finer (dispatched last)
        b -= a.groups_a * a.splits;
        g0 = a.groups_a;
        my_splits = a.splits_b;
        my_rps = a.rows_per_split_b;
    }
    if ((my_splits & 7) == 0) {
        const int s8 = my_splits >> 3;
        const int xcd = b & 7, i = b >> 3;
        split = xcd + 8 * (i % s8);
        group = g0 + i / s8;
    } else {
        split = b % my_splits;
        group = g0 + b / my_splits;
    }
    return { group, split, my_splits, my_rps };
}

// a.only (the matrix-core route's fall-back, adc_mfma.hip): does any query of `group` still want its answer?  Workgroup-uniform.
// adc_scan16q_kernel alone honours the predicate; the launches of the other forms refuse it.
__device__ __forceinline__ bool scan16_group_wanted(const ScanArgs &a, int group)
{
    uint32_t any = 0u;
    for (int q = 0; q < SQ_QT; ++q)
        if (group * SQ_QT + q < a.nq) any |= a.only[group * SQ_QT + q];
    return any != 0u;
}

// first thresholds: pass-all until k rows are known -- or what the other row splits of these queries have already established
__device__ __forceinline__ void scan16_init_thresholds(const ScanArgs &a, int group, int tid, ScanTopK &tk, uint32_t (&thr_pk)[SQ_QT / 2])
{
    if (tid < SQ_QT / 2) {
        uint32_t t2[2] = { 32767u, 32767u };
        if (a.gthr) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int qi = group * SQ_QT + 2 * tid + h;
                if (qi < a.nq) {  // a stale value is an older, looser, still valid bound
                    const uint32_t g = __hip_atomic_load(&a.gthr[qi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    t2[h] = g < t2[h] ? g : t2[h];
                }
            }
        }
        tk.thr_x[2 * tid] = t2[0]; tk.thr_x[2 * tid + 1] = t2[1];
        thr_pk[tid] = t2[0] | (t2[1] << 16);
    }
}

// Chunks are handed out dynamically, in PAIRS (2 p, 2 p + 1): one LDS atomic per two chunks, the odd one follows without asking.
// next_chunk_addr = the LDS address of the workgroup's counter.  Wave-uniform result.
// (the atomic is spelled out: for `if (lane == 0) atomicAdd(...)` hipcc emits its wave-aggregation sequence -- two mbcnt, a
//  compare, a population count and two moves -- around the one-lane atomic: 6 of the loop's 66 vector instructions per row)
__device__ __forceinline__ uint32_t scan16_grab_pair(uint32_t next_chunk_addr, int lane)
{
    uint32_t v;
    asm volatile("" : "=v"(v));  // (only lane 0's value is read: no instruction to define the others)
    if (lane == 0) asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(next_chunk_addr), "v"(1u) : "memory");
    return 2u * (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
// the chunk after `chunk`: its pair's second half, or a new pair (wave-uniform branch)
__device__ __forceinline__ uint32_t scan16_after(uint32_t chunk, uint32_t next_chunk_addr, int lane)
{
    return (chunk & 1u) ? scan16_grab_pair(next_chunk_addr, lane) : chunk + 1u;
}

// the rare path of a row: this lane's row (lrow within the split) goes to the buffer of every query whose plain sum lies under its
// threshold.  Bit done_bit0 + q of `done` remembers what was stored already (a chunk is walked again after a full buffer).
// Returns true when a buffer was full.  (`done` is worked on in a local copy: written through the reference inside the loop, hipcc
// keeps the bits in a branch and the failure in a select -- the other way round than before, and with it another look-up loop.)
__device__ __forceinline__ bool scan16_push_candidates(ScanTopK &tk, const uint32_t (&sums)[4], const uint32_t (&tpk)[SQ_QT / 2], int64_t row_begin,
                                                       uint32_t lrow, int done_bit0, uint32_t &done_io)
{
    uint32_t done = done_io;
    bool failed = false;
#pragma unroll
    for (int q = 0; q < SQ_QT; ++q) {
        const uint32_t bit = 1u << (done_bit0 + q);
        const uint32_t sq = (sums[q >> 1] >> (16 * (q & 1))) & 0xffffu;
        const uint32_t tq = (tpk[q >> 1] >> (16 * (q & 1))) & 0xffffu;
        if (sq < tq && !(done & bit)) {
            bool dummy = false;
            if (topk_push<SQ_QT, SQ_CAP, SQ_TRIG>(tk, q, sq, (uint32_t)(row_begin + lrow), dummy)) done |= bit;
            else failed = true;
        }
    }
    done_io = done;
    return failed;
}

// The compactions of a checkpoint, between its two barriers: one wave per query, in registers; the row splits of a query tighten each
// other's filter through a.gthr (same tables -> same units); then the packed thresholds of the loop are renewed and `stop` is cleared.
// Whole workgroup.
template <int NT, class FixB>
__device__ __forceinline__ void scan16_checkpoint_compact(const ScanArgs &a, int group, ScanTopK &tk, const QuantParams &qp, int (&lazy)[SQ_QT],
                                                          uint32_t (&thr_pk)[SQ_QT / 2], int &stop, const FixB &fixb, const QuantThr &thrx)
{
    constexpr int QT = SQ_QT, NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int keep_max = a.k + 48 < SQ_TRIG - 24 ? a.k + 48 : SQ_TRIG - 24;
    for (int q = wv; q < QT; q += NW) {  // wave-uniform
        const int keep = lazy[q] ? scan_compact_lazy_q<QT, SQ_CAP>(tk, q, a.k, fixb, thrx, qp.slack[q], keep_max, &lazy[q])
                                 : topk_compact_wave_q<QT, SQ_CAP, false>(tk, q, a.k, fixb, thrx);
        if (lane == 0) {
            tk.cnt[q] = keep;
            if (a.gthr) {
                const int qi = group * QT + q;
                if (qi < a.nq) {
                    const uint32_t mine = tk.thr_x[q];
                    const uint32_t seen = atomicMin(&a.gthr[qi], mine);
                    tk.thr_x[q] = seen < mine ? seen : mine;
                }
            }
        }
    }
    __syncthreads();
    if (tid < QT / 2) thr_pk[tid] = tk.thr_x[2 * tid] | (tk.thr_x[2 * tid + 1] << 16);
    if (tid == 0) stop = 0;
}

// Epilogue: the workgroup's lists to its partial slot [qi][split] -- or, IN_PLACE (adc_scan16q / 16p), a group of the first region
// that was scanned in one piece holds its queries' final lists: they go where the caller wants them (a.out_d is only set when that
// region has one split).  A region with fewer splits than the partial stride leaves the other slots empty for the merge.
template <int NT, bool IN_PLACE>
__device__ __forceinline__ void scan16_write_lists(const ScanArgs &a, const ScanTopK &tk, int group, int split, int my_splits)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < SQ_QT; ++q) {
        const int qi = group * SQ_QT + q;
        if (qi >= a.nq) break;
        const int cnt = tk.cnt[q];
        const bool in_place = IN_PLACE ? a.out_d != nullptr && group < a.groups_a : false;
        float *const pd = in_place ? a.out_d : a.part_d;
        int64_t *const pi = in_place ? a.out_id : a.part_id;
        const int64_t o = in_place ? (int64_t)qi * a.k : ((int64_t)qi * a.stride + split) * a.k;
        for (int i = tid; i < a.k; i += NT) {
            if (i < cnt) {
                const unsigned long long e = tk.buf[q][i];
                pd[o + i] = __uint_as_float((uint32_t)(e >> 32));
                pi[o + i] = a.id_base + (int64_t)(uint32_t)e;
            } else {
                pd[o + i] = __uint_as_float(0x7f800000u);
                pi[o + i] = -1;
            }
        }
        if (!in_place && split == 0 && my_splits < a.stride) {
            const int64_t o2 = ((int64_t)qi * a.stride + my_splits) * a.k;
            for (int i = tid; i < (a.stride - my_splits) * a.k; i += NT) {
                a.part_d[o2 + i] = __uint_as_float(0x7f800000u);
                a.part_id[o2 + i] = -1;
            }
        }
    }
}

}  // namespace cvtmi
