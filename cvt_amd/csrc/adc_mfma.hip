// adc_mfma.hip -- large M = 16 ADC batches as a bound filter on v_mfma_i32_32x32x32_i8.  The M = 16 scan is bound by the
// LDS look-up rate; here the (row, query) work is one int8 dot product over the DECODED rows instead.  An ADC sum is the squared distance
// of the query residual r to the decoded row x^ (its sixteen codewords): |r - x^|^2 = |r|^2 + |x^|^2 - 2 r.x^.
//   per index (from the codebooks): centre c and scale s = range / 254 per dimension; per row X = round((x^ - c) / s) as int8 in
//     launch_flat_u8_pack's layout and n^ = |x^|^2 (fp32, rounded up): 132 bytes per row;
//   per call: w = r (.) s, ONE scale t = max |w| / 127, W = round(w / t), delta = w / t - W, and B(row) = floor(n^ / 2t);
//   the filter kernels of flat_u8_tfilter.hip give a = W.X - B per (row, query), an exact integer, with
//       d_ref in C_q - 2 t a +- E_q,   C_q = |r|^2 - 2 r.c,   E_q = 2 (t |delta| X_max + |w| eps_max) + 4 t + fp
//     (X_max >= |X(row)|, eps_max >= |(x^ - c) / s - X(row)|, fp: the reference's own fp32 evaluation of the sum);
//   sample pass: the k-th largest A of the maxima of a over disjoint row sets is reached by k rows, all with d_ref <= C_q - 2 t A + E_q, so
//     a row of the answer has a >= A - E_q / t: the threshold is A - ceil(E_q / t) - 1;
//   filter pass + bucket: the rows at or above it, per query; selection: their exact sums in the reference's order from the fp32 tables
//     (ExactFromLut), sorted by (distance, id) -- the answer is the reference's, bit for bit.
// A query that is not finite, whose sample filled fewer than 1.25 k slots, whose margin cannot be held or whose list ran over raises ITS
// flag; a record region that ran over flags the queries of its chunk (the 256 or fewer whose records it holds).
// Flagged queries: up to MF_REDO of them take a slot and are answered here by the same scheme in exact fp32 over ALL rows (mf_redo_*: the
// k-th smallest of the exact minima over disjoint row sets is a bound tau on the k-th distance, the rows at or below tau are listed, the
// list is ranked); the others, and a slot whose list ran over or met a NaN, are left to the caller's exact scan through rest[q].
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "common.h"
#include "flat_f32_common.h"
#include "adc_scan16.h"
#include "kernels.h"
#include "launch.h"

namespace cvtmi {

namespace {

constexpr double MF_UP = 1.0 + 1e-9;        // every bound is rounded up by this much: the double arithmetic that evaluates it
constexpr double MF_BMAX = 4194304.0;       // floor(n^ / 2t) stays below 2^22: the accumulators stay far inside int32 and n^ - |x^|^2 <= t
constexpr int MF_NSEL = 4096;               // the largest list cap: 64 entries per lane of the selecting wave
constexpr int MF_NSHORT = 1024;             // lists of up to so many entries take the short form of the selection (16 entries per lane), longer ones the long form's launch
constexpr int MF_KEEP = 512;                // rows at or below the k-th distance the selection sorts (k + its ties; more: the exact scan)
constexpr int MF_CALL_WORDS = 64;           // [0] bits of max |w|, [63] the count of flagged queries
constexpr int MF_REDO = 64;                 // flagged queries that get a slot of the exact redo (its list: MF_NSHORT entries)
constexpr int MF_REDO_SLICES = 256;         // row slices of the redo's passes at most, one workgroup per slice and slot ...
constexpr int MF_REDO_SETS = 16 * MF_REDO_SLICES;   // ... each with one row set per 16 lanes: set minima per slot

// [tile][s][lane] 16 bytes: row 32 t + (lane & 31), dimensions 32 s + 16 (lane >> 5) .. + 16 of its decoded int8 row
__global__ __launch_bounds__(kBlock) void mf_pack_kernel(const uint4 *__restrict__ codes, int64_t n, int ks, int step, const int8_t *__restrict__ xb,
                                                         int64_t tile0, int64_t ntiles, uint4 *__restrict__ pack)
{
    const int64_t g = tile0 * ks * 64 + (int64_t)blockIdx.x * kBlock + threadIdx.x;   // tiles [tile0, ntiles)
    if (g >= ntiles * ks * 64) return;
    const int lane = (int)(g & 63);
    const int64_t ts = g >> 6, t = ts / ks;
    const int s_ = (int)(ts - t * ks);
    const int64_t row = t * 32 + (lane & 31);
    uint32_t w[4] = { 0u, 0u, 0u, 0u };   // rows past n: X = 0 (they start at a value no threshold reaches)
    if (row < n) {
        const uint4 cv = codes[row];
        const int d0 = 32 * s_ + 16 * (lane >> 5);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int d = d0 + e, m = d / step, kk = d - m * step;
            const uint32_t word = (m >> 2) == 0 ? cv.x : ((m >> 2) == 1 ? cv.y : ((m >> 2) == 2 ? cv.z : cv.w));
            const uint32_t code = (word >> (8 * (m & 3))) & 0xffu;
            w[e >> 2] |= (uint32_t)(uint8_t)xb[((size_t)m * 256 + code) * step + kk] << (8 * (e & 3));
        }
    }
    pack[g] = make_uint4(w[0], w[1], w[2], w[3]);
}

// n^(row) = |x^|^2 as fp32, rounded up
__global__ __launch_bounds__(kBlock) void mf_norm_kernel(const uint4 *__restrict__ codes, int64_t row0, int64_t n, const double *__restrict__ nrm,
                                                         float *__restrict__ norms)
{
    const int64_t row = row0 + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= n) return;
    const uint4 cv = codes[row];
    const uint32_t cw[4] = { cv.x, cv.y, cv.z, cv.w };
    double s_ = 0.0;
#pragma unroll
    for (int m = 0; m < 16; ++m) s_ += nrm[m * 256 + ((cw[m >> 2] >> (8 * (m & 3))) & 0xffu)];
    norms[row] = __double2float_ru(s_ * (1.0 + 1e-12));
}

__device__ __forceinline__ double mf_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per query: is it finite, and its max |w| (bits of a non-negative fp32, rounded up; 0 when it is not) into wq[q]
__global__ __launch_bounds__(256) void mf_qmax_kernel(const float *__restrict__ q_rot, const float *__restrict__ centroid, const float *__restrict__ s, int D, int nq,
                                                      uint32_t *__restrict__ wq, uint32_t *__restrict__ flags)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= nq) return;
    float mx = 0.0f;
    bool fin = true;
    for (int d = lane; d < D; d += 64) {
        const float r = __fsub_rn(q_rot[(int64_t)q * D + d], centroid[d]);   // the residual the reference's tables are built from
        if (!(fabsf(r) <= FLT_MAX)) fin = false;
        const float w = __double2float_ru(fabs((double)r * (double)s[d]));
        mx = w > mx ? w : mx;
    }
    fin = __ballot(!fin) == 0ull;
    const uint32_t bits = fs_wave_max_u32(__float_as_uint(fin ? mx : 0.0f));
    if (lane == 0) {
        flags[q] = fin ? 0u : 1u;
        wq[q] = bits;
    }
}
// ... and the largest of them into call[0], by one workgroup (ten thousand waves on one word cost more than the rest of the query side)
__global__ __launch_bounds__(1024) void mf_qred_kernel(const uint32_t *__restrict__ wq, int nq, uint32_t *__restrict__ call)
{
    __shared__ uint32_t part[16];
    uint32_t mx = 0u;
    for (int q = threadIdx.x; q < nq; q += 1024) mx = wq[q] > mx ? wq[q] : mx;
    mx = fs_wave_max_u32(mx);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) mx = part[w] > mx ? part[w] : mx;
        call[0] = mx;
    }
}

__device__ __forceinline__ double mf_scale(const uint32_t *call) { return (double)__uint_as_float(call[0]) / 127.0 * (1.0 + 1e-12); }
__device__ __forceinline__ bool mf_scale_ok(double t, double xhat_max) { return t > 0.0 && t <= 1e300 && xhat_max * xhat_max * (1.0 + 1e-6) <= MF_BMAX * 2.0 * t; }

// one wave per query: W, and the margin ceil(E_q / t) + 1 in accumulator units (0 and the query's flag when it cannot be held)
__global__ __launch_bounds__(256) void mf_quant_kernel(const float *__restrict__ q_rot, const float *__restrict__ centroid, const float *__restrict__ s, int D, int nq,
                                                       const uint32_t *__restrict__ call, double x_max, double eps_max, double xhat_max, double gamma,
                                                       int8_t *__restrict__ W, int32_t *__restrict__ margin, uint32_t *__restrict__ flags)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= nq) return;
    const double t = mf_scale(call);
    const bool usable = mf_scale_ok(t, xhat_max) && flags[q] == 0u;
    double d2 = 0.0, w2 = 0.0, r2 = 0.0;
    for (int d = lane; d < D; d += 64) {
        int Wi = 0;
        if (usable) {
            const double r = (double)__fsub_rn(q_rot[(int64_t)q * D + d], centroid[d]);
            const double w = r * (double)s[d];   // exact: two fp32 factors
            const double u = w / t;
            double Wd = rint(u);
            Wd = Wd > 127.0 ? 127.0 : (Wd < -127.0 ? -127.0 : Wd);
            const double dl = u - Wd;
            Wi = (int)Wd;
            d2 += dl * dl; w2 += w * w; r2 += r * r;
        }
        W[(int64_t)q * D + d] = (int8_t)Wi;
    }
    d2 = mf_wave_sum(d2); w2 = mf_wave_sum(w2); r2 = mf_wave_sum(r2);
    if (lane == 0) {
        const double reach = sqrt(r2) * MF_UP + xhat_max;   // >= |r - x^| for every row
        const double fp = gamma * reach * reach + 1e-30;
        const double E = (2.0 * (t * (sqrt(d2) * MF_UP + 1e-9) * x_max + sqrt(w2) * MF_UP * eps_max) + 4.0 * t + fp) * MF_UP;
        const double mg = usable ? ceil(E / t) + 1.0 : 0.0;
        const bool ok = usable && mg < 268435456.0 && reach * reach < 1e37;
        margin[q] = ok ? (int32_t)mg : 0;
        if (!ok) flags[q] = 1u;
    }
}

// B(row) = floor(n^ / 2t), the rows' starting values (negated by the filter kernel)
__global__ __launch_bounds__(kBlock) void mf_bias_kernel(const float *__restrict__ norms, int64_t n, const uint32_t *__restrict__ call, double xhat_max,
                                                         int32_t *__restrict__ bias)
{
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= n) return;
    const double t = mf_scale(call);
    bias[row] = mf_scale_ok(t, xhat_max) ? (int32_t)floor((double)norms[row] / (2.0 * t)) : 0;
}

// one wave per query: A = the k-th largest sample maximum (at least 1.25 k slots must hold a row), the threshold A - margin
template <int NK>   // NK x 64 slots per query
__global__ __launch_bounds__(256) void mf_theta_kernel(const uint32_t *__restrict__ smax, int nq, int k, const int32_t *__restrict__ margin, int32_t *__restrict__ thr,
                                                       uint32_t *__restrict__ cnt, uint32_t *__restrict__ flags)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= nq) return;
    uint32_t key[NK];
    int present = 0;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        key[j] = smax[(size_t)q * (NK * 64) + j * 64 + lane];
        present += __popcll(__ballot(key[j] != 0u));
    }
    const uint32_t sel = fs_wave_select(key, k, k + k / 4 + 8);
    if (lane == 0) {
        int32_t th = 0x7fffffff;   // nothing passes
        if (flags[q] == 0u) {
            if (sel == 0u || 4 * present < 5 * k) flags[q] = 1u;
            else th = (int32_t)(sel ^ 0x80000000u) - margin[q];
        }
        thr[q] = th;
        cnt[q] = 0u;
    }
}

// One wave ranks its exact sums (key: ~(distance bits), larger = nearer, 0 = no entry; at least `want` present): everything at or below
// the k-th smallest distance goes into sel (MF_KEEP pairs of LDS), is sorted by (distance, row), and the first k are query q's answer,
// padded with (+inf, -1).  False, and nothing written, when more than MF_KEEP rows stand at or below the k-th distance.
template <int NK>
__device__ __forceinline__ bool mf_rank_write(const uint32_t (&key)[NK], const uint32_t (&row)[NK], unsigned long long *sel, int want, int k, int64_t q, int64_t id_base,
                                              float *__restrict__ out_d, int64_t *__restrict__ out_id)
{
    const int lane = threadIdx.x;
    const uint32_t kd = fs_wave_select(key, want, want);   // the k-th smallest distance: everything at or below it is sorted
    uint32_t ns = 0;
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const bool in = key[j] != 0u && key[j] >= kd;
        const unsigned long long m = __ballot(in);
        if (m == 0ull) continue;
        const uint32_t pos = ns + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (in && pos < (uint32_t)MF_KEEP) sel[pos] = ((unsigned long long)(~key[j]) << 32) | row[j];
        ns += (uint32_t)__popcll(m);
    }
    if (ns > (uint32_t)MF_KEEP) return false;
    int np = 64;
    while (np < (int)ns) np <<= 1;
    for (int i = (int)ns + lane; i < np; i += 64) sel[i] = ~0ull;   // padding sorts last
    block_bitonic_u64<64>(sel, np);
    for (int i = lane; i < k; i += 64) {
        if ((uint32_t)i < ns) {
            const unsigned long long e = sel[i];
            out_d[q * k + i] = __uint_as_float((uint32_t)(e >> 32));
            out_id[q * k + i] = id_base + (int64_t)(uint32_t)e;
        } else {
            out_d[q * k + i] = __uint_as_float(0x7f800000u);
            out_id[q * k + i] = -1;
        }
    }
    return true;
}

// One wave per query.  Its list holds every row at or above the SAMPLED threshold; now that all rows have been seen, the k-th largest
// score A2 of the list is reached by k rows, so by the sample's argument only rows with a >= A2 - margin can be in the answer: those (about
// k + a band) get their exact sums in the reference's order; the ones at or below the k-th smallest sum are sorted by (distance, row),
// and the first k are written out.
// How the wave reaches memory: the list is read once, whole entries at a clamped index with no predicate (all loads in flight; entries
// past the count are masked afterwards); the rows inside the band are compacted into LDS, and lane l sums entries l, l + 64, ... of them,
// four at a time through ExactFromLutBatch (code rows and table gathers without a predicate, lanes past the end sum row 0 and drop it) --
// three dependent round trips per 256 band rows.  Both selections count keys and do not care where a key sits.
template <int NK>   // NK x 64 list entries at most: 16 = lists of up to 1024 entries, the usual case; MF_NSEL / 64 = the longer ones, a launch of their own
__global__ __launch_bounds__(64) void mf_select_kernel(const uint8_t *__restrict__ codes, const float *__restrict__ lut_g, int K, int nq_lut, int64_t q_base, int64_t n, int k,
                                                       const uint32_t *__restrict__ cnt, const uint2 *__restrict__ cand, uint32_t lcap, const int32_t *__restrict__ margin,
                                                       const uint32_t *__restrict__ pass_flag, int qper, int64_t id_base, float *__restrict__ out_d,
                                                       int64_t *__restrict__ out_id, uint32_t *__restrict__ flags)
{
    __shared__ __attribute__((aligned(16))) unsigned long long sel[NK * 32 > MF_KEEP ? NK * 32 : MF_KEEP];   // the band's rows (NK x 64 words) first, the kept pairs after
    uint32_t *band = reinterpret_cast<uint32_t *>(sel);
    const int lane = threadIdx.x, ql = blockIdx.x;         // the query inside its piece ...
    const int64_t q = q_base + ql;                          // ... and inside the call (tables, margins, flags and results)
    const int64_t want = k < n ? k : n;
    const uint32_t nc = cnt[ql];
    static_assert(NK == MF_NSHORT / 64 || NK == MF_NSEL / 64, "the two forms");
    if constexpr (NK == MF_NSHORT / 64) {
        if (flags[q] != 0u || pass_flag[ql / qper] != 0u || nc > lcap || (int64_t)nc < want) {   // wave-uniform: the exact scan answers this query
            if (lane == 0) flags[q] = 1u;
            return;
        }
        if (nc > (uint32_t)MF_NSHORT) return;   // (the long form's launch, behind this one)
    } else {
        if (flags[q] != 0u || nc <= (uint32_t)MF_NSHORT) return;   // (the short form, ahead of this launch, has raised the flag of every query the scan answers)
    }
    const uint2 *cq = cand + (size_t)ql * lcap;
    uint32_t key[NK], row[NK];   // key: score ^ 0x80000000 (never 0: scores stay far above INT_MIN), 0 = no entry
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const uint32_t i = (uint32_t)(j * 64 + lane);
        const uint2 e = cq[i < nc ? i : nc - 1u];   // (nc >= want >= 1)
        key[j] = i < nc ? (e.x ^ 0x80000000u) : 0u;
        row[j] = e.y;
    }
    const uint32_t a2 = fs_wave_select(key, (int)want, (int)want);
    const uint32_t cut = (uint32_t)((int32_t)(a2 ^ 0x80000000u) - margin[q]) ^ 0x80000000u;
    uint32_t nb = 0;   // the rows inside the band, side by side
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const bool in = key[j] != 0u && key[j] >= cut;
        const unsigned long long m = __ballot(in);
        const uint32_t pos = nb + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (in) band[pos] = row[j];
        nb += (uint32_t)__popcll(m);
        key[j] = 0u;
    }
    __syncthreads();
    // their exact sums: key[j] becomes ~(distance bits), larger = nearer (0 = no entry), row[j] its row
    const ExactFromLutBatch<> fixb{ codes, lut_g, K, nq_lut, (int)(q / SQ_QT) };
#pragma unroll
    for (int b = 0; b < NK / 4; ++b) {
        if ((uint32_t)(b * 256) < nb) {   // wave-uniform
            unsigned long long e[4];
            bool need[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t i = (uint32_t)((4 * b + r) * 64 + lane);
                need[r] = i < nb;
                e[r] = band[need[r] ? i : 0u];
            }
            fixb((int)(q % SQ_QT), e, need);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                key[4 * b + r] = need[r] ? ~(uint32_t)(e[r] >> 32) : 0u;   // (non-negative sums or +inf: never 0)
                row[4 * b + r] = (uint32_t)e[r];
            }
        }
    }
    __syncthreads();   // (the band's words have been read: their space takes the kept pairs)
    if (!mf_rank_write(key, row, sel, (int)want, k, q, id_base, out_d, out_id) && lane == 0) flags[q] = 1u;   // masses of rows at the k-th distance (equal rows): the exact scan
}

// The flagged queries of a call: the first MF_REDO of them take a slot of the exact redo below (slot_q[slot] = q; *count, zeroed by the
// launcher, ends as the number of flagged queries, so slots [0, min(*count, MF_REDO)) are the taken ones); rest[q] is raised for those that
// found none.  One lane per query, one atomic per wave.  Also clears the slots' list counters and fail words, and -- profiled searches --
// leaves stat[0] = queries of the call, stat[1] = how many of them were flagged (stat[1] zeroed by the launcher).
__global__ __launch_bounds__(256) void mf_compact_kernel(const uint32_t *__restrict__ flags, int nq, uint32_t *__restrict__ count, int32_t *__restrict__ slot_q,
                                                         uint32_t *__restrict__ lcnt, uint32_t *__restrict__ fail, uint32_t *__restrict__ rest,
                                                         unsigned long long *__restrict__ stat)
{
    const int q = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x < MF_REDO) { lcnt[threadIdx.x] = 0u; fail[threadIdx.x] = 0u; }
    if (stat && q == 0) stat[0] = (unsigned long long)nq;
    const bool flagged = q < nq && flags[q] != 0u;
    const unsigned long long m = __ballot(flagged);
    uint32_t base = 0;
    if (lane == 0 && m) {
        base = atomicAdd(count, (uint32_t)__popcll(m));
        if (stat) atomicAdd(stat + 1, (unsigned long long)__popcll(m));
    }
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (q >= nq) return;
    const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    const bool taken = flagged && slot < (uint32_t)MF_REDO;
    if (taken) slot_q[slot] = q;
    rest[q] = flagged && !taken ? 1u : 0u;
}

// The exact redo of the queries that took a slot: the route's scheme (bound, collect, finish) over ALL rows in fp32.
// A distance is the reference's sum, m ascending with __fadd_rn over the query's fp32 table (as ExactFromLut; the 16 KB table in LDS);
// its key is the uint bits of that non-negative float.
__device__ __forceinline__ uint32_t mf_redo_sum(const float *t, const uint4 c)
{
    const uint32_t w[4] = { c.x, c.y, c.z, c.w };
    float v[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = t[m * 256 + (int)((w[m >> 2] >> (8 * (m & 3))) & 0xffu)];
    float s = 0.0f;
#pragma unroll
    for (int m = 0; m < 16; ++m) s = __fadd_rn(s, v[m]);
    return __float_as_uint(s);
}
// Both passes over the rows.  Grid (row slices of `per` rows, slot lanes): a workgroup takes slots blockIdx.y, + gridDim.y, ... below the
// taken count (none: it leaves at once); lane t of it sums rows t, t + 256, ... of its slice, four loads in flight.
//   bound (COLLECT false): the minimum over the rows of every 16 lanes -- a row set of its own -- into smin[slot][16 slice + .] (~0: the set
//     holds no row).  mf_redo_tau_kernel takes the k-th smallest of them: k distinct rows reach it, so it bounds the k-th distance.
//     A sum that is NaN (or negative: no key) raises fail[slot]: the exact scan answers that query.
//   collect: every row at or below tau[slot] is appended to list[slot] as (distance bits, row) under lcnt[slot]; entries past MF_NSHORT are
//     dropped, the count shows it.
template <bool COLLECT>
__global__ __launch_bounds__(256) void mf_redo_pass_kernel(const uint4 *__restrict__ codes, int64_t n, int64_t per, const float *__restrict__ lut_g,
                                                           const uint32_t *__restrict__ call, const int32_t *__restrict__ slot_q, uint32_t *__restrict__ smin,
                                                           const uint32_t *__restrict__ tau, uint32_t *__restrict__ lcnt, uint2 *__restrict__ list,
                                                           uint32_t *__restrict__ fail)
{
    __shared__ float4 tab[16 * 256 / 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t taken = call[MF_CALL_WORDS - 1] < (uint32_t)MF_REDO ? call[MF_CALL_WORDS - 1] : (uint32_t)MF_REDO;
    const int64_t row0 = (int64_t)blockIdx.x * per, row1 = row0 + per < n ? row0 + per : n;   // (row0 < n: the grid is blocks_for(n, per))
    for (uint32_t slot = blockIdx.y; slot < taken; slot += gridDim.y) {   // workgroup-uniform
        const float4 *src = reinterpret_cast<const float4 *>(lut_g + (int64_t)slot_q[slot] * 16 * 256);
        __syncthreads();   // (the last slot's table has been read)
        for (int i = tid; i < 16 * 256 / 4; i += 256) tab[i] = src[i];
        __syncthreads();
        const float *t = reinterpret_cast<const float *>(tab);
        const uint32_t cut = COLLECT ? tau[slot] : 0u;
        uint32_t best = ~0u;
        bool bad = false;
        for (int64_t b = row0; b < row1; b += 1024) {
            uint4 c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t r = b + j * 256 + tid;
                c[j] = codes[r < row1 ? r : row1 - 1];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t r = b + j * 256 + tid;
                const uint32_t bits = mf_redo_sum(t, c[j]);
                if constexpr (COLLECT) {
                    const bool in = r < row1 && bits <= cut;
                    const unsigned long long m = __ballot(in);
                    if (m == 0ull) continue;   // wave-uniform
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(lcnt + slot, (uint32_t)__popcll(m));
                    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    const uint32_t pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (in && pos < (uint32_t)MF_NSHORT) list[(size_t)slot * MF_NSHORT + pos] = make_uint2(bits, (uint32_t)r);
                } else if (r < row1) {
                    if (bits > 0x7f800000u) bad = true;
                    else best = bits < best ? bits : best;
                }
            }
        }
        if constexpr (!COLLECT) {
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                const uint32_t other = (uint32_t)__shfl_xor((int)best, o, 64);
                best = other < best ? other : best;
            }
            if ((tid & 15) == 0) smin[(size_t)slot * MF_REDO_SETS + blockIdx.x * 16 + (tid >> 4)] = best;
            if (bad) fail[slot] = 1u;
        }
    }
}
// one wave per slot: tau = the k-th smallest set minimum (distance bits); fewer than `want` sets with a row: no bound, every row passes
__global__ __launch_bounds__(64) void mf_redo_tau_kernel(const uint32_t *__restrict__ smin, int nsets, int want, const uint32_t *__restrict__ call, uint32_t *__restrict__ tau)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    if ((uint32_t)slot >= call[MF_CALL_WORDS - 1]) return;
    uint32_t key[MF_REDO_SETS / 64];   // ~bits: larger = nearer, 0 = no set or a set without a row
#pragma unroll
    for (int j = 0; j < MF_REDO_SETS / 64; ++j) {
        const int i = j * 64 + lane;
        const uint32_t v = smin[(size_t)slot * MF_REDO_SETS + (i < nsets ? i : 0)];
        key[j] = i < nsets ? ~v : 0u;
    }
    const uint32_t sel = fs_wave_select(key, want, want);
    if (lane == 0) tau[slot] = sel != 0u ? ~sel : ~0u;
}
// One wave per slot ranks the slot's list -- every row at or below tau, so every row of the answer -- and writes the answer to the query's
// own place.  A list over its cap, more than MF_KEEP rows at or below the k-th distance or a NaN met by the bound pass: rest[q].
__global__ __launch_bounds__(64) void mf_redo_finish_kernel(const uint32_t *__restrict__ call, const int32_t *__restrict__ slot_q, const uint32_t *__restrict__ lcnt,
                                                            const uint2 *__restrict__ list, const uint32_t *__restrict__ fail, int64_t n, int k, int64_t id_base,
                                                            float *__restrict__ out_d, int64_t *__restrict__ out_id, uint32_t *__restrict__ rest)
{
    __shared__ __attribute__((aligned(16))) unsigned long long sel[MF_KEEP];
    constexpr int NK = MF_NSHORT / 64;
    const int slot = blockIdx.x, lane = threadIdx.x;
    if ((uint32_t)slot >= call[MF_CALL_WORDS - 1]) return;
    const int64_t q = slot_q[slot], want = k < n ? k : n;
    const uint32_t nc = lcnt[slot];
    if (fail[slot] != 0u || nc > (uint32_t)MF_NSHORT || (int64_t)nc < want) {   // wave-uniform
        if (lane == 0) rest[q] = 1u;
        return;
    }
    const uint2 *lq = list + (size_t)slot * MF_NSHORT;
    uint32_t key[NK], row[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        const uint32_t i = (uint32_t)(j * 64 + lane);
        const uint2 e = lq[i < nc ? i : nc - 1u];   // (nc >= want >= 1)
        key[j] = i < nc ? ~e.x : 0u;   // (bits of non-negative sums or +inf: never 0)
        row[j] = e.y;
    }
    if (!mf_rank_write(key, row, sel, (int)want, k, q, id_base, out_d, out_id) && lane == 0) rest[q] = 1u;
}

size_t mf_align(size_t v, size_t a) { return (v + a - 1) / a * a; }

// how a piece of m queries is laid over the filter kernels' grid, and the scratch it needs
constexpr size_t MF_PIECE_BYTES = (size_t)1 << 30;   // lists and record regions of a piece
struct MfShape {
    int chunks, qper, spx, stride;
    int64_t regions;
    uint32_t rec_cap;
    size_t bytes;
};
MfShape mf_shape(int D, int64_t n, int64_t m, int k, int list_cap, int div, bool fill = true)
{
    MfShape s;
    s.chunks = (int)blocks_for(m, 256);
    s.qper = (int)(blocks_for(blocks_for(m, s.chunks), 32) * 32);
    s.spx = s.chunks == 1 ? 32 : (s.chunks == 2 ? 16 : 8);   // a small batch still fills the device; a large one has its chunks for that
    s.stride = 8 * s.spx * 16;
    s.regions = (int64_t)8 * s.spx * s.chunks * 8;
    // Records per wave region.  How many rows per query pass the sampled threshold is the data's business: measured through the fullest
    // region (profiles/adc_mfma_sweep.txt, SIFT-like rows, k = 100, every other tile group sampled) it is about 800 at 1 M rows and grows as
    // the index shrinks (regions of 900 records overrun at 262 144 rows).  The guess max(4 k, 256) x div stands for it; a wave meets its
    // share of those rows -- its tile groups out of all, whole groups: a small index leaves most waves without one -- for the queries of
    // its chunk.  Twice that is the least a piece is given (the piece size follows from it); then the regions grow into what is left of the
    // piece's 1 GB, up to eight times the guess.  A region that still runs over costs its chunk's queries the scan, nobody else.
    const double pass = std::min<double>((double)std::max(4 * k, 256) * div, (double)n);
    const int64_t all_groups = blocks_for(blocks_for(n, 32), u8_filter_rt(D)), streams = (int64_t)8 * s.spx * 8;
    const double share = (double)blocks_for(all_groups, streams) / (double)all_groups;
    const double base = (double)s.qper * pass * share;
    s.rec_cap = (uint32_t)std::min<double>(8192.0, std::max<double>(256.0, 2.0 * base));
    if (fill) {
        const size_t other = mf_align((size_t)m * 4, 256) * 2 + mf_align((size_t)s.chunks * 4, 256) + mf_align((size_t)m * s.stride * 4, 256) +
                             mf_align((size_t)s.regions * 4, 256) + mf_align((size_t)m * list_cap * sizeof(uint2), 256) + 256;
        const size_t room = other < MF_PIECE_BYTES ? (MF_PIECE_BYTES - other) / ((size_t)s.regions * u8_filter_rec_bytes()) : 0;
        const uint32_t want = (uint32_t)std::min<double>(8192.0, 8.0 * base);
        s.rec_cap = std::max(s.rec_cap, (uint32_t)std::min<size_t>(want, room));
    }
    s.bytes = mf_align((size_t)m * 4, 256) * 2 + mf_align((size_t)s.chunks * 4, 256) + mf_align((size_t)m * s.stride * 4, 256) + mf_align((size_t)s.regions * 4, 256) +
              mf_align((size_t)m * list_cap * sizeof(uint2), 256) + mf_align((size_t)s.regions * s.rec_cap * u8_filter_rec_bytes(), 256);
    return s;
}
// the exact redo's scratch: slot_q, list counters, fail words and tau per slot, the set minima (1 MB) and the lists (0.5 MB)
size_t mf_redo_bytes()
{
    return mf_align(MF_REDO * 4, 256) * 4 + mf_align((size_t)MF_REDO * MF_REDO_SETS * 4, 256) + mf_align((size_t)MF_REDO * MF_NSHORT * sizeof(uint2), 256);
}
size_t mf_call_bytes(int D, int64_t n, int64_t nq)
{
    return mf_redo_bytes() + mf_align((size_t)nq * 4, 256) + mf_align(MF_CALL_WORDS * 4, 256) + mf_align((size_t)nq * 4, 256) * 2 + mf_align((size_t)nq * D, 256) + mf_align((size_t)n * 4, 256);
}

}  // namespace

bool adc_mfma_model(const float *books, int D, int K, int8_t *xb, double *nrm, float *c, float *s, double *x_max, double *eps_max, double *xhat_max)
{
    const int M = 16, step = D / M;
    if (K != 256 || D % M != 0) return false;
    for (size_t i = 0; i < (size_t)D * K; ++i)
        if (!std::isfinite(books[i])) return false;
    for (int d = 0; d < D; ++d) {
        const int m = d / step, kk = d % step;
        double lo = books[(size_t)m * K * step + kk], hi = lo;
        for (int j = 1; j < K; ++j) {
            const double v = books[((size_t)m * K + j) * step + kk];
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
        const double range = hi - lo;
        float cf = (float)(0.5 * hi + 0.5 * lo), sf = (float)(range / 254.0);
        if (range == 0.0) { cf = (float)lo; sf = 0.0f; }   // every codeword holds c here: X = 0 is exact
        else if (!(sf >= FLT_MIN) || !std::isfinite(sf) || !std::isfinite(cf)) return false;
        c[d] = cf; s[d] = sf;
    }
    double sx = 0.0, se = 0.0, sn = 0.0;
    for (int m = 0; m < M; ++m) {
        double mx = 0.0, me = 0.0, mn = 0.0;
        for (int j = 0; j < K; ++j) {
            double x2 = 0.0, e2 = 0.0, n2 = 0.0;
            for (int kk = 0; kk < step; ++kk) {
                const int d = m * step + kk;
                const double v = books[((size_t)m * K + j) * step + kk];
                double X = 0.0, e = 0.0;
                if (s[d] > 0.0f) {
                    const double u = (v - (double)c[d]) / (double)s[d];
                    X = std::nearbyint(u);
                    X = X > 127.0 ? 127.0 : (X < -127.0 ? -127.0 : X);
                    e = u - X;
                }
                xb[((size_t)m * 256 + j) * step + kk] = (int8_t)(int)X;
                x2 += X * X; e2 += e * e; n2 += v * v;
            }
            nrm[m * 256 + j] = n2;
            mx = std::max(mx, x2); me = std::max(me, e2); mn = std::max(mn, n2);
        }
        sx += mx; se += me; sn += mn;
    }
    *x_max = std::sqrt(sx) * MF_UP; *eps_max = std::sqrt(se) * MF_UP + 1e-12; *xhat_max = std::sqrt(sn) * MF_UP;
    return std::isfinite(*x_max) && std::isfinite(*eps_max) && std::isfinite(*xhat_max);
}

size_t adc_mfma_pack_bytes(int D, int64_t n) { return (size_t)((n + 31) / 32) * (D / 32) * 64 * sizeof(uint4); }

// rows [row0, n) of the copy (the tile row0 falls into is written again as a whole)
int launch_adc_mfma_pack(const AdcMfmaModel &mm, int D, const uint8_t *codes, int64_t row0, int64_t n, void *pack, float *norms, hipStream_t st)
{
    if (D % 32 != 0 || D < 32 || D > 256 || row0 < 0 || row0 > n) return fail(CVTMI_EINVAL, "adc_mfma_pack: D=%d rows %lld..%lld", D, (long long)row0, (long long)n);
    if (n == row0) return CVTMI_OK;
    const int ks = D / 32;
    const int64_t ntiles = (n + 31) / 32, tile0 = row0 / 32, total = (ntiles - tile0) * ks * 64;
    CVTMI_TRY(launch("mf_pack_kernel", mf_pack_kernel, blocks_for(total, kBlock), kBlock, 0, st, reinterpret_cast<const uint4 *>(codes), n, ks, D / 16, mm.xb, tile0, ntiles,
                     reinterpret_cast<uint4 *>(pack)));
    return launch("mf_norm_kernel", mf_norm_kernel, blocks_for(n - row0, kBlock), kBlock, 0, st, reinterpret_cast<const uint4 *>(codes), row0, n, mm.nrm, norms);
}

static int mf_div(int sample_div) { return sample_div >= 1 && sample_div <= 3 ? sample_div : 2; }

// scratch of a call; *per: queries per piece (a piece's lists and record regions stay under 1 GB)
size_t adc_mfma_scratch_bytes(int D, int64_t n, int64_t nq, int k, int list_cap, int sample_div, int64_t *per)
{
    const int div = mf_div(sample_div);
    int64_t p = nq;
    while (p > 256 && mf_shape(D, n, p, k, list_cap, div, false).bytes > MF_PIECE_BYTES) p = blocks_for(blocks_for(p, 2), 256) * 256;
    if (per) *per = p;
    size_t piece = mf_shape(D, n, p, k, list_cap, div).bytes;
    if (nq % p) piece = std::max(piece, mf_shape(D, n, nq % p, k, list_cap, div).bytes);   // (the last, shorter piece lays itself out anew)
    return mf_call_bytes(D, n, nq) + piece;
}

int launch_adc_mfma(const OpqModelDev &m, const AdcMfmaModel &mm, const uint8_t *codes, const void *pack, const float *norms, int64_t n, int64_t id_base,
                    const float *q_rot, int64_t nq, int k, int list_cap, int sample_div, float *lut_g, void *scratch, float *dist, int64_t *ids,
                    AdcMfmaRedo *redo, unsigned long long *stat, hipStream_t st)
{
    if (m.M != 16 || m.K != 256 || m.D % 32 != 0 || m.D > 256 || k < 1 || k > 128 || n < 1 || n >= 0x7fffffe0LL || nq < 1 || nq > 0x7fffffff || list_cap < 1 ||
        list_cap > MF_NSEL)
        return fail(CVTMI_EUNSUPPORTED, "adc_mfma: shape not covered");
    const int D = m.D, div = mf_div(sample_div);
    int64_t per = 0;
    adc_mfma_scratch_bytes(D, n, nq, k, list_cap, sample_div, &per);
    char *sc = reinterpret_cast<char *>(scratch);
    uint32_t *call = reinterpret_cast<uint32_t *>(sc); sc += mf_align(MF_CALL_WORDS * 4, 256);
    uint32_t *flags = reinterpret_cast<uint32_t *>(sc); sc += mf_align((size_t)nq * 4, 256);
    int32_t *margin = reinterpret_cast<int32_t *>(sc); sc += mf_align((size_t)nq * 4, 256);
    int8_t *W = reinterpret_cast<int8_t *>(sc); sc += mf_align((size_t)nq * D, 256);
    int32_t *bias = reinterpret_cast<int32_t *>(sc); sc += mf_align((size_t)n * 4, 256);
    int32_t *slot_q = reinterpret_cast<int32_t *>(sc); sc += mf_align(MF_REDO * 4, 256);
    uint32_t *lcnt = reinterpret_cast<uint32_t *>(sc); sc += mf_align(MF_REDO * 4, 256);
    uint32_t *rfail = reinterpret_cast<uint32_t *>(sc); sc += mf_align(MF_REDO * 4, 256);
    uint32_t *tau = reinterpret_cast<uint32_t *>(sc); sc += mf_align(MF_REDO * 4, 256);
    uint32_t *smin = reinterpret_cast<uint32_t *>(sc); sc += mf_align((size_t)MF_REDO * MF_REDO_SETS * 4, 256);
    uint2 *rlist = reinterpret_cast<uint2 *>(sc); sc += mf_align((size_t)MF_REDO * MF_NSHORT * sizeof(uint2), 256);
    redo->rest = reinterpret_cast<uint32_t *>(sc); sc += mf_align((size_t)nq * 4, 256);
    CVTMI_HIP(hipMemsetAsync(call, 0, MF_CALL_WORDS * 4, st));
    // (step + 19) roundings of non-negative partial sums in the reference's evaluation of one distance: five to spare
    const double gamma = (double)(m.step + 24) * 5.9604644775390625e-8 * 1.01;
    CVTMI_TRY(launch_lut(m, q_rot, nq, nullptr, lut_g, st, 256));   // [nq][16][256] fp32: what the selection sums
    CVTMI_TRY(launch("mf_qmax_kernel", mf_qmax_kernel, blocks_for(nq, 4), 256, 0, st, q_rot, m.coarse, mm.s, D, (int)nq, reinterpret_cast<uint32_t *>(margin), flags));
    CVTMI_TRY(launch("mf_qred_kernel", mf_qred_kernel, 1, 1024, 0, st, reinterpret_cast<const uint32_t *>(margin), (int)nq, call));   // (margin: written by the next kernel)
    CVTMI_TRY(launch("mf_quant_kernel", mf_quant_kernel, blocks_for(nq, 4), 256, 0, st, q_rot, m.coarse, mm.s, D, (int)nq, call, mm.x_max, mm.eps_max, mm.xhat_max,
                     gamma, W, margin, flags));
    CVTMI_TRY(launch("mf_bias_kernel", mf_bias_kernel, blocks_for(n, kBlock), kBlock, 0, st, norms, n, call, mm.xhat_max, bias));
    const int rt = u8_filter_rt(D);
    const int64_t all_groups = blocks_for(blocks_for(n, 32), rt);
    for (int64_t q0 = 0; q0 < nq; q0 += per) {
        const int64_t mq = std::min(per, nq - q0);
        const MfShape s = mf_shape(D, n, mq, k, list_cap, div);
        char *p = sc;
        int32_t *thr = reinterpret_cast<int32_t *>(p); p += mf_align((size_t)mq * 4, 256);
        uint32_t *cnt = reinterpret_cast<uint32_t *>(p); p += mf_align((size_t)mq * 4, 256);
        uint32_t *cflag = reinterpret_cast<uint32_t *>(p); p += mf_align((size_t)s.chunks * 4, 256);   // a chunk's word: one of its record regions ran over
        uint32_t *smax = reinterpret_cast<uint32_t *>(p); p += mf_align((size_t)mq * s.stride * 4, 256);
        CVTMI_HIP(hipMemsetAsync(cflag, 0, (size_t)s.chunks * 4, st));
        uint32_t *wcnt = reinterpret_cast<uint32_t *>(p); p += mf_align((size_t)s.regions * 4, 256);
        uint2 *cand = reinterpret_cast<uint2 *>(p); p += mf_align((size_t)mq * list_cap * sizeof(uint2), 256);
        void *rec = p;
        // (no memset of smax: s.stride is 8 spx x 16, one slot per half wave of a chunk's workgroups, and the sample pass writes every one of them)
        U8FilterJob j;
        j.pack = pack; j.bias = bias; j.n = n; j.D = D; j.W = W + q0 * D; j.nq = (int)mq; j.chunks = s.chunks; j.qper = s.qper; j.spx = s.spx;
        j.smax = smax; j.smax_stride = s.stride;
        {   // the sample: one tile group in div, a whole number per wave of a chunk, never fewer than 2048 rows' worth of groups
            const int64_t streams = (int64_t)8 * s.spx * 8;
            const int64_t want = std::max<int64_t>(blocks_for(all_groups, div), std::min<int64_t>(all_groups, 2048 / rt));
            j.n_sample = std::min<int64_t>(all_groups, blocks_for(want, streams) * streams);
        }
        j.thr = thr; j.rec = rec; j.wcnt = wcnt; j.rec_cap = s.rec_cap; j.cnt = cnt; j.cand = cand; j.list_cap = (uint32_t)list_cap; j.pass_flag = cflag;
        CVTMI_TRY(launch_u8_filter_sample(j, st));
        auto theta = mf_theta_kernel<16>;
        if (s.stride == 2048) theta = mf_theta_kernel<32>;
        else if (s.stride == 4096) theta = mf_theta_kernel<64>;
        CVTMI_TRY(launch("mf_theta_kernel", theta, blocks_for(mq, 4), 256, 0, st, smax, (int)mq, k, margin + q0, thr, cnt, flags + q0));
        CVTMI_TRY(launch_u8_filter_pass(j, st));
        CVTMI_TRY(launch_u8_filter_bucket(j, st));
        CVTMI_TRY(launch("mf_select_kernel", mf_select_kernel<MF_NSHORT / 64>, mq, 64, 0, st, codes, lut_g, m.K, (int)nq, q0, n, k, cnt, cand, (uint32_t)list_cap, margin, cflag, s.qper,
                         id_base, dist, ids, flags));
        // lists of more than 1024 entries: the same body over MF_NSEL slots, with the registers and the LDS that takes (every workgroup looks at
        // its query's count; the ones whose list the short form took leave at once)
        if (list_cap > MF_NSHORT)
            CVTMI_TRY(launch("mf_select_long_kernel", mf_select_kernel<MF_NSEL / 64>, mq, 64, 0, st, codes, lut_g, m.K, (int)nq, q0, n, k, cnt, cand, (uint32_t)list_cap, margin,
                             cflag, s.qper, id_base, dist, ids, flags));
    }
    // The flagged queries: up to MF_REDO take a slot and are answered here, exactly, over all rows (bound, tau, collect, finish); no
    // memset and no copy of a query: the slots' words are cleared by the compaction, the tables are the selection's.
    if (stat) CVTMI_HIP(hipMemsetAsync(stat, 0, 2 * sizeof(unsigned long long), st));
    CVTMI_TRY(launch("mf_compact_kernel", mf_compact_kernel, blocks_for(nq, 256), 256, 0, st, flags, (int)nq, call + MF_CALL_WORDS - 1, slot_q, lcnt, rfail, redo->rest, stat));
    // row slices: 256 at 1 M rows, never under 256 rows each -- a row per lane, so that a small index still has many more sets than k
    const int64_t rper = std::max<int64_t>(256, blocks_for(n, MF_REDO_SLICES)), slices = blocks_for(n, rper);
    const Grid rgrid{ slices, 8 };   // eight slot lanes: one or two flagged queries leave few workgroups without work, 64 share the rows' reads
    const uint4 *rows = reinterpret_cast<const uint4 *>(codes);
    CVTMI_TRY(launch("mf_redo_bound_kernel", mf_redo_pass_kernel<false>, rgrid, 256, 0, st, rows, n, rper, lut_g, call, slot_q, smin, tau, lcnt, rlist, rfail));
    CVTMI_TRY(launch("mf_redo_tau_kernel", mf_redo_tau_kernel, MF_REDO, 64, 0, st, smin, (int)slices * 16, (int)std::min<int64_t>(k, n), call, tau));
    CVTMI_TRY(launch("mf_redo_collect_kernel", mf_redo_pass_kernel<true>, rgrid, 256, 0, st, rows, n, rper, lut_g, call, slot_q, smin, tau, lcnt, rlist, rfail));
    return launch("mf_redo_finish_kernel", mf_redo_finish_kernel, MF_REDO, 64, 0, st, call, slot_q, lcnt, rlist, rfail, n, k, id_base, dist, ids, redo->rest);
}

}  // namespace cvtmi
