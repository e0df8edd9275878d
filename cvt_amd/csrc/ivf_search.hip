// ivf_search.hip -- row-level top-k over the nprobe nearest coarse lists (cvtmi_opq_search_ivf).
//
// The arithmetic is IVFOPQ::Query's (opq/src/IVFOPQ.cpp:213-320) up to the score of an entry: the probed lists are the nprobe
// smallest (sequential fp32 distance, list) pairs (launch_coarse_probe, query_video.hip), the table of a (query, list) pair is
// built from the residual q - coarse[l] with separate subtract / multiply / add (:273-291), and an entry scores the sum of its
// M table cells, m ascending (:300-306).  Where Query folds the scores into per-video minima clamped at 1.0, this file keeps the
// k smallest (score, id) pairs: id = insertion index (the list-ordered copy carries it, csr_scatter_kernel), no clamp.
//
// One workgroup owns (query, group of G consecutive probe slots, piece): for each list of its group it builds the [M][256] table
// in LDS (16 KB at M = 16, so several workgroups share a CU) and scores the rows of its piece of that list, 256 per tile, pushing
// (key, insertion index) into a TopKShared buffer under the running k-th key.  At the reference's shape (8192 lists, ~122 rows
// each) the table -- 4096 cells x D / M dimensions -- costs far more than the rows, so the build is spread over all threads and the
// first tile's code rows are requested BEFORE it: they land while the table is computed.
//
// Tie rule.  Insertion indices ascend inside a list but not across the lists of a group, so the '<' fast path of block_topk.h
// (which relies on ascending payloads) does not apply: candidates are offered with '<=' against the k-th key, every tie reaches
// the buffer, and the sort of the exact (key, payload) words decides -- the exemption block_topk.h documents.  The merge of
// partial lists below selects on the same words for the same reason: topk_merge_kernel breaks ties by position in its input,
// which is id order only when the lists cover ascending id ranges.
//
// Keys are the raw bits of the scores: sums of squares are >= +0, so the bit patterns order like the values, +inf (0x7f800000)
// after every finite score and NaN patterns after that.  A query holding a NaN scores NaN everywhere; its entries then tie or
// order by NaN payload bits, and what comes back is min(k, entries) distinct entries with NaN distances.
//
// cvtmi_opq_search_ivf_masked is the same scan under a bitmap of allowed entries (the MASKED instantiations, below): the mask is
// brought into list order once per call, and a workgroup leaves a list whose rows are all disallowed before it builds the table.
#include <algorithm>

#include "block_topk.h"
#include "ivf_table.h"
#include "kernels.h"
#include "launch.h"

namespace cvtmi {

constexpr int IVF_CAP = 512, IVF_TRIG = 384;   // k <= 128; larger k: kBigCap / kBigTrig, as the generic exact scan
constexpr unsigned long long IVF_NONE = ~0ull; // an empty slot of a partial list (no entry has key KEY_MAX)
constexpr uint32_t IVF_NO_ROW = ~0u;           // masked scan: the payload of a row the mask does not allow (fewer than 2^32 entries: no insertion index is ~0u)

__device__ __forceinline__ uint32_t ivf_key(float s)
{
    const uint32_t kk = __float_as_uint(s);
    return kk == KEY_MAX ? KEY_MAX - 1 : kk;   // (a NaN pattern; KEY_MAX is the selection's "no k-th entry yet")
}

// one candidate per thread and tile, '<=' on the fast path (see the tie rule above)
template <int CAP, int TRIG>
__device__ __forceinline__ void ivf_offer(TopKShared<1, CAP> &tk, int k, int tile, bool have, uint32_t key, uint32_t pay)
{
    bool want = false;
    uint32_t pending = 0;
    if (have && key <= tk.thr_x[0]) {
        if (!topk_push<1, CAP, TRIG>(tk, 0, key, pay, want)) pending = 1u;
    }
    topk_tile_end<1, CAP, kBlock>(tk, k, tile, want, pending, NoFix(), IdThr(), [&](uint32_t pend) {
        bool dummy = false;
        if (pend && key <= tk.thr_x[0] && !topk_push<1, CAP, TRIG>(tk, 0, key, pay, dummy)) return 1u;
        return 0u;
    });
}

// Masked search (cvtmi_opq_search_ivf_masked).  The caller's mask addresses insertion indices; this kernel brings it into the order
// the scan walks: one lane per row r of the list-ordered copy reads the caller's bit of entry[r] (a gather into a bitmap of n / 8
// bytes, cache-resident), and one __ballot per wave64 is the word of rows [64 w, 64 w + 64), stored by one lane.  No atomics; rows
// behind the copy's end contribute 0.
__global__ __launch_bounds__(kBlock) void ivf_mask_order_kernel(const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ entry,
                                                                int64_t n_csr, unsigned long long *__restrict__ lmask)
{
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool on = false;
    if (r < n_csr) {
        const uint32_t i = entry[r];
        on = (mask[i >> 6] >> (i & 63u)) & 1ull;
    }
    const unsigned long long w = __ballot(on);
    if ((threadIdx.x & 63) == 0 && r < n_csr) lmask[r >> 6] = w;   // (r = 64 w: the word holds at least row r)
}

__device__ __forceinline__ bool ivf_mask_bit(const unsigned long long *__restrict__ lmask, int64_t r)
{
    return (reinterpret_cast<const uint32_t *>(lmask)[r >> 5] >> (r & 31)) & 1u;   // (little endian: bit r of the uint64 view)
}

// does the mask allow any row of [b, e)?  b < e; the words of the range are spread over the workgroup's threads and the two edge words
// are cut to the range (b and e are no multiples of 64).  Every thread that saw a bit raises flag[round % 3] and ALL threads read it
// behind one barrier: every thread gets the same answer, so the caller may branch around barriers on it.  Must be reached by all
// threads of the workgroup, with the workgroup-uniform count of the calls so far as `round`.  The three flags (zero at the start)
// rotate like those of topk_tile_end: the flag of round + 1 is cleared here, BEFORE this round's barrier -- its last readers (round
// - 2) passed the barrier of round - 1 since, and its next writers come after this one.  (__syncthreads_or would do, but the
// library's reduction costs the kernel 6 VGPRs -- a workgroup per CU -- and 256 bytes of LDS.)
__device__ __forceinline__ bool ivf_mask_any(const unsigned long long *__restrict__ lmask, int64_t b, int64_t e, int tid, int *flag, int round)
{
    const int64_t w0 = b >> 6, w1 = (e - 1) >> 6;
    unsigned long long acc = 0ull;
    for (int64_t w = w0 + tid; w <= w1; w += kBlock) {
        unsigned long long x = lmask[w];
        if (w == w0) x &= ~0ull << (b & 63);
        if (w == w1) x &= ~0ull >> (63 - ((e - 1) & 63));
        acc |= x;
    }
    const int f = round % 3;
    if (acc != 0ull) flag[f] = 1;
    if (tid == 0) flag[(round + 1) % 3] = 0;
    __syncthreads();
    return flag[f] != 0;
}

// the same question for one tile, [lo, hi) with hi - lo <= kBlock: at most five words, and EVERY thread reads all of them -- the same
// read-only words at workgroup-uniform addresses, so every thread holds the same answer without a barrier
__device__ __forceinline__ bool ivf_mask_any_tile(const unsigned long long *__restrict__ lmask, int64_t lo, int64_t hi)
{
    const int64_t w0 = lo >> 6, w1 = (hi - 1) >> 6;
    unsigned long long acc = 0ull;
    for (int64_t w = w0; w <= w1; ++w) {
        unsigned long long x = lmask[w];
        if (w == w0) x &= ~0ull << (lo & 63);
        if (w == w1) x &= ~0ull >> (63 - ((hi - 1) & 63));
        acc |= x;
    }
    return acc != 0ull;
}

// part == nullptr: the workgroup holds everything of its query (one group, one piece) and writes the result rows itself;
// otherwise it writes its k best as sorted (key << 32 | insertion index) words to partial list (group * pieces + piece) of the query.
// MASKED: lmask holds one bit per row of the list-ordered copy (ivf_mask_order_kernel) and only rows whose bit is set are offered.
// A workgroup whose [b, e) of a list holds no allowed row leaves the list before its table is built -- the table, not the rows, is
// what a (query, list) pair costs -- and a piece of several tiles skips the tiles without one.  Both decisions are the same in
// every thread (ivf_mask_any: a flag read behind a barrier; ivf_mask_any_tile: the same words read by all), so they are
// workgroup-uniform like the other `continue`s, and `tile` counts only the tiles that reach topk_tile_end (its flags rotate with
// that counter).  The unmasked instantiations take a null lmask and compile no masked line.
template <int CAP, int TRIG, bool MASKED>
__global__ __launch_bounds__(kBlock) void ivf_search_kernel(const float *__restrict__ q_rot, int D, int M, int K, int step,
                                                            const float *__restrict__ coarse, const float *__restrict__ books, int nprobe,
                                                            const int32_t *__restrict__ probe, const int64_t *__restrict__ list_off,
                                                            const uint8_t *__restrict__ codes, const uint32_t *__restrict__ entry, int k, int G,
                                                            int groups, int pieces, int rows_per_piece, int64_t id_base,
                                                            float *__restrict__ out_d, int64_t *__restrict__ out_id,
                                                            unsigned long long *__restrict__ part, const unsigned long long *__restrict__ lmask)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];  // res[D rounded up to 4] + lut[M][256]
    __shared__ TopKShared<1, CAP> tk;
    __shared__ int any_flag[3];   // MASKED: ivf_mask_any's rotating flags (12 bytes; the unmasked instantiations never touch them)
    float *res = sm;
    float *lut = sm + ((D + 3) & ~3);
    const int piece = (int)(blockIdx.x % (unsigned)pieces);
    const int64_t qg = blockIdx.x / (unsigned)pieces;
    const int g = (int)(qg % groups);
    const int64_t qi = qg / groups;
    const int tid = threadIdx.x;
    topk_init(tk);
    if constexpr (MASKED) {
        if (tid < 3) any_flag[tid] = 0;
    }
    __syncthreads();
    const int s0 = g * G, s1 = s0 + G < nprobe ? s0 + G : nprobe;
    int tile = 0, round = 0;
    for (int s = s0; s < s1; ++s) {
        const int l = probe[qi * nprobe + s];
        if (l < 0) continue;  // workgroup-uniform
        const int64_t b = list_off[l] + (int64_t)piece * rows_per_piece;
        int64_t e = b + rows_per_piece;
        e = e < list_off[l + 1] ? e : list_off[l + 1];
        if (b >= e) continue;  // workgroup-uniform: an empty list, or a piece past its end
        bool tiles = false;    // MASKED: the piece has more than one tile, each is asked for an allowed row
        if constexpr (MASKED) {
            if (!ivf_mask_any(lmask, b, e, tid, any_flag, round++)) continue;  // workgroup-uniform (see ivf_mask_any): no allowed row, no table
            tiles = e - b > kBlock;
        }
        // the first tile's rows are on their way while the table is built
        ivf_u32x4 v = { 0u, 0u, 0u, 0u };
        uint32_t pay = MASKED ? IVF_NO_ROW : 0;   // MASKED: the bit of a row travels with it -- pay stays IVF_NO_ROW unless it is set
        if (M == 16 && b + tid < e && (!MASKED || ivf_mask_bit(lmask, b + tid))) {
            v = __builtin_nontemporal_load(reinterpret_cast<const ivf_u32x4 *>(codes) + (b + tid));
            pay = entry[b + tid];
        }
        ivf_build_table(res, lut, q_rot + qi * D, coarse + (int64_t)l * D, books, D, M, K, step, tid);
        for (int64_t base = b; base < e; base += kBlock) {
            const int64_t r = base + tid;
            bool have = r < e;
            float sc = 0.0f;
            if (M == 16) {
                const ivf_u32x4 cur = v;
                const uint32_t cur_pay = pay;
                if constexpr (MASKED) {
                    have = cur_pay != IVF_NO_ROW;   // (of THIS tile's row: read when it was requested)
                    pay = IVF_NO_ROW;
                }
                const int64_t rn = r + kBlock;   // the next tile's row is requested before this one is summed
                if (rn < e && (!MASKED || ivf_mask_bit(lmask, rn))) {
                    v = __builtin_nontemporal_load(reinterpret_cast<const ivf_u32x4 *>(codes) + rn);
                    pay = entry[rn];
                }
                if constexpr (MASKED) {
                    if (tiles && !ivf_mask_any_tile(lmask, base, base + kBlock < e ? base + kBlock : e)) continue;  // workgroup-uniform: a tile without an allowed row
                }
                if (have) sc = ivf_score16(lut, cur);
                ivf_offer<CAP, TRIG>(tk, k, tile, have, ivf_key(sc), cur_pay);
            } else {
                if constexpr (MASKED) {
                    if (tiles && !ivf_mask_any_tile(lmask, base, base + kBlock < e ? base + kBlock : e)) continue;  // workgroup-uniform, as above
                    have = have && ivf_mask_bit(lmask, r);
                }
                uint32_t p = 0;
                if (have) {
                    sc = ivf_score_row(lut, codes + r * M, M);
                    p = entry[r];
                }
                ivf_offer<CAP, TRIG>(tk, k, tile, have, ivf_key(sc), p);
            }
            ++tile;
        }
        // (every tile ended with a barrier: the table and the residual may be overwritten)
    }
    int cnt = 0;
    if (tile > 0) {  // workgroup-uniform; a workgroup that met no row has nothing to sort
        __syncthreads();
        topk_compact(tk, k);
        cnt = tk.cnt[0];
    }
    if (part) {
        unsigned long long *o = part + ((qi * groups + g) * pieces + piece) * k;
        for (int i = tid; i < k; i += kBlock) o[i] = i < cnt ? tk.buf[0][i] : IVF_NONE;
    } else {
        for (int i = tid; i < k; i += kBlock) {
            const unsigned long long w = i < cnt ? tk.buf[0][i] : 0ull;
            out_d[qi * k + i] = __uint_as_float(i < cnt ? (uint32_t)(w >> 32) : 0x7f800000u);
            out_id[qi * k + i] = i < cnt ? id_base + (int64_t)(uint32_t)w : -1;
        }
    }
}

// one workgroup per query: the k smallest words of its `parts` sorted partial lists
template <int CAP, int TRIG>
__global__ __launch_bounds__(kBlock) void ivf_merge_kernel(const unsigned long long *__restrict__ part, int n_cand, int k, int64_t id_base,
                                                           float *__restrict__ out_d, int64_t *__restrict__ out_id)
{
    __shared__ TopKShared<1, CAP> tk;
    const int64_t qi = blockIdx.x;
    const int tid = threadIdx.x;
    const unsigned long long *in = part + qi * n_cand;
    topk_init(tk);
    __syncthreads();
    int tile = 0;
    for (int base = 0; base < n_cand; base += kBlock, ++tile) {
        const int i = base + tid;
        const unsigned long long w = i < n_cand ? in[i] : IVF_NONE;
        ivf_offer<CAP, TRIG>(tk, k, tile, w != IVF_NONE, (uint32_t)(w >> 32), (uint32_t)w);
    }
    __syncthreads();
    topk_compact(tk, k);
    const int cnt = tk.cnt[0];
    for (int i = tid; i < k; i += kBlock) {
        const unsigned long long w = i < cnt ? tk.buf[0][i] : 0ull;
        out_d[qi * k + i] = __uint_as_float(i < cnt ? (uint32_t)(w >> 32) : 0x7f800000u);
        out_id[qi * k + i] = i < cnt ? id_base + (int64_t)(uint32_t)w : -1;
    }
}

// Grid rules (pure host logic).  Wanted: at least two workgroups per CU.
//   1  nq alone gives that: G = nprobe, one workgroup per query walks all its lists whole -- no partial lists, no merge;
//   2  otherwise the probe slots of a query are cut into groups of G (down to one list per workgroup);
//   3  if that is still short and some list is long, lists are cut into pieces of >= 1024 rows (a piece rebuilds the table, so
//      shorter ones would pay more for tables than for rows); with rule 1 in force lists stay whole however long they are;
//   4  partial lists that exceed part_cap bytes halve the pieces, then the groups, until they fit (down to rule 1's shape).
IvfPlan plan_ivf_search(int64_t nq, int nprobe, int k, int64_t longest, size_t part_cap, int cus)
{
    IvfPlan p;
    if (cus <= 0) cus = device_cus();
    const int64_t want = 2 * (int64_t)cus;
    if (nq < 1) nq = 1;
    int groups = (int)std::min<int64_t>(nprobe, (want + nq - 1) / nq);
    groups = std::max(groups, 1);
    p.G = (nprobe + groups - 1) / groups;
    p.groups = (nprobe + p.G - 1) / p.G;
    p.rows_per_piece = (int)std::min<int64_t>(std::max<int64_t>(longest, 1), 0x7fffff00);
    p.pieces = 1;
    p.rule = p.groups > 1 ? 2 : 1;
    if (nq * p.groups < want && longest > 1024) {
        const int64_t wp = (want + nq * p.groups - 1) / (nq * p.groups);
        int64_t rpp = ((longest + wp - 1) / wp + kBlock - 1) / kBlock * kBlock;
        rpp = std::max<int64_t>(rpp, 1024);
        if (rpp < longest) {
            p.rows_per_piece = (int)rpp;
            p.pieces = (int)((longest + rpp - 1) / rpp);
            p.rule = 3;
        }
    }
    while (p.parts() > 1 && (size_t)nq * p.parts() * k * sizeof(unsigned long long) > part_cap) {
        if (p.pieces > 1) {
            p.pieces = (p.pieces + 1) / 2;
            p.rows_per_piece = (int)(((longest + p.pieces - 1) / p.pieces + kBlock - 1) / kBlock * kBlock);
            p.pieces = (int)((longest + p.rows_per_piece - 1) / p.rows_per_piece);
        } else {
            const int gr = (p.groups + 1) / 2;
            p.G = (nprobe + gr - 1) / gr;
            p.groups = (nprobe + p.G - 1) / p.G;
        }
        p.rule = 4;
    }
    return p;
}

size_t ivf_part_bytes(const IvfPlan &p, int64_t nq, int k)
{
    return p.parts() > 1 ? (size_t)nq * p.parts() * k * sizeof(unsigned long long) : 0;
}

size_t ivf_mask_bytes(int64_t n_csr) { return (size_t)std::max<int64_t>((n_csr + 63) / 64, 2) * 8; }

int launch_ivf_mask_order(const uint64_t *mask, const uint32_t *entry, int64_t n_csr, uint64_t *lmask, hipStream_t st)
{
    if (n_csr <= 0) return CVTMI_OK;   // no row, no word: every list is empty and the scan never asks
    if (!mask || !entry || !lmask) return fail(CVTMI_EINVAL, "search_ivf_masked: bad arguments");
    return launch("ivf_mask_order_kernel", ivf_mask_order_kernel, blocks_for(n_csr, kBlock), kBlock, 0, st, reinterpret_cast<const unsigned long long *>(mask), entry,
                  n_csr, reinterpret_cast<unsigned long long *>(lmask));
}

int launch_ivf_search(const OpqModelDev &m, const float *q_rot, int64_t nq, int nprobe, const int32_t *probe, const int64_t *list_off,
                      const uint8_t *codes, const uint32_t *entry, int k, int64_t id_base, const IvfPlan &p, void *part, float *out_d,
                      int64_t *out_id, hipStream_t st, const uint64_t *lmask)
{
    if (nq <= 0) return CVTMI_OK;
    if (m.K > 256) return fail(CVTMI_EUNSUPPORTED, "search_ivf: K=%d > 256", m.K);
    if (m.M > 16) return fail(CVTMI_EUNSUPPORTED, "search_ivf: M=%d > 16", m.M);
    if (k < 1 || k > kBigK) return fail(CVTMI_EUNSUPPORTED, "search_ivf: k=%d outside 1..%d", k, kBigK);
    const int parts = p.parts();
    const int64_t blocks = nq * parts;
    if ((int64_t)parts * k > 0x7fffffff) return fail(CVTMI_EUNSUPPORTED, "search_ivf: grid too large");
    if (parts > 1 && !part) return fail(CVTMI_EINVAL, "search_ivf: no room for partial lists");
    unsigned long long *pw = parts > 1 ? static_cast<unsigned long long *>(part) : nullptr;
    const size_t lds = ((size_t)((m.D + 3) & ~3) + (size_t)m.M * 256) * sizeof(float);
    if (lds + (k <= 128 ? sizeof(TopKShared<1, IVF_CAP>) : sizeof(TopKShared<1, kBigCap>)) > ((size_t)64 << 10))
        return fail(CVTMI_EUNSUPPORTED, "search_ivf: D=%d does not fit the workgroup's LDS", m.D);
    const bool small = k <= 128;   // the selection buffer of block_topk.h that holds k
    const unsigned long long *lm = reinterpret_cast<const unsigned long long *>(lmask);
    auto kern = lm ? (small ? ivf_search_kernel<IVF_CAP, IVF_TRIG, true> : ivf_search_kernel<kBigCap, kBigTrig, true>)
                   : (small ? ivf_search_kernel<IVF_CAP, IVF_TRIG, false> : ivf_search_kernel<kBigCap, kBigTrig, false>);
    CVTMI_TRY(launch(lm ? "ivf_search_kernel<masked>" : "ivf_search_kernel", kern, blocks, kBlock, lds, st, q_rot, m.D, m.M, m.K,
                     m.step, m.coarse, m.books, nprobe, probe, list_off, codes, entry, k, p.G, p.groups, p.pieces, p.rows_per_piece, id_base, out_d, out_id, pw, lm));
    if (parts > 1)
        CVTMI_TRY(launch("ivf_merge_kernel", small ? ivf_merge_kernel<IVF_CAP, IVF_TRIG> : ivf_merge_kernel<kBigCap, kBigTrig>, nq, kBlock, 0, st, pw, parts * k, k, id_base, out_d,
                         out_id));
    return CVTMI_OK;
}

}  // namespace cvtmi
