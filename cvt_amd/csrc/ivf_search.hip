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
#include <algorithm>

#include "block_topk.h"
#include "ivf_table.h"
#include "kernels.h"
#include "launch.h"

namespace cvtmi {

constexpr int IVF_CAP = 512, IVF_TRIG = 384;   // k <= 128; larger k: kBigCap / kBigTrig, as the generic exact scan
constexpr unsigned long long IVF_NONE = ~0ull; // an empty slot of a partial list (no entry has key KEY_MAX)

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

// part == nullptr: the workgroup holds everything of its query (one group, one piece) and writes the result rows itself;
// otherwise it writes its k best as sorted (key << 32 | insertion index) words to partial list (group * pieces + piece) of the query
template <int CAP, int TRIG>
__global__ __launch_bounds__(kBlock) void ivf_search_kernel(const float *__restrict__ q_rot, int D, int M, int K, int step,
                                                            const float *__restrict__ coarse, const float *__restrict__ books, int nprobe,
                                                            const int32_t *__restrict__ probe, const int64_t *__restrict__ list_off,
                                                            const uint8_t *__restrict__ codes, const uint32_t *__restrict__ entry, int k, int G,
                                                            int groups, int pieces, int rows_per_piece, int64_t id_base,
                                                            float *__restrict__ out_d, int64_t *__restrict__ out_id,
                                                            unsigned long long *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];  // res[D rounded up to 4] + lut[M][256]
    __shared__ TopKShared<1, CAP> tk;
    float *res = sm;
    float *lut = sm + ((D + 3) & ~3);
    const int piece = (int)(blockIdx.x % (unsigned)pieces);
    const int64_t qg = blockIdx.x / (unsigned)pieces;
    const int g = (int)(qg % groups);
    const int64_t qi = qg / groups;
    const int tid = threadIdx.x;
    topk_init(tk);
    __syncthreads();
    const int s0 = g * G, s1 = s0 + G < nprobe ? s0 + G : nprobe;
    int tile = 0;
    for (int s = s0; s < s1; ++s) {
        const int l = probe[qi * nprobe + s];
        if (l < 0) continue;  // workgroup-uniform
        const int64_t b = list_off[l] + (int64_t)piece * rows_per_piece;
        int64_t e = b + rows_per_piece;
        e = e < list_off[l + 1] ? e : list_off[l + 1];
        if (b >= e) continue;  // workgroup-uniform: an empty list, or a piece past its end
        // the first tile's rows are on their way while the table is built
        ivf_u32x4 v = { 0u, 0u, 0u, 0u };
        uint32_t pay = 0;
        if (M == 16 && b + tid < e) {
            v = __builtin_nontemporal_load(reinterpret_cast<const ivf_u32x4 *>(codes) + (b + tid));
            pay = entry[b + tid];
        }
        ivf_build_table(res, lut, q_rot + qi * D, coarse + (int64_t)l * D, books, D, M, K, step, tid);
        for (int64_t base = b; base < e; base += kBlock, ++tile) {
            const int64_t r = base + tid;
            const bool have = r < e;
            float sc = 0.0f;
            if (M == 16) {
                const ivf_u32x4 cur = v;
                const uint32_t cur_pay = pay;
                const int64_t rn = r + kBlock;   // the next tile's row is requested before this one is summed
                if (rn < e) {
                    v = __builtin_nontemporal_load(reinterpret_cast<const ivf_u32x4 *>(codes) + rn);
                    pay = entry[rn];
                }
                if (have) sc = ivf_score16(lut, cur);
                ivf_offer<CAP, TRIG>(tk, k, tile, have, ivf_key(sc), cur_pay);
            } else {
                uint32_t p = 0;
                if (have) {
                    sc = ivf_score_row(lut, codes + r * M, M);
                    p = entry[r];
                }
                ivf_offer<CAP, TRIG>(tk, k, tile, have, ivf_key(sc), p);
            }
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

int launch_ivf_search(const OpqModelDev &m, const float *q_rot, int64_t nq, int nprobe, const int32_t *probe, const int64_t *list_off,
                      const uint8_t *codes, const uint32_t *entry, int k, int64_t id_base, const IvfPlan &p, void *part, float *out_d,
                      int64_t *out_id, hipStream_t st)
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
    CVTMI_TRY(launch("ivf_search_kernel", small ? ivf_search_kernel<IVF_CAP, IVF_TRIG> : ivf_search_kernel<kBigCap, kBigTrig>, blocks, kBlock, lds, st, q_rot, m.D, m.M, m.K,
                     m.step, m.coarse, m.books, nprobe, probe, list_off, codes, entry, k, p.G, p.groups, p.pieces, p.rows_per_piece, id_base, out_d, out_id, pw));
    if (parts > 1)
        CVTMI_TRY(launch("ivf_merge_kernel", small ? ivf_merge_kernel<IVF_CAP, IVF_TRIG> : ivf_merge_kernel<kBigCap, kBigTrig>, nq, kBlock, 0, st, pw, parts * k, k, id_base, out_d,
                         out_id));
    return CVTMI_OK;
}

}  // namespace cvtmi
