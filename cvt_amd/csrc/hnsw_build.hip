// hnsw_build.hip -- batch-synchronous construction of a HierarchicalNSW graph (hnsw_sifts_retrieval/hnswlib/hnswalg.h:584-684).
//
// The rows are inserted in batches of consecutive rows.  Every row of a batch runs the reference's insertion against the graph as
// the earlier batches left it (rows of one batch do not see each other), then the batch's back links are applied, per target node
// in increasing (level, source id).  A batch of one row is the reference's sequential addPoint.  Per batch, on one stream, no host
// synchronisation (the host knows every level in advance, so it knows the entry point and the top level before each batch):
//   1. hnsw_build_search_kernel  one wave per row: greedy descent through the levels above the row's own, then searchBaseLayer
//                                (:152-216) with ef_construction on each of its levels from the same entry, leaving the result
//                                queue in its heap layout -- the search kernel's machinery (hnsw_heap.h, dist_f32.h);
//   2. hnsw_build_select_kernel  one wave per (row, level): getNeighborsByHeuristic2(M) (:283-325) and the row's own list in the
//                                order the reference pops it (:346-376); the list entries become back-link proposals;
//   3. hnsw_build_count / _reserve / _scatter  proposals bucketed by target node (a counting pass, atomics decide only WHERE a
//                                proposal is stored, never the order it is applied in);
//   4. hnsw_build_link_kernel    one wave per target: its proposals in increasing (level, source), each exactly as the inner loop of
//                                mutuallyConnectNewElement applies it (:383-441): append while there is room, else re-select with
//                                getNeighborsByHeuristic2(Mcurmax) over (d(new, t), new) and the current list.
// A memset of four counters opens each batch: seven launches per batch.
// cvtmi_hnsw_build starts from an empty graph (row 0 seeds it), cvtmi_hnsw_add from the graph a handle holds: the same batches, the
// schedule continued from the rows already there (launch_hnsw_build: `first`, and the entry point and top level at that row).
#include <atomic>
#include <chrono>
#include <vector>

#include "dist_f32.h"
#include "hnsw_heap.h"
#include "host_util.h"
#include "kernels.h"
#include "launch.h"

namespace cvtmi {

struct HbCounters { unsigned ticket, touched, alloc, pad; };

struct HbArgs {
    const float *vec;          // [n][D], every row present from the start (only rows < row0 are reachable)
    uint32_t *links0;          // [n][maxM0 + 1]
    const int64_t *upper_off;  // [n]
    uint32_t *upper;
    const int32_t *levels;     // [rows] drawn levels of this batch's rows
    int D, M, maxM, maxM0, efc;
    // this batch
    int64_t row0;
    int rows, ntask, maxlevel;
    uint32_t enterpoint;
    const int32_t *tbase;      // [rows]: first task of the row (its task for level l is tbase + l)
    const int32_t *task_row;   // [ntask]
    const int32_t *task_lv;    // [ntask]
    // scratch
    HnEnt *res;                // [ntask][efc + 1] result heaps
    int32_t *res_n;            // [ntask]
    uint32_t *prop;            // [ntask][M] proposals (targets); sources / levels are the task's
    int32_t *prop_n;           // [ntask]
    int32_t *cnt;              // [n] proposals per target (zero between batches)
    int32_t *slot_of;          // [n] target -> touched index
    uint32_t *touched;         // [ntask * M]
    int32_t *t_cnt, *t_off;    // [ntask * M]
    uint64_t *bucket;          // [ntask * M]: level << 32 | source
    HbCounters *ctr;
    uint32_t *visited;         // [slots][words]
    HnEnt *cand_g;             // [slots][gcap + efc + 1]
    int64_t words, gcap;
    int top_lds;
    int *err;
    const uint32_t *dead;      // DEL: a bit per node, set = deleted (the handle's bitmap read as 32-bit words, like `visited`)
};

__device__ __forceinline__ const uint32_t *hb_list(const HbArgs &a, uint32_t id, int level)
{
    return level == 0 ? a.links0 + (int64_t)id * (a.maxM0 + 1) : a.upper + a.upper_off[id] + (int64_t)(level - 1) * (a.maxM + 1);
}

// ---- 1. construction traversal --------------------------------------------------------------------------------------------------
// DEL (cvtmi_hnsw_add on a graph with deleted nodes) is current hnswlib's searchBaseLayer / addPoint over marked
// nodes, the MASKED rule of hnsw_search_kernel with "allowed" = "not in a.dead": the descent walks dead nodes like live ones; on a
// level every accepted neighbour joins the candidate queue and only live ones the result queue; `lower` follows the result queue once
// it holds something (+inf until then); the walk stops on `-c.d > lower` only on a FULL result queue; and when the batch's entry point
// is dead it is pushed into every level's result queue after the walk (hnswlib's epDeleted step), so a graph whose live part cannot
// be reached still links something.  The candidate queue is bounded by the node count alone: the host gives it room for every node.
template <bool IP, int LANES, bool DEL>
__global__ __launch_bounds__(64, 8) void hnsw_build_search_kernel(const HbArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float hb_smem[];
    float *qs = hb_smem;
    HnEnt *top_l = reinterpret_cast<HnEnt *>(hb_smem + ((a.D + 3) & ~3));
    const int ef = a.efc;
    const int ef_cap = ef + 1;
    const int top_cap = ef_cap < a.top_lds ? ef_cap : a.top_lds;
    HnEnt *cand_l = top_l + top_cap;
    const int lane = threadIdx.x;
    const bool w = lane == 0;
    uint32_t *vis = a.visited + (int64_t)blockIdx.x * a.words;
    HnEnt *slot_g = a.cand_g + (int64_t)blockIdx.x * (a.gcap + ef_cap);
    const SplitArr top{ top_l, slot_g, w, top_cap };
    const SplitArr cand{ cand_l, slot_g + ef_cap, w, HN_LCAP };
    const int64_t cand_cap = HN_LCAP + a.gcap;
    auto dist = [&](uint32_t id) {
        float o[1];
        dist_f32_row<IP, LANES, 1>(a.vec + (int64_t)id * a.D, qs, a.D, o);
        return o[0];
    };

    for (;;) {
        // tickets as in hnsw_search_kernel: every lane executes the atomic, lane 0 adds
        const unsigned t = atomicAdd(&a.ctr->ticket, lane == 0 ? 1u : 0u);
        const int r = __builtin_amdgcn_readfirstlane((int)t);
        if (r >= a.rows) break;
        const int64_t row = a.row0 + r;
        const int lvl = a.levels[r];
        for (int i = lane; i < a.D; i += 64) qs[i] = a.vec[row * a.D + i];
        __builtin_amdgcn_s_waitcnt(0);
        __threadfence_block();

        // greedy descent (:629-652): the first neighbour that beats the running minimum, in list order
        uint32_t cur = a.enterpoint;
        float curdist = dist(cur);
        for (int level = a.maxlevel; level > lvl; --level) {
            bool changed = true;
            while (changed) {
                changed = false;
                const uint32_t *ll = hb_list(a, cur, level);
                const int size = (int)ll[0];
                for (int base = 0; base < size; base += 64) {
                    const int j = base + lane;
                    const bool act = j < size;
                    const uint32_t nb = act ? ll[1 + j] : cur;
                    const float o = dist(nb);
                    unsigned long long better = __ballot(act && o < curdist);
                    while (better) {
                        const int b = __ffsll((long long)better) - 1;
                        const float db = __shfl(o, b);
                        const uint32_t ib = (uint32_t)__shfl((int)nb, b);
                        if (db < curdist) { curdist = db; cur = ib; changed = true; }
                        better &= better - 1;
                        better &= __ballot(act && o < curdist);
                    }
                }
            }
        }

        // searchBaseLayer (:152-216) on every level of the row, each from the same entry (:660-667)
        const int top_level = lvl < a.maxlevel ? lvl : a.maxlevel;
        bool overflow = false;
        for (int level = top_level; level >= 0 && !overflow; --level) {
            for (int64_t i = lane; i < a.words; i += 64) vis[i] = 0u;
            __builtin_amdgcn_s_waitcnt(0);
            __threadfence_block();
            const int width = level == 0 ? a.maxM0 : a.maxM;
            int top_n = 0, cand_n = 0;
            {
                const float d0 = dist(cur);
                // (readfirstlane: `cur` is one value in all lanes, and the branch around the wave-wide push must be a scalar one)
                const bool live = !DEL || __builtin_amdgcn_readfirstlane((int)((a.dead[cur >> 5] >> (cur & 31)) & 1u)) == 0;
                if (live) hn_push(top, top_n, d0, cur, lane);
                hn_push(cand, cand_n, -d0, cur, lane);
                if (w) vis[cur >> 5] |= 1u << (cur & 31);
                __builtin_amdgcn_s_waitcnt(0);
            }
            float lower = (!DEL || top_n > 0) ? top.get(0).d : __uint_as_float(0x7f800000u);
            while (cand_n > 0) {
                const HnEnt c = cand.get(0);
                if (-c.d > lower && (!DEL || top_n >= ef)) break;
                const uint32_t *ll = hb_list(a, c.id, level);
                const uint32_t nb0 = lane < width ? ll[1 + lane] : 0u;
                const int size = (int)ll[0];
                hn_pop(cand, cand_n, lane);
                bool act = lane < size;
                const uint32_t nb = nb0;
                bool ok = true;
                if (act) {
                    const uint32_t bit = 1u << (nb & 31);
                    uint32_t dw = 0u;
                    if (DEL) dw = a.dead[nb >> 5];   // requested in the round trip of the visited bit
                    act = (atomicOr(&vis[nb >> 5], bit) & bit) == 0;
                    if (DEL) ok = (dw & bit) == 0;
                }
                float o = 0.0f;
                if (act) o = dist(nb);
                unsigned long long m = __ballot(act && (top_n < ef || lower > o));
                // the lanes' live bits as one wave-uniform word: the branch around the wave-wide result-queue operations is scalar
                const unsigned long long okm = DEL ? __ballot(ok) : ~0ull;
                while (m) {
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float d = __shfl(o, b);
                    const uint32_t id = (uint32_t)__shfl((int)nb, b);
                    if (lower > d || top_n < ef) {
                        if (cand_n >= cand_cap) { overflow = true; break; }
                        hn_push(cand, cand_n, -d, id, lane);   // traversed whether deleted or not
                        if (!DEL || ((okm >> b) & 1ull)) {
                            hn_push(top, top_n, d, id, lane);
                            if (top_n > ef) hn_pop(top, top_n, lane);
                        }
                        if (!DEL || top_n > 0) lower = top.get(0).d;
                        if (top_n >= ef) m &= __ballot(act && lower > o);
                    }
                }
                if (overflow) break;
            }
            if (overflow) break;
            if (DEL) {
                // a dead entry point never entered the queue through the walk (dead nodes do not): no duplicate
                const uint32_t ep = a.enterpoint;
                if (__builtin_amdgcn_readfirstlane((int)((a.dead[ep >> 5] >> (ep & 31)) & 1u)) != 0) {
                    const float de = dist(ep);
                    hn_push(top, top_n, de, ep, lane);
                    if (top_n > ef) hn_pop(top, top_n, lane);
                }
            }
            // the result queue, in its heap layout
            const int task = a.tbase[r] + level;
            HnEnt *out = a.res + (int64_t)task * ef_cap;
            for (int i = lane; i < top_n; i += 64) out[i] = top.get_l(i);
            if (w) a.res_n[task] = top_n;
        }
        if (overflow && w) atomicExch(a.err, 1);
    }
}

// ---- the heuristic (:283-325) on one wave -----------------------------------------------------------------------------------------
// queue_closest is a std::priority_queue of (-d, id) pairs: it yields increasing d, equal d by DECREASING id (-0 and +0 equal).  The
// key below orders floats as `<` does (+-0 folded) and stays a total order for any bit pattern, so the ranks are a permutation.
__device__ __forceinline__ int hb_fkey(float d)
{
    if (d == 0.0f) return 0;
    const int b = __float_as_int(d);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ bool hb_before(HnEnt x, HnEnt y)
{
    const int kx = hb_fkey(x.d), ky = hb_fkey(y.d);
    return kx < ky || (kx == ky && x.id > y.id);
}

// cand[0 .. m) in LDS, m >= lim: keeps at most `lim` of them and writes their ids to out[] in the order the reference pops its
// re-filled top_candidates (the kept pairs pushed in selection order, then popped); returns the count.  sorted / kept / heap: LDS.
template <bool IP, int LANES>
__device__ int hb_heuristic(const HnEnt *cand, int m, int lim, HnEnt *sorted, HnEnt *kept, HnEnt *heap, uint32_t *out,
                            const float *vec, int D, int lane)
{
    for (int i = lane; i < m; i += 64) {
        const HnEnt c = cand[i];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += hb_before(cand[j], c) ? 1 : 0;
        sorted[rank] = c;
    }
    __syncthreads();
    int nk = 0;
    for (int i = 0; i < m && nk < lim; ++i) {
        const HnEnt c = sorted[i];
        bool closer = false;
        if (lane < nk) {
            float o[1];
            dist_f32_row<IP, LANES, 1>(vec + (int64_t)kept[lane].id * D, vec + (int64_t)c.id * D, D, o);
            closer = o[0] < c.d;   // "closer to a kept neighbour than to the query": rejected (no side effects: any() decides)
        }
        if (__ballot(closer) == 0ull) {
            if (lane == 0) kept[nk] = c;
            ++nk;
            __syncthreads();
        }
    }
    const LdsArr h{ heap, lane == 0 };
    int hn = 0;
    for (int i = 0; i < nk; ++i) { const HnEnt e = kept[i]; hn_push(h, hn, e.d, e.id, lane); }
    for (int i = 0; i < nk; ++i) {
        if (lane == 0) out[i] = h.get(0).id;
        hn_pop(h, hn, lane);
    }
    __syncthreads();
    return nk;
}

// ---- 2. selection: one wave per (row, level) --------------------------------------------------------------------------------------
template <bool IP, int LANES>
__global__ __launch_bounds__(64) void hnsw_build_select_kernel(const HbArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float hb_smem[];
    const int ef_cap = a.efc + 1;
    HnEnt *cand = reinterpret_cast<HnEnt *>(hb_smem);
    HnEnt *sorted = cand + ef_cap;
    HnEnt *kept = sorted + ef_cap;
    HnEnt *heap = kept + 64;
    uint32_t *list = reinterpret_cast<uint32_t *>(heap + 64);
    const int lane = threadIdx.x;
    for (int t = blockIdx.x; t < a.ntask; t += gridDim.x) {
        const int64_t row = a.task_row[t];
        const int level = a.task_lv[t];
        int m = a.res_n[t];
        const HnEnt *src = a.res + (int64_t)t * ef_cap;
        for (int i = lane; i < m; i += 64) cand[i] = src[i];
        __syncthreads();
        int cnt = 0;
        if (m < a.M) {   // fewer than M candidates: the heuristic returns the queue untouched, popped as it stands
            const LdsArr h{ cand, lane == 0 };
            while (m > 0) {
                if (lane == 0) list[cnt] = h.get(0).id;
                ++cnt;
                hn_pop(h, m, lane);
            }
            __syncthreads();
        } else {
            cnt = hb_heuristic<IP, LANES>(cand, m, a.M, sorted, kept, heap, list, a.vec, a.D, lane);
        }
        // the row's own list (zero-initialised: entries past the count stay 0, as after the reference's memset)
        uint32_t *ll = const_cast<uint32_t *>(hb_list(a, (uint32_t)row, level));
        for (int i = lane; i < cnt; i += 64) {
            ll[1 + i] = list[i];
            a.prop[(int64_t)t * a.M + i] = list[i];
        }
        if (lane == 0) { ll[0] = (uint32_t)cnt; a.prop_n[t] = cnt; }
        __syncthreads();
    }
}

// ---- 3. bucketing of the proposals by target --------------------------------------------------------------------------------------
__global__ void hnsw_build_count_kernel(const HbArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.ntask * a.M) return;
    const int t = (int)(i / a.M), j = (int)(i % a.M);
    if (j >= a.prop_n[t]) return;
    const uint32_t tgt = a.prop[i];
    if (atomicAdd(&a.cnt[tgt], 1) == 0) {
        const unsigned k = atomicAdd(&a.ctr->touched, 1u);
        a.touched[k] = tgt;
        a.slot_of[tgt] = (int32_t)k;
    }
}
__global__ void hnsw_build_reserve_kernel(const HbArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (int64_t)a.ctr->touched) return;
    const uint32_t tgt = a.touched[k];
    const int c = a.cnt[tgt];
    a.t_cnt[k] = c;
    a.t_off[k] = (int32_t)atomicAdd(&a.ctr->alloc, (unsigned)c);
    a.cnt[tgt] = 0;
}
__global__ void hnsw_build_scatter_kernel(const HbArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.ntask * a.M) return;
    const int t = (int)(i / a.M), j = (int)(i % a.M);
    if (j >= a.prop_n[t]) return;
    const uint32_t tgt = a.prop[i];
    const int k = a.slot_of[tgt];
    const int pos = a.t_off[k] + atomicAdd(&a.cnt[tgt], 1);
    a.bucket[pos] = (uint64_t)a.task_lv[t] << 32 | (uint64_t)(uint32_t)a.task_row[t];
}

// ---- 4. back links: one wave per target ------------------------------------------------------------------------------------------
constexpr int HB_BUCKET_LDS = 2048;   // proposals of one target kept in LDS; more (hub nodes of large batches) are read from HBM

template <bool IP, int LANES>
__global__ __launch_bounds__(64) void hnsw_build_link_kernel(const HbArgs a)
{
    __shared__ uint64_t keys_l[HB_BUCKET_LDS];
    __shared__ HnEnt cand[72], sorted[72], kept[64], heap[64];
    __shared__ uint32_t lst[72], out[64];
    const int lane = threadIdx.x;
    const int ntouched = (int)a.ctr->touched;
    for (int k = blockIdx.x; k < ntouched; k += gridDim.x) {
        const uint32_t tgt = a.touched[k];
        const int c = a.t_cnt[k];
        const uint64_t *keys = a.bucket + a.t_off[k];
        if (c <= HB_BUCKET_LDS) {
            for (int i = lane; i < c; i += 64) keys_l[i] = keys[i];
            __syncthreads();
            keys = keys_l;
        }
        if (lane == 0) a.cnt[tgt] = 0;   // (ready for the next batch)
        const float *tv = a.vec + (int64_t)tgt * a.D;
        int cur_level = -1, mcur = 0;
        uint32_t *gl = nullptr;
        uint64_t prev = 0;
        for (int step = 0; step < c; ++step) {
            // next proposal in increasing (level, source): the smallest key above the previous one (keys are distinct)
            uint64_t best = ~0ull;
            for (int i = lane; i < c; i += 64) {
                const uint64_t kk = keys[i];
                if ((step == 0 || kk > prev) && kk < best) best = kk;
            }
            for (int sh = 32; sh >= 1; sh >>= 1) {
                const uint64_t o = (uint64_t)__shfl_xor((long long)best, sh);
                best = o < best ? o : best;
            }
            prev = best;
            const int level = (int)(best >> 32);
            const uint32_t src = (uint32_t)best;
            if (level != cur_level) {
                if (cur_level >= 0) {
                    for (int i = lane; i <= mcur; i += 64) gl[i] = lst[i];
                    __syncthreads();
                }
                cur_level = level;
                mcur = level == 0 ? a.maxM0 : a.maxM;
                gl = const_cast<uint32_t *>(hb_list(a, tgt, level));
                for (int i = lane; i <= mcur; i += 64) lst[i] = gl[i];   // count, entries, and the stale words past the count
                __syncthreads();
            }
            const int sz = (int)lst[0];
            if (sz < mcur) {
                if (lane == 0) { lst[1 + sz] = src; lst[0] = (uint32_t)(sz + 1); }
                __syncthreads();
                continue;
            }
            // full: candidates (d(new, t), new), then the list in list order (d(x, t), x) (:400-411)
            for (int i = lane; i <= sz; i += 64) {
                const uint32_t id = i == 0 ? src : lst[i];
                float o[1];
                dist_f32_row<IP, LANES, 1>(a.vec + (int64_t)id * a.D, tv, a.D, o);
                HnEnt e; e.d = o[0]; e.id = id;
                cand[i] = e;
            }
            __syncthreads();
            const int nk = hb_heuristic<IP, LANES>(cand, sz + 1, mcur, sorted, kept, heap, out, a.vec, a.D, lane);
            for (int i = lane; i < nk; i += 64) lst[1 + i] = out[i];   // entries past nk keep what they held (:414-420)
            if (lane == 0) lst[0] = (uint32_t)nk;
            __syncthreads();
        }
        if (cur_level >= 0) {
            for (int i = lane; i <= mcur; i += 64) gl[i] = lst[i];
            __syncthreads();
        }
    }
}

// ---- host driver -----------------------------------------------------------------------------------------------------------------
// Default schedule: a batch holds at most 1 / "hnsw_build_frac" of the rows already in the graph (at least one), and at most "hnsw_build_cap" rows.
static double g_hb_ms[5];
static std::mutex g_hb_ms_mu;
void hnsw_build_phase_ms(double *ms)
{
    std::lock_guard<std::mutex> g(g_hb_ms_mu);
    for (int i = 0; i < 5; ++i) ms[i] = g_hb_ms[i];
}

struct HbBatch { int64_t s, e; int maxlevel; uint32_t ep; int64_t toff; int ntask; };
// Scratch the DEL traversals of one call may hold (visited bits + queues of n entries per slot): the budget of a masked search
// (api_hnsw.hip, kHnswMaskedScratch) -- every slot of a graph of up to 120 K nodes, about 1000 traversals in flight at 1 M.
constexpr size_t kHbDelScratch = (size_t)8 << 30;

// bounds of the batches that insert rows first .. n-1 into a graph of `first` rows whose top level is top0 (first == 0: row 0 seeds the
// graph alone, top0 is not read)
void hnsw_build_schedule(const int32_t *levels, int64_t first, int64_t n, int top0, int max_batch, std::vector<int64_t> &bounds)
{
    const int64_t frac = tune_hnsw_build_frac.geti();
    const int64_t cap = max_batch > 0 ? max_batch : tune_hnsw_build_cap.geti();
    bounds.clear();
    bounds.push_back(first);
    if (first >= n) return;
    int maxlevel = top0;
    int64_t s = first;
    if (first == 0) {
        bounds.push_back(1);   // row 0 seeds the graph
        maxlevel = levels[0];
        s = 1;
    }
    while (s < n) {
        int64_t b = s / frac;
        if (b < 1) b = 1;
        if (b > cap) b = cap;
        int64_t e = s + b < n ? s + b : n;
        for (int64_t i = s; i < e; ++i)
            if (levels[i - first] > maxlevel) { e = i + 1; maxlevel = levels[i - first]; break; }   // a row that raises the top level ends its batch
        bounds.push_back(e);
        s = e;
    }
}

// Inserts rows first .. g.n-1 into the graph of rows 0 .. first-1 (entry point ep0, top level top0; first == 0: an empty graph, row 0
// seeds it).  levels: the drawn levels of the inserted rows alone, [g.n - first].  stats (optional): { batches, largest batch }, the
// seed row counted as a batch; *launched (optional) is set once the first kernel that writes the graph is about to be enqueued --
// an error before that leaves the graph as it was.  Per call: the n-word cnt / slot_of arrays and one memset of n words.
int launch_hnsw_build(const char *who, const HnswDevGraph &g, uint32_t *links0, uint32_t *upper, const int32_t *levels, int64_t first,
                      uint32_t ep0, int top0, int metric, int M, int efc, int max_batch, int cus, hipStream_t st, int64_t *stats,
                      bool *launched, const uint64_t *dead)
{
    const auto h0 = std::chrono::steady_clock::now();
    const int64_t n = g.n, m = n - first;
    if (stats) stats[0] = stats[1] = 0;
    if (m <= 0) return CVTMI_OK;
    std::vector<int64_t> bounds;
    hnsw_build_schedule(levels, first, n, top0, max_batch, bounds);
    const int nb = (int)bounds.size() - 1;
    // tasks: (row, level) for every level a row is searched on, batch after batch
    std::vector<HbBatch> batches;
    std::vector<int32_t> tbase((size_t)m, 0), trow, tlv;
    int maxlevel = first == 0 ? levels[0] : top0;
    uint32_t ep = first == 0 ? 0u : ep0;
    int64_t tmax = 0, rmax = 0;
    for (int b = first == 0 ? 1 : 0; b < nb; ++b) {
        HbBatch B;
        B.s = bounds[b]; B.e = bounds[b + 1]; B.maxlevel = maxlevel; B.ep = ep; B.toff = (int64_t)trow.size();
        int32_t tb = 0;
        for (int64_t i = B.s; i < B.e; ++i) {
            const int li = levels[i - first];
            const int top = li < maxlevel ? li : maxlevel;
            tbase[(size_t)(i - first)] = tb;
            for (int l = 0; l <= top; ++l) { trow.push_back((int32_t)i); tlv.push_back(l); }
            tb += top + 1;
        }
        B.ntask = tb;
        if (levels[B.e - 1 - first] > maxlevel) { maxlevel = levels[B.e - 1 - first]; ep = (uint32_t)(B.e - 1); }
        tmax = tb > tmax ? tb : tmax;
        rmax = B.e - B.s > rmax ? B.e - B.s : rmax;
        batches.push_back(B);
    }
    if (stats) { stats[0] = nb; stats[1] = rmax > 1 ? rmax : 1; }
    if (batches.empty()) return CVTMI_OK;
    const int efc1 = efc + 1;
    const int64_t pmax = tmax * M;
    // traversal slots, as hnsw_plan sizes a search
    const int lds_search = hnsw_lds_bytes(g.D, efc);
    int per_cu = (159 * 1024) / lds_search;
    per_cu = per_cu > 32 ? 32 : (per_cu < 1 ? 1 : per_cu);
    int64_t slot_cap = (int64_t)cus * per_cu;
    const int64_t words_max = (n + 31) / 32 + 1;
    int64_t gcap = (int64_t)efc * g.maxM0 * 2;
    // DEL: while few live nodes have been found nothing is pruned and every visited node is queued; a node enters the queue at most
    // once, so room for n entries (HN_LCAP + gcap >= n) rules the overflow out, as hnsw_plan does for a masked search
    if (gcap > n || dead) gcap = n;
    gcap = (gcap > HN_LCAP ? gcap - HN_LCAP : 0) + 64;
    if (dead) {   // ... and the traversals in flight are bounded by the scratch they need (at least one)
        const size_t per_slot = (size_t)words_max * 4 + (size_t)(gcap + efc1) * sizeof(HnEnt);
        const int64_t fit = (int64_t)(kHbDelScratch / per_slot);
        if (slot_cap > fit) slot_cap = fit > 1 ? fit : 1;
    }
    const int64_t slots_max = slot_cap < rmax ? slot_cap : rmax;

    Tmp d_tbase, d_trow, d_tlv, d_lev, res, res_n, prop, prop_n, cnt, slot_of, touched, t_cnt, t_off, bucket, ctr, vis, candg, err;
    CVTMI_TRY(d_tbase.upload(tbase.data(), tbase.size() * 4));
    CVTMI_TRY(d_trow.upload(trow.data(), trow.size() * 4));
    CVTMI_TRY(d_tlv.upload(tlv.data(), tlv.size() * 4));
    CVTMI_TRY(d_lev.upload(levels, (size_t)m * 4));
    CVTMI_TRY(res.alloc((size_t)tmax * efc1 * sizeof(HnEnt)));
    CVTMI_TRY(res_n.alloc((size_t)tmax * 4));
    CVTMI_TRY(prop.alloc((size_t)pmax * 4));
    CVTMI_TRY(prop_n.alloc((size_t)tmax * 4));
    CVTMI_TRY(cnt.alloc((size_t)n * 4));
    CVTMI_TRY(slot_of.alloc((size_t)n * 4));
    CVTMI_TRY(touched.alloc((size_t)pmax * 4));
    CVTMI_TRY(t_cnt.alloc((size_t)pmax * 4));
    CVTMI_TRY(t_off.alloc((size_t)pmax * 4));
    CVTMI_TRY(bucket.alloc((size_t)pmax * 8));
    CVTMI_TRY(ctr.alloc(sizeof(HbCounters)));
    CVTMI_TRY(vis.alloc((size_t)slots_max * words_max * 4));
    CVTMI_TRY(candg.alloc((size_t)slots_max * (gcap + efc1) * sizeof(HnEnt)));
    CVTMI_TRY(err.alloc(16));
    CVTMI_HIP(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, st));
    CVTMI_HIP(hipMemsetAsync(err.p, 0, 16, st));

    HbArgs a;
    a.vec = g.vec; a.links0 = links0; a.upper_off = g.upper_off; a.upper = upper;
    a.D = g.D; a.M = M; a.maxM = g.maxM; a.maxM0 = g.maxM0; a.efc = efc;
    a.res = res.as<HnEnt>(); a.res_n = res_n.as<int32_t>(); a.prop = prop.as<uint32_t>(); a.prop_n = prop_n.as<int32_t>();
    a.cnt = cnt.as<int32_t>(); a.slot_of = slot_of.as<int32_t>(); a.touched = touched.as<uint32_t>();
    a.t_cnt = t_cnt.as<int32_t>(); a.t_off = t_off.as<int32_t>(); a.bucket = bucket.as<uint64_t>(); a.ctr = ctr.as<HbCounters>();
    a.visited = vis.as<uint32_t>(); a.cand_g = candg.as<HnEnt>(); a.gcap = gcap; a.top_lds = hnsw_top_lds(efc); a.err = err.as<int>();
    a.dead = reinterpret_cast<const uint32_t *>(dead);

    const bool ip = metric == CVTMI_METRIC_IP;
    const int lanes = (g.D % 4 != 0) ? 1 : (ip ? 4 : (g.D % 16 == 0 ? 8 : 4));
    const size_t sel_lds = (size_t)(2 * efc1 + 128) * sizeof(HnEnt) + 64 * 4 + 16;
    const bool timing = tune_hnsw_build_phases.geti() != 0;
    std::vector<hipEvent_t> ev;
    auto mark = [&]() -> int {
        if (!timing) return CVTMI_OK;
        hipEvent_t e;
        CVTMI_HIP(hipEventCreate(&e));
        ev.push_back(e);
        CVTMI_HIP(hipEventRecord(e, st));
        return CVTMI_OK;
    };
    // the <IP, LANES> instance of the three kernel families that suits the index
    static constexpr decltype(&hnsw_build_search_kernel<true, 4, false>) search_k[2][5] = {
        { hnsw_build_search_kernel<true, 4, false>, hnsw_build_search_kernel<true, 1, false>, hnsw_build_search_kernel<false, 8, false>,
          hnsw_build_search_kernel<false, 4, false>, hnsw_build_search_kernel<false, 1, false> },
        { hnsw_build_search_kernel<true, 4, true>, hnsw_build_search_kernel<true, 1, true>, hnsw_build_search_kernel<false, 8, true>,
          hnsw_build_search_kernel<false, 4, true>, hnsw_build_search_kernel<false, 1, true> } };
    static constexpr decltype(&hnsw_build_select_kernel<true, 4>) select_k[5] = {
        hnsw_build_select_kernel<true, 4>, hnsw_build_select_kernel<true, 1>, hnsw_build_select_kernel<false, 8>, hnsw_build_select_kernel<false, 4>,
        hnsw_build_select_kernel<false, 1> };
    static constexpr decltype(&hnsw_build_link_kernel<true, 4>) link_k[5] = {
        hnsw_build_link_kernel<true, 4>, hnsw_build_link_kernel<true, 1>, hnsw_build_link_kernel<false, 8>, hnsw_build_link_kernel<false, 4>,
        hnsw_build_link_kernel<false, 1> };
    const int form = ip ? (lanes == 4 ? 0 : 1) : (lanes == 8 ? 2 : lanes == 4 ? 3 : 4);
    const auto search = search_k[dead ? 1 : 0][form];
    const char *search_name = dead ? "hnsw_build_search_kernel<del>" : "hnsw_build_search_kernel";
    const auto select = select_k[form];
    const auto link = link_k[form];
    CVTMI_TRY(set_max_lds("hnsw_build_search_kernel", search, lds_search));
    CVTMI_TRY(set_max_lds("hnsw_build_select_kernel", select, sel_lds));
    const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
    CVTMI_TRY(mark());
    if (launched) *launched = true;
    for (const HbBatch &B : batches) {
        a.row0 = B.s; a.rows = (int)(B.e - B.s); a.ntask = B.ntask; a.maxlevel = B.maxlevel; a.enterpoint = B.ep;
        a.levels = d_lev.as<int32_t>() + (B.s - first);
        a.tbase = d_tbase.as<int32_t>() + (B.s - first);
        a.task_row = d_trow.as<int32_t>() + B.toff;
        a.task_lv = d_tlv.as<int32_t>() + B.toff;
        a.words = (B.s + 31) / 32 + 1;
        const int64_t slots = slot_cap < a.rows ? slot_cap : a.rows;
        const int64_t np = (int64_t)B.ntask * M;
        const int64_t pb = blocks_for(np, 256);
        CVTMI_HIP(hipMemsetAsync(ctr.p, 0, sizeof(HbCounters), st));
        CVTMI_TRY(launch(search_name, search, slots, 64, lds_search, st, a));
        CVTMI_TRY(mark());
        const int64_t sel_grid = B.ntask < (int64_t)cus * 32 ? B.ntask : (int64_t)cus * 32;
        CVTMI_TRY(launch("hnsw_build_select_kernel", select, sel_grid, 64, sel_lds, st, a));
        CVTMI_TRY(mark());
        CVTMI_TRY(launch("hnsw_build_count_kernel", hnsw_build_count_kernel, pb, 256, 0, st, a));
        CVTMI_TRY(launch("hnsw_build_reserve_kernel", hnsw_build_reserve_kernel, pb, 256, 0, st, a));
        CVTMI_TRY(launch("hnsw_build_scatter_kernel", hnsw_build_scatter_kernel, pb, 256, 0, st, a));
        const int64_t link_grid = np < (int64_t)cus * 16 ? np : (int64_t)cus * 16;
        CVTMI_TRY(launch("hnsw_build_link_kernel", link, link_grid > 0 ? link_grid : 1, 64, 0, st, a));
        CVTMI_TRY(mark());
    }
    CVTMI_HIP(hipStreamSynchronize(st));
    int e = 0;
    CVTMI_HIP(hipMemcpy(&e, err.p, 4, hipMemcpyDeviceToHost));
    if (timing) {
        double ms[5] = { 0, 0, 0, 0, host_ms };
        for (size_t i = 0; i + 3 < ev.size(); i += 3) {
            for (int j = 0; j < 3; ++j) {
                float t = 0.0f;
                (void)hipEventElapsedTime(&t, ev[i + j], ev[i + j + 1]);
                ms[j] += t;
            }
        }
        ms[3] = (double)batches.size();
        for (hipEvent_t x : ev) (void)hipEventDestroy(x);
        std::lock_guard<std::mutex> gl(g_hb_ms_mu);
        for (int i = 0; i < 5; ++i) g_hb_ms[i] = ms[i];
    }
    if (e) return fail(CVTMI_EUNSUPPORTED, "%s: candidate queue overflow", who);
    return CVTMI_OK;
}

}  // namespace cvtmi
