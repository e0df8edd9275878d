// hnsw.hip -- batched HNSW search over a graph built and saved by the reference:
// HierarchicalNSW::searchKnn (hnsw_sifts_retrieval/hnswlib/hnswalg.h:688-729) = greedy descent through the
// upper levels (:692-712), searchBaseLayerST (:217-280) with ef = max(ef_, k), then the k best.
//
// One wave per query (the traversal is a chain of dependent gathers: latency-bound, not roofline-bound;
// throughput comes from thousands of queries in flight).  What a wave does per expanded node:
//   * its <= 64 level-0 neighbours are taken one per lane: visited test-and-set on a per-query bitmap in
//     HBM, then every unvisited lane computes its neighbour's full distance in the reference's summation
//     order (dist_f32.h), reading its 4D-byte vector with 16-byte loads;
//   * the accept / push / pop decisions are replayed in list order, exactly as the scalar loop makes them.
// Both queues of the reference are std::priority_queue with CompareByFirst (:78-83), so ties between equal
// distances are decided by the binary-heap mechanics: push_heap / pop_heap of libstdc++ (__push_heap,
// __adjust_heap) are restated literally on arrays in LDS (the candidate queue spills to HBM past LCAP).
// With that, labels and distances are bit-identical to the reference's on the same graph, duplicates included.
#include <atomic>

#include "dist_f32.h"
#include "hnsw_heap.h"
#include "kernels.h"
#include "launch.h"

namespace cvtmi {

struct HnswArgs {
    const float *vec;         // [n][D]
    const uint32_t *links0;   // [n][maxM0 + 1]: count, then neighbours
    const int64_t *labels;    // [n]
    const int64_t *upper_off; // [n]: first word of the element's upper-level block in `upper`, -1 if none
    const uint32_t *upper;    // per element: levels x (maxM + 1) words
    int64_t n;
    int D, maxM, maxM0, maxlevel;
    uint32_t enterpoint;
    const float *q;           // fp32 mode: queries [nq][D]
    const float *lut;         // ADC mode: per-query tables [nq][M][K] (lut_kernel), codes [n][M]
    const uint8_t *codes;
    int M, K;
    int nq, k, ef;
    float *out_d;
    int64_t *out_label;
    uint32_t *visited;        // [slots][words]
    HnEnt *cand_g;            // [slots][gcap]
    int64_t words, gcap;
    int *err;
    int raw_ids;              // 1 = out_label receives internal ids instead of labels (the re-rank pass needs the node)
    int top_lds;              // entries of the top queue kept in LDS (the candidate queue: HN_LCAP)
    int dynamic;              // 1 = queries handed out by the counter err[1] (one ticket per wave), 0 = static stride
    const uint64_t *mask;     // MASKED instances: bit i & 63 of word i >> 6 lets node i into the result queue (ceil(n / 64) words)
};

// Distance evaluators: per-query state in LDS (`prepare`), one neighbour per lane (`operator()`).
template <bool IP, int LANES>
struct DistF32 {
    const HnswArgs &a;
    float *qs;
    __device__ __forceinline__ int smem_floats() const { return (a.D + 3) & ~3; }
    __device__ __forceinline__ void prepare(int qi, int lane) const
    {
        for (int i = lane; i < a.D; i += 64) qs[i] = a.q[(int64_t)qi * a.D + i];
    }
    __device__ __forceinline__ float operator()(uint32_t id) const
    {
        float o[1];
        dist_f32_row<IP, LANES, 1>(a.vec + (int64_t)id * a.D, qs, a.D, o);
        return o[0];
    }
    // level 0: nothing is fetched before the visited test (4 D bytes per neighbour is what bounds this traversal)
    struct Early {};
    __device__ __forceinline__ Early early(uint32_t) const { return Early(); }
    __device__ __forceinline__ float finish(uint32_t id, const Early &) const { return (*this)(id); }
};
// "HNSW over OPQ-compressed vectors": the node's M code bytes index the query's distance tables, summed in m
// order from +0.0f exactly as the ADC scan does (IVFOPQ.cpp:302-306) -- 16 bytes gathered per neighbour
// instead of 4 D.
// Where the fp32 tables live (round 5).  LDS_TABLES = true: copied into LDS per query (16 KB at M = 16: 8 query slots per CU, and 64 loads
// per lane before a traversal can start).  LDS_TABLES = false (default): read where lut_kernel left them -- a lane's 16 entries are 16
// independent 4-byte gathers from the query's 16 KB table (hot in L2 / Infinity Cache: a traversal touches it ~10^4 times), ONE more memory
// round trip per expanded node, the same one the fp32 traversal spends on its 4 D-byte vector gather -- and the slot shrinks to its two
// queues (4 KB): 32 traversals per CU instead of 8.  The traversal is latency-bound, so queries in flight are what it lives on.
template <bool LDS_TABLES>
struct DistADC {
    const HnswArgs &a;
    float *lds;          // [M][K] (LDS_TABLES)
    mutable const float *lut;
    __device__ __forceinline__ int smem_floats() const { return LDS_TABLES ? ((a.M * a.K + 3) & ~3) : 0; }
    __device__ __forceinline__ void prepare(int qi, int lane) const
    {
        const float *src = a.lut + (int64_t)qi * a.M * a.K;
        if (LDS_TABLES) {
            for (int i = lane; i < a.M * a.K; i += 64) lds[i] = src[i];
            lut = lds;
        } else {
            lut = src;
        }
    }
    __device__ __forceinline__ float sum16(const uint4 &v) const
    {
        const uint32_t w[4] = { v.x, v.y, v.z, v.w };
        float e[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) e[m] = lut[m * a.K + ((w[m >> 2] >> (8 * (m & 3))) & 0xffu)];   // 16 independent look-ups first
        float s = 0.0f;
#pragma unroll
        for (int m = 0; m < 16; ++m) s = __fadd_rn(s, e[m]);
        return s;
    }
    __device__ __forceinline__ float operator()(uint32_t id) const
    {
        const uint8_t *c = a.codes + (int64_t)id * a.M;
        if (a.M == 16) return sum16(*reinterpret_cast<const uint4 *>(c));  // one 16-byte gather per neighbour
        float s = 0.0f;
        for (int m = 0; m < a.M; ++m) s = __fadd_rn(s, lut[m * a.K + c[m]]);
        return s;
    }
    // level 0: a neighbour's 16 code bytes are requested together with its visited bit -- 1 KB per expanded node, and the traversal
    // is a chain of dependent round trips: this one now overlaps the test-and-set instead of following it
    struct Early { uint4 v; };
    __device__ __forceinline__ Early early(uint32_t id) const
    {
        Early e;
        e.v = make_uint4(0u, 0u, 0u, 0u);
        if (a.M == 16) e.v = *reinterpret_cast<const uint4 *>(a.codes + (int64_t)id * 16);
        return e;
    }
    __device__ __forceinline__ float finish(uint32_t id, const Early &e) const { return a.M == 16 ? sum16(e.v) : (*this)(id); }
};

// The result queue of searchKnn (:718-726) compares std::pair<dist_t, labeltype> with operator<: "neither distance is less" falls
// through to the label -- for equal distances, for +0.0f beside -0.0f, and for a NaN beside anything.
__device__ __forceinline__ bool hn_pair_less(float da, int64_t la, float db, int64_t lb)
{
    return da < db || (!(db < da) && la < lb);
}
__device__ __forceinline__ void hn_result_push_heap(float *od, int64_t *ol, int hole, float d, int64_t l)   // __push_heap on the pairs
{
    int parent = (hole - 1) / 2;
    while (hole > 0 && hn_pair_less(od[parent], ol[parent], d, l)) {
        od[hole] = od[parent]; ol[hole] = ol[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    od[hole] = d; ol[hole] = l;
}
// One lane, m <= k entries written in ascending pop order.  Without a NaN operator< is a strict weak order and labels are distinct,
// so the queue's output is THE ascending sequence: an insertion pass over runs of equivalent distances, every distance moving
// with its label.  With a NaN it is no order at all (NaN is "equivalent" to everything) and what the reference returns is a
// property of push_heap / pop_heap alone: they are replayed, pushes in pop order (back to front), pop_heap leaving each maximum
// at the end of the shrinking array -- which is the ascending output.
__device__ __forceinline__ void hn_order_result(float *od, int64_t *ol, int m, bool nan)
{
    if (!nan) {
        for (int i = 1; i < m; ++i) {
            const float d = od[i];
            const int64_t l = ol[i];
            int j = i - 1;
            while (j >= 0 && hn_pair_less(d, l, od[j], ol[j])) { od[j + 1] = od[j]; ol[j + 1] = ol[j]; --j; }
            if (j != i - 1) { od[j + 1] = d; ol[j + 1] = l; }
        }
        return;
    }
    for (int i = 0, j = m - 1; i < j; ++i, --j) {
        const float d = od[i]; od[i] = od[j]; od[j] = d;
        const int64_t l = ol[i]; ol[i] = ol[j]; ol[j] = l;
    }
    for (int i = 1; i < m; ++i) hn_result_push_heap(od, ol, i, od[i], ol[i]);
    for (int len = m - 1; len >= 1; --len) {   // __pop_heap + __adjust_heap
        const float vd = od[len];
        const int64_t vl = ol[len];
        od[len] = od[0]; ol[len] = ol[0];
        int hole = 0, second = 0;
        while (second < (len - 1) / 2) {
            second = 2 * (second + 1);
            if (hn_pair_less(od[second], ol[second], od[second - 1], ol[second - 1])) --second;
            od[hole] = od[second]; ol[hole] = ol[second];
            hole = second;
        }
        if ((len & 1) == 0 && second == (len - 2) / 2) {
            second = 2 * (second + 1);
            od[hole] = od[second - 1]; ol[hole] = ol[second - 1];
            hole = second - 1;
        }
        hn_result_push_heap(od, ol, hole, vd, vl);
    }
}

// MASKED (cvtmi_hnsw_search*_masked) is current hnswlib's searchBaseLayerST with isIdAllowed: a.mask decides what enters the RESULT
// queue and never what is traversed.  Every accepted neighbour joins the candidate queue, allowed or not; only allowed ones join the
// top queue; `lower` follows the top queue once it holds something (+inf until then); and the walk may stop on `-c.d > lower` only
// when the top queue is full -- while it is not, the candidate queue running empty is the only end.  With an all-ones mask every
// candidate is also in the top queue while that is not full, so `-c.d > lower` cannot hold then and the extra condition is vacuous:
// the unmasked result, bit for bit.  The candidate queue is no longer bounded by ef (nothing is pruned while few allowed nodes have
// been found): the plan gives it room for n entries, a node enters it at most once (its visited bit), so it cannot overflow and
// the loop ends.  The mask is read as 32-bit words, the same word index and bit as the visited bitmap (little-endian halves of the
// caller's uint64 words); a node id is < n, so nothing behind ceil(n / 64) words is read and bits past n are never looked at.
template <class DIST, bool MASKED>
__global__ __launch_bounds__(64, 8) void hnsw_search_kernel(const HnswArgs a)  // <= 64 VGPRs: 8 waves per SIMD, the traversal lives on queries in flight
{
    extern __shared__ __attribute__((aligned(16))) float hn_smem[];
    const DIST dist{ a, hn_smem };                                     // query state first (padded to 16 bytes; lut: set by prepare)
    HnEnt *top_l = reinterpret_cast<HnEnt *>(hn_smem + dist.smem_floats());
    const int ef_cap = (a.ef > a.k ? a.ef : a.k) + 1;   // the top queue never holds more than ef + 1 entries
    const int top_cap = ef_cap < a.top_lds ? ef_cap : a.top_lds;
    HnEnt *cand_l = top_l + top_cap;
    const int lane = threadIdx.x;
    const bool w = lane == 0;
    uint32_t *vis = a.visited + (int64_t)blockIdx.x * a.words;
    // per-slot HBM scratch: [top queue past HN_LCAP: ef + 1 entries][candidate queue past HN_LCAP: gcap entries]
    HnEnt *slot_g = a.cand_g + (int64_t)blockIdx.x * (a.gcap + ef_cap);
    const SplitArr top{ top_l, slot_g, w, top_cap };
    const SplitArr cand{ cand_l, slot_g + ef_cap, w, HN_LCAP };
    const int ef = a.ef > a.k ? a.ef : a.k;
    const int64_t cand_cap = HN_LCAP + a.gcap;

    // Queries are drawn from a counter (err[1], zeroed with the flag) instead of a static stride: traversals differ in length, and the last
    // of the 1.2 - 2.6 rounds used to wait for its slowest waves.  EVERY lane executes the atomic (a header that only lane 0 executes
    // lets the compiler send lane 0 and the other lanes through the loop on different paths, and the wave-level operations of the
    // body then run without lane 0 -- observed: the kernel never ended), but only lane 0 adds: its old value is a ticket that is
    // unique per wave whether or not the compiler folds the wave's atomics into one.
    for (int it = 0;; ++it) {
        int qi;
        if (a.dynamic) {
            const unsigned t = atomicAdd(reinterpret_cast<unsigned *>(a.err) + 1, lane == 0 ? 1u : 0u);
            qi = __builtin_amdgcn_readfirstlane((int)t);
        } else {
            qi = (int)blockIdx.x + it * (int)gridDim.x;
        }
        if (qi >= a.nq) break;
        dist.prepare(qi, lane);
        for (int64_t i = lane; i < a.words; i += 64) vis[i] = 0u;
        for (int i = lane; i < a.k; i += 64) { a.out_d[(int64_t)qi * a.k + i] = 0.0f; a.out_label[(int64_t)qi * a.k + i] = -1; }
        __builtin_amdgcn_s_waitcnt(0);
        __threadfence_block();
        if (a.n == 0) continue;

        // ---- upper levels: first minimum among the neighbours that beats the current distance (:692-712) ----
        uint32_t cur = a.enterpoint;
        float curdist = dist(cur);
        for (int level = a.maxlevel; level > 0; --level) {
            bool changed = true;
            while (changed) {
                changed = false;
                const uint32_t *ll = a.upper + a.upper_off[cur] + (int64_t)(level - 1) * (a.maxM + 1);
                const int size = (int)ll[0];
                for (int base = 0; base < size; base += 64) {
                    const int j = base + lane;
                    const bool act = j < size;
                    const uint32_t nb = act ? ll[1 + j] : cur;
                    float o[1];
                    o[0] = dist(nb);
                    // the scalar loop keeps the FIRST neighbour that reaches the running minimum
                    unsigned long long better = __ballot(act && o[0] < curdist);
                    while (better) {
                        const int b = __ffsll((long long)better) - 1;
                        const float db = __shfl(o[0], b);
                        const uint32_t ib = (uint32_t)__shfl((int)nb, b);
                        if (db < curdist) { curdist = db; cur = ib; changed = true; }
                        better &= better - 1;
                        better &= __ballot(act && o[0] < curdist);
                    }
                }
            }
        }

        // ---- level 0: searchBaseLayerST (:217-280) ----
        int top_n = 0, cand_n = 0;
        const uint32_t *mask32 = reinterpret_cast<const uint32_t *>(a.mask);
        {
            float o[1];
            o[0] = dist(cur);
            // (readfirstlane: `cur` holds one value in all 64 lanes, and the branch around the wave-wide push must be a scalar one)
            const bool ok = !MASKED || __builtin_amdgcn_readfirstlane((int)((mask32[cur >> 5] >> (cur & 31)) & 1u)) != 0;
            if (ok) hn_push(top, top_n, o[0], cur, lane);
            hn_push(cand, cand_n, -o[0], cur, lane);
            if (w) vis[cur >> 5] |= 1u << (cur & 31);
            __builtin_amdgcn_s_waitcnt(0);
        }
        float lower = (!MASKED || top_n > 0) ? top.get(0).d : __uint_as_float(0x7f800000u);
        bool overflow = false;
        while (cand_n > 0) {
            const HnEnt c = cand.get(0);
            if (-c.d > lower && (!MASKED || top_n >= ef)) break;   // under a mask the walk may only stop on a FULL result queue
            // the expanded node's links are requested BEFORE the pop walks the queue (the walk's deeper levels live in HBM): the two
            // latencies overlap instead of adding up
            // (count and first 64 neighbours in ONE round trip: a node's row always holds maxM0 + 1 words, stale ones past the count
            //  are masked below once the count is known)
            const uint32_t *ll = a.links0 + (int64_t)c.id * (a.maxM0 + 1);
            const uint32_t nb0 = lane < a.maxM0 ? ll[1 + lane] : 0u;
            const int size = (int)ll[0];
            hn_pop(cand, cand_n, lane);
            for (int base = 0; base < size; base += 64) {
                const int j = base + lane;
                bool act = j < size;
                const uint32_t nb = base == 0 ? nb0 : (act ? ll[1 + j] : 0u);
                typename DIST::Early pre = dist.early(act ? nb : c.id);
                bool ok = true;
                if (act) {
                    const uint32_t bit = 1u << (nb & 31);
                    // the neighbour's mask word is requested in the round trip of its visited bit (n / 8 bytes for all queries: L2-resident);
                    // a gather of its own would add one dependent round trip per expanded node
                    uint32_t mw = 0u;
                    if (MASKED) mw = mask32[nb >> 5];
                    act = (atomicOr(&vis[nb >> 5], bit) & bit) == 0;
                    if (MASKED) ok = (mw & bit) != 0;
                }
                float o[1] = { 0.0f };
                if (act) o[0] = dist.finish(nb, pre);
                // list order.  Once the top queue is full its maximum only falls, so a neighbour that fails `lower > d` now fails it
                // for the rest of this list: the rejected ones are dropped by ballot, and the walk visits accepted neighbours only
                // (MASKED: the same holds -- a full top queue stays full, and pushes into it still only lower its maximum)
                unsigned long long m = __ballot(act && (top_n < ef || lower > o[0]));
                // the lanes' mask bits as one wave-uniform word: the branch around the wave-wide top-queue operations below is scalar
                const unsigned long long okm = MASKED ? __ballot(ok) : ~0ull;
                while (m) {
                    const int b = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float d = __shfl(o[0], b);
                    const uint32_t id = (uint32_t)__shfl((int)nb, b);
                    if (lower > d || top_n < ef) {   // lower == top.get(0).d whenever the queue is non-empty
                        if (cand_n >= cand_cap) { overflow = true; break; }
                        hn_push(cand, cand_n, -d, id, lane);   // traversed whether allowed or not
                        if (!MASKED || ((okm >> b) & 1ull)) {
                            hn_push(top, top_n, d, id, lane);
                            if (top_n > ef) hn_pop(top, top_n, lane);
                        }
                        if (!MASKED || top_n > 0) lower = top.get(0).d;
                        if (top_n >= ef) m &= __ballot(act && lower > o[0]);
                    }
                }
                if (overflow) break;
            }
            if (overflow) break;
        }
        if (overflow) {
            if (w) atomicExch(a.err, 1);
            continue;
        }
        while (top_n > a.k) hn_pop(top, top_n, lane);
        // pops come out in non-increasing distance: write them back to front, then give them the order of the reference's result
        // queue (:718-726), a std::priority_queue of (dist, label) pairs that takes them in pop order
        const int m = top_n;
        bool nan = false;
        for (int i = m - 1; i >= 0; --i) {
            const HnEnt e = top.get(0);
            nan |= e.d != e.d;
            if (w) {
                a.out_d[(int64_t)qi * a.k + i] = e.d;
                a.out_label[(int64_t)qi * a.k + i] = a.raw_ids ? (int64_t)e.id : a.labels[e.id];
            }
            hn_pop(top, top_n, lane);
        }
        if (w) hn_order_result(a.out_d + (int64_t)qi * a.k, a.out_label + (int64_t)qi * a.k, m, nan);
    }
}

static void hnsw_fill_args(HnswArgs &a, const HnswDevGraph &g, int64_t nq, int k, int ef, float *out_d, int64_t *out_label,
                           uint32_t *visited, void *cand_scratch, int64_t words, int64_t gcap, int *err)
{
    a.vec = g.vec; a.links0 = g.links0; a.labels = g.labels; a.upper_off = g.upper_off; a.upper = g.upper;
    a.n = g.n; a.D = g.D; a.maxM = g.maxM; a.maxM0 = g.maxM0; a.maxlevel = g.maxlevel; a.enterpoint = g.enterpoint;
    a.q = nullptr; a.lut = nullptr; a.codes = nullptr; a.M = 0; a.K = 0;
    a.nq = (int)nq; a.k = k; a.ef = ef; a.out_d = out_d; a.out_label = out_label;
    a.visited = visited; a.cand_g = reinterpret_cast<HnEnt *>(cand_scratch); a.words = words; a.gcap = gcap; a.err = err;
    a.raw_ids = 0;
    a.dynamic = 1;
    a.top_lds = hnsw_top_lds(ef > k ? ef : k);
    a.mask = nullptr;
}

template <bool MASKED>
static decltype(&hnsw_search_kernel<DistF32<true, 4>, MASKED>) hnsw_f32_kernel(bool ip, int lanes)
{
    if (ip) return lanes == 4 ? hnsw_search_kernel<DistF32<true, 4>, MASKED> : hnsw_search_kernel<DistF32<true, 1>, MASKED>;
    if (lanes == 8) return hnsw_search_kernel<DistF32<false, 8>, MASKED>;
    if (lanes == 4) return hnsw_search_kernel<DistF32<false, 4>, MASKED>;
    return hnsw_search_kernel<DistF32<false, 1>, MASKED>;
}

int launch_hnsw_search(const HnswDevGraph &g, int metric, const float *q, int64_t nq, int k, int ef, float *out_d,
                       int64_t *out_label, uint32_t *visited, void *cand_scratch, int slots, int64_t words, int64_t gcap,
                       int *err, hipStream_t st, const uint64_t *mask)
{
    if (nq <= 0) return CVTMI_OK;
    HnswArgs a;
    hnsw_fill_args(a, g, nq, k, ef, out_d, out_label, visited, cand_scratch, words, gcap, err);
    a.q = q;
    a.mask = mask;
    const size_t lds = (size_t)hnsw_lds_bytes(g.D, ef > k ? ef : k);
    const bool ip = metric == CVTMI_METRIC_IP;
    const int lanes = (g.D % 4 != 0) ? 1 : (ip ? 4 : (g.D % 16 == 0 ? 8 : 4));
    if (mask) return launch_lds("hnsw_search_kernel<masked>", hnsw_f32_kernel<true>(ip, lanes), slots, 64, lds, st, a);
    return launch_lds("hnsw_search_kernel", hnsw_f32_kernel<false>(ip, lanes), slots, 64, lds, st, a);
}

// same traversal, distances = ADC over the nodes' PQ codes (codes [n][M] in internal-id order, lut [nq][M][K])
int launch_hnsw_search_adc(const HnswDevGraph &g, const float *lut, const uint8_t *codes, int M, int K, int64_t nq, int k, int ef,
                           float *out_d, int64_t *out_label, uint32_t *visited, void *cand_scratch, int slots, int64_t words,
                           int64_t gcap, int *err, hipStream_t st, int raw_ids, int state_floats, const uint64_t *mask)
{
    if (nq <= 0) return CVTMI_OK;
    HnswArgs a;
    hnsw_fill_args(a, g, nq, k, ef, out_d, out_label, visited, cand_scratch, words, gcap, err);
    a.lut = lut; a.codes = codes; a.M = M; a.K = K; a.raw_ids = raw_ids;
    a.mask = mask;
    // state_floats: what the caller sized the slots for (hnsw_adc_state_floats, read ONCE per search: M K = tables in LDS, 0 = in the scratch)
    const bool lds_tables = state_floats != 0;
    const size_t lds = (size_t)hnsw_lds_bytes(state_floats, ef > k ? ef : k);
    if (mask)
        return launch_lds("hnsw_search_kernel<masked>", lds_tables ? hnsw_search_kernel<DistADC<true>, true> : hnsw_search_kernel<DistADC<false>, true>,
                          slots, 64, lds, st, a);
    return launch_lds("hnsw_search_kernel", lds_tables ? hnsw_search_kernel<DistADC<true>, false> : hnsw_search_kernel<DistADC<false>, false>, slots, 64, lds, st, a);
}

// Exact re-rank of an ADC result list: ids [nq][R] internal ids (-1 = padding) -> out_d [nq][R] = the fp32 distance of the
// raw query to the node's own vector, in the summation order of the reference's distance functions (+inf for padding).
// One lane per candidate; a wave's 64 gathers of 4 D bytes are what the fp32 traversal pays per expanded node.
template <bool IP, int LANES>
__global__ __launch_bounds__(kBlock) void hnsw_rerank_kernel(const float *__restrict__ vec, int D, const float *__restrict__ q,
                                                             const int64_t *__restrict__ ids, int64_t total, int R,
                                                             float *__restrict__ out_d)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int64_t id = ids[i];
    float o[1] = { __uint_as_float(0x7f800000u) };
    if (id >= 0) dist_f32_row<IP, LANES, 1>(vec + id * D, q + (i / R) * D, D, o);
    out_d[i] = o[0];
}

int launch_hnsw_rerank(const HnswDevGraph &g, int metric, const float *q, int64_t nq, int R, const int64_t *ids, float *out_d,
                       hipStream_t st)
{
    const int64_t total = nq * R;
    if (total <= 0) return CVTMI_OK;
    const bool ip = metric == CVTMI_METRIC_IP;
    const int lanes = (g.D % 4 != 0) ? 1 : (ip ? 4 : (g.D % 16 == 0 ? 8 : 4));  // as launch_hnsw_search picks them
    decltype(&hnsw_rerank_kernel<true, 4>) kern;
    if (ip) { if (lanes == 4) kern = hnsw_rerank_kernel<true, 4>; else kern = hnsw_rerank_kernel<true, 1>; }
    else if (lanes == 8) kern = hnsw_rerank_kernel<false, 8>;
    else if (lanes == 4) kern = hnsw_rerank_kernel<false, 4>;
    else kern = hnsw_rerank_kernel<false, 1>;
    return launch("hnsw_rerank_kernel", kern, blocks_for(total, kBlock), kBlock, 0, st, g.vec, g.D, q, ids, total, R, out_d);
}

// ---- the delete state (cvtmi_hnsw_mark_deleted) ----
// hits: the bitmap the mark step of cvtmi_hnsw_mask_labels left (no bit past the nodes).  One word per thread; the flipped bits are
// counted by a popcount per word, summed over the wave and the workgroup, one atomic per workgroup that flipped something.
__global__ __launch_bounds__(kBlock) void hnsw_dead_fold_kernel(const unsigned long long *__restrict__ hits, unsigned long long *__restrict__ dead,
                                                                int64_t words, int unmark, unsigned long long *__restrict__ flipped)
{
    __shared__ int part[kBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int c = 0;
    if (i < words) {
        const unsigned long long old = dead[i], hit = hits[i];
        const unsigned long long now = unmark ? old & ~hit : old | hit;
        c = __popcll(old ^ now);
        if (c) dead[i] = now;
    }
    for (int sh = 32; sh >= 1; sh >>= 1) c += __shfl_xor(c, sh);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int j = 0; j < kBlock / 64; ++j) s += part[j];
        if (s) atomicAdd(flipped, (unsigned long long)s);
    }
}

int launch_hnsw_dead_fold(const uint64_t *hits, uint64_t *dead, int64_t words, int unmark, unsigned long long *flipped, hipStream_t st)
{
    if (words <= 0) return CVTMI_OK;
    return launch("hnsw_dead_fold_kernel", hnsw_dead_fold_kernel, blocks_for(words, kBlock), kBlock, 0, st,
                  reinterpret_cast<const unsigned long long *>(hits), reinterpret_cast<unsigned long long *>(dead), words, unmark, flipped);
}

// the mask of a search on a graph with dead nodes: what the caller allows (everything, without a mask of theirs) and is not dead
__global__ __launch_bounds__(kBlock) void hnsw_live_mask_kernel(const unsigned long long *__restrict__ dead, const unsigned long long *__restrict__ user,
                                                                unsigned long long *__restrict__ out, int64_t words, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= words) return;
    unsigned long long w = ~dead[i];
    if (user) w &= user[i];
    if (i == words - 1 && (n & 63)) w &= (1ull << (n & 63)) - 1ull;   // the caller's tail bits may hold anything
    out[i] = w;
}

int launch_hnsw_live_mask(const uint64_t *dead, const uint64_t *user, uint64_t *out, int64_t n, hipStream_t st)
{
    const int64_t words = (n + 63) / 64;
    if (words <= 0) return CVTMI_OK;
    return launch("hnsw_live_mask_kernel", hnsw_live_mask_kernel, blocks_for(words, kBlock), kBlock, 0, st,
                  reinterpret_cast<const unsigned long long *>(dead), reinterpret_cast<const unsigned long long *>(user),
                  reinterpret_cast<unsigned long long *>(out), words, n);
}

// LDS bytes of one query slot: query state (floats) + top queue (ef + 1) + the LDS part of the candidate queue
// Entries of the top queue (ef + 1) kept in LDS; the rest of it lives in HBM like the candidate queue's.  Keeping all of it in LDS (8 KB at
// ef = 1000) was measured: fp32 ef = 1000 174 K -> 151 K queries/s, ADC 101 K -> 97 K at 1 M nodes -- the query slots lost per CU cost more than
// the HBM levels of the heap walks, which the wave-wide pop already crosses in one or two round trips.  cvtmi_set_tuning("hnsw_top_lds", n),
// 0 = everything.
int hnsw_top_lds(int ef)
{
    const int cap = tune_hnsw_top_lds.geti();
    const int want = ef + 1;
    return cap > 0 && cap < want ? (cap < 16 ? 16 : cap) : want;
}
int hnsw_lds_bytes(int state_floats, int ef)
{
    return (int)(((state_floats + 3) & ~3) * sizeof(float) + (size_t)(hnsw_top_lds(ef) + HN_LCAP) * sizeof(HnEnt));
}
// cvtmi_set_tuning("hnsw_adc_tables"): 0 = a query's fp32 tables are read from the scratch lut_kernel wrote (default), 1 = copied into LDS
int hnsw_adc_state_floats(int MK) { return tune_hnsw_adc_tables.geti() ? MK : 0; }   // per-slot query state of the ADC traversal, in floats
int hnsw_ef_max() { return HN_EF_MAX; }
int hnsw_lcap() { return HN_LCAP; }

}  // namespace cvtmi
