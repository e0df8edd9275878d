// ivf_range.hip -- every entry of the nprobe nearest coarse lists whose score is under a radius (cvtmi_opq_range_search_ivf).
//
// Probing, tables and scores are ivf_search.hip's (ivf_table.h); an entry is a hit when `score < radius` holds in fp32, the
// strict comparison IVFOPQ::Query's min(score, cell) fold makes against its threshold (opq/src/IVFOPQ.cpp:262, :308): NaN and
// +inf scores never hit.  The result has no fixed length, so the work is counted before it is placed:
//
//   order   per query its probed lists sorted by list id (-1 slots last).  Groups of G consecutive sorted slots then cover
//           ascending ranges of the list-ordered copy, and lists are cut into pieces only when a workgroup holds one list
//           (plan_ivf_range keeps G == 1 there): the parts of a query, in index order, are in the order of the copy.
//   scan    one workgroup per part, ivf_search_kernel's grid and row loop.  Per 256-row tile every wave ballots its hits, the four
//           wave counts meet in LDS, and a hit's rank inside the part is the running count + the waves before + the lanes before: no
//           atomics, the same order on every run.  Hits of rank < C go as (score bits << 32 | position in the copy) into the
//           part's own C-record segment of the spill area; the exact count of the part is always written.
//   offsets exclusive scan of the part counts per query, then of the query counts over the batch: lims (int64).
//   fill    only if lims[nq] <= cap (read on the device: nothing waits for the host).  A part whose hits all fit its segment
//           copies them to lims[f] + its offset, ids and video ids gathered at the recorded positions.
//   rescan  behind the fill, under the same predicate: the parts with more than C hits build their tables again, walk their rows
//           again and write the hits straight to their final places; the other workgroups exit at once.
#include <algorithm>

#include "ivf_table.h"
#include "kernels.h"
#include "launch.h"
#include "range_common.h"

namespace cvtmi {

struct IvfRangeArgs {
    const float *q_rot, *coarse, *books;
    int D, M, K, step, nprobe;
    const int32_t *order;      // [nq][nprobe] probed lists, ascending, -1 last
    const int64_t *list_off;
    const uint8_t *codes;
    const uint32_t *entry;
    const int32_t *videos;
    float radius;
    int G, groups, pieces, rows_per_piece;
    uint32_t C;                // spill records per part
    int64_t nq, cap, id_base;
    uint32_t *part_cnt, *part_off;   // [nq][parts]
    unsigned long long *spill;       // [nq][parts][C]
    int64_t *lims;                   // [nq + 1]
    float *dist;
    int64_t *ids;
    int32_t *video;                  // or null
};

__global__ __launch_bounds__(128) void ivf_range_order_kernel(const int32_t *__restrict__ probe, int nprobe, int32_t *__restrict__ order)
{
    __shared__ uint32_t key[128];
    const int64_t qi = blockIdx.x;
    const int t = threadIdx.x;
    if (t < nprobe) key[t] = (uint32_t)probe[qi * nprobe + t];   // (-1 orders last as 0xffffffff)
    __syncthreads();
    if (t >= nprobe) return;
    const uint32_t k = key[t];
    int rank = 0;
    for (int j = 0; j < nprobe; ++j) rank += (key[j] < k || (key[j] == k && j < t)) ? 1 : 0;
    order[qi * nprobe + rank] = (int32_t)k;
}

// The rows of part blockIdx.x = (query * groups + group) * pieces + piece, hits in the order of the copy.
// FINAL = false: hits of rank < C to the part's spill segment, the count to part_cnt.  FINAL = true: hits to their final places.
template <bool FINAL>
__device__ __forceinline__ void ivf_range_walk(const IvfRangeArgs &a, float *sm, uint32_t (*wcnt)[1][4])
{
    float *res = sm;
    float *lut = sm + ((a.D + 3) & ~3);
    const int64_t blk = blockIdx.x;
    const int piece = (int)(blockIdx.x % (unsigned)a.pieces);
    const int64_t qg = blockIdx.x / (unsigned)a.pieces;
    const int g = (int)(qg % a.groups);
    const int64_t qi = qg / a.groups;
    const int tid = threadIdx.x;
    const int M = a.M;
    int64_t out0 = 0;
    if (FINAL) out0 = a.lims[qi] + a.part_off[blk];
    const int s0 = g * a.G, s1 = s0 + a.G < a.nprobe ? s0 + a.G : a.nprobe;
    uint32_t run[1] = { 0 };   // hits of the part so far (workgroup-uniform)
    int tile = 0;
    for (int s = s0; s < s1; ++s) {
        const int l = a.order[qi * a.nprobe + s];
        if (l < 0) break;  // workgroup-uniform: only empty slots follow
        const int64_t b = a.list_off[l] + (int64_t)piece * a.rows_per_piece;
        int64_t e = b + a.rows_per_piece;
        e = e < a.list_off[l + 1] ? e : a.list_off[l + 1];
        if (b >= e) continue;  // workgroup-uniform: an empty list, or a piece past its end
        ivf_u32x4 v = { 0u, 0u, 0u, 0u };   // the first tile's rows are on their way while the table is built
        if (M == 16 && b + tid < e) v = __builtin_nontemporal_load(reinterpret_cast<const ivf_u32x4 *>(a.codes) + (b + tid));
        ivf_build_table(res, lut, a.q_rot + qi * a.D, a.coarse + (int64_t)l * a.D, a.books, a.D, M, a.K, a.step, tid);
        for (int64_t base = b; base < e; base += kBlock, ++tile) {
            const int64_t r = base + tid;
            const bool have = r < e;
            float sc = 0.0f;
            if (M == 16) {
                const ivf_u32x4 cur = v;
                const int64_t rn = r + kBlock;   // the next tile's row is requested before this one is summed
                if (rn < e) v = __builtin_nontemporal_load(reinterpret_cast<const ivf_u32x4 *>(a.codes) + rn);
                if (have) sc = ivf_score16(lut, cur);
            } else if (have) {
                sc = ivf_score_row(lut, a.codes + r * M, M);
            }
            const bool hit[1] = { have && sc < a.radius };
            range_rank<1>(wcnt, tile, hit, run, [&](int, uint32_t rank) {   // (holds a barrier)
                if (FINAL) {
                    const int64_t o = out0 + rank;
                    a.dist[o] = sc;
                    a.ids[o] = a.id_base + (int64_t)a.entry[r];
                    if (a.video) a.video[o] = a.videos[r];
                } else if (rank < a.C) {
                    a.spill[blk * a.C + rank] = ((unsigned long long)__float_as_uint(sc) << 32) | (uint32_t)r;
                }
            });
        }
        // (every thread passed the last tile's barrier after its last table read: the next list may overwrite res and lut)
    }
    if (!FINAL && tid == 0) a.part_cnt[blk] = run[0];
}

__global__ __launch_bounds__(kBlock) void ivf_range_scan_kernel(const IvfRangeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];  // res[D rounded up to 4] + lut[M][256]
    __shared__ uint32_t wcnt[2][1][4];
    ivf_range_walk<false>(a, sm, wcnt);
}

__global__ __launch_bounds__(kBlock) void ivf_range_rescan_kernel(const IvfRangeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ uint32_t wcnt[2][1][4];
    if (a.lims[a.nq] > a.cap || a.part_cnt[blockIdx.x] <= a.C) return;   // workgroup-uniform
    ivf_range_walk<true>(a, sm, wcnt);
}

__global__ __launch_bounds__(kBlock) void ivf_range_fill_kernel(const IvfRangeArgs a)
{
    const int64_t blk = blockIdx.x;
    const uint32_t cnt = a.part_cnt[blk];
    if (a.lims[a.nq] > a.cap || cnt == 0 || cnt > a.C) return;
    const int64_t qi = blk / ((int64_t)a.groups * a.pieces);
    const int64_t out0 = a.lims[qi] + a.part_off[blk];
    const unsigned long long *in = a.spill + blk * a.C;
    for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) {
        const unsigned long long w = in[i];
        const uint32_t pos = (uint32_t)w;
        a.dist[out0 + i] = __uint_as_float((uint32_t)(w >> 32));
        a.ids[out0 + i] = a.id_base + (int64_t)a.entry[pos];
        if (a.video) a.video[out0 + i] = a.videos[pos];
    }
}

// ---- offsets, for both range searches (launch_range_offsets) ----
// one workgroup per query: part_off = exclusive scan of its part counts, lims[q + 1] = its hit count (summed over the batch below)
__global__ __launch_bounds__(kBlock) void range_part_offsets_kernel(const uint32_t *__restrict__ part_cnt, int parts,
                                                                    uint32_t *__restrict__ part_off, int64_t *__restrict__ lims)
{
    __shared__ uint32_t s[kBlock];
    const int64_t qi = blockIdx.x;
    uint32_t run = 0;   // (a query's hits are distinct rows or entries: fewer than 2^32)
    for (int base = 0; base < parts; base += kBlock) {
        const int i = base + threadIdx.x;
        const uint32_t v = i < parts ? part_cnt[qi * parts + i] : 0u;
        const uint32_t incl = range_block_scan(v, s);
        if (i < parts) part_off[qi * parts + i] = run + incl - v;
        run += s[kBlock - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) lims[qi + 1] = (int64_t)run;
}

// one workgroup: lims[0] = 0, lims[q + 1] = hits of queries 0 .. q
__global__ __launch_bounds__(kBlock) void range_lims_kernel(int64_t *__restrict__ lims, int64_t nq)
{
    __shared__ unsigned long long s[kBlock];
    unsigned long long run = 0;
    if (threadIdx.x == 0) lims[0] = 0;
    for (int64_t base = 0; base < nq; base += kBlock) {
        const int64_t i = base + threadIdx.x;
        const unsigned long long v = i < nq ? (unsigned long long)lims[i + 1] : 0ull;
        const unsigned long long incl = range_block_scan(v, s);
        if (i < nq) lims[i + 1] = (int64_t)(run + incl);
        run += s[kBlock - 1];
        __syncthreads();
    }
}

int launch_range_offsets(const RangeBufs &b, int parts, int64_t nq, int64_t *lims, hipStream_t st)
{
    CVTMI_TRY(launch("range_part_offsets_kernel", range_part_offsets_kernel, nq, kBlock, 0, st, b.part_cnt, parts, b.part_off, lims));
    return launch("range_lims_kernel", range_lims_kernel, 1, kBlock, 0, st, lims, nq);
}

// Grid rules (pure host logic): plan_ivf_search's rules 1-3 with nothing to merge, then
//   (order)  lists are cut into pieces only where a workgroup holds ONE list: with G > 1 the pieces of a group would interleave its
//            lists, and part index order would no longer be the order of the copy;
//   4        the spill area, nq x parts x C x 8 bytes, has to fit `cap_bytes`: C shrinks, down to 0 (every part with a hit is then
//            walked twice).  C is never more than the rows a part can hold.
IvfRangePlan plan_ivf_range(int64_t nq, int nprobe, int64_t longest, int64_t spill, size_t cap_bytes, int cus)
{
    IvfRangePlan p;
    p.grid = plan_ivf_search(nq, nprobe, 1, longest, ~(size_t)0, cus);
    IvfPlan &g = p.grid;
    if (g.pieces > 1 && g.G > 1) {
        g.pieces = 1;
        g.rows_per_piece = (int)std::min<int64_t>(std::max<int64_t>(longest, 1), 0x7fffff00);
        g.rule = 2;
    }
    const int64_t part_rows = g.pieces > 1 ? g.rows_per_piece : (int64_t)g.G * std::max<int64_t>(longest, 1);
    p.spill = std::max<int64_t>(0, std::min<int64_t>(std::min(spill, part_rows), 0x7fffffff));
    const int64_t fit = range_spill_fit(cap_bytes, nq, g.parts());
    if (p.spill > fit) {
        p.spill = fit;
        g.rule = 4;
    }
    return p;
}

size_t ivf_range_carve(void *base, const IvfRangePlan &p, int64_t nq, int nprobe, IvfRangeBufs *b)
{
    if (base && b) b->order = static_cast<int32_t *>(base);
    return range_carve(base, range_up16((size_t)nq * nprobe * sizeof(int32_t)), nq, p.grid.parts(), p.spill, b);
}

static int ivf_range_args(IvfRangeArgs &a, size_t &lds, const OpqModelDev &m, const float *q_rot, int64_t nq, int nprobe, const int64_t *list_off,
                          const uint8_t *codes, float radius, const IvfRangePlan &p, const IvfRangeBufs &b, int64_t *lims)
{
    if (m.K > 256) return fail(CVTMI_EUNSUPPORTED, "range_search_ivf: K=%d > 256", m.K);
    if (m.M > 16) return fail(CVTMI_EUNSUPPORTED, "range_search_ivf: M=%d > 16", m.M);
    if (nprobe < 1 || nprobe > 128) return fail(CVTMI_EUNSUPPORTED, "range_search_ivf: nprobe=%d outside 1..128", nprobe);
    lds = ((size_t)((m.D + 3) & ~3) + (size_t)m.M * 256) * sizeof(float);
    if (lds + 64 > ((size_t)64 << 10)) return fail(CVTMI_EUNSUPPORTED, "range_search_ivf: D=%d does not fit the workgroup's LDS", m.D);
    a = IvfRangeArgs{};
    a.q_rot = q_rot; a.coarse = m.coarse; a.books = m.books;
    a.D = m.D; a.M = m.M; a.K = m.K; a.step = m.step; a.nprobe = nprobe;
    a.order = b.order; a.list_off = list_off; a.codes = codes;
    a.radius = radius;
    a.G = p.grid.G; a.groups = p.grid.groups; a.pieces = p.grid.pieces; a.rows_per_piece = p.grid.rows_per_piece;
    a.C = (uint32_t)p.spill;
    a.nq = nq;
    a.part_cnt = b.part_cnt; a.part_off = b.part_off; a.spill = b.spill; a.lims = lims;
    return CVTMI_OK;
}

int launch_ivf_range_count(const OpqModelDev &m, const float *q_rot, int64_t nq, int nprobe, const int32_t *probe, const int64_t *list_off,
                           const uint8_t *codes, float radius, const IvfRangePlan &p, const IvfRangeBufs &b, int64_t *lims, hipStream_t st)
{
    if (nq <= 0) return CVTMI_OK;
    IvfRangeArgs a;
    size_t lds = 0;
    CVTMI_TRY(ivf_range_args(a, lds, m, q_rot, nq, nprobe, list_off, codes, radius, p, b, lims));
    const int parts = p.grid.parts();
    CVTMI_TRY(launch("ivf_range_order_kernel", ivf_range_order_kernel, nq, 128, 0, st, probe, nprobe, b.order));
    CVTMI_TRY(launch("ivf_range_scan_kernel", ivf_range_scan_kernel, nq * parts, kBlock, lds, st, a));
    return launch_range_offsets(b, parts, nq, lims, st);
}

int launch_ivf_range_fill(const OpqModelDev &m, const float *q_rot, int64_t nq, int nprobe, const int64_t *list_off, const uint8_t *codes,
                          const uint32_t *entry, const int32_t *videos, float radius, int64_t id_base, const IvfRangePlan &p,
                          const IvfRangeBufs &b, const int64_t *lims, int64_t cap, float *dist, int64_t *ids, int32_t *video, hipStream_t st)
{
    if (nq <= 0) return CVTMI_OK;
    IvfRangeArgs a;
    size_t lds = 0;
    CVTMI_TRY(ivf_range_args(a, lds, m, q_rot, nq, nprobe, list_off, codes, radius, p, b, const_cast<int64_t *>(lims)));
    a.entry = entry; a.videos = videos; a.id_base = id_base; a.cap = cap;
    a.dist = dist; a.ids = ids; a.video = video;
    const int64_t blocks = nq * p.grid.parts();
    if (p.spill > 0) CVTMI_TRY(launch("ivf_range_fill_kernel", ivf_range_fill_kernel, blocks, kBlock, 0, st, a));
    return launch("ivf_range_rescan_kernel", ivf_range_rescan_kernel, blocks, kBlock, lds, st, a);
}

}  // namespace cvtmi
