// flat_range.hip -- every row of a flat index whose distance to a query is under a radius (cvtmi_flat_range_search).
//
// The distances are the exact flat kernels' (flat.hip), bit for bit: fp32 through dist_f32.h, uint8 as the exact integer
// |q|^2 + |x|^2 - 2<q,x> on v_dot4 over D / 4 * 4 bytes.  A row hits when its distance is under the threshold the host derived from
// the radius (api_flat.hip): `d < t` in fp32 -- NaN and +inf distances never hit -- or `d < T` in integers.  The result has no fixed
// length, so the work is counted before it is placed, with the structure of ivf_range.hip:
//
//   scan    one workgroup per (group of QT queries, part of the rows), one lane per row, every row read shared by the QT queries.
//           The rows are read as the handle holds them: fp32 in the 64-row blocked layout with the queries in SGPRs
//           (flat_f32_sq_kernel's loop) or row-major with the queries in LDS (flat_f32_kernel's), uint8 row-major with the packed
//           queries in LDS (flat_u8_kernel's).  Per 256-row tile every wave ballots its hits per query, the four wave counts meet in
//           LDS, and a hit's rank inside its (query, part) is the running count + the waves before + the lanes before: no atomics,
//           ascending rows, the same order on every run.  Hits of rank < C go as (distance bits << 32 | row) into the (query,
//           part)'s own C-record segment of the spill area; the exact count is always written.
//   offsets exclusive scan of the part counts per query, then of the query counts over the batch: lims (int64).
//   fill    only if lims[nq] <= cap (read on the device: nothing waits for the host).  A (query, part) whose hits all fit its
//           segment copies them to lims[query] + its offset, labels gathered (explicit) or offset by id_base (implicit).
//   rescan  behind the fill, under the same predicate: the workgroups with a (query, part) of more than C hits walk their rows
//           again and write those queries' hits straight to their final places; the others exit at once.
// Every position is 64-bit: nq * n hits can exceed 2^32.  Rows per handle stay under 2^32 (cvtmi_flat_add), so a row fits the
// record and a query's count fits 32 bits.
#include <algorithm>

#include "dist_f32.h"
#include "dist_u8.h"
#include "kernels.h"
#include "launch.h"
#include "range_common.h"

namespace cvtmi {

struct FlatRangeArgs {
    const void *data;
    const int32_t *norms;      // uint8 with norms: |x - 128|^2 per row (flat_u8_norms_kernel)
    const void *q;
    const int64_t *labels;     // stored labels, or null: id_base + row
    int64_t id_base;
    int64_t n, nq, cap;
    int D, parts;
    int64_t rows_per_part;     // whole 256-row tiles
    uint32_t thr;              // fp32: the bits of t; uint8: T
    uint32_t C;                // spill records per (query, part)
    uint32_t *part_cnt, *part_off;   // [nq][parts]
    unsigned long long *spill;       // [nq][parts][C]
    int64_t *lims;                   // [nq + 1]
    uint32_t *dist;                  // 4-byte fields: float bits / int32
    int64_t *out_labels;
};

// what a workgroup knows about its QT queries; everything here is workgroup-uniform
template <int QT>
struct FlatRangeGroup {
    int64_t group, row_begin, row_end;
    int64_t qi[QT];        // clamped to nq - 1: a padding query reads a real one and never hits
    int64_t cell[QT];      // query * parts + part
    int64_t out0[QT];      // FINAL: where the hits of the cell start
    bool active[QT];       // scan: a real query.  FINAL: a real query whose cell has more than C hits
    uint32_t run[QT];      // hits of the cell so far
};

// false: nothing to do for this workgroup
template <int QT, bool FINAL>
__device__ __forceinline__ bool flat_range_open(const FlatRangeArgs &a, FlatRangeGroup<QT> &g)
{
    if (FINAL && a.lims[a.nq] > a.cap) return false;
    const int part = (int)(blockIdx.x % (unsigned)a.parts);
    const int64_t group = blockIdx.x / (unsigned)a.parts;
    g.group = group;
    g.row_begin = (int64_t)part * a.rows_per_part;
    const int64_t e = g.row_begin + a.rows_per_part;
    g.row_end = e < a.n ? e : a.n;
    bool any = false;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        const int64_t qi = group * QT + q;
        g.active[q] = qi < a.nq;
        g.qi[q] = g.active[q] ? qi : a.nq - 1;
        g.cell[q] = g.qi[q] * a.parts + part;
        g.out0[q] = 0;
        g.run[q] = 0;
        if (FINAL) {
            g.active[q] = g.active[q] && a.part_cnt[g.cell[q]] > a.C;
            if (g.active[q]) g.out0[q] = a.lims[g.qi[q]] + (int64_t)a.part_off[g.cell[q]];
        }
        any = any || g.active[q];
    }
    return any && g.row_begin < g.row_end;
}

// one 256-row tile: `row` is this lane's row, hit[q] / bits[q] its verdict and distance for query q.  Holds one barrier.
template <int QT, bool FINAL>
__device__ __forceinline__ void flat_range_place(const FlatRangeArgs &a, FlatRangeGroup<QT> &g, uint32_t (*wcnt)[QT][4], int tile, int64_t row,
                                                 const bool (&hit)[QT], const uint32_t (&bits)[QT])
{
    range_rank<QT>(wcnt, tile, hit, g.run, [&](int q, uint32_t rank) {
        if (FINAL) {
            const int64_t o = g.out0[q] + rank;
            a.dist[o] = bits[q];
            a.out_labels[o] = a.labels ? a.labels[row] : a.id_base + row;
        } else if (rank < a.C) {
            a.spill[g.cell[q] * (int64_t)a.C + rank] = ((unsigned long long)bits[q] << 32) | (uint32_t)row;
        }
    });
}

template <int QT, bool FINAL>
__device__ __forceinline__ void flat_range_close(const FlatRangeArgs &a, const FlatRangeGroup<QT> &g)
{
    if (FINAL || threadIdx.x != 0) return;
#pragma unroll
    for (int q = 0; q < QT; ++q)
        if (g.active[q]) a.part_cnt[g.cell[q]] = g.run[q];
}

// an empty part of the scan still owes its counts
template <int QT, bool FINAL>
__device__ __forceinline__ void flat_range_skip(const FlatRangeArgs &a, const FlatRangeGroup<QT> &g)
{
    if (!FINAL && g.row_begin >= g.row_end) flat_range_close<QT, FINAL>(a, g);
}

// ---- fp32, blocked rows, queries in SGPRs: two 256-row tiles per pass share the scalar loads ----
template <bool IP, int LANES, int QT, bool FINAL>
__global__ __launch_bounds__(kBlock) void flat_range_f32_blocked_kernel(const FlatRangeArgs a)
{
    __shared__ uint32_t wcnt[2][QT][4];
    FlatRangeGroup<QT> g;
    if (!flat_range_open<QT, FINAL>(a, g)) { flat_range_skip<QT, FINAL>(a, g); return; }
    const int tid = threadIdx.x;
    dist_cfloat *qp[QT];
    dist_f32_uniform<QT>(qp, a.q, g.group, a.nq, a.D);
    const float4 *X = reinterpret_cast<const float4 *>(a.data);
    const float t = __uint_as_float(a.thr);
    const int D = a.D;
    int tile = 0;
    for (int64_t base = g.row_begin; base < g.row_end; base += 2 * kBlock) {
        const float4 *rowp[2];
        int64_t row[2];
        bool valid[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            row[r] = base + r * kBlock + tid;
            valid[r] = row[r] < g.row_end;
            const int64_t rc = valid[r] ? row[r] : g.row_begin;   // rows past the end read a valid row, rejected below
            rowp[r] = X + (rc >> 6) * (int64_t)(D >> 2) * 64 + (rc & 63);
        }
        float d[2][QT];
        dist_f32_blocked<IP, LANES, QT, 2>(rowp, qp, D, d);
#pragma unroll
        for (int r = 0; r < 2; ++r, ++tile) {
            bool hit[QT];
            uint32_t bits[QT];
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                hit[q] = valid[r] && g.active[q] && d[r][q] < t;
                bits[q] = __float_as_uint(d[r][q]);
            }
            flat_range_place<QT, FINAL>(a, g, wcnt, tile, row[r], hit, bits);
        }
    }
    flat_range_close<QT, FINAL>(a, g);
}

// ---- fp32, row-major rows (D % 4 != 0), queries in LDS: the scalar loop ----
template <bool IP, int QT, bool FINAL>
__global__ __launch_bounds__(kBlock) void flat_range_f32_rows_kernel(const FlatRangeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float qs[];  // [QT][D]
    __shared__ uint32_t wcnt[2][QT][4];
    FlatRangeGroup<QT> g;
    if (!flat_range_open<QT, FINAL>(a, g)) { flat_range_skip<QT, FINAL>(a, g); return; }
    const int tid = threadIdx.x;
    dist_f32_stage<QT>(qs, reinterpret_cast<const float *>(a.q), g.group, a.nq, a.D);
    __syncthreads();
    const float *X = reinterpret_cast<const float *>(a.data);
    const float t = __uint_as_float(a.thr);
    int tile = 0;
    for (int64_t base = g.row_begin; base < g.row_end; base += kBlock, ++tile) {
        const int64_t row = base + tid;
        const bool valid = row < g.row_end;
        float d[QT];
        dist_f32_row<IP, 1, QT>(X + (valid ? row : g.row_begin) * a.D, qs, a.D, d);
        bool hit[QT];
        uint32_t bits[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            hit[q] = valid && g.active[q] && d[q] < t;
            bits[q] = __float_as_uint(d[q]);
        }
        flat_range_place<QT, FINAL>(a, g, wcnt, tile, row, hit, bits);
    }
    flat_range_close<QT, FINAL>(a, g);
}

// ---- uint8 rows.  MODE: dist_u8.h's forms -- U8_BYTES (any D), U8_PIECES (D % 16 == 0), U8_SIGNED (... with the handle's norms) ----
template <int MODE, int QT, bool FINAL>
__global__ __launch_bounds__(kBlock) void flat_range_u8_kernel(const FlatRangeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t qw[];  // [QT][W] packed query bytes (MODE 2: ^ 0x80)
    __shared__ uint32_t wcnt[2][QT][4];
    __shared__ uint32_t qq[QT];
    FlatRangeGroup<QT> g;
    if (!flat_range_open<QT, FINAL>(a, g)) { flat_range_skip<QT, FINAL>(a, g); return; }
    const int tid = threadIdx.x;
    const int W = a.D >> 2;   // 32-bit words per row that take part (dist_u8.h)
    dist_u8_stage<MODE, QT>(qw, reinterpret_cast<const uint8_t *>(a.q), g.group, a.nq, a.D);
    __syncthreads();
    dist_u8_qnorms<MODE, QT>(qq, qw, W);
    __syncthreads();
    // QT > 1: U x 16 bytes of the row are requested before the first is used -- with one 16-byte load in flight per lane the
    // walk waits for memory latency, not bandwidth (10 M x 512-d, 8 queries: 1.84 -> 1.35 ms; U = 8 gains nothing more).
    // One query: the plain loop, which the compiler already unrolls with its loads ahead (1.00 ms against 1.16 - 1.24)
    constexpr int U = QT == 1 ? 1 : 4;
    const uint8_t *X = reinterpret_cast<const uint8_t *>(a.data);
    int tile = 0;
    for (int64_t base = g.row_begin; base < g.row_end; base += kBlock, ++tile) {
        const int64_t row = base + tid;
        const bool valid = row < g.row_end;
        const int64_t rc = valid ? row : g.row_begin;
        bool hit[QT];
        uint32_t bits[QT];
        dist_u8_row<MODE, QT, U>(X + rc * a.D, qw, qq, W, MODE == U8_SIGNED ? a.norms + rc : nullptr, bits);
#pragma unroll
        for (int q = 0; q < QT; ++q) hit[q] = valid && g.active[q] && bits[q] < a.thr;
        flat_range_place<QT, FINAL>(a, g, wcnt, tile, row, hit, bits);
    }
    flat_range_close<QT, FINAL>(a, g);
}

// one workgroup per (query, part) whose hits all fit its spill segment
__global__ __launch_bounds__(kBlock) void flat_range_fill_kernel(const FlatRangeArgs a)
{
    const int64_t cell = blockIdx.x;
    const uint32_t cnt = a.part_cnt[cell];
    if (a.lims[a.nq] > a.cap || cnt == 0 || cnt > a.C) return;
    const int64_t qi = cell / a.parts;
    const int64_t out0 = a.lims[qi] + (int64_t)a.part_off[cell];
    const unsigned long long *in = a.spill + cell * (int64_t)a.C;
    for (uint32_t i = threadIdx.x; i < cnt; i += kBlock) {
        const unsigned long long w = in[i];
        const int64_t row = (int64_t)(uint32_t)w;
        a.dist[out0 + i] = (uint32_t)(w >> 32);
        a.out_labels[out0 + i] = a.labels ? a.labels[row] : a.id_base + row;
    }
}

// Grid rules (pure host logic):
//   QT      fp32: flat_qtile's, 4 queries per workgroup from 4 queries on, else 1 (1 as well where 4 row-major queries would not fit
//           32 KB of LDS).  uint8: 1, 4, 8 or 16, the smallest that holds the batch -- the rows, not the dot4, set the pace, so
//           every query group less is a pass over the rows less -- halved while the packed queries do not fit 32 KB of LDS;
//   parts   part_rows == 0: flat_plan_splits' rule -- the (query group, part) workgroups fill the machine once -- with the rows of
//           a part rounded up to whole 256-row tiles; otherwise parts of part_rows rows, rounded up the same way;
//   C       spill < 0: kFlatRangeSpill records; never more than the rows of a part, and the spill area, nq x parts x C x 8 bytes,
//           stays within kFlatRangeSpillBytes: C shrinks to fit, down to 0 (every part with a hit is then walked twice).
FlatRangePlan plan_flat_range(int metric, int D, bool has_norms, int64_t n, int64_t nq, int64_t part_rows, int64_t spill)
{
    FlatRangePlan p;
    if (metric == CVTMI_METRIC_L2U8) p.form = D % 16 != 0 ? 2 : (has_norms ? 4 : 3);
    else p.form = flat_blocked(metric, D) ? 1 : 0;
    p.qt = flat_qtile(nq);
    if (p.form == 0 && (size_t)p.qt * D * sizeof(float) > ((size_t)32 << 10)) p.qt = 1;
    if (p.form >= 2) {
        p.qt = nq <= 1 ? 1 : (nq <= 4 ? 4 : (nq <= 8 ? 8 : 16));
        while (p.qt > 4 && (size_t)p.qt * ((D >> 2) + 1) * sizeof(uint32_t) > ((size_t)32 << 10)) p.qt /= 2;
    }
    const int64_t rows = std::max<int64_t>(n, 1);
    int64_t rpp = part_rows > 0 ? part_rows : blocks_for(rows, flat_plan_splits(rows, std::max<int64_t>(nq, 1), p.qt));
    rpp = std::min<int64_t>(blocks_for(std::max<int64_t>(rpp, 1), kBlock), (int64_t)1 << 24) * kBlock;
    p.rows_per_part = rpp;
    p.parts = (int)std::min<int64_t>(blocks_for(rows, rpp), 0x7fffffff);
    int64_t c = spill < 0 ? kFlatRangeSpill : spill;
    c = std::min(c, rpp);
    p.spill = std::min(c, range_spill_fit(kFlatRangeSpillBytes, nq, p.parts));
    p.spill_bytes = (size_t)std::max<int64_t>(nq, 0) * p.parts * (size_t)p.spill * sizeof(unsigned long long);
    return p;
}

size_t flat_range_carve(void *base, const FlatRangePlan &p, int64_t nq, FlatRangeBufs *b)
{
    return range_carve(base, 0, nq, p.parts, p.spill, b);
}

static int flat_range_args(FlatRangeArgs &a, const FlatRangeRows &x, const void *q, int64_t nq, uint32_t thr, const FlatRangePlan &p,
                           const FlatRangeBufs &b, int64_t *lims)
{
    if (x.n > 0xfffffffeLL) return fail(CVTMI_EUNSUPPORTED, "flat_range_search: %lld rows: rows travel as 32-bit payloads", (long long)x.n);
    if (x.D < 1 || x.D > 4096) return fail(CVTMI_EUNSUPPORTED, "flat_range_search: D=%d outside 1..4096", x.D);
    if (p.qt != 1 && p.qt != 4 && !(p.form >= 2 && (p.qt == 8 || p.qt == 16))) return fail(CVTMI_EINVAL, "flat_range_search: qtile %d", p.qt);
    if (p.parts < 1 || p.rows_per_part < kBlock || p.rows_per_part % kBlock != 0 || (int64_t)p.parts * p.rows_per_part < x.n)
        return fail(CVTMI_EINVAL, "flat_range_search: %d parts of %lld rows do not cover %lld rows", p.parts, (long long)p.rows_per_part, (long long)x.n);
    if (p.form == 4 && !x.norms) return fail(CVTMI_EINVAL, "flat_range_search: the plan wants norms the handle does not hold");
    a = FlatRangeArgs{};
    a.data = x.data; a.norms = x.norms; a.q = q; a.labels = x.labels; a.id_base = x.id_base;
    a.n = x.n; a.nq = nq; a.D = x.D; a.parts = p.parts; a.rows_per_part = p.rows_per_part;
    a.thr = thr; a.C = (uint32_t)p.spill;
    a.part_cnt = b.part_cnt; a.part_off = b.part_off; a.spill = b.spill; a.lims = lims;
    return CVTMI_OK;
}

template <int MODE, bool FINAL>
static decltype(&flat_range_u8_kernel<0, 1, false>) flat_range_u8_pick(int qt)
{
    switch (qt) {
        case 16: return flat_range_u8_kernel<MODE, 16, FINAL>;
        case 8: return flat_range_u8_kernel<MODE, 8, FINAL>;
        case 4: return flat_range_u8_kernel<MODE, 4, FINAL>;
        default: return flat_range_u8_kernel<MODE, 1, FINAL>;
    }
}

template <bool FINAL>
static int flat_range_walk(const char *what, const FlatRangeArgs &a, const FlatRangeRows &x, const FlatRangePlan &p, hipStream_t st)
{
    const int64_t blocks = blocks_for(a.nq, p.qt) * p.parts;
    const bool q4 = p.qt == 4;
    if (p.form == 1) {
        if (x.metric == CVTMI_METRIC_IP)
            return launch(what, q4 ? flat_range_f32_blocked_kernel<true, 4, 4, FINAL> : flat_range_f32_blocked_kernel<true, 4, 1, FINAL>, blocks, kBlock, 0, st, a);
        if (x.D % 16 == 0)
            return launch(what, q4 ? flat_range_f32_blocked_kernel<false, 8, 4, FINAL> : flat_range_f32_blocked_kernel<false, 8, 1, FINAL>, blocks, kBlock, 0, st, a);
        return launch(what, q4 ? flat_range_f32_blocked_kernel<false, 4, 4, FINAL> : flat_range_f32_blocked_kernel<false, 4, 1, FINAL>, blocks, kBlock, 0, st, a);
    }
    if (p.form == 0) {
        const size_t lds = (size_t)p.qt * x.D * sizeof(float);
        if (x.metric == CVTMI_METRIC_IP)
            return launch(what, q4 ? flat_range_f32_rows_kernel<true, 4, FINAL> : flat_range_f32_rows_kernel<true, 1, FINAL>, blocks, kBlock, lds, st, a);
        return launch(what, q4 ? flat_range_f32_rows_kernel<false, 4, FINAL> : flat_range_f32_rows_kernel<false, 1, FINAL>, blocks, kBlock, lds, st, a);
    }
    const size_t lds = (size_t)p.qt * ((x.D >> 2) + 1) * sizeof(uint32_t);
    if (p.form == 2) return launch(what, flat_range_u8_pick<0, FINAL>(p.qt), blocks, kBlock, lds, st, a);
    if (p.form == 3) return launch(what, flat_range_u8_pick<1, FINAL>(p.qt), blocks, kBlock, lds, st, a);
    return launch(what, flat_range_u8_pick<2, FINAL>(p.qt), blocks, kBlock, lds, st, a);
}

int launch_flat_range_count(const FlatRangeRows &x, const void *q, int64_t nq, uint32_t thr, const FlatRangePlan &p, const FlatRangeBufs &b,
                            int64_t *lims, hipStream_t st)
{
    if (nq <= 0 || x.n <= 0) return CVTMI_OK;
    FlatRangeArgs a;
    CVTMI_TRY(flat_range_args(a, x, q, nq, thr, p, b, lims));
    CVTMI_TRY(flat_range_walk<false>("flat_range_scan_kernel", a, x, p, st));
    return launch_range_offsets(b, p.parts, nq, lims, st);
}

int launch_flat_range_fill(const FlatRangeRows &x, const void *q, int64_t nq, uint32_t thr, const FlatRangePlan &p, const FlatRangeBufs &b,
                           const int64_t *lims, int64_t cap, void *dist, int64_t *labels, hipStream_t st)
{
    if (nq <= 0 || x.n <= 0) return CVTMI_OK;
    FlatRangeArgs a;
    CVTMI_TRY(flat_range_args(a, x, q, nq, thr, p, b, const_cast<int64_t *>(lims)));
    a.cap = cap; a.dist = static_cast<uint32_t *>(dist); a.out_labels = labels;
    if (p.spill > 0) CVTMI_TRY(launch("flat_range_fill_kernel", flat_range_fill_kernel, nq * p.parts, kBlock, 0, st, a));
    return flat_range_walk<true>("flat_range_rescan_kernel", a, x, p, st);
}

}  // namespace cvtmi
