// flat_remove.hip -- removal from a flat index (cvtmi_flat_remove_labels): one stable stream compaction of the rows, their labels
// [n] and their norms [n] on the device, in the three passes of opq_remove.hip.
//
//   mark     a bitmap of the dropped rows (one uint64 per 64 rows) and the kept count of every tile of kRmTile rows.
//            implicit labels: the in-range values label - id_base are scattered into the cleared bitmap (launch_rm_mark_ids).
//            explicit labels: one lower_bound per row in the sorted table of distinct removal labels (int64); the top levels of the
//                             search (up to 1024 pivots, 8 KB) sit in LDS, the table itself stays in L2.
//   scan     tile counts -> tile offsets: launch_rm_scan, the two-level scan of opq_remove.hip.
//   move     in CHUNKS of "remove_chunk" rows, ascending; two launches per chunk, a workgroup per tile in both:
//              gather  new row of a kept row = tile offset + popcount of the kept bits below it; rows, labels and norms go to their
//                      compacted places in the chunk-sized scratch, remap is written here
//              copy    the same tiles copy their runs from the scratch to their destination
//            The destination of a chunk never lies past its own first row and the launches of one stream run in order: no row is
//            overwritten before its gather has read it, and nothing larger than a chunk is allocated.  A tile whose rows all stay
//            where they are (everything before the first dropped row) moves nothing.
//
// Row layouts:
//   row-major (uint8 at any D; fp32 where D % 4 != 0): a row is row_bytes bytes, cut into units of the widest type that divides it
//            (16 bytes at D % 16 == 0 uint8).  The scratch holds the kept rows of the chunk back to back; the gather writes it as one
//            contiguous run per tile (unit u of the run comes from kept row u / units-per-row), the copy is contiguous on both sides.
//   blocked  (fp32, D % 4 == 0): float4 c of row r sits at ((r >> 6) * (D / 4) + c) * 64 + (r & 63).  The scratch is blocked the same
//            way and PHASED like the destination: new row j of the chunk's first kept row j0 sits at scratch row j - (j0 & ~63), so a
//            scratch block is a destination block and the copy moves 16-byte slot to the same slot.  A lane owns a kept row; at a fixed
//            c the 64 lanes of a wave read one 1 KB line of the source block and the kept lanes write consecutive 16-byte slots (of at
//            most two blocks); the copy reads and writes consecutive slots.  The scratch is one block longer than the chunk.
//            Rows behind the new end of the last block are stale afterwards: the caller re-runs launch_flat_f32_bias, which zeroes them.
#include <algorithm>

#include "rm_common.h"
#include "launch.h"

namespace cvtmi {

struct FlatRmTable {
    const int64_t *tab;
    int64_t T, stride;   // pivot j = tab[j * stride]
    int np;
};

// ---- mark ----
__global__ __launch_bounds__(256) void flat_rm_mark_labels_kernel(const int64_t *__restrict__ labels, int64_t n, FlatRmTable t,
                                                                 unsigned long long *__restrict__ drop, uint32_t *__restrict__ tile_cnt)
{
    __shared__ int64_t piv[kRmPivots];
    __shared__ uint32_t wsum[4];
    for (int j = threadIdx.x; j < t.np; j += 256) piv[j] = t.tab[(int64_t)j * t.stride];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * kRmWords + wave, row = word * 64 + lane;
    bool hit = false;
    if (row < n) {
        const int64_t v = labels[row];
        int lo = 0, hi = t.np;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (piv[mid] < v) lo = mid + 1; else hi = mid;
        }
        // lo pivots are smaller than v: the answer lies behind pivot lo - 1 and not behind pivot lo
        int64_t a = lo == 0 ? 0 : (int64_t)(lo - 1) * t.stride + 1, b = (int64_t)lo * t.stride;
        if (b > t.T) b = t.T;
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (t.tab[mid] < v) a = mid + 1; else b = mid;
        }
        hit = a < t.T && t.tab[a] == v;
    }
    const unsigned long long d = __ballot(hit);
    if (lane == 0) {
        drop[word] = d;
        wsum[wave] = (uint32_t)__popcll(~d & rm_valid_mask(word * 64, n));
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ---- move ----
struct FlatRmMove {
    void *rows;            // the arrays of the handle; norms may be null
    int64_t *labels;
    int32_t *norms;
    void *s_rows;          // the chunk-sized scratch
    int64_t *s_labels;
    int32_t *s_norms;
    const unsigned long long *drop;
    const uint32_t *tile_off;
    const int64_t *boff, *total;
    int64_t *remap;        // or null
    int64_t n, ntiles, tile0;   // tile0: first tile of the chunk
    int upr;               // row-major: units per row; blocked: float4 per row
};

// what every workgroup of the move knows about its tile
struct FlatRmTile {
    int64_t row_t, pos, cnt, pos0;   // first old row, first new row, kept rows; first new row of the chunk
    bool in_place;                   // nothing dropped up to the end of this tile: its rows stay where they are
};

__device__ __forceinline__ FlatRmTile flat_rm_tile(const FlatRmMove &a)
{
    FlatRmTile t;
    const int64_t tile = a.tile0 + blockIdx.x;
    t.row_t = tile * kRmTile;
    t.pos = rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, tile);
    t.cnt = rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, tile + 1) - t.pos;
    t.pos0 = rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, a.tile0);
    const int64_t rows = a.n - t.row_t < kRmTile ? a.n - t.row_t : kRmTile;
    t.in_place = t.pos == t.row_t && t.cnt == rows;
    return t;
}

// keep / rank of the thread's row inside its tile; remap is written for every row of the tile
__device__ __forceinline__ bool flat_rm_rank(const FlatRmMove &a, const FlatRmTile &t, unsigned long long *kmask, uint32_t *rank_out)
{
    const int64_t tile = a.tile0 + blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < kRmWords) {
        const int64_t word = tile * kRmWords + threadIdx.x;
        kmask[threadIdx.x] = ~a.drop[word] & rm_valid_mask(word * 64, a.n);
    }
    __syncthreads();
    const bool keep = (kmask[wave] >> lane) & 1ull;   // (no bit is set past the last row)
    uint32_t rank = (uint32_t)__popcll(kmask[wave] & ((1ull << lane) - 1ull));
    for (int j = 0; j < wave; ++j) rank += (uint32_t)__popcll(kmask[j]);
    const int64_t row = t.row_t + threadIdx.x;
    if (a.remap && row < a.n) a.remap[row] = keep ? t.pos + rank : -1;
    *rank_out = rank;
    return keep;
}

// U: the widest unit that divides a row
template <class U> __global__ __launch_bounds__(256) void flat_rm_gather_rows_kernel(FlatRmMove a)
{
    __shared__ unsigned long long kmask[kRmWords];
    __shared__ uint16_t src_s[kRmTile];   // row of the tile that holds kept row number `rank`
    const FlatRmTile t = flat_rm_tile(a);
    uint32_t rank;
    const bool keep = flat_rm_rank(a, t, kmask, &rank);
    if (t.in_place) return;   // (workgroup-uniform)
    const int64_t sbase = t.pos - t.pos0;   // the tile's run inside the scratch
    if (keep) {
        const int64_t row = t.row_t + threadIdx.x;
        src_s[rank] = (uint16_t)threadIdx.x;
        a.s_labels[sbase + rank] = a.labels[row];
        if (a.norms) a.s_norms[sbase + rank] = a.norms[row];
    }
    __syncthreads();
    const uint32_t upr = (uint32_t)a.upr, units = (uint32_t)t.cnt * upr;
    const U *src = reinterpret_cast<const U *>(a.rows) + t.row_t * upr;
    U *dst = reinterpret_cast<U *>(a.s_rows) + sbase * upr;
    for (uint32_t u = threadIdx.x; u < units; u += 256) {
        const uint32_t r = u / upr, c = u - r * upr;
        dst[u] = src[(uint32_t)src_s[r] * upr + c];
    }
}

template <class U> __global__ __launch_bounds__(256) void flat_rm_copy_rows_kernel(FlatRmMove a)
{
    const FlatRmTile t = flat_rm_tile(a);
    if (t.in_place) return;
    const int64_t sbase = t.pos - t.pos0;
    const uint32_t upr = (uint32_t)a.upr, units = (uint32_t)t.cnt * upr;
    const U *src = reinterpret_cast<const U *>(a.s_rows) + sbase * upr;
    U *dst = reinterpret_cast<U *>(a.rows) + t.pos * upr;
    for (uint32_t u = threadIdx.x; u < units; u += 256) dst[u] = src[u];
    if ((int64_t)threadIdx.x < t.cnt) {
        a.labels[t.pos + threadIdx.x] = a.s_labels[sbase + threadIdx.x];
        if (a.norms) a.norms[t.pos + threadIdx.x] = a.s_norms[sbase + threadIdx.x];
    }
}

__device__ __forceinline__ int64_t flat_rm_slot(int64_t r, int D4) { return (r >> 6) * (int64_t)D4 * 64 + (r & 63); }

__global__ __launch_bounds__(256) void flat_rm_gather_blocked_kernel(FlatRmMove a)
{
    __shared__ unsigned long long kmask[kRmWords];
    const FlatRmTile t = flat_rm_tile(a);
    uint32_t rank;
    const bool keep = flat_rm_rank(a, t, kmask, &rank);
    if (t.in_place || !keep) return;
    const int64_t row = t.row_t + threadIdx.x, sbase = t.pos - t.pos0;
    a.s_labels[sbase + rank] = a.labels[row];
    const int64_t s = t.pos + rank - (t.pos0 & ~(int64_t)63);   // the scratch is phased like the destination
    const float4 *src = reinterpret_cast<const float4 *>(a.rows) + flat_rm_slot(row, a.upr);
    float4 *dst = reinterpret_cast<float4 *>(a.s_rows) + flat_rm_slot(s, a.upr);
    for (int c = 0; c < a.upr; ++c) dst[(int64_t)c * 64] = src[(int64_t)c * 64];
}

__global__ __launch_bounds__(256) void flat_rm_copy_blocked_kernel(FlatRmMove a)
{
    const FlatRmTile t = flat_rm_tile(a);
    if (t.in_place || (int64_t)threadIdx.x >= t.cnt) return;
    const int64_t sbase = t.pos - t.pos0, nr = t.pos + threadIdx.x;
    a.labels[nr] = a.s_labels[sbase + threadIdx.x];
    const float4 *src = reinterpret_cast<const float4 *>(a.s_rows) + flat_rm_slot(nr - (t.pos0 & ~(int64_t)63), a.upr);
    float4 *dst = reinterpret_cast<float4 *>(a.rows) + flat_rm_slot(nr, a.upr);
    for (int c = 0; c < a.upr; ++c) dst[(int64_t)c * 64] = src[(int64_t)c * 64];
}

__global__ void flat_rm_iota_kernel(int64_t *__restrict__ labels, int64_t n, int64_t base)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) labels[i] = base + i;
}

// ---- host side ----
// the default chunk is the rows of 64 MB.  Measured (tools/flat_remove_sweep.py, profiles/flat_remove_sweep.txt): 16 MB chunks cost 1.5-2 x
// (four times the launches), 256 MB chunks are within -17 .. +2 % of 64 MB for four times the scratch
int64_t flat_rm_chunk_rows(int64_t wanted, size_t row_bytes)
{
    if (wanted <= 0) wanted = std::max<int64_t>(kRmTile, (int64_t)(((size_t)64 << 20) / std::max<size_t>(row_bytes, 1)));
    return (wanted + kRmTile - 1) / kRmTile * kRmTile;
}

FlatRmPlan flat_rm_plan(int64_t n, size_t row_bytes, bool blocked, bool has_norms, int64_t table_len, int64_t chunk_rows)
{
    FlatRmPlan p;
    p.rm = rm_plan(n, 0, 0, flat_rm_chunk_rows(chunk_rows, row_bytes));   // bitmap, tile offsets, scan levels, kept total; chunk clamped to the tiles there are
    p.T = table_len; p.row_bytes = row_bytes; p.blocked = blocked;
    size_t o = p.rm.off_table;   // (nothing of the OPQ plan behind its scan areas is used)
    p.off_table = o;  o += rm_align((size_t)std::max<int64_t>(table_len, 1) * 8);
    p.off_rows = o;   o += rm_align((size_t)(p.rm.chunk + (blocked ? 64 : 0)) * row_bytes);
    p.off_labels = o; o += rm_align((size_t)p.rm.chunk * 8);
    p.off_norms = o;  o += has_norms ? rm_align((size_t)p.rm.chunk * 4) : 0;
    p.bytes = o;
    return p;
}

int launch_flat_rm_mark_labels(const FlatRmPlan &p, void *scratch, const int64_t *labels, hipStream_t st)
{
    if (p.rm.n <= 0 || !labels) return fail(CVTMI_EINVAL, "flat remove: bad arguments");
    FlatRmTable t;
    t.tab = rm_at<const int64_t>(scratch, p.off_table);
    t.T = p.T;
    t.stride = std::max<int64_t>(1, (p.T + kRmPivots - 1) / kRmPivots);
    t.np = (int)((p.T + t.stride - 1) / t.stride);
    CVTMI_TRY(launch("flat_rm_mark_labels_kernel", flat_rm_mark_labels_kernel, p.rm.ntiles, 256, 0, st, labels, p.rm.n, t, rm_at<unsigned long long>(scratch, p.rm.off_drop),
                     rm_at<uint32_t>(scratch, p.rm.off_tile)));
    return launch_rm_scan(p.rm, scratch, st);
}

int launch_flat_rm_move(const FlatRmPlan &p, void *scratch, void *rows, int64_t *labels, int32_t *norms, int64_t *remap, hipStream_t st)
{
    if (!rows || !labels || p.row_bytes < 1 || (p.blocked && p.row_bytes % 16 != 0)) return fail(CVTMI_EINVAL, "flat remove: bad arguments");
    FlatRmMove a;
    a.rows = rows; a.labels = labels; a.norms = norms;
    a.s_rows = rm_at<char>(scratch, p.off_rows); a.s_labels = rm_at<int64_t>(scratch, p.off_labels);
    a.s_norms = norms ? rm_at<int32_t>(scratch, p.off_norms) : nullptr;
    a.drop = rm_at<unsigned long long>(scratch, p.rm.off_drop); a.tile_off = rm_at<uint32_t>(scratch, p.rm.off_tile);
    a.boff = rm_at<int64_t>(scratch, p.rm.off_boff); a.total = rm_at<int64_t>(scratch, p.rm.off_total);
    a.remap = remap; a.n = p.rm.n; a.ntiles = p.rm.ntiles; a.tile0 = 0;
    // (the row buffer comes from hipMalloc and the scratch areas start on 256 bytes: a unit that divides the row is aligned in both)
    const size_t rb = p.row_bytes;
    const int unit = p.blocked ? 16 : (rb % 16 == 0 ? 16 : rb % 8 == 0 ? 8 : rb % 4 == 0 ? 4 : rb % 2 == 0 ? 2 : 1);
    a.upr = (int)(rb / unit);
    auto gather = flat_rm_gather_blocked_kernel, copy = flat_rm_copy_blocked_kernel;
    if (p.blocked) ;
    else if (unit == 16) { gather = flat_rm_gather_rows_kernel<uint4>; copy = flat_rm_copy_rows_kernel<uint4>; }
    else if (unit == 8) { gather = flat_rm_gather_rows_kernel<uint2>; copy = flat_rm_copy_rows_kernel<uint2>; }
    else if (unit == 4) { gather = flat_rm_gather_rows_kernel<uint32_t>; copy = flat_rm_copy_rows_kernel<uint32_t>; }
    else if (unit == 2) { gather = flat_rm_gather_rows_kernel<uint16_t>; copy = flat_rm_copy_rows_kernel<uint16_t>; }
    else { gather = flat_rm_gather_rows_kernel<uint8_t>; copy = flat_rm_copy_rows_kernel<uint8_t>; }
    const int64_t tiles_per_chunk = p.rm.chunk / kRmTile;
    for (int64_t t0 = 0; t0 < p.rm.ntiles; t0 += tiles_per_chunk) {
        a.tile0 = t0;
        const int64_t grid = std::min(tiles_per_chunk, p.rm.ntiles - t0);
        CVTMI_TRY(launch(p.blocked ? "flat_rm_gather_blocked_kernel" : "flat_rm_gather_rows_kernel", gather, grid, 256, 0, st, a));
        CVTMI_TRY(launch(p.blocked ? "flat_rm_copy_blocked_kernel" : "flat_rm_copy_rows_kernel", copy, grid, 256, 0, st, a));
    }
    return CVTMI_OK;
}

int launch_flat_rm_iota(int64_t *labels, int64_t n, int64_t base, hipStream_t st)
{
    if (n <= 0) return CVTMI_OK;
    const int64_t blocks = std::min<int64_t>(blocks_for(n, kBlock), 4096);
    return launch("flat_rm_iota_kernel", flat_rm_iota_kernel, blocks, kBlock, 0, st, labels, n, base);
}

}  // namespace cvtmi
