// opq_remove.hip -- removal from the resident OPQ entries (cvtmi_opq_remove_videos / cvtmi_opq_remove_ids): one stable stream
// compaction of the insertion-ordered arrays codes [n][M], lists [n], videos [n] on the device, in three passes.
//
//   mark     a bitmap of the dropped entries (one uint64 per 64 rows) and the kept count of every TILE of kRmTile rows.
//            videos: one lower_bound per entry in the sorted table of distinct removal ids -- membership and, for the move, the
//                    renumber rank; the top levels of the search (up to 1024 pivots) sit in LDS, the table itself stays in L2.
//            ids:    the bitmap is cleared, the in-range ids are scattered into it (atomicOr), a second kernel counts the tiles.
//   scan     tile counts -> tile offsets, in two levels like the counting sort of query_video.hip: every workgroup scans
//            kRmScanTiles tiles in place and leaves its sum, ONE workgroup scans the sums and leaves the total.  No workgroup
//            waits for another anywhere in this file: the order comes from the launches on the stream.
//   move     in CHUNKS of a fixed number of rows, ascending; two launches per chunk:
//              gather  a workgroup per tile: position of a kept row = tile offset + rank inside the tile (popcount of the kept bits
//                      below it); the tile's kept code rows are staged in LDS and leave as one contiguous run into the chunk-sized
//                      scratch (16-byte units at M = 16), list and video ids go straight to their compacted places in it;
//                      remap and the renumbered video ids are written here
//              copy    the same tiles copy their runs from the scratch to their destination in the arrays
//            The destination of a chunk never lies past its own first row, and the launches of one stream run in order, so no row
//            is overwritten before its gather has read it; nothing larger than a chunk is ever allocated.  A tile whose rows all
//            stay where they are (everything before the first dropped entry) reads and writes no code row at all.
// Every offset stays on the device; the host reads the kept total once.
#include <algorithm>

#include "rm_common.h"
#include "launch.h"

namespace cvtmi {

// ---- the sorted table of distinct removal ids ----
struct RmTable {
    const int32_t *tab;
    int64_t T, stride;   // pivot j = tab[j * stride]
    int np;
};

__device__ __forceinline__ void rm_load_pivots(const RmTable &t, int32_t *piv)
{
    for (int j = threadIdx.x; j < t.np; j += blockDim.x) piv[j] = t.tab[(int64_t)j * t.stride];
    __syncthreads();
}

// first index whose id is >= v (= the number of distinct removal ids smaller than v); *found: v is in the table
__device__ __forceinline__ int64_t rm_lower_bound(const RmTable &t, const int32_t *piv, int32_t v, bool *found)
{
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
    *found = a < t.T && t.tab[a] == v;
    return a;
}

// ---- mark ----
__global__ __launch_bounds__(256) void rm_mark_videos_kernel(const int32_t *__restrict__ videos, int64_t n, RmTable t,
                                                            unsigned long long *__restrict__ drop, uint32_t *__restrict__ tile_cnt)
{
    __shared__ int32_t piv[kRmPivots];
    __shared__ uint32_t wsum[4];
    rm_load_pivots(t, piv);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t word = (int64_t)blockIdx.x * kRmWords + wave, row = word * 64 + lane;
    bool hit = false;
    if (row < n) (void)rm_lower_bound(t, piv, videos ? videos[row] : (int32_t)row, &hit);
    const unsigned long long d = __ballot(hit);
    if (lane == 0) {
        drop[word] = d;
        wsum[wave] = (uint32_t)__popcll(~d & rm_valid_mask(word * 64, n));
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ void rm_scatter_ids_kernel(const int64_t *__restrict__ ids, int64_t n_ids, int64_t id_base, int64_t n, uint32_t *__restrict__ drop32)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_ids; i += (int64_t)gridDim.x * kBlock) {
        const int64_t id = ids[i];
        if (id < id_base) continue;
        const uint64_t r = (uint64_t)id - (uint64_t)id_base;
        if (r < (uint64_t)n) atomicOr(&drop32[r >> 5], 1u << (r & 31));   // (little endian: bit r of the uint64 view)
    }
}

__global__ void rm_count_tiles_kernel(const unsigned long long *__restrict__ drop, int64_t n, int64_t ntiles, uint32_t *__restrict__ tile_cnt)
{
    const int64_t tile = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tile >= ntiles) return;
    uint32_t kept = 0;
    for (int w = 0; w < kRmWords; ++w) {
        const int64_t word = tile * kRmWords + w;
        kept += (uint32_t)__popcll(~drop[word] & rm_valid_mask(word * 64, n));
    }
    tile_cnt[tile] = kept;
}

// ---- scan ----
// first level: tile counts -> offsets inside the workgroup's kRmScanTiles tiles (in place), and their sum
__global__ __launch_bounds__(256) void rm_scan_tiles_kernel(uint32_t *__restrict__ tile_off, int64_t ntiles, uint32_t *__restrict__ bsum)
{
    __shared__ uint32_t part[256];
    const int per = kRmScanTiles / 256;
    const int64_t t0 = (int64_t)blockIdx.x * kRmScanTiles + (int64_t)threadIdx.x * per;
    uint32_t c[per], s = 0;
    for (int j = 0; j < per; ++j) { c[j] = t0 + j < ntiles ? tile_off[t0 + j] : 0u; s += c[j]; }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < 256; ++i) { const uint32_t v = part[i]; part[i] = run; run += v; }
        bsum[blockIdx.x] = run;
    }
    __syncthreads();
    uint32_t run = part[threadIdx.x];
    for (int j = 0; j < per; ++j) {
        if (t0 + j < ntiles) tile_off[t0 + j] = run;
        run += c[j];
    }
}

// second level, one workgroup: sums -> offsets of the first-level workgroups; total[0] = kept entries
__global__ __launch_bounds__(256) void rm_scan_top_kernel(const uint32_t *__restrict__ bsum, int nblk, int64_t *__restrict__ boff, int64_t *__restrict__ total)
{
    __shared__ int64_t part[256];
    const int per = (nblk + 255) / 256;
    const int b0 = threadIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    int64_t s = 0;
    for (int b = b0; b < b1; ++b) s += bsum[b];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < 256; ++i) { const int64_t v = part[i]; part[i] = run; run += v; }
        total[0] = run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int b = b0; b < b1; ++b) { boff[b] = run; run += bsum[b]; }
}

// ---- move ----
struct RmMove {
    uint8_t *codes;        // the arrays of the handle; lists may be null (no list array)
    int32_t *lists, *videos;
    uint8_t *s_codes;      // the chunk-sized scratch
    int32_t *s_lists, *s_videos;
    const unsigned long long *drop;
    const uint32_t *tile_off;
    const int64_t *boff, *total;
    int64_t *remap;        // or null
    int64_t n, ntiles, tile0;   // tile0: first tile of the chunk
    int M;
};

// U: the widest unit that divides a code row (uint4 at M = 16)
template <class U> __global__ __launch_bounds__(256) void rm_gather_kernel(RmMove a, RmTable t, int renumber)
{
    __shared__ int32_t piv[kRmPivots];
    __shared__ unsigned long long kmask[kRmWords];
    __shared__ uint4 stage4[kRmTile];   // kRmTile rows of up to 16 bytes
    U *stage = reinterpret_cast<U *>(stage4);
    if (renumber) rm_load_pivots(t, piv);
    const int64_t tile = a.tile0 + blockIdx.x, row_t = tile * kRmTile;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < kRmWords) {
        const int64_t word = tile * kRmWords + threadIdx.x;
        kmask[threadIdx.x] = ~a.drop[word] & rm_valid_mask(word * 64, a.n);
    }
    __syncthreads();
    const int64_t pos = rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, tile);
    const int64_t cnt = rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, tile + 1) - pos;
    const int64_t rows = a.n - row_t < kRmTile ? a.n - row_t : kRmTile;
    const bool in_place = pos == row_t && cnt == rows;   // nothing dropped up to the end of this tile: its rows stay where they are
    const int64_t sbase = pos - rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, a.tile0);   // the tile's run inside the scratch
    const int upr = a.M / (int)sizeof(U);   // units per row
    const int64_t row = row_t + wave * 64 + lane;
    const bool keep = (kmask[wave] >> lane) & 1ull;   // (no bit is set past the last row)
    uint32_t rank = (uint32_t)__popcll(kmask[wave] & ((1ull << lane) - 1ull));
    for (int j = 0; j < wave; ++j) rank += (uint32_t)__popcll(kmask[j]);
    if (a.remap && row < a.n) a.remap[row] = keep ? pos + rank : -1;
    if (keep) {
        int32_t v = a.videos[row];
        if (renumber) {
            bool hit;
            v -= (int32_t)rm_lower_bound(t, piv, v, &hit);
        }
        if (in_place) {
            if (renumber) a.videos[row] = v;
        } else {
            a.s_videos[sbase + rank] = v;
            if (a.lists) a.s_lists[sbase + rank] = a.lists[row];
            const U *src = reinterpret_cast<const U *>(a.codes) + row * upr;
            for (int u = 0; u < upr; ++u) stage[rank * upr + u] = src[u];
        }
    }
    if (in_place) return;   // (workgroup-uniform)
    __syncthreads();
    U *dst = reinterpret_cast<U *>(a.s_codes) + sbase * upr;
    for (int64_t u = threadIdx.x; u < cnt * upr; u += 256) dst[u] = stage[u];
}

template <class U> __global__ __launch_bounds__(256) void rm_copy_kernel(RmMove a)
{
    const int64_t tile = a.tile0 + blockIdx.x, row_t = tile * kRmTile;
    const int64_t pos = rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, tile);
    const int64_t cnt = rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, tile + 1) - pos;
    const int64_t rows = a.n - row_t < kRmTile ? a.n - row_t : kRmTile;
    if (pos == row_t && cnt == rows) return;
    const int64_t sbase = pos - rm_tile_pos(a.tile_off, a.boff, a.total, a.ntiles, a.tile0);
    const int upr = a.M / (int)sizeof(U);
    const U *src = reinterpret_cast<const U *>(a.s_codes) + sbase * upr;
    U *dst = reinterpret_cast<U *>(a.codes) + pos * upr;
    for (int64_t u = threadIdx.x; u < cnt * upr; u += 256) dst[u] = src[u];
    for (int64_t j = threadIdx.x; j < cnt; j += 256) {
        a.videos[pos + j] = a.s_videos[sbase + j];
        if (a.lists) a.lists[pos + j] = a.s_lists[sbase + j];
    }
}

// video ids in place, where no entry leaves but ids of the set lie below kept ones
__global__ __launch_bounds__(256) void rm_renumber_kernel(int32_t *__restrict__ videos, int64_t n, RmTable t)
{
    __shared__ int32_t piv[kRmPivots];
    rm_load_pivots(t, piv);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        bool hit;
        videos[i] -= (int32_t)rm_lower_bound(t, piv, videos[i], &hit);
    }
}

__global__ void rm_fill_remap_kernel(int64_t *__restrict__ remap, int64_t n, int identity)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) remap[i] = identity ? i : -1;
}

// ---- host side ----
int64_t rm_chunk_rows(int64_t wanted)
{
    if (wanted <= 0) wanted = kRmChunkDefault;
    return (wanted + kRmTile - 1) / kRmTile * kRmTile;
}

RmPlan rm_plan(int64_t n, int M, int64_t table_len, int64_t chunk_rows)
{
    RmPlan p;
    p.n = n; p.M = M; p.T = table_len;
    p.ntiles = (n + kRmTile - 1) / kRmTile;
    p.nblk = (int)((p.ntiles + kRmScanTiles - 1) / kRmScanTiles);
    p.chunk = std::min<int64_t>(rm_chunk_rows(chunk_rows), std::max<int64_t>(p.ntiles, 1) * kRmTile);
    size_t o = 0;
    p.off_drop = o;   o += rm_align((size_t)std::max<int64_t>(p.ntiles, 1) * kRmWords * 8);
    p.off_tile = o;   o += rm_align((size_t)std::max<int64_t>(p.ntiles, 1) * 4);
    p.off_bsum = o;   o += rm_align((size_t)std::max(p.nblk, 1) * 4);
    p.off_boff = o;   o += rm_align((size_t)std::max(p.nblk, 1) * 8);
    p.off_total = o;  o += rm_align(8);
    p.off_table = o;  o += rm_align((size_t)std::max<int64_t>(table_len, 1) * 4);
    p.off_codes = o;  o += rm_align((size_t)p.chunk * M);
    p.off_lists = o;  o += rm_align((size_t)p.chunk * 4);
    p.off_videos = o; o += rm_align((size_t)p.chunk * 4);
    p.bytes = o;
    return p;
}

static RmTable rm_table(const RmPlan &p, void *scratch)
{
    RmTable t;
    t.tab = reinterpret_cast<const int32_t *>(static_cast<char *>(scratch) + p.off_table);
    t.T = p.T;
    t.stride = std::max<int64_t>(1, (p.T + kRmPivots - 1) / kRmPivots);
    t.np = (int)((p.T + t.stride - 1) / t.stride);
    return t;
}

int launch_rm_scan(const RmPlan &p, void *scratch, hipStream_t st)
{
    CVTMI_TRY(launch("rm_scan_tiles_kernel", rm_scan_tiles_kernel, p.nblk, 256, 0, st, rm_at<uint32_t>(scratch, p.off_tile), p.ntiles, rm_at<uint32_t>(scratch, p.off_bsum)));
    return launch("rm_scan_top_kernel", rm_scan_top_kernel, 1, 256, 0, st, rm_at<uint32_t>(scratch, p.off_bsum), p.nblk, rm_at<int64_t>(scratch, p.off_boff),
                  rm_at<int64_t>(scratch, p.off_total));
}

int launch_rm_mark_videos(const RmPlan &p, void *scratch, const int32_t *videos, hipStream_t st)
{
    if (p.n <= 0) return fail(CVTMI_EINVAL, "opq remove: empty index");
    CVTMI_TRY(launch("rm_mark_videos_kernel", rm_mark_videos_kernel, p.ntiles, 256, 0, st, videos, p.n, rm_table(p, scratch), rm_at<unsigned long long>(scratch, p.off_drop),
                     rm_at<uint32_t>(scratch, p.off_tile)));
    return launch_rm_scan(p, scratch, st);
}

int launch_rm_mark_ids(const RmPlan &p, void *scratch, const int64_t *ids, int64_t n_ids, int64_t id_base, hipStream_t st)
{
    if (p.n <= 0) return fail(CVTMI_EINVAL, "opq remove: empty index");
    CVTMI_HIP(hipMemsetAsync(rm_at<char>(scratch, p.off_drop), 0, (size_t)p.ntiles * kRmWords * 8, st));
    if (n_ids > 0) {
        const int64_t blocks = std::min<int64_t>(blocks_for(n_ids, kBlock), 4096);
        CVTMI_TRY(launch("rm_scatter_ids_kernel", rm_scatter_ids_kernel, blocks, kBlock, 0, st, ids, n_ids, id_base, p.n, rm_at<uint32_t>(scratch, p.off_drop)));
    }
    CVTMI_TRY(launch("rm_count_tiles_kernel", rm_count_tiles_kernel, blocks_for(p.ntiles, kBlock), kBlock, 0, st, rm_at<unsigned long long>(scratch, p.off_drop), p.n, p.ntiles,
                     rm_at<uint32_t>(scratch, p.off_tile)));
    return launch_rm_scan(p, scratch, st);
}

template <class U> static int rm_move_chunks(const RmPlan &p, RmMove a, const RmTable &t, int renumber, hipStream_t st)
{
    const int64_t tiles_per_chunk = p.chunk / kRmTile;
    for (int64_t t0 = 0; t0 < p.ntiles; t0 += tiles_per_chunk) {
        a.tile0 = t0;
        const int64_t grid = std::min(tiles_per_chunk, p.ntiles - t0);
        CVTMI_TRY(launch("rm_gather_kernel", rm_gather_kernel<U>, grid, 256, 0, st, a, t, renumber));
        CVTMI_TRY(launch("rm_copy_kernel", rm_copy_kernel<U>, grid, 256, 0, st, a));
    }
    return CVTMI_OK;
}

int launch_rm_move(const RmPlan &p, void *scratch, uint8_t *codes, int32_t *lists, int32_t *videos, int renumber, int64_t *remap, hipStream_t st)
{
    if (!codes || !videos || p.M < 1 || p.M > 16) return fail(CVTMI_EINVAL, "opq remove: bad arguments");
    RmMove a;
    a.codes = codes; a.lists = lists; a.videos = videos;
    a.s_codes = rm_at<uint8_t>(scratch, p.off_codes); a.s_lists = rm_at<int32_t>(scratch, p.off_lists); a.s_videos = rm_at<int32_t>(scratch, p.off_videos);
    a.drop = rm_at<unsigned long long>(scratch, p.off_drop); a.tile_off = rm_at<uint32_t>(scratch, p.off_tile);
    a.boff = rm_at<int64_t>(scratch, p.off_boff); a.total = rm_at<int64_t>(scratch, p.off_total);
    a.remap = remap; a.n = p.n; a.ntiles = p.ntiles; a.tile0 = 0; a.M = p.M;
    const RmTable t = rm_table(p, scratch);
    // (the code buffer comes from hipMalloc and the scratch areas start on 256 bytes: a unit that divides M is aligned in both)
    if (p.M == 16) return rm_move_chunks<uint4>(p, a, t, renumber, st);
    if (p.M % 8 == 0) return rm_move_chunks<uint2>(p, a, t, renumber, st);
    if (p.M % 4 == 0) return rm_move_chunks<uint32_t>(p, a, t, renumber, st);
    if (p.M % 2 == 0) return rm_move_chunks<uint16_t>(p, a, t, renumber, st);
    return rm_move_chunks<uint8_t>(p, a, t, renumber, st);
}

int launch_rm_renumber(const RmPlan &p, void *scratch, int32_t *videos, hipStream_t st)
{
    if (p.n <= 0 || p.T <= 0) return CVTMI_OK;
    const int64_t blocks = std::min<int64_t>(blocks_for(p.n, 256), 4096);
    return launch("rm_renumber_kernel", rm_renumber_kernel, blocks, 256, 0, st, videos, p.n, rm_table(p, scratch));
}

int launch_rm_fill_remap(int64_t *remap, int64_t n, int identity, hipStream_t st)
{
    if (n <= 0) return CVTMI_OK;
    const int64_t blocks = std::min<int64_t>(blocks_for(n, kBlock), 4096);
    return launch("rm_fill_remap_kernel", rm_fill_remap_kernel, blocks, kBlock, 0, st, remap, n, identity);
}

}  // namespace cvtmi
