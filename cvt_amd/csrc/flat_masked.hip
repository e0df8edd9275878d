// flat_masked.hip -- the k nearest rows among those a bitmap allows (cvtmi_flat_search_masked), and the bitmap of a label set
// (cvtmi_flat_mask_labels).
//
//   list     the mask (bit r & 63 of word r >> 6 allows row r) becomes an ascending uint32 list of the allowed rows, with its length,
//            on the device: the set bits of every kRmTile-row tile are counted (bits at or past n masked off), launch_rm_scan turns the
//            counts into offsets, and a workgroup per tile writes row r to tile offset + popcount of the allowed bits below r.  No
//            atomics: the list is the same on every run.  The host never learns its length.
//   search   the bodies of the exact kernels of flat.hip (flat_f32_sq_kernel, flat_f32_kernel, flat_u8_kernel) with one change: the
//            lane's row is list[i], not i.  The blocked layout already works on a per-lane row pointer, so a gathered row needs no new
//            distance code; the distance routines are dist_f32.h's, the selection is block_topk.h's.  The parts of a query group
//            divide the LIST, in whole tiles of kBlock * FLAT_R entries, each workgroup deriving its slice from the device-side length:
//            the work is even however the mask clusters.  A workgroup whose slice is empty writes a padded partial list and leaves;
//            entries past the end of a slice read a valid entry and are rejected with KEY_MAX.  Payloads are rows and ascend with
//            the list: the tie rule of block_topk.h holds as it is.
//   finish   launch_topk_merge over the parts, then rows -> labels, both by the caller (api_flat.hip).
#include <algorithm>

#include "block_topk.h"
#include "dist_f32.h"
#include "dist_u8.h"
#include "launch.h"
#include "rm_common.h"

namespace cvtmi {

constexpr int FM_CAP = 384, FM_TRIG = 256, FM_R = 2;   // flat.hip's FLAT_CAP / FLAT_TRIG / FLAT_R
constexpr int kFmTile = kBlock * FM_R;                 // list entries of a search tile

// ---- list ----
// the allowed bits of mask word `word` that name rows below n (words at or past the end of the rows are not read)
__device__ __forceinline__ unsigned long long fm_word(const unsigned long long *mask, int64_t word, int64_t n)
{
    const unsigned long long valid = rm_valid_mask(word * 64, n);
    return valid ? mask[word] & valid : 0ull;
}

__global__ void flat_masked_count_kernel(const unsigned long long *__restrict__ mask, int64_t n, int64_t ntiles, uint32_t *__restrict__ tile_cnt)
{
    const int64_t tile = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (tile >= ntiles) return;
    uint32_t c = 0;
    for (int w = 0; w < kRmWords; ++w) c += (uint32_t)__popcll(fm_word(mask, tile * kRmWords + w, n));
    tile_cnt[tile] = c;
}

// one workgroup per tile, one wave per mask word
__global__ __launch_bounds__(256) void flat_masked_list_kernel(const unsigned long long *__restrict__ mask, int64_t n, int64_t ntiles,
                                                              const uint32_t *__restrict__ tile_off, const int64_t *__restrict__ boff,
                                                              const int64_t *__restrict__ total, uint32_t *__restrict__ list)
{
    __shared__ unsigned long long m_s[kRmWords];
    const int64_t tile = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < kRmWords) m_s[threadIdx.x] = fm_word(mask, tile * kRmWords + threadIdx.x, n);
    __syncthreads();
    const unsigned long long m = m_s[wave];
    if (!((m >> lane) & 1ull)) return;
    uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    for (int j = 0; j < wave; ++j) rank += (uint32_t)__popcll(m_s[j]);
    // (pos + rank < the allowed total <= n: inside the list's n entries)
    list[rm_tile_pos(tile_off, boff, total, ntiles, tile) + rank] = (uint32_t)(tile * kRmTile + threadIdx.x);
}

int launch_flat_masked_list(const RmPlan &p, void *scratch, const uint64_t *mask, uint32_t *list, hipStream_t st)
{
    if (p.n <= 0 || !mask || !list) return fail(CVTMI_EINVAL, "flat masked: bad arguments");
    const unsigned long long *m = reinterpret_cast<const unsigned long long *>(mask);
    CVTMI_TRY(launch("flat_masked_count_kernel", flat_masked_count_kernel, blocks_for(p.ntiles, kBlock), kBlock, 0, st, m, p.n, p.ntiles,
                     rm_at<uint32_t>(scratch, p.off_tile)));
    CVTMI_TRY(launch_rm_scan(p, scratch, st));
    return launch("flat_masked_list_kernel", flat_masked_list_kernel, p.ntiles, 256, 0, st, m, p.n, p.ntiles, rm_at<uint32_t>(scratch, p.off_tile),
                  rm_at<int64_t>(scratch, p.off_boff), rm_at<int64_t>(scratch, p.off_total), list);
}

// mask[0 .. mask_words) = the first words of a marked bitmap (no bit set past the rows), zeros behind them
__global__ void flat_masked_copy_kernel(const unsigned long long *__restrict__ bits, int64_t have, unsigned long long *__restrict__ mask, int64_t mask_words)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < mask_words; i += (int64_t)gridDim.x * kBlock) mask[i] = i < have ? bits[i] : 0ull;
}

int launch_flat_masked_copy(const RmPlan &p, const void *scratch, uint64_t *mask, int64_t mask_words, hipStream_t st)
{
    if (mask_words <= 0) return CVTMI_OK;
    const int64_t blocks = std::min<int64_t>(blocks_for(mask_words, kBlock), 4096);
    return launch("flat_masked_copy_kernel", flat_masked_copy_kernel, blocks, kBlock, 0, st,
                  reinterpret_cast<const unsigned long long *>(static_cast<const char *>(scratch) + p.off_drop), p.ntiles * kRmWords,
                  reinterpret_cast<unsigned long long *>(mask), mask_words);
}

// ---- search ----
struct FlatMaskedArgs {
    const void *data;
    const void *q;
    int nq, D, k, parts;
    const uint32_t *list;   // the allowed rows, ascending
    const int64_t *len;     // their number (device)
    float *part_d;          // [nq][parts][k]
    int64_t *part_id;
};

// The part workgroup j of query group `group` answers for, and the slice [begin, end) of the list that part walks: whole tiles, spread
// evenly over the parts.  A list of fewer tiles than parts leaves parts empty, the same ones in every group, and workgroup b runs on
// XCD b % 8: with j as the part, the busy workgroups of ALL groups meet on the one or two XCDs those few parts map to.  So where parts
// are empty the groups take them in rotated order and the busy workgroups land on every XCD (1000 queries over 1016 allowed rows of
// 1 M x 128-d with 64 parts: 1.20 -> 0.14 ms; 10 M x 512-byte uint8, 10 000 allowed: 0.85 -> 0.35 ms).  The price is that the groups no
// longer share a part's rows through one XCD's L2, which a few groups over blocked fp32 rows feel (16 queries, 9962 allowed rows:
// 0.116 -> 0.133 ms).  Where every part has work j stays the part, as in flat.hip.  tools/flat_masked_times.py measures all of it.
__device__ __forceinline__ int fm_slice(const FlatMaskedArgs &a, int group, int j, int64_t *begin, int64_t *end)
{
    const int64_t len = a.len[0];
    const int64_t tiles = (len + kFmTile - 1) / kFmTile;
    const int part = tiles < a.parts ? (int)((j + (int64_t)group) % a.parts) : j;
    *begin = tiles * part / a.parts * kFmTile;
    const int64_t e = tiles * (part + 1) / a.parts * kFmTile;
    *end = e < len ? e : len;
    return part;
}

// the lane's entries of the tile at `base`: row and validity (an entry past the slice reads the slice's first row)
__device__ __forceinline__ void fm_rows(const FlatMaskedArgs &a, int64_t base, int64_t begin, int64_t end, uint32_t (&row)[FM_R], bool (&valid)[FM_R])
{
#pragma unroll
    for (int r = 0; r < FM_R; ++r) {
        const int64_t i = base + r * kBlock + threadIdx.x;
        valid[r] = i < end;
        row[r] = a.list[valid[r] ? i : begin];
    }
}

// fp32 rows in the blocked layout (D % 4 == 0), queries in SGPRs: flat_f32_sq_kernel
template <bool IP, int LANES, int QT, int CAP = FM_CAP, int TRIG = FM_TRIG>
__global__ __launch_bounds__(kBlock) void flat_masked_f32_sq_kernel(const FlatMaskedArgs a)
{
    __shared__ TopKShared<QT, CAP> tk;
    const int group = blockIdx.x / a.parts;
    int64_t begin, end;
    const int part = fm_slice(a, group, blockIdx.x % a.parts, &begin, &end);
    if (begin >= end) {   // (workgroup-uniform)
        topk_write_parts<true>(tk, group * QT, a.nq, part, a.parts, a.k, a.part_d, a.part_id, true);
        return;
    }
    dist_cfloat *qp[QT];
    dist_f32_uniform<QT>(qp, a.q, group, a.nq, a.D);
    topk_init(tk);
    __syncthreads();
    const float4 *X = reinterpret_cast<const float4 *>(a.data);
    const int D = a.D;
    int tile = 0;
    for (int64_t base = begin; base < end; base += kFmTile, ++tile) {
        uint32_t key[FM_R][QT], pay[FM_R];
        bool valid[FM_R];
        fm_rows(a, base, begin, end, pay, valid);
        const float4 *rowp[FM_R];
#pragma unroll
        for (int r = 0; r < FM_R; ++r) rowp[r] = X + (int64_t)(pay[r] >> 6) * (D >> 2) * 64 + (pay[r] & 63);
        float d[FM_R][QT];
        dist_f32_blocked<IP, LANES, QT, FM_R>(rowp, qp, D, d);
#pragma unroll
        for (int r = 0; r < FM_R; ++r)
#pragma unroll
            for (int q = 0; q < QT; ++q) key[r][q] = topk_key_f32(d[r][q], valid[r]);
        topk_tile<QT, FM_R, CAP, TRIG>(tk, a.k, tile, key, pay);
    }
    __syncthreads();
    topk_compact(tk, a.k);
    topk_write_parts<true>(tk, group * QT, a.nq, part, a.parts, a.k, a.part_d, a.part_id);
}

// fp32 row-major rows (D % 4 != 0), queries in LDS: flat_f32_kernel
template <bool IP, int QT, int CAP = FM_CAP, int TRIG = FM_TRIG>
__global__ __launch_bounds__(kBlock) void flat_masked_f32_kernel(const FlatMaskedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float fm_qs[];   // [QT][D]
    __shared__ TopKShared<QT, CAP> tk;
    const int group = blockIdx.x / a.parts;
    int64_t begin, end;
    const int part = fm_slice(a, group, blockIdx.x % a.parts, &begin, &end);
    if (begin >= end) {
        topk_write_parts<true>(tk, group * QT, a.nq, part, a.parts, a.k, a.part_d, a.part_id, true);
        return;
    }
    dist_f32_stage<QT>(fm_qs, reinterpret_cast<const float *>(a.q), group, a.nq, a.D);
    topk_init(tk);
    __syncthreads();
    const float *X = reinterpret_cast<const float *>(a.data);
    int tile = 0;
    for (int64_t base = begin; base < end; base += kFmTile, ++tile) {
        uint32_t key[FM_R][QT], pay[FM_R];
        bool valid[FM_R];
        fm_rows(a, base, begin, end, pay, valid);
#pragma unroll
        for (int r = 0; r < FM_R; ++r) {
            float d[QT];
            dist_f32_row<IP, 1, QT>(X + (int64_t)pay[r] * a.D, fm_qs, a.D, d);
#pragma unroll
            for (int q = 0; q < QT; ++q) key[r][q] = topk_key_f32(d[q], valid[r]);
        }
        topk_tile<QT, FM_R, CAP, TRIG>(tk, a.k, tile, key, pay);
    }
    __syncthreads();
    topk_compact(tk, a.k);
    topk_write_parts<true>(tk, group * QT, a.nq, part, a.parts, a.k, a.part_d, a.part_id);
}

// uint8 rows: flat_u8_kernel.  VEC: rows are whole 16-byte pieces (D % 16 == 0)
template <bool VEC, int QT, int CAP = FM_CAP, int TRIG = FM_TRIG>
__global__ __launch_bounds__(kBlock) void flat_masked_u8_kernel(const FlatMaskedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t fm_qw[];   // [QT][D / 4] packed query bytes
    __shared__ TopKShared<QT, CAP> tk;
    __shared__ uint32_t qq[QT];
    constexpr int FORM = VEC ? U8_PIECES : U8_BYTES;
    const int group = blockIdx.x / a.parts;
    int64_t begin, end;
    const int part = fm_slice(a, group, blockIdx.x % a.parts, &begin, &end);
    if (begin >= end) {
        topk_write_parts<false>(tk, group * QT, a.nq, part, a.parts, a.k, a.part_d, a.part_id, true);
        return;
    }
    const int W = a.D >> 2;   // 32-bit words per row that take part (dist_u8.h)
    dist_u8_stage<FORM, QT>(fm_qw, reinterpret_cast<const uint8_t *>(a.q), group, a.nq, a.D);
    topk_init(tk);
    __syncthreads();
    dist_u8_qnorms<FORM, QT>(qq, fm_qw, W);
    __syncthreads();
    const uint8_t *X = reinterpret_cast<const uint8_t *>(a.data);
    int tile = 0;
    for (int64_t base = begin; base < end; base += kFmTile, ++tile) {
        uint32_t key[FM_R][QT], pay[FM_R];
        bool valid[FM_R];
        fm_rows(a, base, begin, end, pay, valid);
#pragma unroll
        for (int r = 0; r < FM_R; ++r) {
            // dist_u8_row's loops, written out: behind the call the 4-query kernels are scheduled differently and the sparse-mask
            // cases of tools/flat_masked_times.py run up to 1 % slower (10 M x 512 bytes, 16 queries, 0.1 %: 0.1203 -> 0.1213 ms)
            const uint8_t *xr = X + (int64_t)pay[r] * a.D;
            uint32_t xx = 0, qx[QT];
#pragma unroll
            for (int q = 0; q < QT; ++q) qx[q] = 0;
            if constexpr (VEC) {
                for (int w = 0; w < W; w += 4) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(xr + 4 * w);
                    const uint32_t xv[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        xx = __builtin_amdgcn_udot4(xv[e], xv[e], xx, false);
#pragma unroll
                        for (int q = 0; q < QT; ++q) qx[q] = __builtin_amdgcn_udot4(fm_qw[q * W + w + e], xv[e], qx[q], false);
                    }
                }
            } else {
                for (int w = 0; w < W; ++w) {
                    const uint8_t *p = xr + 4 * w;
                    const uint32_t xv = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
                    xx = __builtin_amdgcn_udot4(xv, xv, xx, false);
#pragma unroll
                    for (int q = 0; q < QT; ++q) qx[q] = __builtin_amdgcn_udot4(fm_qw[q * W + w], xv, qx[q], false);
                }
            }
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const uint32_t d = qq[q] + xx - 2u * qx[q];   // exact: every term < 2^26
                key[r][q] = valid[r] ? d : KEY_MAX;
            }
        }
        topk_tile<QT, FM_R, CAP, TRIG>(tk, a.k, tile, key, pay);
    }
    __syncthreads();
    topk_compact(tk, a.k);
    topk_write_parts<false>(tk, group * QT, a.nq, part, a.parts, a.k, a.part_d, a.part_id);
}

// ---- host side ----
int flat_masked_form(int metric, int D)
{
    if (metric == CVTMI_METRIC_L2U8) return D % 16 == 0 ? 3 : 2;
    return flat_blocked(metric, D) ? 1 : 0;
}

template <bool IP, int LANES>
static int fm_launch_sq(const FlatMaskedArgs &a, int qt, int64_t blocks, hipStream_t st)
{
    auto kern = flat_masked_f32_sq_kernel<IP, LANES, 1, kBigCap, kBigTrig>;   // k > 128: one query per workgroup, the large selection buffer
    if (a.k <= 128) kern = qt == 4 ? flat_masked_f32_sq_kernel<IP, LANES, 4> : flat_masked_f32_sq_kernel<IP, LANES, 1>;
    return launch("flat_masked_f32_sq_kernel", kern, blocks, kBlock, 0, st, a);
}

template <bool IP>
static int fm_launch_rows(const FlatMaskedArgs &a, int qt, int64_t blocks, hipStream_t st)
{
    auto kern = flat_masked_f32_kernel<IP, 1, kBigCap, kBigTrig>;
    if (a.k <= 128) kern = qt == 4 ? flat_masked_f32_kernel<IP, 4> : flat_masked_f32_kernel<IP, 1>;
    return launch_lds("flat_masked_f32_kernel", kern, blocks, kBlock, (size_t)qt * a.D * sizeof(float), st, a);
}

int launch_flat_masked_search(int metric, int D, const void *data, int64_t n, const void *q, int64_t nq, int k, int qt, int parts,
                              const uint32_t *list, const int64_t *len, float *part_d, int64_t *part_id, hipStream_t st)
{
    if (nq <= 0) return CVTMI_OK;
    if (k < 1 || k > kBigK) return fail(CVTMI_EINVAL, "flat_search_masked: k=%d outside 1..%d", k, kBigK);
    if (n < 1 || n > 0xffffffffLL || nq > 0x7fffffff) return fail(CVTMI_EUNSUPPORTED, "flat_search_masked: index too large");
    if ((qt != 1 && qt != 4) || (k > 128 && qt != 1)) return fail(CVTMI_EINVAL, "flat_search_masked: %d queries per workgroup at k=%d", qt, k);
    if (parts < 1 || parts > 1024) return fail(CVTMI_EINVAL, "flat_search_masked: %d parts", parts);
    if (D < 1 || D > 4096) return fail(CVTMI_EUNSUPPORTED, "flat_search_masked: D=%d outside 1..4096", D);
    FlatMaskedArgs a;
    a.data = data; a.q = q; a.nq = (int)nq; a.D = D; a.k = k; a.parts = parts; a.list = list; a.len = len; a.part_d = part_d; a.part_id = part_id;
    const int64_t blocks = blocks_for(nq, qt) * parts;
    switch (metric) {
        case CVTMI_METRIC_IP:
            if (D % 4 == 0) return fm_launch_sq<true, 4>(a, qt, blocks, st);
            return fm_launch_rows<true>(a, qt, blocks, st);
        case CVTMI_METRIC_L2F:
            if (D % 16 == 0) return fm_launch_sq<false, 8>(a, qt, blocks, st);
            if (D % 4 == 0) return fm_launch_sq<false, 4>(a, qt, blocks, st);
            return fm_launch_rows<false>(a, qt, blocks, st);
        case CVTMI_METRIC_L2U8: {
            const size_t lds = (size_t)qt * ((D >> 2) + 1) * sizeof(uint32_t);
            decltype(&flat_masked_u8_kernel<true, 1>) kern;
            if (k > 128) kern = D % 16 == 0 ? flat_masked_u8_kernel<true, 1, kBigCap, kBigTrig> : flat_masked_u8_kernel<false, 1, kBigCap, kBigTrig>;
            else if (D % 16 == 0) kern = qt == 4 ? flat_masked_u8_kernel<true, 4> : flat_masked_u8_kernel<true, 1>;
            else kern = qt == 4 ? flat_masked_u8_kernel<false, 4> : flat_masked_u8_kernel<false, 1>;
            return launch("flat_masked_u8_kernel", kern, blocks, kBlock, lds, st, a);
        }
        default: break;
    }
    return fail(CVTMI_EINVAL, "flat_search_masked: unknown metric %d", metric);
}

// a result of nothing: every distance field 0x7f800000, every label -1 (an empty index)
__global__ void flat_masked_pad_kernel(uint32_t *__restrict__ dist, int64_t *__restrict__ labels, int64_t count)
{
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (int64_t)gridDim.x * kBlock) {
        dist[i] = 0x7f800000u;
        labels[i] = -1;
    }
}

int launch_flat_masked_pad(void *dist, int64_t *labels, int64_t count, hipStream_t st)
{
    if (count <= 0) return CVTMI_OK;
    const int64_t blocks = std::min<int64_t>(blocks_for(count, kBlock), 4096);
    return launch("flat_masked_pad_kernel", flat_masked_pad_kernel, blocks, kBlock, 0, st, reinterpret_cast<uint32_t *>(dist), labels, count);
}

}  // namespace cvtmi
