// adc_scan_p.hip -- adc_scan16p: the 15-bit filter scan (adc_scan16q, adc_scan.hip) for models with M = 8 or M = 4, NATIVE:
// no padded copy of the rows, no look-ups spent on zero tables.  (opq/src/IVFOPQ.h:24-29: PQindex[16], any M <= 16; the
// reference's own test model is M = 8, opq/src/multi_frame_index_test.cpp.  Scores: opq/src/IVFOPQ.cpp:300-309.)
//
// Round 5 served M < 16 through the M = 16 kernel over rows padded to 16 code bytes: an M = 8 row cost sixteen look-ups, eight of
// them into all-zero tables (3.1-3.4 M queries/s at 10 000 x 1 M rows -- the M = 16 rate for half the work).  Here a lane's 16-byte
// load holds RPL = 16 / M consecutive rows AS THEY LIE IN MEMORY.  The table in LDS keeps its sixteen 16-byte slots per code value
// (64 KB, as for M = 16), filled with 16 / M COPIES of the M sub-spaces' entries: lane c = lane & 15 reads copy c / M, and within it
// walks the sub-spaces in its own rotated order m = (t + c) & (M - 1), t = 0 .. M - 1, so the sixteen lanes of a ds_read_b128 group
// always hit sixteen different slots -- conflict-free, like the M = 16 walk.  The rows are streamed from a pre-rotated copy (row r
// rotated left by ((r / RPL) & (M - 1)) bytes within its M bytes: byte t of the stored row is the code of sub-space (t + c) & (M - 1)),
// so a look-up's LDS address is still one v_perm_b32.  The M look-ups of a row are summed into the four packed accumulators, tested,
// and the same accumulators then take the next row of the load: 16 look-ups, 32 v_add3 and RPL tests per load -- RPL rows for the
// price of one M = 16 row.  Everything else is adc_scan16q's, in adc_scan16q's own text (adc_scan16.h): 15-bit lower-bound tables
// (scan16q_build_tables<NT, M>: per-query scale over the M real tables), the workgroup frame around the loop, lazy selection on the
// integer keys between checkpoints, candidates re-summed exactly from the fp32 tables in the reference's m order
// (ExactFromLutBatch<M>) before they are ranked -- thresholds, kept sets and distances bit-identical to the reference's.
#include "adc_scan16.h"
#include "launch.h"

namespace cvtmi {

// the sixteen table reads of one 16-byte load (RPL rows of MP code bytes, pre-rotated): v[s * MP + t] = look-up t of row s
template <int MP>
__device__ __forceinline__ void scan16p_reads(const uint4 &ld, const uint32_t (&moffp)[MP / 4], const char *lut_b, uint4 (&v)[16])
{
    const uint32_t w[4] = { ld.x, ld.y, ld.z, ld.w };
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int t = i & (MP - 1);   // look-up within the row
        const uint32_t sel = 0x0c0c0000u | ((4u + (t & 3)) << 8) | (uint32_t)(t & 3);
        const uint32_t addr = __builtin_amdgcn_perm(w[i >> 2], moffp[t >> 2], sel);  // code*256 + slot*16
        v[i] = *reinterpret_cast<const uint4 *>(lut_b + addr);
    }
}
// the packed sums of row s of the load, on top of the start values (0, or 0x8000 - T per 16-bit field: see adc_scan16q)
template <int MP>
__device__ __forceinline__ void scan16p_sum(const uint4 (&v)[16], int s, uint32_t &s0, uint32_t &s1, uint32_t &s2, uint32_t &s3)
{
#pragma unroll
    for (int t = 0; t < MP; t += 2) {
        const uint4 &a = v[s * MP + t], &b = v[s * MP + t + 1];
        s0 = s0 + a.x + b.x; s1 = s1 + a.y + b.y; s2 = s2 + a.z + b.z; s3 = s3 + a.w + b.w;
    }
}

// the M look-ups of row s of a load: issue / accumulate separately (software pipelining across the rows of a load).
// FENCE: nothing is scheduled across the end of the issue (scan16p_row does without: with the fence the M = 8 loop comes out longer)
template <int MP, bool FENCE = true>
__device__ __forceinline__ void scan16p_issue(const uint4 &ld, int s, const uint32_t (&moffp)[MP / 4], const char *lut_b, uint4 (&v)[MP])
{
    const uint32_t w[4] = { ld.x, ld.y, ld.z, ld.w };
#pragma unroll
    for (int t = 0; t < MP; ++t) {
        const uint32_t sel = 0x0c0c0000u | ((4u + (t & 3)) << 8) | (uint32_t)(t & 3);
        const uint32_t addr = __builtin_amdgcn_perm(w[(s * MP + t) >> 2], moffp[t >> 2], sel);  // code*256 + slot*16
        v[t] = *reinterpret_cast<const uint4 *>(lut_b + addr);
    }
    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
}
template <int MP>
__device__ __forceinline__ void scan16p_accum(const uint4 (&v)[MP], uint32_t &s0, uint32_t &s1, uint32_t &s2, uint32_t &s3)
{
#pragma unroll
    for (int t = 0; t < MP; t += 2) {
        s0 = s0 + v[t].x + v[t + 1].x; s1 = s1 + v[t].y + v[t + 1].y;
        s2 = s2 + v[t].z + v[t + 1].z; s3 = s3 + v[t].w + v[t + 1].w;
    }
}

// the M look-ups of row s of a load, summed on top of the start values
template <int MP>
__device__ __forceinline__ void scan16p_row(const uint4 &ld, int s, const uint32_t (&moffp)[MP / 4], const char *lut_b,
                                            uint32_t &s0, uint32_t &s1, uint32_t &s2, uint32_t &s3)
{
    uint4 v[MP];
    scan16p_issue<MP, false>(ld, s, moffp, lut_b, v);
    scan16p_accum<MP>(v, s0, s1, s2, s3);
}

// first thresholds from a histogram of the split's first SQ_SEED_CHUNKS loads (64 RPL rows each): scan16q_seed for packed rows
template <int NT, int MP, class Load>
__device__ __forceinline__ void scan16p_seed(int k, const Load &load1k, const uint32_t (&moffp)[MP / 4], const char *lut_b, uint32_t *hist,
                                             const QuantParams &qp, const int *lazy, uint32_t *thr_x, uint32_t *thr_pk)
{
    constexpr int QT = SQ_QT, NW = NT / 64, RPL = 16 / MP;
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < QT * 256; i += NT) hist[i] = 0;
    __syncthreads();
    for (uint32_t ch = wave; ch < SQ_SEED_CHUNKS; ch += NW) {
        const uint4 ld = load1k(ch);
        uint4 v[16];
        scan16p_reads<MP>(ld, moffp, lut_b, v);
#pragma unroll
        for (int s = 0; s < RPL; ++s) {
            uint32_t sm[4] = { 0, 0, 0, 0 };
            scan16p_sum<MP>(v, s, sm[0], sm[1], sm[2], sm[3]);
#pragma unroll
            for (int q = 0; q < QT; ++q) {
                const uint32_t sq = (sm[q >> 1] >> (16 * (q & 1))) & 0xffffu;
                atomicAdd(&hist[q * 256 + (sq >> 7)], 1u);
            }
        }
    }
    __syncthreads();
    scan16_seed_threshold(k, hist, qp, lazy, thr_x, thr_pk);
    __syncthreads();
}

template <int NT, int MP>
__global__ __launch_bounds__(NT, NT / 128) void adc_scan16p_kernel(const ScanArgs a)
{
    constexpr int QT = SQ_QT, RPL = 16 / MP;
    static_assert(MP == 8 || MP == 4, "packed rows: M = 8 (two per load) or M = 4 (four)");
    __shared__ __attribute__((aligned(16))) uint32_t lut[256 * 16 * QT / 2];  // u16 [code j][slot][q]: 16 B per (j, slot)
    __shared__ TopKShared<QT, SQ_CAP> tk;
    __shared__ QuantParams qp;
    __shared__ struct { int stop, done_waves; uint32_t next_chunk; uint32_t thr_pk[QT / 2]; int lazy[QT]; int nonfinite[QT]; } ck;

    const ScanBlock blk = scan16_block(a);
    const int group = blk.group, split = blk.split;
    const int64_t my_rps = blk.my_rps;
    const int tid = threadIdx.x, lane = tid & 63;
    topk_init(tk);
    scan16q_build_tables<NT, MP>(a, group, lut, qp, reinterpret_cast<uint32_t(*)[16]>(&tk.buf[0][0]), ck.nonfinite, ck.lazy);

    const ExactFromLutBatch<MP> fixb{ a.codes, a.lut_g, a.K, a.nq, group };
    const QuantThr thrx{ &qp };
    scan16_init_thresholds(a, group, tid, tk, ck.thr_pk);
    if (tid == 0) { ck.stop = 0; ck.done_waves = 0; ck.next_chunk = 0; }
    __syncthreads();

    const int64_t row_begin = (int64_t)split * my_rps;   // a multiple of 2048 rows: whole 1 KB loads, lane <-> (row / RPL) & 63
    int64_t row_end = row_begin + my_rps;
    row_end = row_end < a.n_rows ? row_end : a.n_rows;
    const uint32_t n_local = (uint32_t)(row_end > row_begin ? row_end - row_begin : 0);
    const char *rows_b = reinterpret_cast<const char *>(a.codes_rot) + row_begin * MP;
    // one 16-byte load per lane = RPL rows; a wave's load = 1 KB = 64 RPL rows.  The last load may read up to 1 KB past the split (the
    // next split's rows, or the kDevSlack bytes every device buffer carries); what is read there is never used (lrow < n_local)
    constexpr uint32_t WROWS = 64 * RPL;
    const uint32_t n_chunks = (n_local + WROWS - 1) / WROWS;
    const uint32_t last_chunk = n_chunks ? n_chunks - 1 : 0;
    const uint32_t lane16 = (uint32_t)lane * 16u;
    auto load_rows = [&](uint32_t chunk) -> uint4 {
        const uint32_t cc = chunk < last_chunk ? chunk : last_chunk;  // wave-uniform
        return *reinterpret_cast<const uint4 *>(rows_b + (size_t)cc * 1024u + lane16);
    };
    auto load1k = [&](uint32_t c1k) -> uint4 { return *reinterpret_cast<const uint4 *>(rows_b + (size_t)c1k * 1024u + lane16); };
    const uint32_t c = tid & 15;
    uint32_t moffp[MP / 4];
#pragma unroll
    for (int w = 0; w < MP / 4; ++w) {
        moffp[w] = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) moffp[w] |= (((((4 * w + b + c) & (MP - 1)) | (c & ~(uint32_t)(MP - 1)))) * 16u) << (8 * b);
    }
    const char *lut_b = reinterpret_cast<const char *>(lut);
    if (a.seed && n_chunks >= 4 * SQ_SEED_CHUNKS)  // workgroup-uniform
        scan16p_seed<NT, MP>(a.k, load1k, moffp, lut_b, reinterpret_cast<uint32_t *>(&tk.buf[0][0]), qp, ck.lazy, tk.thr_x, ck.thr_pk);

    // ---- main loop: adc_scan16q's protocol (waves run on their own between checkpoints; a full buffer stops everybody) ----
    constexpr int NW = NT / 64;
    const uint32_t next_chunk_addr = (uint32_t)(uintptr_t)&ck.next_chunk;
    uint32_t it = scan16_grab_pair(next_chunk_addr, lane), it_next = it + 1u, done = 0, done_for = 0xffffffffu;
    bool counted = false;
    uint4 cur, nxt;
    if (n_local) cur = load_rows(it);
    for (;;) {
        uint32_t tpk[QT / 2], bpk[QT / 2];
#pragma unroll
        for (int i = 0; i < QT / 2; ++i) { tpk[i] = ck.thr_pk[i]; bpk[i] = 0x80008000u - tpk[i]; }
        while (it < n_chunks) {
            const int stop_seen = ck.stop;
            const uint32_t base = it * WROWS;
            nxt = load_rows(it_next);
            bool failed_any = false;
            // row by row: the M look-ups of a row, its test, (rarely) its candidates -- then the same accumulators take the next row of the
            // load.  (All RPL rows' sums kept until one common test spilled registers inside this loop at M = 4: 64 registers per lane.)
            // (M = 4: the four reads of row s + 1 are issued before row s is summed and tested -- a row's own four reads are too few to
            //  cover the LDS latency; at M = 8 two rows in flight would take every register the kernel has)
            constexpr bool PIPE = MP == 4;
            uint4 vr[PIPE ? 2 : 1][MP];
            if constexpr (PIPE) scan16p_issue<MP>(cur, 0, moffp, lut_b, vr[0]);
#pragma unroll
            for (int s = 0; s < RPL; ++s) {
                uint32_t s0 = bpk[0], s1 = bpk[1], s2 = bpk[2], s3 = bpk[3];
                if constexpr (PIPE) {
                    if (s + 1 < RPL) scan16p_issue<MP>(cur, s + 1, moffp, lut_b, vr[(s + 1) & 1]);
                    scan16p_accum<MP>(vr[s & 1], s0, s1, s2, s3);
                } else {
                    scan16p_row<MP>(cur, s, moffp, lut_b, s0, s1, s2, s3);
                }
                const uint32_t sg = (~((s0 & s1) & (s2 & s3))) & 0x80008000u;   // a clear bit 15 = sum < T for that query
                if (__ballot(sg != 0)) {  // rare once the thresholds have tightened
                    if (done_for != it) { done = 0; done_for = it; }
                    bool failed = false;
                    uint32_t lrow = base + (uint32_t)lane * RPL + s;
                    asm volatile("" : "+v"(lrow));
                    if (sg != 0 && lrow < n_local) {
                        const uint32_t sums[4] = { s0 - bpk[0], s1 - bpk[1], s2 - bpk[2], s3 - bpk[3] };   // (field-wise: no borrow)
                        failed = scan16_push_candidates(tk, sums, tpk, row_begin, lrow, s * QT, done);
                    }
                    failed_any |= __ballot(failed) != 0;
                }
            }
            if (failed_any) {  // some buffer is full: stop everyone, come back to this load after the compaction
                if (lane == 0) ck.stop = 1;
                break;
            }
            cur = nxt;
            it = it_next;
            it_next = scan16_after(it, next_chunk_addr, lane);
            if (__builtin_amdgcn_readfirstlane(stop_seen)) break;
        }
        if (it >= n_chunks && !counted) {
            counted = true;
            if (lane == 0) atomicAdd(&ck.done_waves, 1);
        }
        __syncthreads();  // checkpoint (A)
        bool need = ck.stop != 0;
#pragma unroll
        for (int q = 0; q < QT; ++q) need |= tk.cnt[q] >= SQ_TRIG;
        const bool all_done = ck.done_waves == NW;
        if (need) scan16_checkpoint_compact<NT>(a, group, tk, qp, ck.lazy, ck.thr_pk, ck.stop, fixb, thrx);  // workgroup-uniform
        __syncthreads();  // checkpoint (B)
        if (all_done && !need) break;
    }

    __syncthreads();
    topk_compact_wave<QT, SQ_CAP, NT, true>(tk, a.k, fixb, thrx);
    scan16_write_lists<NT, true>(a, tk, group, split, blk.my_splits);
}

int launch_adc_scan16p(const ScanArgs &a, int M, int64_t blocks, hipStream_t st)
{
    if (blocks <= 0) return CVTMI_OK;
    if (!a.codes_rot || !a.lut_g) return fail(CVTMI_EINVAL, "adc_scan16p: pre-rotated rows / table scratch missing");
    if (M != 8 && M != 4) return fail(CVTMI_EUNSUPPORTED, "adc_scan16p: M=%d (8 or 4)", M);
    if (a.only) return fail(CVTMI_EINVAL, "adc_scan16p: no group predicate (only)");   // (adc_scan16q_kernel alone reads it; its one source, adc_mfma.hip, is M = 16)
    return launch("adc_scan16p_kernel", M == 8 ? adc_scan16p_kernel<1024, 8> : adc_scan16p_kernel<1024, 4>, blocks, 1024, 0, st, a);
}

// packed pre-rotation: the 16-byte group g (= 16 / M rows) keeps its rows where they are, each rotated left by (g & (M - 1)) bytes
// within its M bytes: stored byte t of a row = its code byte (t + g) & (M - 1).  Groups [g0, g1).
template <int MP>
__global__ __launch_bounds__(kBlock) void rotate_codes_packed_kernel(const uint4 *__restrict__ codes, uint4 *__restrict__ out, int64_t g0, int64_t g1)
{
    const int64_t g = g0 + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= g1) return;
    const uint4 v = codes[g];
    const uint32_t c = (uint32_t)g & (MP - 1);
    uint4 o;
    if constexpr (MP == 8) {
        const auto rot8 = [&](uint32_t lo, uint32_t hi, uint32_t &olo, uint32_t &ohi) {   // 64-bit value rotated right by 8 c bits
            const unsigned long long x = ((unsigned long long)hi << 32) | lo;
            const unsigned long long y = c ? ((x >> (8 * c)) | (x << (64 - 8 * c))) : x;
            olo = (uint32_t)y; ohi = (uint32_t)(y >> 32);
        };
        rot8(v.x, v.y, o.x, o.y);
        rot8(v.z, v.w, o.z, o.w);
    } else {
        const auto rot4 = [&](uint32_t x) -> uint32_t { return c ? ((x >> (8 * c)) | (x << (32 - 8 * c))) : x; };
        o.x = rot4(v.x); o.y = rot4(v.y); o.z = rot4(v.z); o.w = rot4(v.w);
    }
    out[g] = o;
}

// rows [row0, n) of an M = 8 / M = 4 index: the groups that hold them (a partly filled last group reads the slack behind the rows)
int launch_rotate_codes_packed(const uint8_t *codes, int M, uint8_t *codes_rot, int64_t row0, int64_t n, hipStream_t st)
{
    if (n <= row0) return CVTMI_OK;
    if (M != 8 && M != 4) return fail(CVTMI_EINVAL, "rotate_codes_packed: M=%d", M);
    const int rpl = 16 / M;
    const int64_t g0 = row0 / rpl, g1 = (n + rpl - 1) / rpl;
    return launch("rotate_codes_packed_kernel", M == 8 ? rotate_codes_packed_kernel<8> : rotate_codes_packed_kernel<4>, blocks_for(g1 - g0, kBlock), kBlock, 0, st,
                  reinterpret_cast<const uint4 *>(codes), reinterpret_cast<uint4 *>(codes_rot), g0, g1);
}

}  // namespace cvtmi
