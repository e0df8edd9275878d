// api_internal.h -- what the files of the C-ABI glue share (api.hip: library level, api_opq.hip, api_flat.hip, api_models.hip,
// api_hnsw.hip): the scratch pool of a handle with its lease and its mutation ordering, the staging of a host-pointer entry through
// a leased set (host_call), the set-to-bitmap glue of the mask_* / remove_* / mark_deleted entries (sorted_unique, labels_to_mask,
// mask_host_finish), the handle structs, and the few helpers that cross a file.  Everything a single file uses stays static in that file.
#pragma once
#include <string.h>

#include <algorithm>
#include <functional>
#include <new>
#include <random>
#include <shared_mutex>
#include <vector>

#include "host_util.h"
#include "kernels.h"
#include "shard.h"

// a helper of the glue alone: shared between its files, kept out of the library's symbol table (the exports are the C ABI's business)
#define CVTMI_INTERNAL __attribute__((visibility("hidden")))

namespace cvtmi {

// What a per-call scratch set carries beside its buffers.  A handle keeps a small pool of sets: a search leases one for the duration
// of the call, so searches on one handle overlap -- on the host (several threads inside the library) and on the device (several
// streams).  The set remembers the stream it was last used on and an event recorded when that call returned: the next lessee on
// ANOTHER stream waits for the event first.
struct ScratchBase {
    hipStream_t own = nullptr;      // stream of the host-pointer entry (created on first use)
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool pending = false, busy = false;
    // staging of the host-pointer entries, on `own`: the queries, the two result arrays, the mask words (or the label set) -- see host_call
    DevBuf io_q, io_d, io_i, io_m;
    CVTMI_INTERNAL void release_lease_state()
    {
        for (DevBuf *b : { &io_q, &io_d, &io_i, &io_m }) b->release();
        if (own) (void)hipStreamDestroy(own);
        if (done) (void)hipEventDestroy(done);
        own = nullptr; done = nullptr;
    }
};

// the scratch sets of one handle, and the ordering between the calls that lease a set (Lease) and the calls that change the index
template <class S> struct ScratchPool {
    std::mutex mu;
    std::vector<S *> sets;
    hipEvent_t mutated = nullptr;   // recorded on the stream of the last mutation: searches on other streams wait for it
    hipStream_t mut_stream = nullptr;
    bool mut_pending = false;       // (never set on a handle nothing has mutated yet)
    // a mutation on stream st, between the two calls (the caller holds the handle exclusively): the stream first waits for every
    // search that is still in flight on another stream and for the last mutation, and the searches that follow wait for this one
    void mutation_begin(hipStream_t st)
    {
        std::lock_guard<std::mutex> g(mu);
        for (S *c : sets)
            if (c->pending && c->last != st) (void)hipStreamWaitEvent(st, c->done, 0);
        if (mut_pending && mut_stream != st) (void)hipStreamWaitEvent(st, mutated, 0);
    }
    void mutation_end(hipStream_t st)
    {
        if (!mutated) (void)hipEventCreateWithFlags(&mutated, hipEventDisableTiming);
        if (mutated && hipEventRecord(mutated, st) == hipSuccess) { mut_stream = st; mut_pending = true; }
    }
    void destroy()
    {
        for (S *c : sets) { c->release_all(); delete c; }
        sets.clear();
        if (mutated) (void)hipEventDestroy(mutated);
    }
};

// a scratch set of a handle for the duration of one call on stream st (nullptr + host = true: the set's own stream).  The caller
// holds the handle's rw lock shared, where the handle has one.
template <class S> struct Lease {
    ScratchPool<S> *pool = nullptr;
    S *s = nullptr;
    hipStream_t st = nullptr;
    bool used = false;
    template <class H> int open(H *handle, hipStream_t stream, bool host)
    {
        pool = &handle->pool; st = stream;
        {
            std::lock_guard<std::mutex> g(pool->mu);
            S *any = nullptr;
            for (S *c : pool->sets) {
                if (c->busy) continue;
                if (!host && c->pending && c->last == stream) { s = c; break; }   // same stream as before: nothing to wait for
                if (!any) any = c;
            }
            if (!s) s = any;
            if (!s) {
                s = new (std::nothrow) S();
                if (!s) return fail(CVTMI_ENOMEM, S::kLeaseNoMemory);
                pool->sets.push_back(s);
            }
            s->busy = true;
        }
        if (host) {
            if (!s->own && hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking) != hipSuccess) { close(); return fail(CVTMI_EHIP, "hipStreamCreate failed"); }
            st = s->own;
        }
        if (s->pending && s->last != st) (void)hipStreamWaitEvent(st, s->done, 0);
        if (pool->mut_pending && pool->mut_stream != st) (void)hipStreamWaitEvent(st, pool->mutated, 0);
        used = true;
        return CVTMI_OK;
    }
    void close()
    {
        if (!s) return;
        if (used) {
            if (!s->done) (void)hipEventCreateWithFlags(&s->done, hipEventDisableTiming);
            if (s->done && hipEventRecord(s->done, st) == hipSuccess) { s->last = st; s->pending = true; }
        }
        std::lock_guard<std::mutex> g(pool->mu);
        s->busy = false;
        s = nullptr;
    }
    ~Lease() { close(); }
    Lease() = default;
    Lease(const Lease &) = delete;
    Lease &operator=(const Lease &) = delete;
};

// The second upload of a host-pointer entry beside its queries (mask words, candidate lists): `bytes` from `src` into `to`, a buffer
// of the leased set.  An empty one still reserves 16 bytes -- the pointer selects the masked kernels -- and copies nothing.
struct HostUpload {
    DevBuf *to = nullptr;
    const void *src = nullptr;
    size_t bytes = 0;
};

// A host-pointer entry on an opened host lease (OPQ and flat entries check the mask length under the shared lock before they lease):
// queries, and `extra` where there is one, up through the set's staging buffers; run(S, q_dev, extra_dev, d_dev, i_dev, st) on the
// set's own stream; the result arrays (ib == 0: there is one) down; one wait -- the caller's arrays are complete when this returns.
template <class L, class Q, class D, class F>
CVTMI_INTERNAL int host_call(L &lease, const Q *q, size_t qb, HostUpload extra, D *out_d, size_t db, int64_t *out_i, size_t ib, F &&run)
{
    auto &S = *lease.s;
    hipStream_t st = lease.st;
    CVTMI_TRY(S.io_q.reserve(qb));
    if (extra.to) CVTMI_TRY(extra.to->reserve(std::max<size_t>(extra.bytes, 16)));
    CVTMI_TRY(S.io_d.reserve(db));
    if (ib) CVTMI_TRY(S.io_i.reserve(ib));
    CVTMI_HIP(hipMemcpyAsync(S.io_q.p, q, qb, hipMemcpyHostToDevice, st));
    if (extra.bytes) CVTMI_HIP(hipMemcpyAsync(extra.to->p, extra.src, extra.bytes, hipMemcpyHostToDevice, st));
    const void *extra_dev = extra.to ? extra.to->p : nullptr;
    CVTMI_TRY(run(S, static_cast<const Q *>(S.io_q.p), extra_dev, static_cast<D *>(S.io_d.p), S.io_i.template as<int64_t>(), st));
    CVTMI_HIP(hipMemcpyAsync(out_d, S.io_d.p, db, hipMemcpyDeviceToHost, st));
    if (ib) CVTMI_HIP(hipMemcpyAsync(out_i, S.io_i.p, ib, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    return CVTMI_OK;
}

// the distinct values of a set in host memory, ascending: the table the mark kernels search (mask_*, remove_*, mark_deleted)
template <class T> CVTMI_INTERNAL int sorted_unique(const char *who, const T *set, int64_t n, std::vector<T> &tab)
{
    try {
        tab.assign(set, set + n);
    } catch (...) {
        return fail(CVTMI_ENOMEM, "%s: out of host memory", who);
    }
    std::sort(tab.begin(), tab.end());
    tab.erase(std::unique(tab.begin(), tab.end()), tab.end());
    return CVTMI_OK;
}
// ... of a set on the device: it is sorted on the host, so it comes down first (sizeof(T) bytes per value, one wait on st)
template <class T> CVTMI_INTERNAL int sorted_unique_dev(const char *who, const T *set_dev, int64_t n, std::vector<T> &tab, hipStream_t st)
{
    std::vector<T> raw;
    try {
        raw.resize((size_t)n);
    } catch (...) {
        return fail(CVTMI_ENOMEM, "%s: out of host memory", who);
    }
    CVTMI_HIP(hipMemcpyAsync(raw.data(), set_dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    return sorted_unique(who, raw.data(), n, tab);
}

// The end of a host-pointer mask_* entry.  Only the `words` words that can hold a row pass through the device (io_m): they come down,
// the call waits, and the caller's words behind them are cleared here.
CVTMI_INTERNAL inline int mask_host_finish(const DevBuf &io_m, int64_t words, uint64_t *mask, int64_t mask_words, hipStream_t st)
{
    CVTMI_HIP(hipMemcpyAsync(mask, io_m.p, (size_t)words * 8, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    memset(mask + words, 0, (size_t)(mask_words - words) * 8);
    return CVTMI_OK;
}

// One result array of a host-pointer range search: `elem` bytes per hit, down from the staging buffer `stage` of the leased set
// into `host` (null: the caller does not want it).
struct RangeOut {
    void *host;
    DevBuf *stage;
    size_t elem;
};

// The end of a host-pointer range entry (`who`), behind the count that left lims on the device at lims_dev: lims comes down and the
// call waits -- the one wait it needs to know whether the result fits.  Without room and arrays that is the answer; more hits than
// room fail with the sizes in lims; otherwise the staging buffers grow to lims[nq] hits, fill(total) writes them there and they
// come down.  An array whose host pointer is null gets no staging room: fill must skip it (the entries' argument checks refuse a
// null array the fill always writes whenever cap > 0).
template <size_t N, class F>
CVTMI_INTERNAL int range_host_finish(const char *who, int64_t nq, int64_t cap, int64_t *lims, const int64_t *lims_dev, const RangeOut (&outs)[N],
                                     hipStream_t st, F &&fill)
{
    CVTMI_HIP(hipMemcpyAsync(lims, lims_dev, ((size_t)nq + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    const int64_t total = lims[nq];
    bool wanted = false;
    for (const RangeOut &o : outs) wanted = wanted || o.host;
    if (cap == 0 && !wanted) return CVTMI_OK;   // a count-only call: lims is the answer
    if (total > cap) return fail(CVTMI_ESPACE, "%s: %lld hits, room for %lld (lims holds the sizes)", who, (long long)total, (long long)cap);
    if (total == 0) return CVTMI_OK;
    for (const RangeOut &o : outs)
        if (o.host) CVTMI_TRY(o.stage->reserve((size_t)total * o.elem));
    CVTMI_TRY(fill(total));
    for (const RangeOut &o : outs)
        if (o.host) CVTMI_HIP(hipMemcpyAsync(o.host, o.stage->p, (size_t)total * o.elem, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    return CVTMI_OK;
}

// a cvtmi_*_last_* getter: the small array a search left on its handle, copied under the lock it was written under
template <class P, int N> CVTMI_INTERNAL void copy_last(P &pool, const int64_t (&last)[N], int64_t *out)
{
    std::lock_guard<std::mutex> g(pool.mu);
    for (int i = 0; i < N; ++i) out[i] = last[i];
}

}  // namespace cvtmi

using namespace cvtmi;   // (as every glue file did for itself: this header is theirs alone)

// per-call scratch of an OPQ search: rotated queries, tables (fp32 + the quantised images of adc_scan16h), partial lists, shared
// bounds, spill areas, the item table and the plan it was built from, the staging of the host-pointer entry
struct OpqScratch : ScratchBase {
    static constexpr const char *kLeaseNoMemory = "opq search: out of host memory";
    DevBuf s_qrot, s_part_d, s_part_id, s_lut, s_gthr, s_qlut, s_qp, s_spill, s_items, s_probe;
    DevBuf s_ivf;              // partial lists of an IVF search (ivf_search.hip)
    DevBuf s_masked;           // masked IVF search: the mask in list order; cvtmi_opq_mask_videos: the marked bitmap and its table
    DevBuf s_range;            // range search (ivf_range.hip): probe order, part counts and offsets, spill area; host entry: lims behind them
    DevBuf s_ref_d, s_ref_i;   // cvtmi_opq_search_refine: the [nq][R] candidate lists between the scan and the rerank
    DevBuf s_rank_ms, s_rank_tot, s_rank_seg;   // cvtmi_opq_rank_videos: the score rows of a frame chunk, the totals of a segment group, the segment offsets
    DevBuf io_t;               // ... its host-pointer entry: the totals the caller asked for
    ScanHPlan hplan;                       // the item table s_items holds ...
    int64_t hplan_n = -1, hplan_nq = -1;   // ... and the (rows, queries, forced splits, planner settings) it was built for
    int hplan_splits = 0, hplan_key = 0;
    DevBuf io_v;               // host-pointer range search: the video ids (beside ScratchBase's io_q / io_d / io_i)
    PinBuf io_pin;             // the pinned staging area of the host-pointer search (cvtmi_opq_search)
    void release_all()
    {
        for (DevBuf *b : { &s_qrot, &s_part_d, &s_part_id, &s_lut, &s_gthr, &s_qlut, &s_qp, &s_spill, &s_items, &s_probe, &s_ivf, &s_masked, &s_range, &s_ref_d, &s_ref_i, &s_rank_ms, &s_rank_tot, &s_rank_seg, &io_t, &io_v }) b->release();
        io_pin.release();
        release_lease_state();
    }
};

struct cvtmi_opq_s {
    int device = 0;
    HandleSync sync;
    OpqModelDev m{};
    float *d_coarse = nullptr, *d_books = nullptr, *d_R = nullptr;
    int32_t *d_perm = nullptr;
    // resident entries, insertion order
    DevBuf codes, lists, videos;
    DevBuf codes_rot;     // M = 16: rows rotated by (row & 15) bytes for adc_scan16q, built lazily at search time
    int64_t rot_n = 0;    // rows of codes_rot that are up to date
    DevBuf codes16;       // M < 16: the rows padded to 16 bytes with zeros, what the M = 16 scan kernels read (opq_pads; built lazily like codes_rot, which is then its rotation)
    int64_t pad_n = 0;    // rows of codes16 that are up to date
    int rot_kind = 0;     // what codes_rot holds: 0 = 16-byte rows (M = 16, or the padded copy) rotated by row & 15; 1 = the packed rotation of an M = 8 / 4 index (adc_scan_p.hip)
    // adc_mfma.hip: the int8 matrix-core bound filter of large M = 16 batches.  The model's part (books_h: the codebooks on the host, what
    // it is computed from on first use) and the decoded operand copy of the rows, built lazily like codes_rot (132 bytes per row at 128-d)
    std::vector<float> books_h;
    int mf_state = 0;           // 0 = not looked at yet, 1 = usable, -1 = off for this index (a non-finite codebook entry, K != 256, no memory)
    DevBuf mf_model;            // xb | nrm | c | s
    AdcMfmaModel mf{};
    DevBuf mf_pack, mf_norm;
    DevBuf mf_stat;             // profiled searches: queries and flagged queries of the last search on this route (cvtmi_opq_last_mfma)
    int64_t mf_n = 0;           // rows of mf_pack / mf_norm that are up to date
    int p_mfma = 1, p_mfma_cap = 4096, p_mfma_sample = 2;   // "scan_mfma", "scan_mfma_cap", "scan_mfma_sample"
    int64_t p_mfma_min_nq = 512, p_mfma_min_rows = 1000000, p_mfma_max_rows = -1;   // "scan_mfma_min_nq" / "_min_rows" / "_max_rows" (-1: the copy stays within 1 GB)
    int64_t n = 0;
    bool has_lists = false, has_videos = false;
    int64_t id_base = 0;
    // list-ordered (CSR) copy for the per-video query path, built lazily
    bool csr_valid = false;
    DevBuf csr_codes, csr_videos, csr_off, csr_scratch, csr_stats;
    int64_t csr_kept = 0, csr_longest = 0;  // entries in the CSR copy (list ids outside [0, coarseK) are dropped), longest list
    int32_t csr_vmin = 0, csr_vmax = -1;    // range of the video ids it holds
    // insertion index of every entry of the CSR copy (uint32, CSR order): what cvtmi_opq_search_ivf reports ids from.  Allocated and
    // filled only once an IVF search has been asked for on the handle (want_entry); rebuilt with the copy, invalid whenever it is
    DevBuf csr_entry;
    bool want_entry = false, csr_entry_valid = false;
    int64_t ivf_last[8] = {};               // grid of the last IVF search (cvtmi_opq_last_ivf_plan), written under pool.mu
    int64_t ivf_masked_last[8] = {};        // ... of the last masked IVF search (cvtmi_opq_last_ivf_masked)
    int64_t range_last[8] = {};             // ... and of the last range search (cvtmi_opq_last_range_plan)
    int64_t rank_last[4] = {};              // chunks and areas of the last ranking (cvtmi_opq_last_rank)
    // scratch of the calls that run one at a time (query_video: probe lists, rotated queries)
    DevBuf s_qrot, s_probe, s_rot;
    DevBuf rm_scratch;         // removal (opq_remove.hip): bitmap, tile offsets, the table of removal ids, the chunk-sized row scratch
    int64_t p_rm_chunk = 0;    // "remove_chunk": rows the move works on at a time (0 = the default)
    // Searches (cvtmi_opq_search*) run CONCURRENTLY, as the reference's QueryThrehold de facto may (opq/src/IVFOPQ.cpp:322-422 only
    // reads the index): each leases a scratch set from this pool for the duration of the call (OpqLease) and holds `rw` shared;
    // everything else -- add / reset / reserve, the lazily built copies of the rows, the one-at-a-time entries above -- holds it
    // exclusively (OpqExclusive, on top of the per-handle Serial that orders those calls among themselves).
    std::shared_timed_mutex rw;
    ScratchPool<OpqScratch> pool;
    // tuning / measurement
    int p_splits = 0, p_qtile = 0, p_profile = 0, p_variant = 7;
    int p_encode = 0;  // 0 = choose, 1 = VALU encode, 2 = matrix-core filter + exact resolution
    int p_prerot = 1;  // adc_scan16q reads a pre-rotated copy of the code rows (+16 bytes of HBM per row)
    int p_tail = 1, p_groups_a = 0, p_splits_b = 0;  // two-region scan plan: on / forced shape (tests)
    int p_lazy = 1, p_share = 1;  // adc_scan16q: lazy selection between checkpoints; row splits share their thresholds
    int p_small = 1;              // 1 .. 8 queries take the small-batch path (adc_scan_h.hip) when the library chooses the scan (scan_variant 7)
    static constexpr int kEvRing = 64;
    hipEvent_t ev0[kEvRing] = {}, ev1[kEvRing] = {};
    int ev_count = 0;  // scan launches recorded since the last cvtmi_opq_last_scan
    int64_t last_bytes = 0;
    int last_qt = 0, last_splits = 0;
};

// per-call scratch of a flat search
struct FlatScratch : ScratchBase {
    static constexpr const char *kLeaseNoMemory = "flat search: out of host memory";
    DevBuf s_part_d, s_part_id, s_gthr, s_stage;
    DevBuf f_stats, f_thr, f_marg, f_cnt, f_cand, f_sd, f_si, f_sd2, f_si2, f_seld, f_seli;   // matrix-core filter pipelines
    DevBuf fs_redo, fs_scratch;                                                                // fp32 stream
    DevBuf redo_count;                                                                         // "flat_count_redo": the count of the flags
    DevBuf s_range;                 // range search (flat_range.hip): part counts and offsets, spill area; host entry: lims behind them
    DevBuf io_c;                    // host-pointer entries: the candidate lists of cvtmi_flat_rerank, the label set of cvtmi_flat_mask_labels
    DevBuf s_masked;                // masked search (flat_masked.hip): tile offsets, scan levels, the row list; mask_labels: the marked bitmap and its table
    PinBuf io_pin;                  // small calls: [queries | distances | labels] in page-locked memory the kernels write into
    void release_all()
    {
        for (DevBuf *b : { &s_part_d, &s_part_id, &s_gthr, &s_stage, &f_stats, &f_thr, &f_marg, &f_cnt, &f_cand, &f_sd, &f_si, &f_sd2,
                           &f_si2, &f_seld, &f_seli, &fs_redo, &fs_scratch, &redo_count, &s_range, &io_c, &s_masked })
            b->release();
        io_pin.release();
        release_lease_state();
    }
};

struct cvtmi_flat_s {
    int device = 0;
    // searches hold `rw` shared, everything that changes the index (add, reset, the lazily built operand copies) exclusively
    std::shared_timed_mutex rw;
    ScratchPool<FlatScratch> pool;
    int metric = 0, D = 0;
    size_t row_bytes = 0;
    DevBuf data, labels, norms;  // norms: int32 |x-128|^2 per row, uint8 metric with D % 32 == 0 (MFMA path)
    DevBuf add_stage;            // staging of host rows on their way into the blocked layout
    DevBuf rm_scratch;           // removal (flat_remove.hip): bitmap, tile offsets, the table of removal labels, the chunk-sized row scratch
    int64_t p_rm_chunk = 0;      // "remove_chunk": rows the move works on at a time (0 = the default)
    int64_t p_range_part_rows = 0;   // "range_part_rows": rows per part of a range search (0 = the default)
    int64_t p_range_spill = -1;      // "range_spill": spill records per (query, part) (-1 = the default)
    int64_t range_last[6] = {};      // plan of the last range search (cvtmi_flat_last_range_plan), written under pool.mu
    int64_t p_rerank_rows_copy = 0;  // "rerank_rows_copy": 1 = a rerank builds / extends the row-major copy f_rows it would otherwise do without
    int64_t rerank_last[4] = {};     // the last rerank (cvtmi_flat_last_rerank), written under pool.mu
    int64_t p_masked_parts = 0;      // "masked_parts": parts per query group of a masked search (0 = the plan)
    int64_t masked_last[4] = {};     // the last masked search (cvtmi_flat_last_masked), written under pool.mu
    int64_t n = 0;
    int64_t id_base = 0;   // row r reports label id_base + r while labels are implicit (row shards, cvtmi_flat_set_id_base)
    bool identity = true;  // label == row
    // matrix-core filter of the fp32 search (flat_mfma.hip): bf16 operand copy of the rows, built on first use
    DevBuf f_pack, f_bias, f_istats;   // f_istats: [0] max |x|^2, [1] rows with a non-finite value (of the operand copy)
    int64_t f_pack_n = -1;      // rows the copy covers (-1: none)
    DevBuf f_rows;              // fp32: row-major copy of the rows for the threshold filter's exact finish ("flat_f32_rows_copy"; the blocked layout gathers 16 of every 128 bytes it fetches)
    int64_t f_rows_n = -1;      // rows it covers (-1: none)
    bool f_rows_failed = false; // it did not fit once: not tried again on this handle
    int f_pack_nch = 0;         // its K steps per row (the threshold filter of a width between two kernels pads with zeros)
    bool f_nonfinite = false;   // a row holds inf / NaN: the filter is not used
    std::atomic<int> f_last_filtered{0};    // how the last search was answered (0 exact, 1 filter pipeline, 2 fp32 stream, 3 fp32 threshold filter)
    std::atomic<long long> f_last_worst{0};  // its largest candidate list
    std::atomic<long long> f_last_redo{-1};  // queries of the last search the exact kernels answered under a redo flag (-1: not counted)
    // fp32 stream (flat_f32_stream.hip): per-row score bias, statistics of the rows ([0] max |x|^2, [1] non-finite rows)
    DevBuf fs_bias, fs_stats;
    int64_t fs_stats_n = -1;    // index size the host copy of the statistics belongs to
    bool fs_nonfinite = false;
};

// per-call scratch of an HNSW search: visited bits, spilled queues, re-rank lists
struct HnswScratch : ScratchBase {
    static constexpr const char *kLeaseNoMemory = "hnsw search: out of host memory";
    DevBuf s_vis, s_cand, s_err, s_rr_d, s_rr_id;
    DevBuf s_mark;   // cvtmi_hnsw_mask_labels: the marked bitmap, its tile counts and the table of the label set
    DevBuf s_live;   // a search on a graph with dead nodes: the caller's mask (or all ones) without the dead nodes
    void release_all()
    {
        for (DevBuf *b : { &s_vis, &s_cand, &s_err, &s_rr_d, &s_rr_id, &s_mark, &s_live }) b->release();
        release_lease_state();
    }
};
struct cvtmi_hnsw_s {
    uint32_t magic = 0x484e5357u;
    int device = 0, metric = 0, D = 0;
    HnswDevGraph g{};
    DevBuf vec, links0, labels, upper_off, upper;
    // the delete state (cvtmi_hnsw_mark_deleted): bit i & 63 of word i >> 6 = node i is deleted, ceil(n / 64) words in
    // use, the bits past n zero; n_dead = the bits set.  links0 keeps plain counts: the file's mark bit exists in save / load alone.
    DevBuf dead;
    int64_t n_dead = 0;
    // what cvtmi_hnsw_save needs beyond the device graph: the header fields as the file (or the build) set them, and the number
    // of upper levels of every element
    std::vector<int32_t> levels;
    uint64_t max_elements = 0, M = 0, efc = 0;
    double mult = 0.0;
    int32_t hdr_maxlevel = 0;
    uint32_t hdr_enterpoint = 0;
    ScratchPool<HnswScratch> pool;
    int64_t masked_last[4] = {};   // the last masked search (cvtmi_hnsw_last_masked), written under pool.mu
    int slots_per_cu_max = 32, cus = 256;
    // cvtmi_hnsw_add: searches (and cvtmi_hnsw_save) hold `rw` shared -- HnswLease takes it --, add / reserve / set_level_draws / mark_deleted / unmark_deleted exclusively
    std::shared_timed_mutex rw;
    int64_t upper_words = 0;       // words of `upper` in use: where the next row's upper-level block goes
    // the level stream (hnswalg.h:139-149): the engine after `level_draws` draws.  A build of n rows leaves n, a load 0 (the
    // reference's loadIndex leaves level_generator_ at its initialiser)
    std::default_random_engine level_rng = std::default_random_engine(100);
    int64_t level_draws = 0;
    int64_t add_last[4] = {};      // the last cvtmi_hnsw_add (cvtmi_hnsw_last_add)
    bool broken = false;           // an add failed after its kernels had begun to rewrite link lists: only destroy is answered
};

using OpqLease = Lease<OpqScratch>;
using FlatLease = Lease<FlatScratch>;
// a search on an HNSW handle: the scratch set, and the handle held shared against cvtmi_hnsw_add for as long as the set is
struct HnswLease : Lease<HnswScratch> {
    std::shared_lock<std::shared_timed_mutex> rd;
    int open(cvtmi_hnsw_s *handle, hipStream_t stream, bool host)
    {
        rd = std::shared_lock<std::shared_timed_mutex>(handle->rw);
        return Lease<HnswScratch>::open(handle, stream, host);
    }
    ~HnswLease() { close(); }   // the set's event is recorded before the handle is let go
};

namespace cvtmi {

extern thread_local std::string g_err;   // text of cvtmi_last_error (api.hip)
extern std::atomic<int> g_scanh_key;   // bumped by a REPLAN tuning key (api.hip); api_opq.hip compares it

int use_device(int dev);
int opq_rotate_impl(cvtmi_opq_t h, const float *x, int64_t n, float *y, hipStream_t st);   // api_opq.hip
// api_opq.hip: the first steps of a search on the leased set S: *q_rot = the queries as the codes see them (q itself, or S.s_qrot after
// the rotation), and for nprobe >= 1 the nprobe nearest lists of every query in S.s_probe (int32 [nq][nprobe]); nprobe == 0 rotates only
CVTMI_INTERNAL int opq_rotate_probe(cvtmi_opq_t h, OpqScratch &S, const float *q, int64_t nq, int rotate, int nprobe, hipStream_t st, const float **q_rot);
// api_flat.hip: the bitmap of the rows (nodes) whose label is in a set, on the scratch buffer W: the mark step of the flat removal over
// the n explicit labels `labels_dev`.  table: the T > 0 distinct labels of the set, ascending, in host memory (the caller waits for st
// before it lets them go); mask: a device pointer of mask_words > 0 words; n > 0
CVTMI_INTERNAL int labels_to_mask(DevBuf &W, const int64_t *labels_dev, int64_t n, const int64_t *table, int64_t T, uint64_t *mask, int64_t mask_words, hipStream_t st);
// api_flat.hip: cvtmi_flat_rerank_dev behind its argument checks (device pointers, stream st); skip_minus_one: a candidate of -1 is padding
int flat_rerank_on_stream(cvtmi_flat_t h, const void *q, int64_t nq, const int64_t *cand, int R, int64_t cand_base, bool skip_minus_one, int k,
                          void *dist, int64_t *labels, hipStream_t st);
int sharded_local_failure(cvtmi_comm_t c);
using ShardLocalSearch = std::function<int(int, const void *, float *, int64_t *)>;
int sharded_all(cvtmi_comm_t *comms, int ndev, const void *q, size_t q_bytes, int64_t nq, int k, void *dist, int64_t *ids,
                const int *devices, const ShardLocalSearch &local_search);

}  // namespace cvtmi

// the first lines of an entry that takes a handle: the handle is there (HNSW: and is one), its device is current
#define CHECK_H(h) \
    if (!(h)) return fail(CVTMI_EINVAL, "%s: null handle", __func__); \
    CVTMI_TRY(use_device((h)->device))
#define CHECK_HN(h) do { if (!(h) || (h)->magic != 0x484e5357u) return fail(CVTMI_EINVAL, "bad hnsw handle"); \
    if ((h)->broken) return fail(CVTMI_EINVAL, "hnsw handle: a cvtmi_hnsw_add failed part-way, the graph is incomplete; destroy the handle"); \
    CVTMI_TRY(use_device((h)->device)); } while (0)
