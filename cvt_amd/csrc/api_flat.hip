// api_flat.hip -- the flat (exhaustive fp32 / uint8) handle of the C ABI (include/cvtmi.h): add / reset, the exact search over a row
// range, the pipeline drivers, the dispatch between them (flat_route, flat_prepare), the search entries and their sharded forms.
#include <float.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "api_internal.h"
#include "launch.h"
#include "rm_common.h"

extern "C" {

// ================================================================ flat ========================
int cvtmi_flat_create(int metric, int D, cvtmi_flat_t *out)
{
    if (!out) return fail(CVTMI_EINVAL, "cvtmi_flat_create: null out");
    *out = nullptr;
    if (metric != CVTMI_METRIC_IP && metric != CVTMI_METRIC_L2F && metric != CVTMI_METRIC_L2U8)
        return fail(CVTMI_EINVAL, "cvtmi_flat_create: unknown metric %d", metric);
    if (D < 1 || D > 4096) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_create: D=%d outside 1..4096", D);
    int dev = 0;
    CVTMI_HIP(hipGetDevice(&dev));
    cvtmi_flat_s *h = new (std::nothrow) cvtmi_flat_s();
    if (!h) return fail(CVTMI_ENOMEM, "cvtmi_flat_create: out of host memory");
    h->device = dev; h->metric = metric; h->D = D;
    h->row_bytes = metric == CVTMI_METRIC_L2U8 ? (size_t)D : (size_t)D * sizeof(float);
    *out = h;
    return CVTMI_OK;
}

int cvtmi_flat_destroy(cvtmi_flat_t h)
{
    if (!h) return CVTMI_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    for (DevBuf *b : { &h->data, &h->labels, &h->norms, &h->add_stage, &h->rm_scratch, &h->f_pack, &h->f_bias, &h->f_istats, &h->fs_bias, &h->fs_stats, &h->f_rows })
        b->release();
    h->pool.destroy();
    delete h;
    return CVTMI_OK;
}

__global__ void iota_i64_kernel(int64_t *p, int64_t begin, int64_t end)
{
    for (int64_t i = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < end; i += (int64_t)gridDim.x * kBlock) p[i] = i;
}

static int flat_add_common(cvtmi_flat_t h, const void *x, const int64_t *labels, int64_t n, hipMemcpyKind kind,
                           hipStream_t st)
{
    if (n < 0 || (n > 0 && !x)) return fail(CVTMI_EINVAL, "cvtmi_flat_add: bad arguments");
    if (n == 0) return CVTMI_OK;
    const int64_t total = h->n + n;
    if (total > 0xfffffffeLL) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_add: more than 2^32-2 rows per handle");
    // (the operand copies keep covering their rows; flat_prepare packs the appended ones)
    bool explicit_labels = labels != nullptr;
    if (explicit_labels && kind == hipMemcpyHostToDevice && h->identity) {
        bool same = true;
        for (int64_t i = 0; i < n && same; ++i) same = labels[i] == h->n + i;
        if (same) explicit_labels = false;
    }
    const bool blocked = flat_blocked(h->metric, h->D);  // fp32 rows live in 64-row blocks: whole blocks are kept
    const size_t rows_held = blocked ? (size_t)((h->n + 63) / 64 * 64) : (size_t)h->n;
    const size_t rows_need = blocked ? (size_t)((total + 63) / 64 * 64) : (size_t)total;
    if (rows_need * h->row_bytes > h->data.cap) {
        size_t rows = std::max<size_t>(rows_need, (h->data.cap / h->row_bytes) * 2);
        rows = std::max<size_t>(rows, 1024);
        CVTMI_TRY(h->data.grow(rows * h->row_bytes, rows_held * h->row_bytes, st));
    }
    if (explicit_labels && h->identity) {
        h->identity = false;
        CVTMI_TRY(h->labels.grow((size_t)std::max<int64_t>(total, 1024) * 8, 0, st));
        if (h->n) {
            CVTMI_TRY(launch("iota_i64_kernel", iota_i64_kernel, 1024, kBlock, 0, st, h->labels.as<int64_t>(), (int64_t)0, h->n));
        }
    }
    if (!h->identity && (size_t)total * 8 > h->labels.cap)
        CVTMI_TRY(h->labels.grow(std::max<size_t>((size_t)total, h->labels.cap / 4) * 8, (size_t)h->n * 8, st));
    if (blocked) {
        const float *src = static_cast<const float *>(x);
        if (kind == hipMemcpyHostToDevice || ((uintptr_t)x & 15) != 0) {  // staged: host rows, or a device pointer off 16 bytes
            CVTMI_TRY(h->add_stage.reserve((size_t)n * h->row_bytes));
            CVTMI_HIP(hipMemcpyAsync(h->add_stage.p, x, (size_t)n * h->row_bytes, kind, st));
            src = h->add_stage.as<float>();
        }
        CVTMI_TRY(launch_flat_block(src, n, h->D, h->n, h->data.as<float>(), st));
        if (flat_f32_stream_qmax(h->D) > 0 || flat_f32_tfilter_width(h->D)) {   // score bias + row statistics of the streaming search / the threshold filter, padding rows zeroed
            if (!h->fs_stats.p) {
                CVTMI_TRY(h->fs_stats.reserve(16));
                CVTMI_HIP(hipMemsetAsync(h->fs_stats.p, 0, 16, st));
            }
            if (rows_need * 4 > h->fs_bias.cap)
                CVTMI_TRY(h->fs_bias.grow(std::max<size_t>(rows_need, h->fs_bias.cap / 2) * 4, rows_held * 4, st));
            CVTMI_TRY(launch_flat_f32_bias(h->data.as<float>(), h->D, h->metric, h->n, total, h->fs_bias.as<float>(), h->fs_stats.as<uint32_t>(), st));
            h->fs_stats_n = -1;
        }
    } else {
        CVTMI_HIP(hipMemcpyAsync(h->data.as<uint8_t>() + (size_t)h->n * h->row_bytes, x, (size_t)n * h->row_bytes, kind, st));
    }
    if (!h->identity) {
        if (labels) CVTMI_HIP(hipMemcpyAsync(h->labels.as<int64_t>() + h->n, labels, (size_t)n * 8, kind, st));
        else {
            CVTMI_TRY(launch("iota_i64_kernel", iota_i64_kernel, 1024, kBlock, 0, st, h->labels.as<int64_t>(), h->n, total));
        }
    }
    if (h->metric == CVTMI_METRIC_L2U8 && h->D % 32 == 0 && h->D <= 512) {
        if ((size_t)total * 4 > h->norms.cap)
            CVTMI_TRY(h->norms.grow(std::max<size_t>((size_t)total, h->norms.cap / 2) * 4, (size_t)h->n * 4, st));
        CVTMI_TRY(launch_flat_u8_norms(h->data.as<uint8_t>() + (size_t)h->n * h->row_bytes, n, h->D,
                                       h->norms.as<int32_t>() + h->n, st));
    }
    if (kind == hipMemcpyHostToDevice) CVTMI_HIP(stream_wait(st));
    h->n = total;
    return CVTMI_OK;
}

// a mutation on stream st: exclusive, ordered after every search that is still in flight on another stream, and searches
// that come later on other streams wait for it (Lease::open)
struct FlatMutation {
    cvtmi_flat_s *h;
    hipStream_t st;
    std::unique_lock<std::shared_timed_mutex> lk;
    FlatMutation(cvtmi_flat_s *handle, hipStream_t stream) : h(handle), st(stream), lk(handle->rw)
    {
        h->pool.mutation_begin(st);
    }
    ~FlatMutation() { h->pool.mutation_end(st); }
};

int cvtmi_flat_add(cvtmi_flat_t h, const void *x, const int64_t *labels, int64_t n)
{
    CHECK_H(h);
    FlatMutation mut(h, nullptr);
    return flat_add_common(h, x, labels, n, hipMemcpyHostToDevice, nullptr);
}

int cvtmi_flat_add_dev(cvtmi_flat_t h, const void *x, const int64_t *labels, int64_t n, void *stream)
{
    CHECK_H(h);
    FlatMutation mut(h, (hipStream_t)stream);
    return flat_add_common(h, x, labels, n, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

// ---- removal: one stable compaction of the rows, labels and norms on the device (flat_remove.hip) ----
// The set is a device array of labels.  Implicit labels: it is scattered into the bitmap as it is.  Explicit labels: `table` is the
// sorted table of its distinct values (host memory: it is uploaded into the scratch).  Everything the call needs is reserved before
// the first row moves; the host waits once, for the kept count, BEFORE the move: a call that drops nothing leaves the handle, its
// derived copies and its implicit labels alone.
static int flat_remove_common(cvtmi_flat_t h, const int64_t *set_dev, int64_t n_set, const int64_t *table, int64_t T, int64_t *removed,
                              int64_t *remap_dev, hipStream_t st)
{
    if (removed) *removed = 0;
    const int64_t n = h->n;
    if (n == 0) return CVTMI_OK;
    const bool blocked = flat_blocked(h->metric, h->D);
    const bool has_norms = h->metric == CVTMI_METRIC_L2U8 && h->D % 32 == 0 && h->D <= 512;   // (as flat_add_common keeps them)
    const FlatRmPlan p = flat_rm_plan(n, h->row_bytes, blocked, has_norms, h->identity ? 0 : T, h->p_rm_chunk);
    CVTMI_TRY(h->rm_scratch.reserve(p.bytes));
    void *S = h->rm_scratch.p;
    if (h->identity) {
        CVTMI_TRY(launch_rm_mark_ids(p.rm, S, set_dev, n_set, h->id_base, st));
    } else {
        if (T > 0) CVTMI_HIP(hipMemcpyAsync(static_cast<char *>(S) + p.off_table, table, (size_t)T * 8, hipMemcpyHostToDevice, st));
        CVTMI_TRY(launch_flat_rm_mark_labels(p, S, h->labels.as<int64_t>(), st));
    }
    int64_t kept = 0;
    CVTMI_HIP(hipMemcpyAsync(&kept, static_cast<char *>(S) + p.rm.off_total, sizeof kept, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    if (kept < 0 || kept > n) return fail(CVTMI_ESTATE, "cvtmi_flat_remove_labels: kept count %lld of %lld rows", (long long)kept, (long long)n);
    if (kept == n) {
        if (remap_dev) CVTMI_TRY(launch_rm_fill_remap(remap_dev, n, 1, st));
        return CVTMI_OK;
    }
    if (h->identity) {   // kept rows keep their labels: id_base + old row becomes an array, as cvtmi_flat_add does for the first explicit label
        CVTMI_TRY(h->labels.grow((size_t)std::max<int64_t>(n, 1024) * 8, 0, st));
        CVTMI_TRY(launch_flat_rm_iota(h->labels.as<int64_t>(), n, h->id_base, st));
        h->identity = false;
    }
    CVTMI_TRY(launch_flat_rm_move(p, S, h->data.p, h->labels.as<int64_t>(), has_norms ? h->norms.as<int32_t>() : nullptr, remap_dev, st));
    h->n = kept;
    // what the handle derives from its rows describes the kept rows only: the operand copies are rebuilt by the next search that
    // needs them (never taken for a prefix: flat_prepare extends a copy only where 0 < f_pack_n < n) ...
    h->f_pack_n = -1; h->f_rows_n = -1;
    if (blocked && h->fs_bias.p && h->fs_stats.p) {   // ... bias and statistics of the stream are recomputed here; the stale rows of the last block are zeroed
        CVTMI_HIP(hipMemsetAsync(h->fs_stats.p, 0, 16, st));
        CVTMI_TRY(launch_flat_f32_bias(h->data.as<float>(), h->D, h->metric, 0, kept, h->fs_bias.as<float>(), h->fs_stats.as<uint32_t>(), st));
        h->fs_stats_n = -1;
    }
    if (removed) *removed = n - kept;
    return CVTMI_OK;
}

// arguments first, before anything touches the device
static int flat_remove_check(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_flat_remove_labels: null handle");
    if (n_labels < 0 || (n_labels > 0 && !labels)) return fail(CVTMI_EINVAL, "cvtmi_flat_remove_labels: bad arguments");
    return CVTMI_OK;
}

int cvtmi_flat_remove_labels_dev(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, int64_t *removed, int64_t *remap, void *stream)
{
    CVTMI_TRY(flat_remove_check(h, labels, n_labels));
    CHECK_H(h);
    hipStream_t st = (hipStream_t)stream;
    FlatMutation mut(h, st);
    std::vector<int64_t> tab;   // explicit labels: the table of the set
    if (!h->identity && n_labels > 0 && h->n > 0) CVTMI_TRY(sorted_unique_dev("cvtmi_flat_remove_labels", labels, n_labels, tab, st));
    return flat_remove_common(h, labels, n_labels, tab.data(), (int64_t)tab.size(), removed, remap, st);
}

int cvtmi_flat_remove_labels(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, int64_t *removed, int64_t *remap)
{
    CVTMI_TRY(flat_remove_check(h, labels, n_labels));
    CHECK_H(h);
    FlatMutation mut(h, nullptr);
    const int64_t n0 = h->n;
    std::vector<int64_t> tab;
    Tmp ds, dm;
    if (n_labels > 0 && n0 > 0) {
        if (h->identity) CVTMI_TRY(ds.upload(labels, (size_t)n_labels * sizeof(int64_t)));
        else CVTMI_TRY(sorted_unique("cvtmi_flat_remove_labels", labels, n_labels, tab));
    }
    if (remap && n0 > 0) CVTMI_TRY(dm.alloc((size_t)n0 * sizeof(int64_t)));
    CVTMI_TRY(flat_remove_common(h, ds.as<int64_t>(), ds.p ? n_labels : 0, tab.data(), (int64_t)tab.size(), removed, dm.as<int64_t>(), nullptr));
    if (dm.p) CVTMI_HIP(hipMemcpy(remap, dm.p, (size_t)n0 * sizeof(int64_t), hipMemcpyDeviceToHost));
    else CVTMI_HIP(stream_wait(nullptr));
    return CVTMI_OK;
}

int cvtmi_flat_set_param(cvtmi_flat_t h, const char *name, int64_t value)
{
    if (!h || !name) return fail(CVTMI_EINVAL, "cvtmi_flat_set_param: null");
    if (!strcmp(name, "remove_chunk")) {
        if (value < 0 || value > ((int64_t)1 << 32)) return fail(CVTMI_EINVAL, "cvtmi_flat_set_param: remove_chunk must be 0 .. 2^32 rows");
        std::unique_lock<std::shared_timed_mutex> lk(h->rw);
        h->p_rm_chunk = value ? flat_rm_chunk_rows(value, h->row_bytes) : 0;   // whole tiles
        return CVTMI_OK;
    }
    if (!strcmp(name, "range_part_rows")) {
        if (value < 0 || value > ((int64_t)1 << 32)) return fail(CVTMI_EINVAL, "cvtmi_flat_set_param: range_part_rows must be 0 .. 2^32 rows");
        std::unique_lock<std::shared_timed_mutex> lk(h->rw);
        h->p_range_part_rows = blocks_for(value, kBlock) * kBlock;   // whole tiles
        return CVTMI_OK;
    }
    if (!strcmp(name, "range_spill")) {
        if (value < -1) return fail(CVTMI_EINVAL, "cvtmi_flat_set_param: range_spill must be -1 (the default) or a record count");
        std::unique_lock<std::shared_timed_mutex> lk(h->rw);
        h->p_range_spill = value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "rerank_rows_copy")) {
        if (value != 0 && value != 1) return fail(CVTMI_EINVAL, "cvtmi_flat_set_param: rerank_rows_copy must be 0 or 1");
        std::unique_lock<std::shared_timed_mutex> lk(h->rw);
        h->p_rerank_rows_copy = value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "masked_parts")) {
        if (value < 0 || value > 1024) return fail(CVTMI_EINVAL, "cvtmi_flat_set_param: masked_parts must be 0 (the plan) or 1 .. 1024 parts");
        std::unique_lock<std::shared_timed_mutex> lk(h->rw);
        h->p_masked_parts = value;
        return CVTMI_OK;
    }
    return fail(CVTMI_EINVAL, "cvtmi_flat_set_param: unknown parameter '%s'", name);
}

int cvtmi_flat_ntotal(cvtmi_flat_t h, int64_t *n)
{
    if (!h || !n) return fail(CVTMI_EINVAL, "cvtmi_flat_ntotal: null");
    *n = h->n;
    return CVTMI_OK;
}

int cvtmi_flat_reset(cvtmi_flat_t h)
{
    CHECK_H(h);
    FlatMutation mut(h, nullptr);
    h->n = 0; h->identity = true; h->f_pack_n = -1; h->f_rows_n = -1;
    h->fs_stats_n = -1; h->fs_nonfinite = false;
    (void)hipDeviceSynchronize();
    if (h->fs_stats.p) CVTMI_HIP(hipMemset(h->fs_stats.p, 0, 16));
    h->f_pack.release(); h->f_bias.release(); h->f_rows.release(); h->f_rows_failed = false;  // the filter's copies are as large as the rows: give them back
    return CVTMI_OK;
}

// the exact search over rows [0, n_rows) of the handle: k smallest (distance, row) per query, rows not yet mapped to labels
// max_stream_passes: the uint8 streaming kernel serves 128 queries per pass; callers that search a short row range for many queries (the
// filter pipeline's sample stage) cap the passes and fall through to the row-tile kernels beyond
static int flat_search_rows(cvtmi_flat_t h, FlatScratch &S, int64_t n_rows, const void *q, int64_t nq, int k, float *dist, int64_t *rows, hipStream_t st,
                            int64_t max_stream_passes = INT64_MAX, const uint32_t *only_if = nullptr)
{
    // uint8: anything the filter pipeline did not take goes through the streaming matrix-core kernel, 128 queries per pass (its cost hardly
    // depends on k: 10 M x 512-d, k = 128: nq = 1000 40.6 -> 10 ms, nq = 4096 117 -> 40 ms against the row-tile kernels)
    if (h->metric == CVTMI_METRIC_L2U8 && tune_flat_variant.geti() != 1 && h->norms.p && nq >= 1 && flat_u8_mstream_applies(h->D, n_rows, std::min<int64_t>(nq, 128), k) &&
        ((uintptr_t)q & 15) == 0 && (nq + 127) / 128 <= max_stream_passes && !only_if) {   // (a predicated run: the row-per-lane kernels, which take one)
        const int64_t passes = (nq + 127) / 128, per = (nq + passes - 1) / passes;   // balanced: 129 queries = 65 + 64
        const int NS = flat_u8_stream_slices();
        int nqp = 0, waves = 0;
        const size_t bytes = flat_u8_mstream_scratch(n_rows, per, &nqp, &waves);
        CVTMI_TRY(S.s_stage.reserve(bytes));
        CVTMI_TRY(S.s_part_d.reserve((size_t)per * NS * k * sizeof(float)));
        CVTMI_TRY(S.s_part_id.reserve((size_t)per * NS * k * sizeof(int64_t)));
        for (int64_t a = 0; a < nq; a += per) {
            const int64_t m = std::min(per, nq - a);
            (void)flat_u8_mstream_scratch(n_rows, m, &nqp, &waves);
            const uint8_t *qa = reinterpret_cast<const uint8_t *>(q) + a * h->D;
            int32_t *tmin = S.s_stage.as<int32_t>(), *wmin = tmin + (size_t)flat_u8_mstream_groups(n_rows) * nqp;
            CVTMI_TRY(launch_flat_u8_mstream(h->D, h->data.as<uint8_t>(), h->norms.as<int32_t>(), n_rows, qa, m, tmin, wmin, st));
            CVTMI_TRY(launch_flat_u8_mstream_finish(h->D, h->data.as<uint8_t>(), n_rows, qa, m, k, wmin, waves, tmin, nqp, flat_u8_mstream_group(), S.s_part_d.as<float>(),
                                                    S.s_part_id.as<int64_t>(), dist + a * k, rows + a * k, st));
        }
        return CVTMI_OK;
    }
    const bool mfma = h->metric == CVTMI_METRIC_L2U8 && !only_if && flat_u8_mfma_qtile(h->D, k, nq) > 0;
    const int qt = mfma ? flat_u8_mfma_qtile(h->D, k, nq) : (k > 128 ? 1 : flat_qtile(nq));   // k > 128: one query per workgroup (kernels.h: kBigK)
    int splits = mfma ? flat_u8_mfma_splits(n_rows, nq, qt) : flat_plan_splits(n_rows, nq, qt);
    if (mfma && splits >= 8) splits = (splits / 8) * 8;  // a row split per XCD: query groups share its L2
    // a predicated re-run normally finds nothing to do, and what it finds is a few queries: its row splits do not follow the plan for the
    // whole batch (1000 queries: one or two splits -- ONE flagged query then waited for a single workgroup to read every row: 5 ms on
    // 0.5 GB of 300-d rows) but are 32 wherever the rows allow it; an empty workgroup costs a dispatch and the read of its flags
    // (never fewer than the plan's own: a small batch has few query groups and the plan cuts the rows finer for it -- 15 queries over 300 000 x
    //  2048-d rows, 11 of them flagged: 146 splits instead of 32, 5.4 -> 1.9 ms)
    if (only_if && !mfma) {
        splits = (int)std::max<int64_t>(splits, std::min<int64_t>(32, n_rows / 8192));
        // (the partial lists of a re-run are sized for every query, flagged or not: at most ~1 GB of them)
        const int64_t room = std::max<int64_t>(1, (int64_t)(1LL << 30) / std::max<int64_t>(1, nq * (int64_t)k * 12));
        if (splits > room) splits = (int)room;
    }
    float *pd = dist;
    int64_t *pi = rows;
    if (splits > 1) {
        const size_t cnt = (size_t)nq * splits * k;
        CVTMI_TRY(S.s_part_d.reserve(cnt * sizeof(float)));
        CVTMI_TRY(S.s_part_id.reserve(cnt * sizeof(int64_t)));
        pd = S.s_part_d.as<float>();
        pi = S.s_part_id.as<int64_t>();
    }
    if (mfma) {
        CVTMI_TRY(S.s_gthr.reserve((size_t)nq * (1 + 16) * sizeof(uint32_t)));
        CVTMI_TRY(launch_flat_u8_mfma(h->D, h->data.as<uint8_t>(), h->norms.as<int32_t>(), n_rows,
                                      reinterpret_cast<const uint8_t *>(q), nq, k, splits, pd, pi, S.s_gthr.as<uint32_t>(), st));
    }
    else
        CVTMI_TRY(launch_flat_search(h->metric, h->D, h->data.p, n_rows, q, nq, k, qt, splits, pd, pi, st, only_if));
    if (splits > 1) CVTMI_TRY(launch_topk_merge(pd, pi, nq, splits, k, dist, rows, st, only_if));
    return CVTMI_OK;
}

// "flat_count_redo" 1: how many of a search's nq queries the threshold filters / the fp32 stream flagged for the exact kernels
// (h->f_last_redo, cvtmi_flat_last_redo).  Off by default: the count is copied back and waited for
static int flat_count_redo(cvtmi_flat_t h, FlatScratch &S, const uint32_t *flags, int64_t nq, hipStream_t st)
{
    if (!tune_flat_count_redo.geti()) return CVTMI_OK;
    CVTMI_TRY(S.redo_count.reserve(sizeof(uint32_t)));
    CVTMI_TRY(launch_count_nonzero(flags, nq, S.redo_count.as<uint32_t>(), st));
    uint32_t c = 0;
    CVTMI_HIP(hipMemcpyAsync(&c, S.redo_count.p, sizeof(c), hipMemcpyDeviceToHost, st));
    CVTMI_HIP(hipStreamSynchronize(st));
    h->f_last_redo = (long long)c;
    return CVTMI_OK;
}

// fp32 search as a stream over the rows (flat_f32_stream.hip).  *done = false: not applicable, the other paths answer
static int flat_search_streamed(cvtmi_flat_t h, FlatScratch &S, const float *q, int64_t nq, int k, float *dist, int64_t *rows, hipStream_t st, bool *done,
                                int *how = nullptr)
{
    *done = false;
    const int D = h->D;
    const int64_t n = h->n;
    if (!h->fs_bias.p || !h->fs_stats.p || h->fs_stats_n != n || h->fs_nonfinite) return CVTMI_OK;
    if (flat_f32_tfilter_applies(h->metric, D, n, nq, k) && h->f_pack.p && h->f_pack_n == n && h->f_pack_nch == flat_f32_tfilter_nch(D) && !h->f_nonfinite &&
        S.fs_scratch.reserve(flat_f32_tfilter_scratch(nq, k)) == CVTMI_OK) {
        // large batches (round 6, flat_f32_tfilter.hip): sample maxima -> per-query threshold -> barrier-free threshold filter (queries in
        // LDS, the rows' bf16 operand copy in registers) -> exact distances of the candidates; flagged queries go through the exact
        // kernels below, as for the stream
        CVTMI_TRY(S.fs_redo.reserve((size_t)nq * 2 * sizeof(uint32_t)));
        CVTMI_TRY(launch_flat_f32_tfilter(h->metric, D, h->data.as<float>(), (h->f_rows.p && h->f_rows_n == n) ? h->f_rows.as<float>() : nullptr, h->f_pack.p, h->f_istats.as<uint32_t>(), h->fs_bias.as<float>(), h->fs_stats.as<uint32_t>(), n, q, nq, k,
                                          S.fs_scratch.p, dist, rows, S.fs_redo.as<uint32_t>(), st));
        CVTMI_TRY(flat_count_redo(h, S, S.fs_redo.as<uint32_t>(), nq, st));
        CVTMI_TRY(flat_search_rows(h, S, n, q, nq, k, dist, rows, st, INT64_MAX, S.fs_redo.as<uint32_t>()));
        *done = true;
        if (how) *how = 3;
        return CVTMI_OK;
    }
    (void)hipGetLastError();
    if (!flat_f32_stream_applies(h->metric, D, n, k)) return CVTMI_OK;   // (a width only the threshold filter takes)
    const int qmax = flat_f32_stream_qmax(D), qpriv = flat_f32_stream_private_max(D);
    int64_t passes = blocks_for(nq, qmax);
    // just past one private-ring pass, two of them beat one pass of the shared ring (1 M x 128-d, 128 queries: 0.28 against 0.32 ms)
    if (nq > qpriv && nq <= 2 * qpriv) passes = 2;
    const int64_t per = blocks_for(nq, passes);
    if (S.fs_scratch.reserve(flat_f32_stream_scratch(D, n, per)) != CVTMI_OK) return CVTMI_OK;   // no room: the exact path answers
    CVTMI_TRY(S.fs_redo.reserve((size_t)nq * 2 * sizeof(uint32_t)));   // redo flags, then list counters
    // round 6: the bf16 operand copy of the threshold filter, when the handle keeps one, is what a small batch streams (half the bytes)
    const bool have_pack = h->f_pack.p && h->f_istats.p && h->f_pack_n == n && D % 16 == 0 && h->f_pack_nch == D / 16 && !h->f_nonfinite;
    for (int64_t a = 0; a < nq; a += per) {
        const int64_t m = std::min(per, nq - a);
        CVTMI_TRY(launch_flat_f32_stream(h->metric, D, h->data.as<float>(), h->fs_bias.as<float>(), h->fs_stats.as<uint32_t>(), n, q + a * D, m, k,
                                         S.fs_scratch.p, dist + a * k, rows + a * k, S.fs_redo.as<uint32_t>() + a,
                                         S.fs_redo.as<uint32_t>() + nq + a, st, have_pack ? h->f_pack.p : nullptr,
                                         have_pack ? h->f_istats.as<uint32_t>() : nullptr,
                                         (h->f_rows.p && h->f_rows_n == n) ? h->f_rows.as<float>() : nullptr));
    }
    // queries the bound does not cover / whose lists ran over: the exact kernels, predicated on the flags (they exit at once otherwise)
    CVTMI_TRY(flat_count_redo(h, S, S.fs_redo.as<uint32_t>(), nq, st));
    CVTMI_TRY(flat_search_rows(h, S, n, q, nq, k, dist, rows, st, INT64_MAX, S.fs_redo.as<uint32_t>()));
    *done = true;
    return CVTMI_OK;
}

// fp32 search through the matrix-core filter (flat_mfma.hip).  *done = false: not applicable / gave up, take the exact path
static int flat_search_filtered(cvtmi_flat_t h, FlatScratch &S, const float *q, int64_t nq, int k, float *dist, int64_t *rows, hipStream_t st, bool *done)
{
    *done = false;
    const int D = h->D;
    const int64_t n = h->n;
    if (h->f_pack_n != n || h->f_pack_nch != D / 16 || h->f_nonfinite) return CVTMI_OK;   // no operand copy (flat_prepare could not build it) / non-finite rows: exact path
    CVTMI_TRY(S.f_stats.reserve(16));
    CVTMI_HIP(hipMemcpyAsync(S.f_stats.p, h->f_istats.p, 8, hipMemcpyDeviceToDevice, st));   // [0] max |x|^2, [1] non-finite rows; [2], [3] are this call's
    // 1. exact search of a leading sample: its k-th best bounds the global k-th best
    // a smaller sample costs less exact work but doubles the survivors: worth it while k is small
    const int frac = k <= 16 ? 32 : 16;
    int64_t ns = std::max<int64_t>(frac == 32 ? 32768 : 65536, (n / frac + 63) / 64 * 64);
    const int cap = ((frac == 32 ? 48 : 24) * k + 1024 + 63) / 64 * 64;
    CVTMI_TRY(S.f_sd.reserve((size_t)nq * k * sizeof(float)));
    CVTMI_TRY(S.f_si.reserve((size_t)nq * k * sizeof(int64_t)));
    CVTMI_TRY(S.f_thr.reserve((size_t)nq * sizeof(float)));
    CVTMI_TRY(S.f_cnt.reserve((size_t)nq * sizeof(uint32_t)));
    const uint64_t pair_cap64 = (uint64_t)nq * cap;
    const uint32_t pair_cap = pair_cap64 > 0x7ffffff0ull ? 0x7ffffff0u : (uint32_t)pair_cap64;
    // the big scratch (16 bytes per survivor slot + 8 per list entry): if it does not fit, the exact path answers
    if (S.f_cand.reserve((size_t)pair_cap * sizeof(uint4)) != CVTMI_OK || S.f_seld.reserve((size_t)nq * cap * sizeof(float)) != CVTMI_OK ||
        S.f_seli.reserve((size_t)nq * cap * sizeof(int32_t)) != CVTMI_OK)
        return CVTMI_OK;
    CVTMI_TRY(S.f_marg.reserve((size_t)nq * sizeof(float)));
    uint32_t *stats = S.f_stats.as<uint32_t>();  // [0] max |x|^2, [1] non-finite rows, [2] overflow / worst list, [3] pair count
    // one filter stage: given the exact top k of rows [0, r0) in (sd, si), the exact top k of rows [0, r1) into (od, oi):
    // thresholds, filter over [r0, r1), second cut on approximate scores, exact distances of what is left, sort
    auto stage = [&](int64_t r0, int64_t r1, const float *sd, const int64_t *si, float *od, int64_t *oi, uint32_t *worst) -> int {
        CVTMI_HIP(hipMemsetAsync(stats + 2, 0, 8, st));
        CVTMI_TRY(launch_flat_thr(q, nq, D, h->metric, sd, k, stats, S.f_thr.as<float>(), S.f_marg.as<float>(), st));
        CVTMI_HIP(hipMemsetAsync(S.f_cnt.p, 0, (size_t)nq * sizeof(uint32_t), st));
        CVTMI_TRY(launch_flat_filter(q, nq, D, h->f_pack.as<uint4>(), h->f_bias.as<uint32_t>(), S.f_thr.as<float>(), r0, r1, pair_cap,
                                     stats + 3, S.f_cand.as<uint4>(), st));
        CVTMI_TRY(launch_flat_finish(h->metric, h->data.as<float>(), r1, D, q, nq, stats + 3, pair_cap, S.f_cand.as<uint4>(), cap, k,
                                     S.f_marg.as<float>(), sd, si, S.f_cnt.as<uint32_t>(), S.f_seld.as<float>(), S.f_seli.as<int32_t>(),
                                     od, oi, stats + 2, st));
        CVTMI_HIP(hipMemcpyAsync(worst, stats + 2, 4, hipMemcpyDeviceToHost, st));
        CVTMI_HIP(stream_wait(st));
        return CVTMI_OK;
    };
    // 1. the exact top k of the leading ns rows.  The exact kernels only see a sample of the sample (ns / 16 rows); a first
    //    filter stage extends it to ns (falling back to the exact kernels on all ns rows if a list runs over)
    uint32_t worst = 0;
    const int64_t ns0 = std::max<int64_t>(8192, (ns / 16 + 63) / 64 * 64);
    bool have_sample = false;
    if (ns0 * 4 <= ns && nq >= 256) {  // (small batches: the extra launches and the sync cost more than the exact work saved)
        CVTMI_TRY(S.f_sd2.reserve((size_t)nq * k * sizeof(float)));
        CVTMI_TRY(S.f_si2.reserve((size_t)nq * k * sizeof(int64_t)));
        CVTMI_TRY(flat_search_rows(h, S, ns0, q, nq, k, S.f_sd2.as<float>(), S.f_si2.as<int64_t>(), st));
        CVTMI_TRY(stage(ns0, ns, S.f_sd2.as<float>(), S.f_si2.as<int64_t>(), S.f_sd.as<float>(), S.f_si.as<int64_t>(), &worst));
        have_sample = worst <= (uint32_t)cap;
    }
    if (!have_sample) CVTMI_TRY(flat_search_rows(h, S, ns, q, nq, k, S.f_sd.as<float>(), S.f_si.as<int64_t>(), st));
    // 2. the remaining rows
    CVTMI_TRY(stage(ns, n, S.f_sd.as<float>(), S.f_si.as<int64_t>(), dist, rows, &worst));
    h->f_last_worst = (long long)worst;
    if (worst > (uint32_t)cap) return CVTMI_OK;  // a list ran over: the exact path answers this call (and overwrites the output)
    *done = true;
    return CVTMI_OK;
}

// uint8 L2 through the filter pipeline (flat_mfma.hip): exact integer distances on the i8 matrix cores, thresholds from an
// exactly searched leading sample.  *done = false: not applicable / a list ran over, the row-tile kernels answer
static int flat_search_filtered_u8(cvtmi_flat_t h, FlatScratch &S, const uint8_t *q, int64_t nq, int k, float *dist, int64_t *rows, hipStream_t st, bool *done)
{
    *done = false;
    const int D = h->D;
    const int64_t n = h->n;
    if (h->f_pack_n != n) return CVTMI_OK;   // no operand copy (flat_prepare could not build it): the row-tile kernels answer
    // (at least 262 144 rows where the table has twice that: the smallest sample the streaming kernel takes -- through the row-tile
    //  kernels a sample costs ~1 ms whatever its size)
    const int64_t ns = std::max<int64_t>(n >= 2 * 262144 ? 262144 : 65536, (n / 32 + 63) / 64 * 64);
    const int cap = std::min(4096 - k, (48 * k + 1024 + 63) / 64 * 64);
    const uint64_t pair_cap64 = (uint64_t)nq * cap;
    const uint32_t pair_cap = pair_cap64 > 0x7ffffff0ull ? 0x7ffffff0u : (uint32_t)pair_cap64;
    CVTMI_TRY(S.f_stats.reserve(16));
    CVTMI_TRY(S.f_sd.reserve((size_t)nq * k * sizeof(float)));
    CVTMI_TRY(S.f_si.reserve((size_t)nq * k * sizeof(int64_t)));
    CVTMI_TRY(S.f_cnt.reserve((size_t)nq * sizeof(uint32_t)));
    if (S.f_cand.reserve((size_t)pair_cap * sizeof(uint4)) != CVTMI_OK || S.f_seld.reserve((size_t)nq * cap * sizeof(float)) != CVTMI_OK ||
        S.f_seli.reserve((size_t)nq * cap * sizeof(int32_t)) != CVTMI_OK)
        return CVTMI_OK;
    uint32_t *stats = S.f_stats.as<uint32_t>();  // [2] worst list / overflow, [3] pair count
    // one filter stage: the exact top k of rows [0, r0) in (sd, si) -> the exact top k of rows [0, r1) in (od, oi)
    uint32_t worst = 0;
    auto stage = [&](int64_t r0, int64_t r1, const float *sd, const int64_t *si, float *od, int64_t *oi) -> int {
        CVTMI_HIP(hipMemsetAsync(stats + 2, 0, 8, st));
        CVTMI_HIP(hipMemsetAsync(S.f_cnt.p, 0, (size_t)nq * sizeof(uint32_t), st));
        CVTMI_TRY(launch_flat_u8_filter(q, nq, D, h->f_pack.as<uint4>(), h->norms.as<int32_t>(), sd, k, r0, r1, pair_cap, stats + 3,
                                        S.f_cand.as<uint4>(), st));
        CVTMI_TRY(launch_flat_u8_finish(nq, stats + 3, pair_cap, S.f_cand.as<uint4>(), cap, k, sd, si, S.f_cnt.as<uint32_t>(),
                                        S.f_seld.as<float>(), S.f_seli.as<int32_t>(), od, oi, stats + 2, st));
        CVTMI_HIP(hipMemcpyAsync(&worst, stats + 2, 4, hipMemcpyDeviceToHost, st));
        CVTMI_HIP(stream_wait(st));
        return CVTMI_OK;
    };
    // (a two-level sample -- exact kernels on ns / 8 rows, a first filter stage up to ns, as the fp32 path does -- was measured and lost:
    //  the second stage's launches and host sync cost more than the 1.2 ms of exact search they save; nq = 1000: 6.4 -> 7.0 ms)
    // The sample goes through the streaming kernel (128 queries per pass, ~0.12 ms per pass over 312 K rows) while that is cheaper than the
    // row-tile kernels' exact search of it (1.0-2.1 ms whatever the batch: every query block warms its thresholds up from scratch): up to
    // ten passes.  10 M x 512-d, k = 10 (tools/sweep_u8_sample.py, round 5): nq = 256 2.6 -> 1.6 ms, 384 / 512 3.9 -> 3.0, 640 / 768
    // 5.2 -> 4.5, 1000 6.3 -> 5.9-6.0, 1280 7.6 -> 7.4; equal at 1536, slower from 2048 on (16 passes 11.4 against 11.15 ms).
    CVTMI_TRY(flat_search_rows(h, S, ns, q, nq, k, S.f_sd.as<float>(), S.f_si.as<int64_t>(), st, tune_flat_u8_sample_passes.geti()));
    CVTMI_TRY(stage(ns, n, S.f_sd.as<float>(), S.f_si.as<int64_t>(), dist, rows));
    h->f_last_worst = (long long)worst;
    if (worst > (uint32_t)cap) return CVTMI_OK;
    *done = true;
    return CVTMI_OK;
}

// uint8 L2 as a threshold filter (flat_u8_tfilter.hip: batches, and every search with k > 128).  Queries it could not answer (sample not
// filled, list over, masses of ties at the k-th place; every query of a pass in which a wave's record region ran over) are re-run by the
// row-per-lane kernels under the flags as a predicate, their lists written over the filter's -- nothing on this path waits for the device.
// *done = false: not applicable (no operand copy / no room for the scratch): the round-5 paths answer the call
static int flat_search_bigk_u8(cvtmi_flat_t h, FlatScratch &S, const uint8_t *q, int64_t nq, int k, float *dist, int64_t *rows, hipStream_t st, bool *done)
{
    *done = false;
    const int64_t n = h->n;
    const int D = h->D;
    if (h->f_pack_n != n) return CVTMI_OK;   // no operand copy (flat_prepare could not build it)
    if (S.fs_scratch.reserve(flat_u8_tfilter_scratch(D, n, nq, k)) != CVTMI_OK) { (void)hipGetLastError(); return CVTMI_OK; }
    CVTMI_TRY(S.fs_redo.reserve((size_t)(nq + 1) * sizeof(uint32_t)));
    uint32_t *flags = S.fs_redo.as<uint32_t>();
    CVTMI_TRY(launch_flat_u8_tfilter(D, h->f_pack.p, h->norms.as<int32_t>(), n, q, nq, k, S.fs_scratch.p, dist, rows, flags, st));
    CVTMI_TRY(flat_count_redo(h, S, flags + 1, nq, st));
    CVTMI_TRY(flat_search_rows(h, S, n, q, nq, k, dist, rows, st, INT64_MAX, flags + 1));
    h->f_last_worst = 0;
    *done = true;
    return CVTMI_OK;
}

// which of the pipelines a search of nq queries takes (the dispatch rules, in one place: flat_prepare builds what they need)
struct FlatRoute { bool stream, tfilter, filt_f32, filt_u8, big_u8; };
// the tuning values a search dispatches on, read ONCE per call: flat_prepare and flat_search_leased must see the same route even if
// another thread calls cvtmi_set_tuning between the two
struct FlatTuning {
    int variant, f32_stream;
    static FlatTuning now() { return { tune_flat_variant.geti(), tune_flat_f32_stream.geti() }; }
};
static FlatRoute flat_route(const cvtmi_flat_s *h, const void *q, int64_t nq, int k, const FlatTuning &tun)
{
    FlatRoute r = { false, false, false, false, false };
    const bool aligned = ((uintptr_t)q & 15) == 0;
    // fp32: one stream over the rows (flat_f32_stream.hip).  flat_variant 2 asks for the older sample + filter pipeline, 1 for the exact kernels
    const bool f32_fast = ((tun.variant == 0 && tun.f32_stream == 1) || (tun.variant != 1 && tun.f32_stream == 2)) && aligned &&
                          h->fs_bias.p && h->fs_stats.p;
    r.stream = f32_fast && flat_f32_stream_applies(h->metric, h->D, h->n, k);
    r.tfilter = f32_fast && flat_f32_tfilter_applies(h->metric, h->D, h->n, nq, k);   // batches as a threshold filter (round 6), widths up to 512-d
    r.filt_f32 = tun.variant != 1 && aligned && nq <= 65535 &&
                 flat_filter_applies(h->metric, h->D, tun.variant == 2 ? std::max<int64_t>(h->n, 131072) : h->n,
                                     tun.variant == 2 ? std::max<int64_t>(nq, 16) : nq, k) && h->n >= 2 * 65536;
    // uint8: large batches go through the filter pipeline with the software-pipelined (LDS-DMA) kernel -- measured at 10 M x 512-d:
    // 4096 queries 27.4 -> 21.0 ms, 512 queries 4.6 -> 3.8 ms; smaller batches are one stream over the raw rows (flat_search_rows).
    // flat_variant 2 forces the pipeline wherever it applies, 1 forbids it.
    // (from 256 queries at every width: 10 M x 128-d nq = 256 / 512 / 1000 1.52 / 2.78 / 5.5 ms in streaming passes, 1.03 / 2.08 / 3.25 here;
    //  256-d nq = 256 1.87 against 1.26; between 257 and ~400 queries the two are within 5 %)
    // Round 5 (tools/sweep_u8_dispatch.py, profiles/r05_u8_dispatch_sweep.txt): once the pipeline's sample could go through the streaming
    // kernel on tables of any size (flat_search_filtered_u8: at least 262 144 sample rows) it beats the passes from ~1.3e11 row bytes x
    // queries on, at every width and table size measured (128 / 256 / 512-d, 0.6 .. 10 M rows, k = 10 / 64) -- 10 M x 512-d from 129
    // queries (2.2 -> 1.6 ms), 2 M x 512-d from 129 as well (256 queries: 1.47 ms under the old rule, which took the pipeline with a
    // row-tile sample, 0.49 now), 1 M x 128-d from ~1000; below that the two are within 5-20 % with the passes ahead.
    const bool u8_auto = tun.variant == 0 && flat_u8_gfilter_shape(h->D) && nq >= tune_flat_u8_filter_min_nq.geti() &&
                         h->n >= tune_flat_u8_filter_min_rows.get() && k <= 64 &&
                         (double)h->n * (double)h->D * (double)nq >= 1e9 * (double)tune_flat_u8_filter_min_work.get();
    r.filt_u8 = (tun.variant == 2 || u8_auto) && h->metric == CVTMI_METRIC_L2U8 && aligned && nq <= 65535 * 256 && h->norms.p &&
                flat_u8_filter_applies(h->D, std::max<int64_t>(h->n, 262144), std::max<int64_t>(nq, 256), k) && h->n >= 2 * 65536;
    // k > 128 (round 6, flat_u8_tfilter.hip): the stream and the pipeline above stop at 128 / 64 neighbours, the exact kernels behind them
    // take one query per workgroup (2 M x 512-d, 1000 queries: k = 128 3.9 ms, k = 129 139 ms)
    r.big_u8 = (tun.variant == 0 || (tun.variant == 2 && k > 128)) && h->metric == CVTMI_METRIC_L2U8 && aligned && h->norms.p && flat_u8_tfilter_applies(h->D, h->n, nq, k);
    return r;
}

// the grid rule of launch.h, for the CPU test that pins it (include/cvtmi.h)
// (a grid that passes is noted in the thread's launch log as launch() notes it, block 1 and no LDS: the log's CPU test needs no device)
extern "C" int cvtmi_describe_launch_grid(int64_t x, int64_t y, int64_t z)
{
    CVTMI_TRY(check_grid("cvtmi_describe_launch_grid", Grid(x, y, z)));
    log_launch("cvtmi_describe_launch_grid", Grid(x, y, z), 1, 0);
    return CVTMI_OK;
}

// which pipeline a flat search would take under the current tuning values, for inspection and for the CPU tests that pin the
// dispatch rules (include/cvtmi.h)
extern "C" int cvtmi_flat_describe_dispatch(int metric, int D, int64_t n_rows, int64_t nq, int k, int out[4])
{
    if (!out || metric < 0 || metric > 2 || D < 1 || n_rows < 0 || nq < 1 || k < 1) return fail(CVTMI_EINVAL, "cvtmi_flat_describe_dispatch: bad arguments");
    cvtmi_flat_s h;   // nothing of it touches a device; the buffers a route asks about count as present
    static char present[16];
    h.metric = metric; h.D = D; h.n = n_rows;
    h.fs_bias.p = present; h.fs_stats.p = present; h.norms.p = present;
    alignas(16) static const char aligned_q[16] = {};
    const FlatRoute r = flat_route(&h, aligned_q, nq, k, FlatTuning::now());
    h.fs_bias.p = nullptr; h.fs_stats.p = nullptr; h.norms.p = nullptr;
    out[0] = r.tfilter ? 2 : (r.stream ? 1 : 0);
    out[1] = r.filt_f32 ? 1 : 0;
    out[2] = r.big_u8 ? 2 : (r.filt_u8 ? 1 : 0);
    out[3] = (metric == CVTMI_METRIC_L2U8 && !r.filt_u8 && !r.big_u8 && flat_u8_mstream_applies(D, n_rows, std::min<int64_t>(nq, 128), k)) ? 1 : 0;
    return CVTMI_OK;
}

// how the uint8 stream's finish kernel would be cut for one pass of nq queries over n_rows rows, for the CPU test that pins the slice
// rule against the kernel's round tables (include/cvtmi.h)
extern "C" int cvtmi_flat_describe_stream_finish(int64_t n_rows, int64_t nq, int out[3])
{
    if (!out || n_rows < 1 || n_rows >= 0x7fffffff || nq < 1 || nq > 128) return fail(CVTMI_EINVAL, "cvtmi_flat_describe_stream_finish: bad arguments");
    int waves = 0;
    (void)flat_u8_mstream_scratch(n_rows, nq, nullptr, &waves);
    out[0] = flat_u8_stream_finish_plan(n_rows, nq, waves, &out[1], &out[2]);
    return CVTMI_OK;
}

// The row-major copy f_rows of blocked fp32 rows, brought up to the handle's n rows: only the rows appended since it was made are
// unblocked, the buffer grows by halves.  The caller holds the handle exclusively (FlatMutation on st); the stream is drained before
// the copy counts as current.  No room: CVTMI_OK with f_rows_failed set -- the readers gather from the blocked rows.  Shared by
// flat_prepare (the threshold filter's exact finish) and flat_rerank_prepare ("rerank_rows_copy")
static int flat_rows_copy_build(cvtmi_flat_t h, hipStream_t st)
{
    const int64_t n = h->n;
    int64_t row0 = (h->f_rows.p && h->f_rows_n > 0 && h->f_rows_n < n) ? h->f_rows_n : 0;
    h->f_rows_n = -1;
    const size_t need_b = (size_t)n * h->D * sizeof(float);
    bool ok = true;
    if (row0 > 0 && need_b > h->f_rows.cap &&
        h->f_rows.grow(std::max(need_b, h->f_rows.cap + h->f_rows.cap / 2), (size_t)row0 * h->D * sizeof(float), st) != CVTMI_OK) { (void)hipGetLastError(); row0 = 0; }
    if (row0 == 0 && h->f_rows.reserve(need_b) != CVTMI_OK) { (void)hipGetLastError(); ok = false; h->f_rows_failed = true; }   // no room: the finish gathers from the blocked rows
    if (ok) {
        CVTMI_TRY(launch_flat_unblock(h->data.as<float>(), row0, n, h->D, h->f_rows.as<float>(), st));
        CVTMI_HIP(stream_wait(st));
        h->f_rows_n = n;
    }
    return CVTMI_OK;
}

// The lazily built parts of the index a route needs -- the host copy of the row statistics (fp32 stream), the operand copies of
// the filter pipelines -- are built under the EXCLUSIVE lock, once per index state, and the stream is drained before the lock
// is given back.  Called before the search takes its shared lock.
static int flat_prepare(cvtmi_flat_t h, const void *q, int64_t nq, int k, hipStream_t st, const FlatTuning &tun)
{
    for (int attempt = 0; attempt < 2; ++attempt) {
        FlatRoute r;
        bool need_fs, need_f32, need_u8, need_rm;
        int want_nch = 0;
        {
            std::shared_lock<std::shared_timed_mutex> rd(h->rw);
            r = flat_route(h, q, nq, k, tun);
            need_fs = (r.stream || r.tfilter) && h->fs_stats_n != h->n;
            // the threshold filter reads the copy, and so do the stream kernels for small batches on tables of its size
            const bool tf = (r.tfilter || (r.stream && h->D % 16 == 0 && flat_f32_tfilter_nch(h->D) == h->D / 16 && h->n >= tune_flat_f32_tfilter_min_rows.get())) &&
                            !h->fs_nonfinite;
            want_nch = tf ? flat_f32_tfilter_nch(h->D) : h->D / 16;
            need_f32 = (h->f_pack_n != h->n || h->f_pack_nch != want_nch) &&
                       (tf ? !need_fs : (r.filt_f32 && !(r.stream && !need_fs && !h->fs_nonfinite)));   // (the stream answers: no copy needed)
            need_u8 = (r.filt_u8 || r.big_u8) && h->f_pack_n != h->n;
            const int rows_copy = tune_flat_f32_rows_copy.geti();
            need_rm = tf && rows_copy != 0 && h->D >= rows_copy && h->D % 4 == 0 && h->f_rows_n != h->n &&
                      !h->f_rows_failed;
            if (!need_fs && !need_f32 && !need_u8 && !need_rm) return CVTMI_OK;
        }
        FlatMutation mut(h, st);
        const int64_t n = h->n;
        if (need_fs && h->fs_stats_n != n) {   // once per index state: do the rows hold non-finite values?
            uint32_t stats[2] = { 0, 0 };
            CVTMI_HIP(hipMemcpyAsync(stats, h->fs_stats.p, sizeof stats, hipMemcpyDeviceToHost, st));
            CVTMI_HIP(stream_wait(st));
            h->fs_nonfinite = stats[1] != 0;
            h->fs_stats_n = n;
            continue;   // the route may not need an operand copy after all
        }
        if (need_f32 && (h->f_pack_n != n || h->f_pack_nch != want_nch)) {   // bf16 operand copy of the rows (same bytes as the fp32 rows)
            // rows appended since the copy was made (the reference adds video by video): only those are packed, the buffers grow by halves
            int64_t row0 = (h->f_pack.p && h->f_bias.p && h->f_istats.p && h->f_pack_nch == want_nch && h->f_pack_n > 0 && h->f_pack_n < n) ? h->f_pack_n : 0;
            h->f_pack_n = -1;
            const size_t need_p = flat_pack_bytes(want_nch, n), need_b = (size_t)((n + 31) / 32) * 32 * sizeof(uint32_t);
            if (row0 > 0) {
                const size_t keep_p = flat_pack_bytes(want_nch, row0), keep_b = (size_t)((row0 + 31) / 32) * 32 * sizeof(uint32_t);
                if (need_p > h->f_pack.cap && h->f_pack.grow(std::max(need_p, h->f_pack.cap + h->f_pack.cap / 2), keep_p, st) != CVTMI_OK) { (void)hipGetLastError(); row0 = 0; }
                if (row0 > 0 && need_b > h->f_bias.cap) CVTMI_TRY(h->f_bias.grow(std::max(need_b, h->f_bias.cap + h->f_bias.cap / 2), keep_b, st));
            }
            if (row0 == 0) {
                if (h->f_pack.reserve(need_p) != CVTMI_OK) return CVTMI_OK;   // no room: the exact path answers
                CVTMI_TRY(h->f_bias.reserve(need_b));
                CVTMI_TRY(h->f_istats.reserve(16));
            }
            CVTMI_TRY(launch_flat_pack(h->data.as<float>(), n, h->D, want_nch, h->metric, h->f_pack.as<uint4>(), h->f_bias.as<uint32_t>(),
                                       h->f_istats.as<uint32_t>(), st, row0));
            uint32_t stats[2] = { 0, 0 };
            CVTMI_HIP(hipMemcpyAsync(stats, h->f_istats.p, sizeof stats, hipMemcpyDeviceToHost, st));
            CVTMI_HIP(stream_wait(st));
            h->f_nonfinite = stats[1] != 0 || !(__builtin_bit_cast(float, stats[0]) <= 3.0e38f);
            h->f_pack_n = n;
            h->f_pack_nch = want_nch;
        }
        if (need_rm && h->f_rows_n != n && !need_fs) CVTMI_TRY(flat_rows_copy_build(h, st));
        if (need_u8 && h->f_pack_n != n) {    // operand-ordered copy of the rows (x - 128 as int8)
            // rows appended since the copy was made: only their tiles are packed (from the last, partly filled one on), the buffer grows by halves
            int64_t row0 = (h->f_pack.p && h->f_pack_n > 0 && h->f_pack_n < n) ? h->f_pack_n / 32 * 32 : 0;
            h->f_pack_n = -1;
            const size_t need_p = flat_u8_pack_bytes(h->D, n);
            if (row0 > 0 && need_p > h->f_pack.cap &&
                h->f_pack.grow(std::max(need_p, h->f_pack.cap + h->f_pack.cap / 2), flat_u8_pack_bytes(h->D, row0), st) != CVTMI_OK) { (void)hipGetLastError(); row0 = 0; }
            if (row0 == 0 && h->f_pack.reserve(need_p) != CVTMI_OK) return CVTMI_OK;
            CVTMI_TRY(launch_flat_u8_pack(h->data.as<uint8_t>(), n, h->D, h->f_pack.as<uint4>(), st, row0));
            CVTMI_HIP(stream_wait(st));
            h->f_pack_n = n;
        }
        return CVTMI_OK;
    }
    return CVTMI_OK;
}

// the search proper, on a leased scratch set, under the shared lock
static int flat_search_leased(cvtmi_flat_t h, FlatScratch &S, const void *q, int64_t nq, int k, void *dist, int64_t *labels, hipStream_t st,
                              const FlatTuning &tun)
{
    bool done = false;
    long long worst0 = 0;
    h->f_last_worst = worst0;
    h->f_last_redo = tune_flat_count_redo.geti() ? 0 : -1;   // (the routes with redo flags overwrite it)
    int how = 0;
    const FlatRoute r = flat_route(h, q, nq, k, tun);
    if (r.stream || r.tfilter) {
        int how_s = 2;
        CVTMI_TRY(flat_search_streamed(h, S, reinterpret_cast<const float *>(q), nq, k, reinterpret_cast<float *>(dist), labels, st, &done, &how_s));
        if (done) how = how_s;
    }
    if (!done && r.filt_f32)
        CVTMI_TRY(flat_search_filtered(h, S, reinterpret_cast<const float *>(q), nq, k, reinterpret_cast<float *>(dist), labels, st, &done));
    if (!done && r.big_u8) {
        CVTMI_TRY(flat_search_bigk_u8(h, S, reinterpret_cast<const uint8_t *>(q), nq, k, reinterpret_cast<float *>(dist), labels, st, &done));
        if (done) how = 4;
    }
    if (!done && r.filt_u8)
        CVTMI_TRY(flat_search_filtered_u8(h, S, reinterpret_cast<const uint8_t *>(q), nq, k, reinterpret_cast<float *>(dist), labels, st, &done));
    h->f_last_filtered = done ? (how ? how : 1) : 0;
    if (!done) CVTMI_TRY(flat_search_rows(h, S, h->n, q, nq, k, reinterpret_cast<float *>(dist), labels, st));
    if (!h->identity) CVTMI_TRY(launch_gather_labels(labels, nq * k, h->labels.as<int64_t>(), st));
    else if (h->id_base != 0) CVTMI_TRY(launch_offset_labels(labels, nq * k, h->id_base, st));
    return CVTMI_OK;
}

int cvtmi_flat_search_dev(cvtmi_flat_t h, const void *q, int64_t nq, int k, void *dist, int64_t *labels, void *stream)
{
    CHECK_H(h);
    if (nq < 0 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_flat_search: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_search: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (nq == 0) return CVTMI_OK;
    hipStream_t st = (hipStream_t)stream;
    const FlatTuning tun = FlatTuning::now();
    CVTMI_TRY(flat_prepare(h, q, nq, k, st, tun));
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    FlatLease lease;
    CVTMI_TRY(lease.open(h, st, false));
    return flat_search_leased(h, *lease.s, q, nq, k, dist, labels, st, tun);
}

// ---- range search: every row under a distance radius (flat_range.hip) ----
// A search like the others: `rw` shared, a leased scratch set, nothing of the handle changes.  A call is a count (scan, offsets: lims
// is complete on the device) and, where the caller gave room, a fill (fill + rescan, both predicated on the device on
// lims[nq] <= cap).
struct FlatRangeCall {
    FlatRangePlan plan;
    FlatRangeBufs bufs;
    FlatRangeRows rows;
    uint32_t thr = 0;
    int64_t *lims_scratch = nullptr;   // nq + 1 words behind the carved areas (the host entry's device lims)
};

// the radius as the kernels compare against it: fp32 the smallest float t >= radius (d < t in fp32 is d < radius in real numbers),
// uint8 T = ceil(radius) in [0, 2^31] (2^31: every row -- no distance reaches it)
static uint32_t flat_range_threshold(int metric, double radius)
{
    if (metric == CVTMI_METRIC_L2U8) {
        if (!(radius > 0.0)) return 0u;
        if (radius >= 2147483648.0) return 0x80000000u;
        return (uint32_t)std::min(ceil(radius), 2147483647.0);
    }
    float t;
    if (radius > (double)FLT_MAX) t = INFINITY;
    else if (radius < -(double)FLT_MAX) t = radius == -(double)INFINITY ? -INFINITY : -FLT_MAX;
    else {
        t = (float)radius;
        if ((double)t < radius) t = nextafterf(t, INFINITY);
    }
    return __builtin_bit_cast(uint32_t, t);
}

// arguments first, before anything touches the device
static int flat_range_check(cvtmi_flat_t h, const void *q, int64_t nq, double radius, int64_t cap, const int64_t *lims, const void *dist,
                            const int64_t *labels)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_flat_range_search: null handle");
    if (!q || !lims || nq < 0 || cap < 0) return fail(CVTMI_EINVAL, "cvtmi_flat_range_search: bad arguments");
    if (cap > 0 && (!dist || !labels)) return fail(CVTMI_EINVAL, "cvtmi_flat_range_search: cap=%lld without result arrays", (long long)cap);
    if (radius != radius) return fail(CVTMI_EINVAL, "cvtmi_flat_range_search: the radius is NaN");
    if (nq > INT32_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_range_search: nq=%lld above 2^31-1", (long long)nq);
    return CVTMI_OK;
}

// plan and scratch (all of it, before the first kernel), then the count.  The caller holds `rw` shared and the lease; h->n > 0, nq > 0
static int flat_range_count_leased(cvtmi_flat_t h, FlatScratch &S, const void *q, int64_t nq, double radius, bool spill, int64_t *lims,
                                   FlatRangeCall &c, hipStream_t st)
{
    const bool has_norms = h->metric == CVTMI_METRIC_L2U8 && h->D % 32 == 0 && h->D <= 512 && h->norms.p;   // (as flat_add_common keeps them)
    c.plan = plan_flat_range(h->metric, h->D, has_norms, h->n, nq, h->p_range_part_rows, spill ? h->p_range_spill : 0);
    c.thr = flat_range_threshold(h->metric, radius);
    c.rows.metric = h->metric; c.rows.D = h->D; c.rows.data = h->data.p; c.rows.norms = has_norms ? h->norms.as<int32_t>() : nullptr;
    c.rows.n = h->n; c.rows.labels = h->identity ? nullptr : h->labels.as<int64_t>(); c.rows.id_base = h->id_base;
    const size_t carved = flat_range_carve(nullptr, c.plan, nq, nullptr);
    CVTMI_TRY(S.s_range.reserve(carved + ((size_t)nq + 1) * sizeof(int64_t)));
    flat_range_carve(S.s_range.p, c.plan, nq, &c.bufs);
    c.lims_scratch = reinterpret_cast<int64_t *>(S.s_range.as<char>() + carved);
    {
        std::lock_guard<std::mutex> g(h->pool.mu);
        const int64_t v[6] = { c.plan.qt, c.plan.parts, c.plan.rows_per_part, c.plan.spill, (int64_t)c.plan.spill_bytes, c.plan.form };
        for (int i = 0; i < 6; ++i) h->range_last[i] = v[i];
    }
    return launch_flat_range_count(c.rows, q, nq, c.thr, c.plan, c.bufs, lims ? lims : c.lims_scratch, st);
}

int cvtmi_flat_range_search_dev(cvtmi_flat_t h, const void *q, int64_t nq, double radius, int64_t cap, int64_t *lims, void *dist, int64_t *labels,
                                void *stream)
{
    CVTMI_TRY(flat_range_check(h, q, nq, radius, cap, lims, dist, labels));
    CVTMI_TRY(use_device(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (nq == 0) {
        CVTMI_HIP(hipMemsetAsync(lims, 0, sizeof(int64_t), st));
        return CVTMI_OK;
    }
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    FlatLease lease;
    CVTMI_TRY(lease.open(h, st, false));
    if (h->n == 0) {   // an empty index: no hits
        CVTMI_HIP(hipMemsetAsync(lims, 0, ((size_t)nq + 1) * sizeof(int64_t), st));
        return CVTMI_OK;
    }
    FlatRangeCall c;
    CVTMI_TRY(flat_range_count_leased(h, *lease.s, q, nq, radius, cap > 0, lims, c, st));
    if (cap == 0) return CVTMI_OK;   // a count-only call
    return launch_flat_range_fill(c.rows, q, nq, c.thr, c.plan, c.bufs, lims, cap, dist, labels, st);
}

// host pointers: the queries go up and lims comes back through the leased set's staging buffers -- the one wait the call needs to
// know whether the result fits; then the two arrays, sized by lims[nq]
int cvtmi_flat_range_search(cvtmi_flat_t h, const void *q, int64_t nq, double radius, int64_t cap, int64_t *lims, void *dist, int64_t *labels)
{
    CVTMI_TRY(flat_range_check(h, q, nq, radius, cap, lims, dist, labels));
    CVTMI_TRY(use_device(h->device));
    lims[0] = 0;
    if (nq == 0) return CVTMI_OK;
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    if (h->n == 0) {   // an empty index: no hits
        memset(lims, 0, ((size_t)nq + 1) * sizeof(int64_t));
        return CVTMI_OK;
    }
    FlatLease lease;
    CVTMI_TRY(lease.open(h, nullptr, true));
    FlatScratch &S = *lease.s;
    hipStream_t st = lease.st;
    const size_t qb = (size_t)nq * h->row_bytes;
    CVTMI_TRY(S.io_q.reserve(qb));
    CVTMI_HIP(hipMemcpyAsync(S.io_q.p, q, qb, hipMemcpyHostToDevice, st));
    FlatRangeCall c;
    CVTMI_TRY(flat_range_count_leased(h, S, S.io_q.p, nq, radius, cap > 0, nullptr, c, st));
    const RangeOut outs[] = { { dist, &S.io_d, 4 }, { labels, &S.io_i, sizeof(int64_t) } };
    return range_host_finish("cvtmi_flat_range_search", nq, cap, lims, c.lims_scratch, outs, st, [&](int64_t total) {
        return launch_flat_range_fill(c.rows, S.io_q.p, nq, c.thr, c.plan, c.bufs, c.lims_scratch, total, S.io_d.p, S.io_i.as<int64_t>(), st);
    });
}

int cvtmi_flat_last_range_plan(cvtmi_flat_t h, int64_t out[6])
{
    if (!h || !out) return fail(CVTMI_EINVAL, "cvtmi_flat_last_range_plan: null");
    copy_last(h->pool, h->range_last, out);
    return CVTMI_OK;
}

int cvtmi_flat_set_id_base(cvtmi_flat_t h, int64_t base)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_flat_set_id_base: null");
    h->id_base = base;
    return CVTMI_OK;
}

// row-sharded exhaustive search (the flat twin of cvtmi_opq_search_sharded_dev): local search into the communicator's slot,
// one all-gather, merge.  uint8 L2: the int32 distances travel and merge as their bit patterns (shard.hip).
int cvtmi_flat_search_sharded_dev(cvtmi_flat_t h, cvtmi_comm_t c, const void *q, int64_t nq, int k, void *dist, int64_t *labels, void *stream)
{
    CVTMI_TRY(comm_validate(c));
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded: null handle");
    if (nq < 0 || (nq > 0 && (!dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_search_sharded: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (nq == 0) return CVTMI_OK;
    Serial serial_c(*comm_sync(c), (hipStream_t)stream);
    CHECK_H(h);
    if (comm_world(c) == 1 && !comm_has_transport(c)) return cvtmi_flat_search_dev(h, q, nq, k, dist, labels, stream);
    int rc = comm_device(c) != h->device ? fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded: handle and communicator live on different devices") : CVTMI_OK;
    float *sd = nullptr;
    int64_t *si = nullptr;
    if (rc == CVTMI_OK) rc = !q ? fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded: null queries") : sharded_local_failure(c);
    if (rc == CVTMI_OK) rc = comm_local_slot(c, nq, k, &sd, &si);
    if (rc == CVTMI_OK) rc = cvtmi_flat_search_dev(h, q, nq, k, sd, si, stream);
    return comm_exchange_merge(c, nq, k, rc, reinterpret_cast<float *>(dist), labels, (hipStream_t)stream);
}

int cvtmi_flat_search_sharded(cvtmi_flat_t h, cvtmi_comm_t c, const void *q, int64_t nq, int k, void *dist, int64_t *labels)
{
    CVTMI_TRY(comm_validate(c));
    CHECK_H(h);
    if (nq < 0 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_search_sharded: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (nq == 0) return CVTMI_OK;
    Tmp dq, dd, di;
    CVTMI_TRY(dq.upload(q, (size_t)nq * h->row_bytes));
    CVTMI_TRY(dd.alloc((size_t)nq * k * 4));
    CVTMI_TRY(di.alloc((size_t)nq * k * 8));
    CVTMI_TRY(cvtmi_flat_search_sharded_dev(h, c, dq.p, nq, k, dd.p, di.as<int64_t>(), nullptr));
    CVTMI_HIP(hipMemcpy(dist, dd.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(labels, di.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    {   // (as in cvtmi_opq_search_sharded)
        Serial serial_c(*comm_sync(c), nullptr);
        CVTMI_TRY(comm_take_deferred(c));
    }
    return CVTMI_OK;
}

int cvtmi_flat_search_sharded_all(cvtmi_flat_t *handles, cvtmi_comm_t *comms, int ndev, const void *q, int64_t nq, int k, void *dist,
                                  int64_t *labels)
{
    if (!handles || !comms || ndev < 1) return fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded_all: bad arguments");
    if (nq < 0 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded_all: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_search_sharded_all: k=%d outside 1..%d", k, CVTMI_K_MAX);
    std::vector<int> devices(ndev);
    for (int d = 0; d < ndev; ++d) {
        CVTMI_TRY(comm_validate(comms[d]));
        if (!handles[d]) return fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded_all: null handle %d", d);
        if (comm_world(comms[d]) != ndev || comm_rank(comms[d]) != d || comm_device(comms[d]) != handles[d]->device)
            return fail(CVTMI_EINVAL, "cvtmi_flat_search_sharded_all: communicator %d does not belong to handle %d", d, d);
        devices[d] = handles[d]->device;
    }
    if (nq == 0) return CVTMI_OK;
    return sharded_all(comms, ndev, q, (size_t)nq * handles[0]->row_bytes, nq, k, dist, labels, devices.data(),
                       [&](int d, const void *qd, float *sd, int64_t *si) { return cvtmi_flat_search_dev(handles[d], qd, nq, k, sd, si, nullptr); });
}

int cvtmi_flat_last_search(cvtmi_flat_t h, int *filtered, int64_t *max_candidates)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_flat_last_search: null handle");
    if (filtered) *filtered = h->f_last_filtered;
    if (max_candidates) *max_candidates = h->f_last_worst;
    return CVTMI_OK;
}

int cvtmi_flat_last_redo(cvtmi_flat_t h, int64_t *redone)
{
    if (!h || !redone) return fail(CVTMI_EINVAL, "cvtmi_flat_last_redo: null argument");
    *redone = h->f_last_redo;
    return CVTMI_OK;
}

// host pointers in and out.  Every call runs on the stream of its own scratch set (staging buffers included), so callers on
// several threads -- the reference's searchKnn is a pure read, brutoforce.hpp:73-93 -- proceed side by side.
int cvtmi_flat_search(cvtmi_flat_t h, const void *q, int64_t nq, int k, void *dist, int64_t *labels)
{
    CHECK_H(h);
    if (nq < 0 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_flat_search: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_search: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (nq == 0) return CVTMI_OK;
    alignas(16) static const char aligned_probe[16] = {};
    const FlatTuning tun = FlatTuning::now();
    CVTMI_TRY(flat_prepare(h, aligned_probe, nq, k, nullptr, tun));   // (the staged queries are 16-byte aligned)
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    FlatLease lease;
    CVTMI_TRY(lease.open(h, nullptr, true));
    FlatScratch &S = *lease.s;
    hipStream_t st = lease.st;
    CVTMI_TRY(S.io_q.reserve((size_t)nq * h->row_bytes));
    // Small calls (the brute_force CLI's shape, one searchKnn per query: brute_force_search/src/brute_force.cpp:86): the three copies
    // are a tenth of such a call.  The queries go up from a page-locked staging area (a truly asynchronous copy), and the last kernel of
    // the search writes the lists straight into that area (device-visible host memory) -- no copy engine on the way back.
    const size_t qn = (size_t)nq * h->row_bytes, dn = (size_t)nq * k * 4, in = (size_t)nq * k * 8;
    if (tune_flat_small_zero_copy.geti() && qn <= ((size_t)64 << 10) && dn + in <= ((size_t)768 << 10)) {
        const size_t qoff = (qn + 255) & ~(size_t)255, doff = (dn + 255) & ~(size_t)255;
        CVTMI_TRY(S.io_pin.reserve(std::max(qoff + doff + in, (size_t)1 << 20)));
        void *pin_dev = nullptr;
        if (hipHostGetDevicePointer(&pin_dev, S.io_pin.p, 0) == hipSuccess && pin_dev) {
            char *pin = S.io_pin.as<char>(), *pd = static_cast<char *>(pin_dev);
            memcpy(pin, q, qn);
            CVTMI_HIP(hipMemcpyAsync(S.io_q.p, pin, qn, hipMemcpyHostToDevice, st));
            CVTMI_TRY(flat_search_leased(h, S, S.io_q.p, nq, k, pd + qoff, reinterpret_cast<int64_t *>(pd + qoff + doff), st, tun));
            CVTMI_HIP(stream_wait(st));
            memcpy(dist, pin + qoff, dn);
            memcpy(labels, pin + qoff + doff, in);
            return CVTMI_OK;
        }
        (void)hipGetLastError();
    }
    CVTMI_TRY(S.io_d.reserve((size_t)nq * k * 4));
    CVTMI_TRY(S.io_i.reserve((size_t)nq * k * 8));
    CVTMI_HIP(hipMemcpyAsync(S.io_q.p, q, (size_t)nq * h->row_bytes, hipMemcpyHostToDevice, st));
    CVTMI_TRY(flat_search_leased(h, S, S.io_q.p, nq, k, S.io_d.p, S.io_i.as<int64_t>(), st, tun));
    CVTMI_HIP(hipMemcpyAsync(dist, S.io_d.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(hipMemcpyAsync(labels, S.io_i.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    return CVTMI_OK;
}

}  // extern "C"

// ---- rerank: the exact top k among the candidate rows the caller names (flat_rerank.hip) ----
// A search like the others: `rw` shared, a leased scratch set, nothing of the handle changes -- but for "rerank_rows_copy" = 1, where
// the first call that finds no current row-major copy of blocked rows builds it under the exclusive lock first, as flat_prepare does.
static int flat_rerank_prepare(cvtmi_flat_t h, hipStream_t st)
{
    {
        std::shared_lock<std::shared_timed_mutex> rd(h->rw);
        if (!h->p_rerank_rows_copy || !flat_blocked(h->metric, h->D) || h->n == 0 || h->f_rows_n == h->n || h->f_rows_failed) return CVTMI_OK;
    }
    FlatMutation mut(h, st);
    if (h->n > 0 && h->f_rows_n != h->n && !h->f_rows_failed) CVTMI_TRY(flat_rows_copy_build(h, st));
    return CVTMI_OK;
}

// arguments first, before anything touches the device
static int flat_rerank_check(cvtmi_flat_t h, const void *q, int64_t nq, const int64_t *cand, int R, int k, const void *dist, const int64_t *labels)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_flat_rerank: null handle");
    if (nq < 0 || (nq > 0 && (!q || !cand || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_flat_rerank: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EINVAL, "cvtmi_flat_rerank: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (R < 1 || R > CVTMI_RERANK_MAX) return fail(CVTMI_EINVAL, "cvtmi_flat_rerank: R=%d outside 1..%d", R, CVTMI_RERANK_MAX);
    return CVTMI_OK;
}

// the launch, on a leased scratch set's stream or the caller's, under the shared lock
static int flat_rerank_leased(cvtmi_flat_t h, const void *q, int64_t nq, const int64_t *cand, int R, int64_t cand_base, bool skip_minus_one, int k,
                              void *dist, int64_t *labels, hipStream_t st)
{
    if (h->n >= ((int64_t)1 << 32)) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_rerank: %lld rows: rows travel as 32-bit words", (long long)h->n);
    const bool blocked = flat_blocked(h->metric, h->D);
    const bool copy = blocked && h->f_rows.p && h->f_rows_n == h->n;   // (a stale copy -- rows added since -- is not read)
    const int src = !blocked ? 0 : (copy ? 2 : 1);
    int64_t info[4];
    CVTMI_TRY(launch_flat_rerank(h->metric, h->D, copy ? h->f_rows.p : h->data.p, src, h->n, h->identity ? nullptr : h->labels.as<int64_t>(), h->id_base, q, nq, cand,
                                 R, cand_base, skip_minus_one, k, dist, labels, info, st));
    std::lock_guard<std::mutex> g(h->pool.mu);
    for (int i = 0; i < 4; ++i) h->rerank_last[i] = info[i];
    return CVTMI_OK;
}

int cvtmi::flat_rerank_on_stream(cvtmi_flat_t h, const void *q, int64_t nq, const int64_t *cand, int R, int64_t cand_base, bool skip_minus_one, int k,
                                 void *dist, int64_t *labels, hipStream_t st)
{
    CVTMI_TRY(flat_rerank_prepare(h, st));
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    FlatLease lease;
    CVTMI_TRY(lease.open(h, st, false));
    return flat_rerank_leased(h, q, nq, cand, R, cand_base, skip_minus_one, k, dist, labels, st);
}

extern "C" {

int cvtmi_flat_rerank_dev(cvtmi_flat_t h, const void *q, int64_t nq, const int64_t *cand, int R, int64_t cand_base, int k, void *dist,
                          int64_t *labels, void *stream)
{
    CVTMI_TRY(flat_rerank_check(h, q, nq, cand, R, k, dist, labels));
    CVTMI_TRY(use_device(h->device));
    if (nq == 0) return CVTMI_OK;
    return flat_rerank_on_stream(h, q, nq, cand, R, cand_base, false, k, dist, labels, (hipStream_t)stream);
}

// host pointers: queries and candidate lists up, the two result arrays down, through the leased set's staging buffers and its stream
int cvtmi_flat_rerank(cvtmi_flat_t h, const void *q, int64_t nq, const int64_t *cand, int R, int64_t cand_base, int k, void *dist, int64_t *labels)
{
    CVTMI_TRY(flat_rerank_check(h, q, nq, cand, R, k, dist, labels));
    CVTMI_TRY(use_device(h->device));
    if (nq == 0) return CVTMI_OK;
    CVTMI_TRY(flat_rerank_prepare(h, nullptr));
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    FlatLease lease;
    CVTMI_TRY(lease.open(h, nullptr, true));
    return host_call(lease, q, (size_t)nq * h->row_bytes, HostUpload{ &lease.s->io_c, cand, (size_t)nq * R * sizeof(int64_t) }, dist, (size_t)nq * k * 4, labels,
                     (size_t)nq * k * sizeof(int64_t), [&](FlatScratch &, const void *dq, const void *dc, void *dd, int64_t *dl, hipStream_t st) {
                         return flat_rerank_leased(h, dq, nq, static_cast<const int64_t *>(dc), R, cand_base, false, k, dd, dl, st);
                     });
}

int cvtmi_flat_last_rerank(cvtmi_flat_t h, int64_t out[4])
{
    if (!h || !out) return fail(CVTMI_EINVAL, "cvtmi_flat_last_rerank: null");
    copy_last(h->pool, h->rerank_last, out);
    return CVTMI_OK;
}

}  // extern "C"

// ---- masked search: the k nearest rows among those a bitmap allows (flat_masked.hip) ----
// A search like the others: `rw` shared, a leased scratch set, nothing of the handle changes.  The mask becomes a row list in the
// leased set, the exact kernels walk the list, the parts merge, rows become labels; nothing of it reaches the host.
static int flat_masked_check(cvtmi_flat_t h, const void *q, int64_t nq, int k, const uint64_t *mask, int64_t mask_words, const void *dist,
                             const int64_t *labels)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_flat_search_masked: null handle");
    if (nq < 0 || mask_words < 0 || (nq > 0 && (!q || !mask || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_flat_search_masked: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EINVAL, "cvtmi_flat_search_masked: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (nq > INT32_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_flat_search_masked: nq=%lld above 2^31-1", (long long)nq);
    return CVTMI_OK;
}

// under the shared lock: the mask covers the rows there are now
static int flat_mask_covers(cvtmi_flat_t h, int64_t mask_words, const char *who)
{
    if (h->n >= ((int64_t)1 << 32)) return fail(CVTMI_EUNSUPPORTED, "%s: %lld rows: rows travel as 32-bit words", who, (long long)h->n);
    if (mask_words < (h->n + 63) / 64)
        return fail(CVTMI_EINVAL, "%s: %lld mask words for %lld rows (%lld needed)", who, (long long)mask_words, (long long)h->n, (long long)((h->n + 63) / 64));
    return CVTMI_OK;
}

// the launches, on a leased scratch set, under the shared lock; h->n > 0, nq > 0; all pointers are device pointers
static int flat_masked_leased(cvtmi_flat_t h, FlatScratch &S, const void *q, int64_t nq, int k, const uint64_t *mask, void *dist, int64_t *labels,
                              hipStream_t st)
{
    const int64_t n = h->n;
    const int qt = k > 128 ? 1 : flat_qtile(nq);   // k > 128: one query per workgroup (kernels.h: kBigK)
    // planned for the worst case, a mask that allows every row: the host never learns how many it allows
    int parts = h->p_masked_parts ? (int)h->p_masked_parts : flat_plan_splits(n, nq, qt);
    const int64_t room = std::max<int64_t>(1, (int64_t)(1LL << 30) / std::max<int64_t>(1, nq * (int64_t)k * 12));   // at most ~1 GB of partial lists
    if (parts > room) parts = (int)room;
    const RmPlan p = rm_plan(n, 0, 0, 0);
    const size_t off_list = p.off_table, list_bytes = (size_t)n * sizeof(uint32_t);   // (nothing of the plan behind its scan areas is used)
    CVTMI_TRY(S.s_masked.reserve(off_list + list_bytes));
    float *pd = reinterpret_cast<float *>(dist);
    int64_t *pi = labels;
    if (parts > 1) {
        const size_t cnt = (size_t)nq * parts * k;
        CVTMI_TRY(S.s_part_d.reserve(cnt * sizeof(float)));
        CVTMI_TRY(S.s_part_id.reserve(cnt * sizeof(int64_t)));
        pd = S.s_part_d.as<float>();
        pi = S.s_part_id.as<int64_t>();
    }
    {
        std::lock_guard<std::mutex> g(h->pool.mu);
        const int64_t v[4] = { qt, parts, (int64_t)list_bytes, flat_masked_form(h->metric, h->D) };
        for (int i = 0; i < 4; ++i) h->masked_last[i] = v[i];
    }
    uint32_t *list = rm_at<uint32_t>(S.s_masked.p, off_list);
    CVTMI_TRY(launch_flat_masked_list(p, S.s_masked.p, mask, list, st));
    CVTMI_TRY(launch_flat_masked_search(h->metric, h->D, h->data.p, n, q, nq, k, qt, parts, list, rm_at<int64_t>(S.s_masked.p, p.off_total), pd, pi, st));
    if (parts > 1) CVTMI_TRY(launch_topk_merge(pd, pi, nq, parts, k, reinterpret_cast<float *>(dist), labels, st));
    if (!h->identity) CVTMI_TRY(launch_gather_labels(labels, nq * k, h->labels.as<int64_t>(), st));
    else if (h->id_base != 0) CVTMI_TRY(launch_offset_labels(labels, nq * k, h->id_base, st));
    return CVTMI_OK;
}

// ---- the bitmap of a label set: the mark step of the removal, on a leased scratch set (the handle does not change) ----
static int flat_mask_labels_check(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, const uint64_t *mask, int64_t mask_words)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_flat_mask_labels: null handle");
    if (n_labels < 0 || mask_words < 0 || (n_labels > 0 && !labels) || (mask_words > 0 && !mask)) return fail(CVTMI_EINVAL, "cvtmi_flat_mask_labels: bad arguments");
    return CVTMI_OK;
}

// set_dev: the labels on the device (implicit labels); table: their distinct values, ascending, in host memory (explicit labels).
// Under the shared lock; mask is a device pointer of mask_words words
static int flat_mask_labels_leased(cvtmi_flat_t h, FlatScratch &S, const int64_t *set_dev, int64_t n_set, const int64_t *table, int64_t T, uint64_t *mask,
                                   int64_t mask_words, hipStream_t st)
{
    if (mask_words == 0) return CVTMI_OK;
    if (h->n == 0 || n_set == 0) {
        CVTMI_HIP(hipMemsetAsync(mask, 0, (size_t)mask_words * 8, st));
        return CVTMI_OK;
    }
    if (!h->identity) return labels_to_mask(S.s_masked, h->labels.as<int64_t>(), h->n, table, T, mask, mask_words, st);
    const RmPlan p = rm_plan(h->n, 0, 0, 0);   // the mark's areas alone: no row moves, so no chunk scratch
    CVTMI_TRY(S.s_masked.reserve(p.off_table + rm_align(8)));
    CVTMI_TRY(launch_rm_mark_ids(p, S.s_masked.p, set_dev, n_set, h->id_base, st));
    return launch_flat_masked_copy(p, S.s_masked.p, mask, mask_words, st);
}

int cvtmi::labels_to_mask(DevBuf &W, const int64_t *labels_dev, int64_t n, const int64_t *table, int64_t T, uint64_t *mask, int64_t mask_words, hipStream_t st)
{
    FlatRmPlan p;   // the mark's areas and the table alone: nothing moves
    p.rm = rm_plan(n, 0, 0, 0);
    p.T = T;
    p.off_table = p.rm.off_table;
    p.bytes = p.off_table + rm_align((size_t)T * 8);
    CVTMI_TRY(W.reserve(p.bytes));
    CVTMI_HIP(hipMemcpyAsync(rm_at<char>(W.p, p.off_table), table, (size_t)T * 8, hipMemcpyHostToDevice, st));
    CVTMI_TRY(launch_flat_rm_mark_labels(p, W.p, labels_dev, st));
    return launch_flat_masked_copy(p.rm, W.p, mask, mask_words, st);
}

extern "C" {

int cvtmi_flat_search_masked_dev(cvtmi_flat_t h, const void *q, int64_t nq, int k, const uint64_t *mask, int64_t mask_words, void *dist, int64_t *labels,
                                 void *stream)
{
    CVTMI_TRY(flat_masked_check(h, q, nq, k, mask, mask_words, dist, labels));
    CVTMI_TRY(use_device(h->device));
    if (nq == 0) return CVTMI_OK;
    hipStream_t st = (hipStream_t)stream;
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    CVTMI_TRY(flat_mask_covers(h, mask_words, "cvtmi_flat_search_masked"));
    FlatLease lease;
    CVTMI_TRY(lease.open(h, st, false));
    if (h->n == 0) return launch_flat_masked_pad(dist, labels, nq * k, st);   // an empty index pads everything
    return flat_masked_leased(h, *lease.s, q, nq, k, mask, dist, labels, st);
}

// host pointers: queries and mask words up, the two result arrays down, through the leased set's staging buffers and its stream
int cvtmi_flat_search_masked(cvtmi_flat_t h, const void *q, int64_t nq, int k, const uint64_t *mask, int64_t mask_words, void *dist, int64_t *labels)
{
    CVTMI_TRY(flat_masked_check(h, q, nq, k, mask, mask_words, dist, labels));
    CVTMI_TRY(use_device(h->device));
    if (nq == 0) return CVTMI_OK;
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    CVTMI_TRY(flat_mask_covers(h, mask_words, "cvtmi_flat_search_masked"));
    if (h->n == 0) {   // an empty index pads everything
        for (int64_t i = 0; i < nq * k; ++i) { reinterpret_cast<uint32_t *>(dist)[i] = 0x7f800000u; labels[i] = -1; }
        return CVTMI_OK;
    }
    FlatLease lease;
    CVTMI_TRY(lease.open(h, nullptr, true));
    const HostUpload words{ &lease.s->io_m, mask, (size_t)((h->n + 63) / 64) * 8 };   // (the words behind the rows are never read)
    return host_call(lease, q, (size_t)nq * h->row_bytes, words, dist, (size_t)nq * k * 4, labels, (size_t)nq * k * sizeof(int64_t),
                     [&](FlatScratch &S, const void *dq, const void *dm, void *dd, int64_t *dl, hipStream_t st) {
                         return flat_masked_leased(h, S, dq, nq, k, static_cast<const uint64_t *>(dm), dd, dl, st);
                     });
}

int cvtmi_flat_last_masked(cvtmi_flat_t h, int64_t out[4])
{
    if (!h || !out) return fail(CVTMI_EINVAL, "cvtmi_flat_last_masked: null");
    copy_last(h->pool, h->masked_last, out);
    return CVTMI_OK;
}

int cvtmi_flat_mask_labels_dev(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, uint64_t *mask, int64_t mask_words, void *stream)
{
    CVTMI_TRY(flat_mask_labels_check(h, labels, n_labels, mask, mask_words));
    CVTMI_TRY(use_device(h->device));
    hipStream_t st = (hipStream_t)stream;
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    CVTMI_TRY(flat_mask_covers(h, mask_words, "cvtmi_flat_mask_labels"));
    FlatLease lease;
    CVTMI_TRY(lease.open(h, st, false));
    std::vector<int64_t> tab;   // explicit labels: the table of the set
    if (!h->identity && n_labels > 0 && h->n > 0 && mask_words > 0) CVTMI_TRY(sorted_unique_dev("cvtmi_flat_mask_labels", labels, n_labels, tab, st));
    CVTMI_TRY(flat_mask_labels_leased(h, *lease.s, labels, n_labels, tab.data(), (int64_t)tab.size(), mask, mask_words, st));
    if (!tab.empty()) CVTMI_HIP(stream_wait(st));   // (the table leaves host memory that ends with this call)
    return CVTMI_OK;
}

int cvtmi_flat_mask_labels(cvtmi_flat_t h, const int64_t *labels, int64_t n_labels, uint64_t *mask, int64_t mask_words)
{
    CVTMI_TRY(flat_mask_labels_check(h, labels, n_labels, mask, mask_words));
    CVTMI_TRY(use_device(h->device));
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    CVTMI_TRY(flat_mask_covers(h, mask_words, "cvtmi_flat_mask_labels"));
    if (mask_words == 0) return CVTMI_OK;
    if (h->n == 0 || n_labels == 0) {
        memset(mask, 0, (size_t)mask_words * 8);
        return CVTMI_OK;
    }
    FlatLease lease;
    CVTMI_TRY(lease.open(h, nullptr, true));
    FlatScratch &S = *lease.s;
    hipStream_t st = lease.st;
    const int64_t words = (h->n + 63) / 64;   // (the words that can hold a row)
    std::vector<int64_t> tab;
    if (h->identity) {
        CVTMI_TRY(S.io_c.reserve((size_t)n_labels * 8));
        CVTMI_HIP(hipMemcpyAsync(S.io_c.p, labels, (size_t)n_labels * 8, hipMemcpyHostToDevice, st));
    } else {
        CVTMI_TRY(sorted_unique("cvtmi_flat_mask_labels", labels, n_labels, tab));
    }
    CVTMI_TRY(S.io_m.reserve((size_t)words * 8));
    CVTMI_TRY(flat_mask_labels_leased(h, S, S.io_c.as<int64_t>(), n_labels, tab.data(), (int64_t)tab.size(), S.io_m.as<uint64_t>(), words, st));
    return mask_host_finish(S.io_m, words, mask, mask_words, st);
}

}  // extern "C"
