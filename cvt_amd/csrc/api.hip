// api.hip -- the C ABI of libcvtmi (include/cvtmi.h): handles, HBM residency, host<->device
// staging for the host-pointer entry points, and dispatch to the HIP kernels.  No compute happens
// on the CPU here; without a HIP device every entry fails with CVTMI_EHIP.
// This file: the library level -- error state, devices, the tuning values and cvtmi_set_tuning, page-locked memory, top-k
// select / merge, what the sharded entries share.  The handle types live in api_opq.hip, api_flat.hip and api_hnsw.hip, the
// handle-less model entries in api_models.hip; api_internal.h is what they share.
#include <stdarg.h>
#include <string.h>

#include <algorithm>

#include "api_internal.h"

namespace cvtmi {

static int host_spin_default()
{
    const char *e = getenv("CVTMI_HOST_SPIN_US");   // (measurement aid: the CLIs have no tuning switch)
    return e ? atoi(e) : 200;
}
std::atomic<int> g_host_spin_us{host_spin_default()};   // host_util.h: stream_wait
thread_local std::string g_err;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// the values cvtmi_set_tuning sets (declared in api_internal.h for the files that read them)
std::atomic<int> g_ivf_part_cap_mb{256};   // cvtmi_set_tuning("ivf_part_cap_mb"): room for the partial lists of an IVF search
std::atomic<int64_t> g_ivf_range_spill{4096};   // cvtmi_set_tuning("ivf_range_spill"): hits a part of a range search may leave in the spill area
std::atomic<int> g_hnsw_slots_cap{0};   // cvtmi_set_tuning("hnsw_slots"): cap on traversals per CU (0 = what LDS allows, at most 32)
std::atomic<int> g_small_zero_copy{1};   // cvtmi_set_tuning("opq_small_zero_copy"): 1 .. 8-query host-pointer searches read / write the pinned staging area from the kernels
std::atomic<int64_t> g_scans_max_work{(int64_t)48 << 20};   // cvtmi_set_tuning("scans_max_work"): rows x query groups up to which the OPQ small-batch form answers (scans_chosen)
std::atomic<int> g_scan_bigk{1};          // cvtmi_set_tuning("scan_bigk"): 0 = k > 128 on the exact kernels only (one query per workgroup: rounds 4-5), 1 = the filter pipeline
std::atomic<int> g_scan_packed{1};        // cvtmi_set_tuning("scan_packed_m"): 0 = M = 8 / 4 through the padded rows like every other M < 16 (round 5), 1 = adc_scan16p
std::atomic<int> g_scan_pad{1};           // cvtmi_set_tuning("scan_pad_m"): 0 = an OPQ index with M < 16 stays on the row-per-lane scan kernels (opq_pads)
std::atomic<int> g_sq8_host_small{1};     // cvtmi_set_tuning("sq8_host_small"): small SQ8 host-pointer calls run out of a page-locked scratch area (Sq8HostScratch)
std::atomic<int> g_flat_f32_rows_copy{4};   // cvtmi_set_tuning("flat_f32_rows_copy"): narrowest fp32 row that gets a row-major copy beside the blocked rows once the threshold filter
                                                  // answers on the handle (0 = never): + 4 D bytes per row, the exact finish reads whole cache lines
std::atomic<int> g_flat_u8_filter_min_nq{129};            // cvtmi_set_tuning("flat_u8_filter_min_nq" / "_min_rows" / "_min_work"): smallest batch, table and
std::atomic<int64_t> g_flat_u8_filter_min_rows{524288};   // rows x width x queries (in 1e9) the dispatch hands to the uint8 sample + filter pipeline
std::atomic<int64_t> g_flat_u8_filter_min_work{130};
std::atomic<int> g_flat_u8_sample_passes{10};  // cvtmi_set_tuning("flat_u8_sample_passes"): the uint8 filter pipeline's sample goes through the streaming kernel up to this many 128-query passes
std::atomic<int> g_flat_small_zero_copy{1};   // cvtmi_set_tuning("flat_small_zero_copy"): small host-pointer flat searches write their lists into pinned memory from the kernels
std::atomic<int> g_host_zero_copy{1};   // cvtmi_set_tuning("opq_host_zero_copy"): page-locked result arrays are written by the kernels themselves, the batch is not cut
std::atomic<int> g_host_chunks{4096};  // cvtmi_set_tuning("opq_host_chunk"): queries per piece of a pipelined host-pointer OPQ batch (0 = one piece)
std::atomic<int> g_scanh_key{0};  // bumped when a planner setting of adc_scan16h changes: cached item tables are rebuilt
static std::atomic<int> g_inject_failure{-1};  // cvtmi_set_tuning("comm_inject_failure", r): the local search of rank r of a sharded search fails (tests)
std::atomic<int> g_flat_variant{0};  // cvtmi_set_tuning("flat_variant"): 0 = choose, 1 = exact kernels only, 2 = matrix-core filter wherever it applies
std::atomic<int> g_flat_f32_stream{1};  // cvtmi_set_tuning("flat_f32_stream"): 0 = off, 1 = choose, 2 = wherever it applies
std::atomic<int> g_flat_count_redo{0};  // cvtmi_set_tuning("flat_count_redo"): 1 = count the redo flags of each search (a copy back and a wait per search)

int use_device(int dev)
{
    int cur = -1;
    CVTMI_HIP(hipGetDevice(&cur));
    if (cur != dev) CVTMI_HIP(hipSetDevice(dev));
    return CVTMI_OK;
}

int sharded_local_failure(cvtmi_comm_t c)
{
    if (const int inj = g_inject_failure.load(); inj >= 0 && inj == comm_rank(c)) return fail(CVTMI_ESTATE, "injected failure of rank %d (comm_inject_failure)", comm_rank(c));
    return CVTMI_OK;
}

// One process, every GPU: handles[d] holds the row block of device d (its id base set), comms = cvtmi_comm_create_all.  The
// queries go up to every device, the local searches are enqueued device after device (they run side by side), the all-gathers
// leave as one group, the merge runs on the first device.
int sharded_all(cvtmi_comm_t *comms, int ndev, const void *q, size_t q_bytes, int64_t nq, int k, void *dist, int64_t *ids,
                const int *devices, const ShardLocalSearch &local_search)
{
    std::vector<Tmp> dq(ndev);
    std::vector<int> status(ndev, CVTMI_OK);
    for (int d = 0; d < ndev; ++d) {
        CVTMI_HIP(hipSetDevice(devices[d]));
        float *sd = nullptr;
        int64_t *si = nullptr;
        int rc = sharded_local_failure(comms[d]);
        if (rc == CVTMI_OK) rc = dq[d].alloc(q_bytes);
        if (rc == CVTMI_OK && hipMemcpyAsync(dq[d].p, q, q_bytes, hipMemcpyHostToDevice, nullptr) != hipSuccess) rc = fail(CVTMI_EHIP, "query upload to device %d failed", devices[d]);
        if (rc == CVTMI_OK) rc = comm_local_slot(comms[d], nq, k, &sd, &si);
        if (rc == CVTMI_OK) rc = local_search(d, dq[d].p, sd, si);
        status[d] = rc;
    }
    CVTMI_HIP(hipSetDevice(devices[0]));
    Tmp dd, di;
    CVTMI_TRY(dd.alloc((size_t)nq * k * 4));
    CVTMI_TRY(di.alloc((size_t)nq * k * 8));
    const int rc = comm_exchange_merge_all(comms, ndev, nq, k, status.data(), dd.as<float>(), di.as<int64_t>());
    for (int d = 0; d < ndev; ++d) {   // the temporaries die with this frame: drain every device first
        (void)hipSetDevice(devices[d]);
        (void)hipDeviceSynchronize();
    }
    CVTMI_HIP(hipSetDevice(devices[0]));
    if (rc != CVTMI_OK) return rc;
    CVTMI_HIP(hipMemcpy(dist, dd.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(ids, di.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

}  // namespace cvtmi

extern "C" {

// ================================================================ library =====================
int cvtmi_version(void) { return CVTMI_VERSION; }
const char *cvtmi_last_error(void) { return g_err.c_str(); }

int cvtmi_device_count(int *count)
{
    if (!count) return fail(CVTMI_EINVAL, "cvtmi_device_count: null");
    *count = 0;
    CVTMI_HIP(hipGetDeviceCount(count));
    return CVTMI_OK;
}

int cvtmi_set_tuning(const char *name, int64_t value)
{
    if (!name) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: null name");
    if (!strcmp(name, "assign_variant")) {
        if (value < 0 || value > 2) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: assign_variant must be 0, 1 or 2");
        set_assign_variant((int)value);
        return CVTMI_OK;
    }
    if (!strcmp(name, "flat_variant")) {
        if (value < 0 || value > 2) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: flat_variant must be 0, 1 or 2");
        g_flat_variant = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "probe_variant")) {
        if (value < 0 || value > 2) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: probe_variant must be 0, 1 or 2");
        set_probe_variant((int)value);
        return CVTMI_OK;
    }
    if (!strcmp(name, "flat_f32_nt")) {
        if (value < 0 || value > 2) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: flat_f32_nt must be 0, 1 or 2");
        set_flat_f32_nt((int)value);
        return CVTMI_OK;
    }
    if (!strcmp(name, "scanh_balance")) {
        if (value < 0 || value > 2) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: scanh_balance must be 0, 1 or 2");
        set_scanh_balance((int)value);
        ++g_scanh_key;
        return CVTMI_OK;
    }
    if (!strcmp(name, "scans_dbg")) { set_scans_dbg((int)value); return CVTMI_OK; }
    if (!strcmp(name, "opq_host_chunk")) {
        if (value < 0 || value > (1 << 24)) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: opq_host_chunk must be 0..2^24");
        g_host_chunks = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "scanh_fix")) { set_scanh_fix(value); ++g_scanh_key; return CVTMI_OK; }
    if (!strcmp(name, "scanh_share_hist")) { set_scanh_share_hist((int)value); return CVTMI_OK; }
    if (!strcmp(name, "scanh_tail")) {
        set_scanh_tail((int)value);
        ++g_scanh_key;
        return CVTMI_OK;
    }
    if (!strcmp(name, "scanh_min_rows")) {
        if (value < 1) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: scanh_min_rows must be positive");
        set_scanh_min_rows(value);
        ++g_scanh_key;
        return CVTMI_OK;
    }
    if (!strcmp(name, "scan_seed")) {
        if (value < 0 || value > 1) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: scan_seed must be 0 or 1");
        set_scan_seed((int)value);
        return CVTMI_OK;
    }
    if (!strcmp(name, "flat_f32_stream")) {
        if (value < 0 || value > 2) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: flat_f32_stream must be 0, 1 or 2");
        g_flat_f32_stream = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "flat_f32_dbg")) { set_flat_f32_dbg((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_count_redo")) {
        if (value < 0 || value > 1) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: flat_count_redo must be 0 or 1");
        g_flat_count_redo = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "flat_f32_tfilter")) { set_flat_f32_tfilter((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_tfilter_min")) { set_flat_f32_tfilter_min((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_tfilter_one")) { set_flat_f32_tfilter_one((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_tfilter_bigk")) { set_flat_f32_tfilter_bigk((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_tfilter_retry")) { set_flat_f32_tfilter_retry((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_tfilter_wide_band")) { set_flat_f32_tfilter_wide_band((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_packed")) { set_flat_f32_packed((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_tfilter_min_rows")) { set_flat_f32_tfilter_min_rows((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_tfilter_sample")) { set_flat_f32_tfilter_sample((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_share")) {
        if (value < 0 || value > 1) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: flat_f32_share must be 0 or 1 (the eight- and twelve-wave forms are gone)");
        set_flat_f32_share((int)value);
        return CVTMI_OK;
    }
    if (!strcmp(name, "opq_small_zero_copy")) { g_small_zero_copy = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "host_spin_us")) { g_host_spin_us = value < 0 ? 0 : (int)value; return CVTMI_OK; }
    if (!strcmp(name, "hnsw_top_lds")) { set_hnsw_top_lds((int)value); return CVTMI_OK; }
    if (!strcmp(name, "hnsw_build_frac")) { set_hnsw_build_frac((int)std::min<int64_t>(value, 1 << 30)); return CVTMI_OK; }
    if (!strcmp(name, "hnsw_build_cap")) { set_hnsw_build_cap((int)std::min<int64_t>(value, 1 << 30)); return CVTMI_OK; }
    if (!strcmp(name, "hnsw_build_phases")) { set_hnsw_build_phases((int)value); return CVTMI_OK; }
    if (!strcmp(name, "hnsw_adc_tables")) { set_hnsw_adc_tables((int)value); return CVTMI_OK; }
    if (!strcmp(name, "hnsw_slots")) { g_hnsw_slots_cap = (int)value; return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_tfilter")) { set_flat_u8_tfilter((int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_tfilter_min_rows")) { set_flat_u8_tfilter_min_rows(value); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_tfilter_small_min_nq")) { set_flat_u8_tfilter_small_min_nq((int)std::min<int64_t>(value, 1 << 30)); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_tfilter_min_k")) { set_flat_u8_tfilter_min_k((int)std::min<int64_t>(value, 1 << 20)); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_tfilter_min_nq_k65")) { set_flat_u8_tfilter_min_nq_k65((int)std::min<int64_t>(value, 1 << 30)); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_tfilter_min_nq")) { set_flat_u8_tfilter_min_nq((int)std::min<int64_t>(value, 1 << 30)); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_tfilter_chunks")) { set_flat_u8_tfilter_chunks((int)std::min<int64_t>(value, 4)); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_tfilter_sample")) { set_flat_u8_tfilter_sample((int)std::min<int64_t>(value, 64)); return CVTMI_OK; }
    if (!strcmp(name, "flat_f32_rows_copy")) { g_flat_f32_rows_copy = value < 0 ? 0 : (value > (1 << 20) ? (1 << 20) : (int)value); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_gfilter")) { set_flat_u8_gfilter((int)value); return CVTMI_OK; }
    if (!strcmp(name, "sq8_encode_wave")) { set_sq8_encode_wave(value != 0); return CVTMI_OK; }
    if (!strcmp(name, "sq8_filter")) { set_sq8_filter(value != 0); return CVTMI_OK; }
    if (!strcmp(name, "scan_pad_m")) { g_scan_pad = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "scan_packed_m")) { g_scan_packed = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "scan_bigk")) { g_scan_bigk = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "sq8_host_small")) { g_sq8_host_small = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "scans_max_work")) { g_scans_max_work = value < 0 ? 0 : value; return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_filter_min_nq")) { g_flat_u8_filter_min_nq = value < 1 ? 1 : value > (1 << 30) ? (1 << 30) : (int)value; return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_filter_min_rows")) { g_flat_u8_filter_min_rows = value < 0 ? 0 : value; return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_filter_min_work")) { g_flat_u8_filter_min_work = value < 0 ? 0 : value; return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_sample_passes")) { g_flat_u8_sample_passes = value < 0 ? 0 : value > 64 ? 64 : (int)value; return CVTMI_OK; }
    if (!strcmp(name, "flat_small_zero_copy")) { g_flat_small_zero_copy = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "opq_host_zero_copy")) { g_host_zero_copy = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "scan_tail_splits")) { set_scan_tail_splits((int)value); return CVTMI_OK; }
    if (!strcmp(name, "ivf_part_cap_mb")) {
        if (value < 0 || value > 4096) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: ivf_part_cap_mb must be 0 .. 4096");
        g_ivf_part_cap_mb = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "ivf_range_spill")) {
        if (value < 0) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: ivf_range_spill must be >= 0");
        g_ivf_range_spill = value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "sq8_flags")) { set_sq8_flags((int)value); return CVTMI_OK; }
    if (!strcmp(name, "sq8_wave_blocks")) {
        if (value < 1 || value > 64) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: sq8_wave_blocks must be 1..64");
        set_sq8_wave_blocks((int)value);
        return CVTMI_OK;
    }
    if (!strcmp(name, "flat_u8_mstream_min_rows")) { set_flat_u8_mstream_min_rows(value); return CVTMI_OK; }
    if (!strcmp(name, "flat_u8_mstream_min")) {
        if (value < 1 || value > 129) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: flat_u8_mstream_min must be 1..129");
        set_flat_u8_mstream_min((int)value);
        return CVTMI_OK;
    }
    if (!strcmp(name, "flat_u8_dbg")) {
        if (set_flat_u8_dbg((int)value) != CVTMI_OK) return fail(CVTMI_EUNSUPPORTED, "cvtmi_set_tuning: flat_u8_dbg needs a -DCVTMI_GF_DBG build (timing experiments, results wrong)");
        return CVTMI_OK;
    }
    if (!strcmp(name, "flat_u8_opt")) {
        if (value < 0 || value > 3) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: flat_u8_opt must be 0..3");
        set_flat_u8_opt((int)value);
        return CVTMI_OK;
    }
    if (!strcmp(name, "comm_force_rccl")) { comm_set_force_rccl(value != 0); return CVTMI_OK; }
    if (!strcmp(name, "comm_check_status")) { comm_set_check_status(value != 0); return CVTMI_OK; }
    if (!strcmp(name, "comm_inject_failure")) { g_inject_failure = (int)value; return CVTMI_OK; }
    return fail(CVTMI_EINVAL, "cvtmi_set_tuning: unknown parameter '%s'", name);
}

int cvtmi_set_device(int device)
{
    CVTMI_HIP(hipSetDevice(device));
    return CVTMI_OK;
}

// page-locked host memory for the arrays of the host-pointer entries (queries in, results out)
int cvtmi_host_alloc(size_t bytes, void **p)
{
    if (!p) return fail(CVTMI_EINVAL, "cvtmi_host_alloc: null");
    *p = nullptr;
    hipError_t e = hipHostMalloc(p, bytes ? bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess) { *p = nullptr; return fail(CVTMI_ENOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
    return CVTMI_OK;
}

int cvtmi_host_free(void *p)
{
    if (p) CVTMI_HIP(hipHostFree(p));
    return CVTMI_OK;
}

// ================================================================ merge =======================
int cvtmi_topk_merge_dev(const float *in_dist, const int64_t *in_ids, int64_t nq, int L, int k, float *dist, int64_t *ids,
                         void *stream)
{
    if (nq < 0 || L < 1 || (nq > 0 && (!in_dist || !in_ids || !dist || !ids)))
        return fail(CVTMI_EINVAL, "cvtmi_topk_merge: bad arguments");
    return launch_topk_merge(in_dist, in_ids, nq, L, k, dist, ids, (hipStream_t)stream);
}

int cvtmi_topk_merge(const float *in_dist, const int64_t *in_ids, int64_t nq, int L, int k, float *dist, int64_t *ids)
{
    if (nq < 0 || L < 1 || k < 1 || (nq > 0 && (!in_dist || !in_ids || !dist || !ids)))
        return fail(CVTMI_EINVAL, "cvtmi_topk_merge: bad arguments");
    if (nq == 0) return CVTMI_OK;
    const size_t cnt = (size_t)nq * L * k, oc = (size_t)nq * k;
    Tmp a, b, c, d;
    CVTMI_TRY(a.upload(in_dist, cnt * sizeof(float)));
    CVTMI_TRY(b.upload(in_ids, cnt * sizeof(int64_t)));
    CVTMI_TRY(c.alloc(oc * sizeof(float)));
    CVTMI_TRY(d.alloc(oc * sizeof(int64_t)));
    CVTMI_TRY(cvtmi_topk_merge_dev(a.as<float>(), b.as<int64_t>(), nq, L, k, c.as<float>(), d.as<int64_t>(), nullptr));
    CVTMI_HIP(hipMemcpy(dist, c.p, oc * sizeof(float), hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(ids, d.p, oc * sizeof(int64_t), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

int cvtmi_topk_select_dev(const float *scores, int64_t nq, int64_t n, int k, float *dist, int64_t *ids, void *stream)
{
    if (nq < 0 || n < 0 || (nq > 0 && (!dist || !ids || (n > 0 && !scores))))
        return fail(CVTMI_EINVAL, "cvtmi_topk_select: bad arguments");
    return launch_topk_select(scores, nullptr, nq, n, k, dist, ids, (hipStream_t)stream);
}

int cvtmi_topk_select(const float *scores, int64_t nq, int64_t n, int k, float *dist, int64_t *ids)
{
    if (nq < 0 || n < 0 || k < 1 || (nq > 0 && (!dist || !ids || (n > 0 && !scores))))
        return fail(CVTMI_EINVAL, "cvtmi_topk_select: bad arguments");
    if (nq == 0) return CVTMI_OK;
    Tmp a, c, d;
    CVTMI_TRY(a.upload(scores, (size_t)nq * n * sizeof(float)));
    CVTMI_TRY(c.alloc((size_t)nq * k * sizeof(float)));
    CVTMI_TRY(d.alloc((size_t)nq * k * sizeof(int64_t)));
    CVTMI_TRY(cvtmi_topk_select_dev(a.as<float>(), nq, n, k, c.as<float>(), d.as<int64_t>(), nullptr));
    CVTMI_HIP(hipMemcpy(dist, c.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(ids, d.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

}  // extern "C"
