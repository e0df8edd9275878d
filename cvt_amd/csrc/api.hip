// api.hip -- the C ABI of libcvtmi (include/cvtmi.h): handles, HBM residency, host<->device
// staging for the host-pointer entry points, and dispatch to the HIP kernels.  No compute happens
// on the CPU here; without a HIP device every entry fails with CVTMI_EHIP.
// This file: the library level -- error state, devices, the tuning values (tuning.def) and cvtmi_set_tuning / cvtmi_get_tuning, page-locked memory, top-k
// select / merge, what the sharded entries share.  The handle types live in api_opq.hip, api_flat.hip and api_hnsw.hip, the
// handle-less model entries in api_models.hip; api_internal.h is what they share.
#include <stdarg.h>
#include <string.h>

#include <algorithm>

#include "api_internal.h"
#include "launch.h"

namespace cvtmi {

thread_local std::string g_err;

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

// ---- the launch log of launch.h: per thread, off unless cvtmi_debug_launch_log_begin turned it on (include/cvtmi.h) ----
struct LaunchLog {
    struct Rec { const char *what; int64_t x, y, z, block, lds; };
    std::vector<Rec> recs;
    int depth = 0;
};
__thread LaunchLog *g_launch_log = nullptr;          // what launch() tests: the thread's log while depth > 0
static thread_local LaunchLog g_launch_log_store;    // the records outlive the last _end until the next outermost _begin

void launch_log_note(const char *what, const Grid &grid, unsigned block_x, size_t lds)
{
    try {
        g_launch_log->recs.push_back({ what, grid.x, grid.y, grid.z, (int64_t)block_x, (int64_t)lds });
    } catch (...) {   // out of host memory: the launch goes ahead, the note is lost
    }
}

extern "C" int64_t cvtmi_debug_launch_log_begin(void)
{
    LaunchLog &L = g_launch_log_store;
    if (L.depth == 0) L.recs.clear();
    ++L.depth;
    g_launch_log = &L;
    return (int64_t)L.recs.size();
}

extern "C" int64_t cvtmi_debug_launch_log_end(void)
{
    LaunchLog &L = g_launch_log_store;
    if (L.depth <= 0) return fail(CVTMI_EINVAL, "cvtmi_debug_launch_log_end: no cvtmi_debug_launch_log_begin of this thread is open");
    if (--L.depth == 0) g_launch_log = nullptr;
    return (int64_t)L.recs.size();
}

extern "C" int64_t cvtmi_debug_launch_log_read(int64_t first, int64_t cap, cvtmi_launch_record *out)
{
    const LaunchLog &L = g_launch_log_store;
    const int64_t total = (int64_t)L.recs.size();
    if (first < 0 || cap < 0 || (cap > 0 && !out)) return fail(CVTMI_EINVAL, "cvtmi_debug_launch_log_read: bad arguments");
    for (int64_t i = first; i < total && i - first < cap; ++i) {
        const LaunchLog::Rec &r = L.recs[(size_t)i];
        cvtmi_launch_record &o = out[i - first];
        snprintf(o.name, sizeof o.name, "%s", r.what);
        o.grid[0] = r.x; o.grid[1] = r.y; o.grid[2] = r.z; o.block = r.block; o.lds = r.lds;
    }
    return total;
}

// ---- the tuning values: one object per line of tuning.def, and the four rules that are more than a range ----
std::atomic<int> g_scanh_key{0};  // bumped when a planner setting of adc_scan16h changes (REPLAN): cached item tables are rebuilt

static int tune_scanh_fix_rule(int64_t *v) { if (*v <= 0) *v = 160000; return CVTMI_OK; }
static int tune_flat_u8_tfilter_chunks_rule(int64_t *v) { *v = *v >= 4 ? 4 : (*v >= 2 ? 2 : 1); return CVTMI_OK; }
static int tune_scanh_min_rows_rule(int64_t *v)
{
    if (*v < 1) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: scanh_min_rows must be positive");
    *v = std::max<int64_t>(*v, 2048);
    return CVTMI_OK;
}
static int tune_flat_u8_dbg_rule(int64_t *v)
{
#ifdef CVTMI_GF_DBG
    *v = std::clamp<int64_t>(*v, INT32_MIN, INT32_MAX);
    return CVTMI_OK;
#else
    return fail(CVTMI_EUNSUPPORTED, "cvtmi_set_tuning: flat_u8_dbg needs a -DCVTMI_GF_DBG build (timing experiments, results wrong)");
#endif
}
#define REJECT(lo, hi) Tunable::kReject, (lo), (hi), nullptr
#define CLAMP(lo, hi) Tunable::kClamp, (lo), (hi), nullptr
#define BOOL Tunable::kBool, 0, 1, nullptr
#define ANY CLAMP(INT32_MIN, INT32_MAX)
#define HOOK(fn) Tunable::kHook, 0, 0, (fn)
#define TUNE(name, def, rule, flags) [[clang::require_constant_initialization]] Tunable tune_##name{#name, (def), rule, (flags)};
#include "tuning.def"
#undef TUNE
#define TUNE(name, def, rule, flags) &tune_##name,
Tunable *const tune_all[] = {
#include "tuning.def"
};
#undef TUNE
#undef REJECT
#undef CLAMP
#undef BOOL
#undef ANY
#undef HOOK
// ENV_DEFAULT, the one default read at load time (a measurement aid: the CLIs have no tuning switch)
static const int g_env_defaults = [] {
    if (const char *e = getenv("CVTMI_HOST_SPIN_US"))
        for (Tunable *t : tune_all)
            if (t->flags & ENV_DEFAULT) t->v.store(atoi(e), std::memory_order_relaxed);
    return 0;
}();

static Tunable *find_tunable(const char *name)
{
    for (Tunable *t : tune_all)
        if (!strcmp(name, t->name)) return t;
    return nullptr;
}

int use_device(int dev)
{
    int cur = -1;
    CVTMI_HIP(hipGetDevice(&cur));
    if (cur != dev) CVTMI_HIP(hipSetDevice(dev));
    return CVTMI_OK;
}

int sharded_local_failure(cvtmi_comm_t c)
{
    if (const int inj = tune_comm_inject_failure.geti(); inj >= 0 && inj == comm_rank(c)) return fail(CVTMI_ESTATE, "injected failure of rank %d (comm_inject_failure)", comm_rank(c));
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
    Tunable *t = find_tunable(name);
    if (!t) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: unknown parameter '%s'", name);
    switch (t->rule) {
    case Tunable::kReject:
        if (value < t->lo) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: %s must be at least %lld", name, (long long)t->lo);
        if (value > t->hi) return fail(CVTMI_EINVAL, "cvtmi_set_tuning: %s must be at most %lld", name, (long long)t->hi);
        break;
    case Tunable::kClamp: value = std::clamp(value, t->lo, t->hi); break;
    case Tunable::kBool: value = value != 0; break;
    case Tunable::kHook: CVTMI_TRY(t->hook(&value)); break;
    }
    t->v.store(value, std::memory_order_relaxed);
    if (t->flags & REPLAN) ++g_scanh_key;
    return CVTMI_OK;
}

int cvtmi_get_tuning(const char *name, int64_t *value)
{
    if (!name || !value) return fail(CVTMI_EINVAL, "cvtmi_get_tuning: null argument");
    const Tunable *t = find_tunable(name);
    if (!t) return fail(CVTMI_EINVAL, "cvtmi_get_tuning: unknown parameter '%s'", name);
    *value = t->get();
    return CVTMI_OK;
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
