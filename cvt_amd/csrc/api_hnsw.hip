// api_hnsw.hip -- the HNSW handle of the C ABI (include/cvtmi.h): load / build / add / save, the search, the search over OPQ codes (ADC)
// with and without the exact re-rank, each of them under a node mask as well, the mask of a label set, and the delete state of the nodes.
#include <string.h>

#include <algorithm>
#include <cmath>
#include <random>
#include <vector>

#include "api_internal.h"
#include "launch.h"
#include "rm_common.h"

// ================================================================ HNSW search ==================
// searchKnn is a pure read in the reference (hnswalg.h:688-728): searches on one handle run side by side, each on a leased scratch set
// (visited bits, spilled queues, re-rank lists, host staging) and the stream of its caller (the host-pointer entries: the set's own
// stream).  The one call that changes a graph, cvtmi_hnsw_add, holds the handle exclusively (HnswLease holds it shared); every search
// plans its scratch from the node count it finds, so a set that served a smaller graph is re-sized, never reused as it was.

int cvtmi_hnsw_load(const void *file, int64_t bytes, int metric, int D, cvtmi_hnsw_t *out)
{
    if (!file || !out || D < 1 || (metric != CVTMI_METRIC_IP && metric != CVTMI_METRIC_L2F))
        return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: bad arguments (metric must be IP or L2F)");
    if (bytes < 96) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: not a saveIndex file (too short)");
    const uint8_t *f = static_cast<const uint8_t *>(file), *p = f;
    uint64_t offsetLevel0, max_elements, cur_count, size_per, label_off, offsetData, maxM, maxM0, M, efc;
    int32_t maxlevel; uint32_t enterpoint; double mult;
    auto rd = [&](void *dst, size_t nb) { memcpy(dst, p, nb); p += nb; };
    rd(&offsetLevel0, 8); rd(&max_elements, 8); rd(&cur_count, 8); rd(&size_per, 8); rd(&label_off, 8); rd(&offsetData, 8);
    rd(&maxlevel, 4); rd(&enterpoint, 4); rd(&maxM, 8); rd(&maxM0, 8); rd(&M, 8); rd(&mult, 8); rd(&efc, 8);
    if (size_per != 4 + 4 * maxM0 + 4 * (uint64_t)D + 8 || offsetData != 4 + 4 * maxM0 || label_off != offsetData + 4 * (uint64_t)D ||
        offsetLevel0 != 0 || cur_count > max_elements || maxM0 > 4096 || maxM > 4096)
        return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: header does not describe %d-d fp32 vectors (size_data_per_element=%llu)", D,
                    (unsigned long long)size_per);
    // the header is untrusted: the product below must not wrap, and the counts size host allocations
    if (max_elements > ((uint64_t)bytes - 96) / size_per) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: truncated level-0 block");
    if (cur_count > 0 && maxlevel < 0) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: negative maxlevel");
    const int64_t n = (int64_t)cur_count;
    const uint8_t *l0 = p;
    p += max_elements * size_per;
    std::vector<float> vec;
    std::vector<uint32_t> links0, upper;
    std::vector<int64_t> labels, uoff;
    std::vector<int32_t> levels;  // upper levels a node has link blocks for
    std::vector<uint64_t> dead;   // current hnswlib's markDelete: DELETE_MARK = 0x01 in byte 2 of the level-0 count word, the count below it
    int64_t n_dead = 0;
    const uint64_t links_per = 4 * maxM + 4;
    try {
        vec.resize((size_t)n * D);
        links0.resize((size_t)n * (maxM0 + 1));
        labels.resize((size_t)n);
        uoff.assign((size_t)n, -1);
        levels.assign((size_t)n, 0);
        dead.assign((size_t)((n + 63) / 64), 0ull);
        for (int64_t i = 0; i < n; ++i) {
            const uint8_t *e = l0 + (uint64_t)i * size_per;
            uint32_t &cw = links0[(size_t)i * (maxM0 + 1)];
            memcpy(&cw, e, 4 * (maxM0 + 1));
            if ((cw >> 17) != 0 || (cw & 0xffffu) > maxM0) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: corrupt link count");
            if (cw >> 16) { dead[(size_t)(i >> 6)] |= 1ull << (i & 63); ++n_dead; }
            cw &= 0xffffu;   // the device copy holds plain counts
            memcpy(&vec[(size_t)i * D], e + offsetData, 4 * (size_t)D);
            uint64_t lab; memcpy(&lab, e + label_off, 8);
            labels[(size_t)i] = (int64_t)lab;
        }
        for (uint64_t i = 0; i < max_elements; ++i) {
            if ((uint64_t)(f + bytes - p) < 4) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: truncated link lists");
            uint32_t sz; memcpy(&sz, p, 4); p += 4;
            if (sz) {
                if ((uint64_t)(f + bytes - p) < sz || sz % links_per != 0) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: corrupt link list");
                if ((int64_t)i < n) {
                    uoff[(size_t)i] = (int64_t)upper.size();
                    levels[(size_t)i] = (int32_t)(sz / links_per);
                    upper.resize(upper.size() + sz / 4);
                    memcpy(&upper[(size_t)uoff[(size_t)i]], p, sz);
                }
                p += sz;
            }
        }
    } catch (const std::exception &) {
        return fail(CVTMI_ENOMEM, "cvtmi_hnsw_load: out of host memory for %llu elements", (unsigned long long)cur_count);
    }
    // every link must point inside the graph, and a link at level L at a node that HAS a level-L block: the kernel
    // follows them without further checks (hnsw.hip: a.upper + a.upper_off[cur] + (level - 1) * (maxM + 1))
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t *l = &links0[(size_t)i * (maxM0 + 1)];
        for (uint32_t j = 1; j <= l[0]; ++j) if (l[j] >= (uint64_t)n) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: link out of range");
        for (int32_t lv = 1; lv <= levels[(size_t)i]; ++lv) {
            const uint32_t *u = &upper[(size_t)uoff[(size_t)i] + (size_t)(lv - 1) * (maxM + 1)];
            if (u[0] > maxM) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: corrupt upper link count");
            for (uint32_t j = 1; j <= u[0]; ++j) {
                if (u[j] >= (uint64_t)n) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: link out of range");
                if (levels[u[j]] < lv) return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: level-%d link to a node without that level", lv);
            }
        }
    }
    if (n > 0 && (enterpoint >= (uint64_t)n || levels[enterpoint] < maxlevel))
        return fail(CVTMI_EINVAL, "cvtmi_hnsw_load: bad entry point");
    int dev = 0;
    CVTMI_HIP(hipGetDevice(&dev));  // no device: fails here, there is no CPU path
    cvtmi_hnsw_s *h = new (std::nothrow) cvtmi_hnsw_s();
    if (!h) return fail(CVTMI_ENOMEM, "cvtmi_hnsw_load: out of host memory");
    h->device = dev; h->metric = metric; h->D = D; h->cus = device_cus();
    auto up = [&](DevBuf &b, const void *src, size_t nb) -> int {
        CVTMI_TRY(b.reserve(nb ? nb : 16));
        if (nb) CVTMI_HIP(hipMemcpy(b.p, src, nb, hipMemcpyHostToDevice));
        return CVTMI_OK;
    };
    int rc = up(h->vec, vec.data(), vec.size() * 4);
    if (rc == CVTMI_OK) rc = up(h->links0, links0.data(), links0.size() * 4);
    if (rc == CVTMI_OK) rc = up(h->labels, labels.data(), labels.size() * 8);
    if (rc == CVTMI_OK) rc = up(h->upper_off, uoff.data(), uoff.size() * 8);
    if (rc == CVTMI_OK) rc = up(h->upper, upper.data(), upper.size() * 4);
    if (rc == CVTMI_OK) rc = up(h->dead, dead.data(), dead.size() * 8);
    if (rc != CVTMI_OK) { cvtmi_hnsw_destroy(h); return rc; }
    h->n_dead = n_dead;
    h->g.vec = h->vec.as<float>(); h->g.links0 = h->links0.as<uint32_t>(); h->g.labels = h->labels.as<int64_t>();
    h->g.upper_off = h->upper_off.as<int64_t>(); h->g.upper = h->upper.as<uint32_t>();
    h->g.n = n; h->g.D = D; h->g.maxM = (int)maxM; h->g.maxM0 = (int)maxM0; h->g.maxlevel = n > 0 ? maxlevel : 0;
    h->g.enterpoint = enterpoint;
    h->levels.swap(levels);
    h->max_elements = max_elements; h->M = M; h->efc = efc; h->mult = mult;
    h->hdr_maxlevel = maxlevel; h->hdr_enterpoint = enterpoint;
    h->upper_words = (int64_t)upper.size();   // (the level stream stays at its initialiser: 0 draws, as after the reference's loadIndex)
    *out = h;
    return CVTMI_OK;
}

// Graph construction (hnswalg.h:584-684), batch-synchronous: hnsw_build.hip.  The constructor's fields (:104-127): maxM = M,
// maxM0 = 2 M, mult = 1 / ln M, ef_construction = max(efc, M); levels are the draws of std::default_random_engine(100) in row
// order (getRandomLevel, :143-148), made here on the host as the reference makes them.
static int hnsw_build_impl(const float *x, bool dev, int64_t n, int D, int metric, int M, int efc, const uint64_t *labels, int max_batch,
                           cvtmi_hnsw_t *out, hipStream_t st)
{
    if (out) *out = nullptr;
    if (!x || !out || n < 1 || D < 1 || (metric != CVTMI_METRIC_IP && metric != CVTMI_METRIC_L2F) || M < 2 || efc < 1 || max_batch < 0)
        return fail(CVTMI_EINVAL, "cvtmi_hnsw_build: bad arguments (n >= 1, D >= 1, metric IP or L2F, M >= 2, ef_construction >= 1, max_batch >= 0)");
    if (M > 32) return fail(CVTMI_EINVAL, "cvtmi_hnsw_build: M=%d > 32 (a level-0 list of 2 M links is one wave)", M);
    const int efe = efc > M ? efc : M;
    if (efe > hnsw_ef_max()) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_build: ef_construction=%d > %d", efe, hnsw_ef_max());
    if (n > 0x7fffffffLL) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_build: n too large");
    if (D > 4096) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_build: D=%d > 4096", D);
    const int maxM = M, maxM0 = 2 * M;
    const double mult = 1 / log(1.0 * M);
    std::vector<int32_t> levels;
    std::vector<int64_t> uoff;
    std::vector<int64_t> lab;
    int32_t maxlevel = 0;
    uint32_t ep = 0;
    int64_t upper_words = 0;
    std::default_random_engine rng(100);
    try {
        levels.resize((size_t)n);
        uoff.assign((size_t)n, -1);
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        for (int64_t i = 0; i < n; ++i) {
            levels[(size_t)i] = (int32_t)(-log(u01(rng)) * mult);
            if (levels[(size_t)i] > 0) { uoff[(size_t)i] = upper_words; upper_words += (int64_t)levels[(size_t)i] * (maxM + 1); }
            if (i == 0 || levels[(size_t)i] > maxlevel) { maxlevel = levels[(size_t)i]; ep = (uint32_t)i; }
        }
        if (!labels) { lab.resize((size_t)n); for (int64_t i = 0; i < n; ++i) lab[(size_t)i] = i; }
    } catch (const std::exception &) {
        return fail(CVTMI_ENOMEM, "cvtmi_hnsw_build: out of host memory for %lld rows", (long long)n);
    }
    int devn = 0;
    CVTMI_HIP(hipGetDevice(&devn));
    cvtmi_hnsw_s *h = new (std::nothrow) cvtmi_hnsw_s();
    if (!h) return fail(CVTMI_ENOMEM, "cvtmi_hnsw_build: out of host memory");
    h->device = devn; h->metric = metric; h->D = D; h->cus = device_cus();
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    auto run = [&]() -> int {
        const size_t vb = (size_t)n * D * 4, l0b = (size_t)n * (maxM0 + 1) * 4, ub = (size_t)upper_words * 4;
        CVTMI_TRY(h->vec.reserve(vb));
        CVTMI_TRY(h->links0.reserve(l0b));
        CVTMI_TRY(h->labels.reserve((size_t)n * 8));
        CVTMI_TRY(h->upper_off.reserve((size_t)n * 8));
        CVTMI_TRY(h->upper.reserve(ub ? ub : 16));
        CVTMI_TRY(h->dead.reserve((size_t)((n + 63) / 64) * 8));
        CVTMI_HIP(hipMemsetAsync(h->dead.p, 0, (size_t)((n + 63) / 64) * 8, st));
        CVTMI_HIP(hipMemcpyAsync(h->vec.p, x, vb, in, st));
        CVTMI_HIP(hipMemsetAsync(h->links0.p, 0, l0b, st));
        if (ub) CVTMI_HIP(hipMemsetAsync(h->upper.p, 0, ub, st));
        if (labels) CVTMI_HIP(hipMemcpyAsync(h->labels.p, labels, (size_t)n * 8, in, st));
        else CVTMI_HIP(hipMemcpyAsync(h->labels.p, lab.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
        CVTMI_HIP(hipMemcpyAsync(h->upper_off.p, uoff.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
        h->g.vec = h->vec.as<float>(); h->g.links0 = h->links0.as<uint32_t>(); h->g.labels = h->labels.as<int64_t>();
        h->g.upper_off = h->upper_off.as<int64_t>(); h->g.upper = h->upper.as<uint32_t>();
        h->g.n = n; h->g.D = D; h->g.maxM = maxM; h->g.maxM0 = maxM0; h->g.maxlevel = maxlevel; h->g.enterpoint = ep;
        // (launch_hnsw_build synchronises the stream before it returns: the host vectors above outlive every copy from them)
        return launch_hnsw_build("cvtmi_hnsw_build", h->g, h->links0.as<uint32_t>(), h->upper.as<uint32_t>(), levels.data(), 0, 0u, 0, metric, M,
                                 efe, max_batch, h->cus, st, nullptr, nullptr);
    };
    const int rc = run();
    if (rc != CVTMI_OK) { (void)hipStreamSynchronize(st); cvtmi_hnsw_destroy(h); return rc; }
    h->levels.swap(levels);
    h->max_elements = (uint64_t)n; h->M = (uint64_t)M; h->efc = (uint64_t)efe; h->mult = mult;
    h->hdr_maxlevel = maxlevel; h->hdr_enterpoint = ep;
    h->upper_words = upper_words;
    h->level_rng = rng; h->level_draws = n;   // cvtmi_hnsw_add continues the stream: build + add draws what a longer build draws
    *out = h;
    return CVTMI_OK;
}

int cvtmi_hnsw_build(const float *x, int64_t n, int D, int metric, int M, int ef_construction, const uint64_t *labels, int max_batch,
                     cvtmi_hnsw_t *out)
{
    return hnsw_build_impl(x, false, n, D, metric, M, ef_construction, labels, max_batch, out, nullptr);
}
int cvtmi_hnsw_build_dev(const float *x, int64_t n, int D, int metric, int M, int ef_construction, const uint64_t *labels,
                         int max_batch, cvtmi_hnsw_t *out, void *stream)
{
    return hnsw_build_impl(x, true, n, D, metric, M, ef_construction, labels, max_batch, out, (hipStream_t)stream);
}
int cvtmi_hnsw_build_phases(double *ms)
{
    if (!ms) return fail(CVTMI_EINVAL, "cvtmi_hnsw_build_phases: null pointer");
    hnsw_build_phase_ms(ms);
    return CVTMI_OK;
}

// ================================================================ incremental insertion ========
// cvtmi_hnsw_add: the build's batches continued from the graph as it stands.  Everything comes from the handle:
// M / maxM / maxM0 / mult / ef_construction from its header, the levels from its level stream, the entry point and the top level
// from the graph.  Order: checks, level draws (on a copy of the engine), storage -- every buffer grown, contents kept, before anything
// is written --, the new rows' vectors / labels / zeroed lists behind the rows in use (no search reads there), launch_hnsw_build
// from row ntotal, and only then the counts, the header fields and the level stream.  A failure before the first kernel leaves the
// handle as it was; one after it (a launch that failed, a candidate queue that overflowed) has rewritten some link lists: broken.
static int hnsw_grow(DevBuf &b, size_t bytes, size_t keep, hipStream_t st)
{
    if (bytes <= b.cap) return CVTMI_OK;
    if (2 * b.cap > bytes && b.grow(2 * b.cap, keep, st) == CVTMI_OK) return CVTMI_OK;   // geometric; where that does not fit, what is needed
    return b.grow(bytes, keep, st);
}

static int hnsw_add_impl(cvtmi_hnsw_t h, const float *x, bool dev, int64_t m, const uint64_t *labels, int max_batch, hipStream_t st)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_hnsw_add: null handle");
    if (m < 0 || max_batch < 0 || (m > 0 && !x))
        return fail(CVTMI_EINVAL, "cvtmi_hnsw_add: bad arguments (m >= 0, max_batch >= 0, rows for m > 0)");
    CHECK_HN(h);
    std::unique_lock<std::shared_timed_mutex> wr(h->rw);
    if (m == 0) return CVTMI_OK;
    const int64_t n0 = h->g.n, n1 = n0 + m;
    const int D = h->D, maxM = h->g.maxM, maxM0 = h->g.maxM0;
    if (maxM0 > 64 || maxM > maxM0 || maxM < 1)
        return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_add: maxM=%d, maxM0=%d (a list of at most 64 links is one wave, and maxM <= maxM0)", maxM, maxM0);
    if (h->M < 1 || h->M > (uint64_t)maxM) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_add: M=%llu outside 1..maxM=%d", (unsigned long long)h->M, maxM);
    if (h->efc < 1 || h->efc > (uint64_t)hnsw_ef_max())
        return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_add: ef_construction=%llu outside 1..%d", (unsigned long long)h->efc, hnsw_ef_max());
    if (n1 > 0x7fffffffLL) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_add: %lld + %lld rows: too many", (long long)n0, (long long)m);
    if (D > 4096) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_add: D=%d > 4096", D);
    if (!(h->mult >= 0.0 && h->mult <= 16.0)) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_add: level multiplier %g outside 0..16", h->mult);
    std::vector<int32_t> lv;
    std::vector<int64_t> uoff, lab;
    std::default_random_engine rng = h->level_rng;
    int64_t uw = h->upper_words;
    int32_t top = n0 > 0 ? h->g.maxlevel : 0;
    uint32_t ep = h->g.enterpoint;
    try {
        lv.resize((size_t)m);
        uoff.assign((size_t)m, -1);
        std::uniform_real_distribution<double> u01(0.0, 1.0);
        for (int64_t i = 0; i < m; ++i) {
            lv[(size_t)i] = (int32_t)(-log(u01(rng)) * h->mult);
            if (lv[(size_t)i] > 0) { uoff[(size_t)i] = uw; uw += (int64_t)lv[(size_t)i] * (maxM + 1); }
            if ((n0 == 0 && i == 0) || lv[(size_t)i] > top) { top = lv[(size_t)i]; ep = (uint32_t)(n0 + i); }
        }
        if (!labels) { lab.resize((size_t)m); for (int64_t i = 0; i < m; ++i) lab[(size_t)i] = n0 + i; }
        h->levels.reserve((size_t)n1);   // (the append below cannot fail any more)
    } catch (const std::exception &) {
        return fail(CVTMI_ENOMEM, "cvtmi_hnsw_add: out of host memory for %lld rows", (long long)m);
    }
    // searches still in flight on other streams read the buffers that growing frees
    h->pool.mutation_begin(st);
    const size_t l0w = (size_t)maxM0 + 1;
    int rc = hnsw_grow(h->vec, (size_t)n1 * D * 4, (size_t)n0 * D * 4, st);
    if (rc == CVTMI_OK) rc = hnsw_grow(h->links0, (size_t)n1 * l0w * 4, (size_t)n0 * l0w * 4, st);
    if (rc == CVTMI_OK) rc = hnsw_grow(h->labels, (size_t)n1 * 8, (size_t)n0 * 8, st);
    if (rc == CVTMI_OK) rc = hnsw_grow(h->upper_off, (size_t)n1 * 8, (size_t)n0 * 8, st);
    if (rc == CVTMI_OK) rc = hnsw_grow(h->upper, (size_t)(uw ? uw : 4) * 4, (size_t)h->upper_words * 4, st);
    const size_t dw0 = (size_t)((n0 + 63) / 64), dw1 = (size_t)((n1 + 63) / 64);   // the delete bitmap: contents kept, new rows arrive live
    if (rc == CVTMI_OK) rc = hnsw_grow(h->dead, dw1 * 8, dw0 * 8, st);
    // (a buffer that grew before another failed holds what it held, at a new address)
    h->g.vec = h->vec.as<float>(); h->g.links0 = h->links0.as<uint32_t>(); h->g.labels = h->labels.as<int64_t>();
    h->g.upper_off = h->upper_off.as<int64_t>(); h->g.upper = h->upper.as<uint32_t>();
    if (rc != CVTMI_OK) return rc;
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    bool launched = false;
    int64_t stats[2] = { 0, 0 };
    auto run = [&]() -> int {
        CVTMI_HIP(hipMemcpyAsync(h->vec.as<float>() + (size_t)n0 * D, x, (size_t)m * D * 4, in, st));
        CVTMI_HIP(hipMemsetAsync(h->links0.as<uint32_t>() + (size_t)n0 * l0w, 0, (size_t)m * l0w * 4, st));
        if (uw > h->upper_words) CVTMI_HIP(hipMemsetAsync(h->upper.as<uint32_t>() + h->upper_words, 0, (size_t)(uw - h->upper_words) * 4, st));
        if (labels) CVTMI_HIP(hipMemcpyAsync(h->labels.as<int64_t>() + n0, labels, (size_t)m * 8, in, st));
        else CVTMI_HIP(hipMemcpyAsync(h->labels.as<int64_t>() + n0, lab.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
        CVTMI_HIP(hipMemcpyAsync(h->upper_off.as<int64_t>() + n0, uoff.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
        if (dw1 > dw0) CVTMI_HIP(hipMemsetAsync(h->dead.as<uint64_t>() + dw0, 0, (dw1 - dw0) * 8, st));   // (the bits past n0 in word dw0 - 1 are zero already)
        HnswDevGraph g1 = h->g;
        g1.n = n1;
        CVTMI_TRY(launch_hnsw_build("cvtmi_hnsw_add", g1, h->links0.as<uint32_t>(), h->upper.as<uint32_t>(), lv.data(), n0, h->g.enterpoint,
                                    h->g.maxlevel, h->metric, (int)h->M, (int)h->efc, max_batch, h->cus, st, stats, &launched,
                                    h->n_dead > 0 ? h->dead.as<uint64_t>() : nullptr));
        CVTMI_HIP(hipStreamSynchronize(st));   // (a call that only seeds launches nothing: the copies above still read host vectors)
        return CVTMI_OK;
    };
    rc = run();
    if (rc != CVTMI_OK) {
        const std::string why = g_err;
        (void)hipStreamSynchronize(st);
        if (launched) h->broken = true;
        return fail(rc, "%s%s", why.c_str(), launched ? " -- the graph is incomplete: the handle is broken, destroy it" : "");
    }
    h->levels.insert(h->levels.end(), lv.begin(), lv.end());
    h->g.n = n1; h->g.maxlevel = top; h->g.enterpoint = ep;
    h->hdr_maxlevel = top; h->hdr_enterpoint = ep;
    h->upper_words = uw;
    h->level_rng = rng; h->level_draws += m;
    if (h->max_elements < (uint64_t)n1) h->max_elements = (uint64_t)n1;
    h->add_last[0] = n0; h->add_last[1] = stats[0]; h->add_last[2] = stats[1]; h->add_last[3] = (int64_t)h->max_elements;
    h->pool.mutation_end(st);
    return CVTMI_OK;
}

int cvtmi_hnsw_add(cvtmi_hnsw_t h, const float *x, int64_t m, const uint64_t *labels, int max_batch)
{
    return hnsw_add_impl(h, x, false, m, labels, max_batch, nullptr);
}
int cvtmi_hnsw_add_dev(cvtmi_hnsw_t h, const float *x, int64_t m, const uint64_t *labels, int max_batch, void *stream)
{
    return hnsw_add_impl(h, x, true, m, labels, max_batch, (hipStream_t)stream);
}

int cvtmi_hnsw_reserve(cvtmi_hnsw_t h, int64_t max_elements)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_hnsw_reserve: null handle");
    if (max_elements < 0) return fail(CVTMI_EINVAL, "cvtmi_hnsw_reserve: negative max_elements");
    CHECK_HN(h);
    if (max_elements > 0x7fffffffLL) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_reserve: max_elements too large");
    std::unique_lock<std::shared_timed_mutex> wr(h->rw);
    if ((uint64_t)max_elements > h->max_elements) h->max_elements = (uint64_t)max_elements;   // (never lowered; device storage follows the rows, not this)
    return CVTMI_OK;
}

int cvtmi_hnsw_level_draws(cvtmi_hnsw_t h, int64_t *draws)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_hnsw_level_draws: null handle");
    if (!draws) return fail(CVTMI_EINVAL, "cvtmi_hnsw_level_draws: null pointer");
    CHECK_HN(h);
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    *draws = h->level_draws;
    return CVTMI_OK;
}

// re-seed and draw: a draw is one call of the distribution, however many engine steps libstdc++ spends on it
int cvtmi_hnsw_set_level_draws(cvtmi_hnsw_t h, int64_t draws)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_hnsw_set_level_draws: null handle");
    if (draws < 0) return fail(CVTMI_EINVAL, "cvtmi_hnsw_set_level_draws: negative count");
    CHECK_HN(h);
    std::unique_lock<std::shared_timed_mutex> wr(h->rw);
    std::default_random_engine rng(100);
    std::uniform_real_distribution<double> u01(0.0, 1.0);
    for (int64_t i = 0; i < draws; ++i) (void)u01(rng);
    h->level_rng = rng; h->level_draws = draws;
    return CVTMI_OK;
}

int cvtmi_hnsw_last_add(cvtmi_hnsw_t h, int64_t out[4])
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_hnsw_last_add: null handle");
    if (!out) return fail(CVTMI_EINVAL, "cvtmi_hnsw_last_add: null pointer");
    CHECK_HN(h);
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    for (int i = 0; i < 4; ++i) out[i] = h->add_last[i];
    return CVTMI_OK;
}

// saveIndex (:491-519): header, max_elements level-0 blocks (links, vector, label), then per element the size of its upper-level
// block and the block.  Slots past cur_element_count are written as zeros.
int cvtmi_hnsw_save(cvtmi_hnsw_t h, void *buf, int64_t cap, int64_t *bytes)
{
    CHECK_HN(h);
    if (!bytes) return fail(CVTMI_EINVAL, "cvtmi_hnsw_save: null size pointer");
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    const int64_t n = h->g.n;
    const uint64_t maxM = (uint64_t)h->g.maxM, maxM0 = (uint64_t)h->g.maxM0, D = (uint64_t)h->D;
    const uint64_t link0 = 4 + 4 * maxM0, per = link0 + 4 * D + 8, upb = 4 * maxM + 4;
    uint64_t total = 96 + h->max_elements * per + 4 * h->max_elements;
    for (int64_t i = 0; i < n; ++i) total += upb * (uint64_t)h->levels[(size_t)i];
    *bytes = (int64_t)total;
    if (!buf) return CVTMI_OK;
    if (cap < (int64_t)total) return fail(CVTMI_EINVAL, "cvtmi_hnsw_save: buffer of %lld bytes, the file needs %lld", (long long)cap,
                                          (long long)total);
    std::vector<uint32_t> links0, upper;
    std::vector<float> vec;
    std::vector<int64_t> labels, uoff;
    std::vector<uint64_t> dead;
    size_t upper_words = 0;
    for (int64_t i = 0; i < n; ++i) upper_words += (size_t)h->levels[(size_t)i] * (maxM + 1);
    try {
        links0.resize((size_t)n * (maxM0 + 1)); vec.resize((size_t)n * D); labels.resize((size_t)n); uoff.resize((size_t)n);
        upper.resize(upper_words);
        if (h->n_dead > 0) dead.resize((size_t)((n + 63) / 64));
    } catch (const std::exception &) {
        return fail(CVTMI_ENOMEM, "cvtmi_hnsw_save: out of host memory");
    }
    if (n) {
        CVTMI_HIP(hipMemcpy(links0.data(), h->links0.p, links0.size() * 4, hipMemcpyDeviceToHost));
        CVTMI_HIP(hipMemcpy(vec.data(), h->vec.p, vec.size() * 4, hipMemcpyDeviceToHost));
        CVTMI_HIP(hipMemcpy(labels.data(), h->labels.p, labels.size() * 8, hipMemcpyDeviceToHost));
        CVTMI_HIP(hipMemcpy(uoff.data(), h->upper_off.p, uoff.size() * 8, hipMemcpyDeviceToHost));
        if (upper_words) CVTMI_HIP(hipMemcpy(upper.data(), h->upper.p, upper_words * 4, hipMemcpyDeviceToHost));
        if (!dead.empty()) CVTMI_HIP(hipMemcpy(dead.data(), h->dead.p, dead.size() * 8, hipMemcpyDeviceToHost));
    }
    // hnswlib's DELETE_MARK: bit 16 of a dead node's level-0 count word; a graph without dead nodes writes the bytes it always wrote
    for (size_t w = 0; w < dead.size(); ++w)
        for (uint64_t b = dead[w]; b; b &= b - 1) links0[(w * 64 + (size_t)__builtin_ctzll(b)) * (maxM0 + 1)] |= 1u << 16;
    uint8_t *p = static_cast<uint8_t *>(buf);
    auto put = [&](const void *src, size_t nb) { memcpy(p, src, nb); p += nb; };
    const uint64_t zero = 0, cnt = (uint64_t)n, offd = link0, offl = link0 + 4 * D;
    put(&zero, 8); put(&h->max_elements, 8); put(&cnt, 8); put(&per, 8); put(&offl, 8); put(&offd, 8);
    put(&h->hdr_maxlevel, 4); put(&h->hdr_enterpoint, 4);
    put(&maxM, 8); put(&maxM0, 8); put(&h->M, 8); put(&h->mult, 8); put(&h->efc, 8);
    for (int64_t i = 0; i < n; ++i) {
        put(&links0[(size_t)i * (maxM0 + 1)], link0);
        put(&vec[(size_t)i * D], 4 * D);
        put(&labels[(size_t)i], 8);
    }
    memset(p, 0, (size_t)((h->max_elements - (uint64_t)n) * per));
    p += (h->max_elements - (uint64_t)n) * per;
    for (uint64_t i = 0; i < h->max_elements; ++i) {
        const uint32_t sz = (int64_t)i < n ? (uint32_t)(upb * (uint64_t)h->levels[(size_t)i]) : 0u;
        put(&sz, 4);
        if (sz) put(&upper[(size_t)uoff[(size_t)i]], sz);
    }
    return CVTMI_OK;
}

int cvtmi_hnsw_destroy(cvtmi_hnsw_t h)
{
    if (!h) return CVTMI_OK;
    if (h->magic != 0x484e5357u) return fail(CVTMI_EINVAL, "bad hnsw handle");
    CVTMI_TRY(use_device(h->device));   // (a handle cvtmi_hnsw_add left broken is destroyed like any other)
    h->vec.release(); h->links0.release(); h->labels.release(); h->upper_off.release(); h->upper.release(); h->dead.release();
    (void)hipDeviceSynchronize();   // searches still in flight on other streams read the graph
    h->pool.destroy();
    h->magic = 0;
    delete h;
    return CVTMI_OK;
}

int64_t cvtmi_hnsw_ntotal(cvtmi_hnsw_t h) { return (h && h->magic == 0x484e5357u && !h->broken) ? h->g.n : -1; }

// scratch of one traversal launch: `slots` concurrent queries (one wave each), a visited bit per node and the spilled queues per slot
struct HnswPlan { int slots; int64_t words, gcap; };
// Scratch a masked search may reserve (visited bits + queues of all its slots).  A masked slot holds a candidate queue of n entries
// (8 n bytes, below), 256 times the unmasked bound at 1 M nodes and ef = 64; at 32 slots per CU that would be 65 GB.  8 GiB keeps
// about 1000 traversals in flight at 1 M nodes (4 per CU) and every traversal of a graph of up to 120 K nodes, and leaves the
// rest of the 288 GB to the index itself and to the other searches of the handle, each of which leases a set of its own.
constexpr size_t kHnswMaskedScratch = (size_t)8 << 30;
// masked_form >= 0: the plan of a masked search (form as cvtmi_hnsw_last_masked reports it)
static int hnsw_plan(cvtmi_hnsw_t h, HnswScratch &S, int lds_dim, int64_t nq, int k, int ef, HnswPlan &pl, hipStream_t st, int masked_form = -1)
{
    const int efe = ef > k ? ef : k;
    int per_cu = (159 * 1024) / hnsw_lds_bytes(lds_dim, efe);  // query slots (one wave each) a CU's 160 KB of LDS hold
    per_cu = per_cu > 32 ? 32 : (per_cu < 1 ? 1 : per_cu);
    if (const int cap = tune_hnsw_slots.geti(); cap > 0 && per_cu > cap) per_cu = cap;   // cvtmi_set_tuning("hnsw_slots"): measurement hook
    // (filling the rounds of a batch evenly with fewer slots per CU was measured: no effect -- throughput grows with the traversals in
    //  flight all the way to 32 per CU: 12 / 16 / 20 / 24 / 28 / 32 slots -> 144 / 164 / 178 / 184 / 192 / 201 K queries/s over codes at ef = 1000)
    pl.slots = h->cus * per_cu;
    if (pl.slots > nq) pl.slots = (int)nq;
    pl.words = (h->g.n + 31) / 32 + 1;
    int64_t gcap = (int64_t)efe * h->g.maxM0 * 2;
    if (gcap > h->g.n) gcap = h->g.n;
    // Under a mask that bound does not hold: while few allowed nodes have been found nothing is pruned and every visited node is queued
    // (measured on the CPU model, (k, ef) = (10, 16), sparse masks: 622 - 1554 entries against 2 ef maxM0 = 384 / 512).  A node enters
    // the queue at most once, so n entries are always enough and the overflow check behind the launch stays a guard.
    if (masked_form >= 0) gcap = h->g.n;
    gcap = gcap > hnsw_lcap() ? gcap - hnsw_lcap() : 0;
    pl.gcap = gcap + 64;
    if (masked_form >= 0) {
        const size_t per_slot = (size_t)pl.words * 4 + (size_t)(pl.gcap + efe + 1) * 8;
        const int64_t fit = std::max<int64_t>(1, (int64_t)(kHnswMaskedScratch / per_slot));
        if (pl.slots > fit) pl.slots = (int)fit;
        std::lock_guard<std::mutex> g(h->pool.mu);
        h->masked_last[0] = pl.slots; h->masked_last[1] = hnsw_lcap() + pl.gcap;
        h->masked_last[2] = (int64_t)(per_slot * (size_t)pl.slots); h->masked_last[3] = masked_form;
    }
    CVTMI_TRY(S.s_vis.reserve((size_t)pl.slots * pl.words * 4));
    CVTMI_TRY(S.s_cand.reserve((size_t)pl.slots * (pl.gcap + efe + 1) * 8));  // per slot: spilled top queue + spilled candidates
    CVTMI_TRY(S.s_err.reserve(16));
    CVTMI_HIP(hipMemsetAsync(S.s_err.p, 0, 8, st));  // [0] overflow flag, [1] query counter
    return CVTMI_OK;
}
static int hnsw_check_overflow(HnswScratch &S, const char *who, int ef, hipStream_t st)
{
    int err = 0;
    CVTMI_HIP(hipMemcpyAsync(&err, S.s_err.p, 4, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    if (err) return fail(CVTMI_EUNSUPPORTED, "%s: candidate queue overflow (ef=%d)", who, ef);
    return CVTMI_OK;
}

// A handle with dead nodes (cvtmi_hnsw_mark_deleted) answers every search through the MASKED kernels: hnswlib's rule for a deleted node
// is the rule for a node the mask forbids.  The mask is what the caller allows (everything, on the unmasked entries) without the
// dead nodes, formed in the leased set; the caller's words are only read.  n_dead == 0: nothing happens here, the mask stays the caller's.
static int hnsw_live_mask(cvtmi_hnsw_t h, HnswScratch &S, const uint64_t *&mask, hipStream_t st)
{
    if (h->n_dead == 0 || h->g.n == 0) return CVTMI_OK;
    CVTMI_TRY(S.s_live.reserve((size_t)((h->g.n + 63) / 64) * 8));
    CVTMI_TRY(launch_hnsw_live_mask(h->dead.as<uint64_t>(), mask, S.s_live.as<uint64_t>(), h->g.n, st));
    mask = S.s_live.as<uint64_t>();
    return CVTMI_OK;
}

// mask (device pointer, ceil(n / 64) words) != null: the masked search
static int hnsw_search_leased(cvtmi_hnsw_t h, HnswScratch &S, const float *q, int64_t nq, int k, int ef, float *dist, int64_t *labels, hipStream_t st,
                              const uint64_t *mask = nullptr)
{
    HnswPlan pl;
    CVTMI_TRY(hnsw_live_mask(h, S, mask, st));
    CVTMI_TRY(hnsw_plan(h, S, h->D, nq, k, ef, pl, st, mask ? 0 : -1));
    CVTMI_TRY(launch_hnsw_search(h->g, h->metric, q, nq, k, ef, dist, labels, S.s_vis.as<uint32_t>(), S.s_cand.p, pl.slots, pl.words,
                                 pl.gcap, S.s_err.as<int>(), st, mask));
    return hnsw_check_overflow(S, mask ? "cvtmi_hnsw_search_masked" : "cvtmi_hnsw_search", ef, st);
}

static int hnsw_search_args(cvtmi_hnsw_t h, const char *who, const void *q, int64_t nq, int k, int ef, const void *dist, const void *labels)
{
    (void)h;
    if (nq < 0 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "%s: bad arguments", who);
    if (k < 1 || k > hnsw_ef_max()) return fail(CVTMI_EUNSUPPORTED, "%s: k=%d outside 1..%d", who, k, hnsw_ef_max());
    if (ef < 1 || ef > hnsw_ef_max()) return fail(CVTMI_EUNSUPPORTED, "%s: ef=%d outside 1..%d", who, ef, hnsw_ef_max());
    if (nq > 0x7fffffff) return fail(CVTMI_EUNSUPPORTED, "%s: nq too large", who);
    return CVTMI_OK;
}

int cvtmi_hnsw_search_dev(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, int ef, float *dist, int64_t *labels, void *stream)
{
    CHECK_HN(h);
    CVTMI_TRY(hnsw_search_args(h, "cvtmi_hnsw_search", q, nq, k, ef, dist, labels));
    if (nq == 0) return CVTMI_OK;
    HnswLease lease;
    CVTMI_TRY(lease.open(h, (hipStream_t)stream, false));
    return hnsw_search_leased(h, *lease.s, q, nq, k, ef, dist, labels, lease.st);
}

// The host-pointer entries: queries in and [nq][k] distances and labels out, staged through the leased set's own buffers on its own
// stream (host_call); masked: with the mask words that can hold a node beside the queries (the caller's words behind them are never read)
template <typename F> static int hnsw_host_search(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, const uint64_t *mask, float *dist, int64_t *labels, F &&run)
{
    HnswLease lease;
    CVTMI_TRY(lease.open(h, nullptr, true));
    const HostUpload words = mask ? HostUpload{ &lease.s->io_m, mask, (size_t)((h->g.n + 63) / 64) * 8 } : HostUpload{};
    return host_call(lease, q, (size_t)nq * h->D * sizeof(float), words, dist, (size_t)nq * k * 4, labels, (size_t)nq * k * 8, run);
}

int cvtmi_hnsw_search(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, int ef, float *dist, int64_t *labels)
{
    CHECK_HN(h);
    CVTMI_TRY(hnsw_search_args(h, "cvtmi_hnsw_search", q, nq, k, ef, dist, labels));
    if (nq == 0) return CVTMI_OK;
    return hnsw_host_search(h, q, nq, k, nullptr, dist, labels, [&](HnswScratch &S, const float *dq, const void *, float *dd, int64_t *dl, hipStream_t st) {
        return hnsw_search_leased(h, S, dq, nq, k, ef, dd, dl, st);
    });
}

// HNSW over OPQ-compressed vectors: the graph of `h`, distances = ADC over the codes held by `opq` (one code
// row per graph node, appended in internal-id order).  Queries are rotated and their tables built by the OPQ
// handle's own kernels, into a scratch set leased from the OPQ handle (so a later cvtmi_opq_add waits for this search);
// the OPQ handle is held shared for the duration, like a search of its own.
static int hnsw_search_adc_leased(cvtmi_hnsw_t h, HnswScratch &S, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                                  float *dist, int64_t *labels, hipStream_t st, int raw_ids, const uint64_t *mask = nullptr)
{
    if (!opq) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc: null OPQ handle");
    CVTMI_TRY(hnsw_search_args(h, mask ? "cvtmi_hnsw_search_adc_masked" : "cvtmi_hnsw_search_adc", q, nq, k, ef, dist, labels));
    if (opq->m.coarseK != 1) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_search_adc: needs an OPQ model with coarseK == 1");
    if (opq->m.D != h->D) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc: OPQ model is %d-d, graph is %d-d", opq->m.D, h->D);
    if (opq->device != h->device) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc: handles live on different devices");
    if (nq == 0) return CVTMI_OK;
    std::shared_lock<std::shared_timed_mutex> rd(opq->rw);
    if (opq->n != h->g.n) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc: %lld code rows for %lld graph nodes", (long long)opq->n,
                                      (long long)h->g.n);
    OpqLease ol;
    CVTMI_TRY(ol.open(opq, st, false));
    OpqScratch &OS = *ol.s;
    const float *q_rot = nullptr;
    CVTMI_TRY(opq_rotate_probe(opq, OS, q, nq, rotate, 0, st, &q_rot));
    CVTMI_TRY(OS.s_lut.reserve((size_t)nq * opq->m.M * opq->m.K * sizeof(float)));
    CVTMI_TRY(launch_lut(opq->m, q_rot, nq, nullptr, OS.s_lut.as<float>(), st));
    CVTMI_TRY(hnsw_live_mask(h, S, mask, st));
    HnswPlan pl;
    const int state_floats = hnsw_adc_state_floats(opq->m.M * opq->m.K);   // one reading of the tuning flag for the slot count AND the launch
    CVTMI_TRY(hnsw_plan(h, S, state_floats, nq, k, ef, pl, st, mask ? (state_floats ? 2 : 1) : -1));
    CVTMI_TRY(launch_hnsw_search_adc(h->g, OS.s_lut.as<float>(), opq->codes.as<uint8_t>(), opq->m.M, opq->m.K, nq, k, ef, dist,
                                     labels, S.s_vis.as<uint32_t>(), S.s_cand.p, pl.slots, pl.words, pl.gcap, S.s_err.as<int>(), st, raw_ids,
                                     state_floats, mask));
    return hnsw_check_overflow(S, mask ? "cvtmi_hnsw_search_adc_masked" : "cvtmi_hnsw_search_adc", ef, st);
}

int cvtmi_hnsw_search_adc_dev(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef, float *dist,
                              int64_t *labels, void *stream)
{
    CHECK_HN(h);
    HnswLease lease;
    CVTMI_TRY(lease.open(h, (hipStream_t)stream, false));
    return hnsw_search_adc_leased(h, *lease.s, opq, q, nq, rotate, k, ef, dist, labels, lease.st, 0);
}

// ADC traversal with a result list of `rerank` nodes, then their exact fp32 distances (the graph's own vectors, the summation
// order of the reference's distance functions) and the k smallest; equal exact distances keep their ADC order
static int hnsw_search_adc_rerank_leased(cvtmi_hnsw_t h, HnswScratch &S, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef,
                                         int rerank, float *dist, int64_t *labels, hipStream_t st, const uint64_t *mask = nullptr)
{
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_hnsw_search_adc_rerank: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (rerank < k || rerank > hnsw_ef_max()) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc_rerank: rerank=%d outside k..%d", rerank, hnsw_ef_max());
    if (nq < 0 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc_rerank: bad arguments");
    if (nq == 0) return CVTMI_OK;
    CVTMI_TRY(S.s_rr_d.reserve((size_t)nq * rerank * sizeof(float)));
    CVTMI_TRY(S.s_rr_id.reserve((size_t)nq * rerank * sizeof(int64_t)));
    CVTMI_TRY(hnsw_search_adc_leased(h, S, opq, q, nq, rotate, rerank, ef, S.s_rr_d.as<float>(), S.s_rr_id.as<int64_t>(), st, 1, mask));
    CVTMI_TRY(launch_hnsw_rerank(h->g, h->metric, q, nq, rerank, S.s_rr_id.as<int64_t>(), S.s_rr_d.as<float>(), st));
    CVTMI_TRY(launch_topk_select(S.s_rr_d.as<float>(), S.s_rr_id.as<int64_t>(), nq, rerank, k, dist, labels, st));
    return launch_gather_labels(labels, nq * k, h->g.labels, st);
}

int cvtmi_hnsw_search_adc_rerank_dev(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef, int rerank,
                                     float *dist, int64_t *labels, void *stream)
{
    CHECK_HN(h);
    HnswLease lease;
    CVTMI_TRY(lease.open(h, (hipStream_t)stream, false));
    return hnsw_search_adc_rerank_leased(h, *lease.s, opq, q, nq, rotate, k, ef, rerank, dist, labels, lease.st);
}

int cvtmi_hnsw_search_adc_rerank(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef, int rerank,
                                 float *dist, int64_t *labels)
{
    CHECK_HN(h);
    if (nq < 0 || k < 1 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc_rerank: bad arguments");
    if (nq == 0) return CVTMI_OK;
    return hnsw_host_search(h, q, nq, k, nullptr, dist, labels, [&](HnswScratch &S, const float *dq, const void *, float *dd, int64_t *dl, hipStream_t st) {
        return hnsw_search_adc_rerank_leased(h, S, opq, dq, nq, rotate, k, ef, rerank, dd, dl, st);
    });
}

int cvtmi_hnsw_search_adc(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef, float *dist,
                          int64_t *labels)
{
    CHECK_HN(h);
    if (nq < 0 || k < 1 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc: bad arguments");
    if (nq == 0) return CVTMI_OK;
    return hnsw_host_search(h, q, nq, k, nullptr, dist, labels, [&](HnswScratch &S, const float *dq, const void *, float *dd, int64_t *dl, hipStream_t st) {
        return hnsw_search_adc_leased(h, S, opq, dq, nq, rotate, k, ef, dd, dl, st, 0);
    });
}

// ================================================================ masked search ================
// The entries above under a node mask (hnsw.hip: the MASKED instances).  Same leases, same streams, same argument answers; the mask
// is checked first, and the host-pointer entries stage its ceil(n / 64) words through the leased set beside the queries.
#define CHECK_HN_MASKED(h) do { if (!(h)) return fail(CVTMI_EINVAL, "%s: null handle", __func__); CHECK_HN(h); } while (0)

static int hnsw_mask_args(cvtmi_hnsw_t h, const char *who, const void *q, int64_t nq, const uint64_t *mask, int64_t mask_words, const void *dist,
                          const void *labels)
{
    if (nq < 0 || mask_words < 0 || (nq > 0 && (!q || !mask || !dist || !labels))) return fail(CVTMI_EINVAL, "%s: bad arguments", who);
    if (mask_words < (h->g.n + 63) / 64)
        return fail(CVTMI_EINVAL, "%s: %lld mask words for %lld nodes (%lld needed)", who, (long long)mask_words, (long long)h->g.n,
                    (long long)((h->g.n + 63) / 64));
    return CVTMI_OK;
}

extern "C" {

int cvtmi_hnsw_search_masked_dev(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, int ef, const uint64_t *mask, int64_t mask_words,
                                 float *dist, int64_t *labels, void *stream)
{
    CHECK_HN_MASKED(h);
    CVTMI_TRY(hnsw_mask_args(h, "cvtmi_hnsw_search_masked", q, nq, mask, mask_words, dist, labels));
    CVTMI_TRY(hnsw_search_args(h, "cvtmi_hnsw_search_masked", q, nq, k, ef, dist, labels));
    if (nq == 0) return CVTMI_OK;
    HnswLease lease;
    CVTMI_TRY(lease.open(h, (hipStream_t)stream, false));
    return hnsw_search_leased(h, *lease.s, q, nq, k, ef, dist, labels, lease.st, mask);
}

int cvtmi_hnsw_search_masked(cvtmi_hnsw_t h, const float *q, int64_t nq, int k, int ef, const uint64_t *mask, int64_t mask_words, float *dist,
                             int64_t *labels)
{
    CHECK_HN_MASKED(h);
    CVTMI_TRY(hnsw_mask_args(h, "cvtmi_hnsw_search_masked", q, nq, mask, mask_words, dist, labels));
    CVTMI_TRY(hnsw_search_args(h, "cvtmi_hnsw_search_masked", q, nq, k, ef, dist, labels));
    if (nq == 0) return CVTMI_OK;
    return hnsw_host_search(h, q, nq, k, mask, dist, labels, [&](HnswScratch &S, const float *dq, const void *dm, float *dd, int64_t *dl, hipStream_t st) {
        return hnsw_search_leased(h, S, dq, nq, k, ef, dd, dl, st, static_cast<const uint64_t *>(dm));
    });
}

int cvtmi_hnsw_search_adc_masked_dev(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef, const uint64_t *mask,
                                     int64_t mask_words, float *dist, int64_t *labels, void *stream)
{
    CHECK_HN_MASKED(h);
    CVTMI_TRY(hnsw_mask_args(h, "cvtmi_hnsw_search_adc_masked", q, nq, mask, mask_words, dist, labels));
    if (nq == 0) return CVTMI_OK;   // (the mask pointer selects the kernel: it is there from here on)
    HnswLease lease;
    CVTMI_TRY(lease.open(h, (hipStream_t)stream, false));
    return hnsw_search_adc_leased(h, *lease.s, opq, q, nq, rotate, k, ef, dist, labels, lease.st, 0, mask);
}

int cvtmi_hnsw_search_adc_masked(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef, const uint64_t *mask,
                                 int64_t mask_words, float *dist, int64_t *labels)
{
    CHECK_HN_MASKED(h);
    CVTMI_TRY(hnsw_mask_args(h, "cvtmi_hnsw_search_adc_masked", q, nq, mask, mask_words, dist, labels));
    if (k < 1) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc_masked: bad arguments");   // as cvtmi_hnsw_search_adc answers it
    if (nq == 0) return CVTMI_OK;
    return hnsw_host_search(h, q, nq, k, mask, dist, labels, [&](HnswScratch &S, const float *dq, const void *dm, float *dd, int64_t *dl, hipStream_t st) {
        return hnsw_search_adc_leased(h, S, opq, dq, nq, rotate, k, ef, dd, dl, st, 0, static_cast<const uint64_t *>(dm));
    });
}

int cvtmi_hnsw_search_adc_rerank_masked_dev(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef, int rerank,
                                            const uint64_t *mask, int64_t mask_words, float *dist, int64_t *labels, void *stream)
{
    CHECK_HN_MASKED(h);
    CVTMI_TRY(hnsw_mask_args(h, "cvtmi_hnsw_search_adc_rerank_masked", q, nq, mask, mask_words, dist, labels));
    if (nq == 0) return CVTMI_OK;
    HnswLease lease;
    CVTMI_TRY(lease.open(h, (hipStream_t)stream, false));
    return hnsw_search_adc_rerank_leased(h, *lease.s, opq, q, nq, rotate, k, ef, rerank, dist, labels, lease.st, mask);
}

int cvtmi_hnsw_search_adc_rerank_masked(cvtmi_hnsw_t h, cvtmi_opq_t opq, const float *q, int64_t nq, int rotate, int k, int ef, int rerank,
                                        const uint64_t *mask, int64_t mask_words, float *dist, int64_t *labels)
{
    CHECK_HN_MASKED(h);
    CVTMI_TRY(hnsw_mask_args(h, "cvtmi_hnsw_search_adc_rerank_masked", q, nq, mask, mask_words, dist, labels));
    if (k < 1) return fail(CVTMI_EINVAL, "cvtmi_hnsw_search_adc_rerank_masked: bad arguments");   // as cvtmi_hnsw_search_adc_rerank answers it
    if (nq == 0) return CVTMI_OK;
    return hnsw_host_search(h, q, nq, k, mask, dist, labels, [&](HnswScratch &S, const float *dq, const void *dm, float *dd, int64_t *dl, hipStream_t st) {
        return hnsw_search_adc_rerank_leased(h, S, opq, dq, nq, rotate, k, ef, rerank, dd, dl, st, static_cast<const uint64_t *>(dm));
    });
}

int cvtmi_hnsw_last_masked(cvtmi_hnsw_t h, int64_t out[4])
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_hnsw_last_masked: null handle");
    if (!out || h->magic != 0x484e5357u) return fail(CVTMI_EINVAL, "cvtmi_hnsw_last_masked: bad arguments");
    if (h->broken) return fail(CVTMI_EINVAL, "cvtmi_hnsw_last_masked: the handle is broken (a cvtmi_hnsw_add failed part-way)");
    copy_last(h->pool, h->masked_last, out);
    return CVTMI_OK;
}

}  // extern "C"

// ---- the bitmap of a label set: the mark step of the flat removal over the graph's labels (flat_remove.hip), on a leased set ----
static int hnsw_mask_labels_check(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, const uint64_t *mask, int64_t mask_words)
{
    if (n_labels < 0 || mask_words < 0 || (n_labels > 0 && !labels) || (mask_words > 0 && !mask)) return fail(CVTMI_EINVAL, "cvtmi_hnsw_mask_labels: bad arguments");
    if (mask_words < (h->g.n + 63) / 64)
        return fail(CVTMI_EINVAL, "cvtmi_hnsw_mask_labels: %lld mask words for %lld nodes (%lld needed)", (long long)mask_words, (long long)h->g.n,
                    (long long)((h->g.n + 63) / 64));
    return CVTMI_OK;
}
// (the table of the set -- sorted_unique: its distinct labels, ascending as int64, the order the mark's lower bound walks -- goes through
//  labels_to_mask on the leased set's s_mark)

extern "C" {

int cvtmi_hnsw_mask_labels_dev(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, uint64_t *mask, int64_t mask_words, void *stream)
{
    CHECK_HN_MASKED(h);
    CVTMI_TRY(hnsw_mask_labels_check(h, labels, n_labels, mask, mask_words));
    if (mask_words == 0) return CVTMI_OK;
    HnswLease lease;
    CVTMI_TRY(lease.open(h, (hipStream_t)stream, false));
    hipStream_t st = lease.st;
    if (h->g.n == 0 || n_labels == 0) {
        CVTMI_HIP(hipMemsetAsync(mask, 0, (size_t)mask_words * 8, st));
        return CVTMI_OK;
    }
    std::vector<int64_t> tab;
    CVTMI_TRY(sorted_unique_dev("cvtmi_hnsw_mask_labels", labels, n_labels, tab, st));
    CVTMI_TRY(labels_to_mask(lease.s->s_mark, h->g.labels, h->g.n, tab.data(), (int64_t)tab.size(), mask, mask_words, st));
    CVTMI_HIP(stream_wait(st));   // (the table leaves host memory that ends with this call)
    return CVTMI_OK;
}

int cvtmi_hnsw_mask_labels(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, uint64_t *mask, int64_t mask_words)
{
    CHECK_HN_MASKED(h);
    CVTMI_TRY(hnsw_mask_labels_check(h, labels, n_labels, mask, mask_words));
    if (mask_words == 0) return CVTMI_OK;
    if (h->g.n == 0 || n_labels == 0) {
        memset(mask, 0, (size_t)mask_words * 8);
        return CVTMI_OK;
    }
    std::vector<int64_t> tab;
    CVTMI_TRY(sorted_unique("cvtmi_hnsw_mask_labels", labels, n_labels, tab));
    HnswLease lease;
    CVTMI_TRY(lease.open(h, nullptr, true));
    HnswScratch &S = *lease.s;
    hipStream_t st = lease.st;
    const int64_t words = (h->g.n + 63) / 64;   // (the words that can hold a node)
    CVTMI_TRY(S.io_m.reserve((size_t)words * 8));
    CVTMI_TRY(labels_to_mask(S.s_mark, h->g.labels, h->g.n, tab.data(), (int64_t)tab.size(), S.io_m.as<uint64_t>(), words, st));
    return mask_host_finish(S.io_m, words, mask, mask_words, st);
}

}  // extern "C"

// ================================================================ deletion =====================
// cvtmi_hnsw_mark_deleted / _unmark_deleted: hnswlib's markDelete over a label set.  The mark step of
// cvtmi_hnsw_mask_labels finds the nodes that carry one of the labels; hnsw_dead_fold_kernel folds them into the handle's bitmap and
// counts the bits that flip.  Mutating and exclusive, like cvtmi_hnsw_add: the scratch set is leased under the handle's exclusive lock
// (Lease, not HnswLease, which would take it shared), the stream first waits for the searches in flight, later searches wait for it.
// labels: a host pointer, or (dev) a device pointer that comes down first, as in cvtmi_hnsw_mask_labels_dev.
static int hnsw_set_deleted(cvtmi_hnsw_t h, const char *who, const int64_t *labels, bool dev, int64_t n_labels, int64_t *changed, int unmark,
                            hipStream_t stream)
{
    if (!h) return fail(CVTMI_EINVAL, "%s: null handle", who);
    if (n_labels < 0 || (n_labels > 0 && !labels)) return fail(CVTMI_EINVAL, "%s: bad arguments (n_labels >= 0, labels for n_labels > 0)", who);
    CHECK_HN(h);
    std::unique_lock<std::shared_timed_mutex> wr(h->rw);
    if (changed) *changed = 0;
    if (n_labels == 0 || h->g.n == 0 || (unmark && h->n_dead == 0)) return CVTMI_OK;
    Lease<HnswScratch> lease;
    CVTMI_TRY(lease.open(h, stream, !dev));
    HnswScratch &S = *lease.s;
    hipStream_t st = lease.st;
    std::vector<int64_t> tab;
    if (dev) CVTMI_TRY(sorted_unique_dev(who, labels, n_labels, tab, st));
    else CVTMI_TRY(sorted_unique(who, labels, n_labels, tab));
    FlatRmPlan p;   // the mark's areas, the table, and one word behind it for the count of flipped bits
    p.rm = rm_plan(h->g.n, 0, 0, 0);
    p.T = (int64_t)tab.size();
    p.off_table = p.rm.off_table;
    const size_t off_flips = p.off_table + rm_align((size_t)p.T * 8);
    p.bytes = off_flips + rm_align(8);
    CVTMI_TRY(S.s_mark.reserve(p.bytes));
    void *W = S.s_mark.p;
    unsigned long long *flips = rm_at<unsigned long long>(W, off_flips);
    h->pool.mutation_begin(st);
    CVTMI_HIP(hipMemcpyAsync(rm_at<char>(W, p.off_table), tab.data(), (size_t)p.T * 8, hipMemcpyHostToDevice, st));
    CVTMI_HIP(hipMemsetAsync(flips, 0, 8, st));
    CVTMI_TRY(launch_flat_rm_mark_labels(p, W, h->g.labels, st));
    // (the marked bitmap holds ntiles * kRmWords >= ceil(n / 64) words and no bit past the nodes: the tail of `dead` stays zero)
    CVTMI_TRY(launch_hnsw_dead_fold(rm_at<uint64_t>(W, p.rm.off_drop), h->dead.as<uint64_t>(), (h->g.n + 63) / 64, unmark, flips, st));
    unsigned long long f = 0;
    CVTMI_HIP(hipMemcpyAsync(&f, flips, 8, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));   // (the table and the count live in host memory that ends with this call)
    h->n_dead += unmark ? -(int64_t)f : (int64_t)f;
    h->pool.mutation_end(st);
    if (changed) *changed = (int64_t)f;
    return CVTMI_OK;
}

static int hnsw_get_deleted_impl(cvtmi_hnsw_t h, uint64_t *mask, int64_t mask_words, bool dev, hipStream_t stream)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_hnsw_get_deleted: null handle");
    if (mask_words < 0 || (mask_words > 0 && !mask)) return fail(CVTMI_EINVAL, "cvtmi_hnsw_get_deleted: bad arguments");
    CHECK_HN(h);
    HnswLease lease;
    CVTMI_TRY(lease.open(h, stream, !dev));
    const int64_t words = (h->g.n + 63) / 64;
    if (mask_words < words)
        return fail(CVTMI_EINVAL, "cvtmi_hnsw_get_deleted: %lld mask words for %lld nodes (%lld needed)", (long long)mask_words, (long long)h->g.n,
                    (long long)words);
    if (mask_words == 0) return CVTMI_OK;
    hipStream_t st = lease.st;
    if (dev) {
        if (words) CVTMI_HIP(hipMemcpyAsync(mask, h->dead.p, (size_t)words * 8, hipMemcpyDeviceToDevice, st));
        if (mask_words > words) CVTMI_HIP(hipMemsetAsync(mask + words, 0, (size_t)(mask_words - words) * 8, st));
        return CVTMI_OK;
    }
    if (words) CVTMI_HIP(hipMemcpyAsync(mask, h->dead.p, (size_t)words * 8, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    memset(mask + words, 0, (size_t)(mask_words - words) * 8);
    return CVTMI_OK;
}

extern "C" {

int cvtmi_hnsw_mark_deleted(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, int64_t *changed)
{
    return hnsw_set_deleted(h, "cvtmi_hnsw_mark_deleted", labels, false, n_labels, changed, 0, nullptr);
}
int cvtmi_hnsw_mark_deleted_dev(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, int64_t *changed, void *stream)
{
    return hnsw_set_deleted(h, "cvtmi_hnsw_mark_deleted", labels, true, n_labels, changed, 0, (hipStream_t)stream);
}
int cvtmi_hnsw_unmark_deleted(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, int64_t *changed)
{
    return hnsw_set_deleted(h, "cvtmi_hnsw_unmark_deleted", labels, false, n_labels, changed, 1, nullptr);
}
int cvtmi_hnsw_unmark_deleted_dev(cvtmi_hnsw_t h, const int64_t *labels, int64_t n_labels, int64_t *changed, void *stream)
{
    return hnsw_set_deleted(h, "cvtmi_hnsw_unmark_deleted", labels, true, n_labels, changed, 1, (hipStream_t)stream);
}

int cvtmi_hnsw_deleted_count(cvtmi_hnsw_t h, int64_t *count)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_hnsw_deleted_count: null handle");
    if (!count) return fail(CVTMI_EINVAL, "cvtmi_hnsw_deleted_count: null pointer");
    CHECK_HN(h);
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    *count = h->n_dead;
    return CVTMI_OK;
}

int cvtmi_hnsw_get_deleted(cvtmi_hnsw_t h, uint64_t *mask, int64_t mask_words)
{
    return hnsw_get_deleted_impl(h, mask, mask_words, false, nullptr);
}
int cvtmi_hnsw_get_deleted_dev(cvtmi_hnsw_t h, uint64_t *mask, int64_t mask_words, void *stream)
{
    return hnsw_get_deleted_impl(h, mask, mask_words, true, (hipStream_t)stream);
}

}  // extern "C"
