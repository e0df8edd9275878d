// api_opq.hip -- the OPQ / IVFOPQ handle of the C ABI (include/cvtmi.h): model, encode, add, the list-ordered copy, the exhaustive
// search and its sharded forms, the per-video query, the IVF search, removal, parameters.
#include <string.h>

#include <algorithm>
#include <thread>

#include "api_internal.h"
#include "launch.h"

// the exclusive side: taken by the outermost of the (Serial-ordered) non-search calls of an OPQ handle; the stream first waits for
// the searches that are still in flight on other streams, and the searches that follow wait for this call
struct OpqExclusive {
    cvtmi_opq_s *h;
    hipStream_t st;
    bool own = false;
    OpqExclusive(cvtmi_opq_s *handle, hipStream_t stream) : h(handle), st(stream)
    {
        if (h->sync.depth != 1) return;   // an inner call of this thread: the outermost one holds the lock
        h->rw.lock();
        own = true;
        h->pool.mutation_begin(st);
    }
    ~OpqExclusive()
    {
        if (!own) return;
        h->pool.mutation_end(st);
        h->rw.unlock();
    }
    OpqExclusive(const OpqExclusive &) = delete;
    OpqExclusive &operator=(const OpqExclusive &) = delete;
};

// CHECK_H + the handle's lock and stream ordering (see Serial) for the rest of the enclosing scope
#define CHECK_H_SERIAL(h, stream) \
    CHECK_H(h); \
    Serial serial_##h((h)->sync, (hipStream_t)(stream)); \
    OpqExclusive excl_##h((h), (hipStream_t)(stream))

// Pure reads of the MODEL (rotation matrix / permutation, codebooks: immutable after cvtmi_opq_create) into the caller's own buffers:
// shared, like a search -- they neither drain the searches in flight nor make later searches wait on their stream.  Entries that hold
// this must not call each other (the shared lock is not recursive): they share the *_impl / launch_* functions instead.
#define CHECK_H_SHARED(h) \
    CHECK_H(h); \
    std::shared_lock<std::shared_timed_mutex> rd_##h((h)->rw)

// true when p points into page-locked host memory the device can reach (cvtmi_host_alloc, or the caller's own hipHostMalloc /
// hipHostRegister): such buffers are handed to the copy engines as they are, without the staging copy
static bool host_pinned(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

int cvtmi::opq_rotate_impl(cvtmi_opq_t h, const float *x, int64_t n, float *y, hipStream_t st)
{
    if (h->m.perm) return launch_permute(h->m.perm, h->m.D, x, n, y, st);
    if (h->m.R) return launch_rotate_gemm(h->m.R, h->m.D, x, n, y, st);
    if (n > 0) CVTMI_HIP(hipMemcpyAsync(y, x, (size_t)n * h->m.D * sizeof(float), hipMemcpyDeviceToDevice, st));
    return CVTMI_OK;
}

int cvtmi::opq_rotate_probe(cvtmi_opq_t h, OpqScratch &S, const float *q, int64_t nq, int rotate, int nprobe, hipStream_t st, const float **q_rot)
{
    *q_rot = q;
    if (rotate && (h->m.perm || h->m.R)) {
        CVTMI_TRY(S.s_qrot.reserve((size_t)nq * h->m.D * sizeof(float)));
        CVTMI_TRY(opq_rotate_impl(h, q, nq, S.s_qrot.as<float>(), st));
        *q_rot = S.s_qrot.as<float>();
    }
    if (nprobe == 0) return CVTMI_OK;
    const size_t probe_bytes = ((size_t)nq * nprobe * sizeof(int32_t) + 15) / 16 * 16;
    CVTMI_TRY(S.s_probe.reserve(probe_bytes + coarse_probe_scratch_bytes(nq, nprobe)));
    return launch_coarse_probe(h->m, *q_rot, nq, nprobe, S.s_probe.as<int32_t>(), st, S.s_probe.as<char>() + probe_bytes);
}

extern "C" {

// ================================================================ OPQ =========================
int cvtmi_opq_create(int D, int coarseK, int M, int K, const float *coarse, const float *books, const float *R,
                     const int32_t *perm, cvtmi_opq_t *out)
{
    if (!out) return fail(CVTMI_EINVAL, "cvtmi_opq_create: null out");
    *out = nullptr;
    if (D < 1 || coarseK < 1 || M < 1 || K < 1 || !coarse || !books)
        return fail(CVTMI_EINVAL, "cvtmi_opq_create: bad model shape D=%d coarseK=%d M=%d K=%d", D, coarseK, M, K);
    if (D % M != 0) return fail(CVTMI_EINVAL, "cvtmi_opq_create: D=%d not divisible by M=%d", D, M);
    if (M > 16) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_create: M=%d > 16 (IVFelem::PQindex[16])", M);
    if (K > 256) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_create: K=%d > 256 (codes are uint8)", K);
    if (R && perm) return fail(CVTMI_EINVAL, "cvtmi_opq_create: give R or perm, not both");
    if (perm)
        for (int i = 0; i < D; ++i)
            if (perm[i] < 0 || perm[i] >= D) return fail(CVTMI_EINVAL, "cvtmi_opq_create: perm[%d]=%d out of range", i, perm[i]);
    int dev = 0;
    CVTMI_HIP(hipGetDevice(&dev));
    cvtmi_opq_s *h = new (std::nothrow) cvtmi_opq_s();
    if (!h) return fail(CVTMI_ENOMEM, "cvtmi_opq_create: out of host memory");
    h->device = dev;
    int rc = dev_alloc_copy(&h->d_coarse, coarse, (size_t)coarseK * D);
    if (rc == CVTMI_OK) rc = dev_alloc_copy(&h->d_books, books, (size_t)D * K);
    if (rc == CVTMI_OK && R) rc = dev_alloc_copy(&h->d_R, R, (size_t)D * D);
    if (rc == CVTMI_OK && perm) rc = dev_alloc_copy(&h->d_perm, perm, (size_t)D);
    if (rc != CVTMI_OK) { cvtmi_opq_destroy(h); return rc; }
    h->m.D = D; h->m.coarseK = coarseK; h->m.M = M; h->m.K = K; h->m.step = D / M;
    h->m.coarse = h->d_coarse; h->m.books = h->d_books; h->m.R = h->d_R; h->m.perm = h->d_perm;
    if (M == 16 && K == 256 && coarseK == 1) {   // (what the matrix-core bound filter's operands are made from on first use, adc_mfma.hip)
        try { h->books_h.assign(books, books + (size_t)D * K); } catch (...) { h->mf_state = -1; }
    }
    *out = h;
    return CVTMI_OK;
}

int cvtmi_opq_destroy(cvtmi_opq_t h)
{
    if (!h) return CVTMI_OK;
    (void)hipSetDevice(h->device);
    if (h->d_coarse) (void)hipFree(h->d_coarse);
    if (h->d_books) (void)hipFree(h->d_books);
    if (h->d_R) (void)hipFree(h->d_R);
    if (h->d_perm) (void)hipFree(h->d_perm);
    h->codes.release(); h->lists.release(); h->videos.release(); h->codes_rot.release(); h->codes16.release();
    h->mf_model.release(); h->mf_pack.release(); h->mf_norm.release(); h->mf_stat.release();
    h->csr_codes.release(); h->csr_videos.release(); h->csr_off.release(); h->csr_scratch.release(); h->csr_stats.release(); h->csr_entry.release();
    h->s_qrot.release(); h->s_probe.release(); h->s_rot.release(); h->rm_scratch.release();
    h->pool.destroy();
    for (int e = 0; e < cvtmi_opq_s::kEvRing; ++e) {
        if (h->ev0[e]) (void)hipEventDestroy(h->ev0[e]);
        if (h->ev1[e]) (void)hipEventDestroy(h->ev1[e]);
    }
    h->sync.destroy();
    delete h;
    return CVTMI_OK;
}

int cvtmi_opq_rotate_dev(cvtmi_opq_t h, const float *x, int64_t n, float *y, void *stream)
{
    CHECK_H_SHARED(h);
    if (n < 0 || (n > 0 && (!x || !y))) return fail(CVTMI_EINVAL, "cvtmi_opq_rotate: bad arguments");
    return opq_rotate_impl(h, x, n, y, (hipStream_t)stream);
}

int cvtmi_opq_rotate(cvtmi_opq_t h, const float *x, int64_t n, float *y)
{
    CHECK_H_SHARED(h);
    if (n < 0 || (n > 0 && (!x || !y))) return fail(CVTMI_EINVAL, "cvtmi_opq_rotate: bad arguments");
    if (n == 0) return CVTMI_OK;
    const size_t bytes = (size_t)n * h->m.D * sizeof(float);
    Tmp dx, dy;
    CVTMI_TRY(dx.upload(x, bytes));
    CVTMI_TRY(dy.alloc(bytes));
    CVTMI_TRY(opq_rotate_impl(h, dx.as<float>(), n, dy.as<float>(), nullptr));
    CVTMI_HIP(hipMemcpy(y, dy.p, bytes, hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

int cvtmi_opq_encode_dev(cvtmi_opq_t h, const float *x_rot, int64_t n, int32_t *list_id, uint8_t *codes, void *stream)
{
    CHECK_H_SERIAL(h, stream);
    if (n < 0 || (n > 0 && (!x_rot || !codes))) return fail(CVTMI_EINVAL, "cvtmi_opq_encode: bad arguments");
    if (n == 0) return CVTMI_OK;
    hipStream_t st = (hipStream_t)stream;
    int32_t *lists = list_id;
    if (h->m.coarseK > 1 && !lists) {
        CVTMI_TRY(h->s_probe.reserve((size_t)n * sizeof(int32_t)));
        lists = h->s_probe.as<int32_t>();
    }
    // coarseK == 1: every valid row lands in list 0; the residual is taken against centroid 0 either way, and the
    // matrix-core encode kernel writes the assignment itself
    if (lists && h->m.coarseK == 1 && pq_encode_fuses_lists(h->m, x_rot, n, h->p_encode))
        return launch_pq_encode(h->m, x_rot, n, nullptr, codes, st, h->p_encode, lists);
    if (lists) CVTMI_TRY(launch_coarse_assign(h->m, x_rot, n, lists, st));
    return launch_pq_encode(h->m, x_rot, n, h->m.coarseK > 1 ? lists : nullptr, codes, st, h->p_encode);
}

int cvtmi_opq_encode(cvtmi_opq_t h, const float *x_rot, int64_t n, int32_t *list_id, uint8_t *codes)
{
    CHECK_H_SERIAL(h, nullptr);
    if (n < 0 || (n > 0 && (!x_rot || !codes))) return fail(CVTMI_EINVAL, "cvtmi_opq_encode: bad arguments");
    if (n == 0) return CVTMI_OK;
    Tmp dx, dl, dc;
    CVTMI_TRY(dx.upload(x_rot, (size_t)n * h->m.D * sizeof(float)));
    CVTMI_TRY(dl.alloc((size_t)n * sizeof(int32_t)));
    CVTMI_TRY(dc.alloc((size_t)n * h->m.M));
    CVTMI_TRY(cvtmi_opq_encode_dev(h, dx.as<float>(), n, dl.as<int32_t>(), dc.as<uint8_t>(), nullptr));
    CVTMI_HIP(hipMemcpy(codes, dc.p, (size_t)n * h->m.M, hipMemcpyDeviceToHost));
    if (list_id) CVTMI_HIP(hipMemcpy(list_id, dl.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

// Rotation + encode of raw rows without a caller-side buffer of rotated rows: the rows go through a handle-owned scratch in
// chunks of 128 K rows (64 MB at D = 128) that is reused for every chunk, so the rotated rows live in the 256 MB Infinity
// Cache between the two kernels and their 2 x 4 D bytes per row need not reach HBM.  (The two kernels are bound by different
// pipes -- fp32 matrix cores vs VALU -- but the encode kernel owns the whole register file of its CU, so they cannot share a CU;
// a single fused kernel would have to give up the encode's software pipeline for the rotation's accumulators.)
int cvtmi_opq_rotate_encode_dev(cvtmi_opq_t h, const float *x, int64_t n, int32_t *list_id, uint8_t *codes, void *stream)
{
    CHECK_H_SERIAL(h, stream);
    if (n < 0 || (n > 0 && (!x || !codes))) return fail(CVTMI_EINVAL, "cvtmi_opq_rotate_encode: bad arguments");
    if (n == 0) return CVTMI_OK;
    if (!h->m.perm && !h->m.R) return cvtmi_opq_encode_dev(h, x, n, list_id, codes, stream);
    // the reference's own rotation is a permutation (reorder_, IVFOPQ.cpp:424-439): the exhaustive-model encode gathers through it,
    // no permuted copy of the rows is made
    if (h->m.perm && h->m.coarseK == 1 && pq_encode_takes_perm(h->m, x, n, h->p_encode))
        return launch_pq_encode(h->m, x, n, nullptr, codes, (hipStream_t)stream, h->p_encode, list_id, h->m.perm);
    const int64_t chunk = 131072;
    CVTMI_TRY(h->s_rot.reserve((size_t)std::min(n, chunk) * h->m.D * sizeof(float)));
    for (int64_t a = 0; a < n; a += chunk) {
        const int64_t m = std::min(chunk, n - a);
        CVTMI_TRY(opq_rotate_impl(h, x + a * h->m.D, m, h->s_rot.as<float>(), (hipStream_t)stream));   // (this call holds the handle exclusively)
        CVTMI_TRY(cvtmi_opq_encode_dev(h, h->s_rot.as<float>(), m, list_id ? list_id + a : nullptr, codes + a * h->m.M, stream));
    }
    return CVTMI_OK;
}

int cvtmi_opq_rotate_encode(cvtmi_opq_t h, const float *x, int64_t n, int32_t *list_id, uint8_t *codes)
{
    CHECK_H_SERIAL(h, nullptr);
    if (n < 0 || (n > 0 && (!x || !codes))) return fail(CVTMI_EINVAL, "cvtmi_opq_rotate_encode: bad arguments");
    if (n == 0) return CVTMI_OK;
    Tmp dx, dl, dc;
    CVTMI_TRY(dx.upload(x, (size_t)n * h->m.D * sizeof(float)));
    CVTMI_TRY(dl.alloc((size_t)n * sizeof(int32_t)));
    CVTMI_TRY(dc.alloc((size_t)n * h->m.M));
    CVTMI_TRY(cvtmi_opq_rotate_encode_dev(h, dx.as<float>(), n, dl.as<int32_t>(), dc.as<uint8_t>(), nullptr));
    CVTMI_HIP(hipMemcpy(codes, dc.p, (size_t)n * h->m.M, hipMemcpyDeviceToHost));
    if (list_id) CVTMI_HIP(hipMemcpy(list_id, dl.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

static int opq_ensure_rows(cvtmi_opq_t h, int64_t total, hipStream_t st)
{
    const size_t M = (size_t)h->m.M;
    if ((size_t)total * M > h->codes.cap) {
        size_t want = std::max((size_t)total, (size_t)(h->codes.cap / M) * 2);
        want = std::max(want, (size_t)4096);
        CVTMI_TRY(h->codes.grow(want * M, (size_t)h->n * M, st));
    }
    if (h->has_lists && (size_t)total * 4 > h->lists.cap)
        CVTMI_TRY(h->lists.grow(std::max((size_t)total, h->lists.cap / 2) * 4, (size_t)h->n * 4, st));
    if (h->has_videos && (size_t)total * 4 > h->videos.cap)
        CVTMI_TRY(h->videos.grow(std::max((size_t)total, h->videos.cap / 2) * 4, (size_t)h->n * 4, st));
    return CVTMI_OK;
}

__global__ void iota_i32_kernel(int32_t *p, int64_t begin, int64_t end, int32_t value, int is_iota)
{
    for (int64_t i = begin + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < end; i += (int64_t)gridDim.x * kBlock)
        p[i] = is_iota ? (int32_t)i : value;
}

static int fill_i32(int32_t *p, int64_t begin, int64_t end, int32_t value, int is_iota, hipStream_t st)
{
    if (end <= begin) return CVTMI_OK;
    int64_t blocks = blocks_for(end - begin, kBlock);
    if (blocks > 4096) blocks = 4096;
    return launch("iota_i32_kernel", iota_i32_kernel, blocks, kBlock, 0, st, p, begin, end, value, is_iota);
}

static int opq_add_common(cvtmi_opq_t h, const uint8_t *codes, const int32_t *list_id, const int32_t *video_id, int64_t n,
                          hipMemcpyKind kind, hipStream_t st)
{
    if (n < 0 || (n > 0 && !codes)) return fail(CVTMI_EINVAL, "cvtmi_opq_add_codes: bad arguments");
    if (n == 0) return CVTMI_OK;
    if (!list_id && h->m.coarseK > 1) return fail(CVTMI_EINVAL, "cvtmi_opq_add_codes: list_id required when coarseK > 1");
    const int64_t total = h->n + n;
    if (total > 0xfffffffeLL) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_add_codes: more than 2^32-2 entries per handle");
    // first explicit list / video ids: materialise the implicit prefix
    if (list_id && h->m.coarseK > 1 && !h->has_lists) {
        h->has_lists = true;
        CVTMI_TRY(h->lists.grow((size_t)std::max<int64_t>(total, 4096) * 4, 0, st));
        CVTMI_TRY(fill_i32(h->lists.as<int32_t>(), 0, h->n, 0, 0, st));
    }
    if (video_id && !h->has_videos) {
        h->has_videos = true;
        CVTMI_TRY(h->videos.grow((size_t)std::max<int64_t>(total, 4096) * 4, 0, st));
        CVTMI_TRY(fill_i32(h->videos.as<int32_t>(), 0, h->n, 0, 1, st));
    }
    CVTMI_TRY(opq_ensure_rows(h, total, st));
    const size_t M = (size_t)h->m.M;
    CVTMI_HIP(hipMemcpyAsync(h->codes.as<uint8_t>() + (size_t)h->n * M, codes, (size_t)n * M, kind, st));
    if (h->has_lists) {
        if (list_id) CVTMI_HIP(hipMemcpyAsync(h->lists.as<int32_t>() + h->n, list_id, (size_t)n * 4, kind, st));
        else CVTMI_TRY(fill_i32(h->lists.as<int32_t>(), h->n, total, 0, 0, st));
    }
    if (h->has_videos) {
        if (video_id) CVTMI_HIP(hipMemcpyAsync(h->videos.as<int32_t>() + h->n, video_id, (size_t)n * 4, kind, st));
        else CVTMI_TRY(fill_i32(h->videos.as<int32_t>(), h->n, total, 0, 1, st));
    }
    if (kind == hipMemcpyHostToDevice) CVTMI_HIP(stream_wait(st));
    h->n = total;
    h->csr_valid = false; h->csr_entry_valid = false;
    return CVTMI_OK;
}

int cvtmi_opq_add_codes(cvtmi_opq_t h, const uint8_t *codes, const int32_t *list_id, const int32_t *video_id, int64_t n)
{
    CHECK_H_SERIAL(h, nullptr);
    return opq_add_common(h, codes, list_id, video_id, n, hipMemcpyHostToDevice, nullptr);
}

int cvtmi_opq_add_codes_dev(cvtmi_opq_t h, const uint8_t *codes, const int32_t *list_id, const int32_t *video_id,
                            int64_t n, void *stream)
{
    CHECK_H_SERIAL(h, stream);
    return opq_add_common(h, codes, list_id, video_id, n, hipMemcpyDeviceToDevice, (hipStream_t)stream);
}

int cvtmi_opq_reserve(cvtmi_opq_t h, int64_t n_total)
{
    CHECK_H_SERIAL(h, nullptr);
    if (n_total < 0 || n_total > 0xfffffffeLL) return fail(CVTMI_EINVAL, "cvtmi_opq_reserve: bad size");
    return h->codes.grow((size_t)n_total * h->m.M, (size_t)h->n * h->m.M, nullptr);
}

int cvtmi_opq_ntotal(cvtmi_opq_t h, int64_t *n)
{
    if (!h || !n) return fail(CVTMI_EINVAL, "cvtmi_opq_ntotal: null");
    *n = h->n;
    return CVTMI_OK;
}

int cvtmi_opq_reset(cvtmi_opq_t h)
{
    CHECK_H_SERIAL(h, nullptr);
    h->n = 0; h->has_lists = false; h->has_videos = false; h->csr_valid = false; h->csr_entry_valid = false; h->rot_n = 0; h->pad_n = 0; h->mf_n = 0;
    return CVTMI_OK;
}

int cvtmi_opq_set_id_base(cvtmi_opq_t h, int64_t base)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_opq_set_id_base: null");
    h->id_base = base;
    return CVTMI_OK;
}

// list-ordered copy of the entries (stable: insertion order inside a list, as m_ivfList holds them), built on the device
// by a counting sort (query_video.hip); only 16 bytes of statistics come back to the host
static int opq_build_csr(cvtmi_opq_t h, hipStream_t st)
{
    if (h->csr_valid && (!h->want_entry || h->csr_entry_valid)) return CVTMI_OK;
    const int64_t n = h->n;
    const int M = h->m.M, L = h->m.coarseK;
    int nb = 1;
    h->csr_valid = false; h->csr_entry_valid = false;
    if (h->want_entry) CVTMI_TRY(h->csr_entry.reserve(std::max<size_t>((size_t)n * 4, 16)));
    CVTMI_TRY(h->csr_scratch.reserve(csr_scratch_bytes(n, L, &nb)));
    CVTMI_TRY(h->csr_codes.reserve(std::max<size_t>((size_t)n * M, 16)));
    CVTMI_TRY(h->csr_videos.reserve(std::max<size_t>((size_t)n * 4, 16)));
    CVTMI_TRY(h->csr_off.reserve(((size_t)L + 1) * 8));
    CVTMI_TRY(h->csr_stats.reserve(16));
    CVTMI_TRY(launch_csr_build(h->has_lists ? h->lists.as<int32_t>() : nullptr, h->has_videos ? h->videos.as<int32_t>() : nullptr,
                               h->codes.as<uint8_t>(), n, L, M, h->csr_scratch.p, h->csr_off.as<int64_t>(), h->csr_codes.as<uint8_t>(),
                               h->csr_videos.as<int32_t>(), h->csr_stats.p, st, h->want_entry ? h->csr_entry.as<uint32_t>() : nullptr));
    struct { int64_t longest; int32_t vmin, vmax; } stats;
    int64_t kept = 0;
    CVTMI_HIP(hipMemcpyAsync(&stats, h->csr_stats.p, sizeof stats, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(hipMemcpyAsync(&kept, h->csr_off.as<int64_t>() + L, sizeof kept, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    h->csr_longest = stats.longest; h->csr_vmin = stats.vmin; h->csr_vmax = stats.vmax; h->csr_kept = kept;
    h->csr_valid = true;
    h->csr_entry_valid = h->want_entry;
    return CVTMI_OK;
}

int cvtmi_opq_get_entries(cvtmi_opq_t h, int64_t *list_off, int32_t *video_id, uint8_t *codes)
{
    CHECK_H_SERIAL(h, nullptr);
    CVTMI_TRY(opq_build_csr(h, nullptr));
    if (list_off) CVTMI_HIP(hipMemcpy(list_off, h->csr_off.p, ((size_t)h->m.coarseK + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (video_id && h->csr_kept) CVTMI_HIP(hipMemcpy(video_id, h->csr_videos.p, (size_t)h->csr_kept * 4, hipMemcpyDeviceToHost));
    if (codes && h->csr_kept) CVTMI_HIP(hipMemcpy(codes, h->csr_codes.p, (size_t)h->csr_kept * h->m.M, hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

int cvtmi_opq_lut_dev(cvtmi_opq_t h, const float *q_rot, int64_t nq, const int32_t *list_id, float *lut, void *stream)
{
    CHECK_H_SHARED(h);
    if (nq < 0 || (nq > 0 && (!q_rot || !lut))) return fail(CVTMI_EINVAL, "cvtmi_opq_lut: bad arguments");
    return launch_lut(h->m, q_rot, nq, list_id, lut, (hipStream_t)stream);
}

int cvtmi_opq_lut(cvtmi_opq_t h, const float *q_rot, int64_t nq, const int32_t *list_id, float *lut)
{
    CHECK_H_SHARED(h);
    if (nq < 0 || (nq > 0 && (!q_rot || !lut))) return fail(CVTMI_EINVAL, "cvtmi_opq_lut: bad arguments");
    if (nq == 0) return CVTMI_OK;
    if (list_id)
        for (int64_t i = 0; i < nq; ++i)
            if (list_id[i] >= h->m.coarseK) return fail(CVTMI_EINVAL, "cvtmi_opq_lut: list_id[%lld] out of range", (long long)i);
    Tmp dq, dl, dt;
    CVTMI_TRY(dq.upload(q_rot, (size_t)nq * h->m.D * sizeof(float)));
    if (list_id) CVTMI_TRY(dl.upload(list_id, (size_t)nq * sizeof(int32_t)));
    const size_t lb = (size_t)nq * h->m.M * h->m.K * sizeof(float);
    CVTMI_TRY(dt.alloc(lb));
    CVTMI_TRY(launch_lut(h->m, dq.as<float>(), nq, list_id ? dl.as<int32_t>() : nullptr, dt.as<float>(), nullptr));
    CVTMI_HIP(hipMemcpy(lut, dt.p, lb, hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

// profile mode: shape of the last scan launch, one consistent triple however many searches run side by side
static void opq_note_scan(cvtmi_opq_t h, int64_t bytes, int qt, int splits)
{
    std::lock_guard<std::mutex> g(h->pool.mu);
    h->last_bytes = bytes; h->last_qt = qt; h->last_splits = splits;
}

// profile mode: a slot of the handle's event ring for one scan launch (searches may run side by side)
static int opq_profile_slot(cvtmi_opq_t h, int *slot)
{
    std::lock_guard<std::mutex> g(h->pool.mu);
    *slot = h->ev_count++ % cvtmi_opq_s::kEvRing;
    if (!h->ev0[*slot]) { CVTMI_HIP(hipEventCreate(&h->ev0[*slot])); CVTMI_HIP(hipEventCreate(&h->ev1[*slot])); }
    return CVTMI_OK;
}

// scan_variant 6 (adc_scan16h, adc_scan_h.hip): tables once per query group, a persistent grid over a host-built item table,
// candidates in per-workgroup spill areas, one selection per (segment, query), merge of the groups' partial lists
static int opq_search_h(cvtmi_opq_t h, OpqScratch &S, const float *q_rot, int64_t nq, int k, float *dist, int64_t *ids, const uint8_t *codes_rot,
                        hipStream_t st)
{
    if (S.hplan_n != h->n || S.hplan_nq != nq || S.hplan_splits != h->p_splits || S.hplan_key != g_scanh_key) {
        scanh_plan(h->n, nq, h->p_splits, S.hplan);
        const size_t bytes = S.hplan.items.size() * sizeof(ScanItem), mbytes = S.hplan.multi.size() * sizeof(uint32_t);
        CVTMI_TRY(S.s_items.reserve(std::max<size_t>(bytes + mbytes, 16)));
        // (pageable sources: the runtime stages them before the call returns, so the vectors may change afterwards)
        if (bytes) CVTMI_HIP(hipMemcpyAsync(S.s_items.p, S.hplan.items.data(), bytes, hipMemcpyHostToDevice, st));
        if (mbytes) CVTMI_HIP(hipMemcpyAsync(S.s_items.as<char>() + bytes, S.hplan.multi.data(), mbytes, hipMemcpyHostToDevice, st));
        S.hplan_n = h->n; S.hplan_nq = nq; S.hplan_splits = h->p_splits; S.hplan_key = g_scanh_key;
    }
    const ScanHPlan &hp = S.hplan;
    float *pd = dist;
    int64_t *pi = ids;
    if (hp.stride > 1) {
        const size_t cnt = (size_t)nq * hp.stride * k;
        CVTMI_TRY(S.s_part_d.reserve(cnt * sizeof(float)));
        CVTMI_TRY(S.s_part_id.reserve(cnt * sizeof(int64_t)));
        pd = S.s_part_d.as<float>();
        pi = S.s_part_id.as<int64_t>();
    }
    CVTMI_TRY(S.s_lut.reserve((size_t)nq * 16 * 256 * sizeof(float)));
    CVTMI_TRY(S.s_qlut.reserve(scanh_qlut_bytes(nq)));
    CVTMI_TRY(S.s_qp.reserve(scanh_qp_bytes(nq)));
    CVTMI_TRY(S.s_spill.reserve(scanh_spill_bytes(hp.grid)));
    uint32_t *gthr = nullptr;
    if (hp.stride > 1 && h->p_share) {
        CVTMI_TRY(S.s_gthr.reserve(scanh_gthr_bytes(nq)));   // the bounds and, behind them, the histograms the segments of a query share
        gthr = S.s_gthr.as<uint32_t>();
    }
    int slot = 0;
    if (h->p_profile) {
        CVTMI_TRY(opq_profile_slot(h, &slot));
        CVTMI_HIP(hipEventRecord(h->ev0[slot], st));
    }
    CVTMI_TRY(launch_adc_scan_h(h->m, h->codes.as<uint8_t>(), codes_rot, h->n, h->id_base, q_rot, nq, k, hp, S.s_items.as<ScanItem>(), pd, pi, dist, ids,
                                S.s_lut.as<float>(), S.s_qlut.p, S.s_qp.p, S.s_spill.p, gthr, h->p_lazy, scan_seed_enabled(), st));
    if (h->p_profile) {
        CVTMI_HIP(hipEventRecord(h->ev1[slot], st));
        opq_note_scan(h, ((nq + 7) / 8) * h->n * h->m.M, 8, hp.stride);  // passes x rows x M code bytes
    }
    if (hp.stride > 1)  // (queries of groups scanned in one piece are already in place: the merge skips them)
        CVTMI_TRY(launch_topk_merge(pd, pi, nq, hp.stride, k, dist, ids, st,
                                    reinterpret_cast<const uint32_t *>(S.s_items.as<char>() + hp.items.size() * sizeof(ScanItem))));
    return CVTMI_OK;
}

// M < 16 (the reference's own test model has M = 8: opq/src/multi_frame_index_test.cpp) only had the round-1 row-per-lane kernels: 1.0 M
// queries/s at C2's shape against 3.1 M for M = 16, which does twice the work (round 5, tools/opq_m_sweep.py).  The M = 16 kernels take
// such an index as it is once the rows are padded to 16 code bytes with zeros and every query gets 16 - M all-zero tables behind its own:
// a zero byte looks up a zero, integer bounds and fp32 sums are unchanged (x + 0.0f == x for the non-negative sums here), the exact
// re-sum still adds the model's M entries in the reference's order first.  Costs 16 + 16 bytes per row of derived copies.
static bool opq_pads(const cvtmi_opq_s *h)
{
    return tune_scan_pad_m.geti() && h->m.M >= 1 && h->m.M < 16 && h->m.K >= 1 && h->m.K <= 256 && h->m.D <= 256;
}
static ScanPlan opq_plan(cvtmi_opq_t h, int64_t nq, int k)
{
    if (opq_pads(h) && (h->p_variant == 7 || h->p_variant >= 3) && h->p_qtile == 0) {
        OpqModelDev m16 = h->m;
        m16.M = 16;
        // (the persistent grid and the small-batch form build their tables from the codebooks themselves: adc_scan16q / 16a only)
        // (planned as at least four queries: below that plan_scan prefers the fp32-table kernels, which build their tables from the codebooks)
        // M = 8 / 4 natively (adc_scan16p: 16 / M rows per 16-byte load; needs the pre-rotated copy): planned in units of loads -- a load
        // costs what an M = 16 row costs, so the split decision sees n / RPL "rows"
        const bool packed = tune_scan_packed_m.geti() && (h->m.M == 8 || h->m.M == 4) && h->p_prerot && h->p_variant != 4 && h->p_variant != 5;
        const int64_t n_plan = packed ? (h->n * h->m.M + 15) / 16 : h->n;
        ScanPlan pp = plan_scan(m16, n_plan, std::max<int64_t>(nq, 4), k, 0, h->p_splits, h->p_variant == 4 || h->p_variant == 5 ? h->p_variant : 3);
        if (pp.variant >= 3 && pp.variant <= 5) {
            pp.real_M = h->m.M;
            pp.packed = packed && pp.variant == 3;
            if (!h->p_tail) { pp.groups_a = 0; pp.splits_b = 0; }
            return pp;
        }
    }
    ScanPlan plan = plan_scan(h->m, h->n, nq, k, h->p_qtile, h->p_splits, h->p_variant);
    if (plan.variant == 6) return plan;
    if (!h->p_tail) { plan.groups_a = 0; plan.splits_b = 0; }
    if (h->p_groups_a > 0 && h->p_splits_b > plan.splits && plan.variant >= 3 &&
        h->p_groups_a < (nq + plan.qtile - 1) / plan.qtile) {
        plan.groups_a = h->p_groups_a; plan.splits_b = h->p_splits_b;
    }
    return plan;
}

// Does a search of this shape ask for the matrix-core bound filter (adc_mfma.hip)?  Everything but the state of the operand
// copy: forced scan forms (scan_variant, qtile, splits) bypass it, the bounds are the handle's "scan_mfma*" parameters.
static bool mfma_wanted(const cvtmi_opq_s *h, int64_t nq, int k)
{
    const int64_t max_rows = h->p_mfma_max_rows >= 0 ? h->p_mfma_max_rows : ((int64_t)1 << 30) / (h->m.D + 4);   // the copy: D + 4 bytes per row
    return h->p_mfma && h->mf_state >= 0 && !h->books_h.empty() && h->m.M == 16 && h->m.K == 256 && h->m.D % 32 == 0 && h->m.D <= 256 && h->m.coarseK == 1 &&
           k >= 1 && k <= 128 && h->p_variant == 7 && h->p_qtile == 0 && h->p_splits == 0 && nq >= h->p_mfma_min_nq && nq <= 0x7fffffff &&
           h->n >= h->p_mfma_min_rows && h->n <= max_rows && h->n < 0x7fffffe0LL;
}

// the model's part of that filter (once per handle) and the decoded operand copy of the rows, built and extended like codes_rot.  Whatever
// does not fit in memory, or a codebook the bound cannot be stated for, turns the route off for the handle: the scan answers.
static int opq_prepare_mfma(cvtmi_opq_t h, int64_t nq, int k, hipStream_t st)
{
    {
        std::shared_lock<std::shared_timed_mutex> rd(h->rw);
        if (h->n == 0 || !mfma_wanted(h, nq, k)) return CVTMI_OK;
        if (h->mf_state == 1 && h->mf_n == h->n) return CVTMI_OK;
    }
    Serial serial(h->sync, st);
    OpqExclusive excl(h, st);
    const auto soft = [&](int rc) {   // out of memory: off, and not an error
        if (rc != CVTMI_ENOMEM) return rc;
        (void)hipGetLastError(); g_err.clear();
        h->mf_state = -1; h->mf_n = 0; h->mf_pack.release(); h->mf_norm.release();
        return (int)CVTMI_OK;
    };
    const int D = h->m.D;
    if (h->mf_state == 0) {
        const size_t o_xb = 4096 * sizeof(double), o_c = o_xb + (size_t)256 * D, o_s = o_c + (size_t)D * sizeof(float), bytes = o_s + (size_t)D * sizeof(float);
        std::vector<double> blob((bytes + 7) / 8);   // nrm | xb | c | s
        char *b = reinterpret_cast<char *>(blob.data());
        double x_max = 0.0, eps_max = 0.0, xhat_max = 0.0;
        if (!adc_mfma_model(h->books_h.data(), D, h->m.K, reinterpret_cast<int8_t *>(b + o_xb), blob.data(), reinterpret_cast<float *>(b + o_c),
                            reinterpret_cast<float *>(b + o_s), &x_max, &eps_max, &xhat_max)) {
            h->mf_state = -1;
            return CVTMI_OK;
        }
        int rc = h->mf_model.reserve(bytes);
        if (rc == CVTMI_OK) rc = h->mf_stat.reserve(2 * sizeof(unsigned long long));
        if (rc != CVTMI_OK) return soft(rc);
        CVTMI_HIP(hipMemsetAsync(h->mf_stat.p, 0, 2 * sizeof(unsigned long long), st));
        CVTMI_HIP(hipMemcpyAsync(h->mf_model.p, b, bytes, hipMemcpyHostToDevice, st));
        CVTMI_HIP(stream_wait(st));   // (the blob goes out of scope)
        const char *d = h->mf_model.as<char>();
        h->mf.nrm = reinterpret_cast<const double *>(d); h->mf.xb = reinterpret_cast<const int8_t *>(d + o_xb);
        h->mf.c = reinterpret_cast<const float *>(d + o_c); h->mf.s = reinterpret_cast<const float *>(d + o_s);
        h->mf.x_max = x_max; h->mf.eps_max = eps_max; h->mf.xhat_max = xhat_max;
        h->mf_state = 1;
    }
    if (h->mf_state != 1) return CVTMI_OK;
    if (h->mf_n > h->n) h->mf_n = 0;
    const size_t need = adc_mfma_pack_bytes(D, h->n);
    if (h->mf_pack.cap < need || h->mf_norm.cap < (size_t)h->n * sizeof(float)) {
        const int64_t room = std::max<int64_t>(h->n, (int64_t)(h->codes.cap / 16));   // as many rows as the code buffer holds: appended rows extend the copy
        int rc = h->mf_pack.reserve(adc_mfma_pack_bytes(D, room));
        if (rc == CVTMI_ENOMEM) rc = h->mf_pack.reserve(need);
        h->mf_n = 0;   // reserve() does not keep the old contents
        if (rc != CVTMI_OK) return soft(rc);
        rc = h->mf_norm.reserve((size_t)room * sizeof(float));
        if (rc != CVTMI_OK) return soft(rc);
    }
    CVTMI_TRY(launch_adc_mfma_pack(h->mf, D, h->codes.as<uint8_t>(), h->mf_n, h->n, h->mf_pack.p, h->mf_norm.as<float>(), st));
    h->mf_n = h->n;
    return CVTMI_OK;
}

// what a search needs of the index beyond the rows: the pre-rotated copy the M = 16 scans stream, extended under the EXCLUSIVE lock
// (once per index state; the searches that follow on other streams wait for the event the exclusive call leaves)
static int opq_prepare_rot(cvtmi_opq_t h, int64_t nq, int k, hipStream_t st);
static int opq_prepare(cvtmi_opq_t h, int64_t nq, int k, hipStream_t st)
{
    CVTMI_TRY(opq_prepare_rot(h, nq, k, st));
    return opq_prepare_mfma(h, nq, k, st);
}
static int opq_prepare_rot(cvtmi_opq_t h, int64_t nq, int k, hipStream_t st)
{
    bool padded = false, packed = false;
    {
        std::shared_lock<std::shared_timed_mutex> rd(h->rw);
        if (h->n == 0) return CVTMI_OK;
        const ScanPlan plan = opq_plan(h, nq, k);
        packed = plan.packed;
        padded = plan.real_M > 0 && !packed;
        const bool want_rot = h->p_prerot && ((h->m.M == 16 && (plan.variant >= 3 || scans_applies(h->m, h->n, nq, k) ||
                                                                (tune_scan_bigk.geti() && scank_applies(h->m, h->n, nq, k)))) || padded || packed);
        if (!padded && !want_rot) return CVTMI_OK;
        const bool pad_ok = !padded || (h->pad_n == h->n && h->codes16.cap >= (size_t)h->n * 16);
        const bool rot_ok = !want_rot || (h->rot_n == h->n && h->rot_kind == (packed ? 1 : 0) &&
                                          h->codes_rot.cap >= (packed ? ((size_t)h->n * h->m.M + 15) / 16 * 16 : (size_t)h->n * 16));
        if (pad_ok && rot_ok) return CVTMI_OK;
    }
    Serial serial(h->sync, st);
    OpqExclusive excl(h, st);
    if (packed) {   // the rows themselves, rotated inside their 16-byte groups: M bytes per row, no padded copy
        if (h->rot_kind != 1) { h->rot_kind = 1; h->rot_n = 0; }
        if (h->rot_n > h->n) h->rot_n = 0;
        const size_t need = ((size_t)h->n * h->m.M + 15) / 16 * 16;
        if (h->codes_rot.cap < need) {
            int rc = h->codes_rot.reserve(std::max<size_t>((h->codes.cap + 15) / 16 * 16, need));
            if (rc == CVTMI_ENOMEM) rc = h->codes_rot.reserve(need);
            h->rot_n = 0;
            if (rc == CVTMI_ENOMEM) { (void)hipGetLastError(); g_err.clear(); return CVTMI_OK; }   // (the search falls back to the padded / row-per-lane forms)
            CVTMI_TRY(rc);
        }
        CVTMI_TRY(launch_rotate_codes_packed(h->codes.as<uint8_t>(), h->m.M, h->codes_rot.as<uint8_t>(), h->rot_n, h->n, st));
        h->rot_n = h->n;
        return CVTMI_OK;
    }
    if (h->rot_kind != 0) { h->rot_kind = 0; h->rot_n = 0; }
    if (padded) {   // the 16-byte rows first: the rotated copy is made from them
        if (h->pad_n > h->n) h->pad_n = 0;
        if (h->codes16.cap < (size_t)h->n * 16) {
            // The derived copies are an optimisation (16 + 16 bytes per row beside M): when HBM does not hold them the search must still
            // answer -- the row-per-lane kernels take the index as it is (opq_search_leased checks pad_n == n).  ADVICE r5.
            int rc = h->codes16.reserve(std::max<size_t>(h->codes.cap / (size_t)h->m.M * 16, (size_t)h->n * 16));
            if (rc == CVTMI_ENOMEM) rc = h->codes16.reserve((size_t)h->n * 16);   // without the growth margin of the code buffer
            h->pad_n = 0;  // reserve() does not keep the old contents
            if (rc == CVTMI_ENOMEM) { (void)hipGetLastError(); g_err.clear(); return CVTMI_OK; }
            CVTMI_TRY(rc);
        }
        CVTMI_TRY(launch_pad_codes(h->codes.as<uint8_t>(), h->m.M, h->codes16.as<uint8_t>(), h->pad_n, h->n, st));
        h->pad_n = h->n;
        if (!h->p_prerot) return CVTMI_OK;
    }
    if (h->rot_n > h->n) h->rot_n = 0;
    if (h->codes_rot.cap < (size_t)h->n * 16) {
        int rc = h->codes_rot.reserve(std::max<size_t>(padded ? h->codes16.cap : h->codes.cap, (size_t)h->n * 16));
        if (rc == CVTMI_ENOMEM) rc = h->codes_rot.reserve((size_t)h->n * 16);
        h->rot_n = 0;  // reserve() does not keep the old contents
        if (rc == CVTMI_ENOMEM) { (void)hipGetLastError(); g_err.clear(); return CVTMI_OK; }   // (the scans rotate in registers without it)
        CVTMI_TRY(rc);
    }
    CVTMI_TRY(launch_rotate_codes(padded ? h->codes16.as<uint8_t>() : h->codes.as<uint8_t>(), h->codes_rot.as<uint8_t>(), h->rot_n, h->n, st));
    h->rot_n = h->n;
    return CVTMI_OK;
}

// Does the dispatch take the small-batch form (adc_scan_h.hip: scans, up to 128 queries)?  Its per-group passes over the whole table
// were fitted at 1 M rows; round 5 swept the table size (tools/sweep_scan_dispatch.py, profiles/r05_scan_dispatch_sweep.txt): it is
// ahead of the persistent grid while rows x query groups stays under ~48 M (2 M rows: up to 128 queries; 10 M: up to 32; 30 M: 8)
// and behind by up to 2x beyond (100 M rows, 128 queries: 8.3 against 3.7 ms).
static bool scans_chosen(const cvtmi_opq_s *h, int64_t nq, int k)
{
    return h->p_variant == 7 && h->p_splits == 0 && h->p_qtile == 0 && h->p_small && scans_applies(h->m, h->n, nq, k) &&
           h->n * ((nq + 7) / 8) <= tune_scans_max_work.get();
}

// the dispatch a search would take, for inspection and for the CPU tests that pin the rules (include/cvtmi.h)
extern "C" int cvtmi_opq_describe_dispatch(int D, int M, int K, int64_t n_rows, int64_t nq, int k, int out[7])
{
    if (!out || D < 1 || M < 1 || M > 16 || D % M != 0 || K < 1 || K > 256 || n_rows < 0 || nq < 1 || k < 1)
        return fail(CVTMI_EINVAL, "cvtmi_opq_describe_dispatch: bad arguments");
    cvtmi_opq_s h;   // default settings; nothing of it touches a device
    h.m.D = D; h.m.M = M; h.m.K = K; h.m.step = D / M; h.m.coarseK = 1;
    h.n = n_rows;
    const bool small = scans_chosen(&h, nq, k);
    const ScanPlan p = opq_plan(&h, nq, k);
    out[0] = small ? 1 : 0; out[1] = p.variant; out[2] = p.qtile; out[3] = p.splits; out[4] = p.groups_a; out[5] = p.splits_b; out[6] = p.real_M;
    return CVTMI_OK;
}

// one search on stream st with the scratch set S; the caller holds h->rw shared
static int opq_search_leased(cvtmi_opq_t h, OpqScratch &S, const float *q, int64_t nq, int rotate, int k, float *dist, int64_t *ids, hipStream_t st)
{
    if (h->n == 0)  // an empty index (e.g. a rank whose row block is empty): all padding, (+inf, -1)
        return launch_topk_select(nullptr, nullptr, nq, 0, k, dist, ids, st);
    bool mfma = mfma_wanted(h, nq, k) && h->mf_state == 1 && h->mf_n == h->n && h->mf_pack.p;
    // what the flagged queries the route's own exact redo leaves over (rest) go through: the planned 8-query scan, a group scanned when one of its queries is
    // flagged -- a call whose every query is flagged then costs the filter plus the scan it would have been without the route
    ScanPlan redo_plan = plan_scan(h->m, h->n, nq, k, 8, 0, 3);
    redo_plan.groups_a = 0; redo_plan.splits_b = 0;
    const bool redo_fast = redo_plan.variant == 3 && redo_plan.qtile == 8;
    if (mfma) {   // the route's scratch (about 1 GB at most) is its own need: without the memory the scan answers, as without the operand copy
        int rc = S.s_lut.reserve((size_t)nq * 16 * 256 * sizeof(float));
        if (rc == CVTMI_OK) rc = S.s_spill.reserve(adc_mfma_scratch_bytes(h->m.D, h->n, nq, k, h->p_mfma_cap, h->p_mfma_sample, nullptr));
        if (rc == CVTMI_OK && redo_fast && redo_plan.stride() > 1) {
            rc = S.s_part_d.reserve((size_t)nq * redo_plan.stride() * k * sizeof(float));
            if (rc == CVTMI_OK) rc = S.s_part_id.reserve((size_t)nq * redo_plan.stride() * k * sizeof(int64_t));
        }
        if (rc == CVTMI_ENOMEM) { (void)hipGetLastError(); g_err.clear(); mfma = false; }
        else CVTMI_TRY(rc);
    }
    if (!mfma && h->p_profile && h->mf_stat.p)   // (cvtmi_opq_last_mfma speaks of the last profiled search: this one did not take the route)
        CVTMI_HIP(hipMemsetAsync(h->mf_stat.p, 0, 2 * sizeof(unsigned long long), st));
    if (mfma) {
        // large batches, k <= 128: the int8 matrix-core bound filter over the decoded rows, exact sums of the survivors (adc_mfma.hip);
        // the queries it could not answer are flagged and go through the scan kernels behind it under a predicate
        const float *q_rot = nullptr;
        CVTMI_TRY(opq_rotate_probe(h, S, q, nq, rotate, 0, st, &q_rot));
        int slot = 0;
        if (h->p_profile) {
            CVTMI_TRY(opq_profile_slot(h, &slot));
            CVTMI_HIP(hipEventRecord(h->ev0[slot], st));
        }
        AdcMfmaRedo redo{};
        CVTMI_TRY(launch_adc_mfma(h->m, h->mf, h->codes.as<uint8_t>(), h->mf_pack.p, h->mf_norm.as<float>(), h->n, h->id_base, q_rot, nq, k, h->p_mfma_cap,
                                  h->p_mfma_sample, S.s_lut.as<float>(), S.s_spill.p, dist, ids, &redo, h->p_profile ? h->mf_stat.as<unsigned long long>() : nullptr, st));
        // The route has answered up to 64 flagged queries itself, exactly and over all rows (mf_redo_*, adc_mfma.hip).  The scan kernels run
        // under redo.rest for whoever is left: flagged queries beyond those 64, and the few a slot could not answer.
        if (redo_fast) {
            const uint8_t *crot = (h->p_prerot && h->rot_kind == 0 && h->rot_n == h->n && h->codes_rot.p) ? h->codes_rot.as<uint8_t>() : nullptr;
            const bool split = redo_plan.stride() > 1;
            CVTMI_TRY(launch_adc_scan(h->m, h->codes.as<uint8_t>(), h->n, h->id_base, q_rot, nq, k, redo_plan, split ? S.s_part_d.as<float>() : dist,
                                      split ? S.s_part_id.as<int64_t>() : ids, S.s_lut.as<float>(), crot, st, nullptr, h->p_lazy, nullptr, nullptr, redo.rest, true));
            if (split) CVTMI_TRY(launch_topk_merge(S.s_part_d.as<float>(), S.s_part_id.as<int64_t>(), nq, redo_plan.stride(), k, dist, ids, st, redo.rest));
        } else {   // (shapes the 8-query kernel is not planned for: one workgroup per flagged query)
            ScanPlan exact;
            exact.qtile = 1; exact.splits = 1; exact.variant = 0;
            CVTMI_TRY(launch_adc_scan(h->m, h->codes.as<uint8_t>(), h->n, h->id_base, q_rot, nq, k, exact, dist, ids, nullptr, nullptr, st, nullptr, h->p_lazy, nullptr,
                                      nullptr, redo.rest));
        }
        if (h->p_profile) {
            CVTMI_HIP(hipEventRecord(h->ev1[slot], st));
            opq_note_scan(h, ((nq + 7) / 8) * h->n * h->m.M, 8, 1);   // the scan's passes x rows x M code bytes: an EQUIVALENT look-up rate
        }
        return CVTMI_OK;
    }
    if (scans_chosen(h, nq, k)) {
        // 1 .. 128 queries (up to sixteen query groups): global bounds first, candidate lists, one selection workgroup per query
        // (adc_scan_h.hip) -- four launches, the rotation folded into the first
        const uint8_t *crot = (h->m.M == 16 && h->p_prerot && h->rot_n == h->n && h->codes_rot.p) ? h->codes_rot.as<uint8_t>() : nullptr;
        CVTMI_TRY(S.s_lut.reserve((size_t)((nq + 7) / 8 * 8) * 16 * 256 * sizeof(float)));
        CVTMI_TRY(S.s_qlut.reserve(scanh_qlut_bytes(nq)));
        CVTMI_TRY(S.s_qp.reserve(scanh_qp_bytes(nq)));
        CVTMI_TRY(S.s_spill.reserve(scans_scratch_bytes()));
        int slot = 0;
        if (h->p_profile) {
            CVTMI_TRY(opq_profile_slot(h, &slot));
            CVTMI_HIP(hipEventRecord(h->ev0[slot], st));
        }
        const float *qs = q;
        int rot = rotate && (h->m.perm || h->m.R);
        if (rot && !scans_fuses_rotation(h->m)) {   // a dense rotation wider than 128: the rotation kernel first
            CVTMI_TRY(S.s_qrot.reserve((size_t)nq * h->m.D * sizeof(float)));
            CVTMI_TRY(opq_rotate_impl(h, q, nq, S.s_qrot.as<float>(), st));
            qs = S.s_qrot.as<float>(); rot = 0;
        }
        CVTMI_TRY(launch_adc_scan_small(h->m, h->codes.as<uint8_t>(), crot, h->n, h->id_base, qs, rot, nq, k, dist, ids, S.s_lut.as<float>(), S.s_qlut.p,
                                        S.s_qp.p, S.s_spill.p, h->p_lazy, st));
        if (h->p_profile) {
            CVTMI_HIP(hipEventRecord(h->ev1[slot], st));
            opq_note_scan(h, h->n * h->m.M, 8, 1);
        }
        return CVTMI_OK;
    }
    const float *q_rot = nullptr;
    CVTMI_TRY(opq_rotate_probe(h, S, q, nq, rotate, 0, st, &q_rot));
    if (tune_scan_bigk.geti() && h->p_variant == 7 && h->p_qtile == 0 && h->p_splits == 0 && scank_applies(h->m, h->n, nq, k)) {
        // k = 129 .. 2048 (round 6): sampled histogram bound, candidate lists, one selection workgroup per query (adc_scan_h.hip); the
        // queries it could not answer (a list that overflowed, a crowded band, tables that bound nothing) are flagged and go through the
        // exact kernel behind it.  Batches whose candidate lists would pass 1 GB go in pieces.
        const uint8_t *crot = (h->p_prerot && h->rot_kind == 0 && h->rot_n == h->n && h->codes_rot.p) ? h->codes_rot.as<uint8_t>() : nullptr;
        int64_t per = nq;
        while (per > 8 && scank_scratch_bytes(h->n, per, k) > ((size_t)1 << 30)) per = ((per / 2) + 7) / 8 * 8;
        CVTMI_TRY(S.s_lut.reserve((size_t)((per + 7) / 8 * 8) * 16 * 256 * sizeof(float)));
        CVTMI_TRY(S.s_qlut.reserve(scanh_qlut_bytes(per)));
        CVTMI_TRY(S.s_qp.reserve(scanh_qp_bytes(per)));
        CVTMI_TRY(S.s_spill.reserve(scank_scratch_bytes(h->n, per, k)));
        int slot = 0;
        if (h->p_profile) {
            CVTMI_TRY(opq_profile_slot(h, &slot));
            CVTMI_HIP(hipEventRecord(h->ev0[slot], st));
        }
        ScanPlan exact;
        exact.qtile = 1; exact.splits = 1; exact.variant = 0;
        for (int64_t q0 = 0; q0 < nq; q0 += per) {
            const int64_t n1 = std::min(per, nq - q0);
            uint32_t *flags = nullptr;
            CVTMI_TRY(launch_adc_scan_bigk(h->m, h->codes.as<uint8_t>(), crot, h->n, h->id_base, q_rot + q0 * h->m.D, n1, k, dist + q0 * k, ids + q0 * k,
                                           S.s_lut.as<float>(), S.s_qlut.p, S.s_qp.p, S.s_spill.p, h->p_lazy, &flags, st));
            CVTMI_TRY(launch_adc_scan(h->m, h->codes.as<uint8_t>(), h->n, h->id_base, q_rot + q0 * h->m.D, n1, k, exact, dist + q0 * k, ids + q0 * k,
                                      nullptr, nullptr, st, nullptr, h->p_lazy, nullptr, nullptr, flags));
        }
        if (h->p_profile) {
            CVTMI_HIP(hipEventRecord(h->ev1[slot], st));
            opq_note_scan(h, ((nq + 7) / 8) * h->n * h->m.M * 5 / 4, 8, 1);   // passes x rows x M code bytes, the sampled pass included
        }
        return CVTMI_OK;
    }
    ScanPlan plan = opq_plan(h, nq, k);
    if (plan.packed && !(h->rot_kind == 1 && h->rot_n == h->n && h->codes_rot.p))   // (the packed rotation is not there: as before)
        plan = plan_scan(h->m, h->n, nq, k, h->p_qtile, h->p_splits, h->p_variant);
    if (plan.real_M > 0 && !plan.packed && !(h->pad_n == h->n && h->codes16.p)) plan = plan_scan(h->m, h->n, nq, k, h->p_qtile, h->p_splits, h->p_variant);   // (the padded rows are not there: as before)
    const bool packed = plan.packed, padded = plan.real_M > 0 && !packed;
    OpqModelDev m_scan = h->m;
    if (padded || packed) m_scan.M = 16;
    const uint8_t *scan_rows = padded ? h->codes16.as<uint8_t>() : h->codes.as<uint8_t>();
    // the scan streams the pre-rotated copy of the rows when it is up to date (opq_prepare); otherwise it rotates in registers
    const uint8_t *codes_rot = packed ? h->codes_rot.as<uint8_t>()
                             : (plan.variant >= 3 && (h->m.M == 16 || padded) && h->p_prerot && h->rot_kind == 0 && h->rot_n == h->n && h->codes_rot.p) ? h->codes_rot.as<uint8_t>() : nullptr;
    if (plan.variant == 6) return opq_search_h(h, S, q_rot, nq, k, dist, ids, codes_rot, st);
    float *pd = dist;
    int64_t *pi = ids;
    if (plan.stride() > 1) {
        const size_t cnt = (size_t)nq * plan.stride() * k;
        CVTMI_TRY(S.s_part_d.reserve(cnt * sizeof(float)));
        CVTMI_TRY(S.s_part_id.reserve(cnt * sizeof(int64_t)));
        pd = S.s_part_d.as<float>();
        pi = S.s_part_id.as<int64_t>();
    }
    int slot = 0;
    if (h->p_profile) {
        CVTMI_TRY(opq_profile_slot(h, &slot));
        CVTMI_HIP(hipEventRecord(h->ev0[slot], st));
    }
    float *lut_scratch = nullptr;
    if (plan.variant >= 3) {  // per-query fp32 tables in HBM (16 KB per query at M=16, K=256)
        CVTMI_TRY(S.s_lut.reserve((size_t)nq * m_scan.M * 256 * sizeof(float)));
        lut_scratch = S.s_lut.as<float>();
    }
    uint32_t *gthr = nullptr;
    if (plan.variant >= 3 && plan.stride() > 1 && h->p_share) {
        CVTMI_TRY(S.s_gthr.reserve((size_t)nq * sizeof(uint32_t)));
        gthr = S.s_gthr.as<uint32_t>();
    }
    // (two-region plan, first region in one piece: those queries' lists are written in place by the scan, the merge starts behind them)
    const int64_t placed = plan.stride() > 1 ? scan_in_place_queries(plan, m_scan.M, nq) : 0;
    CVTMI_TRY(launch_adc_scan(m_scan, scan_rows, h->n, h->id_base, q_rot, nq, k, plan, pd, pi, lut_scratch,
                              codes_rot, st, gthr, h->p_lazy, placed ? dist : nullptr, placed ? ids : nullptr));
    if (h->p_profile) {
        CVTMI_HIP(hipEventRecord(h->ev1[slot], st));
        const int64_t groups = (nq + plan.qtile - 1) / plan.qtile;
        opq_note_scan(h, groups * h->n * h->m.M, plan.qtile, plan.splits);  // passes x rows x M code bytes
    }
    if (plan.stride() > 1)
        CVTMI_TRY(launch_topk_merge(pd + placed * plan.stride() * k, pi + placed * plan.stride() * k, nq - placed, plan.stride(), k, dist + placed * k,
                                    ids + placed * k, st));
    return CVTMI_OK;
}

int cvtmi_opq_search_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int k, float *dist, int64_t *ids,
                         void *stream)
{
    CHECK_H(h);
    if (nq < 0 || (nq > 0 && (!q || !dist || !ids))) return fail(CVTMI_EINVAL, "cvtmi_opq_search: bad arguments");
    if (h->m.coarseK != 1)
        return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search: exhaustive search needs coarseK == 1 (use cvtmi_opq_query_video)");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (nq == 0) return CVTMI_OK;
    hipStream_t st = (hipStream_t)stream;
    CVTMI_TRY(opq_prepare(h, nq, k, st));
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    OpqLease lease;
    CVTMI_TRY(lease.open(h, st, false));
    return opq_search_leased(h, *lease.s, q, nq, rotate, k, dist, ids, st);
}


// Host-pointer search, the reference's own call shape (opq/src/multi_frame_index_test.cpp:45-54 hands over host buffers).  A large
// batch is cut into chunks that alternate between TWO scratch sets with their own streams: while chunk i is scanned, the queries of
// chunk i + 1 go up and the results of chunk i - 1 come down (pinned staging areas the sets keep), and the scan kernels of
// neighbouring chunks fill each other's last, partly occupied round of workgroups.
int cvtmi_opq_search(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int k, float *dist, int64_t *ids)
{
    CHECK_H(h);
    if (nq < 0 || (nq > 0 && (!q || !dist || !ids))) return fail(CVTMI_EINVAL, "cvtmi_opq_search: bad arguments");
    if (nq == 0) return CVTMI_OK;
    if (h->m.coarseK != 1)
        return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search: exhaustive search needs coarseK == 1 (use cvtmi_opq_query_video)");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search: k=%d outside 1..%d", k, CVTMI_K_MAX);
    const int D = h->m.D;
    // pieces of `per` queries: 4096 by default = 512 query groups = ONE full round of the scan's workgroups on 256 CUs, so cutting
    // the batch there costs the scan nothing (10 000 queries: 1 + 1 + 0.44 rounds either way)
    // Page-locked result arrays (cvtmi_host_alloc): the kernels write the lists straight into them (device-visible host memory, posted
    // PCIe writes: 12 MB over the 3 ms of a 10 000-query scan) -- no device copy of the results, no copy engine, and therefore no
    // reason to cut the batch: ONE launch chain, the same the device-pointer entry issues; the query groups that are scanned in one
    // piece deliver their lists as their workgroups end.  Round 5: 3.45-3.55 -> 3.15-3.25 ms per 10 000 queries (device pointers: 3.0-3.1).
    const bool q_pinned = host_pinned(q), out_pinned = host_pinned(dist) && host_pinned(ids);
    float *zd = nullptr;
    int64_t *zi = nullptr;
    if (out_pinned && tune_opq_host_zero_copy.geti()) {
        void *pd = nullptr, *pi = nullptr;
        if (hipHostGetDevicePointer(&pd, dist, 0) == hipSuccess && hipHostGetDevicePointer(&pi, ids, 0) == hipSuccess && pd && pi) {
            zd = static_cast<float *>(pd); zi = static_cast<int64_t *>(pi);
        } else {
            (void)hipGetLastError();
        }
    }
    int64_t per = tune_opq_host_chunk.geti();
    const int64_t per_default = per > 0 ? per : 4096;
    if (per <= 0 || nq < per + per / 4 || zd) per = nq;
    // (zero-copy results keep the batch whole only while its QUERIES fit the staging guard below: past that -- more than 131 072
    //  queries at D = 128 -- the batch goes out in the default pieces, still straight into the caller's arrays, rather than through a
    //  freshly allocated device copy of everything: ADVICE r5)
    if (zd && (per > (64 << 20) / (int64_t)(D * 4) || (size_t)per * k * 12 > ((size_t)256 << 20))) per = per_default;
    per = (per + 7) / 8 * 8;   // whole query groups
    const int chunks = (int)((nq + per - 1) / per);
    if (per > (64 << 20) / (int64_t)(D * 4) || (size_t)per * k * 12 > ((size_t)256 << 20)) {
        // very large pieces: no staging area of that size is kept around
        Tmp dq, dd, di;
        const size_t qb = (size_t)nq * D * sizeof(float), db = (size_t)nq * k * sizeof(float), ib = (size_t)nq * k * sizeof(int64_t);
        CVTMI_TRY(dq.upload(q, qb));
        CVTMI_TRY(dd.alloc(db));
        CVTMI_TRY(di.alloc(ib));
        CVTMI_TRY(cvtmi_opq_search_dev(h, dq.as<float>(), nq, rotate, k, dd.as<float>(), di.as<int64_t>(), nullptr));
        CVTMI_HIP(hipMemcpy(dist, dd.p, db, hipMemcpyDeviceToHost));
        CVTMI_HIP(hipMemcpy(ids, di.p, ib, hipMemcpyDeviceToHost));
        return CVTMI_OK;
    }
    CVTMI_TRY(opq_prepare(h, per, k, nullptr));
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    OpqLease lease[2];
    const int nsets = chunks > 1 ? 2 : 1;
    for (int i = 0; i < nsets; ++i) CVTMI_TRY(lease[i].open(h, nullptr, true));
    const size_t qb = (size_t)per * D * sizeof(float), db = (size_t)per * k * sizeof(float), ib = (size_t)per * k * sizeof(int64_t);
    for (int i = 0; i < nsets; ++i) {
        OpqScratch &S = *lease[i].s;
        CVTMI_TRY(S.io_q.reserve(qb));
        if (zd && !scans_applies(h->m, h->n, nq, k)) {   // (what may take the small-batch form below stages everything)
            if (!q_pinned) CVTMI_TRY(S.io_pin.reserve(qb));
            continue;
        }
        CVTMI_TRY(S.io_d.reserve(db));
        CVTMI_TRY(S.io_i.reserve(ib));
        CVTMI_TRY(S.io_pin.reserve(qb + db + ib));   // [queries | distances | ids]
    }
    struct InFlight { int64_t q0 = 0, n = 0; } fl[2];
    // pinned staging -> the caller's (pageable) arrays: a large copy is shared with a helper thread (one core moves ~10 GB/s: the
    // 12 MB of a 10 000 x 100 result would otherwise cost a third of the scan's time)
    const auto copy_out = [](void *dst, const void *src, size_t bytes) {
        if (bytes < ((size_t)1 << 20)) { memcpy(dst, src, bytes); return; }
        const size_t half = (bytes / 2) & ~(size_t)63;
        try {   // (thread creation can throw std::system_error: nothing may cross the C ABI)
            std::thread helper([=]() { memcpy(static_cast<char *>(dst) + half, static_cast<const char *>(src) + half, bytes - half); });
            memcpy(dst, src, half);
            helper.join();
        } catch (...) {
            memcpy(dst, src, bytes);
        }
    };
    // results of the chunk a set holds -> the caller's arrays (after its stream has drained)
    const auto drain = [&](int i) -> int {
        if (!fl[i].n) return CVTMI_OK;
        OpqScratch &S = *lease[i].s;
        CVTMI_HIP(stream_wait(lease[i].st));
        copy_out(dist + fl[i].q0 * k, S.io_pin.as<char>() + qb, (size_t)fl[i].n * k * sizeof(float));
        copy_out(ids + fl[i].q0 * k, S.io_pin.as<char>() + qb + db, (size_t)fl[i].n * k * sizeof(int64_t));
        fl[i].n = 0;
        return CVTMI_OK;
    };
    // Small batches (the reference's call pattern: a handful of frames per Query; here whatever takes the small-batch path, up to 128
    // queries): the copies are a third of such a call.  The table kernel reads the queries and the selection kernel writes the results straight from / to the pinned staging area (page-locked
    // host memory is device-visible: one PCIe read of the queries, posted writes of the lists) -- no copy engine in the chain.
    if (chunks == 1 && tune_opq_small_zero_copy.geti() && h->n > 0 && scans_chosen(h, nq, k)) {
        OpqScratch &S = *lease[0].s;
        hipStream_t st = lease[0].st;
        void *pin_dev = nullptr;
        if (hipHostGetDevicePointer(&pin_dev, S.io_pin.p, 0) == hipSuccess && pin_dev) {
            char *pin = S.io_pin.as<char>(), *pd = static_cast<char *>(pin_dev);
            const size_t qn = (size_t)nq * D * sizeof(float), dn = (size_t)nq * k * sizeof(float), in = (size_t)nq * k * sizeof(int64_t);
            memcpy(pin, q, qn);
            CVTMI_TRY(opq_search_leased(h, S, reinterpret_cast<const float *>(pd), nq, rotate, k, reinterpret_cast<float *>(pd + qb),
                                        reinterpret_cast<int64_t *>(pd + qb + db), st));
            CVTMI_HIP(stream_wait(st));
            memcpy(dist, pin + qb, dn);
            memcpy(ids, pin + qb + db, in);
            return CVTMI_OK;
        }
        (void)hipGetLastError();
    }
    int c = 0;
    // a piece that fails leaves earlier pieces in flight, writing into the caller's arrays or the staging areas: nothing is handed
    // back (and no lease released) before both streams have drained
    const auto fail_after_drain = [&](int rc) -> int {
        for (int j = 0; j < nsets; ++j) (void)stream_wait(lease[j].st);
        return rc;
    };
    for (int64_t q0 = 0; q0 < nq; q0 += per, ++c) {
        const int i = c % nsets;
        const int64_t n = std::min(per, nq - q0);
        CVTMI_TRY(drain(i));   // the set's previous chunk: its staging area is about to be overwritten
        OpqScratch &S = *lease[i].s;
        hipStream_t st = lease[i].st;
        const void *src = q + q0 * D;
        if (zd && c >= nsets) CVTMI_HIP(stream_wait(st));   // (zero-copy pieces: the set's query upload of two pieces ago must have been consumed)
        if (!q_pinned) { memcpy(S.io_pin.p, src, (size_t)n * D * sizeof(float)); src = S.io_pin.p; }
        CVTMI_HIP(hipMemcpyAsync(S.io_q.p, src, (size_t)n * D * sizeof(float), hipMemcpyHostToDevice, st));
        if (zd) {   // (normally one piece: the final wait below is all that is left)
            const int rc = opq_search_leased(h, S, S.io_q.as<float>(), n, rotate, k, zd + q0 * k, zi + q0 * k, st);
            if (rc != CVTMI_OK) return fail_after_drain(rc);
            continue;
        }
        {
            const int rc = opq_search_leased(h, S, S.io_q.as<float>(), n, rotate, k, S.io_d.as<float>(), S.io_i.as<int64_t>(), st);
            if (rc != CVTMI_OK) return fail_after_drain(rc);
        }
        if (out_pinned) {  // straight into the caller's page-locked arrays; the final drain only waits for the streams
            CVTMI_HIP(hipMemcpyAsync(dist + q0 * k, S.io_d.p, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, st));
            CVTMI_HIP(hipMemcpyAsync(ids + q0 * k, S.io_i.p, (size_t)n * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        } else {
            CVTMI_HIP(hipMemcpyAsync(S.io_pin.as<char>() + qb, S.io_d.p, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost, st));
            CVTMI_HIP(hipMemcpyAsync(S.io_pin.as<char>() + qb + db, S.io_i.p, (size_t)n * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            fl[i].q0 = q0; fl[i].n = n;
        }
    }
    if (out_pinned)
        for (int i = 0; i < nsets; ++i) CVTMI_HIP(stream_wait(lease[i].st));
    for (int i = 0; i < nsets; ++i) CVTMI_TRY(drain((c + i) % nsets));
    return CVTMI_OK;
}

// row-sharded search: the local scan writes its lists straight into this rank's slot of the communicator's gather buffer,
// then one all-gather + merge (shard.hip).  Lock order: communicator first, then the handle -- collectives on one
// communicator leave in the order its lock was taken, which therefore has to be the same on every rank (drive one
// communicator from one thread, or issue the searches that share it in one order everywhere).
int cvtmi_opq_search_sharded_dev(cvtmi_opq_t h, cvtmi_comm_t c, const float *q, int64_t nq, int rotate, int k, float *dist,
                                 int64_t *ids, void *stream)
{
    CVTMI_TRY(comm_validate(c));
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded: null handle");
    if (nq < 0 || (nq > 0 && (!dist || !ids))) return fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search_sharded: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (nq == 0) return CVTMI_OK;
    Serial serial_c(*comm_sync(c), (hipStream_t)stream);
    CHECK_H(h);
    if (comm_world(c) == 1 && !comm_has_transport(c)) return cvtmi_opq_search_dev(h, q, nq, rotate, k, dist, ids, stream);
    // from here on every rank reaches the collective, whatever its local search did
    int rc = comm_device(c) != h->device ? fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded: handle and communicator live on different devices") : CVTMI_OK;
    float *sd = nullptr;
    int64_t *si = nullptr;
    if (rc == CVTMI_OK) rc = !q ? fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded: null queries") : sharded_local_failure(c);
    if (rc == CVTMI_OK) rc = comm_local_slot(c, nq, k, &sd, &si);
    if (rc == CVTMI_OK) rc = cvtmi_opq_search_dev(h, q, nq, rotate, k, sd, si, stream);
    return comm_exchange_merge(c, nq, k, rc, dist, ids, (hipStream_t)stream);
}

int cvtmi_opq_search_sharded(cvtmi_opq_t h, cvtmi_comm_t c, const float *q, int64_t nq, int rotate, int k, float *dist, int64_t *ids)
{
    CVTMI_TRY(comm_validate(c));
    CHECK_H(h);
    if (nq < 0 || (nq > 0 && (!q || !dist || !ids))) return fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search_sharded: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (nq == 0) return CVTMI_OK;
    Tmp dq, dd, di;
    CVTMI_TRY(dq.upload(q, (size_t)nq * h->m.D * sizeof(float)));
    CVTMI_TRY(dd.alloc((size_t)nq * k * sizeof(float)));
    CVTMI_TRY(di.alloc((size_t)nq * k * sizeof(int64_t)));
    CVTMI_TRY(cvtmi_opq_search_sharded_dev(h, c, dq.as<float>(), nq, rotate, k, dd.as<float>(), di.as<int64_t>(), nullptr));
    CVTMI_HIP(hipMemcpy(dist, dd.p, (size_t)nq * k * sizeof(float), hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(ids, di.p, (size_t)nq * k * sizeof(int64_t), hipMemcpyDeviceToHost));
    {   // the copies above synchronised: a failure the deferred status check saw in THIS search is known now
        Serial serial_c(*comm_sync(c), nullptr);
        CVTMI_TRY(comm_take_deferred(c));
    }
    return CVTMI_OK;
}

int cvtmi_opq_search_sharded_all(cvtmi_opq_t *handles, cvtmi_comm_t *comms, int ndev, const float *q, int64_t nq, int rotate, int k,
                                 float *dist, int64_t *ids)
{
    if (!handles || !comms || ndev < 1) return fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded_all: bad arguments");
    if (nq < 0 || (nq > 0 && (!q || !dist || !ids))) return fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded_all: bad arguments");
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search_sharded_all: k=%d outside 1..%d", k, CVTMI_K_MAX);
    std::vector<int> devices(ndev);
    for (int d = 0; d < ndev; ++d) {
        CVTMI_TRY(comm_validate(comms[d]));
        if (!handles[d]) return fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded_all: null handle %d", d);
        if (comm_world(comms[d]) != ndev || comm_rank(comms[d]) != d || comm_device(comms[d]) != handles[d]->device)
            return fail(CVTMI_EINVAL, "cvtmi_opq_search_sharded_all: communicator %d does not belong to handle %d", d, d);
        devices[d] = handles[d]->device;
    }
    if (nq == 0) return CVTMI_OK;
    return sharded_all(comms, ndev, q, (size_t)nq * handles[0]->m.D * sizeof(float), nq, k, dist, ids, devices.data(),
                       [&](int d, const void *qd, float *sd, int64_t *si) {
                           return cvtmi_opq_search_dev(handles[d], static_cast<const float *>(qd), nq, rotate, k, sd, si, nullptr);
                       });
}

// IVFOPQ::Query / QueryThrehold (IVFOPQ.cpp:213-422) only read the index: like the exhaustive search, a query leases a scratch set
// (rotated frames, probe lists) and holds the handle shared, so callers on several threads proceed side by side.  The list-ordered
// copy of the entries is (re)built under the exclusive lock by the first query after an append.
static int opq_query_prepare(cvtmi_opq_t h, hipStream_t st)
{
    {
        std::shared_lock<std::shared_timed_mutex> rd(h->rw);
        if (h->csr_valid) return CVTMI_OK;
    }
    Serial serial(h->sync, st);
    OpqExclusive excl(h, st);
    return opq_build_csr(h, st);
}
// ... and for the entries that report ENTRY ids (the IVF searches): the first of them on a handle whose list-ordered copy has no
// insertion indices yet rebuilds the copy as well
static int opq_ivf_prepare(cvtmi_opq_t h, hipStream_t st)
{
    {
        std::shared_lock<std::shared_timed_mutex> rd(h->rw);
        if (h->csr_valid && h->csr_entry_valid) return CVTMI_OK;
    }
    Serial serial(h->sync, st);
    OpqExclusive excl(h, st);
    h->want_entry = true;
    return opq_build_csr(h, st);
}
// under the shared lock: the mask covers the entries there are now
static int opq_mask_covers(cvtmi_opq_t h, int64_t mask_words, const char *fn)
{
    if (mask_words < (h->n + 63) / 64)
        return fail(CVTMI_EINVAL, "%s: %lld mask words, %lld entries need %lld", fn, (long long)mask_words, (long long)h->n, (long long)((h->n + 63) / 64));
    return CVTMI_OK;
}
}  // extern "C"

// The way into every entry that reads the list-ordered copy, in this order: the preparation under the exclusive lock (entry_ids: the
// insertion indices are needed too), `rw` shared -- an append between the two sends the call round again, at most 8 times; after that
// the _leased body answers "the index changed" --, the mask length against the entries there are now (mask_words >= 0: a masked search),
// the lease on (stream, host), and run(lease) under both.
template <class F> static int opq_ivf_enter(cvtmi_opq_t h, bool entry_ids, hipStream_t stream, bool host, int64_t mask_words, F &&run)
{
    for (int attempt = 0;; ++attempt) {
        CVTMI_TRY(entry_ids ? opq_ivf_prepare(h, stream) : opq_query_prepare(h, stream));
        std::shared_lock<std::shared_timed_mutex> rd(h->rw);
        if (!(h->csr_valid && (h->csr_entry_valid || !entry_ids)) && attempt < 8) continue;
        if (mask_words >= 0) CVTMI_TRY(opq_mask_covers(h, mask_words, "cvtmi_opq_search_ivf_masked"));
        OpqLease lease;
        CVTMI_TRY(lease.open(h, stream, host));
        return run(lease);
    }
}

extern "C" {

static int opq_query_video_leased(cvtmi_opq_t h, OpqScratch &S, const float *q, int64_t nq, int rotate, int nprobe, int img_num, float *match_score,
                                  hipStream_t st)
{
    if (!h->csr_valid) return fail(CVTMI_EINVAL, "cvtmi_opq_query_video: the index changed while the query was being prepared");
    if (nprobe > h->m.coarseK) nprobe = h->m.coarseK;  // the reference pops an empty heap here (UB)
    if (h->csr_kept > 0 && (h->csr_vmin < 0 || h->csr_vmax >= img_num))
        return fail(CVTMI_EINVAL, "cvtmi_opq_query_video: video id %d outside img_num=%d", h->csr_vmin < 0 ? h->csr_vmin : h->csr_vmax, img_num);
    const float *q_rot = nullptr;
    CVTMI_TRY(opq_rotate_probe(h, S, q, nq, rotate, nprobe, st, &q_rot));
    return launch_query_video(h->m, q_rot, nq, nprobe, S.s_probe.as<int32_t>(), h->csr_off.as<int64_t>(), h->csr_codes.as<uint8_t>(),
                              h->csr_videos.as<int32_t>(), img_num, match_score, h->csr_longest, st);
}

// host = true: frames in and the dense [frames][videos] score matrix out through the leased set's staging buffers (kept between
// calls: the reference's own call is a handful of frames, a device allocation per call would cost more than the query)
static int opq_query_video_common(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int img_num, float *match_score, hipStream_t stream,
                                  bool host)
{
    if (nq < 0 || img_num < 0 || (nq > 0 && img_num > 0 && (!q || !match_score)))
        return fail(CVTMI_EINVAL, "cvtmi_opq_query_video: bad arguments");
    if (nprobe < 1) return fail(CVTMI_EINVAL, "cvtmi_opq_query_video: nprobe=%d", nprobe);
    if (nq == 0 || img_num == 0) return CVTMI_OK;
    const auto run = [&](OpqScratch &S, const float *dq, const void *, float *ms, int64_t *, hipStream_t st) {
        return opq_query_video_leased(h, S, dq, nq, rotate, nprobe, img_num, ms, st);
    };
    return opq_ivf_enter(h, false, stream, host, -1, [&](OpqLease &lease) {
        if (!host) return run(*lease.s, q, nullptr, match_score, nullptr, lease.st);
        return host_call(lease, q, (size_t)nq * h->m.D * sizeof(float), HostUpload{}, match_score, (size_t)nq * img_num * sizeof(float), nullptr, 0, run);
    });
}

int cvtmi_opq_query_video_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int img_num, float *match_score,
                              void *stream)
{
    CHECK_H(h);
    return opq_query_video_common(h, q, nq, rotate, nprobe, img_num, match_score, (hipStream_t)stream, false);
}

int cvtmi_opq_query_video(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int img_num,
                          float *match_score)
{
    CHECK_H(h);
    return opq_query_video_common(h, q, nq, rotate, nprobe, img_num, match_score, nullptr, true);
}

// ---- cvtmi_opq_rank_videos: the whole query of multi_frame_index_test.cpp:51-84 for several query videos (video_rank.hip) ----
// The frames are rotated and probed once, as cvtmi_opq_query_video over all of them would; the dense score rows exist a chunk of whole
// frames at a time (s_rank_ms), each chunk is folded into the totals of its segments in frame order, and launch_topk_select reads the
// totals.  Without a `total` of the caller's the totals of a group of segments live in s_rank_tot and the group is selected before the
// next begins.  Both areas are bounded by "ivf_part_cap_mb" (at least one frame / one segment).  A search: shared lock, leased set.
struct RankPlan {
    int64_t frames_per_chunk = 1, segs_per_group = 1, chunks = 0;
    size_t ms_bytes = 0, tot_bytes = 0;
};
static RankPlan plan_rank(const int64_t *seg_off, int64_t nseg, int img_num, bool own_totals, size_t cap_bytes)
{
    RankPlan p;
    const size_t row = (size_t)img_num * sizeof(float);
    const int64_t fit = std::max<int64_t>(1, (int64_t)(cap_bytes / row));
    const int64_t frames = seg_off[nseg];
    p.frames_per_chunk = std::min(fit, std::max<int64_t>(frames, 1));
    p.segs_per_group = own_totals ? std::min(fit, nseg) : nseg;
    for (int64_t g0 = 0; g0 < nseg; g0 += p.segs_per_group) {
        const int64_t g1 = std::min(nseg, g0 + p.segs_per_group);
        p.chunks += blocks_for(seg_off[g1] - seg_off[g0], p.frames_per_chunk);
    }
    p.ms_bytes = frames > 0 ? (size_t)p.frames_per_chunk * row : 0;
    p.tot_bytes = own_totals ? (size_t)p.segs_per_group * row : 0;
    return p;
}

static int opq_rank_videos_leased(cvtmi_opq_t h, OpqScratch &S, const float *q, const int64_t *seg_off, int64_t nseg, int rotate, int nprobe, int img_num,
                                  int k, float *score, int64_t *video, float *total, hipStream_t st)
{
    if (!h->csr_valid) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: the index changed while the query was being prepared");
    if (h->csr_kept > 0 && (h->csr_vmin < 0 || h->csr_vmax >= img_num))
        return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: video id %d outside img_num=%d", h->csr_vmin < 0 ? h->csr_vmin : h->csr_vmax, img_num);
    const int64_t frames = seg_off[nseg];
    const RankPlan plan = plan_rank(seg_off, nseg, img_num, !total, (size_t)tune_ivf_part_cap_mb.geti() << 20);
    {
        std::lock_guard<std::mutex> g(h->pool.mu);
        const int64_t v[4] = { plan.chunks, plan.frames_per_chunk, (int64_t)plan.ms_bytes, (int64_t)plan.tot_bytes };
        for (int i = 0; i < 4; ++i) h->rank_last[i] = v[i];
    }
    if (plan.ms_bytes) CVTMI_TRY(S.s_rank_ms.reserve(plan.ms_bytes));
    if (plan.tot_bytes) CVTMI_TRY(S.s_rank_tot.reserve(plan.tot_bytes));
    CVTMI_TRY(S.s_rank_seg.reserve(((size_t)nseg + 1) * sizeof(int64_t)));
    int64_t *seg_dev = S.s_rank_seg.as<int64_t>();
    CVTMI_TRY(launch_video_seg_table(seg_off, nseg + 1, seg_dev, st));
    const float *q_rot = nullptr;
    if (frames > 0) CVTMI_TRY(opq_rotate_probe(h, S, q, frames, rotate, nprobe, st, &q_rot));
    float *ms = S.s_rank_ms.as<float>();
    for (int64_t g0 = 0; g0 < nseg; g0 += plan.segs_per_group) {
        const int64_t g1 = std::min(nseg, g0 + plan.segs_per_group);
        float *tot = total ? total : S.s_rank_tot.as<float>();   // row of segment s: tot + (s - tot_s0) * img_num
        const int64_t tot_s0 = total ? 0 : g0;
        bool empty = false;
        for (int64_t s = g0; s < g1 && !empty; ++s) empty = seg_off[s] == seg_off[s + 1];
        if (empty) CVTMI_TRY(launch_video_total_zero(seg_dev, g0, g1, img_num, tot, tot_s0, st));
        int64_t s_lo = g0;
        for (int64_t c0 = seg_off[g0]; c0 < seg_off[g1]; c0 += plan.frames_per_chunk) {
            const int64_t c1 = std::min(seg_off[g1], c0 + plan.frames_per_chunk);
            CVTMI_TRY(launch_query_video(h->m, q_rot + c0 * h->m.D, c1 - c0, nprobe, S.s_probe.as<int32_t>() + c0 * nprobe, h->csr_off.as<int64_t>(),
                                         h->csr_codes.as<uint8_t>(), h->csr_videos.as<int32_t>(), img_num, ms, h->csr_longest, st));
            while (seg_off[s_lo + 1] <= c0) ++s_lo;           // the segment of frame c0 ...
            int64_t s_hi = s_lo + 1;
            while (s_hi < g1 && seg_off[s_hi] < c1) ++s_hi;   // ... up to the segment of frame c1 - 1
            CVTMI_TRY(launch_video_frame_sum(ms, c0, c1, seg_dev, s_lo, s_hi, img_num, tot, tot_s0, st));
        }
        CVTMI_TRY(launch_topk_select(tot + (g0 - tot_s0) * img_num, nullptr, g1 - g0, img_num, k, score + g0 * k, video + g0 * k, st));
    }
    return CVTMI_OK;
}

// arguments first, before anything touches the device
static int opq_rank_videos_check(cvtmi_opq_t h, const float *q, const int64_t *seg_off, int64_t nseg, int *nprobe, int img_num, int k, const float *score,
                                 const int64_t *video)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: null handle");
    if (!seg_off || !score || !video || nseg < 0) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: bad arguments");
    if (seg_off[0] != 0) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: seg_off[0]=%lld, not 0", (long long)seg_off[0]);
    for (int64_t s = 0; s < nseg; ++s)
        if (seg_off[s + 1] < seg_off[s]) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: seg_off decreases at segment %lld", (long long)s);
    if (!q && seg_off[nseg] > 0) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: null frames");
    if (*nprobe < 1) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: nprobe=%d", *nprobe);
    if (img_num < 1) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: img_num=%d", img_num);
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EINVAL, "cvtmi_opq_rank_videos: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (h->m.K > 256) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_rank_videos: K=%d > 256", h->m.K);
    if (*nprobe > h->m.coarseK) *nprobe = h->m.coarseK;
    if (*nprobe > 128) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_rank_videos: nprobe=%d outside 1..128", *nprobe);
    return CVTMI_OK;
}

// host = true: frames up and the lists (and the totals, where the caller wants them) down through the leased set's staging buffers
static int opq_rank_videos_common(cvtmi_opq_t h, const float *q, const int64_t *seg_off, int64_t nseg, int rotate, int nprobe, int img_num, int k, float *score,
                                  int64_t *video, float *total, hipStream_t stream, bool host)
{
    CVTMI_TRY(opq_rank_videos_check(h, q, seg_off, nseg, &nprobe, img_num, k, score, video));
    CVTMI_TRY(use_device(h->device));
    if (nseg == 0) return CVTMI_OK;
    return opq_ivf_enter(h, false, stream, host, -1, [&](OpqLease &lease) -> int {
        OpqScratch &S = *lease.s;
        hipStream_t st = lease.st;
        if (!host) return opq_rank_videos_leased(h, S, q, seg_off, nseg, rotate, nprobe, img_num, k, score, video, total, st);
        const size_t qb = (size_t)seg_off[nseg] * h->m.D * sizeof(float), sb = (size_t)nseg * k * sizeof(float), vb = (size_t)nseg * k * sizeof(int64_t);
        const size_t tb = total ? (size_t)nseg * img_num * sizeof(float) : 0;
        if (qb) CVTMI_TRY(S.io_q.reserve(qb));
        CVTMI_TRY(S.io_d.reserve(sb));
        CVTMI_TRY(S.io_i.reserve(vb));
        if (tb) CVTMI_TRY(S.io_t.reserve(tb));
        if (qb) CVTMI_HIP(hipMemcpyAsync(S.io_q.p, q, qb, hipMemcpyHostToDevice, st));
        CVTMI_TRY(opq_rank_videos_leased(h, S, S.io_q.as<float>(), seg_off, nseg, rotate, nprobe, img_num, k, S.io_d.as<float>(), S.io_i.as<int64_t>(),
                                         tb ? S.io_t.as<float>() : nullptr, st));
        CVTMI_HIP(hipMemcpyAsync(score, S.io_d.p, sb, hipMemcpyDeviceToHost, st));
        CVTMI_HIP(hipMemcpyAsync(video, S.io_i.p, vb, hipMemcpyDeviceToHost, st));
        if (tb) CVTMI_HIP(hipMemcpyAsync(total, S.io_t.p, tb, hipMemcpyDeviceToHost, st));
        CVTMI_HIP(stream_wait(st));
        return CVTMI_OK;
    });
}

int cvtmi_opq_rank_videos_dev(cvtmi_opq_t h, const float *q, const int64_t *seg_off, int64_t nseg, int rotate, int nprobe, int img_num, int k, float *score,
                              int64_t *video, float *total, void *stream)
{
    return opq_rank_videos_common(h, q, seg_off, nseg, rotate, nprobe, img_num, k, score, video, total, (hipStream_t)stream, false);
}

int cvtmi_opq_rank_videos(cvtmi_opq_t h, const float *q, const int64_t *seg_off, int64_t nseg, int rotate, int nprobe, int img_num, int k, float *score,
                          int64_t *video, float *total)
{
    return opq_rank_videos_common(h, q, seg_off, nseg, rotate, nprobe, img_num, k, score, video, total, nullptr, true);
}

int cvtmi_opq_last_rank(cvtmi_opq_t h, int64_t out[4])
{
    if (!h || !out) return fail(CVTMI_EINVAL, "cvtmi_opq_last_rank: null");
    copy_last(h->pool, h->rank_last, out);
    return CVTMI_OK;
}

// ---- IVF search: the k nearest ENTRIES of the nprobe nearest lists (ivf_search.hip) ----
// Concurrency as for query_video: shared lock + leased scratch set; the first search after an append (or the first IVF search of
// a handle whose list-ordered copy has no insertion indices yet) rebuilds the copy under the exclusive lock (opq_ivf_enter).
// mask != null (cvtmi_opq_search_ivf_masked): the caller's words on the device, at least ceil(n / 64) of them.  What is derived from
// them -- the mask in list order -- lives in the leased set like the partial lists: searches with different masks run side by side
static int opq_search_ivf_leased(cvtmi_opq_t h, OpqScratch &S, const float *q, int64_t nq, int rotate, int nprobe, int k, float *dist, int64_t *ids,
                                 hipStream_t st, const uint64_t *mask = nullptr)
{
    if (!h->csr_valid || !h->csr_entry_valid) return fail(CVTMI_EINVAL, "cvtmi_opq_search_ivf: the index changed while the search was being prepared");
    const size_t lmb = mask ? ivf_mask_bytes(h->csr_kept) : 0;
    if (mask) {
        CVTMI_TRY(S.s_masked.reserve(lmb));
        CVTMI_TRY(launch_ivf_mask_order(mask, h->csr_entry.as<uint32_t>(), h->csr_kept, S.s_masked.as<uint64_t>(), st));
    }
    const float *q_rot = nullptr;
    CVTMI_TRY(opq_rotate_probe(h, S, q, nq, rotate, nprobe, st, &q_rot));
    const IvfPlan plan = plan_ivf_search(nq, nprobe, k, h->csr_longest, (size_t)tune_ivf_part_cap_mb.geti() << 20);
    const size_t pb = ivf_part_bytes(plan, nq, k);
    if (pb) CVTMI_TRY(S.s_ivf.reserve(pb));
    {
        std::lock_guard<std::mutex> g(h->pool.mu);
        const int64_t v[8] = { plan.rule, plan.G, plan.groups, plan.pieces, plan.rows_per_piece, plan.parts(), (int64_t)pb, (int64_t)h->csr_entry.cap };
        if (mask) {
            for (int i = 0; i < 6; ++i) h->ivf_masked_last[i] = v[i];
            h->ivf_masked_last[6] = (int64_t)pb; h->ivf_masked_last[7] = (int64_t)lmb;
        } else {
            for (int i = 0; i < 8; ++i) h->ivf_last[i] = v[i];
        }
    }
    return launch_ivf_search(h->m, q_rot, nq, nprobe, S.s_probe.as<int32_t>(), h->csr_off.as<int64_t>(), h->csr_codes.as<uint8_t>(),
                             h->csr_entry.as<uint32_t>(), k, h->id_base, plan, pb ? S.s_ivf.p : nullptr, dist, ids, st,
                             mask ? S.s_masked.as<uint64_t>() : nullptr);
}
// arguments first, before anything touches the device
static int opq_search_ivf_check(cvtmi_opq_t h, const float *q, int64_t nq, int *nprobe, int k, const float *dist, const int64_t *ids)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_opq_search_ivf: null handle");
    if (!q || !dist || !ids || nq < 0) return fail(CVTMI_EINVAL, "cvtmi_opq_search_ivf: bad arguments");
    if (*nprobe < 1) return fail(CVTMI_EINVAL, "cvtmi_opq_search_ivf: nprobe=%d", *nprobe);
    if (k < 1 || k > CVTMI_K_MAX) return fail(CVTMI_EINVAL, "cvtmi_opq_search_ivf: k=%d outside 1..%d", k, CVTMI_K_MAX);
    if (*nprobe > h->m.coarseK) *nprobe = h->m.coarseK;
    if (*nprobe > 128) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search_ivf: nprobe=%d outside 1..128", *nprobe);
    if (h->m.K > 256 || h->m.M > 16) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search_ivf: K=%d M=%d outside K <= 256, M <= 16", h->m.K, h->m.M);
    if (h->n >= ((int64_t)1 << 32)) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_search_ivf: %lld entries: ids travel as 32-bit payloads", (long long)h->n);
    return CVTMI_OK;
}

// ... of the masked search (cvtmi_opq_search_ivf_masked): the k nearest entries of the probed lists among those a bitmap of insertion
// indices allows.  A search like cvtmi_opq_search_ivf: same preparation, shared lock, leased set; the mask's length is checked under the lock.
static int opq_ivf_masked_check(cvtmi_opq_t h, const float *q, int64_t nq, int *nprobe, int k, const uint64_t *mask, int64_t mask_words, const float *dist,
                                const int64_t *ids)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_opq_search_ivf_masked: null handle");
    if (mask_words < 0 || (nq > 0 && !mask)) return fail(CVTMI_EINVAL, "cvtmi_opq_search_ivf_masked: bad arguments");
    return opq_search_ivf_check(h, q, nq, nprobe, k, dist, ids);
}

// The four entries of the two searches.  host = true: queries (and the mask words that can hold an entry: the words behind them are
// never read) up, the two result arrays down, through the leased set's staging buffers and its own stream
static int opq_search_ivf_common(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k, bool masked, const uint64_t *mask,
                                 int64_t mask_words, float *dist, int64_t *ids, hipStream_t stream, bool host)
{
    if (masked) CVTMI_TRY(opq_ivf_masked_check(h, q, nq, &nprobe, k, mask, mask_words, dist, ids));
    else CVTMI_TRY(opq_search_ivf_check(h, q, nq, &nprobe, k, dist, ids));
    CVTMI_TRY(use_device(h->device));
    if (nq == 0) return CVTMI_OK;
    const auto run = [&](OpqScratch &S, const float *dq, const void *dm, float *dd, int64_t *di, hipStream_t st) {
        return opq_search_ivf_leased(h, S, dq, nq, rotate, nprobe, k, dd, di, st, static_cast<const uint64_t *>(dm));
    };
    return opq_ivf_enter(h, true, stream, host, masked ? mask_words : -1, [&](OpqLease &lease) {
        if (!host) return run(*lease.s, q, mask, dist, ids, lease.st);
        const HostUpload words = masked ? HostUpload{ &lease.s->io_m, mask, (size_t)((h->n + 63) / 64) * 8 } : HostUpload{};
        return host_call(lease, q, (size_t)nq * h->m.D * sizeof(float), words, dist, (size_t)nq * k * sizeof(float), ids, (size_t)nq * k * sizeof(int64_t), run);
    });
}

int cvtmi_opq_search_ivf_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k, float *dist, int64_t *ids, void *stream)
{
    return opq_search_ivf_common(h, q, nq, rotate, nprobe, k, false, nullptr, 0, dist, ids, (hipStream_t)stream, false);
}

int cvtmi_opq_search_ivf(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k, float *dist, int64_t *ids)
{
    return opq_search_ivf_common(h, q, nq, rotate, nprobe, k, false, nullptr, 0, dist, ids, nullptr, true);
}

int cvtmi_opq_last_ivf_plan(cvtmi_opq_t h, int64_t out[8])
{
    if (!h || !out) return fail(CVTMI_EINVAL, "cvtmi_opq_last_ivf_plan: null");
    copy_last(h->pool, h->ivf_last, out);
    out[7] = (int64_t)h->csr_entry.cap;
    return CVTMI_OK;
}

int cvtmi_opq_ivf_plan(int64_t nq, int nprobe, int k, int64_t longest_list, int cus, int64_t out[6])
{
    if (!out || nq < 1 || nprobe < 1 || k < 1 || k > CVTMI_K_MAX || longest_list < 0) return fail(CVTMI_EINVAL, "cvtmi_opq_ivf_plan: bad arguments");
    const IvfPlan p = plan_ivf_search(nq, nprobe, k, longest_list, (size_t)tune_ivf_part_cap_mb.geti() << 20, cus > 0 ? cus : 256);
    const int64_t v[6] = { p.rule, p.G, p.groups, p.pieces, p.rows_per_piece, p.parts() };
    for (int i = 0; i < 6; ++i) out[i] = v[i];
    return CVTMI_OK;
}

int cvtmi_opq_search_ivf_masked_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k, const uint64_t *mask, int64_t mask_words,
                                    float *dist, int64_t *ids, void *stream)
{
    return opq_search_ivf_common(h, q, nq, rotate, nprobe, k, true, mask, mask_words, dist, ids, (hipStream_t)stream, false);
}

int cvtmi_opq_search_ivf_masked(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, int k, const uint64_t *mask, int64_t mask_words,
                                float *dist, int64_t *ids)
{
    return opq_search_ivf_common(h, q, nq, rotate, nprobe, k, true, mask, mask_words, dist, ids, nullptr, true);
}

int cvtmi_opq_last_ivf_masked(cvtmi_opq_t h, int64_t out[8])
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_opq_last_ivf_masked: null handle");
    if (!out) return fail(CVTMI_EINVAL, "cvtmi_opq_last_ivf_masked: null");
    copy_last(h->pool, h->ivf_masked_last, out);
    return CVTMI_OK;
}

// ---- the bitmap of a set of video ids: the mark step of the removal on a leased scratch set (the handle does not change) ----
static int opq_mask_videos_check(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, const uint64_t *mask, int64_t mask_words)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_opq_mask_videos: null handle");
    if (nv < 0 || mask_words < 0 || (nv > 0 && !video_ids) || (mask_words > 0 && !mask)) return fail(CVTMI_EINVAL, "cvtmi_opq_mask_videos: bad arguments");
    return CVTMI_OK;
}

// table: the distinct ids of the set, ascending, in host memory; mask: a device pointer of mask_words words.  Under the shared lock
static int opq_mask_videos_leased(cvtmi_opq_t h, OpqScratch &S, const int32_t *table, int64_t T, uint64_t *mask, int64_t mask_words, hipStream_t st)
{
    if (mask_words == 0) return CVTMI_OK;
    if (h->n == 0 || T == 0) {
        CVTMI_HIP(hipMemsetAsync(mask, 0, (size_t)mask_words * 8, st));
        return CVTMI_OK;
    }
    const RmPlan p = rm_plan(h->n, 0, T, 0);   // the mark's areas alone (everything before off_codes): no row moves
    CVTMI_TRY(S.s_masked.reserve(p.off_codes));
    void *W = S.s_masked.p;
    CVTMI_HIP(hipMemcpyAsync(static_cast<char *>(W) + p.off_table, table, (size_t)T * 4, hipMemcpyHostToDevice, st));
    CVTMI_TRY(launch_rm_mark_videos(p, W, h->has_videos ? h->videos.as<int32_t>() : nullptr, st));
    return launch_flat_masked_copy(p, W, mask, mask_words, st);
}

int cvtmi_opq_mask_videos_dev(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, uint64_t *mask, int64_t mask_words, void *stream)
{
    CVTMI_TRY(opq_mask_videos_check(h, video_ids, nv, mask, mask_words));
    CVTMI_TRY(use_device(h->device));
    hipStream_t st = (hipStream_t)stream;
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    CVTMI_TRY(opq_mask_covers(h, mask_words, "cvtmi_opq_mask_videos"));
    OpqLease lease;
    CVTMI_TRY(lease.open(h, st, false));
    std::vector<int32_t> tab;
    if (nv > 0 && h->n > 0 && mask_words > 0) CVTMI_TRY(sorted_unique_dev("cvtmi_opq_mask_videos", video_ids, nv, tab, st));
    CVTMI_TRY(opq_mask_videos_leased(h, *lease.s, tab.data(), (int64_t)tab.size(), mask, mask_words, st));
    if (!tab.empty()) CVTMI_HIP(stream_wait(st));   // (the table leaves host memory that ends with this call)
    return CVTMI_OK;
}

int cvtmi_opq_mask_videos(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, uint64_t *mask, int64_t mask_words)
{
    CVTMI_TRY(opq_mask_videos_check(h, video_ids, nv, mask, mask_words));
    CVTMI_TRY(use_device(h->device));
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    CVTMI_TRY(opq_mask_covers(h, mask_words, "cvtmi_opq_mask_videos"));
    if (mask_words == 0) return CVTMI_OK;
    if (h->n == 0 || nv == 0) {
        memset(mask, 0, (size_t)mask_words * 8);
        return CVTMI_OK;
    }
    std::vector<int32_t> tab;
    CVTMI_TRY(sorted_unique("cvtmi_opq_mask_videos", video_ids, nv, tab));
    OpqLease lease;
    CVTMI_TRY(lease.open(h, nullptr, true));
    OpqScratch &S = *lease.s;
    hipStream_t st = lease.st;
    const int64_t words = (h->n + 63) / 64;   // (the words that can hold an entry)
    CVTMI_TRY(S.io_m.reserve((size_t)words * 8));
    CVTMI_TRY(opq_mask_videos_leased(h, S, tab.data(), (int64_t)tab.size(), S.io_m.as<uint64_t>(), words, st));
    return mask_host_finish(S.io_m, words, mask, mask_words, st);
}

// ---- refine: R ADC candidates per query (IVF lists, or the exhaustive scan for nprobe == 0), exact finish against a flat index ----
// The candidate lists stay in the leased set (s_ref_d, s_ref_i).  Lock order: THIS handle's shared lock (and lease) first, the flat
// handle's -- its preparation under the exclusive lock included -- inside it; nothing takes the two the other way round.
static int opq_refine_check(cvtmi_opq_t h, cvtmi_flat_t flat, const float *q, int64_t nq, int *nprobe, int k, int R, const float *dist, const int64_t *labels)
{
    if (!h || !flat) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: null handle");
    if (nq < 0 || (nq > 0 && (!q || !dist || !labels))) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: bad arguments");
    if (k < 1 || R < k || R > CVTMI_K_MAX) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: 1 <= k <= R <= %d does not hold for k=%d R=%d", CVTMI_K_MAX, k, R);
    if (*nprobe < 0) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: nprobe=%d", *nprobe);
    if (*nprobe == 0 && h->m.coarseK != 1) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: nprobe == 0 is the exhaustive scan, which needs coarseK == 1");
    if (flat->metric != CVTMI_METRIC_IP && flat->metric != CVTMI_METRIC_L2F) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: the flat index must hold fp32 rows");
    if (flat->D != h->m.D) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: flat D=%d, model D=%d", flat->D, h->m.D);
    if (flat->n != h->n) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: %lld flat rows, %lld entries", (long long)flat->n, (long long)h->n);
    if (flat->device != h->device) return fail(CVTMI_EINVAL, "cvtmi_opq_search_refine: the handles live on different devices");
    if (*nprobe >= 1) {
        float probe_d = 0.0f;   // (the IVF search's own limits; its outputs are the leased lists)
        int64_t probe_i = 0;
        CVTMI_TRY(opq_search_ivf_check(h, q ? q : &probe_d, nq, nprobe, R, &probe_d, &probe_i));
    }
    return CVTMI_OK;
}

// candidates into the leased lists, rerank into (dist, labels): device pointers, stream st; the caller holds h->rw shared
static int opq_refine_leased(cvtmi_opq_t h, cvtmi_flat_t flat, OpqScratch &S, const float *q, int64_t nq, int rotate, int nprobe, int k, int R,
                             float *dist, int64_t *labels, hipStream_t st)
{
    CVTMI_TRY(S.s_ref_d.reserve((size_t)nq * R * sizeof(float)));
    CVTMI_TRY(S.s_ref_i.reserve((size_t)nq * R * sizeof(int64_t)));
    if (nprobe >= 1) CVTMI_TRY(opq_search_ivf_leased(h, S, q, nq, rotate, nprobe, R, S.s_ref_d.as<float>(), S.s_ref_i.as<int64_t>(), st));
    else CVTMI_TRY(opq_search_leased(h, S, q, nq, rotate, R, S.s_ref_d.as<float>(), S.s_ref_i.as<int64_t>(), st));
    return flat_rerank_on_stream(flat, q, nq, S.s_ref_i.as<int64_t>(), R, h->id_base, true, k, dist, labels, st);
}

static int opq_refine_common(cvtmi_opq_t h, cvtmi_flat_t flat, const float *q, int64_t nq, int rotate, int nprobe, int k, int R, float *dist,
                             int64_t *labels, hipStream_t stream, bool host)
{
    CVTMI_TRY(opq_refine_check(h, flat, q, nq, &nprobe, k, R, dist, labels));
    CVTMI_TRY(use_device(h->device));
    if (nq == 0) return CVTMI_OK;
    const auto run = [&](OpqScratch &S, const float *dq, const void *, float *dd, int64_t *dl, hipStream_t st) {
        return opq_refine_leased(h, flat, S, dq, nq, rotate, nprobe, k, R, dd, dl, st);
    };
    const auto leased = [&](OpqLease &lease) {
        if (!host) return run(*lease.s, q, nullptr, dist, labels, lease.st);
        return host_call(lease, q, (size_t)nq * h->m.D * sizeof(float), HostUpload{}, dist, (size_t)nq * k * sizeof(float), labels, (size_t)nq * k * sizeof(int64_t), run);
    };
    if (nprobe >= 1) return opq_ivf_enter(h, true, stream, host, -1, leased);   // (the way in of cvtmi_opq_search_ivf)
    CVTMI_TRY(opq_prepare(h, nq, R, stream));   // nprobe == 0: the way in of cvtmi_opq_search_dev
    std::shared_lock<std::shared_timed_mutex> rd(h->rw);
    OpqLease lease;
    CVTMI_TRY(lease.open(h, stream, host));
    return leased(lease);
}

int cvtmi_opq_search_refine_dev(cvtmi_opq_t h, cvtmi_flat_t flat, const float *q, int64_t nq, int rotate, int nprobe, int k, int R, float *dist,
                                int64_t *labels, void *stream)
{
    return opq_refine_common(h, flat, q, nq, rotate, nprobe, k, R, dist, labels, (hipStream_t)stream, false);
}

int cvtmi_opq_search_refine(cvtmi_opq_t h, cvtmi_flat_t flat, const float *q, int64_t nq, int rotate, int nprobe, int k, int R, float *dist,
                            int64_t *labels)
{
    return opq_refine_common(h, flat, q, nq, rotate, nprobe, k, R, dist, labels, nullptr, true);
}

// ---- range search: every entry of the probed lists under a score radius (ivf_range.hip) ----
// Concurrency and preparation are the IVF search's.  A call is a count (probe order, scan, offsets: lims is complete on the device)
// and, where the caller gave room, a fill (fill + rescan, both predicated on the device on lims[nq] <= cap).
struct OpqRangeCall {
    IvfRangePlan plan;
    IvfRangeBufs bufs;
    const float *q_rot = nullptr;
    int64_t *lims_scratch = nullptr;   // nq + 1 words behind the carved areas (the host entry's device lims)
};
static int opq_range_count_leased(cvtmi_opq_t h, OpqScratch &S, const float *q, int64_t nq, int rotate, int nprobe, float radius, bool spill,
                                  int64_t *lims, OpqRangeCall &c, hipStream_t st)
{
    if (!h->csr_valid || !h->csr_entry_valid) return fail(CVTMI_EINVAL, "cvtmi_opq_range_search_ivf: the index changed while the search was being prepared");
    CVTMI_TRY(opq_rotate_probe(h, S, q, nq, rotate, nprobe, st, &c.q_rot));
    c.plan = plan_ivf_range(nq, nprobe, h->csr_longest, spill ? tune_ivf_range_spill.get() : 0, (size_t)tune_ivf_part_cap_mb.geti() << 20);
    const size_t carved = ivf_range_carve(nullptr, c.plan, nq, nprobe, nullptr);
    CVTMI_TRY(S.s_range.reserve(carved + ((size_t)nq + 1) * sizeof(int64_t)));
    ivf_range_carve(S.s_range.p, c.plan, nq, nprobe, &c.bufs);
    c.lims_scratch = reinterpret_cast<int64_t *>(S.s_range.as<char>() + carved);
    {
        std::lock_guard<std::mutex> g(h->pool.mu);
        const IvfPlan &p = c.plan.grid;
        const int64_t v[8] = { p.rule, p.G, p.groups, p.pieces, p.rows_per_piece, p.parts(), c.plan.spill,
                               (int64_t)((size_t)nq * p.parts() * c.plan.spill * sizeof(unsigned long long)) };
        for (int i = 0; i < 8; ++i) h->range_last[i] = v[i];
    }
    return launch_ivf_range_count(h->m, c.q_rot, nq, nprobe, S.s_probe.as<int32_t>(), h->csr_off.as<int64_t>(), h->csr_codes.as<uint8_t>(), radius,
                                  c.plan, c.bufs, lims ? lims : c.lims_scratch, st);
}
static int opq_range_fill_leased(cvtmi_opq_t h, const OpqRangeCall &c, int64_t nq, int nprobe, float radius, const int64_t *lims, int64_t cap,
                                 float *dist, int64_t *ids, int32_t *video, hipStream_t st)
{
    return launch_ivf_range_fill(h->m, c.q_rot, nq, nprobe, h->csr_off.as<int64_t>(), h->csr_codes.as<uint8_t>(), h->csr_entry.as<uint32_t>(),
                                 h->csr_videos.as<int32_t>(), radius, h->id_base, c.plan, c.bufs, lims, cap, dist, ids, video, st);
}
// arguments first, before anything touches the device
static int opq_range_check(cvtmi_opq_t h, const float *q, int64_t nq, int *nprobe, float radius, int64_t cap, const int64_t *lims, const float *dist,
                           const int64_t *ids)
{
    if (!h) return fail(CVTMI_EINVAL, "cvtmi_opq_range_search_ivf: null handle");
    if (!q || !lims || nq < 0 || cap < 0) return fail(CVTMI_EINVAL, "cvtmi_opq_range_search_ivf: bad arguments");
    if (cap > 0 && (!dist || !ids)) return fail(CVTMI_EINVAL, "cvtmi_opq_range_search_ivf: cap=%lld without result arrays", (long long)cap);
    if (*nprobe < 1) return fail(CVTMI_EINVAL, "cvtmi_opq_range_search_ivf: nprobe=%d", *nprobe);
    if (radius != radius) return fail(CVTMI_EINVAL, "cvtmi_opq_range_search_ivf: the radius is NaN");
    if (*nprobe > h->m.coarseK) *nprobe = h->m.coarseK;
    if (*nprobe > 128) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_range_search_ivf: nprobe=%d outside 1..128", *nprobe);
    if (h->m.K > 256 || h->m.M > 16) return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_range_search_ivf: K=%d M=%d outside K <= 256, M <= 16", h->m.K, h->m.M);
    if (h->n >= ((int64_t)1 << 32))
        return fail(CVTMI_EUNSUPPORTED, "cvtmi_opq_range_search_ivf: %lld entries: positions travel as 32-bit payloads", (long long)h->n);
    return CVTMI_OK;
}

int cvtmi_opq_range_search_ivf_dev(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, float radius, int64_t cap, int64_t *lims,
                                   float *dist, int64_t *ids, int32_t *video, void *stream)
{
    CVTMI_TRY(opq_range_check(h, q, nq, &nprobe, radius, cap, lims, dist, ids));
    CVTMI_TRY(use_device(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (nq == 0) {
        CVTMI_HIP(hipMemsetAsync(lims, 0, sizeof(int64_t), st));
        return CVTMI_OK;
    }
    return opq_ivf_enter(h, true, st, false, -1, [&](OpqLease &lease) -> int {
        OpqRangeCall c;
        CVTMI_TRY(opq_range_count_leased(h, *lease.s, q, nq, rotate, nprobe, radius, cap > 0, lims, c, st));
        if (cap == 0) return CVTMI_OK;   // a count-only call
        return opq_range_fill_leased(h, c, nq, nprobe, radius, lims, cap, dist, ids, video, st);
    });
}

// host pointers: the queries go up and lims comes back through the leased set's staging buffers -- the one wait the call needs to
// know whether the result fits; then the three arrays, sized by lims[nq]
int cvtmi_opq_range_search_ivf(cvtmi_opq_t h, const float *q, int64_t nq, int rotate, int nprobe, float radius, int64_t cap, int64_t *lims,
                               float *dist, int64_t *ids, int32_t *video)
{
    CVTMI_TRY(opq_range_check(h, q, nq, &nprobe, radius, cap, lims, dist, ids));
    CVTMI_TRY(use_device(h->device));
    lims[0] = 0;
    if (nq == 0) return CVTMI_OK;
    return opq_ivf_enter(h, true, nullptr, true, -1, [&](OpqLease &lease) -> int {
        OpqScratch &S = *lease.s;
        hipStream_t st = lease.st;
        const size_t qb = (size_t)nq * h->m.D * sizeof(float);
        CVTMI_TRY(S.io_q.reserve(qb));
        CVTMI_HIP(hipMemcpyAsync(S.io_q.p, q, qb, hipMemcpyHostToDevice, st));
        OpqRangeCall c;
        CVTMI_TRY(opq_range_count_leased(h, S, S.io_q.as<float>(), nq, rotate, nprobe, radius, cap > 0, nullptr, c, st));
        const RangeOut outs[] = { { dist, &S.io_d, sizeof(float) }, { ids, &S.io_i, sizeof(int64_t) }, { video, &S.io_v, sizeof(int32_t) } };
        return range_host_finish("cvtmi_opq_range_search_ivf", nq, cap, lims, c.lims_scratch, outs, st, [&](int64_t total) {
            return opq_range_fill_leased(h, c, nq, nprobe, radius, c.lims_scratch, total, S.io_d.as<float>(), S.io_i.as<int64_t>(),
                                         video ? S.io_v.as<int32_t>() : nullptr, st);
        });
    });
}

int cvtmi_opq_last_range_plan(cvtmi_opq_t h, int64_t out[8])
{
    if (!h || !out) return fail(CVTMI_EINVAL, "cvtmi_opq_last_range_plan: null");
    copy_last(h->pool, h->range_last, out);
    return CVTMI_OK;
}

// ---- removal: one stable compaction of the resident arrays on the device (opq_remove.hip) ----
// The set is either a sorted table of distinct video ids (host memory: it is uploaded into the scratch) or a device array of entry
// ids.  Everything the call needs is reserved before the first row moves; the host waits once, for the kept count, BEFORE the move:
// a call that drops nothing then leaves the handle and its derived copies alone.
static int opq_remove_common(cvtmi_opq_t h, const int32_t *table, int64_t T, const int64_t *ids_dev, int64_t n_ids, bool by_ids, int renumber,
                             int64_t *removed, int64_t *remap_dev, hipStream_t st)
{
    if (removed) *removed = 0;
    const int64_t n = h->n;
    if (n == 0) return CVTMI_OK;
    const RmPlan p = rm_plan(n, h->m.M, by_ids ? 0 : T, h->p_rm_chunk);
    CVTMI_TRY(h->rm_scratch.reserve(p.bytes));
    void *S = h->rm_scratch.p;
    if (by_ids) {
        CVTMI_TRY(launch_rm_mark_ids(p, S, ids_dev, n_ids, h->id_base, st));
    } else {
        if (T > 0) CVTMI_HIP(hipMemcpyAsync(static_cast<char *>(S) + p.off_table, table, (size_t)T * 4, hipMemcpyHostToDevice, st));
        CVTMI_TRY(launch_rm_mark_videos(p, S, h->has_videos ? h->videos.as<int32_t>() : nullptr, st));
    }
    int64_t kept = 0;
    CVTMI_HIP(hipMemcpyAsync(&kept, static_cast<char *>(S) + p.off_total, sizeof kept, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(stream_wait(st));
    if (kept < 0 || kept > n) return fail(CVTMI_ESTATE, "cvtmi_opq_remove: kept count %lld of %lld entries", (long long)kept, (long long)n);
    const int64_t dropped = n - kept;
    const bool shift = !by_ids && renumber && T > 0;   // ids of the set below a kept one lower it, whether or not they are in the index
    if (dropped == 0 && !shift) {
        if (remap_dev) CVTMI_TRY(launch_rm_fill_remap(remap_dev, n, 1, st));
        return CVTMI_OK;
    }
    if (!h->has_videos) {   // the implicit video ids (insertion indices) become an array, as for the first explicit id of an append
        CVTMI_TRY(h->videos.grow((size_t)std::max<int64_t>(n, 4096) * 4, 0, st));
        CVTMI_TRY(fill_i32(h->videos.as<int32_t>(), 0, n, 0, 1, st));
        h->has_videos = true;
    }
    if (dropped == 0) {   // only video ids change: the code rows and their rotated / padded copies stay valid
        CVTMI_TRY(launch_rm_renumber(p, S, h->videos.as<int32_t>(), st));
        if (remap_dev) CVTMI_TRY(launch_rm_fill_remap(remap_dev, n, 1, st));
        h->csr_valid = false; h->csr_entry_valid = false;
        return CVTMI_OK;
    }
    CVTMI_TRY(launch_rm_move(p, S, h->codes.as<uint8_t>(), h->has_lists ? h->lists.as<int32_t>() : nullptr, h->videos.as<int32_t>(), shift ? 1 : 0,
                             remap_dev, st));
    h->n = kept;
    h->rot_n = 0; h->pad_n = 0; h->mf_n = 0; h->csr_valid = false; h->csr_entry_valid = false;
    if (removed) *removed = dropped;
    return CVTMI_OK;
}

// arguments first, before anything touches the device
static int opq_remove_check(const char *fn, cvtmi_opq_t h, const void *set, int64_t count)
{
    if (!h) return fail(CVTMI_EINVAL, "%s: null handle", fn);
    if (count < 0 || (count > 0 && !set)) return fail(CVTMI_EINVAL, "%s: bad arguments", fn);
    return CVTMI_OK;
}

int cvtmi_opq_remove_videos_dev(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, int renumber, int64_t *removed, int64_t *remap, void *stream)
{
    CVTMI_TRY(opq_remove_check(__func__, h, video_ids, nv));
    CHECK_H_SERIAL(h, stream);
    hipStream_t st = (hipStream_t)stream;
    std::vector<int32_t> tab;
    if (nv > 0) CVTMI_TRY(sorted_unique_dev("cvtmi_opq_remove_videos", video_ids, nv, tab, st));
    return opq_remove_common(h, tab.data(), (int64_t)tab.size(), nullptr, 0, false, renumber, removed, remap, st);
}

int cvtmi_opq_remove_videos(cvtmi_opq_t h, const int32_t *video_ids, int64_t nv, int renumber, int64_t *removed, int64_t *remap)
{
    CVTMI_TRY(opq_remove_check(__func__, h, video_ids, nv));
    CHECK_H_SERIAL(h, nullptr);
    std::vector<int32_t> tab;
    if (nv > 0) CVTMI_TRY(sorted_unique("cvtmi_opq_remove_videos", video_ids, nv, tab));
    const int64_t n0 = h->n;
    Tmp dm;
    if (remap && n0 > 0) CVTMI_TRY(dm.alloc((size_t)n0 * sizeof(int64_t)));
    CVTMI_TRY(opq_remove_common(h, tab.data(), (int64_t)tab.size(), nullptr, 0, false, renumber, removed, dm.as<int64_t>(), nullptr));
    if (dm.p) CVTMI_HIP(hipMemcpy(remap, dm.p, (size_t)n0 * sizeof(int64_t), hipMemcpyDeviceToHost));
    else CVTMI_HIP(stream_wait(nullptr));
    return CVTMI_OK;
}

int cvtmi_opq_remove_ids_dev(cvtmi_opq_t h, const int64_t *ids, int64_t n_ids, int64_t *removed, int64_t *remap, void *stream)
{
    CVTMI_TRY(opq_remove_check(__func__, h, ids, n_ids));
    CHECK_H_SERIAL(h, stream);
    return opq_remove_common(h, nullptr, 0, ids, n_ids, true, 0, removed, remap, (hipStream_t)stream);
}

int cvtmi_opq_remove_ids(cvtmi_opq_t h, const int64_t *ids, int64_t n_ids, int64_t *removed, int64_t *remap)
{
    CVTMI_TRY(opq_remove_check(__func__, h, ids, n_ids));
    CHECK_H_SERIAL(h, nullptr);
    const int64_t n0 = h->n;
    Tmp di, dm;
    if (n_ids > 0 && n0 > 0) CVTMI_TRY(di.upload(ids, (size_t)n_ids * sizeof(int64_t)));
    if (remap && n0 > 0) CVTMI_TRY(dm.alloc((size_t)n0 * sizeof(int64_t)));
    CVTMI_TRY(opq_remove_common(h, nullptr, 0, di.as<int64_t>(), di.p ? n_ids : 0, true, 0, removed, dm.as<int64_t>(), nullptr));
    if (dm.p) CVTMI_HIP(hipMemcpy(remap, dm.p, (size_t)n0 * sizeof(int64_t), hipMemcpyDeviceToHost));
    else CVTMI_HIP(stream_wait(nullptr));
    return CVTMI_OK;
}

int cvtmi_opq_set_param(cvtmi_opq_t h, const char *name, int64_t value)
{
    if (!h || !name) return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: null");
    if (!strcmp(name, "splits")) { h->p_splits = (int)value; return CVTMI_OK; }
    if (!strcmp(name, "tail_split")) { h->p_tail = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "prerotate")) { h->p_prerot = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "groups_a")) { h->p_groups_a = (int)value; return CVTMI_OK; }
    if (!strcmp(name, "splits_b")) { h->p_splits_b = (int)value; return CVTMI_OK; }
    if (!strcmp(name, "qtile")) {
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
            return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: qtile must be 0, 1, 2, 4 or 8");
        h->p_qtile = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "profile")) { h->p_profile = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "remove_chunk")) {
        if (value < 0 || value > ((int64_t)1 << 32)) return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: remove_chunk must be 0 .. 2^32 rows");
        h->p_rm_chunk = value ? rm_chunk_rows(value) : 0;   // whole tiles
        return CVTMI_OK;
    }
    if (!strcmp(name, "scan_lazy")) { h->p_lazy = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "scan_small")) { h->p_small = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "scan_share")) { h->p_share = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "encode_variant")) {
        if (value < 0 || value > 2) return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: encode_variant must be 0, 1 or 2");
        h->p_encode = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "scan_mfma")) { h->p_mfma = value != 0; return CVTMI_OK; }
    if (!strcmp(name, "scan_mfma_min_nq") || !strcmp(name, "scan_mfma_min_rows")) {
        if (value < 1) return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: %s must be at least 1", name);
        (strcmp(name, "scan_mfma_min_nq") == 0 ? h->p_mfma_min_nq : h->p_mfma_min_rows) = value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "scan_mfma_max_rows")) { h->p_mfma_max_rows = value; return CVTMI_OK; }   // negative: the default
    if (!strcmp(name, "scan_mfma_cap")) {
        if (value < 1 || value > 4096) return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: scan_mfma_cap must be 1 .. 4096");
        h->p_mfma_cap = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "scan_mfma_sample")) {
        if (value < 1 || value > 3) return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: scan_mfma_sample must be 1 .. 3");
        h->p_mfma_sample = (int)value;
        return CVTMI_OK;
    }
    if (!strcmp(name, "scan_variant")) {
        if (value < 0 || value > 7) return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: scan_variant must be 0..7");
        h->p_variant = (int)value;
        return CVTMI_OK;
    }
    return fail(CVTMI_EINVAL, "cvtmi_opq_set_param: unknown parameter '%s'", name);
}

// the pieces a batch would go through on the "scan_mfma" route, for inspection and for the CPU tests of that arithmetic (include/cvtmi.h)
int cvtmi_opq_mfma_plan(int D, int64_t n_rows, int64_t nq, int k, int list_cap, int sample, int64_t out[3])
{
    if (!out || D < 32 || D > 256 || D % 32 != 0 || n_rows < 1 || nq < 1 || k < 1 || k > 128 || list_cap < 1 || list_cap > 4096)
        return fail(CVTMI_EINVAL, "cvtmi_opq_mfma_plan: bad arguments");
    int64_t per = 0;
    out[2] = (int64_t)adc_mfma_scratch_bytes(D, n_rows, nq, k, list_cap, sample, &per);
    out[0] = per; out[1] = (nq + per - 1) / per;
    return CVTMI_OK;
}

int cvtmi_opq_last_mfma(cvtmi_opq_t h, int64_t out[2])
{
    CHECK_H_SERIAL(h, nullptr);
    if (!out) return fail(CVTMI_EINVAL, "cvtmi_opq_last_mfma: null out");
    out[0] = out[1] = 0;
    if (!h->mf_stat.p) return CVTMI_OK;
    CVTMI_HIP(hipDeviceSynchronize());
    CVTMI_HIP(hipMemcpy(out, h->mf_stat.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

int cvtmi_opq_last_scan(cvtmi_opq_t h, float *ms, int64_t *code_bytes, int *qtile, int *splits)
{
    CHECK_H_SERIAL(h, nullptr);
    if (h->ev_count == 0) return fail(CVTMI_ESTATE, "cvtmi_opq_last_scan: no profiled search since the last call");
    const int cnt = h->ev_count < cvtmi_opq_s::kEvRing ? h->ev_count : cvtmi_opq_s::kEvRing;
    double sum = 0.0;
    for (int e = 0; e < cnt; ++e) {
        CVTMI_HIP(hipEventSynchronize(h->ev1[e]));
        float t = 0.f;
        CVTMI_HIP(hipEventElapsedTime(&t, h->ev0[e], h->ev1[e]));
        sum += t;
    }
    h->ev_count = 0;
    if (ms) *ms = (float)(sum / cnt);
    std::lock_guard<std::mutex> g(h->pool.mu);
    if (code_bytes) *code_bytes = h->last_bytes;
    if (qtile) *qtile = h->last_qt;
    if (splits) *splits = h->last_splits;
    return CVTMI_OK;
}

}  // extern "C"
