// api_models.hip -- the handle-less model entries of the C ABI (include/cvtmi.h): SQ8 train / encode / decode, PCA projection,
// k-means and OPQ codebook training.
#include <string.h>

#include "api_internal.h"

extern "C" {

// ================================================================ SQ8 =========================
int cvtmi_sq8_train_dev(const float *x, int64_t n, int d, int l2norm, float *vmin, float *vdiff, void *stream)
{
    if (n < 0 || d < 1 || !vmin || !vdiff || (n > 0 && !x)) return fail(CVTMI_EINVAL, "cvtmi_sq8_train: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    Tmp den, keys;
    if (l2norm && n > 0 && !sq8_single_pass(d, x, nullptr, nullptr, nullptr, n)) CVTMI_TRY(den.alloc((size_t)n * sizeof(float)));
    CVTMI_TRY(keys.alloc((size_t)d * 2 * sizeof(uint32_t)));
    CVTMI_TRY(launch_sq8_train(x, n, d, l2norm, den.as<float>(), keys.as<uint32_t>(), keys.as<uint32_t>() + d, vmin, vdiff,
                               st));
    CVTMI_HIP(stream_wait(st));  // the temporaries die with this frame
    return CVTMI_OK;
}

int cvtmi_sq8_train(const float *x, int64_t n, int d, int l2norm, float *vmin, float *vdiff)
{
    if (n < 0 || d < 1 || !vmin || !vdiff || (n > 0 && !x)) return fail(CVTMI_EINVAL, "cvtmi_sq8_train: bad arguments");
    Tmp dx, dmin, ddiff;
    CVTMI_TRY(dx.upload(x, (size_t)n * d * sizeof(float)));
    CVTMI_TRY(dmin.alloc((size_t)d * sizeof(float)));
    CVTMI_TRY(ddiff.alloc((size_t)d * sizeof(float)));
    CVTMI_TRY(cvtmi_sq8_train_dev(dx.as<float>(), n, d, l2norm, dmin.as<float>(), ddiff.as<float>(), nullptr));
    CVTMI_HIP(hipMemcpy(vmin, dmin.p, (size_t)d * sizeof(float), hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(vdiff, ddiff.p, (size_t)d * sizeof(float), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

int cvtmi_sq8_encode_dev(const float *vmin, const float *vdiff, int d, float *x, int64_t n, int l2norm, uint8_t *codes,
                         void *stream)
{
    if (n < 0 || d < 1 || !vmin || !vdiff || (n > 0 && (!x || !codes))) return fail(CVTMI_EINVAL, "cvtmi_sq8_encode: bad arguments");
    if (n == 0) return CVTMI_OK;
    hipStream_t st = (hipStream_t)stream;
    Tmp den;
    const bool two_pass = l2norm && !sq8_single_pass(d, x, codes, vmin, vdiff, n);
    if (two_pass) CVTMI_TRY(den.alloc((size_t)n * sizeof(float)));
    CVTMI_TRY(launch_sq8_encode_rows(vmin, vdiff, d, x, n, l2norm ? 1 : 0, l2norm == 2 ? 0 : 1, codes, den.as<float>(), st));
    if (two_pass) CVTMI_HIP(stream_wait(st));  // the temporary dies with this frame
    return CVTMI_OK;
}

}  // extern "C"

// Small SQ8 calls through the host-pointer entries -- the reference encodes and decodes ONE feature vector per call (int8_quan.cc:72-132) --
// used to pay four device allocations, four copies and four frees per call (65-80 us, 270 at 2048-d).  They now run out of a page-locked
// scratch area: the model, the rows and the results live in device-visible host memory, the kernels read and write it directly
// (everything is touched once), and nothing is allocated per call.  The areas are kept per device for the life of the process (a handful
// of 1 MB buffers; the SQ8 entries have no handle that could own them).
namespace {
struct Sq8HostScratch {
    PinBuf pin;
    hipStream_t st = nullptr;
    int device = -1;
    bool busy = false;
};
std::mutex g_sq8_host_mu;
std::vector<Sq8HostScratch *> g_sq8_host_pool;   // never shrinks, never freed (process lifetime)
constexpr size_t SQ8_HOST_SMALL = (size_t)1 << 20;
struct Sq8HostLease {
    Sq8HostScratch *s = nullptr;
    int open()
    {
        int dev = 0;
        CVTMI_HIP(hipGetDevice(&dev));
        {
            std::lock_guard<std::mutex> g(g_sq8_host_mu);
            for (Sq8HostScratch *c : g_sq8_host_pool)
                if (!c->busy && c->device == dev) { s = c; break; }
            if (!s) {
                s = new (std::nothrow) Sq8HostScratch();
                if (!s) return fail(CVTMI_ENOMEM, "sq8: out of host memory");
                s->device = dev;
                g_sq8_host_pool.push_back(s);
            }
            s->busy = true;
        }
        if (!s->st) CVTMI_HIP(hipStreamCreateWithFlags(&s->st, hipStreamNonBlocking));
        return s->pin.reserve(SQ8_HOST_SMALL + 4096);
    }
    ~Sq8HostLease()
    {
        if (!s) return;
        std::lock_guard<std::mutex> g(g_sq8_host_mu);
        s->busy = false;
    }
};
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

extern "C" {

int cvtmi_sq8_encode(const float *vmin, const float *vdiff, int d, float *x, int64_t n, int l2norm, uint8_t *codes)
{
    if (n < 0 || d < 1 || !vmin || !vdiff || (n > 0 && (!x || !codes))) return fail(CVTMI_EINVAL, "cvtmi_sq8_encode: bad arguments");
    if (n == 0) return CVTMI_OK;
    {
        const size_t mb = up256((size_t)d * sizeof(float)), xb = up256((size_t)n * d * sizeof(float)), cb = up256((size_t)n * d);
        const size_t nb = up256((size_t)n * sizeof(float));   // row norms of the widths that take two passes
        if (tune_sq8_host_small.geti() && 2 * mb + xb + cb + nb <= SQ8_HOST_SMALL) {
            Sq8HostLease lease;
            CVTMI_TRY(lease.open());
            void *pd_ = nullptr;
            if (hipHostGetDevicePointer(&pd_, lease.s->pin.p, 0) == hipSuccess && pd_) {
                char *pin = lease.s->pin.as<char>(), *pd = static_cast<char *>(pd_);
                memcpy(pin, vmin, (size_t)d * sizeof(float));
                memcpy(pin + mb, vdiff, (size_t)d * sizeof(float));
                memcpy(pin + 2 * mb, x, (size_t)n * d * sizeof(float));
                CVTMI_TRY(launch_sq8_encode_rows(reinterpret_cast<float *>(pd), reinterpret_cast<float *>(pd + mb), d, reinterpret_cast<float *>(pd + 2 * mb), n,
                                                 l2norm ? 1 : 0, l2norm == 2 ? 0 : 1, reinterpret_cast<uint8_t *>(pd + 2 * mb + xb),
                                                 reinterpret_cast<float *>(pd + 2 * mb + xb + cb), lease.s->st));
                CVTMI_HIP(stream_wait(lease.s->st));
                memcpy(codes, pin + 2 * mb + xb, (size_t)n * d);
                if (l2norm == 1) memcpy(x, pin + 2 * mb, (size_t)n * d * sizeof(float));
                return CVTMI_OK;
            }
            (void)hipGetLastError();
        }
    }
    Tmp dmin, ddiff, dx, dc;
    CVTMI_TRY(dmin.upload(vmin, (size_t)d * sizeof(float)));
    CVTMI_TRY(ddiff.upload(vdiff, (size_t)d * sizeof(float)));
    CVTMI_TRY(dx.upload(x, (size_t)n * d * sizeof(float)));
    CVTMI_TRY(dc.alloc((size_t)n * d));
    CVTMI_TRY(cvtmi_sq8_encode_dev(dmin.as<float>(), ddiff.as<float>(), d, dx.as<float>(), n, l2norm, dc.as<uint8_t>(), nullptr));
    CVTMI_HIP(hipMemcpy(codes, dc.p, (size_t)n * d, hipMemcpyDeviceToHost));
    if (l2norm == 1) CVTMI_HIP(hipMemcpy(x, dx.p, (size_t)n * d * sizeof(float), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

// ================================================================ PCA =========================
int cvtmi_pca_project_dev(const float *mean, const float *vectors, int din, int dout, const float *x, int64_t n, int l2norm,
                          float *y, void *stream)
{
    if (n < 0 || !mean || !vectors || (n > 0 && (!x || !y))) return fail(CVTMI_EINVAL, "cvtmi_pca_project: bad arguments");
    return launch_pca_project(mean, vectors, din, dout, x, n, l2norm, y, (hipStream_t)stream);
}

int cvtmi_pca_project(const float *mean, const float *vectors, int din, int dout, const float *x, int64_t n, int l2norm, float *y)
{
    if (n < 0 || din < 1 || dout < 1 || !mean || !vectors || (n > 0 && (!x || !y))) return fail(CVTMI_EINVAL, "cvtmi_pca_project: bad arguments");
    if (n == 0) return CVTMI_OK;
    Tmp dm, de, dx, dy;
    CVTMI_TRY(dm.upload(mean, (size_t)din * sizeof(float)));
    CVTMI_TRY(de.upload(vectors, (size_t)dout * din * sizeof(float)));
    CVTMI_TRY(dx.upload(x, (size_t)n * din * sizeof(float)));
    CVTMI_TRY(dy.alloc((size_t)n * dout * sizeof(float)));
    CVTMI_TRY(cvtmi_pca_project_dev(dm.as<float>(), de.as<float>(), din, dout, dx.as<float>(), n, l2norm, dy.as<float>(), nullptr));
    CVTMI_HIP(hipMemcpy(y, dy.p, (size_t)n * dout * sizeof(float), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

static int sq8_decode_dev_mode(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n, float *x, void *stream, int mode)
{
    if (n < 0 || d < 1 || !vmin || !vdiff || (n > 0 && (!x || !codes))) return fail(CVTMI_EINVAL, "cvtmi_sq8_decode: bad arguments");
    return launch_sq8_decode(vmin, vdiff, d, codes, n, x, (hipStream_t)stream, mode);
}
static int sq8_decode_host_mode(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n, float *x, int mode)
{
    if (n < 0 || d < 1 || !vmin || !vdiff || (n > 0 && (!x || !codes))) return fail(CVTMI_EINVAL, "cvtmi_sq8_decode: bad arguments");
    if (n == 0) return CVTMI_OK;
    {   // small calls: out of the page-locked scratch area (see Sq8HostScratch)
        const size_t mb = up256((size_t)d * sizeof(float)), xb = up256((size_t)n * d * sizeof(float)), cb = up256((size_t)n * d);
        if (tune_sq8_host_small.geti() && 2 * mb + xb + cb <= SQ8_HOST_SMALL) {
            Sq8HostLease lease;
            CVTMI_TRY(lease.open());
            void *pd_ = nullptr;
            if (hipHostGetDevicePointer(&pd_, lease.s->pin.p, 0) == hipSuccess && pd_) {
                char *pin = lease.s->pin.as<char>(), *pd = static_cast<char *>(pd_);
                memcpy(pin, vmin, (size_t)d * sizeof(float));
                memcpy(pin + mb, vdiff, (size_t)d * sizeof(float));
                memcpy(pin + 2 * mb, codes, (size_t)n * d);
                CVTMI_TRY(sq8_decode_dev_mode(reinterpret_cast<float *>(pd), reinterpret_cast<float *>(pd + mb), d, reinterpret_cast<uint8_t *>(pd + 2 * mb), n,
                                              reinterpret_cast<float *>(pd + 2 * mb + cb), lease.s->st, mode));
                CVTMI_HIP(stream_wait(lease.s->st));
                memcpy(x, pin + 2 * mb + cb, (size_t)n * d * sizeof(float));
                return CVTMI_OK;
            }
            (void)hipGetLastError();
        }
    }
    Tmp dmin, ddiff, dx, dc;
    CVTMI_TRY(dmin.upload(vmin, (size_t)d * sizeof(float)));
    CVTMI_TRY(ddiff.upload(vdiff, (size_t)d * sizeof(float)));
    CVTMI_TRY(dc.upload(codes, (size_t)n * d));
    CVTMI_TRY(dx.alloc((size_t)n * d * sizeof(float)));
    CVTMI_TRY(sq8_decode_dev_mode(dmin.as<float>(), ddiff.as<float>(), d, dc.as<uint8_t>(), n, dx.as<float>(), nullptr, mode));
    CVTMI_HIP(hipMemcpy(x, dx.p, (size_t)n * d * sizeof(float), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

int cvtmi_sq8_decode_dev(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n, float *x, void *stream)
{
    return sq8_decode_dev_mode(vmin, vdiff, d, codes, n, x, stream, 0);
}
int cvtmi_sq8_decode(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n, float *x)
{
    return sq8_decode_host_mode(vmin, vdiff, d, codes, n, x, 0);
}
int cvtmi_sq8_decode_faiss_dev(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n, float *x, void *stream)
{
    return sq8_decode_dev_mode(vmin, vdiff, d, codes, n, x, stream, 1);
}
int cvtmi_sq8_decode_faiss(const float *vmin, const float *vdiff, int d, const uint8_t *codes, int64_t n, float *x)
{
    return sq8_decode_host_mode(vmin, vdiff, d, codes, n, x, 1);
}

}  // extern "C"

// ================================================================ codebook training ===========
static uint64_t splitmix64(uint64_t &s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int cvtmi_kmeans_dev(const float *x, int64_t ld, int64_t n, int d, int k, int niter, uint64_t seed, float *centroids,
                     int32_t *assign, int *iters_done, void *stream)
{
    if (!x || !centroids || n < 1 || d < 1 || k < 1 || ld < d) return fail(CVTMI_EINVAL, "cvtmi_kmeans: bad arguments");
    if (n < k) return fail(CVTMI_EINVAL, "cvtmi_kmeans: fewer rows (%lld) than centroids (%d)", (long long)n, k);
    if (d > 512) return fail(CVTMI_EUNSUPPORTED, "cvtmi_kmeans: d=%d > 512", d);
    hipStream_t st = (hipStream_t)stream;
    // seeding: k distinct rows, index = splitmix64() % n, redraw on repeats (host side, k values)
    std::vector<int64_t> rows((size_t)k);
    {
        std::vector<uint8_t> taken((size_t)n, 0);
        uint64_t s = seed;
        for (int c = 0; c < k; ++c) {
            int64_t r;
            do { r = (int64_t)(splitmix64(s) % (uint64_t)n); } while (taken[(size_t)r]);
            taken[(size_t)r] = 1;
            rows[(size_t)c] = r;
        }
    }
    Tmp drows, dassign, dchanged;
    CVTMI_TRY(drows.upload(rows.data(), (size_t)k * sizeof(int64_t)));
    CVTMI_TRY(launch_kmeans_gather(x, ld, d, drows.as<int64_t>(), k, centroids, st));
    int32_t *as = assign;
    if (!as) {
        CVTMI_TRY(dassign.alloc((size_t)n * sizeof(int32_t)));
        as = dassign.as<int32_t>();
    }
    CVTMI_TRY(launch_kmeans_fill(as, n, -2, st));
    CVTMI_TRY(dchanged.alloc(sizeof(unsigned long long)));
    const int max_iter = niter > 0 ? niter : 100;
    int it = 0;
    for (;;) {
        CVTMI_HIP(hipMemsetAsync(dchanged.p, 0, sizeof(unsigned long long), st));
        CVTMI_TRY(launch_kmeans_assign(x, ld, n, d, centroids, k, as, dchanged.as<unsigned long long>(), st));
        unsigned long long changed = 0;
        CVTMI_HIP(hipMemcpyAsync(&changed, dchanged.p, sizeof changed, hipMemcpyDeviceToHost, st));
        CVTMI_HIP(stream_wait(st));
        if (changed == 0 || it >= max_iter) break;
        CVTMI_TRY(launch_kmeans_update(x, ld, n, d, as, k, centroids, st));
        ++it;
    }
    if (iters_done) *iters_done = it;
    CVTMI_HIP(stream_wait(st));  // the temporaries die with this frame
    return CVTMI_OK;
}

int cvtmi_kmeans(const float *x, int64_t n, int d, int k, int niter, uint64_t seed, float *centroids, int32_t *assign,
                 int *iters_done)
{
    if (!x || !centroids || n < 1 || d < 1 || k < 1) return fail(CVTMI_EINVAL, "cvtmi_kmeans: bad arguments");
    Tmp dx, dc, da;
    CVTMI_TRY(dx.upload(x, (size_t)n * d * sizeof(float)));
    CVTMI_TRY(dc.alloc((size_t)k * d * sizeof(float)));
    CVTMI_TRY(da.alloc((size_t)n * sizeof(int32_t)));
    CVTMI_TRY(cvtmi_kmeans_dev(dx.as<float>(), d, n, d, k, niter, seed, dc.as<float>(), da.as<int32_t>(), iters_done, nullptr));
    CVTMI_HIP(hipMemcpy(centroids, dc.p, (size_t)k * d * sizeof(float), hipMemcpyDeviceToHost));
    if (assign) CVTMI_HIP(hipMemcpy(assign, da.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

int cvtmi_opq_train_dev(const float *x, int64_t n, int D, int coarseK, int M, int K, int niter, uint64_t seed, float *coarse,
                        float *books, void *stream)
{
    if (!x || !coarse || !books || n < 1 || D < 1 || M < 1 || M > 16 || D % M != 0 || K < 1 || K > 256 || coarseK < 1)
        return fail(CVTMI_EINVAL, "cvtmi_opq_train: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int step = D / M;
    Tmp assign, res;
    CVTMI_TRY(assign.alloc((size_t)n * sizeof(int32_t)));
    CVTMI_TRY(res.alloc((size_t)n * D * sizeof(float)));
    CVTMI_TRY(cvtmi_kmeans_dev(x, D, n, D, coarseK, niter, seed, coarse, assign.as<int32_t>(), nullptr, stream));
    CVTMI_TRY(launch_kmeans_residual(x, n, D, coarse, assign.as<int32_t>(), res.as<float>(), st));
    for (int m = 0; m < M; ++m)
        CVTMI_TRY(cvtmi_kmeans_dev(res.as<float>() + m * step, D, n, step, K, niter, seed, books + (size_t)m * K * step,
                                   assign.as<int32_t>(), nullptr, stream));
    CVTMI_HIP(stream_wait(st));
    return CVTMI_OK;
}

int cvtmi_opq_train(const float *x, int64_t n, int D, int coarseK, int M, int K, int niter, uint64_t seed, float *coarse,
                    float *books)
{
    if (!x || !coarse || !books || n < 1 || D < 1) return fail(CVTMI_EINVAL, "cvtmi_opq_train: bad arguments");
    Tmp dx, dc, db;
    CVTMI_TRY(dx.upload(x, (size_t)n * D * sizeof(float)));
    CVTMI_TRY(dc.alloc((size_t)coarseK * D * sizeof(float)));
    CVTMI_TRY(db.alloc((size_t)K * D * sizeof(float)));
    CVTMI_TRY(cvtmi_opq_train_dev(dx.as<float>(), n, D, coarseK, M, K, niter, seed, dc.as<float>(), db.as<float>(), nullptr));
    CVTMI_HIP(hipMemcpy(coarse, dc.p, (size_t)coarseK * D * sizeof(float), hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(books, db.p, (size_t)K * D * sizeof(float), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}
