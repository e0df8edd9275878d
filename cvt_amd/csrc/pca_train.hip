// pca_train.hip -- PCA training: mean, centred covariance, eigendecomposition (the arithmetic contract is in
// include/cvtmi.h, "PCA training").
//
// Reference: trainPCA (pca_train_project/train/src/opencv_utils.hpp:27-39) = cv::PCA(data, Mat(), DATA_AS_ROW, dout),
// called by train/src/train.cpp on 2048-d CNN features.  OpenCV is absent here: PARITY UNPINNED.
//
//   pca_colsum_kernel    column sums in double over one row block            -> part[block][din]
//   pca_mean_kernel      mean[j] = float(sum over blocks, in block order / n)
//   pca_cov_kernel       one workgroup per (64 x 64 tile on or below the diagonal, row block): the rows are centred in fp32
//                        while they are staged into LDS, widened to double (exact) and fed to v_mfma_f64_16x16x4_f64
//                                                                                   -> part[block][tile][64][64]
//   pca_cov_reduce_kernel  cov[i][j] = cov[j][i] = (sum over blocks, in block order) / n, for i >= j
//   rocsolver_dsyevd     eigenvalues ascending, eigenvectors in place (column k of the column-major result)
//   pca_finish_kernel    the dout largest, descending; sign fix; fp32
//
// The row blocks depend on (n, din) alone, and every sum runs in one fixed order, so a call is deterministic.
// The covariance is compute-bound (n * din * (din + 1) flop for the lower triangle); a 64 x 64 tile needs 512 B of rows
// per 8192 fp64 multiply-adds, which the L2 and the last-level cache serve when the tiles that run together share their row
// block (the tile index is the fastest grid dimension).  rocSOLVER is bound at run time (dlopen, as shard.hip binds RCCL):
// processes that never train never load it.
#include <dlfcn.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <mutex>
#include <string>

#include "host_util.h"
#include "launch.h"

namespace cvtmi {

namespace {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int PT_THREADS = 256;
constexpr int PT_TILE = 64;                 // covariance tile edge
constexpr int PT_KC = 32;                   // rows per staged chunk
constexpr int PT_LD = 2 * PT_TILE + 16;     // staged row: 64 columns of tile row i, 64 of tile column j, padding (floats)
constexpr int PT_COV_TARGET = 4096;         // covariance workgroups aimed at (256 CUs, ~8 rounds: a short tail)
constexpr int64_t PT_COV_MIN_ROWS = 256;    // smallest covariance row block
constexpr int PT_MEAN_BLOCKS = 1024;        // mean row blocks aimed at
constexpr int64_t PT_MEAN_MIN_ROWS = 256;
constexpr int PT_MAX_DIN = 2048;

struct Plan {
    int64_t mean_rows, mean_blocks;  // mean pass: rows per block, blocks
    int64_t cov_rows, cov_blocks;    // covariance: rows per block (multiple of PT_KC), blocks
    int tiles;                       // 64 x 64 tiles on and below the diagonal
};

Plan make_plan(int64_t n, int din)
{
    Plan p;
    p.mean_rows = std::max<int64_t>(PT_MEAN_MIN_ROWS, (n + PT_MEAN_BLOCKS - 1) / PT_MEAN_BLOCKS);
    p.mean_blocks = (n + p.mean_rows - 1) / p.mean_rows;
    const int nt = (din + PT_TILE - 1) / PT_TILE;
    p.tiles = nt * (nt + 1) / 2;
    const int64_t want = (PT_COV_TARGET + p.tiles - 1) / p.tiles;
    int64_t rows = blocks_for(n, want);
    rows = std::max<int64_t>(PT_COV_MIN_ROWS, (rows + PT_KC - 1) / PT_KC * PT_KC);
    p.cov_rows = rows;
    p.cov_blocks = (n + rows - 1) / rows;
    return p;
}

// ---- mean ---------------------------------------------------------------------------------------------------------------
// grid (row blocks, ceil(din / 1024)): a workgroup takes up to 256 float4 columns; when a row is narrower, 256 / cols rows go
// side by side and their sums are combined in row-lane order at the end.  Each thread adds its rows in ascending order.
__global__ __launch_bounds__(PT_THREADS) void pca_colsum_kernel(const float *__restrict__ x, int64_t n, int din, int64_t rows_per_block,
                                                                double *__restrict__ part)
{
    __shared__ double red[PT_THREADS * 4];
    const int tid = threadIdx.x;
    const int q4 = din / 4, c0 = blockIdx.y * PT_THREADS;
    const int cols = min(PT_THREADS, q4 - c0), lanes = PT_THREADS / cols;
    const int c = tid % cols, rl = tid / cols;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (rl < lanes) {
        const float *p = x + 4 * (c0 + c);
        int64_t r = r0 + rl;
        for (; r + 3 * lanes < r1; r += 4 * lanes) {  // four loads in flight; the additions keep row order
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(p + (r + u * lanes) * din);
#pragma unroll
            for (int u = 0; u < 4; ++u) { s0 += (double)v[u].x; s1 += (double)v[u].y; s2 += (double)v[u].z; s3 += (double)v[u].w; }
        }
        for (; r < r1; r += lanes) {
            const float4 v = *reinterpret_cast<const float4 *>(p + r * din);
            s0 += (double)v.x; s1 += (double)v.y; s2 += (double)v.z; s3 += (double)v.w;
        }
    }
    red[tid * 4 + 0] = s0; red[tid * 4 + 1] = s1; red[tid * 4 + 2] = s2; red[tid * 4 + 3] = s3;
    __syncthreads();
    if (tid < cols) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int l = 0; l < lanes; ++l)
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] += red[(l * cols + tid) * 4 + e];
#pragma unroll
        for (int e = 0; e < 4; ++e) part[(int64_t)blockIdx.x * din + 4 * (c0 + tid) + e] = t[e];
    }
}

__global__ __launch_bounds__(PT_THREADS) void pca_mean_kernel(const double *__restrict__ part, int64_t blocks, int din, int64_t n,
                                                              float *__restrict__ mean)
{
    const int j = blockIdx.x * PT_THREADS + threadIdx.x;
    if (j >= din) return;
    double s = 0.0;
    for (int64_t b = 0; b < blocks; ++b) s += part[b * din + j];
    mean[j] = (float)(s / (double)n);
}

// ---- covariance ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tile_of(int t, int &ti, int &tj)
{
    int i = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    while (i * (i + 1) / 2 > t) --i;
    ti = i;
    tj = t - i * (i + 1) / 2;
}

// grid (tiles, row blocks), 4 waves.  Tile (ti, tj), ti >= tj, is C[i][j] = sum_r d[r][64 ti + i] * d[r][64 tj + j].
// A chunk of 32 rows is staged as [row][128 + 16] floats: columns 0..63 are the tile's rows (64 ti + .), 64..127 its columns
// (64 tj + .), centred in fp32 on the way in; rows past the block and columns past din enter as exact zeros (they add
// nothing).  Wave w owns the 32 x 32 quarter (w >> 1, w & 1) = 2 x 2 MFMA tiles of 16 x 16; one v_mfma_f64_16x16x4_f64
// sums four rows: A[i][k] = d[k][i] (lane: i = lane & 15, k = lane >> 4), B[k][j] = d[k][j] (lane: j = lane & 15,
// k = lane >> 4); C/D: col = lane & 15, row = (lane >> 4) + 4 * reg (the f64 map, not the f32 one).
// Chunk c + 1 is loaded into registers while chunk c feeds the matrix cores; one LDS-only barrier per chunk.
__global__ __launch_bounds__(PT_THREADS) void pca_cov_kernel(const float *__restrict__ x, int64_t n, int din,
                                                             const float *__restrict__ mean, int64_t rows_per_block,
                                                             double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float smem[2][PT_KC * PT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wi = wave >> 1, wj = wave & 1;
    int ti, tj;
    tile_of(blockIdx.x, ti, tj);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block, r1 = min(n, r0 + rows_per_block);
    const int nch = (int)((r1 - r0 + PT_KC - 1) / PT_KC);
    // loader: float4 number f = p * 256 + tid of the [32][128] chunk: row 8p + (tid >> 5), staged column 4 * (tid & 31)
    const int sc = 4 * (tid & 31), sr = tid >> 5;
    const int gc = sc < PT_TILE ? PT_TILE * ti + sc : PT_TILE * tj + sc - PT_TILE;
    const bool col_live = gc < din;  // din % 4 == 0: a float4 is inside or outside as a whole
    const int gcc = col_live ? gc : 0;
    const float4 pm = *reinterpret_cast<const float4 *>(mean + gcc);
    float4 px[4];
    bool live[4];
    auto fetch = [&](int c) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int64_t r = r0 + (int64_t)c * PT_KC + p * 8 + sr;
            live[p] = col_live && r < r1;
            const int64_t rc = r < r1 ? r : r1 - 1;  // clamped address; the value of a dead row is replaced by zeros
            px[p] = *reinterpret_cast<const float4 *>(x + rc * din + gcc);
        }
    };
    auto stash = [&](float *buf) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (live[p]) d = make_float4(__fsub_rn(px[p].x, pm.x), __fsub_rn(px[p].y, pm.y), __fsub_rn(px[p].z, pm.z), __fsub_rn(px[p].w, pm.w));
            *reinterpret_cast<float4 *>(buf + (p * 8 + sr) * PT_LD + sc) = d;
        }
    };
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (int c = 0; c < nch; ++c) {
        float *buf = smem[c & 1];
        stash(buf);                    // this stage was last read two chunks ago: every wave is past that barrier
        if (c + 1 < nch) fetch(c + 1); // lands while the MFMAs below run
        lds_barrier();
        const float *pa = buf + lk * PT_LD + wi * 32 + li;
        const float *pb = buf + lk * PT_LD + PT_TILE + wj * 32 + li;
#pragma unroll
        for (int kk = 0; kk < PT_KC; kk += 4) {
            const double a0 = (double)pa[kk * PT_LD], a1 = (double)pa[kk * PT_LD + 16];
            const double b0 = (double)pb[kk * PT_LD], b1 = (double)pb[kk * PT_LD + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    double *out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (PT_TILE * PT_TILE);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = wi * 32 + a * 16 + lk + 4 * e, j = wj * 32 + b * 16 + li;
                out[i * PT_TILE + j] = acc[a][b][e];
            }
}

// one thread per element on or below the diagonal; the blocks' partials are added in block order
__global__ __launch_bounds__(PT_THREADS) void pca_cov_reduce_kernel(const double *__restrict__ part, int64_t blocks, int tiles, int din,
                                                                    int64_t n, double *__restrict__ cov)
{
    const int64_t idx = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x;
    if (idx >= (int64_t)din * din) return;
    const int i = (int)(idx / din), j = (int)(idx % din);
    if (j > i) return;
    const int ti = i / PT_TILE, tj = j / PT_TILE;
    const double *p = part + (size_t)(ti * (ti + 1) / 2 + tj) * (PT_TILE * PT_TILE) + (i % PT_TILE) * PT_TILE + (j % PT_TILE);
    const size_t stride = (size_t)tiles * (PT_TILE * PT_TILE);
    double s = 0.0;
    int64_t b = 0;
    for (; b + 4 <= blocks; b += 4) {
        const double v0 = p[b * stride], v1 = p[(b + 1) * stride], v2 = p[(b + 2) * stride], v3 = p[(b + 3) * stride];
        s += v0; s += v1; s += v2; s += v3;
    }
    for (; b < blocks; ++b) s += p[b * stride];
    const double v = s / (double)n;
    cov[(int64_t)i * din + j] = v;
    cov[(int64_t)j * din + i] = v;
}

// ---- finish -------------------------------------------------------------------------------------------------------------
// output o = eigenpair din - 1 - o of dsyevd (ascending); evec: column-major, column k = eigenvector k.  The largest |v_i|
// (lowest i on ties) decides the sign.
__global__ __launch_bounds__(PT_THREADS) void pca_finish_kernel(const double *__restrict__ evec, const double *__restrict__ evals, int din,
                                                                float *__restrict__ vectors, float *__restrict__ values)
{
    __shared__ double bm[PT_THREADS];
    __shared__ int bi[PT_THREADS];
    const int o = blockIdx.x, k = din - 1 - o, tid = threadIdx.x;
    const double *v = evec + (size_t)k * din;
    double m = -1.0;
    int mi = din;
    for (int i = tid; i < din; i += PT_THREADS) {
        const double a = fabs(v[i]);
        if (a > m) { m = a; mi = i; }  // ascending i: ties keep the first
    }
    bm[tid] = m; bi[tid] = mi;
    __syncthreads();
    for (int s = PT_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double m2 = bm[tid + s];
            const int i2 = bi[tid + s];
            if (m2 > bm[tid] || (m2 == bm[tid] && i2 < bi[tid])) { bm[tid] = m2; bi[tid] = i2; }
        }
        __syncthreads();
    }
    const bool flip = v[bi[0] < din ? bi[0] : 0] < 0.0;
    for (int i = tid; i < din; i += PT_THREADS) vectors[(size_t)o * din + i] = (float)(flip ? -v[i] : v[i]);
    if (tid == 0) values[o] = (float)evals[k];
}

// ---- rocSOLVER, bound at run time ---------------------------------------------------------------------------------------
struct SolverApi {
    void *so = nullptr;
    decltype(&rocblas_create_handle) CreateHandle = nullptr;
    decltype(&rocblas_set_stream) SetStream = nullptr;
    decltype(&rocblas_start_device_memory_size_query) StartQuery = nullptr;
    decltype(&rocblas_stop_device_memory_size_query) StopQuery = nullptr;
    decltype(&rocsolver_dsyevd) Dsyevd = nullptr;
    std::string why;
    std::mutex mu;                      // a handle's stream and workspace are shared state: one solve at a time per process
    rocblas_handle handle[64] = {};     // per device, created on first use
};

SolverApi *solver()
{
    static SolverApi api;
    static std::once_flag once;
    std::call_once(once, [] {
      try {   // nothing may throw across the C ABI (std::string can)
        // the rocBLAS entries are looked up through rocSOLVER's own dependency, so both come from one installation
        const char *names[] = { "librocsolver.so.0", "librocsolver.so", "/opt/rocm/lib/librocsolver.so.0" };
        for (const char *nm : names) {
            api.so = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
            if (api.so) break;
        }
        if (!api.so) {
            const char *e = dlerror();   // (one call: dlerror() clears the state it reports)
            api.why = std::string("librocsolver.so.0: ") + (e ? e : "not found");
            return;
        }
        auto sym = [&](const char *nm) -> void * {
            void *p = dlsym(api.so, nm);
            if (!p && api.why.empty()) api.why = std::string("symbol missing in librocsolver.so.0 / librocblas.so: ") + nm;
            return p;
        };
        api.CreateHandle = reinterpret_cast<decltype(&rocblas_create_handle)>(sym("rocblas_create_handle"));
        api.SetStream = reinterpret_cast<decltype(&rocblas_set_stream)>(sym("rocblas_set_stream"));
        api.StartQuery = reinterpret_cast<decltype(&rocblas_start_device_memory_size_query)>(sym("rocblas_start_device_memory_size_query"));
        api.StopQuery = reinterpret_cast<decltype(&rocblas_stop_device_memory_size_query)>(sym("rocblas_stop_device_memory_size_query"));
        api.Dsyevd = reinterpret_cast<decltype(&rocsolver_dsyevd)>(sym("rocsolver_dsyevd"));
      } catch (...) {
        api.so = nullptr;
        api.why = "librocsolver.so.0: could not be bound";
      }
    });
    return &api;
}

// the solver and this device's handle; the caller holds api->mu
int solver_handle(SolverApi *api, rocblas_handle *h)
{
    int dev = 0;
    CVTMI_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(CVTMI_EUNSUPPORTED, "pca_train: device %d", dev);
    if (!api->handle[dev]) {
        const rocblas_status s = api->CreateHandle(&api->handle[dev]);
        if (s != rocblas_status_success) {
            api->handle[dev] = nullptr;
            return fail(CVTMI_EHIP, "pca_train: rocblas_create_handle failed (status %d)", (int)s);
        }
    }
    *h = api->handle[dev];
    return CVTMI_OK;
}

int check_args(const char *who, const void *x, int64_t n, int din, const void *a, const void *b)
{
    if (!x || !a || !b) return fail(CVTMI_EINVAL, "%s: null pointer", who);
    if (n < 1) return fail(CVTMI_EINVAL, "%s: n = %lld (needs at least one row)", who, (long long)n);
    if (din < 4 || din > PT_MAX_DIN || din % 4 != 0)
        return fail(CVTMI_EINVAL, "%s: din = %d (needs a multiple of 4 in [4, %d])", who, din, PT_MAX_DIN);
    if (n > ((int64_t)1 << 40)) return fail(CVTMI_EINVAL, "%s: n = %lld rows", who, (long long)n);
    return CVTMI_OK;
}

size_t scratch_bytes(const Plan &p, int din)
{
    return (size_t)p.mean_blocks * din * sizeof(double) + (size_t)p.cov_blocks * p.tiles * PT_TILE * PT_TILE * sizeof(double);
}

int fits(const char *who, size_t need)
{
    size_t free_b = 0, total_b = 0;
    CVTMI_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t margin = (size_t)64 << 20;
    if (need + margin > free_b)
        return fail(CVTMI_ENOMEM, "%s: needs %zu MB of device memory, %zu MB are free", who, (need >> 20) + 64, free_b >> 20);
    return CVTMI_OK;
}

// mean + covariance on `st`; the scratch is allocated here and released after the stream has drained
int covariance(const float *x, int64_t n, int din, float *mean, double *cov, hipStream_t st)
{
    const Plan p = make_plan(n, din);
    Tmp mpart, cpart;
    CVTMI_TRY(mpart.alloc((size_t)p.mean_blocks * din * sizeof(double)));
    CVTMI_TRY(cpart.alloc((size_t)p.cov_blocks * p.tiles * PT_TILE * PT_TILE * sizeof(double)));
    const int cgroups = (din / 4 + PT_THREADS - 1) / PT_THREADS;
    CVTMI_TRY(launch("pca_colsum_kernel", pca_colsum_kernel, { p.mean_blocks, cgroups }, PT_THREADS, 0, st, x, n, din, p.mean_rows, mpart.as<double>()));
    CVTMI_TRY(launch("pca_mean_kernel", pca_mean_kernel, blocks_for(din, PT_THREADS), PT_THREADS, 0, st, mpart.as<double>(), p.mean_blocks, din, n, mean));
    CVTMI_TRY(launch("pca_cov_kernel", pca_cov_kernel, { p.tiles, p.cov_blocks }, PT_THREADS, 0, st, x, n, din, mean, p.cov_rows, cpart.as<double>()));
    const int64_t el = (int64_t)din * din;
    CVTMI_TRY(launch("pca_cov_reduce_kernel", pca_cov_reduce_kernel, blocks_for(el, PT_THREADS), PT_THREADS, 0, st, cpart.as<double>(), p.cov_blocks, p.tiles, din, n, cov));
    CVTMI_HIP(hipStreamSynchronize(st));
    return CVTMI_OK;
}

// the whole training on `st`; x_bytes: what the caller still has to place on the device (host entries), for the memory check
int train(const float *x, int64_t n, int din, int dout, float *mean, float *vectors, float *values, hipStream_t st,
          size_t x_bytes, const float *host_x)
{
    SolverApi *api = solver();
    if (!api->so || !api->why.empty())
        return fail(CVTMI_EUNSUPPORTED, "pca_train: rocSOLVER is not available (%s)", api->why.empty() ? "librocsolver.so.0" : api->why.c_str());
    std::lock_guard<std::mutex> lock(api->mu);
    rocblas_handle h = nullptr;
    CVTMI_TRY(solver_handle(api, &h));
    const size_t dd = (size_t)din * din;
    Tmp dcov, dw, de, dinfo;
    CVTMI_TRY(dcov.alloc(dd * sizeof(double)));
    CVTMI_TRY(dw.alloc((size_t)din * sizeof(double)));
    CVTMI_TRY(de.alloc((size_t)din * sizeof(double)));
    CVTMI_TRY(dinfo.alloc(sizeof(rocblas_int)));
    // the solver's workspace, asked for before anything large is placed
    size_t ws = 0;
    {
        rocblas_status s = api->StartQuery(h);
        if (s == rocblas_status_success) {
            s = api->Dsyevd(h, rocblas_evect_original, rocblas_fill_lower, din, dcov.as<double>(), din, dw.as<double>(), de.as<double>(),
                            dinfo.as<rocblas_int>());
            const rocblas_status s2 = api->StopQuery(h, &ws);
            if (s == rocblas_status_success || s == rocblas_status_size_increased || s == rocblas_status_size_unchanged) s = s2;
        }
        if (s != rocblas_status_success) return fail(CVTMI_EHIP, "pca_train: rocsolver_dsyevd workspace query failed (status %d)", (int)s);
    }
    const Plan p = make_plan(n, din);
    CVTMI_TRY(fits("pca_train", x_bytes + scratch_bytes(p, din) + ws));
    Tmp dx;
    if (host_x) {
        CVTMI_TRY(dx.upload(host_x, x_bytes));
        x = dx.as<float>();
    }
    CVTMI_TRY(covariance(x, n, din, mean, dcov.as<double>(), st));
    if (host_x) { (void)hipFree(dx.p); dx.p = nullptr; }  // the rows are no longer needed: leave their memory to the solver
    rocblas_status s = api->SetStream(h, st);
    if (s != rocblas_status_success) return fail(CVTMI_EHIP, "pca_train: rocblas_set_stream failed (status %d)", (int)s);
    s = api->Dsyevd(h, rocblas_evect_original, rocblas_fill_lower, din, dcov.as<double>(), din, dw.as<double>(), de.as<double>(),
                    dinfo.as<rocblas_int>());
    if (s != rocblas_status_success) return fail(CVTMI_EHIP, "pca_train: rocsolver_dsyevd failed (status %d)", (int)s);
    rocblas_int info = 0;
    CVTMI_HIP(hipMemcpyAsync(&info, dinfo.p, sizeof info, hipMemcpyDeviceToHost, st));
    CVTMI_HIP(hipStreamSynchronize(st));
    if (info != 0) return fail(CVTMI_EHIP, "pca_train: rocsolver_dsyevd did not converge (info = %d)", (int)info);
    CVTMI_TRY(launch("pca_finish_kernel", pca_finish_kernel, dout, PT_THREADS, 0, st, dcov.as<double>(), dw.as<double>(), din, vectors, values));
    CVTMI_HIP(hipStreamSynchronize(st));
    return CVTMI_OK;
}

}  // namespace

}  // namespace cvtmi

using namespace cvtmi;

extern "C" {

int cvtmi_pca_covariance_dev(const float *x, int64_t n, int din, float *mean, double *cov, void *stream)
{
    CVTMI_TRY(check_args("cvtmi_pca_covariance", x, n, din, mean, cov));
    if ((((uintptr_t)x) | ((uintptr_t)mean)) & 15) return fail(CVTMI_EINVAL, "cvtmi_pca_covariance: x and mean must be 16-byte aligned");
    CVTMI_TRY(fits("cvtmi_pca_covariance", scratch_bytes(make_plan(n, din), din)));
    return covariance(x, n, din, mean, cov, (hipStream_t)stream);
}

int cvtmi_pca_covariance(const float *x, int64_t n, int din, float *mean, double *cov)
{
    CVTMI_TRY(check_args("cvtmi_pca_covariance", x, n, din, mean, cov));
    const size_t xb = (size_t)n * din * sizeof(float), cb = (size_t)din * din * sizeof(double);
    CVTMI_TRY(fits("cvtmi_pca_covariance", xb + cb + scratch_bytes(make_plan(n, din), din)));
    Tmp dx, dm, dc;
    CVTMI_TRY(dx.upload(x, xb));
    CVTMI_TRY(dm.alloc((size_t)din * sizeof(float)));
    CVTMI_TRY(dc.alloc(cb));
    CVTMI_TRY(covariance(dx.as<float>(), n, din, dm.as<float>(), dc.as<double>(), nullptr));
    CVTMI_HIP(hipMemcpy(mean, dm.p, (size_t)din * sizeof(float), hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(cov, dc.p, cb, hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

int cvtmi_pca_train_dev(const float *x, int64_t n, int din, int dout, float *mean, float *vectors, float *values, void *stream)
{
    CVTMI_TRY(check_args("cvtmi_pca_train", x, n, din, mean, vectors));
    if (!values) return fail(CVTMI_EINVAL, "cvtmi_pca_train: null pointer");
    if (dout < 1 || dout > din || dout > n)
        return fail(CVTMI_EINVAL, "cvtmi_pca_train: dout = %d (needs 1 <= dout <= min(din = %d, n = %lld))", dout, din, (long long)n);
    if ((((uintptr_t)x) | ((uintptr_t)mean)) & 15) return fail(CVTMI_EINVAL, "cvtmi_pca_train: x and mean must be 16-byte aligned");
    return train(x, n, din, dout, mean, vectors, values, (hipStream_t)stream, 0, nullptr);
}

int cvtmi_pca_train(const float *x, int64_t n, int din, int dout, float *mean, float *vectors, float *values)
{
    CVTMI_TRY(check_args("cvtmi_pca_train", x, n, din, mean, vectors));
    if (!values) return fail(CVTMI_EINVAL, "cvtmi_pca_train: null pointer");
    if (dout < 1 || dout > din || dout > n)
        return fail(CVTMI_EINVAL, "cvtmi_pca_train: dout = %d (needs 1 <= dout <= min(din = %d, n = %lld))", dout, din, (long long)n);
    Tmp dm, dv, dl;
    CVTMI_TRY(dm.alloc((size_t)din * sizeof(float)));
    CVTMI_TRY(dv.alloc((size_t)dout * din * sizeof(float)));
    CVTMI_TRY(dl.alloc((size_t)dout * sizeof(float)));
    CVTMI_TRY(train(nullptr, n, din, dout, dm.as<float>(), dv.as<float>(), dl.as<float>(), nullptr, (size_t)n * din * sizeof(float), x));
    CVTMI_HIP(hipMemcpy(mean, dm.p, (size_t)din * sizeof(float), hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(vectors, dv.p, (size_t)dout * din * sizeof(float), hipMemcpyDeviceToHost));
    CVTMI_HIP(hipMemcpy(values, dl.p, (size_t)dout * sizeof(float), hipMemcpyDeviceToHost));
    return CVTMI_OK;
}

}  // extern "C"
