// mfma_f64_rate.hip -- sustained rate of v_mfma_f64_16x16x4_f64 (the PCA covariance kernel's instruction): back-to-back
// independent instructions, every CU, one kernel.   hipcc --offload-arch=gfx950 -O3 -o mfma_f64_rate mfma_f64_rate.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
typedef double v4d __attribute__((ext_vector_type(4)));
template <int WPS>
__global__ __launch_bounds__(256 * WPS) void k(const double *src, double *out, int iters)
{
    double a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { a[i] = src[(i * 64 + threadIdx.x) & 4095]; b[i] = src[(i * 64 + threadIdx.x + 2048) & 4095]; }
    v4d acc[4] = {};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[(i + c) & 7], b[i], acc[c], 0, 0, 0);
    }
    double s = 0;
    for (int c = 0; c < 4; ++c) for (int e = 0; e < 4; ++e) s += acc[c][e];
    out[blockIdx.x * 256 * WPS + threadIdx.x] = s;
}
int main()
{
    int cus = 0;
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0);
    double *src, *out;
    hipMalloc(&src, 4096 * 8); hipMalloc(&out, (size_t)cus * 512 * 8);
    static double h[4096];
    unsigned x = 777;
    for (auto &v : h) { x = x * 1664525u + 1013904223u; v = ((int)(x >> 8) - (1 << 23)) * (1.0 / (1 << 23)); }
    hipMemcpy(src, h, sizeof h, hipMemcpyHostToDevice);
    for (int wps = 1; wps <= 2; ++wps) {
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        const int iters = 2000;
        for (int rep = 0; rep < 2; ++rep) {  // the first launch warms the clocks
            hipEventRecord(e0);
            if (wps == 1) hipLaunchKernelGGL(k<1>, dim3(cus), dim3(256), 0, 0, src, out, iters);
            else hipLaunchKernelGGL(k<2>, dim3(cus), dim3(512), 0, 0, src, out, iters);
            hipEventRecord(e1); hipEventSynchronize(e1);
        }
        float ms; hipEventElapsedTime(&ms, e0, e1);
        const double flops = (double)iters * cus * 4 * wps * 8 * 4 * (16.0 * 16 * 4 * 2);
        printf("v_mfma_f64_16x16x4_f64, %d CUs, %d wave(s) per SIMD: %.3f ms, %.2f TFLOP/s\n", cus, wps, ms, flops / ms / 1e9);
    }
    return 0;
}
