// launch.h -- the one place a kernel is launched from (host side, inline templates only).
// launch() checks the grid before anything is narrowed, launches, and checks the runtime's answer for that launch alone;
// launch_lds() / launch_lds_once() also raise the kernel's dynamic-LDS limit first.  gfx950 only.
#pragma once
#include <atomic>

#include "common.h"

namespace cvtmi {

// blocks of `per_block` items that cover `count` items
constexpr int64_t blocks_for(int64_t count, int64_t per_block) { return (count + per_block - 1) / per_block; }

// a grid before narrowing: `blocks`, `{ x, y }` or `{ x, y, z }`
struct Grid {
    int64_t x, y, z;
    constexpr Grid(int64_t x_, int64_t y_ = 1, int64_t z_ = 1) : x(x_), y(y_), z(z_) {}
};

constexpr int64_t kGridMaxX = 0x7fffffff, kGridMaxYZ = 65535;

// the grid rule of every launch: each dimension at least 1, x <= 0x7fffffff, y and z <= 65535
inline int check_grid(const char *what, const Grid &g)
{
    if (g.x < 1 || g.x > kGridMaxX) return fail(CVTMI_EUNSUPPORTED, "%s: grid x = %lld outside 1..%lld", what, (long long)g.x, (long long)kGridMaxX);
    if (g.y < 1 || g.y > kGridMaxYZ) return fail(CVTMI_EUNSUPPORTED, "%s: grid y = %lld outside 1..%lld", what, (long long)g.y, (long long)kGridMaxYZ);
    if (g.z < 1 || g.z > kGridMaxYZ) return fail(CVTMI_EUNSUPPORTED, "%s: grid z = %lld outside 1..%lld", what, (long long)g.z, (long long)kGridMaxYZ);
    return CVTMI_OK;
}

// The launch log (cvtmi_debug_launch_log_begin / _end / _read, include/cvtmi.h): while the calling thread has it on, every launch that
// passed the grid rule is noted with its name, grid, block and dynamic LDS.  Off -- the default -- it costs a launch the test of one
// thread-local pointer: no lock, no allocation, nothing on the device.  `what` is kept as a pointer: pass string literals.
struct LaunchLog;
extern __thread LaunchLog *g_launch_log;   // api.hip; null while the thread's log is off
void launch_log_note(const char *what, const Grid &grid, unsigned block_x, size_t lds);
inline void log_launch(const char *what, const Grid &grid, unsigned block_x, size_t lds)
{
    if (__builtin_expect(g_launch_log != nullptr, 0)) launch_log_note(what, grid, block_x, lds);
}

// `what` names the kernel in the messages.  The arguments convert to the kernel's parameter types exactly as in a direct launch.
template <class... KA, class... A>
inline int launch(const char *what, void (*kernel)(KA...), const Grid &grid, dim3 block, size_t lds, hipStream_t st, A &&...args)
{
    CVTMI_TRY(check_grid(what, grid));
    log_launch(what, grid, block.x, lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid.x, (unsigned)grid.y, (unsigned)grid.z), block, lds, st, static_cast<A &&>(args)...);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CVTMI_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return CVTMI_OK;
}

template <class... KA>
inline int set_max_lds(const char *what, void (*kernel)(KA...), size_t lds)
{
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return fail(CVTMI_EHIP, "dynamic LDS limit of %s (%zu bytes) failed: %s", what, lds, hipGetErrorString(e));
    return CVTMI_OK;
}

// dynamic LDS above the default: the limit is set to `lds` on every call
template <class... KA, class... A>
inline int launch_lds(const char *what, void (*kernel)(KA...), const Grid &grid, dim3 block, size_t lds, hipStream_t st, A &&...args)
{
    CVTMI_TRY(set_max_lds(what, kernel, lds));
    return launch(what, kernel, grid, block, lds, st, static_cast<A &&>(args)...);
}

// the limit set once per device (the attribute is per device; several host threads may search at once: setting it twice is
// harmless).  `done` belongs to one kernel; `limit` is the same on every call and at least every call's `lds`.
using LdsOnce = std::atomic<bool>[16];
template <class... KA>
inline int set_max_lds_once(const char *what, void (*kernel)(KA...), size_t lds, LdsOnce &done)
{
    int dev = 0;
    CVTMI_HIP(hipGetDevice(&dev));
    if (dev >= 16 || !done[dev].load(std::memory_order_acquire)) {
        CVTMI_TRY(set_max_lds(what, kernel, lds));
        if (dev < 16) done[dev].store(true, std::memory_order_release);
    }
    return CVTMI_OK;
}
template <class... KA, class... A>
inline int launch_lds_once(const char *what, void (*kernel)(KA...), LdsOnce &done, size_t limit, const Grid &grid, dim3 block, size_t lds, hipStream_t st,
                           A &&...args)
{
    CVTMI_TRY(set_max_lds_once(what, kernel, limit, done));
    return launch(what, kernel, grid, block, lds, st, static_cast<A &&>(args)...);
}

// CUs of the current device: a constant of the process once read (256 if the runtime does not say)
inline int device_cus()
{
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}

}  // namespace cvtmi
