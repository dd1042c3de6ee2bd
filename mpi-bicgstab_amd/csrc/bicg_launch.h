// bicg_launch.h -- how the kernel translation units launch: the debug check behind every launch and the launch with
// optional per-kernel timing events. One copy, included by every unit that launches a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>   // hipExtLaunchKernelGGL: start/stop events bound to ONE kernel (roofline timing)
#include <cstdio>
#include <cstdlib>

namespace bicg {

// launch with optional per-kernel timing events (kernel-accurate, unlike events recorded around a launch)
// BICG_DEBUG=1: report a launch the runtime refused (or an error an earlier call left behind) where it happens
static inline void launch_debug(const char *what)
{
    static const bool debug = getenv("BICG_DEBUG") != nullptr;
    if (!debug) return;
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) fprintf(stderr, "bicgstab_hip: HIP error \"%s\" noticed at: %s\n", hipGetErrorString(err), what);
}
#define BICG_LAUNCH(kernel, ...)                 \
    do {                                         \
        hipLaunchKernelGGL(kernel, __VA_ARGS__); \
        launch_debug(#kernel);                   \
    } while (0)

template <class K, class... Args>
static void launch_timed_lds(K kernel, dim3 g, dim3 b, unsigned lds_bytes, hipStream_t st, hipEvent_t e0, hipEvent_t e1, Args... args)
{
    launch_debug("(left behind by an earlier call)");
    if (e0 && e1) hipExtLaunchKernelGGL(kernel, g, b, lds_bytes, st, e0, e1, 0, args...);
    else hipLaunchKernelGGL(kernel, g, b, lds_bytes, st, args...);
    launch_debug(__PRETTY_FUNCTION__);
}
template <class K, class... Args>
static void launch_timed(K kernel, dim3 g, dim3 b, hipStream_t st, hipEvent_t e0, hipEvent_t e1, Args... args)
{
    launch_timed_lds(kernel, g, b, 0u, st, e0, e1, args...);
}

// look a kernel up: the runtime loads the code object of its translation unit now (preload_kernels, bicg_spmv_sell.hip)
template <class K> static void preload_kernel(K kernel)
{
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(kernel));
    (void)hipGetLastError();
}

}  // namespace bicg
