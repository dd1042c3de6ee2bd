// bicg_reorder.hip -- a reordered context's vectors crossing the permutation (BICG_PLAN="reorder=1|2").
// The caller's numbering stays on the host side; everything on the device is in the new one. Both directions are GATHERS with
// coalesced stores, which is why both perm (perm[new] = old) and inv (inv[old] = new) stay on the device, 4 bytes each per row:
//   k_permute_in    dst[j][new] = src[j][perm[new]]      (the caller's vector, staged on the device, into a solver vector)
//   k_permute_out   dst[j][old] = src[j][inv[old]]       (a solver vector into the staging buffer the host copy reads)
// for nvec vectors in one launch (blockIdx.y), source and destination with strides of their own. A lane owns kPerLane consecutive
// elements: one 16-byte load of indices, kPerLane 8-byte gathers, two 16-byte stores. gfx950 only.
#include "bicg_device.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicg {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int kThreads = 256;
constexpr int kPerLane = 4;

// WIDE: dst vectors and idx are 16-byte aligned (the launcher checks); otherwise one element per lane
template <bool WIDE>
__device__ __forceinline__ void permute_body(const double *__restrict__ src, size_t src_stride, double *__restrict__ dst, size_t dst_stride,
                                             const uint32_t *__restrict__ idx, uint32_t n)
{
    const double *s = src + (size_t)blockIdx.y * src_stride;
    double *d = dst + (size_t)blockIdx.y * dst_stride;
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (!WIDE) {
        if (t < n) d[t] = s[idx[t]];
        return;
    }
    const size_t i0 = t * kPerLane;
    if (i0 + kPerLane <= n) {
        const uint4 q = *reinterpret_cast<const uint4 *>(idx + i0);
        const double a = s[q.x], b = s[q.y], c = s[q.z], e = s[q.w];
        f64x2 lo, hi;
        lo.x = a; lo.y = b; hi.x = c; hi.y = e;
        *reinterpret_cast<f64x2 *>(d + i0) = lo;
        *reinterpret_cast<f64x2 *>(d + i0 + 2) = hi;
    } else {
        for (size_t i = i0; i < n; ++i) d[i] = s[idx[i]];          // the last lane with rows: fewer than kPerLane left
    }
}

template <bool WIDE>
__global__ void __launch_bounds__(kThreads) k_permute_in(const double *__restrict__ src, size_t src_stride, double *__restrict__ dst, size_t dst_stride,
                                                         const uint32_t *__restrict__ perm, uint32_t n)
{
    permute_body<WIDE>(src, src_stride, dst, dst_stride, perm, n);
}

template <bool WIDE>
__global__ void __launch_bounds__(kThreads) k_permute_out(const double *__restrict__ src, size_t src_stride, double *__restrict__ dst, size_t dst_stride,
                                                          const uint32_t *__restrict__ inv, uint32_t n)
{
    permute_body<WIDE>(src, src_stride, dst, dst_stride, inv, n);
}

bool wide_ok(const double *dst, size_t dst_stride, const uint32_t *idx)
{
    return (uintptr_t)dst % 16 == 0 && dst_stride % 2 == 0 && (uintptr_t)idx % 16 == 0;
}
dim3 permute_grid(uint32_t n, int nvec, bool wide)
{
    const uint64_t per_block = (uint64_t)kThreads * (wide ? kPerLane : 1);
    return dim3((unsigned)(((uint64_t)n + per_block - 1) / per_block), (unsigned)nvec, 1);
}

}  // namespace

void launch_permute_in(const double *src, size_t src_stride, double *dst, size_t dst_stride, const uint32_t *perm, uint32_t n, int nvec, hipStream_t st)
{
    if (n == 0 || nvec <= 0) return;
    const bool wide = wide_ok(dst, dst_stride, perm);
    if (wide) hipLaunchKernelGGL(k_permute_in<true>, permute_grid(n, nvec, true), dim3(kThreads), 0, st, src, src_stride, dst, dst_stride, perm, n);
    else hipLaunchKernelGGL(k_permute_in<false>, permute_grid(n, nvec, false), dim3(kThreads), 0, st, src, src_stride, dst, dst_stride, perm, n);
}

void launch_permute_out(const double *src, size_t src_stride, double *dst, size_t dst_stride, const uint32_t *inv, uint32_t n, int nvec, hipStream_t st)
{
    if (n == 0 || nvec <= 0) return;
    const bool wide = wide_ok(dst, dst_stride, inv);
    if (wide) hipLaunchKernelGGL(k_permute_out<true>, permute_grid(n, nvec, true), dim3(kThreads), 0, st, src, src_stride, dst, dst_stride, inv, n);
    else hipLaunchKernelGGL(k_permute_out<false>, permute_grid(n, nvec, false), dim3(kThreads), 0, st, src, src_stride, dst, dst_stride, inv, n);
}

}  // namespace bicg
