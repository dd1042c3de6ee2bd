// bicg_precond.hip -- the diagonal preconditioner's install (bicg_precond_diagonal / _device): one kernel
// turns the caller's d into 1 / d. The caller's array is in the caller's numbering: a reordered context reads it through perm
// (perm[new] = old), the gather of bicg_vecio.hip, so that the stores are coalesced. One correctly rounded division per row and
// nothing else; a zero or non-finite d raises the flag (the quotient of such a row is stored all the same -- the host discards the
// whole result when the flag is up, bicg_api.cpp). Plain loads and stores: the solver reads dinv next. gfx950 only.
#include "bicg_device.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicg {
namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_dinv(const double *__restrict__ d, const uint32_t *__restrict__ perm, uint32_t n,
                                                   double *__restrict__ out, int *flag)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;      // (the launcher keeps the grid within 32 bits: n < 2^32)
    bool bad = false;
    if (i < n) {
        const double v = d[perm ? perm[i] : i];
        bad = v == 0.0 || !isfinite(v);
        out[i] = 1.0 / v;
    }
    // one store per wavefront that saw a bad entry (every writer stores the same word: no atomic needed)
    if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) *flag = 1;
}

}  // namespace

void launch_dinv(const double *d, const uint32_t *perm, uint32_t n, double *out, int *flag, hipStream_t st)
{
    if (n == 0) return;
    const unsigned grid = (unsigned)(((uint64_t)n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_dinv, dim3(grid), dim3(kThreads), 0, st, d, perm, n, out, flag);
}

}  // namespace bicg
