// bicg_refresh.hip -- new values for a resident matrix, same sparsity pattern (bicg_update_values, bicg_refresh.cpp; DESIGN.md
// section 4.18). The plan depends on the pattern only, so every stored form of the values is rewritten IN PLACE, at the positions
// the layout defines, from the caller's CSR-ordered values (struct RefreshSrc): kernel arguments and captured graphs keep their
// addresses. No map from stored entry to source entry exists for the sliced layouts -- the layout already determines it:
//   k_refresh_verify   read-only: the values of constant and masked slices live in lists shared between slices (SellDev::uval,
//                      StencilTab) and are never rewritten; any new value that differs from its list entry raises the flag
//   k_refresh_pad      padded slices: entry k of row r -> slice_base[r / 64] + 64 k + r % 64 (k_plan_fill's rule); padding untouched
//   k_refresh_jag      jagged slices: one wavefront per slice replays fill_slices' packing -- at step k the lanes whose row is
//                      longer than k (a ballot) store in lane order behind the entries of the steps before
//   k_refresh_rows     CSR order, one wavefront per row (the row blocks of a reordered context: row r' comes from caller row perm[r'])
//   k_refresh_persist  the persistent plan's padded slices through its source map (PersistPlan::psrc)
// Wave64, lane = row as in the products: each lane walks its own source row with 8-byte loads, the stores of a step are
// coalesced. No atomics, no LDS. gfx950 only.
#include "bicg_device.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicg {
namespace {

constexpr int kThreads = kGroupRows;
constexpr uint32_t kSlicesPerGroup = kGroupRows / kSliceRows;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// first source entry of the context's row r
__device__ __forceinline__ const double *row_src(const RefreshSrc &s, uint32_t r)
{
    return s.val + s.ptr[s.rowmap ? s.rowmap[r] : r];
}

__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// one wavefront per slice, lane = row (list-held slices have all their 64 rows and are never dealt out by length)
__global__ void __launch_bounds__(kThreads) k_refresh_verify(RefreshSrc src, const uint32_t *__restrict__ dptr, uint32_t nrows, uint32_t nslices,
                                                             const uint32_t *__restrict__ slice_len, const uint32_t *__restrict__ vbase,
                                                             const uint32_t *__restrict__ mbase, const unsigned short *__restrict__ rmask,
                                                             const double *__restrict__ uval, int *flag)
{
    const uint32_t sl = blockIdx.x * kSlicesPerGroup + threadIdx.x / kSliceRows, lane = threadIdx.x % kSliceRows;
    if (sl >= nslices) return;                                                    // (wave-uniform, like the two below)
    const uint32_t vb = vbase[sl];
    if (vb == kNone) return;
    const uint32_t mb = mbase ? mbase[sl] : kNone;
    const uint32_t r = sl * kSliceRows + lane;
    bool ok = true;
    if (r < nrows) {
        const double *v = row_src(src, r);
        const uint32_t len = dptr[r + 1] - dptr[r];
        if (mb != kNone) {                                                        // the j-th stored entry sits at the j-th set bit of the row's mask
            const uint32_t ulen = mb >> 26, mask = rmask[(size_t)(mb & 0x03FFFFFFu) * kSliceRows + lane];
            uint32_t j = 0;
            for (uint32_t k = 0; k < ulen && j < len; ++k)
                if ((mask >> k) & 1u) { ok = ok && same_bits(v[j], uval[vb + k]); ++j; }
        } else {
            const uint32_t n = min(len, slice_len[sl]);
            for (uint32_t k = 0; k < n; ++k) ok = ok && same_bits(v[k], uval[vb + k]);
        }
    }
    if (!ok) *flag = 1;                                                           // (every writer stores the same word)
}

// one workgroup per 256-row group of the sliced path (glist: the groups, null = 0 .. gridDim.x - 1)
__global__ void __launch_bounds__(kThreads) k_refresh_pad(RefreshSrc src, const uint32_t *__restrict__ dptr, uint32_t nrows,
                                                          const uint32_t *__restrict__ glist, const uint32_t *__restrict__ slice_base,
                                                          double *__restrict__ sval)
{
    const uint32_t g = glist ? glist[blockIdx.x] : blockIdx.x;
    const uint32_t r = g * kGroupRows + threadIdx.x;
    if (r >= nrows) return;
    const double *v = row_src(src, r);
    const uint32_t len = dptr[r + 1] - dptr[r];
    double *out = sval + (size_t)slice_base[r / kSliceRows] + r % kSliceRows;
    for (uint32_t k = 0; k < len; ++k) out[(size_t)k * kSliceRows] = v[k];         // consecutive lanes write consecutive entries
}

__global__ void __launch_bounds__(kThreads) k_refresh_jag(RefreshSrc src, const uint32_t *__restrict__ dptr, uint32_t nrows, uint32_t nslices,
                                                          const uint32_t *__restrict__ glist, const uint32_t *__restrict__ slice_base,
                                                          const unsigned char *__restrict__ perm, double *__restrict__ sval)
{
    const uint32_t g = glist ? glist[blockIdx.x] : blockIdx.x;
    const uint32_t sl = g * kSlicesPerGroup + threadIdx.x / kSliceRows;
    if (sl >= nslices) return;                                                    // (wave-uniform)
    // the row this lane works on: fill_slices' row_of()
    const uint32_t r = g * kGroupRows + (perm ? (uint32_t)perm[(size_t)g * kGroupRows + threadIdx.x] : threadIdx.x);
    const bool live = r < nrows;
    const double *v = live ? row_src(src, r) : src.val;
    const uint32_t len = live ? dptr[r + 1] - dptr[r] : 0u;
    size_t e = slice_base[sl];
    for (uint32_t k = 0;; ++k) {
        const unsigned long long longer = __ballot(len > k);
        if (!longer) break;
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(longer >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)longer, 0u));
        if (len > k) sval[e + before] = v[k];
        e += (uint32_t)__popcll(longer);
    }
}

// four rows per workgroup, a wavefront each
__global__ void __launch_bounds__(kThreads) k_refresh_rows(RefreshSrc src, const uint32_t *__restrict__ dptr, uint32_t nrows, double *__restrict__ dst)
{
    const uint32_t r = blockIdx.x * kSlicesPerGroup + threadIdx.x / kSliceRows, lane = threadIdx.x % kSliceRows;
    if (r >= nrows) return;
    const double *v = row_src(src, r);
    const uint32_t a = dptr[r], len = dptr[r + 1] - a;
    for (uint32_t k = lane; k < len; k += kSliceRows) dst[(size_t)a + k] = v[k];
}

__global__ void __launch_bounds__(kThreads) k_refresh_persist(const double *__restrict__ dval, const double *__restrict__ oval, uint32_t nnz_d,
                                                              const uint32_t *__restrict__ psrc, uint32_t n, double *__restrict__ pval)
{
    const uint32_t e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const uint32_t s = psrc[e];
    pval[e] = s == kNone ? 0.0 : (s < nnz_d ? dval[s] : oval[s - nnz_d]);
}

}  // namespace

void launch_refresh_verify(const RefreshSrc &src, const uint32_t *dptr, uint32_t nrows, const SellDev &d, int *flag, hipStream_t st)
{
    const uint32_t nslices = (nrows + kSliceRows - 1) / kSliceRows;
    if (!d.vbase || nslices == 0) return;
    hipLaunchKernelGGL(k_refresh_verify, dim3((nslices + kSlicesPerGroup - 1) / kSlicesPerGroup), dim3(kThreads), 0, st, src, dptr, nrows, nslices,
                       d.slice_len, d.vbase, d.mbase, d.rmask, d.uval, flag);
}

void launch_refresh_sell(const RefreshSrc &src, const uint32_t *dptr, uint32_t nrows, const SellDev &d, const uint32_t *glist, uint32_t nlist,
                         double *sval, hipStream_t st)
{
    if (nlist == 0) return;
    const uint32_t nslices = (nrows + kSliceRows - 1) / kSliceRows;
    if (d.jag) hipLaunchKernelGGL(k_refresh_jag, dim3(nlist), dim3(kThreads), 0, st, src, dptr, nrows, nslices, glist, d.slice_base, d.perm, sval);
    else hipLaunchKernelGGL(k_refresh_pad, dim3(nlist), dim3(kThreads), 0, st, src, dptr, nrows, glist, d.slice_base, sval);
}

void launch_refresh_rows(const RefreshSrc &src, const uint32_t *dptr, uint32_t nrows, double *dst, hipStream_t st)
{
    if (nrows == 0) return;
    hipLaunchKernelGGL(k_refresh_rows, dim3((nrows + kSlicesPerGroup - 1) / kSlicesPerGroup), dim3(kThreads), 0, st, src, dptr, nrows, dst);
}

void launch_refresh_persist(const double *dval, const double *oval, uint32_t nnz_d, const uint32_t *psrc, uint32_t n, double *pval, hipStream_t st)
{
    if (n == 0) return;
    hipLaunchKernelGGL(k_refresh_persist, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, dval, oval, nnz_d, psrc, n, pval);
}

}  // namespace bicg
