// bicg_vecio.hip -- the caller's DEVICE vectors crossing into / out of the solver's vectors (bicg_load_device, bicg_fetch_device and
// the calls built on them). One kernel family: up to two (source, destination) pairs x nvec columns in one
// launch -- load moves x0 and b together, fetch x and r --, blockIdx.y = pair * nvec + column as in bicg_reorder.hip, source and
// destination with leading dimensions of their own (the caller's ld, the solver's stride).
//   identity   dst[j][i] = src[j][i]
//   gather     dst[j][i] = src[j][idx[i]]      (a reordered context: idx = perm on the way in, inv on the way out, so that the
//                                               stores are coalesced in both directions -- permute_body's gather, bicg_reorder.hip)
// A lane owns kPerLane consecutive elements. The caller's arrays are 8-byte aligned in general (a view that starts one element into
// a buffer, an odd ld), the solver's vectors 256-byte aligned with stride % 32 == 0: a side whose pointer and leading dimension
// allow it is accessed 16 bytes at a time (SRC16 / DST16), the other 8; the launcher decides per pair. The last lane with rows
// takes the n % kPerLane elements left. Plain loads and stores: the solver (or the caller) reads these vectors next, they should
// stay in the caches. The sources are never written. gfx950 only.
#include "bicg_device.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicg {
namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int kThreads = 256;
constexpr int kPerLane = 4;

struct VecioArgs {
    VecPair p[2];
    const uint32_t *idx;      // GATHER only
    uint32_t n, nvec;
    uint32_t idx16;           // idx is 16-byte aligned: one load for a lane's four indices
};

template <bool GATHER, bool SRC16, bool DST16>
__global__ void __launch_bounds__(kThreads) k_vecio(const VecioArgs a)
{
    const uint32_t pair = blockIdx.y / a.nvec, col = blockIdx.y - pair * a.nvec;      // (uniform; the launcher keeps pair < 2)
    const VecPair pr = a.p[pair];
    const double *__restrict__ s = pr.src + (size_t)col * pr.src_ld;
    double *__restrict__ d = pr.dst + (size_t)col * pr.dst_ld;
    const size_t n = a.n;
    const size_t i0 = ((size_t)blockIdx.x * kThreads + threadIdx.x) * kPerLane;
    if (i0 >= n) return;
    if (i0 + kPerLane > n) {                                           // the last lane with rows: fewer than kPerLane left
        for (size_t i = i0; i < n; ++i) d[i] = GATHER ? s[a.idx[i]] : s[i];
        return;
    }
    double v0, v1, v2, v3;
    if (GATHER) {
        uint4 q;
        if (a.idx16) q = *reinterpret_cast<const uint4 *>(a.idx + i0);
        else { q.x = a.idx[i0]; q.y = a.idx[i0 + 1]; q.z = a.idx[i0 + 2]; q.w = a.idx[i0 + 3]; }
        v0 = s[q.x]; v1 = s[q.y]; v2 = s[q.z]; v3 = s[q.w];
    } else if (SRC16) {
        const f64x2 lo = *reinterpret_cast<const f64x2 *>(s + i0), hi = *reinterpret_cast<const f64x2 *>(s + i0 + 2);
        v0 = lo.x; v1 = lo.y; v2 = hi.x; v3 = hi.y;
    } else {
        v0 = s[i0]; v1 = s[i0 + 1]; v2 = s[i0 + 2]; v3 = s[i0 + 3];
    }
    if (DST16) {
        f64x2 lo, hi;
        lo.x = v0; lo.y = v1; hi.x = v2; hi.y = v3;
        *reinterpret_cast<f64x2 *>(d + i0) = lo;
        *reinterpret_cast<f64x2 *>(d + i0 + 2) = hi;
    } else {
        d[i0] = v0; d[i0 + 1] = v1; d[i0 + 2] = v2; d[i0 + 3] = v3;
    }
}

// 16-byte accesses need every column of the side to start on a 16-byte boundary (one column: the leading dimension is not used)
bool side16(const double *p, size_t ld, int nvec) { return (uintptr_t)p % 16 == 0 && (nvec == 1 || ld % 2 == 0); }

void launch_pairs(const VecPair *pairs, int npairs, bool src16, bool dst16, const uint32_t *idx, uint32_t n, int nvec, hipStream_t st)
{
    VecioArgs a{};
    for (int i = 0; i < npairs; ++i) a.p[i] = pairs[i];
    a.idx = idx; a.n = n; a.nvec = (uint32_t)nvec; a.idx16 = (uintptr_t)idx % 16 == 0 ? 1u : 0u;
    const uint64_t per_block = (uint64_t)kThreads * kPerLane;
    const dim3 grid((unsigned)(((uint64_t)n + per_block - 1) / per_block), (unsigned)(npairs * nvec), 1), block(kThreads);
    if (idx) {
        if (dst16) hipLaunchKernelGGL((k_vecio<true, false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_vecio<true, false, false>), grid, block, 0, st, a);
    } else if (src16) {
        if (dst16) hipLaunchKernelGGL((k_vecio<false, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_vecio<false, true, false>), grid, block, 0, st, a);
    } else {
        if (dst16) hipLaunchKernelGGL((k_vecio<false, false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_vecio<false, false, false>), grid, block, 0, st, a);
    }
}

}  // namespace

void launch_vecio(const VecPair *pairs, int npairs, const uint32_t *idx, uint32_t n, int nvec, hipStream_t st)
{
    if (n == 0 || nvec <= 0 || npairs <= 0) return;
    if (npairs > 2) npairs = 2;
    bool s16[2], d16[2];
    for (int i = 0; i < npairs; ++i) {
        s16[i] = !idx && side16(pairs[i].src, pairs[i].src_ld, nvec);      // (a gathered source is read 8 bytes at a time)
        d16[i] = side16(pairs[i].dst, pairs[i].dst_ld, nvec);
    }
    // one launch when both pairs take the same accesses (the usual case: two views of equal alignment), else one per pair
    if (npairs == 2 && s16[0] == s16[1] && d16[0] == d16[1]) { launch_pairs(pairs, 2, s16[0], d16[0], idx, n, nvec, st); return; }
    for (int i = 0; i < npairs; ++i) launch_pairs(pairs + i, 1, s16[i], d16[i], idx, n, nvec, st);
}

}  // namespace bicg
