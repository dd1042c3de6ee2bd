// bicg_bjacobi.hip -- the block-Jacobi preconditioner (bicg_precond_block_diagonal / _device, BICG_BICGSTAB_BLOCK; DESIGN.md section
// 4.21): M = the bs x bs diagonal blocks of the caller's choosing, bs = 1 .. 16, blocks in the CALLER's numbering.
//   k_bjac_invert   install, one-off: one thread per block, Gauss-Jordan with partial pivoting in place, in call-temporary scratch
//                   laid out entry-major (entry (a, j) of block k at w[(a bs + j) nblocks + k]: neighbouring threads touch
//                   neighbouring words). A non-finite entry, a zero or non-finite pivot or a non-finite result raises the flag.
//   k_bjac_planes   the clean inverses into the resident layout: bs planes of `stride` doubles in the CONTEXT's numbering,
//                   minv[j stride + i] = the entry that multiplies mate j of row i; zeros in the planes beyond a partial block.
//   k_bjac_apply    hot: out[i] = sum_j minv[j stride + i] in[mate_j(i)], one row per lane, every plane read coalesced, the mates
//                   read straight from `in` (a block's mates are neighbours in memory: the lanes of a wavefront share their lines).
//                   acc = m_0 v_0, then acc = fma(m_j, v_j, acc) for j ascending over the block's rows -- the same for every grid
//                   shape, rank count and layout. A block may straddle wavefronts and workgroups: no lane depends on another.
//   k_bjac_apply_set  the same on the columns of a multi-RHS set in one launch, a row's plane entries loaded once for the set (below)
// A reordered context keeps the blocks the caller's: context row i belongs to block perm[i] / bs and finds its mates through inv.
// Vector loads and stores only. gfx950 only.
#include "bicg_device.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bicg {
namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads) k_bjac_invert(const double *__restrict__ blocks, uint32_t n, uint32_t bs, uint32_t nb,
                                                          double *__restrict__ w, int *flag)
{
    const uint32_t k = blockIdx.x * kThreads + threadIdx.x;      // (the launcher keeps the grid within 32 bits: nb <= n < 2^32)
    bool bad = false;
    if (k < nb) {
        const uint32_t m = min(bs, n - k * bs);                  // rows the block covers: only its leading m x m part is read
        const double *src = blocks + (size_t)k * bs * bs;
        auto W = [&](uint32_t a, uint32_t j) -> double & { return w[((size_t)a * bs + j) * nb + k]; };
        for (uint32_t a = 0; a < m; ++a)
            for (uint32_t j = 0; j < m; ++j) {
                const double v = src[a * bs + j];
                bad |= !isfinite(v);
                W(a, j) = v;
            }
        uint64_t piv = 0;                                        // the row exchanged with row c, four bits each
        for (uint32_t c = 0; c < m; ++c) {
            uint32_t p = c;
            double best = fabs(W(c, c));
            for (uint32_t a = c + 1; a < m; ++a) {               // largest magnitude in column c among rows >= c, the first wins a tie
                const double t = fabs(W(a, c));
                if (t > best) { best = t; p = a; }
            }
            if (p != c)
                for (uint32_t j = 0; j < m; ++j) { const double t = W(c, j); W(c, j) = W(p, j); W(p, j) = t; }
            piv |= (uint64_t)p << (4u * c);
            const double pv = W(c, c);
            bad |= pv == 0.0 || !isfinite(pv);
            W(c, c) = 1.0;                                       // (in place: column c takes the inverse's column from here on)
            for (uint32_t j = 0; j < m; ++j) W(c, j) = W(c, j) / pv;
            for (uint32_t a = 0; a < m; ++a) {
                if (a == c) continue;
                const double f = W(a, c);
                W(a, c) = 0.0;
                for (uint32_t j = 0; j < m; ++j) W(a, j) = W(a, j) - f * W(c, j);
            }
        }
        for (uint32_t c = m; c-- > 0;) {                         // the row exchanges come back as column exchanges, last first
            const uint32_t p = (uint32_t)(piv >> (4u * c)) & 15u;
            if (p != c)
                for (uint32_t a = 0; a < m; ++a) { const double t = W(a, c); W(a, c) = W(a, p); W(a, p) = t; }
        }
        for (uint32_t a = 0; a < m; ++a)
            for (uint32_t j = 0; j < m; ++j) bad |= !isfinite(W(a, j));
    }
    // one store per wavefront that saw a bad block (every writer stores the same word: no atomic needed)
    if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) *flag = 1;
}

__global__ void __launch_bounds__(kThreads) k_bjac_planes(const double *__restrict__ w, const uint32_t *__restrict__ perm, uint32_t n,
                                                          uint32_t bs, uint32_t nb, double *__restrict__ minv, size_t stride)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = perm ? perm[i] : i;                       // the caller's row
    const uint32_t k = o / bs, a = o - k * bs;
    const uint32_t m = min(bs, n - k * bs);
    for (uint32_t j = 0; j < bs; ++j) minv[(size_t)j * stride + i] = j < m ? w[((size_t)a * bs + j) * nb + k] : 0.0;
}

template <int BS, bool RO>
__global__ void __launch_bounds__(kThreads) k_bjac_apply(const double *__restrict__ minv, size_t stride, const uint32_t *__restrict__ perm,
                                                         const uint32_t *__restrict__ inv, const double *__restrict__ in,
                                                         double *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = RO ? perm[i] : i;
    const uint32_t base = (o / (uint32_t)BS) * (uint32_t)BS;     // the block's first row, caller's numbering
    const uint32_t m = min((uint32_t)BS, n - base);
    double mv[BS], vv[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j) mv[j] = minv[(size_t)j * stride + i];
#pragma unroll
    for (int j = 0; j < BS; ++j) {
        const uint32_t mate = base + (uint32_t)j;
        vv[j] = (uint32_t)j < m ? in[RO ? inv[mate] : mate] : 0.0;
    }
    double acc = mv[0] * vv[0];
#pragma unroll
    for (int j = 1; j < BS; ++j)
        if ((uint32_t)j < m) acc = fma(mv[j], vv[j], acc);
    out[i] = acc;
}

template <int BS>
void apply_bs(const double *minv, size_t stride, const uint32_t *perm, const uint32_t *inv, const double *in, double *out, uint32_t n,
              hipStream_t st)
{
    const unsigned grid = (unsigned)(((uint64_t)n + kThreads - 1) / kThreads);
    if (perm) hipLaunchKernelGGL((k_bjac_apply<BS, true>), dim3(grid), dim3(kThreads), 0, st, minv, stride, perm, inv, in, out, n);
    else hipLaunchKernelGGL((k_bjac_apply<BS, false>), dim3(grid), dim3(kThreads), 0, st, minv, stride, perm, inv, in, out, n);
}

// k_bjac_apply on the columns of a multi-RHS set (bicg_solve_multi, method 5) in ONE launch: column c of in / out starts at
// c vstride. A thread owns one row: its BS plane entries, and on a reordered context its BS mate indices, are loaded ONCE and stay in
// registers while it walks the CH columns blockIdx.y selects -- the planes cost 8 BS bytes per row and chunk instead of per column.
// The mate loads of FLY columns are in flight before the first fma. A column's sum is k_bjac_apply's, term for term: the same bytes.
// A column whose flag S->active is 0 is neither read nor written; the flags are workgroup-uniform and read once, before any vector.
template <int BS, bool RO, int CH>
__global__ void __launch_bounds__(kThreads) k_bjac_apply_set(const double *__restrict__ minv, size_t stride, const uint32_t *__restrict__ perm,
                                                             const uint32_t *__restrict__ inv, const double *__restrict__ in,
                                                             double *__restrict__ out, size_t vstride, uint32_t n, int nv,
                                                             const MultiScal *__restrict__ S)
{
    constexpr int FLY = BS <= 4 ? (CH < 8 ? CH : 8) : BS <= 8 ? 4 : 2;      // columns in flight: at most 32 mates in registers
    static_assert(CH % FLY == 0 && CH <= kSpmmCols, "a chunk is whole groups of FLY columns");
    const int c0 = (int)blockIdx.y * CH;
    unsigned live = 0;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        if (c0 + c < nv && S->active[c0 + c]) live |= 1u << c;
    if (!live) return;
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t o = RO ? perm[i] : i;
    const uint32_t base = (o / (uint32_t)BS) * (uint32_t)BS;     // the block's first row, caller's numbering
    const uint32_t m = min((uint32_t)BS, n - base);
    double mv[BS];
    uint32_t at[BS];                                             // the mates in the context's numbering (0 beyond a partial block: not read)
#pragma unroll
    for (int j = 0; j < BS; ++j) mv[j] = minv[(size_t)j * stride + i];
#pragma unroll
    for (int j = 0; j < BS; ++j) {
        const uint32_t mate = base + (uint32_t)j;
        at[j] = (uint32_t)j < m ? (RO ? inv[mate] : mate) : 0u;
    }
#pragma unroll
    for (int g = 0; g < CH; g += FLY) {
        if (!((live >> g) & ((1u << FLY) - 1u))) continue;
        double vv[FLY][BS];
#pragma unroll
        for (int f = 0; f < FLY; ++f) {
            const double *col = in + (size_t)(c0 + g + f) * vstride;
#pragma unroll
            for (int j = 0; j < BS; ++j) vv[f][j] = ((live >> (g + f)) & 1u) && (uint32_t)j < m ? col[at[j]] : 0.0;
        }
#pragma unroll
        for (int f = 0; f < FLY; ++f) {
            if (!((live >> (g + f)) & 1u)) continue;
            double acc = mv[0] * vv[f][0];
#pragma unroll
            for (int j = 1; j < BS; ++j)
                if ((uint32_t)j < m) acc = fma(mv[j], vv[f][j], acc);
            out[(size_t)(c0 + g + f) * vstride + i] = acc;
        }
    }
}

template <int BS, int CH>
void apply_set_ch(const double *minv, size_t stride, const uint32_t *perm, const uint32_t *inv, const double *in, double *out, size_t vstride,
                  uint32_t n, int nv, const MultiScal *S, hipStream_t st)
{
    const dim3 grid((unsigned)(((uint64_t)n + kThreads - 1) / kThreads), (unsigned)((nv + CH - 1) / CH));
    if (perm) hipLaunchKernelGGL((k_bjac_apply_set<BS, true, CH>), grid, dim3(kThreads), 0, st, minv, stride, perm, inv, in, out, vstride, n, nv, S);
    else hipLaunchKernelGGL((k_bjac_apply_set<BS, false, CH>), grid, dim3(kThreads), 0, st, minv, stride, perm, inv, in, out, vstride, n, nv, S);
}

template <int BS>
void apply_set_bs(const double *minv, size_t stride, const uint32_t *perm, const uint32_t *inv, const double *in, double *out, size_t vstride,
                  uint32_t n, int nv, const MultiScal *S, int chunk, hipStream_t st)
{
    switch (chunk) {
    case 4:  apply_set_ch<BS, 4>(minv, stride, perm, inv, in, out, vstride, n, nv, S, st); break;
    case 8:  apply_set_ch<BS, 8>(minv, stride, perm, inv, in, out, vstride, n, nv, S, st); break;
    case 16: apply_set_ch<BS, 16>(minv, stride, perm, inv, in, out, vstride, n, nv, S, st); break;
    default: apply_set_ch<BS, bjac_set_chunk(BS)>(minv, stride, perm, inv, in, out, vstride, n, nv, S, st); break;
    }
}

}  // namespace

void launch_bjac_invert(const double *blocks, uint32_t n, int bs, double *work, int *flag, hipStream_t st)
{
    if (n == 0) return;
    const uint32_t nb = bjac_blocks(n, bs);
    const unsigned grid = (unsigned)(((uint64_t)nb + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_bjac_invert, dim3(grid), dim3(kThreads), 0, st, blocks, n, (uint32_t)bs, nb, work, flag);
}

void launch_bjac_planes(const double *work, const uint32_t *perm, uint32_t n, int bs, double *minv, size_t stride, hipStream_t st)
{
    if (n == 0) return;
    const unsigned grid = (unsigned)(((uint64_t)n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_bjac_planes, dim3(grid), dim3(kThreads), 0, st, work, perm, n, (uint32_t)bs, bjac_blocks(n, bs), minv, stride);
}

void launch_bjac_apply(const double *minv, size_t stride, int bs, const uint32_t *perm, const uint32_t *inv, const double *in, double *out,
                       uint32_t n, hipStream_t st)
{
    if (n == 0) return;
    switch (bs) {
#define BICG_BJAC_CASE(B) case B: apply_bs<B>(minv, stride, perm, inv, in, out, n, st); break;
    BICG_BJAC_CASE(1) BICG_BJAC_CASE(2) BICG_BJAC_CASE(3) BICG_BJAC_CASE(4) BICG_BJAC_CASE(5) BICG_BJAC_CASE(6) BICG_BJAC_CASE(7) BICG_BJAC_CASE(8)
    BICG_BJAC_CASE(9) BICG_BJAC_CASE(10) BICG_BJAC_CASE(11) BICG_BJAC_CASE(12) BICG_BJAC_CASE(13) BICG_BJAC_CASE(14) BICG_BJAC_CASE(15) BICG_BJAC_CASE(16)
#undef BICG_BJAC_CASE
    default: break;      // (the installer admits 1 .. 16 only)
    }
}

void launch_bjac_apply_set(const double *minv, size_t stride, int bs, const uint32_t *perm, const uint32_t *inv, const double *in, double *out,
                           size_t vstride, uint32_t n, int nv, const MultiScal *S, int chunk, hipStream_t st)
{
    if (n == 0 || nv < 1) return;
    switch (bs) {
#define BICG_BJAC_CASE(B) case B: apply_set_bs<B>(minv, stride, perm, inv, in, out, vstride, n, nv, S, chunk, st); break;
    BICG_BJAC_CASE(1) BICG_BJAC_CASE(2) BICG_BJAC_CASE(3) BICG_BJAC_CASE(4) BICG_BJAC_CASE(5) BICG_BJAC_CASE(6) BICG_BJAC_CASE(7) BICG_BJAC_CASE(8)
    BICG_BJAC_CASE(9) BICG_BJAC_CASE(10) BICG_BJAC_CASE(11) BICG_BJAC_CASE(12) BICG_BJAC_CASE(13) BICG_BJAC_CASE(14) BICG_BJAC_CASE(15) BICG_BJAC_CASE(16)
#undef BICG_BJAC_CASE
    default: break;
    }
}

}  // namespace bicg
