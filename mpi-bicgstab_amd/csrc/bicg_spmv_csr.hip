// bicg_spmv_csr.hip -- the products that read the CSR arrays as they are: the row-block stream kernel (k_spmv) and rows over
// lanes (k_spmv_rows, long rows).
//
//   k_spmv        CSR "row-block stream" SpMV: a 256-thread workgroup owns a block of whole rows
//                 holding <= 2048 non-zeros, streams val/col fully coalesced (8 per thread, all
//                 loads in flight before the first use), gathers x, stages the products in LDS
//                 and reduces every row from LDS in stored order; fused dot-product epilogue.
//                 Replaces mult() + MPI_csr_spmv_ovlap (reference src/matrix.c:498-516, 428-441).
//
// Compiled with -ffp-contract=off: every a*b+c keeps the two roundings of the reference's scalar
// loops, so the element-wise phases and every SpMV row are bit-identical to the CPU oracle; only
// the association of the dot-product sums differs.
#include "bicg_device.h"
#include "bicg_devfn.h"
#include "bicg_reduce.h"
#include "bicg_knobs.h"
#include "bicg_launch.h"

namespace bicg {

// ------------------------------------------------------------------------------------------
// CSR SpMV, row-block stream
// ------------------------------------------------------------------------------------------
// CSR row-block stream kernel (ragged / long-row groups; the whole matrix when BICG_NO_SELL=1).
// Variants that were measured on Transport and dropped (profiles/r01_csr_baseline): an XCD-aware
// block mapping (fabric reads 386 -> 309 MB, wall time +3-5 %), 16-byte val/col loads (+2 us), a
// 2048-workgroup persistent grid-stride form (67.8 vs 60.5 us) and a software-pipelined persistent
// form that prefetches the next block's stream (67 us, flat in the number of resident workgroups):
// the kernel is bound by the vector L1's tag rate on the row-major x gather, which is what the
// sliced-ELL kernel below removes.

template <bool NT, class T> __device__ __forceinline__ T stream_load(const T *p)
{
    if (NT) return __builtin_nontemporal_load(p);
    return *p;
}

template <int NDOT, bool OFFD, bool NT, int MODE>
__global__ void __launch_bounds__(kBlock) k_spmv(SpmvArgs a)
{
    if (MODE == RED_WAVE) {
        __shared__ FinishLds fl;
        if (a.fin.seq && (blockIdx.x < (unsigned)kShards || (a.fin.roles & FIN_APPLY))) (void)finish_group(a.S, a.fin, a.fin.roles, blockIdx.x, gridDim.x, fl, nullptr);
    }
    // The sticky convergence flag is requested here but only consumed where state would be
    // modified (y stores, dot publication): an early `if (done) return` would put one more
    // dependent global load in front of every workgroup's stream.
    const int done = a.S->done;
    __shared__ __attribute__((aligned(16))) double prod[kChunk];
    __shared__ double sm[5 * (NDOT > 0 ? NDOT : 1)];

    const unsigned tid = threadIdx.x;
    const double *__restrict__ x = a.x;

    double acc[NDOT > 0 ? NDOT : 1];
#pragma unroll
    for (int d = 0; d < (NDOT > 0 ? NDOT : 1); ++d) acc[d] = 0.0;

    const unsigned first = blockIdx.x, last = a.nlist, step = gridDim.x;

    for (unsigned bi = first; bi < last; bi += step) {
        // one 16-byte descriptor per row block {first row, end row, first nnz, end nnz}: a single
        // wave-uniform load instead of the dependent chain rowblk -> ptr -> val/col
        const uint4 d = a.desc[bi];
        const uint32_t r0 = d.x, r1 = d.y, j0 = d.z, j1 = d.w;
        const uint32_t jw = j0;                                      // start of the staged window

        // this thread's (first) row: its pointers and dot operand are requested now, together with
        // the val/col stream, not after the barrier
        const uint32_t rme = r0 + tid;
        const bool mine = rme < r1;
        const uint32_t pa = mine ? a.diag.ptr[rme] : 0u, pb = mine ? a.diag.ptr[rme + 1] : 0u;
        uint32_t oa = 0u, ob = 0u;
        if (OFFD && mine) { oa = a.offd.ptr[rme]; ob = a.offd.ptr[rme + 1]; }
        double ume = 0.0;
        if (NDOT >= 1 && mine) ume = a.u[rme];

        auto finish_row = [&](uint32_t r, uint32_t a0, uint32_t a1, uint32_t o0, uint32_t o1, double ur) {
            double sum = 0.0;
            // 8 LDS reads in flight, then added in stored order (the order of reference
            // src/matrix.c:511-513); entries past the row end are replaced by +0.0, which leaves the
            // running sum unchanged bit for bit (a sum that is -0.0 would become +0.0, and the
            // reference's `0.0 + tempy` does that anyway)
            for (uint32_t k = a0; k < a1; k += 8) {
                double t[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint32_t kk = k + e < a1 ? k + e : a1 - 1;
                    t[e] = prod[kk];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) sum += (k + e < a1) ? t[e] : 0.0;
            }
            double yi = 0.0 + sum;                           // y = 0 ; y += tempy  (src/matrix.c:434-437, 514)
            if (OFFD) {
                double so = 0.0;
                for (uint32_t k = o0; k < o1; ++k) so += a.offd.val[k] * x[a.offd.col[k]];
                yi += so;                                    // second mult() call, src/matrix.c:440
            }
            if (a.has_shift) yi += a.shift * x[r];           // (A + sigma I) x, src/shifted_solver.c:260
            if (!done) a.y[r] = yi;
            if (NDOT >= 1) acc[0] += ur * yi;
            if (NDOT == 2) acc[NDOT >= 2 ? 1 : 0] += yi * yi;
            if (NDOT == 3) acc[NDOT >= 2 ? 1 : 0] += ur * ur;
        };

        if (j1 - jw <= (uint32_t)kChunk) {
            // stream: all val/col loads of the block are issued before the first gather
            {
                uint32_t c[kNnzPerThread];
                double   v[kNnzPerThread];
#pragma unroll
                for (int i = 0; i < kNnzPerThread; ++i) {
                    const uint32_t j = j0 + tid + i * kBlock;
                    const bool ok = j < j1;
                    c[i] = ok ? stream_load<NT>(a.diag.col + j) : 0u;
                    v[i] = ok ? stream_load<NT>(a.diag.val + j) : 0.0;
                }
#pragma unroll
                for (int i = 0; i < kNnzPerThread; ++i) prod[tid + i * kBlock] = v[i] * x[c[i]];
            }
            __syncthreads();
            // one thread per row
            if (mine) finish_row(rme, pa - jw, pb - jw, oa, ob, ume);
            for (uint32_t r = rme + kBlock; r < r1; r += kBlock)     // blocks of very short rows
                finish_row(r, a.diag.ptr[r] - jw, a.diag.ptr[r + 1] - jw, OFFD ? a.offd.ptr[r] : 0u,
                           OFFD ? a.offd.ptr[r + 1] : 0u, NDOT >= 1 ? a.u[r] : 0.0);
        } else {
            // a single row longer than the chunk: strided partial sums + workgroup reduction
            double part[1] = {0.0};
            for (uint32_t j = j0 + tid; j < j1; j += kBlock) part[0] += a.diag.val[j] * x[a.diag.col[j]];
            block_sum<1>(part, sm);
            if (tid == 0) {
                double yi = 0.0 + part[0];
                if (OFFD) {
                    double so = 0.0;
                    for (uint32_t k = oa; k < ob; ++k) so += a.offd.val[k] * x[a.offd.col[k]];
                    yi += so;
                }
                if (a.has_shift) yi += a.shift * x[r0];
                if (!done) a.y[r0] = yi;
                if (NDOT >= 1) acc[0] += ume * yi;
                if (NDOT == 2) acc[NDOT >= 2 ? 1 : 0] += yi * yi;
                if (NDOT == 3) acc[NDOT >= 2 ? 1 : 0] += ume * ume;
            }
        }
        __syncthreads();   // prod is rewritten by the next row block
    }
    if (NDOT > 0 && !done) {
        if (MODE == RED_WAVE) wave_publish<(NDOT > 0 ? NDOT : 1)>(acc, a.red.partial, a.red.slot_base + blockIdx.x);
        else reduce_publish<(NDOT > 0 ? NDOT : 1), MODE == RED_TICKET_HEAVY>(acc, a.S, a.red, a.red.slot_base + blockIdx.x, sm);
    }
}

// One workgroup per row block: the hardware dispatcher balances the ~12k workgroups of a
// Transport-sized matrix better than a persistent grid; beyond kSpmvMaxGrid row blocks the kernel's
// loop strides. That grid is spmv_grid() (bicg_spmv_plan.cpp).
//
// Slot contract with the launch plan of the distributed product (spmv_plan, bicg_plan.h): workgroup b
// of a launch publishes its dot partials in slot a.red.slot_base + b, and the plan numbers the slots
// of the launches that share a dot group by adding up spmv_grid() and sell_grid(). The grid launched
// below and the grid the plan counts must therefore be the same function.

template <int NDOT, bool OFFD>
static void launch_spmv_var(const SpmvArgs &a, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    dim3 g(spmv_grid(a.nlist)), b(kBlock);
    const int mode = red_mode(a.red, a.fin, NDOT > 0);
    constexpr int HV = NDOT > 0 ? RED_TICKET_HEAVY : RED_TICKET;   // without dots there is no epilogue to be heavy
    if (mode == RED_WAVE) {
        if (a.nt) launch_timed(k_spmv<NDOT, OFFD, true, RED_WAVE>, g, b, st, e0, e1, a);
        else launch_timed(k_spmv<NDOT, OFFD, false, RED_WAVE>, g, b, st, e0, e1, a);
    } else if (mode == RED_TICKET_HEAVY) {
        if (a.nt) launch_timed(k_spmv<NDOT, OFFD, true, HV>, g, b, st, e0, e1, a);
        else launch_timed(k_spmv<NDOT, OFFD, false, HV>, g, b, st, e0, e1, a);
    } else {
        if (a.nt) launch_timed(k_spmv<NDOT, OFFD, true, RED_TICKET>, g, b, st, e0, e1, a);
        else launch_timed(k_spmv<NDOT, OFFD, false, RED_TICKET>, g, b, st, e0, e1, a);
    }
}

// ------------------------------------------------------------------------------------------
// Rows over lanes (long rows). Lane = row (sliced ELL) needs >= 256 rows per workgroup: a block of a few ten
// thousand rows with ~1000 entries each (synthetic banded CSR, half-bandwidth 512: 23 415 rows = 92 workgroups
// for 256 CUs, every lane walking 128 dependent batches) ran at 0.27 of the HBM roofline. Here a row is spread
// over T = 8..64 lanes (T from the block's mean row length, wave-uniform): lane l adds entries l, l + T, l + 2T, ...
// of its row in stored order, 8 loads of val and col in flight per lane, the T partial sums are combined by a
// fixed butterfly (DPP inside rows of 16 lanes, two bpermute steps above) -- so val / col are read fully
// coalesced straight from the CSR arrays (16-bit column offsets when they fit: 10 B per non-zero), a workgroup
// holds a few rows only (row blocks of <= 8192 non-zeros) and a 24 M-non-zero matrix makes ~3000 workgroups
// whatever its row length. The association of a row's sum differs from mult() (reference src/matrix.c:506-515):
// the result agrees to ~1e-16 x sum |a_ij x_j|, tested at 1e-13 (north_star: a stated tolerance); it is fixed, so
// runs are bit-reproducible. Taken when the block's rows average >= 128 entries and lane = row would leave the
// GPU short of workgroups (bicg_create; BICG_ROWSPLIT=0/1 overrides).
// ------------------------------------------------------------------------------------------
template <int T>
__device__ __forceinline__ double lanes_sum(double v)     // every lane of each aligned group of T lanes gets the group's sum
{
    v = dpp_add<0xB1, 0xF>(v);                   // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xF>(v);                   // quad_perm [2,3,0,1]
    if (T >= 8) v = dpp_add<0x141, 0xF>(v);      // row_half_mirror
    if (T >= 16) v = dpp_add<0x140, 0xF>(v);     // row_mirror
    if (T >= 32) v += __shfl_xor(v, 16);
    if (T >= 64) v += __shfl_xor(v, 32);
    return v;
}

template <int NDOT, bool OFFD, bool NT, bool C16, int T, int MODE>
__device__ __forceinline__ void rows_block(const SpmvArgs &a, uint32_t r0, uint32_t r1, int done, double (&acc)[NDOT > 0 ? NDOT : 1])
{
    constexpr int U = 8;
    constexpr uint32_t NSUB = kBlock / T;
    const unsigned tid = threadIdx.x, sub = tid / T, l = tid % T;
    const double *__restrict__ x = a.x;
    for (uint32_t rb = r0; rb < r1; rb += NSUB) {               // workgroup-uniform trip count
        const uint32_t r = rb + sub;
        const bool have = r < r1;
        const uint32_t pa = have ? a.diag.ptr[r] : 0u, pb = have ? a.diag.ptr[r + 1] : 0u;
        const uint32_t rs = have ? r : r0;                      // a safe x index for lanes without an entry
        double ur = 0.0;
        if (NDOT >= 1 && have && l == 0) ur = a.u[r];
        double s = 0.0;
        for (uint32_t j0 = pa + l; j0 < pb; j0 += U * T) {
            uint32_t c[U];
            double   v[U];
            // raw loads only inside the predicated part (a use of a loaded value there costs one round trip per
            // entry, see sell_row); out-of-range entries multiply 0.0 with x[row]
#pragma unroll
            for (int e = 0; e < U; ++e) {
                const uint32_t j = j0 + e * T;
                const bool ok = j < pb;
                v[e] = 0.0;
                if (C16) {
                    int d = 0;
                    if (ok) { d = NT ? __builtin_nontemporal_load(a.diag_col16 + j) : a.diag_col16[j]; v[e] = stream_load<NT>(a.diag.val + j); }
                    c[e] = rs + (uint32_t)d;
                } else {
                    c[e] = rs;
                    if (ok) { c[e] = stream_load<NT>(a.diag.col + j); v[e] = stream_load<NT>(a.diag.val + j); }
                }
            }
            double xv[U];
#pragma unroll
            for (int e = 0; e < U; ++e) xv[e] = x[c[e]];
#pragma unroll
            for (int e = 0; e < U; ++e) s += v[e] * xv[e];
        }
        s = lanes_sum<T>(s);
        if (have && l == 0) {
            double yi = 0.0 + s;                                 // y = 0 ; y += tempy  (src/matrix.c:434-437)
            if (OFFD) {
                double so = 0.0;
                for (uint32_t k = a.offd.ptr[r]; k < a.offd.ptr[r + 1]; ++k) so += a.offd.val[k] * x[a.offd.col[k]];
                yi += so;                                        // second mult() call, src/matrix.c:440
            }
            if (a.has_shift) yi += a.shift * x[r];
            if (!done) a.y[r] = yi;
            if (NDOT >= 1) acc[0] += ur * yi;
            if (NDOT == 2) acc[NDOT >= 2 ? 1 : 0] += yi * yi;
            if (NDOT == 3) acc[NDOT >= 2 ? 1 : 0] += ur * ur;
        }
    }
}

template <int NDOT, bool OFFD, bool NT, bool C16, int MODE>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(MODE == RED_TICKET ? 8 : 4, 8))) k_spmv_rows(SpmvArgs a)
{
    if (MODE == RED_WAVE) {
        __shared__ FinishLds fl;
        if (a.fin.seq && (blockIdx.x < (unsigned)kShards || (a.fin.roles & FIN_APPLY))) (void)finish_group(a.S, a.fin, a.fin.roles, blockIdx.x, gridDim.x, fl, nullptr);
    }
    const int done = a.S->done;
    __shared__ double sm[5 * (NDOT > 0 ? NDOT : 1)];
    double acc[NDOT > 0 ? NDOT : 1];
#pragma unroll
    for (int d = 0; d < (NDOT > 0 ? NDOT : 1); ++d) acc[d] = 0.0;
    for (unsigned bi = blockIdx.x; bi < a.nlist; bi += gridDim.x) {
        const uint4 d = a.desc[bi];
        const uint32_t nr = d.y - d.x, mean = nr ? (d.w - d.z) / nr : 0u;
        // lanes per row from the block's mean row length (workgroup-uniform): ~8 entries per lane and batch
        if (mean >= 320u) rows_block<NDOT, OFFD, NT, C16, 64, MODE>(a, d.x, d.y, done, acc);
        else if (mean >= 160u) rows_block<NDOT, OFFD, NT, C16, 32, MODE>(a, d.x, d.y, done, acc);
        else if (mean >= 80u) rows_block<NDOT, OFFD, NT, C16, 16, MODE>(a, d.x, d.y, done, acc);
        else rows_block<NDOT, OFFD, NT, C16, 8, MODE>(a, d.x, d.y, done, acc);
    }
    if (NDOT > 0 && !done) {
        if (MODE == RED_WAVE) wave_publish<(NDOT > 0 ? NDOT : 1)>(acc, a.red.partial, a.red.slot_base + blockIdx.x);
        else reduce_publish<(NDOT > 0 ? NDOT : 1), MODE == RED_TICKET_HEAVY>(acc, a.S, a.red, a.red.slot_base + blockIdx.x, sm);
    }
}

template <int NDOT, bool OFFD>
static void launch_spmv_rows_var(const SpmvArgs &a, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    dim3 g(spmv_grid(a.nlist)), b(kBlock);
    const int mode = red_mode(a.red, a.fin, NDOT > 0);
    constexpr int HV = NDOT > 0 ? RED_TICKET_HEAVY : RED_TICKET;
    const bool c16 = a.diag_col16 != nullptr, nt = a.nt != 0;
#define ROWS_GO(MD)                                                                                        \
    do {                                                                                                   \
        if (c16) { if (nt) launch_timed(k_spmv_rows<NDOT, OFFD, true, true, MD>, g, b, st, e0, e1, a);       \
                   else launch_timed(k_spmv_rows<NDOT, OFFD, false, true, MD>, g, b, st, e0, e1, a); }      \
        else { if (nt) launch_timed(k_spmv_rows<NDOT, OFFD, true, false, MD>, g, b, st, e0, e1, a);          \
               else launch_timed(k_spmv_rows<NDOT, OFFD, false, false, MD>, g, b, st, e0, e1, a); }         \
    } while (0)
    if (mode == RED_WAVE) ROWS_GO(RED_WAVE);
    else if (mode == RED_TICKET_HEAVY) ROWS_GO(HV);
    else ROWS_GO(RED_TICKET);
#undef ROWS_GO
}

static bool launch_spmv_rows(const SpmvArgs &a, int ndot, bool with_offd, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    if (with_offd) {
        if (ndot == 0) launch_spmv_rows_var<0, true>(a, st, e0, e1); else if (ndot == 1) launch_spmv_rows_var<1, true>(a, st, e0, e1);
        else if (ndot == 2) launch_spmv_rows_var<2, true>(a, st, e0, e1); else launch_spmv_rows_var<3, true>(a, st, e0, e1);
    } else {
        if (ndot == 0) launch_spmv_rows_var<0, false>(a, st, e0, e1); else if (ndot == 1) launch_spmv_rows_var<1, false>(a, st, e0, e1);
        else if (ndot == 2) launch_spmv_rows_var<2, false>(a, st, e0, e1); else launch_spmv_rows_var<3, false>(a, st, e0, e1);
    }
    return true;
}

unsigned g_product_kernels = 0;

bool launch_spmv(const SpmvArgs &a, int ndot, bool with_offd, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    if (a.nlist == 0) return false;
    g_product_kernels |= a.rowsplit ? PK_ROWS : PK_CSR;
    if (a.rowsplit) return launch_spmv_rows(a, ndot, with_offd, st, e0, e1);
    if (with_offd) {
        if (ndot == 0) launch_spmv_var<0, true>(a, st, e0, e1); else if (ndot == 1) launch_spmv_var<1, true>(a, st, e0, e1);
        else if (ndot == 2) launch_spmv_var<2, true>(a, st, e0, e1); else launch_spmv_var<3, true>(a, st, e0, e1);
    } else {
        if (ndot == 0) launch_spmv_var<0, false>(a, st, e0, e1); else if (ndot == 1) launch_spmv_var<1, false>(a, st, e0, e1);
        else if (ndot == 2) launch_spmv_var<2, false>(a, st, e0, e1); else launch_spmv_var<3, false>(a, st, e0, e1);
    }
    return true;
}

void preload_csr_kernels() { preload_kernel(k_spmv<0, false, false, RED_TICKET>); }

}  // namespace bicg
