// bicg_multi.hip -- the element-wise phases and the scalar finish of multi-RHS plain BiCGStab (bicg_solve_multi, bicg_multi.cpp):
// up to kSpmmCols independent recurrences of reference src/solver.c:74-120 that share the two products of an iteration.
//
//   k_multi_vec<PH>     grid (multi_grid(n), columns): blockIdx.y is the column. Its scalars and its active flag are
//                       workgroup-uniform; the workgroups of a frozen column return before their first vector load, so a frozen
//                       column costs nothing outside the SpMM. The streaming shape of bicg_vec.hip's tiled k_vec: one contiguous
//                       tile of kVecTile pairs per thread, 16-byte accesses, every load of the tile in flight before the first
//                       store; x, touched once per iteration, with non-temporal accesses. Dots: wavefront -> LDS -> ONE partial
//                       per (column, workgroup), a plain store. The grid depends on n only: so does the order of every sum.
//   k_multi_finish<PH>  one workgroup per column: thread t adds the column's partials t, t + 256, ... in index order, the 256
//                       sums are folded by a fixed tree in LDS, thread 0 applies the recurrence to the column's scalars.
//                       No atomics, no tickets: the order of a column's sums depends neither on the number of columns nor on
//                       the column's place in the set.
//   k_multi_sum<PH>, k_multi_apply<PH>  the finish across ranks, split around one all-reduce that acts as an all-gather (below).
//
// Methods 4 and 5 (right-preconditioned) run the same kernels with four more phases: no launch added for the
// diagonal, whose hat vectors are written by the pass that produces p or q.
//
// Compiled with -ffp-contract=off like every unit: each daxpy / dscal of the reference stays a rounding of its own.
#include "bicg_device.h"
#include "bicg_devfn.h"
#include "bicg_launch.h"

namespace bicg {

constexpr int kMultiTile = 4;      // = bicg_vec.hip's kVecTile: 16 KiB of every stream per workgroup

namespace {
struct pr { double a, b; };
__device__ __forceinline__ pr ldp(const double *p, uint32_t i)
{
    const f64x2 t = *reinterpret_cast<const f64x2 *>(p + i);
    return {t.x, t.y};
}
__device__ __forceinline__ pr ldp_nt(const double *p, uint32_t i)
{
    const f64x2 t = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(p + i));
    return {t.x, t.y};
}
__device__ __forceinline__ void stp(double *p, uint32_t i, pr v)
{
    f64x2 t; t.x = v.a; t.y = v.b;
    *reinterpret_cast<f64x2 *>(p + i) = t;
}
__device__ __forceinline__ void stp_nt(double *p, uint32_t i, pr v)
{
    f64x2 t; t.x = v.a; t.y = v.b;
    __builtin_nontemporal_store(t, reinterpret_cast<f64x2 *>(p + i));
}
// y + a x: my_daxpy's rounding per element (src/vector.c), the product and the sum rounded separately
__device__ __forceinline__ double axpy(double y, double a, double x) { return y + a * x; }
__device__ __forceinline__ pr axpy(pr y, double a, pr x) { return {y.a + a * x.a, y.b + a * x.b}; }
__device__ __forceinline__ pr scal(double a, pr x) { return {a * x.a, a * x.b}; }
__device__ __forceinline__ double dot2(pr x, pr y) { return x.a * y.a + x.b * y.b; }

// MV_*_D / MV_XR_H: the right-preconditioned forms (methods 4 and 5) of the phase they are named after -- what FInitDiag, FDiagQ,
// FDiagXR and FDiagP (bicg_vec.hip) do for one vector. _D: the pass also writes the hat vector of what it produces, dinv o (p or q),
// dinv ONE plane for every column (no column offset); MV_XR_H, for either preconditioner: x takes alpha p^ + omega q^.
enum MultiVecPhase { MV_INIT = 0, MV_DOT_RS = 1, MV_Q = 2, MV_DOT_QY = 3, MV_XR = 4, MV_P = 5, MV_INIT_D = 6, MV_Q_D = 7, MV_XR_H = 8, MV_P_D = 9 };
template <int PH> struct mv_dots {
    static constexpr int value = (PH == MV_INIT || PH == MV_DOT_RS || PH == MV_INIT_D) ? 1 : (PH == MV_DOT_QY || PH == MV_XR || PH == MV_XR_H) ? 2 : 0;
};

// One element (T = double: the odd tail) or one 16-byte pair (T = pr) of phase PH: the loads of `In`, then the arithmetic.
template <int PH, class T> struct In { T a, b, c, d, e, f; };

template <int PH> __device__ __forceinline__ In<PH, pr> fetch(const MultiVecs &v, size_t o, uint32_t i)
{
    In<PH, pr> in{};
    if constexpr (PH == MV_INIT)   { in.a = ldp(v.r + o, i); in.b = ldp(v.s + o, i); }
    if constexpr (PH == MV_DOT_RS) { in.a = ldp(v.rh + o, i); in.b = ldp(v.s + o, i); }
    if constexpr (PH == MV_Q)      { in.a = ldp(v.r + o, i); in.b = ldp(v.s + o, i); }
    if constexpr (PH == MV_DOT_QY) { in.a = ldp(v.r + o, i); in.b = ldp(v.y + o, i); }
    if constexpr (PH == MV_XR)     { in.a = ldp(v.r + o, i); in.b = ldp_nt(v.x + o, i); in.c = ldp(v.p + o, i); in.d = ldp(v.y + o, i); in.e = ldp(v.rh + o, i); }
    if constexpr (PH == MV_P)      { in.a = ldp(v.p + o, i); in.b = ldp(v.r + o, i); in.c = ldp(v.s + o, i); }
    if constexpr (PH == MV_INIT_D) { in.a = ldp(v.r + o, i); in.b = ldp(v.s + o, i); in.c = ldp(v.dinv, i); }
    if constexpr (PH == MV_Q_D)    { in.a = ldp(v.r + o, i); in.b = ldp(v.s + o, i); in.c = ldp(v.dinv, i); }
    if constexpr (PH == MV_XR_H)   { in.a = ldp(v.r + o, i); in.b = ldp_nt(v.x + o, i); in.c = ldp(v.ph + o, i); in.d = ldp(v.y + o, i); in.e = ldp(v.rh + o, i); in.f = ldp(v.qh + o, i); }
    if constexpr (PH == MV_P_D)    { in.a = ldp(v.p + o, i); in.b = ldp(v.r + o, i); in.c = ldp(v.s + o, i); in.d = ldp(v.dinv, i); }
    return in;
}
template <int PH> __device__ __forceinline__ In<PH, double> fetch1(const MultiVecs &v, size_t o, uint32_t i)
{
    In<PH, double> in{};
    if constexpr (PH == MV_INIT)   { in.a = v.r[o + i]; in.b = v.s[o + i]; }
    if constexpr (PH == MV_DOT_RS) { in.a = v.rh[o + i]; in.b = v.s[o + i]; }
    if constexpr (PH == MV_Q)      { in.a = v.r[o + i]; in.b = v.s[o + i]; }
    if constexpr (PH == MV_DOT_QY) { in.a = v.r[o + i]; in.b = v.y[o + i]; }
    if constexpr (PH == MV_XR)     { in.a = v.r[o + i]; in.b = v.x[o + i]; in.c = v.p[o + i]; in.d = v.y[o + i]; in.e = v.rh[o + i]; }
    if constexpr (PH == MV_P)      { in.a = v.p[o + i]; in.b = v.r[o + i]; in.c = v.s[o + i]; }
    if constexpr (PH == MV_INIT_D) { in.a = v.r[o + i]; in.b = v.s[o + i]; in.c = v.dinv[i]; }
    if constexpr (PH == MV_Q_D)    { in.a = v.r[o + i]; in.b = v.s[o + i]; in.c = v.dinv[i]; }
    if constexpr (PH == MV_XR_H)   { in.a = v.r[o + i]; in.b = v.x[o + i]; in.c = v.ph[o + i]; in.d = v.y[o + i]; in.e = v.rh[o + i]; in.f = v.qh[o + i]; }
    if constexpr (PH == MV_P_D)    { in.a = v.p[o + i]; in.b = v.r[o + i]; in.c = v.s[o + i]; in.d = v.dinv[i]; }
    return in;
}
__device__ __forceinline__ double dotT(double x, double y) { return x * y; }
__device__ __forceinline__ double dotT(pr x, pr y) { return dot2(x, y); }
__device__ __forceinline__ double scal(double a, double x) { return a * x; }
__device__ __forceinline__ double had(double d, double x) { return d * x; }                     // dinv o x: one rounding per entry
__device__ __forceinline__ pr had(pr d, pr x) { return {d.a * x.a, d.b * x.b}; }
__device__ __forceinline__ void put(double *p, size_t o, uint32_t i, double v) { p[o + i] = v; }
__device__ __forceinline__ void put(double *p, size_t o, uint32_t i, pr v) { stp(p + o, i, v); }
__device__ __forceinline__ void put_nt(double *p, size_t o, uint32_t i, double v) { __builtin_nontemporal_store(v, p + o + i); }
__device__ __forceinline__ void put_nt(double *p, size_t o, uint32_t i, pr v) { stp_nt(p + o, i, v); }

// the scalars of a column a phase uses
struct Coef { double alpha, omega, beta, c; };

template <int PH, class T>
__device__ __forceinline__ void compute(const MultiVecs &v, size_t o, uint32_t i, const In<PH, T> &in, const Coef &k, double *acc)
{
    if constexpr (PH == MV_INIT) {             // r = b - A x ; r# = r ; p = r ; (r,r)                  (src/solver.c:75-78)
        const T rr = axpy(in.a, -1.0, in.b);
        put(v.r, o, i, rr); put(v.rh, o, i, rr); put(v.p, o, i, rr);
        acc[0] += dotT(rr, rr);
    }
    if constexpr (PH == MV_DOT_RS) acc[0] += dotT(in.a, in.b);                                           // (:89)
    if constexpr (PH == MV_Q) put(v.r, o, i, axpy(in.a, -k.alpha, in.b));                                 // (:94)
    if constexpr (PH == MV_DOT_QY) { acc[0] += dotT(in.a, in.b); acc[1] += dotT(in.b, in.b); }           // (:97, 99)
    if constexpr (PH == MV_XR) {               // x += alpha p ; x += omega q ; r = q - omega y ; (r,r), (r#,r)   (:105-111)
        T xx = axpy(in.b, k.alpha, in.c);
        xx = axpy(xx, k.omega, in.a);
        put_nt(v.x, o, i, xx);
        const T rr = axpy(in.a, -k.omega, in.d);
        put(v.r, o, i, rr);
        acc[0] += dotT(rr, rr);
        acc[1] += dotT(in.e, rr);
    }
    if constexpr (PH == MV_P) {                // p = beta p ; p += r ; p += (-beta omega) s              (:117-119)
        T pp = scal(k.beta, in.a);
        pp = axpy(pp, 1.0, in.b);
        pp = axpy(pp, k.c, in.c);
        put(v.p, o, i, pp);
    }
    if constexpr (PH == MV_INIT_D) {           // MV_INIT ; p^ = dinv o p
        const T rr = axpy(in.a, -1.0, in.b);
        put(v.r, o, i, rr); put(v.rh, o, i, rr); put(v.p, o, i, rr);
        put(v.ph, o, i, had(in.c, rr));
        acc[0] += dotT(rr, rr);
    }
    if constexpr (PH == MV_Q_D) {              // MV_Q ; q^ = dinv o q
        const T q = axpy(in.a, -k.alpha, in.b);
        put(v.r, o, i, q);
        put(v.qh, o, i, had(in.c, q));
    }
    if constexpr (PH == MV_XR_H) {             // x = (x + alpha p^) + omega q^ ; r, (r,r), (r#,r) as MV_XR
        T xx = axpy(in.b, k.alpha, in.c);
        xx = axpy(xx, k.omega, in.f);
        put_nt(v.x, o, i, xx);
        const T rr = axpy(in.a, -k.omega, in.d);
        put(v.r, o, i, rr);
        acc[0] += dotT(rr, rr);
        acc[1] += dotT(in.e, rr);
    }
    if constexpr (PH == MV_P_D) {              // MV_P ; p^ = dinv o p
        T pp = scal(k.beta, in.a);
        pp = axpy(pp, 1.0, in.b);
        pp = axpy(pp, k.c, in.c);
        put(v.p, o, i, pp);
        put(v.ph, o, i, had(in.d, pp));
    }
}

}  // namespace

template <int PH>
__global__ void __launch_bounds__(kBlock) k_multi_vec(MultiVecs v, const MultiScal *S, double *part)
{
    constexpr int ND = mv_dots<PH>::value;
    const int col = blockIdx.y;
    if (PH != MV_INIT && PH != MV_INIT_D && !S->active[col]) return;      // frozen: workgroup-uniform, before the first vector load
    const size_t o = (size_t)col * v.stride;
    const uint32_t n = v.n, npair = n >> 1;
    const uint32_t t0 = blockIdx.x * (uint32_t)(kBlock * kMultiTile) + threadIdx.x;
    In<PH, pr> in[kMultiTile];
#pragma unroll
    for (int u = 0; u < kMultiTile; ++u) {
        const uint32_t i = t0 + (uint32_t)u * kBlock;
        if (i < npair) in[u] = fetch<PH>(v, o, 2 * i);
    }
    Coef k{};
    if constexpr (PH == MV_Q || PH == MV_Q_D) k.alpha = S->alpha[col];
    if constexpr (PH == MV_XR || PH == MV_XR_H) { k.alpha = S->alpha[col]; k.omega = S->omega[col]; }
    if constexpr (PH == MV_P || PH == MV_P_D) { k.beta = S->beta[col]; k.c = -S->beta[col] * S->omega[col]; }
    double acc[ND > 0 ? ND : 1] = {};
#pragma unroll
    for (int u = 0; u < kMultiTile; ++u) {
        const uint32_t i = t0 + (uint32_t)u * kBlock;
        if (i < npair) compute<PH, pr>(v, o, 2 * i, in[u], k, acc);
    }
    if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) compute<PH, double>(v, o, n - 1, fetch1<PH>(v, o, n - 1), k, acc);
    if constexpr (ND > 0) {
        __shared__ double sm[(kBlock / 64) * ND];
        const int w = threadIdx.x >> 6;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const double s = wave_sum(acc[d]);
            if ((threadIdx.x & 63) == 0) sm[w * ND + d] = s;
        }
        __syncthreads();
        if (threadIdx.x < ND) {
            double s = sm[threadIdx.x];
            for (int ww = 1; ww < kBlock / 64; ++ww) s += sm[ww * ND + threadIdx.x];
            part[((size_t)threadIdx.x * kSpmmCols + col) * gridDim.x + blockIdx.x] = s;
        }
    }
}

// the column's partials of slot d, summed in an order that depends on nwg alone
static __device__ __forceinline__ double column_sum(const double *part, int d, int col, unsigned nwg, double *sm)
{
    const double *p = part + ((size_t)d * kSpmmCols + col) * nwg;
    double s = 0.0;
    for (unsigned i = threadIdx.x; i < nwg; i += kBlock) s += p[i];
    __syncthreads();           // (sm may still be read from the previous slot's sum)
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
        __syncthreads();
    }
    return sm[0];
}

// the recurrence of dot group PH on one column's scalars, given the group's sums (one thread per column)
template <int PH> static __device__ __forceinline__ void multi_recur(MultiScal *S, int col, double d0, double d1)
{
    if constexpr (PH == MP_INIT) {             // (src/solver.c:78-83, 86)
        S->rTr[col] = d0; S->dot_r[col] = d0; S->dot_zero[col] = d0;
        S->rTr_old[col] = 0.0; S->alpha[col] = 0.0; S->omega[col] = 0.0; S->beta[col] = 0.0;
        S->k[col] = 0; S->breakdown[col] = 0;
        S->active[col] = (d0 > S->tol2 * d0 && 0 < S->max_iter) ? 1 : 0;
    }
    if constexpr (PH == MP_ALPHA) S->alpha[col] = S->rTr[col] / d0;      // (:93)
    if constexpr (PH == MP_OMEGA) S->omega[col] = d0 / d1;               // (:104)
    if constexpr (PH == MP_END) {              // (:108-116, 120, 86)
        const double alpha = S->alpha[col], omega = S->omega[col];
        const double rTr_old = S->rTr[col];
        const double beta = (alpha / omega) * (d1 / rTr_old);
        S->dot_r[col] = d0; S->rTr_old[col] = rTr_old; S->rTr[col] = d1; S->beta[col] = beta;
        const int k = S->k[col] + 1;
        S->k[col] = k;
        if (S->trace && k <= S->trace_cap) {
            double *t = S->trace + (size_t)col * S->trace_cap + (k - 1);
            const size_t q = (size_t)kSpmmCols * S->trace_cap;
            t[0] = alpha; t[q] = omega; t[2 * q] = beta; t[3 * q] = d0;
        }
        if (!(d0 > S->tol2 * S->dot_zero[col] && k < S->max_iter)) S->active[col] = 0;
        if (!(isfinite(alpha) && isfinite(beta) && isfinite(omega) && isfinite(d0)) && !S->breakdown[col]) S->breakdown[col] = k;
    }
}

template <int PH>
__global__ void __launch_bounds__(kBlock) k_multi_finish(MultiScal *S, const double *part, unsigned nwg)
{
    __shared__ double sm[kBlock];
    const int col = blockIdx.x;
    if (PH != MP_INIT && !S->active[col]) return;
    const double d0 = column_sum(part, 0, col, nwg, sm);
    double d1 = 0.0;
    if constexpr (PH == MP_OMEGA || PH == MP_END) d1 = column_sum(part, 1, col, nwg, sm);
    if (threadIdx.x != 0) return;
    multi_recur<PH>(S, col, d0, d1);
}

// Across ranks (bicg_solve_multi with nranks > 1) the finish is three steps: k_multi_sum, ONE all-reduce of red, k_multi_apply.
// red[nranks][2][kSpmmCols]: k_multi_sum fills this rank's row with the local sums of all kSpmmCols columns (0.0 for a frozen or
// unused column) and zeroes every other row, so the all-reduce adds each value to zeros only -- x + 0.0 is exact: it GATHERS every
// rank's local sums, the same bytes on every rank whatever order the transport adds in.
template <int PH>
__global__ void __launch_bounds__(kBlock) k_multi_sum(const MultiScal *S, const double *part, unsigned nwg, int nv, double *red,
                                                      int nranks, int rank)
{
    __shared__ double sm[kBlock];
    const int col = blockIdx.x;                // grid: kSpmmCols workgroups, whatever nv is
    const bool live = col < nv && (PH == MP_INIT || S->active[col]);      // workgroup-uniform
    double d0 = 0.0, d1 = 0.0;
    if (live) {
        d0 = column_sum(part, 0, col, nwg, sm);
        if constexpr (PH == MP_OMEGA || PH == MP_END) d1 = column_sum(part, 1, col, nwg, sm);
    }
    for (int t = threadIdx.x; t < 2 * nranks; t += kBlock) {
        const int p = t >> 1, d = t & 1;
        red[((size_t)p * 2 + d) * kSpmmCols + col] = p == rank ? (d ? d1 : d0) : 0.0;
    }
}

// one thread per column: the ranks' local sums added in a fixed order, then the recurrence of k_multi_finish<PH>. The order is
// rank_tree_sum's (bicg_devfn.h), the association of a recursive-doubling all-reduce ((s0 + s1) + (s2 + s3)) + ... -- ascending
// rank order up to three ranks --: what the library's other sums over ranks use and what the reference's MPI_Iallreduce computes
// under MPICH (oracle/bicg_oracle.c, orc_dist_dot), so that with one row per rank a column follows the reference bit for bit.
// In place in red: k_multi_sum rewrites every entry before the next all-reduce.
template <int PH>
__global__ void __launch_bounds__(64) k_multi_apply(MultiScal *S, double *red, int nv, int nranks)
{
    const int col = threadIdx.x;
    if (col >= nv) return;
    if (PH != MP_INIT && !S->active[col]) return;
    constexpr int row = 2 * kSpmmCols;
    double *v0 = red + col, *v1 = red + kSpmmCols + col;
    for (int stride = 1; stride < nranks; stride <<= 1)
        for (int i = 0; i + stride < nranks; i += 2 * stride) {
            v0[(size_t)i * row] += v0[(size_t)(i + stride) * row];
            v1[(size_t)i * row] += v1[(size_t)(i + stride) * row];
        }
    multi_recur<PH>(S, col, v0[0], v1[0]);
}

template <int PH> static void run_multi(const MultiVecs &v, int nv, MultiScal *S, double *part, hipStream_t st)
{
    BICG_LAUNCH((k_multi_vec<PH>), dim3(multi_grid(v.n), (unsigned)nv), dim3(kBlock), 0, st, v, S, part);
}

// workgroups per column: one tile of kBlock * kMultiTile pairs each, a function of n alone
unsigned multi_grid(uint32_t n)
{
    const uint32_t tile = (uint32_t)(kBlock * kMultiTile);
    const uint32_t g = ((n >> 1) + tile - 1) / tile;
    return g ? g : 1u;
}

void launch_multi_init(const MultiVecs &v, int nv, MultiScal *S, double *part, hipStream_t st) { run_multi<MV_INIT>(v, nv, S, part, st); }
void launch_multi_dot_rs(const MultiVecs &v, int nv, MultiScal *S, double *part, hipStream_t st) { run_multi<MV_DOT_RS>(v, nv, S, part, st); }
void launch_multi_q(const MultiVecs &v, int nv, MultiScal *S, hipStream_t st) { run_multi<MV_Q>(v, nv, S, nullptr, st); }
void launch_multi_dot_qy(const MultiVecs &v, int nv, MultiScal *S, double *part, hipStream_t st) { run_multi<MV_DOT_QY>(v, nv, S, part, st); }
void launch_multi_xr(const MultiVecs &v, int nv, MultiScal *S, double *part, hipStream_t st) { run_multi<MV_XR>(v, nv, S, part, st); }
void launch_multi_p(const MultiVecs &v, int nv, MultiScal *S, hipStream_t st) { run_multi<MV_P>(v, nv, S, nullptr, st); }
void launch_multi_init_diag(const MultiVecs &v, int nv, MultiScal *S, double *part, hipStream_t st) { run_multi<MV_INIT_D>(v, nv, S, part, st); }
void launch_multi_q_diag(const MultiVecs &v, int nv, MultiScal *S, hipStream_t st) { run_multi<MV_Q_D>(v, nv, S, nullptr, st); }
void launch_multi_xr_hat(const MultiVecs &v, int nv, MultiScal *S, double *part, hipStream_t st) { run_multi<MV_XR_H>(v, nv, S, part, st); }
void launch_multi_p_diag(const MultiVecs &v, int nv, MultiScal *S, hipStream_t st) { run_multi<MV_P_D>(v, nv, S, nullptr, st); }

void launch_multi_finish(int phase, int nv, MultiScal *S, const double *part, unsigned nwg, hipStream_t st)
{
    const dim3 g((unsigned)nv), b(kBlock);
    switch (phase) {
    case MP_INIT:  BICG_LAUNCH((k_multi_finish<MP_INIT>), g, b, 0, st, S, part, nwg); break;
    case MP_ALPHA: BICG_LAUNCH((k_multi_finish<MP_ALPHA>), g, b, 0, st, S, part, nwg); break;
    case MP_OMEGA: BICG_LAUNCH((k_multi_finish<MP_OMEGA>), g, b, 0, st, S, part, nwg); break;
    default:       BICG_LAUNCH((k_multi_finish<MP_END>), g, b, 0, st, S, part, nwg); break;
    }
}

void launch_multi_sum(int phase, int nv, const MultiScal *S, const double *part, unsigned nwg, double *red, int nranks, int rank, hipStream_t st)
{
    const dim3 g((unsigned)kSpmmCols), b(kBlock);
    switch (phase) {
    case MP_INIT:  BICG_LAUNCH((k_multi_sum<MP_INIT>), g, b, 0, st, S, part, nwg, nv, red, nranks, rank); break;
    case MP_ALPHA: BICG_LAUNCH((k_multi_sum<MP_ALPHA>), g, b, 0, st, S, part, nwg, nv, red, nranks, rank); break;
    case MP_OMEGA: BICG_LAUNCH((k_multi_sum<MP_OMEGA>), g, b, 0, st, S, part, nwg, nv, red, nranks, rank); break;
    default:       BICG_LAUNCH((k_multi_sum<MP_END>), g, b, 0, st, S, part, nwg, nv, red, nranks, rank); break;
    }
}

void launch_multi_apply(int phase, int nv, MultiScal *S, double *red, int nranks, hipStream_t st)
{
    const dim3 g(1), b(64);
    switch (phase) {
    case MP_INIT:  BICG_LAUNCH((k_multi_apply<MP_INIT>), g, b, 0, st, S, red, nv, nranks); break;
    case MP_ALPHA: BICG_LAUNCH((k_multi_apply<MP_ALPHA>), g, b, 0, st, S, red, nv, nranks); break;
    case MP_OMEGA: BICG_LAUNCH((k_multi_apply<MP_OMEGA>), g, b, 0, st, S, red, nv, nranks); break;
    default:       BICG_LAUNCH((k_multi_apply<MP_END>), g, b, 0, st, S, red, nv, nranks); break;
    }
}

}  // namespace bicg
