// bicg_vec.hip -- the fused element-wise phases of the solvers and the stand-alone finisher of their dot groups (k_finish).
//
//   k_vec<...>    fused element-wise phases of the four iterations (replace the my_daxpy /
//                 my_dscal / my_dcopy / my_ddot call sequences of reference src/solver.c).
//   reductions    __shfl_down over the 64-lane wavefront -> LDS across the 4 wavefronts -> one
//                 partial per workgroup -> the LAST workgroup to arrive sums the partials in a
//                 fixed order (deterministic) and applies the scalar recurrence on the device (bicg_reduce.h).
//
// Compiled with -ffp-contract=off: every a*b+c keeps the two roundings of the reference's scalar
// loops, so the element-wise phases and every SpMV row are bit-identical to the CPU oracle; only
// the association of the dot-product sums differs.
// k_vec, run_vec and the pair types: bicg_vec.h (shared with bicg_stab2.hip).
#include "bicg_vec.h"

namespace bicg {

// stand-alone finisher (set-up phases, host reads, transports whose all-reduce the host enqueues)
__global__ void __launch_bounds__(kBlock) k_finish(Scal *S, Finish f)
{
    __shared__ FinishLds L;
    (void)finish_group(S, f, f.roles, blockIdx.x, gridDim.x, L, nullptr);
}

void launch_finish(const Launch &L)
{
    BICG_LAUNCH(k_finish, dim3(L.fin.roles & FIN_SHARDS ? kShards : 1), dim3(kBlock), 0, L.st, L.S, L.fin);
}

static unsigned g_vec_grid_cap = 0;
void set_vec_grid_cap(unsigned cap) { g_vec_grid_cap = cap; }
// pairs per thread of an element-wise launch over n rows (0: grid-stride loop over <= kMaxGrid workgroups)
static unsigned vec_ppt(uint32_t n)
{
    static const int ppt_env = [] { const char *v = knob_x("BICG_VEC_PPT"); return v ? atoi(v) : -1; }();
    // (tiles from 2^24 rows = 128 MiB per vector: 256^3 plain 0.512 -> 0.442, CA 0.662 -> 0.573 ms per iteration; at 6.4 M rows --
    // 49 MiB per vector, what one kernel writes the next still finds in the Infinity Cache -- plain loses 3.6 %, pipelined gains 1.7 %;
    // at Transport size plain loses 7 %: profiles/r05/ab_vec_tile_sizes.txt)
    return ppt_env >= 0 ? (unsigned)ppt_env : (n >= (1u << 24) ? (unsigned)kVecTile : 0u);
}
// ... as contiguous tiles with non-temporal accesses (k_vec<.., TILE>; BICG_VEC_TILE=0: the strided form of round 4)
bool vec_tiled(uint32_t n)
{
    static const bool on = env_on_x("BICG_VEC_TILE", true);
    return on && !g_vec_grid_cap && vec_ppt(n) == (unsigned)kVecTile;
}
unsigned vec_grid(uint32_t n)
{
    // 256 CUs x 8 resident workgroups, grid-stride beyond (BICG_VEC_GRID: measurement knob, <= kMaxGrid)
    static const unsigned env_cap = [] {
        const char *v = knob_x("BICG_VEC_GRID");
        const int g = v ? atoi(v) : kMaxGrid;
        return (unsigned)(g >= 1 && g <= kMaxGrid ? g : kMaxGrid);
    }();
    // Vectors far beyond the caches (>= 16.8 M rows): one workgroup per tile of 4 element pairs per thread (16 KiB per stream)
    // instead of <= 2048 persistent workgroups striding through the vectors -- short workgroups stream faster (STREAM read:
    // +12 %, profiles/NOTES.md; 512^3 Laplacian: plain 9.12 -> 8.65 ms, CA 10.86 -> 10.10 ms per iteration, round 4). At
    // 16.8 M rows (256^3) and at Transport size the two forms tie. BICG_VEC_PPT=p forces p pairs per thread everywhere
    // (0: never); the grid is capped at the partial-sum slots every context has.
    unsigned g = ((n >> 1) + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    const unsigned ppt = vec_ppt(n);
    if (ppt && !g_vec_grid_cap) {
        g = (g + ppt - 1) / ppt;
        const unsigned slots = std::max<unsigned>(kMaxGrid, (n + kGroupRows - 1) / kGroupRows);      // ctx_state: nslots >= row groups
        return g < slots ? g : slots;
    }
    const unsigned cap = g_vec_grid_cap && g_vec_grid_cap < env_cap ? g_vec_grid_cap : env_cap;
    if (g > cap) g = cap;
    return g;
}

// ---- init: r = b - Ax ; r# = r ; [p = r] ; [bsave = b] ; (r,r)     (src/solver.c:74-78, 475-479)
struct FInit {
    static constexpr int ND = 1;
    static constexpr int kModes = kAnyMode;
    double *r, *rh, *p, *bs; const double *ax;
    __device__ void load(const Scal *) {}
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        T b = ld<T>(r, i);
        if (bs) st(bs, i, b);
        T rr = b + (-1.0) * ld<T>(ax, i);
        st(r, i, rr); st(rh, i, rr);
        if (p) st(p, i, rr);
        acc[0] += hsum(rr * rr);
    }
};
void launch_init_residual(const Vecs &v, bool copy_p, bool save_b, const Launch &L, Reduce red)
{
    run_vec(FInit{v.r, v.rh, copy_p ? v.p : nullptr, save_b ? v.b : nullptr, v.ax}, v.n, L, red);
}

// ---- plain: q = r - alpha s (kept in r)                               (src/solver.c:94)
struct FPlainQ {
    static constexpr int ND = 0;
    static constexpr int kModes = kAnyMode | kHandMode;
    static constexpr int kHandPhase = PH_PLAIN_ALPHA, kHandN = 1;
    static constexpr bool kSplit = true;
    double *r; const double *s; double alpha;
    template <class T> struct In { T r, s; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(r, i), ld<T>(s, i)}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        st(r, i, in.r + (-alpha) * in.s);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_plain_q(const Vecs &v, const Launch &L) { run_vec(FPlainQ{v.r, v.s, 0.0}, v.n, L, Reduce{}); }

// ---- plain: x += alpha p + omega q ; r = q - omega y ; (r,r), (r#,r)   (src/solver.c:105-111)
template <bool XNT> struct FPlainXR {
    static constexpr int ND = 2;
    static constexpr int kModes = kAnyMode | kHandMode;
    static constexpr int kHandPhase = PH_OMEGA, kHandN = 2;
    static constexpr bool kSplit = true;
    double *x, *r; const double *q, *p, *y, *rh; double alpha, omega;      // q: where q lives (r itself, or the fused iteration's own buffer)
    template <class T> struct In { T q, x, p, y, rh; };
    __device__ void load(const Scal *S) { alpha = S->alpha; omega = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {ld<T>(q, i), XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(p, i), ld<T>(y, i), ld<T>(rh, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + alpha * in.p;
        xx = xx + omega * in.q;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T rr = in.q + (-omega) * in.y;
        st(r, i, rr);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(in.rh * rr);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_plain_xr(const Vecs &v, const Launch &L, Reduce red, const double *q)
{
    if (stream_x()) run_vec(FPlainXR<true>{v.x, v.r, q ? q : v.r, v.p, v.y, v.rh, 0.0, 0.0}, v.n, L, red);
    else run_vec(FPlainXR<false>{v.x, v.r, q ? q : v.r, v.p, v.y, v.rh, 0.0, 0.0}, v.n, L, red);
}

// ---- plain: p = beta p ; p += r ; p += (-beta*omega) s                (src/solver.c:117-119)
struct FPlainP {
    static constexpr int ND = 0;
    static constexpr int kModes = kAnyMode | kHandMode;
    static constexpr int kHandPhase = PH_PLAIN_END, kHandN = 2;
    static constexpr bool kSplit = true;
    double *p; const double *r, *s; double beta, c;
    template <class T> struct In { T p, r, s; };
    __device__ void load(const Scal *S) { beta = S->beta; c = -S->beta * S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(p, i), ld<T>(r, i), ld<T>(s, i)}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T pp = beta * in.p;
        pp = pp + 1.0 * in.r;
        pp = pp + c * in.s;
        st(p, i, pp);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_plain_p(const Vecs &v, const Launch &L) { run_vec(FPlainP{v.p, v.r, v.s, 0.0, 0.0}, v.n, L, Reduce{}); }

// ---- diagonally (right-) preconditioned plain BiCGStab, M = diag(d), dinv = 1 / d: the three phases
// above with the hat vectors p^ = dinv o p and q^ = dinv o q -- the inputs of the two products -- written by the pass that
// produces p or q. One rounding per hat entry; with dinv = 1 every phase computes what its plain counterpart computes.
// init: r = b - Ax ; r# = r ; p = r ; p^ = dinv o p ; (r,r)
struct FInitDiag {
    static constexpr int ND = 1;
    static constexpr int kModes = kAnyMode;
    double *r, *rh, *p, *ph; const double *ax, *dinv;
    __device__ void load(const Scal *) {}
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        T rr = ld<T>(r, i) + (-1.0) * ld<T>(ax, i);
        st(r, i, rr); st(rh, i, rr); st(p, i, rr);
        st(ph, i, ld<T>(dinv, i) * rr);
        acc[0] += hsum(rr * rr);
    }
};
void launch_init_residual_diag(const Vecs &v, const double *dinv, const Launch &L, Reduce red)
{
    run_vec(FInitDiag{v.r, v.rh, v.p, v.z, v.ax, dinv}, v.n, L, red);
}

// q = r - alpha s (kept in r) ; q^ = dinv o q
struct FDiagQ {
    static constexpr int ND = 0;
    static constexpr int kModes = kAnyMode;
    static constexpr bool kSplit = true;
    double *r, *qh; const double *s, *dinv; double alpha;
    template <class T> struct In { T r, s, d; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(r, i), ld<T>(s, i), ld<T>(dinv, i)}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T q = in.r + (-alpha) * in.s;
        st(r, i, q);
        st(qh, i, in.d * q);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_diag_q(const Vecs &v, const double *dinv, const Launch &L) { run_vec(FDiagQ{v.r, v.w, v.s, dinv, 0.0}, v.n, L, Reduce{}); }

// x += alpha p^ + omega q^ ; r = q - omega y ; (r,r), (r#,r)
template <bool XNT> struct FDiagXR {
    static constexpr int ND = 2;
    static constexpr int kModes = kAnyMode;
    static constexpr bool kSplit = true;
    double *x, *r; const double *ph, *qh, *y, *rh; double alpha, omega;
    template <class T> struct In { T q, x, ph, qh, y, rh; };
    __device__ void load(const Scal *S) { alpha = S->alpha; omega = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {ld<T>(r, i), XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(ph, i), ld<T>(qh, i), ld<T>(y, i), ld<T>(rh, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + alpha * in.ph;
        xx = xx + omega * in.qh;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T rr = in.q + (-omega) * in.y;
        st(r, i, rr);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(in.rh * rr);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_diag_xr(const Vecs &v, const Launch &L, Reduce red)
{
    if (stream_x()) run_vec(FDiagXR<true>{v.x, v.r, v.z, v.w, v.y, v.rh, 0.0, 0.0}, v.n, L, red);
    else run_vec(FDiagXR<false>{v.x, v.r, v.z, v.w, v.y, v.rh, 0.0, 0.0}, v.n, L, red);
}

// p = beta p ; p += r ; p += (-beta omega) s ; p^ = dinv o p
struct FDiagP {
    static constexpr int ND = 0;
    static constexpr int kModes = kAnyMode;
    static constexpr bool kSplit = true;
    double *p, *ph; const double *r, *s, *dinv; double beta, c;
    template <class T> struct In { T p, r, s, d; };
    __device__ void load(const Scal *S) { beta = S->beta; c = -S->beta * S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(p, i), ld<T>(r, i), ld<T>(s, i), ld<T>(dinv, i)}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T pp = beta * in.p;
        pp = pp + 1.0 * in.r;
        pp = pp + c * in.s;
        st(p, i, pp);
        st(ph, i, in.d * pp);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_diag_p(const Vecs &v, const double *dinv, const Launch &L) { run_vec(FDiagP{v.p, v.z, v.r, v.s, dinv, 0.0, 0.0}, v.n, L, Reduce{}); }

// ---- CA: p = r + beta(p - omega s) ; s = w + beta(s - omega z)         (src/solver.c:217-222)
struct FCaPS {
    static constexpr int ND = 0;
    static constexpr int kModes = kAnyMode;
    static constexpr bool kSplit = true;
    double *p, *s; const double *r, *z, *w; double beta, omega;
    template <class T> struct In { T p, s, r, z, w; };
    __device__ void load(const Scal *S) { beta = S->beta; omega = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {ld<T>(p, i), ld<T>(s, i), ld<T>(r, i), ld<T>(z, i), ld<T>(w, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        st(p, i, recur3<T>(in.p, in.s, in.r, omega, beta));
        st(s, i, recur3<T>(in.s, in.z, in.w, omega, beta));
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_ca_ps(const Vecs &v, const Launch &L) { run_vec(FCaPS{v.p, v.s, v.r, v.z, v.w, 0.0, 0.0}, v.n, L, Reduce{}); }

// ---- q = r - alpha s (in r) ; y = w - alpha z (in w) ; (q,y), (y,y)    (src/solver.c:225-228, 361-364)
struct FQY {
    static constexpr int ND = 2;
    static constexpr int kModes = kAnyMode;
    static constexpr bool kSplit = true;
    double *r, *w; const double *s, *z; double alpha;
    template <class T> struct In { T r, s, w, z; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(r, i), ld<T>(s, i), ld<T>(w, i), ld<T>(z, i)}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T q = in.r + (-alpha) * in.s;
        T y = in.w + (-alpha) * in.z;
        st(r, i, q); st(w, i, y);
        acc[0] += hsum(q * y);
        acc[1] += hsum(y * y);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_qy(const Vecs &v, const Launch &L, Reduce red) { run_vec(FQY{v.r, v.w, v.s, v.z, 0.0}, v.n, L, red); }

// ---- CA: x += alpha p + omega q ; r = q - omega y ; (r,r), (r#,r), [slot 2 left for (r#,w)], (r#,s), (r#,z)
//      (src/solver.c:233-236, 240, 242-243; (r#,w) comes from the following SpMV's epilogue)
template <bool XNT> struct FCaXR {
    static constexpr int ND = 5;
    static constexpr int kModes = kAnyMode;
    static constexpr bool kSplit = true;
    double *x, *r; const double *p, *w, *rh, *s, *z; double alpha, omega;
    template <class T> struct In { T q, x, p, w, rh, s, z; };
    __device__ void load(const Scal *S) { alpha = S->alpha; omega = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {ld<T>(r, i), XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(p, i), ld<T>(w, i), ld<T>(rh, i), ld<T>(s, i), ld<T>(z, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + alpha * in.p;
        xx = xx + omega * in.q;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T rr = in.q + (-omega) * in.w;
        st(r, i, rr);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(in.rh * rr);
        acc[3] += hsum(in.rh * in.s);
        acc[4] += hsum(in.rh * in.z);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_ca_xr(const Vecs &v, const Launch &L, Reduce red)
{
    red.p2p.mask &= ~4u;    // slot 2 belongs to the following SpMV's epilogue
    if (stream_x()) run_vec(FCaXR<true>{v.x, v.r, v.p, v.w, v.rh, v.s, v.z, 0.0, 0.0}, v.n, L, red);
    else run_vec(FCaXR<false>{v.x, v.r, v.p, v.w, v.rh, v.s, v.z, 0.0, 0.0}, v.n, L, red);
}

// ---- pipelined phase 1: p, s, z recurrences ; q, y ; (q,y), (y,y)       (src/solver.c:352-364)
// y = w - alpha z goes to its own vector yb (the reference keeps it in w, :363-364): w is the input of the
// SpMV t = A w in whose epilogue this phase may run (k_spmv_sell_epi), so it cannot be overwritten there
struct FPipe1 {
    static constexpr int ND = 2;
    static constexpr int kModes = kWaveOnly;
    static constexpr bool kSplit = true;
    double *p, *s, *z, *r, *yb; const double *w, *t, *v; double alpha, beta, omega;
    template <class T> struct In { T r, w, s, z, p, v, t; };
    __device__ void load(const Scal *S) { alpha = S->alpha; beta = S->beta; omega = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {ld<T>(r, i), ld<T>(w, i), ld<T>(s, i), ld<T>(z, i), ld<T>(p, i), ld<T>(v, i), ld<T>(t, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        st(p, i, recur3<T>(in.p, in.s, in.r, omega, beta));
        T s1 = recur3<T>(in.s, in.z, in.w, omega, beta);
        T z1 = recur3<T>(in.z, in.v, in.t, omega, beta);
        st(s, i, s1); st(z, i, z1);
        T q = in.r + (-alpha) * s1;
        T y = in.w + (-alpha) * z1;
        st(r, i, q); st(yb, i, y);
        acc[0] += hsum(q * y);
        acc[1] += hsum(y * y);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_pipe_f1(const Vecs &v, const Launch &L, Reduce red)
{
    run_vec(FPipe1{v.p, v.s, v.z, v.r, v.y, v.w, v.t, v.v, 0.0, 0.0, 0.0}, v.n, L, red);
}

// ---- pipelined phase 2: x ; r = q - omega y ; w = y - omega (t - alpha v) ; five dots  (src/solver.c:370-380)
// t - alpha v is not written back: t is overwritten by the next SpMV (src/solver.c:381).
template <bool XNT> struct FPipe2 {
    static constexpr int ND = 5;
    static constexpr int kModes = kWaveOnly;
    static constexpr bool kSplit = true;
    double *x, *r, *w; const double *yb, *p, *t, *v, *rh, *s, *z; double alpha, omega;
    template <class T> struct In { T q, y, x, p, t, v, rh, s, z; };
    __device__ void load(const Scal *S) { alpha = S->alpha; omega = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {ld<T>(r, i), ld<T>(yb, i), XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(p, i), ld<T>(t, i), ld<T>(v, i), ld<T>(rh, i),
                ld<T>(s, i), ld<T>(z, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + alpha * in.p;
        xx = xx + omega * in.q;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T rr = in.q + (-omega) * in.y;
        st(r, i, rr);
        T tt = in.t + (-alpha) * in.v;
        T ww = in.y + (-omega) * tt;
        st(w, i, ww);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(in.rh * rr);
        acc[2] += hsum(in.rh * ww);
        acc[3] += hsum(in.rh * in.s);
        acc[4] += hsum(in.rh * in.z);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_pipe_f2(const Vecs &v, const Launch &L, Reduce red)
{
    if (stream_x()) run_vec(FPipe2<true>{v.x, v.r, v.w, v.y, v.p, v.t, v.v, v.rh, v.s, v.z, 0.0, 0.0}, v.n, L, red);
    else run_vec(FPipe2<false>{v.x, v.r, v.w, v.y, v.p, v.t, v.v, v.rh, v.s, v.z, 0.0, 0.0}, v.n, L, red);
}

// ---- residual replacement pieces
struct FPUpdate {   // p = r + beta (p - omega s)                            (src/solver.c:494-496)
    static constexpr int ND = 0;
    static constexpr int kModes = kWaveOnly;
    double *p; const double *s, *r; double beta, omega;
    __device__ void load(const Scal *S) { beta = S->beta; omega = S->omega; }
    template <class T> __device__ void apply(uint32_t i, double *) const
    {
        st(p, i, recur3<T>(ld<T>(p, i), ld<T>(s, i), ld<T>(r, i), omega, beta));
    }
};
void launch_p_update(const Vecs &v, const Launch &L) { run_vec(FPUpdate{v.p, v.s, v.r, 0.0, 0.0}, v.n, L, Reduce{}); }

struct FXUpdate {   // x += alpha p ; x += omega q                           (src/solver.c:519-520)
    static constexpr int ND = 0;
    static constexpr int kModes = kWaveOnly;
    double *x; const double *p, *r; double alpha, omega;
    __device__ void load(const Scal *S) { alpha = S->alpha; omega = S->omega; }
    template <class T> __device__ void apply(uint32_t i, double *) const
    {
        T xx = ld<T>(x, i) + alpha * ld<T>(p, i);
        st(x, i, xx + omega * ld<T>(r, i));
    }
};
void launch_x_update(const Vecs &v, const Launch &L) { run_vec(FXUpdate{v.x, v.p, v.r, 0.0, 0.0}, v.n, L, Reduce{}); }

struct FTrueRes {   // r = b ; r += -1.0 * Ax                                (src/solver.c:524-525)
    static constexpr int ND = 0;
    static constexpr int kModes = kWaveOnly;
    double *r; const double *b, *ax;
    __device__ void load(const Scal *) {}
    template <class T> __device__ void apply(uint32_t i, double *) const
    {
        st(r, i, ld<T>(b, i) + (-1.0) * ld<T>(ax, i));
    }
};
void launch_true_residual(const Vecs &v, const Launch &L) { run_vec(FTrueRes{v.r, v.b, v.ax}, v.n, L, Reduce{}); }

struct FDots5 {     // (r,r), (r#,r), (r#,w), (r#,s), (r#,z)                 (src/solver.c:533-538)
    static constexpr int ND = 5;
    static constexpr int kModes = kWaveOnly;
    const double *r, *rh, *w, *s, *z;
    __device__ void load(const Scal *) {}
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        T rr = ld<T>(r, i), h = ld<T>(rh, i);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(h * rr);
        acc[2] += hsum(h * ld<T>(w, i));
        acc[3] += hsum(h * ld<T>(s, i));
        acc[4] += hsum(h * ld<T>(z, i));
    }
};
void launch_dots5(const Vecs &v, const Launch &L, Reduce red) { run_vec(FDots5{v.r, v.rh, v.w, v.s, v.z}, v.n, L, red); }

// ---- shifted BiCGStab (reference src/shifted_solver.c:182-354) ---------------------------------
struct FShiftInit {   // r# = r ; p[seed] = r ; (r,r)                                  (:238-250)
    static constexpr int ND = 1;
    const double *r; double *rh, *ps;
    __device__ void load(const Scal *) {}
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        T rr = ld<T>(r, i);
        st(rh, i, rr); st(ps, i, rr);
        acc[0] += hsum(rr * rr);
    }
};
void launch_shift_init(const Vecs &v, double *p_seed, Scal *S, Reduce red, hipStream_t s)
{
    run_vec(FShiftInit{v.r, v.rh, p_seed}, v.n, S, red, s);
}

struct FShiftQ {      // r_old = r ; q = r - alpha[seed] s (kept in r)                  (:269, 275)
    static constexpr int ND = 0;
    double *r, *rold; const double *s; double alpha;
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ void apply(uint32_t i, double *) const
    {
        T r0 = ld<T>(r, i);
        st(rold, i, r0);
        st(r, i, r0 + (-alpha) * ld<T>(s, i));
    }
};
void launch_shift_q(const Vecs &v, Scal *S, hipStream_t s) { run_vec(FShiftQ{v.r, v.ax, v.s, 0.0}, v.n, S, Reduce{}, s); }

// One pass over BOTH vector sets: the seed's x and r, the two dots, and for every other shift j the
// p_j update that the reference does at the top of the iteration (:264-266, with r = r_old), the
// x_j update (:296-297) and the second p_j update (:298-299) -- the same operations on every
// element in the same order, but p_j and x_j are read and written ONCE per iteration
// (32 n bytes per shift instead of the reference's 136 n).
template <bool SNT> struct FShiftUpdate {
    static constexpr int ND = 2;
    double *xs, *r, *pset, *xset; const double *ps, *y, *rh, *rold; const ShiftDev *H; uint32_t stride;
    double alpha, omega; int nsig, seed;
    const double *beta_j, *alpha_j, *cp, *cx, *c1, *c2;
    __device__ void load(const Scal *S)
    {
        alpha = S->alpha; omega = S->omega;
        nsig = H->nsig; seed = H->seed;
        beta_j = H->beta; alpha_j = H->alpha; cp = H->cp; cx = H->cx; c1 = H->c1; c2 = H->c2;
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        const T q = ld<T>(r, i), ro = ld<T>(rold, i);
        T xx = ld<T>(xs, i) + alpha * ld<T>(ps, i);             // x[seed] += alpha p[seed] ; += omega q   (:292-293)
        st(xs, i, xx + omega * q);
        for (int j = 0; j < nsig; ++j) {
            if (j == seed) continue;
            double *pj = pset + (size_t)j * stride, *xj = xset + (size_t)j * stride;
            T p = beta_j[j] * (SNT ? ldnt<T>(pj, i) : ld<T>(pj, i));   // my_dscal(beta[j])                 (:265)
            p = p + cp[j] * ro;                                  // += 1/(pi zeta) r   (r == r_old here)    (:266)
            T x = (SNT ? ldnt<T>(xj, i) : ld<T>(xj, i)) + cx[j] * q;   // (:296)
            x = x + alpha_j[j] * p;                              // (:297)
            if (SNT) stnt(xj, i, x); else st(xj, i, x);
            p = p + c1[j] * q;                                   // (:298)
            p = p + c2[j] * ro;                                  // (:299)
            if (SNT) stnt(pj, i, p); else st(pj, i, p);
        }
        const T rr = q + (-omega) * ld<T>(y, i);                // r = q - omega y                         (:303)
        st(r, i, rr);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(ld<T>(rh, i) * rr);
    }
};
void launch_shift_update(const Vecs &v, double *p_set, double *x_set, uint32_t set_stride, int seed, const ShiftDev *H,
                         Scal *S, Reduce red, hipStream_t s)
{
    auto go = [&](auto f) {
        f.xs = x_set + (size_t)seed * set_stride; f.ps = p_set + (size_t)seed * set_stride;
        f.r = v.r; f.pset = p_set; f.xset = x_set; f.y = v.y; f.rh = v.rh; f.rold = v.ax; f.H = H; f.stride = set_stride;
        run_vec(f, v.n, S, red, s);
    };
    if (stream_sets()) go(FShiftUpdate<true>{}); else go(FShiftUpdate<false>{});
}

// ---- seed-switching shifted solvers (reference src/shifted_switching_solver.c:376-446) -----------
struct FSwQ {         // r_old = r ; q = r - alpha s -> r and q_copy                       (:376, 393-394)
    static constexpr int ND = 0;
    double *r, *rold, *qc; const double *s; double alpha;
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ void apply(uint32_t i, double *) const
    {
        T r0 = ld<T>(r, i);
        st(rold, i, r0);
        T q = r0 + (-alpha) * ld<T>(s, i);
        st(r, i, q); st(qc, i, q);
    }
};
void launch_sw_q(const Vecs &v, double *qcopy, Scal *S, hipStream_t s) { run_vec(FSwQ{v.r, v.ax, qcopy, v.s, 0.0}, v.n, S, Reduce{}, s); }

struct FSwSeed {      // x[seed] += alpha p[seed] ; += omega q ; r = q - omega y ; (r,r), (r#,r)   (:413-418)
    static constexpr int ND = 2;
    double *xs, *r; const double *ps, *y, *rh; double alpha, omega;
    __device__ void load(const Scal *S) { alpha = S->alpha; omega = S->omega; }
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        const T q = ld<T>(r, i);
        T xx = ld<T>(xs, i) + alpha * ld<T>(ps, i);
        st(xs, i, xx + omega * q);
        const T rr = q + (-omega) * ld<T>(y, i);
        st(r, i, rr);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(ld<T>(rh, i) * rr);
    }
};
void launch_sw_seed(const Vecs &v, double *x_seed, const double *p_seed, Scal *S, Reduce red, hipStream_t s)
{
    run_vec(FSwSeed{x_seed, v.r, p_seed, v.y, v.rh, 0.0, 0.0}, v.n, S, red, s);
}

// p[seed] = beta p[seed] + r - beta omega s (:423-425) and, for every shift that is neither the seed
// nor frozen, the six updates of :438-446 in the reference's order; each p_j and x_j is read and
// written once.
template <bool SNT> struct FSwShifts {
    static constexpr int ND = 0;
    double *ps, *pset, *xset; const double *r, *s, *qc, *rold; const ShiftDev *H; uint32_t stride;
    double beta, omega; int nsig;
    const int *skip; const double *beta_j, *alpha_j, *cp, *cx, *c1, *c2;
    __device__ void load(const Scal *S)
    {
        beta = S->beta; omega = S->omega; nsig = H->nsig;
        skip = H->skip; beta_j = H->beta; alpha_j = H->alpha; cp = H->cp; cx = H->cx; c1 = H->c1; c2 = H->c2;
    }
    template <class T> __device__ void apply(uint32_t i, double *) const
    {
        const T rr = ld<T>(r, i), q = ld<T>(qc, i), ro = ld<T>(rold, i);
        T p = beta * ld<T>(ps, i);                               // my_dscal(beta)            (:423)
        p = p + 1.0 * rr;                                        // += 1.0 r                  (:424)
        p = p + (-beta * omega) * ld<T>(s, i);                   // += (-beta omega) s        (:425)
        st(ps, i, p);
        for (int j = 0; j < nsig; ++j) {
            if (skip[j]) continue;
            double *pj = pset + (size_t)j * stride, *xj = xset + (size_t)j * stride;
            T pp = SNT ? ldnt<T>(pj, i) : ld<T>(pj, i);
            T x = (SNT ? ldnt<T>(xj, i) : ld<T>(xj, i)) + cx[j] * q;     // (:438)
            x = x + alpha_j[j] * pp;                                 // (:439)
            if (SNT) stnt(xj, i, x); else st(xj, i, x);
            pp = pp + c1[j] * q;                                     // (:440)
            pp = pp + c2[j] * ro;                                    // (:441)
            pp = beta_j[j] * pp;                                     // my_dscal(beta_j)      (:444)
            pp = pp + cp[j] * rr;                                    // (:445)
            if (SNT) stnt(pj, i, pp); else st(pj, i, pp);
        }
    }
};
void launch_sw_shifts(const Vecs &v, const double *qcopy, double *p_set, double *x_set, uint32_t set_stride, int seed,
                      const ShiftDev *H, Scal *S, hipStream_t s)
{
    auto go = [&](auto f) {
        f.ps = p_set + (size_t)seed * set_stride; f.pset = p_set; f.xset = x_set; f.r = v.r; f.s = v.s; f.qc = qcopy;
        f.rold = v.ax; f.H = H; f.stride = set_stride;
        run_vec(f, v.n, S, Reduce{}, s);
    };
    if (stream_sets()) go(FSwShifts<true>{}); else go(FSwShifts<false>{});
}

// x <- a x (my_dscal, src/vector.c:17-21); runs while the device is paused at a seed switch
__global__ void __launch_bounds__(kBlock) k_scale(double *x, uint32_t n, double a)
{
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) x[i] = a * x[i];
}
void launch_scale(double *x, uint32_t n, double a, hipStream_t s)
{
    if (n == 0) return;
    unsigned g = (n + kBlock - 1) / kBlock;
    if (g > (unsigned)kMaxGrid) g = kMaxGrid;
    BICG_LAUNCH(k_scale, dim3(g), dim3(kBlock), 0, s, x, n, a);
}

// ---- pipelined shifted variant (reference src/shifted_solver.c:794-843)
struct FShPipe1 {   // p[seed], s, z recurrences ; r_old = r ; q, y ; (q,y), (y,y)          (:794-813)
    static constexpr int ND = 2;
    double *p, *s, *z, *r, *w, *rold; const double *t, *v; double alpha, beta, omega;
    __device__ void load(const Scal *S) { alpha = S->alpha; beta = S->beta; omega = S->omega; }
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        T r0 = ld<T>(r, i), w0 = ld<T>(w, i), s0 = ld<T>(s, i), z0 = ld<T>(z, i);
        st(p, i, recur3<T>(ld<T>(p, i), s0, r0, omega, beta));
        T s1 = recur3<T>(s0, z0, w0, omega, beta);
        T z1 = recur3<T>(z0, ld<T>(v, i), ld<T>(t, i), omega, beta);
        st(s, i, s1); st(z, i, z1);
        st(rold, i, r0);
        T q = r0 + (-alpha) * s1;
        T y = w0 + (-alpha) * z1;
        st(r, i, q); st(w, i, y);
        acc[0] += hsum(q * y);
        acc[1] += hsum(y * y);
    }
};
void launch_shift_pipe1(const Vecs &v, double *p_seed, Scal *S, Reduce red, hipStream_t s)
{
    run_vec(FShPipe1{p_seed, v.s, v.z, v.r, v.w, v.ax, v.t, v.v, 0.0, 0.0, 0.0}, v.n, S, red, s);
}

template <bool SNT> struct FShPipe2 {   // x[seed] ; every p_j, x_j ; r ; w = y - omega (t - alpha v) ; five dots   (:829-848)
    static constexpr int ND = 5;
    double *xs, *r, *w, *pset, *xset; const double *ps, *t, *v, *rh, *s, *z, *rold; const ShiftDev *H; uint32_t stride;
    double alpha, omega; int nsig, seed;
    const double *beta_j, *alpha_j, *cp, *cx, *c1, *c2;
    __device__ void load(const Scal *S)
    {
        alpha = S->alpha; omega = S->omega;
        nsig = H->nsig; seed = H->seed;
        beta_j = H->beta; alpha_j = H->alpha; cp = H->cp; cx = H->cx; c1 = H->c1; c2 = H->c2;
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        const T q = ld<T>(r, i), y = ld<T>(w, i), ro = ld<T>(rold, i);
        T xx = ld<T>(xs, i) + alpha * ld<T>(ps, i);
        st(xs, i, xx + omega * q);
        for (int j = 0; j < nsig; ++j) {
            if (j == seed) continue;
            double *pj = pset + (size_t)j * stride, *xj = xset + (size_t)j * stride;
            T p = beta_j[j] * (SNT ? ldnt<T>(pj, i) : ld<T>(pj, i));   // (:806)
            p = p + cp[j] * ro;                                  // (:807)
            T x = (SNT ? ldnt<T>(xj, i) : ld<T>(xj, i)) + cx[j] * q;   // (:834)
            x = x + alpha_j[j] * p;                              // (:835)
            if (SNT) stnt(xj, i, x); else st(xj, i, x);
            p = p + c1[j] * q;                                   // (:836)
            p = p + c2[j] * ro;                                  // (:837)
            if (SNT) stnt(pj, i, p); else st(pj, i, p);
        }
        const T rr = q + (-omega) * y;                           // (:840)
        st(r, i, rr);
        const T tt = ld<T>(t, i) + (-alpha) * ld<T>(v, i);       // (:842)
        const T ww = y + (-omega) * tt;                          // (:843)
        st(w, i, ww);
        const T h = ld<T>(rh, i);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(h * rr);
        acc[2] += hsum(h * ww);
        acc[3] += hsum(h * ld<T>(s, i));
        acc[4] += hsum(h * ld<T>(z, i));
    }
};
void launch_shift_pipe2(const Vecs &v, double *p_set, double *x_set, uint32_t set_stride, int seed, const ShiftDev *H,
                        Scal *S, Reduce red, hipStream_t s)
{
    auto go = [&](auto f) {
        f.xs = x_set + (size_t)seed * set_stride; f.ps = p_set + (size_t)seed * set_stride;
        f.r = v.r; f.w = v.w; f.pset = p_set; f.xset = x_set; f.t = v.t; f.v = v.v; f.rh = v.rh; f.s = v.s; f.z = v.z;
        f.rold = v.ax; f.H = H; f.stride = set_stride;
        run_vec(f, v.n, S, red, s);
    };
    if (stream_sets()) go(FShPipe2<true>{}); else go(FShPipe2<false>{});
}

struct FShiftPSeed {  // p[seed] = beta p[seed] ; += r ; += (-beta omega) s                (:317-319)
    static constexpr int ND = 0;
    double *p; const double *r, *s; double beta, c;
    __device__ void load(const Scal *S) { beta = S->beta; c = -S->beta * S->omega; }
    template <class T> __device__ void apply(uint32_t i, double *) const
    {
        T pp = beta * ld<T>(p, i);
        pp = pp + 1.0 * ld<T>(r, i);
        pp = pp + c * ld<T>(s, i);
        st(p, i, pp);
    }
};
void launch_shift_pseed(const Vecs &v, double *p_seed, Scal *S, hipStream_t s)
{
    run_vec(FShiftPSeed{p_seed, v.r, v.s, 0.0, 0.0}, v.n, S, Reduce{}, s);
}

struct FDrift {     // how far the recursive residual has drifted from the true one (adaptive replacement)
    static constexpr int ND = 2;
    static constexpr int kModes = kAnyMode;
    const double *b, *ax, *r;
    __device__ void load(const Scal *) {}
    template <class T> __device__ void apply(uint32_t i, double *acc) const
    {
        const T rr = ld<T>(r, i);
        const T dlt = (ld<T>(b, i) + (-1.0) * ld<T>(ax, i)) - rr;
        acc[0] += hsum(dlt * dlt);
        acc[1] += hsum(rr * rr);
    }
};
void launch_drift(const Vecs &v, const Launch &L, Reduce red) { run_vec(FDrift{v.b, v.ax, v.r}, v.n, L, red); }

struct FDot {
    static constexpr int ND = 1;
    const double *x, *y;
    __device__ void load(const Scal *) {}
    template <class T> __device__ void apply(uint32_t i, double *acc) const { acc[0] += hsum(ld<T>(x, i) * ld<T>(y, i)); }
};
void launch_dot(const double *x, const double *y, uint32_t n, Scal *S, Reduce red, hipStream_t s)
{
    run_vec(FDot{x, y}, n, S, red, s);
}

void preload_vec_kernels() { preload_kernel(k_scale); }

}  // namespace bicg
