// bicg_stab2.hip -- the element-wise passes of a BiCGStab(2) sweep (method BICG_BICGSTAB2 and, further down, its right-preconditioned
// forms BICG_BICGSTAB2_DIAG / _BLOCK; the sweep: include/bicgstab_hip.h, the sequence of launches, its dot groups and bytes per row:
// DESIGN.md sections 4.23 and 4.24). Functors on the k_vec / run_vec machinery of
// bicg_vec.h: pairs per thread, 16-byte accesses, the tiled form from 2^24 rows, dots through bicg_reduce.h as FPlainXR's.
//
// The method runs the multi-launch form with the producer-side finish only, so the functors are built for the two ticket modes
// (run_vec's default) and read their scalars from the one scalar block: alpha, beta, g2 = Scal::omega, g1 = Scal::red[kRedG1].
// Every expression is one multiply and one add per term, in the order written here (-ffp-contract=off): a row's result depends on
// neither the grid nor the rank count; only the association of the dot sums does.
// Vectors (Driver::iter_stab2): r0 = v.r, r# = v.rh, u0 = v.p, u1 = v.s, u2 = v.z, r1 = v.y, r2 = v.w.
#include "bicg_vec.h"

namespace bicg {

// ---- V1: u0 = r0 - beta u0                                              (j = 0)
struct FS2U0 {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *u0; const double *r0; double beta;
    template <class T> struct In { T u0, r0; };
    __device__ void load(const Scal *S) { beta = S->beta; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(u0, i), ld<T>(r0, i)}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        st(u0, i, in.r0 + (-beta) * in.u0);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_u0(const Vecs &v, const Launch &L) { run_vec(FS2U0{v.p, v.r, 0.0}, v.n, L, Reduce{}); }

// ---- V2: r0 -= alpha u1                                                 (j = 0; its x += alpha u0 rides in V3)
struct FS2R0 {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *r0; const double *u1; double alpha;
    template <class T> struct In { T r0, u1; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(r0, i), ld<T>(u1, i)}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        st(r0, i, in.r0 + (-alpha) * in.u1);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_r0(const Vecs &v, const Launch &L) { run_vec(FS2R0{v.r, v.s, 0.0}, v.n, L, Reduce{}); }

// ---- V3: x += alpha u0 (step j = 0: u0 is still that step's, and so is Scal::alpha) ; u0 = r0 - beta u0 ; u1 = r1 - beta u1   (j = 1)
template <bool XNT> struct FS2XU {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *x, *u0, *u1; const double *r0, *r1; double alpha, beta;
    template <class T> struct In { T x, u0, u1, r0, r1; };
    __device__ void load(const Scal *S) { alpha = S->alpha; beta = S->beta; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(u0, i), ld<T>(u1, i), ld<T>(r0, i), ld<T>(r1, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T xx = in.x + alpha * in.u0;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        st(u0, i, in.r0 + (-beta) * in.u0);
        st(u1, i, in.r1 + (-beta) * in.u1);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_xu(const Vecs &v, const Launch &L)
{
    if (stream_x()) run_vec(FS2XU<true>{v.x, v.p, v.s, v.r, v.y, 0.0, 0.0}, v.n, L, Reduce{});
    else run_vec(FS2XU<false>{v.x, v.p, v.s, v.r, v.y, 0.0, 0.0}, v.n, L, Reduce{});
}

// ---- V4: x += alpha u0 ; r0 -= alpha u1 ; r1 -= alpha u2 ; (r1,r1), (r0,r1)     (j = 1 ; a11 and b1 of the MR part)
template <bool XNT> struct FS2XRR {
    static constexpr int ND = 2;
    static constexpr bool kSplit = true;
    double *x, *r0, *r1; const double *u0, *u1, *u2; double alpha;
    template <class T> struct In { T x, r0, r1, u0, u1, u2; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(r0, i), ld<T>(r1, i), ld<T>(u0, i), ld<T>(u1, i), ld<T>(u2, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + alpha * in.u0;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T a = in.r0 + (-alpha) * in.u1;
        T b = in.r1 + (-alpha) * in.u2;
        st(r0, i, a); st(r1, i, b);
        acc[0] += hsum(b * b);
        acc[1] += hsum(a * b);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_xrr(const Vecs &v, const Launch &L, Reduce red)
{
    if (stream_x()) run_vec(FS2XRR<true>{v.x, v.r, v.y, v.p, v.s, v.z, 0.0}, v.n, L, red);
    else run_vec(FS2XRR<false>{v.x, v.r, v.y, v.p, v.s, v.z, 0.0}, v.n, L, red);
}

// ---- D: (r0,r2)     (b2 of the MR part: r2 exists only behind the product r2 = A r1, whose epilogue takes two sums)
struct FS2Dot {
    static constexpr int ND = 1;
    static constexpr bool kSplit = true;
    const double *r0, *r2;
    template <class T> struct In { T r0, r2; };
    __device__ void load(const Scal *) {}
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(r0, i), ld<T>(r2, i)}; }
    template <class T> __device__ void compute(uint32_t, const In<T> &in, double *acc) const { acc[0] += hsum(in.r0 * in.r2); }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_dot(const Vecs &v, const Launch &L, Reduce red) { run_vec(FS2Dot{v.r, v.w}, v.n, L, red); }

// ---- V5 (MR): x += g1 r0 + g2 r1 ; r0 -= g1 r1 + g2 r2 ; u0 -= g1 u1 + g2 u2 ; (r0,r0), (r#,r0)
// each as (v + c1 a) + c2 b, c = g or -g
template <bool XNT> struct FS2MR {
    static constexpr int ND = 2;
    static constexpr bool kSplit = true;
    double *x, *r0, *u0; const double *r1, *r2, *u1, *u2, *rh; double g1, g2;
    template <class T> struct In { T x, r0, u0, r1, r2, u1, u2, rh; };
    __device__ void load(const Scal *S) { g1 = S->red[kRedG1]; g2 = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(r0, i), ld<T>(u0, i), ld<T>(r1, i), ld<T>(r2, i), ld<T>(u1, i), ld<T>(u2, i),
                ld<T>(rh, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + g1 * in.r0;
        xx = xx + g2 * in.r1;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T rr = in.r0 + (-g1) * in.r1;
        rr = rr + (-g2) * in.r2;
        st(r0, i, rr);
        T uu = in.u0 + (-g1) * in.u1;
        uu = uu + (-g2) * in.u2;
        st(u0, i, uu);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(in.rh * rr);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_mr(const Vecs &v, const Launch &L, Reduce red)
{
    if (stream_x()) run_vec(FS2MR<true>{v.x, v.r, v.p, v.y, v.w, v.s, v.z, v.rh, 0.0, 0.0}, v.n, L, red);
    else run_vec(FS2MR<false>{v.x, v.r, v.p, v.y, v.w, v.s, v.z, v.rh, 0.0, 0.0}, v.n, L, red);
}

// ------------------------------------------------------------------------------------------
// Right-preconditioned sweep (methods BICG_BICGSTAB2_DIAG / _BLOCK): method 6's sweep on A M^-1. The passes
// V1' .. V5' are V1 .. V5 with the hat streams u^0 = v.v, u^1 = v.t, r^0 = v.b, r^1 = v.ax riding along -- the four vectors of the
// slab that method 6 leaves idle (v.ax once the set-up has used A x0). The products take the hats, x is updated with them, r0 stays
// the residual of the caller's system. DIAG = true forms the four applications dinv o v in the pass that produces v (one more
// 8-byte read stream, no launch); DIAG = false leaves them out -- the driver follows the pass with k_bjac_apply, which writes the
// hat only -- and is otherwise the same arithmetic. The two recurrences u^0 = r^0 - beta u^0 (V3') and r^0 -= alpha u^1 (V4') feed
// x alone: every product input is a fresh application. With dinv = 1 every hat equals its vector bit for bit (1 * v = v, signed
// zeros included) and the sweep is method 6's.
// ---- V1': u0 = r0 - beta u0 ; u^0 = dinv o u0
template <bool DIAG> struct FS2HU0 {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *u0, *uh0; const double *r0, *dinv; double beta;
    template <class T> struct In { T u0, r0, d; };
    __device__ void load(const Scal *S) { beta = S->beta; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(u0, i), ld<T>(r0, i), DIAG ? ld<T>(dinv, i) : T{}}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T u = in.r0 + (-beta) * in.u0;
        st(u0, i, u);
        if (DIAG) st(uh0, i, in.d * u);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2h_u0(const Vecs &v, const double *dinv, const Launch &L)
{
    if (dinv) run_vec(FS2HU0<true>{v.p, v.v, v.r, dinv, 0.0}, v.n, L, Reduce{});
    else run_vec(FS2HU0<false>{v.p, v.v, v.r, nullptr, 0.0}, v.n, L, Reduce{});
}

// ---- V2': r0 -= alpha u1 ; r^0 = dinv o r0                               (its x += alpha u^0 rides in V3')
template <bool DIAG> struct FS2HR0 {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *r0, *rh0; const double *u1, *dinv; double alpha;
    template <class T> struct In { T r0, u1, d; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const { return {ld<T>(r0, i), ld<T>(u1, i), DIAG ? ld<T>(dinv, i) : T{}}; }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T r = in.r0 + (-alpha) * in.u1;
        st(r0, i, r);
        if (DIAG) st(rh0, i, in.d * r);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2h_r0(const Vecs &v, const double *dinv, const Launch &L)
{
    if (dinv) run_vec(FS2HR0<true>{v.r, v.b, v.s, dinv, 0.0}, v.n, L, Reduce{});
    else run_vec(FS2HR0<false>{v.r, v.b, v.s, nullptr, 0.0}, v.n, L, Reduce{});
}

// ---- V3': x += alpha u^0 (step j = 0) ; u0 = r0 - beta u0 ; u^0 = r^0 - beta u^0 ; u1 = r1 - beta u1 ; u^1 = dinv o u1
template <bool DIAG, bool XNT> struct FS2HXU {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *x, *u0, *u1, *uh0, *uh1; const double *r0, *r1, *rh0, *dinv; double alpha, beta;
    template <class T> struct In { T x, u0, u1, uh0, r0, r1, rh0, d; };
    __device__ void load(const Scal *S) { alpha = S->alpha; beta = S->beta; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(u0, i), ld<T>(u1, i), ld<T>(uh0, i), ld<T>(r0, i), ld<T>(r1, i), ld<T>(rh0, i),
                DIAG ? ld<T>(dinv, i) : T{}};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T xx = in.x + alpha * in.uh0;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        st(u0, i, in.r0 + (-beta) * in.u0);
        st(uh0, i, in.rh0 + (-beta) * in.uh0);
        T u = in.r1 + (-beta) * in.u1;
        st(u1, i, u);
        if (DIAG) st(uh1, i, in.d * u);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
template <bool DIAG> static void stab2h_xu(const Vecs &v, const double *dinv, const Launch &L)
{
    if (stream_x()) run_vec(FS2HXU<DIAG, true>{v.x, v.p, v.s, v.v, v.t, v.r, v.y, v.b, dinv, 0.0, 0.0}, v.n, L, Reduce{});
    else run_vec(FS2HXU<DIAG, false>{v.x, v.p, v.s, v.v, v.t, v.r, v.y, v.b, dinv, 0.0, 0.0}, v.n, L, Reduce{});
}
void launch_stab2h_xu(const Vecs &v, const double *dinv, const Launch &L)
{
    if (dinv) stab2h_xu<true>(v, dinv, L); else stab2h_xu<false>(v, nullptr, L);
}

// ---- V4': x += alpha u^0 ; r0 -= alpha u1 ; r^0 -= alpha u^1 ; r1 -= alpha u2 ; r^1 = dinv o r1 ; (r1,r1), (r0,r1)
// nine input and five output streams (DIAG): the widest pass of the library
template <bool DIAG, bool XNT> struct FS2HXRR {
    static constexpr int ND = 2;
    static constexpr bool kSplit = true;
    double *x, *r0, *r1, *rh0, *rh1; const double *uh0, *u1, *u2, *uh1, *dinv; double alpha;
    template <class T> struct In { T x, r0, r1, rh0, uh0, u1, u2, uh1, d; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(r0, i), ld<T>(r1, i), ld<T>(rh0, i), ld<T>(uh0, i), ld<T>(u1, i), ld<T>(u2, i),
                ld<T>(uh1, i), DIAG ? ld<T>(dinv, i) : T{}};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + alpha * in.uh0;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T a = in.r0 + (-alpha) * in.u1;
        T b = in.r1 + (-alpha) * in.u2;
        st(r0, i, a); st(r1, i, b);
        st(rh0, i, in.rh0 + (-alpha) * in.uh1);
        if (DIAG) st(rh1, i, in.d * b);
        acc[0] += hsum(b * b);
        acc[1] += hsum(a * b);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
template <bool DIAG> static void stab2h_xrr(const Vecs &v, const double *dinv, const Launch &L, Reduce red)
{
    if (stream_x()) run_vec(FS2HXRR<DIAG, true>{v.x, v.r, v.y, v.b, v.ax, v.v, v.s, v.z, v.t, dinv, 0.0}, v.n, L, red);
    else run_vec(FS2HXRR<DIAG, false>{v.x, v.r, v.y, v.b, v.ax, v.v, v.s, v.z, v.t, dinv, 0.0}, v.n, L, red);
}
void launch_stab2h_xrr(const Vecs &v, const double *dinv, const Launch &L, Reduce red)
{
    if (dinv) stab2h_xrr<true>(v, dinv, L, red); else stab2h_xrr<false>(v, nullptr, L, red);
}

// ---- V5' (MR): x += g1 r^0 + g2 r^1 ; r0 -= g1 r1 + g2 r2 ; u0 -= g1 u1 + g2 u2 ; (r0,r0), (r#,r0)
// no application: u^0 is formed afresh by the next sweep's V1'. One functor for both kinds.
template <bool XNT> struct FS2HMR {
    static constexpr int ND = 2;
    static constexpr bool kSplit = true;
    double *x, *r0, *u0; const double *rh0, *rh1, *r1, *r2, *u1, *u2, *rh; double g1, g2;
    template <class T> struct In { T x, r0, u0, rh0, rh1, r1, r2, u1, u2, rh; };
    __device__ void load(const Scal *S) { g1 = S->red[kRedG1]; g2 = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        return {XNT ? ldnt<T>(x, i) : ld<T>(x, i), ld<T>(r0, i), ld<T>(u0, i), ld<T>(rh0, i), ld<T>(rh1, i), ld<T>(r1, i), ld<T>(r2, i),
                ld<T>(u1, i), ld<T>(u2, i), ld<T>(rh, i)};
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + g1 * in.rh0;
        xx = xx + g2 * in.rh1;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T rr = in.r0 + (-g1) * in.r1;
        rr = rr + (-g2) * in.r2;
        st(r0, i, rr);
        T uu = in.u0 + (-g1) * in.u1;
        uu = uu + (-g2) * in.u2;
        st(u0, i, uu);
        acc[0] += hsum(rr * rr);
        acc[1] += hsum(in.rh * rr);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2h_mr(const Vecs &v, const Launch &L, Reduce red)
{
    if (stream_x()) run_vec(FS2HMR<true>{v.x, v.r, v.p, v.b, v.ax, v.y, v.w, v.s, v.z, v.rh, 0.0, 0.0}, v.n, L, red);
    else run_vec(FS2HMR<false>{v.x, v.r, v.p, v.b, v.ax, v.y, v.w, v.s, v.z, v.rh, 0.0, 0.0}, v.n, L, red);
}

}  // namespace bicg
