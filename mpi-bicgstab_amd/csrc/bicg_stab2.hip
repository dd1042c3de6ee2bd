// bicg_stab2.hip -- the element-wise passes of a BiCGStab(2) sweep: method BICG_BICGSTAB2 and its right-preconditioned forms
// BICG_BICGSTAB2_DIAG / _BLOCK (the sweep: include/bicgstab_hip.h, the sequence of launches, its dot groups and bytes per row:
// DESIGN.md sections 4.23 and 4.24). Functors on the k_vec / run_vec machinery of
// bicg_vec.h: pairs per thread, 16-byte accesses, the tiled form from 2^24 rows, dots through bicg_reduce.h as FPlainXR's.
//
// The method runs the multi-launch form with the producer-side finish only, so the functors are built for the two ticket modes
// (run_vec's default) and read their scalars from the one scalar block: alpha, beta, g2 = Scal::omega, g1 = Scal::red[kRedG1].
// Every expression is one multiply and one add per term, in the order written here (-ffp-contract=off): a row's result depends on
// neither the grid nor the rank count; only the association of the dot sums does.
// Vectors (Driver::iter_stab2): r0 = v.r, r# = v.rh, u0 = v.p, u1 = v.s, u2 = v.z, r1 = v.y, r2 = v.w.
//
// One functor per pass, templated on the preconditioner (Precond::Kind). Preconditioned, the sweep is the same one on A M^-1: the
// hat streams u^0 = v.v, u^1 = v.t, r^0 = v.b, r^1 = v.ax ride along -- the four vectors of the slab that the unpreconditioned
// sweep leaves idle (v.ax once the set-up has used A x0). The products take the hats, x is updated with them, r0 stays the residual
// of the caller's system.
//   NONE      no hat stream: the hat pointers are a base that is empty, so the functor's layout, loads and machine code are those
//             of the sweep that knows no preconditioner.
//   DIAGONAL  forms the four applications dinv o v in the pass that produces v (one more 8-byte read stream, no launch).
//   BLOCK     leaves them out -- the driver follows the pass with k_bjac_apply, which writes the hat only -- and is otherwise
//             DIAGONAL's arithmetic.
// The two recurrences u^0 = r^0 - beta u^0 (V3) and r^0 -= alpha u^1 (V4) feed x alone: every product input is a fresh
// application. With dinv = 1 every hat equals its vector bit for bit (1 * v = v, signed zeros included) and the sweep is NONE's.
#include <type_traits>

#include "bicg_vec.h"

namespace bicg {

using Kind = Precond::Kind;
constexpr bool hatted(Kind k) { return k != Precond::NONE; }
struct NoHat { template <class T> struct In {}; };
// a pass's hat streams -- the pointers, and In<T>: what fetch loads of them -- or the empty base of the functor and of its In<T>
template <bool HAT, class H> using HatPart = std::conditional_t<HAT, H, NoHat>;
template <bool HAT, class H> static HatPart<HAT, H> hat_part(H h)
{
    if constexpr (HAT) return h; else return {};
}
// the kind as a template argument: fn(constant of the kind) ; by_kind_x: and x's streaming policy, fn(kind, XNT)
template <class Fn> static void by_kind(Kind k, Fn fn)
{
    if (k == Precond::NONE) fn(std::integral_constant<Kind, Precond::NONE>{});
    else if (k == Precond::DIAGONAL) fn(std::integral_constant<Kind, Precond::DIAGONAL>{});
    else fn(std::integral_constant<Kind, Precond::BLOCK>{});
}
template <class Fn> static void by_kind_x(Kind k, Fn fn)
{
    by_kind(k, [&](auto kc) { if (stream_x()) fn(kc, std::true_type{}); else fn(kc, std::false_type{}); });
}

// ---- V1: u0 = r0 - beta u0 ; DIAGONAL: u^0 = dinv o u0                   (j = 0)
struct HatU0 { double *uh0; const double *dinv; template <class T> struct In { T d; }; };
template <Kind K> struct FS2U0 : HatPart<hatted(K), HatU0> {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *u0; const double *r0; double beta;
    template <class T> struct In : HatPart<hatted(K), HatU0>::template In<T> { T u0, r0; };
    __device__ void load(const Scal *S) { beta = S->beta; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        In<T> in{{}, ld<T>(u0, i), ld<T>(r0, i)};
        if constexpr (K == Precond::DIAGONAL) in.d = ld<T>(this->dinv, i);
        return in;
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T u = in.r0 + (-beta) * in.u0;
        st(u0, i, u);
        if constexpr (K == Precond::DIAGONAL) st(this->uh0, i, in.d * u);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_u0(const Vecs &v, Kind hat, const double *dinv, const Launch &L)
{
    by_kind(hat, [&](auto k) { run_vec(FS2U0<k>{hat_part<hatted(k)>(HatU0{v.v, dinv}), v.p, v.r, 0.0}, v.n, L, Reduce{}); });
}

// ---- V2: r0 -= alpha u1 ; DIAGONAL: r^0 = dinv o r0                      (j = 0; its x += alpha u0 rides in V3)
struct HatR0 { double *rh0; const double *dinv; template <class T> struct In { T d; }; };
template <Kind K> struct FS2R0 : HatPart<hatted(K), HatR0> {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *r0; const double *u1; double alpha;
    template <class T> struct In : HatPart<hatted(K), HatR0>::template In<T> { T r0, u1; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        In<T> in{{}, ld<T>(r0, i), ld<T>(u1, i)};
        if constexpr (K == Precond::DIAGONAL) in.d = ld<T>(this->dinv, i);
        return in;
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T r = in.r0 + (-alpha) * in.u1;
        st(r0, i, r);
        if constexpr (K == Precond::DIAGONAL) st(this->rh0, i, in.d * r);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_r0(const Vecs &v, Kind hat, const double *dinv, const Launch &L)
{
    by_kind(hat, [&](auto k) { run_vec(FS2R0<k>{hat_part<hatted(k)>(HatR0{v.b, dinv}), v.r, v.s, 0.0}, v.n, L, Reduce{}); });
}

// ---- V3: x += alpha u0 (step j = 0: u0 is still that step's, and so is Scal::alpha) ; u0 = r0 - beta u0 ; u1 = r1 - beta u1   (j = 1)
// hatted: x += alpha u^0 instead ; u^0 = r^0 - beta u^0 ; DIAGONAL: u^1 = dinv o u1
struct HatXU { double *uh0, *uh1; const double *rh0, *dinv; template <class T> struct In { T uh0, rh0, d; }; };
template <Kind K, bool XNT> struct FS2XU : HatPart<hatted(K), HatXU> {
    static constexpr int ND = 0;
    static constexpr bool kSplit = true;
    double *x, *u0, *u1; const double *r0, *r1; double alpha, beta;
    template <class T> struct In : HatPart<hatted(K), HatXU>::template In<T> { T x, u0, u1, r0, r1; };
    __device__ void load(const Scal *S) { alpha = S->alpha; beta = S->beta; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        In<T> in{};      // the loads in the order compute wants them
        in.x = XNT ? ldnt<T>(x, i) : ld<T>(x, i); in.u0 = ld<T>(u0, i); in.u1 = ld<T>(u1, i);
        if constexpr (hatted(K)) in.uh0 = ld<T>(this->uh0, i);
        in.r0 = ld<T>(r0, i); in.r1 = ld<T>(r1, i);
        if constexpr (hatted(K)) in.rh0 = ld<T>(this->rh0, i);
        if constexpr (K == Precond::DIAGONAL) in.d = ld<T>(this->dinv, i);
        return in;
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *) const
    {
        T xx;
        if constexpr (hatted(K)) xx = in.x + alpha * in.uh0; else xx = in.x + alpha * in.u0;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        st(u0, i, in.r0 + (-beta) * in.u0);
        if constexpr (hatted(K)) st(this->uh0, i, in.rh0 + (-beta) * in.uh0);
        T u = in.r1 + (-beta) * in.u1;
        st(u1, i, u);
        if constexpr (K == Precond::DIAGONAL) st(this->uh1, i, in.d * u);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_xu(const Vecs &v, Kind hat, const double *dinv, const Launch &L)
{
    by_kind_x(hat, [&](auto k, auto nt) {
        run_vec(FS2XU<k, nt>{hat_part<hatted(k)>(HatXU{v.v, v.t, v.b, dinv}), v.x, v.p, v.s, v.r, v.y, 0.0, 0.0}, v.n, L, Reduce{});
    });
}

// ---- V4: x += alpha u0 ; r0 -= alpha u1 ; r1 -= alpha u2 ; (r1,r1), (r0,r1)     (j = 1 ; a11 and b1 of the MR part)
// hatted: u0 is u^0 (the pass has no other use of u0) ; r^0 -= alpha u^1 ; DIAGONAL: r^1 = dinv o r1 -- nine input and five output
// streams, the widest pass of the library
struct HatXRR { double *rh0, *rh1; const double *uh1, *dinv; template <class T> struct In { T rh0, uh1, d; }; };
template <Kind K, bool XNT> struct FS2XRR : HatPart<hatted(K), HatXRR> {
    static constexpr int ND = 2;
    static constexpr bool kSplit = true;
    double *x, *r0, *r1; const double *u0, *u1, *u2; double alpha;
    template <class T> struct In : HatPart<hatted(K), HatXRR>::template In<T> { T x, r0, r1, u0, u1, u2; };
    __device__ void load(const Scal *S) { alpha = S->alpha; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        In<T> in{};
        in.x = XNT ? ldnt<T>(x, i) : ld<T>(x, i); in.r0 = ld<T>(r0, i); in.r1 = ld<T>(r1, i);
        if constexpr (hatted(K)) in.rh0 = ld<T>(this->rh0, i);
        in.u0 = ld<T>(u0, i); in.u1 = ld<T>(u1, i); in.u2 = ld<T>(u2, i);
        if constexpr (hatted(K)) in.uh1 = ld<T>(this->uh1, i);
        if constexpr (K == Precond::DIAGONAL) in.d = ld<T>(this->dinv, i);
        return in;
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx = in.x + alpha * in.u0;
        if (XNT) stnt(x, i, xx); else st(x, i, xx);
        T a = in.r0 + (-alpha) * in.u1;
        T b = in.r1 + (-alpha) * in.u2;
        st(r0, i, a); st(r1, i, b);
        if constexpr (hatted(K)) st(this->rh0, i, in.rh0 + (-alpha) * in.uh1);
        if constexpr (K == Precond::DIAGONAL) st(this->rh1, i, in.d * b);
        acc[0] += hsum(b * b);
        acc[1] += hsum(a * b);
    }
    template <class T> __device__ void apply(uint32_t i, double *acc) const { compute<T>(i, fetch<T>(i), acc); }
};
void launch_stab2_xrr(const Vecs &v, Kind hat, const double *dinv, const Launch &L, Reduce red)
{
    by_kind_x(hat, [&](auto k, auto nt) {
        run_vec(FS2XRR<k, nt>{hat_part<hatted(k)>(HatXRR{v.b, v.ax, v.t, dinv}), v.x, v.r, v.y, hatted(k) ? v.v : v.p, v.s, v.z, 0.0},
                v.n, L, red);
    });
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

// ---- V5 (MR): x += g1 r0 + g2 r1 (hatted: g1 r^0 + g2 r^1) ; r0 -= g1 r1 + g2 r2 ; u0 -= g1 u1 + g2 u2 ; (r0,r0), (r#,r0)
// each as (v + c1 a) + c2 b, c = g or -g. No application: u^0 is formed afresh by the next sweep's V1, so hatted or not is all
// the pass knows of the kind.
struct HatMR { const double *rh0, *rh1; template <class T> struct In { T rh0, rh1; }; };
template <bool HAT, bool XNT> struct FS2MR : HatPart<HAT, HatMR> {
    static constexpr int ND = 2;
    static constexpr bool kSplit = true;
    double *x, *r0, *u0; const double *r1, *r2, *u1, *u2, *rh; double g1, g2;
    template <class T> struct In : HatPart<HAT, HatMR>::template In<T> { T x, r0, u0, r1, r2, u1, u2, rh; };
    __device__ void load(const Scal *S) { g1 = S->red[kRedG1]; g2 = S->omega; }
    template <class T> __device__ In<T> fetch(uint32_t i) const
    {
        In<T> in{};
        in.x = XNT ? ldnt<T>(x, i) : ld<T>(x, i); in.r0 = ld<T>(r0, i); in.u0 = ld<T>(u0, i);
        if constexpr (HAT) { in.rh0 = ld<T>(this->rh0, i); in.rh1 = ld<T>(this->rh1, i); }
        in.r1 = ld<T>(r1, i); in.r2 = ld<T>(r2, i); in.u1 = ld<T>(u1, i); in.u2 = ld<T>(u2, i); in.rh = ld<T>(rh, i);
        return in;
    }
    template <class T> __device__ void compute(uint32_t i, const In<T> &in, double *acc) const
    {
        T xx;
        if constexpr (HAT) { xx = in.x + g1 * in.rh0; xx = xx + g2 * in.rh1; }
        else { xx = in.x + g1 * in.r0; xx = xx + g2 * in.r1; }
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
void launch_stab2_mr(const Vecs &v, Kind hat, const Launch &L, Reduce red)
{
    by_kind_x(hat, [&](auto k, auto nt) {
        run_vec(FS2MR<hatted(k), nt>{hat_part<hatted(k)>(HatMR{v.b, v.ax}), v.x, v.r, v.p, v.y, v.w, v.s, v.z, v.rh, 0.0, 0.0}, v.n, L, red);
    });
}

}  // namespace bicg
