// bicg_vec.h -- the machinery of the fused element-wise phases, shared by the units that define their functors (bicg_vec.hip: the
// solvers of reference src/solver.c and the shifted family; bicg_stab2.hip: BiCGStab(2)): the pair types and their accesses, the kernel
// k_vec and the launch wrapper run_vec. Templates and statics only; what has one owner (the grid, the tiled form) is declared here
// and defined in bicg_vec.hip.
#pragma once

#include "bicg_device.h"
#include "bicg_devfn.h"
#include "bicg_reduce.h"
#include "bicg_knobs.h"
#include "bicg_launch.h"

namespace bicg {

// ------------------------------------------------------------------------------------------
// fused element-wise phases
// ------------------------------------------------------------------------------------------
// Two-wide value so that one functor body serves the 16-byte vectorised main loop and the tail.
struct d2 { double a, b; };
__device__ __forceinline__ d2 operator+(d2 p, d2 q) { return {p.a + q.a, p.b + q.b}; }
__device__ __forceinline__ d2 operator-(d2 p, d2 q) { return {p.a - q.a, p.b - q.b}; }
__device__ __forceinline__ d2 operator*(d2 p, d2 q) { return {p.a * q.a, p.b * q.b}; }
__device__ __forceinline__ d2 operator*(double s, d2 q) { return {s * q.a, s * q.b}; }
__device__ __forceinline__ double hsum(d2 p) { return p.a + p.b; }
__device__ __forceinline__ double hsum(double p) { return p; }

// the same pair for launches over vectors far beyond the caches (tiled k_vec): every access of it is non-temporal
struct d2n { double a, b; };
__device__ __forceinline__ d2n operator+(d2n p, d2n q) { return {p.a + q.a, p.b + q.b}; }
__device__ __forceinline__ d2n operator-(d2n p, d2n q) { return {p.a - q.a, p.b - q.b}; }
__device__ __forceinline__ d2n operator*(d2n p, d2n q) { return {p.a * q.a, p.b * q.b}; }
__device__ __forceinline__ d2n operator*(double s, d2n q) { return {s * q.a, s * q.b}; }
__device__ __forceinline__ double hsum(d2n p) { return p.a + p.b; }

template <class T> __device__ __forceinline__ T ld(const double *p, uint32_t i);
template <> __device__ __forceinline__ double ld<double>(const double *p, uint32_t i) { return p[i]; }
template <> __device__ __forceinline__ d2n ld<d2n>(const double *p, uint32_t i)
{
    const f64x2 t = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(p + i));
    return {t.x, t.y};
}
template <> __device__ __forceinline__ d2 ld<d2>(const double *p, uint32_t i)
{
    const f64x2 t = *reinterpret_cast<const f64x2 *>(p + i);
    return {t.x, t.y};
}
// Streaming policy for vectors that are read and written exactly once per iteration (the solution
// x; the shifted solvers' x_j and p_j sets): non-temporal accesses keep them out of the Infinity
// Cache, which the matrix stream and the re-read work vectors use better. Measured on Transport:
// plain 150.4 -> 145.6 us, CA 170 -> 166, pipelined 168 -> 163, 16 shifts 312 -> 294 us per
// iteration. BICG_X_NT=0 / BICG_SET_NT=0 switch it off (read once).
static bool env_on_x(const char *name, bool dflt)        // measurement knob (bicg_knobs.h): the default unless built with EXPERIMENTS=1
{
    const char *v = knob_x(name);
    return v ? atoi(v) != 0 : dflt;
}
static bool stream_x() { static const bool on = env_on_x("BICG_X_NT", true); return on; }
static bool stream_sets() { static const bool on = env_on_x("BICG_SET_NT", true); return on; }

// streaming variants for vectors touched once per iteration (x): keep the Infinity Cache for the
// matrix and the vectors that are re-read soon
template <class T> __device__ __forceinline__ T ldnt(const double *p, uint32_t i);
template <> __device__ __forceinline__ double ldnt<double>(const double *p, uint32_t i) { return __builtin_nontemporal_load(p + i); }
template <> __device__ __forceinline__ d2 ldnt<d2>(const double *p, uint32_t i)
{
    const f64x2 t = __builtin_nontemporal_load(reinterpret_cast<const f64x2 *>(p + i));
    return {t.x, t.y};
}
template <> __device__ __forceinline__ d2n ldnt<d2n>(const double *p, uint32_t i) { return ld<d2n>(p, i); }
__device__ __forceinline__ void stnt(double *p, uint32_t i, d2n v)
{
    f64x2 t; t.x = v.a; t.y = v.b;
    __builtin_nontemporal_store(t, reinterpret_cast<f64x2 *>(p + i));
}
__device__ __forceinline__ void st(double *p, uint32_t i, d2n v) { stnt(p, i, v); }
__device__ __forceinline__ void stnt(double *p, uint32_t i, double v) { __builtin_nontemporal_store(v, p + i); }
__device__ __forceinline__ void stnt(double *p, uint32_t i, d2 v)
{
    f64x2 t; t.x = v.a; t.y = v.b;
    __builtin_nontemporal_store(t, reinterpret_cast<f64x2 *>(p + i));
}
__device__ __forceinline__ void st(double *p, uint32_t i, double v) { p[i] = v; }
__device__ __forceinline__ void st(double *p, uint32_t i, d2 v)
{
    f64x2 t; t.x = v.a; t.y = v.b;
    *reinterpret_cast<f64x2 *>(p + i) = t;
}

// F::ND dot products, F::load(S) fetches the scalars once, F::apply<T>(i, acc) handles element(s) i.
// Functors of the four solvers additionally split apply into fetch (all loads of an element pair,
// none of which depends on a scalar) and compute: a kernel that finishes a dot group issues the
// loads of its first pair BEFORE waiting for the sums, so the wait runs underneath them.
// F::kModes: bit RedMode set = that instantiation is launched (keeps the others from being compiled).
template <class F, class = void> struct vec_modes { static constexpr int value = (1 << RED_TICKET) | (1 << RED_TICKET_HEAVY); };
template <class F> struct vec_modes<F, decltype((void)F::kModes)> { static constexpr int value = F::kModes; };
template <class F, class = void> struct vec_split { static constexpr bool value = false; };
template <class F> struct vec_split<F, decltype((void)F::kSplit)> { static constexpr bool value = F::kSplit; };
constexpr int kWaveOnly = 1 << RED_WAVE, kAnyMode = (1 << RED_TICKET) | (1 << RED_TICKET_HEAVY) | (1 << RED_WAVE);
// ... and the hand-over (plain BiCGStab's three element-wise kernels): F::kHandPhase / F::kHandN = the group the functor consumes
constexpr int kHandMode = 1 << RED_HAND;

// TILE > 0 (vectors far beyond the caches, vec_tiled()): a workgroup takes ONE contiguous tile of TILE pairs per thread -- 16 KiB
// of every stream for TILE = 4 --, all loads of the tile are in flight before the first store, every access is non-temporal
// (pair type d2n) and the workgroup ends: the shape that streams fastest on this GPU (bicg_stream_bench: copy 4.5 TB/s as a
// grid-stride loop, 5.9 as one workgroup per tile, 6.35 with non-temporal accesses on top). Same arithmetic per element;
// the dot partials are summed over another set of rows per workgroup than in the strided form.
constexpr int kVecTile = 4;
template <class F, int MODE, int TILE = 0>
__global__ void __launch_bounds__(kBlock) k_vec(F f, uint32_t n, Scal *S, Reduce red, Finish fin)
{
    constexpr int ND = F::ND > 0 ? F::ND : 1;
    double acc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) acc[d] = 0.0;
    const uint32_t npair = n >> 1;
    const uint32_t i0 = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    if constexpr (TILE > 0) {
        static_assert(vec_split<F>::value, "tiled launches need the functor's fetch / compute split");
        const uint32_t t0 = blockIdx.x * (uint32_t)(kBlock * TILE) + threadIdx.x;
        typename F::template In<d2n> in[TILE];
        auto fetch_tile = [&]() {
#pragma unroll
            for (int u = 0; u < TILE; ++u) {
                const uint32_t i = t0 + (uint32_t)u * kBlock;
                if (i < npair) in[u] = f.template fetch<d2n>(2 * i);
            }
        };
        auto compute_tile = [&]() {
#pragma unroll
            for (int u = 0; u < TILE; ++u) {
                const uint32_t i = t0 + (uint32_t)u * kBlock;
                if (i < npair) f.template compute<d2n>(2 * i, in[u], acc);
            }
            if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) f.template apply<double>(n - 1, acc);
        };
        if constexpr (MODE == RED_WAVE) {
            __shared__ FinishLds fl;
            __shared__ Scal priv;
            const Scal *sc = S;
            const bool helper = fin.seq && (fin.roles & FIN_SHARDS) && blockIdx.x < (unsigned)kShards;      // (see below)
            if (!helper) fetch_tile();
            if (fin.seq) sc = finish_group(S, fin, fin.roles, blockIdx.x, gridDim.x, fl, &priv);
            if (helper) fetch_tile();
            if (sc->done) return;
            f.load(sc);
            compute_tile();
            if (F::ND > 0) wave_publish<ND>(acc, red.partial, red.slot_base + blockIdx.x);
        } else if constexpr (MODE == RED_HAND) {
            Scal T;
            fetch_tile();
            hand_consume<F::kHandN, F::kHandPhase>(S, fin, T);
            if (T.done) return;
            f.load(&T);
            compute_tile();
            if constexpr (F::ND > 0) {
                __shared__ double sm[5 * ND];
                hand_publish<ND>(acc, fin.Snext, red, blockIdx.x, sm, blockIdx.x);
            }
        } else {
            // (the tile's loads depend on no scalar: they are in flight before `done` and the scalars are asked for)
            fetch_tile();
            if (S->done) return;
            __shared__ double sm[5 * ND];
            f.load(S);
            compute_tile();
            if (F::ND > 0) reduce_publish<ND, MODE == RED_TICKET_HEAVY>(acc, S, red, blockIdx.x, sm);
        }
        return;
    }
    if constexpr (MODE == RED_WAVE) {
        __shared__ FinishLds fl;
        __shared__ Scal priv;
        const Scal *sc = S;
        if constexpr (vec_split<F>::value) {
            typename F::template In<d2> pre{};
            const bool have = i0 < npair;
            // Loads return in issue order (vmcnt), so a workgroup that sums a shard must not queue its
            // partial-sum loads behind its own vector loads: the shard totals are what every other
            // workgroup of the launch is waiting for. Everybody else fetches first and waits underneath.
            const bool helper = fin.seq && (fin.roles & FIN_SHARDS) && blockIdx.x < (unsigned)kShards;
            if (have && !helper) pre = f.template fetch<d2>(2 * i0);
            if (fin.seq) sc = finish_group(S, fin, fin.roles, blockIdx.x, gridDim.x, fl, &priv);
            if (have && helper) pre = f.template fetch<d2>(2 * i0);
            if (sc->done) return;
            f.load(sc);
            if (have) f.template compute<d2>(2 * i0, pre, acc);
            for (uint32_t i = i0 + stride; i < npair; i += stride) f.template compute<d2>(2 * i, f.template fetch<d2>(2 * i), acc);
        } else {
            if (fin.seq) sc = finish_group(S, fin, fin.roles, blockIdx.x, gridDim.x, fl, &priv);
            if (sc->done) return;
            f.load(sc);
            for (uint32_t i = i0; i < npair; i += stride) f.template apply<d2>(2 * i, acc);
        }
        if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) f.template apply<double>(n - 1, acc);
        if (F::ND > 0) wave_publish<ND>(acc, red.partial, red.slot_base + blockIdx.x);
    } else if constexpr (MODE == RED_HAND) {
        // hand-over: the first pair's loads, then the producer's shard totals and the scalar block in one batch; every wavefront
        // adds the totals and applies the recurrence on its own copy (hand_consume) -- no LDS, no barrier in front of the loop
        Scal T;
        typename F::template In<d2> pre{};
        const bool have = i0 < npair;
        if (have) pre = f.template fetch<d2>(2 * i0);
        hand_consume<F::kHandN, F::kHandPhase>(S, fin, T);
        if (T.done) return;
        f.load(&T);
        if (have) f.template compute<d2>(2 * i0, pre, acc);
        for (uint32_t i = i0 + stride; i < npair; i += stride) f.template compute<d2>(2 * i, f.template fetch<d2>(2 * i), acc);
        if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) f.template apply<double>(n - 1, acc);
        if constexpr (F::ND > 0) {
            __shared__ double sm[5 * ND];
            hand_publish<ND>(acc, fin.Snext, red, blockIdx.x, sm, blockIdx.x);
        }
    } else {
        __shared__ double sm[5 * ND];
        if constexpr (vec_split<F>::value) {
            // the first pair's loads depend on no scalar: they are in flight before `done` and the scalars are asked for
            typename F::template In<d2> pre{};
            const bool have = i0 < npair;
            if (have) pre = f.template fetch<d2>(2 * i0);
            if (S->done) return;
            f.load(S);
            if (have) f.template compute<d2>(2 * i0, pre, acc);
            for (uint32_t i = i0 + stride; i < npair; i += stride) f.template compute<d2>(2 * i, f.template fetch<d2>(2 * i), acc);
        } else {
            if (S->done) return;
            f.load(S);
            for (uint32_t i = i0; i < npair; i += stride) f.template apply<d2>(2 * i, acc);
        }
        if ((n & 1u) && blockIdx.x == 0 && threadIdx.x == 0) f.template apply<double>(n - 1, acc);
        if (F::ND > 0) reduce_publish<ND, MODE == RED_TICKET_HEAVY>(acc, S, red, blockIdx.x, sm);
    }
}

// bicg_vec.hip: the grid of an element-wise launch over n rows (vec_grid, bicg_device.h) and whether it takes the tiled form
bool vec_tiled(uint32_t n);

template <class F>
static void run_vec(F f, uint32_t n, const Launch &L, Reduce red)
{
    const unsigned g = vec_grid(n);
    red.expected = g;
    red.slot_base = 0;
    constexpr int modes = vec_modes<F>::value;
    const int mode = modes == kWaveOnly ? RED_WAVE : red_mode(red, L.fin, F::ND > 0);
    if (!((modes >> mode) & 1)) {
        fprintf(stderr, "ERROR: bicgstab_hip: element-wise kernel launched in reduction mode %d it is not built for\n", mode);
        abort();
    }
    if constexpr ((modes >> RED_HAND) & 1) {
        if (mode == RED_HAND) {
            if (!(L.fin.seq && (L.fin.roles & FIN_HAND)) || (F::ND > 0) != (red.hand != 0)) {
                fprintf(stderr, "ERROR: bicgstab_hip: hand-over launch without the group it consumes / produces\n");
                abort();
            }
            if (vec_tiled(n)) BICG_LAUNCH((k_vec<F, RED_HAND, kVecTile>), dim3(g), dim3(kBlock), 0, L.st, f, n, L.S, red, L.fin);
            else BICG_LAUNCH((k_vec<F, RED_HAND>), dim3(g), dim3(kBlock), 0, L.st, f, n, L.S, red, L.fin);
            return;
        }
    }
    if constexpr (vec_split<F>::value) {
        if (vec_tiled(n)) {
            if constexpr ((modes >> RED_WAVE) & 1)
                if (mode == RED_WAVE) { BICG_LAUNCH((k_vec<F, RED_WAVE, kVecTile>), dim3(g), dim3(kBlock), 0, L.st, f, n, L.S, red, L.fin); return; }
            if constexpr (((modes >> RED_TICKET_HEAVY) & 1) && F::ND > 0)
                if (mode == RED_TICKET_HEAVY) { BICG_LAUNCH((k_vec<F, RED_TICKET_HEAVY, kVecTile>), dim3(g), dim3(kBlock), 0, L.st, f, n, L.S, red, L.fin); return; }
            if constexpr ((modes >> RED_TICKET) & 1)
                if (mode != RED_WAVE) { BICG_LAUNCH((k_vec<F, RED_TICKET, kVecTile>), dim3(g), dim3(kBlock), 0, L.st, f, n, L.S, red, L.fin); return; }
        }
    }
    if constexpr ((modes >> RED_WAVE) & 1)
        if (mode == RED_WAVE) { BICG_LAUNCH((k_vec<F, RED_WAVE>), dim3(g), dim3(kBlock), 0, L.st, f, n, L.S, red, L.fin); return; }
    if constexpr (((modes >> RED_TICKET_HEAVY) & 1) && F::ND > 0)
        if (mode == RED_TICKET_HEAVY) { BICG_LAUNCH((k_vec<F, RED_TICKET_HEAVY>), dim3(g), dim3(kBlock), 0, L.st, f, n, L.S, red, L.fin); return; }
    if constexpr ((modes >> RED_TICKET) & 1)
        BICG_LAUNCH((k_vec<F, RED_TICKET>), dim3(g), dim3(kBlock), 0, L.st, f, n, L.S, red, L.fin);
}
// shifted solvers and kernel-level entry points: scalar block updated in place, ticket reductions
template <class F>
static void run_vec(F f, uint32_t n, Scal *S, Reduce red, hipStream_t stream)
{
    run_vec(f, n, Launch{S, Finish{}, stream}, red);
}

}  // namespace bicg
