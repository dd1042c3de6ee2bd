// bicg_spmv_sell.h -- the sliced-ELL product: device helpers, the row product every layout shares (sell_row), the two kernels
// (k_spmv_sell, k_spmv_sell_epi) and the three function templates through which ONE layout's instantiations are reached.
// bicg_spmv_sell_lay.hip instantiates them for one layout per translation unit; bicg_spmv_sell.hip picks the layout.
#pragma once
#include "bicg_device.h"
#include "bicg_devfn.h"
#include "bicg_reduce.h"
#include "bicg_knobs.h"
#include "bicg_launch.h"

namespace bicg {

// ------------------------------------------------------------------------------------------
// Sliced-ELL SpMV (the default path for rows whose slice pads by < 25 %)
//
// Why: the CSR row-block kernel above is limited by the vector L1 (TCP), not by HBM: with lanes
// walking the non-zeros row-major, the x gather of a wavefront touches ~20 different cache lines
// per instruction; rocprofv3 shows 26 M TCP tag accesses per SpMV (1.1 per non-zero), the TCP
// clock-enabled 85 % of the kernel, and the time does not react to fabric traffic or occupancy.
// With lane = row (SELL-64) consecutive lanes read consecutive entries of val/col AND, for banded
// matrices, consecutive entries of x: ~0.35 tag accesses per non-zero, no LDS, no barrier.
// Each lane accumulates its own row in stored order -> bit-identical to mult() (reference
// src/matrix.c:506-515) for every row. Padding entries are loaded (coalescing) but never added.
// ------------------------------------------------------------------------------------------
typedef short i16x4 __attribute__((ext_vector_type(4)));

// C16: column indices are read as 16-bit offsets from the row (col = row + delta), four
// consecutive entries of a lane packed in one 8-byte word: 10 instead of 12 bytes per non-zero.
// Used when every entry of the sliced-ELL copy satisfies |col - row| < 32768 (banded matrices).
// y_i of this lane's row of list entry gi (diag part in stored order, then the offd part, then the shift):
// the body shared by the SpMV kernel and the SpMV-with-epilogue kernel below
extern __shared__ double dyn_lds[];      // the x window of LAY_JAGW launches (SellDev::win_slots doubles)

// LAY_JAGW: copy the x values the group's rows touch into LDS (all 256 threads; the caller's loop is workgroup-uniform)
__device__ __forceinline__ void sell_stage_window(const SpmvArgs &a, unsigned g, double *win)
{
    __syncthreads();                                          // the previous group's reads of the window are done
    const uint32_t r0 = a.sell.win_ptr[g], r1 = a.sell.win_ptr[g + 1];
    for (uint32_t r = r0; r < r1; ++r) {
        const uint2 run = a.sell.win_runs[r];                 // wave-uniform
        const uint32_t len = run.y & 0xFFFFu, slot0 = run.y >> 16;
        for (uint32_t i = threadIdx.x; i < len; i += kBlock) win[slot0 + i] = a.x[run.x + i];
    }
    __syncthreads();
}

// A list-driven slice whose descriptor is known (SellDev::sdesc): the sum of one row of a CONSTANT slice (MASKED = false: every
// row has every entry of the list) or of a MASKED slice (pm = the entries this lane's row has). Distances and values arrive as
// scalar loads of whole batches (the lists are padded with zeros to a multiple of 8 + 16), x is addressed as
// (uniform base) + (32-bit byte offset of the row): two vector instructions of arithmetic per entry next to its load,
// where the general loop spent twenty-odd on a slice of the 7-point Laplacian. The entries are added in list = stored order, the
// ones a row does not have are not added: the same sum, bit for bit, as the general loop's (reference src/matrix.c:506-515).
// (the lists, the descriptors and the group list are read-only for every launch: loads through the constant address space are
// scalar loads whatever the compiler can prove about the stores of the kernel)
#define BICG_KCONST __attribute__((address_space(4)))
struct SellPre { unsigned g; uint4 d; uint32_t pm; };      // group, descriptor and row mask of the wavefront's slice, requested ahead by the product
typedef int sell_i8 __attribute__((ext_vector_type(8)));
typedef unsigned sell_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 sell_desc_load(const uint4 *p)       // (a native vector type: uint4's copy constructor would drop the address space)
{
    const sell_u4 v = *(const BICG_KCONST sell_u4 *)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}
template <bool MASKED>
__device__ __forceinline__ double sell_list_row(const double *__restrict__ x, uint32_t row, uint32_t len, const int *uo_g, const double *uv_g,
                                                uint32_t pm)
{
    const BICG_KCONST int *uo = (const BICG_KCONST int *)uo_g;
    const BICG_KCONST double *uv = (const BICG_KCONST double *)uv_g;
    const uint32_t boff = row << 3;                               // rows < 2^29 (build_slice_desc)
    double sum = 0.0;
    for (uint32_t k0 = 0; k0 < len; k0 += 8) {
        const sell_i8 o = *(const BICG_KCONST sell_i8 *)(uo + k0);
        double v[8], xv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = uv[k0 + e];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (MASKED) {
                // an absent neighbour may lie outside the vector: the lane reads x of its own row instead
                const uint32_t off = ((pm >> (k0 + e)) & 1u) ? (uint32_t)o[e] << 3 : 0u;
                xv[e] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(x) + (uint32_t)(boff + off));
            } else {
                xv[e] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(x + o[e]) + boff);   // (padding: distance 0)
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (MASKED ? ((pm >> (k0 + e)) & 1u) != 0u : k0 + e < len) sum += v[e] * xv[e];
    }
    return sum;
}

// The same sum for a list of exactly N <= 8 entries (SellDev::all_lists): no loop, no tests of the length; the distances arrive as
// byte offsets (SellDev::uoff8) and are added to the row's byte offset modulo 2^32 -- one vector addition per entry, the load
// takes (uniform base of x) + (32-bit offset). o8 / v: the list, already in scalar registers (the caller keeps the list of the
// previous slice: the interior of a stencil has ONE).
template <int N, bool MASKED>
__device__ __forceinline__ double sell_list_fixed(const double *x, uint32_t boff, const sell_i8 &o8, const double (&v)[8], uint32_t pm,
                                                  double *yp, double yv)
{
    double xv[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const uint32_t off = (!MASKED || ((pm >> e) & 1u)) ? (uint32_t)o8[e] : 0u;      // (an absent neighbour may lie outside the vector)
        xv[e] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(x) + (uint32_t)(boff + off));
    }
    // the PREVIOUS slice's result is stored here, behind this slice's gathers: issued right after its own slice it would be the
    // youngest request in flight when the loop comes round, and the wait for the next descriptor (vector loads return in order)
    // a wait for the store's acknowledgement. (Unconditional: with a path that does not store, the wait for the last gather
    // becomes a wait for everything.)
    *yp = yv;
    double sum = 0.0;
#pragma unroll
    for (int e = 0; e < N; ++e)
        if (!MASKED || ((pm >> e) & 1u) != 0u) sum += v[e] * xv[e];                       // list = stored order
    return sum;
}
template <bool MASKED>
__device__ __forceinline__ double sell_list_switch(uint32_t len, const double *x, uint32_t boff, const sell_i8 &o8, const double (&v)[8], uint32_t pm,
                                                   double *yp, double yv)
{
    switch (len) {                                                // wave-uniform
    case 1: return sell_list_fixed<1, MASKED>(x, boff, o8, v, pm, yp, yv);
    case 2: return sell_list_fixed<2, MASKED>(x, boff, o8, v, pm, yp, yv);
    case 3: return sell_list_fixed<3, MASKED>(x, boff, o8, v, pm, yp, yv);
    case 4: return sell_list_fixed<4, MASKED>(x, boff, o8, v, pm, yp, yv);
    case 5: return sell_list_fixed<5, MASKED>(x, boff, o8, v, pm, yp, yv);
    case 6: return sell_list_fixed<6, MASKED>(x, boff, o8, v, pm, yp, yv);
    case 7: return sell_list_fixed<7, MASKED>(x, boff, o8, v, pm, yp, yv);
    default: return sell_list_fixed<8, MASKED>(x, boff, o8, v, pm, yp, yv);
    }
}

template <bool OFFD, bool NT, int LAY, bool LL, int U = 8>      // U entries per lane in flight (4, 8, 16 measured identical on Transport)
__device__ __forceinline__ double sell_row(const SpmvArgs &a, unsigned gi, int done, uint32_t &row, bool &live, bool &ll_failed,
                                           const double *win = nullptr, bool have_pre = false, SellPre pre = SellPre{0u, {0u, 0u, 0u, 0u}, 0u})
{
    constexpr bool WIN = LAY == LAY_JAGW, C16 = (LAY & 1) != 0 || WIN, JAG = LAY >= LAY_JAG32 && LAY <= LAY_JAGW, CONSTV = LAY >= LAY_PAD32C;
    // (the wavefront's number as a SCALAR: the slice's base, length and list positions then come through the scalar cache and the
    // tests on them are scalar branches -- as a vector value the compiler masked and unmasked lanes around every entry)
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const double *__restrict__ x = a.x;
    const unsigned g = have_pre ? pre.g : (a.glist ? a.glist[gi] : gi);
    row = g * kGroupRows + tid;                                // = slice * 64 + lane
    if (LAY == LAY_JAGW && a.sell.perm) row = g * kGroupRows + a.sell.perm[(size_t)g * kGroupRows + tid];
    const uint32_t slice = g * (kGroupRows / kSliceRows) + wave;
    live = row < a.nrows;

    // constant and masked slices by their descriptor (SellDev::sdesc): all 64 rows exist, nothing else of the slice's
    // metadata is read
    bool listed = false;
    double lsum = 0.0;
    if (CONSTV && a.sell.sdesc && slice * kSliceRows < a.nrows) {
        uint4 d;
        if (have_pre) d = pre.d;
        else {
            d = sell_desc_load(a.sell.sdesc + slice);
        }
        const uint32_t kind = d.x >> 16, dlen = d.x & 0xFFFFu;
        if (kind == kSliceConstant) {
            listed = true;
            lsum = sell_list_row<false>(x, row, dlen, a.sell.uoff + d.y, a.sell.uval + d.z, 0u);
        } else if (kind == kSliceMasked) {
            listed = true;
            const uint32_t pm = have_pre ? pre.pm : (uint32_t)a.sell.rmask[(size_t)d.w * kSliceRows + lane];
            lsum = sell_list_row<true>(x, row, dlen, a.sell.uoff + d.y, a.sell.uval + d.z, pm);
        }
    }

    uint32_t base = 0u, len = 0u, base16 = 0u;
    if (slice * kSliceRows < a.nrows && !(CONSTV && listed)) {
        base = a.sell.slice_base[slice]; len = a.sell.slice_len[slice];
        if (C16 && !JAG) base16 = a.sell.slice_base16[slice];
    }
    // uniform slice: the columns are row + uoff[k], one list for the whole slice (scalar loads) -- no col / col16 traffic.
    // Same loop as the padded slices (one body: a second copy of it cost the ticket-mode kernels three spilled registers)
    const int *__restrict__ uo = nullptr;                         // padded with zeros to a multiple of U (+ U)
    const double *__restrict__ uv = nullptr;                      // constant slice: the values too (padded with zeros alike)
    if (!JAG && a.sell.ubase && slice * kSliceRows < a.nrows && !(CONSTV && listed)) {
        const uint32_t ub = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.sell.ubase[slice]);
        if (ub != 0xFFFFFFFFu) {
            uo = a.sell.uoff + ub;
            if (CONSTV) {
                const uint32_t vb = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.sell.vbase[slice]);
                if (vb != 0xFFFFFFFFu) uv = a.sell.uval + vb;
            }
        }
    }
    // masked slice (SellDev::mbase): list of (distance, value) pairs + one word per row saying which of them the row has
    bool masked = false;
    uint32_t pm = 0u;
    if (CONSTV && uv && a.sell.mbase) {
        const uint32_t mb = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.sell.mbase[slice]);
        if (mb != 0xFFFFFFFFu) {
            masked = true;
            len = mb >> 26;                                       // the list's length, not the longest row's
            pm = a.sell.rmask[(size_t)(mb & 0x03FFFFFFu) * kSliceRows + lane];
        }
    }
    // (a list-driven slice knows its rows' lengths: all equal to the slice's, or given by the masks -- no row-pointer loads)
    uint32_t mylen = 0u, oa = 0u, ob = 0u;
    if (live) {
        mylen = (uo || (CONSTV && listed)) ? len : a.diag.ptr[row + 1] - a.diag.ptr[row];
        if (OFFD && (!LL || gi >= a.ll.first_bnd)) { oa = a.offd.ptr[row]; ob = a.offd.ptr[row + 1]; }
    }

    double sum = 0.0;
    if (JAG) {
        // Jagged slice: step k of the slice holds the entries of the lanes whose row has more than k entries, and
        // only those, in lane order -- no padding is stored or read. A lane's entry is at (entries of the earlier
        // steps) + (live lanes below it): a ballot, a population count and mbcnt, all from the row lengths, so
        // every load of a batch is still issued back to back. With equal row lengths this IS the padded layout.
        const uint32_t rb = live ? row : 0u;
        uint32_t pos = base;                                  // wave-uniform: first entry of step k
        for (uint32_t k0 = 0; k0 < len; k0 += U) {
            uint32_t c[U];
            double   v[U];
            bool     mine[U];
            // The val / col loads are predicated per lane, and NOTHING that depends on a loaded value sits inside
            // the predicated block (the compiler waits for a load before the block ends otherwise: one round trip per
            // entry instead of one per batch). The gathers are unpredicated for the same reason: a lane whose row
            // has ended reads x of its own row.
#pragma unroll
            for (int e = 0; e < U; ++e) {
                mine[e] = k0 + e < mylen;
                const unsigned long long m = __ballot(mine[e]);
                const uint32_t j = pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                pos += (uint32_t)__builtin_popcountll(m);
                c[e] = 0u; v[e] = 0.0;
                if (mine[e]) {
                    if (WIN) {
                        const unsigned short *sl = reinterpret_cast<const unsigned short *>(a.sell.col16);
                        c[e] = NT ? __builtin_nontemporal_load(sl + j) : sl[j];
                    } else if (C16) {
                        c[e] = (uint32_t)(int)(NT ? __builtin_nontemporal_load(a.sell.col16 + j) : a.sell.col16[j]);
                    } else {
                        c[e] = NT ? __builtin_nontemporal_load(a.sell.col + j) : a.sell.col[j];
                    }
                    v[e] = NT ? __builtin_nontemporal_load(a.sell.val + j) : a.sell.val[j];
                }
            }
            double xv[U];
#pragma unroll
            for (int e = 0; e < U; ++e) {
                if (WIN) xv[e] = win[c[e]];                   // slot 0 for a lane whose row has ended
                else xv[e] = x[mine[e] ? (C16 ? rb + c[e] : c[e]) : rb];
            }
#pragma unroll
            for (int e = 0; e < U; ++e)
                if (mine[e]) sum += v[e] * xv[e];             // stored order
        }
    }
    for (uint32_t k0 = 0; !JAG && k0 < len; k0 += U) {
        uint32_t c[U];
        double   v[U];
        // lanes past the last row hold padding only: their offsets are 0 and must not turn into
        // reads of x[row >= nrows] (the vector may end before the 64-row slice does)
        const uint32_t rb = live ? row : 0u;
        if (CONSTV && masked) {
#pragma unroll
            for (int e = 0; e < U; ++e) c[e] = rb + (((pm >> (k0 + e)) & 1u) ? (uint32_t)uo[k0 + e] : 0u);   // an absent neighbour may lie outside the vector
        } else if (uo) {
#pragma unroll
            for (int e = 0; e < U; ++e) c[e] = rb + (uint32_t)uo[k0 + e];
        } else if (C16) {
            static_assert(U % 4 == 0, "packed 16-bit columns come four at a time");
#pragma unroll
            for (int q = 0; q < U / 4; ++q) {
                const bool ok = k0 + 4 * q < len;             // wave-uniform; the quad is padded
                const i16x4 *p = reinterpret_cast<const i16x4 *>(a.sell.col16) +
                                 ((size_t)base16 / 4 + (size_t)((k0 / 4) + q) * kSliceRows + lane);
                i16x4 dq = (i16x4)(0);
                if (ok) dq = NT ? __builtin_nontemporal_load(p) : *p;
                c[4 * q + 0] = rb + (int)dq.x; c[4 * q + 1] = rb + (int)dq.y;
                c[4 * q + 2] = rb + (int)dq.z; c[4 * q + 3] = rb + (int)dq.w;
            }
        }
#pragma unroll
        for (int e = 0; e < U; ++e) {
            const bool ok = k0 + e < len;                     // wave-uniform
            const uint32_t j = base + (k0 + e) * kSliceRows + lane;
            if (!C16 && !uo) c[e] = ok ? (NT ? __builtin_nontemporal_load(a.sell.col + j) : a.sell.col[j]) : 0u;
            if (CONSTV && uv) v[e] = uv[k0 + e];              // (wave-uniform branch, scalar load)
            else v[e] = ok ? (NT ? __builtin_nontemporal_load(a.sell.val + j) : a.sell.val[j]) : 0.0;
        }
        double xv[U];
#pragma unroll
        for (int e = 0; e < U; ++e) xv[e] = x[c[e]];
#pragma unroll
        for (int e = 0; e < U; ++e)
            if ((CONSTV && masked) ? ((pm >> (k0 + e)) & 1u) != 0u : k0 + e < mylen) sum += v[e] * xv[e];   // stored order; padding never added
    }
    if (CONSTV && listed) sum = lsum;
    double yi = 0.0 + sum;                                    // y = 0 ; y += tempy  (src/matrix.c:434-437, 514)
    if (OFFD) {
        double so = 0.0;
        for (uint32_t k = oa; k < ob; ++k) {
            double xh;
            if (LL) {
                // the value comes straight from the landing ring; the diag part above ran while it travelled
                xh = 0.0;
                if (!done && !ll_wait(a.ll.ring + ((size_t)(a.ll.seq % kHaloRing) * a.ll.halo + (a.offd.col[k] - a.nrows)) * 2,
                                      a.ll.seq, a.ll.timeout_ticks, &xh))
                    ll_failed = true;
            } else {
                xh = x[a.offd.col[k]];
            }
            so += a.offd.val[k] * xh;
        }
        yi += so;                                             // second mult() call, src/matrix.c:440
    }
    if (a.has_shift && live) yi += a.shift * x[row];          // (A + sigma I) x, src/shifted_solver.c:260
    return yi;
}

// the leading workgroups of a launch with in-kernel halo exchange: store the send list into the peers' landing rings
__device__ __forceinline__ void sell_halo_push(const SpmvArgs &a, unsigned bid, int done)
{
    if (done) return;
    for (uint32_t i = bid * kBlock + threadIdx.x; i < a.ll.nsend; i += a.ll.npush * kBlock)
        ll_store(reinterpret_cast<llword *>(a.ll.dst0[i] + (unsigned long long)(a.ll.seq % kHaloRing) * a.ll.dstride[i]),
                 a.x[a.ll.send_idx[i]], a.ll.seq);
}

template <int NDOT, bool OFFD, bool NT, int LAY, bool LL, int MODE>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(((MODE == RED_TICKET || MODE == RED_HAND) && LAY < LAY_PAD32C) ? 8 : 4, 8))) k_spmv_sell(SpmvArgs a)   // (layouts with list-driven slices: no pin, they spilled 200 bytes per lane at 64 registers)
{
    const int done = a.S->done;       // consumed at the stores only (see k_spmv)
    __shared__ double sm[5 * (NDOT > 0 ? NDOT : 1)];
    unsigned bid = blockIdx.x, nblocks = gridDim.x;
    bool ll_failed = false;
    if (LL) {
        // peer-to-peer exchange inside the launch: the leading workgroups are scheduled first and
        // send; x is complete (it was written by earlier kernels), so nothing has to be waited for
        if (bid < a.ll.npush) { sell_halo_push(a, bid, done); return; }
        bid -= a.ll.npush; nblocks -= a.ll.npush;
    }
    if (MODE == RED_WAVE) {
        // a dot group of EARLIER kernels rides on this launch: its first workgroups add up the shards
        // (and hand the sums to the other ranks) while everybody else already streams the matrix
        // (only the workgroups that have a part in it: the others would still wait for `done` inside finish_group before their
        // first row -- one round trip per workgroup, 40.4 instead of 33.1 us per product of the pipelined iteration)
        __shared__ FinishLds fl;
        if (a.fin.seq && (bid < (unsigned)kShards || (a.fin.roles & FIN_APPLY))) (void)finish_group(a.S, a.fin, a.fin.roles, bid, nblocks, fl, nullptr);
    }

    double acc[NDOT > 0 ? NDOT : 1];
#pragma unroll
    for (int d = 0; d < (NDOT > 0 ? NDOT : 1); ++d) acc[d] = 0.0;

    // Which groups: workgroup bid stands for VIRTUAL workgroup vb of the canonical order -- XCD-contiguous (workgroup b runs on
    // XCD b % 8: XCD x gets the x-th eighth of the virtual workgroups, so one L2 fetches what neighbouring groups share) and,
    // every other product, reversed -- and takes the CONTIGUOUS groups vb * each ... of the list. Its partial sums go to slot vb
    // whichever physical workgroup computed them: the association of a dot sum does not depend on placement. Direction: with ONE
    // group per workgroup it does not matter either; with several (each > 1, grids beyond 65 536 groups) a reversed launch adds a
    // workgroup's groups in the opposite order -- a different, equally fixed association, and every solve / stand-alone call starts
    // from the same direction (bicg_ctx::spmv_dir is reset there), so repeated calls on one context give the same bits.
    // (Launches with the halo exchange inside keep the strided assignment: their leading workgroups are the senders.)
    unsigned vb = bid;
    if (a.xcd_map && !LL && bid < (nblocks / 8u) * 8u) vb = (bid % 8u) * (nblocks / 8u) + bid / 8u;
    if (a.reverse && !LL) vb = nblocks - 1u - vb;
    const unsigned each = LL ? 1u : (a.nlist + nblocks - 1u) / nblocks;
    const unsigned slot = LL ? bid : vb;
    const unsigned gfirst = LL ? bid : vb * each, gend = LL ? a.nlist : (gfirst + each < a.nlist ? gfirst + each : a.nlist);
    // Blocks with list-driven slices (SellDev::sdesc): what a wavefront needs to know about its next slices is requested while
    // it multiplies the current one -- the group number three groups ahead, the descriptor two ahead, the row masks one ahead --
    // so that a constant or masked slice is the scalar loads of its lists (scalar cache) and ONE vector round trip, the x gathers,
    // instead of four dependent trips (group, metadata, lists / masks, x). The requests are VECTOR loads of wave-uniform
    // addresses on purpose: vector loads return in order and are waited for by count, so they stay in flight across the product
    // of the current slice; scalar loads can only be waited for all at once, i.e. at the very next scalar load.
    constexpr bool PRE = LAY >= LAY_PAD32C && !LL;
    const bool pre_on = PRE && a.sell.sdesc != nullptr;
    unsigned vzero = 0u;
    if (PRE) asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));      // a zero the compiler takes for lane-dependent
    const unsigned wvec = threadIdx.x >> 6;
    // Every slice list-driven, lists of at most 8 entries (SellDev::all_lists -- a constant-coefficient stencil): a loop of its own
    // below. Its four wavefronts do not take four CONSECUTIVE slices but four slices `ystride` apart (SellDev::ystride = slices
    // per grid line: the same x segment of four consecutive grid lines) -- the +line gather of one wavefront is then the own-row
    // gather of the next, through the CU's L1 while both are in flight (56 instead of 80 cache lines per four slices of the
    // 7-point Laplacian). Any ystride gives each slice to exactly one wavefront: slice = (g / S) 4 S + wave S + g % S.
    const bool lean = PRE && pre_on && a.sell.all_lists != 0 && !OFFD && !a.has_shift;
    const unsigned ys = lean ? (unsigned)a.sell.ystride : 0u;
    auto slice_of = [&](unsigned g, unsigned w) -> uint32_t {
        const unsigned sh = (unsigned)__builtin_ctz(ys | 0x80000000u);                         // ystride is a power of two (or 0)
        return ys ? ((g >> sh) << (sh + 2u)) + (w << sh) + (g & (ys - 1u)) : g * (kGroupRows / kSliceRows) + w;
    };
    auto group_idx = [&](unsigned q) -> unsigned { return a.reverse ? gfirst + (gend - 1u - q) : q; };      // (q < gend)
    auto group_vec = [&](unsigned q) -> unsigned { return a.glist ? a.glist[group_idx(q) + vzero] : group_idx(q); };
    auto desc_vec = [&](unsigned g) -> uint4 {
        const uint32_t sl = slice_of(g, wvec);
        uint4 d = make_uint4(0u, 0u, 0u, 0u);
        if (sl * kSliceRows < a.nrows) d = a.sell.sdesc[sl];
        return d;
    };
    auto first_lane = [](uint4 v) -> uint4 {
        return make_uint4((uint32_t)__builtin_amdgcn_readfirstlane((int)v.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)v.y),
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)v.z), (uint32_t)__builtin_amdgcn_readfirstlane((int)v.w));
    };
    auto mask_vec = [&](const uint4 &d) -> uint32_t {
        return (d.x >> 16) == (uint32_t)kSliceMasked ? (uint32_t)a.sell.rmask[(size_t)d.w * kSliceRows + (threadIdx.x & 63u)] : 0u;
    };
    SellPre pcur = {0u, make_uint4(0u, 0u, 0u, 0u), 0u};
    unsigned g1 = 0u, gv2 = 0u;                                   // group of the next slice (scalar), of the one after it (as loaded)
    uint4 dv1 = make_uint4(0u, 0u, 0u, 0u);                       // descriptor of the next slice (as loaded)
    if (PRE && pre_on && gfirst < gend) {
        pcur.g = (unsigned)__builtin_amdgcn_readfirstlane((int)group_vec(gfirst));
        pcur.d = first_lane(desc_vec(pcur.g));
        pcur.pm = mask_vec(pcur.d);
        if (gfirst + 1u < gend) { g1 = (unsigned)__builtin_amdgcn_readfirstlane((int)group_vec(gfirst + 1u)); dv1 = desc_vec(g1); }
        if (gfirst + 2u < gend) gv2 = group_vec(gfirst + 2u);
    }
    // The loop of its own (SellDev::all_lists). Per slice: the descriptor (requested two slices ahead), the lists only when they
    // are not the previous slice's, N gathers of a compile-time N, N products; 85 vector + 134 scalar instructions per slice of
    // the 7-point Laplacian went through sell_row (rocprofv3: the scalar unit busy half of the time, waves waiting for memory a
    // fifth of theirs).
    if (PRE && !OFFD && lean && !done && gfirst < gend) {         // (done: nothing is stored and nothing published -- nothing to do)
        const double *__restrict__ x = a.x;
        const unsigned last = gend - 1u;                          // (requests past the workgroup's last group repeat it: no tests)
        uint32_t cy = 0xFFFFFFFFu, cz = 0xFFFFFFFFu;              // the lists in registers
        sell_i8 o8 = (sell_i8)(0);
        double lv[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const unsigned pw = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
        double *yp = a.y + (slice_of(pcur.g, pw) * kSliceRows + lane);   // where the previous slice's result goes (first slice: a zero
        double yv = 0.0;                                          // into its own row, overwritten by its result one slice later)
        for (unsigned gq = gfirst; gq < gend; ++gq) {
            SellPre pnext;
            pnext.g = g1; pnext.d = first_lane(dv1);              // (arrived during the previous slice)
            const unsigned g2 = (unsigned)__builtin_amdgcn_readfirstlane((int)gv2);
            pnext.pm = mask_vec(pnext.d);
            dv1 = desc_vec(g2);
            gv2 = group_vec(gq + 3u < last ? gq + 3u : last);
            const uint32_t row = slice_of(pcur.g, pw) * kSliceRows + lane;
            const uint32_t kind = pcur.d.x >> 16, len = pcur.d.x & 0xFFFFu;
            {                                                     // (no slice without rows: build_slice_desc -- a path that requests
                                                                  // nothing would make every wait of the loop a wait for everything)
                double upre = 0.0;
                if (NDOT >= 1) upre = a.u[row];
                if (pcur.d.y != cy || pcur.d.z != cz) {
                    cy = pcur.d.y; cz = pcur.d.z;
                    o8 = *(const BICG_KCONST sell_i8 *)(a.sell.uoff8 + cy);
                    const BICG_KCONST double *uv = (const BICG_KCONST double *)(a.sell.uval + cz);
#pragma unroll
                    for (int e = 0; e < 8; ++e) lv[e] = uv[e];
                }
                const uint32_t boff = row << 3;
                const double sum = kind == (uint32_t)kSliceMasked ? sell_list_switch<true>(len, x, boff, o8, lv, pcur.pm, yp, yv)
                                                                  : sell_list_switch<false>(len, x, boff, o8, lv, 0u, yp, yv);
                const double yi = 0.0 + sum;                      // y = 0 ; y += tempy  (src/matrix.c:434-437, 514)
                yp = a.y + row; yv = yi;
                if (NDOT >= 1) {
                    acc[0] += upre * yi;
                    if (NDOT == 2) acc[NDOT >= 2 ? 1 : 0] += yi * yi;
                    if (NDOT == 3) acc[NDOT >= 2 ? 1 : 0] += upre * upre;
                }
            }
            pcur = pnext; g1 = g2;
        }
        *yp = yv;
    }
    for (unsigned gq = gfirst; gq < gend && !(PRE && !OFFD && lean); gq += LL ? nblocks : 1u) {
        const unsigned gi = (a.reverse && !LL) ? gfirst + (gend - 1u - gq) : gq;      // a reversed product walks its groups backwards too
        uint32_t row;
        bool live;
        if (LAY == LAY_JAGW) sell_stage_window(a, a.glist ? a.glist[gi] : gi, dyn_lds);
        SellPre pnext = pcur;
        unsigned g2 = 0u;
        if (PRE && pre_on) {
            pnext.g = g1; pnext.d = first_lane(dv1);              // (arrived during the previous slice)
            g2 = (unsigned)__builtin_amdgcn_readfirstlane((int)gv2);
            pnext.pm = gq + 1u < gend ? mask_vec(pnext.d) : 0u;
            if (gq + 2u < gend) dv1 = desc_vec(g2);
            if (gq + 3u < gend) gv2 = group_vec(gq + 3u);
        }
        // the dot operand of this lane's row is requested BEFORE the row product (one load in front of the product's
        // batches; after it, it was a dependent round trip at the very end of every workgroup)
        double upre = 0.0;
        const uint32_t rguess = ((PRE && pre_on) ? pcur.g : (a.glist ? a.glist[gi] : gi)) * kGroupRows + threadIdx.x;
        if (NDOT >= 1 && rguess < a.nrows) upre = a.u[rguess];
        const double yi = sell_row<OFFD, NT, LAY, LL>(a, gi, done, row, live, ll_failed, dyn_lds, PRE && pre_on, pcur);
        if (PRE && pre_on) { pcur = pnext; g1 = g2; }
        if (live && !done) a.y[row] = yi;
        if (NDOT >= 1 && live) {
            const double ume = row == rguess ? upre : a.u[row];
            acc[0] += ume * yi;
            if (NDOT == 2) acc[NDOT >= 2 ? 1 : 0] += yi * yi;
            if (NDOT == 3) acc[NDOT >= 2 ? 1 : 0] += ume * ume;
        }
    }
    if (LL && ll_failed) { a.S->comm_error = 1; a.S->done = 1; }
    if (NDOT > 0 && !done) {
        if constexpr (MODE == RED_WAVE) wave_publish<(NDOT > 0 ? NDOT : 1)>(acc, a.red.partial, a.red.slot_base + slot);
        else if constexpr (MODE == RED_HAND) hand_publish<(NDOT > 0 ? NDOT : 1)>(acc, a.S, a.red, a.red.slot_base + slot, sm, a.red.slot_base + bid);
        else reduce_publish<(NDOT > 0 ? NDOT : 1), MODE == RED_TICKET_HEAVY>(acc, a.S, a.red, a.red.slot_base + slot, sm, a.red.slot_base + bid);
    }
}

// ------------------------------------------------------------------------------------------
// SpMV + element-wise phase in ONE launch: the pipelined iteration as two kernels
//   EPI = 1:  v = A z ; then phase 2 on the workgroup's own rows (x, r, w, five dots; src/solver.c:366-380)
//   EPI = 2:  t = A w ; then phase 1 of the NEXT iteration (p, s, z, q, y, two dots; src/solver.c:352-364)
// The phase needs, per row, only values of that row -- among them the y_i this lane has just
// computed -- so it rides in the SpMV's epilogue: two launches per iteration instead of four, and the
// dot group the phase's scalars come from (produced by the previous launch) is summed by this
// launch's first workgroups while everybody streams the matrix; by the time a workgroup reaches its
// epilogue the totals are there. On a 200 k-row rank (1/8 of Transport) every launch boundary and
// every exposed reduction costs as much as the arithmetic, which is what this removes.
// The phase's expressions are those of FPipe1 / FPipe2, operation for operation; y lives in its own
// vector (a.epi.y) because w is this SpMV's input while the epilogue of EPI = 2 produces y.
// ------------------------------------------------------------------------------------------
template <int EPI, bool OFFD, bool NT, int LAY, bool LL>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) k_spmv_sell_epi(SpmvArgs a)
{
    constexpr int ND = EPI == 1 ? 5 : 2;
    const int done = a.S->done;
    __shared__ FinishLds fl;
    __shared__ Scal priv;
    unsigned bid = blockIdx.x, nblocks = gridDim.x;
    bool ll_failed = false;
    if (LL) {
        if (bid < a.ll.npush) { sell_halo_push(a, bid, done); return; }
        bid -= a.ll.npush; nblocks -= a.ll.npush;
    }
    // The open dot group. kShards DEDICATED workgroups in front of the row workgroups sum the shards (and,
    // peer-to-peer, the first of them hands the local sums to the other ranks) and leave; the first one also applies
    // the recurrence and writes the next scalar block. A workgroup with rows of its own would start them that much
    // later, and the launch ends with its slowest workgroup. Row workgroups apply privately at their epilogue.
    const unsigned nhelp = a.fin.seq && (a.fin.roles & FIN_SHARDS) ? (unsigned)kShards : 0u;
    if (bid < nhelp) {
        (void)finish_group(a.S, a.fin, a.fin.roles & (FIN_SHARDS | FIN_PUSH), bid, nhelp, fl, nullptr);
        if (bid == 0) {
            // ... applies the recurrence, writes the next scalar block, and hands the few scalars the phase needs to the
            // row workgroups as LL words (row kShards of the shard-total table): one small poll at their epilogue
            // instead of kShards x n totals, a reduction and the recurrence in every workgroup
            (void)finish_group(a.S, a.fin, FIN_APPLY, 0u, nhelp, fl, &priv);
        }
        return;
    }
    bid -= nhelp; nblocks -= nhelp;
    // staged by an earlier launch (or nothing to sum): row workgroup 0 publishes the scalar block
    const unsigned fin_bid = nhelp ? bid + 1u : bid;
    double acc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) acc[d] = 0.0;
    const Vecs &e = a.epi;
    bool have = false;
    int sdone = done;
    double alpha = 0.0, beta = 0.0, omega = 0.0;
#define EPI_SCALARS()                                                                                     \
    do {                                                                                                  \
        const Scal *sc_ = a.S;                                                                            \
        bool got_ = false;                                                                                \
        if (done) {                        /* converged before this launch: nothing is published, nothing changes */ \
            got_ = true; sdone = 1;                                                                       \
        } else if (a.fin.seq && nhelp) {   /* the scalars as published by helper workgroup 0 */           \
            if (threadIdx.x == 0) fl.missing = 0u;                                                        \
            __syncthreads();                                                                              \
            if (threadIdx.x < 4) {                                                                        \
                double v_;                                                                                \
                const llword *w_ = a.fin.shard + ((size_t)kShards * kRedSlots + threadIdx.x) * 2;         \
                if (a.fin.p2p.seq ? ll_wait_agent(w_, a.fin.seq, a.fin.p2p.timeout_ticks, &v_)            \
                                  : ll_try_agent(w_, a.fin.seq, a.fin.spin_ticks, &v_))                   \
                    fl.sums[threadIdx.x] = v_;                                                            \
                else atomicOr(&fl.missing, 1u);                                                           \
            }                                                                                             \
            __syncthreads();                                                                              \
            got_ = fl.missing == 0u;                                                                      \
            if (got_) { alpha = fl.sums[0]; beta = fl.sums[1]; omega = fl.sums[2]; sdone = fl.sums[3] != 0.0 ? 1 : 0; } \
            __syncthreads();                                                                              \
        }                                                                                                 \
        if (!got_) {                       /* staged earlier, nothing open, or helper 0 is late: apply here */ \
            if (a.fin.seq) sc_ = finish_group(a.S, a.fin, FIN_APPLY, fin_bid, nblocks, fl, &priv);        \
            sdone = sc_->done; alpha = sc_->alpha; beta = sc_->beta; omega = sc_->omega;                  \
        }                                                                                                 \
        have = true;                                                                                      \
    } while (0)
    unsigned slot = bid;
    for (unsigned gi0 = bid; gi0 < a.nlist; gi0 += nblocks) {
        const unsigned gi = (a.reverse && !LL) ? a.nlist - 1u - gi0 : gi0;
        if (nblocks == a.nlist) slot = gi;
        uint32_t row;
        bool live;
        if (LAY == LAY_JAGW) sell_stage_window(a, a.glist ? a.glist[gi] : gi, dyn_lds);
        const double yi = sell_row<OFFD, NT, LAY, LL, 8>(a, gi, done, row, live, ll_failed, dyn_lds);
        if (live && !done) a.y[row] = yi;
        // The phase's inputs (values of this lane's own row) are requested right after the row product and BEFORE the
        // scalars are waited for: their round trip and the scalar poll's are one. (Requested before the row product
        // they sit in front of its loads -- loads return in issue order -- and delay every batch: BICG_EPI_EARLY.)
        const uint32_t rr_ = live ? row : 0u;
        double in0, in1, in2, in3, in4, in5, in6 = 0.0, in7 = 0.0;
        if (EPI == 1) { in0 = e.r[rr_]; in1 = e.y[rr_]; in2 = e.x[rr_]; in3 = e.p[rr_]; in4 = e.t[rr_]; in5 = e.rh[rr_]; in6 = e.s[rr_]; in7 = e.z[rr_]; }
        else { in0 = e.r[rr_]; in1 = e.w[rr_]; in2 = e.s[rr_]; in3 = e.z[rr_]; in4 = e.p[rr_]; in5 = e.v[rr_]; }
        if (!have) EPI_SCALARS();
        if (EPI == 1) {
            const double q = in0, y = in1, x0 = in2, p0 = in3, t0 = in4, h = in5, s0 = in6, z0 = in7;
            if (live && !sdone) {
                double xx = x0 + alpha * p0;
                xx = xx + omega * q;
                e.x[row] = xx;
                const double rr = q + (-omega) * y;
                e.r[row] = rr;
                const double tt = t0 + (-alpha) * yi;
                const double ww = y + (-omega) * tt;
                e.w[row] = ww;
                acc[0] += rr * rr; acc[1] += h * rr; acc[2] += h * ww; acc[3] += h * s0; acc[4] += h * z0;
            }
        } else {
            const double r0 = in0, w0 = in1, s0 = in2, z0 = in3, p0 = in4, v0 = in5;
            if (live && !sdone) {
                e.p[row] = recur3<double>(p0, s0, r0, omega, beta);
                const double s1 = recur3<double>(s0, z0, w0, omega, beta);
                const double z1 = recur3<double>(z0, v0, yi, omega, beta);
                e.s[row] = s1; e.z[row] = z1;
                const double q = r0 + (-alpha) * s1;
                const double y = w0 + (-alpha) * z1;
                e.r[row] = q; e.y[row] = y;
                acc[0] += q * y; acc[1] += y * y;
            }
        }
    }
    if (!have && fin_bid == 0) EPI_SCALARS();  // the publishing workgroup writes the scalar block even without rows
#undef EPI_SCALARS
    if (LL && ll_failed) { a.S->comm_error = 1; a.S->done = 1; }
    if (have && !sdone) wave_publish<ND>(acc, a.red.partial, a.red.slot_base + slot);
    else if (!have && !done) wave_publish<ND>(acc, a.red.partial, a.red.slot_base + slot);
}

static inline int sell_layout(const SellDev &d)
{
    if (d.win_slots) return LAY_JAGW;
    if (!d.jag && d.vbase) return d.col16 ? LAY_PAD16C : LAY_PAD32C;
    return (d.jag ? LAY_JAG32 : LAY_PAD32) + (d.col16 ? 1 : 0);
}

// One sliced-ELL layout's instantiations (96 SpMV kernels + 12 with an epilogue): a translation unit each. The three templates
// below are explicitly instantiated for one layout by bicg_spmv_sell_lay.hip and declared `extern template` where they are
// called (bicg_spmv_sell.hip), so no other unit instantiates a sliced-ELL kernel.
#define SELL_LAY_ARGS const SpmvArgs &, int, bool, hipStream_t, hipEvent_t, hipEvent_t, bool
template <int LAY>
bool sell_launch_layout(const SpmvArgs &a, int ndot, bool with_offd, hipStream_t st, hipEvent_t e0, hipEvent_t e1, bool fused_halo)
{
    if (a.nlist == 0 && !(fused_halo && a.ll.npush > 0)) return false;
    dim3 g(sell_grid(a.nlist, a.groups_per_wg) + (fused_halo ? a.ll.npush : 0u)), b(kBlock);
    const unsigned lds = LAY == LAY_JAGW ? a.sell.win_slots * (unsigned)sizeof(double) : 0u;
#define SELL_MODE(ND, OF, LLV, MD)                                                                 \
    do {                                                                                           \
        if (nt) launch_timed_lds(k_spmv_sell<ND, OF, true, LAY, LLV, MD>, g, b, lds, st, e0, e1, a);   \
        else launch_timed_lds(k_spmv_sell<ND, OF, false, LAY, LLV, MD>, g, b, lds, st, e0, e1, a);     \
    } while (0)
#define SELL_CASE(ND, OF, LLV)                                                                     \
    do {                                                                                           \
        const bool nt = a.nt != 0;                                                                 \
        const int mode = red_mode(a.red, a.fin, (ND) > 0);                                         \
        constexpr int HV = (ND) > 0 ? RED_TICKET_HEAVY : RED_TICKET;                               \
        if (mode == RED_HAND) {                                                                    \
            /* hand-over: the padded 16-bit layout's products with dots, one rank (no offd, no exchange inside) */ \
            if constexpr ((ND) > 0 && !(OF) && !(LLV) && LAY == LAY_PAD16) SELL_MODE(ND, OF, LLV, RED_HAND); \
            else { fprintf(stderr, "ERROR: bicgstab_hip: no hand-over form of this sliced-ELL product\n"); abort(); } \
        } else if (mode == RED_WAVE) SELL_MODE(ND, OF, LLV, RED_WAVE);                             \
        else if (mode == RED_TICKET_HEAVY) SELL_MODE(ND, OF, LLV, HV);                             \
        else SELL_MODE(ND, OF, LLV, RED_TICKET);                                                   \
    } while (0)
    if (fused_halo) {
        if (ndot == 0) SELL_CASE(0, true, true); else if (ndot == 1) SELL_CASE(1, true, true); else if (ndot == 2) SELL_CASE(2, true, true); else SELL_CASE(3, true, true);
    } else if (with_offd) {
        if (ndot == 0) SELL_CASE(0, true, false); else if (ndot == 1) SELL_CASE(1, true, false); else if (ndot == 2) SELL_CASE(2, true, false); else SELL_CASE(3, true, false);
    } else {
        if (ndot == 0) SELL_CASE(0, false, false); else if (ndot == 1) SELL_CASE(1, false, false); else if (ndot == 2) SELL_CASE(2, false, false); else SELL_CASE(3, false, false);
    }
#undef SELL_CASE
#undef SELL_MODE
    return true;
}

template <int LAY>
bool sell_epi_launch_layout(const SpmvArgs &a, int epi, bool with_offd, hipStream_t st, hipEvent_t e0, hipEvent_t e1, bool fused_halo)
{
    if (a.nlist == 0 && !(fused_halo && a.ll.npush > 0)) return false;
    const unsigned nhelp = a.fin.seq && (a.fin.roles & FIN_SHARDS) ? (unsigned)kShards : 0u;      // dedicated shard summers
    dim3 g(sell_grid(a.nlist, a.groups_per_wg) + (fused_halo ? a.ll.npush : 0u) + nhelp), b(kBlock);
    const bool nt = a.nt != 0;
    const unsigned lds = LAY == LAY_JAGW ? a.sell.win_slots * (unsigned)sizeof(double) : 0u;
#define EPI_CASE(EP, OF, LLV)                                                                      \
    do {                                                                                           \
        if (nt) launch_timed_lds(k_spmv_sell_epi<EP, OF, true, LAY, LLV>, g, b, lds, st, e0, e1, a);   \
        else launch_timed_lds(k_spmv_sell_epi<EP, OF, false, LAY, LLV>, g, b, lds, st, e0, e1, a);     \
    } while (0)
    if (epi == 1) {
        if (fused_halo) EPI_CASE(1, true, true); else if (with_offd) EPI_CASE(1, true, false); else EPI_CASE(1, false, false);
    } else {
        if (fused_halo) EPI_CASE(2, true, true); else if (with_offd) EPI_CASE(2, true, false); else EPI_CASE(2, false, false);
    }
#undef EPI_CASE
    return true;
}

// ---- code objects loaded at set-up, not at the first launch -------------------------------------------------------------
// The runtime loads a translation unit's code object when the first of its kernels is looked up: 10-80 ms for a unit with a few
// hundred sliced-ELL instantiations, paid in the MIDDLE of a solve whenever a kernel of a unit not used so far comes up (the
// first replacement step of pipe_bicgstab_rr, the first product with two dots, a leg of bench.py that follows a leg with
// another layout -- the "queue stall" of rounds 2-3). bicg_create looks up one kernel of every unit its context can launch
// from; BICG_PRELOAD=0 leaves the loading to the first launch.
template <int LAY> void preload_layout()
{
    hipFuncAttributes at;
    (void)hipFuncGetAttributes(&at, reinterpret_cast<const void *>(k_spmv_sell<0, false, false, LAY, false, RED_TICKET>));
    (void)hipGetLastError();
}

}  // namespace bicg
