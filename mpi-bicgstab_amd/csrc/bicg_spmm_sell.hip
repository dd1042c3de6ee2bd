// bicg_spmm_sell.hip -- the fall-back products over several vectors at once on the sliced-ELL copy: row-major X (k_spmm_sell)
// and the windowed form (k_spmm_win), with the column sums and the two transposes they need. bicg_spmm.hip and
// bicg_spmm_jag.hip hold the pipelined forms that most matrices get.
#include "bicg_spmv_sell.h"   // sell_layout, i16x4, dyn_lds

namespace bicg {

// ------------------------------------------------------------------------------------------
// Sliced-ELL SpMM: Y_j = (A + sigma_j I) X_j for kSpmmCols vectors at once -- the verification loop of
// the reference's shifted driver (src/test_shifted.c:129-154: one SpMV per shift, A read nsig
// times) with A read ONCE. X is held row-major, kSpmmCols values per row = one 128-byte line.
// A wavefront works on 8 rows at a time, 8 lanes per row, each lane owning TWO columns: the load of
// the X values of one matrix entry is then one instruction over 8 fully used lines (a first version
// with lane = row touched 64 lines per instruction, 16 bytes of each: 0.56 ms on Transport, bound by
// the vector L1's tag rate). val / col are read from memory once per wavefront, lane = row, fully
// coalesced, into LDS; the 8 lanes of a row then take them from there with broadcast reads (a
// version in which they loaded the same word from memory issued 8 x the load instructions of the
// SpMV: 469 us). Every column of every row is accumulated in stored order like mult() (reference
// src/matrix.c:506-515), so each Y_j is bit-identical to the SpMV of that column. With b given,
// || b - Y_j ||^2 is fused (workgroup sums go to partial[wg][col], k_colsum adds them in a fixed
// order) and Y is never written.
// ------------------------------------------------------------------------------------------
template <int LAY, bool OFFD>
__global__ void __launch_bounds__(kBlock) k_spmm_sell(SpmmArgs a)
{
    // LAY: the block's sliced-ELL layout (SellLayout). Padded slices: entry k of lane l at base + k * 64 + l. Jagged slices
    // (ragged rows): step k holds the entries of the rows longer than k only -- the staging pass finds a lane's entry with
    // a ballot like sell_row does. With x windows the stored 16-bit value is an LDS slot of the SpMV's window: the column
    // comes back through the group's runs. Rows dealt to the lanes by decreasing length (SellDev::perm): the lane -> row
    // map of the slice goes through LDS.
    constexpr bool WIN = LAY == LAY_JAGW, C16 = (LAY & 1) != 0 || WIN, JAG = LAY >= LAY_JAG32;
    constexpr int NB = kSpmmCols;
    constexpr int KC = 16;                                   // matrix entries per row staged in LDS at a time
    static_assert(NB == 16, "8 lanes per row x 2 columns per lane");
    struct Ent { double v; uint32_t off, pad; };            // value and byte offset of the row of X it multiplies
    __shared__ Ent se[kBlock / 64][KC][kSliceRows];          // this wavefront's slice, entry-major: read from memory ONCE,
                                                             // lane = row, fully coalesced
    __shared__ double sm[(kBlock / 64) * NB];
    __shared__ uint32_t rowmap[kBlock];                      // row of slice lane l (identity without SellDev::perm)
    __shared__ uint2 wruns[WIN ? 64 : 1];                    // the group's window runs (WIN)
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned sub = lane >> 3, cp = lane & 7u;          // row within an 8-row batch, column pair
    // XCD-contiguous mapping: workgroup b runs on XCD b % 8 (observed placement, used for speed only), so
    // giving XCD x the x-th eighth of the row groups makes one L2 fetch (almost) every line of X once
    // instead of all eight fetching all of it (16 vectors: 8 x 205 MB on Transport)
    unsigned g = blockIdx.x;
    if (a.xcd_map) {
        const unsigned per = (a.ngroups + 7u) / 8u;
        g = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    }
    double acc0 = 0.0, acc1 = 0.0;
    unsigned nwr = 0;
    if (g < a.ngroups) {
        rowmap[tid] = g * kGroupRows + ((WIN && a.sell.perm) ? (uint32_t)a.sell.perm[(size_t)g * kGroupRows + tid] : tid);
        if (WIN) {
            const uint32_t r0 = a.sell.win_ptr[g];
            nwr = a.sell.win_ptr[g + 1] - r0;
            if (tid < nwr && tid < 64u) wruns[tid] = a.sell.win_runs[r0 + tid];
        }
    }
    __syncthreads();
    if (g < a.ngroups) {
        const uint32_t slice = g * (kGroupRows / kSliceRows) + wave;      // this wavefront's 64 rows
        uint32_t base = 0u, len = 0u, base16 = 0u;
        if (slice * kSliceRows < a.nrows) {
            base = a.sell.slice_base[slice]; len = a.sell.slice_len[slice];
            if (C16 && !JAG) base16 = a.sell.slice_base16[slice];
        }
        const double sg0 = a.sigma ? a.sigma[2 * cp] : 0.0, sg1 = a.sigma ? a.sigma[2 * cp + 1] : 0.0;
        const char *const xb = reinterpret_cast<const char *>(a.xt) + 16u * cp;     // this lane's two columns
        // stage role: lane = row of the slice
        const uint32_t srow = rowmap[wave * kSliceRows + lane];
        const uint32_t srb = srow < a.nrows ? srow : 0u;
        const uint32_t slen_me = srow < a.nrows ? a.dptr[srow + 1] - a.dptr[srow] : 0u;
        uint32_t jpos = base;                                // jagged: first entry of the current step (wave-uniform)
        // shortest row of the slice: entries below it need no per-row test (the usual case is all of them)
        uint32_t minlen = slen_me;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(minlen, off, 64); minlen = o < minlen ? o : minlen; }
        // compute role: 8 batches of 8 rows; this lane's row in batch bt is bt * 8 + sub
        double s0[kSliceRows / 8], s1[kSliceRows / 8];
        uint32_t mylen[kSliceRows / 8];
#pragma unroll
        for (int bt = 0; bt < kSliceRows / 8; ++bt) {
            const uint32_t row = rowmap[wave * kSliceRows + bt * 8 + sub];
            s0[bt] = 0.0; s1[bt] = 0.0;
            mylen[bt] = row < a.nrows ? a.dptr[row + 1] - a.dptr[row] : 0u;
        }
        for (uint32_t k0 = 0; k0 < len; k0 += KC) {
            const uint32_t kn = len - k0 < (uint32_t)KC ? len - k0 : (uint32_t)KC;
            // ---- stage: coalesced loads, 512 bytes of val per instruction
            if (JAG) {
                for (uint32_t e = 0; e < kn; ++e) {
                    const bool mine = k0 + e < slen_me;
                    const unsigned long long m = __ballot(mine);
                    const uint32_t j = jpos + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    jpos += (uint32_t)__builtin_popcountll(m);
                    uint32_t colv = srb;
                    double vv = 0.0;
                    if (mine) {
                        vv = a.sell.val[j];
                        if (WIN) {
                            const uint32_t slot = reinterpret_cast<const unsigned short *>(a.sell.col16)[j];
                            unsigned r = 0;
                            while (r + 1 < nwr && (wruns[r + 1].y >> 16) <= slot) ++r;
                            colv = wruns[r].x + (slot - (wruns[r].y >> 16));
                        } else if (C16) {
                            colv = srb + (uint32_t)(int)a.sell.col16[j];
                        } else {
                            colv = a.sell.col[j];
                        }
                    }
                    se[wave][e][lane].off = colv * (NB * 8u);
                    se[wave][e][lane].v = vv;
                }
            } else if (C16) {
                for (uint32_t q = 0; 4 * q < kn; ++q) {
                    const i16x4 dq = *(reinterpret_cast<const i16x4 *>(a.sell.col16) + ((size_t)base16 / 4 + (size_t)(k0 / 4 + q) * kSliceRows + lane));
                    se[wave][4 * q + 0][lane].off = (srb + (int)dq.x) * (NB * 8u); se[wave][4 * q + 1][lane].off = (srb + (int)dq.y) * (NB * 8u);
                    se[wave][4 * q + 2][lane].off = (srb + (int)dq.z) * (NB * 8u); se[wave][4 * q + 3][lane].off = (srb + (int)dq.w) * (NB * 8u);
                }
            }
            for (uint32_t e = 0; !JAG && e < kn; ++e) {
                const uint32_t j = base + (k0 + e) * kSliceRows + lane;
                if (!C16) se[wave][e][lane].off = a.sell.col[j] * (NB * 8u);
                se[wave][e][lane].v = a.sell.val[j];
            }
            __builtin_amdgcn_wave_barrier();      // same wavefront writes and reads: program order of its LDS operations is enough
            // ---- multiply: per batch and entry one broadcast LDS read of {val, offset} and ONE load of 8 full lines
            // of X; the 8 batches are independent, their loads are in flight together. Entries below the slice's
            // shortest row take the path without per-row tests (the kernel is bound by instruction issue).
            const uint32_t nfast = k0 >= minlen ? 0u : (minlen - k0 < kn ? minlen - k0 : kn);
            for (uint32_t e = 0; e < nfast; ++e) {
                f64x2 x[kSliceRows / 8];
                double v[kSliceRows / 8];
#pragma unroll
                for (int bt = 0; bt < kSliceRows / 8; ++bt) {
                    const Ent en = se[wave][e][bt * 8 + sub];
                    v[bt] = en.v;
                    x[bt] = *reinterpret_cast<const f64x2 *>(xb + en.off);
                }
#pragma unroll
                for (int bt = 0; bt < kSliceRows / 8; ++bt) { s0[bt] += v[bt] * x[bt].x; s1[bt] += v[bt] * x[bt].y; }     // stored order
            }
            for (uint32_t e = nfast; e < kn; ++e) {
#pragma unroll
                for (int bt = 0; bt < kSliceRows / 8; ++bt) {
                    const Ent en = se[wave][e][bt * 8 + sub];
                    const f64x2 x = *reinterpret_cast<const f64x2 *>(xb + en.off);
                    if (k0 + e < mylen[bt]) { s0[bt] += en.v * x.x; s1[bt] += en.v * x.y; }                                 // padding never added
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
#pragma unroll
        for (int bt = 0; bt < kSliceRows / 8; ++bt) {
            const uint32_t row = rowmap[wave * kSliceRows + bt * 8 + sub];
            const bool live = row < a.nrows;
            double y0 = 0.0 + s0[bt], y1 = 0.0 + s1[bt];                  // y = 0 ; y += tempy  (src/matrix.c:434-437, 514)
            if (OFFD && live) {
                double o0 = 0.0, o1 = 0.0;
                for (uint32_t k = a.offd.ptr[row]; k < a.offd.ptr[row + 1]; ++k) {
                    const double v = a.offd.val[k];
                    const f64x2 x = *reinterpret_cast<const f64x2 *>(a.xt + (size_t)a.offd.col[k] * NB + 2 * cp);
                    o0 += v * x.x; o1 += v * x.y;
                }
                y0 += o0; y1 += o1;                                       // second mult() call, src/matrix.c:440
            }
            if (live) {
                if (a.sigma) {
                    const f64x2 x = *reinterpret_cast<const f64x2 *>(a.xt + (size_t)row * NB + 2 * cp);
                    y0 += sg0 * x.x; y1 += sg1 * x.y;                     // += sigma_j x_j (src/test_shifted.c:133)
                }
                if (a.yt) { f64x2 t; t.x = y0; t.y = y1; *reinterpret_cast<f64x2 *>(a.yt + (size_t)row * NB + 2 * cp) = t; }
                if (a.b) {
                    const double bi = a.b[row];
                    const double d0 = (bi + (-1.0) * y0) - 0.0, d1 = (bi + (-1.0) * y1) - 0.0;
                    acc0 += d0 * d0; acc1 += d1 * d1;
                }
            }
        }
    }
    if (a.b) {
        // lanes with the same column pair sit 8 apart: fold the 8 row positions, then the 4 wavefronts
#pragma unroll
        for (int off = 32; off >= 8; off >>= 1) { acc0 += __shfl_down(acc0, off, 64); acc1 += __shfl_down(acc1, off, 64); }
        if (lane < 8) { sm[wave * NB + 2 * lane] = acc0; sm[wave * NB + 2 * lane + 1] = acc1; }
        __syncthreads();
        if (tid < NB) {
            double t = sm[tid];
            for (int w = 1; w < kBlock / 64; ++w) t += sm[w * NB + tid];
            a.partial[(size_t)blockIdx.x * NB + tid] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------
// Windowed SpMM (round 4): the same product with X read ONCE and no layout change. The row-major kernel above pulls a
// 128-byte line of X through the vector L1 for every matrix entry (2.4 GB per launch on Transport, 1.6 x the algorithmic
// bytes from memory, + 97 us of transposes). Here a workgroup owns a 256-row group like the SpMV does (lane = row), stages the
// x values the group touches for NV vectors at a time in LDS -- straight from the shift-major vectors, every run of
// consecutive columns one coalesced copy per vector, exactly what sell_stage_window does for one vector -- and then walks
// its rows once per pass: every matrix entry is loaded once per NV vectors and multiplies NV LDS reads (consecutive lanes
// read consecutive slots: conflict-free). Y goes back shift-major. Where the columns come from:
//   MODE 0  padded slices with 16-bit offsets (banded / stencil-like matrices): the offsets fall into <= 4 clusters (struct
//           FusedWindow), cluster k of every group is the run [g0 + lo_k, g0 + 255 + hi_k], slot = thread + offset + bias_k;
//   MODE 1  jagged slices with x windows (ragged rows): the stored 16-bit value IS the slot, the runs are the SpMV's.
// Per row and vector the sum runs in stored order like mult() (reference src/matrix.c:506-515): every column is bit-identical
// to bicg_spmv of that vector. NV = 8 on Transport (79 KB of LDS, two workgroups per CU); the first 16 entries of every row
// stay in registers across the passes, so the matrix is read once per launch whatever NV.
// ------------------------------------------------------------------------------------------
template <int MODE, bool OFFD, int NV>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 4))) k_spmm_win(SpmmArgs a)      // (the LDS window allows two workgroups per CU)
{
    constexpr bool WIN = MODE == 1;
    constexpr int U = 8;
    __shared__ double sm[(kBlock / 64) * NV];
    double *const win = dyn_lds;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    unsigned g = blockIdx.x;
    if (a.xcd_map) {
        const unsigned per = (a.ngroups + 7u) / 8u;
        g = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    }
    if (a.b && tid < (unsigned)kSpmmCols && (g >= a.ngroups || (int)tid >= a.nvec)) a.partial[(size_t)blockIdx.x * kSpmmCols + tid] = 0.0;
    if (g >= a.ngroups) return;                               // (grid padded to a multiple of 8: workgroup-uniform)
    const unsigned W = a.wslots;
    const uint32_t g0 = g * kGroupRows;
    const uint32_t row = g0 + ((WIN && a.sell.perm) ? (uint32_t)a.sell.perm[(size_t)g0 + tid] : tid);
    const uint32_t slice = g * (kGroupRows / kSliceRows) + wave;
    const bool live = row < a.nrows;
    uint32_t base = 0u, len = 0u, base16 = 0u;
    if (slice * kSliceRows < a.nrows) {
        base = a.sell.slice_base[slice]; len = a.sell.slice_len[slice];
        if (!WIN) base16 = a.sell.slice_base16[slice];
    }
    const uint32_t mylen = live ? a.dptr[row + 1] - a.dptr[row] : 0u;
    uint32_t oa = 0u, ob = 0u;
    if (OFFD && live) { oa = a.offd.ptr[row]; ob = a.offd.ptr[row + 1]; }
    const double bi = (a.b && live) ? a.b[row] : 0.0;
    const unsigned short *const slots16 = reinterpret_cast<const unsigned short *>(a.sell.col16);
    __shared__ uint2 wruns[WIN ? 64 : 1];                    // the group's window runs (spmm_possible: at most 64)
    unsigned nwr = 0;
    // (round 6) LIST: the group's window is a list of its distinct columns (SellDev::win_list, the layout k_spmv_jagl stages from):
    // slot s = position in the list, column = the group's first row + a 16-bit distance -- no runs, any number of them
    const bool LIST = WIN && a.sell.win_list != nullptr;
    const uint32_t lbase = LIST ? a.sell.win_lptr[g] : 0u, ltotal = LIST ? a.sell.win_ltotal[g] : 0u;
    if (WIN && !LIST) {
        const uint32_t r0 = a.sell.win_ptr[g];
        nwr = a.sell.win_ptr[g + 1] - r0;
        if (tid < nwr && tid < 64u) wruns[tid] = a.sell.win_runs[r0 + tid];
    }

    // ---- the head of the row -- its first K entries, all of it for most matrices -- is loaded ONCE and kept in registers for
    // every pass (value, LDS slot, "counts" bit): the matrix is then read once per launch, not once per NV vectors
    constexpr int K = 16;
    double hv[K];
    unsigned hs[K];
    unsigned hon = 0u;
    uint32_t pos = base;                                      // jagged: first entry of step k (wave-uniform), as in sell_row
    auto slot_of = [&](int d) -> unsigned {                   // padded layout: slot = thread + distance + bias of the distance's cluster
        int bias = a.cl.bias[0];
        if (a.cl.ncl > 1 && d >= a.cl.lo[1]) bias = a.cl.bias[1];
        if (a.cl.ncl > 2 && d >= a.cl.lo[2]) bias = a.cl.bias[2];
        if (a.cl.ncl > 3 && d >= a.cl.lo[3]) bias = a.cl.bias[3];
        return (unsigned)((int)tid + d + bias);               // padding: distance 0, the row's own column
    };
    const i16x4 *const q16 = reinterpret_cast<const i16x4 *>(a.sell.col16) + ((size_t)base16 / 4 + lane);
    if (a.dbg & 4) {
#pragma unroll
        for (int e = 0; e < K; ++e) { hs[e] = tid; hv[e] = 1.0; hon |= 1u << e; }
    } else if (WIN) {
#pragma unroll
        for (int e = 0; e < K; ++e) {
            hs[e] = 0u; hv[e] = 0.0;
            if ((uint32_t)e < len) {                          // wave-uniform
                const bool mine = (uint32_t)e < mylen;
                const unsigned long long m = __ballot(mine);
                const uint32_t j = pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                pos += (uint32_t)__builtin_popcountll(m);
                if (mine) { hs[e] = slots16[j]; hv[e] = a.sell.val[j]; hon |= 1u << e; }
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            i16x4 dq = (i16x4)(0);
            if ((uint32_t)(4 * q) < len) dq = q16[(size_t)q * kSliceRows];        // wave-uniform test; the quad is padded
            hs[4 * q + 0] = slot_of(dq.x); hs[4 * q + 1] = slot_of(dq.y); hs[4 * q + 2] = slot_of(dq.z); hs[4 * q + 3] = slot_of(dq.w);
        }
#pragma unroll
        for (int e = 0; e < K; ++e) {
            hv[e] = (uint32_t)e < len ? a.sell.val[base + (uint32_t)e * kSliceRows + lane] : 0.0;
            if ((uint32_t)e < mylen) hon |= 1u << e;
        }
    }
    const uint32_t pos_tail = pos;

    for (int v0 = 0; v0 < a.nvec; v0 += NV) {
        const int nv = a.nvec - v0 < NV ? a.nvec - v0 : NV;
        __syncthreads();                                      // the previous pass has finished reading the window (and sm)
        // ---- stage the group's window of vectors v0 .. v0 + nv - 1: JB slots per thread and round, all their NV values
        // requested before the first is stored (one dependent round trip per run and vector: 743 us per launch on Transport;
        // one slot per round: 430 us)
        constexpr int JB = 40 / NV;                           // Transport's 1 240 slots in ONE round: two waves per SIMD hide no second trip
        for (unsigned s0 = 0; s0 < W; s0 += JB * kBlock) {
            int c[JB];                                        // column of the slot; -1: unused slot / clipped by the matrix boundary
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                const unsigned sl = s0 + (unsigned)j * kBlock + tid;
                c[j] = -1;
                if (sl < W) {
                    if (LIST) {
                        if (sl < ltotal) {
                            const uint32_t word = a.sell.win_list[lbase + (sl >> 9) * (unsigned)kGroupRows + (sl & 255u)];
                            c[j] = (int)g0 + (int)(short)((sl & 256u) ? word >> 16 : word & 0xFFFFu);
                        }
                    } else if (WIN) {
                        unsigned r = 0;
                        while (r + 1 < nwr && (wruns[r + 1].y >> 16) <= sl) ++r;      // runs are few and ordered by slot
                        const unsigned off = sl - (wruns[r].y >> 16);
                        if (nwr && off < (wruns[r].y & 0xFFFFu)) c[j] = (int)(wruns[r].x + off);
                    } else {
                        int k = 0;
                        if (a.cl.ncl > 1 && (int)sl >= a.cl.bias[1] + a.cl.lo[1]) k = 1;
                        if (a.cl.ncl > 2 && (int)sl >= a.cl.bias[2] + a.cl.lo[2]) k = 2;
                        if (a.cl.ncl > 3 && (int)sl >= a.cl.bias[3] + a.cl.lo[3]) k = 3;
                        const int bk = k == 0 ? a.cl.bias[0] : k == 1 ? a.cl.bias[1] : k == 2 ? a.cl.bias[2] : a.cl.bias[3];
                        const int cc = (int)g0 + (int)sl - bk;                      // slot = (column - g0) + bias_k
                        if (cc >= 0 && cc < (int)a.nrows) c[j] = cc;
                    }
                }
            }
            double t[JB][NV];
#pragma unroll
            for (int j = 0; j < JB; ++j) {
#pragma unroll
                for (int v = 0; v < NV; ++v) t[j][v] = (c[j] >= 0 && v < nv && !(a.dbg & 1)) ? a.xs[(size_t)(v0 + v) * a.vstride + (unsigned)c[j]] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                const unsigned sl = s0 + (unsigned)j * kBlock + tid;
                if (sl < W) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) win[(unsigned)v * W + sl] = t[j][v];
                }
            }
        }
        __syncthreads();
        // ---- the rows, NV sums per lane: the head from registers, whatever follows streamed
        double acc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = 0.0;
        // Straight-line code per half of the head: with a (wave-uniform) branch around every entry the compiler waited for each
        // LDS read before issuing the next -- 120 exposed LDS latencies per pass and lane, 412 us per launch on Transport. Entries
        // past the slice's length read slot 0 and are never added.
        // (the slots are made opaque once per pass: otherwise the 16 x NV LDS addresses slot + v W are hoisted out of the pass
        // loop as invariants and held in 128 registers)
#pragma unroll
        for (int e = 0; e < K; ++e) asm volatile("" : "+v"(hs[e]));
        auto half = [&](int e0) {
#pragma unroll
            for (int e = e0; e < e0 + K / 2; ++e) {
                double xr[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) xr[v] = win[(unsigned)v * W + hs[e]];
                const bool on = (hon >> e) & 1u;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const double t = acc[v] + hv[e] * xr[v];  // stored order; padding never added
                    acc[v] = on ? t : acc[v];
                }
                // (two entries = 16 reads in flight are enough; left alone the scheduler hoists all 64 of a half: 256 registers)
                if ((e & 1) == 1) __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (!(a.dbg & 2)) {
        half(0);
        if (len > (uint32_t)(K / 2)) half(K / 2);
        }
        pos = pos_tail;
        for (uint32_t k0 = K; k0 < len && !(a.dbg & 2); k0 += U) {
            double val[U];
            unsigned sl[U];
            bool on[U];
            if (WIN) {
#pragma unroll
                for (int e = 0; e < U; ++e) {
                    on[e] = k0 + e < mylen;
                    const unsigned long long m = __ballot(on[e]);
                    const uint32_t j = pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    pos += (uint32_t)__builtin_popcountll(m);
                    sl[e] = 0u; val[e] = 0.0;
                    if (on[e]) { sl[e] = slots16[j]; val[e] = a.sell.val[j]; }
                }
            } else {
#pragma unroll
                for (int q = 0; q < U / 4; ++q) {
                    i16x4 dq = (i16x4)(0);
                    if (k0 + 4 * q < len) dq = q16[(size_t)(k0 / 4 + q) * kSliceRows];
                    sl[4 * q + 0] = slot_of(dq.x); sl[4 * q + 1] = slot_of(dq.y); sl[4 * q + 2] = slot_of(dq.z); sl[4 * q + 3] = slot_of(dq.w);
                }
#pragma unroll
                for (int e = 0; e < U; ++e) {
                    val[e] = k0 + e < len ? a.sell.val[base + (k0 + e) * kSliceRows + lane] : 0.0;
                    on[e] = k0 + e < mylen;
                }
            }
#pragma unroll
            for (int e = 0; e < U; ++e) {
                double xr[NV];
#pragma unroll
                for (int v = 0; v < NV; ++v) xr[v] = win[(unsigned)v * W + sl[e]];
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const double t = acc[v] + val[e] * xr[v]; // stored order
                    acc[v] = on[e] ? t : acc[v];
                }
            }
        }
        double r2[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            r2[v] = 0.0;
            if (v < nv && live) {
                const double *xv = a.xs + (size_t)(v0 + v) * a.vstride;
                double y = 0.0 + acc[v];                      // y = 0 ; y += tempy  (src/matrix.c:434-437, 514)
                if (OFFD) {
                    double so = 0.0;
                    for (uint32_t k = oa; k < ob; ++k) so += a.offd.val[k] * xv[a.offd.col[k]];
                    y += so;                                  // second mult() call, src/matrix.c:440
                }
                // += sigma_j x_j (src/test_shifted.c:133); with clusters the row's own column is in the window (distance 0 is always
                // part of a cluster): no trip to memory at the end of the pass
                if (a.sigma) y += a.sigma[v0 + v] * (WIN ? xv[row] : win[(unsigned)v * W + slot_of(0)]);
                if (a.ys) a.ys[(size_t)(v0 + v) * a.vstride + row] = y;
                if (a.b) { const double dd = (bi + (-1.0) * y) - 0.0; r2[v] = dd * dd; }
            }
        }
        if (a.b) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const double t = wave_sum(r2[v]);
                if (lane == 0) sm[wave * NV + v] = t;
            }
            __syncthreads();
            if ((int)tid < nv) {
                double t = sm[tid];
                for (int w = 1; w < kBlock / 64; ++w) t += sm[w * NV + tid];
                a.partial[(size_t)blockIdx.x * kSpmmCols + v0 + tid] = t;
            }
        }
    }
}

// out[col] = sum over workgroups of partial[wg][col], fixed order; one workgroup per column
__global__ void __launch_bounds__(kBlock) k_colsum(const double *partial, unsigned nwg, double *out)
{
    constexpr int NB = kSpmmCols;
    __shared__ double sm[5];
    const unsigned col = blockIdx.x;
    double t[1] = {0.0};
    for (unsigned w = threadIdx.x; w < nwg; w += kBlock) t[0] += partial[(size_t)w * NB + col];
    block_sum<1>(t, sm);
    if (threadIdx.x == 0) out[col] = t[0];
}

// shift-major vectors x[j * stride + i] <-> row-major xt[i * kSpmmCols + j] (columns >= nvec are zero), a tile of
// 256 rows through LDS so that both the reads and the writes are coalesced
__global__ void __launch_bounds__(kBlock) k_rows_from_vectors(const double *x, size_t stride, int nvec, uint32_t n, double *xt)
{
    constexpr int NB = kSpmmCols;
    __shared__ double tile[kBlock][NB + 1];
    const uint32_t r0 = blockIdx.x * kBlock, i = r0 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < NB; ++j) tile[threadIdx.x][j] = (j < nvec && i < n) ? x[(size_t)j * stride + i] : 0.0;
    __syncthreads();
    // piece q of the tile = 16 bytes: row q / 8, columns 2 (q % 8), +1; consecutive threads write consecutive pieces
    for (unsigned q = threadIdx.x; q < kBlock * (NB / 2); q += kBlock) {
        const unsigned row = q / (NB / 2), c2 = (q % (NB / 2)) * 2;
        if (r0 + row < n) {
            f64x2 t; t.x = tile[row][c2]; t.y = tile[row][c2 + 1];
            *reinterpret_cast<f64x2 *>(xt + (size_t)(r0 + row) * NB + c2) = t;
        }
    }
}
__global__ void __launch_bounds__(kBlock) k_vectors_from_rows(const double *yt, size_t stride, int nvec, uint32_t n, double *y)
{
    constexpr int NB = kSpmmCols;
    __shared__ double tile[kBlock][NB + 1];
    const uint32_t r0 = blockIdx.x * kBlock, i = r0 + threadIdx.x;
    for (unsigned q = threadIdx.x; q < kBlock * (NB / 2); q += kBlock) {
        const unsigned row = q / (NB / 2), c2 = (q % (NB / 2)) * 2;
        if (r0 + row < n) {
            const f64x2 t = *reinterpret_cast<const f64x2 *>(yt + (size_t)(r0 + row) * NB + c2);
            tile[row][c2] = t.x; tile[row][c2 + 1] = t.y;
        }
    }
    __syncthreads();
    if (i < n) {
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (j < nvec) y[(size_t)j * stride + i] = tile[threadIdx.x][j];
    }
}

void launch_spmm_sell(const SpmmArgs &a, bool with_offd, hipStream_t st)
{
    if (a.ngroups == 0) return;
    const unsigned grid = a.xcd_map ? ((a.ngroups + 7u) / 8u) * 8u : a.ngroups;
#define SPMM_GO(LAYV)                                                                                      \
    do {                                                                                                   \
        if (with_offd) BICG_LAUNCH((k_spmm_sell<LAYV, true>), dim3(grid), dim3(kBlock), 0, st, a);         \
        else BICG_LAUNCH((k_spmm_sell<LAYV, false>), dim3(grid), dim3(kBlock), 0, st, a);                  \
    } while (0)
    switch (sell_layout(a.sell)) {
    case LAY_PAD16: SPMM_GO(LAY_PAD16); break;
    case LAY_JAG32: SPMM_GO(LAY_JAG32); break;
    case LAY_JAG16: SPMM_GO(LAY_JAG16); break;
    case LAY_JAGW:  SPMM_GO(LAY_JAGW); break;
    default:        SPMM_GO(LAY_PAD32); break;
    }
#undef SPMM_GO
}
// vectors per window: as many as leave room for two workgroups per CU (80 KB each), else whatever fits one

int spmm_win_vectors(unsigned wslots)
{
    if (wslots == 0) return 0;
    static const int forced = knob_x("BICG_SPMM_NV") ? atoi(knob_x("BICG_SPMM_NV")) : 0;      // measurement knob: 4 or 8 vectors per window
    if ((forced == 4 || forced == 8) && (size_t)forced * wslots * 8u <= 156u * 1024u) return forced;
    // (the head of every row stays in registers across the passes, so more vectors per window save barriers, not matrix traffic:
    // 16 per window was dropped -- its 256 LDS reads per thread in flight cost the occupancy)
    for (int nv : {8, 4}) if ((size_t)nv * wslots * 8u <= 80u * 1024u) return nv;
    for (int nv : {8, 4}) if ((size_t)nv * wslots * 8u <= 156u * 1024u) return nv;
    return 0;
}
hipError_t launch_spmm_win(const SpmmArgs &a, bool with_offd, hipStream_t st, hipEvent_t e0, hipEvent_t e1)
{
    if (a.ngroups == 0) return hipSuccess;
    const int nv = spmm_win_vectors(a.wslots);
    if (!nv) return hipErrorInvalidValue;
    const unsigned grid = a.xcd_map ? ((a.ngroups + 7u) / 8u) * 8u : a.ngroups;
    const unsigned lds = (unsigned)nv * a.wslots * 8u;
    const bool runs = a.cl.ncl == 0;
    auto go = [&](auto kernel) {
        // (the runtime answers "invalid argument" and launches with > 64 KiB of dynamic LDS all the same: bicg_persist.hip)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 159 * 1024);
        (void)hipGetLastError();
        if (e0 && e1) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, e0, e1, 0, a);
        else hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds, st, a);
        return hipGetLastError();
    };
#define WIN_GO(NVV)                                                                                                   \
    (runs ? (with_offd ? go(k_spmm_win<1, true, NVV>) : go(k_spmm_win<1, false, NVV>))                                 \
          : (with_offd ? go(k_spmm_win<0, true, NVV>) : go(k_spmm_win<0, false, NVV>)))
    const hipError_t err = nv == 8 ? WIN_GO(8) : WIN_GO(4);
#undef WIN_GO
    return err;
}
unsigned spmm_grid(uint32_t ngroups, bool xcd_map) { return xcd_map ? ((ngroups + 7u) / 8u) * 8u : ngroups; }
void launch_colsum(const double *partial, unsigned nwg, double *out, hipStream_t st)
{
    BICG_LAUNCH(k_colsum, dim3(kSpmmCols), dim3(kBlock), 0, st, partial, nwg, out);
}
void launch_rows_from_vectors(const double *x, size_t stride, int nvec, uint32_t n, double *xt, hipStream_t st)
{
    if (n) BICG_LAUNCH(k_rows_from_vectors, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, x, stride, nvec, n, xt);
}
void launch_vectors_from_rows(const double *yt, size_t stride, int nvec, uint32_t n, double *y, hipStream_t st)
{
    if (n) BICG_LAUNCH(k_vectors_from_rows, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, yt, stride, nvec, n, y);
}

void preload_spmm_sell_kernels() { preload_kernel(k_colsum); }

}  // namespace bicg
