// bicg_plan.h -- the plans that are made on the host without a device: the persistent iteration's (persist_plan_host,
// bicg_plan.cpp), the sliced-ELL plan of the diag block (sell_plan_host, bicg_sell_plan.cpp) and the renumbering of a badly
// numbered diag block (reorder_rcm / permute_block, bicg_reorder.cpp). Plain data: device vector
// types appear as element types only, nothing here calls the HIP runtime or reads the environment.
#pragma once

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../../include/bicgstab_hip.h"
#include "bicg_device.h"
#include "bicg_knobs.h"

namespace bicg {

// plan of the persistent iteration (bicg_persist.hip): see persist_plan_host in bicg_plan.cpp
struct PersistPlan {
    uint32_t nrows = 0, nslices = 0, spw = 0, nwg = 0;     // spw: slices per workgroup = nrw * rpt
    uint32_t nrw = 0, rpt = 1;                             // row wavefronts per workgroup, rows per thread
    uint32_t win_slots = 0, max_runs = 0, max_entries = 0;
    std::vector<unsigned short> rlen, rdiag;      // [nrows] entries of a row / of its diag part
    std::vector<uint32_t> wptr;                   // [nwg + 1] runs of workgroup g
    std::vector<uint32_t> runs;                   // pairs {first column, (first slot << 16) | length}
    std::vector<uint32_t> pbase;                  // [nslices + 1]
    std::vector<double> pval;                     // padded slices
    std::vector<uint32_t> psrc;                   // [pval entries] where the entry came from: index into (diag values | offd values), kPersistNoSource: padding
    std::vector<unsigned short> pslot;
};
constexpr uint32_t kPersistNoSource = 0xFFFFFFFFu;
bool persist_plan_host(const CSR_Matrix *diag, const unsigned *optr, const unsigned *ocol, const double *oval, unsigned gmax,
                       PersistPlan &P);

// BICG_PLAN_TRACE=1: seconds per part of the plan on stderr (the caller decides whether it is on: rank 0 only)
struct PlanTrace {
    bool on = false;
    double t = 0.0;
    static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    explicit PlanTrace(bool enabled = false) : on(enabled), t(now()) {}
    void mark(const char *what)
    {
        if (!on) return;
        const double t1 = now();
        fprintf(stderr, "bicgstab_hip: plan  %-34s %8.4f s\n", what, t1 - t);
        t = t1;
    }
};

// what all ranks share and the sliced-ELL plan depends on (decisions that change the sequence of exchanges or the association
// of the row sums must come out the same on every rank)
struct PlanFacts {
    int P = 1;                      // ranks
    uint32_t rows_global = 0;
    uint64_t nnz_diag_all = 0;      // diag non-zeros of all ranks
    bool fuse_small = true;         // the average block has < 6 M non-zeros (bicg_ctx::fuse_small)
};

// The sliced-ELL plan of one rank's diag block: what sell_plan_host decides and lays out, and sell_plan_upload (bicg_create.cpp)
// turns into device memory. Array names are those of the device side (SellDev, bicg_device.h).
struct SellPlan {
    uint32_t nrows = 0, nslices = 0, ngroups = 0;
    uint32_t nnz_d = 0;
    bool rowsplit = false;          // long rows: the whole block goes to k_spmv_rows
    bool jag = false;               // jagged slices (else padded)
    bool win = false;               // x windows in LDS
    bool win_list_mode = false;     // ... list-driven (SellDev::win_list)
    bool retried = false;           // a requested window did not fit: groups selected again for padded slices
    bool c16 = false;               // 16-bit column offsets / window slots
    bool csr16 = false;             // rows-over-lanes kernel: 16-bit column offsets in CSR order
    uint64_t sell_entries = 0, sell_nnz = 0, n16 = 0;
    uint32_t sell_rows = 0;
    uint64_t uniform_entries = 0, constant_entries = 0, masked_rows = 0;
    uint32_t win_slots = 0, win_max_runs = 0, jag_tail16_max = 0;
    bool win_near16 = false;
    FusedWindow fw{};
    std::vector<uint32_t> slice_len, slice_base, slice_base16;
    // (allocated without a fill: the threads that write a slice also zero its padding -- 330 MB of zeros from one thread were a
    // third of this part)
    std::unique_ptr<double[]> sval;                 // [max(sell_entries, 1)]
    std::unique_ptr<uint32_t[]> scol;               // [max(sell_entries, 1)], null with 16-bit offsets: the 32-bit columns are not uploaded
    std::unique_ptr<short[]> scol16;                // [n16_alloc()]
    size_t n16_alloc() const { return c16 ? (size_t)n16 : 1; }
    std::vector<unsigned char> perm;                // SellDev::perm (empty: natural order)
    std::vector<char> group_is_sell;
    std::vector<uint32_t> gl_int, gl_bnd;           // sliced-ELL groups: interior / halo-touching
    std::vector<uint4> bint, bbnd;                  // CSR row blocks: interior / halo-touching
    std::vector<uint32_t> win_ptr;
    std::vector<uint2> win_runs;
    std::vector<uint32_t> list, lptr, total;        // the list-driven window (SellDev::win_list / win_lptr / win_ltotal)
    std::vector<uint32_t> ubase, vbase, mbase;
    std::vector<int> uoff;
    std::vector<double> uval;
    std::vector<unsigned short> rmask;
    std::vector<unsigned short> lane_info;          // SellDev::lane_info (empty: a row longer than 255 entries, or padded slices)
    std::vector<short> dcol16;
    uint32_t nblk() const { return (uint32_t)(bint.size() + bbnd.size()); }
};
// diag: the rank's diag block; optr: the row pointers of its offd block (read with several ranks only). False: an internal
// inconsistency (the caller ends the program).
bool sell_plan_host(const CSR_Matrix *diag, const uint32_t *optr, const PlanFacts &facts, const PlanSwitches &sw, SellPlan &plan,
                    PlanTrace *trace = nullptr);

// bicg_sell_plan_digest (include/bicgstab_hip.h section 5): lengths of its two output arrays
constexpr int kSellSummaryLen = 22, kSellDigestLen = 26;
void sell_plan_summary(const SellPlan &plan, unsigned long long summary[kSellSummaryLen]);
void sell_plan_digest(const SellPlan &plan, unsigned long long digest[kSellDigestLen]);

// BICG_PLAN="reorder=1|2" (bicg_reorder.cpp; C views: bicg_reorder_plan / bicg_permute_block, include/bicgstab_hip.h section 5).
// reorder_rcm: perm[new] = old, reverse Cuthill-McKee on the symmetrised pattern, and the eight stats of bicg_reorder_plan.
// permute_block: P A P^T, the entries of a row in their stored order; inv_out (optional, rows entries): inv[old] = new. False
// when perm is not a permutation of 0 .. rows - 1.
void reorder_rcm(const CSR_Matrix *diag, uint32_t *perm, unsigned long long stats[8]);
bool permute_block(const CSR_Matrix *diag, const uint32_t *perm, uint32_t *ptr_out, uint32_t *col_out, double *val_out,
                   uint32_t *inv_out = nullptr);

}  // namespace bicg
