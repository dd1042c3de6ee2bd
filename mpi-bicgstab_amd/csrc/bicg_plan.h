// bicg_plan.h -- the plans that are made on the host without a device: the persistent iteration's (persist_plan_host,
// bicg_plan.cpp), the sliced-ELL plan of the diag block (sell_plan_host, bicg_sell_plan.cpp), the launch plan of a product
// (spmv_plan, bicg_spmv_plan.cpp), who closes a dot group (dot_group_plan, bicg_dot_plan.cpp) and the renumbering of a badly
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

// The launch plan of one distributed product y = A x (spmv_plan, bicg_spmv_plan.cpp): every decision about
// the SHAPE of the product -- which launches exist, over which list, where each one's dot partials start, how many partial slots
// the group expects -- as a pure function of a few integers, so that the CPU suite pins it (tests/test_spmv_plan.py). spmv()
// (bicg_solver.cpp) only executes it. No HIP call, no environment, no heap, no static state: it runs once per product on ranks
// that are host-bound at a few microseconds per launch.
enum SpmvTransport { SPMV_SINGLE = 0, SPMV_P2P = 1, SPMV_HOSTED = 2 };
struct SpmvShape {      // what a context says about its product (spmv_shape, bicg_solver.cpp) ...
    uint32_t ng_int = 0, ng_bnd = 0;      // sliced-ELL groups: interior / halo-touching
    uint32_t n_int = 0, n_bnd = 0;        // CSR row blocks: interior / halo-touching
    uint32_t nblk = 0;
    bool glist_all = false;
    int transport = SPMV_SINGLE;
    bool ll_fused = false;                // peer-to-peer: the exchange can ride inside the sliced-ELL launch
    bool has_send = false;                // ... and this rank has values to push (that launch exists even without groups)
    bool own_stream = false;              // hosted: the exchange runs on the communication stream
    bool stencil_ok = false;              // stencil_product(c)
    uint32_t stencil_wgs = 0;             // stencil_grid(c->sell.st)
    int sell_gpw = 1, sell_gpw_dots = 1;
    uint32_t wg_cap = 0;
};
struct SpmvCall {       // ... and what one call adds
    int ndot = 0, epi = 0;
    bool has_shift = false;
    bool tail = false;                    // the caller's Reduce carries a tail tag
    bool wave = false;                    // ... is a per-wavefront group (consumer-side finish)
};
enum SpmvFamily { FAM_SELL = 0, FAM_SELL_EPI = 1, FAM_STENCIL = 2, FAM_CSR = 3 };
enum SpmvList { LIST_ALL = 0, LIST_INT = 1, LIST_BND = 2, LIST_FUSED = 3, LIST_BLK_INT = 4, LIST_BLK_BND = 5 };
enum SpmvPlanError {
    SPMV_PLAN_OK = 0,
    SPMV_ERR_EPI3 = 1,                    // CA-BiCGStab's epilogue without the plane-marching product on one rank
    SPMV_ERR_EPI_MULTI = 2,               // an epilogue on a product of several launches
    SPMV_ERR_STENCIL_DECLINED = 3,        // the plane-marching launch would decline: its epilogue with a per-wavefront group
};
struct SpmvStep {
    int family = FAM_SELL, list = LIST_ALL;
    uint32_t nlist = 0;
    bool with_offd = false, fused_halo = false;
    uint32_t slot_base = 0;               // first partial slot of the launch's workgroups
    bool after_halo = false;              // runs behind the point where the halo has landed
};
constexpr int kSpmvMaxSteps = 4;
struct SpmvPlan {
    int error = SPMV_PLAN_OK;
    int groups_per_wg = 1;
    bool stencil = false, fused = false, merged = false;
    uint32_t expected = 0;                // partial slots of the dot group = workgroups of all launches
    uint32_t hand_nsh = 0;                // shard totals a hand-over group leaves (bicg_ctx::Hand::nsh)
    bool sets_nparts = false;             // bicg_ctx::Group::nparts = expected * wavefronts per workgroup
    bool tail = false;                    // the tail finish stays (else: arrival tickets)
    int nsteps = 0;
    SpmvStep step[kSpmvMaxSteps];
};
SpmvPlan spmv_plan(const SpmvShape &s, const SpmvCall &k);
const char *spmv_plan_error(int error);   // the message spmv() ends the program with
// bicg_spmv_launch_plan (include/bicgstab_hip.h section 5): lengths of its arrays
constexpr int kSpmvShapeLen = 15, kSpmvCallLen = 5, kSpmvPlanLen = 10, kSpmvStepLen = 7;

// Who closes a dot group (dot_group_plan, bicg_dot_plan.cpp): what the producer's Reduce says and the ordered
// operations that turn the group's sums into scalars, as a pure function of what the context says (DotShape) and what one call
// says (DotCall), so that the CPU suite pins it (tests/test_dot_group_plan.py). DotGroups (bicg_host.h, bicg_dots.cpp) only
// executes it. No HIP call, no environment, no heap, no static state. The transports are SpmvTransport's.
enum DotRegime { DOT_TICKET = 0, DOT_WAVE = 1, DOT_HAND = 2 };      // tickets / tail finish, consumer-side finish, hand-over
// what happens to the group: NOW / DEFER open one (closed at once / riding across the next product); FORCE: the host or a product
// needs the open group's scalars before a consumer came; CONSUME: the consuming kernel's launch; CONTRIBUTE: a producer that
// neither opens nor closes (a product without dots; the first of two producers of one group)
enum DotEvent { DOT_NOW = 0, DOT_DEFER = 1, DOT_FORCE = 2, DOT_CONSUME = 3, DOT_CONTRIBUTE = 4 };
enum DotOpen { DOT_OPEN_NONE = 0, DOT_OPEN_PLAIN = 1, DOT_OPEN_DEFERRED = 2, DOT_OPEN_STAGED = 3 };   // the group open when the call is made
struct DotShape {
    int transport = SPMV_SINGLE;
    bool stream_ordered = false, overlap = false;      // hosted: the transport's collectives run in stream order; two streams
    bool inline_apply = false;                         // peer-to-peer: the producer's last workgroup may collect and apply
    bool tail_finish = false;                          // the switch is on and the tables exist
    bool graph_replay = false;                         // iterations are captured and replayed (BICG_GRAPH=1)
    bool handover = false;                             // the switch is on, the tables exist and the product's layout allows it
};
struct DotCall {
    int regime = DOT_TICKET, n = 0, off = 0, phase = 0;
    bool apply_single = true;
    int event = DOT_NOW, open = DOT_OPEN_NONE;
    bool by_product = false;                           // the call comes from a product (its own dots, or it meets the open group)
};
enum DotOp {
    DOT_OP_NOTHING = 0,        // the producer's last workgroup did it
    DOT_OP_FINISH = 1,         // stand-alone finish (roles)
    DOT_OP_ALLREDUCE = 2, DOT_OP_APPLY = 3, DOT_OP_APPLY_P2P = 4,
    DOT_OP_RECORD = 5, DOT_OP_WAIT = 6,      // an event recorded on `stream` / `stream` waits for the event recorded last
    DOT_OP_STAGE = 7,          // staged by the next product's first launch (roles)
    DOT_OP_CONSUMER = 8,       // finished by the consuming kernel (roles)
};
enum DotWhen { DOT_AT_CLOSE = 0, DOT_BEHIND_HALO = 1, DOT_AFTER_PRODUCT = 2, DOT_IN_CONSUMER = 3 };
enum DotStream { DOT_COMPUTE = 0, DOT_COMM = 1 };
enum DotPlanError { DOT_PLAN_OK = 0, DOT_ERR_OPEN = 1, DOT_ERR_STAGE_DOTS = 2, DOT_ERR_HAND_NONE = 3 };
struct DotStep { int op = DOT_OP_NOTHING, when = DOT_AT_CLOSE, stream = DOT_COMPUTE, roles = 0, n = 0, off = 0, phase = 0; };
constexpr int kDotMaxSteps = 7;
struct DotPlan {
    int error = DOT_PLAN_OK;
    bool wave = false, hand = false, apply_now = false;      // the producer's Reduce ...
    int n_collect = 0;                                        // ... its p2p.n_collect
    bool tail = false;                                        // ... carries a new tail tag
    bool mailbox = false;                                     // ... publishes to the peers' mailboxes (carries the group's descriptor)
    bool deferred = false;                                    // the group rides across the next product
    int nsteps = 0;
    DotStep step[kDotMaxSteps];
};
bool dot_tail_available(const DotShape &s);      // can a ticket group take the tail finish
bool dot_handover(const DotShape &s);            // does plain BiCGStab hand its groups over to the consuming kernels
DotPlan dot_group_plan(const DotShape &s, const DotCall &k);
const char *dot_plan_error(int error);           // the message the executor ends the program with
// bicg_dot_group_plan (include/bicgstab_hip.h section 5): lengths of its arrays
constexpr int kDotShapeLen = 7, kDotCallLen = 8, kDotPlanLen = 9, kDotStepLen = 7;

// BICG_PLAN="reorder=1|2" (bicg_reorder.cpp; C views: bicg_reorder_plan / bicg_permute_block, include/bicgstab_hip.h section 5).
// reorder_rcm: perm[new] = old, reverse Cuthill-McKee on the symmetrised pattern, and the eight stats of bicg_reorder_plan.
// permute_block: P A P^T, the entries of a row in their stored order; inv_out (optional, rows entries): inv[old] = new. False
// when perm is not a permutation of 0 .. rows - 1.
void reorder_rcm(const CSR_Matrix *diag, uint32_t *perm, unsigned long long stats[8]);
bool permute_block(const CSR_Matrix *diag, const uint32_t *perm, uint32_t *ptr_out, uint32_t *col_out, double *val_out,
                   uint32_t *inv_out = nullptr);

}  // namespace bicg
