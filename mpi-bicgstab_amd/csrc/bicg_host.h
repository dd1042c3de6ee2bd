// bicg_host.h -- what the host-side translation units of the library share: the context of a rank (struct bicg_ctx), the
// device-memory helpers and their owner (dev_alloc / dev_free, struct DevOwner), section timing, and the prototypes of the functions that cross file boundaries.
//   bicg_dots.cpp     the dot groups (struct DotGroups): one owner, open / close, the executor of dot_group_plan (bicg_dot_plan.cpp, host only)
//   bicg_solver.cpp   the distributed SpMV (its launch plan: bicg_spmv_plan.cpp, host only), the four iterations of reference src/solver.c, run_begin / iterate / end
//   bicg_shifted.cpp  the shifted family (src/shifted_solver.c, src/shifted_switching_solver.c) and its section prints
//   bicg_multi.cpp    bicg_solve_multi: plain BiCGStab on up to kSpmmCols right-hand sides per pass over the matrix
//   bicg_create.cpp   bicg_create / bicg_create_device_csr: halo plan, upload of the diag block's plan (made by bicg_sell_plan.cpp,
//                     host only: bicg_plan.h) into bicg_ctx::sell / diag / offd, slice descriptors, stencil plan, transport,
//                     persistent set-up, destroy (clears the context's DevOwner: the one owner of its device memory)
//   bicg_refresh.cpp  bicg_update_values / bicg_update_values_device: new values for the resident matrix, written in place
//   bicg_precond.cpp  the context's preconditioner (struct Precond): install, release, apply, bicg_precond_* / bicg_csr_*diagonal
//   bicg_dropin.cpp   the reference's own symbols (solver.h, shifted_solver.h, shifted_switching_solver.h), matrix residency
//   bicg_api.cpp      the additive handle API (load / fetch / spmv / dot / spmm / info calls; their *_device variants)
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "bicg_comm.h"
#include "bicg_knobs.h"
#include "bicg_plan.h"
#include "bicg_parallel.h"
#include <memory>
#include "bicg_device.h"

using namespace bicg;



constexpr int kEvRing = 16;
constexpr int kMaxTimed = 8192;
constexpr int kPersistChunk = 128;   // iterations per persistent launch, at least (run_iterate)

inline double now_sec()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// device allocations made through the helpers below and not yet freed, in this process (bicg_device_allocations)
inline std::atomic<long long> &dev_live()
{
    static std::atomic<long long> n{0};
    return n;
}

template <class T> T *dev_alloc(size_t n)
{
    T *p = nullptr;
    BICG_HIP(hipMalloc((void **)&p, sizeof(T) * (n ? n : 1)));
    ++dev_live();
    return p;
}

template <class T> T *dev_upload(const T *src, size_t n)
{
    T *p = dev_alloc<T>(n);
    if (n) BICG_HIP(hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return p;
}

// n entries followed by `pad` zero entries (16-byte loads may run past the last non-zero)
template <class T> T *dev_upload_padded(const T *src, size_t n, size_t pad)
{
    T *p = dev_alloc<T>(n + pad);
    BICG_HIP(hipMemset(p + n, 0, sizeof(T) * pad));
    if (n) BICG_HIP(hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice));
    return p;
}

// the counterpart of the three helpers above (a temporary of one function); null: nothing. checked = false: on the way out
// after a failure or at tear-down, where an error of the device is not news
inline void dev_free(const void *p, bool checked = true)
{
    if (!p) return;
    if (checked) BICG_HIP(hipFree(const_cast<void *>(p)));
    else (void)hipFree(const_cast<void *>(p));
    --dev_live();
}

// Device memory that lives as long as its holder: whatever is allocated through an owner is freed by clear() (bicg_destroy), so
// a buffer added to the context cannot be left off a list. free / regrow are for the buffers that grow with the largest call.
struct DevOwner {
    std::vector<void *> ptrs;
    template <class T> T *adopt(T *p) { ptrs.push_back((void *)p); return p; }      // a dev_alloc made before the holder existed
    template <class T> T *alloc(size_t n) { return adopt(dev_alloc<T>(n)); }
    template <class T> T *upload(const T *src, size_t n) { return adopt(dev_upload(src, n)); }
    template <class T> T *upload_padded(const T *src, size_t n, size_t pad) { return adopt(dev_upload_padded(src, n, pad)); }
    void free(const void *p)
    {
        if (!p) return;
        ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), (void *)p), ptrs.end());
        dev_free(p);
    }
    template <class T> T *regrow(T *p, size_t n) { free(p); return alloc<T>(n); }
    void clear()
    {
        for (void *p : ptrs) dev_free(p, false);
        ptrs.clear();
    }
};

// What the host code needs to know about a solver method (the enum of include/bicgstab_hip.h), in one place
struct MethodInfo {
    int nvec;                   // work vectors counted for the matrix-stream policy (run_begin)
    bool pipelined;             // dot groups deferred across a product: consumer-side finish (DotGroups::wave_mode)
    Precond::Kind precond;      // the preconditioner the method needs on the context
    bool persist;               // may take the persistent launch at all (run_iterate decides per context)
    bool stab2;                 // BiCGStab(2) sweeps: its own set-up, steps come in pairs (run_iterate), no captured iteration
};
constexpr MethodInfo kMethod[] = {
    {6, false, Precond::NONE, true, false},         // BICG_BICGSTAB
    {8, false, Precond::NONE, true, false},         // BICG_CA_BICGSTAB
    {10, true, Precond::NONE, true, false},         // BICG_PIPE_BICGSTAB
    {11, true, Precond::NONE, true, false},         // BICG_PIPE_BICGSTAB_RR
    {9, false, Precond::DIAGONAL, false, false},    // BICG_BICGSTAB_DIAG: the plain one's six, two hat vectors, 1 / d
    {8, false, Precond::BLOCK, false, false},       // BICG_BICGSTAB_BLOCK: ... and the bs planes, which run_begin adds
    {9, false, Precond::NONE, false, true},         // BICG_BICGSTAB2: x, r#, r0, r1, r2, u0, u1, u2 and the set-up's Ax; multi-launch form only
    {13, false, Precond::DIAGONAL, false, true},    // BICG_BICGSTAB2_DIAG: method 6's eight, the four hat vectors (one in Ax's place), 1 / d
    {12, false, Precond::BLOCK, false, true},       // BICG_BICGSTAB2_BLOCK: ... and the bs planes, which run_begin adds
};
constexpr int kMethods = (int)(sizeof kMethod / sizeof kMethod[0]);
static_assert(BICG_BICGSTAB == 0 && BICG_BICGSTAB2 == 6 && BICG_BICGSTAB2_BLOCK == kMethods - 1, "kMethod follows the method enum");
inline Precond::Kind precond_kind_of(int method) { return method >= 0 && method < kMethods ? kMethod[method].precond : Precond::NONE; }
inline bool method_stab2(int method) { return method >= 0 && method < kMethods && kMethod[method].stab2; }

// The dot groups of a context (bicg_dots.cpp): every buffer, counter, event and piece of bookkeeping of the
// three regimes -- tickets / tail finish, consumer-side finish (wave), hand-over -- and the one interface through which the solvers
// open and close a group. WHICH operations close a group is dot_group_plan's decision (bicg_plan.h, host only, pinned by the CPU
// suite); the methods below execute that plan and keep the sequence numbers, on which the ranks agree only because every rank
// runs the same host code. A group is opened once -- n, offset, phase, now or deferred -- and close() takes no argument.
struct bicg_ctx;
struct DotGroups {
    bicg_ctx *c = nullptr;
    // ---- device memory (init; the context's DevOwner frees it) and switches
    unsigned nslots = 0;
    double *partial = nullptr, *shard_tot = nullptr;      // ticket groups: one partial per workgroup, shard totals
    unsigned *counter = nullptr;                          // ... arrival tickets
    llword *tail_tab = nullptr, *tail_shard = nullptr;    // tail finish of ticket groups (struct Reduce): LL table + shard totals
    bool tail_finish = true;                              // BICG_TAIL_FINISH=0: arrival tickets
    double *wpart[2] = {nullptr, nullptr};                // wave groups: per-wavefront partial sums, alternating between groups
    llword *shard_ll = nullptr;                           // 2 x [kShards][kRedSlots][2], alternating like wpart
    unsigned long long spin_ticks = 2000;                 // 20 us before a workgroup sums a missing shard itself (BICG_TEST="spin-ticks=n")
    // hand-over of plain BiCGStab's three groups (RED_HAND): two shard-total tables [kRedSlots][kShards][2] that alternate group by
    // group (FPlainXR reads one group's totals while its last workgroups write the next group's). BICG_PLAN="handover=0": off
    bool handover = true;
    llword *hand_shard = nullptr;
    bool inline_apply = true;                             // peer-to-peer, BICG_P2P_INLINE_APPLY=0: always the separate apply kernel
    hipEvent_t ev_dots[kEvRing] = {}, ev_red[kEvRing] = {};
    unsigned i_dots = 0, i_red = 0;
    // ---- bookkeeping
    bool wave_mode = false;      // this solve's groups are wave groups (reset); false: tickets
    int cur = 0;                 // the current scalar block: c->S == c->Sbuf + cur
    unsigned grp_seq = 0, tail_seq = 0;
    struct Group {               // the open ticket or wave group
        bool active = false;     // opened, not yet closed / consumed
        bool staged = false;     // a product's launch has already summed the shards / pushed the sums to the peers
        unsigned seq = 0, mail_seq = 0, nparts = 0;
        int buf = 0;
        DotCall call;            // what open() was told
        DotPlan plan;            // ... and what dot_group_plan made of it
    } grp;
    struct Hand {
        unsigned seq = 0, nsh = 0;   // tag of the open group (0: none), shard totals its producer leaves
        int n = 0, phase = 0, buf = 0;
    } hand;
    struct Pending {             // a closed group whose remaining steps ride on the next product
        bool on = false, joined = false;
        DotPlan plan;
        hipEvent_t ev = nullptr;
        unsigned seq = 0;        // its mailbox number (peer-to-peer)
    } pend;

    void init(bicg_ctx *ctx, unsigned slots);      // device memory (zeroed), events, switches
    // a solve or a stand-alone call begins: regime, no group open, fresh arrival tickets, and the current scalar block (both: and the
    // idle one) set to *block (null: zeroed)
    void reset(bool wave, const Scal *block = nullptr, bool both = false);
    DotShape shape() const;                        // what the context tells dot_group_plan (handover: switch and tables only)
    DotShape shp;                                  // ... as of the last reset (solve_shape)
    bool tail_available() const { return dot_tail_available(shape()); }
    void next_block();                             // everything enqueued from now on reads the other scalar block
    // open a group in the solve's regime (event: DOT_NOW / DOT_DEFER) and return its producer's Reduce; nwg: the producer's
    // workgroups (0: a product, which reports them through producer_grid)
    Reduce open(int n, int phase, int event = DOT_NOW, int off = 0, unsigned nwg = 0, bool by_product = false);
    Reduce open_hand(int n, int phase, unsigned nwg = 0);
    Reduce contribute(int off, bool apply_single); // a producer that neither opens nor closes (CA-BiCGStab's first of two)
    Reduce no_dots() { return contribute(0, true); }      // a product without dots
    void close();                                  // the plan's "at close" steps
    bool is_open() const { return grp.active && grp.plan.wave; }      // a wave group is open (a ticket group is closed by the call that follows its producer)
    void force(bool by_product = false);           // the host or a product needs the open wave group's scalars now
    Launch consume();                              // the launch descriptor of a kernel that finishes the open wave group (if any)
    Launch consume_hand();
    // spmv(): the open wave group as the product's first launch sees it; what its launches publish; the two points of a product
    Finish before_product(bool has_dots);
    void producer_grid(const Reduce &red, unsigned expected, unsigned hand_nsh, bool sets_nparts);
    void behind_halo();
    void after_product();
    void flush();                                  // a deferred group that no product picked up
private:
    const DotShape &solve_shape();
    Reduce ticket(const DotPlan &p, int off, int phase);
    Finish desc(int roles) const;
    void run(const DotPlan &plan, int when, unsigned mail_seq = 0);
};

constexpr unsigned kWaitCap = 4096;      // samples per row of PersistArgs::waitlog
struct bicg_ctx {
    Comm *comm = nullptr;                  // null once the communicator has been replaced (contexts_orphan)
    int device = 0;
    int nranks = 1, rank = 0;
    uint32_t n_loc = 0, n_glob = 0, halo = 0, stride = 0, nnz_d = 0, nnz_o = 0;

    // Device memory of the context's lifetime: every allocation goes through `own` (the persistent plan's through `persist_own`,
    // which ctx_finish drops as a whole when the ranks do not agree on it); bicg_destroy clears both. Outside them: the landing
    // ring (the transport's shared memory, release_p2p), the pinned host blocks, events, streams, graphs.
    DevOwner own, persist_own;
    // matrix + plan (device): the structs the product kernels take, filled once by set-up (sell_plan_upload, build_slice_desc,
    // build_stencil_plan, stencil_across_ranks, bicg_create_device_csr) and copied into every launch's arguments
    SellDev sell{};                        // sliced-ELL copy of the diag block (rows whose 256-row group pads by < 25 %)
    CsrDev diag{}, offd{};                 // CSR blocks: local columns / columns renumbered to rows + halo position
    uint4 *desc_int = nullptr, *desc_bnd = nullptr;   // CSR row-block descriptors: interior / halo-touching
    FusedWindow fw{};                      // clusters of column distances of a padded 16-bit block (fw.ncl > 0): the windows of the SpMM kernels
    bool rowsplit = false;                 // long rows: the row blocks go to k_spmv_rows (a row spread over T lanes)
    short *d_col16 = nullptr;              // ... with CSR-order 16-bit column offsets when they fit
    uint32_t nblk = 0, n_int = 0, n_bnd = 0;
    int sell_gpw = 1, sell_gpw_dots = 1;   // 256-row groups per workgroup: plain SpMV / SpMV with fused dots
    uint32_t sell_blocked = 0;             // the groups are taken plane block by plane block (sell_order_for_big_grids): block size
    int spmv_dir = 0;                      // direction of the last sliced-ELL product (SpmvArgs::reverse)
    int sell_alt = 1;                      // BICG_SELL_ALT=0: every product forward; default: consecutive products alternate direction
    int sell_xcd = 1;                      // BICG_SELL_XCD=0: round robin; default: XCD-contiguous group order (SpmvArgs::xcd_map)
    int sell_nt_env = -1;                  // BICG_SELL_NT: force (1) / forbid (0) non-temporal matrix loads
    bool sell_nt = false;                  // decided per solve from the working-set size (run_begin)
    uint64_t matrix_bytes = 0;             // bytes one SpMV streams from the matrix arrays
    uint64_t stencil_matrix_bytes = 0;     // ... when the plane-marching product runs (StencilDev)
    hipEvent_t region_ev[2] = {nullptr, nullptr};   // bicg_run_iterate_timed
    unsigned *waitlog = nullptr;           // PersistArgs::waitlog (multi-rank persistent launches), 3 rows of kWaitCap samples
    double t_enq = 0.0;
    uint64_t device_matrix_bytes = 0;      // bytes of matrix storage resident on the GPU
    // host-side facts of the plan (BICG_PLAN="uniform=0" / "constant=0" / "masked=0" / "desc=0" / "lists=0" / "stencil=0" switch
    // the matching SellDev members off)
    uint64_t uniform_entries = 0;          // sliced-ELL entries whose columns the SpMV does not read (SellDev::ubase / uoff)
    uint32_t far_rows = 0;                 // farthest column distance of a uniform slice, in rows (a grid's plane size)
    uint64_t masked_rows = 0;              // rows of masked slices (SellDev::mbase / rmask)
    uint32_t plan_collisions = 0;          // list-driven slices the device plan's verification pass put back (bicg_plan_collisions)
    bool st_multi = false;                 // several ranks: the halo-free rows of this rank are the whole planes z_lo .. z_hi - 1 of its grid
    bool ca_fuse = true;                   // CA-BiCGStab: q, y and their dots in the epilogue of z = A s (plane-marching product only; BICG_PLAN="ca-fuse=0")
    uint64_t constant_entries = 0;         // ... whose values it does not read either (SellDev::vbase / uval)
    uint32_t jag_tail16_max = 0;           // most entries one jagged slice holds behind the 16th entry of its rows
    bool win_near16 = false;               // every window column lies within 16 bits of its group's first row (k_spmm_jpipe packs them)
    bool jagw_fast = true;                 // the three-trip product of bicg_jagw.hip (BICG_PLAN="jagw=0": k_spmv_sell's loop, which
                                           // spmv() selects by passing SellDev::lane_info as null)
    uint32_t *glist_int = nullptr, *glist_bnd = nullptr;
    uint32_t ng_int = 0, ng_bnd = 0, sell_rows = 0;
    uint64_t sell_entries = 0, sell_nnz = 0;
    bool glist_int_identity = false;
    bool glist_all = false;        // every 256-row group is on the sliced-ELL path (one merged launch possible)

    // halo exchange
    std::vector<int> scnt, sdsp, rcnt, rdsp;
    uint32_t nsend = 0;
    uint32_t *send_idx = nullptr;
    double *sendbuf = nullptr;
    // the exchange of a SET of vectors (spmm_pass, halo_set): kSpmmCols x nsend / kSpmmCols x halo doubles laid out peer-major, and
    // per entry of the send list / of the halo {first entry, entries} of its peer (k_halo_pack_set); made with the SpMM buffers
    double *set_send = nullptr, *set_recv = nullptr;
    uint2 *set_smap = nullptr, *set_rmap = nullptr;
    std::vector<int> set_cnt[4];           // scnt, sdsp, rcnt, rdsp of the current set: the context's times its vectors
    // transport calls issued for this context since bicg_create (bicg_comm_counts): Comm::exchange, Comm::allreduce_sum
    unsigned long long n_exchange = 0, n_allreduce = 0;
    // peer-to-peer transport (comm->p2p): landing ring for incoming halo values and, per entry of
    // the send list, where it goes in the ring of the rank that needs it
    P2p *p2p = nullptr;
    llword *halo_ring = nullptr;                              // [kHaloRing][halo][2]
    unsigned long long *push_dst0 = nullptr, *push_stride = nullptr;
    std::vector<void *> ring_mapped;
    unsigned halo_seq = 0;          // exchanges started (sequence number of the last one)
    int halo_unsynced = 0;          // exchanges since the last all-reduce or barrier (flow control)
    bool comm_failed = false;       // a peer-to-peer wait timed out (BICG_P2P_SOFT_FAIL)
    bool soft_fail = false;         // ... report it through comm_failed instead of ending the program (drop-in fallback)
    // Exchange folded into the SpMV launch (HaloLL): possible when every halo-touching row is on the
    // sliced-ELL path. One launch covers push + interior + halo-touching groups (listed in that order).
    bool ll_fused = false;
    uint32_t *glist_ll = nullptr;
    int fault_after = 0;            // BICG_TEST="p2p-fault-after=n" (tests): from the n-th exchange on this rank sends nothing

    Precond pc;                     // the one preconditioner of the context (bicg_precond.cpp)

    // vectors and scalars
    double *slab = nullptr;
    Vecs v{};
    Scal *S = nullptr;           // the scalar block kernels enqueued from now on read (= Sbuf + dots.cur; DotGroups::next_block)
    Scal *Sbuf = nullptr;        // two blocks: a kernel that finishes a dot group reads one and writes the other
    Scal *hS = nullptr;          // pinned mirror
    DotGroups dots;              // the dot groups: their buffers, counters, events and who closes them (bicg_dots.cpp)
    bool spmm_ok = false;        // spmm_possible() on every rank (the SpMM exchanges the halos of all its vectors at once)
    bool fuse_plan_ok = false;   // every row on the sliced-ELL path and one launch per SpMV -- ON EVERY RANK (the fused and the
                                 // separate flow exchange their dot groups differently: the choice is collective)
    bool fuse_pipe = true;       // pipelined solvers: element-wise phases in the SpMV epilogues (BICG_PLAN="fuse-pipe=0|1" overrides)
    bool fuse_small = true;      // ... the average block has < 6 M non-zeros: fused whatever the layout
    int  pipe_probe = 0;         // BICG_PLAN="pipe-probe": the first pipelined solve TIMES both forms on this matrix and keeps the faster
    bool pipe_probed = false;    // ... done (the choice holds for the life of the context)
    double probe_ms[2] = {0, 0}; // ... ms per iteration measured for {separate kernels, phases in the SpMV epilogues}
    bool f1_done = false;        // phase 1 of the NEXT iteration has already run in the previous launch's epilogue
    // persistent pipelined iteration (bicg_persist.hip, struct PersistArgs): plan + LL buffers; persist.nwg == 0: not available
    PersistArgs persist{};
    // bicg_update_values refills persist.pval through this map (PersistPlan::psrc, in the CALLER's entry numbering also on a
    // reordered context); persist_own like the plan itself, and like the caller's row pointers below not matrix storage
    int *refresh_flag = nullptr;           // bicg_update_values: raised by the read-only pass over list-held values (one word, zero between calls)
    uint32_t *persist_psrc = nullptr;
    uint32_t persist_entries = 0;
    bool persist_on = false;     // use it for pipe_bicgstab (every rank agrees); BICG_PERSIST=0 (or off) keeps the multi-launch iteration
    bool persist_plain = true;   // ... and for plain BiCGStab (BICG_PERSIST_PLAIN=0: the five-launch iteration)
    bool last_shifted_persist = false;   // the last shifted solve ran as persistent launches (bicg_result.flags of bicg_solve_shifted)
    unsigned persist_seq = 0;    // LL tags used so far (dot tables)
    unsigned persist_vseq = 0;   // ... by the pipelined kernel's vector images
    unsigned wg_cap = 0;         // ranks sharing this GPU (tests): workgroups per launch that may wait for another rank
    int *alarm = nullptr, *h_alarm = nullptr;
    double *trace = nullptr;     // 4 * trace_cap
    int trace_cap = 0;
    int last_iters = 0;

    hipStream_t sc = nullptr, sm = nullptr;   // compute, communication
    hipEvent_t ev_pack[kEvRing] = {}, ev_halo[kEvRing] = {};
    unsigned i_pack = 0, i_halo = 0;
    // the *_device entry points (cross_begin / cross_end below): [0] recorded on the caller's stream, the compute stream waits for
    // it; [1] recorded on the compute stream, the caller's stream waits for it. Timing disabled; created by the first such call
    hipEvent_t cross_ev[2] = {nullptr, nullptr};

    // shifted solver (bicg_solve_shifted): per-shift scalar state and the two vector sets
    double *sw_buf = nullptr;        // seed-switching variants: archives (doubles) followed by the flag arrays
    size_t sw_cap = 0;
    ShiftDev *sh_dev = nullptr;
    double *sh_arrays = nullptr, *p_set = nullptr, *x_set = nullptr;
    int sh_cap = 0;
    double cur_shift = 0.0;
    bool cur_has_shift = false;

    // SpMM (bicg_spmm, bicg_shifted_residuals): kSpmmCols shift-major vectors with halo tails, their row-major
    // image [rows + halo][kSpmmCols], the row-major result and the per-workgroup column sums
    double *mm_in = nullptr, *mm_xt = nullptr, *mm_yt = nullptr, *mm_part = nullptr, *mm_out = nullptr, *mm_sigma = nullptr;
    bool mm_xcd = true;          // XCD-contiguous row groups in the SpMM (BICG_SPMM_XCD=0: round robin like the SpMV)
    // A rank WITHOUT rows (more ranks than rows, or an empty block of a non-zero balanced partition; the reference's loops simply
    // run over zero rows there, src/matrix.c:295-298) holds ONE phantom row here -- the 1 x 1 block [1.0], decoupled from every
    // other row, with x = b = 0: all its vector entries stay 0, it adds 0.0 to every dot sum, sends and receives nothing, and so
    // takes part in every exchange and every launch path without a zero-row form of any kernel. The caller's vectors are empty:
    // host reads come from / host writes go to a scratch (host_in / host_out below).
    bool phantom = false;
    std::vector<double> ph_scratch;
    bool mm_win = false;         // the last SpMM pass ran the windowed kernel (vectors stay shift-major, X staged in LDS)
    int  mm_win_env = 3;         // BICG_PLAN="spmm-window=0": the row-major kernel, 1: k_spmm_win everywhere, 3 (default): k_spmm_pipe where the block qualifies
    bool mm_dma = false;         // the last SpMM pass ran the pipelined kernel (bicg_spmm.hip)
    int  mm_tile = 0;            // ... k_spmm_pipe with this many rows per tile (512 or 256); 0: any other kernel

    // multi-RHS BiCGStab (bicg_solve_multi, bicg_multi.cpp): one set of kSpmmCols columns of X, R, R#, P, S, Y in one slab, the
    // set's scalar block, its dot partials and its trace; allocated by the first call. The traces of the last call's sets are
    // kept on the host for bicg_multi_trace: [column][4][mt_iters[column]]
    double *mt_slab = nullptr, *mt_part = nullptr, *mt_trace = nullptr;
    MultiScal *mt_S = nullptr;
    double *mt_hat = nullptr;              // P^ and Q^, two more sets: one allocation of its own, made by the first preconditioned call (methods 4, 5)
    double *mt_red = nullptr;              // [nranks][2][kSpmmCols]: every rank's local dot sums, gathered by one all-reduce (k_multi_sum)
    int mt_trace_cap = 0;
    std::vector<std::vector<double>> mt_host_trace;
    std::vector<int> mt_iters;

    // BICG_PLAN="reorder=1|2" (DESIGN.md section 4.14b): the diag block was renumbered before it was planned. Everything on the device is
    // in the new numbering; the caller's vectors cross through perm / inv (vec_upload / vec_download below).
    int reorder_mode = 0;                // the token's value (ctx_read_switches)
    bool reordered = false;
    uint32_t *ro_perm = nullptr, *ro_inv = nullptr;      // perm[new] = old, inv[old] = new
    uint32_t *ro_src_ptr = nullptr;      // the caller's row pointers (bicg_update_values takes values in the caller's numbering)
    std::vector<uint32_t> ro_perm_host, ro_src_ptr_host;     // ... and both on the host while bicg_create builds the persistent plan
    double *ro_stage = nullptr;          // staging for host copies: ro_stage_vecs vectors, `stride` apart; grows with the largest call
    int ro_stage_vecs = 0;
    unsigned long long ro_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // bicg_reorder_info
    std::vector<uint32_t> ro_ptr, ro_col;                // the permuted block while bicg_create plans and uploads it
    std::vector<double> ro_val;

    // state of the solve in progress (run_begin / run_iterate / run_end)
    bicg_options opt{};
    int method = 0, it = 0, printed = 0, adaptive_rr = 0;
    double t_begin = 0.0, t_init = 0.0, t_iter = 0.0;

    // per-SpMV timing
    bool time_kernels = false;
    std::vector<hipEvent_t> tev;
    int tev_used = 0, spmv_calls_timed = 0;

    // section timing (bicg_options.time_kernels & 2): an event on the compute stream wherever the kind of work
    // changes; the time between two marks belongs to the section the first one opened. The counterpart of the
    // reference's MEASURE_SECTION_TIME (src/shifted_switching_solver.c:77-81, 132-154, 230-247: MPI_Wtime around the
    // shift loops, seed = total - shift), on the device's clock instead of the host's.
    bool time_sections = false, sec_exhausted = false;
    std::vector<hipEvent_t> sec_ev;
    std::vector<unsigned char> sec_lab;
    // finer attribution of a mark (the reference's ten sections, src/shifted_switching_solver.c:678-695): iteration it belongs to,
    // which product of the iteration (1 / 2), and what inside the product (0 the rows / everything, 1 halo exchange, 2 halo-touching rows)
    std::vector<int> sec_k;
    std::vector<unsigned char> sec_sub;
    int cur_k = 0, cur_prod = 0, cur_sub = 0;
    bool sec_dump = false;                 // BICG_SECTION_TIME=2: the per-iteration table of DISPLAY_SECTION_TIME
    double switch_sec = 0.0;               // host time spent in seed switches
    int sec_used = 0, sec_cur = 255;
    double sec_ms[4] = {0, 0, 0, 0};
    int sec_iters = 0;

    // BICG_TEST="force-comm" (tests): run the multi-rank code path (pack, exchange, packed all-reduce,
    // apply kernels, two streams) even with one rank, so that it can be exercised on a one-GPU box
    bool force_comm = false;
    bool single() const { return nranks == 1 && !force_comm; }

    // Use the second (communication) stream to overlap the halo exchange with the interior rows and
    // the pipelined variant's all-reduces with the next SpMV (reference src/matrix.c:432-440,
    // src/solver.c:363-367). A cross-stream hand-off costs ~7 us each way, the interior SpMV of a
    // 200 k-row rank only ~6 us, so below ~6 M local non-zeros everything is enqueued in order on
    // the compute stream instead. BICG_OVERLAP=0/1 overrides.
    bool overlap = false;

    // hipGraph replay of the iteration body (BICG_GRAPH): one captured iteration per method
    int graph_mode = -1;                 // -1 auto, 0 off, 1 on
    hipGraphExec_t graph_exec[kMethods] = {};
    int graph_warm[kMethods] = {};       // eager iterations done since the context was created
    bool graph_nt[kMethods] = {};
};

// contexts alive in this process: a context holds pointers into its communicator (transport, peer-to-peer state),
// so replacing the communicator (bicg_comm_init_*, bicg_comm_finalize) orphans them -- they can still be
// destroyed, nothing else
extern std::vector<bicg_ctx *> g_live;

// host vectors of a rank without rows (bicg_ctx::phantom): `count` zeros to read / a place to write
inline const double *host_in(bicg_ctx *c, const double *p, size_t count = 1)
{
    if (!c->phantom) return p;
    c->ph_scratch.assign(std::max<size_t>(count, 1), 0.0);
    return c->ph_scratch.data();
}
inline double *host_out(bicg_ctx *c, double *p, size_t count = 1)
{
    if (!c->phantom || !p) return p;
    if (c->ph_scratch.size() < count) c->ph_scratch.assign(count, 0.0);
    return c->ph_scratch.data();
}

// A caller's vectors crossing into / out of device memory: nvec vectors of n_loc doubles, one after the other on the host,
// dev_stride doubles apart on the device. async: enqueued on the compute stream (the caller synchronises before it returns);
// otherwise blocking copies. A context that is not reordered does exactly these copies; a reordered one goes through its
// staging buffer and the permutation kernels on the compute stream (reorder_upload / reorder_download, bicg_api.cpp).
void reorder_upload(bicg_ctx *c, double *dev, size_t dev_stride, const double *host, int nvec, bool async);
void reorder_download(bicg_ctx *c, double *host, const double *dev, size_t dev_stride, int nvec, bool async);
inline void vec_upload(bicg_ctx *c, double *dev, size_t dev_stride, const double *host, int nvec = 1, bool async = false)
{
    if (c->reordered) { reorder_upload(c, dev, dev_stride, host, nvec, async); return; }
    const size_t n = c->n_loc;
    for (int j = 0; j < nvec; ++j) {
        if (async) BICG_HIP(hipMemcpyAsync(dev + (size_t)j * dev_stride, host + (size_t)j * n, sizeof(double) * n, hipMemcpyHostToDevice, c->sc));
        else BICG_HIP(hipMemcpy(dev + (size_t)j * dev_stride, host + (size_t)j * n, sizeof(double) * n, hipMemcpyHostToDevice));
    }
}
inline void vec_download(bicg_ctx *c, double *host, const double *dev, size_t dev_stride, int nvec = 1, bool async = false)
{
    if (c->reordered) { reorder_download(c, host, dev, dev_stride, nvec, async); return; }
    const size_t n = c->n_loc;
    for (int j = 0; j < nvec; ++j) {
        if (async) BICG_HIP(hipMemcpyAsync(host + (size_t)j * n, dev + (size_t)j * dev_stride, sizeof(double) * n, hipMemcpyDeviceToHost, c->sc));
        else BICG_HIP(hipMemcpy(host + (size_t)j * n, dev + (size_t)j * dev_stride, sizeof(double) * n, hipMemcpyDeviceToHost));
    }
}

// A caller's DEVICE vectors crossing (the *_device entry points, bicg_api.cpp): nvec columns `ld` doubles
// apart on the caller's side, dev_stride apart on the solver's, in the caller's numbering also on a reordered context -- one
// launch of bicg_vecio.hip on the compute stream for up to two vectors (a null caller pointer: that vector stays out), no staging
// buffer, no allocation. A rank without rows copies nothing: cross_in zeroes its phantom row instead, as host_in's zeros would.
// cross_begin / cross_end order the compute stream behind the caller's stream and the caller's stream behind the compute stream
// through the context's two events, without a host wait.
void cross_begin(bicg_ctx *c, hipStream_t user);
void cross_end(bicg_ctx *c, hipStream_t user);
void cross_in(bicg_ctx *c, double *dev0, const double *user0, double *dev1, const double *user1, size_t dev_stride, size_t ld, int nvec);
void cross_out(bicg_ctx *c, double *user0, const double *dev0, double *user1, const double *dev1, size_t dev_stride, size_t ld, int nvec);

// every transport collective of a context goes through these two: they count (bicg_comm_counts)
inline void ctx_allreduce(bicg_ctx *c, double *dev, int n, hipStream_t st)
{
    c->n_allreduce++;
    c->comm->allreduce_sum(dev, n, st);
}
inline void ctx_exchange(bicg_ctx *c, const double *send, const int *scnt, const int *sdsp, double *recv, const int *rcnt, const int *rdsp,
                         hipStream_t st)
{
    c->n_exchange++;
    c->comm->exchange(send, scnt, sdsp, recv, rcnt, rdsp, st);
}

inline void use_device(const bicg_ctx *c)
{
    if (!c->comm)
        die("bicg_ctx", "the communicator this context was built on has been replaced or finalized; only bicg_destroy is valid now");
    BICG_HIP(hipSetDevice(c->device));
}

// ---- section timing (bicg_solver.cpp)
enum { SEC_VEC = 0, SEC_SPMV = 1, SEC_SHIFT = 2, SEC_REDUCE = 3, SEC_COUNT = 4, SEC_STOP = 255 };
constexpr int kMaxSectionMarks = 1 << 16;
void sec_mark(bicg_ctx *c, int label);
void sec_remark(bicg_ctx *c);
void sec_begin(bicg_ctx *c, bool on);
void sec_collect(bicg_ctx *c, int iters);
struct SubSection {    // the enclosed launches are part `sub` of the current product
    bicg_ctx *c; int prev;
    SubSection(bicg_ctx *ctx, int sub) : c(ctx), prev(ctx->cur_sub) { c->cur_sub = sub; sec_remark(c); }
    ~SubSection() { c->cur_sub = prev; sec_remark(c); }
};
struct Section {       // the enclosed launches belong to `label`; afterwards the enclosing section continues
    bicg_ctx *c; int prev;
    Section(bicg_ctx *ctx, int label) : c(ctx), prev(ctx->sec_cur) { if (prev != SEC_STOP) sec_mark(c, label); }
    ~Section() { if (prev != SEC_STOP) sec_mark(c, prev); }
};

// ---- dot groups, products, iterations (bicg_solver.cpp)
bool stencil_product(const bicg_ctx *c);
bool plain_handover(const bicg_ctx *c);      // plain BiCGStab on this context hands its dot groups over to the consuming kernels
bool hosted(const bicg_ctx *c);      // several ranks whose collectives the host enqueues (RCCL / host transports)
void spmv(bicg_ctx *c, double *xin, double *yout, int ndot, const double *u, Reduce red, Finish fin = Finish{}, int epi = 0,
          Scal *S = nullptr);
void spmv_grp(bicg_ctx *c, double *xin, double *yout, int ndot = 0, const double *u = nullptr, int phase = PH_NONE, int event = DOT_NOW);
void spmv_epi(bicg_ctx *c, double *xin, double *yout, int epi, int nd, int phase, int event);
void halo_only(bicg_ctx *c, double *xin);
void halo_set(bicg_ctx *c, double *in, int nvec);      // ... of nvec vectors c->stride apart in ONE transport exchange
void spmm_pass(bicg_ctx *c, int nvec, const double *sigma_host, bool with_b, bool sigma_staged = false, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr,
               double *in = nullptr, double *out = nullptr);
void spmm_stage_sigma(bicg_ctx *c, int nvec, const double *sigma_host);
bool spmm_possible(const bicg_ctx *c);
void spmm_buffers(bicg_ctx *c);
void scal_reset(bicg_ctx *c);
Scal scal_block(const bicg_ctx *c, const bicg_options &o);      // the scalar block a solve starts from
void persist_args(bicg_ctx *c, PersistArgs &a, unsigned groups, unsigned fixed_iters);      // what every persistent launch is told
void fetch_scal(bicg_ctx *c);
void run_begin(bicg_ctx *c, int method, const bicg_options *opt_in);
int run_iterate(bicg_ctx *c, int nsteps);
int run_end(bicg_ctx *c, bicg_result *res);
int run_solver(bicg_ctx *c, int method, const bicg_options *opt_in, bicg_result *res);
// ---- the shifted family (bicg_shifted.cpp)
int run_shifted(bicg_ctx *c, int mode, double *x_set_host, double *r_host, const double *sigma, int nsig, int seed,
                const bicg_options *opt_in, bicg_result *res);
// ---- plan and context (bicg_create.cpp)
bool all_ranks(Comm *comm, bool mine);
void sell_order_for_big_grids(bicg_ctx *c, uint32_t ngroups);
// ---- persistent launches (bicg_solver.cpp; the shifted family's: bicg_shifted.cpp)
bool persist_chunk(bicg_ctx *c, int niter);
void persist_account(bicg_ctx *c);
bool persist_chunk_shifted(bicg_ctx *c, int mode, int niter, int it0, int nsig, int seed, double shift);
// ---- the context's preconditioner (bicg_precond.cpp)
void precond_apply(bicg_ctx *c, const double *in, double *out);      // out = M^-1 in, one launch on the compute stream
// ... and on the nv columns of a multi-RHS set whose flag S->active is up, c->stride apart: still one launch (BLOCK only; chunk: launch_bjac_apply_set)
void precond_apply_set(bicg_ctx *c, const double *in, double *out, int nv, const MultiScal *S, int chunk = 0);
// a preconditioned method on a context that does not hold ITS preconditioner: the solving calls return -2 and touch nothing
inline bool diag_refused(const bicg_ctx *c, int method) { return c && precond_kind_of(method) != Precond::NONE && c->pc.kind != precond_kind_of(method); }
// ---- drop-in entry points (bicg_dropin.cpp)
void check_square(const INFO_Matrix *info);
void env_options(bicg_options *o);

