// bicg_solver.cpp -- GPU-resident iteration drivers behind include/bicgstab_hip.h (the C ABI itself: bicg_api.cpp, bicg_dropin.cpp;
// contexts and plans: bicg_create.cpp; the shifted family: bicg_shifted.cpp; the preconditioner: bicg_precond.cpp; what they share:
// bicg_host.h).
//
// One context per rank: the rank's diag/offd CSR blocks, the SpMV plan (row blocks, interior /
// boundary split, halo lists), twelve vectors of rows+halo doubles, and a small device-resident
// scalar block. An iteration is a fixed sequence of kernel launches (and, across ranks, halo
// exchanges and packed all-reduces) with NO host synchronisation: alpha/beta/omega live on the
// device, the convergence test of the reference's while loop (src/solver.c:86) is evaluated on the
// device and turns every later kernel into a no-op, and the host only looks every `check_every`
// iterations.
#include "bicg_host.h"


// ---------------------------------------------------------------- section timing
void sec_mark(bicg_ctx *c, int label)
{
    if (!c->time_sections || label == c->sec_cur) return;
    if (c->sec_used + 1 >= (int)c->sec_ev.size()) {      // pool used up: close the open section, stop marking
        if (c->sec_cur != SEC_STOP && c->sec_used < (int)c->sec_ev.size()) {
            BICG_HIP(hipEventRecord(c->sec_ev[c->sec_used], c->sc));
            c->sec_lab[c->sec_used++] = SEC_STOP;
        }
        c->sec_cur = SEC_STOP; c->time_sections = false; c->sec_exhausted = true;
        return;
    }
    BICG_HIP(hipEventRecord(c->sec_ev[c->sec_used], c->sc));
    c->sec_k[c->sec_used] = c->cur_k; c->sec_sub[c->sec_used] = (unsigned char)((c->cur_prod << 4) | c->cur_sub);
    c->sec_lab[c->sec_used++] = (unsigned char)label;
    c->sec_cur = label;
}
// a mark although the label stays: a new iteration, or another part of the same product
void sec_remark(bicg_ctx *c)
{
    if (!c->time_sections || c->sec_cur == SEC_STOP) return;
    const int label = c->sec_cur;
    c->sec_cur = -1;
    sec_mark(c, label);
}
void sec_begin(bicg_ctx *c, bool on)
{
    c->time_sections = on; c->sec_exhausted = false;
    c->sec_used = 0; c->sec_cur = SEC_STOP; c->sec_iters = 0;
    c->cur_k = 0; c->cur_prod = 0; c->cur_sub = 0; c->switch_sec = 0.0;
    for (double &m : c->sec_ms) m = 0.0;
    if (on && c->sec_ev.empty()) {
        c->sec_ev.resize(kMaxSectionMarks);
        c->sec_lab.resize(kMaxSectionMarks);
        c->sec_k.resize(kMaxSectionMarks); c->sec_sub.resize(kMaxSectionMarks);
        for (auto &e : c->sec_ev) BICG_HIP(hipEventCreate(&e));
    }
}
// after the stream has been synchronised: sum the spans (sections marked so far), covering `iters` iterations
void sec_collect(bicg_ctx *c, int iters)
{
    if (c->sec_used == 0) return;
    for (double &m : c->sec_ms) m = 0.0;
    for (int i = 0; i + 1 < c->sec_used; ++i) {
        if (c->sec_lab[i] == SEC_STOP) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->sec_ev[i], c->sec_ev[i + 1]) == hipSuccess) c->sec_ms[c->sec_lab[i]] += ms;
    }
    c->sec_iters = iters;
}

// transports whose collectives the host enqueues (RCCL, host callbacks)
bool hosted(const bicg_ctx *c) { return !c->single() && !c->p2p; }

// every row on the sliced-ELL path, and the plan found a grid's 7-point stencil (build_stencil_plan)
bool stencil_product(const bicg_ctx *c)
{
    // (whatever order the groups are listed in; across ranks: the halo-free rows are whole planes, StencilDev::z_lo / z_hi)
    return c->sell.st.on && c->nblk == 0 && c->glist_all && (c->single() ? c->ng_bnd == 0 : c->st_multi);
}

// Peer-to-peer exchanges are numbered; a landing ring holds kHaloRing of them. When nothing has throttled the senders for a while
// (no all-reduce or barrier since kHaloRing - 2 exchanges) a barrier goes first. Returns the sequence number of the next exchange.
static unsigned p2p_next_exchange(bicg_ctx *c, Scal *S)
{
    if (c->halo_unsynced >= kHaloRing - 2) {
        launch_p2p_barrier(c->p2p->red_desc(c->p2p->bar_seq++), c->p2p->timeout_ticks, S, c->sc);
        c->halo_unsynced = 0;
    }
    c->halo_unsynced++;
    return ++c->halo_seq;
}

// ---------------------------------------------------------------- distributed SpMV
// What a context tells spmv_plan (bicg_plan.h) about its product: the only place where the product's grids are read.
static SpmvShape spmv_shape(const bicg_ctx *c)
{
    SpmvShape s;
    s.ng_int = c->ng_int; s.ng_bnd = c->ng_bnd; s.n_int = c->n_int; s.n_bnd = c->n_bnd; s.nblk = c->nblk;
    s.glist_all = c->glist_all;
    s.transport = c->single() ? SPMV_SINGLE : c->p2p ? SPMV_P2P : SPMV_HOSTED;
    s.ll_fused = c->ll_fused; s.has_send = c->nsend > 0;
    s.own_stream = hosted(c) && c->comm->stream_ordered() && c->overlap;
    s.stencil_ok = stencil_product(c);
    s.stencil_wgs = s.stencil_ok ? stencil_grid(c->sell.st) : 0u;
    s.sell_gpw = c->sell_gpw; s.sell_gpw_dots = c->sell_gpw_dots; s.wg_cap = c->wg_cap;
    return s;
}

// One halo exchange in two halves; afterwards xin[rows .. rows + halo) holds the other ranks' values. Whatever is enqueued on the
// compute stream between the halves runs while the values travel.
// peer-to-peer (exchange number seq): the send list is stored straight into the landing rings of the ranks that need it (send =
// false: BICG_TEST="p2p-fault-after=n"), one kernel decodes the ring slot into the halo tail of x.
// hosted: pack, then the transport's exchange -- in stream order, or (own_stream) on the communication stream behind the pack, and
// then halo_start returns the event halo_land makes the compute stream wait for.
static hipEvent_t halo_start(bicg_ctx *c, double *xin, Scal *S, unsigned seq, bool send, bool own_stream)
{
    if (c->p2p) {
        if (send) launch_halo_push(xin, c->send_idx, c->nsend, c->push_dst0, c->push_stride, seq, S, c->sc);
        return nullptr;
    }
    launch_halo_pack(xin, c->send_idx, c->nsend, c->sendbuf, S, c->sc);
    if (own_stream) {
        hipEvent_t ep = c->ev_pack[c->i_pack++ % kEvRing];
        BICG_HIP(hipEventRecord(ep, c->sc));
        BICG_HIP(hipStreamWaitEvent(c->sm, ep, 0));
    }
    ctx_exchange(c, c->sendbuf, c->scnt.data(), c->sdsp.data(), xin + c->n_loc, c->rcnt.data(), c->rdsp.data(), own_stream ? c->sm : c->sc);
    if (!own_stream) return nullptr;
    hipEvent_t eh = c->ev_halo[c->i_halo++ % kEvRing];
    BICG_HIP(hipEventRecord(eh, c->sm));
    return eh;
}
static void halo_land(bicg_ctx *c, double *xin, Scal *S, unsigned seq, hipEvent_t landed)
{
    if (c->p2p) launch_halo_unpack(c->halo_ring, c->halo, seq, xin + c->n_loc, S, c->p2p->timeout_ticks, c->sc);
    else if (landed) BICG_HIP(hipStreamWaitEvent(c->sc, landed, 0));
}

// one step of the plan through its launch wrapper; false: there was nothing to launch
static bool launch_step(bicg_ctx *c, SpmvArgs &a, const SpmvStep &t, int ndot, int epi, hipEvent_t e0, hipEvent_t e1)
{
    switch (t.list) {
    case LIST_ALL: a.glist = nullptr; break;
    case LIST_INT: a.glist = c->glist_int_identity ? nullptr : c->glist_int; break;
    case LIST_BND: a.glist = c->glist_bnd; break;
    case LIST_FUSED: a.glist = c->glist_ll; break;
    case LIST_BLK_INT: a.glist = nullptr; a.desc = c->desc_int; break;      // (the CSR kernels read no group list)
    case LIST_BLK_BND: a.glist = nullptr; a.desc = c->desc_bnd; break;
    }
    a.nlist = t.nlist; a.red.slot_base = t.slot_base;
    switch (t.family) {
    case FAM_STENCIL:
        // (the plan only selects tilings the kernel is built for, and the epilogue only with ticket reductions: a launch that
        // is declined here would leave y unwritten and a ticket group waiting for partial sums that never come)
        if (!launch_spmv_stencil(a, ndot, epi == 3 ? 1 : 0, c->sc, e0, e1)) die("internal", spmv_plan_error(SPMV_ERR_STENCIL_DECLINED));
        return true;
    case FAM_SELL_EPI: return launch_spmv_sell_epi(a, epi, t.with_offd, c->sc, e0, e1, t.fused_halo);
    case FAM_CSR: return launch_spmv(a, ndot, t.with_offd, c->sc, e0, e1);
    default: return launch_spmv_sell(a, ndot, t.with_offd, c->sc, e0, e1, t.fused_halo);
    }
}

// y = A x (+ fused dots). Replaces MPI_csr_spmv_ovlap (reference src/matrix.c:428-441): the halo
// exchange runs on the communication stream while the interior row blocks are multiplied; row
// blocks that touch the halo run after it has landed. Every row is produced by exactly one
// workgroup as (0 + sum_diag) + sum_offd, the reference's order.
// Which launches that takes, over which lists and with which partial slots: spmv_plan (bicg_spmv_plan.cpp). Here the plan is
// enqueued: start the exchange, the steps that do not read the halo, land it, the steps that do, the joins.
// fin: a dot group of earlier kernels that the first kernel launched here finishes (DotGroups::before_product).
void spmv(bicg_ctx *c, double *xin, double *yout, int ndot, const double *u, Reduce red, Finish fin, int epi,
          Scal *S)
{
    Section sec(c, SEC_SPMV);      // halo exchange and the joins of deferred all-reduces included
    SpmvArgs a;
    a.fin = fin;
    a.epi = c->v;
    a.sell = c->sell; a.diag = c->diag; a.offd = c->offd;
    if (!c->jagw_fast) a.sell.lane_info = nullptr;      // BICG_PLAN="jagw=0": k_spmv_sell's loop instead of the three-trip product
    a.glist = nullptr;
    a.nrows = c->n_loc;
    a.diag_col16 = c->d_col16; a.rowsplit = c->rowsplit ? 1 : 0;
    a.desc = nullptr; a.nlist = 0;
    a.x = xin; a.y = yout; a.u = u; a.S = S ? S : c->S;
    Scal *const Sh = a.S;        // every kernel of this call reads the same scalar block
    a.nt = c->sell_nt ? 1 : 0;
    a.shift = c->cur_shift; a.has_shift = c->cur_has_shift ? 1 : 0;
    a.xcd_map = c->sell_xcd;
    // Consecutive products of a solve run over the matrix in alternating directions (BICG_SELL_ALT=0: always forward): matrix +
    // vectors of a Transport-sized system exceed the 256 MiB Infinity Cache by a quarter, so a product that starts where the
    // previous one ended finds the most recently streamed part of the matrix still cached, while cyclic forward passes
    // evict it just before it is needed. Rows, hence results of the product, are unaffected; the dot partials of a
    // reversed launch land in mirrored slots (a different, equally fixed association).
    a.reverse = (c->sell_alt && c->single()) ? (c->spmv_dir ^= 1) : 0;

    const SpmvShape shape = spmv_shape(c);
    SpmvCall call;
    call.ndot = ndot; call.epi = epi; call.has_shift = a.has_shift != 0; call.tail = red.tail_seq != 0; call.wave = red.wave != 0;
    const SpmvPlan plan = spmv_plan(shape, call);
    if (plan.error) die("internal", spmv_plan_error(plan.error));
    a.groups_per_wg = plan.groups_per_wg;
    red.expected = plan.expected; red.slot_base = 0;
    if (!plan.tail) red.tail_seq = 0;
    a.red = red;
    c->dots.producer_grid(red, plan.expected, plan.hand_nsh, plan.sets_nparts);

    // per-kernel timing: every SpMV kernel of this call gets its own start/stop event pair
    const bool timed = c->time_kernels && c->tev_used + 8 <= (int)c->tev.size();
    bool any_timed = false;
    auto run = [&](bool after_halo) {
        for (int i = 0; i < plan.nsteps; ++i) {
            if (plan.step[i].after_halo != after_halo) continue;
            if (!launch_step(c, a, plan.step[i], ndot, epi, timed ? c->tev[c->tev_used] : nullptr, timed ? c->tev[c->tev_used + 1] : nullptr)) continue;
            a.fin.seq = 0;          // the first kernel of this SpMV finished the open group
            if (timed) { c->tev_used += 2; any_timed = true; }
        }
    };

    const bool multi = !c->single(), host = hosted(c);
    unsigned seq = 0;
    bool send = true;
    hipEvent_t landed = nullptr;
    if (c->p2p) {
        seq = p2p_next_exchange(c, Sh);
        send = !(c->fault_after > 0 && seq >= (unsigned)c->fault_after);   // BICG_TEST="p2p-fault-after=n" (tests)
    }
    if (plan.fused) {
        // the exchange rides inside the first step's launch
        a.ll.ring = c->halo_ring; a.ll.halo = c->halo; a.ll.seq = seq;
        a.ll.nsend = send ? c->nsend : 0u;
        a.ll.npush = c->nsend ? std::min<unsigned>((c->nsend + kBlock - 1) / kBlock, 64u) : 0u;
        a.ll.first_bnd = c->ng_int;
        a.ll.send_idx = c->send_idx; a.ll.dst0 = c->push_dst0; a.ll.dstride = c->push_stride;
        a.ll.timeout_ticks = c->p2p->timeout_ticks;
    } else if (multi) {
        if (host) { c->cur_sub = 1; sec_remark(c); }      // the exchange: the reference's "agv" section (src/matrix.c:432)
        landed = halo_start(c, xin, Sh, seq, send, shape.own_stream);
        if (host) { c->cur_sub = 0; sec_remark(c); }
        if (host) c->dots.behind_halo();      // a deferred all-reduce starts behind the halo traffic
    }
    run(false);
    if (multi && !plan.fused) halo_land(c, xin, Sh, seq, landed);
    const bool second = host && !plan.merged;      // the rows that touch the halo: the reference's second mult() (src/matrix.c:440)
    if (second) { c->cur_sub = 2; sec_remark(c); }
    run(true);
    if (second) { c->cur_sub = 0; sec_remark(c); }
    c->dots.after_product();                      // ... and is joined here; peer-to-peer: collected and applied here
    if (a.fin.seq) {   // no SpMV kernel was launched (a rank without work): finish the group on its own
        Finish f = a.fin;
        f.roles |= FIN_BLOCK0;
        launch_finish(Launch{c->S, f, c->sc});
    }
    if (any_timed) c->spmv_calls_timed++;
}


// SpMV of the pipelined solvers (consumer-side finish): a deferred group of earlier kernels is staged
// by this launch; the SpMV's own dots (ndot > 0) open the next group.
void spmv_grp(bicg_ctx *c, double *xin, double *yout, int ndot, const double *u, int phase, int event)
{
    const Finish fin = c->dots.before_product(ndot > 0);
    Reduce red{};
    if (ndot > 0) red = c->dots.open(ndot, phase, event, 0, 0, true);
    spmv(c, xin, yout, ndot, u, red, fin);
    if (ndot > 0) c->dots.close();
}

// The halo exchange of spmv() on its own: afterwards xin[rows .. rows + halo) holds the other ranks' values.
void halo_only(bicg_ctx *c, double *xin)
{
    if (c->single() || (c->halo == 0 && c->nsend == 0)) return;
    const unsigned seq = c->p2p ? p2p_next_exchange(c, c->S) : 0u;
    halo_land(c, xin, c->S, seq, halo_start(c, xin, c->S, seq, true, false));
}

// The halo exchange of a set: nvec <= kSpmmCols vectors c->stride apart, ONE pack launch, ONE transport exchange, ONE unpack launch
// instead of nvec of each (on the host transport every exchange ends in a stream synchronisation, on RCCL it is a grouped send /
// recv). The buffers are peer-major (k_halo_pack_set), so the transport sees an ordinary exchange whose counts and displacements
// are the context's times nvec. The halo tails receive exactly the values halo_only delivers: the products do not change by a bit.
// Not for the peer-to-peer data path: its landing ring holds one vector per slot (spmm_pass keeps halo_only there).
void halo_set(bicg_ctx *c, double *in, int nvec)
{
    if (c->single() || (c->halo == 0 && c->nsend == 0)) return;      // (halo_only's rule: such a rank has no part in the exchange)
    if (!c->set_send) die("internal", "a set exchange without its buffers (spmm_buffers)");
    const int P = c->nranks;
    const std::vector<int> *src[4] = {&c->scnt, &c->sdsp, &c->rcnt, &c->rdsp};
    for (int q = 0; q < 4; ++q) {
        c->set_cnt[q].resize((size_t)P);
        for (int p = 0; p < P; ++p) c->set_cnt[q][(size_t)p] = nvec * (*src[q])[(size_t)p];
    }
    launch_halo_pack_set(in, c->stride, nvec, c->send_idx, c->set_smap, c->nsend, c->set_send, c->S, c->sc);
    ctx_exchange(c, c->set_send, c->set_cnt[0].data(), c->set_cnt[1].data(), c->set_recv, c->set_cnt[2].data(), c->set_cnt[3].data(), c->sc);
    // (in + n_loc + j * stride + i, i < halo <= stride - n_loc: every write stays inside its own vector, the 64 doubles of slack
    // behind the last vector of mm_in / mt_slab that k_spmm_pipe may read are never written)
    launch_halo_unpack_set(c->set_recv, c->set_rmap, c->halo, nvec, in + c->n_loc, c->stride, c->S, c->sc);
}

// Y_j = (A + sigma_j I) X_j for nvec <= kSpmmCols vectors that sit shift-major in c->mm_in: one pass over A.
// with_b: c->v.b holds b, c->mm_out receives || b - Y_j ||^2 (this rank's rows); otherwise c->mm_yt receives Y.
// the shifts of a pass go to the device BEFORE the pass is timed: the upload ends in a host-side wait (the values live on the
// caller's stack frame), which used to sit inside bicg_spmm's event bracket -- 30-40 us of an idle GPU counted as kernel time
void spmm_stage_sigma(bicg_ctx *c, int nvec, const double *sigma_host)
{
    double sg[kSpmmCols] = {0};
    for (int j = 0; j < nvec; ++j) sg[j] = sigma_host[j];
    BICG_HIP(hipMemcpyAsync(c->mm_sigma, sg, sizeof sg, hipMemcpyHostToDevice, c->sc));
    BICG_HIP(hipStreamSynchronize(c->sc));     // sg lives on this stack frame
}

// e0 / e1 (optional): stamped at the start / end of the SpMM KERNEL where the launch can carry them (the windowed and the pipelined
// form), else around the pass
// in / out (optional, bicg_multi.cpp): the shift-major input is read in place from `in` instead of c->mm_in, and the forms that
// write shift-major (windowed, pipelined) write to `out` instead of c->mm_yt; the row-major form leaves its result in c->mm_yt
void spmm_pass(bicg_ctx *c, int nvec, const double *sigma_host, bool with_b, bool sigma_staged, hipEvent_t e0, hipEvent_t e1,
               double *in, double *out)
{
    const size_t st = c->stride;
    if (!in) in = c->mm_in;
    if (!out) out = c->mm_yt;
    // the halos of the set in one exchange (BICG_PLAN="halo-set=0", read here: one exchange per vector, as on the peer-to-peer path)
    if (!c->single() && !c->p2p && nvec > 1 && !plan_off("halo-set")) halo_set(c, in, nvec);
    else for (int j = 0; j < nvec; ++j) halo_only(c, in + (size_t)j * st);
    // the windowed form (k_spmm_win) reads the shift-major vectors directly and writes Y shift-major into mm_yt
    const unsigned wslots = c->sell.win_slots ? c->sell.win_slots : (c->sell.col16 && !c->sell.jag && c->fw.ncl > 0 ? c->fw.slots : 0u);
    c->mm_win = c->mm_win_env != 0 && spmm_win_vectors(wslots) > 0;
    if (!c->mm_win) launch_rows_from_vectors(in, st, nvec, c->n_loc + c->halo, c->mm_xt, c->sc);
    SpmmArgs a{};
    a.sell = c->sell;
    a.sell.vbase = nullptr;      // sell_layout(): the SpMM kernels have no instantiation of the constant-slice layouts (they read val / col)
    a.dptr = c->diag.ptr; a.offd = c->offd;
    a.nrows = c->n_loc; a.ngroups = c->ng_int + c->ng_bnd;
    a.xt = c->mm_xt; a.yt = with_b ? nullptr : c->mm_yt; a.b = with_b ? c->v.b : nullptr; a.partial = c->mm_part;
    a.xcd_map = c->mm_xcd ? 1 : 0;
    if (sigma_host) {
        if (!sigma_staged) spmm_stage_sigma(c, nvec, sigma_host);
        a.sigma = c->mm_sigma;
    }
    c->mm_dma = false;
    c->mm_tile = 0;
    if (c->mm_win) {
        a.xs = in; a.ys = with_b ? nullptr : out; a.vstride = st; a.nvec = nvec; a.wslots = wslots;
        a.tail_most = c->jag_tail16_max;
        if (const char *sv = test_tok("spmm-skip")) a.dbg = atoi(sv);
        if (!c->sell.win_slots) a.cl = c->fw;
        // the pipelined form where the block qualifies (BICG_PLAN="spmm-window=1": k_spmm_win everywhere)
        c->mm_dma = c->mm_win_env == 3 && !a.dbg && launch_spmm_pipe(a, !c->single(), c->sc, e0, e1, &c->mm_tile) == hipSuccess;
        if (!c->mm_dma) c->mm_tile = 0;
        // ... and its form for ragged rows (jagged slices with x windows: bicg_spmm_jag.hip)
        if (!c->mm_dma && c->mm_win_env == 3 && c->sell.win_slots && c->win_near16) c->mm_dma = launch_spmm_jpipe(a, !c->single(), c->sc, e0, e1) == hipSuccess;
        if (!c->mm_dma && launch_spmm_win(a, !c->single(), c->sc, e0, e1) != hipSuccess) die("bicg_spmm", "the windowed kernel could not be launched (BICG_PLAN=spmm-window=0 selects the row-major form)");
    } else {
        if (e0) BICG_HIP(hipEventRecord(e0, c->sc));
        launch_spmm_sell(a, !c->single(), c->sc);
        if (e1) BICG_HIP(hipEventRecord(e1, c->sc));
    }
    if (with_b) launch_colsum(c->mm_part, spmm_grid(a.ngroups, a.xcd_map != 0), c->mm_out, c->sc);
}

// every row on the sliced-ELL path, and 32-bit byte offsets into the row-major X (128 B per row) suffice
bool spmm_possible(const bicg_ctx *c)
{
    // (x windows: the kernel keeps a group's runs in 64 LDS entries -- or reads the group's column list, round 6)
    return c->glist_all && c->nblk == 0 && c->sell_entries > 0 && (c->sell.win_max_runs <= 64 || c->sell.win_list) && (uint64_t)c->stride < (1ull << 25);
}

void spmm_buffers(bicg_ctx *c)
{
    if (c->mm_in) return;
    const size_t st = c->stride, ngroups = c->ng_int + c->ng_bnd;
    c->mm_in = c->own.alloc<double>((size_t)kSpmmCols * st + 64);      // (+64: k_spmm_pipe copies 16-byte pairs, the last one may reach one column past a vector)
    c->mm_xt = c->own.alloc<double>((size_t)kSpmmCols * st);
    c->mm_yt = c->own.alloc<double>((size_t)kSpmmCols * st);
    c->mm_part = c->own.alloc<double>((ngroups + 8) * kSpmmCols);
    c->mm_out = c->own.alloc<double>(kSpmmCols);
    c->mm_sigma = c->own.alloc<double>(kSpmmCols);
    if (!c->single() && (c->halo || c->nsend)) {      // the set exchange (halo_set)
        if ((uint64_t)kSpmmCols * std::max(c->halo, c->nsend) > 0x7fffffffull) die("bicg_spmm", "halo too long for a set exchange");
        c->set_send = c->own.alloc<double>((size_t)kSpmmCols * c->nsend);
        c->set_recv = c->own.alloc<double>((size_t)kSpmmCols * c->halo);
        std::vector<uint2> sm(c->nsend), rm(c->halo);
        for (int p = 0; p < c->nranks; ++p) {
            for (int i = 0; i < c->scnt[(size_t)p]; ++i) sm[(size_t)(c->sdsp[(size_t)p] + i)] = make_uint2((unsigned)c->sdsp[(size_t)p], (unsigned)c->scnt[(size_t)p]);
            for (int i = 0; i < c->rcnt[(size_t)p]; ++i) rm[(size_t)(c->rdsp[(size_t)p] + i)] = make_uint2((unsigned)c->rdsp[(size_t)p], (unsigned)c->rcnt[(size_t)p]);
        }
        c->set_smap = c->own.upload(sm.data(), sm.size());
        c->set_rmap = c->own.upload(rm.data(), rm.size());
    }
    BICG_HIP(hipMemset(c->mm_in, 0, sizeof(double) * kSpmmCols * st));
    BICG_HIP(hipDeviceSynchronize());      // the memset ran on the null stream: c->sc does not wait for it
    c->mm_xcd = !(knob_x("BICG_SPMM_XCD") && atoi(knob_x("BICG_SPMM_XCD")) == 0);
    c->mm_win_env = plan_tok("spmm-window") ? atoi(plan_tok("spmm-window")) : 3;      // 3: pipelined form where possible, else windowed
}

// SpMV whose epilogue runs a pipelined phase on the workgroup's own rows (k_spmv_sell_epi): the open dot group is
// summed by the launch's first workgroups and applied at the epilogue; the phase's own nd dots open the next group.
void spmv_epi(bicg_ctx *c, double *xin, double *yout, int epi, int nd, int phase, int event)
{
    const Launch L = c->dots.consume();
    Reduce red = c->dots.open(nd, phase, event);
    spmv(c, xin, yout, 0, nullptr, red, L.fin, epi, L.S);
    c->dots.close();
}

// Hand-over of plain BiCGStab's dot groups (struct Reduce / FIN_HAND): one rank, tail finish, eager launches, and every product of
// the iteration a single launch of k_spmv_sell on padded slices with 16-bit offsets and streamed values -- the layout whose
// product the hand-over epilogue leaves without scratch at eight wavefronts per SIMD (tests/test_handover_resources.py; the
// 32-bit layout keeps 12 bytes of it with two dots, the list-driven ones run at five or six wavefronts whatever their epilogue).
bool plain_handover(const bicg_ctx *c)
{
    DotShape s = c->dots.shape();      // switch and tables; here: the layout
    s.handover = s.handover && c->nblk == 0 && c->glist_all && c->sell_entries > 0 && !c->sell.jag && !c->sell.win_slots && c->sell.col16 &&
                 !c->sell.vbase && c->ng_bnd == 0 && c->n_int == 0 && c->n_bnd == 0 && !stencil_product(c);
    return dot_handover(s);
}

// the scalar block a solve starts from: tolerance, iteration limit, where the trace goes
Scal scal_block(const bicg_ctx *c, const bicg_options &o)
{
    Scal h;
    memset(&h, 0, sizeof h);
    h.tol2 = o.tol * o.tol;
    h.max_iter = o.max_iter;
    h.tr_alpha = c->trace;
    h.tr_omega = c->trace + c->trace_cap;
    h.tr_beta = c->trace + 2 * (size_t)c->trace_cap;
    h.tr_dotr = c->trace + 3 * (size_t)c->trace_cap;
    return h;
}

// ---------------------------------------------------------------- the four iterations
struct Driver {
    bicg_ctx *c;
    int method;
    Precond::Kind hat; // the preconditioner of the plain iteration: how the hat vectors p^ (v.z) and q^ (v.w) are formed, NONE: not at all
    int krr, nrr;
    Vecs &v;
    unsigned vg;       // workgroups of an element-wise kernel

    Driver(bicg_ctx *ctx, int m, int kr, int nr) : c(ctx), method(m), hat(precond_kind_of(m)), krr(kr), nrr(nr), v(ctx->v), vg(vec_grid(ctx->v.n)) {}

    // element-wise kernel without / with dots: it finishes the open group, then opens its own
    template <class Fn> void vec(Fn launch)
    {
        const Launch L = c->dots.consume();
        launch(v, L);
    }
    template <class Fn> void vec_dots(Fn launch, int n, int phase, int event)
    {
        const Launch L = c->dots.consume();
        const Reduce r = c->dots.open(n, phase, event, 0, vg);
        launch(v, L, r);
        c->dots.close();
    }

    // plain and CA-BiCGStab: ticket reductions, scalars applied in place by the producer's last workgroup
    Launch here() const { return Launch{c->S, Finish{}, c->sc}; }

    void init()
    {
        const bool plain = method == BICG_BICGSTAB || (hat != Precond::NONE && !kMethod[method].stab2);      // the plain iteration, preconditioned or not
        const bool rr = method == BICG_PIPE_BICGSTAB_RR || (method == BICG_PIPE_BICGSTAB && c->opt.rr_drift > 0.0);
        if (!c->dots.wave_mode) {
            spmv(c, v.x, v.ax, 0, nullptr, c->dots.no_dots());                       // Ax = A x0
            if (kMethod[method].stab2) {      // the plain set-up without p, and rho1 = (r#,r0): seeded from (r0,r0), since r# = r0 here; no hat vector yet
                launch_init_residual(v, false, false, here(), c->dots.open(1, PH_S2_INIT));
                c->dots.close();
                return;
            }
            // r = b - Ax, r# = r, (r,r); the plain iterations: p = r; DIAGONAL: and p^ = dinv o p in the same pass
            if (hat == Precond::DIAGONAL) launch_init_residual_diag(v, c->pc.planes, here(), c->dots.open(1, PH_INIT));
            else launch_init_residual(v, plain, rr, here(), c->dots.open(1, PH_INIT));
            c->dots.close();
            if (hat == Precond::BLOCK) precond_apply(c, v.p, v.z);                    // p^ = M^-1 p
            if (plain) return;
            spmv(c, v.r, v.w, 1, v.r, c->dots.open(1, PH_INIT_ALPHA));             // w = A r, (r,w)
            c->dots.close();
            return;
        }
        spmv_grp(c, v.x, v.ax);                                                    // Ax = A x0
        vec_dots([&](const Vecs &vv, const Launch &L, Reduce r) { launch_init_residual(vv, plain, rr, L, r); }, 1, PH_INIT, DOT_NOW);
        spmv_grp(c, v.r, v.w, 1, v.r, PH_INIT_ALPHA, DOT_DEFER);                   // w = A r, (r,w); overlaps t = A w (src/solver.c:339-343)
        spmv_grp(c, v.w, v.t);
        c->dots.flush();
    }

    bool handover() const { return plain_handover(c); }
    // Plain BiCGStab, as it stands or right-preconditioned (`hat`; DESIGN.md sections 4.20, 4.21): one sequence of operations, dot
    // groups and phases. Preconditioned, the products take the hat vectors p^ = M^-1 p (v.z) and q^ = M^-1 q (v.w) -- idle in the
    // plain iteration, zeroed with their halo tails by run_begin -- and x is updated with them; r stays the residual of the caller's
    // system. DIAGONAL forms them in the pass that produces q / p (no launch added). BLOCK cannot: p is updated in place and a row's
    // block-mates live in other lanes or workgroups, so each takes a launch of k_bjac_apply (seven launches), which writes v.z / v.w
    // only -- iterations enqueued behind a converged one change neither x, r nor the scalars. Both always run the multi-launch form
    // with the producer-side finish: the hand-over is the unpreconditioned method's alone.
    void iter_plain()   // reference src/solver.c:88-119
    {
        if (hat == Precond::NONE && handover()) {
            DotGroups &d = c->dots;
            spmv(c, v.p, v.s, 1, v.rh, d.open_hand(1, PH_PLAIN_ALPHA));       // s = A p, (r#,s)
            launch_plain_q(v, d.consume_hand());                              // -> alpha ; q = r - alpha s
            spmv(c, v.r, v.y, 2, v.r, d.open_hand(2, PH_OMEGA));              // y = A q, (q,y), (y,y)
            const Launch L = d.consume_hand();                                // -> omega ; x, r, (r,r), (r#,r)
            launch_plain_xr(v, L, d.open_hand(2, PH_PLAIN_END, vg));
            launch_plain_p(v, d.consume_hand());                              // -> beta, k++ ; p = r + beta (p - omega s)
            return;
        }
        const double *dinv = c->pc.planes;
        spmv(c, hat ? v.z : v.p, v.s, 1, v.rh, c->dots.open(1, PH_PLAIN_ALPHA));   // s = A p (A p^), (r#,s) -> alpha
        c->dots.close();
        if (hat == Precond::DIAGONAL) launch_diag_q(v, dinv, here());   // q = r - alpha s (in v.r) ; q^ = dinv o q
        else launch_plain_q(v, here());
        if (hat == Precond::BLOCK) precond_apply(c, v.r, v.w);          // q^ = M^-1 q
        spmv(c, hat ? v.w : v.r, v.y, 2, v.r, c->dots.open(2, PH_OMEGA));          // y = A q (A q^), (q,y), (y,y) -> omega
        c->dots.close();
        // x += alpha p + omega q (alpha p^ + omega q^), r, (r,r), (r#,r) -> beta, k++
        if (hat) launch_diag_xr(v, here(), c->dots.open(2, PH_PLAIN_END));
        else launch_plain_xr(v, here(), c->dots.open(2, PH_PLAIN_END));
        c->dots.close();
        if (hat == Precond::DIAGONAL) launch_diag_p(v, dinv, here());   // p = r + beta (p - omega s) ; p^ = dinv o p
        else launch_plain_p(v, here());
        if (hat == Precond::BLOCK) precond_apply(c, v.p, v.z);          // p^ = M^-1 p
    }

    // One sweep of BiCGStab(2) = two BiCG steps and the two-dimensional minimal-residual step, as it stands or right-preconditioned
    // (`hat`: the sweep on A M^-1; the algorithm: include/bicgstab_hip.h at BICG_BICGSTAB2 and BICG_BICGSTAB2_DIAG / _BLOCK; launches, dot
    // groups and bytes per row: DESIGN.md sections 4.23, 4.24): one sequence of operations, dot groups and phases. The vectors live in
    // the slab's work vectors, all zeroed with their halo tails by run_begin, which defines u0 = u1 = u2 = 0:
    //   r0 = v.r   r# = v.rh   u0 = v.p   u1 = v.s   u2 = v.z   r1 = v.y   r2 = v.w   (the set-up's A x0: v.ax; idle without a hat: v.v, v.t, v.b)
    // rho0 / rho1 are Scal::rTr_old / rTr, g2 is Scal::omega, g1 sits in Scal::red[kRedG1]. Ten launches, five dot groups:
    // the three products with (r#, out) close a group each, the MR group's five sums come from three producers -- V4 and the product
    // r2 = A r1 contribute, the dot pass closes --, and V5 closes the sweep's last one. Always ticket groups, producer-side finish.
    // Preconditioned, the products' outputs, dot groups and phases are the same; the products take the hat vectors, x is updated with
    // them, r0 stays the residual of the caller's system. The hats live in the four vectors that are idle otherwise:
    //   u^0 = v.v   u^1 = v.t   r^0 = v.b   r^1 = v.ax (the set-up is done with A x0 by then)
    // each written over all local rows before its first read in the first sweep (V1, V2, V3, V4 in this order), halo tails zeroed by
    // run_begin and filled by the products' exchanges. Four applications of M^-1 per sweep -- u^0, r^0, u^1, r^1, in the pass that
    // produces the vector (DIAGONAL: ten launches) or by a launch of k_bjac_apply behind it (BLOCK: fourteen), which writes the hat
    // only: sweeps enqueued behind a stopped solve change neither x, r nor a scalar -- and two recurrences (u^0 in V3, r^0 in V4)
    // that feed x alone.
    void iter_stab2()
    {
        DotGroups &d = c->dots;
        const bool blk = hat == Precond::BLOCK;
        const double *dinv = hat == Precond::DIAGONAL ? c->pc.planes : nullptr;
        launch_stab2_u0(v, hat, dinv, here());                                  // V1: u0 = r0 - beta u0 ; u^0 = M^-1 u0
        if (blk) precond_apply(c, v.p, v.v);
        spmv(c, hat ? v.v : v.p, v.s, 1, v.rh, d.open(1, PH_S2_ALPHA0)); d.close();   // u1 = A u0 (A u^0), (r#,u1) -> alpha
        launch_stab2_r0(v, hat, dinv, here());                                  // V2: r0 -= alpha u1 ; r^0 = M^-1 r0
        if (blk) precond_apply(c, v.r, v.b);
        spmv(c, hat ? v.b : v.r, v.y, 1, v.rh, d.open(1, PH_S2_BETA)); d.close();     // r1 = A r0 (A r^0), (r#,r1) -> rho1, beta
        launch_stab2_xu(v, hat, dinv, here());                                  // V3: x += alpha u0 (u^0; j = 0) ; u0, u^0, u1 ; u^1 = M^-1 u1
        if (blk) precond_apply(c, v.s, v.t);
        spmv(c, hat ? v.t : v.s, v.z, 1, v.rh, d.open(1, PH_S2_ALPHA1)); d.close();   // u2 = A u1 (A u^1), (r#,u2) -> alpha
        launch_stab2_xrr(v, hat, dinv, here(), d.contribute(0, false));         // V4: x, r0, r^0, r1 ; r^1 = M^-1 r1 ; (r1,r1), (r0,r1) -> red[0], red[1]
        if (blk) precond_apply(c, v.y, v.ax);
        spmv(c, hat ? v.ax : v.y, v.w, 2, v.y, d.contribute(2, false));         // r2 = A r1 (A r^1), (r1,r2), (r2,r2) -> red[2], red[3]
        launch_stab2_dot(v, here(), d.open(5, PH_S2_MR, DOT_NOW, 4)); d.close();   // D: (r0,r2) -> red[4] ; the five -> g1, g2
        launch_stab2_mr(v, hat, here(), d.open(2, PH_S2_END)); d.close();       // V5: x (with r^0, r^1), r0, u0 ; (r0,r0), (r#,r0) -> dot_r, rho1, k += 2
    }

    void iter_ca()      // reference src/solver.c:217-251
    {
        launch_ca_ps(v, here());                                // p, s recurrences
        if (c->ca_fuse && c->single() && stencil_product(c) && !c->cur_has_shift) {
            // z = A s with q = r - alpha s, y = w - alpha z, (q,y), (y,y) on the product's own rows: s_i and z_i are registers there
            spmv(c, v.s, v.z, 2, nullptr, c->dots.open(2, PH_OMEGA), Finish{}, 3);
        } else {
            spmv(c, v.s, v.z, 0, nullptr, c->dots.no_dots());   // z = A s
            launch_qy(v, here(), c->dots.open(2, PH_OMEGA)); // q, y, (q,y), (y,y) -> omega
        }
        c->dots.close();
        launch_ca_xr(v, here(), c->dots.contribute(0, false));     // x, r, (r,r), (r#,r), (r#,s), (r#,z)
        spmv(c, v.r, v.w, 1, v.rh, c->dots.open(5, PH_RECUR_END, DOT_NOW, 2));     // w = A r, (r#,w) -> beta, alpha, k++
        c->dots.close();
    }

    bool replaces(int it) const { return method == BICG_PIPE_BICGSTAB_RR && krr > 0 && (it % krr == 0) && it > 0 && it <= krr * nrr; }
    // two launches per iteration (phases in the SpMV epilogues): every row on the sliced-ELL path and a single
    // SpMV launch per product (one rank, or the peer-to-peer exchange folded into the launch)
    bool fused() const
    {
        return c->fuse_pipe && c->dots.wave_mode && !hosted(c) && c->fuse_plan_ok;
    }

    // last: the caller looks at x / r after this iteration (end of a run_iterate call, adaptive replacement check):
    // phase 1 of the next iteration, which overwrites r with q, must not have run yet
    void iter_pipe(int it, bool force_replace, bool last)   // reference src/solver.c:352-390 and 494-548
    {
        const bool replace = force_replace || replaces(it);
        if (!replace) {
            if (!c->f1_done) {
                vec_dots(launch_pipe_f1, 2, PH_OMEGA, DOT_DEFER);                   // p, s, z, q, y, (q,y), (y,y)
            }
            c->f1_done = false;
            if (fused()) {
                spmv_epi(c, v.z, v.v, 1, 5, PH_RECUR_END, DOT_DEFER);               // v = A z ; x, r, w, five dots   || all-reduce of (q,y), (y,y)
                if (!last && !replaces(it + 1)) {
                    spmv_epi(c, v.w, v.t, 2, 2, PH_OMEGA, DOT_DEFER);               // t = A w ; phase 1 of iteration it + 1   || all-reduce of the five
                    c->f1_done = true;
                } else {
                    spmv_grp(c, v.w, v.t);                               // t = A w   || all-reduce
                }
            } else {
                spmv_grp(c, v.z, v.v);                                   // v = A z   || all-reduce
                vec_dots(launch_pipe_f2, 5, PH_RECUR_END, DOT_DEFER);               // x, r, w, five dots
                spmv_grp(c, v.w, v.t);                                   // t = A w   || all-reduce
            }
        } else {
            if (c->f1_done) die("internal", "replacement step after phase 1 of the same iteration has run");
            vec(launch_p_update);
            spmv_grp(c, v.p, v.s);                                   // s = A p
            spmv_grp(c, v.s, v.z);                                   // z = A s
            vec_dots(launch_qy, 2, PH_OMEGA, DOT_DEFER);
            spmv_grp(c, v.z, v.v);                                   // v = A z
            vec(launch_x_update);
            spmv_grp(c, v.x, v.ax);                                  // Ax = A x
            vec(launch_true_residual);                               // r = b - Ax
            spmv_grp(c, v.r, v.w);                                   // w = A r
            vec_dots(launch_dots5, 5, PH_RECUR_END, DOT_DEFER);
            spmv_grp(c, v.w, v.t);                                   // t = A w
        }
        c->dots.flush();
    }

    void iterate(int it, bool force_replace = false, bool last = true)
    {
        switch (method) {
        case BICG_BICGSTAB: case BICG_BICGSTAB_DIAG: case BICG_BICGSTAB_BLOCK: iter_plain(); break;
        case BICG_CA_BICGSTAB: iter_ca(); break;
        case BICG_BICGSTAB2: case BICG_BICGSTAB2_DIAG: case BICG_BICGSTAB2_BLOCK: iter_stab2(); break;
        default: iter_pipe(it, force_replace, last); break;
        }
    }

    // adaptive residual replacement (additive): true residual vs recursive one
    double drift()
    {
        spmv_grp(c, v.x, v.ax);
        vec_dots(launch_drift, 2, PH_NONE, DOT_NOW);
        fetch_scal(c);
        return c->hS->red[1] > 0.0 ? sqrt(c->hS->red[0] / c->hS->red[1]) : 0.0;
    }
};

// a fresh scalar block and ticket counters for a stand-alone kernel (bicg_spmv, bicg_dot, the form probe)
void scal_reset(bicg_ctx *c)
{
    c->spmv_dir = 0;             // stand-alone products and dots: always the same direction, whatever ran before
    c->dots.reset(false);
}
bool all_ranks(Comm *comm, bool mine);

void fetch_scal(bicg_ctx *c)
{
    c->dots.force();                     // the host wants the scalars: finish the open wave group now
    BICG_HIP(hipMemcpyAsync(c->hS, c->S, sizeof(Scal), hipMemcpyDeviceToHost, c->sc));
    if (c->p2p || c->persist_on) BICG_HIP(hipMemcpyAsync(c->h_alarm, c->alarm, sizeof(int), hipMemcpyDeviceToHost, c->sc));
    BICG_HIP(hipStreamSynchronize(c->sc));
    if (c->sm) BICG_HIP(hipStreamSynchronize(c->sm));
    if (c->hS->comm_error || ((c->p2p || c->persist_on) && *c->h_alarm)) {
        c->hS->comm_error = 1; c->hS->done = 1;
        // BICG_P2P_SOFT_FAIL=1: report through bicg_comm_failed() and stop iterating instead of
        // exiting (bench.py then falls back to the RCCL collectives)
        const char *soft = getenv("BICG_P2P_SOFT_FAIL");
        // no peer-to-peer path: the only waits are those between the workgroups of a persistent launch (they spin on each other
        // and need to be co-resident: another long-running kernel on the same GPU can starve them) or, in every other launch, those
        // of a dot group's finishing workgroups on its producers
        if (!c->p2p && !c->soft_fail && (!soft || atoi(soft) == 0) && !c->persist_on)
            die("dot group", "the producers of a dot group never delivered their partial sums: the workgroups that finish the group "
                             "gave up waiting for them (tail finish; BICG_TAIL_FINISH=0 selects arrival tickets)");
        if (!c->p2p && !c->soft_fail && (!soft || atoi(soft) == 0))
            die("persistent kernel", "workgroups waited for each other longer than the time-out -- is another kernel holding CUs of this GPU? "
                                     "(BICG_PERSIST=0 selects the multi-launch iteration)");
        if (!c->soft_fail && (!soft || atoi(soft) == 0))
            die("peer-to-peer transport", "timed out waiting for another rank (BICG_P2P_TIMEOUT_MS)");
        if (!c->comm_failed)
            fprintf(stderr, "bicgstab_hip: rank %d: peer-to-peer transport timed out waiting for another rank\n", c->rank);
        c->comm_failed = true;
    }
}

// A solve in three steps so that callers (and bench.py) can time exactly K iterations:
// run_begin = set-up phase of the reference (src/solver.c:74-83 etc.), run_iterate = up to n more
// iterations of its while loop, run_end = summary lines and result.
void run_begin(bicg_ctx *c, int method, const bicg_options *opt_in)
{
    bicg_options &o = c->opt;
    if (opt_in) o = *opt_in; else bicg_default_options(&o);
    if (method < 0 || method >= kMethods) die("bicg_run", "unknown method");
    if (diag_refused(c, method))
        die("bicg_run", precond_kind_of(method) == Precond::DIAGONAL ? "a diagonally preconditioned method without its preconditioner (bicg_precond_diagonal)"
                                                                     : "a block-Jacobi preconditioned method without its preconditioner (bicg_precond_block_diagonal)");
    if (o.max_iter < 0) o.max_iter = 0;
    if (o.check_every < 1) o.check_every = 1;
    c->method = method;
    use_device(c);
    // Plain and CA-BiCGStab need every scalar right after the kernel that produces its sums: the ticket
    // chain at the end of the producer (memory system draining) is then the shortest path. The
    // pipelined solvers defer their groups across an SpMV (src/solver.c:363-367, 377-385): there the sums
    // are staged by that SpMV and finished by the kernel that consumes them, off the critical path.
    c->f1_done = false;
    c->spmv_dir = 0;             // every solve starts in the same direction (its first product toggles this to 1 = reversed):
                                 // run-to-run bit reproducibility, also with several groups per workgroup
    // Matrix stream policy. The Infinity Cache (256 MiB) is shared by the matrix stream and the
    // solver's vectors. If matrix + vectors exceed it by less than ~25 % ordinary loads win: a good
    // part of the matrix survives from one SpMV to the next (Transport, plain: 149.5 vs 155.0 us
    // per iteration). Beyond that the matrix only evicts the vectors and is streamed with
    // non-temporal loads instead (Transport, pipelined, 10 vectors: 167.3 vs 173.8 us).
    {
        // (kMethod counts the vectors; the planes of a block preconditioner come on top, a diagonal is already counted)
        const double ws = (double)c->matrix_bytes + 8.0 * c->stride * (kMethod[method].nvec + (kMethod[method].precond == Precond::BLOCK ? c->pc.bs : 0));
        // (round 4: with the products alternating direction, ordinary loads pay up to 35 % over the cache -- CA-BiCGStab
        // 166.9 -> 150.6 us per iteration; the pipelined solvers' ten vectors are past that: 157.2 vs 160.9)
        // (round 5, the products of rounds 4-5 and an irregular matrix: ordinary loads win far beyond that -- FEM-like, 1.6 M rows,
        // pipelined, 1.42 x the cache: 161 against 180 us; 2.4 M rows plain 1.85 x: 220 against 239; 3.2 M rows plain 2.47 x: 294
        // against 306, pipelined 2.85 x: 338 against 325 -- the cross-over is near 2.5 x: profiles/r05/ab_matrix_stream_policy.txt)
        c->sell_nt = ws > (c->sell_alt ? 2.5 : 1.25) * 256.0 * 1048576.0;
        if (c->sell_nt_env >= 0) c->sell_nt = c->sell_nt_env != 0;
    }

    // trace storage: the (r,r) history is always kept (progress lines), 4 arrays of max_iter
    if (c->trace_cap < o.max_iter) {
        c->trace_cap = o.max_iter > 0 ? o.max_iter : 1;
        c->trace = c->own.regrow(c->trace, 4 * (size_t)c->trace_cap);
    }
    const Scal h = scal_block(c, o);
    c->dots.reset(kMethod[method].pipelined, &h, true);
    BICG_HIP(hipMemsetAsync(c->alarm, 0, sizeof(int), c->sc));
    if (c->waitlog) BICG_HIP(hipMemsetAsync(c->waitlog, 0, sizeof(unsigned) * 3 * kWaitCap, c->sc));
    // every work vector starts at zero: defines the reads of p, s, z, v that the reference makes
    // before writing them (src/solver.c:217-222, 352-360) and keeps halo tails finite
    const size_t st = c->stride;
    BICG_HIP(hipMemsetAsync(c->slab + 2 * st, 0, sizeof(double) * 10 * st, c->sc));
    c->time_kernels = (o.time_kernels & 1) != 0;
    sec_begin(c, (o.time_kernels & 2) != 0); c->sec_dump = (o.time_kernels & 4) != 0;
    c->tev_used = 0; c->spmv_calls_timed = 0;
    if (c->time_kernels && c->tev.empty()) {
        c->tev.resize(kMaxTimed);
        for (auto &e : c->tev) BICG_HIP(hipEventCreate(&e));
    }
    BICG_HIP(hipStreamSynchronize(c->sc));

    c->it = 0; c->printed = 0; c->t_iter = 0.0; c->adaptive_rr = 0;
    c->t_begin = now_sec();
    Driver d(c, method, o.krr, o.nrr);
    d.init();
    fetch_scal(c);
    c->t_init = now_sec() - c->t_begin;
}

// hipGraph replay of one iteration. The iteration body is a fixed sequence of launches (and, across
// ranks, RCCL calls on the communication stream joined back by events), identical from one
// iteration to the next except for pipe_bicgstab_rr's replacement steps, so it is captured once
// per method and replayed: one graph launch instead of 5-17 enqueue calls per iteration. This is
// what keeps an 8-GPU run (20-25 us of GPU work per iteration) from being bound by the host's
// ~3-4 us per launch. Two eager iterations come first so that every lazy initialisation (RCCL
// connections, kernel loading) happens outside the capture. Returns false when the caller has to
// run the iteration eagerly.
bool graph_iteration(bicg_ctx *c, Driver &d)
{
    const int m = c->method;
    // Off unless BICG_GRAPH=1: measured on one MI355X, eager in-order enqueueing already keeps the
    // GPU busy (54 us vs 60 us replayed per 17-op iteration of a 200 k-row rank); replay only pays
    // when the two-stream overlap mode is on (80 vs 105 us).
    const bool want = c->graph_mode == 1 && !kMethod[m].stab2;      // (BiCGStab(2), preconditioned or not, has no captured iteration: it runs eagerly)
    // consumer-side finish alternates between two scalar blocks: launch arguments change from one
    // iteration to the next unless the host enqueues the collectives itself
    if (c->dots.wave_mode && !hosted(c)) return false;
    if (!want || c->p2p || m == BICG_PIPE_BICGSTAB_RR || c->opt.rr_drift > 0.0 || c->time_kernels || c->time_sections || c->sec_exhausted ||
        !c->comm->stream_ordered()) return false;
    if (c->graph_exec[m] && c->graph_nt[m] != c->sell_nt) {     // captured with the other streaming policy
        (void)hipGraphExecDestroy(c->graph_exec[m]);
        c->graph_exec[m] = nullptr;
    }
    if (!c->graph_exec[m]) {
        if (c->graph_warm[m] < 2) { c->graph_warm[m]++; return false; }
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(c->sc, hipStreamCaptureModeThreadLocal) != hipSuccess) { c->graph_mode = 0; return false; }
        d.iterate(c->it, false, true);
        const hipError_t e = hipStreamEndCapture(c->sc, &g);
        if (e != hipSuccess || !g) {
            fprintf(stderr, "bicgstab_hip: graph capture failed (%s); continuing with eager launches\n", hipGetErrorString(e));
            (void)hipGetLastError();
            c->graph_mode = 0;
            return false;   // nothing was executed during the failed capture
        }
        const hipError_t e2 = hipGraphInstantiate(&c->graph_exec[m], g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e2 != hipSuccess) { c->graph_exec[m] = nullptr; c->graph_mode = 0; return false; }
        c->graph_nt[m] = c->sell_nt;
    }
    BICG_HIP(hipGraphLaunch(c->graph_exec[m], c->sc));
    return true;
}

// What every persistent launch is told besides its vectors: patience, workgroup order, and where its sequence numbers start.
// fixed_iters: the iterations of a kernel that uses `groups` dot groups (tags, mailbox numbers) and two exchanges per iteration,
// converged early or not -- every rank advances its numbers by the whole chunk here. 0: the pipelined kernels number hand-offs
// and groups densely and report what they used (replacement iterations and drift checks make the count data dependent):
// persist_account() advances the counters after the launch.
void persist_args(bicg_ctx *c, PersistArgs &a, unsigned groups, unsigned fixed_iters)
{
    a.timeout_ticks = c->p2p ? c->p2p->timeout_ticks : 200000000ull;          // 2 s inside one GPU
    static const int xcd_map = knob_x("BICG_PERSIST_XCD") ? atoi(knob_x("BICG_PERSIST_XCD")) : 1;
    a.xcd_map = xcd_map;
    static const int first_sleep = knob_x("BICG_PERSIST_SLEEP") ? atoi(knob_x("BICG_PERSIST_SLEEP")) : 1;
    a.first_sleep = (unsigned)first_sleep;
    c->persist_seq += groups * fixed_iters;
    if (a.multi) {
        a.halo_seq0 = c->halo_seq;
        a.p2p = c->p2p->red_desc(c->p2p->red_seq);
        c->halo_seq += 2u * fixed_iters; c->p2p->red_seq += groups * fixed_iters;
        a.ring = c->halo_ring;
        c->halo_unsynced = 0;
    }
}

// niter iterations of pipe_bicgstab in one launch (the open dot group has been closed: fetch_scal precedes every chunk)
bool persist_chunk(bicg_ctx *c, int niter)
{
    if (c->dots.is_open()) die("internal", "persistent chunk with an open dot group");
    if (c->f1_done) die("internal", "persistent chunk after phase 1 of the next iteration has run");
    const bool plain = c->method == BICG_BICGSTAB;
    const bool pipe = kMethod[c->method].pipelined;
    const unsigned groups = plain ? 3u : 2u;                  // dot groups (tags, mailbox numbers) per iteration
    PersistArgs a = c->persist;
    a.v = c->v; a.S = c->S; a.alarm = c->alarm; a.niter = niter;
    a.seq0 = c->persist_seq;
    a.vseq0 = c->persist_vseq;
    a.it0 = c->it;
    a.krr = c->method == BICG_PIPE_BICGSTAB_RR ? c->opt.krr : 0; a.nrr = c->opt.nrr;
    a.force_first = 0;
    a.drift_every = (pipe && c->opt.rr_drift > 0.0) ? c->opt.check_every : 0;
    a.drift_tol2 = c->opt.rr_drift * c->opt.rr_drift;
    persist_args(c, a, groups, pipe ? 0u : (unsigned)niter);
    if (a.multi) {
        if (!c->waitlog) { c->waitlog = c->own.alloc<unsigned>(3 * (size_t)kWaitCap); BICG_HIP(hipMemsetAsync(c->waitlog, 0, sizeof(unsigned) * 3 * kWaitCap, c->sc)); }
        a.waitlog = c->waitlog; a.waitcap = kWaitCap;
    }
    static const bool want_trace = knob_x("BICG_PERSIST_TRACE") != nullptr;
    unsigned long long *dbg = nullptr;
    if (want_trace) {
        dbg = dev_alloc<unsigned long long>(64 * 16);
        BICG_HIP(hipMemset(dbg, 0, 64 * 16 * sizeof(unsigned long long)));
        a.dbg = dbg;
    }
    hipError_t err;
    if (plain) err = launch_plain_persist(a, c->sc);
    else if (c->method == BICG_CA_BICGSTAB) err = launch_ca_persist(a, c->sc);
    else err = launch_pipe_persist(a, c->sc);
    if (err != hipSuccess) {
        // nothing ran: hand the chunk back to the multi-launch kernels (every rank sees the same failure: same kernel, same
        // plan limits; the sequence numbers reserved above are simply skipped on all of them)
        dev_free(dbg, false);
        if (c->nranks > 1) die("persistent kernel", "launch failed on a multi-rank run (BICG_PERSIST=0 selects the multi-launch iteration)");
        fprintf(stderr, "bicgstab_hip: falling back to the multi-launch iteration\n");
        c->persist_on = false;
        return false;
    }
    if (want_trace && c->method != BICG_PIPE_BICGSTAB) { BICG_HIP(hipStreamSynchronize(c->sc)); dev_free(dbg); }
    if (want_trace && c->method == BICG_PIPE_BICGSTAB) {
        // 10 ns ticks of one row workgroup (0 start, 1 z and partials published, 2 window staged, 3 product done, 4 omega here,
        // 5 w and partials published, 6 window, 7 product, 8 scalars here) and of the helper (10 / 11: group 1 / 2 published)
        std::vector<unsigned long long> h(64 * 16);
        BICG_HIP(hipStreamSynchronize(c->sc));
        BICG_HIP(hipMemcpy(h.data(), dbg, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        dev_free(dbg);
        for (int it = std::max(0, std::min(niter, 32) - 5); it < std::min(niter, 32); ++it)
            for (int who = 0; who < 2; ++who) {
                const unsigned long long *q = h.data() + (size_t)(it * 2 + who) * 16, *q0 = h.data() + (size_t)(it * 2) * 16;
                fprintf(stderr, "persist trace it %2d %s:", it, who ? "comm" : "row ");
                for (int i = 0; i <= 8; ++i) fprintf(stderr, " %d:%+.2f", i, 0.01 * (double)(long long)(q[i] - q0[0]));
                if (!who) fprintf(stderr, "  helper g1 %+.2f g2 %+.2f", 0.01 * (double)(long long)(q[10] - q0[0]), 0.01 * (double)(long long)(q[11] - q0[0]));
                else fprintf(stderr, "  helper g1: arrived %+.2f summed %+.2f applied %+.2f", 0.01 * (double)(long long)(q[12] - q0[0]),
                             0.01 * (double)(long long)(q[13] - q0[0]), 0.01 * (double)(long long)(q[14] - q0[0]));
                fprintf(stderr, "\n");
            }
    }
    return true;
}

// after a pipelined persistent launch (fetch_scal has brought the scalar block back): advance the sequence counters by what
// the launch consumed. Identical on every rank -- the decisions inside the launch depend on globally reduced sums only.
void persist_account(bicg_ctx *c)
{
    const unsigned nv = (unsigned)c->hS->red[kRedUsedV], ng = (unsigned)c->hS->red[kRedUsedG];
    c->persist_seq += ng;
    c->persist_vseq += nv;
    if (!c->single()) { c->halo_seq += nv; c->p2p->red_seq += ng; }
    c->adaptive_rr += (int)c->hS->red[kRedAdaptive];
}

int run_iterate(bicg_ctx *c, int nsteps)
{
    const bicg_options &o = c->opt;
    use_device(c);
    Driver d(c, c->method, o.krr, o.nrr);
    const bool talk = c->rank == 0 && !o.quiet;
    const double t0 = now_sec();
    const int stop = std::min(o.max_iter, c->it + std::max(nsteps, 0));
    while (!c->hS->done && c->it < stop) {
        // (section marks are host-side events between launches: the multi-launch forms are what they can time)
        const bool pipe = kMethod[c->method].pipelined;
        bool persist = kMethod[c->method].persist && c->persist_on && !c->time_kernels && !c->time_sections && !c->sec_exhausted &&
                             ((pipe && (c->persist.rpt == 1u || (c->method == BICG_PIPE_BICGSTAB && o.rr_drift <= 0.0))) ||
                              (!pipe && c->persist_plain && (c->persist.rpt == 1u || (c->persist.rpt == 2u && !c->persist.mat_entries))));
        // A persistent launch costs ~27 us of set-up (matrix slices and x window into LDS) and stops by itself at
        // convergence: it covers at least kPersistChunk iterations whatever the host check interval (200 k-row rank,
        // pipelined: 12.5 us per iteration at 16 per launch, 11.0 at 128, 10.9 at 512 -- tools/persist_chunk_times.py)
        const int persist_chunk_min = knob_tok("BICG_PERSIST", "chunk") ? std::max(1, atoi(knob_tok("BICG_PERSIST", "chunk"))) : kPersistChunk;
        const int chunk = std::min(persist ? std::max(o.check_every, persist_chunk_min) : o.check_every, stop - c->it);
        bool force = false;
        // (the persistent kernel checks the drift itself, every check_every iterations inside the launch)
        if (!persist && o.rr_drift > 0.0 && (c->method == BICG_PIPE_BICGSTAB || c->method == BICG_PIPE_BICGSTAB_RR) && c->it > 0 && d.drift() > o.rr_drift) {
            force = true;
            c->adaptive_rr++;
        }
        sec_mark(c, SEC_VEC);
        const double t_chunk = now_sec();
        if (persist) persist = persist_chunk(c, chunk);   // one launch for the whole chunk (bicg_persist.hip); false: it could not be launched
        int steps = chunk;      // what the chunk advances c->it by
        if (kMethod[c->method].stab2) {      // steps come in pairs: ceil(chunk / 2) sweeps (the device's loop condition keeps k <= max_iter)
            const int sweeps = (chunk + 1) / 2;
            for (int j = 0; j < sweeps; ++j) d.iterate(c->it + 2 * j, false, j == sweeps - 1);
            steps = 2 * sweeps;
        } else if (!persist) {
            for (int j = 0; j < chunk; ++j) {
                // the last iteration before the caller (or the drift check) reads x / r leaves them as the reference would
                const bool last = j == chunk - 1 && (c->it + chunk >= stop || o.rr_drift > 0.0);
                if (j == 0 && force) { d.iterate(c->it, true, last); continue; }
                if (!graph_iteration(c, d)) d.iterate(c->it + j, false, last);
            }
        }
        c->it += steps;
        sec_mark(c, SEC_STOP);
        c->t_enq += now_sec() - t_chunk;          // (bicg_run_iterate_timed: host time until the chunk's launches were enqueued)
        fetch_scal(c);
        if (persist && pipe) persist_account(c);
        if (talk && o.out_iter > 0) {   // reference src/solver.c:122-126
            const int k = c->hS->k;
            const int upto = (k / o.out_iter) * o.out_iter;
            if (upto > c->printed) {
                std::vector<double> hist(k);
                BICG_HIP(hipMemcpy(hist.data(), c->trace + 3 * (size_t)c->trace_cap, sizeof(double) * k, hipMemcpyDeviceToHost));
                for (int q = c->printed + o.out_iter; q <= upto; q += o.out_iter)
                    printf("Iteration: %d, Residual: %e\n", q, sqrt(hist[q - 1] / c->hS->dot_zero));
                c->printed = upto;
            }
        }
    }
    c->t_iter += now_sec() - t0;
    return c->hS->k;
}

int run_end(bicg_ctx *c, bicg_result *res)
{
    const bicg_options &o = c->opt;
    // (a drop-in solve that lost its peer-to-peer path is about to be repeated: no summary of the aborted attempt)
    const bool talk = c->rank == 0 && !o.quiet && !(c->comm_failed && c->soft_fail);
    const int k = c->hS->k;
    c->last_iters = k;
    double spmv_ms = 0.0;
    int spmv_n = 0;
    if (c->time_kernels) {
        for (int i = 0; i + 1 < c->tev_used; i += 2) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->tev[i], c->tev[i + 1]) == hipSuccess) spmv_ms += ms;
        }
        spmv_n = c->spmv_calls_timed;
    }
    sec_collect(c, k);
    const double total = c->t_init + c->t_iter;
    if (res) {
        res->iterations = k;
        res->dot_r = c->hS->dot_r;
        res->dot_zero = c->hS->dot_zero;
        res->seconds = total;
        res->iter_seconds = c->t_iter;
        res->spmv_ms_total = spmv_ms;
        res->spmv_launches = spmv_n;
        res->breakdown_iteration = c->hS->breakdown_k;
        res->adaptive_replacements = c->adaptive_rr;
    }
    if (c->hS->breakdown_k && c->rank == 0 && !o.quiet)
        fprintf(stderr, "bicgstab_hip: recurrence broke down (non-finite scalar) at iteration %d\n", c->hS->breakdown_k);
    if (talk) {   // reference src/solver.c:134-141, verbatim
        printf("Total iter   : %d\n", k);
        printf("Final r      : %e\n", sqrt(c->hS->dot_r / c->hS->dot_zero));
        printf("Total time   : %e [sec.] \n", total);
        printf("Avg time/iter: %e [sec.] \n", total / k);
        fflush(stdout);
    }
    return k;
}

// Which pipelined form? By default a constant decides (fuse_small / x windows, set in bicg_create): the same program then
// takes the same form on every run, which keeps results bit-reproducible from run to run -- the two forms associate the dot
// sums differently. BICG_PLAN="pipe-probe" measures instead: the first pipelined solve on a context runs 2 + 6 iterations of each
// form on the system A x = A 1, x0 = 0 (the caller's x0 / b are restored afterwards), all ranks agree on the slower rank's times, the
// faster form stays. The extra solves advance the exchange sequence numbers: a probed solve is not bit-identical to an unprobed one
// whenever the chosen form differs from the rule's (probing trades away that reproducibility; it is opt-in).
void probe_pipe_form(bicg_ctx *c, int method, const bicg_options *opt_in)
{
    bicg_options o;
    if (opt_in) o = *opt_in; else bicg_default_options(&o);
    const bool persist = c->persist_on && method == BICG_PIPE_BICGSTAB && o.rr_drift <= 0.0 && !(o.time_kernels & 3);
    if (!c->fuse_plan_ok || hosted(c)) { c->pipe_probed = true; return; }      // this context has one form only
    if (persist || o.max_iter < 16) return;      // this solve takes the persistent form / is too short to pay for it: a later one may probe
    c->pipe_probed = true;
    use_device(c);
    const size_t n = c->n_loc;
    // (the copies below run on the null stream, which the compute stream does not order itself against: after bicg_load_device x and
    // r may still be on their way in. After bicg_load the stream is idle and this returns at once)
    BICG_HIP(hipStreamSynchronize(c->sc));
    double *keep = dev_alloc<double>(2 * n);
    BICG_HIP(hipMemcpy(keep, c->v.x, sizeof(double) * n, hipMemcpyDeviceToDevice));
    BICG_HIP(hipMemcpy(keep + n, c->v.r, sizeof(double) * n, hipMemcpyDeviceToDevice));
    o.quiet = 1; o.tol = 0.0; o.max_iter = 8; o.check_every = 8; o.out_iter = 0; o.time_kernels = 0; o.record_trace = 0;
    // The probe does not iterate on the caller's data (an x0 that already solves the system would make the recurrences divide by
    // ~0 inside the probe): it solves A x = A 1 from x0 = 0, the reference's own test system (src/main.c:109-117). A breakdown all
    // the same counts as a tie: the rule's form stays.
    const bool rule_form = c->fuse_pipe;
    double *bsyn = dev_alloc<double>(n ? n : 1);
    {
        std::vector<double> ones(n ? n : 1, 1.0);
        scal_reset(c);
        BICG_HIP(hipMemcpyAsync(c->v.p, ones.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->sc));
        c->time_kernels = false;
        spmv(c, c->v.p, c->v.s, 0, nullptr, c->dots.no_dots());
        BICG_HIP(hipMemcpyAsync(bsyn, c->v.s, sizeof(double) * n, hipMemcpyDeviceToDevice, c->sc));
        BICG_HIP(hipStreamSynchronize(c->sc));
    }
    double t[2] = {0.0, 0.0};
    bool broke = false;
    for (int form = 1; form >= 0; --form) {
        c->fuse_pipe = form != 0;
        BICG_HIP(hipMemset(c->v.x, 0, sizeof(double) * n));
        BICG_HIP(hipMemcpy(c->v.r, bsyn, sizeof(double) * n, hipMemcpyDeviceToDevice));
        run_begin(c, method, &o);
        run_iterate(c, 2);
        const double t0 = now_sec();
        run_iterate(c, 6);
        t[form] = (now_sec() - t0) / 6.0 * 1.0e3;
        broke = broke || c->hS->breakdown_k != 0 || c->hS->comm_error != 0;
    }
    dev_free(bsyn);
    if (c->nranks > 1) {      // the slower rank's time counts, and every rank must take the same decision
        const int P = c->nranks;
        std::vector<int> cnt(P, 2 * (int)sizeof(double)), off(P);
        std::vector<double> mine(2 * (size_t)P), all(2 * (size_t)P, 0.0);
        for (int p = 0; p < P; ++p) { off[p] = 2 * p * (int)sizeof(double); mine[2 * p] = t[0]; mine[2 * p + 1] = t[1]; }
        c->comm->alltoallv_host(mine.data(), cnt.data(), off.data(), all.data(), cnt.data(), off.data());
        all[2 * c->rank] = t[0]; all[2 * c->rank + 1] = t[1];
        for (int p = 0; p < P; ++p) { t[0] = std::max(t[0], all[2 * p]); t[1] = std::max(t[1], all[2 * p + 1]); }
    }
    c->probe_ms[0] = t[0]; c->probe_ms[1] = t[1];
    if (c->nranks > 1) broke = !all_ranks(c->comm, !broke);
    c->fuse_pipe = broke ? rule_form : t[1] <= t[0];
    BICG_HIP(hipMemcpy(c->v.x, keep, sizeof(double) * n, hipMemcpyDeviceToDevice));
    BICG_HIP(hipMemcpy(c->v.r, keep + n, sizeof(double) * n, hipMemcpyDeviceToDevice));
    dev_free(keep);
    if (c->rank == 0 && knob_x("BICG_PIPE_PROBE_VERBOSE"))
        fprintf(stderr, "bicgstab_hip: pipelined form probe: separate kernels %.4f ms, SpMV epilogues %.4f ms per iteration -> %s\n", t[0], t[1],
                c->fuse_pipe ? "epilogues" : "separate kernels");
}

int run_solver(bicg_ctx *c, int method, const bicg_options *opt_in, bicg_result *res)
{
    if (c->pipe_probe && !c->pipe_probed && (method == BICG_PIPE_BICGSTAB || method == BICG_PIPE_BICGSTAB_RR)) probe_pipe_form(c, method, opt_in);
    run_begin(c, method, opt_in);
    run_iterate(c, c->opt.max_iter);
    return run_end(c, res);
}

