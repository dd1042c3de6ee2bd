// bicg_dots.cpp -- the dot groups of a context (struct DotGroups, bicg_host.h): their memory, the open / close
// interface of the solvers, and the one executor of dot_group_plan (bicg_dot_plan.cpp). Nothing here decides who closes a group:
// open() asks the plan once and remembers it, the other methods enqueue its steps where they belong and advance the sequence
// numbers (grp_seq, tail_seq, P2p::red_seq, halo_unsynced), which must move identically on every rank.
#include "bicg_host.h"

template <class T> static T *zeroed(DevOwner &own, size_t n)
{
    T *p = own.alloc<T>(n);
    BICG_HIP(hipMemset(p, 0, sizeof(T) * n));
    return p;
}

void DotGroups::init(bicg_ctx *ctx, unsigned slots)
{
    c = ctx; nslots = slots;
    DevOwner &own = c->own;
    partial = own.alloc<double>((size_t)nslots * kPartialStride);      // (written before they are read: not zeroed)
    shard_tot = own.alloc<double>((size_t)kShards * kPartialStride);
    counter = zeroed<unsigned>(own, (kShards + 1) * kCounterStride);
    tail_tab = zeroed<llword>(own, (size_t)nslots * kTailStride);
    tail_shard = zeroed<llword>(own, (size_t)kShards * kRedSlots * 2);
    if (const char *sv = getenv("BICG_TAIL_FINISH")) tail_finish = atoi(sv) != 0;      // 0: every ticket-mode group closes by arrival tickets
    hand_shard = zeroed<llword>(own, (size_t)2 * kRedSlots * kShards * 2);
    c->Sbuf = zeroed<Scal>(own, 2);
    c->S = c->Sbuf; cur = 0;
    for (double *&w : wpart) w = zeroed<double>(own, (size_t)nslots * (kBlock / 64) * kPartialStride);
    shard_ll = zeroed<llword>(own, (size_t)2 * kShardLL * kRedSlots * 2);
    for (int i = 0; i < kEvRing; ++i) {
        BICG_HIP(hipEventCreateWithFlags(&ev_dots[i], hipEventDisableTiming));
        BICG_HIP(hipEventCreateWithFlags(&ev_red[i], hipEventDisableTiming));
    }
}

void DotGroups::reset(bool wave, const Scal *block, bool both)
{
    wave_mode = wave;
    grp = Group{};
    shp = shape();      // the transport does not change under a solve: asked once, not per group
    for (int i = 0; i < (both ? 2 : 1); ++i) {      // (both: the idle block must not carry `done` of an earlier solve)
        Scal *dst = both ? c->Sbuf + i : c->S;
        if (block) BICG_HIP(hipMemcpyAsync(dst, block, sizeof(Scal), hipMemcpyHostToDevice, c->sc));
        else BICG_HIP(hipMemsetAsync(dst, 0, sizeof(Scal), c->sc));
    }
    BICG_HIP(hipMemsetAsync(counter, 0, sizeof(unsigned) * (kShards + 1) * kCounterStride, c->sc));
}

DotShape DotGroups::shape() const
{
    DotShape s;
    s.transport = c->single() ? SPMV_SINGLE : c->p2p ? SPMV_P2P : SPMV_HOSTED;
    s.stream_ordered = s.transport == SPMV_HOSTED && c->comm->stream_ordered();
    s.overlap = c->overlap; s.inline_apply = inline_apply;
    s.tail_finish = tail_finish && tail_tab; s.graph_replay = c->graph_mode == 1;
    s.handover = handover && hand_shard;
    return s;
}

void DotGroups::next_block()
{
    cur ^= 1;
    c->S = c->Sbuf + cur;
}

static int open_state(const DotGroups::Group &g)
{
    return !g.active ? DOT_OPEN_NONE : g.staged ? DOT_OPEN_STAGED : g.plan.deferred ? DOT_OPEN_DEFERRED : DOT_OPEN_PLAIN;
}
static const DotPlan &checked(const DotPlan &p)
{
    if (p.error) die("internal", dot_plan_error(p.error));
    return p;
}
// what open / consume / force ask the plan with: the shape of the last reset, and whether iterations are replayed NOW (a capture
// that fails switches graph_mode off in mid-solve)
const DotShape &DotGroups::solve_shape()
{
    shp.graph_replay = c->graph_mode == 1;
    return shp;
}

// the Reduce of a ticket-mode producer
Reduce DotGroups::ticket(const DotPlan &p, int off, int phase)
{
    Reduce r{};
    r.partial = partial; r.shard_tot = shard_tot; r.counter = counter; r.expected = 0; r.slot_base = 0;
    r.red_off = off; r.phase = phase;
    r.apply_now = p.apply_now ? 1 : 0;
    r.hand = p.hand ? 1 : 0;
    r.p2p = P2pRed{};
    r.tail_tab = tail_tab; r.tail_shard = tail_shard;
    r.tail_seq = p.tail ? ++tail_seq : 0u;
    if (p.mailbox) {      // the group being produced: its number is taken when it is closed
        r.p2p = c->p2p->red_desc(c->p2p->red_seq);
        r.p2p.n_collect = p.n_collect;
    }
    return r;
}

Reduce DotGroups::open(int n, int phase, int event, int off, unsigned nwg, bool by_product)
{
    DotCall k;
    k.regime = wave_mode ? DOT_WAVE : DOT_TICKET; k.n = n; k.off = off; k.phase = phase; k.event = event; k.by_product = by_product;
    if (wave_mode) {
        if (by_product && grp.active && grp.staged) force(true);      // staged by an earlier product: closed before this one opens its own
        k.open = open_state(grp);
    }
    Group &g = grp;
    g.plan = dot_group_plan(solve_shape(), k);      // (written in place: one plan per group, no copy)
    const DotPlan &p = checked(g.plan);
    g.active = true; g.staged = false; g.call = k;
    g.seq = g.mail_seq = g.nparts = 0; g.buf = 0;
    if (!p.wave) return ticket(p, off, phase);
    g.seq = ++grp_seq;
    g.buf = (int)(g.seq & 1u);
    g.nparts = nwg * (kBlock / 64);               // products: producer_grid
    if (c->p2p) g.mail_seq = c->p2p->red_seq++;
    Reduce r{};
    r.partial = wpart[g.buf];
    r.wave = 1; r.red_off = off; r.phase = phase;
    return r;
}

// the producer's last workgroups leave the shard totals in the table the previous group does not use
Reduce DotGroups::open_hand(int n, int phase, unsigned nwg)
{
    DotCall k;
    k.regime = DOT_HAND; k.n = n; k.phase = phase;
    Reduce r = ticket(checked(dot_group_plan(solve_shape(), k)), 0, phase);
    hand.buf ^= 1; hand.seq = r.tail_seq; hand.n = n; hand.phase = phase;
    if (nwg) hand.nsh = std::min<unsigned>(nwg, (unsigned)kShards);
    r.tail_shard = hand_shard + (size_t)hand.buf * kRedSlots * kShards * 2;
    return r;
}

Reduce DotGroups::contribute(int off, bool apply_single)
{
    DotCall k;
    k.off = off; k.phase = PH_NONE; k.apply_single = apply_single; k.event = DOT_CONTRIBUTE;
    return ticket(dot_group_plan(solve_shape(), k), off, PH_NONE);
}

void DotGroups::producer_grid(const Reduce &red, unsigned expected, unsigned hand_nsh, bool sets_nparts)
{
    if (red.hand) hand.nsh = hand_nsh;
    if (sets_nparts) grp.nparts = expected * (kBlock / 64);
}

Finish DotGroups::desc(int roles) const
{
    const Group &g = grp;
    Finish f{};
    f.partial = wpart[g.buf]; f.nparts = g.nparts; f.seq = g.seq;
    f.shard = shard_ll + (size_t)g.buf * kShardLL * kRedSlots * 2;
    f.shard_clear = shard_ll + (size_t)(g.buf ^ 1) * kShardLL * kRedSlots * 2;
    f.n = g.call.n; f.red_off = g.call.off; f.phase = g.call.phase; f.roles = roles;
    f.spin_ticks = spin_ticks;
    if (c->p2p) { f.p2p = c->p2p->red_desc(g.mail_seq); f.alarm = c->alarm; }
    return f;
}

// the steps of a plan that belong to one point, in order, on the scalar block that is current now
void DotGroups::run(const DotPlan &plan, int when, unsigned mail_seq)
{
    for (int i = 0; i < plan.nsteps; ++i) {
        const DotStep &t = plan.step[i];
        if (t.when != when) continue;
        const hipStream_t st = t.stream == DOT_COMM ? c->sm : c->sc;
        switch (t.op) {
        case DOT_OP_NOTHING: if (c->p2p) c->halo_unsynced = 0; break;
        case DOT_OP_FINISH: {      // in place on the current scalar block
            Finish f = desc(t.roles);
            f.phase = t.phase;
            launch_finish(Launch{c->S, f, c->sc});
            break;
        }
        case DOT_OP_ALLREDUCE: ctx_allreduce(c, c->S->red + t.off, t.n, st); break;
        case DOT_OP_APPLY: launch_apply(c->S, t.phase, st); break;
        case DOT_OP_APPLY_P2P:     // (an all-reduce is a barrier among the ranks)
            launch_apply_p2p(c->S, t.phase, t.n, c->p2p->red_desc(mail_seq), c->p2p->timeout_ticks, c->sc);
            c->halo_unsynced = 0;
            break;
        case DOT_OP_RECORD:
            pend.ev = t.stream == DOT_COMM ? ev_red[i_red++ % kEvRing] : ev_dots[i_dots++ % kEvRing];
            BICG_HIP(hipEventRecord(pend.ev, st));
            break;
        case DOT_OP_WAIT: BICG_HIP(hipStreamWaitEvent(st, pend.ev, 0)); break;
        default: break;            // DOT_OP_STAGE: before_product; DOT_OP_CONSUMER: consume
        }
    }
}

void DotGroups::close()
{
    Group &g = grp;
    if (!g.active) return;
    const DotPlan &p = g.plan;
    if (p.wave && !hosted(c)) return;      // stays open for the kernel that consumes it
    const unsigned seq = p.mailbox ? c->p2p->red_seq++ : 0u;      // a ticket group takes its mailbox number when it is closed
    if (!c->single() && !p.deferred) {
        Section sec(c, SEC_REDUCE);
        run(p, DOT_AT_CLOSE, seq);
    } else {
        run(p, DOT_AT_CLOSE, seq);
    }
    g.active = false;
    if (p.deferred) { pend.on = true; pend.plan = p; pend.seq = seq; }
}

void DotGroups::force(bool by_product)
{
    if (!grp.active || !grp.plan.wave) return;
    DotCall k = grp.call;
    k.event = DOT_FORCE; k.open = open_state(grp); k.by_product = by_product;
    run(dot_group_plan(solve_shape(), k), DOT_AT_CLOSE);
    grp.active = false;
    if (c->p2p) c->halo_unsynced = 0;
}

// everything enqueued afterwards reads the scalar block the consuming kernel writes
Launch DotGroups::consume()
{
    Launch L{c->S, Finish{}, c->sc};
    if (!grp.active || !grp.plan.wave) return L;
    DotCall k = grp.call;
    k.event = DOT_CONSUME; k.open = open_state(grp);
    L.fin = desc(dot_group_plan(solve_shape(), k).step[0].roles);
    next_block();
    L.fin.Snext = c->S;
    grp.active = false;
    if (c->p2p) c->halo_unsynced = 0;      // an all-reduce is a barrier among the ranks
    return L;
}

// it reads the current scalar block and the open group's totals and writes the other block
Launch DotGroups::consume_hand()
{
    DotCall k;
    k.regime = DOT_HAND; k.event = DOT_CONSUME; k.n = hand.n; k.phase = hand.phase; k.open = hand.seq ? DOT_OPEN_PLAIN : DOT_OPEN_NONE;
    const DotPlan p = checked(dot_group_plan(solve_shape(), k));
    Launch L{c->S, Finish{}, c->sc};
    L.fin.seq = hand.seq; L.fin.nparts = hand.nsh; L.fin.n = hand.n; L.fin.red_off = 0; L.fin.phase = hand.phase; L.fin.roles = p.step[0].roles;
    L.fin.shard = hand_shard + (size_t)hand.buf * kRedSlots * kShards * 2;
    next_block();
    L.fin.Snext = c->S;
    hand.seq = 0;
    return L;
}

// The open wave group as seen by the next product: a deferred group is staged by the product's first launch (shards summed, sums
// on their way to the peers) and stays open; anything else is closed first. has_dots: the product opens a group of its own, with
// the same launch -- it cannot stage one too (open() reports that).
Finish DotGroups::before_product(bool has_dots)
{
    Group &g = grp;
    if (!g.active || !g.plan.wave) return Finish{};
    if (hosted(c) || !g.plan.deferred) { force(true); return Finish{}; }
    if (g.staged || has_dots) return Finish{};
    g.staged = true;
    for (int i = 0; i < g.plan.nsteps; ++i)
        if (g.plan.step[i].op == DOT_OP_STAGE) return desc(g.plan.step[i].roles);
    return Finish{};
}

void DotGroups::behind_halo()
{
    if (!pend.on || !hosted(c)) return;
    pend.on = false;
    run(pend.plan, DOT_BEHIND_HALO);
    pend.joined = true;
}

void DotGroups::after_product()
{
    if (c->p2p && pend.on) {
        pend.on = false;
        run(pend.plan, DOT_AFTER_PRODUCT, pend.seq);
    }
    if (pend.joined) {
        pend.joined = false;
        run(pend.plan, DOT_AFTER_PRODUCT);
        pend.ev = nullptr;
    }
}

void DotGroups::flush()
{
    if (wave_mode && !hosted(c)) return;      // consumed by the next element-wise kernel or by fetch_scal
    if (!pend.on) return;
    Section sec(c, SEC_REDUCE);
    pend.on = false;
    run(pend.plan, DOT_BEHIND_HALO);
    run(pend.plan, DOT_AFTER_PRODUCT, pend.seq);
    pend.ev = nullptr;
}
