// bicg_dot_plan.cpp -- who closes a dot group (dot_group_plan, bicg_plan.h). Host only: nothing here calls
// the HIP runtime or reads the environment. C view for tests: bicg_dot_group_plan.
//
// Three regimes. TICKET: the producers' workgroups add the group up themselves (arrival tickets or the tail finish) and, on one
// rank, apply the recurrence; across ranks the sums still have to meet. WAVE: the producers leave one partial per wavefront, a
// later launch adds them up -- the kernel that consumes the scalars, helped by the product in between when the group is deferred.
// HAND: the producer's tail finish stops at the shard totals, the consuming kernel does the rest. Times four transports.
#include <algorithm>

#include "bicg_plan.h"

namespace bicg {

bool dot_tail_available(const DotShape &s)
{
    // (not under hipGraph replay: a captured launch would meet its own earlier words under the same tag)
    return s.tail_finish && s.transport != SPMV_P2P && !s.graph_replay;
}

bool dot_handover(const DotShape &s) { return s.handover && s.transport == SPMV_SINGLE && dot_tail_available(s); }

const char *dot_plan_error(int error)
{
    switch (error) {
    case DOT_ERR_OPEN: return "a dot group was produced while the previous one was still open";
    case DOT_ERR_STAGE_DOTS: return "an SpMV with dots was asked to stage a deferred group";
    case DOT_ERR_HAND_NONE: return "hand-over: a consumer without an open dot group";
    default: return "";
    }
}

DotPlan dot_group_plan(const DotShape &s, const DotCall &k)
{
    DotPlan p;
    const bool single = s.transport == SPMV_SINGLE, p2p = s.transport == SPMV_P2P, hosted = s.transport == SPMV_HOSTED;
    auto add = [&p](int op, int when, int stream, int roles, int n, int off, int phase) {
        DotStep &t = p.step[p.nsteps++];
        t.op = op; t.when = when; t.stream = stream; t.roles = roles; t.n = n; t.off = off; t.phase = phase;
    };
    // what a product has done for the open group already
    const int staged = k.open == DOT_OPEN_STAGED ? (FIN_SHARDS | FIN_PUSH) : 0;

    if (k.event == DOT_CONSUME) {
        if (k.regime == DOT_HAND) {
            if (k.open == DOT_OPEN_NONE) { p.error = DOT_ERR_HAND_NONE; return p; }
            add(DOT_OP_CONSUMER, DOT_IN_CONSUMER, DOT_COMPUTE, FIN_HAND, k.n, 0, k.phase);
        } else if (k.regime == DOT_WAVE && k.open != DOT_OPEN_NONE) {
            add(DOT_OP_CONSUMER, DOT_IN_CONSUMER, DOT_COMPUTE, (FIN_APPLY | FIN_SHARDS | FIN_PUSH) & ~staged, k.n, k.off, k.phase);
        }
        return p;
    }
    if (k.event == DOT_FORCE) {
        // (ticket groups have nothing to force: their scalars are applied, or the group is pending and stays so)
        if (k.regime == DOT_WAVE && k.open != DOT_OPEN_NONE) {
            // a hosted product deposits this rank's sums only and leaves the recurrence alone (section 4.3, "oddities")
            const bool local = hosted && k.by_product;
            add(DOT_OP_FINISH, DOT_AT_CLOSE, DOT_COMPUTE, ((FIN_BLOCK0 | FIN_SHARDS | FIN_PUSH) & ~staged) | (local ? FIN_LOCAL : 0), k.n, k.off,
                local ? (int)PH_NONE : k.phase);
        }
        return p;
    }

    // hosted: all-reduce and k_apply. Nothing can overlap a group that closes now, so both go to the compute stream itself (a round
    // trip through the communication stream costs two cross-stream hand-offs); a deferred one starts behind the next product's halo
    // traffic on the communication stream and is joined after that product (reference src/solver.c:363-367, 377-385)
    auto hosted_steps = [&](int off) {
        if (p.deferred) {
            add(DOT_OP_RECORD, DOT_AT_CLOSE, DOT_COMPUTE, 0, k.n, off, k.phase);
            add(DOT_OP_WAIT, DOT_BEHIND_HALO, DOT_COMM, 0, k.n, off, k.phase);
            add(DOT_OP_ALLREDUCE, DOT_BEHIND_HALO, DOT_COMM, 0, k.n, off, k.phase);
            add(DOT_OP_APPLY, DOT_BEHIND_HALO, DOT_COMM, 0, k.n, off, k.phase);
            add(DOT_OP_RECORD, DOT_BEHIND_HALO, DOT_COMM, 0, k.n, off, k.phase);
            add(DOT_OP_WAIT, DOT_AFTER_PRODUCT, DOT_COMPUTE, 0, k.n, off, k.phase);
        } else {
            add(DOT_OP_ALLREDUCE, DOT_AT_CLOSE, DOT_COMPUTE, 0, k.n, off, k.phase);
            add(DOT_OP_APPLY, DOT_AT_CLOSE, DOT_COMPUTE, 0, k.n, off, k.phase);
        }
    };
    const bool two_streams = hosted && s.overlap && s.stream_ordered;

    if (k.regime == DOT_WAVE) {
        if (k.event == DOT_CONTRIBUTE) return p;      // a product without dots: an empty Reduce
        if (k.open != DOT_OPEN_NONE && !k.by_product) { p.error = DOT_ERR_OPEN; return p; }
        // (a product closes a group that is not deferred, or was staged by an earlier product, before it opens its own; one that
        // would have to stage it cannot open its own with the same launch)
        if (k.open == DOT_OPEN_DEFERRED) { p.error = DOT_ERR_STAGE_DOTS; return p; }
        p.wave = true;
        p.deferred = k.event == DOT_DEFER && (!hosted || two_streams);
        if (!hosted) {      // the group stays open for the kernel that consumes it
            if (p.deferred) add(DOT_OP_STAGE, DOT_BEHIND_HALO, DOT_COMPUTE, FIN_SHARDS | FIN_PUSH, k.n, k.off, k.phase);
            add(DOT_OP_CONSUMER, DOT_IN_CONSUMER, DOT_COMPUTE, FIN_APPLY | (p.deferred ? 0 : FIN_SHARDS | FIN_PUSH), k.n, k.off, k.phase);
        } else {            // this rank's sums -> Scal::red, then as a ticket group
            add(DOT_OP_FINISH, DOT_AT_CLOSE, DOT_COMPUTE, FIN_BLOCK0 | FIN_SHARDS | FIN_PUSH | FIN_LOCAL, k.n, k.off, PH_NONE);
            hosted_steps(k.off);
        }
        return p;
    }

    p.tail = dot_tail_available(s);
    p.mailbox = p2p;
    p.apply_now = single && k.apply_single;
    if (k.regime == DOT_HAND) {
        p.hand = true; p.apply_now = false;
        add(DOT_OP_CONSUMER, DOT_IN_CONSUMER, DOT_COMPUTE, FIN_HAND, k.n, 0, k.phase);
        return p;
    }
    if (k.event == DOT_CONTRIBUTE) return p;
    p.deferred = k.event == DOT_DEFER && (p2p || two_streams);
    if (single && p.apply_now) add(DOT_OP_NOTHING, DOT_AT_CLOSE, DOT_COMPUTE, 0, k.n, 0, k.phase);
    if (p2p) {      // the producers store their sums into every rank's mailbox
        if (!p.deferred && k.apply_single && k.n > 0 && s.inline_apply) {      // ... and the last of them collects and applies
            p.apply_now = true; p.n_collect = k.n;
            add(DOT_OP_NOTHING, DOT_AT_CLOSE, DOT_COMPUTE, 0, k.n, 0, k.phase);
        } else {    // deferred: collected after the next product, the sums cross the links while it runs
            add(DOT_OP_APPLY_P2P, p.deferred ? DOT_AFTER_PRODUCT : DOT_AT_CLOSE, DOT_COMPUTE, 0, k.n, 0, k.phase);
        }
    }
    if (hosted) hosted_steps(0);      // (the sums of a ticket group are all-reduced from Scal::red[0] whatever its offset)
    return p;
}

}  // namespace bicg

// C view for tests of the plan (include/bicgstab_hip.h section 5 documents the orders)
extern "C" int bicg_dot_group_plan(const int shape[7], const int call[8], int plan[9], int steps[49])
{
    using namespace bicg;
    static_assert(kDotShapeLen == 7 && kDotCallLen == 8 && kDotPlanLen == 9 && kDotStepLen * kDotMaxSteps == 49, "lengths documented in bicgstab_hip.h");
    if (!shape || !call || !plan || !steps || shape[0] < 0 || shape[0] > SPMV_HOSTED || call[0] < 0 || call[0] > DOT_HAND || call[5] < 0 ||
        call[5] > DOT_CONTRIBUTE || call[6] < 0 || call[6] > DOT_OPEN_STAGED)
        return 1;
    DotShape s;
    s.transport = shape[0]; s.stream_ordered = shape[1] != 0; s.overlap = shape[2] != 0; s.inline_apply = shape[3] != 0;
    s.tail_finish = shape[4] != 0; s.graph_replay = shape[5] != 0; s.handover = shape[6] != 0;
    DotCall k;
    k.regime = call[0]; k.n = call[1]; k.off = call[2]; k.phase = call[3]; k.apply_single = call[4] != 0; k.event = call[5]; k.open = call[6];
    k.by_product = call[7] != 0;
    const DotPlan p = dot_group_plan(s, k);
    const int head[kDotPlanLen] = {p.error, p.wave, p.hand, p.apply_now, p.n_collect, p.tail, p.mailbox, p.deferred, p.nsteps};
    std::copy(head, head + kDotPlanLen, plan);
    std::fill(steps, steps + kDotStepLen * kDotMaxSteps, 0);
    for (int i = 0; i < p.nsteps; ++i) {
        const DotStep &t = p.step[i];
        const int row[kDotStepLen] = {t.op, t.when, t.stream, t.roles, t.n, t.off, t.phase};
        std::copy(row, row + kDotStepLen, steps + i * kDotStepLen);
    }
    return 0;
}
