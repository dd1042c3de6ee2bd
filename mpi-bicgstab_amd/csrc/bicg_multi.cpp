// bicg_multi.cpp -- bicg_solve_multi / bicg_multi_trace: plain BiCGStab (reference src/solver.c:74-120) on nrhs independent
// systems that share the resident matrix, kSpmmCols columns per set, every product of a set ONE pass over the matrix (spmm_pass
// reading P and R in place). Kernels: bicg_multi.hip. See bicg_host.h and DESIGN.md section 4.17.
//
// A set: X, R, R#, P, S, Y with kSpmmCols columns each, the columns c->stride apart (a multiple of 32 doubles: every column is
// 256-byte aligned), one MultiScal block, the dot partials. Per iteration (each element-wise phase a launch over all columns of
// the set, each finish one tiny launch with a workgroup per column):
//   S = A P | (r#,s) | alpha | r -= alpha s | Y = A Q | (q,y), (y,y) | omega | x, r updates with (r,r), (r#,r) | beta, k, flag | p
// The loop condition of a column is evaluated by the last finish ON THE DEVICE at every iteration; the workgroups of a column
// whose condition is false return at once, so its x and r stay as they are. The host reads the flags every check_every iterations.
//
// Right-preconditioned (methods 4 and 5 on a context that holds the matching preconditioner): every column
// runs Driver::iter_plain's preconditioned form (bicg_solver.cpp). Two more sets, P^ = M^-1 P and Q^ = M^-1 Q (mt_hat, an allocation
// of its own made by the first such call), are what the two products read; x += alpha p^ + omega q^; r stays the residual of the
// caller's system, so the dots, the scalars and the loop condition are the plain call's. DIAGONAL: the passes that produce p and q
// write the hat vectors too -- the plain call's launch sequence. BLOCK: one k_bjac_apply_set launch for the whole set behind each of
// them (and one behind the set-up phase): two launches more per iteration and set. The planes are read as installed at the call.
//
// Across ranks (nranks > 1) the call is collective. Every product of a set is one spmm_pass -- ONE halo exchange for the set
// (halo_set) -- or, without the SpMM, one collective spmv() per column the agreed flags show as live. Every finish is k_multi_sum,
// ONE all-reduce of mt_red[nranks][2][kSpmmCols] that gathers the ranks' local sums (each rank's row is added to zeros only), and
// k_multi_apply, which adds the rows in a fixed order: the scalars, hence the flags the host reads, are the same bytes on every rank,
// so the ranks cannot disagree about the next collective. On a peer-to-peer context the products use its data path (halo_only /
// spmv) while these all-reduces go through the transport underneath (c->comm->allreduce_sum): correct, not optimised.
//
// bicg_solve_multi_device is the same call on the caller's device arrays: solve_multi_any below serves
// both, they differ in how a set's columns cross (vec_upload / vec_download against cross_in / cross_out, bicg_host.h).
#include "bicg_host.h"

namespace {

void multi_buffers(bicg_ctx *c)
{
    if (c->mt_slab) return;
    const size_t st = c->stride;
    // (+64: k_spmm_pipe copies 16-byte pairs, the last one may reach one column past a vector -- as for mm_in, spmm_buffers)
    const size_t slab = 6 * (size_t)kSpmmCols * st + 64;
    c->mt_slab = c->own.alloc<double>(slab);
    c->mt_part = c->own.alloc<double>(2 * (size_t)kSpmmCols * multi_grid(c->n_loc));
    c->mt_S = c->own.alloc<MultiScal>(1);
    BICG_HIP(hipMemset(c->mt_slab, 0, sizeof(double) * slab));      // padding rows and unused columns stay finite
    BICG_HIP(hipDeviceSynchronize());      // the memset ran on the null stream: c->sc does not wait for it
}

// P^ and Q^ of the right-preconditioned methods: ONE more allocation, made by the first such call on the context and zeroed once
// (halo tails, padding rows and unused columns stay finite), with mt_slab's 64 doubles of slack: the products read these two sets
void multi_hat_buffers(bicg_ctx *c)
{
    if (c->mt_hat) return;
    const size_t slab = 2 * (size_t)kSpmmCols * c->stride + 64;
    c->mt_hat = c->own.alloc<double>(slab);
    BICG_HIP(hipMemset(c->mt_hat, 0, sizeof(double) * slab));
    BICG_HIP(hipDeviceSynchronize());      // (the null stream again)
}

// hat: the preconditioner the call's method runs with -- the planes as they are installed NOW
MultiVecs multi_vecs(const bicg_ctx *c, Precond::Kind hat)
{
    const size_t set = (size_t)kSpmmCols * c->stride;
    double *b = c->mt_slab;
    MultiVecs v{b, b + set, b + 2 * set, b + 3 * set, b + 4 * set, b + 5 * set, c->stride, c->n_loc, nullptr, nullptr, nullptr};
    if (hat != Precond::NONE) { v.ph = c->mt_hat; v.qh = c->mt_hat + set; }
    if (hat == Precond::DIAGONAL) v.dinv = c->pc.planes;
    return v;
}

// out = A in for the nv columns of a set (`live`: the columns the host still knows to be active; a frozen column's product is
// harmless and only the per-column form can skip it)
void multi_product(bicg_ctx *c, bool spmm, double *in, double *out, int nv, const int *live)
{
    const size_t st = c->stride;
    if (spmm) {
        spmm_pass(c, nv, nullptr, false, true, nullptr, nullptr, in, out);
        if (!c->mm_win) launch_vectors_from_rows(c->mm_yt, st, nv, c->n_loc, out, c->sc);      // the row-major form's second transpose
        return;
    }
    for (int j = 0; j < nv; ++j)
        if (live[j]) spmv(c, in + (size_t)j * st, out + (size_t)j * st, 0, nullptr, c->dots.no_dots());
}

void fetch_multi(bicg_ctx *c, MultiScal *h)
{
    BICG_HIP(hipMemcpyAsync(h, c->mt_S, sizeof(MultiScal), hipMemcpyDeviceToHost, c->sc));
    if (c->p2p) fetch_scal(c);      // synchronises, and reports a peer that never delivered its halo values
    else BICG_HIP(hipStreamSynchronize(c->sc));
}

constexpr int kRedRow = 2 * kSpmmCols;      // doubles per rank in mt_red

void multi_red_buffer(bicg_ctx *c)
{
    if (!c->mt_red) c->mt_red = c->own.alloc<double>((size_t)c->nranks * kRedRow);
}

// the dot group `phase` of a set: one rank -> k_multi_finish; several -> local sums, one gathering all-reduce, apply
void multi_finish(bicg_ctx *c, int phase, int nv, unsigned nwg)
{
    if (c->nranks == 1) { launch_multi_finish(phase, nv, c->mt_S, c->mt_part, nwg, c->sc); return; }
    launch_multi_sum(phase, nv, c->mt_S, c->mt_part, nwg, c->mt_red, c->nranks, c->rank, c->sc);
    ctx_allreduce(c, c->mt_red, c->nranks * kRedRow, c->sc);
    launch_multi_apply(phase, nv, c->mt_S, c->mt_red, c->nranks, c->sc);
}

// Collective: did every rank pass the same arguments? Each rank writes what the sequence of collectives depends on into its row
// of the gather buffer (every value an integer a double holds exactly; tol as the two halves of its bit pattern), one all-reduce
// gathers the rows, every rank compares them all -- so every rank reaches the same verdict.
// local_bad: this rank's own arrays are refusable (device variant: a missing array, ld < local_rows) -- the others cannot see that, so it
// travels with the arguments and every rank refuses together
bool multi_agree(bicg_ctx *c, int method, int nrhs, const bicg_options &o, bool spmm, bool local_bad = false)
{
    const int P = c->nranks;
    unsigned long long tb = 0;
    static_assert(sizeof tb == sizeof o.tol, "tol is a double");
    memcpy(&tb, &o.tol, sizeof tb);
    const double mine[7] = {(double)nrhs, (double)method, (double)o.max_iter, (double)o.check_every, (double)(tb & 0xffffffffull),
                            (double)(tb >> 32), spmm ? 1.0 : 0.0};
    std::vector<double> all((size_t)P * kRedRow, 0.0);
    std::copy(mine, mine + 7, all.begin() + (size_t)c->rank * kRedRow);
    all[(size_t)c->rank * kRedRow + 7] = local_bad ? 1.0 : 0.0;
    BICG_HIP(hipMemcpyAsync(c->mt_red, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice, c->sc));
    BICG_HIP(hipStreamSynchronize(c->sc));      // (all is pageable: the copy has left it before the transport may touch the stream)
    ctx_allreduce(c, c->mt_red, P * kRedRow, c->sc);
    BICG_HIP(hipMemcpyAsync(all.data(), c->mt_red, sizeof(double) * all.size(), hipMemcpyDeviceToHost, c->sc));
    BICG_HIP(hipStreamSynchronize(c->sc));
    for (int p = 0; p < P; ++p)
        if (memcmp(all.data() + (size_t)p * kRedRow, mine, sizeof mine) != 0 || all[(size_t)p * kRedRow + 7] != 0.0) return false;
    return true;
}

// bicg_solve_multi (device = false: host arrays, ld = local_rows) and bicg_solve_multi_device (the caller's device arrays, columns
// ld apart, `user` its stream): the same call but for how a set's columns cross, vec_upload / vec_download or cross_in / cross_out
int solve_multi_any(bicg_ctx *c, int method, double *x_loc_set, double *r_loc_set, size_t ld, int nrhs, const bicg_options *opt_in,
                    bicg_result *res, bool device, hipStream_t user)
{
    if (!c) return -1;
    bicg_options o;
    if (opt_in) o = *opt_in; else bicg_default_options(&o);
    if (o.max_iter < 0) o.max_iter = 0;
    if (o.check_every < 1) o.check_every = 1;
    if (c->nranks > 1) {
        // collective from here on: a rank whose own arguments are refusable still takes part in the check, or the others would wait
        use_device(c);
        multi_red_buffer(c);
        // (... and a rank without the method's preconditioner: bs and the blocks are a rank's own, that one is installed is not)
        const bool bad = (device && !c->phantom && (!x_loc_set || !r_loc_set || ld < c->n_loc)) || diag_refused(c, method);
        if (!multi_agree(c, method, nrhs, o, c->spmm_ok && !plan_off("spmm"), bad) && !bad) return -1;
    }
    if (device && !c->phantom && (!x_loc_set || !r_loc_set)) return -1;
    // plain BiCGStab, as it stands or right-preconditioned with the preconditioner the context holds
    const Precond::Kind hat = precond_kind_of(method);
    if ((method != BICG_BICGSTAB && hat == Precond::NONE) || method_stab2(method) || diag_refused(c, method)) return -2;      // (no BiCGStab(2) sets)
    if (nrhs < 1 || (device && !c->phantom && ld < c->n_loc)) return -2;
    use_device(c);
    std::vector<double> ph_x, ph_r;        // a context without rows holds one phantom row: zeros in, nothing out (host_in)
    if (c->phantom && !device) { ph_x.assign((size_t)nrhs, 0.0); ph_r.assign((size_t)nrhs, 0.0); x_loc_set = ph_x.data(); r_loc_set = ph_r.data(); }

    scal_reset(c);                         // the per-column products read the context's scalar block like bicg_spmv
    c->time_kernels = false;
    const bool spmm = c->spmm_ok && !plan_off("spmm");
    if (spmm) spmm_buffers(c);
    multi_buffers(c);
    if (hat != Precond::NONE) multi_hat_buffers(c);
    const bool tracing = o.record_trace != 0 && o.max_iter > 0;
    if (tracing && c->mt_trace_cap < o.max_iter) {
        c->mt_trace_cap = o.max_iter;
        c->mt_trace = c->own.regrow(c->mt_trace, 4 * (size_t)kSpmmCols * c->mt_trace_cap);
    }
    c->mt_host_trace.clear(); c->mt_iters.clear();
    if (tracing) { c->mt_host_trace.resize((size_t)nrhs); c->mt_iters.assign((size_t)nrhs, 0); }

    const MultiVecs v = multi_vecs(c, hat);
    double *const in_p = hat ? v.ph : v.p, *const in_q = hat ? v.qh : v.r;      // what the two products of an iteration read
    const size_t n = c->n_loc;
    const unsigned nwg = multi_grid(c->n_loc);
    MultiScal h;
    int kmax = 0;
    double t_total = 0.0, t_iter = 0.0;
    for (int j0 = 0; j0 < nrhs; j0 += kSpmmCols) {
        const int nv = std::min(kSpmmCols, nrhs - j0);
        memset(&h, 0, sizeof h);
        h.tol2 = o.tol * o.tol;
        h.max_iter = o.max_iter;
        h.trace = tracing ? c->mt_trace : nullptr;
        h.trace_cap = tracing ? c->mt_trace_cap : 0;
        BICG_HIP(hipMemcpyAsync(c->mt_S, &h, sizeof h, hipMemcpyHostToDevice, c->sc));
        if (device) {
            cross_begin(c, user);
            cross_in(c, v.x, x_loc_set + (size_t)j0 * ld, v.r, r_loc_set + (size_t)j0 * ld, c->stride, ld, nv);
            cross_end(c, user);
        } else {
            vec_upload(c, v.x, c->stride, x_loc_set + (size_t)j0 * n, nv, true);
            vec_upload(c, v.r, c->stride, r_loc_set + (size_t)j0 * n, nv, true);
        }
        BICG_HIP(hipStreamSynchronize(c->sc));      // (h is reused below; the uploads are not part of the timed span)

        // ---- set-up phase (src/solver.c:74-83): s = A x ; r = b - s ; r# = r ; p = r ; (r,r)
        const double t0 = now_sec();
        int live[kSpmmCols];
        for (int j = 0; j < kSpmmCols; ++j) live[j] = j < nv;
        multi_product(c, spmm, v.x, v.s, nv, live);
        if (hat == Precond::DIAGONAL) launch_multi_init_diag(v, nv, c->mt_S, c->mt_part, c->sc);   // ... ; p^ = dinv o p
        else launch_multi_init(v, nv, c->mt_S, c->mt_part, c->sc);
        multi_finish(c, MP_INIT, nv, nwg);
        if (hat == Precond::BLOCK) precond_apply_set(c, v.p, v.ph, nv, c->mt_S);                   // p^ = M^-1 p, the columns the finish left active
        fetch_multi(c, &h);
        const double t1 = now_sec();

        // ---- iterations (src/solver.c:86-120)
        for (int it = 0; it < o.max_iter;) {
            bool any = false;
            for (int j = 0; j < nv; ++j) { live[j] = h.active[j]; any = any || live[j]; }
            if (!any) break;
            const int chunk = std::min(o.check_every, o.max_iter - it);
            for (int i = 0; i < chunk; ++i) {
                multi_product(c, spmm, in_p, v.s, nv, live);                             // s = A p (A p^)
                launch_multi_dot_rs(v, nv, c->mt_S, c->mt_part, c->sc);                  // (r#,s)
                multi_finish(c, MP_ALPHA, nv, nwg);
                if (hat == Precond::DIAGONAL) launch_multi_q_diag(v, nv, c->mt_S, c->sc); // q = r - alpha s (kept in r) ; q^ = dinv o q
                else launch_multi_q(v, nv, c->mt_S, c->sc);                              // q = r - alpha s (kept in r)
                if (hat == Precond::BLOCK) precond_apply_set(c, v.r, v.qh, nv, c->mt_S); // q^ = M^-1 q
                multi_product(c, spmm, in_q, v.y, nv, live);                             // y = A q (A q^)
                launch_multi_dot_qy(v, nv, c->mt_S, c->mt_part, c->sc);                  // (q,y), (y,y)
                multi_finish(c, MP_OMEGA, nv, nwg);
                if (hat) launch_multi_xr_hat(v, nv, c->mt_S, c->mt_part, c->sc);         // x += alpha p^ + omega q^, r ; (r,r), (r#,r)
                else launch_multi_xr(v, nv, c->mt_S, c->mt_part, c->sc);                 // x, r ; (r,r), (r#,r)
                multi_finish(c, MP_END, nv, nwg);
                if (hat == Precond::DIAGONAL) launch_multi_p_diag(v, nv, c->mt_S, c->sc); // p ; p^ = dinv o p
                else launch_multi_p(v, nv, c->mt_S, c->sc);                              // p
                if (hat == Precond::BLOCK) precond_apply_set(c, v.p, v.ph, nv, c->mt_S); // p^ = M^-1 p
            }
            it += chunk;
            fetch_multi(c, &h);
        }
        const double t2 = now_sec();
        t_total += t2 - t0; t_iter += t2 - t1;

        if (device) {
            cross_begin(c, user);
            cross_out(c, x_loc_set + (size_t)j0 * ld, v.x, r_loc_set + (size_t)j0 * ld, v.r, c->stride, ld, nv);
            cross_end(c, user);
        } else {
            vec_download(c, x_loc_set + (size_t)j0 * n, v.x, c->stride, nv, true);
            vec_download(c, r_loc_set + (size_t)j0 * n, v.r, c->stride, nv, true);
        }
        BICG_HIP(hipStreamSynchronize(c->sc));
        for (int j = 0; j < nv; ++j) {
            kmax = std::max(kmax, h.k[j]);
            if (res) {
                bicg_result &q = res[j0 + j];
                memset(&q, 0, sizeof q);
                q.iterations = h.k[j]; q.dot_r = h.dot_r[j]; q.dot_zero = h.dot_zero[j]; q.breakdown_iteration = h.breakdown[j];
            }
            if (tracing) {
                const int k = h.k[j];
                std::vector<double> &t = c->mt_host_trace[(size_t)(j0 + j)];
                t.resize(4 * (size_t)k);
                c->mt_iters[(size_t)(j0 + j)] = k;
                for (int q = 0; q < 4 && k > 0; ++q)
                    BICG_HIP(hipMemcpy(t.data() + (size_t)q * k, c->mt_trace + ((size_t)q * kSpmmCols + j) * c->mt_trace_cap, sizeof(double) * k,
                                       hipMemcpyDeviceToHost));
            }
        }
    }
    if (res)
        for (int j = 0; j < nrhs; ++j) { res[j].seconds = t_total; res[j].iter_seconds = t_iter; }
    return kmax;
}

}  // namespace

extern "C" {

int bicg_solve_multi(bicg_ctx *c, int method, double *x_loc_set, double *r_loc_set, int nrhs, const bicg_options *opt_in,
                     bicg_result *res)
{
    return solve_multi_any(c, method, x_loc_set, r_loc_set, c ? c->n_loc : 0, nrhs, opt_in, res, false, nullptr);
}

int bicg_solve_multi_device(bicg_ctx *c, int method, double *x_set_d, double *r_set_d, size_t ld, int nrhs, const bicg_options *opt_in,
                            bicg_result *res, void *stream)
{
    return solve_multi_any(c, method, x_set_d, r_set_d, ld, nrhs, opt_in, res, true, (hipStream_t)stream);
}

// measurement only (tools/multi_precond_probe.py): `reps` set applications P -> P^ of the installed block preconditioner on ncols
// columns of ones, back to back between two events, every column's flag up. chunk: launch_bjac_apply_set's. Not collective.
int bicg_precond_apply_set_bench(bicg_ctx *c, int ncols, int chunk, int reps, double *ms_per_apply)
{
    if (!c || c->pc.kind != Precond::BLOCK || ncols < 1 || ncols > kSpmmCols || !ms_per_apply) return -2;
    use_device(c);
    multi_buffers(c);
    multi_hat_buffers(c);
    const MultiVecs v = multi_vecs(c, Precond::BLOCK);
    MultiScal h;
    memset(&h, 0, sizeof h);
    for (int j = 0; j < ncols; ++j) h.active[j] = 1;
    std::vector<double> ones(c->n_loc, 1.0);
    BICG_HIP(hipMemcpyAsync(c->mt_S, &h, sizeof h, hipMemcpyHostToDevice, c->sc));
    for (int j = 0; j < ncols; ++j)
        BICG_HIP(hipMemcpyAsync(v.p + (size_t)j * c->stride, ones.data(), sizeof(double) * c->n_loc, hipMemcpyHostToDevice, c->sc));
    BICG_HIP(hipStreamSynchronize(c->sc));
    for (int i = 0; i < 3; ++i) precond_apply_set(c, v.p, v.ph, ncols, c->mt_S, chunk);
    hipEvent_t a, b;
    BICG_HIP(hipEventCreate(&a)); BICG_HIP(hipEventCreate(&b));
    BICG_HIP(hipEventRecord(a, c->sc));
    for (int i = 0; i < reps; ++i) precond_apply_set(c, v.p, v.ph, ncols, c->mt_S, chunk);
    BICG_HIP(hipEventRecord(b, c->sc));
    BICG_HIP(hipEventSynchronize(b));
    BICG_HIP(hipGetLastError());
    float ms = 0.f;
    BICG_HIP(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    *ms_per_apply = (double)ms / (reps > 0 ? reps : 1);
    return 0;
}

int bicg_multi_trace(bicg_ctx *c, int column, double *alpha, double *omega, double *beta, double *dot_r)
{
    if (!c || column < 0 || (size_t)column >= c->mt_host_trace.size()) return 1;
    const int k = c->mt_iters[(size_t)column];
    const std::vector<double> &t = c->mt_host_trace[(size_t)column];
    double *dst[4] = {alpha, omega, beta, dot_r};
    for (int q = 0; q < 4; ++q)
        if (dst[q] && k > 0) memcpy(dst[q], t.data() + (size_t)q * k, sizeof(double) * k);
    return 0;
}

}  // extern "C"
