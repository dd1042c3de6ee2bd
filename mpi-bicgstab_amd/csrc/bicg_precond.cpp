// bicg_precond.cpp -- the preconditioner of a context (struct Precond, bicg_host.h; kernels: bicg_precond.hip, bicg_bjacobi.hip):
// bicg_precond_diagonal / _block_diagonal and their _device variants, _clear, _kind, _apply, _apply_bench, and the host helpers
// bicg_csr_diagonal / bicg_csr_block_diagonal. DESIGN.md sections 4.20 (diagonal) and 4.21 (block Jacobi).
#include "bicg_host.h"

// A captured iteration of a preconditioned method (BICG_GRAPH=1, graph_iteration) holds the ADDRESS of the planes (and bs) as a
// kernel argument -- the one pointer of a captured iteration that does not live as long as the context. Whenever the array is freed
// or a new one is made the captured iteration of the method that kind serves goes too, and its two eager warm-up iterations are
// due again.
static void graph_drop(bicg_ctx *c, Precond::Kind kind)
{
    for (int m = 0; m < kMethods; ++m) {
        if (kMethod[m].precond != kind) continue;
        if (c->graph_exec[m]) { (void)hipGraphExecDestroy(c->graph_exec[m]); c->graph_exec[m] = nullptr; }
        c->graph_warm[m] = 0;
    }
}
static void precond_release(bicg_ctx *c)
{
    if (c->pc.kind == Precond::NONE) return;
    graph_drop(c, c->pc.kind);
    c->own.free(c->pc.planes);
    c->pc = Precond{};
}
// The resident array an install of (kind, bs) writes into. The array that is there stays, with its captured iteration, when it is
// of this kind and this bs; anything else is released first. Called only once the preparing kernel has reported success, so a
// refused install leaves whatever was installed, of either kind.
static double *precond_hold(bicg_ctx *c, Precond::Kind kind, int bs)
{
    Precond &m = c->pc;
    if (m.kind == kind && m.bs == bs) return m.planes;
    precond_release(c);
    graph_drop(c, kind);
    m.kind = kind; m.bs = bs;
    m.stride = kind == Precond::DIAGONAL ? (size_t)c->n_loc : ((size_t)c->n_loc + 31) / 32 * 32;
    m.planes = c->own.alloc<double>(m.stride * (size_t)bs);
    return m.planes;
}

// out = M^-1 in. The diagonal is the one-plane case in the context's own numbering (z_i = dinv_i v_i, the product FDiagQ / FDiagP
// form); blocks follow the caller's numbering, so a reordered context passes its permutation and the inverse.
void precond_apply(bicg_ctx *c, const double *in, double *out)
{
    const Precond &m = c->pc;
    const bool ro = m.kind == Precond::BLOCK && c->reordered;
    launch_bjac_apply(m.planes, m.stride, m.bs, ro ? c->ro_perm : nullptr, ro ? c->ro_inv : nullptr, in, out, c->n_loc, c->sc);
}

void precond_apply_set(bicg_ctx *c, const double *in, double *out, int nv, const MultiScal *S, int chunk)
{
    const Precond &m = c->pc;
    const bool ro = m.kind == Precond::BLOCK && c->reordered;
    launch_bjac_apply_set(m.planes, m.stride, m.bs, ro ? c->ro_perm : nullptr, ro ? c->ro_inv : nullptr, in, out, c->stride, c->n_loc, nv, S,
                          chunk, c->sc);
}

// src_dev: the caller's d (DIAGONAL) or blocks (BLOCK) on the device, caller's numbering. One launch prepares the result outside
// the resident array and raises the flag for an entry or block it has to refuse: 1 / d -- through the permutation on a reordered
// context -- into the context's ax vector (free between any two calls: every solver writes it, a product's output, before it reads
// it, and no product takes it as input, so its halo tail does not matter); the inverted blocks into scratch of the call. Only a
// clean result goes into the resident planes: a copy, or the change of layout (through the permutation). Synchronised on return.
static int precond_install(bicg_ctx *c, Precond::Kind kind, const double *src_dev, int bs)
{
    const bool block = kind == Precond::BLOCK;
    const uint32_t *perm = c->reordered ? c->ro_perm : nullptr;
    int flag = 0;
    double *work = block ? dev_alloc<double>((size_t)bjac_blocks(c->n_loc, bs) * bs * bs) : nullptr;
    if (block) launch_bjac_invert(src_dev, c->n_loc, bs, work, c->refresh_flag, c->sc);
    else launch_dinv(src_dev, perm, c->n_loc, c->v.ax, c->refresh_flag, c->sc);
    BICG_HIP(hipGetLastError());
    BICG_HIP(hipMemcpyAsync(&flag, c->refresh_flag, sizeof(int), hipMemcpyDeviceToHost, c->sc));
    BICG_HIP(hipStreamSynchronize(c->sc));
    if (flag != 0) {                                                   // (zero again for the next call)
        BICG_HIP(hipMemsetAsync(c->refresh_flag, 0, sizeof(int), c->sc));
    } else {
        double *planes = precond_hold(c, kind, bs);
        if (block) {
            launch_bjac_planes(work, perm, c->n_loc, bs, planes, c->pc.stride, c->sc);
            BICG_HIP(hipGetLastError());
        } else BICG_HIP(hipMemcpyAsync(planes, c->v.ax, sizeof(double) * c->n_loc, hipMemcpyDeviceToDevice, c->sc));
    }
    BICG_HIP(hipStreamSynchronize(c->sc));
    dev_free(work);
    return flag != 0 ? 1 : 0;
}

// The four installing entry points. src: the caller's array, on the host (staged into a temporary of the call) or, device = true,
// on the device (what the caller enqueued on its stream -- the kernel that fills the array -- comes first). A rank without rows:
// its phantom row [1.0] is its own preconditioner, one plane with bs 1.
static int precond_entry(bicg_ctx *c, Precond::Kind kind, const double *src, int bs, bool device, void *stream)
{
    if (!c) return -1;
    if (bs < 1 || bs > 16) return -2;
    use_device(c);
    if (c->phantom) {
        const double one = 1.0;
        BICG_HIP(hipStreamSynchronize(c->sc));
        BICG_HIP(hipMemcpy(precond_hold(c, kind, 1), &one, sizeof one, hipMemcpyHostToDevice));
        return 0;
    }
    if (!src) return -1;
    double *stage = nullptr;
    if (device) cross_begin(c, (hipStream_t)stream);
    else {
        const size_t len = kind == Precond::BLOCK ? (size_t)bjac_blocks(c->n_loc, bs) * bs * bs : (size_t)c->n_loc;
        stage = dev_alloc<double>(len);
        BICG_HIP(hipMemcpyAsync(stage, src, sizeof(double) * len, hipMemcpyHostToDevice, c->sc));
        src = stage;
    }
    const int rc = precond_install(c, kind, src, bs);
    dev_free(stage);
    return rc;
}

extern "C" {

int bicg_precond_diagonal(bicg_ctx *c, const double *d_loc) { return precond_entry(c, Precond::DIAGONAL, d_loc, 1, false, nullptr); }
int bicg_precond_diagonal_device(bicg_ctx *c, const double *d_d, void *stream) { return precond_entry(c, Precond::DIAGONAL, d_d, 1, true, stream); }
int bicg_precond_block_diagonal(bicg_ctx *c, const double *blocks, int bs) { return precond_entry(c, Precond::BLOCK, blocks, bs, false, nullptr); }
int bicg_precond_block_diagonal_device(bicg_ctx *c, const double *blocks_d, int bs, void *stream)
{
    return precond_entry(c, Precond::BLOCK, blocks_d, bs, true, stream);
}

int bicg_precond_clear(bicg_ctx *c)
{
    if (!c) return -1;
    if (c->pc.kind == Precond::NONE) return 0;
    use_device(c);
    BICG_HIP(hipStreamSynchronize(c->sc));
    precond_release(c);
    return 0;
}

int bicg_precond_kind(bicg_ctx *c) { return c ? (int)c->pc.kind : 0; }

int bicg_precond_apply(bicg_ctx *c, const double *v_loc, double *z_loc)
{
    if (!c || c->pc.kind == Precond::NONE) return -2;
    use_device(c);
    v_loc = host_in(c, v_loc); z_loc = host_out(c, z_loc);
    vec_upload(c, c->v.p, c->stride, v_loc, 1, true);
    precond_apply(c, c->v.p, c->v.z);
    BICG_HIP(hipGetLastError());
    vec_download(c, z_loc, c->v.z, c->stride, 1, true);
    BICG_HIP(hipStreamSynchronize(c->sc));
    return 0;
}

int bicg_precond_apply_bench(bicg_ctx *c, int reps, double *ms_per_apply)
{
    if (!c || c->pc.kind == Precond::NONE) return -2;
    use_device(c);
    std::vector<double> ones(c->n_loc, 1.0);
    BICG_HIP(hipMemcpyAsync(c->v.p, ones.data(), sizeof(double) * c->n_loc, hipMemcpyHostToDevice, c->sc));
    BICG_HIP(hipStreamSynchronize(c->sc));
    for (int i = 0; i < 3; ++i) precond_apply(c, c->v.p, c->v.z);
    hipEvent_t a, b;
    BICG_HIP(hipEventCreate(&a)); BICG_HIP(hipEventCreate(&b));
    BICG_HIP(hipEventRecord(a, c->sc));
    for (int i = 0; i < reps; ++i) precond_apply(c, c->v.p, c->v.z);
    BICG_HIP(hipEventRecord(b, c->sc));
    BICG_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    BICG_HIP(hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    *ms_per_apply = (double)ms / (reps > 0 ? reps : 1);
    return 0;
}

int bicg_csr_block_diagonal(const CSR_Matrix *diag, int bs, double *blocks_out)
{
    if (bs < 1 || bs > 16) return -2;      // (nothing written)
    const size_t nb = ((size_t)diag->rows + (size_t)bs - 1) / (size_t)bs;
    std::fill(blocks_out, blocks_out + nb * (size_t)bs * (size_t)bs, 0.0);
    int missing = 0;
    for (unsigned i = 0; i < diag->rows; ++i) {
        const unsigned base = i / (unsigned)bs * (unsigned)bs;
        double *row = blocks_out + (size_t)i * (size_t)bs;             // (block k, row a) starts at (k bs + a) bs = i bs
        unsigned stored = 0;                                           // the in-block columns met so far, a bit each: the first one assigns
        bool have = false;
        for (unsigned k = diag->ptr[i]; k < diag->ptr[i + 1]; ++k) {
            const unsigned col = diag->col[k];
            if (col < base || col - base >= (unsigned)bs) continue;
            const unsigned j = col - base;
            row[j] = (stored >> j & 1u) ? row[j] + diag->val[k] : diag->val[k];
            stored |= 1u << j;
            if (col == i) have = true;
        }
        if (!have) ++missing;
    }
    return missing;
}

int bicg_csr_diagonal(const CSR_Matrix *diag, double *d_out)
{
    int missing = 0;
    for (unsigned i = 0; i < diag->rows; ++i) {
        bool have = false;
        double sum = 0.0;
        for (unsigned k = diag->ptr[i]; k < diag->ptr[i + 1]; ++k)
            if (diag->col[k] == i) { sum = have ? sum + diag->val[k] : diag->val[k]; have = true; }
        d_out[i] = have ? sum : 0.0;
        if (!have) ++missing;
    }
    return missing;
}

}  // extern "C"
