// bicg_refresh.cpp -- bicg_update_values / bicg_update_values_device: new values for the matrix of a context, same sparsity
// pattern, written into the arrays that are already on the device (kernels: bicg_refresh.hip). The plan
// -- layout, windows, lists, 16-bit offsets, row blocks, group selection -- follows from the pattern alone, so nothing is planned
// again and no address changes. Where the values live, and how each copy is refilled:
//   c->diag.val      CSR order, only where row blocks exist (k_spmv, k_spmv_rows)         copy; reordered: row by row through perm
//   c->offd.val      stored order (the halo plan renumbers columns only)                  copy
//   c->sell.val      padded or jagged slices of the groups on the sliced path             k_refresh_pad / k_refresh_jag
//   c->persist.pval  the persistent plan's padded slices                                  through c->persist_psrc
//   sell.uval, StencilTab   values of constant / masked slices, shared between slices     never rewritten: verified first, any
//                                                                                         difference refuses the whole call
#include "bicg_host.h"

namespace {

// Every rank-local step of the refill, on the compute stream. dval / oval: device arrays in the caller's CSR order; they may BE
// c->diag.val / c->offd.val (the host variant uploads straight into them where that is the stored form).
int refresh_device(bicg_ctx *c, const double *dval, const double *oval)
{
    const RefreshSrc src{dval, c->reordered ? c->ro_src_ptr : c->diag.ptr, c->reordered ? c->ro_perm : nullptr};
    hipStream_t st = c->sc;
    if (c->constant_entries > 0 && c->sell.vbase) {
        int flag = 0;
        launch_refresh_verify(src, c->diag.ptr, c->n_loc, c->sell, c->refresh_flag, st);
        BICG_HIP(hipMemcpyAsync(&flag, c->refresh_flag, sizeof(int), hipMemcpyDeviceToHost, st));
        BICG_HIP(hipStreamSynchronize(st));
        if (flag != 0) {                                               // (zero again for the next call)
            BICG_HIP(hipMemsetAsync(c->refresh_flag, 0, sizeof(int), st));
            BICG_HIP(hipStreamSynchronize(st));
            return 1;
        }
    }
    if (c->nblk > 0 && dval != c->diag.val) {
        double *dst = const_cast<double *>(c->diag.val);
        if (c->reordered) launch_refresh_rows(src, c->diag.ptr, c->n_loc, dst, st);
        else BICG_HIP(hipMemcpyAsync(dst, dval, sizeof(double) * c->nnz_d, hipMemcpyDeviceToDevice, st));
    }
    if (c->nnz_o > 0 && oval != c->offd.val)
        BICG_HIP(hipMemcpyAsync(const_cast<double *>(c->offd.val), oval, sizeof(double) * c->nnz_o, hipMemcpyDeviceToDevice, st));
    if (c->sell_entries > 0) {
        double *sval = const_cast<double *>(c->sell.val);
        launch_refresh_sell(src, c->diag.ptr, c->n_loc, c->sell, c->glist_int_identity ? nullptr : c->glist_int, c->ng_int, sval, st);
        launch_refresh_sell(src, c->diag.ptr, c->n_loc, c->sell, c->glist_bnd, c->ng_bnd, sval, st);
    }
    if (c->persist_psrc && c->persist_entries > 0)
        launch_refresh_persist(dval, oval, c->nnz_d, c->persist_psrc, c->persist_entries, const_cast<double *>(c->persist.pval), st);
    BICG_HIP(hipGetLastError());
    BICG_HIP(hipStreamSynchronize(st));
    return 0;
}

// 0: go on; otherwise the value to return at once (a rank without rows has nothing to update)
int refresh_args(bicg_ctx *c, const double *diag_val, const double *offd_val, bool *nothing)
{
    *nothing = false;
    if (!c) return -1;
    if (c->phantom) { *nothing = true; return 0; }
    if ((c->nnz_d > 0 && !diag_val) || (c->nnz_o > 0 && !offd_val)) return -1;
    return 0;
}

}  // namespace

extern "C" {

int bicg_update_values_device(bicg_ctx *c, const double *diag_val_d, const double *offd_val_d)
{
    bool nothing;
    if (const int rc = refresh_args(c, diag_val_d, offd_val_d, &nothing)) return rc;
    if (nothing) return 0;
    use_device(c);
    return refresh_device(c, diag_val_d, offd_val_d);
}

int bicg_update_values(bicg_ctx *c, const double *diag_val, const double *offd_val)
{
    bool nothing;
    if (const int rc = refresh_args(c, diag_val, offd_val, &nothing)) return rc;
    if (nothing) return 0;
    use_device(c);
    // A context that keeps CSR values anyway takes the upload straight into them -- unless list-held values have to be verified
    // before anything is written, or the stored order is not the caller's (reordered). Otherwise a staging buffer of this call.
    const bool direct_ok = !(c->constant_entries > 0 && c->sell.vbase);
    const bool d_direct = direct_ok && c->nblk > 0 && !c->reordered;
    double *stage_d = nullptr, *stage_o = nullptr;
    const double *dval = c->diag.val, *oval = c->offd.val;
    if (c->nnz_d > 0) {
        double *dst = d_direct ? const_cast<double *>(c->diag.val) : (stage_d = dev_alloc<double>(c->nnz_d));
        BICG_HIP(hipMemcpyAsync(dst, diag_val, sizeof(double) * c->nnz_d, hipMemcpyHostToDevice, c->sc));
        dval = dst;
    }
    if (c->nnz_o > 0) {
        double *dst = direct_ok ? const_cast<double *>(c->offd.val) : (stage_o = dev_alloc<double>(c->nnz_o));
        BICG_HIP(hipMemcpyAsync(dst, offd_val, sizeof(double) * c->nnz_o, hipMemcpyHostToDevice, c->sc));
        oval = dst;
    }
    const int rc = refresh_device(c, dval, oval);
    if (rc != 0) BICG_HIP(hipStreamSynchronize(c->sc));
    dev_free(stage_d);
    dev_free(stage_o);
    return rc;
}

}  // extern "C"
