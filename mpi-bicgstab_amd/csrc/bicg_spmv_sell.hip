// bicg_spmv_sell.hip -- the sliced-ELL product's host side: the choice of the layout's translation unit
// (bicg_spmv_sell_lay.hip, one per layout) and the code objects loaded at set-up. No kernel is instantiated here.
// (the grid, sell_grid: bicg_spmv_plan.cpp)
#include "bicg_spmv_sell.h"

namespace bicg {

// The layouts, each instantiated in a translation unit of its own (the Makefile's SELL_LAYS names the same seven). The first
// entry serves a layout value that is not in the list.
#define SELL_LAYS(X) X(LAY_PAD32) X(LAY_PAD16) X(LAY_JAG32) X(LAY_JAG16) X(LAY_JAGW) X(LAY_PAD32C) X(LAY_PAD16C)
#define SELL_LAY_EXTERN(L)                                         \
    extern template bool sell_launch_layout<L>(SELL_LAY_ARGS);     \
    extern template bool sell_epi_launch_layout<L>(SELL_LAY_ARGS); \
    extern template void preload_layout<L>();
SELL_LAYS(SELL_LAY_EXTERN)
#undef SELL_LAY_EXTERN

struct SellLay {
    int lay;
    bool (*spmv)(SELL_LAY_ARGS);
    bool (*spmv_epi)(SELL_LAY_ARGS);
    void (*preload)();
};
static const SellLay &sell_lay(const SellDev &d)
{
#define SELL_LAY_ENTRY(L) {L, sell_launch_layout<L>, sell_epi_launch_layout<L>, preload_layout<L>},
    static const SellLay lays[] = {SELL_LAYS(SELL_LAY_ENTRY)};
#undef SELL_LAY_ENTRY
    const int lay = sell_layout(d);
    for (const SellLay &l : lays)
        if (l.lay == lay) return l;
    return lays[0];
}
#undef SELL_LAYS

// ---- code objects loaded at set-up, not at the first launch -------------------------------------------------------------
// (why: preload_layout, bicg_spmv_sell.h) One kernel of each of the four units every context launches from -- the scalar /
// exchange kernels, the element-wise phases, the CSR products, the fall-back SpMM -- then the unit of the context's layout.
void preload_kernels(const SellDev &d, bool sell)
{
    preload_exchange_kernels();
    preload_vec_kernels();
    preload_csr_kernels();
    preload_spmm_sell_kernels();
    if (!sell) return;
    sell_lay(d).preload();
}

bool launch_spmv_sell(const SpmvArgs &a, int ndot, bool with_offd, hipStream_t st, hipEvent_t e0, hipEvent_t e1, bool fused_halo)
{
    const int lay = sell_layout(a.sell);
    if (a.nlist) {
        g_product_kernels |= lay == LAY_JAGW ? (jagw_fast_ok(a, with_offd, fused_halo) ? 0u : (unsigned)PK_SELL_WINLOOP)
                             : (lay == LAY_JAG32 || lay == LAY_JAG16) ? (jagd_fast_ok(a, with_offd, fused_halo) ? 0u : (unsigned)PK_SELL_JAG)
                             : (unsigned)PK_SELL_PAD;
    }
    if ((lay == LAY_JAG32 || lay == LAY_JAG16) && jagd_fast_ok(a, with_offd, fused_halo)) return launch_spmv_jagd(a, ndot, st, e0, e1);
    if (lay == LAY_JAGW && jagw_fast_ok(a, with_offd, fused_halo)) return launch_spmv_jagw(a, ndot, st, e0, e1);
    return sell_lay(a.sell).spmv(a, ndot, with_offd, st, e0, e1, fused_halo);
}

bool launch_spmv_sell_epi(const SpmvArgs &a, int epi, bool with_offd, hipStream_t st, hipEvent_t e0, hipEvent_t e1, bool fused_halo)
{
    if (a.nlist) g_product_kernels |= PK_SELL_EPI;
    return sell_lay(a.sell).spmv_epi(a, epi, with_offd, st, e0, e1, fused_halo);
}

}  // namespace bicg
