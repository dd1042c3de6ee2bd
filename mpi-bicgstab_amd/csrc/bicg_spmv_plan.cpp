// bicg_spmv_plan.cpp -- the launch plan of the distributed product (spmv_plan, bicg_plan.h) and the grid arithmetic it adds up.
// Host only: nothing here calls the HIP runtime or reads the environment. C view for tests: bicg_spmv_launch_plan.
//
// Up to four launches share one dot group, one partial slot per workgroup, numbered in launch order: {sliced-ELL groups, CSR row
// blocks} x {interior, halo-touching}. What the plan counts has to agree with what the kernels publish, slot for slot: a group
// that expects more slots than its launches write waits for partial sums that never come. So the grids the launch wrappers use
// (sell_grid, spmv_grid, stencil_grid: declared in bicg_device.h) are defined here, next to the sums made of them.
#include <algorithm>

#include "bicg_plan.h"

namespace bicg {

// workgroups launched for ngroups 256-row groups: every workgroup gets the same number (+-1)
unsigned sell_grid(uint32_t ngroups, int per_wg)
{
    if (ngroups == 0) return 0;
    if (per_wg < 1) per_wg = 1;
    const unsigned per = (unsigned)per_wg;
    const unsigned grid0 = (ngroups + per - 1) / per;             // upper bound on workgroups
    const unsigned each = (ngroups + grid0 - 1) / grid0;
    return (ngroups + each - 1) / each;
}

// CSR row blocks: one workgroup per row block, beyond kSpmvMaxGrid the kernel's loop strides (bicg_spmv_csr.hip)
unsigned spmv_grid(uint32_t nlist)
{
    if (nlist == 0) return 0;
    return nlist < (uint32_t)kSpmvMaxGrid ? nlist : (unsigned)kSpmvMaxGrid;
}

// the plane-marching product's own tiling (bicg_stencil.hip)
unsigned stencil_grid(const StencilDev &st)
{
    if (!st.on) return 0u;
    const unsigned nyw = (st.ny + 4u * st.lines - 1u) / (4u * st.lines), nzb = (st.z_hi - st.z_lo + st.zl - 1u) / st.zl;
    return (st.wide ? st.nxs / st.wide : st.nxs) * nyw * nzb;
}

const char *spmv_plan_error(int error)
{
    switch (error) {
    case SPMV_ERR_EPI3: return "CA-BiCGStab's fused q / y epilogue without the plane-marching product";
    case SPMV_ERR_EPI_MULTI: return "SpMV epilogue on a multi-launch SpMV";
    case SPMV_ERR_STENCIL_DECLINED: return "the plane-marching product declined a launch its plan had selected (lines per wavefront / reduction mode)";
    default: return "";
    }
}

SpmvPlan spmv_plan(const SpmvShape &s, const SpmvCall &k)
{
    SpmvPlan p;
    const bool single = s.transport == SPMV_SINGLE, p2p = s.transport == SPMV_P2P;
    const unsigned ng = s.ng_int + s.ng_bnd;
    p.groups_per_wg = k.ndot > 0 ? s.sell_gpw_dots : s.sell_gpw;
    // Ranks SHARING a GPU (tests; bicg_ctx::wg_cap): a launch with the halo exchange inside may consist of workgroups that ALL wait
    // for another rank's values (a numbering without locality: every 256-row group touches the halo). The first rank's launch would
    // fill the device with waiting workgroups and keep the launches that hold the awaited pushes out until the time-out; every
    // rank's launch, pushing workgroups included, has to fit beside the others'.
    if (s.wg_cap && p2p && s.ll_fused) {
        const unsigned room = s.wg_cap > 80u ? s.wg_cap - 64u : 16u;
        p.groups_per_wg = std::max<int>(p.groups_per_wg, (int)((ng + room - 1) / room));
    }
    // the plane-marching product (bicg_stencil.hip) takes the rank's halo-free planes in one launch of its own tiling; across ranks
    // the halo-touching planes follow behind the exchange through the slice-by-slice kernel, as separate launches (never the
    // launch with the exchange inside)
    p.stencil = s.stencil_ok && (k.epi == 0 || k.epi == 3) && !k.has_shift;
    if (k.epi == 3 && !(p.stencil && single)) { p.error = SPMV_ERR_EPI3; return p; }
    p.fused = p2p && s.ll_fused && !p.stencil;
    // hosted, nothing overlaps the exchange: one launch over ALL sliced-ELL groups (rows without offd entries simply find an empty
    // offd range) instead of an interior + a boundary launch
    p.merged = !single && !p.stencil && (p.fused || (!p2p && !s.own_stream && s.glist_all));
    const unsigned g_si = p.stencil ? s.stencil_wgs : sell_grid(s.ng_int, p.groups_per_wg), g_ci = spmv_grid(s.n_int);
    const unsigned g_sb = sell_grid(s.ng_bnd, p.groups_per_wg), g_cb = spmv_grid(s.n_bnd);
    const unsigned g_sall = sell_grid(ng, p.groups_per_wg);
    p.expected = p.merged ? g_sall + g_ci + g_cb : g_si + g_ci + g_sb + g_cb;
    p.tail = k.tail;
    if (p.tail) {
        // The tail finish keeps the group's last min(expected, kShards) workgroups IN LAUNCH ORDER behind to add the slots. All of
        // them must belong to the launch that comes last on this stream: a stayer of an earlier launch would wait for slots that
        // only a later launch writes, and that launch cannot start behind it. So a group whose workgroups come from several
        // launches, the last of them smaller than that, closes by arrival tickets instead -- same slots, same shard membership,
        // same order of every sum, hence the same bits. (The launch with the exchange inside never carries a tail finish.)
        const unsigned grids[4] = {p.merged ? g_sall : g_si, g_ci, p.merged || single ? 0u : g_sb, single ? 0u : g_cb};
        unsigned launches = 0, last = 0;
        for (unsigned g : grids)
            if (g) { ++launches; last = g; }
        if (launches > 1 && last < std::min<unsigned>(p.expected, (unsigned)kShards)) p.tail = false;
    }
    p.hand_nsh = std::min<unsigned>(p.expected, (unsigned)kShards);      // what the consuming kernel will find
    p.sets_nparts = k.wave && (k.ndot > 0 || k.epi);                     // one partial per wavefront
    if (k.epi && !(s.glist_all && s.nblk == 0 && (single || p.fused))) { p.error = SPMV_ERR_EPI_MULTI; return p; }
    // (the plane-marching launch takes its epilogue with ticket reductions only: declined, it would leave y unwritten and a ticket
    // group waiting for partial sums that never come)
    // A necessary condition only: the wrapper also declines tilings it is not built for and judges the reduction mode from the whole
    // Reduce / Finish pair, which the plan does not see. launch_step (bicg_solver.cpp) keeps the authoritative check.
    if (p.stencil && k.epi && k.wave) { p.error = SPMV_ERR_STENCIL_DECLINED; return p; }
    // Epilogue launches publish one partial row per WAVEFRONT for 32 helper workgroups to add: beyond a few thousand
    // workgroups that sum, not the matrix, sets the pace (16.8 M rows = 65 k workgroups: 4.6 instead of 1.25 ms per
    // iteration), so a workgroup takes several 256-row groups. Ranks sharing a GPU (tests): every row workgroup of
    // the launch waits for the scalars, all ranks' launches must fit on the GPU together.
    // (the slot bases, the tail decision and hand_nsh above keep the grids from before the cap: DESIGN.md section 5.1, "oddities")
    const unsigned epi_cap = s.wg_cap ? s.wg_cap : 8192u;
    if (k.epi && !p.stencil && ng > epi_cap) {
        p.groups_per_wg = std::max<int>(p.groups_per_wg, (int)((ng + epi_cap - 1) / epi_cap));
        p.expected = sell_grid(ng, p.groups_per_wg) + g_ci;
        p.sets_nparts = true;
    }

    // a launch its wrapper would decline for nlist == 0 is not a step
    auto add = [&p](int family, int list, uint32_t nlist, bool with_offd, uint32_t slot_base, bool after_halo, bool fused_halo = false,
                    bool even_empty = false) {
        if (nlist == 0 && !even_empty) return;
        SpmvStep &t = p.step[p.nsteps++];
        t.family = family; t.list = list; t.nlist = nlist; t.with_offd = with_offd; t.fused_halo = fused_halo;
        t.slot_base = slot_base; t.after_halo = after_halo;
    };
    if (single && k.epi && !p.stencil) {
        add(FAM_SELL_EPI, LIST_ALL, s.ng_int, false, 0, false);
    } else if (p.fused) {
        // ONE launch: leading workgroups push, the others multiply; halo-touching groups come last and read the landing ring directly
        add(k.epi ? FAM_SELL_EPI : FAM_SELL, LIST_FUSED, ng, true, 0, false, true, s.has_send);
        add(FAM_CSR, LIST_BLK_INT, s.n_int, false, g_sall, false);
    } else if (p.merged) {
        add(FAM_SELL, LIST_ALL, ng, true, 0, true);
        add(FAM_CSR, LIST_BLK_INT, s.n_int, false, g_sall, true);
        add(FAM_CSR, LIST_BLK_BND, s.n_bnd, true, g_sall + g_ci, true);
    } else {
        if (p.stencil) add(FAM_STENCIL, LIST_INT, s.ng_int, false, 0, false, false, true);
        else add(FAM_SELL, LIST_INT, s.ng_int, false, 0, false);
        add(FAM_CSR, LIST_BLK_INT, s.n_int, false, g_si, false);
        if (!single) {
            add(FAM_SELL, LIST_BND, s.ng_bnd, true, g_si + g_ci, true);
            add(FAM_CSR, LIST_BLK_BND, s.n_bnd, true, g_si + g_ci + g_sb, true);
        }
    }
    return p;
}

}  // namespace bicg

// C view for tests of the launch plan (include/bicgstab_hip.h section 5 documents the orders)
extern "C" int bicg_spmv_launch_plan(const unsigned int shape[15], const int call[5], unsigned int plan[10], unsigned int steps[28])
{
    using namespace bicg;
    static_assert(kSpmvShapeLen == 15 && kSpmvCallLen == 5 && kSpmvPlanLen == 10 && kSpmvStepLen * kSpmvMaxSteps == 28,
                  "lengths documented in bicgstab_hip.h");
    if (!shape || !call || !plan || !steps || shape[6] > (unsigned)SPMV_HOSTED) return 1;
    SpmvShape s;
    s.ng_int = shape[0]; s.ng_bnd = shape[1]; s.n_int = shape[2]; s.n_bnd = shape[3]; s.nblk = shape[4];
    s.glist_all = shape[5] != 0; s.transport = (int)shape[6]; s.ll_fused = shape[7] != 0; s.has_send = shape[8] != 0;
    s.own_stream = shape[9] != 0; s.stencil_ok = shape[10] != 0; s.stencil_wgs = shape[11];
    s.sell_gpw = (int)shape[12]; s.sell_gpw_dots = (int)shape[13]; s.wg_cap = shape[14];
    SpmvCall k;
    k.ndot = call[0]; k.epi = call[1]; k.has_shift = call[2] != 0; k.tail = call[3] != 0; k.wave = call[4] != 0;
    const SpmvPlan p = spmv_plan(s, k);
    const unsigned head[kSpmvPlanLen] = {(unsigned)p.error, (unsigned)p.groups_per_wg, p.stencil, p.fused, p.merged, p.expected,
                                         p.hand_nsh, p.sets_nparts, p.tail, (unsigned)p.nsteps};
    std::copy(head, head + kSpmvPlanLen, plan);
    std::fill(steps, steps + kSpmvStepLen * kSpmvMaxSteps, 0u);
    for (int i = 0; i < p.nsteps; ++i) {
        const SpmvStep &t = p.step[i];
        const unsigned row[kSpmvStepLen] = {(unsigned)t.family, (unsigned)t.list, t.nlist, t.with_offd, t.fused_halo, t.slot_base, t.after_halo};
        std::copy(row, row + kSpmvStepLen, steps + i * kSpmvStepLen);
    }
    return 0;
}
