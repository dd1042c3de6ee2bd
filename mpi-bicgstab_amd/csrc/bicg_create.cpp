// bicg_create.cpp -- building a context. bicg_create reads as a table of contents: facts shared by all ranks, halo plan,
// the plan of the diag block (made on the host by sell_plan_host, bicg_sell_plan.cpp), sell_plan_upload -- the only place that
// turns that plan into device memory and adds up the matrix's bytes --, slice descriptors and the stencil plan, the peer-to-peer
// transport, and the tail it shares with bicg_create_device_csr (ctx_finish: state, persistent set-up, streams, code objects);
// tearing a context down again. Split from bicg_solver.cpp in round 5; see bicg_host.h.
#include "bicg_host.h"

std::vector<bicg_ctx *> g_live;

// BICG_PLAN_TRACE (a user switch: the plan's stages and their seconds on stderr), read here only
static const char *plan_trace_env() { return getenv("BICG_PLAN_TRACE"); }

bool all_ranks(Comm *comm, bool mine)
{
    const int P = comm->nranks;
    if (P == 1) return mine;
    std::vector<int> cnt(P, (int)sizeof(int)), dsp(P), out(P, mine ? 1 : 0), in(P, 0);
    for (int p = 0; p < P; ++p) dsp[p] = p * (int)sizeof(int);
    comm->alltoallv_host(out.data(), cnt.data(), dsp.data(), in.data(), cnt.data(), dsp.data());
    in[comm->rank] = mine ? 1 : 0;
    for (int p = 0; p < P; ++p) if (!in[p]) return false;
    return true;
}


static void build_stencil_plan(bicg_ctx *c, uint32_t nslices, uint32_t nrows, const std::vector<uint4> &d, const std::vector<int> &uoff,
                               const std::vector<double> &uval, const unsigned short *rmask_host);
static void build_slice_desc(bicg_ctx *c, uint32_t nslices, uint32_t nrows, const uint32_t *slice_len, const std::vector<uint32_t> &ubase,
                             const std::vector<uint32_t> &vbase, const std::vector<uint32_t> &mbase, const std::vector<int> &uoff,
                             const std::vector<double> &uval, const unsigned short *rmask_host)
{
    if (vbase.empty() || ubase.empty() || (uint64_t)nrows >= (1ull << 29)) return;
    if (plan_off("desc")) return;
    std::vector<uint4> d(nslices);
    bool all_lists = !plan_off("lists") && nrows % kGroupRows == 0;
    for (uint32_t sl = 0; sl < nslices; ++sl) {
        const uint32_t ub = ubase[sl], vb = vbase[sl], mb = mbase.empty() ? 0xFFFFFFFFu : mbase[sl];
        uint32_t len = slice_len[sl] & 0xFFFFu, kind = kSliceGeneral, w = 0;
        if (ub != 0xFFFFFFFFu && slice_len[sl] <= 0xFFFFu) {
            kind = kSliceUniform;
            if (vb != 0xFFFFFFFFu) {
                kind = kSliceConstant;
                if (mb != 0xFFFFFFFFu) { kind = kSliceMasked; len = mb >> 26; w = mb & 0x03FFFFFFu; }
            }
        }
        d[sl] = make_uint4(len | (kind << 16), kind >= kSliceConstant ? ub : 0u, kind >= kSliceConstant ? vb : 0u, w);
        if ((uint64_t)sl * kSliceRows < nrows && (kind < kSliceConstant || len == 0 || len > 8u)) all_lists = false;
    }
    if (all_lists) {                              // (SellDev::all_lists: the distances once more, as byte offsets)
        std::vector<int> u8(uoff.size());
        for (size_t i = 0; i < uoff.size(); ++i) u8[i] = (int)((uint32_t)uoff[i] * 8u);      // (modulo 2^32: the product adds it to the row's byte offset modulo 2^32)
        c->sell.uoff8 = c->own.upload(u8.data(), u8.size());
        c->sell.all_lists = 1;
        // SellDev::ystride from the longest list (the interior's): its second-largest distance is a grid line when it is a multiple
        // of 64 rows. (Only the speed depends on the guess: any value gives every slice to exactly one wavefront.)
        uint32_t best_len = 0, best_at = 0;
        for (uint32_t sl = 0; sl < nslices; ++sl) { const uint32_t l = d[sl].x & 0xFFFFu; if ((d[sl].x >> 16) == kSliceConstant && l > best_len) { best_len = l; best_at = d[sl].y; } }
        // (measured, 512^3: 0.923 against 0.929 ms per product, 256^3 0.146 against 0.123 ms -- off unless BICG_SELL_YGROUP=1)
        if (best_len >= 5 && knob_x("BICG_SELL_YGROUP") && atoi(knob_x("BICG_SELL_YGROUP")) != 0) {
            std::vector<int> dist(uoff.begin() + best_at, uoff.begin() + best_at + best_len);
            std::sort(dist.begin(), dist.end());
            const int line = dist[best_len - 2];
            const uint32_t S = line > 0 ? (uint32_t)line / kSliceRows : 0u;
            if (S >= 1 && (uint32_t)line % kSliceRows == 0 && (S & (S - 1u)) == 0 && nslices % (4u * S) == 0) c->sell.ystride = (int)S;   // (a power of two: shifts in the kernel)
        }
    }
    c->sell.sdesc = c->own.upload(d.data(), d.size());
    if (all_lists) build_stencil_plan(c, nslices, nrows, d, uoff, uval, rmask_host);
}

// The plane-marching product (struct StencilDev, bicg_stencil.hip): is this block the 7-point stencil of a grid? Decided from the
// lists alone -- the interior's list must be (-sz, -sy, -1, 0, +1, +sy, +sz) with sy a multiple of 64 rows, sz a multiple of sy,
// the rows a multiple of sz, and every other list a sub-sequence of it in the same order. Values may differ from list to list
// (every (distance list, value list) pair gets a table entry); rows of masked slices get their entries as canonical bits.
static void build_stencil_plan(bicg_ctx *c, uint32_t nslices, uint32_t nrows, const std::vector<uint4> &d, const std::vector<int> &uoff,
                               const std::vector<double> &uval, const unsigned short *rmask_host)
{
    if (plan_off("stencil")) return;
    uint32_t best_at = 0, best_len = 0;
    // the interior's list: the longest one, of a constant slice or (a grid one x segment wide has no other) of a masked one
    for (uint32_t sl = 0; sl < nslices; ++sl) { const uint32_t l = d[sl].x & 0xFFFFu; if ((d[sl].x >> 16) >= kSliceConstant && l > best_len) { best_len = l; best_at = d[sl].y; } }
    if (best_len != 7) return;
    const int *L = uoff.data() + best_at;
    if (!(L[3] == 0 && L[2] == -1 && L[4] == 1 && L[5] > 1 && L[6] > L[5] && L[1] == -L[5] && L[0] == -L[6])) return;
    const uint32_t sy = (uint32_t)L[5], sz = (uint32_t)L[6];
    if (sy % kSliceRows || sz % sy || nrows % sz || sy / kSliceRows > 64u) return;
    const uint32_t nxs = sy / kSliceRows, ny = sz / sy, nz = nrows / sz;
    if (ny % 2u) return;
    const int canon[7] = {-(int)sz, -(int)sy, -1, 0, 1, (int)sy, (int)sz};
    struct Entry { StencilTab t; signed char pos[8]; };
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, uint32_t> pairs;
    std::vector<Entry> entries;
    std::vector<uint32_t> code(nslices), which(nslices);
    unsigned long long mcols = 0;
    for (uint32_t sl = 0; sl < nslices; ++sl) {
        const uint32_t kind = d[sl].x >> 16, len = d[sl].x & 0xFFFFu;
        const auto key = std::make_tuple(d[sl].y, d[sl].z, len);
        auto it = pairs.find(key);
        if (it == pairs.end()) {
            if (entries.size() >= 65536u) return;
            Entry e;
            memset(&e, 0, sizeof e);
            int cpos = -1;
            for (uint32_t k = 0; k < len; ++k) {
                int at = -1;
                for (int q = cpos + 1; q < 7; ++q) if (canon[q] == uoff[d[sl].y + k]) { at = q; break; }
                if (at < 0) return;                                   // a distance the grid does not have, or out of order: not this product
                cpos = at;
                e.t.v[at] = uval[d[sl].z + k];
                e.t.bits |= 1ull << at;
                e.pos[k] = (signed char)at;
            }
            it = pairs.emplace(key, (uint32_t)entries.size()).first;
            entries.push_back(e);
        }
        const uint32_t xs = sl % nxs, line = sl / nxs, yy = line % ny, zz = line / ny;
        which[sl] = it->second;
        code[((size_t)zz * nxs + xs) * ny + yy] = it->second;
        if (kind == kSliceMasked) mcols |= 1ull << xs;
    }
    const uint32_t nmc = (uint32_t)__builtin_popcountll(mcols);
    std::vector<unsigned char> cmask;
    if (nmc) {
        std::vector<unsigned short> rm_dl;
        if (!rmask_host) {                                            // the device plan wrote the rows' masks on the GPU
            uint32_t top = 0;
            for (uint32_t sl = 0; sl < nslices; ++sl) if ((d[sl].x >> 16) == kSliceMasked) top = std::max(top, d[sl].w + 1u);
            rm_dl.resize((size_t)top * kSliceRows);
            BICG_HIP(hipMemcpy(rm_dl.data(), c->sell.rmask, sizeof(unsigned short) * rm_dl.size(), hipMemcpyDeviceToHost));
            rmask_host = rm_dl.data();
        }
        cmask.assign((size_t)(nslices / nxs) * nmc * kSliceRows, 0);
        parallel_ranges(nslices, 4096, [&](size_t s0, size_t s1, int) {
            for (size_t sl = s0; sl < s1; ++sl) {
                const uint32_t xs = (uint32_t)(sl % nxs);
                if (!((mcols >> xs) & 1ull)) continue;
                const uint32_t dense = (uint32_t)__builtin_popcountll(mcols & ((1ull << xs) - 1ull));
                unsigned char *out = cmask.data() + ((sl / nxs) * nmc + dense) * kSliceRows;
                const Entry &e = entries[which[sl]];
                if ((d[sl].x >> 16) == kSliceMasked) {
                    const unsigned short *pm = rmask_host + (size_t)d[sl].w * kSliceRows;
                    const uint32_t len = d[sl].x & 0xFFFFu;
                    for (uint32_t l = 0; l < kSliceRows; ++l) {
                        unsigned bits = 0;
                        for (uint32_t k = 0; k < len; ++k) if ((pm[l] >> k) & 1u) bits |= 1u << e.pos[k];
                        out[l] = (unsigned char)bits;
                    }
                } else {
                    for (uint32_t l = 0; l < kSliceRows; ++l) out[l] = (unsigned char)e.t.bits;
                }
            }
        });
    }
    std::vector<StencilTab> tab(entries.size());
    for (size_t i = 0; i < entries.size(); ++i) tab[i] = entries[i].t;
    // The wide form (bicg_stencil.hip, k_spmv_stencil_w): 2 or 4 rows per lane. It needs ONE value per canonical position -- every
    // table entry agrees with the full one wherever it has an entry -- and whole groups of x segments per line.
    uint32_t wide = 0, ref = 0;
    {
        bool have = false, same = true;
        for (size_t i = 0; i < tab.size() && !have; ++i) if ((tab[i].bits & 0x7Full) == 0x7Full) { ref = (uint32_t)i; have = true; }
        for (size_t i = 0; have && i < tab.size(); ++i)
            for (int k = 0; k < 7; ++k)
                if (((tab[i].bits >> k) & 1ull) && memcmp(&tab[i].v[k], &tab[ref].v[k], sizeof(double)) != 0) same = false;
        // two rows per lane wherever the grid is large enough for the traffic to matter (512^3: product 0.461 -> 0.423 ms, 256^3:
        // 0.0535 -> 0.052 ms, plain iteration 0.441 -> 0.424 ms; four rows per lane need 200-256 registers and lose what two gain:
        // profiles/r06/stencil_notes.txt)
        uint32_t want = nrows >= (1u << 22) ? 2u : 0u;
        if (const char *v = plan_tok("wide")) want = (uint32_t)atoi(v);
        if (have && same && (want == 2u || want == 4u) && nxs % want == 0) wide = want;
        else if (want && c->rank == 0 && plan_tok("wide")) fprintf(stderr, "bicgstab_hip: BICG_PLAN wide=%u not taken (%s)\n", want, !(want == 2u || want == 4u) ? "2 or 4 rows per lane" : nxs % want ? "the lines are not whole groups of segments" : "values differ between the lists of the block");
    }
    // lines per wavefront and planes per tile: enough workgroups for several rounds of the 1024 a GPU holds, tiles as deep as that allows
    uint32_t lines = 0, zl = 0;
    const uint32_t nxt = wide ? nxs / wide : nxs;          // tiles per line
    {
        static const uint32_t cand[][2] = {{4, 64}, {4, 32}, {4, 16}, {2, 32}, {2, 16}, {4, 8}, {2, 8}, {2, 4}};
        const uint64_t enough = wide ? 1000 : 3000;        // (the wide form keeps fewer, larger workgroups resident)
        uint64_t most = 0;
        for (auto &cd : cand) {
            if (ny % cd[0] || (!wide && cd[1] > 32)) continue;
            const uint64_t wgs = (uint64_t)nxt * ((ny + 4 * cd[0] - 1) / (4 * cd[0])) * ((nz + cd[1] - 1) / cd[1]);
            if (wgs >= enough) { lines = cd[0]; zl = cd[1]; break; }
            if (wgs > most) { most = wgs; lines = cd[0]; zl = cd[1]; }
        }
        if (const char *v = plan_tok("lines")) { const uint32_t r = (uint32_t)atoi(v); if ((r == 2 || r == 4) && ny % r == 0) lines = r; }
        if (const char *v = plan_tok("planes")) {
            // every workgroup of the product publishes one row of partial sums: the tiling must not need more rows than the table
            // has (ctx_state: max(256-row groups, kMaxGrid) + 64) -- thin grids with few planes per tile would
            const int z = atoi(v);
            const uint64_t wgs = z >= 1 ? (uint64_t)nxt * ((ny + 4 * lines - 1) / (4 * lines)) * ((nz + (uint32_t)z - 1) / (uint32_t)z) : 0;
            const uint64_t room = std::max<uint64_t>(((uint64_t)nrows + kGroupRows - 1) / kGroupRows, (uint64_t)kMaxGrid);
            if (z >= 1 && wgs <= room) zl = (uint32_t)z;
            else if (c->rank == 0) fprintf(stderr, "bicgstab_hip: BICG_PLAN planes=%s ignored (%llu workgroups, room for %llu partial-sum rows)\n", v, (unsigned long long)wgs, (unsigned long long)room);
        }
    }
    const uint32_t *wbits_d = nullptr;
    if (wide) {
        std::vector<uint32_t> wb((size_t)nz * nxt * ny);
        parallel_ranges(wb.size(), 65536, [&](size_t i0, size_t i1, int) {
            for (size_t i = i0; i < i1; ++i) {
                const size_t yy = i % ny, xw = (i / ny) % nxt, zz = i / ((size_t)ny * nxt);
                uint32_t word = 0;
                for (uint32_t q = 0; q < wide; ++q) word |= (uint32_t)(tab[code[(zz * nxs + xw * wide + q) * ny + yy]].bits & 0x7Full) << (8u * q);
                wb[i] = word;
            }
        });
        wbits_d = c->own.upload(wb.data(), wb.size());
    }
    const uint32_t *code_d = c->own.upload(code.data(), code.size());
    const StencilTab *tab_d = c->own.upload(tab.data(), tab.size());
    const unsigned char *cmask_d = nmc ? c->own.upload(cmask.data(), cmask.size()) : nullptr;
    // Input + output vector far beyond the 256 MiB Infinity Cache (512^3: 2 x 1 GiB): y is stored non-temporally and the tiles go to
    // the XCDs round-robin (product 0.480 -> 0.460 ms, CA-BiCGStab 5.40 -> 5.31 ms per iteration); a grid whose vectors the cache
    // holds (256^3) keeps ordinary stores and the XCD-contiguous order (0.053 against 0.061 ms): profiles/r05/stencil_sweep_xcd_nt.txt
    const bool st_big = 16.0 * (double)nrows > 2.0 * 256.0 * 1048576.0;
    // ... and since round 6 (the wide form) in the sweep order: an XCD takes its own eighth of the line blocks plane block by plane
    // block (0.428 -> 0.423 ms; L2 misses 13.9 M -> 12.8 M per product)
    int st_xcd = knob_x("BICG_STENCIL_XCD") ? atoi(knob_x("BICG_STENCIL_XCD")) : (st_big ? (wide ? 2 : 0) : 1);
    if (st_xcd == 2 && ((ny + 4 * lines - 1) / (4 * lines)) % 8u) st_xcd = st_big ? 0 : 1;       // (the sweep order deals whole line blocks to the XCDs)
    const int st_nt = knob_x("BICG_STENCIL_NT") ? atoi(knob_x("BICG_STENCIL_NT")) : (st_big ? 1 : 0);
    c->sell.st = StencilDev{1, sy, sz, nxs, ny, nz, 0u, nz, zl, lines, nmc, st_xcd, st_nt, mcols, code_d, tab_d, cmask_d, wide, ref, wbits_d};
    if (const char *v = plan_tok("ca-fuse")) c->ca_fuse = atoi(v) != 0;
    // what this product streams from the matrix side: 4 bytes per slice, one byte per row of the masked x segments
    // (the wide form: 4 bytes per `wide` slices)
    c->stencil_matrix_bytes = 4ull * nslices / (wide ? wide : 1u) + (uint64_t)cmask.size();
    if (plan_trace_env())
        fprintf(stderr, "bicgstab_hip: plane-marching product: %u x %u x %u grid (x segments of 64 rows: %u), %zu list pairs, %u masked x segments, %u lines x %u planes per wavefront, %u rows per lane, %u workgroups\n",
                sy, ny, nz, nxs, tab.size(), nmc, lines, zl, wide ? wide : 1u, stencil_grid(c->sell.st));
}


// Very large structured blocks (the 512^3 Laplacian: 524 288 row groups, z neighbours 262 144 rows = 2 MB of x away).
//  * groups per workgroup: with one 256-row group of 7-entry rows per workgroup the per-workgroup part of a product with dots
//    (block sum, hand-over of the partials) is a third of the kernel (2.16 ms without dots, 2.76 / 3.13 ms with one / two);
//    workgroups take ceil(groups / 65536) contiguous groups each.
//  * order of the groups: an XCD sweeps its eighth of the rows plane by plane, and the three planes a sweep front touches (6 MB
//    of x) do not fit its 4 MB L2 -- every x value comes from the Infinity Cache three times. The groups of an XCD's share are
//    therefore taken block by block through the planes: B consecutive groups of plane z, the same B of plane z + 1, ... so that
//    what a block fetched as its far neighbours is still in the L2 when it becomes the block's own rows. Only the ORDER of the
//    list changes (SpmvArgs::glist): rows, sums of a row and results are those of the natural order; the dot partials are
//    added in list order (a different, equally fixed association).
// BICG_SELL_BLOCK = B (groups, default 256; 0: natural order).
void sell_order_for_big_grids(bicg_ctx *c, uint32_t ngroups)
{
    if (!knob_x("BICG_SELL_GPW") && !knob_x("BICG_SELL_GPW_DOTS")) c->sell_gpw = c->sell_gpw_dots = (int)std::max<uint32_t>(1u, (ngroups + 65535u) / 65536u);
    if (const char *sv = knob_x("BICG_SELL_GPW")) c->sell_gpw = std::max(1, atoi(sv));
    if (const char *sv = knob_x("BICG_SELL_GPW_DOTS")) c->sell_gpw_dots = std::max(1, atoi(sv));
    const uint32_t B = knob_x("BICG_SELL_BLOCK") ? (uint32_t)atoi(knob_x("BICG_SELL_BLOCK")) : 256u;
    const uint32_t P = (c->far_rows + kGroupRows / 2) / kGroupRows;          // groups per plane
    if (B == 0 || P < 4 * B || c->sell_gpw != c->sell_gpw_dots || (uint64_t)c->far_rows * 24ull <= (3ull << 19)) return;   // three planes fit half an L2
    const uint32_t nblocks = sell_grid(ngroups, c->sell_gpw), each = (ngroups + nblocks - 1) / nblocks;
    std::vector<uint32_t> list(ngroups);
    for (uint32_t x = 0; x <= 8; ++x) {
        // XCD x's share of the list (the last segment: what the division left over); within it block y of every plane, plane
        // after plane, then block y + 1 ... -- the order a sort by (block, group) would give, enumerated directly
        const uint32_t s0 = std::min<uint64_t>(ngroups, (uint64_t)x * (nblocks / 8u) * each);
        const uint32_t s1 = x == 8 ? ngroups : std::min<uint64_t>(ngroups, (uint64_t)(x + 1) * (nblocks / 8u) * each);
        uint32_t o = s0;
        for (uint32_t y0 = 0; y0 < P && o < s1; y0 += B)
            for (uint64_t z0 = s0; z0 < s1; z0 += P)
                for (uint64_t g = z0 + y0; g < std::min<uint64_t>({(uint64_t)s1, z0 + y0 + B, z0 + P}); ++g) list[o++] = (uint32_t)g;
    }
    c->own.free(c->glist_int);
    c->glist_int = c->own.upload(list.data(), list.size());
    c->glist_int_identity = false;
    c->sell_blocked = B;
}

// ---------------------------------------------------------------- persistent pipelined iteration: plan
// Which rows a workgroup owns, its part of the matrix in padded slices (diag entries first, then offd entries in the
// x_ext numbering [local rows | halo positions]) with window slots instead of columns, the window runs, and -- multi
// rank -- the send-list entries of every workgroup. Returns false when the block does not qualify.
bool persist_build(bicg_ctx *c, const CSR_Matrix *diag, const std::vector<uint32_t> &optr, const std::vector<uint32_t> &ocol,
                   const std::vector<double> &oval, const std::vector<uint32_t> &send_idx, const std::vector<unsigned long long> &dst0,
                   const std::vector<unsigned long long> &dstride)
{
    const uint32_t nrows = c->n_loc;
    const bool multi = !c->single();
    if (nrows == 0 || c->fault_after > 0) return false;
    if (!(c->glist_all && c->nblk == 0 && !c->rowsplit && (c->single() || (c->p2p && c->ll_fused)))) return false;
    hipDeviceProp_t prop;
    BICG_HIP(hipGetDeviceProperties(&prop, c->device));
    const int cus = prop.multiProcessorCount;
    // one workgroup per CU (its LDS): ranks sharing a GPU (tests) share the CUs; one CU is the helper's
    const int gmax = cus / std::max(1, c->comm->ranks_on_device) - 1;
    if (gmax < 1) return false;
    PersistPlan P;
    if (!persist_plan_host(diag, multi ? optr.data() : nullptr, multi ? ocol.data() : nullptr, multi ? oval.data() : nullptr, (unsigned)gmax, P))
        return false;
    const uint32_t nslices = P.nslices, spw = P.spw, nwg = P.nwg, grows = spw * kSliceRows;
    const uint32_t slots_used = P.win_slots, max_runs = P.max_runs, max_entries = P.max_entries;
    const std::vector<uint32_t> &pbase = P.pbase, &wptr = P.wptr;
    const std::vector<double> &pval = P.pval;
    const std::vector<unsigned short> &pslot = P.pslot, &rlen = P.rlen, &rdiag = P.rdiag;
    static_assert(sizeof(uint2) == 2 * sizeof(uint32_t), "run = two 32-bit words");
    std::vector<uint2> runs(P.runs.size() / 2 + 1);
    for (size_t i = 0; i < P.runs.size() / 2; ++i) runs[i] = make_uint2(P.runs[2 * i], P.runs[2 * i + 1]);
    PersistArgs &a = c->persist;
    a = PersistArgs{};
    a.nrows = nrows; a.nslices = nslices; a.nwg = nwg; a.spw = P.nrw; a.rpt = P.rpt;
    a.win_slots = slots_used; a.max_runs = max_runs;
    // the matrix goes to LDS when everything fits next to the window
    a.mat_entries = P.rpt == 1 ? max_entries : 0;
    if (knob_x("BICG_PERSIST_LDSMAT") && atoi(knob_x("BICG_PERSIST_LDSMAT")) == 0) a.mat_entries = 0;
    // what a workgroup may ask for on THIS device (gfx950: 160 KiB per CU; the static part of the kernels is < 6 KiB)
    const unsigned lds_max = std::min<unsigned>(kPersistMaxLds, prop.sharedMemPerBlock > 8192 ? (unsigned)prop.sharedMemPerBlock - 6144u : 0u);
    if (persist_lds_bytes(a) > lds_max) a.mat_entries = 0;
    if (persist_lds_bytes(a) > lds_max) { a = PersistArgs{}; return false; }
    DevOwner &own = c->persist_own;
    a.pval = own.upload(pval.data(), pval.size());
    // where every entry of pval came from (bicg_update_values): positions in the block the plan was made from; a reordered
    // context's are turned into positions in the caller's block, entry for entry in stored order
    if (c->reordered) {
        const uint32_t nnz_d = diag->ptr[nrows];
        std::vector<uint32_t> old_of(nnz_d ? nnz_d : 1);
        parallel_ranges(nrows, 4096, [&](size_t ra, size_t rb, int) {
            for (size_t r = ra; r < rb; ++r)
                for (uint32_t j = diag->ptr[r], k = 0; j < diag->ptr[r + 1]; ++j, ++k) old_of[j] = c->ro_src_ptr_host[c->ro_perm_host[r]] + k;
        });
        for (uint32_t &s : P.psrc) if (s != kPersistNoSource && s < nnz_d) s = old_of[s];
    }
    c->persist_psrc = own.upload(P.psrc.data(), P.psrc.size());
    c->persist_entries = pbase[nslices];
    a.pslot = own.upload(pslot.data(), pslot.size());
    a.pbase = own.upload(pbase.data(), pbase.size());
    a.rlen = own.upload(rlen.data(), rlen.size());
    a.rdiag = own.upload(rdiag.data(), rdiag.size());
    a.win_ptr = own.upload(wptr.data(), wptr.size());
    a.win_runs = own.upload(runs.data(), runs.size());
    for (int i = 0; i < 4; ++i) {
        a.llv[i] = own.alloc<llword>(2 * (size_t)nrows);
        BICG_HIP(hipMemset(a.llv[i], 0, sizeof(llword) * 2 * (size_t)nrows));
    }
    for (int i = 0; i < 2; ++i) {
        a.dtab[i] = own.alloc<llword>((size_t)nwg * kRedSlots * 2);
        BICG_HIP(hipMemset(a.dtab[i], 0, sizeof(llword) * (size_t)nwg * kRedSlots * 2));
        a.arow[i] = own.alloc<llword>(8);
        BICG_HIP(hipMemset(a.arow[i], 0, sizeof(llword) * 8));
        a.crow[i] = own.alloc<llword>(6 * kPersistMaxShifts * 2);      // shifted kernel: per-shift coefficients
        BICG_HIP(hipMemset(a.crow[i], 0, sizeof(llword) * 6 * kPersistMaxShifts * 2));
    }
    a.multi = multi ? 1 : 0;
    if (multi) {
        // send-list entries by owning workgroup (the list is grouped by destination, a row may go to several ranks)
        std::vector<uint32_t> sptr(nwg + 1, 0u);
        for (uint32_t i = 0; i < c->nsend; ++i) sptr[send_idx[i] / grows + 1]++;
        for (uint32_t g = 0; g < nwg; ++g) sptr[g + 1] += sptr[g];
        std::vector<uint32_t> fill(sptr.begin(), sptr.end() - 1);
        std::vector<unsigned short> srow(c->nsend ? c->nsend : 1);
        std::vector<unsigned long long> sd0(c->nsend ? c->nsend : 1), sst(c->nsend ? c->nsend : 1);
        for (uint32_t i = 0; i < c->nsend; ++i) {
            const uint32_t g = send_idx[i] / grows, at = fill[g]++;
            srow[at] = (unsigned short)(send_idx[i] - g * grows); sd0[at] = dst0[i]; sst[at] = dstride[i];
        }
        a.snd_ptr = own.upload(sptr.data(), sptr.size());
        a.snd_row = own.upload(srow.data(), srow.size());
        a.snd_dst0 = own.upload(sd0.data(), sd0.size());
        a.snd_stride = own.upload(sst.data(), sst.size());
        a.ring = c->halo_ring; a.halo = c->halo;
    }
    a.v = c->v;
    a.alarm = c->alarm;
    if (getenv("BICG_DEBUG"))
        fprintf(stderr, "bicgstab_hip: rank %d: persistent plan: %u workgroups x (%u + 64) threads x %u rows (+1 helper), window %u slots (%u runs at most), "
                        "matrix %s (%u entries per workgroup), %u bytes of LDS\n", c->rank, nwg, 64 * P.nrw, P.rpt, slots_used, max_runs,
                a.mat_entries ? "in LDS" : "in memory", max_entries, persist_lds_bytes(a));
    return true;
}


// vectors, reduction scratch and scalar blocks of a context whose plan (n_loc, halo, nblk) is known
static void ctx_state(bicg_ctx *c, Comm *comm, uint32_t ngroups)
{
    // ---- vectors: 12 x (rows + halo), each 256-byte aligned; order x r | rh p s y z w v t ax b
    c->stride = ((c->n_loc + c->halo + 31u) / 32u) * 32u;
    // (BICG_STRIDE_PAD = doubles added to the distance between two vectors, a multiple of 32: measurement knob for grids whose
    // vectors would otherwise lie a power of two bytes apart -- 512^3: exactly 1 GiB)
    if (const char *sv = knob_x("BICG_STRIDE_PAD")) c->stride += ((uint32_t)std::max(0, atoi(sv)) / 32u) * 32u;
    c->slab = c->own.alloc<double>(12 * (size_t)c->stride);
    BICG_HIP(hipMemset(c->slab, 0, sizeof(double) * 12 * (size_t)c->stride));
    double *base = c->slab;
    double **slots[12] = {&c->v.x, &c->v.r, &c->v.rh, &c->v.p, &c->v.s, &c->v.y, &c->v.z, &c->v.w, &c->v.v, &c->v.t, &c->v.ax, &c->v.b};
    for (int i = 0; i < 12; ++i) *slots[i] = base + (size_t)i * c->stride;
    c->v.n = c->n_loc;

    c->dots.init(c, std::max<unsigned>(ngroups + c->nblk, kMaxGrid) + 64);      // the dot groups' memory, events and the two scalar blocks
    c->alarm = c->own.alloc<int>(1);
    BICG_HIP(hipMemset(c->alarm, 0, sizeof(int)));
    c->refresh_flag = c->own.alloc<int>(1);
    BICG_HIP(hipMemset(c->refresh_flag, 0, sizeof(int)));
    BICG_HIP(hipHostMalloc((void **)&c->h_alarm, sizeof(int), hipHostMallocDefault));
    *c->h_alarm = 0;
    if (comm->ranks_on_device > 1) {
        // one-GPU box standing in for a node: 1024 = 256 CUs x 4 resident workgroups of the largest kernels
        c->wg_cap = 1024u / (unsigned)(comm->ranks_on_device + 1);
        set_vec_grid_cap(c->wg_cap);
    }
}

static void ctx_streams(bicg_ctx *c, int P)
{
    BICG_HIP(hipStreamCreateWithFlags(&c->sc, hipStreamNonBlocking));
    if (P > 1 || c->force_comm) BICG_HIP(hipStreamCreateWithFlags(&c->sm, hipStreamNonBlocking));
    for (int i = 0; i < kEvRing; ++i) {
        BICG_HIP(hipEventCreateWithFlags(&c->ev_pack[i], hipEventDisableTiming));
        BICG_HIP(hipEventCreateWithFlags(&c->ev_halo[i], hipEventDisableTiming));
    }
    BICG_HIP(hipDeviceSynchronize());       // uploads and memsets above used the null stream
}

// =====================================================================================  C ABI
extern "C" {

int bicg_has_experiments(void) { return kExperiments ? 1 : 0; }
int bicg_switch_unknown(const char *set, char *out, int cap) { return set ? knob_unknown(set, out, cap > 0 ? (size_t)cap : 0) : 0; }
// once per process, from bicg_create: a token none of the lists knows is reported, not obeyed
static void warn_unknown_switches()
{
    static bool done = false;
    if (done) return;
    done = true;
    for (const char *set : {"BICG_PLAN", "BICG_PERSIST", "BICG_TEST"}) {
        char first[64];
        const int n = knob_unknown(set, first, sizeof first);
        if (n) fprintf(stderr, "bicgstab_hip: %s has %d token%s this library does not know (first: \"%s\"); see INTEGRATION.md section 6\n", set, n, n == 1 ? "" : "s", first);
    }
}
int bicg_switch_value(const char *set, const char *name, char *out, int cap)
{
    const char *v = set && name ? knob_tok(set, name) : nullptr;
    if (!v) return -1;
    if (out && cap > 0) { strncpy(out, v, (size_t)cap - 1); out[cap - 1] = 0; }
    return (int)strlen(v);
}
const char *bicg_version(void) { return "bicgstab_hip 0.1 (gfx950)"; }

void bicg_default_options(bicg_options *o)
{
    memset(o, 0, sizeof *o);
    o->tol = 1.0e-15;      // reference EPS       (src/solver.c:3)
    o->max_iter = 1000;    // reference MAX_ITER  (src/solver.c:4)
    o->out_iter = 100;     // reference OUT_ITER  (src/solver.c:9)
    o->check_every = 16;
}

// the code objects this context launches from, loaded now (preload_kernels, bicg_spmv_sell.hip)
static void preload_for(bicg_ctx *c)
{
    if (knob_x("BICG_PRELOAD") && atoi(knob_x("BICG_PRELOAD")) == 0) return;
    preload_kernels(c->sell, c->sell_entries > 0);
    if (c->persist_on) preload_persist_kernels();
    if (c->sell.st.on) preload_stencil_kernels();
    if (c->sell.lane_info && c->jagw_fast) preload_jagw_kernels();
}

// switches both constructors read into the context
static void ctx_read_switches(bicg_ctx *c)
{
    if (const char *sv = knob_x("BICG_SELL_NT")) c->sell_nt_env = atoi(sv);
    if (const char *sv = knob_x("BICG_SELL_ALT")) c->sell_alt = atoi(sv);
    if (const char *sv = knob_x("BICG_SELL_XCD")) c->sell_xcd = atoi(sv);
    if (const char *sv = test_tok("force-comm")) c->force_comm = atoi(sv) != 0;
    if (const char *sv = plan_tok("reorder")) c->reorder_mode = atoi(sv);
    c->dots.handover = !plan_off("handover");
}

// what the halo plan leaves on the host for the later stages (uploads, the persistent plan, the transport)
namespace {
struct HaloHost {
    std::vector<uint32_t> ocol, optr, send_idx;
    std::vector<double> oval;
    std::vector<unsigned long long> dst0, dstride;      // p2p_transport: where every entry of the send list lands, and its slot size
};
}  // namespace

// The common tail of both constructors: vectors and scalar blocks, the form of the pipelined iteration, what every rank must
// agree on, the persistent plan (host: the blocks bicg_create was given; null: none), streams, code objects.
static void ctx_finish(bicg_ctx *c, Comm *comm, uint32_t ngroups, const CSR_Matrix *diag, const HaloHost *host, PlanTrace &trace)
{
    ctx_state(c, comm, ngroups);
    if (const char *sv = test_tok("spin-ticks")) c->dots.spin_ticks = strtoull(sv, nullptr, 10);
    // Round 4: with the products alternating direction and reading no column index in uniform slices, a big block is faster
    // as two plain products + two element-wise kernels (Transport-shaped, one GPU: 139.0 vs 152.0 us per pipelined iteration;
    // profiles/NOTES.md): the fused two-launch form stays what it was built for -- the latency-bound ranks.
    c->fuse_pipe = c->fuse_small;
    if (const char *sv = plan_tok("fuse-pipe")) c->fuse_pipe = atoi(sv) != 0;
    else if (const char *pv = plan_tok("pipe-probe")) c->pipe_probe = atoi(pv);
    c->spmm_ok = all_ranks(comm, spmm_possible(c));
    c->fuse_plan_ok = all_ranks(comm, c->glist_all && c->nblk == 0 && (c->single() || (c->p2p && c->ll_fused)));
    BICG_HIP(hipHostMalloc((void **)&c->hS, sizeof(Scal), hipHostMallocDefault));
    memset(c->hS, 0, sizeof(Scal));
    if (host) {   // persistent pipelined iteration for latency-bound ranks: available when the plan fits on EVERY rank
        const bool off = knob_tok("BICG_PERSIST", "0") || knob_tok("BICG_PERSIST", "off");
        bool mine = !off && persist_build(c, diag, host->optr, host->ocol, host->oval, host->send_idx, host->dst0, host->dstride);
        c->persist_on = all_ranks(comm, mine);
        if (const char *pp = knob_x("BICG_PERSIST_PLAIN")) c->persist_plain = atoi(pp) != 0;
        if (!c->persist_on && mine) { c->persist_own.clear(); c->persist = PersistArgs{}; }
        if (!c->persist_on) { c->persist_psrc = nullptr; c->persist_entries = 0; }
    }
    trace.mark("transport, persistent plan");
    ctx_streams(c, c->nranks);
    trace.mark("streams");
    preload_for(c);
    trace.mark("code objects");
}

// Every rank learns every rank's (non-zeros, rows). The enqueue mode changes the ORDER of RCCL calls,
// so all ranks must take the same decision: it is based on the average number of local non-zeros.
// (a rank without rows carries a phantom row and counts as a rank like any other; only an EMPTY MATRIX is refused: false)
static bool shared_facts(bicg_ctx *c, Comm *comm, const INFO_Matrix *info, PlanFacts &facts)
{
    const int P = c->nranks;
    uint64_t total = c->nnz_d;
    bool empty = c->n_loc == 0;
    if (P > 1) {
        std::vector<int> cnt(P, 2 * (int)sizeof(uint32_t)), off(P);
        std::vector<uint32_t> mine(2 * (size_t)P), all(2 * (size_t)P, 0u);
        for (int p = 0; p < P; ++p) { off[p] = 2 * p * (int)sizeof(uint32_t); mine[2 * p] = c->nnz_d; mine[2 * p + 1] = c->n_loc; }
        comm->alltoallv_host(mine.data(), cnt.data(), off.data(), all.data(), cnt.data(), off.data());
        all[2 * c->rank] = c->nnz_d; all[2 * c->rank + 1] = c->n_loc;
        total = 0;
        for (int p = 0; p < P; ++p) { total += all[2 * p]; empty = empty || all[2 * p + 1] == 0; }
    }
    if (empty) {
        if (c->rank == 0) fprintf(stderr, "ERROR: bicg_create: empty matrix (%u rows over %d ranks)\n", info->rows, P);
        return false;
    }
    c->overlap = total / (uint64_t)P >= 6000000u;
    // two launches per pipelined iteration (phases in the SpMV epilogues): latency on small ranks (200 k rows 26.2
    // vs 34.1 us), the traffic of v and t on large ones (1.6 M rows 159 vs 163 us, banded b = 8 158 vs 169, the
    // 16.8 M-row Laplacian share 1.14 vs 1.25 ms) -- except with x windows, whose epilogue kernels at 4 waves per
    // SIMD lose on large blocks (FEM-like 189 vs 175 us). Like the enqueue mode this changes the sequence of
    // exchanges, so it is decided from facts all ranks share (see fuse_plan_ok), never from the local block alone.
    c->fuse_small = total / (uint64_t)P < 6000000u;
    facts.P = P; facts.rows_global = info->rows; facts.nnz_diag_all = total; facts.fuse_small = c->fuse_small;
    return true;
}

// ---- halo plan (multi rank): which of x's remote entries this rank needs, who needs ours
static void halo_plan(bicg_ctx *c, Comm *comm, const CSR_Matrix *offd, const INFO_Matrix *info, HaloHost &h)
{
    const int P = c->nranks;
    h.optr.assign(c->n_loc + 1, 0u);
    c->scnt.assign(P, 0); c->sdsp.assign(P, 0); c->rcnt.assign(P, 0); c->rdsp.assign(P, 0);
    if (P == 1) return;
    if (offd->rows != c->n_loc) die("bicg_create", "offd block row count differs from diag block");
    c->nnz_o = offd->ptr[offd->rows];
    std::vector<uint32_t> halo_cols(c->nnz_o ? c->nnz_o : 1);
    h.ocol.resize(c->nnz_o ? c->nnz_o : 1);
    c->halo = (uint32_t)bicg_halo_plan(offd, info, P, c->n_loc, halo_cols.data(), c->rcnt.data(), h.ocol.data());
    h.optr.assign(offd->ptr, offd->ptr + c->n_loc + 1);
    h.oval.assign(offd->val, offd->val + c->nnz_o);
    for (int p = 1; p < P; ++p) c->rdsp[p] = c->rdsp[p - 1] + c->rcnt[p - 1];
    // tell every owner which of its rows we need; learn which of ours the others need
    auto tramp = [](const void *sbuf, const int *sc, const int *sd, void *rbuf, const int *rc, const int *rd, void *user) {
        static_cast<Comm *>(user)->alltoallv_host(sbuf, sc, sd, rbuf, rc, rd);
    };
    const int total = bicg_halo_send_counts(P, c->rcnt.data(), tramp, comm, c->scnt.data());
    h.send_idx.resize(total > 0 ? total : 1);
    const int got = bicg_halo_send_lists(c->rank, P, info, c->n_loc, halo_cols.data(), c->rcnt.data(), c->scnt.data(),
                                         tramp, comm, h.send_idx.data());
    if (got < 0) die("bicg_create", "halo request outside the owner's rows");
    c->nsend = (uint32_t)got;
    for (int p = 1; p < P; ++p) c->sdsp[p] = c->sdsp[p - 1] + c->scnt[p - 1];
}

// BICG_PLAN="reorder=1|2" (DESIGN.md section 4.14b): the diag block renumbered by reverse Cuthill-McKee (bicg_reorder.cpp) before it is
// planned, so that the kernels see a matrix they are already good at. Returns the block to plan and upload: the permuted one,
// kept in the context's host vectors until bicg_create returns, or `diag` itself where the reordering is declined or -- mode 2 --
// not worth it. `plan` holds the plan of the returned block when *planned comes back true.
//   mode 1  always reorder
//   mode 2  plan the block as given first; reorder only when that plan is jagged and ends without an x window, and keep the
//           reordered plan only if it gains a window or 16-bit column offsets (stencil, banded and generator-order inputs are never
//           touched)
// One rank only, a decision: with contiguous row blocks a badly numbered matrix on P ranks keeps (P - 1) / P of its entries in the
// offd block, where renumbering the diag block changes nothing.
static const CSR_Matrix *reorder_block(bicg_ctx *c, const CSR_Matrix *diag, const uint32_t *optr, const PlanFacts &facts, const PlanSwitches &sw,
                                       CSR_Matrix &ro, SellPlan &plan, bool *planned, PlanTrace &trace)
{
    *planned = false;
    if (c->reorder_mode != 1 && c->reorder_mode != 2) return diag;
    if (c->nranks > 1 || c->phantom) {
        if (c->rank == 0)
            fprintf(stderr, "bicgstab_hip: BICG_PLAN reorder=%d not taken (%s)\n", c->reorder_mode,
                    c->nranks > 1 ? "one rank only: across ranks most entries of a badly numbered matrix are in the offd blocks" : "a rank without rows");
        return diag;
    }
    if (c->reorder_mode == 2) {
        if (!sell_plan_host(diag, optr, facts, sw, plan, &trace)) die("bicg_create", "internal: sorted slices do not add up");
        *planned = true;
        if (!(plan.jag && !plan.win)) return diag;          // the given numbering is not the problem
    }
    const double t0 = now_sec();
    const uint32_t n = diag->rows;
    std::vector<uint32_t> perm(n), inv(n);
    unsigned long long stats[8];
    reorder_rcm(diag, perm.data(), stats);
    c->ro_ptr.resize((size_t)n + 1); c->ro_col.resize(std::max<uint32_t>(c->nnz_d, 1u)); c->ro_val.resize(std::max<uint32_t>(c->nnz_d, 1u));
    if (!permute_block(diag, perm.data(), c->ro_ptr.data(), c->ro_col.data(), c->ro_val.data(), inv.data())) die("bicg_create", "internal: the reordering is not a permutation");
    stats[7] = (unsigned long long)(1.0e6 * (now_sec() - t0));
    trace.mark("reorder");
    ro = *diag;
    ro.ptr = c->ro_ptr.data(); ro.col = c->ro_col.data(); ro.val = c->ro_val.data();
    if (c->reorder_mode == 2) {
        SellPlan again;
        if (!sell_plan_host(&ro, optr, facts, sw, again, &trace)) die("bicg_create", "internal: sorted slices do not add up");
        if (!(again.win || (again.c16 && !plan.c16))) return diag;      // nothing gained: the first plan stands
        plan = std::move(again);
    }
    c->reordered = true;
    memcpy(c->ro_stats, stats, sizeof stats);
    c->ro_perm = c->own.upload(perm.data(), perm.size());
    c->ro_inv = c->own.upload(inv.data(), inv.size());
    c->ro_src_ptr = c->own.upload(diag->ptr, (size_t)n + 1);
    c->ro_src_ptr_host.assign(diag->ptr, diag->ptr + n + 1);
    c->ro_perm_host = std::move(perm);
    return &ro;
}

// The only place that turns the plan of the diag block (sell_plan_host, bicg_sell_plan.cpp) into device memory, and the one
// place that adds up the bytes of the matrix.
// Only what some kernel reads goes to the GPU: the CSR val/col arrays when there are row blocks for the
// CSR kernel (none for banded matrices: everything is on the sliced-ELL path), the 32-bit sliced-ELL
// columns when the 16-bit offsets do not apply. (Round 1 kept all of them: 2.3 x the matrix.)
// (The offd block and the send list of the halo plan go up from here too, where they always have: the order of the allocations,
// and with it every device address, is the same from build to build, so timings of two builds stay comparable.)
static void sell_plan_upload(bicg_ctx *c, const CSR_Matrix *diag, const SellPlan &p, const PlanSwitches &sw, const HaloHost &h)
{
    const uint32_t nrows = p.nrows, nslices = p.nslices;
    const uint64_t sell_entries = p.sell_entries;
    const bool c16 = p.c16, csr16 = p.csr16;
    DevOwner &own = c->own;
    SellDev &d = c->sell;
    c->rowsplit = p.rowsplit; c->fw = p.fw;
    c->sell_entries = sell_entries; c->sell_nnz = p.sell_nnz; c->sell_rows = p.sell_rows;
    d.jag = p.jag && sell_entries > 0 ? 1 : 0;
    c->uniform_entries = p.uniform_entries; c->constant_entries = p.constant_entries; c->masked_rows = p.masked_rows;
    c->n_int = (uint32_t)p.bint.size(); c->n_bnd = (uint32_t)p.bbnd.size();
    c->nblk = c->n_int + c->n_bnd;
    c->ng_int = (uint32_t)p.gl_int.size(); c->ng_bnd = (uint32_t)p.gl_bnd.size();
    c->glist_int_identity = c->ng_int == p.ngroups;     // every group, in order: index directly
    c->glist_all = c->ng_int + c->ng_bnd == p.ngroups;
    const bool need_csr = c->nblk > 0;
    c->diag.val = own.upload_padded(diag->val, need_csr ? c->nnz_d : 0, kPadEntries);
    c->diag.col = own.upload_padded(diag->col, need_csr && !csr16 ? c->nnz_d : 0, kPadEntries);
    if (csr16) c->d_col16 = own.upload(p.dcol16.data(), p.dcol16.size());
    c->diag.ptr = own.upload(diag->ptr, (size_t)c->n_loc + 1);
    c->offd.val = own.upload(h.oval.data(), c->nnz_o);
    c->offd.col = own.upload(h.ocol.data(), c->nnz_o);
    c->offd.ptr = own.upload(h.optr.data(), (size_t)c->n_loc + 1);
    c->desc_int = own.upload(p.bint.data(), p.bint.size());
    c->desc_bnd = own.upload(p.bbnd.data(), p.bbnd.size());
    // (jagged slices: lanes whose row has ended read up to one entry past the last -- kPadEntries of slack)
    d.val = own.upload_padded(p.sval.get(), (size_t)sell_entries, kPadEntries);
    d.col = own.upload_padded(p.scol.get(), c16 ? 0 : (size_t)sell_entries, kPadEntries);
    if (!p.vbase.empty()) {
        d.vbase = own.upload(p.vbase.data(), p.vbase.size());
        d.uval = own.upload(p.uval.data(), p.uval.size());
    }
    if (!p.mbase.empty()) {
        d.mbase = own.upload(p.mbase.data(), p.mbase.size());
        d.rmask = own.upload(p.rmask.data(), p.rmask.size());
    }
    if (!p.ubase.empty()) {
        d.ubase = own.upload(p.ubase.data(), p.ubase.size());
        d.uoff = own.upload(p.uoff.data(), p.uoff.size());
    }
    build_slice_desc(c, nslices, nrows, p.slice_len.data(), p.ubase, p.vbase, p.mbase, p.uoff, p.uval, p.rmask.empty() ? nullptr : p.rmask.data());
    if (c16) {
        d.col16 = own.upload_padded(p.scol16.get(), p.n16_alloc(), kPadEntries);
        d.slice_base16 = own.upload(p.slice_base16.data(), p.slice_base16.size());
    }
    if (p.win) {
        d.win_ptr = own.upload(p.win_ptr.data(), p.win_ptr.size());
        d.win_runs = own.upload(p.win_runs.data(), p.win_runs.size());
        d.win_slots = p.win_slots; d.win_max_runs = p.win_max_runs; c->win_near16 = p.win_near16;
        if (p.win_list_mode) {
            d.win_list = own.upload(p.list.data(), p.list.size());
            d.win_lptr = own.upload(p.lptr.data(), p.lptr.size());
            d.win_ltotal = own.upload(p.total.data(), p.total.size());
        }
        if (!p.perm.empty()) d.perm = own.upload(p.perm.data(), p.perm.size());
    }
    if (p.jag && sell_entries > 0) {
        c->jag_tail16_max = p.jag_tail16_max;
        if (!p.lane_info.empty()) d.lane_info = own.upload(p.lane_info.data(), p.lane_info.size());
        if (sw.jagw >= 0) c->jagw_fast = sw.jagw != 0;
    }
    d.slice_base = own.upload(p.slice_base.data(), p.slice_base.size());
    d.slice_len = own.upload(p.slice_len.data(), p.slice_len.size());
    c->glist_int = own.upload(p.gl_int.data(), p.gl_int.size());
    c->glist_bnd = own.upload(p.gl_bnd.data(), p.gl_bnd.size());
    c->send_idx = own.upload(h.send_idx.data(), c->nsend);
    c->sendbuf = own.alloc<double>(c->nsend);

    // ---- bytes. matrix_bytes: what one SpMV streams from the matrix arrays; device_matrix_bytes: what is resident.
    const uint64_t ptr_bytes = 4ull * (nrows + 1);
    const uint64_t list_bytes = p.win && p.win_list_mode ? 4ull * p.list.size() + 8ull * p.lptr.size() : 0ull;
    const uint64_t run_bytes = p.win ? 4ull * p.win_ptr.size() + 8ull * p.win_runs.size() : 0ull;
    const uint64_t lane_bytes = d.lane_info ? 2ull * p.lane_info.size() : 0ull;
    // (16 bytes of descriptor per slice where base + length were counted; the list-driven product reads the list, not the runs)
    const uint64_t streamed = (uint64_t)sell_entries * (c16 ? 10 : 12) - p.uniform_entries * (c16 ? 2 : 4) - p.constant_entries * 8ull + 2ull * p.masked_rows +
                              8ull * nslices + ptr_bytes + (uint64_t)(c->nnz_d - c->sell_nnz) * (csr16 ? 10 : 12) + (uint64_t)c->nnz_o * 12 +
                              (d.sdesc ? 8ull * nslices : 0ull) + list_bytes + (p.win_list_mode ? 0ull : run_bytes) + lane_bytes;
    // (one rank: every product goes through the three-trip kernels, which do not read the row pointers)
    c->matrix_bytes = streamed - (d.lane_info && c->nranks == 1 && streamed > ptr_bytes ? ptr_bytes : 0ull);
    c->device_matrix_bytes = (need_csr ? (csr16 ? 10ull : 12ull) * c->nnz_d : 0ull) + 4ull * (c->n_loc + 1) + 12ull * c->nnz_o + 4ull * (c->n_loc + 1) +
                             8ull * sell_entries + (c16 ? 2ull * p.n16 : 4ull * sell_entries) + 12ull * nslices + list_bytes + run_bytes + lane_bytes;
}

// Across ranks (a z-slab of BASELINE.json configs[3]: 64 planes of 512^2 per GPU) the plane-marching product takes the
// planes without halo entries; the halo-touching planes go through the slice-by-slice kernel behind the exchange. That
// needs the two sets to BE whole planes: every group of a plane with a halo-touching group is halo-touching, and the
// others form one range of planes. (Collective.)
static void stencil_across_ranks(bicg_ctx *c, Comm *comm, const std::vector<uint32_t> &gl_bnd)
{
    StencilDev &st = c->sell.st;
    const uint32_t gpp = (st.on && st.sz % kGroupRows == 0) ? st.sz / kGroupRows : 0u;
    std::vector<char> bnd_plane(st.on ? st.nz : 1u, 0);
    bool ok = gpp > 0 && c->glist_all && c->nblk == 0;
    for (uint32_t g : gl_bnd) if (ok) bnd_plane[(size_t)g / gpp] = 1;
    uint32_t nb = 0, lo = st.nz, hi = 0;
    for (uint32_t z = 0; ok && z < st.nz; ++z) { if (bnd_plane[z]) ++nb; else { lo = std::min(lo, z); hi = std::max(hi, z + 1); } }
    ok = ok && (uint64_t)nb * gpp == gl_bnd.size() && lo < hi;
    for (uint32_t z = lo; ok && z < hi; ++z) ok = !bnd_plane[z];
    ok = all_ranks(comm, ok);       // (every rank takes the same form of the exchange: collective)
    if (ok) { st.z_lo = lo; st.z_hi = hi; c->st_multi = true; }
    if (plan_trace_env() && c->rank == 0)
        fprintf(stderr, "bicgstab_hip: plane-marching product across ranks: %s (planes %u .. %u of %u without halo entries)\n", ok ? "yes" : "no", lo, hi, st.nz);
}

// ---- peer-to-peer transport: publish this rank's halo landing ring, learn where every entry
// of the send list lands in the ring of the rank that needs it (collective), and decide whether the exchange rides inside
// the product's launch
static void p2p_transport(bicg_ctx *c, Comm *comm, const SellPlan &plan, HaloHost &h)
{
    const int P = c->nranks;
    c->p2p = comm->p2p;
    if (const char *sv = test_tok("p2p-fault-after")) c->fault_after = atoi(sv);
    // in-kernel collect needs the HEAVY kernel instantiations (occupancy 5 instead of 8 waves per SIMD,
    // ~3 % per SpMV): worth it unless the local problem is so large that 3 % exceeds the ~10 us per
    // iteration the separate apply kernels cost
    c->dots.inline_apply = c->nnz_d < 40000000u;
    if (const char *sv = knob_x("BICG_P2P_INLINE_APPLY")) c->dots.inline_apply = atoi(sv) != 0;
    if (!(c->p2p && !c->single())) { c->p2p = nullptr; return; }
    c->halo_ring = (llword *)c->p2p->alloc(sizeof(llword) * 2 * (size_t)kHaloRing * c->halo);
    std::vector<void *> rings;
    if (c->p2p->share(c->halo_ring, rings, c->ring_mapped) != 0)
        die("bicg_create", "could not map the halo rings of the other ranks (peer-to-peer transport)");
    // to rank p: where ITS values land in my ring, and my ring's slot size
    std::vector<int> mine(2 * (size_t)P), theirs(2 * (size_t)P, 0), cnt(P, 2 * (int)sizeof(int)), dsp(P);
    for (int p = 0; p < P; ++p) {
        mine[2 * p] = c->rdsp[p]; mine[2 * p + 1] = (int)c->halo;
        dsp[p] = 2 * p * (int)sizeof(int);
    }
    comm->alltoallv_host(mine.data(), cnt.data(), dsp.data(), theirs.data(), cnt.data(), dsp.data());
    h.dst0.assign(c->nsend ? c->nsend : 1, 0ull); h.dstride.assign(c->nsend ? c->nsend : 1, 0ull);
    for (int p = 0; p < P; ++p)
        for (int j = 0; j < c->scnt[p]; ++j) {
            const size_t i = (size_t)c->sdsp[p] + j;
            h.dst0[i] = (unsigned long long)(uintptr_t)rings[p] + 16ull * ((unsigned long long)theirs[2 * p] + j);
            h.dstride[i] = 16ull * (unsigned long long)theirs[2 * p + 1];
        }
    c->push_dst0 = c->own.upload(h.dst0.data(), h.dst0.size());
    c->push_stride = c->own.upload(h.dstride.data(), h.dstride.size());
    c->ll_fused = c->n_bnd == 0 && c->ng_int + c->ng_bnd > 0;
    // Ragged rows (jagged slices): the launch with the exchange inside runs k_spmv_sell's loop over EVERY group, the rank's
    // halo-free groups included; as separate launches -- push, interior, unpack, boundary -- the interior goes through the
    // three-trip products of bicg_jagw.hip. Worth two more launches when the interior is large (measured with two 800 k-row
    // ranks of the RCM-numbered mesh matrix sharing a GPU: profiles/r06/ragged_ranks_fused_or_split.txt); BICG_PLAN="halo-fused=0|1" decides.
    if (c->ll_fused && c->sell.jag && c->sell.lane_info && c->jagw_fast && (uint64_t)c->nnz_d >= 4000000ull) c->ll_fused = false;
    if (const char *sv = plan_tok("halo-fused")) c->ll_fused = c->n_bnd == 0 && c->ng_int + c->ng_bnd > 0 && atoi(sv) != 0;
    if (const char *sv = knob_x("BICG_P2P_FUSED")) c->ll_fused = c->ll_fused && atoi(sv) != 0;
    if (c->ll_fused) {
        std::vector<uint32_t> order(plan.gl_int);
        order.insert(order.end(), plan.gl_bnd.begin(), plan.gl_bnd.end());
        c->glist_ll = c->own.upload(order.data(), order.size());
    }
}

bicg_ctx *bicg_create(const CSR_Matrix *diag, const CSR_Matrix *offd, const INFO_Matrix *info)
{
    Comm *comm = comm_get();
    BICG_HIP(hipSetDevice(comm->device));
    if (comm->rank == 0) warn_unknown_switches();
    if (info->rows != info->cols) { fprintf(stderr, "ERROR: bicg_create: matrix is not square\n"); return nullptr; }

    bicg_ctx *c = new bicg_ctx;
    c->comm = comm; c->device = comm->device; c->nranks = comm->nranks; c->rank = comm->rank;
    g_live.push_back(c);
    // a rank without rows: one phantom row (see bicg_ctx::phantom)
    static double ph_val[1] = {1.0};
    static unsigned ph_col[1] = {0u}, ph_ptr1[2] = {0u, 1u}, ph_ptr0[2] = {0u, 0u};
    CSR_Matrix ph_d, ph_o;
    if (diag->rows == 0 && info->rows > 0 && comm->nranks > 1) {
        c->phantom = true;
        ph_d.val = ph_val; ph_d.col = ph_col; ph_d.ptr = ph_ptr1; ph_d.nz = 1; ph_d.rows = 1; ph_d.cols = 1;
        ph_o.val = ph_val; ph_o.col = ph_col; ph_o.ptr = ph_ptr0; ph_o.nz = 0; ph_o.rows = 1; ph_o.cols = info->cols;
        diag = &ph_d; offd = &ph_o;
    }
    c->n_loc = diag->rows; c->n_glob = info->rows;
    c->nnz_d = diag->rows ? diag->ptr[diag->rows] : 0u;
    ctx_read_switches(c);
    if (const char *sv = getenv("BICG_GRAPH")) c->graph_mode = atoi(sv);

    // ---- facts shared by all ranks (collective)
    PlanFacts facts;
    if (!shared_facts(c, comm, info, facts)) {
        bicg_destroy(c);          // nothing is allocated yet; takes the context out of the registry of live ones
        return nullptr;
    }
    if (const char *sv = getenv("BICG_OVERLAP")) c->overlap = atoi(sv) != 0;
    if (const char *sv = knob_x("BICG_SELL_GPW")) c->sell_gpw = atoi(sv);
    if (const char *sv = knob_x("BICG_SELL_GPW_DOTS")) c->sell_gpw_dots = atoi(sv);

    HaloHost halo;
    halo_plan(c, comm, offd, info, halo);

    // (BICG_PLAN_TRACE=1: seconds per part of the plan on stderr, rank 0)
    const char *tv = plan_trace_env();
    PlanTrace trace(tv && atoi(tv) != 0 && comm->rank == 0);
    trace.mark("state, halo plan");

    // ---- the plan of the diag block (renumbered first where BICG_PLAN="reorder" asks for it), on the host, and its upload
    const PlanSwitches sw = read_plan_switches();
    SellPlan plan;
    CSR_Matrix ro_blk;
    bool planned = false;
    diag = reorder_block(c, diag, halo.optr.data(), facts, sw, ro_blk, plan, &planned, trace);
    if (!planned && !sell_plan_host(diag, halo.optr.data(), facts, sw, plan, &trace)) die("bicg_create", "internal: sorted slices do not add up");
    sell_plan_upload(c, diag, plan, sw, halo);
    if (c->nranks > 1) stencil_across_ranks(c, comm, plan.gl_bnd);
    trace.mark("upload");

    p2p_transport(c, comm, plan, halo);
    ctx_finish(c, comm, plan.ngroups, diag, &halo, trace);
    std::vector<uint32_t>().swap(c->ro_ptr); std::vector<uint32_t>().swap(c->ro_col); std::vector<double>().swap(c->ro_val);
    std::vector<uint32_t>().swap(c->ro_perm_host); std::vector<uint32_t>().swap(c->ro_src_ptr_host);
    return c;
}

// Single rank, the matrix ALREADY in device memory as CSR: the sliced-ELL plan (slice lengths, bases, the column-major
// padded copy, 16-bit column offsets when they fit) is built by kernels (bicg_plan_device.hip) -- no host copy of the
// matrix ever exists. This is what makes BASELINE.json configs[3] at its stated size fit a bench run: the 512^3 Laplacian
// (134 M rows, 938 M non-zeros, 11 GB of CSR) is generated on the GPU (bicg_stencil7_device) and planned in a fraction of
// a second, where the one-thread host plan of bicg_create would take the better part of a minute after a 15 GB transfer.
// Blocks whose rows are too ragged for padded slices (or long enough for the rows-over-lanes kernel) are refused: the
// caller downloads the CSR and takes bicg_create.
bicg_ctx *bicg_create_device_csr(const double *val_d, const unsigned int *col_d, const unsigned int *ptr_d, unsigned int rows,
                                 double *plan_seconds)
{
    Comm *comm = comm_get();
    BICG_HIP(hipSetDevice(comm->device));
    if (comm->nranks != 1) { fprintf(stderr, "ERROR: bicg_create_device_csr: single rank only\n"); return nullptr; }
    warn_unknown_switches();
    if (rows == 0) { fprintf(stderr, "ERROR: bicg_create_device_csr: empty matrix\n"); return nullptr; }
    const double t0 = now_sec();
    unsigned nnz = 0;
    BICG_HIP(hipMemcpy(&nnz, ptr_d + rows, sizeof(unsigned), hipMemcpyDeviceToHost));
    const uint32_t nslices = (rows + kSliceRows - 1) / kSliceRows, ngroups = (rows + kGroupRows - 1) / kGroupRows;
    uint32_t *slen_d = dev_alloc<uint32_t>(nslices);
    int *far_d = dev_alloc<int>(1);
    BICG_HIP(hipMemset(slen_d, 0, sizeof(uint32_t) * nslices));
    BICG_HIP(hipMemset(far_d, 0, sizeof(int)));
    launch_plan_rowstats(ptr_d, col_d, rows, slen_d, far_d, nullptr);
    std::vector<uint32_t> slen(nslices), sbase(nslices), sbase16(nslices);
    int far = 0;
    BICG_HIP(hipMemcpy(slen.data(), slen_d, sizeof(uint32_t) * nslices, hipMemcpyDeviceToHost));
    BICG_HIP(hipMemcpy(&far, far_d, sizeof(int), hipMemcpyDeviceToHost));
    uint64_t entries = 0, n16 = 0, padded_rows = 0;
    uint32_t longest = 0;
    for (uint32_t sl = 0; sl < nslices; ++sl) {
        sbase[sl] = (uint32_t)entries; sbase16[sl] = (uint32_t)n16;
        entries += (uint64_t)slen[sl] * kSliceRows;
        n16 += (uint64_t)((slen[sl] + 3) / 4) * 4 * kSliceRows;
        padded_rows += (uint64_t)slen[sl] * std::min<uint32_t>(kSliceRows, rows - sl * kSliceRows);
        longest = std::max(longest, slen[sl]);
    }
    const bool c16 = !far && n16 < 0xFFFFFF00ull && !plan_off("col16");
    const char *why = nullptr;
    if (entries >= 0xFFFFFF00ull) why = "more than 2^32 sliced-ELL entries";
    else if (padded_rows > (uint64_t)nnz + nnz / 50) why = "ragged rows (jagged slices are planned on the host)";
    else if ((uint64_t)nnz / rows >= 128 && ngroups < 512) why = "long rows (the rows-over-lanes plan is built on the host)";
    else if (longest > std::max<uint64_t>(64, 4 * (uint64_t)nnz / rows)) why = "a row much longer than the average";
    if (why) {
        fprintf(stderr, "bicgstab_hip: bicg_create_device_csr: %s -- use bicg_create\n", why);
        dev_free(slen_d); dev_free(far_d);
        return nullptr;
    }
    bicg_ctx *c = new bicg_ctx;
    c->comm = comm; c->device = comm->device; c->nranks = 1; c->rank = 0;
    g_live.push_back(c);
    c->n_loc = rows; c->n_glob = rows; c->nnz_d = nnz;
    ctx_read_switches(c);
    if (c->force_comm) die("bicg_create_device_csr", "BICG_TEST=force-comm is not supported on this path");
    if (c->reorder_mode) fprintf(stderr, "bicgstab_hip: BICG_PLAN reorder=%d not taken (bicg_create_device_csr plans on the device; the host plan of bicg_create reorders)\n", c->reorder_mode);
    c->overlap = nnz >= 6000000u; c->fuse_small = nnz < 6000000u;
    c->scnt.assign(1, 0); c->sdsp.assign(1, 0); c->rcnt.assign(1, 0); c->rdsp.assign(1, 0);
    c->sell_entries = entries; c->sell_nnz = nnz; c->sell_rows = rows;
    // (what the set-up kernels write is built through these local pointers and published in c->sell when it is complete)
    DevOwner &own = c->own;
    SellDev &d = c->sell;
    double *sval = own.alloc<double>((size_t)entries + kPadEntries);
    BICG_HIP(hipMemset(sval, 0, sizeof(double) * ((size_t)entries + kPadEntries)));
    uint32_t *scol = nullptr;
    short *scol16 = nullptr;
    if (c16) {
        scol16 = own.alloc<short>((size_t)n16 + kPadEntries);
        BICG_HIP(hipMemset(scol16, 0, sizeof(short) * ((size_t)n16 + kPadEntries)));
        d.slice_base16 = own.upload(sbase16.data(), sbase16.size());
        scol = own.alloc<uint32_t>(kPadEntries);
    } else {
        scol = own.alloc<uint32_t>((size_t)entries + kPadEntries);
        BICG_HIP(hipMemset(scol, 0, sizeof(uint32_t) * ((size_t)entries + kPadEntries)));
    }
    d.slice_base = own.upload(sbase.data(), sbase.size());
    d.slice_len = own.adopt(slen_d);
    launch_plan_fill(ptr_d, col_d, val_d, rows, d.slice_base, d.slice_base16, sval, c16 ? nullptr : scol, c16 ? scol16 : nullptr, nullptr);
    d.val = sval; d.col = scol; d.col16 = scol16;
    // uniform slices (SellDev::ubase): found by a kernel, grouped by the hash of their distance lists here; one list per group
    // is fetched from the CSR (a stencil has a few dozen)
    uint64_t uniform_entries = 0, constant_entries = 0;
    uint32_t far_rows = 0;
    if (!plan_off("uniform")) {
        const bool want_constant = !plan_off("constant");
        uint32_t *ubase_d = nullptr, *vbase_d = nullptr, *mbase_d = nullptr;      // (rewritten after launch_plan_verify where hashes collided)
        unsigned long long *uh_d = dev_alloc<unsigned long long>(2 * (size_t)nslices), *vh_d = uh_d + nslices;
        BICG_HIP(hipMemset(uh_d, 0, sizeof(unsigned long long) * 2 * (size_t)nslices));
        launch_plan_uniform(ptr_d, col_d, val_d, rows, uh_d, want_constant ? vh_d : nullptr, nullptr);
        std::vector<unsigned long long> uh(nslices), vh(nslices);
        BICG_HIP(hipMemcpy(uh.data(), uh_d, sizeof(unsigned long long) * nslices, hipMemcpyDeviceToHost));
        BICG_HIP(hipMemcpy(vh.data(), vh_d, sizeof(unsigned long long) * nslices, hipMemcpyDeviceToHost));
        dev_free(uh_d);
        // tests: every hash lands in one of TWO buckets -- slices with different lists collide in their thousands and
        // k_plan_verify has to catch each one (tests/test_full_size.py::test_device_plan_survives_hash_collisions)
        const bool collide = test_tok("plan-collide") != nullptr;
        if (collide) for (uint32_t sl = 0; sl < nslices; ++sl) { if (uh[sl]) uh[sl] = 1ull + (uh[sl] >> 63); if (vh[sl]) vh[sl] = 1ull + (vh[sl] >> 63); }
        std::vector<uint32_t> vbase, mbase;
        std::vector<double> uval, vals;
        std::map<unsigned long long, uint32_t> vlists;
        std::vector<uint32_t> ubase(nslices, 0xFFFFFFFFu);
        std::vector<int> uoff;
        std::map<unsigned long long, uint32_t> lists;
        std::vector<uint32_t> cols;
        for (uint32_t sl = 0; sl < nslices; ++sl) {
            if (!uh[sl]) continue;
            auto it = lists.find(uh[sl]);
            if (it == lists.end()) {
                if (lists.size() >= 4096) continue;                           // not a structured matrix: leave the rest to col / col16
                const uint32_t r0 = sl * kSliceRows, len = slen[sl];
                uint32_t p0 = 0;
                BICG_HIP(hipMemcpy(&p0, ptr_d + r0, sizeof(uint32_t), hipMemcpyDeviceToHost));
                cols.resize(len);
                BICG_HIP(hipMemcpy(cols.data(), col_d + p0, sizeof(uint32_t) * len, hipMemcpyDeviceToHost));
                it = lists.emplace(uh[sl], (uint32_t)uoff.size()).first;
                for (uint32_t k = 0; k < len; ++k) uoff.push_back((int)((int64_t)cols[k] - (int64_t)r0));
                uoff.resize((uoff.size() + 7) / 8 * 8 + 16, 0);
            }
            ubase[sl] = it->second;
            uniform_entries += (uint64_t)slen[sl] * kSliceRows;
            if (!vh[sl]) continue;                                                // constant slice (SellDev::vbase)
            auto vt = vlists.find(vh[sl]);
            if (vt == vlists.end()) {
                if (vlists.size() >= 4096) continue;
                const uint32_t r0 = sl * kSliceRows, len = slen[sl];
                uint32_t p0 = 0;
                BICG_HIP(hipMemcpy(&p0, ptr_d + r0, sizeof(uint32_t), hipMemcpyDeviceToHost));
                vals.resize(len);
                BICG_HIP(hipMemcpy(vals.data(), val_d + p0, sizeof(double) * len, hipMemcpyDeviceToHost));
                vt = vlists.emplace(vh[sl], (uint32_t)uval.size()).first;
                uval.insert(uval.end(), vals.begin(), vals.end());
                uval.resize((uval.size() + 7) / 8 * 8 + 16, 0.0);
            }
            if (vbase.empty()) vbase.assign(nslices, 0xFFFFFFFFu);
            vbase[sl] = vt->second;
            constant_entries += (uint64_t)slen[sl] * kSliceRows;
        }
        for (int d : uoff) far_rows = std::max<uint32_t>(far_rows, (uint32_t)std::abs(d));      // the farthest distance of a uniform slice
        // masked slices (SellDev::mbase): the slices next to a grid face. Found by a kernel (hash of the slice's list of
        // (distance, value) pairs), one representative per hash is fetched and its list rebuilt here, the rows' masks are
        // written by a second pass over the slices that were kept.
        if (want_constant && !plan_off("masked")) {
            unsigned long long *mh_d = dev_alloc<unsigned long long>(nslices);
            BICG_HIP(hipMemset(mh_d, 0, sizeof(unsigned long long) * nslices));
            launch_plan_masked(ptr_d, col_d, val_d, rows, mh_d, nullptr, nullptr, nullptr);
            std::vector<unsigned long long> mh(nslices);
            BICG_HIP(hipMemcpy(mh.data(), mh_d, sizeof(unsigned long long) * nslices, hipMemcpyDeviceToHost));
            dev_free(mh_d);
            if (collide) for (uint32_t sl = 0; sl < nslices; ++sl) if (mh[sl]) mh[sl] = (mh[sl] & 31ull) | (32ull << (mh[sl] >> 63));
            std::map<unsigned long long, std::pair<uint32_t, uint32_t>> mlists;       // hash -> (position in uoff, position in uval)
            std::vector<uint32_t> rp(kSliceRows + 1), rc;
            std::vector<double> rv;
            uint32_t nmasked = 0;
            for (uint32_t sl = 0; sl < nslices; ++sl) {
                if (ubase[sl] != 0xFFFFFFFFu || !mh[sl] || (sl + 1) * kSliceRows > rows) continue;
                const uint32_t ulen = (uint32_t)(mh[sl] & 31ull);
                auto it = mlists.find(mh[sl]);
                if (it == mlists.end()) {
                    if (mlists.size() >= 4096) continue;
                    const uint32_t r0 = sl * kSliceRows;
                    BICG_HIP(hipMemcpy(rp.data(), ptr_d + r0, sizeof(uint32_t) * (kSliceRows + 1), hipMemcpyDeviceToHost));
                    const uint32_t ne = rp[kSliceRows] - rp[0];
                    rc.resize(ne); rv.resize(ne);
                    BICG_HIP(hipMemcpy(rc.data(), col_d + rp[0], sizeof(uint32_t) * ne, hipMemcpyDeviceToHost));
                    BICG_HIP(hipMemcpy(rv.data(), val_d + rp[0], sizeof(double) * ne, hipMemcpyDeviceToHost));
                    std::map<int, double> un;
                    for (uint32_t l = 0; l < kSliceRows; ++l)
                        for (uint32_t j = rp[l]; j < rp[l + 1]; ++j) un.emplace((int)((int64_t)rc[j - rp[0]] - (int64_t)(r0 + l)), rv[j - rp[0]]);
                    if (un.size() != ulen) continue;                              // (cannot happen: the kernel built the same list)
                    it = mlists.emplace(mh[sl], std::make_pair((uint32_t)uoff.size(), (uint32_t)uval.size())).first;
                    for (auto &kv : un) { uoff.push_back(kv.first); uval.push_back(kv.second); far_rows = std::max<uint32_t>(far_rows, (uint32_t)std::abs(kv.first)); }
                    uoff.resize((uoff.size() + 7) / 8 * 8 + 16, 0);
                    uval.resize((uval.size() + 7) / 8 * 8 + 16, 0.0);
                }
                if (mbase.empty()) mbase.assign(nslices, 0xFFFFFFFFu);
                if (vbase.empty()) vbase.assign(nslices, 0xFFFFFFFFu);
                ubase[sl] = it->second.first; vbase[sl] = it->second.second;
                mbase[sl] = (ulen << 26) | nmasked++;
                uniform_entries += (uint64_t)slen[sl] * kSliceRows; constant_entries += (uint64_t)slen[sl] * kSliceRows;
            }
            if (nmasked) {
                mbase_d = own.upload(mbase.data(), mbase.size());
                unsigned short *rmask = own.alloc<unsigned short>((size_t)nmasked * kSliceRows);
                BICG_HIP(hipMemset(rmask, 0, sizeof(unsigned short) * (size_t)nmasked * kSliceRows));
                launch_plan_masked(ptr_d, col_d, val_d, rows, nullptr, mbase_d, rmask, nullptr);
                BICG_HIP(hipDeviceSynchronize());
                d.rmask = rmask;
                c->masked_rows = (uint64_t)nmasked * kSliceRows;
            }
        }
        if (uniform_entries) {
            ubase_d = own.upload(ubase.data(), ubase.size());
            d.uoff = own.upload(uoff.data(), uoff.size());
        }
        if (constant_entries) {
            vbase_d = own.upload(vbase.data(), vbase.size());
            d.uval = own.upload(uval.data(), uval.size());
        }
        // The groups above are keyed by 64-bit hashes: every list-driven slice is now compared with the list it was given
        // (k_plan_verify), and a slice that differs -- a collision -- goes back to its stored columns and values, which
        // launch_plan_fill has written for every slice. (The host plan keys on the full lists and needs no such pass.)
        if (uniform_entries) {
            unsigned char *bad_d = dev_alloc<unsigned char>(nslices);
            BICG_HIP(hipMemset(bad_d, 0, nslices));
            launch_plan_verify(ptr_d, col_d, val_d, rows, slen_d, ubase_d, vbase_d, mbase_d, d.rmask, d.uoff, d.uval, bad_d, nullptr);
            std::vector<unsigned char> bad(nslices);
            BICG_HIP(hipMemcpy(bad.data(), bad_d, nslices, hipMemcpyDeviceToHost));
            dev_free(bad_d);
            uint32_t nbad = 0;
            for (uint32_t sl = 0; sl < nslices; ++sl) {
                if (!bad[sl]) continue;
                ++nbad;
                const uint64_t e = (uint64_t)slen[sl] * kSliceRows;
                uniform_entries -= e;
                if (!vbase.empty() && vbase[sl] != 0xFFFFFFFFu) { constant_entries -= e; vbase[sl] = 0xFFFFFFFFu; }
                if (!mbase.empty() && mbase[sl] != 0xFFFFFFFFu) { c->masked_rows -= kSliceRows; mbase[sl] = 0xFFFFFFFFu; }
                ubase[sl] = 0xFFFFFFFFu;
            }
            c->plan_collisions = nbad;
            if (nbad) {
                BICG_HIP(hipMemcpy(ubase_d, ubase.data(), sizeof(uint32_t) * nslices, hipMemcpyHostToDevice));
                if (vbase_d) BICG_HIP(hipMemcpy(vbase_d, vbase.data(), sizeof(uint32_t) * nslices, hipMemcpyHostToDevice));
                if (mbase_d) BICG_HIP(hipMemcpy(mbase_d, mbase.data(), sizeof(uint32_t) * nslices, hipMemcpyHostToDevice));
                if (plan_trace_env()) fprintf(stderr, "bicgstab_hip: %u list-driven slices did not match their list (hash collision): stored as general slices\n", nbad);
            }
        }
        d.ubase = ubase_d; d.vbase = vbase_d; d.mbase = mbase_d;
        if (constant_entries) build_slice_desc(c, nslices, rows, slen.data(), ubase, vbase, mbase, uoff, uval, nullptr);
    }
    c->uniform_entries = uniform_entries;
    c->constant_entries = constant_entries;
    c->far_rows = far_rows;
    uint32_t *dptr = own.alloc<uint32_t>((size_t)rows + 1);
    BICG_HIP(hipMemcpy(dptr, ptr_d, sizeof(uint32_t) * ((size_t)rows + 1), hipMemcpyDeviceToDevice));
    c->diag = {own.alloc<double>(kPadEntries), own.alloc<uint32_t>(kPadEntries), dptr};
    double *oval = own.alloc<double>(1);
    uint32_t *ocol = own.alloc<uint32_t>(1), *optr = own.alloc<uint32_t>((size_t)rows + 1);
    BICG_HIP(hipMemset(optr, 0, sizeof(uint32_t) * ((size_t)rows + 1)));
    c->offd = {oval, ocol, optr};
    c->desc_int = own.alloc<uint4>(1); c->desc_bnd = own.alloc<uint4>(1);
    c->glist_int = own.alloc<uint32_t>(1); c->glist_bnd = own.alloc<uint32_t>(1);
    c->send_idx = own.alloc<uint32_t>(1); c->sendbuf = own.alloc<double>(1);
    c->ng_int = ngroups; c->ng_bnd = 0; c->n_int = c->n_bnd = c->nblk = 0;
    c->glist_int_identity = true; c->glist_all = true;
    sell_order_for_big_grids(c, ngroups);
    c->matrix_bytes = entries * (c16 ? 10 : 12) - uniform_entries * (c16 ? 2 : 4) - constant_entries * 8ull + 2ull * c->masked_rows + 8ull * nslices + 4ull * ((uint64_t)rows + 1);
    if (d.sdesc) c->matrix_bytes += 8ull * nslices;
    c->device_matrix_bytes = 8ull * ((uint64_t)rows + 1) + 8ull * entries + (c16 ? 2ull * n16 : 4ull * entries) + 12ull * nslices;
    dev_free(far_d);
    PlanTrace quiet;
    ctx_finish(c, comm, ngroups, nullptr, nullptr, quiet);
    if (plan_seconds) *plan_seconds = now_sec() - t0;
    return c;
}

namespace {
// the halo landing ring lives in the transport's shared memory: give it back while the transport exists
void release_p2p(bicg_ctx *c)
{
    if (!c->p2p) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    c->p2p->unmap(c->ring_mapped);
    c->p2p->release(c->halo_ring);
    c->ring_mapped.clear(); c->halo_ring = nullptr; c->p2p = nullptr;
}
}  // namespace

// called by comm_set() before the communicator goes away (bicg_comm.cpp)
extern "C++" {
void bicg::contexts_orphan()
{
    for (bicg_ctx *c : g_live) { release_p2p(c); c->comm = nullptr; }
}
}

void bicg_destroy(bicg_ctx *c)
{
    if (!c) return;
    g_live.erase(std::remove(g_live.begin(), g_live.end(), c), g_live.end());
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    c->own.clear();
    c->persist_own.clear();
    release_p2p(c);
    if (c->hS) (void)hipHostFree(c->hS);
    if (c->h_alarm) (void)hipHostFree(c->h_alarm);
    for (int i = 0; i < kEvRing; ++i) {
        for (hipEvent_t e : {c->ev_pack[i], c->ev_halo[i], c->dots.ev_dots[i], c->dots.ev_red[i]})
            if (e) (void)hipEventDestroy(e);      // a context that failed early in bicg_create has none
    }
    for (auto &e : c->tev) (void)hipEventDestroy(e);
    for (auto &e : c->region_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->cross_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : c->sec_ev) (void)hipEventDestroy(e);
    for (auto &ge : c->graph_exec) if (ge) (void)hipGraphExecDestroy(ge);
    if (c->sc) (void)hipStreamDestroy(c->sc);
    if (c->sm) (void)hipStreamDestroy(c->sm);
    delete c;
}


}  // extern "C"
