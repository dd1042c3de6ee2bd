// bicg_sell_plan.cpp -- the sliced-ELL plan of a rank's diag block, made on the host without a device (struct SellPlan,
// bicg_plan.h): which layout, which groups, x windows, column offsets, the slices themselves, list-driven slices, CSR row
// blocks, lane info. sell_plan_host runs the stages in order; sell_plan_upload (bicg_create.cpp) is the only reader that touches
// the GPU. Nothing here calls the HIP runtime or reads the environment: switches arrive as PlanSwitches, what the ranks share
// as PlanFacts. Every loop handed to parallel_ranges writes its own indices only: the plan does not depend on the thread count.
#include "bicg_plan.h"
#include "bicg_parallel.h"

#include <algorithm>
#include <cstring>
#include <map>

namespace bicg {
namespace {

constexpr uint32_t kSlicesPerGroup = kGroupRows / kSliceRows;

// Long rows: lane = row needs 256 rows per workgroup, so a block of few, long rows (banded, half-bandwidth 512:
// 23 k rows of 1025 entries = 92 workgroups for 256 CUs) starves the GPU. Such a block goes to the rows-over-lanes
// kernel (k_spmv_rows) as a whole: row blocks of <= 8192 non-zeros, a row spread over 8..64 lanes. The row sums
// are then associated differently from mult() (tolerance 1e-13 x sum |a_ij x_j| instead of bit-exact).
// Decided from the GLOBAL shape (mean row length, rows per rank) so that all ranks agree.
bool rows_over_lanes(const PlanFacts &f, const PlanSwitches &sw, bool use_sell)
{
    const uint64_t mean_len = f.rows_global ? f.nnz_diag_all / f.rows_global : 0;     // (INFO_Matrix.nz is not always filled in)
    const uint64_t groups_per_rank = ((uint64_t)f.rows_global / (uint64_t)f.P + kGroupRows - 1) / kGroupRows;
    bool rowsplit = use_sell && (mean_len >= 256 || (mean_len >= 128 && groups_per_rank < 512));
    if (sw.rowsplit >= 0) rowsplit = sw.rowsplit != 0;
    return rowsplit;
}

// Slice lengths, and the layout: jagged is chosen for the whole block when padding would add > 2 % entries.
void choose_layout(const CSR_Matrix *diag, const PlanSwitches &sw, SellPlan &p)
{
    const uint32_t nrows = p.nrows, nslices = p.nslices;
    p.slice_len.assign(nslices, 0u);
    p.slice_base.assign(nslices, 0u);
    for (uint32_t r = 0; r < nrows; ++r)
        p.slice_len[r / kSliceRows] = std::max(p.slice_len[r / kSliceRows], diag->ptr[r + 1] - diag->ptr[r]);
    uint64_t padded_rows = 0;
    for (uint32_t sl = 0; sl < nslices; ++sl)
        padded_rows += (uint64_t)p.slice_len[sl] * std::min<uint32_t>(kSliceRows, nrows - sl * kSliceRows);
    p.jag = padded_rows > (uint64_t)p.nnz_d + p.nnz_d / 50;
    if (sw.layout >= 0) p.jag = sw.layout == 1;
}

bool group_fits(const CSR_Matrix *diag, const SellPlan &p, uint32_t jag_max_row, uint32_t g, uint64_t *stored_out)
{
    const uint32_t nrows = p.nrows;
    const uint32_t r0 = g * kGroupRows, r1 = std::min(nrows, r0 + kGroupRows);
    const uint64_t nnz_g = diag->ptr[r1] - diag->ptr[r0];
    if (p.jag) {
        // a lane walks its row alone: an outlier row would keep its wavefront busy long after the launch's other
        // rows are done, so it goes to the CSR kernel, which spreads one row over a workgroup
        *stored_out = nnz_g;
        for (uint32_t sl = r0 / kSliceRows; sl * kSliceRows < r1; ++sl)
            if (p.slice_len[sl] > jag_max_row) return false;
        return true;
    }
    // storage always covers 64 lanes per slice; the criterion only counts lanes that hold a row, so
    // that the last, partly filled group of a block does not fall to the CSR kernel (an extra
    // launch per SpMV for a few dozen rows)
    uint64_t padded = 0, padded_rows = 0;
    for (uint32_t sl = r0 / kSliceRows; sl * kSliceRows < r1; ++sl) {
        padded += (uint64_t)p.slice_len[sl] * kSliceRows;
        padded_rows += (uint64_t)p.slice_len[sl] * std::min<uint32_t>(kSliceRows, r1 - sl * kSliceRows);
    }
    *stored_out = padded;
    return padded_rows <= nnz_g + nnz_g / 4 + 2 * kSliceRows;
}

// Which groups go to the sliced-ELL kernels in the layout p.jag, where their slices start, and which of them touch the halo.
// (Round 1, before the jagged layout: a ragged matrix left only a few groups under the padding limit; two
// kernels per SpMV were then slower than the CSR kernel alone -- synth.fem_like 70 vs 63 us -- and sorting rows
// by length inside the groups, SELL-C-sigma, removes the padding but also the coalesced x gather: 66.9 us.)
void select_groups(const CSR_Matrix *diag, const uint32_t *optr, int P, bool use_sell, uint32_t jag_max_row, SellPlan &p)
{
    const uint32_t nrows = p.nrows, ngroups = p.ngroups;
    bool sell_worthwhile = use_sell;
    p.sell_entries = 0; p.sell_nnz = 0; p.sell_rows = 0;
    p.gl_int.clear(); p.gl_bnd.clear();
    if (use_sell) {
        uint64_t rows_fit = 0, dummy;
        for (uint32_t g = 0; g < ngroups; ++g)
            if (group_fits(diag, p, jag_max_row, g, &dummy)) rows_fit += std::min(nrows, (g + 1) * (uint32_t)kGroupRows) - g * kGroupRows;
        sell_worthwhile = 2 * rows_fit >= nrows;
    }
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t r0 = g * kGroupRows, r1 = std::min(nrows, r0 + kGroupRows);
        const uint64_t nnz_g = diag->ptr[r1] - diag->ptr[r0];
        uint64_t stored = 0;
        const bool sell = sell_worthwhile && group_fits(diag, p, jag_max_row, g, &stored) && p.sell_entries + stored < 0xFFFFFF00ull;
        p.group_is_sell[g] = sell;
        if (!sell) continue;
        for (uint32_t sl = r0 / kSliceRows; sl * kSliceRows < r1; ++sl) {
            p.slice_base[sl] = (uint32_t)p.sell_entries;
            if (p.jag) p.sell_entries += diag->ptr[std::min(nrows, (sl + 1) * (uint32_t)kSliceRows)] - diag->ptr[sl * kSliceRows];
            else p.sell_entries += (uint64_t)p.slice_len[sl] * kSliceRows;
        }
        p.sell_nnz += nnz_g; p.sell_rows += r1 - r0;
        const bool touches_halo = P > 1 && optr[r1] > optr[r0];
        (touches_halo ? p.gl_bnd : p.gl_int).push_back(g);
    }
}

// x windows of the selected groups: runs of consecutive columns, or -- where those are too many -- the list-driven form.
// False: some group's window does not fit (no windows for this block).
bool plan_windows(const CSR_Matrix *diag, const PlanFacts &f, const PlanSwitches &sw, SellPlan &p)
{
    const uint32_t nrows = p.nrows, ngroups = p.ngroups;
    // per group: the columns its rows touch, merged into runs of consecutive columns (bicg_plan.cpp)
    constexpr uint32_t kWinGap = 8;
    bool ok = p.sell_entries > 0;
    long nruns = ok ? bicg_window_plan(diag->ptr, diag->col, nrows, kGroupRows, p.group_is_sell.data(), kWinMaxSlots, kWinGap,
                                       nullptr, nullptr, nullptr) : -1;
    if (nruns >= 0) {
        p.win_ptr.assign(ngroups + 1, 0u);
        p.win_runs.assign((size_t)nruns + 1, make_uint2(0u, 0u));
        static_assert(sizeof(uint2) == 2 * sizeof(unsigned int), "run = two 32-bit words");
        bicg_window_plan(diag->ptr, diag->col, nrows, kGroupRows, p.group_is_sell.data(), kWinMaxSlots, kWinGap, p.win_ptr.data(),
                         reinterpret_cast<unsigned int *>(p.win_runs.data()), &p.win_slots);
    } else {
        ok = false;
    }
    // The window pays through k_spmv_jagw only (three dependent trips per group, bicg_jagw.hip): at most kJagwMaxRuns runs per
    // group and kJagwMaxSlots slots. A numbering whose groups touch MANY short runs (reverse Cuthill-McKee of a tetrahedral
    // mesh: up to 170 runs, 2 657 slots) would go through k_spmv_sell's window loop, which stages run after run: 169 us per
    // product on the 1.6 M-row mesh matrix against 56.5 us for the same jagged slices with 16-bit offsets gathered through
    // the caches (profiles/r06/mesh_probe_baseline.txt, mesh_probe_plans.txt). Unless BICG_PLAN="window=1" insists, such a
    // block keeps its jagged slices and drops the window.
    if (ok && sw.window != 1) {
        uint32_t most_runs = 0;
        for (uint32_t g = 0; g < ngroups; ++g) most_runs = std::max(most_runs, p.win_ptr[g + 1] - p.win_ptr[g]);
        if (most_runs > kJagwMaxRuns || p.win_slots > kJagwMaxSlots) ok = false;
        // ... unless the group's DISTINCT columns fit the window one by one (no gaps merged): the list-driven window of
        // k_spmv_jagw<.., LIST> (SellDev::win_list). One rank only -- launches with offd entries or the exchange inside go
        // through k_spmv_sell's loop, which would have to stage hundreds of runs -- and not for blocks whose pipelined
        // phases ride in the products' epilogues (the same loop). BICG_PLAN="window-list=0" keeps the gathers.
        if (!ok && f.P == 1 && !f.fuse_small && p.sell_entries > 0 && sw.window_list) {
            long nr = bicg_window_plan(diag->ptr, diag->col, nrows, kGroupRows, p.group_is_sell.data(), kJagwMaxSlots, 0u, nullptr, nullptr, nullptr);
            bool near = nr >= 0;
            for (uint32_t g = 0; near && g < ngroups; ++g) {      // 16-bit list entries: distance from the group's first row
                if (!p.group_is_sell[g]) continue;
                const uint32_t r0 = g * kGroupRows, r1 = std::min(nrows, r0 + kGroupRows);
                for (uint32_t j = diag->ptr[r0]; j < diag->ptr[r1]; ++j) {
                    const long d = (long)diag->col[j] - (long)r0;
                    if (d < -32768 || d > 32767) { near = false; break; }
                }
            }
            if (near) {
                p.win_ptr.assign(ngroups + 1, 0u);
                p.win_runs.assign((size_t)nr + 1, make_uint2(0u, 0u));
                bicg_window_plan(diag->ptr, diag->col, nrows, kGroupRows, p.group_is_sell.data(), kJagwMaxSlots, 0u, p.win_ptr.data(),
                                 reinterpret_cast<unsigned int *>(p.win_runs.data()), &p.win_slots);
                p.win_list_mode = true;
                ok = true;
            }
        }
    }
    return ok;
}

// With windows: deal the rows of every group to the lanes by decreasing length (SellDev::perm). The group's
// entries stay where they are as a whole; the slices inside it change length. False: the sorted slices do not add up.
bool deal_rows_by_length(const CSR_Matrix *diag, SellPlan &p)
{
    const uint32_t nrows = p.nrows, nslices = p.nslices, ngroups = p.ngroups;
    p.perm.assign((size_t)ngroups * kGroupRows, 0);
    std::vector<uint32_t> slice_sum(nslices, 0u);             // entries of a slice after the rows were dealt out
    parallel_ranges(ngroups, 64, [&](size_t ga, size_t gb, int) {
        for (uint32_t g = (uint32_t)ga; g < (uint32_t)gb; ++g) {
            unsigned char *pg = p.perm.data() + (size_t)g * kGroupRows;
            for (uint32_t t = 0; t < kGroupRows; ++t) pg[t] = (unsigned char)t;
            if (!p.group_is_sell[g]) continue;
            const uint32_t r0 = g * kGroupRows;
            auto len_of = [&](unsigned t) -> uint32_t { return r0 + t < nrows ? diag->ptr[r0 + t + 1] - diag->ptr[r0 + t] : 0u; };
            std::stable_sort(pg, pg + kGroupRows, [&](unsigned char x, unsigned char y) { return len_of(x) > len_of(y); });
            for (uint32_t w = 0; w < kSlicesPerGroup; ++w) {
                const uint32_t sl = g * kSlicesPerGroup + w;
                if (sl >= nslices) break;
                uint32_t longest = 0; uint64_t sum = 0;
                for (uint32_t l = 0; l < kSliceRows; ++l) { const uint32_t n = len_of(pg[w * kSliceRows + l]); longest = std::max(longest, n); sum += n; }
                p.slice_len[sl] = longest; slice_sum[sl] = (uint32_t)sum;
            }
        }
    });
    uint64_t at = 0;
    for (uint32_t g = 0; g < ngroups; ++g) {
        if (!p.group_is_sell[g]) continue;
        for (uint32_t sl = g * kSlicesPerGroup; sl < std::min(nslices, (g + 1) * kSlicesPerGroup); ++sl) { p.slice_base[sl] = (uint32_t)at; at += slice_sum[sl]; }
    }
    return at == p.sell_entries;
}

// the row lane `lane` of slice `sl` works on
inline uint32_t row_of(const SellPlan &p, uint32_t sl, uint32_t lane)
{
    if (p.perm.empty()) return sl * kSliceRows + lane;
    const uint32_t g = sl / kSlicesPerGroup, w = sl % kSlicesPerGroup;
    return g * kGroupRows + p.perm[(size_t)g * kGroupRows + w * kSliceRows + lane];
}

// 16-bit column offsets when every sliced-ELL entry is within +-32767 of its row (p.c16, p.slice_base16, p.n16), and the
// fused-window clusters of a padded 16-bit block (p.fw).
void column_offsets_and_clusters(const CSR_Matrix *diag, const PlanSwitches &sw, SellPlan &p)
{
    const uint32_t nrows = p.nrows, nslices = p.nslices;
    p.c16 = p.sell_entries > 0 && (p.win || sw.col16);
    p.slice_base16.assign(nslices, 0u);
    p.n16 = 0;
    if (p.jag) p.n16 = p.sell_entries;
    else
        for (uint32_t sl = 0; sl < nslices; ++sl) {
            p.slice_base16[sl] = (uint32_t)p.n16;
            if (p.group_is_sell[sl / kSlicesPerGroup]) p.n16 += (uint64_t)((p.slice_len[sl] + 3) / 4) * 4 * kSliceRows;
        }
    if (p.n16 >= 0xFFFFFF00ull) p.c16 = false;
    std::vector<int> offsets_seen;          // distinct column offsets (col - row), while they stay few: the fused-window clusters
    bool offsets_few = true;
    if (p.c16 && !p.win) {
        // row ranges on several threads, a map of the offsets seen per thread; merged below (ascending: the order does not matter,
        // the clusters are formed from the sorted list)
        std::vector<std::vector<unsigned char>> marks((size_t)plan_threads());
        std::vector<char> bad((size_t)plan_threads(), 0);
        const int np = parallel_ranges(nrows, 4096, [&](size_t ra, size_t rb, int part) {
            std::vector<unsigned char> &mark = marks[(size_t)part];
            mark.assign(65536, 0);
            for (uint32_t r = (uint32_t)ra; r < (uint32_t)rb && !bad[(size_t)part]; ++r) {
                if (!p.group_is_sell[r / kGroupRows]) continue;
                for (uint32_t j = diag->ptr[r]; j < diag->ptr[r + 1]; ++j) {
                    const int64_t dlt = (int64_t)diag->col[j] - (int64_t)r;
                    if (dlt < -32767 || dlt > 32767) { bad[(size_t)part] = 1; break; }
                    mark[dlt + 32768] = 1;
                }
            }
        });
        for (int q = 0; q < np; ++q) if (bad[(size_t)q]) p.c16 = false;
        for (int d = 0; p.c16 && d < 65536; ++d) {
            bool any = false;
            for (int q = 0; q < np && !any; ++q) any = marks[(size_t)q][(size_t)d] != 0;
            if (!any) continue;
            if (offsets_seen.size() >= 4096) { offsets_few = false; break; }
            offsets_seen.push_back(d - 32768);
        }
    }
    // Fused-window clusters (struct FusedWindow): the offsets fall into <= 4 clusters (gaps of more than 512 columns separate
    // them) and a group's window -- 256 + span columns per cluster -- fits 2048 LDS slots. Padded slices with 16-bit offsets,
    // every row on the sliced-ELL path. (The fused product itself is a one-rank form; the windowed SpMM uses the clusters on every rank.)
    if (p.c16 && !p.jag && !p.win && offsets_few && p.sell_entries > 0) {
        offsets_seen.push_back(0);
        std::sort(offsets_seen.begin(), offsets_seen.end());
        FusedWindow f{};
        int ncl = 0, slots = 0;
        bool ok = true;
        for (size_t i = 0; i < offsets_seen.size() && ok;) {
            size_t k = i;
            while (k + 1 < offsets_seen.size() && offsets_seen[k + 1] - offsets_seen[k] <= 512) ++k;
            if (ncl == kFwMaxClusters) { ok = false; break; }
            f.lo[ncl] = offsets_seen[i]; f.hi[ncl] = offsets_seen[k];
            f.bias[ncl] = slots - f.lo[ncl];
            slots += kGroupRows + f.hi[ncl] - f.lo[ncl];
            ++ncl;
            i = k + 1;
        }
        if (ok && slots <= 2048) { f.ncl = ncl; f.slots = (unsigned)slots; p.fw = f; }
    }
}

// The slices themselves (p.sval, p.scol or p.scol16), on several threads: a slice's entries (and its padding, zeros) are its
// own range of the arrays.
void fill_slices(const CSR_Matrix *diag, SellPlan &p)
{
    const uint32_t nrows = p.nrows, nslices = p.nslices;
    const uint64_t sell_entries = p.sell_entries;
    const bool jag = p.jag, win = p.win, c16 = p.c16;
    p.sval.reset(new double[sell_entries ? sell_entries : 1]);
    p.scol16.reset(new short[p.n16_alloc()]);
    if (!c16) { p.scol16[0] = 0; p.scol.reset(new uint32_t[sell_entries ? sell_entries : 1]); }
    double *const sval = p.sval.get();
    short *const scol16 = p.scol16.get();
    uint32_t *const scol = p.scol.get();
    const std::vector<uint32_t> &slice_base = p.slice_base, &slice_len = p.slice_len, &slice_base16 = p.slice_base16;
    if (sell_entries == 0) { sval[0] = 0.0; if (scol) scol[0] = 0u; }
    auto slot_of = [&](uint32_t g, uint32_t col) -> uint32_t {
        return bicg_window_slot(reinterpret_cast<const unsigned int *>(p.win_runs.data()), p.win_ptr[g], p.win_ptr[g + 1], col);
    };
    parallel_ranges(nslices, 256, [&](size_t sa, size_t sb, int) {
        for (uint32_t sl = (uint32_t)sa; sl < (uint32_t)sb; ++sl) {
            const uint32_t g = sl / kSlicesPerGroup;
            if (!p.group_is_sell[g]) continue;
            if (jag) {
                size_t e = slice_base[sl];
                for (uint32_t k = 0; k < slice_len[sl]; ++k)
                    for (uint32_t lane = 0; lane < kSliceRows; ++lane) {
                        const uint32_t r = row_of(p, sl, lane);
                        if (r >= nrows || diag->ptr[r + 1] - diag->ptr[r] <= k) continue;
                        const uint32_t j = diag->ptr[r] + k;
                        sval[e] = diag->val[j];
                        if (scol) scol[e] = diag->col[j];
                        if (win) scol16[e] = (short)(unsigned short)slot_of(g, diag->col[j]);
                        else if (c16) scol16[e] = (short)((int64_t)diag->col[j] - (int64_t)r);
                        ++e;
                    }
                continue;
            }
            const size_t b0 = slice_base[sl], n = (size_t)slice_len[sl] * kSliceRows;
            std::fill(sval + b0, sval + b0 + n, 0.0);
            if (scol) std::fill(scol + b0, scol + b0 + n, 0u);
            if (c16) std::fill(scol16 + slice_base16[sl], scol16 + slice_base16[sl] + (size_t)((slice_len[sl] + 3) / 4) * 4 * kSliceRows, (short)0);
            for (uint32_t lane = 0; lane < kSliceRows; ++lane) {
                const uint32_t r = sl * kSliceRows + lane;
                if (r >= nrows) break;
                for (uint32_t j = diag->ptr[r], k = 0; j < diag->ptr[r + 1]; ++j, ++k) {
                    const size_t e = b0 + (size_t)k * kSliceRows + lane;
                    sval[e] = diag->val[j];
                    if (scol) scol[e] = diag->col[j];
                    if (c16) scol16[(size_t)slice_base16[sl] + ((size_t)(k / 4) * kSliceRows + lane) * 4 + (k % 4)] =
                                 (short)((int64_t)diag->col[j] - (int64_t)r);
                }
            }
        }
    });
}

// the shared tables of distance lists (p.uoff) and value lists (p.uval), keyed by their full content
struct ListTables {
    std::map<std::vector<int>, uint32_t> lists, vlists;
    // position of `cur` in uoff, appended when new; false: the table is full (it stays small: scalar cache)
    bool distances(SellPlan &p, const std::vector<int> &cur, uint32_t *at)
    {
        auto it = lists.find(cur);
        if (it == lists.end()) {
            if (p.uoff.size() + cur.size() + 32 > (1u << 24)) return false;
            it = lists.emplace(cur, (uint32_t)p.uoff.size()).first;
            p.uoff.insert(p.uoff.end(), cur.begin(), cur.end());
            p.uoff.resize((p.uoff.size() + 7) / 8 * 8 + 16, 0);               // batches of up to 16 entries read past the list
        }
        *at = it->second;
        return true;
    }
    bool values(SellPlan &p, const std::vector<int> &vkey, const double *v, uint32_t len, uint32_t *at)
    {
        auto vt = vlists.find(vkey);
        if (vt == vlists.end()) {
            if (p.uval.size() + len + 32 > (1u << 22)) return false;
            vt = vlists.emplace(vkey, (uint32_t)p.uval.size()).first;
            p.uval.insert(p.uval.end(), v, v + len);
            p.uval.resize((p.uval.size() + 7) / 8 * 8 + 16, 0.0);
        }
        *at = vt->second;
        return true;
    }
};

// masked slice (SellDev::mbase): the rows are sub-sequences of one ascending list of <= 16 (distance, value) pairs
void try_masked_slice(const CSR_Matrix *diag, uint32_t sl, ListTables &tab, SellPlan &p)
{
    const uint32_t r0 = sl * kSliceRows, len = p.slice_len[sl];
    std::map<int, long long> un;                                      // distance -> value bits
    bool ok = true;
    for (uint32_t l = 0; l < kSliceRows && ok; ++l) {
        const uint32_t p0 = diag->ptr[r0 + l], p1 = diag->ptr[r0 + l + 1];
        ok = p1 > p0 && p1 - p0 <= 16u;
        for (uint32_t j = p0; j < p1 && ok; ++j) {
            if (j > p0 && diag->col[j] <= diag->col[j - 1]) { ok = false; break; }      // ascending columns
            const int d = (int)((int64_t)diag->col[j] - (int64_t)(r0 + l));
            long long b; memcpy(&b, diag->val + j, 8);
            auto f = un.find(d);
            if (f == un.end()) un.emplace(d, b); else ok = f->second == b;
        }
        ok = ok && un.size() <= 16u;
    }
    if (!ok) return;
    const uint32_t ulen = (uint32_t)un.size();
    std::vector<int> cur, vkey;
    std::vector<double> uv_list;
    for (auto &kv : un) { cur.push_back(kv.first); double v; memcpy(&v, &kv.second, 8); uv_list.push_back(v); }
    vkey.assign(cur.begin(), cur.end());
    for (auto &kv : un) { vkey.push_back((int)(kv.second & 0xFFFFFFFF)); vkey.push_back((int)(kv.second >> 32)); }
    uint32_t uat, vat;
    if (!tab.distances(p, cur, &uat)) return;
    if (!tab.values(p, vkey, uv_list.data(), ulen, &vat)) return;
    if (p.vbase.empty()) p.vbase.assign(p.nslices, 0xFFFFFFFFu);
    if (p.mbase.empty()) p.mbase.assign(p.nslices, 0xFFFFFFFFu);
    p.ubase[sl] = uat; p.vbase[sl] = vat;
    p.mbase[sl] = (ulen << 26) | (uint32_t)(p.rmask.size() / kSliceRows);
    for (uint32_t l = 0; l < kSliceRows; ++l) {
        unsigned m = 0;
        for (uint32_t j = diag->ptr[r0 + l]; j < diag->ptr[r0 + l + 1]; ++j) {
            const int d = (int)((int64_t)diag->col[j] - (int64_t)(r0 + l));
            m |= 1u << (unsigned)std::distance(un.begin(), un.find(d));
        }
        p.rmask.push_back((unsigned short)m);
    }
    p.uniform_entries += (uint64_t)len * kSliceRows; p.constant_entries += (uint64_t)len * kSliceRows;     // (padded entries the product no longer reads)
    p.masked_rows += kSliceRows;
}

// Uniform slices (SellDev::ubase): all 64 rows present, equally long, entry k at the same distance from its row in
// every row. Lists are shared between slices (a banded matrix has ONE for its whole interior) and padded with zeros.
// Constant slices (SellDev::vbase): entry k also holds the same value in all 64 rows. Padded slices only.
void classify_slices(const CSR_Matrix *diag, const PlanSwitches &sw, SellPlan &p)
{
    const uint32_t nrows = p.nrows, nslices = p.nslices;
    const bool want_constant = sw.constant, want_masked = sw.masked;
    if (p.jag || p.sell_entries == 0 || !sw.uniform) return;
    p.ubase.assign(nslices, 0xFFFFFFFFu);
    ListTables tab;
    std::vector<int> cur, vkey;
    auto candidate = [&](uint32_t sl) { return p.group_is_sell[sl / kSlicesPerGroup] && (sl + 1) * kSliceRows <= nrows && p.slice_len[sl] != 0; };
    // which slices are uniform (1) / uniform and constant (2): 64 rows x length comparisons per slice, on several threads; the
    // lists themselves are numbered by the pass below, in slice order
    std::vector<char> cls(nslices, 0);
    parallel_ranges(nslices, 256, [&](size_t sa, size_t sb, int) {
        for (uint32_t sl = (uint32_t)sa; sl < (uint32_t)sb; ++sl) {
            if (!candidate(sl)) continue;
            const uint32_t r0 = sl * kSliceRows, len = p.slice_len[sl], p0 = diag->ptr[r0];
            bool uni = true;
            for (uint32_t l = 0; l < kSliceRows && uni; ++l) uni = diag->ptr[r0 + l + 1] - diag->ptr[r0 + l] == len;
            for (uint32_t l = 1; l < kSliceRows && uni; ++l)
                for (uint32_t k = 0; k < len; ++k)
                    if ((int64_t)diag->col[diag->ptr[r0 + l] + k] - (int64_t)(r0 + l) != (int64_t)diag->col[p0 + k] - (int64_t)r0) { uni = false; break; }
            if (!uni) continue;
            bool con = want_constant;
            for (uint32_t l = 1; l < kSliceRows && con; ++l) con = memcmp(diag->val + diag->ptr[r0 + l], diag->val + p0, sizeof(double) * len) == 0;
            cls[sl] = con ? 2 : 1;
        }
    });
    for (uint32_t sl = 0; sl < nslices; ++sl) {
        if (!candidate(sl)) continue;
        const uint32_t r0 = sl * kSliceRows, len = p.slice_len[sl];
        if (cls[sl] == 0) {
            if (want_constant && want_masked) try_masked_slice(diag, sl, tab, p);
            continue;
        }
        cur.assign(len, 0);
        for (uint32_t k = 0; k < len; ++k) cur[k] = (int)((int64_t)diag->col[diag->ptr[r0] + k] - (int64_t)r0);
        if (!tab.distances(p, cur, &p.ubase[sl])) { p.ubase[sl] = 0xFFFFFFFFu; continue; }
        p.uniform_entries += (uint64_t)len * kSliceRows;
        // constant slice: entry k holds the same value in all 64 rows (SellDev::vbase)
        if (!want_constant) continue;
        const double *v0 = diag->val + diag->ptr[r0];
        if (cls[sl] != 2) continue;
        vkey.assign(cur.begin(), cur.end());                                  // distances, then the value bits
        for (uint32_t k = 0; k < len; ++k) { long long b; memcpy(&b, v0 + k, 8); vkey.push_back((int)(b & 0xFFFFFFFF)); vkey.push_back((int)(b >> 32)); }
        uint32_t vat;
        if (!tab.values(p, vkey, v0, len, &vat)) continue;
        if (p.vbase.empty()) p.vbase.assign(nslices, 0xFFFFFFFFu);
        p.vbase[sl] = vat;
        p.constant_entries += (uint64_t)len * kSliceRows;
    }
    if (p.uniform_entries == 0) { p.ubase.clear(); p.uoff.clear(); }
}

// CSR row blocks over the maximal runs of non-SELL groups
void plan_row_blocks(const CSR_Matrix *diag, const uint32_t *optr, int P, SellPlan &p)
{
    const uint32_t nrows = p.nrows, ngroups = p.ngroups;
    std::vector<uint32_t> rb(nrows + 1);
    for (uint32_t g = 0; g < ngroups;) {
        if (p.group_is_sell[g]) { ++g; continue; }
        uint32_t g1 = g;
        while (g1 < ngroups && !p.group_is_sell[g1]) ++g1;
        const uint32_t r0 = g * kGroupRows, r1 = std::min(nrows, g1 * kGroupRows);
        // bicg_row_blocks works on a ptr array that starts at the run's first row
        const uint32_t nb = p.rowsplit ? bicg_row_blocks(diag->ptr + r0, r1 - r0, 8192, 256, rb.data())
                                       : bicg_row_blocks(diag->ptr + r0, r1 - r0, kRowBlockNnz, 1024, rb.data());
        for (uint32_t b = 0; b < nb; ++b) {
            const uint32_t a0 = r0 + rb[b], a1 = r0 + rb[b + 1];
            const bool touches_halo = P > 1 && optr[a1] > optr[a0];
            (touches_halo ? p.bbnd : p.bint).push_back(make_uint4(a0, a1, diag->ptr[a0], diag->ptr[a1]));
        }
        g = g1;
    }
}

// rows-over-lanes kernel: 16-bit column offsets in CSR order when every entry fits
void plan_csr16(const CSR_Matrix *diag, const PlanSwitches &sw, SellPlan &p)
{
    p.csr16 = p.rowsplit && p.nblk() > 0 && sw.col16;
    if (!p.csr16) return;
    p.dcol16.resize((size_t)p.nnz_d + kPadEntries, 0);
    for (uint32_t r = 0; p.csr16 && r < p.nrows; ++r)
        for (uint32_t j = diag->ptr[r]; j < diag->ptr[r + 1]; ++j) {
            const int64_t dlt = (int64_t)diag->col[j] - (int64_t)r;
            if (dlt < -32767 || dlt > 32767) { p.csr16 = false; break; }
            p.dcol16[j] = (short)dlt;
        }
    if (!p.csr16) { p.dcol16.clear(); p.dcol16.shrink_to_fit(); }
}

// What the kernels want to know about the windows as a whole, and the list-driven window's list.
void finish_windows(SellPlan &p)
{
    const uint32_t ngroups = p.ngroups;
    const std::vector<uint32_t> &win_ptr = p.win_ptr;
    const std::vector<uint2> &win_runs = p.win_runs;
    for (uint32_t g = 0; g < ngroups; ++g) p.win_max_runs = std::max(p.win_max_runs, win_ptr[g + 1] - win_ptr[g]);
    p.win_near16 = true;
    for (uint32_t g = 0; g < ngroups && p.win_near16; ++g)
        for (uint32_t r = win_ptr[g]; r < win_ptr[g + 1]; ++r) {
            const long lo = (long)win_runs[r].x - (long)(g * kGroupRows), hi = lo + (long)(win_runs[r].y & 0xFFFFu) - 1;
            if (lo < -32767 || hi > 32767) { p.win_near16 = false; break; }
        }
    if (!p.win_list_mode) return;
    // the runs spelled out, 16 bits per column (distance from the group's first row), two slots per word: word j of thread t
    // (at lptr[g] + 256 j + t) holds slots t + 512 j (low half) and t + 512 j + 256 -- the slots thread t stages
    std::vector<uint32_t> &lptr = p.lptr, &total = p.total, &list = p.list;
    lptr.assign(ngroups + 1, 0u);
    total.assign(ngroups, 0u);
    for (uint32_t g = 0; g < ngroups; ++g) {
        uint32_t n = 0;
        for (uint32_t r = win_ptr[g]; r < win_ptr[g + 1]; ++r) n += win_runs[r].y & 0xFFFFu;
        total[g] = n;
        lptr[g + 1] = lptr[g] + kGroupRows * ((n + 2u * kGroupRows - 1u) / (2u * kGroupRows));
    }
    list.assign((size_t)lptr[ngroups] + 8, 0u);
    parallel_ranges(ngroups, 64, [&](size_t ga, size_t gb, int) {
        for (uint32_t g = (uint32_t)ga; g < (uint32_t)gb; ++g) {
            uint32_t s = 0;
            for (uint32_t r = win_ptr[g]; r < win_ptr[g + 1]; ++r)
                for (uint32_t k = 0; k < (win_runs[r].y & 0xFFFFu); ++k, ++s) {
                    const uint32_t d = (uint32_t)((int)(win_runs[r].x + k) - (int)(g * kGroupRows)) & 0xFFFFu;
                    const uint32_t j = s / (2u * kGroupRows), rest = s % (2u * kGroupRows);
                    uint32_t &w = list[(size_t)lptr[g] + (size_t)j * kGroupRows + rest % kGroupRows];
                    w |= rest < kGroupRows ? d : d << 16;
                }
        }
    });
}

// (with or without a window: the three-trip products of bicg_jagw.hip read one word per lane instead of two row pointers)
// SellDev::lane_info: row in the group + its length per lane, in the order the lanes work (perm or natural)
void plan_lane_info(const CSR_Matrix *diag, SellPlan &p)
{
    const uint32_t nrows = p.nrows, ngroups = p.ngroups;
    std::vector<unsigned short> &li = p.lane_info;
    li.assign((size_t)ngroups * kGroupRows, 0);
    std::vector<char> too_long((size_t)plan_threads(), 0);
    std::vector<uint32_t> tail_most((size_t)plan_threads(), 0u);      // entries behind the 16th of its rows, per slice (k_spmm_jpipe keeps them in LDS)
    parallel_ranges(ngroups, 64, [&](size_t ga, size_t gb, int part) {
        for (uint32_t g = (uint32_t)ga; g < (uint32_t)gb; ++g) {
            uint32_t tail = 0;
            for (uint32_t t = 0; t < kGroupRows; ++t) {
                const uint32_t in_group = p.perm.empty() ? t : p.perm[(size_t)g * kGroupRows + t], r = g * kGroupRows + in_group;
                const uint32_t n = (r < nrows && p.group_is_sell[g]) ? diag->ptr[r + 1] - diag->ptr[r] : 0u;
                if (n > 255u) too_long[(size_t)part] = 1;
                li[(size_t)g * kGroupRows + t] = (unsigned short)(in_group | (n << 8));
                if (t % kSliceRows == 0) tail = 0;
                tail += n > 16u ? n - 16u : 0u;
                tail_most[(size_t)part] = std::max(tail_most[(size_t)part], tail);
            }
        }
    });
    bool ok = true;
    for (char b : too_long) ok = ok && !b;
    for (uint32_t t : tail_most) p.jag_tail16_max = std::max(p.jag_tail16_max, t);
    if (!ok) { li.clear(); li.shrink_to_fit(); }
}

}  // namespace

// ---- SpMV plan. Rows are cut into groups of 256 (4 slices of 64 rows = one workgroup, lane = row).
// Two layouts of a slice: PADDED to its longest row (banded matrices: nothing to pad, 8-byte loads of four
// 16-bit column offsets) or JAGGED (ragged rows: step k stores the rows longer than k only; exactly the CSR's
// bytes, lane = row kept). Jagged is chosen for the whole block when padding would add > 2 % entries. Groups
// with a very long row go to the CSR row-block kernel (strided workgroup reduction of one row). Either kind
// is "boundary" when one of its rows has offd entries (it then runs after the halo has landed).
bool sell_plan_host(const CSR_Matrix *diag, const uint32_t *optr, const PlanFacts &facts, const PlanSwitches &sw, SellPlan &p,
                    PlanTrace *trace)
{
    PlanTrace silent;
    PlanTrace &tr = trace ? *trace : silent;
    const uint32_t nrows = diag->rows;
    p.nrows = nrows;
    p.nslices = (nrows + kSliceRows - 1) / kSliceRows;
    p.ngroups = (nrows + kGroupRows - 1) / kGroupRows;
    p.nnz_d = nrows ? diag->ptr[nrows] : 0u;
    bool use_sell = !sw.no_sell;
    p.rowsplit = rows_over_lanes(facts, sw, use_sell);
    if (p.rowsplit) use_sell = false;
    p.group_is_sell.assign(p.ngroups, 0);
    const uint32_t jag_max_row = std::max<uint64_t>(64, nrows ? 4 * (uint64_t)p.nnz_d / nrows : 0);   // 4 x the average row
    choose_layout(diag, sw, p);
    // x windows in LDS (SellDev::win_*): wanted for ragged rows, where the x gather of one step touches many cache
    // lines (FEM-like: 63 -> 58 us per SpMV). With equal rows the gathers are perfectly coalesced and the window
    // only adds staging loads and two barriers per group (Transport-shaped +2 %, 256^3 Laplacian +9 % although its
    // columns shrink from 32 to 16 bits), so there it is taken on request only: BICG_PLAN="window=1" asks for it
    // whenever it fits, 0 never. It needs the jagged layout.
    const bool jag_auto = p.jag;
    bool want_win = use_sell && sw.window != 0 && (sw.window == 1 || jag_auto);
    if (want_win) p.jag = true;
    select_groups(diag, optr, facts.P, use_sell, jag_max_row, p);
    if (want_win && !plan_windows(diag, facts, sw, p)) {      // some group's window does not fit: no windows for this block
        want_win = false; p.win_slots = 0; p.win_runs.clear(); p.win_ptr.clear();
        if (!jag_auto) {                                      // ... and the jagged layout was only taken for their sake
            p.jag = false; p.retried = true;
            std::fill(p.group_is_sell.begin(), p.group_is_sell.end(), 0);
            select_groups(diag, optr, facts.P, use_sell, jag_max_row, p);
        }
    }
    p.win = want_win && p.win_slots > 0;
    if (p.win && sw.sell_sort && !deal_rows_by_length(diag, p)) return false;
    tr.mark("groups, windows, row order");
    column_offsets_and_clusters(diag, sw, p);
    tr.mark("column offsets, clusters");
    fill_slices(diag, p);
    tr.mark("sliced-ELL arrays");
    classify_slices(diag, sw, p);
    tr.mark("uniform / constant / masked slices");
    plan_row_blocks(diag, optr, facts.P, p);
    tr.mark("row blocks");
    plan_csr16(diag, sw, p);
    if (p.win) finish_windows(p);
    if (p.jag && p.sell_entries > 0) plan_lane_info(diag, p);
    return true;
}

// ---- the plan as numbers: bicg_sell_plan_digest (include/bicgstab_hip.h section 5 documents both orders)
void sell_plan_summary(const SellPlan &p, unsigned long long s[kSellSummaryLen])
{
    const unsigned long long v[kSellSummaryLen] = {
        p.jag ? 1ull : 0ull, p.c16 ? 1ull : 0ull, (unsigned long long)p.fw.ncl, p.win ? (p.win_list_mode ? 2ull : 1ull) : 0ull,
        p.retried ? 1ull : 0ull, p.rowsplit ? 1ull : 0ull, p.sell_entries, p.sell_nnz, p.sell_rows, p.uniform_entries,
        p.constant_entries, p.masked_rows, p.nblk(), p.gl_int.size(), p.gl_bnd.size(), p.csr16 ? 1ull : 0ull, p.win_slots,
        p.win_max_runs, p.win_near16 ? 1ull : 0ull, p.jag_tail16_max, p.bbnd.size(), p.lane_info.empty() ? 0ull : 1ull};
    for (int i = 0; i < kSellSummaryLen; ++i) s[i] = v[i];
}

static unsigned long long fnv1a(const void *data, size_t bytes)
{
    const unsigned char *b = static_cast<const unsigned char *>(data);
    unsigned long long h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
template <class T> static unsigned long long fnv1a(const std::vector<T> &v) { return fnv1a(v.data(), sizeof(T) * v.size()); }

void sell_plan_digest(const SellPlan &p, unsigned long long d[kSellDigestLen])
{
    const unsigned long long v[kSellDigestLen] = {
        fnv1a(p.slice_len), fnv1a(p.slice_base), fnv1a(p.slice_base16),
        fnv1a(p.sval.get(), sizeof(double) * (size_t)p.sell_entries),
        fnv1a(p.scol.get(), p.scol ? sizeof(uint32_t) * (size_t)p.sell_entries : 0),
        fnv1a(p.scol16.get(), p.c16 ? sizeof(short) * (size_t)p.n16 : 0),
        fnv1a(p.perm), fnv1a(p.group_is_sell), fnv1a(p.gl_int), fnv1a(p.gl_bnd), fnv1a(p.bint), fnv1a(p.bbnd),
        fnv1a(p.win_ptr), fnv1a(p.win_runs), fnv1a(p.list), fnv1a(p.lptr), fnv1a(p.total),
        fnv1a(p.ubase), fnv1a(p.vbase), fnv1a(p.mbase), fnv1a(p.uoff), fnv1a(p.uval), fnv1a(p.rmask),
        fnv1a(p.lane_info), fnv1a(p.dcol16), fnv1a(&p.fw, sizeof p.fw)};
    for (int i = 0; i < kSellDigestLen; ++i) d[i] = v[i];
}

}  // namespace bicg
