// bicg_reorder.cpp -- BICG_PLAN="reorder=1|2": a bandwidth-reducing renumbering of a rank's diag block, made on the host without a
// device. reorder_rcm orders the rows by reverse Cuthill-McKee on the symmetrised pattern; permute_block
// builds P A P^T with the entries of every row in their stored order, so that a row's sum is associated exactly as mult()
// (reference src/matrix.c:498-516) associates it on the caller's matrix. Like bicg_sell_plan.cpp nothing here calls the HIP runtime
// or reads the environment, and every loop handed to parallel_ranges writes its own indices only (the adjacency lists are filled
// through atomic cursors and then sorted row by row): the order does not depend on the thread count.
#include "bicg_plan.h"
#include "bicg_parallel.h"

#include <algorithm>
#include <cstring>

namespace bicg {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// the symmetrised pattern without the diagonal: row v's neighbours are adj[start[v] .. start[v] + deg[v]), ascending, each once
struct Graph {
    std::vector<uint64_t> start;
    std::vector<uint32_t> deg, adj;
};

void build_graph(const CSR_Matrix *A, Graph &g)
{
    const uint32_t n = A->rows;
    std::vector<uint32_t> own(n, 0u), cnt(n, 0u);
    // entry (i, j) makes i and j neighbours whichever of the two is stored: list i gets j, list j gets i, duplicates go below.
    // A list holds the row's own columns first, in place, and behind them the rows that name it, in arrival order.
    parallel_ranges(n, 4096, [&](size_t r0, size_t r1, int) {
        for (size_t r = r0; r < r1; ++r)
            for (uint32_t k = A->ptr[r]; k < A->ptr[r + 1]; ++k) {
                const uint32_t j = A->col[k];
                if (j == r || j >= n) continue;
                ++own[r];
                __atomic_fetch_add(&cnt[j], 1u, __ATOMIC_RELAXED);
            }
    });
    g.start.assign((size_t)n + 1, 0ull);
    for (uint32_t v = 0; v < n; ++v) g.start[v + 1] = g.start[v] + own[v] + cnt[v];
    g.adj.resize(std::max<uint64_t>(g.start[n], 1ull));
    std::vector<uint64_t> cur(n);
    for (uint32_t v = 0; v < n; ++v) cur[v] = g.start[v] + own[v];
    parallel_ranges(n, 4096, [&](size_t r0, size_t r1, int) {
        for (size_t r = r0; r < r1; ++r) {
            uint64_t o = g.start[r];
            for (uint32_t k = A->ptr[r]; k < A->ptr[r + 1]; ++k) {
                const uint32_t j = A->col[k];
                if (j == r || j >= n) continue;
                g.adj[o++] = j;
                g.adj[__atomic_fetch_add(&cur[j], 1ull, __ATOMIC_RELAXED)] = (uint32_t)r;
            }
        }
    });
    // (the cursors hand out places in arrival order: sorting each list makes the result independent of it)
    g.deg.assign(n, 0u);
    parallel_ranges(n, 4096, [&](size_t r0, size_t r1, int) {
        for (size_t v = r0; v < r1; ++v) {
            uint32_t *a = g.adj.data() + g.start[v], *b = g.adj.data() + g.start[v + 1];
            std::sort(a, b);
            g.deg[v] = (uint32_t)(std::unique(a, b) - a);
        }
    });
}

// Cuthill-McKee, reversed component by component. Returns the number of components with at least two rows.
uint32_t rcm_order(const Graph &g, uint32_t n, uint32_t *perm, uint32_t *isolated_out)
{
    // ---- start vertices: with the vertices taken by (degree, original index), the first one not yet swept is the lowest-numbered
    // vertex of minimum degree of ITS component -- no sweep of its own is needed to find the components (counting sort by degree)
    uint32_t maxdeg = 0;
    for (uint32_t v = 0; v < n; ++v) maxdeg = std::max(maxdeg, g.deg[v]);
    std::vector<uint32_t> first((size_t)maxdeg + 2, 0u), cand(n);
    for (uint32_t v = 0; v < n; ++v) ++first[g.deg[v] + 1];
    for (uint32_t d = 0; d <= maxdeg; ++d) first[d + 1] += first[d];
    for (uint32_t v = 0; v < n; ++v) cand[first[g.deg[v]]++] = v;
    // ---- one breadth-first sweep per component: the unvisited neighbours of the vertex at the head of the order join it by
    // (degree, original index) -- within a level that is (parent's position, degree, original index)
    std::vector<unsigned char> seen(n, 0);
    std::vector<uint32_t> sweep(n), next;
    struct Comp { uint32_t start, base, len; };
    std::vector<Comp> comps;
    uint32_t out = 0;
    for (uint32_t s : cand) {
        if (seen[s] || g.deg[s] == 0) continue;
        const uint32_t base = out;
        uint32_t head = out;
        sweep[out++] = s; seen[s] = 1;
        while (head < out) {
            const uint32_t v = sweep[head++];
            const uint32_t *a = g.adj.data() + g.start[v];
            next.clear();
            for (uint32_t k = 0; k < g.deg[v]; ++k) if (!seen[a[k]]) { seen[a[k]] = 1; next.push_back(a[k]); }
            // (the list is ascending: a stable sort by degree leaves equal degrees in index order)
            std::stable_sort(next.begin(), next.end(), [&](uint32_t x, uint32_t y) { return g.deg[x] < g.deg[y]; });
            for (uint32_t w : next) sweep[out++] = w;
        }
        std::reverse(sweep.begin() + base, sweep.begin() + out);
        comps.push_back(Comp{s, base, out - base});
    }
    // ---- the components in ascending order of their start vertex; rows without neighbours last, in their original order
    std::sort(comps.begin(), comps.end(), [](const Comp &a, const Comp &b) { return a.start < b.start; });
    uint32_t at = 0;
    for (const Comp &c : comps) { std::copy(sweep.begin() + c.base, sweep.begin() + c.base + c.len, perm + at); at += c.len; }
    uint32_t isolated = 0;
    for (uint32_t v = 0; v < n; ++v) if (g.deg[v] == 0) { perm[at++] = v; ++isolated; }
    *isolated_out = isolated;
    return (uint32_t)comps.size();
}

// max |i - j| over the stored entries and the most distinct columns one 256-row group touches, for the rows taken in the order
// rows_in[new] (null: as given) with the columns renamed through inv (null: as given)
void numbering_stats(const CSR_Matrix *A, const uint32_t *rows_in, const uint32_t *inv, unsigned long long *band_out, unsigned long long *distinct_out)
{
    const uint32_t n = A->rows, ngroups = (n + kGroupRows - 1) / kGroupRows;
    std::vector<unsigned long long> band(plan_threads(), 0ull), most(plan_threads(), 0ull);
    parallel_ranges(ngroups, 16, [&](size_t g0, size_t g1, int part) {
        // the group's columns go through an open-addressing set of at least twice as many places as the group has entries
        std::vector<uint32_t> set;
        for (size_t g = g0; g < g1; ++g) {
            const uint32_t i0 = (uint32_t)g * kGroupRows, i1 = (uint32_t)std::min<uint64_t>(n, (g + 1) * (uint64_t)kGroupRows);
            uint64_t entries = 0;
            for (uint32_t i = i0; i < i1; ++i) { const uint32_t r = rows_in ? rows_in[i] : i; entries += A->ptr[r + 1] - A->ptr[r]; }
            size_t cap = 1024;
            while (cap < 2 * entries) cap *= 2;
            set.assign(cap, kNone);
            unsigned long long distinct = 0;
            for (uint32_t i = i0; i < i1; ++i) {
                const uint32_t r = rows_in ? rows_in[i] : i;
                for (uint32_t k = A->ptr[r]; k < A->ptr[r + 1]; ++k) {
                    const uint32_t j = inv && A->col[k] < n ? inv[A->col[k]] : A->col[k];
                    band[part] = std::max<unsigned long long>(band[part], j > i ? j - i : i - j);
                    size_t h = ((size_t)j * 0x9E3779B1u) & (cap - 1);
                    while (set[h] != kNone && set[h] != j) h = (h + 1) & (cap - 1);
                    if (set[h] == kNone) { set[h] = j; ++distinct; }
                }
            }
            most[part] = std::max(most[part], distinct);
        }
    });
    *band_out = *std::max_element(band.begin(), band.end());
    *distinct_out = *std::max_element(most.begin(), most.end());
}

}  // namespace

void reorder_rcm(const CSR_Matrix *diag, uint32_t *perm, unsigned long long stats[8])
{
    const uint32_t n = diag->rows;
    for (int i = 0; i < 8; ++i) stats[i] = 0ull;
    if (n == 0) return;
    uint32_t isolated = 0, comps = 0;
    {
        Graph g;
        build_graph(diag, g);
        comps = rcm_order(g, n, perm, &isolated);
    }
    std::vector<uint32_t> inv(n);
    parallel_ranges(n, 65536, [&](size_t i0, size_t i1, int) { for (size_t i = i0; i < i1; ++i) inv[perm[i]] = (uint32_t)i; });
    stats[0] = n; stats[1] = comps; stats[6] = isolated;
    numbering_stats(diag, nullptr, nullptr, &stats[2], &stats[4]);
    numbering_stats(diag, perm, inv.data(), &stats[3], &stats[5]);
}

bool permute_block(const CSR_Matrix *diag, const uint32_t *perm, uint32_t *ptr_out, uint32_t *col_out, double *val_out, uint32_t *inv_out)
{
    const uint32_t n = diag->rows;
    std::vector<uint32_t> inv_own;
    if (!inv_out) { inv_own.resize(std::max<uint32_t>(n, 1u)); inv_out = inv_own.data(); }
    std::fill(inv_out, inv_out + n, kNone);
    for (uint32_t i = 0; i < n; ++i) {
        if (perm[i] >= n || inv_out[perm[i]] != kNone) return false;
        inv_out[perm[i]] = i;
    }
    ptr_out[0] = 0u;
    for (uint32_t i = 0; i < n; ++i) ptr_out[i + 1] = ptr_out[i] + (diag->ptr[perm[i] + 1] - diag->ptr[perm[i]]);
    // row `new` is row perm[new] with every column renamed, entry for entry: nothing is sorted
    parallel_ranges(n, 4096, [&](size_t i0, size_t i1, int) {
        for (size_t i = i0; i < i1; ++i) {
            const uint32_t a = diag->ptr[perm[i]], len = diag->ptr[perm[i] + 1] - a, o = ptr_out[i];
            for (uint32_t k = 0; k < len; ++k) {
                const uint32_t j = diag->col[a + k];
                col_out[o + k] = j < n ? inv_out[j] : j;
                val_out[o + k] = diag->val[a + k];
            }
        }
    });
    return true;
}

}  // namespace bicg

extern "C" int bicg_reorder_plan(const CSR_Matrix *diag, int method, unsigned int *perm, unsigned long long stats[8])
{
    if (!diag || !perm || !stats || method != 1) return 1;
    bicg::reorder_rcm(diag, perm, stats);
    return 0;
}

extern "C" int bicg_permute_block(const CSR_Matrix *diag, const unsigned int *perm, unsigned int *ptr_out, unsigned int *col_out, double *val_out)
{
    return bicg::permute_block(diag, perm, ptr_out, col_out, val_out) ? 0 : -1;
}
