"""Crafted matrices with ragged rows that sit ON the plan limits of the ragged-row products (k_spmv_jagw / k_spmv_jagl / k_spmv_jagd,
csrc/bicg_jagw.hip; k_spmm_jpipe, csrc/bicg_spmm_jag.hip) -- a plain helper of tests/test_ragged_limits.py (CPU: the plan of every
case is what this file promises) and tests/test_ragged_limits_gpu.py. Plain numpy: no library call in here.

Every generator returns (synth.CSR, facts). `facts` is what the sliced-ELL plan must report for the matrix (the entries of
hipsolver.SELL_SUMMARY named in FACT_KEYS) plus "kernel", the product kernel hipsolver.product_kernels() must name. The facts are
worked out here, from the pattern alone, by `plan_facts` -- the limits as csrc/bicg_sell_plan.cpp and csrc/bicg_device.h document
them -- and every generator asserts on them what it was built for (e.g. runs(64): exactly 64 runs in every group).

The limits (rows are cut into groups of 256 = 4 slices of 64):
    runs per group      <= 64    (kJagwMaxRuns: lane r of a wavefront holds run r; runs = the group's columns, gaps <= 8 merged)
    slots per window    <= 2048  (kJagwMaxSlots: 8 values staged per thread)
    row length          <= 255   (one 16-bit word per lane: row in the group + its length; else no lane_info)
    list entries        16-bit distances from the group's first row, -32768 .. 32767, <= 2048 distinct columns per group; one
                        rank with at least 6 000 000 diag non-zeros (the list-driven window, window = 2)
    16-bit offsets      |column - row| <= 32767 without a window, else 32-bit columns (k_spmv_jagd<C16 = false>)
    SpMM (k_spmm_jpipe) windows of at most 2047 slots within 16 bits of their groups, and
                        16 W + 8192 + 640 + 40 roundup64(jag_tail16_max) <= 81920 bytes, W = (win_slots + 2) & ~1

Values on one pattern (`values=`): "generic" standard normal; "integer" from {1, 2, 3}; "dominant" standard normal with every stored
diagonal entry replaced by 1 + the sum of the row's other magnitudes. `seed` picks another draw of the same law on the same pattern.
Entries of a row are in ascending column order."""
from __future__ import annotations

import functools

import numpy as np

from mpi_bicgstab_amd import synth

GROUP, SLICE = 256, 64
MAX_RUNS, MAX_SLOTS, RUN_GAP, RUN_WINDOW_CAP = 64, 2048, 8, 4096
LIST_MIN_NNZ = 6_000_000
FACT_KEYS = ("window", "win_slots", "win_max_runs", "lane_info", "c16", "win_near16", "jag_tail16_max", "nblk")


class Pattern:
    """rows x rows sparsity pattern: ptr (int64, rows + 1), col (int64), rows sorted by column, no entry twice"""

    def __init__(self, n, rows, cols, presorted=False):
        rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
        if not presorted:
            order = np.lexsort((cols, rows))
            rows, cols = rows[order], cols[order]
        assert len(cols) == 0 or (cols.min() >= 0 and cols.max() < n and rows.min() >= 0 and rows.max() < n)
        same_row = rows[1:] == rows[:-1]
        assert np.all(rows[1:] >= rows[:-1]) and np.all(cols[1:][same_row] > cols[:-1][same_row]), "ascending columns, no entry twice"
        self.n, self.row, self.col = int(n), rows, cols
        self._group_keys = None          # (group_runs: the distinct columns of every group, sorted)
        self.ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=n), out=self.ptr[1:])

    @property
    def lens(self):
        return np.diff(self.ptr)

    def csr(self, values="generic", seed=0):
        rng = np.random.default_rng([seed, {"generic": 1, "integer": 2, "dominant": 3}[values]])
        nnz = len(self.col)
        if values == "integer":
            val = rng.integers(1, 4, size=nnz).astype(np.float64)
        else:
            val = rng.standard_normal(nnz)
            if values == "dominant":
                diag = self.row == self.col
                off = np.bincount(self.row[~diag], weights=np.abs(val[~diag]), minlength=self.n)
                val[diag] = 1.0 + off[self.row[diag]]
        return synth.CSR(self.n, self.n, self.ptr.astype(np.uint32), self.col.astype(np.uint32), val)


# ---- the plan's decisions for a one-rank block with ragged rows, from the pattern alone -----------------------------------------------
def group_runs(P, gap):
    """per 256-row group: (runs, slots, nearest and furthest run end as distances from the group's first row) of its distinct columns
    with gaps of at most `gap` columns merged (bicg_window_plan)"""
    ng = -(-P.n // GROUP)
    if P._group_keys is None:
        P._group_keys = np.unique((P.row // GROUP) * (1 << 32) + P.col)
    key = P._group_keys
    g, c = key >> 32, key & 0xFFFFFFFF
    first = np.ones(len(key), dtype=bool)
    first[1:] = (g[1:] != g[:-1]) | (c[1:] - c[:-1] > gap + 1)
    last = np.append(first[1:], True)
    runs = np.bincount(g[first], minlength=ng)
    slots = np.bincount(g[first], weights=(c[last] - c[first] + 1).astype(np.float64), minlength=ng).astype(np.int64)
    lo, hi = np.zeros(ng, dtype=np.int64), np.zeros(ng, dtype=np.int64)
    np.minimum.at(lo, g[first], c[first] - g[first] * GROUP)
    np.maximum.at(hi, g[last], c[last] - g[last] * GROUP)
    return runs, slots, lo, hi


def plan_facts(P, window=None, large=False):
    """FACT_KEYS + "kernel" of a one-rank block whose rows are ragged enough for the jagged layout, every group on the sliced-ELL
    path. window: the BICG_PLAN switch (None or 0); large: the block counts as one of at least LIST_MIN_NNZ non-zeros"""
    lens = P.lens
    padded = sum(int(lens[s:s + SLICE].max()) * len(lens[s:s + SLICE]) for s in range(0, P.n, SLICE))
    nnz = int(P.ptr[-1])
    assert padded > nnz + nnz // 50, "ragged rows: padding would add more than 2 %"
    assert int(lens.max()) <= max(64, 4 * nnz // P.n), "no row so long that its group leaves the sliced-ELL path"
    assert nnz // P.n < 128, "rows over lanes stays off"
    kind, slots, most_runs, near16 = 0, 0, 0, 0
    if window != 0:
        runs, sl, lo, hi = group_runs(P, RUN_GAP)
        if runs.max() <= MAX_RUNS and sl.max() <= MAX_SLOTS:
            kind = 1
        elif large and sl.max() <= RUN_WINDOW_CAP:      # (the list is tried only where the run windows fit their own 4096 slots)
            runs, sl, lo, hi = group_runs(P, 0)
            d = P.col - (P.row // GROUP) * GROUP
            if sl.max() <= MAX_SLOTS and d.min() >= -32768 and d.max() <= 32767:
                kind = 2
        if kind:
            slots, most_runs, near16 = int(sl.max()), int(runs.max()), int(lo.min() >= -32767 and hi.max() <= 32767)
    # the lanes of a group take its rows in natural order, or -- with a window -- by decreasing length
    padded_lens = np.zeros(-(-P.n // GROUP) * GROUP, dtype=np.int64)
    padded_lens[:P.n] = lens
    by_group = padded_lens.reshape(-1, GROUP)
    if kind:
        by_group = -np.sort(-by_group, axis=1)
    tail = int(np.maximum(by_group - 16, 0).reshape(-1, SLICE).sum(axis=1).max())
    lane_info = int(lens.max() <= 255)
    c16 = 1 if kind else int(np.abs(P.col - P.row).max() <= 32767)
    kernel = (("jagw", "jagw_list")[kind - 1] if kind else "jagd") if lane_info else ("sell_window_loop" if kind else "sell_jagged")
    return dict(window=kind, win_slots=slots, win_max_runs=most_runs, lane_info=lane_info, c16=c16, win_near16=near16,
                jag_tail16_max=tail, nblk=0, kernel=kernel)


def _done(P, facts, values, seed):
    return P.csr(values, seed), dict(facts)


def _near(rng, r, n, half, count):
    """`count` distinct columns around row r, the diagonal among them: within `half` of r, or of the nearest row that leaves room"""
    lo = min(max(r - half, 0), n - (2 * half + 1))
    cand = np.arange(lo, lo + 2 * half + 1)
    cand = cand[cand != r]
    return np.append(rng.choice(cand, size=count - 1, replace=False), r)


def _banded(n, lens, half, seed):
    """row r holds lens[r] entries (0: none), its diagonal and columns within `half` of it"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r in range(n):
        if lens[r]:
            c = _near(rng, r, n, half, int(lens[r]))
            rows.append(np.full(len(c), r)); cols.append(c)
    return Pattern(n, np.concatenate(rows), np.concatenate(cols))


# ---- the small cases ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _runs(k):
    n = 2000
    rng = np.random.default_rng(100 + k)
    rows, cols = [], []
    for r0 in range(0, n, GROUP):
        nr = min(GROUP, n - r0)
        # run 0 is the group's diagonal block; k - 1 more of 1 .. 3 columns, 20 columns apart, none within 10 of the block
        anchors = np.arange(5, n - 3, 20)
        anchors = anchors[(anchors + 2 < r0 - 10) | (anchors > r0 + nr - 1 + 10)]
        anchors = np.sort(anchors[np.argsort(np.abs(anchors - (r0 + nr // 2)), kind="stable")[:k - 1]])
        assert len(anchors) == k - 1 <= nr
        run_cols = np.concatenate([a + np.arange(1 + j % 3) for j, a in enumerate(anchors)])
        for t in range(nr):
            want = int(rng.integers(1, 25))
            c = [np.array([r0 + t])]
            if t < k - 1:                                   # every run is touched, in all of its columns
                c.append(anchors[t] + np.arange(1 + t % 3))
                want = max(want, 1 + len(c[1]))
            c = np.concatenate(c)
            rest = np.setdiff1d(run_cols, c)
            c = np.append(c, rng.choice(rest, size=want - len(c), replace=False))
            rows.append(np.full(len(c), r0 + t)); cols.append(c)
    P = Pattern(n, np.concatenate(rows), np.concatenate(cols))
    f = plan_facts(P)
    runs, _, _, _ = group_runs(P, RUN_GAP)
    assert np.all(runs == k) and 1 <= P.lens.min() and P.lens.max() <= 24
    assert (f["window"], f["win_max_runs"], f["kernel"]) == ((1, k, "jagw") if k <= MAX_RUNS else (0, 0, "jagd")) and f["c16"] == 1
    return P, f


def runs(k, values="generic", seed=0):
    """every group touches exactly k runs more than 9 columns apart (its diagonal block and k - 1 runs of 1 .. 3 columns); rows of
    1 .. 24 entries; 2000 rows, the last group partly filled. k = 65: no window, k_spmv_jagd with 16-bit offsets"""
    return _done(*_runs(k), values, seed)


@functools.lru_cache(maxsize=None)
def _span(w, long_group=None, long_len=0, long_one=0):
    n = 2700
    rng = np.random.default_rng(200 + w)
    rows, cols = [], []
    for gi, r0 in enumerate(range(0, n, GROUP)):
        nr = min(GROUP, n - r0)
        s = min(max(r0 + nr // 2 - w // 2, 0), n - w)
        assert s <= r0 and r0 + nr <= s + w
        # the span's first and last column and every 8th in between, outside the diagonal block (which the diagonals touch)
        forced = np.unique(np.append(np.arange(s, s + w, 8), s + w - 1))
        forced = forced[(forced < r0) | (forced >= r0 + nr)]
        assert len(forced) <= 2 * nr
        span = np.arange(s, s + w)
        for t in range(nr):
            c = np.unique(np.array([r0 + t, forced[(2 * t) % len(forced)], forced[(2 * t + 1) % len(forced)]]))
            want = len(c) + int(rng.integers(0, 11))
            if gi == long_group and t < SLICE:
                want = long_len + (1 if t == 5 and long_one else 0)
            c = np.append(c, rng.choice(np.setdiff1d(span, c), size=want - len(c), replace=False))
            rows.append(np.full(len(c), r0 + t)); cols.append(c)
    P = Pattern(n, np.concatenate(rows), np.concatenate(cols))
    f = plan_facts(P)
    runs_, slots_, _, _ = group_runs(P, RUN_GAP)
    assert np.all(runs_ == 1) and np.all(slots_ == w)
    return P, f


def slots(w, values="generic", seed=0):
    """the columns of every group form ONE span of w columns with gaps <= 8 (one run of w slots); 2700 rows, the last group partly
    filled. w = 2049: no window, k_spmv_jagd with 16-bit offsets"""
    P, f = _span(w)
    assert (f["window"], f["win_slots"], f["kernel"]) == ((1, w, "jagw") if w <= MAX_SLOTS else (0, 0, "jagd")) and f["c16"] == 1
    return _done(P, f, values, seed)


def jpipe_edge(tail, win_slots=2047, values="generic", seed=0):
    """slots(win_slots) with rows of at most 13 entries, except that the 64 longest rows of group 3 hold 31 entries each -- for
    tail = 961 one of them 32: jag_tail16_max = tail, on either side of k_spmm_jpipe's LDS budget (W = 2048 for 2047 slots:
    32768 + 8192 + 640 + 40 * 960 = 80000 <= 81920 < 82560 = ... + 40 * 1024). 2048 slots are one more than that kernel takes."""
    assert tail in (960, 961)
    P, f = _span(win_slots, 3, 31, tail - 960)
    assert (f["window"], f["win_slots"], f["win_near16"], f["jag_tail16_max"], f["kernel"]) == (1, win_slots, 1, tail, "jagw")
    return _done(P, f, values, seed)


LENGTHS_JAGW = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33)      # the batch edges of k_spmv_jagw: two batches of 8 in flight
LENGTHS_JAGD = (5, 6, 7, 11, 12, 13, 17, 18, 19, 24, 25)             # ... of k_spmv_jagd: batches of 6, a third prefetched, a tail loop from 18
LENGTHS_EXTRA = ("all_empty", "slice_empty", "single_entry")         # the groups behind the one per length, then a partly filled one


@functools.lru_cache(maxsize=None)
def _lengths(Ls):
    rng = np.random.default_rng(300 + len(Ls))
    lens = []
    for L in Ls:          # the group's longest row is L, the rest ragged down to 0
        l = rng.integers(0, L + 1, size=GROUP)
        at = rng.choice(GROUP, size=2, replace=False)
        l[at[0]], l[at[1]] = L, 0
        lens.append(l)
    lens.append(np.zeros(GROUP, dtype=np.int64))                       # every row empty
    l = rng.integers(1, 13, size=GROUP); l[2 * SLICE:3 * SLICE] = 0      # one whole slice empty (by length: the last one)
    lens.append(l)
    lens.append(np.ones(GROUP, dtype=np.int64))                        # single-entry rows
    lens.append(rng.integers(1, 11, size=100))                         # the last group: two of four slices
    lens = np.concatenate(lens)
    P = _banded(len(lens), lens, 40, 301)
    assert np.array_equal(P.lens, lens)
    return P


def lengths(kernel="jagw", values="generic", seed=0):
    """one group per slice length L of LENGTHS_JAGW (kernel="jagw": plans with a window) or LENGTHS_JAGD (kernel="jagd": to be planned
    under switches(window=0)), then the groups of LENGTHS_EXTRA and a last group of 100 rows; columns within 40 of the row"""
    Ls = {"jagw": LENGTHS_JAGW, "jagd": LENGTHS_JAGD}[kernel]
    P = _lengths(Ls)
    f = plan_facts(P, window=None if kernel == "jagw" else 0)
    longest = P.lens[:len(Ls) * GROUP].reshape(-1, GROUP).max(axis=1)
    assert tuple(longest) == Ls and f["kernel"] == kernel and f["window"] == (kernel == "jagw") and f["c16"] == 1
    f["groups"] = {**{L: i for i, L in enumerate(Ls)}, **{name: len(Ls) + i for i, name in enumerate(LENGTHS_EXTRA)}}
    return _done(P, f, values, seed)


@functools.lru_cache(maxsize=None)
def _longrow(m):
    n = 14 * 97
    rng = np.random.default_rng(400)
    lens = rng.integers(40, 121, size=n)
    lens[::97] = m
    return _banded(n, lens, 200, 401)


def longrow(m, values="generic", seed=0):
    """every 97th row holds m entries, the others 40 .. 120 (mean about 81: no row leaves the sliced-ELL path, rows over lanes stays
    off). m = 255 is the longest row one 16-bit lane word holds; with 256 the plan drops lane_info: k_spmv_sell's loop"""
    P = _longrow(m)
    f = plan_facts(P)
    assert P.lens.max() == m and 64 <= P.ptr[-1] // P.n < 128
    assert (f["window"], f["lane_info"], f["kernel"]) == (1, int(m <= 255), "jagw" if m <= 255 else "sell_window_loop")
    return _done(P, f, values, seed)


@functools.lru_cache(maxsize=None)
def _tail(t):
    n = 3 * GROUP + t
    return _banded(n, np.random.default_rng(500 + t).integers(1, 25, size=n), 40, 501 + t)


def tail(t, values="generic", seed=0):
    """3 * 256 + t rows of 1 .. 24 entries: the last group holds t rows -- it lacks 3, 2, 1 or 0 of its slices"""
    P = _tail(t)
    f = plan_facts(P)
    assert (f["window"], f["kernel"]) == (1, "jagw")
    f["slices_of_last_group"] = -(-t // SLICE)
    return _done(P, f, values, seed)


@functools.lru_cache(maxsize=None)
def _far32(far):
    n = 40000
    rng = np.random.default_rng(600)
    lens = rng.integers(0, 12, size=n)                        # entries beside the diagonal
    r = np.repeat(np.arange(n), lens)
    c = r + rng.integers(-3000, 3001, size=len(r))
    c = np.where(c < 0, -c, np.where(c >= n, 2 * (n - 1) - c, c))
    # on the limit of a 16-bit offset in both directions; `far`: one column one further than that
    r = np.concatenate([r, np.arange(n), [100, 39000]])
    c = np.concatenate([c, np.arange(n), [100 + 32767 + (1 if far else 0), 39000 - 32767]])
    key = np.unique(r * (1 << 32) + c)
    return Pattern(n, key >> 32, key & 0xFFFFFFFF, presorted=True)


def far32(far=True, values="generic", seed=0):
    """40 000 ragged rows whose groups touch far too many scattered columns for a window; one entry 32767 columns to the left of
    its row and one 32767 to the right -- far=True: 32768 to the right, so the block keeps 32-bit columns (k_spmv_jagd<C16 = false>)"""
    P = _far32(bool(far))
    f = plan_facts(P)
    assert int(np.abs(P.col - P.row).max()) == 32767 + (1 if far else 0)
    assert (f["window"], f["c16"], f["kernel"]) == (0, 0 if far else 1, "jagd")
    return _done(P, f, values, seed)


# ---- the large case: the list-driven window at its limits ------------------------------------------------------------------------------
LIST_ROWS = 371_237
LIST_OFFSETS = (1, 2, 3, 26, 27, 28, 29, 30, 57, 58, 390, 391, 392, 417, 418, 419, 420, 421, 780, 781, 799, 800)
LIST_GROUPS = {"far_a": 160, "far_b": 170, "runs65": 50, "near2048": 100}      # crafted groups (the same in the 90 000-row versions)
LIST_NEIGHBOURS = ("2049", "-32769", "+32768")


def _dealt(rng, r0, columns, lens):
    """the columns dealt to the rows r0 .. at random, lens[t] to row t (every column to exactly one row)"""
    assert lens.sum() == len(columns)
    return np.repeat(r0 + np.arange(len(lens)), lens), rng.permutation(columns)


@functools.lru_cache(maxsize=None)
def _list_limits(n, neighbour):
    rng = np.random.default_rng(700)
    offs = np.array(sorted([0] + list(LIST_OFFSETS) + [-o for o in LIST_OFFSETS]), dtype=np.int64)
    assert len(offs) == 45 and np.abs(offs).max() == 800
    keep = rng.random((n, len(offs))) < 0.4
    keep[:, len(offs) // 2] = True                             # the diagonal
    for g in LIST_GROUPS.values():
        keep[g * GROUP:(g + 1) * GROUP] = False
    c = np.arange(n, dtype=np.int64)[:, None] + offs[None, :]
    keep &= (c >= 0) & (c < n)
    rows, cols = [np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], c.shape)[keep]], [c[keep]]
    ragged = np.append(np.tile(np.arange(1, 16), 17), 8)       # 256 row lengths 1 .. 15 that add up to 2048
    assert len(ragged) == GROUP and ragged.sum() == MAX_SLOTS
    for name in ("far_a", "far_b"):
        # exactly 2048 distinct columns at least 16 apart, the first 32768 to the left of the group's first row, the last 32767 to its right
        r0 = LIST_GROUPS[name] * GROUP
        grid = r0 - 32768 + 16 * np.arange(1, 4095)
        picked = np.concatenate([[r0 - 32768], np.sort(rng.choice(grid, size=MAX_SLOTS - 2, replace=False)), [r0 + 32767]])
        lens = ragged.copy()
        if name == "far_a" and neighbour == "2049":
            picked = np.append(picked, np.setdiff1d(grid, picked)[0]); lens[0] += 1
        if name == "far_a" and neighbour == "-32769":
            picked[0] -= 1
        if name == "far_a" and neighbour == "+32768":
            picked[MAX_SLOTS - 1] += 1
        r, cc = _dealt(rng, r0, picked, lens)
        rows.append(r); cols.append(cc)
    r0 = LIST_GROUPS["near2048"] * GROUP                       # 2048 distinct columns, all within 1000 of the group's rows
    r, cc = _dealt(rng, r0, rng.choice(np.arange(r0 - 1000, r0 + GROUP + 1000), size=MAX_SLOTS, replace=False), ragged)
    rows.append(r); cols.append(cc)
    r0 = LIST_GROUPS["runs65"] * GROUP                         # 65 runs of 1 .. 3 columns, 20 columns apart
    anchors = r0 - 650 + 20 * np.arange(65)
    run_cols = np.concatenate([a + np.arange(1 + j % 3) for j, a in enumerate(anchors)])
    for t in range(GROUP):
        cc = anchors[t] + np.arange(1 + t % 3) if t < 65 else np.zeros(0, dtype=np.int64)
        want = max(len(cc), int(rng.integers(1, 25)))
        cc = np.append(cc, rng.choice(np.setdiff1d(run_cols, cc), size=want - len(cc), replace=False))
        rows.append(np.full(len(cc), r0 + t)); cols.append(np.sort(cc))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    key = np.sort(rows * (1 << 32) + cols)
    return Pattern(n, key >> 32, key & 0xFFFFFFFF, presorted=True)


def list_limits(n=LIST_ROWS, neighbour=None, values="generic", seed=0):
    """ragged filler rows (45 offsets within 800 of the diagonal, each kept with probability 0.4) around four crafted groups: two with
    exactly 2048 distinct columns from r0 - 32768 to r0 + 32767, one with 65 runs, one with 2048 distinct columns within 1000 of its
    rows; the last group partly filled. n = LIST_ROWS: more than 6 000 000 non-zeros, the list-driven window with real facts.
    neighbour (LIST_NEIGHBOURS; smaller n, to be planned with inflated facts): 2049 distinct columns, or a distance of -32769 or
    +32768, in the first crafted group -- no window, 32-bit columns"""
    assert neighbour is None or neighbour in LIST_NEIGHBOURS
    assert n % GROUP and n > (max(LIST_GROUPS.values()) + 1) * GROUP + 32768
    P = _list_limits(n, neighbour)
    f = plan_facts(P, large=True)
    runs8, slots8, _, _ = group_runs(P, RUN_GAP)
    runs0, slots0, lo, hi = group_runs(P, 0)
    fa = LIST_GROUPS["far_a"]
    assert runs8.max() > MAX_RUNS and runs8[LIST_GROUPS["runs65"]] == 65, "run windows do not take this block"
    assert slots0[LIST_GROUPS["far_b"]] == MAX_SLOTS == slots0[LIST_GROUPS["near2048"]] and (lo[LIST_GROUPS["far_b"]], hi[LIST_GROUPS["far_b"]]) == (-32768, 32767)
    assert np.delete(slots0, fa).max() == MAX_SLOTS
    if neighbour is None:
        assert (slots0[fa], lo[fa], hi[fa]) == (MAX_SLOTS, -32768, 32767)
        assert (f["window"], f["win_slots"], f["win_near16"], f["kernel"]) == (2, MAX_SLOTS, 0, "jagw_list")
    else:
        assert (slots0[fa], lo[fa], hi[fa]) == {"2049": (2049, -32768, 32767), "-32769": (2048, -32769, 32767), "+32768": (2048, -32768, 32768)}[neighbour]
        assert (f["window"], f["c16"], f["kernel"]) == (0, 0, "jagd")
    return _done(P, f, values, seed)


# ---- the cases by name: (generator, its arguments, the BICG_PLAN switches the case is planned and run under) -----------------------------
SMALL = {}
for _k in (63, 64, 65):
    SMALL[f"runs{_k}"] = (runs, (_k,), {})
for _w in (2040, 2048, 2049):
    SMALL[f"slots{_w}"] = (slots, (_w,), {})
SMALL["lengths_jagw"] = (lengths, ("jagw",), {})
SMALL["lengths_jagd"] = (lengths, ("jagd",), {"window": 0})
for _m in (255, 256):
    SMALL[f"longrow{_m}"] = (longrow, (_m,), {})
for _t in (1, 63, 64, 65, 128, 129, 192, 193, 255):
    SMALL[f"tail{_t}"] = (tail, (_t,), {})
SMALL["far32"] = (far32, (True,), {})
SMALL["far32_near"] = (far32, (False,), {})
SMALL["jpipe960"] = (jpipe_edge, (960,), {})
SMALL["jpipe961"] = (jpipe_edge, (961,), {})
SMALL["jpipe960_slots2048"] = (jpipe_edge, (960, 2048), {})
CASES = dict(SMALL, list_limits=(list_limits, (), {}))


def build(name, values="generic", seed=0):
    """(CSR, facts, switches) of a case of CASES"""
    gen, args, sw = CASES[name]
    A, facts = gen(*args, values=values, seed=seed)
    return A, facts, dict(sw)
