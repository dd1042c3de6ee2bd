"""Crafted matrices that sit ON the plan limits of the multi-vector products over PADDED slices with 16-bit column offsets
(k_spmm_pipe<OFFD, 512 | 256>, csrc/bicg_spmm.hip; k_spmm_win<0, OFFD, 8 | 4> and k_spmm_sell<LAY_PAD16 | LAY_PAD32, OFFD>,
csrc/bicg_spmm_sell.hip) and of the fused-window cluster plan that decides between them (column_offsets_and_clusters,
csrc/bicg_sell_plan.cpp) -- a plain helper of tests/test_padded_limits.py (CPU: the plan of every case is what this file promises),
tests/test_padded_limits_gpu.py and tests/mp_padded_workers.py. Plain numpy: no library call in here.

build(name, values, seed) returns (synth.CSR, facts, switches). `facts` is worked out here from the matrix alone (`plan_facts`):
    offsets     the sorted distinct distances column - row, together with 0
    c16         every |distance| <= 32767: 16-bit offsets (else 32-bit columns, no clusters)
    clusters    [(lo, hi)]: the offsets split where a gap is greater than 512 -- none when that gives more than 4 of them, or when
                W256 = sum(256 + hi - lo), the slots of a 256-row group's window, is greater than 2048
    W256        that sum (0 without clusters)
    empty_rows  rows without an entry
and `spmm_kind(facts, ...)` mirrors which kernel a pass runs, with which tile or how many vectors per window.

The limits (every one with a case on either side of it; CASES):
    gap between clusters        <= 512 one cluster, 513 two
    clusters                    4, with 5 no cluster plan: the row-major kernel
    window of a 256-row group   W256 <= 2048, 2049: no cluster plan
    pipeline, T-row tile        every lo'_k > hi'_{k-1} + T and sum(T + hi' - lo') <= 2048 (T = 512) / 1536 (T = 256), where
                                lo' = lo & ~1 and hi' = (hi + 1) & ~1 (16-byte copies: even distances, even counts)
    windowed kernel             8 vectors per window while 8 W256 doubles fit 80 KB (W256 <= 1280), else 4
    16-bit offsets              +-32767; 32768: 32-bit columns (LAY_PAD32)
    tiles per workgroup         more tiles than resident workgroups (512 of 512 rows, 768 of 256 rows): `walk`

Values on one pattern (`values=`): "generic" standard normal; "integer" from {1, 2, 3} (tests/ragged_cases.py's laws). `seed` picks
another draw on the same pattern. Entries of a row are in ascending column order."""
from __future__ import annotations

import functools

import numpy as np

from ragged_cases import Pattern

GROUP, SLICE = 256, 64
GAP, MAX_CLUSTERS, MAX_WINDOW = 512, 4, 2048            # column_offsets_and_clusters (kFwMaxClusters)
PIPE_SLOTS = {512: 2048, 256: 1536}                     # 2 x StageShape<T>::J x T: the 16-byte pairs a thread stages per vector
PIPE_RESIDENT = {512: 512, 256: 768}                    # SPMM_RESIDENT512, SPMM_RESIDENT
WIN8_SLOTS = 1280                                       # 8 vectors x 1280 slots x 8 bytes = 80 KB
FACT_KEYS = ("c16", "clusters")                         # entries of hipsolver.SELL_SUMMARY the facts name (clusters: how many)


# ---- the plan's decisions, from the matrix alone -----------------------------------------------------------------------------------------
def plan_facts(P):
    """the facts of a one-rank block whose rows are all on the sliced-ELL path in padded slices, from its pattern"""
    dist = np.unique(np.append(P.col - P.row, 0)).astype(np.int64)
    c16 = int(len(P.col) > 0 and dist.min() >= -32767 and dist.max() <= 32767)
    clusters = []
    if c16:
        cut = np.flatnonzero(np.diff(dist) > GAP)
        first, last = np.append(0, cut + 1), np.append(cut, len(dist) - 1)
        clusters = [(int(dist[a]), int(dist[b])) for a, b in zip(first, last)]
    W256 = sum(GROUP + hi - lo for lo, hi in clusters)
    if len(clusters) > MAX_CLUSTERS or W256 > MAX_WINDOW:
        clusters = []
    return dict(offsets=dist.tolist(), c16=c16, clusters=len(clusters), cluster_list=clusters,
                W256=sum(GROUP + hi - lo for lo, hi in clusters), empty_rows=np.flatnonzero(P.lens == 0),
                max_row=int(P.lens.max()), rows=P.n)


def rounded(clusters):
    """the clusters as the pipeline lays them out: even first distance (rounded towards minus infinity), even count"""
    return [(lo & ~1, (hi + 1) & ~1) for lo, hi in clusters]


def pipe_slots(clusters, T):
    return sum(T + hi - lo for lo, hi in rounded(clusters))


def pipe_fits(clusters, T):
    """spmm_pipe_plan(.., T, ..): the runs of two clusters do not meet within a tile, and a thread's pairs cover the window"""
    r = rounded(clusters)
    apart = all(r[k][0] > r[k - 1][1] + T for k in range(1, len(r)))
    return bool(r) and apart and pipe_slots(clusters, T) <= PIPE_SLOTS[T]


def spmm_kind(facts, spmm_window=None, spmm_tile=None):
    """(kind, tile, vectors per window) of a pass over a padded block with these facts -- the kernel hipsolver.Context.last_spmm_kind()
    names, last_spmm_tile(), and the NV of k_spmm_win -- under BICG_PLAN="spmm-window=" and BICG_TEST="spmm-tile=". Read in:
      spmm_pass (csrc/bicg_solver.cpp): the window is fw.slots = W256 doubles per vector when the block has 16-bit offsets, padded
        slices and clusters, else 0; spmm-window=0 or spmm_win_vectors(0) = 0: k_spmm_sell ("rowmajor": LAY_PAD16 with c16, else
        LAY_PAD32); spmm-window=1: k_spmm_win; default (3): launch_spmm_pipe first, k_spmm_win where it refuses.
      launch_spmm_pipe (csrc/bicg_spmm.hip): tile = 512 unless spmm-tile=256; 512 refused by spmm_pipe_plan: 256; 256 refused:
        hipErrorInvalidValue (a forced 256 is never retried at 512).
      spmm_pipe_plan (same file): lo' = lo & ~1, hi' = (hi + 1) & ~1; refuses when lo'_k <= hi'_{k-1} + tile or when
        sum(tile + hi' - lo') > 2 * StageShape<tile>::J * tile (2048 / 1536). Its last test -- two buffers of 2 vectors of slots + 2
        doubles within 158 KB -- cannot bind: 4 * 2050 * 8 = 65 600 bytes at most.
      spmm_win_vectors (csrc/bicg_spmm_sell.hip): 8 vectors when 8 * wslots * 8 <= 80 KB, i.e. W256 <= 1280, else 4 (4 * 2048 * 8
        = 64 KB always fits)."""
    cl = facts["cluster_list"]
    if not cl or spmm_window == 0:
        return ("rowmajor", 0, 0)
    nv = 8 if facts["W256"] <= WIN8_SLOTS else 4
    if spmm_window == 1:
        return ("windowed", 0, nv)
    T = 256 if spmm_tile == 256 else 512
    if T == 512 and not pipe_fits(cl, 512):
        T = 256
    if not pipe_fits(cl, T):
        return ("windowed", 0, nv)
    return ("pipelined", T, 0)


def row_layout(facts):
    """the layout k_spmm_sell is instantiated for: sell_layout() of padded slices"""
    return "LAY_PAD16" if facts["c16"] else "LAY_PAD32"


def pipe_ownership(rows, T, gstep=None):
    """tiles per workgroup of k_spmm_pipe, from spmm_pipe_shape and the kernel's first lines (csrc/bicg_spmm.hip): -> (grid, the list
    of tiles each workgroup takes, in its order). Default: grid = the tiles rounded up to 8 while they are at most the resident
    workgroups, else those; XCD x = workgroup % 8 owns tiles x per .. (x + 1) per - 1, per = ceil(tiles / 8), and its workgroup
    j = workgroup / 8 takes x per + j, + grid / 8, ... gstep (BICG_TEST="spmm-gstep=", thousandths; >= 1000): s = gstep / 1000,
    g = floor(tiles / s) + 1 lowered while (g - 1) s >= tiles, grid = g rounded up to 8; virtual workgroup vb = (b % 8)(grid / 8) +
    b / 8 takes the consecutive tiles floor(vb s) .. floor((vb + 1) s) - 1, capped at the last tile."""
    ntiles = -(-rows // T)
    own = []
    if gstep is not None and gstep >= 1000:
        s = 1e-3 * gstep
        g = int(ntiles / s) + 1
        while (g - 1) * s >= ntiles:
            g -= 1
        grid = (g + 7) & ~7
        for b in range(grid):
            vb = (b % 8) * (grid // 8) + b // 8
            first, upto = int(vb * s), (vb + 1) * s
            end = ntiles if upto >= ntiles else int(upto)
            own.append(list(range(first, end)))
        return grid, own
    grid = (ntiles + 7) & ~7 if ntiles <= PIPE_RESIDENT[T] else PIPE_RESIDENT[T]
    per = -(-ntiles // 8)
    for b in range(grid):
        xcd, j = b % 8, b // 8
        own.append(list(range(xcd * per + j, min((xcd + 1) * per, ntiles), grid // 8)))
    return grid, own


# ---- patterns ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _banded(n, offsets):
    """one entry per offset in every row, clipped to the matrix (synth.from_offsets' pattern)"""
    offs = np.array(sorted(offsets), dtype=np.int64)
    rows = np.arange(n, dtype=np.int64)
    cols = rows[:, None] + offs[None, :]
    ok = (cols >= 0) & (cols < n)
    P = Pattern(n, np.broadcast_to(rows[:, None], cols.shape)[ok], cols[ok], presorted=True)
    return P, plan_facts(P)


LENGTHS = (1, 4, 5, 8, 9, 16, 17, 24, 25, 33, 0, 7)      # one 64-row slice each: both halves of the head of 16, the streamed batches of 8
LENGTHS_TAIL = (37, 11)                                  # then a partly filled slice: rows, length


LENGTHS_ROWS = len(LENGTHS) * SLICE + LENGTHS_TAIL[0]


@functools.lru_cache(maxsize=None)
def _lengths(copies=1):
    """copies > 1: that many blocks of LENGTHS_ROWS rows below each other, each laid out like the first from ITS first row on; the
    rows at the end of a block reach into the next one (clipped only at the end of the matrix)"""
    m, n = LENGTHS_ROWS, LENGTHS_ROWS * copies
    lens = np.zeros(m, dtype=np.int64)
    special = {}
    for s, L in enumerate(LENGTHS + (LENGTHS_TAIL[1],)):
        r0, nr = s * SLICE, min(SLICE, m - s * SLICE)
        lens[r0:r0 + nr] = L
        if L > 2:          # a row with a single entry, one without entries, one that is one entry short of the slice
            special[s] = (r0 + 2 + s % 5, r0 + 20 + s % 7, r0 + 9 + s % 3)
            lens[list(special[s])] = 1, 0, L - 1
    lens = np.tile(lens, copies)
    lens = np.minimum(lens, (n - 1 - np.arange(n)) // 2 + 1)          # distances 0, 2, 4, ... to the right, clipped to the matrix
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    col = row + 2 * (np.arange(len(row)) - ptr[row])
    P = Pattern(n, row, col, presorted=True)
    f = plan_facts(P)
    for c in range(copies):          # the slices of every block, counted from the block's first row
        slice_max = [int(P.lens[c * m + s:min(c * m + s + SLICE, (c + 1) * m)].max()) for s in range(0, m, SLICE)]
        assert tuple(slice_max) == LENGTHS + (LENGTHS_TAIL[1],), slice_max
        for s, (one, none, short) in special.items():
            assert (P.lens[c * m + one], P.lens[c * m + none], P.lens[c * m + short]) == (1, 0, slice_max[s] - 1)
    assert f["clusters"] == 1 and f["cluster_list"] == [(0, 64)] and f["W256"] == 320
    f["slices"] = slice_max
    return P, f


# ---- the cases by name: (rows, offsets, the BICG_PLAN switches the case is planned and run under) -------------------------------------------
WALK_ROWS = 512 * 512 + 3 * 512 + 77
TRI_ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4096, 4097)
BANDED = {
    "gap512": (5000, (-1, 0, 512)),
    "gap513": (5000, (0, 513)),
    "gap514_even": (5000, (0, 514)),
    "gap514_odd": (5000, (0, 1, 515)),
    "clusters4": (9000, (-1200, -600, 0, 1800)),          # (both sides of the diagonal: across ranks, halo on both sides)
    "clusters4_odd": (9000, (-1200, -601, 0, 1800)),
    "clusters5": (9000, (-1200, -600, 0, 1800, 2400)),
    "pipe1536": (9000, (0, 256, 1000, 1256, 2000, 2256)),
    "pipe1538": (9000, (0, 256, 1000, 1256, 2000, 2257)),
    "slots2048": (12000, (0, 256, 1000, 1256, 2000, 2256, 3000, 3256)),
    "slots2049": (12000, (0, 257, 1000, 1256, 2000, 2256, 3000, 3256)),
    "win1280": (5000, (0, 512, 1024)),
    "win1281": (5000, (0, 512, 1024, 1025)),          # (a span of 1025 in gaps of at most 512 takes four offsets)
    "far32767": (70001, (-32767, 0, 32767)),
    "far32768": (70001, (-32767, 0, 32768)),
    "walk": (WALK_ROWS, (-600, -1, 0, 1, 600)),
}
BANDED.update({f"tri{n}": (n, (-1, 0, 1)) for n in TRI_ROWS})
CASES = list(BANDED) + ["lengths"]
SMALL = [c for c in CASES if c != "walk"]
# Across three ranks (equal row ranges, no multiples of 64): `lengths` itself cannot be cut that way -- a cut inside its slices pairs rows
# of different lengths in one slice of the rank's block, the padding passes what the plan accepts (a quarter of the group's
# entries + 128) and the rank's rows go to CSR row blocks, which have no SpMM kernel. `lengths_x3` is three such blocks below each
# other: every rank's diag block IS the pattern of `lengths`, its last rows with entries in the next rank's columns.
RANK_CASES = ("clusters4_odd", "lengths_x3")


def pattern(name):
    """(Pattern, facts, switches) of a case"""
    if name in ("lengths", "lengths_x3"):
        P, f = _lengths(3 if name == "lengths_x3" else 1)
        return P, f, {"layout": "pad"}
    P, f = _banded(*BANDED[name])
    return P, f, {}


def build(name, values="generic", seed=0):
    """(CSR, facts, switches) of a case of CASES"""
    P, f, sw = pattern(name)
    return P.csr(values, seed), dict(f), dict(sw)


# ---- the integer systems behind the exact residual norms ------------------------------------------------------------------------------------
MAX_VECTORS = 17


@functools.lru_cache(maxsize=None)
def integer_system(name):
    """(A, facts, switches, X [17][n], sigma [17], b, the exact relative residual norms [17]) for the integer values of a case"""
    A, facts, sw = build(name, "integer")
    n = A.rows
    assert set(np.unique(A.val)) <= {1.0, 2.0, 3.0}
    rng = np.random.default_rng(4000)
    X = rng.integers(1, 4, size=(MAX_VECTORS, n))
    b = rng.integers(1, 4, size=n)
    sigma = np.arange(1, MAX_VECTORS + 1)
    row, col, _ = A.to_coo()
    row, col, ival = row.astype(np.int64), col.astype(np.int64), A.val.astype(np.int64)
    bb = int((b * b).sum())
    assert 0 < bb < 2 ** 53
    want = np.zeros(len(X))
    for j in range(len(X)):
        terms = ival * X[j][col]
        assert int(terms.sum()) < 2 ** 53          # (so the float64 weights below add up exactly)
        Ax = np.bincount(row, weights=terms.astype(np.float64), minlength=n).astype(np.int64)
        res = b - (Ax + int(sigma[j]) * X[j])
        sq = int((res * res).sum())                # (int64: |res| < 2^20, fewer than 2^20 rows)
        assert int(np.abs(res).max()) < 2 ** 20 and n < 2 ** 20 and 0 <= sq < 2 ** 53
        want[j] = np.sqrt(np.float64(sq) / np.float64(bb))          # the expression in bicg_shifted_residuals
    out = (X.astype(np.float64), sigma.astype(np.float64), b.astype(np.float64), want)
    for a in out:
        a.setflags(write=False)
    return (A, facts, sw) + out
