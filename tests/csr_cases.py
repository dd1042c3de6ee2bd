"""Crafted matrices that sit ON the plan limits of the two products that read the CSR arrays as they are (csrc/bicg_spmv_csr.hip):
k_spmv_rows (rows over lanes) and k_spmv (row-block stream) -- a plain helper of tests/test_csr_limits.py (CPU: the plan of every
case is what this file promises), tests/test_csr_limits_gpu.py and tests/mp_csr_workers.py. Plain numpy: no library call in here.

Every generator returns (synth.CSR, facts). `facts` is what the sliced-ELL plan must report for the one-rank matrix -- the entries
of hipsolver.SELL_SUMMARY named in FACT_KEYS --, "blocks" (the row-block descriptors {first row, end row, first nnz, end nnz}, an
int64 array [nblk][4]), "kernels" (what hipsolver.product_kernels() must name) and "empty_groups" (256-row groups without an entry).
They are worked out here from the pattern alone by `plan_facts`, the rules as csrc/bicg_sell_plan.cpp documents them:

    rows over lanes   the mean row length nnz / rows (integer division) is >= 256, or >= 128 with fewer than 512 groups of 256 rows.
                      No group is sliced; the row blocks are the greedy blocks of at most 8192 non-zeros and 256 rows over the whole
                      matrix; 16-bit column offsets (csr16) when every |col - row| <= 32767 -- a symmetric range -- and col16 is on.
    otherwise         jagged slices when padding every 64-row slice to its longest row would add more than 2 %. A group leaves the
                      sliced-ELL path when one of its slices holds a row longer than max(64, 4 nnz / rows); ALL groups leave it when
                      fewer than half of the rows sit in groups that stay. Row blocks: the greedy blocks of at most 2044 non-zeros
                      (kRowBlockNnz) and 1024 rows over every maximal run of groups off the sliced path, never across two runs.
    greedy blocks     `row_blocks`: a block takes at least one row, then rows while it stays within the two limits
                      (bicg_row_blocks, csrc/bicg_plan.cpp).

In the kernels: k_spmv_rows spreads a row over T lanes, T from the block's integer mean nnz / rows (>= 320: 64, >= 160: 32, >= 80: 16,
else 8; `lanes_of`), 256 / T rows per pass; k_spmv stages a block of at most 2048 non-zeros (kChunk) in LDS and adds every row in
stored order -- the oracle's mult() bit for bit --, and reduces a single row of more than 2048 with strided partial sums
(`strided_rows`: another association).

Rows hold a contiguous run of columns around their diagonal (clipped at the matrix edges), so every row with an entry stores its
diagonal; the far16 cases add single entries +-32767 / 32768 columns away. Values on one pattern (`values=`) as in
tests/ragged_cases.py: "generic", "integer" from {1, 2, 3}; "dominant" is scaled row by row (`_done`); `seed` picks another draw
on the same pattern.

`rows_model` is the float64 restatement of the association k_spmv_rows promises; `exact_row_sums` and
`abs_row_sums` are what tests/test_csr_limits.py measures it against."""
from __future__ import annotations

import functools
import math

import numpy as np

from ragged_cases import Pattern

GROUP, SLICE = 256, 64
ROWS_CHUNK, ROWS_MAX_ROWS = 8192, 256          # row blocks of k_spmv_rows
STREAM_CHUNK, STREAM_MAX_ROWS = 2044, 1024     # ... of k_spmv (kRowBlockNnz; the 1024-row cap)
STAGED = 2048                                  # kChunk: a block of more non-zeros is one row, reduced with strided partial sums
FACT_KEYS = ("rowsplit", "jag", "nblk", "csr16", "sell_rows", "n_bnd", "window", "lane_info")


# ---- the plan's decisions, from the pattern alone ---------------------------------------------------------------------------------------
def row_blocks(ptr, r0, r1, chunk, max_rows):
    """the greedy row blocks over rows r0 .. r1 - 1 as (first row, end row) pairs"""
    out, r = [], r0
    ptr = [int(p) for p in ptr]
    while r < r1:
        start, base = r, ptr[r]
        r += 1
        while r < r1 and r - start < max_rows and ptr[r + 1] - base <= chunk:
            r += 1
        out.append((start, r))
    return out


def descriptors(ptr, pairs):
    return np.array([(a, b, int(ptr[a]), int(ptr[b])) for a, b in pairs], dtype=np.int64).reshape(-1, 4)


def lanes_of(desc):
    """T of every row block of k_spmv_rows, from the integer mean of its row lengths"""
    rows, nnz = desc[:, 1] - desc[:, 0], desc[:, 3] - desc[:, 2]
    mean = nnz // np.maximum(rows, 1)
    return np.where(mean >= 320, 64, np.where(mean >= 160, 32, np.where(mean >= 80, 16, 8)))


def block_means(desc):
    return (desc[:, 3] - desc[:, 2]) // (desc[:, 1] - desc[:, 0])


def plan_facts(ptr, col, n, col16=1):
    """FACT_KEYS (but "window" and "lane_info", which a case with sliced groups sets itself), "blocks", "sliced" (which groups stay
    on the sliced-ELL path) and "empty_groups" of the one-rank block with row pointers ptr and columns col"""
    ptr = np.asarray(ptr, dtype=np.int64)
    lens = np.diff(ptr)
    nnz, ng = int(ptr[-1]), -(-n // GROUP)
    mean = nnz // n
    rowsplit = mean >= 256 or (mean >= 128 and ng < 512)
    slice_max = np.array([int(lens[s:s + SLICE].max()) for s in range(0, n, SLICE)])
    padded = sum(int(slice_max[i]) * len(lens[s:s + SLICE]) for i, s in enumerate(range(0, n, SLICE)))
    jag = padded > nnz + nnz // 50
    sliced = np.zeros(ng, dtype=bool)
    if rowsplit:
        pairs = row_blocks(ptr, 0, n, ROWS_CHUNK, ROWS_MAX_ROWS)
    else:
        assert jag, "the stream cases have ragged rows"
        limit = max(64, 4 * nnz // n)
        per_group = GROUP // SLICE
        fits = np.array([slice_max[g * per_group:(g + 1) * per_group].max() <= limit for g in range(ng)])
        rows_of = np.minimum(n, (np.arange(ng) + 1) * GROUP) - np.arange(ng) * GROUP
        if 2 * int(rows_of[fits].sum()) >= n:
            sliced = fits
        pairs, g = [], 0
        while g < ng:
            if sliced[g]:
                g += 1
                continue
            g1 = g
            while g1 < ng and not sliced[g1]:
                g1 += 1
            pairs += row_blocks(ptr, g * GROUP, min(n, g1 * GROUP), STREAM_CHUNK, STREAM_MAX_ROWS)
            g = g1
    desc = descriptors(ptr, pairs)
    rows_of = np.minimum(n, (np.arange(ng) + 1) * GROUP) - np.arange(ng) * GROUP
    csr16 = 0
    if rowsplit and len(desc) and col16:
        row = np.repeat(np.arange(n, dtype=np.int64), lens)
        csr16 = int(np.abs(np.asarray(col, dtype=np.int64) - row).max() <= 32767)
    group_nnz = np.add.reduceat(np.append(lens, 0), np.arange(ng) * GROUP)
    return dict(rowsplit=int(rowsplit), jag=int(jag), nblk=len(desc), csr16=csr16, sell_rows=int(rows_of[sliced].sum()), n_bnd=0,
                window=0, lane_info=0, blocks=desc, sliced=sliced, empty_groups=np.flatnonzero(group_nnz == 0).tolist())


def strided_rows(facts):
    """rows of a stream case that k_spmv reduces with strided partial sums: blocks of more than 2048 non-zeros (one row each)"""
    d = facts["blocks"]
    big = d[:, 3] - d[:, 2] > STAGED
    assert np.all(d[big, 1] - d[big, 0] == 1)
    return d[big, 0]


def fnv1a(desc):
    """64-bit FNV-1a over the descriptors as an array of four 32-bit words each (sell_plan_digest, csrc/bicg_sell_plan.cpp)"""
    h = 0xcbf29ce484222325
    for byte in np.ascontiguousarray(desc, dtype=np.uint32).tobytes():
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- the reference models -------------------------------------------------------------------------------------------------------------
def rows_model(A, desc, x, lanes=None):
    """y = A x as k_spmv_rows promises it (the comment above lanes_sum in csrc/bicg_spmv_csr.hip), in float64
    numpy: per row block T = lanes_of; per row T lane sums start at +0.0, lane l adds fl(a x) of the row's entries l, l + T, l + 2T, ...
    in stored order; the lane sums are combined by repeated s[0::2] + s[1::2] -- the xor-1 / 2 / 4 / 8 / 16 / 32 butterfly is this
    balanced tree because IEEE addition commutes --; y = 0.0 + that sum. (A lane past the row's end adds +-0.0 products to a sum
    that is never -0.0: they change no bit, and the model leaves them out.)"""
    ptr = A.ptr.astype(np.int64)
    prod = A.val * np.asarray(x, dtype=np.float64)[A.col.astype(np.int64)]          # one rounding per product
    prod = np.append(prod, 0.0)                                                  # (index nnz: a lane without an entry)
    y = np.zeros(A.rows)
    override, lanes = lanes or {}, lanes_of(desc)
    for b, t in override.items():                  # (tests/test_csr_limits.py: what a kernel with another T would give)
        lanes[b] = t
    for T in (8, 16, 32, 64):
        mine = desc[lanes == T]
        if not len(mine):
            continue
        rows = np.concatenate([np.arange(a, b) for a, b in mine[:, :2]])
        start, end = ptr[rows], ptr[rows + 1]
        s = np.zeros((len(rows), T))
        lane = np.arange(T, dtype=np.int64)
        k, live = 0, np.arange(len(rows))
        while len(live):
            j = start[live, None] + k * T + lane[None, :]
            s[live] += prod[np.where(j < end[live, None], j, len(prod) - 1)]
            k += 1
            live = live[end[live] - start[live] > k * T]
        while s.shape[1] > 1:
            s = s[:, 0::2] + s[:, 1::2]
        y[rows] = 0.0 + s[:, 0]
    return y


def _two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker's product with Veltkamp's split; no overflow at these magnitudes)"""
    p = a * b
    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi
    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def exact_row_sums(A, x):
    """the correctly rounded row sums of A x: math.fsum over the exact products, each as its two-term expansion"""
    ptr = A.ptr.astype(np.int64)
    p, e = _two_product(A.val, np.asarray(x, dtype=np.float64)[A.col.astype(np.int64)])
    return np.array([math.fsum(np.concatenate((p[a:b], e[a:b]))) for a, b in zip(ptr[:-1], ptr[1:])])


def abs_row_sums(A, x):
    """sum_j |a_ij x_j| per row (numpy's pairwise sum: a scale, good to a few ulp)"""
    ptr = A.ptr.astype(np.int64)
    t = np.abs(A.val * np.asarray(x, dtype=np.float64)[A.col.astype(np.int64)])
    return np.array([t[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])])


# ---- patterns --------------------------------------------------------------------------------------------------------------------------
def _windows(lens, extra=()):
    """row r holds lens[r] consecutive columns around r (clipped to the matrix), plus the (row, column) pairs of `extra`"""
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    assert lens.max() <= n
    start = np.clip(np.arange(n) - lens // 2, 0, n - lens)
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    col = start[row] + (np.arange(len(row)) - ptr[row])
    if len(extra):
        er, ec = np.array(extra, dtype=np.int64).T
        key = np.sort(np.concatenate((row * (1 << 32) + col, er * (1 << 32) + ec)))
        assert len(np.unique(key)) == len(key)
        row, col = key >> 32, key & 0xFFFFFFFF
    return Pattern(n, row, col, presorted=True)


def _spread(rng, rows, total, lo=1, first=None):
    """`rows` row lengths >= lo that add up to `total`, ragged; first: the length of the first row"""
    assert rows >= 1
    if first is not None:
        if rows == 1:
            assert first == total
            return np.array([first], dtype=np.int64)
        return np.append(first, _spread(rng, rows - 1, total - first, lo))
    base = total // rows
    assert base >= lo
    lens = np.full(rows, base, dtype=np.int64)
    lens[:total - base * rows] += 1
    for _ in range(2 * rows):                      # move entries between pairs of rows
        i, j = rng.integers(0, rows, size=2)
        d = int(rng.integers(0, max(1, (lens[j] - lo) // 2 + 1)))
        if i != j and lens[i] + d <= base + base // 2:      # (no row grows past 1.5 x the mean)
            lens[i] += d; lens[j] -= d
    assert lens.sum() == total and lens.min() >= lo
    return lens


def _rows_case(blocks, extra=()):
    """pattern and facts of a rows-over-lanes case given as a list of row blocks (each an array of row lengths); asserts that the plan
    cuts exactly these blocks"""
    lens = np.concatenate(blocks)
    P = _windows(lens, extra)
    f = plan_facts(P.ptr, P.col, P.n)
    edges = np.cumsum([0] + [len(b) for b in blocks])
    assert f["rowsplit"] == 1 and f["sell_rows"] == 0, (int(P.ptr[-1]) // P.n, P.n)
    assert np.array_equal(f["blocks"][:, 0], edges[:-1]) and np.array_equal(f["blocks"][:, 1], edges[1:]), "the plan cuts other blocks"
    f["kernels"] = ["rows"]
    return P, f


def _heavy(rng, count, rows=16, total=ROWS_CHUNK):
    """`count` row blocks of exactly 8192 non-zeros: they lift the matrix's mean row length over 128 and close the block before"""
    return [_spread(rng, rows, total, lo=total // rows // 2) for _ in range(count)]


@functools.lru_cache(maxsize=None)
def _t_edges():
    rng = np.random.default_rng(10)
    want = (79, 80, 159, 160, 319, 320)
    shape = {79: (100, 7999), 80: (100, 8000), 159: (51, 8159), 160: (51, 8160), 319: (25, 7999), 320: (25, 8000)}
    # every block opens with a row of 200: 200 more than any block's total passes 8192, so the block before ends where it should
    blocks = [_spread(rng, *shape[m], lo=20, first=200) for _ in range(2) for m in want]
    P, f = _rows_case(blocks)
    assert tuple(block_means(f["blocks"])) == want * 2
    assert tuple(lanes_of(f["blocks"])) == (8, 16, 16, 32, 32, 64) * 2
    return P, f


def t_edges(values="generic", seed=0):
    """consecutive row blocks whose integer mean row length is 79, 80, 159, 160, 319 and 320 (twice): T = 8 | 16, 16 | 32 and
    32 | 64 on both sides of each threshold"""
    return _done(*_t_edges(), values, seed)


@functools.lru_cache(maxsize=None)
def _batch_edges():
    rng = np.random.default_rng(11)
    blocks, at = [], {}
    # (T, rows, total): the block's mean selects T; its first row is its longest special one, long enough to close the block before
    for T, rows, total in ((64, 20, 8000), (32, 40, 8100), (16, 70, 8150), (8, 150, 8150)):
        special = [8 * T + 1, 8 * T - 1, 8 * T, 1, 0, T - 1]
        rest = _spread(rng, rows - len(special), total - sum(special), lo=2)
        mid = len(rest) // 2
        blocks.append(np.concatenate((special[:3], rest[:mid], special[3:], rest[mid:])).astype(np.int64))
        at[T] = len(blocks) - 1
    blocks += _heavy(rng, 12) + _heavy(rng, 20, rows=32)
    P, f = _rows_case(blocks)
    T = lanes_of(f["blocks"])
    for t, b in at.items():
        a0, a1 = f["blocks"][b, :2]
        assert T[b] == t and {8 * t - 1, 8 * t, 8 * t + 1, 1, 0, t - 1} <= set(P.lens[a0:a1].tolist())
    return P, f


def batch_edges(values="generic", seed=0):
    """for T = 64, 32, 16 and 8 one row block that holds rows of 8T - 1, 8T, 8T + 1 (one batch of 8 per lane, and its neighbours),
    1, 0 and T - 1 entries"""
    return _done(*_batch_edges(), values, seed)


ODD_ROWS = ((64, 3), (64, 5), (32, 7), (32, 9), (16, 15), (16, 17), (8, 31), (8, 33), (8, 255))


@functools.lru_cache(maxsize=None)
def _odd_rows():
    rng = np.random.default_rng(12)
    mean = {64: 400, 32: 200, 16: 100, 8: 30}
    one = np.array([ROWS_CHUNK], dtype=np.int64)          # a row of 8192: a block of one row, and nothing fits beside it
    # mean 150: T = 16, 16 rows per pass, 54 = 3 passes + 6 rows
    blocks = [one] + [_spread(rng, 54, 8150, lo=100) for _ in range(74)] + [one]
    for T, rows in ODD_ROWS:                                            # (in the middle: of three equal row ranges the second holds them)
        blocks += [_spread(rng, rows, mean[T] * rows + rows // 2, lo=mean[T] // 2), one]
    blocks += [_spread(rng, 54, 8150, lo=100) for _ in range(74)]
    blocks += [one, _spread(rng, 17, 1700, lo=50)]                      # the last block: 17 rows with T = 16
    P, f = _rows_case(blocks)
    T, rows = lanes_of(f["blocks"]), f["blocks"][:, 1] - f["blocks"][:, 0]
    seen = set(zip(T.tolist(), rows.tolist()))
    assert set(ODD_ROWS) <= seen and (64, 1) in seen
    assert rows[0] == 1 and (T[-1], rows[-1]) == (16, 17), "lanes without a row in the first and in the last block"
    return P, f


def odd_rows(values="generic", seed=0):
    """row blocks of 1 row, of 256 / T - 1 and 256 / T + 1 rows for every T, and of 255 rows: the last pass of such a block has lanes
    without a row -- in the first block, the last one and in between. Rows of 8192 entries (blocks of their own) separate them."""
    return _done(*_odd_rows(), values, seed)


@functools.lru_cache(maxsize=None)
def _outlier():
    rng = np.random.default_rng(13)
    short = rng.permutation(np.array([2] * 81 + [1] * 28, dtype=np.int64))      # 109 rows, 190 non-zeros
    first = np.concatenate((short[:50], [8000], short[50:]))           # 110 rows, 8190 non-zeros: mean 74, T = 8
    blocks = [first, np.array([8193]), np.array([20011])]
    blocks += [_spread(rng, 63, 8190, lo=100) for _ in range(318)]      # mean 130
    P, f = _rows_case(blocks)
    d, T = f["blocks"], lanes_of(f["blocks"])
    assert (T[0], d[0, 1], d[0, 3]) == (8, 110, 8190) and P.lens[50] == 8000 and -(-8000 // (8 * 8)) == 125
    assert tuple(T[1:3]) == (64, 64) and tuple(d[1:3, 3] - d[1:3, 2]) == (8193, 20011)
    return P, f


def outlier_in_short_block(values="generic", seed=0):
    """one row of 8000 entries among 109 rows of 1 or 2 in ONE block of mean 74 (T = 8: 125 batches of 8 per lane); then single rows
    of 8193 and of 20011 entries, each a block of its own (longer than a block's 8192 non-zeros) with T = 64"""
    return _done(*_outlier(), values, seed)


@functools.lru_cache(maxsize=None)
def _full_blocks():
    rng = np.random.default_rng(14)
    blocks = [np.full(256, 20), np.full(64, 128), np.full(256, 32), _spread(rng, 256, 5000, lo=4)]
    blocks += _heavy(rng, 14) + [np.full(64, 128)] * 4 + _heavy(rng, 4, rows=32)
    blocks = [np.asarray(b, dtype=np.int64) for b in blocks]
    P, f = _rows_case(blocks)
    d = f["blocks"]
    rows, nnz = d[:, 1] - d[:, 0], d[:, 3] - d[:, 2]
    assert (rows[0], nnz[0]) == (256, 5120) and (rows[1], nnz[1]) == (64, 8192) and (rows[2], nnz[2]) == (256, 8192) and rows[3] == 256
    return P, f


def full_blocks(values="generic", seed=0):
    """row blocks of exactly 256 rows (the row cap ends them), of exactly 8192 non-zeros (one more row would pass it), and both at
    once: 256 rows of 32 entries"""
    return _done(*_full_blocks(), values, seed)


FAR_ROWS = 33000


@functools.lru_cache(maxsize=None)
def _far16(far):
    up, down = (100, 100 + 32767), (32900, 32900 - 32767)
    if far == "+32768":
        up = (100, 100 + 32768)
    if far == "-32768":
        down = (32900, 32900 - 32768)
    lens = np.full(FAR_ROWS, 128, dtype=np.int64)
    P = _windows(lens, extra=(up, down))
    f = plan_facts(P.ptr, P.col, P.n)
    dist = P.col - P.row
    assert (int(dist.max()), int(dist.min())) == (up[1] - up[0], down[1] - down[0])
    assert f["rowsplit"] == 1 and int(P.ptr[-1]) // P.n == 128 and f["csr16"] == (far is None)
    assert np.all(lanes_of(f["blocks"]) == 16)
    f["kernels"] = ["rows"]
    return P, f


def near16(values="generic", seed=0):
    """33 000 rows of 128 entries around the diagonal, one entry 32767 columns to the right of its row and one 32767 to the left:
    16-bit offsets in CSR order (csr16), a symmetric range"""
    return _done(*_far16(None), values, seed)


def far32(far="+32768", values="generic", seed=0):
    """near16 with ONE entry one column further, to the right (+32768) or to the left (-32768): 32-bit columns for the whole block"""
    assert far in ("+32768", "-32768")
    return _done(*_far16(far), values, seed)


# ---- row-block stream ------------------------------------------------------------------------------------------------------------------
SINGLE_ROWS = (2044, 2045, 2048, 2049, 2050, 5000)
BATCH_ROWS = (7, 8, 9, 15, 16, 17)                  # finish_row reads the staged products in batches of 8


@functools.lru_cache(maxsize=None)
def _all_blocks():
    rng = np.random.default_rng(20)
    mix = lambda k: rng.integers(0, 3, size=k)
    stretch = np.concatenate((mix(1024), np.zeros(1024, dtype=np.int64), mix(1060)))
    stretch[0] = 2                                                       # (a block opens with an entry)
    specials = np.concatenate((SINGLE_ROWS, np.full(28, 73), [1], BATCH_ROWS, [3])).astype(np.int64)
    body = lambda k: rng.integers(1, 25, size=k)
    lens = np.concatenate((stretch, specials, body(4300)))
    n = len(lens)
    # every group that is not wholly inside the stretch gets one row of 65 .. 114 entries among its ordinary rows
    first_body = len(stretch) + len(specials)
    for g in range(first_body // GROUP + 1, -(-n // GROUP)):
        lens[min(n - 1, g * GROUP + 7 + g)] = 65 + g
    P = _windows(lens)
    f = plan_facts(P.ptr, P.col, P.n)
    nnz = int(P.ptr[-1])
    limit = max(64, 4 * nnz // n)
    assert f["rowsplit"] == 0 and f["jag"] == 1 and limit == 64 and nnz // n < 128
    # the groups of the stretch would stay sliced, every other group holds a row of more than 64 entries; they are fewer than half
    long_groups = np.unique(np.flatnonzero(lens > limit) // GROUP)
    assert set(long_groups.tolist()) == set(range(len(stretch) // GROUP, -(-n // GROUP)))
    assert 2 * (len(stretch) // GROUP) * GROUP < n and f["sell_rows"] == 0 and not f["sliced"].any()
    d = f["blocks"]
    rows, bn = d[:, 1] - d[:, 0], d[:, 3] - d[:, 2]
    assert tuple(rows[:3]) == (1024, 1024, 1024) and bn[1] == 0 and bn[0] <= STREAM_CHUNK and bn[2] <= STREAM_CHUNK, "blocks at the 1024-row cap, one of empty rows only"
    s0 = len(stretch)
    at = {int(a): (int(b - a), int(m)) for a, b, m in zip(d[:, 0], d[:, 1], bn)}
    for i, L in enumerate(SINGLE_ROWS):
        assert at[s0 + i] == (1, L), "every single row is a block of its own"
    k = s0 + len(SINGLE_ROWS)
    assert at[k] == (28, STREAM_CHUNK) and lens[k + 28] == 1, "a block of exactly 2044 non-zeros; its next row would make 2045"
    assert sorted(strided_rows(f).tolist()) == [s0 + 3, s0 + 4, s0 + 5], "2044, 2045 and 2048 are staged; 2049, 2050 and 5000 are not"
    assert bn[bn <= STAGED].max() == 2048 and bn.max() == 5000
    assert set(BATCH_ROWS) <= set(lens.tolist())
    f["kernels"] = ["csr"]
    return P, f


def all_blocks(values="generic", seed=0):
    """no group on the sliced-ELL path (sell_rows = 0): 3108 rows of 0, 1 or 2 entries first -- three blocks at the 1024-row cap, the
    second of them 1024 empty rows --, whose groups would stay sliced but hold fewer than half of the rows; every other group holds a
    row of more than max(64, 4 mean) = 64 entries. Then single rows of 2044, 2045, 2048 (staged: at most 2048 non-zeros), 2049, 2050
    and 5000 entries (strided partial sums), a block of exactly 2044 non-zeros in 28 rows followed by a row of one entry, rows of
    7, 8, 9, 15, 16 and 17 entries, and 4300 rows of 1 .. 24. (1024 consecutive empty rows cover whole groups, which no long row can
    push off the sliced path: the plan's half-of-the-rows rule does.)"""
    return _done(*_all_blocks(), values, seed)


MIXED_CSR_GROUPS = (0, 5, 6, 11)


@functools.lru_cache(maxsize=None)
def _mixed():
    rng = np.random.default_rng(21)
    n = 11 * GROUP + 100
    lens = rng.integers(1, 25, size=n)
    for g in MIXED_CSR_GROUPS:
        lens[g * GROUP + 40 + g] = 300 + g
    P = _windows(lens)
    f = plan_facts(P.ptr, P.col, P.n)
    assert f["rowsplit"] == 0 and f["jag"] == 1 and n % GROUP
    assert np.flatnonzero(~f["sliced"]).tolist() == list(MIXED_CSR_GROUPS) and 2 * f["sell_rows"] >= n
    # three maximal runs -- the first group, two adjacent groups in the middle, the partly filled last group --, no block across two
    runs = [(0, GROUP), (5 * GROUP, 7 * GROUP), (11 * GROUP, n)]
    d = f["blocks"]
    for a, b in d[:, :2]:
        assert sum(lo <= a and b <= hi for lo, hi in runs) == 1
    for lo, hi in runs:
        mine = d[(d[:, 0] >= lo) & (d[:, 1] <= hi)]
        assert mine[0, 0] == lo and mine[-1, 1] == hi and np.array_equal(mine[1:, 0], mine[:-1, 1])
    assert (d[:, 3] - d[:, 2]).max() <= STREAM_CHUNK and len(strided_rows(f)) == 0
    # the sliced groups: one run of consecutive columns per group, rows of at most 24 entries -- a run window and lane words (k_spmv_jagw)
    f.update(window=1, lane_info=1, kernels=sorted(["csr", "jagw"]))
    return P, f


def mixed(values="generic", seed=0):
    """2916 rows of 1 .. 24 entries; groups 0, 5, 6 and 11 (the last, 100 rows) hold a row of about 300 and go to CSR row blocks in
    three maximal runs, the other eight groups stay sliced: every product is two launches"""
    return _done(*_mixed(), values, seed)


# ---- the one-past neighbours of the plan's own thresholds (tests/test_csr_limits.py) ---------------------------------------------------------
def uniform_rows(n, length):
    """n rows of `length` entries each: the mean row length IS `length`"""
    P = _windows(np.full(n, length, dtype=np.int64))
    return P.csr(), plan_facts(P.ptr, P.col, P.n) if length >= 128 else None


def longest_row(extra):
    """1024 ragged rows with a mean of exactly 20 entries -- a row leaves the sliced path when longer than 80 -- whose longest row
    holds 80 + extra"""
    rng = np.random.default_rng(30)
    n = 1024
    lens = _spread(rng, n - 1, 20 * n - 80 - extra, lo=5)
    assert lens.max() < 80
    lens = np.insert(lens, 300, 80 + extra)
    P = _windows(lens)
    assert int(P.ptr[-1]) == 20 * n and max(64, 4 * int(P.ptr[-1]) // n) == 80
    f = plan_facts(P.ptr, P.col, P.n)
    return P.csr(), f


def _done(P, facts, values, seed):
    A = P.csr(values, seed)
    if values == "dominant":
        # Row lengths from 1 to 20 000 would spread the diagonals of ragged_cases' law over four decades, and six iterations on such
        # a system amplify the association of the dot sums beyond any bar (the oracle over 1 and over 5 virtual ranks then differs
        # by 1e-6 and more). Here every row is scaled: its off-diagonal magnitudes add up to less than 1/4, its diagonal is drawn
        # from [1, 9) -- the spectrum is spread enough that six iterations do not reach the rounding floor either.
        # tests/test_csr_limits.py asserts both on the oracle alone.
        row = np.repeat(np.arange(P.n, dtype=np.int64), P.lens)
        on = row == P.col
        d = np.ones(P.n)
        d[row[on]] = A.val[on]
        A.val[:] = 0.25 * A.val / d[row]
        A.val[on] = 1.0 + 8.0 * np.random.default_rng([seed, 4]).random(P.n)[row[on]]
    return A, dict(facts)


# ---- the cases by name: (generator, its arguments, the BICG_PLAN switches the case is planned and run under) -----------------------------
ROWS = {
    "t_edges": (t_edges, (), {}),
    "batch_edges": (batch_edges, (), {}),
    "odd_rows": (odd_rows, (), {}),
    "outlier_in_short_block": (outlier_in_short_block, (), {}),
    "full_blocks": (full_blocks, (), {}),
    "near16": (near16, (), {}),
    "near16_col16_off": (near16, (), {"col16": 0}),
    "far32_plus": (far32, ("+32768",), {}),
    "far32_minus": (far32, ("-32768",), {}),
}
STREAM = {"all_blocks": (all_blocks, (), {}), "mixed": (mixed, (), {})}
CASES = dict(ROWS, **STREAM)


def build(name, values="generic", seed=0):
    """(CSR, facts, switches) of a case of CASES"""
    gen, args, sw = CASES[name]
    A, facts = gen(*args, values=values, seed=seed)
    if sw.get("col16") == 0:
        facts["csr16"] = 0
    return A, facts, dict(sw)
