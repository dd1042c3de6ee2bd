"""Integer test systems whose first BiCGStab iteration is EXACT in floating point, and its reference in Python integers -- a plain
helper of tests/test_exact_dots.py (CPU) and tests/test_dot_groups_gpu.py, tests/mp_dot_workers.py (GPU). The reference is numpy
int64 and Python integers / Fractions; the library appears only in host_blocks, which wraps a rank's arrays for it.

The matrix family is A = 4 I + (U - U^T) with small integer entries: n rows, band offsets +1 and +2 with entries from
{+-1, +-2}, each mirrored with the opposite sign; for every g in `csr_groups` the first row of the 256-row group g carries L more
entries +-1 to one side (the next columns to the right that are no group's first, where L of them exist, else to the left), mirrored as well: that group pads far beyond 25 % and the
plan sends it to the CSR row blocks. b has entries from {-2, -1, 1, 2, 3}, x0 = 0.

Why the first iteration is exact. K = U - U^T is skew: b^T K b = 0, so (b, Ab) = 4 (b, b) -- and since every entry and every
partial sum is an integer below 2^53, also in floating point and under every association of the sum. Hence
    dot_zero = (b, b)                    an integer
    alpha_1  = (b, b) / (b, Ab) = 1/4    exactly
    s = b - Ab/4,  y = A s               exact multiples of 1/4 (s4 = 4 s and y4 = 4 y = A s4 are integer vectors)
    (y, s) = (y4, s4)/16, (y, y) = (y4, y4)/16     exact
    omega_1 = (y, s)/(y, y)              ONE correctly rounded division: float(Fraction((y4, s4), (y4, y4)))
(csrc/bicg_devfn.h, apply_phase: PH_INIT -> dot_zero, PH_PLAIN_ALPHA / PH_INIT_ALPHA -> alpha = rTr / d[0], PH_OMEGA -> omega =
d[0] / d[1]; r = b - A 0 = b.) So dot_zero, the trace's alpha[0] and omega[0] have ONE right answer as bytes whichever finish adds
the partial sums: a missing, doubled or misplaced partial cannot hide behind a tolerance -- provided no partial is zero, which
`preconditions` asserts for the partials of every 256-row group and every CSR row block.

The third dot group of the iteration, (r, r) and (r#, r) of r = s - omega y, is not exact (omega is not a small dyadic number):
`residual_dots` replays it in rational arithmetic and gives derived bounds, see there.

The shifted family (tests/test_shifted_exact_gpu.py, tests/mp_shifted_workers.py) has its own part at the end: `ShiftedFirst`, the
first iteration on A + sigma_seed I in integers, the shift lists and the cases."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np

GROUP = 256          # rows per sliced-ELL group (kGroupRows)
TILE = 512           # elements per workgroup of an element-wise kernel: 256 threads, one pair each
U = Fraction(1, 2 ** 53)


class Matrix:
    """CSR arrays (ptr / col uint32, val float64, rows sorted by column) beside the integer copy the reference works on"""

    def __init__(self, n, ptr, col, ival, csr_groups):
        self.n, self.csr_groups = n, tuple(csr_groups)
        self.ptr, self.col, self.ival = ptr, col, ival
        self.val = ival.astype(np.float64)

    def times(self, v):
        """A v for an int64 vector, in int64 (every caller stays far below 2^62: `preconditions`)"""
        prod = self.ival * v[self.col]
        return np.add.reduceat(prod, self.ptr[:-1].astype(np.int64))       # (no row is empty: the diagonal)

    def block(self, lo, hi):
        """rows lo .. hi - 1 as (diag ptr, diag col, diag val, offd ptr, offd col, offd val): local / global columns, like
        synth.split_blocks"""
        p = self.ptr.astype(np.int64)
        a, b = int(p[lo]), int(p[hi])
        col, val = self.col[a:b].astype(np.int64), self.val[a:b]
        rowid = np.repeat(np.arange(hi - lo), np.diff(p[lo:hi + 1]))
        local = (col >= lo) & (col < hi)
        out = []
        for mask, shift in ((local, lo), (~local, 0)):
            q = np.zeros(hi - lo + 1, dtype=np.int64)
            np.cumsum(np.bincount(rowid[mask], minlength=hi - lo), out=q[1:])
            out += [q.astype(np.uint32), (col[mask] - shift).astype(np.uint32), val[mask].copy()]
        return tuple(out)


@functools.lru_cache(maxsize=None)
def system(n, csr_groups=(), L=600, seed=5):
    """(Matrix, b as int64) of the module docstring"""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [np.arange(n)], [np.arange(n)], [np.full(n, 4, dtype=np.int64)]

    def mirrored(r, c, v):
        rows.extend((r, c)); cols.extend((c, r)); vals.extend((v, -v))
    for off in (1, 2):
        if n > off:
            r = np.arange(n - off)
            mirrored(r, r + off, rng.choice(np.array([-2, -1, 1, 2]), size=n - off))
    for g in csr_groups:
        r0 = GROUP * g
        assert r0 < n
        # (never in the first column of a group: the long row of another group of csr_groups may already hold the mirrored place)
        right, left = np.arange(r0 + 3, n), np.arange(r0 - 3, -1, -1)
        right, left = right[right % GROUP != 0], left[left % GROUP != 0]
        c = right[:L] if len(right) >= L else np.sort(left[:L])
        assert len(c) == L
        mirrored(np.full(L, r0), c, rng.choice(np.array([-1, 1]), size=L))
    rows, cols, vals = (np.concatenate(a).astype(np.int64) for a in (rows, cols, vals))
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    assert not np.any((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])), "two entries in one place"
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    b = rng.choice(np.array([-2, -1, 1, 2, 3]), size=n).astype(np.int64)
    return Matrix(n, ptr.astype(np.uint32), cols.astype(np.uint32), vals, csr_groups), b


class First:
    """the first iteration in integers: bb = (b, b); bAb = (b, Ab); s4 = 4 s; y4 = 4 y; ys = (y4, s4); yy = (y4, y4)"""

    def __init__(self, A, b):
        self.A, self.b = A, b
        self.Ab = A.times(b)
        self.s4 = 4 * b - self.Ab
        self.y4 = A.times(self.s4)
        self.bb, self.bAb = isum(b * b), isum(b * self.Ab)
        self.ys, self.yy = isum(self.y4 * self.s4), isum(self.y4 * self.y4)
        assert self.bAb == 4 * self.bb and self.yy > 0
        self.dot_zero = float(self.bb)
        self.alpha = float(Fraction(self.bb, self.bAb))
        self.omega = float(Fraction(self.ys, self.yy))
        assert self.alpha == 0.25


def isum(v):
    return sum(int(t) for t in v)


@functools.lru_cache(maxsize=None)
def first(n, csr_groups=(), L=600, seed=5):
    return First(*system(n, csr_groups, L, seed))


def row_blocks(ptr, r0, r1, chunk, max_rows):
    """the greedy CSR row blocks over rows r0 .. r1 - 1 (bicg_row_blocks, csrc/bicg_plan.cpp; plan_row_blocks of
    csrc/bicg_sell_plan.cpp calls it per maximal run of groups off the sliced-ELL path): at least one row, then rows while the
    block stays within `chunk` entries and `max_rows` rows"""
    out, r = [], r0
    while r < r1:
        start, base = r, int(ptr[r])
        r += 1
        while r < r1 and r - start < max_rows and int(ptr[r + 1]) - base <= chunk:
            r += 1
        out.append((start, r))
    return out


def producer_units(ptr, n, csr_groups, lo=0, rowsplit=False):
    """row ranges (global rows) whose partial sums ONE workgroup of a product publishes, for the rows lo .. lo + n - 1 of a rank
    whose diag block has the row pointers `ptr`: the 256-row groups on the sliced-ELL path, and the row blocks of every maximal run
    of groups in `csr_groups` (local group numbers). Returns (sliced groups, row blocks)."""
    ng = -(-n // GROUP)
    csr = set(csr_groups)
    sliced = [(lo + g * GROUP, lo + min(n, (g + 1) * GROUP)) for g in range(ng) if g not in csr]
    blocks, g = [], 0
    while g < ng:
        if g not in csr:
            g += 1
            continue
        g1 = g
        while g1 < ng and g1 in csr:
            g1 += 1
        chunk, most = (8192, 256) if rowsplit else (2044, 1024)          # (kRowBlockNnz, csrc/bicg_device.h)
        blocks += [(lo + a, lo + c) for a, c in row_blocks(ptr, g * GROUP, min(n, g1 * GROUP), chunk, most)]
        g = g1
    return sliced, blocks


def preconditions(F, units):
    """what the byte comparison rests on, from the reference alone: every numerator, denominator and sum of absolute terms below
    2^53, and no producer unit (row range) with a zero partial in (b, Ab), (y, s) or (y, y). Returns the smallest |partial|."""
    b, Ab, s4, y4 = F.b, F.Ab, F.s4, F.y4
    for terms in (b * b, b * Ab, y4 * s4, y4 * y4):
        assert isum(np.abs(terms)) < 2 ** 53
    assert max(int(np.abs(v).max()) for v in (Ab, s4, y4)) < 2 ** 26          # products of two entries stay below 2^52
    least = None
    for lo, hi in units:
        assert lo < hi
        for terms in (b[lo:hi] * Ab[lo:hi], y4[lo:hi] * s4[lo:hi], y4[lo:hi] * y4[lo:hi]):
            part = isum(terms)
            assert part != 0, ("a producer's partial sum is zero: the comparison could not miss it", lo, hi)
            least = abs(part) if least is None else min(least, abs(part))
    return least


def same_bytes(got, want):
    """got is the double `want`, bit for bit (a NaN is not, -0.0 is not 0.0)"""
    return np.float64(got).tobytes() == np.float64(want).tobytes()


def residual_dots(F):
    """The iteration's third dot group, from the x/r kernel (FPlainXR, csrc/bicg_vec.hip): r_i = fl(s_i + fl(-omega y_i)),
    dotr = sum fl(r_i r_i), rho = sum fl(b_i r_i) (r# = b), beta = fl(fl(alpha/omega) fl(rho / (b,b))) (PH_PLAIN_END). The replay
    takes omega as the rational it is and forms everything exactly; the bounds are derived, u = 2^-53, t_i = |s_i| + |omega y_i|:

      r_i:   the product costs u |omega y_i|, the sum u (|s_i| + |omega y_i|)(1 + u): |r^_i - r_i| <= 2 u t_i, and |r^_i| <= (1 + 2u) t_i.
      dotr:  |r^_i^2 - r_i^2| = |r^_i - r_i| |r^_i + r_i| <= 2 u t_i (2 + 2u) t_i, the product's rounding adds u (1 + 2u)^2 t_i^2, a
             sum of n terms in ANY order gamma_(n-1) sum fl(r^_i^2) (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2,
             as in tests/test_device_memory_gpu.py): together (n + 4) u sum t_i^2 to first order. Doubling that covers the
             second-order cross terms with room, and the bar of this suite doubles once more and says
                 |dotr - ref| <= 8 (n + 4) u sum t_i^2.
      rho:   the same steps with one factor |b_i| for one t_i: |rho - ref| <= (n + 3) u sum |b_i| t_i to first order; the bar is
                 E_rho = 2 (n + 4) u sum |b_i| t_i.
      beta:  three more roundings, the two quotients and their product: beta = (alpha/omega)(rho/(b,b)) (1 + d)^3, |d| <= u, so
                 |beta - ref| <= |alpha/omega| / (b,b) * (E_rho + 4 u (|rho_ref| + E_rho)).

    `tile_least`: the smallest share of sum r_i^2 that one workgroup of the element-wise kernel contributes -- workgroup w takes
    the element pairs 256 w .. 256 w + 255, workgroup 0 also the single trailing element of an odd n. Where every share is 1000
    dotr bounds and more (tests/test_exact_dots.py asserts it) a lost workgroup moves dotr far beyond the bound."""
    n = len(F.b)
    om = Fraction(F.omega)
    assert om.denominator & (om.denominator - 1) == 0
    p, q = om.numerator, om.denominator
    # 4 q r_i = q s4_i - p y4_i, integers
    r4q = [q * int(s) - p * int(y) for s, y in zip(F.s4, F.y4)]
    t4q = [q * abs(int(s)) + abs(p) * abs(int(y)) for s, y in zip(F.s4, F.y4)]
    scale = 16 * q * q
    dotr = Fraction(sum(r * r for r in r4q), scale)
    rho = Fraction(sum(int(bi) * r for bi, r in zip(F.b, r4q)), 4 * q)
    dotr_bound = 8 * (n + 4) * U * Fraction(sum(t * t for t in t4q), scale)
    e_rho = 2 * (n + 4) * U * Fraction(sum(abs(int(bi)) * t for bi, t in zip(F.b, t4q)), 4 * q)
    ratio = abs(Fraction(F.alpha) / om) / F.bb
    beta = Fraction(F.alpha) / om * rho / F.bb
    beta_bound = ratio * (e_rho + 4 * U * (abs(rho) + e_rho))
    npair = n // 2
    shares = []
    for w in range(max(1, -(-npair // (TILE // 2)))):
        lo, hi = TILE * w, min(2 * npair, TILE * (w + 1))
        part = sum(r * r for r in r4q[lo:hi])
        if w == 0 and n % 2:
            part += r4q[n - 1] ** 2
        shares.append(Fraction(part, scale))
    return dict(dotr=dotr, dotr_bound=dotr_bound, beta=beta, beta_bound=beta_bound, tile_least=min(shares), tiles=len(shares))


def within(got, ref, bound):
    """|got - ref| <= bound with got a finite double, ref and bound rationals: compared exactly"""
    g = float(got)
    return g == g and abs(g) != float("inf") and abs(Fraction(g) - ref) <= bound


# ---- the shapes of tests/test_dot_groups_gpu.py; tests/test_exact_dots.py pins their plans without a GPU
# name -> (n, csr_groups, L, (sliced-ELL groups, CSR row blocks))
PLAIN_N = (200, 512, 513, 514, 1792, 2048, 2049, 2050, 7936, 8192, 8193, 8194, 15872, 16384, 16385, 16386, 16640)
SHAPES = {"n%d" % n: (n, (), 600, (-(-n // GROUP), 0)) for n in PLAIN_N}
SHAPES.update({
    "span_3_1": (4 * GROUP, (3,), 600, (3, 1)),
    "span_17_1": (18 * GROUP, (17,), 600, (17, 1)),
    "span_32_1": (33 * GROUP, (32,), 600, (32, 1)),
    "span_33_2": (33 * GROUP + 1, (32,), 3000, (33, 2)),
    "span_49_20": (64 * GROUP + 17, tuple(range(48, 64)), 600, (49, 20)),
    "span_32_40": (64 * GROUP, tuple(range(32, 64)), 600, (32, 40)),
})
# two ranks of 18 groups each: name -> (n, csr_groups, L, per rank (interior groups, halo-touching groups, interior row blocks,
# halo-touching row blocks))
RANK_SHAPES = {
    "ranks_interior_blocks": (36 * GROUP, (10, 28), 600, ((16, 1, 2, 0), (16, 1, 2, 0))),
    "ranks_boundary_block": (36 * GROUP, (17, 35), 600, ((17, 0, 0, 1), (15, 2, 1, 0))),
}


def host_blocks(A, nranks=1, rank=0):
    """(hipsolver.HostBlocks of this rank's rows under the reference's equal-rows partition, first row, rows)"""
    from mpi_bicgstab_amd import hipsolver as H, synth
    counts, displs = synth.partition(A.n, nranks)
    lo, nl = int(displs[rank]), int(counts[rank])
    dp, dc, dv, op, oc, ov = A.block(lo, lo + nl)
    offd = synth.CSR(nl, A.n, op, oc, ov) if nranks > 1 else None
    return H.HostBlocks(synth.CSR(nl, nl, dp, dc, dv), offd, A.n, counts, displs), lo, nl


def vec_workgroups(n):
    """workgroups of an element-wise kernel over n rows (vec_grid, csrc/bicg_vec.hip, below its caps): one per 256 element pairs"""
    return max(1, -(-(n >> 1) // 256))


# ---- the shifted family (tests/test_shifted_exact_gpu.py, tests/mp_shifted_workers.py; tests/test_exact_dots.py for the CPU half)
# The seed system of shifted_lopbicgstab, shifted_pipe_lopbicgstab, shifted_lopbicg and shifted_lopbicg_switching is
# A + sigma_seed I = d I + K with d = 4 + sigma_seed. Where d is a power of two the WHOLE first iteration is exact:
#     alpha_1 = (b, b) / (b, (A + sigma) b) = 1/d                         K is skew
#     q = b - (A + sigma) b / d,  y = (A + sigma) q                       d q and d y are integer vectors
#     lop-type:  omega_1 = (q, q) / (q, y) = 1/d                          K is skew once more
#                r = q - y/d  (d^2 r an integer vector), (r, r) and (r#, r) = (b, r) exact,
#                beta_1 = (alpha/omega) ((b, r) / (b, b)) = 1 * one correctly rounded division
#     pipe:      w = (A + sigma) b, z = (A + sigma) w from the set-up, y = w - z/d is (A + sigma) q entry for entry,
#                omega_1 = (q, y) / (y, y), one correctly rounded division; r = q - omega y is rounded (`ShiftedFirst.residual_dots`)
#     shifted_bicgstab: the seed system is A itself whatever the list says: alpha_1 = 1/4 and omega_1 = (q, y)/(y, y) of `First`
# The per-shift coefficients are scalar IEEE operations on these scalars in the reference's order, so every x_j of the first
# iteration has one right answer as bytes: the CPU oracle's.
SHIFT_STEP = 2.0 ** -6
LOP_TYPE = ("shifted_lopbicgstab", "shifted_lopbicg", "shifted_lopbicg_switching")
SHIFTED_VARIANTS = LOP_TYPE[:1] + ("shifted_pipe_lopbicgstab", "shifted_bicgstab") + LOP_TYPE[1:]


def recurrence(which):
    """which of the three seed recurrences a variant runs: "lop", "pipe" or "xi" (shifted_bicgstab)"""
    return "lop" if which in LOP_TYPE else "pipe" if which == "shifted_pipe_lopbicgstab" else "xi"


def shift_list(nsig, seed, sigma_seed):
    """sigma_j = sigma_seed + (j - seed) 2^-6: pairwise different, exact doubles, |sigma_seed - sigma_j| <= nsig / 64. For
    shifted_bicgstab the caller passes seed = 0 and sigma_seed = 0: its seed system is A, shift index 0"""
    assert 0 <= seed < nsig
    return np.array([sigma_seed + (j - seed) * SHIFT_STEP for j in range(nsig)], dtype=np.float64)


def shifted_case(which, nsig, seed, sigma_seed):
    """(sigma list, seed, sigma_seed) as `which` is called for the list (nsig, seed): shifted_bicgstab always with seed 0 on A"""
    if recurrence(which) == "xi":
        seed, sigma_seed = 0, 0
    return shift_list(nsig, seed, sigma_seed), seed, sigma_seed


def tiles(lo, hi):
    """index arrays (global rows) of the elements each workgroup of an element-wise kernel over the rows lo .. hi - 1 sums: workgroup
    w the element pairs 256 w .. 256 w + 255, workgroup 0 also the single trailing element of an odd count (residual_dots)"""
    n = hi - lo
    npair = n // 2
    out = []
    for w in range(vec_workgroups(n)):
        idx = np.arange(TILE * w, min(2 * npair, TILE * (w + 1)))
        if w == 0 and n % 2:
            idx = np.append(idx, n - 1)
        out.append(lo + idx)
    return out


class ShiftedFirst:
    """the first iteration of the shifted family on (A + sigma_seed I) in integers, d = 4 + sigma_seed a power of two:
    Mb = (A + sigma) b; dMb = d Mb; dq = d q; dy = d y; d2r = d^2 r (lop-type); w = Mb and z = (A + sigma) w (pipe's set-up).
    Expected doubles: dot_zero, alpha, omega["lop" | "pipe" | "xi"], beta and dotr (lop-type)."""

    def __init__(self, A, b, sigma_seed):
        d = 4 + int(sigma_seed)
        assert d == 4 + sigma_seed and d >= 1 and d & (d - 1) == 0, "4 + sigma_seed is a power of two"
        self.A, self.b, self.d, self.sigma_seed = A, b, d, int(sigma_seed)
        self._least = {}
        sg = self.sigma_seed
        self.Mb = A.times(b) + sg * b
        self.dMb = d * self.Mb
        self.dq = d * b - self.Mb
        self.dy = A.times(self.dq) + sg * self.dq
        self.d2r = d * self.dq - self.dy
        self.w = self.Mb
        self.z = A.times(self.w) + sg * self.w
        assert np.array_equal(d * self.w - self.z, self.dy), "pipe: y = w - z/d is (A + sigma) q entry for entry"
        self.bb, self.bMb = isum(b * b), isum(b * self.Mb)
        self.qq, self.qy, self.yy = isum(self.dq * self.dq), isum(self.dq * self.dy), isum(self.dy * self.dy)
        self.rr, self.br = isum(self.d2r * self.d2r), isum(b * self.d2r)
        assert self.bMb == d * self.bb and self.qy == d * self.qq and self.qq > 0 and self.yy > 0
        self.plain = First(A, b)                  # shifted_bicgstab iterates on A
        self.dot_zero = float(self.bb)
        self.alpha = float(Fraction(self.bb, self.bMb))
        self.omega = {"lop": float(Fraction(self.qq, self.qy)), "pipe": float(Fraction(self.qy, self.yy)), "xi": self.plain.omega}
        assert self.alpha == 1.0 / d and self.omega["lop"] == 1.0 / d
        self.dotr = float(Fraction(self.rr, d ** 4))
        self.beta = float(Fraction(self.br, d * d * self.bb))        # (alpha/omega) = 1; (b, r) = br / d^2 is a double

    def scalars(self, which):
        """dict(dot_zero, alpha, omega) and, for the lop-type variants, beta and dotr: the doubles `which` must report"""
        kind = recurrence(which)
        out = dict(dot_zero=self.dot_zero, alpha=0.25 if kind == "xi" else self.alpha, omega=self.omega[kind])
        if kind == "lop":
            out.update(beta=self.beta, dotr=self.dotr)
        return out

    def exact_terms(self, kind):
        """the integer term vectors of the exact dots of recurrence `kind`, those of the end group last"""
        b = self.b
        if kind == "xi":
            P = self.plain
            return [b * b, b * P.Ab, P.y4 * P.s4, P.y4 * P.y4], []
        if kind == "pipe":
            return [b * b, b * self.Mb, self.dq * self.dy, self.dy * self.dy], []
        return [b * b, b * self.Mb, self.dq * self.dq, self.dq * self.dy], [self.d2r * self.d2r, b * self.d2r]

    def preconditions(self, kind, units, rows, sigma, seed):
        """what the byte comparison of recurrence `kind` rests on, from the integers alone: every absolute sum below 2^53 and every
        vector entry below 2^26; no producer unit (row range of `units`) and no element-wise workgroup (`tiles` of each rank's
        (lo, hi) in `rows`) with a zero partial in any exact dot -- the end group's (r, r) and (b, r) are summed by element-wise
        workgroups only --; |omega_1 (sigma_seed - sigma_j)| < 1 for every shift. Returns the smallest |partial|."""
        sg_seed = 0.0 if kind == "xi" else float(self.sigma_seed)
        for j, sg in enumerate(sigma):
            if j != seed:
                assert abs(self.omega[kind] * (sg_seed - float(sg))) < 1.0, (j, sg)
        key = (kind, tuple(units), tuple(rows))
        if key in self._least:                    # (the sums do not depend on the shift list)
            return self._least[key]
        first, end = self.exact_terms(kind)
        for terms in first + end:
            assert isum(np.abs(terms)) < 2 ** 53
        vectors = (self.plain.Ab, self.plain.s4, self.plain.y4) if kind == "xi" else (self.dMb, self.dq, self.dy, self.d2r, self.w, self.z)
        assert max(int(np.abs(v).max()) for v in vectors) < 2 ** 26
        least = None
        pieces = [np.arange(lo, hi) for lo, hi in units]
        for p in pieces:
            assert len(p)
        pieces = [(p, first) for p in pieces] + [(t, first + end) for lo, hi in rows for t in tiles(lo, hi)]
        for idx, dots in pieces:
            for terms in dots:
                part = int(terms[idx].sum())          # (int64: every absolute sum is below 2^53)
                assert part != 0, ("a partial sum is zero: the comparison could not miss it", int(idx[0]), int(idx[-1]))
                least = abs(part) if least is None else min(least, abs(part))
        self._least[key] = least
        return least

    def residual_dots(self, kind):
        """(r, r) and beta of the first iteration where omega is not dyadic ("pipe", "xi"): r_i = fl(q_i + fl(-omega y_i)) in the
        kernels of either form, dotr = sum fl(r_i r_i), rho = sum fl(b_i r_i), beta = fl(fl(alpha/omega) fl(rho / (b, b))) (PH_SH_END,
        PH_SHP_END in csrc/bicg_devfn.h). The rational replay and the bounds of `residual_dots` above with d for 4:
        dict(dotr, dotr_bound, beta, beta_bound) as Fractions."""
        if kind == "xi":
            R = residual_dots(self.plain)
            return {k: R[k] for k in ("dotr", "dotr_bound", "beta", "beta_bound")}
        assert kind == "pipe"
        n, d = len(self.b), self.d
        om = Fraction(self.omega[kind])
        p, q = om.numerator, om.denominator
        # d q_den r_i = q_den dq_i - p dy_i, integers
        rs = [q * int(s) - p * int(y) for s, y in zip(self.dq, self.dy)]
        ts = [q * abs(int(s)) + abs(p) * abs(int(y)) for s, y in zip(self.dq, self.dy)]
        scale = d * d * q * q
        dotr = Fraction(sum(r * r for r in rs), scale)
        rho = Fraction(sum(int(bi) * r for bi, r in zip(self.b, rs)), d * q)
        dotr_bound = 8 * (n + 4) * U * Fraction(sum(t * t for t in ts), scale)
        e_rho = 2 * (n + 4) * U * Fraction(sum(abs(int(bi)) * t for bi, t in zip(self.b, ts)), d * q)
        ratio = abs(Fraction(self.alpha) / om) / self.bb
        beta = Fraction(self.alpha) / om * rho / self.bb
        return dict(dotr=dotr, dotr_bound=dotr_bound, beta=beta, beta_bound=ratio * (e_rho + 4 * U * (abs(rho) + e_rho)))


@functools.lru_cache(maxsize=None)
def shifted_first(n, csr_groups=(), L=600, sigma_seed=0, seed=5):
    return ShiftedFirst(*system(n, csr_groups, L, seed), sigma_seed)


# the shapes of tests/test_shifted_exact_gpu.py: name -> (n, csr_groups, L, (sliced-ELL groups, CSR row blocks), seed= of `system`);
# n65 is one short group (one element-wise workgroup, an odd count), the others are SHAPES'. n513 takes another seed: with seed 5
# and sigma_seed = -2 the one-row group 512 has a zero partial (tests/test_exact_dots.py: test_shifted_preconditions)
SHIFTED_SHAPES = {"n65": (65, (), 600, (1, 0), 5)}
SHIFTED_SHAPES.update({k: SHAPES[k] + (0 if k == "n513" else 5,) for k in ("n513", "n2049", "n16385", "span_3_1", "span_33_2")})


def shifted_system(name):
    """(Matrix, b) of a shape of SHIFTED_SHAPES"""
    n, groups, L, _, s = SHIFTED_SHAPES[name]
    return system(n, groups, L, s)


def shifted_first_of(name, sigma_seed):
    n, groups, L, _, s = SHIFTED_SHAPES[name]
    return shifted_first(n, groups, L, sigma_seed, s)
# (nsig, seed) in the order every context runs them -- the per-shift buffers grow, shrink and grow --, on the batch edges of
# shift_pass (8 / 9, a seed that is the last of a batch, the first of the next, the last shift), the trip counts of comm_coefs
# (6 nsig coefficients by 64 lanes: 10 / 11, 21 / 22) and kPersistMaxShifts = 32 / 33
SHIFT_LISTS = ((1, 0), (9, 8), (33, 32), (2, 1), (8, 7), (9, 0), (11, 5), (22, 7), (32, 31), (32, 0), (33, 8), (16, 15))
SIGMA_SEEDS = (0, 4, -2, 12)                     # d = 4, 8, 2, 16, cycled along SHIFT_LISTS
# (nsig, seed, sigma_seed) of the tests that run more than one iteration. The lop recurrence has omega_k = (q, q) / (q, (d I + K) q)
# = 1/d at EVERY iteration (K is skew), so r_k = -(K/d) q_k: it contracts only where ||K|| < d, and ||K|| <= 8 (four band entries of
# magnitude <= 2 per row) -- with d = 4 and d = 2 the reference recurrence itself diverges on these systems (the CPU oracle runs
# into its iteration limit with an infinite residual). Several iterations are therefore compared on d = 16 and d = 8 only, alternating.
ITER_CASES = ((9, 8, 12), (22, 7, 4), (32, 31, 12), (33, 8, 4))
RANK_SHIFTED = (36 * GROUP, (1, 9))              # two ranks of 18 groups, the lists (9, 8) and (32, 0)


def list_case(i):
    """(nsig, seed, sigma_seed) of SHIFT_LISTS[i]"""
    return SHIFT_LISTS[i] + (SIGMA_SEEDS[i % len(SIGMA_SEEDS)],)


def oracle_shifted(A, b, which, sigma, seed, nranks=1, **kw):
    """the CPU oracle's run of variant `which` (tests/oracle_lib.py: solve_shifted / solve_switching) on the whole integer system"""
    import oracle_lib as O
    row = np.repeat(np.arange(A.n, dtype=np.uint32), np.diff(A.ptr.astype(np.int64)))
    fn = O.solve_switching if which in LOP_TYPE[1:] else O.solve_shifted
    return fn(A.n, row, A.col, A.val, b.astype(np.float64), sigma, seed, nranks=nranks, which=which, **kw)


def true_residuals(A, b, x, sigma):
    """|| b - (A + sigma_j I) x_j || / || b || for every shift, the product in numpy from the integer matrix"""
    ptr = A.ptr[:-1].astype(np.int64)
    bf = b.astype(np.float64)
    return np.array([np.linalg.norm(bf - (np.add.reduceat(A.val * xj[A.col], ptr) + sg * xj)) / np.linalg.norm(bf) for xj, sg in zip(x, sigma)])
