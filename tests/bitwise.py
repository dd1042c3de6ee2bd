"""Byte comparisons and the integer systems behind them -- a plain helper of the tests that put a product kernel on its plan limits
(tests/test_ragged_limits_gpu.py on tests/ragged_cases.py, tests/test_csr_limits_gpu.py and tests/mp_csr_workers.py on
tests/csr_cases.py, tests/test_padded_limits_gpu.py and tests/mp_padded_workers.py on tests/padded_cases.py). Nothing in here touches a GPU; the library appears only through the context a caller hands to `check_first_dots`."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import oracle_lib as O

GROUP = 256          # rows per sliced-ELL group (kGroupRows): the finest producer of a dot partial on the sliced path


def same_bits(got, want):
    return np.ascontiguousarray(got, dtype=np.float64).tobytes() == np.ascontiguousarray(want, dtype=np.float64).tobytes()


def assert_same_bits(got, want, what):
    if not same_bits(got, want):
        bad = np.flatnonzero(np.asarray(got).view(np.uint64).ravel() != np.asarray(want).view(np.uint64).ravel())
        raise AssertionError(f"{what}: {len(bad)} of {np.size(want)} values differ in their bits, the first at {bad[:8].tolist()}")


def oracle_spmv(A, x):
    """the CPU oracle's A x: a row's products added in stored order, one rounding per product and per sum, y = 0.0 + that sum"""
    row, col, val = A.to_coo()
    return O.spmv(A.rows, row, col, val, x)


class IntegerSystem:
    """the integer values of a case of `cases` (a module with build(name, values, seed) -> (CSR, facts, switches): ragged_cases,
    csr_cases), b from {1, 2, 3}, and the first iteration's exact scalars: dot_zero = (b, b) and alpha_1 = (b, b) / (b, A b)
    (x0 = 0: r = r# = p = b). Asserts what the byte comparison rests on. Groups without an entry have a zero partial by construction:
    exactly those the case names are allowed (facts["groups"]["all_empty"], or the list facts["empty_groups"])."""

    def __init__(self, name, cases):
        self.A, self.facts, self.sw = cases.build(name, "integer")
        A = self.A
        n = A.rows
        assert set(np.unique(A.val)) <= {1.0, 2.0, 3.0}
        row, col, _ = A.to_coo()
        b = np.random.default_rng(2000).integers(1, 4, size=n)
        ival = A.val.astype(np.int64)
        terms = ival * b[col.astype(np.int64)]
        assert int(terms.sum()) < 2 ** 53          # (so the float64 weights below add up exactly)
        Ab = np.bincount(row.astype(np.int64), weights=terms.astype(np.float64), minlength=n).astype(np.int64)
        self.b, self.Ab = b, Ab
        self.bb, self.bAb = int((b * b).sum()), int((b * Ab).sum())
        assert 0 < self.bb < 2 ** 53 and 0 < self.bAb < 2 ** 53 and int(Ab.max()) < 2 ** 26      # (all terms are positive: the sums are the absolute sums)
        # one partial of (b, A b) per 256-row group, at the finest: none is zero, except where the group holds no entry at all
        groups = np.arange(n) // GROUP
        part = np.bincount(groups, weights=(b * Ab).astype(np.float64))
        holds = np.bincount(row.astype(np.int64) // GROUP, minlength=len(part)) > 0
        assert np.all(part[holds] > 0)
        empty = sorted(np.flatnonzero(~holds).tolist())
        if "empty_groups" in self.facts:
            allowed = sorted(self.facts["empty_groups"])
        else:
            allowed = [self.facts["groups"]["all_empty"]] if "groups" in self.facts else []
        assert empty == allowed, "only the groups crafted to be empty"
        self.dot_zero = float(self.bb)
        self.alpha = float(Fraction(self.bb, self.bAb))


def check_first_dots(ctx, S, what, method="bicgstab"):
    """one iteration of `method` on the integer system S: dot_zero and alpha_1 are the exact values' bytes"""
    got = ctx.solve(method, S.b.astype(np.float64), tol=0.0, max_iter=1, check_every=1)
    assert got["k"] == 1, what
    assert same_bits(got["result"].dot_zero, S.dot_zero), (what, got["result"].dot_zero, S.bb)
    alpha = ctx.trace(1)["alpha"][0]
    assert same_bits(alpha, S.alpha), (what, float(alpha), S.alpha, S.bb, S.bAb)
