"""Without a GPU: what tests/test_dot_groups_gpu.py rests on (tests/exact_dots.py says why the first BiCGStab iteration of its
integer systems is exact).

  * the exactness preconditions, from the integer reference alone: every sum below 2^53, no producer (256-row group, CSR row
    block) with a zero partial in (b, Ab), (y, s) or (y, y), every element-wise workgroup's share of (r, r) a thousand times the
    bound on (r, r) and more;
  * the plan geometry of every shape, from bicg_sell_plan_digest: how many sliced-ELL groups and CSR row blocks a product has,
    interior and halo-touching, on one rank and on each of two -- the GPU tests choose their shapes by these counts (fewer than,
    exactly and more than the 32 shards; a second launch of 1, 2, 20 and 40 workgroups);
  * that the comparison can fail: a reference with one producer's partial dropped, or added twice, is rejected as bytes."""
from fractions import Fraction

import numpy as np
import pytest

import exact_dots as E
from mpi_bicgstab_amd import hipsolver as H

ONE_RANK = list(E.SHAPES)
TWO_RANKS = [(name, rank) for name in E.RANK_SHAPES for rank in (0, 1)]


def plan(A, nranks=1, rank=0):
    blk, lo, nl = E.host_blocks(A, nranks, rank)
    nnz = int(A.ptr[-1]) - (sum(int(E.host_blocks(A, nranks, r)[0].offd.nz) for r in range(nranks)) if nranks > 1 else 0)
    summary, _ = H.sell_plan_digest(blk, nranks, A.n, nnz)
    return summary, blk, lo, nl


def units_of(A, summary, blk, lo, nl, nranks, rank):
    """the producer units of this rank's products (exact_dots.producer_units), their counts checked against the plan's"""
    per_rank = -(-A.n // nranks) // E.GROUP if nranks > 1 else 0
    local = [g - rank * per_rank for g in A.csr_groups if nranks == 1 or rank * per_rank <= g < (rank + 1) * per_rank]
    ptr = np.ctypeslib.as_array(blk.diag.ptr, shape=(nl + 1,))
    sliced, blocks = E.producer_units(ptr, nl, local, lo, rowsplit=bool(summary["rowsplit"]))
    assert len(sliced) == summary["ng_int"] + summary["ng_bnd"] and len(blocks) == summary["nblk"]
    assert sum(hi - lo_ for lo_, hi in sliced) == summary["sell_rows"]
    return sliced + blocks


@pytest.mark.parametrize("name", ONE_RANK)
def test_one_rank_shapes(name):
    n, groups, L, (want_groups, want_blocks) = E.SHAPES[name]
    A, _ = E.system(n, groups, L)
    summary, blk, lo, nl = plan(A)
    assert (summary["ng_int"], summary["ng_bnd"], summary["nblk"], summary["n_bnd"]) == (want_groups, 0, want_blocks, 0), summary
    if not groups:
        assert not summary["jag"] and summary["c16"], summary          # padded slices, 16-bit offsets: the hand-over's layout
    F = E.first(n, groups, L)
    least = E.preconditions(F, units_of(A, summary, blk, lo, nl, 1, 0))
    assert least >= 1
    assert E.same_bytes(F.alpha, 0.25) and E.same_bytes(F.omega, (F.ys / 16.0) / (F.yy / 16.0))
    R = E.residual_dots(F)
    assert R["tiles"] == E.vec_workgroups(n)
    assert R["tile_least"] >= 1000 * R["dotr_bound"], (float(R["tile_least"]), float(R["dotr_bound"]))
    assert R["dotr"] > 0 and R["beta"] != 0


@pytest.mark.parametrize("name,rank", TWO_RANKS)
def test_two_rank_shapes(name, rank):
    n, groups, L, want = E.RANK_SHAPES[name]
    A, _ = E.system(n, groups, L)
    summary, blk, lo, nl = plan(A, 2, rank)
    got = (summary["ng_int"], summary["ng_bnd"], summary["nblk"] - summary["n_bnd"], summary["n_bnd"])
    assert got == want[rank], summary
    # the condition the fix of spmv() is about, on the interior + boundary path: the last launch with workgroups is smaller than
    # min(workgroups of the group, 32)
    launches = [g for g in (got[0], got[2], got[1], got[3]) if g]
    assert len(launches) > 1 and launches[-1] < min(sum(launches), 32)
    E.preconditions(E.first(n, groups, L), units_of(A, summary, blk, lo, nl, 2, rank))


def test_one_rank_shapes_cover_the_edges():
    """the workgroup counts at which the finishes change shape"""
    products = [E.SHAPES[k][3][0] for k in E.SHAPES if not E.SHAPES[k][1]]
    assert {1, 2, 3, 7, 8, 9, 31, 32, 33, 62, 64, 65} <= set(products)
    assert {28, 32, 36} <= {4 * g for g in products}                  # one partial per wavefront: around the 32 shards
    assert {1, 2, 4, 5, 16, 17, 31, 32, 33} <= {E.vec_workgroups(n) for n in E.PLAIN_N}
    assert any(n % 2 for n in E.PLAIN_N) and any(n % E.GROUP == 1 for n in E.PLAIN_N)
    spans = [E.SHAPES[k][3] for k in E.SHAPES if E.SHAPES[k][1]]
    assert spans == [(3, 1), (17, 1), (32, 1), (33, 2), (49, 20), (32, 40)]
    # second launch smaller than min(all, 32) in all but the last, which keeps the tail finish across two launches
    assert [b < min(g + b, 32) for g, b in spans] == [True] * 5 + [False]


@pytest.mark.parametrize("name", ["n2049", "span_17_1", "span_33_2"])
def test_a_dropped_or_doubled_partial_is_rejected(name):
    """the mutation is made on the reference's side: one producer's partial left out of, or added twice to, an exact sum -- the
    byte comparison that the GPU tests apply to the library's numbers then fails, for every producer"""
    n, groups, L, _ = E.SHAPES[name]
    A, _ = E.system(n, groups, L)
    F = E.first(n, groups, L)
    summary, blk, lo, nl = plan(A)
    assert E.same_bytes(F.dot_zero, float(F.bb)) and not E.same_bytes(0.0, -0.0) and E.same_bytes(float("nan"), float("nan"))
    for lo_, hi in units_of(A, summary, blk, lo, nl, 1, 0):
        b, Ab, s4, y4 = (v[lo_:hi] for v in (F.b, F.Ab, F.s4, F.y4))
        for sign in (-1, 1):
            bAb = F.bAb + sign * E.isum(b * Ab)
            ys, yy = F.ys + sign * E.isum(y4 * s4), F.yy + sign * E.isum(y4 * y4)
            assert not E.same_bytes(F.bb / bAb, F.alpha)
            # (both sums lose the same producer, or only one of them does)
            for wrong in (Fraction(ys, yy), Fraction(ys, F.yy), Fraction(F.ys, yy)):
                assert not E.same_bytes(float(wrong), F.omega)
    for lo_, hi in [(0, min(n, E.GROUP))]:
        assert not E.same_bytes(float(F.bb - E.isum(F.b[lo_:hi] ** 2)), F.dot_zero)
    # the third group: a lost element-wise workgroup moves (r, r) beyond its bound; the exact value itself passes
    R = E.residual_dots(F)
    assert E.within(float(R["dotr"]), R["dotr"], R["dotr_bound"]) and E.within(float(R["beta"]), R["beta"], R["beta_bound"])
    assert not E.within(float(R["dotr"] - R["tile_least"]), R["dotr"], R["dotr_bound"])
    assert not E.within(float("nan"), R["dotr"], R["dotr_bound"])
