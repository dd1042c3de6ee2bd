"""Without a GPU: what tests/test_dot_groups_gpu.py rests on (tests/exact_dots.py says why the first BiCGStab iteration of its
integer systems is exact).

  * the exactness preconditions, from the integer reference alone: every sum below 2^53, no producer (256-row group, CSR row
    block) with a zero partial in (b, Ab), (y, s) or (y, y), every element-wise workgroup's share of (r, r) a thousand times the
    bound on (r, r) and more;
  * the plan geometry of every shape, from bicg_sell_plan_digest: how many sliced-ELL groups and CSR row blocks a product has,
    interior and halo-touching, on one rank and on each of two -- the GPU tests choose their shapes by these counts (fewer than,
    exactly and more than the 32 shards; a second launch of 1, 2, 20 and 40 workgroups);
  * that the comparison can fail: a reference with one producer's partial dropped, or added twice, is rejected as bytes.

And what tests/test_shifted_exact_gpu.py rests on (second half): the preconditions of exact_dots.ShiftedFirst for every shape,
shift list and recurrence; the CPU oracle's first scalars equal to the integer replay as bytes, at one and two ranks, its x_j
finite and pairwise different; the shift lists on the edges of the per-shift machinery; a swapped sigma, a dropped update and a
moved seed rejected as bytes; every iteration of the four-iteration test moving every shift by 1000 bars and more; the oracle
converging inside one persistent chunk on the cases of the run to tolerance."""
import functools
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


# ---- the shifted family: what tests/test_shifted_exact_gpu.py and tests/mp_shifted_workers.py rest on
SHIFTED = list(E.SHIFTED_SHAPES)
KINDS = ("lop", "pipe", "xi")


@functools.lru_cache(maxsize=None)
def shifted_units(name):
    """(producer units, [(first row, end row)]) of a one-rank shape of SHIFTED_SHAPES, the counts checked against the plan"""
    n, groups, L, (want_groups, want_blocks), _ = E.SHIFTED_SHAPES[name]
    A, _ = E.shifted_system(name)
    summary, blk, lo, nl = plan(A)
    assert (summary["ng_int"], summary["ng_bnd"], summary["nblk"], summary["n_bnd"]) == (want_groups, 0, want_blocks, 0), summary
    return tuple(units_of(A, summary, blk, lo, nl, 1, 0)), ((0, n),)


def oracle_first(name, which, i, nranks=1, **kw):
    """(ShiftedFirst, sigma, seed, the oracle's one iteration) of variant `which` on list i of a shape (i: an index into SHIFT_LISTS,
    or the case (nsig, seed, sigma_seed) itself)"""
    A, b = E.shifted_system(name)
    nsig, seed, sg = E.list_case(i) if isinstance(i, int) else i
    sigma, seed, sg = E.shifted_case(which, nsig, seed, sg)
    kw = dict(dict(tol=0.0, max_iter=1), **kw)
    return E.shifted_first_of(name, sg), sigma, seed, E.oracle_shifted(A, b, which, sigma, seed, nranks=nranks, **kw)


def check_oracle_scalars(F, which, o, its=1):
    """the oracle's first scalars are ShiftedFirst's as bytes (pipe, shifted_bicgstab: beta and dotr within the derived bounds)"""
    want = F.scalars(which)
    assert o["k"] == its + (which == "shifted_lopbicg_switching")        # (the switching variant counts from 1)
    assert E.same_bytes(o["dot_zero"], want["dot_zero"])
    for key in ("alpha", "omega", "beta", "dotr"):
        if key in want:
            assert E.same_bytes(o[key][0], want[key]), (which, key, o[key][0], want[key])
    if "beta" not in want:
        R = F.residual_dots(E.recurrence(which))
        assert E.within(o["dotr"][0], R["dotr"], R["dotr_bound"]) and E.within(o["beta"][0], R["beta"], R["beta_bound"]), which


def check_distinct(x):
    assert np.isfinite(x).all()
    rows = {xj.tobytes() for xj in x}
    assert len(rows) == len(x) and np.zeros(x.shape[1]).tobytes() not in rows, "a swapped or idle shift could pass"


@pytest.mark.parametrize("name", SHIFTED)
def test_shifted_preconditions(name):
    n, groups = E.SHIFTED_SHAPES[name][:2]
    units, rows = shifted_units(name)
    for i in range(len(E.SHIFT_LISTS)):
        nsig, seed, sg = E.list_case(i)
        for kind in KINDS:
            which = {"lop": "shifted_lopbicgstab", "pipe": "shifted_pipe_lopbicgstab", "xi": "shifted_bicgstab"}[kind]
            sigma, sd, s0 = E.shifted_case(which, nsig, seed, sg)
            F = E.shifted_first_of(name, s0)
            assert F.preconditions(kind, units, rows, sigma, sd) >= 1
            assert len(set(sigma.tolist())) == nsig and sigma[sd] == s0
    assert len(E.tiles(0, n)) == E.vec_workgroups(n) and sum(len(t) for t in E.tiles(0, n)) == n
    # the form run_shifted takes: the persistent one needs a product without CSR row blocks (persist_build, csrc/bicg_create.cpp,
    # refuses nblk > 0 before it plans) and a plan with one row per thread (256 CUs: 255 workgroups beside the helper's)
    A, _ = E.shifted_system(name)
    blocks = E.SHIFTED_SHAPES[name][3][1]
    assert (blocks > 0) == bool(groups) and plan(A)[0]["nblk"] == blocks
    if not groups:
        P = H.persist_plan(E.host_blocks(A)[0], 1, 255)
        assert P is not None and P["rpt"] == 1, P and P["rpt"]


def test_shift_lists_sit_on_the_edges():
    """8 / 9 (a batch of shift_pass), 10 / 11 and 21 / 22 (64 lanes fetching 6 nsig coefficients), 32 / 33 (kPersistMaxShifts); a seed
    that is the last of a batch, the first of the next, the last and the first shift; the buffers grow, shrink and grow"""
    sizes = [nsig for nsig, _ in E.SHIFT_LISTS]
    assert {1, 2, 8, 9, 11, 16, 22, 32, 33} <= set(sizes)
    assert [6 * a <= 64 * t < 6 * b for a, b, t in ((10, 11, 1), (21, 22, 2))] == [True, True]
    assert {(9, 8), (8, 7), (33, 32), (33, 8), (32, 31), (32, 0), (16, 15), (9, 0)} <= set(E.SHIFT_LISTS)
    steps = np.sign(np.diff(sizes))
    assert (steps > 0).any() and (steps < 0).any() and sizes[2] == max(sizes) and sizes[3] < sizes[2] < 34
    assert {c[:2] for c in E.ITER_CASES} == {(9, 8), (22, 7), (32, 31), (33, 8)} and {4 + c[2] for c in E.ITER_CASES} == {8, 16}


@pytest.mark.parametrize("which", E.SHIFTED_VARIANTS)
@pytest.mark.parametrize("name", SHIFTED)
def test_oracle_first_iteration_is_the_integer_replay(name, which):
    for i in range(len(E.SHIFT_LISTS)):
        for nranks in (1, 2):
            F, sigma, seed, o = oracle_first(name, which, i, nranks)
            check_oracle_scalars(F, which, o)
            check_distinct(o["x"])


@pytest.mark.parametrize("which", ["shifted_lopbicgstab", "shifted_pipe_lopbicgstab", "shifted_lopbicg_switching"])
@pytest.mark.parametrize("name", ["n2049", "span_3_1"])
def test_a_perturbed_shift_is_rejected(name, which):
    """the mutations are made on the oracle's side, for every list: two shifts' sigma swapped, one shift's update dropped, the seed
    moved by one -- the byte comparison the GPU tests apply to the library's x set (and scalars) then fails"""
    A, b = E.shifted_system(name)
    run = lambda sigma, seed: E.oracle_shifted(A, b, which, sigma, seed, tol=0.0, max_iter=1)
    for i in range(len(E.SHIFT_LISTS)):
        F, sigma, seed, o = oracle_first(name, which, i)
        nsig, want = len(sigma), o["x"].tobytes()
        for j in range(nsig):                                     # a dropped update: x_j stays x0 = 0
            x = o["x"].copy()
            x[j] = 0.0
            assert x.tobytes() != want
        if nsig == 1:
            continue
        a, c = ((seed + 1) % nsig, (seed + 2) % nsig) if nsig > 2 else (0, 1)
        swapped = sigma.copy()
        swapped[[a, c]] = sigma[[c, a]]
        assert run(swapped, seed)["x"].tobytes() != want
        moved = run(sigma, seed + 1 if seed + 1 < nsig else seed - 1)
        assert moved["x"].tobytes() != want and not E.same_bytes(moved["alpha"][0], F.alpha)


@pytest.mark.parametrize("which", ["shifted_lopbicgstab", "shifted_pipe_lopbicgstab", "shifted_bicgstab"])
@pytest.mark.parametrize("name", ["n2049", "span_3_1"])
def test_four_iterations_move_every_shift(name, which):
    """the bar of the four-iteration GPU test, 1e-8 max|x_j|, is a thousand times smaller than the smallest change any iteration
    k <= 4 makes to any shift: a shift that misses one iteration's update cannot pass it"""
    least = None
    for i in E.ITER_CASES:
        xs = [oracle_first(name, which, i, max_iter=k)[3]["x"] for k in range(1, 5)]
        bar = 1e-8 * np.abs(xs[-1]).max(axis=1)
        prev = np.zeros_like(xs[0])
        for k, x in enumerate(xs, 1):
            step = np.abs(x - prev).max(axis=1)
            assert (step >= 1000 * bar).all(), (name, which, i, k, float((step / bar).min()))
            least = float((step / bar).min()) if least is None else min(least, float((step / bar).min()))
            prev = x
    print(name, which, "smallest per-iteration change / bar:", least)


def test_two_rank_shifted_case():
    """tests/mp_shifted_workers.py: both ranks' producers and element-wise workgroups, the persistent plan of each rank (127
    workgroups: persist_build with two ranks on one device), the oracle at two ranks"""
    n, lists = E.RANK_SHIFTED
    A, b = E.system(n)
    units, rows = [], []
    for rank in (0, 1):
        summary, blk, lo, nl = plan(A, 2, rank)
        units += units_of(A, summary, blk, lo, nl, 2, rank)
        rows.append((lo, lo + nl))
        P = H.persist_plan(blk, 2, 127)
        assert P is not None and P["rpt"] == 1 and P["halo"] > 0, P and P["rpt"]
    for i in lists:
        nsig, seed, sg = E.list_case(i)
        F = E.shifted_first(n, (), 600, sg)
        for which in ("shifted_lopbicgstab", "shifted_pipe_lopbicgstab"):
            sigma = E.shift_list(nsig, seed, sg)
            assert F.preconditions(E.recurrence(which), tuple(units), tuple(rows), sigma, seed) >= 1
            o = E.oracle_shifted(A, b, which, sigma, seed, nranks=2, tol=0.0, max_iter=1)
            check_oracle_scalars(F, which, o)
            check_distinct(o["x"])


@pytest.mark.parametrize("which", ["shifted_lopbicgstab", "shifted_pipe_lopbicgstab", "shifted_bicgstab"])
def test_the_oracle_converges_inside_one_persistent_chunk(which):
    """what the run to tol = 1e-10 of the GPU file rests on: on n2049 the oracle stops well inside 128 iterations (kPersistChunk) with
    every shift solved, for every case of ITER_CASES -- and on d = 4 the lop recurrence does not (exact_dots.ITER_CASES says why)"""
    A, b = E.shifted_system("n2049")
    for case in E.ITER_CASES:
        F, sigma, seed, o = oracle_first("n2049", which, case, tol=1e-10, max_iter=1000)
        true_sigma = np.r_[0.0, sigma[1:]] if which == "shifted_bicgstab" else sigma
        res = E.true_residuals(A, b, o["x"], true_sigma)
        print(which, case, "k", o["k"], "largest true residual %.3e" % res.max())
        assert o["k"] <= 64 and res.max() <= 1e-9, (which, case, o["k"], res.max())
    F, sigma, seed, o = oracle_first("n2049", "shifted_lopbicgstab", (9, 8, 0), tol=1e-10, max_iter=1000)
    assert o["k"] == 1000 and not np.abs(o["x"]).max() < 1e50
