"""`-m gpu`: the multi-vector products over padded slices with 16-bit column offsets -- k_spmm_pipe<OFFD, 512 | 256>
(csrc/bicg_spmm.hip), k_spmm_win<0, OFFD, 8 | 4> and k_spmm_sell<LAY_PAD16 | LAY_PAD32, OFFD> (csrc/bicg_spmm_sell.hip) -- on the
crafted matrices of tests/padded_cases.py, each of which sits ON a limit of the fused-window cluster plan or of a kernel: a gap of
512 / 513 columns, 4 / 5 clusters, 2048 / 2050 and 1536 / 1538 pipeline slots, 2048 / 2049 window slots, 8 / 4 vectors per window at
1280 / 1281 slots, distances of 32767 / 32768, rows of 1 .. 33 entries (both halves of the register head, the streamed batches, rows
shorter than their slice, empty rows and an empty slice), every shape of a partly filled last tile, more tiles than resident
workgroups at both tile sizes, and the consecutive-tiles form. tests/test_padded_limits.py checks on the CPU that every matrix plans
as its generator promises; `padded_cases.spmm_kind` says which kernel and tile each pass must report.

No tolerance anywhere. References:
  products    the CPU oracle's spmv (tests/oracle_lib.py) per column: a row's products added in stored order, one rounding per
              product and per sum; a row without entries is exactly +0.0. Row j of an SpMM with shifts = that + sigma_j x_j in
              float64 numpy: one rounding for the product, one for the sum.
  norms       integer matrices, X, shifts and b: sum (b - (A + sigma_j I) x_j)^2 and (b, b) are Python integers below 2^53, so
              every partial sum is exact however the tiles and workgroups are added, and bicg_shifted_residuals returns
              sqrt(double(sq_j) / double(bb)) in its bytes -- through the SpMM's fused norms and, under spmm=0, one product per shift.
  multi-RHS   bicg_solve_multi(max_iter = 0): r = b - oracle spmv(x0), the pass reading its input from the solver's own slab.
Every context is created under switches(persist=0); spmm-window is read by the context's first pass and spmm-tile / spmm-gstep at
every launch, so a context's tokens stay set while it is in use (`running`)."""
import contextlib
import functools

import numpy as np
import pytest

import padded_cases as K
from bitwise import assert_same_bits, oracle_spmv, same_bits
from mpi_bicgstab_amd import hipsolver as H

pytestmark = pytest.mark.gpu
NVEC = (1, 3, 16, 17)
NORM_CASES = ("walk", "clusters4", "pipe1536", "slots2048", "clusters5", "lengths", "tri1", "tri257", "tri513")
MULTI_CASES = ("gap513", "lengths")


@pytest.fixture(scope="module", autouse=True)
def _single_rank():
    H.lib().bicg_comm_init_single(0)      # (once: a new communicator orphans the contexts of the one before)
    yield


@contextlib.contextmanager
def running(A, sw, **tokens):
    """a context of the one-rank block A under persist=0, the case's switches and `tokens`, which stay set until it is closed"""
    tokens = dict(sw, persist=0, **tokens)
    H.switches(**tokens)
    ctx = None
    try:
        ctx = H.Context(H.single_rank_blocks(A))
        yield ctx
    finally:
        if ctx is not None:
            ctx.close()
        H.switches(**{k: None for k in tokens})


def forms(facts):
    """the forms a case runs under: [(tokens, (kind, tile, vectors per window))] -- as planned; with clusters also the windowed and
    the row-major kernel; where the pipeline takes 512-row tiles and the mirror says 256 fit, those too"""
    out = [({}, K.spmm_kind(facts))]
    if facts["clusters"]:
        out += [({"spmm_window": w}, K.spmm_kind(facts, spmm_window=w)) for w in (1, 0)]
        if out[0][1][1] == 512 and K.pipe_fits(facts["cluster_list"], 256):
            out.append(({"spmm_tile": 256}, K.spmm_kind(facts, spmm_tile=256)))
    return out


def describe(name, facts, tokens, expect):
    kind, tile, nv = expect
    what = {"pipelined": f"tile {tile}", "windowed": f"{nv} vectors per window", "rowmajor": K.row_layout(facts)}[kind]
    print(f"{name} {tokens or ''}: {kind}, {what}; {facts['clusters']} clusters, W256 {facts['W256']}, rows {facts['rows']}")


@functools.lru_cache(maxsize=None)
def spmm_reference(name):
    """(X [17][n], 17 distinct sigma, the oracle's A x_j [17][n]) for the generic values of a case -- computed once, never written to"""
    A, _, _ = K.build(name)
    X = np.random.default_rng(3000).standard_normal((max(NVEC), A.rows))
    sigma = (np.arange(max(NVEC)) + 1.0) * 0.013
    AX = np.stack([oracle_spmv(A, X[j]) for j in range(len(X))])
    for a in (X, sigma, AX):
        a.setflags(write=False)
    return X, sigma, AX


def check_spmm(ctx, name, facts, expect, nvecs=NVEC, what=""):
    X, sigma, AX = spmm_reference(name)
    empty = facts["empty_rows"]
    for nvec in nvecs:
        for sg in (None, sigma[:nvec]):
            want = AX[:nvec] if sg is None else AX[:nvec] + sg[:, None] * X[:nvec]      # one rounding for the product, one for the sum
            for turn in ("", ", again"):
                Y, _ = ctx.spmm(X[:nvec], sg)
                assert (ctx.last_spmm_kind(), ctx.last_spmm_tile()) == expect[:2], (name, what, nvec, expect)
                for j in range(nvec):
                    assert_same_bits(Y[j], want[j], f"{name}{what}: SpMM of {nvec} vectors, vector {j}, sigma {None if sg is None else sg[j]}{turn}")
                if sg is None:
                    assert same_bits(Y[:, empty], np.zeros((nvec, len(empty)))), (name, what, "rows without entries give +0.0")


# ---- 1. product bits, as planned ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CASES)
def test_spmm_is_the_oracles_bit_for_bit(name):
    A, facts, sw = K.build(name)
    X, _, AX = spmm_reference(name)
    expect = K.spmm_kind(facts)
    describe(name, facts, {}, expect)
    with running(A, sw) as ctx:
        assert ctx.flags()["spmm"]
        assert_same_bits(ctx.spmv(X[0]), AX[0], f"{name}: spmv of column 0")
        check_spmm(ctx, name, facts, expect)


# ---- 2. all forms on every case that has clusters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c for c in K.SMALL if K.pattern(c)[1]["clusters"]] + ["walk"])
def test_every_form_gives_the_same_bits(name):
    A, facts, sw = K.build(name)
    for tokens, expect in forms(facts)[1:]:
        describe(name, facts, tokens, expect)
        with running(A, sw, **tokens) as ctx:
            check_spmm(ctx, name, facts, expect, what=f" {tokens}")


# ---- 3. more than one tile per workgroup --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tokens,tile,tiles,grid,most", [
    ("walk", {}, 512, 516, 512, 2), ("walk", {"spmm_tile": 256}, 256, 1031, 768, 2),
    ("clusters4", {"spmm_gstep": 2500}, 512, 18, 8, 3), ("clusters4", {"spmm_gstep": 1000}, 512, 18, 24, 1)])
def test_a_workgroup_crosses_a_tile_change(name, tokens, tile, tiles, grid, most):
    """`walk`: 516 tiles of 512 rows against 512 resident workgroups (an XCD owns 65 tiles, its 64 workgroups take them 64 apart:
    workgroup 0 of seven XCDs takes two), 1031 tiles of 256 rows against 768 (129 per XCD, 96 workgroups: 33 take two);
    `clusters4` under spmm-gstep: 18 tiles over 8 workgroups that take 2 or 3 consecutive tiles, and the same form with one tile each"""
    A, facts, sw = K.build(name)
    g, own = K.pipe_ownership(A.rows, tile, tokens.get("spmm_gstep"))
    assert -(-A.rows // tile) == tiles and g == grid and sorted(t for o in own for t in o) == list(range(tiles))
    assert max(len(o) for o in own) == most and (most >= 2 or "spmm_gstep" in tokens)
    expect = K.spmm_kind(facts, spmm_tile=tokens.get("spmm_tile"))
    assert expect[:2] == ("pipelined", tile)
    print(f"{name} {tokens}: pipelined, tile {tile}; {tiles} tiles over {grid} workgroups, at most {most} each"
          + (", consecutive tiles (spmm-gstep)" if "spmm_gstep" in tokens else ""))
    with running(A, sw, **tokens) as ctx:
        check_spmm(ctx, name, facts, expect, nvecs=(16, 17), what=f" {tokens}")


# ---- 4. fused residual norms, exact ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NORM_CASES)
def test_fused_residual_norms_are_exact(name):
    A, facts, sw, X, sigma, b, want = K.integer_system(name)
    for tokens, expect in forms(facts) + [({"spmm": 0}, None)]:
        with running(A, sw, **tokens) as ctx:
            for nvec in NVEC:
                for turn in ("", ", again"):
                    got = ctx.shifted_residuals(X[:nvec], b, sigma[:nvec])
                    if expect is not None:
                        assert (ctx.last_spmm_kind(), ctx.last_spmm_tile()) == expect[:2], (name, tokens, nvec)
                    assert_same_bits(got, want[:nvec], f"{name} {tokens}: residual norms of {nvec} shifts{turn}")


# ---- 5. the multi-RHS caller --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MULTI_CASES)
def test_solve_multi_set_up_reads_its_own_slab(name):
    A, facts, sw = K.build(name)
    X, _, AX = spmm_reference(name)
    B = np.random.default_rng(5000).standard_normal((max(NVEC), A.rows))
    expect = K.spmm_kind(facts)
    assert expect[:2] == {"gap513": ("pipelined", 256), "lengths": ("pipelined", 512)}[name]
    with running(A, sw) as ctx:
        for nrhs in (1, 16, 17):
            got = ctx.solve_multi(B[:nrhs], X0=X[:nrhs], max_iter=0)          # set-up only: r = b - A x0
            assert got["rc"] == 0 and not got["k"].any()
            assert (ctx.last_spmm_kind(), ctx.last_spmm_tile()) == expect[:2]
            assert same_bits(got["x"], X[:nrhs])
            for j in range(nrhs):
                assert_same_bits(got["r"][j], B[j] - AX[j], f"{name}: residual of column {j} of {nrhs}")
