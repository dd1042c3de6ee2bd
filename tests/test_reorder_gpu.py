"""`-m gpu`: BICG_PLAN="reorder=1|2" end to end on one rank. bicg_create renumbers the diag block (reverse Cuthill-McKee,
csrc/bicg_reorder.cpp) before it plans it; every vector the caller hands in or gets back crosses the permutation on the device
(k_permute_in / k_permute_out, csrc/bicg_reorder.hip), so the caller keeps its own numbering throughout.

Two meshes in RANDOM numbering (mpi_bicgstab_amd.mesh): m = 40 (64 000 rows), the smallest shape where the given numbering loses
its 16-bit column offsets, so that the plan visibly changes; m = 76 (438 976 rows, 7.09 M non-zeros), the smallest above the
6 M-non-zero line where the list-driven x window exists (k_spmv_jagw with a list: "jagw_list").

Products are compared bit for bit with the oracle's mult() (reference src/matrix.c:498-516) on the CALLER's matrix: the permuted
block keeps the stored order of every row's entries. Trajectories are compared at the tolerances of tests/test_mesh_gpu.py, whose
head comment derives them; renumbering changes only the association of the dot sums (the oracle's own scalars move by at most 2.9e-9
relative between A and P A P^T over these 8 iterations, 6e-12 over the 6 shifted ones)."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import mesh

pytestmark = pytest.mark.gpu
_dp = C.POINTER(C.c_double)
K_FIX = 8


def _context(A, **sw):
    """a context created under the given BICG_PLAN tokens; the tokens are cleared again whatever happens"""
    H.switches(**sw)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(**{k: None for k in sw})


@pytest.fixture(scope="module")
def small():
    """m = 40, random numbering: (A, coo, context without the switch, context with reorder=1)"""
    H.lib().bicg_comm_init_single(0)
    A = mesh.fem_unstructured(40, "random", scale_decades=2.0)
    plain, ro = _context(A), _context(A, reorder=1)
    yield A, A.to_coo(), plain, ro
    plain.close()
    ro.close()


@pytest.fixture(scope="module")
def large():
    """m = 76, random numbering: (A, coo, context with reorder=1)"""
    H.lib().bicg_comm_init_single(0)
    A = mesh.fem_unstructured(76, "random", scale_decades=2.0)
    ro = _context(A, reorder=1)
    yield A, A.to_coo(), ro
    ro.close()


def test_flags_and_info(small):
    A, _, plain, ro = small
    assert A.rows == 64000
    assert not plain.flags()["reordered"] and ro.flags()["reordered"]
    assert not plain.flags()["col16"] and ro.flags()["col16"]
    assert plain.reorder_info() is None
    _, stats = H.reorder_plan(H.single_rank_blocks(A))
    info = ro.reorder_info()
    for k in H.REORDER_STATS[:7]:
        assert info[k] == stats[k], (k, info, stats)
    assert info["microseconds"] > 0


def test_spmv_bit_for_bit_in_the_callers_numbering(small):
    A, (row, col, val), plain, ro = small
    x = np.random.default_rng(5).standard_normal(A.rows)
    want = O.spmv(A.rows, row, col, val, x)
    y0, y1 = plain.spmv(x), ro.spmv(x)
    assert np.array_equal(y0, want)
    assert np.array_equal(y1, want)
    assert np.array_equal(y0, y1)


def test_load_fetch_round_trip(small):
    A, _, _, ro = small
    rng = np.random.default_rng(6)
    x0, b = rng.standard_normal(A.rows), rng.standard_normal(A.rows)
    ro.load(x0, b)
    x, r = ro.fetch()
    assert np.array_equal(x, x0) and np.array_equal(r, b)


def test_dot(small):
    A, _, _, ro = small
    rng = np.random.default_rng(7)
    x = rng.standard_normal(A.rows)
    y = x + 0.5 * rng.standard_normal(A.rows)          # (x, y) ~ 64 000: a sum without cancellation, so a relative bound means something
    # the same 64 000 products summed in another association: the oracle's serial sum is off by about eps sqrt(n) |sum| / 3 = 1e-14
    for u, v in ((x, y), (x, x)):
        want = O.ddot(u, v)
        assert abs(ro.dot(u, v) - want) <= 1e-13 * abs(want)


def test_spmm_and_shifted_residuals(small):
    A, _, plain, ro = small
    rng = np.random.default_rng(8)
    X = rng.standard_normal((5, A.rows))
    sg = (np.arange(5) + 1.0) * 0.002
    assert ro.flags()["spmm"]
    Y, _ = ro.spmm(X, sg)
    for j in range(5):
        assert np.array_equal(Y[j], ro.spmv(X[j]) + sg[j] * X[j]), j
    b = rng.standard_normal(A.rows)
    got = np.asarray(ro.shifted_residuals(X, b, sg))
    want = np.array([np.linalg.norm(b - Y[j]) / np.linalg.norm(b) for j in range(5)])
    np.testing.assert_allclose(got, want, rtol=1e-12)
    # more vectors than the staging buffer holds at once (kSpmmCols = 16): the set crosses in chunks
    X20 = rng.standard_normal((20, A.rows))
    Y20, _ = ro.spmm(X20)
    for j in (0, 15, 16, 19):
        assert np.array_equal(Y20[j], plain.spmv(X20[j])), j


def test_shifted_solve(small):
    A, (row, col, val), _, ro = small
    sigma, seed = np.array([0.01, 0.02, 0.03, 0.04]), 1
    b = ro.spmv(np.ones(A.rows)) + sigma[seed] * np.ones(A.rows)
    got = ro.solve_shifted(b, sigma, seed, tol=0.0, max_iter=6, check_every=6, which="shifted_lopbicgstab")
    orc = O.solve_shifted(A.rows, row, col, val, b, sigma, seed, tol=0.0, max_iter=6, which="shifted_lopbicgstab")
    assert got["k"] == orc["k"] == 6
    tr = ro.trace(6)
    for key in ("alpha", "omega", "beta", "dotr"):
        np.testing.assert_allclose(tr[key], orc[key], rtol=1e-7, err_msg=key)
    for j in range(4):          # x comes back in the caller's order
        assert np.abs(got["x"][j] - orc["x"][j]).max() <= 1e-8 * np.abs(orc["x"][j]).max(), j


def test_dropin_gets_the_feature_from_the_environment(small):
    A, _, _, ro = small
    L = H.lib()
    b = ro.spmv(np.ones(A.rows))
    want = ro.solve("bicgstab", b, max_iter=K_FIX)
    blk = H.single_rank_blocks(A)
    H.switches(reorder=1)
    os.environ["BICG_MAX_ITER"] = str(K_FIX)
    os.environ["BICG_QUIET"] = "1"
    try:
        L.bicg_dropin_release()
        x, r = np.zeros(A.rows), b.copy()
        k = L.bicgstab(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), x.ctypes.data_as(_dp), r.ctypes.data_as(_dp))
        ctx = L.bicg_dropin_context(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info))
        assert ctx and int(L.bicg_ctx_flags(ctx)) & H.Context.FLAGS["reordered"]
        assert k == want["k"] == K_FIX
        assert np.array_equal(x, want["x"]) and np.array_equal(r, want["r"])
    finally:
        os.environ.pop("BICG_MAX_ITER", None)
        os.environ.pop("BICG_QUIET", None)
        L.bicg_dropin_release()
        H.switches(reorder=None)


def test_mode_2_reorders_only_where_the_numbering_is_the_problem(small):
    A, (row, col, val), plain, _ = small
    G = mesh.fem_unstructured(40, "generator", scale_decades=2.0)
    base, kept = _context(G), _context(G, reorder=2)
    try:
        assert not kept.flags()["reordered"] and kept.reorder_info() is None
        assert kept.flags() == base.flags() and kept.plan_info() == base.plan_info()
    finally:
        base.close()
        kept.close()
    ro2 = _context(A, reorder=2)
    try:
        assert ro2.flags()["reordered"] and ro2.flags()["col16"]
        x = np.cos(np.arange(A.rows))
        assert np.array_equal(ro2.spmv(x), plain.spmv(x))
    finally:
        ro2.close()


def test_the_list_driven_window_on_the_reordered_mesh(large):
    A, (row, col, val), ro = large
    assert A.rows == 76 ** 3 and A.nnz > 6_000_000
    fl = ro.flags()
    assert fl["reordered"] and fl["window"] and fl["col16"], fl
    H.product_kernels()
    ro.spmv_bench(3)
    assert H.product_kernels() == ["jagw_list"]
    plain = _context(A)
    try:
        assert not plain.flags()["col16"] and not plain.flags()["reordered"]
        H.product_kernels()
        plain.spmv_bench(3)
        assert H.product_kernels() == ["jagd"]
    finally:
        plain.close()
    x = np.random.default_rng(9).standard_normal(A.rows)
    assert np.array_equal(ro.spmv(x), O.spmv(A.rows, row, col, val, x))


def test_first_iterations_against_the_oracle(large):
    A, (row, col, val), ro = large
    b = ro.spmv(np.ones(A.rows))
    assert np.array_equal(b, O.spmv(A.rows, row, col, val, np.ones(A.rows)))
    for method in ("bicgstab", "ca_bicgstab", "pipe_bicgstab", "pipe_bicgstab_rr"):
        H.product_kernels()
        got = ro.solve(method, b, tol=0.0, max_iter=K_FIX, krr=5, nrr=1, check_every=K_FIX)
        orc = O.solve(method, A.rows, row, col, val, b, tol=0.0, max_iter=K_FIX, krr=5, nrr=1)
        assert got["k"] == orc["k"] == K_FIX
        assert "jagw_list" in H.product_kernels(), method
        tr = ro.trace(K_FIX)
        for key in ("alpha", "omega", "beta", "dotr"):
            np.testing.assert_allclose(tr[key], orc[key], rtol=1e-6, err_msg=f"{method} {key}")
        assert np.abs(got["x"] - orc["x"]).max() <= 1e-6 * np.abs(orc["x"]).max(), method
