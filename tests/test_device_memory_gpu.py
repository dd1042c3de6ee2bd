"""`-m gpu`: a context gives back every device allocation it made (csrc/bicg_host.h, struct DevOwner). The library counts the
allocations of its host code that are not yet freed (bicg_device_allocations); the count after close() must equal the count before
the context was built -- exactly, so a single leaked array of a few bytes fails, which the free-memory tests with their 8 MiB margin
(tests/test_gpu_parity.py, tests/test_multi_rhs_gpu.py) cannot see. In between every call that allocates lazily runs, those with a
growing buffer twice so that the buffer regrows.

Each case is the smallest shape that reaches its set of optional arrays of the context; along the way one product is checked: a
context that frees the right memory must also still point at it. y = A x is compared bit for bit with the oracle (reference
src/matrix.c:498-516; rows of at most 2048 entries, as in tests/test_gpu_parity.py) and with synth.CSR.matvec. numpy adds a row's
products pairwise, the kernels in stored order: two sums of the same n products differ by at most 2 gamma_n sum |a_ij x_j| with
gamma_n = n u / (1 - n u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); the bar below takes
n + 2 for n, which covers the denominator and the rounding of the bar itself for the rows used here (n <= 3000)."""
import numpy as np
import pytest

import mp_workers as W
import oracle_lib as O
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import mesh, synth

pytestmark = pytest.mark.gpu
WALL_LIMIT = 240.0      # seconds for the two-rank case (tests/test_multi_rhs_ranks_gpu.py)
GRID_WEIGHTS = (6.5, -1.2, -0.8, -1.1, -0.9, -1.0, -1.0)


def check_product(y, A, x, lo=0, nranks=1):
    """y = (A x)[lo : lo + len(y)]: the oracle's bits, and numpy's sum within the re-association bar of the module docstring"""
    rows = slice(lo, lo + len(y))
    row, col, val = A.to_coo()
    lens = np.diff(A.ptr.astype(np.int64))[rows]
    want = O.spmv(A.rows, row, col, val, x, nranks=nranks)[rows]
    assert np.array_equal(y[lens <= 2048], want[lens <= 2048])
    mag = synth.CSR(A.rows, A.cols, A.ptr, A.col, np.abs(A.val)).matvec(np.abs(x))[rows]
    assert np.all(np.abs(y - A.matvec(x)[rows]) <= 2.0 * (lens + 2) * 2.0 ** -53 * mag)


def exercise(ctx, b):
    """every call of a context that allocates lazily (the solvers' results are other tests' business)"""
    n = len(b)
    rng = np.random.default_rng(7)
    ctx.solve("bicgstab", b, tol=0.0, max_iter=3, check_every=3, record_trace=1)
    ctx.solve("pipe_bicgstab", b, tol=0.0, max_iter=7, check_every=7, record_trace=1)      # the trace regrows
    ctx.solve_shifted(b, 0.01 * (np.arange(3) + 1.0), 1, tol=0.0, max_iter=4, check_every=4)
    ctx.solve_shifted(b, 0.01 * (np.arange(5) + 1.0), 2, tol=0.0, max_iter=4, check_every=4)      # the shift buffers regrow
    ctx.solve_shifted(b, 0.02 * 2.0 ** np.arange(5), 4, tol=0.0, max_iter=4, check_every=2, which="shifted_lopbicg_switching")
    if ctx.flags()["spmm"]:
        ctx.spmm(rng.standard_normal((3, n)), 0.25 * np.arange(3))
    ctx.solve_multi(np.stack([b, 0.5 * b, rng.standard_normal(n)]), tol=0.0, max_iter=4, check_every=2, record_trace=1)
    return ctx.spmv(np.ones(n))


def _host(A, **sw):
    def build():
        H.switches(**sw)
        try:
            return H.Context(H.single_rank_blocks(A()))
        finally:
            H.switches(**{k: None for k in sw})
    return A, build


def _device(m, **sw):
    def build():
        H.switches(**sw)
        try:
            return H.Context.stencil7_on_device(m, GRID_WEIGHTS)[0]
        finally:
            H.switches(**{k: None for k in sw})
    return (lambda: synth.stencil7(m, GRID_WEIGHTS)), build


def _mesh_rcm(tmp_path_factory):
    cache = tmp_path_factory.getbasetemp() / "mesh_cache"      # shared with tests/test_mesh_gpu.py: assembled once per session
    cache.mkdir(exist_ok=True)
    return mesh.fem_unstructured(117, "rcm", scale_decades=2.0, cache_dir=str(cache))


def _kernel_of_a_product(ctx, n):
    H.product_kernels()
    ctx.spmv(np.ones(n))
    return H.product_kernels()


# name -> (the matrix on the host, the context, what proves that the context has the optional arrays the case is here for)
CASES = {
    # padded 16-bit slices, uniform lists, cluster windows
    "transport_like": lambda t: _host(lambda: synth.transport_like(n=40_000)) + (
        lambda c, fl: fl["col16"] and fl["uniform"] and not fl["jagged"] and not fl["constant"] and c.uniform_entries() > 0,),
    # constant and masked slices, descriptors, the stencil plan
    "grid7": lambda t: _host(lambda: synth.grid7(64, 8, 8)) + (
        lambda c, fl: fl["constant"] and c.masked_rows() > 0 and c.stencil_info()["on"] == 1,),
    # bicg_create_device_csr
    "device_planned": lambda t: _device(64) + (
        lambda c, fl: fl["constant"] and c.masked_rows() > 0 and c.plan_collisions() == 0,),
    # ... and its rewrite of the lists after k_plan_verify
    "device_planned_collisions": lambda t: _device(64, plan_collide=1) + (lambda c, fl: c.plan_collisions() > 0,),
    # jagged slices, windows, permutation, lane_info (the three-trip product needs the per-lane words)
    "fem_like": lambda t: _host(lambda: synth.fem_like(n=20_000)) + (
        lambda c, fl: fl["jagged"] and fl["window"] and fl["col16"] and _kernel_of_a_product(c, 20_000) == ["jagw"],),
    # the list-driven window
    "mesh_rcm": lambda t: _host(lambda: _mesh_rcm(t)) + (
        lambda c, fl: fl["jagged"] and fl["window"] and _kernel_of_a_product(c, 117 ** 3) == ["jagw_list"],),
    # CSR row blocks beside slices: 17 sliced-ELL groups and 14 row blocks, two launches per product
    "random_rows": lambda t: _host(lambda: synth.random_rows(5_000, 40, seed=11, empty_frac=0.15,
                                                             long_rows={5: 2500, 1777: 2999, 2999: 2100})) + (
        lambda c, fl: not fl["all_sell"] and c.plan_info()["sell_rows"] < 5_000 and "csr" in _kernel_of_a_product(c, 5_000),),
    # the reordered context
    "fem_like_reordered": lambda t: _host(lambda: synth.fem_like(n=20_000), reorder=1) + (lambda c, fl: fl["reordered"],),
}


@pytest.mark.parametrize("name", list(CASES))
def test_a_context_gives_back_every_allocation(name, tmp_path_factory):
    H.lib().bicg_comm_init_single(0)
    make_A, build, reached = CASES[name](tmp_path_factory)
    A = make_A()
    x = np.random.default_rng(3).standard_normal(A.rows)
    before = H.device_allocations()
    ctx = build()
    assert H.device_allocations() > before
    assert reached(ctx, ctx.flags()), (name, ctx.flags(), ctx.plan_info())
    b = exercise(ctx, A.matvec(np.ones(A.rows)))
    check_product(b, A, np.ones(A.rows))
    check_product(ctx.spmv(x), A, x)
    ctx.close()
    assert H.device_allocations() == before


def test_two_ranks_give_back_every_allocation():
    """two ranks on the host transport with the peer-to-peer data path (tests/mp_workers.py, memory_worker): the launch with the
    exchange inside (its group list), the push tables, the set-exchange buffers, the persistent plan; each rank asserts its own
    balance before it exits"""
    W.run_ranks(W.memory_worker, 2, "offsets+p2p", WALL_LIMIT)
