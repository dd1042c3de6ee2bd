"""`-m gpu`, one rank: bicg_update_values / bicg_update_values_device (csrc/bicg_refresh.cpp, bicg_refresh.hip; DESIGN.md section
4.18) -- new values for a resident matrix, same sparsity pattern, written in place.

The bar everywhere is BYTES: a context created on A and updated to A2 must compute what a fresh context created on A2 under the same
tokens computes -- the products, the iterates, the residuals and the traces of the solves -- bit for bit, because after the update
every stored copy of the values holds what bicg_create would have put there. Where the product is the oracle's bit for bit (every
layout but rows over lanes and the long rows of CSR row blocks, whose sums are associated differently), spmv is compared with
oracle_lib.spmv on A2 as well.

`revalued` (tests/test_update_values.py): val * s, s in [1.0, 1.2] on the diagonal and in [0.9, 1.1] elsewhere. Every case first
takes a product-only update whose matrix also has three off-diagonal values set to exactly 0.0 (a stored zero is a value), then
the update the solves run on.

Shapes are the smallest that reach the layout a case is there for; each case asserts the flags / kernels it is about."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import mesh, synth
from test_update_values import revalued

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE = dict(tol=1e-10, max_iter=300, record_trace=1)


@pytest.fixture(scope="module", autouse=True)
def _single_rank():
    H.lib().bicg_comm_init_single(0)      # (once: a new communicator orphans the contexts of the one before)
    yield


def _context(A, **sw):
    """a context created under the given tokens; the tokens are cleared again whatever happens"""
    H.switches(**sw)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(**{k: None for k in sw})


def _vectors(n, count, seed=3):
    return np.random.default_rng(seed).standard_normal((count, n))


def products(ctx, n):
    """spmv of two vectors and, where the context has it, spmm of five -- as bytes"""
    X = _vectors(n, 5)
    out = [ctx.spmv(X[0]).tobytes(), ctx.spmv(X[1]).tobytes()]
    if ctx.flags()["spmm"]:
        out.append(ctx.spmm(X)[0].tobytes())
    return out


def solved(ctx, method, b, **opts):
    got = ctx.solve(method, b, **(opts or SOLVE))
    tr = ctx.trace(got["k"])
    return (got["k"], got["x"].tobytes(), got["r"].tobytes(), tuple(tr[k].tobytes() for k in ("alpha", "omega", "beta", "dotr")))


def csr_blocks(ctx):
    """CSR row blocks of the context: plan_info's row_blocks counts the workgroups of a product, sliced 256-row groups included"""
    info = ctx.plan_info()
    return info["row_blocks"] - -(-info["sell_rows"] // 256)


def solves(ctx, A2):
    b = A2.matvec(np.ones(A2.rows))
    out = [solved(ctx, "bicgstab", b)]
    if ctx.flags()["persist"]:
        out.append(solved(ctx, "pipe_bicgstab", b))
    return out


def plan_facts(ctx):
    return (ctx.plan_info(), ctx.device_matrix_bytes(), ctx.uniform_entries(), ctx.constant_entries(), ctx.masked_rows())


def facts(ctx):
    return (ctx.flags(),) + plan_facts(ctx)


def update(ctx, A2, how="host"):
    """update_values with the allocation count taken around the call itself; returns the call's return value"""
    if how == "device":
        import torch
        src = torch.from_numpy(np.ascontiguousarray(A2.val)).cuda()
        torch.cuda.synchronize()
    else:
        src = A2
    before = H.device_allocations()
    rc = ctx.update_values(src)
    assert H.device_allocations() == before, "the update left an allocation behind (or freed one)"
    return rc


def oracle_spmv(A, x):
    row, col, val = A.to_coo()
    return O.spmv(A.rows, row, col, val, x)


@functools.lru_cache(maxsize=None)
def _mesh(kind, m=40):
    return mesh.fem_unstructured(m, kind, scale_decades=2.0)


def mixed_rows(n=16000, nlong=16, length=3000, seed=4):
    """five diagonals on n rows with `nlong` rows, 1000 apart, replaced by rows of `length` scattered entries that keep the row
    dominant: their 256-row groups go to the CSR row blocks (48 blocks here, three per group), the others stay sliced; plain
    BiCGStab converges in about 8 iterations"""
    A = synth.from_offsets(n, (0, 1, -1, 37, -37), 9.0, seed=5)
    rng = np.random.default_rng(seed)
    ptr = A.ptr.astype(np.int64)
    lens = np.diff(ptr)
    long_rows = 500 + 1000 * np.arange(nlong)
    new_lens = lens.copy()
    new_lens[long_rows] = length
    out = np.concatenate(([0], np.cumsum(new_lens)))
    col, val = np.empty(out[-1], dtype=np.uint32), np.empty(out[-1])
    rid = np.repeat(np.arange(n), lens)
    keep = np.ones(n, dtype=bool)
    keep[long_rows] = False
    m = keep[rid]
    dst = (out[:-1][rid] + (np.arange(ptr[-1]) - ptr[:-1][rid]))[m]
    col[dst], val[dst] = A.col[m], A.val[m]
    for r in long_rows:
        c = rng.choice(n, size=length, replace=False)
        if r not in c:
            c[0] = r
        c.sort()
        v = -(0.5 + 0.5 * rng.random(length)) / length
        v[c == r] = 9.0 + rng.random()
        col[out[r]:out[r + 1]], val[out[r]:out[r + 1]] = c, v
    return synth.CSR(n, n, out.astype(np.uint32), col, val)


LONG_ROWS = {100: 3000, 2500: 2000, 4100: 5000, 6000: 900}
OFFSETS7 = (0, 1, -1, 37, -37, 2999, -2999)
# name -> (matrix, tokens, what the context must be for the case to reach its layout)
CASES = {
    "padded16_uniform_persist": (lambda: synth.from_offsets(30011, OFFSETS7, 9.0, seed=5), {},
                                 lambda c: c.flags()["col16"] and c.flags()["uniform"] and c.flags()["persist"]),
    "padded16_no_persist": (lambda: synth.from_offsets(30011, OFFSETS7, 9.0, seed=5), {"persist": 0},
                            lambda c: c.flags()["handover"] and not c.flags()["persist"]),
    "padded32": (lambda: synth.from_offsets(70001, (0, 1, -1, 40000, -40000), 6.0, seed=2), {},
                 lambda c: not c.flags()["col16"] and not c.flags()["jagged"] and c.flags()["all_sell"]),
    "jagged_run_windows": (lambda: synth.fem_like(n=117 * 117 * 3), {}, lambda c: c.flags()["jagged"] and c.flags()["window"]),
    # (the list-driven window is a plan of large blocks -- 6 M non-zeros and more, plan_windows in csrc/bicg_sell_plan.cpp: the
    # m = 40 mesh in this numbering gets run-free gathers instead, so this case takes the m = 76 mesh of tests/test_reorder_gpu.py)
    "jagged_list_window": (lambda: _mesh("rcm", 76), {}, lambda c: c.flags()["jagged"] and "jagw_list" in _kernels(c)),
    "jagged_no_window": (lambda: _mesh("random"), {}, lambda c: c.flags()["jagged"] and "jagd" in _kernels(c)),
    # (persistent as well: the source map of the persistent plan is then translated to the caller's entry numbers, bicg_create.cpp)
    "reordered": (lambda: _mesh("random"), {"reorder": 1}, lambda c: c.flags()["reordered"] and c.flags()["persist"]),
    "row_blocks_beside_slices": (lambda: synth.random_rows(8000, 12, seed=3, empty_frac=0.1, long_rows=LONG_ROWS), {},
                                 lambda c: 0 < c.plan_info()["sell_rows"] < c.plan_info()["rows"] and not c.flags()["all_sell"] and csr_blocks(c) == 11),
    # (11 CSR row blocks above: the product's second launch is smaller than the 32 shards; 48 here)
    "row_blocks_48": (mixed_rows, {}, lambda c: 0 < c.plan_info()["sell_rows"] < c.plan_info()["rows"] and csr_blocks(c) >= 32),
    "rows_over_lanes": (lambda: synth.banded(4099, 200), {}, lambda c: c.flags()["rowsplit"]),
}
for _n in (1, 63, 65, 257):
    CASES["n%d" % _n] = (functools.partial(synth.from_offsets, _n, (0, 1, -1, 3, -3), 5.0, seed=_n), {}, lambda c: True)


def _kernels(ctx):
    """names of the product kernels one spmv of this context launches"""
    H.product_kernels()
    ctx.spmv(np.ones(ctx.n))
    return H.product_kernels()


@pytest.mark.parametrize("name", list(CASES))
def test_an_updated_context_is_a_fresh_one(name):
    make, sw, reaches = CASES[name]
    A = make()
    A1, A2 = revalued(A, 22, zeros=3 if A.rows > 3 else 0), revalued(A, 21)
    ctx = _context(A, **sw)
    assert reaches(ctx), (name, ctx.flags(), ctx.plan_info())
    if name == "padded16_uniform_persist":
        ctx.solve("pipe_bicgstab", A.matvec(np.ones(A.rows)), **SOLVE)      # graphs, persistent launches and traces exist before the update
    was = facts(ctx)
    # ---- product-only update, with stored zeros
    assert update(ctx, A1) == 0
    assert facts(ctx) == was, "the update changed the context's plan facts"
    fresh1 = _context(A1, **sw)
    assert plan_facts(fresh1) == was[1:], "a fresh context on the new values is planned differently: the case does not test what it says"
    assert products(ctx, A.rows) == products(fresh1, A.rows), name
    fresh1.close()
    # ---- the update the solves run on
    assert update(ctx, A2) == 0
    assert facts(ctx) == was, "the update changed the context's plan facts"
    fresh = _context(A2, **sw)
    assert plan_facts(fresh) == was[1:] and reaches(fresh)
    assert products(ctx, A.rows) == products(fresh, A.rows), name
    if name != "rows_over_lanes":
        x = _vectors(A.rows, 1)[0]
        y, want = ctx.spmv(x), oracle_spmv(A2, x)
        if name.startswith("row_blocks"):
            # the CSR row-block kernel spreads a row longer than one 2048-entry chunk over a workgroup: its sum is associated
            # differently from the oracle's (tests/test_gpu_parity.py: 1e-13 x sum |a_ij x_j|); every other row, in a row block or in
            # a slice, is summed in stored order and is the oracle's bit for bit
            short = np.diff(A.ptr.astype(np.int64)) <= 2048
            assert not short.all()
            assert y[short].tobytes() == want[short].tobytes(), "spmv after the update is not the oracle's on the rows summed in order"
            absA = synth.CSR(A2.rows, A2.cols, A2.ptr, A2.col, np.abs(A2.val))
            assert np.all(np.abs(y - want) <= 1e-13 * absA.matvec(np.abs(x)))
        else:
            assert y.tobytes() == want.tobytes(), "spmv after the update is not the oracle's on the new values"
    assert solves(ctx, A2) == solves(fresh, A2), name
    ctx.close()
    fresh.close()


@pytest.mark.parametrize("name", ["padded16_uniform_persist", "jagged_run_windows", "row_blocks_beside_slices", "row_blocks_48"])
def test_round_trip_leaves_nothing_behind(name):
    """A -> A2 -> A gives the bytes of a context that was never touched: padding is still zero, nothing stale is left"""
    make, sw, _ = CASES[name]
    A = make()
    ctx, untouched = _context(A, **sw), _context(A, **sw)
    assert update(ctx, revalued(A, 21)) == 0
    assert products(ctx, A.rows) != products(untouched, A.rows)
    assert update(ctx, A) == 0
    assert products(ctx, A.rows) == products(untouched, A.rows)
    assert solves(ctx, A) == solves(untouched, A)
    ctx.close()
    untouched.close()


@pytest.mark.parametrize("name", ["padded16_uniform_persist", "jagged_list_window"])
def test_device_arrays_give_the_bytes_of_host_arrays(name):
    make, sw, reaches = CASES[name]
    A = make()
    A2 = revalued(A, 21)
    host, dev = _context(A, **sw), _context(A, **sw)
    assert reaches(dev)
    assert update(host, A2, "host") == 0 and update(dev, A2, "device") == 0
    assert products(dev, A.rows) == products(host, A.rows)
    assert solves(dev, A2) == solves(host, A2)
    host.close()
    dev.close()


def test_values_held_in_lists_are_verified_never_rewritten():
    """synth.grid7(64, 12, 16, wrap_y=True), the "grid7_wrap_y" entry of tests/test_sell_plan.py: every slice is constant or masked.
    (stencil7(12) is planned with jagged slices -- padding its 12-row lines would add more than 2 % -- and holds no value in a list.)"""
    A = synth.grid7(64, 12, 16, wrap_y=True)
    ctx = _context(A)
    assert ctx.constant_entries() > 0 and ctx.masked_rows() > 0
    before = products(ctx, A.rows)
    same = synth.CSR(A.rows, A.cols, A.ptr.copy(), A.col.copy(), A.val.copy())
    assert update(ctx, same) == 0
    assert products(ctx, A.rows) == before
    changed = synth.CSR(A.rows, A.cols, A.ptr, A.col, A.val.copy())
    r = 64 * (12 * 8 + 6) + 30                                      # an interior row: its diagonal entry
    j = int(A.ptr[r]) + int(np.flatnonzero(A.col[int(A.ptr[r]):int(A.ptr[r + 1])] == r)[0])
    changed.val[j] *= 1.25
    assert update(ctx, changed) == 1
    assert update(ctx, changed, "device") == 1
    assert products(ctx, A.rows) == before, "a refused update wrote something"
    assert update(ctx, same) == 0                                   # ... and the context still takes a valid one
    ctx.close()
    # the same matrix planned without list-held values accepts the change
    free = _context(A, constant=0)
    assert free.constant_entries() == 0 and free.masked_rows() == 0
    assert update(free, changed) == 0
    fresh = _context(changed, constant=0)
    assert products(free, A.rows) == products(fresh, A.rows)
    assert solves(free, changed) == solves(fresh, changed)
    free.close()
    fresh.close()


def _with_identity_rows(A, lo, hi):
    """A with the rows lo .. hi - 1 replaced by rows of the identity (Dirichlet nodes)"""
    ptr = A.ptr.astype(np.int64)
    keep = np.ones(A.nnz, dtype=bool)
    rows = np.repeat(np.arange(A.rows), np.diff(ptr))
    inside = (rows >= lo) & (rows < hi)
    keep[inside & (A.col != rows)] = False
    val = A.val.copy()
    val[inside] = 1.0
    counts = np.bincount(rows[keep], minlength=A.rows)
    newptr = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
    return synth.CSR(A.rows, A.cols, newptr, A.col[keep].copy(), val[keep])


def test_identity_rows_in_a_varying_matrix():
    """constant slices of Dirichlet rows pass the verification while everything else changes"""
    A = _with_identity_rows(synth.from_offsets(4099, (0, 1, -1, 37, -37), 9.0, seed=5), 640, 768)
    ctx = _context(A)
    assert ctx.constant_entries() > 0
    A2 = revalued(A, 21)
    rows = np.repeat(np.arange(A.rows), np.diff(A.ptr.astype(np.int64)))
    ident = (rows >= 640) & (rows < 768)
    A2.val[ident] = 1.0                                             # the update leaves those rows alone
    assert update(ctx, A2) == 0
    fresh = _context(A2)
    assert fresh.constant_entries() == ctx.constant_entries()
    assert products(ctx, A.rows) == products(fresh, A.rows)
    assert solves(ctx, A2) == solves(fresh, A2)
    before = products(ctx, A.rows)
    A3 = synth.CSR(A.rows, A.cols, A.ptr, A.col, A2.val.copy())
    A3.val[np.flatnonzero(ident)[70]] = 2.0
    assert update(ctx, A3) == 1
    assert products(ctx, A.rows) == before
    ctx.close()
    fresh.close()


def test_multi_rhs_after_an_update():
    """solve_multi of 5 columns: the first call happens before the update, so the set buffers already exist"""
    from test_multi_rhs_gpu import solutions, whole_state
    A = synth.from_offsets(30011, OFFSETS7, 9.0, seed=5)
    A2 = revalued(A, 21)
    xs = solutions(A.rows, 5)
    B = np.array([A2.matvec(x) for x in xs])
    ctx = _context(A)
    ctx.solve_multi(np.array([A.matvec(x) for x in xs]), tol=1e-12, record_trace=1)
    assert update(ctx, A2) == 0
    fresh = _context(A2)
    got, want = ctx.solve_multi(B, tol=1e-12, record_trace=1), fresh.solve_multi(B, tol=1e-12, record_trace=1)
    assert whole_state(ctx, got) == whole_state(fresh, want)
    ctx.close()
    fresh.close()


def test_null_arguments_are_refused():
    L = H.lib()
    A = synth.from_offsets(257, (0, 1, -1), 5.0, seed=1)
    ctx = _context(A)
    val = np.ascontiguousarray(A.val)
    assert L.bicg_update_values(None, val.ctypes.data_as(C.POINTER(C.c_double)), None) == -1
    assert L.bicg_update_values(ctx.h, None, None) == -1
    assert L.bicg_update_values_device(None, None, None) == -1
    assert L.bicg_update_values_device(ctx.h, None, None) == -1
    assert ctx.update_values(A) == 0                                # offd_val = NULL: the context has no offd entries
    ctx.close()


DROPIN = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %(root)r)
from mpi_bicgstab_amd import hipsolver as H, synth
L = H.lib()
L.bicg_comm_init_single(0)
A = synth.from_offsets(30011, (0, 1, -1, 37, -37, 2999, -2999), 9.0, seed=5)
blk = H.single_rank_blocks(A)
b = A.matvec(np.ones(A.rows))
dp = C.POINTER(C.c_double)
def call():
    x, r = np.zeros(A.rows), b.copy()
    k = L.bicgstab(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), x.ctypes.data_as(dp), r.ctypes.data_as(dp))
    return k, x, r
call()
blk._keep[0][12345] *= 1.5          # in-place edit of one value: same arrays, same pattern
k, x, r = call()
h, m = C.c_uint(0), C.c_uint(0)
L.bicg_dropin_stats(C.byref(h), C.byref(m))
L.bicg_dropin_release()
np.savez(sys.argv[1], k=k, x=x, r=r, refreshes=H.dropin_refreshes(), hits=h.value, misses=m.value)
"""


def _dropin_child(tmp_path, tag, cache):
    env = {k: v for k, v in os.environ.items() if k != "BICG_DROPIN_CACHE"}
    env.update(BICG_QUIET="1", BICG_MAX_ITER="40")
    if cache is not None:
        env["BICG_DROPIN_CACHE"] = cache
    out = str(tmp_path / (tag + ".npz"))
    p = subprocess.run([sys.executable, "-c", DROPIN % dict(root=ROOT), out], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(out)


def test_dropin_cache_2_updates_the_resident_context(tmp_path):
    off, refresh, default = (_dropin_child(tmp_path, t, c) for t, c in (("off", "0"), ("refresh", "2"), ("default", None)))
    assert int(refresh["refreshes"]) == 1 and (int(refresh["hits"]), int(refresh["misses"])) == (0, 2)
    assert int(default["refreshes"]) == 0 and int(off["refreshes"]) == 0
    assert (int(default["hits"]), int(default["misses"])) == (0, 2)
    for got in (refresh, default):
        assert int(got["k"]) == int(off["k"]) and got["x"].tobytes() == off["x"].tobytes() and got["r"].tobytes() == off["r"].tobytes()


def test_a_context_planned_on_the_device_is_served_too():
    """bicg_create_device_csr keeps ptr on the device and plans padded slices; a 64^3 grid is the smallest whose lines fill whole
    64-row slices. With its constant coefficients every slice holds its values in a list: the same values pass, a changed one is
    refused; planned under constant=0 the context takes new values and multiplies like the oracle."""
    W = (6.5, -1.2, -0.8, -1.1, -0.9, -1.0, -1.0)
    A = synth.stencil7(64, W)
    ctx = H.Context.stencil7_on_device(64, W)[0]
    assert ctx.constant_entries() > 0
    x = _vectors(A.rows, 1)[0]
    before = ctx.spmv(x).tobytes()
    assert update(ctx, A) == 0 and ctx.spmv(x).tobytes() == before
    A2 = revalued(A, 21)
    assert update(ctx, A2) == 1 and update(ctx, A2, "device") == 1
    assert ctx.spmv(x).tobytes() == before, "a refused update wrote something"
    ctx.close()
    H.switches(constant=0)
    try:
        free = H.Context.stencil7_on_device(64, W)[0]
    finally:
        H.switches(constant=None)
    assert free.constant_entries() == 0 and not free.flags()["jagged"]
    given = oracle_spmv(A, x).tobytes()
    assert free.spmv(x).tobytes() == given
    was = plan_facts(free)
    assert update(free, A2) == 0 and plan_facts(free) == was
    assert free.spmv(x).tobytes() == oracle_spmv(A2, x).tobytes()
    assert update(free, A, "device") == 0 and free.spmv(x).tobytes() == given
    free.close()
