"""`-m gpu`, one rank: the device-resident vector calls (bicg_load_device / bicg_fetch_device / bicg_solve_device / bicg_spmv_device /
bicg_solve_multi_device, csrc/bicg_api.cpp, bicg_multi.cpp, bicg_vecio.hip) through Context.load / fetch /
solve / spmv / solve_multi on CUDA float64 torch tensors.

The bar everywhere is BYTES: the device variant runs the same solver on the same numbers, so k, x, r, dot_r, dot_zero,
breakdown_iteration and the traces are bit-identical to the host variant's on the same context (which other tests pin to the oracle).

Matrices: synth.from_offsets(n, (0, 1, -1, 37, -37), 9.0, seed=5) with n = 259 (one partly filled block of the crossing kernel) and
n = 16001 (n % 4 == 1: the tail lane; 16 blocks); mesh.fem_unstructured(40, "random", scale_decades=2.0), the smallest shape
tests/test_reorder_gpu.py uses for the permutation, without and with reorder=1 (the crossing then gathers through perm / inv)."""
import ctypes as C

import numpy as np
import pytest
import torch

from mpi_bicgstab_amd import hipsolver as H
from mpi_bicgstab_amd import mesh, synth

pytestmark = pytest.mark.gpu
SOLVE = dict(tol=1e-10, max_iter=300, record_trace=1)
METHODS = ("bicgstab", "ca_bicgstab", "pipe_bicgstab", "pipe_bicgstab_rr")
NAMES = ("n259", "n16001", "mesh", "mesh_ro")
SENTINEL = -7.25


def _context(A, **sw):
    """a context created under the given tokens; the tokens are cleared again whatever happens"""
    H.switches(**sw)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(**{k: None for k in sw})


def _matrix(name):
    if name.startswith("n"):
        return synth.from_offsets(int(name[1:]), (0, 1, -1, 37, -37), 9.0, seed=5)
    return mesh.fem_unstructured(40, "random", scale_decades=2.0)


@pytest.fixture(scope="module")
def cases():
    """name -> (A, context, x0, b, b2): made once, the arrays read-only"""
    H.lib().bicg_comm_init_single(0)      # (once: a new communicator orphans the contexts of the one before)
    out, made = {}, {}
    for name in NAMES:
        key = name.replace("_ro", "")
        if key not in made:
            A = _matrix(key)
            rng = np.random.default_rng(11)
            x0 = 0.1 * rng.standard_normal(A.rows)
            b, b2 = A.matvec(1.0 + 0.5 * rng.random(A.rows)), A.matvec(1.0 + 0.5 * rng.random(A.rows))
            for a in (x0, b, b2):
                a.setflags(write=False)
            made[key] = (A, x0, b, b2)
        A, x0, b, b2 = made[key]
        out[name] = (A, _context(A, reorder=1) if name.endswith("_ro") else _context(A), x0, b, b2)
    assert out["mesh_ro"][1].flags()["reordered"] and not out["mesh"][1].flags()["reordered"]
    yield out
    for _, ctx, *_ in out.values():
        ctx.close()


def dev(a):
    t = torch.from_numpy(np.array(a, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy()


def inner_view(a, lead=1, tail=1):
    """(buffer, view): `a` as a view that starts `lead` elements into a larger buffer full of SENTINEL -- lead = 1: 8-byte aligned only"""
    a = np.asarray(a, dtype=np.float64)
    buf = torch.full((lead + a.size + tail,), SENTINEL, dtype=torch.float64, device="cuda")
    view = buf[lead:lead + a.size]
    view.copy_(torch.from_numpy(np.array(a)))
    torch.cuda.synchronize()
    assert view.data_ptr() % 16 == (8 * lead) % 16
    return buf, view


def outside_untouched(buf, n, lead=1):
    h = host(buf)
    return bool(np.all(h[:lead] == SENTINEL) and np.all(h[lead + n:] == SENTINEL))


def state(ctx, got):
    """everything a solve reports, as bytes"""
    tohost = (lambda t: host(t)) if hasattr(got["x"], "data_ptr") else (lambda a: a)
    k, q = got["k"], got["result"]
    tr = ctx.trace(k)
    return (k, q.iterations, q.breakdown_iteration, np.float64(q.dot_r).tobytes(), np.float64(q.dot_zero).tobytes(),
            tohost(got["x"]).tobytes(), tohost(got["r"]).tobytes(), tuple(tr[key].tobytes() for key in ("alpha", "omega", "beta", "dotr")))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", NAMES)
def test_solve_on_tensors_is_the_host_solve_bit_for_bit(cases, name, method):
    A, ctx, x0, b, _ = cases[name]
    want = state(ctx, ctx.solve(method, b, x0=x0, **SOLVE))
    tb, tx0 = dev(b), dev(x0)
    got = ctx.solve(method, tb, x0=tx0, **SOLVE)
    assert got["x"].is_cuda and got["r"].is_cuda and got["x"].data_ptr() != tx0.data_ptr() and got["r"].data_ptr() != tb.data_ptr()
    assert state(ctx, got) == want
    assert host(tb).tobytes() == b.tobytes() and host(tx0).tobytes() == x0.tobytes(), "the caller's b / x0 were modified"
    # without x0: zeros, as in the numpy form
    assert state(ctx, ctx.solve(method, tb, **SOLVE)) == state(ctx, ctx.solve(method, b, **SOLVE))


@pytest.mark.parametrize("name", NAMES)
def test_views_that_are_only_8_byte_aligned(cases, name):
    """every input and output starts one element into a larger buffer: the same bytes, and nothing outside the views is written"""
    A, ctx, x0, b, _ = cases[name]
    n = A.rows
    want = state(ctx, ctx.solve("bicgstab", b, x0=x0, **SOLVE))
    xbuf, xv = inner_view(x0)
    rbuf, rv = inner_view(b)
    got = ctx.solve("bicgstab", rv, x0=xv, inplace=True, **SOLVE)
    assert got["x"].data_ptr() == xv.data_ptr() and got["r"].data_ptr() == rv.data_ptr()
    assert state(ctx, got) == want
    assert outside_untouched(xbuf, n) and outside_untouched(rbuf, n)
    # the product, input and output misaligned
    want_y = ctx.spmv(x0)
    _, xin = inner_view(x0)
    ybuf, yv = inner_view(np.zeros(n))
    assert ctx.spmv(xin, out=yv).data_ptr() == yv.data_ptr()
    assert host(yv).tobytes() == want_y.tobytes() and outside_untouched(ybuf, n)
    assert host(xin).tobytes() == x0.tobytes()
    # load and fetch: one vector aligned, the other not (the two pairs of the launch take different accesses), then both misaligned
    for lead in ((0, 1), (1, 0), (1, 1)):
        _, x_in = inner_view(x0, lead[0])
        _, b_in = inner_view(b, lead[1])
        ctx.load(x_in, b_in)
        fx, xo = inner_view(np.zeros(n), lead[1])
        fr, ro = inner_view(np.zeros(n), lead[0])
        ctx.fetch(x=xo, r=ro)
        assert host(xo).tobytes() == x0.tobytes() and host(ro).tobytes() == b.tobytes(), lead
        assert outside_untouched(fx, n, lead[1]) and outside_untouched(fr, n, lead[0]), lead


@pytest.mark.parametrize("name", NAMES)
def test_spmv_on_tensors_is_spmv_on_numpy(cases, name):
    A, ctx, x0, b, _ = cases[name]
    tx = dev(b)
    y = ctx.spmv(tx)
    assert y.is_cuda and y.dtype == torch.float64 and y.shape == (A.rows,)
    assert host(y).tobytes() == ctx.spmv(b).tobytes()
    assert host(tx).tobytes() == b.tobytes()
    # a strided input is made contiguous
    wide = torch.zeros((A.rows, 2), dtype=torch.float64, device="cuda")
    wide[:, 0] = tx
    assert host(ctx.spmv(wide[:, 0])).tobytes() == host(y).tobytes()
    with pytest.raises(ValueError):
        ctx.spmv(tx, out=tx)


@pytest.mark.parametrize("name", ("n16001", "mesh_ro"))
def test_load_run_in_steps_fetch(cases, name):
    A, ctx, x0, b, _ = cases[name]

    def steps(load, fetch):
        load()
        ctx.run_begin("pipe_bicgstab", **SOLVE)
        k1 = ctx.run_iterate(3)
        k2 = ctx.run_iterate(300)
        res = ctx.run_end()
        x, r = fetch()
        tr = ctx.trace(k2)
        return (k1, k2, res.iterations, np.float64(res.dot_r).tobytes(), x.tobytes(), r.tobytes(), tuple(tr[key].tobytes() for key in tr))

    want = steps(lambda: ctx.load(x0, b), ctx.fetch)
    tx0, tb = dev(x0), dev(b)
    got = steps(lambda: ctx.load(tx0, tb), lambda: tuple(host(t) for t in ctx.fetch(device=True)))
    assert got == want and want[0] == 3
    # either output omitted
    x, r = ctx.fetch(device=True, r=False)
    assert r is None and host(x).tobytes() == want[4]
    x, r = ctx.fetch(device=True, x=False)
    assert x is None and host(r).tobytes() == want[5]
    hx, hr = ctx.fetch(r=False)
    assert hr is None and hx.tobytes() == want[4]


@pytest.mark.parametrize("name", ("n16001", "mesh_ro"))
def test_warm_start_from_the_solution_the_context_holds(cases, name):
    A, ctx, x0, b, b2 = cases[name]
    first = ctx.solve("bicgstab", b, **SOLVE)
    second = ctx.solve("bicgstab", b2, x0=first["x"], **SOLVE)
    want = (second["result"].iterations, np.float64(second["result"].dot_r).tobytes(), second["x"].tobytes(), second["r"].tobytes())
    assert second["result"].iterations > 0
    got1 = ctx.solve("bicgstab", dev(b), **SOLVE)
    assert host(got1["x"]).tobytes() == first["x"].tobytes()
    ctx.load(None, dev(b2))
    res = ctx.run("bicgstab", **SOLVE)
    x, r = ctx.fetch(device=True)
    assert (res.iterations, np.float64(res.dot_r).tobytes(), host(x).tobytes(), host(r).tobytes()) == want


def multi_state(ctx, got):
    tohost = (lambda t: host(t)) if hasattr(got["x"], "data_ptr") else (lambda a: a)
    x, r = tohost(got["x"]), tohost(got["r"])
    out = []
    for j in range(len(got["k"])):
        q = got["results"][j]
        tr = ctx.multi_trace(j, int(got["k"][j]))
        out.append((int(got["k"][j]), q.iterations, q.breakdown_iteration, np.float64(q.dot_r).tobytes(), np.float64(q.dot_zero).tobytes(),
                    np.ascontiguousarray(x[j]).tobytes(), np.ascontiguousarray(r[j]).tobytes(), tuple(tr[key].tobytes() for key in ("alpha", "omega", "beta", "dotr"))))
    return out


def multi_inputs(A, nrhs=17):
    rng = np.random.default_rng(23)
    B = np.array([A.matvec(1.0 + 0.5 * rng.random(A.rows)) for _ in range(nrhs)])
    B[1] = 0.0                                           # a column that is done at k = 0
    X0 = 0.1 * rng.standard_normal((nrhs, A.rows))
    X0[1] = 0.0
    return B, X0


def padded_set(a, pad):
    """(buffer [nrhs][n + pad] full of SENTINEL but for a, its view [nrhs][n])"""
    nrhs, n = a.shape
    buf = torch.full((nrhs, n + pad), SENTINEL, dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(a)
    torch.cuda.synchronize()
    return buf, buf[:, :n]


@pytest.mark.parametrize("name,pad", [("n259", 3), ("n16001", 3), ("n16001", 2), ("mesh", 3), ("mesh_ro", 3)])
def test_solve_multi_of_17_columns_in_a_padded_buffer(cases, name, pad):
    """two sets, the last with one column; ld = n + pad: 16004 (every column 16-byte aligned) and 16003 (every other one) on n = 16001"""
    A, ctx, *_ = cases[name]
    n = A.rows
    B, X0 = multi_inputs(A)
    want = multi_state(ctx, ctx.solve_multi(B, X0=X0, **SOLVE))
    assert want[1][0] == 0 and max(s[0] for s in want) > 0
    allocs = H.device_allocations()
    xbuf, xv = padded_set(X0, pad)
    rbuf, rv = padded_set(B, pad)
    assert xv.stride(0) == n + pad
    got = ctx.solve_multi(rv, X0=xv, inplace=True, **SOLVE)
    assert got["rc"] == max(s[0] for s in want) and got["x"].data_ptr() == xv.data_ptr()
    assert multi_state(ctx, got) == want
    assert H.device_allocations() == allocs, "a multi call on tensors after a host multi call allocated (or freed) device memory"
    for buf in (xbuf, rbuf):
        assert bool(torch.all(buf[:, n:] == SENTINEL)), "the padding columns were written"
    # fresh tensors by default, the caller's sets stay
    tB, tX0 = dev(B), dev(X0)
    got = ctx.solve_multi(tB, X0=tX0, **SOLVE)
    assert multi_state(ctx, got) == want and got["x"].data_ptr() != tX0.data_ptr()
    assert host(tB).tobytes() == B.tobytes() and host(tX0).tobytes() == X0.tobytes()


def test_a_refused_multi_call_touches_neither_set(cases):
    A, ctx, *_ = cases["n16001"]
    n = A.rows
    B, X0 = multi_inputs(A)
    xbuf, xv = padded_set(X0, 3)
    rbuf, rv = padded_set(B, 3)
    keep = (host(xbuf).tobytes(), host(rbuf).tobytes())
    got = ctx.solve_multi(rv, X0=xv, method="pipe_bicgstab", inplace=True, **SOLVE)
    assert got["rc"] == -2
    o = ctx.options(quiet=1, **SOLVE)
    rc = H.lib().bicg_solve_multi_device(ctx.h, 0, C.c_void_p(xbuf.data_ptr()), C.c_void_p(rbuf.data_ptr()), n - 1, 17, C.byref(o), None, None)
    assert rc == -2, "ld < local_rows"
    assert H.lib().bicg_solve_multi_device(ctx.h, 0, None, C.c_void_p(rbuf.data_ptr()), n, 17, C.byref(o), None, None) == -1
    torch.cuda.synchronize()
    assert (host(xbuf).tobytes(), host(rbuf).tobytes()) == keep


def _delay(stream, ms_wanted=8):
    """several milliseconds of device work on `stream`: a chain of 4096^3 fp32 products (137 GFLOP each, about a millisecond)"""
    with torch.cuda.stream(stream):
        a = torch.ones((4096, 4096), device="cuda")
        for _ in range(ms_wanted):
            a = (a @ a) * 2.0 ** -12
    return a


def test_the_load_waits_for_the_callers_stream(cases):
    """b is written into its tensor on a side stream behind a delay; solve(stream=side) right away, no host wait: a load that did not
    wait for the stream would read the zeros the tensor held"""
    A, ctx, x0, b, _ = cases["n16001"]
    want = state(ctx, ctx.solve("bicgstab", b, **SOLVE))
    side = torch.cuda.Stream()
    _delay(side, 1)                                       # (library set-up of the first product is not part of the delay)
    pinned = torch.from_numpy(np.array(b)).pin_memory()
    tb = torch.zeros(A.rows, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _delay(side)
    with torch.cuda.stream(side):
        tb.copy_(pinned, non_blocking=True)
    got = ctx.solve("bicgstab", tb, stream=side, **SOLVE)
    assert state(ctx, got) == want
    # the in-place form reads the caller's array itself
    tb2, tx = torch.zeros(A.rows, dtype=torch.float64, device="cuda"), torch.zeros(A.rows, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _delay(side)
    with torch.cuda.stream(side):
        tb2.copy_(pinned, non_blocking=True)
    got = ctx.solve("bicgstab", tb2, x0=tx, inplace=True, stream=side, **SOLVE)
    assert state(ctx, got) == want
    torch.cuda.synchronize()


def test_the_callers_stream_waits_for_the_fetch(cases):
    """fetch(device=True, stream=side) behind a delay on side, x.clone() enqueued on side at once, no host wait in between"""
    A, ctx, x0, b, _ = cases["n16001"]
    ctx.solve("bicgstab", b, **SOLVE)
    want_x, want_r = ctx.fetch()
    side = torch.cuda.Stream()
    _delay(side, 1)
    x = torch.full((A.rows,), SENTINEL, dtype=torch.float64, device="cuda")
    r = torch.full((A.rows,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    _delay(side)
    ctx.fetch(x=x, r=r, stream=side)
    with torch.cuda.stream(side):
        xc, rc = x.clone(), r.clone()
    torch.cuda.synchronize()
    assert host(xc).tobytes() == want_x.tobytes() and host(rc).tobytes() == want_r.tobytes()


def test_the_crossing_allocates_nothing():
    """a fresh reordered context (whose host copies would allocate the staging buffer) and a fresh plain one: the allocation count
    is the same after load, fetch, spmv and solve on tensors as before each"""
    H.lib().bicg_comm_init_single(0)
    A = _matrix("n16001")
    b = A.matvec(np.ones(A.rows))
    for sw in (dict(reorder=1), dict()):
        ctx = _context(A, **sw)
        try:
            assert ctx.flags()["reordered"] == bool(sw)
            tb, tx, ty = dev(b), dev(np.zeros(A.rows)), dev(np.zeros(A.rows))
            calls = {"load": lambda: ctx.load(tx, tb), "warm load": lambda: ctx.load(None, tb), "fetch": lambda: ctx.fetch(x=tx, r=ty),
                     "spmv": lambda: ctx.spmv(tb, out=ty)}
            for what, call in calls.items():
                before = H.device_allocations()
                call()
                ctx.sync()
                assert H.device_allocations() == before, (sw, what)
            ctx.solve("bicgstab", b, **SOLVE)                 # (a context's first solve allocates its trace, whoever makes it)
            before = H.device_allocations()
            got = ctx.solve("bicgstab", tb, x0=tx, inplace=True, **SOLVE)
            assert got["k"] > 0 and H.device_allocations() == before, sw
        finally:
            ctx.close()
