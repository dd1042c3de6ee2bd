#!/usr/bin/env python3
"""What the device-resident vector calls (bicg_load_device / bicg_fetch_device / bicg_solve_device) buy a
caller whose right-hand side and solution live in device memory, measured in one process on one build, for the Transport-shaped
matrix (synth.transport_like) and the unstructured FEM matrix in "rcm" numbering (mpi_bicgstab_amd.mesh, m = 117: 1.6 M rows).
Per matrix, best of --reps, wall clock around the raw library calls on arrays allocated beforehand, the device idle before and
synchronised after:
  load + fetch      bicg_load + bicg_fetch on pageable host arrays      against  bicg_load_device + bicg_fetch_device on tensors
  solve, K = 10/50  bicg_solve (plain BiCGStab, tol = 0, max_iter = K, check_every = K)  against  bicg_solve_device
The host calls are the code every caller had before: a caller with device data additionally pays its own device-to-host and
host-to-device copies around them, which are not counted here. A measuring tool, not a test: no threshold; the only assertion is
that both forms return the same bytes.
    python tools/device_vectors_probe.py [--matrix transport|mesh|both] [--n ROWS] [--m 117] [--reps 5] [--reorder 0|1] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--matrix", default="both", choices=("transport", "mesh", "both"))
ap.add_argument("--n", type=int, default=None, help="rows of the Transport-shaped matrix (default: Transport's)")
ap.add_argument("--m", type=int, default=117)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--reorder", type=int, default=0, help="create the contexts under BICG_PLAN=reorder=N (the crossing then gathers)")
ap.add_argument("--out", default=None)
a = ap.parse_args()

import torch  # noqa: E402
from mpi_bicgstab_amd import hipsolver as H, mesh, synth  # noqa: E402

L = H.lib()
L.bicg_comm_init_single(0)
_dp = C.POINTER(C.c_double)


def best(fn, reps, before=None):
    times = []
    for _ in range(reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return min(times)


results = []
for name in (("transport", "mesh") if a.matrix == "both" else (a.matrix,)):
    if name == "transport":
        A = synth.transport_like(a.n) if a.n else synth.transport_like()
    else:
        cache = os.path.join(tempfile.gettempdir(), "bicg_mesh_cache")
        os.makedirs(cache, exist_ok=True)
        A = mesh.fem_unstructured(a.m, "rcm", scale_decades=2.0, cache_dir=cache)
    if a.reorder:
        H.switches(reorder=a.reorder)
    ctx = H.Context(H.single_rank_blocks(A))
    H.switches(reorder=None)
    n = A.rows
    out = dict(matrix=name, rows=n, nnz=A.nnz, reordered=ctx.flags()["reordered"], vector_bytes=8 * n)
    b = ctx.spmv(np.ones(n))
    x0 = np.zeros(n)
    hx, hr = np.zeros(n), np.zeros(n)
    tb, tx0 = torch.from_numpy(b).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda")
    tx, tr = torch.empty_like(tb), torch.empty_like(tb)
    p = lambda arr: arr.ctypes.data_as(_dp)
    d = lambda t: C.c_void_p(t.data_ptr())

    # ---- load + fetch alone
    host_lf = lambda: (L.bicg_load(ctx.h, p(x0), p(b)), L.bicg_fetch(ctx.h, p(hx), p(hr)))
    dev_lf = lambda: (L.bicg_load_device(ctx.h, d(tx0), d(tb), None), L.bicg_fetch_device(ctx.h, d(tx), d(tr), None))
    host_lf(); dev_lf()                                             # code objects loaded, staging made, clocks up
    out["load_fetch_host_ms"] = round(1e3 * best(host_lf, a.reps), 3)
    out["load_fetch_device_ms"] = round(1e3 * best(dev_lf, a.reps), 3)
    torch.cuda.synchronize()
    assert np.array_equal(hr, b) and np.array_equal(tr.cpu().numpy(), b) and np.array_equal(tx.cpu().numpy(), x0)

    # ---- a whole solve at a fixed iteration count
    for K in (10, 50):
        o = ctx.options(quiet=1, tol=0.0, max_iter=K, check_every=K)
        res = H.Result()

        def host_reset():
            hx[:] = 0.0
            np.copyto(hr, b)

        def dev_reset():
            tx.zero_()
            tr.copy_(tb)

        host_solve = lambda: L.bicg_solve(ctx.h, 0, p(hx), p(hr), C.byref(o), C.byref(res))
        dev_solve = lambda: L.bicg_solve_device(ctx.h, 0, d(tx), d(tr), C.byref(o), C.byref(res), None)
        host_reset(); host_solve(); dev_reset(); dev_solve()
        out[f"solve{K}_host_ms"] = round(1e3 * best(host_solve, a.reps, host_reset), 3)
        out[f"solve{K}_device_ms"] = round(1e3 * best(dev_solve, a.reps, dev_reset), 3)
        torch.cuda.synchronize()
        assert res.iterations == K
        assert tx.cpu().numpy().tobytes() == hx.tobytes() and tr.cpu().numpy().tobytes() == hr.tobytes(), "the two forms differ"
    ctx.close()
    results.append(out)
    print(json.dumps(out), flush=True)

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(cases=results), f, indent=1)
