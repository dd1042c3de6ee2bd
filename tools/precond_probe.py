#!/usr/bin/env python3
"""What an iteration of the diagonally preconditioned BiCGStab (BICG_BICGSTAB_DIAG) costs beside an
iteration of the plain one, measured on the same context in one process: ms per iteration on the device clock
(bicg_run_iterate_timed) for the Transport-shaped matrix (synth.transport_like) and the unstructured FEM matrix in "rcm" numbering
(mpi_bicgstab_amd.mesh, m = 117), both at 1.6 M rows.

The preconditioned iteration moves 40 bytes per row more than the plain one (two reads of 1/d, two stores of hat vectors, one more
read in the x / r kernel). To time exactly that and nothing else the installed diagonal is d = 1: the iteration is then the plain
one bit for bit (tests/test_precond_gpu.py), so both methods walk through the same unconverged iterates -- tol = 0 on a badly scaled
system (scale_decades) -- and every kernel of every timed iteration does its full work. Per method: --warmup iterations, then the
best of --reps regions of --steps iterations. A measuring tool, not a test: no threshold; it asserts only that every timed region
ran its --steps iterations and that the two methods end on the same bytes.
    python tools/precond_probe.py [--matrix transport|mesh|both] [--n ROWS] [--m 117] [--steps 100] [--warmup 20] [--reps 5] [--out FILE.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--matrix", default="both", choices=("transport", "mesh", "both"))
ap.add_argument("--n", type=int, default=None, help="rows of the Transport-shaped matrix (default: Transport's)")
ap.add_argument("--m", type=int, default=117)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()

from mpi_bicgstab_amd import hipsolver as H, mesh, synth  # noqa: E402

H.lib().bicg_comm_init_single(0)
results = []
for name in (("transport", "mesh") if a.matrix == "both" else (a.matrix,)):
    if name == "transport":
        A = synth.transport_like(a.n, scale_decades=4.0) if a.n else synth.transport_like(scale_decades=4.0)
    else:
        cache = os.path.join(tempfile.gettempdir(), "bicg_mesh_cache")
        os.makedirs(cache, exist_ok=True)
        A = mesh.fem_unstructured(a.m, "rcm", scale_decades=2.0, cache_dir=cache)
    ctx = H.Context(H.single_rank_blocks(A))
    n = A.rows
    fl = ctx.flags()
    out = dict(matrix=name, rows=n, nnz=A.nnz, steps=a.steps, reps=a.reps, handover=fl["handover"], jagged=fl["jagged"],
               extra_bytes_per_iteration=40 * n)
    b = ctx.spmv(np.ones(n))
    assert ctx.set_diagonal(np.ones(n)) == 0
    total = a.warmup + a.steps * a.reps
    final = {}
    for method in ("bicgstab", "bicgstab_diag"):
        ctx.load(np.zeros(n), b)
        ctx.run_begin(method, tol=0.0, max_iter=total, check_every=a.steps)
        k = ctx.run_iterate(a.warmup)
        per_it = []
        for _ in range(a.reps):
            k1, ms = ctx.run_iterate_timed(a.steps)
            assert k1 - k == a.steps, f"{name} {method}: a timed region ran {k1 - k} of {a.steps} iterations (converged or broke down)"
            k = k1
            per_it.append(ms["device_ms"] / a.steps)
        res = ctx.run_end()
        final[method] = (res.iterations, ctx.fetch()[0].tobytes())
        out[f"{method}_ms_per_iteration"] = round(min(per_it), 5)
        out[f"{method}_ms_per_iteration_all"] = [round(v, 5) for v in per_it]
    assert final["bicgstab"] == final["bicgstab_diag"], "d = 1 did not reproduce the plain iteration"
    out["ratio"] = round(out["bicgstab_diag_ms_per_iteration"] / out["bicgstab_ms_per_iteration"], 4)
    ctx.close()
    results.append(out)
    print(json.dumps(out), flush=True)

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(cases=results), f, indent=1)
