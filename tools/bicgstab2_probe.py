#!/usr/bin/env python3
"""What a sweep of BiCGStab(2) (BICG_BICGSTAB2) costs beside two iterations of plain BiCGStab, measured on
one context per matrix in one process: ms on the device clock (bicg_run_iterate_timed), best of --reps regions of --steps steps, for
the Transport-shaped matrix (synth.transport_like) and the unstructured FEM matrix in "rcm" numbering (mpi_bicgstab_amd.mesh,
m = 117), both at 1.6 M rows.

A sweep is two BiCG steps -- four products and six element-wise passes, 288 bytes per row beside the products -- so its yardstick is
TWO iterations of method 0 in the multi-launch form (BICG_PLAN=handover=0, BICG_PERSIST=0: the parent's kernels, 2 x (two products
+ 112 bytes per row)) on a context of the same matrix; method 0 in its default form is timed too. The model's ratio is
(4 P + 288 n) / (4 P + 224 n) with P the bytes of a product; the spread of the plain regions is the margin.
--solve adds the time to tol 1e-10 of both methods on the (m, c) = (16, 5) convection stencil of the issue's table scaled up to
--solve-m (117: 1.6 M rows), with their k.
A measuring tool, not a test: no threshold; it asserts only that every timed region ran its steps.
    python tools/bicgstab2_probe.py [--matrix transport|mesh|both|none] [--n ROWS] [--m 117] [--steps 100] [--warmup 20] [--reps 5]
                                    [--solve] [--solve-m 117] [--out FILE.json]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--matrix", default="both", choices=("transport", "mesh", "both", "none"))
ap.add_argument("--n", type=int, default=None, help="rows of the Transport-shaped matrix (default: Transport's)")
ap.add_argument("--m", type=int, default=117)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--solve", action="store_true")
ap.add_argument("--solve-m", type=int, default=117)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if a.steps < 2 or a.steps % 2 or a.warmup % 2:
    ap.error("--steps and --warmup must be even (a sweep of BiCGStab(2) is two steps), --steps at least 2")

from mpi_bicgstab_amd import hipsolver as H, mesh, synth  # noqa: E402

H.lib().bicg_comm_init_single(0)


def context(A, **sw):
    H.switches(**sw)
    try:
        return H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(**{k: None for k in sw})


def regions(ctx, method, b, n):
    """ms per step of `method`: the best region and all of them"""
    total = a.warmup + a.steps * a.reps
    ctx.load(np.zeros(n), b)
    ctx.run_begin(method, tol=0.0, max_iter=total + 2, check_every=a.steps)
    k = ctx.run_iterate(a.warmup)
    per_step = []
    for _ in range(a.reps):
        k1, ms = ctx.run_iterate_timed(a.steps)
        assert k1 - k == a.steps, f"{method}: a timed region ran {k1 - k} of {a.steps} steps (converged or broke down)"
        k = k1
        per_step.append(ms["device_ms"] / a.steps)
    ctx.run_end()
    return min(per_step), [round(v, 5) for v in per_step]


results = []
for name in (("transport", "mesh") if a.matrix == "both" else () if a.matrix == "none" else (a.matrix,)):
    if name == "transport":
        A = synth.transport_like(a.n, scale_decades=4.0) if a.n else synth.transport_like(scale_decades=4.0)
    else:
        cache = os.path.join(tempfile.gettempdir(), "bicg_mesh_cache")
        os.makedirs(cache, exist_ok=True)
        A = mesh.fem_unstructured(a.m, "rcm", scale_decades=2.0, cache_dir=cache)
    n = A.rows
    out = dict(matrix=name, rows=n, nnz=A.nnz, steps=a.steps, reps=a.reps)
    multi = context(A, persist=0, handover=0)      # the multi-launch form: method 6 always, method 0 as the yardstick
    b = multi.spmv(np.ones(n))
    P = multi.spmv_matrix_bytes() + 16 * n      # a product: the matrix stream, x read and y written once
    out["model_ratio"] = round((4 * P + 288 * n) / (4 * P + 224 * n), 4)
    best, every = regions(multi, "bicgstab2", b, n)
    out["bicgstab2_ms_per_sweep"], out["bicgstab2_ms_per_sweep_all"] = round(2 * best, 5), [round(2 * v, 5) for v in every]
    best, every = regions(multi, "bicgstab", b, n)
    out["plain_multi_launch_ms_per_two_iterations"] = round(2 * best, 5)
    out["plain_multi_launch_ms_per_two_iterations_all"] = [round(2 * v, 5) for v in every]
    out["plain_multi_launch_spread"] = round(max(every) / min(every) - 1.0, 4)
    multi.close()
    dflt = context(A)
    fl = dflt.flags()
    out["plain_default_form"] = "persistent" if fl["persist"] else "hand-over" if fl["handover"] else "multi-launch"
    best, every = regions(dflt, "bicgstab", b, n)
    out["plain_default_ms_per_two_iterations"] = round(2 * best, 5)
    dflt.close()
    out["ratio"] = round(out["bicgstab2_ms_per_sweep"] / out["plain_multi_launch_ms_per_two_iterations"], 4)
    results.append(out)
    print(json.dumps(out), flush=True)

if a.solve:
    c = 5.0
    A = synth.stencil7(a.solve_m, (6.05, -1 - c, -1 + c, -1 - c, -1 + c, -1 - c, -1 + c))
    n = A.rows
    b = A.matvec(1.0 + 0.5 * synth._uniform(np.arange(n, dtype=np.int64), 78))
    ctx = context(A, persist=0)
    out = dict(matrix=f"convection stencil m={a.solve_m} c=5", rows=n, nnz=A.nnz, tol=1e-10)
    for method in ("bicgstab2", "bicgstab"):
        ctx.solve(method, b, tol=0.0, max_iter=4)      # (kernels loaded)
        got = ctx.solve(method, b, tol=1e-10, max_iter=4000, check_every=20)
        res = got["result"]
        out[method] = dict(k=got["k"], breakdown=res.breakdown_iteration, iter_seconds=round(res.iter_seconds, 5),
                           relres=float(np.sqrt(res.dot_r / res.dot_zero)),
                           true_relres=float(np.linalg.norm(b - A.matvec(got["x"])) / np.linalg.norm(b)))
    ctx.close()
    results.append(out)
    print(json.dumps(out), flush=True)

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(cases=results), f, indent=1)
