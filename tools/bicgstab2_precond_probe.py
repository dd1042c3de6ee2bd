#!/usr/bin/env python3
"""What a sweep of the right-preconditioned BiCGStab(2) (BICG_BICGSTAB2_DIAG / _BLOCK) costs beside a sweep of
BiCGStab(2) itself, measured on ONE context per matrix in one process: ms on the device clock (bicg_run_iterate_timed), best of --reps
regions of --steps steps, for the Transport-shaped matrix (synth.transport_like) and the unstructured FEM matrix in "rcm" numbering
(mpi_bicgstab_amd.mesh, m = 117), both at 1.6 M rows.

Method 7 runs with d = 1 and method 8 with identity blocks of 4, so all three methods do the same arithmetic on the same numbers
(they are bit-identical) and differ only in what they move: beside the four products a sweep of method 6 moves 288 bytes per row,
one of method 7 416 (the four hat streams and the plane of 1 / d), one of method 8 384 in its passes and the applications' outputs
plus, per application, the input and the bs planes (8 + 8 bs bytes per row): 544 at bs = 4, in four more launches. The model's
ratios are (4 P + 416 n) / (4 P + 288 n) and (4 P + 544 n) / (4 P + 288 n) with P the bytes of a product; the spread of method 6's
regions is the margin. Method 6's code is the same before and after these methods were added, so it is its own yardstick.
A measuring tool, not a test: no threshold; it asserts only that every timed region ran its steps.
    python tools/bicgstab2_precond_probe.py [--matrix transport|mesh|both] [--n ROWS] [--m 117] [--steps 100] [--warmup 20] [--reps 5]
                                            [--out FILE.json]"""
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
if a.steps < 2 or a.steps % 2 or a.warmup % 2:
    ap.error("--steps and --warmup must be even (a sweep is two steps), --steps at least 2")

from mpi_bicgstab_amd import hipsolver as H, mesh, synth  # noqa: E402

H.lib().bicg_comm_init_single(0)
BS = 4


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
for name in (("transport", "mesh") if a.matrix == "both" else (a.matrix,)):
    if name == "transport":
        A = synth.transport_like(a.n, scale_decades=4.0) if a.n else synth.transport_like(scale_decades=4.0)
    else:
        cache = os.path.join(tempfile.gettempdir(), "bicg_mesh_cache")
        os.makedirs(cache, exist_ok=True)
        A = mesh.fem_unstructured(a.m, "rcm", scale_decades=2.0, cache_dir=cache)
    n = A.rows
    out = dict(matrix=name, rows=n, nnz=A.nnz, steps=a.steps, reps=a.reps, bs=BS)
    H.switches(persist=0)
    try:
        ctx = H.Context(H.single_rank_blocks(A))
    finally:
        H.switches(persist=None)
    b = ctx.spmv(np.ones(n))
    P = ctx.spmv_matrix_bytes() + 16 * n      # a product: the matrix stream, x read and y written once
    base = 4 * P + 288 * n
    out["model_ratio_diag"] = round((4 * P + 416 * n) / base, 4)
    out["model_ratio_block"] = round((4 * P + (384 + 4 * (8 + 8 * BS)) * n) / base, 4)
    best, every = regions(ctx, "bicgstab2", b, n)
    out["bicgstab2_ms_per_sweep"], out["bicgstab2_ms_per_sweep_all"] = round(2 * best, 5), [round(2 * v, 5) for v in every]
    out["bicgstab2_spread"] = round(max(every) / min(every) - 1.0, 4)
    assert ctx.set_diagonal(np.ones(n)) == 0
    best, every = regions(ctx, "bicgstab2_diag", b, n)
    out["diag_ms_per_sweep"], out["diag_ms_per_sweep_all"] = round(2 * best, 5), [round(2 * v, 5) for v in every]
    eye = np.zeros((-(-n // BS), BS, BS))
    eye[:, np.arange(BS), np.arange(BS)] = 1.0
    assert ctx.set_block_diagonal(eye, BS) == 0
    best, every = regions(ctx, "bicgstab2_block", b, n)
    out["block_ms_per_sweep"], out["block_ms_per_sweep_all"] = round(2 * best, 5), [round(2 * v, 5) for v in every]
    best, every = regions(ctx, "bicgstab2", b, n)      # method 6 once more, behind the others: drift of the machine, if any
    out["bicgstab2_again_ms_per_sweep"] = round(2 * best, 5)
    ctx.close()
    out["ratio_diag"] = round(out["diag_ms_per_sweep"] / out["bicgstab2_ms_per_sweep"], 4)
    out["ratio_block"] = round(out["block_ms_per_sweep"] / out["bicgstab2_ms_per_sweep"], 4)
    results.append(out)
    print(json.dumps(out), flush=True)

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(cases=results), f, indent=1)
