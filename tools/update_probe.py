#!/usr/bin/env python3
"""What bicg_update_values buys a caller whose matrix changes values and keeps its pattern, measured in one process on one build,
for the Transport-shaped matrix (synth.transport_like) and the unstructured FEM matrix in "rcm" numbering (mpi_bicgstab_amd.mesh,
m = 117: 1.6 M rows). Per matrix, best of --reps:
  (a) bicg_update_values_device   new values already on the device (a torch tensor)
  (b) bicg_update_values          new values in pageable host memory
  (c) bicg_destroy + bicg_create  on the same blocks: what a caller had to do before
  (d) a device-to-device copy of nnz doubles (hipMemcpy through torch), the floor for (a)
A measuring tool, not a test: nothing is asserted but that the product after (a) and (b) is the product of a fresh context.
    python tools/update_probe.py [--matrix transport|mesh|both] [--n ROWS] [--m 117] [--reps 3] [--out FILE.json]"""
import argparse
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
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()

import torch  # noqa: E402
from mpi_bicgstab_amd import hipsolver as H, mesh, synth  # noqa: E402

H.lib().bicg_comm_init_single(0)


def best(fn, reps):
    times = []
    for _ in range(reps):
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
    rng = np.random.default_rng(21)
    val2 = np.ascontiguousarray(A.val * (0.9 + 0.2 * rng.random(A.nnz)))
    A2 = synth.CSR(A.rows, A.cols, A.ptr, A.col, val2)
    blocks = H.single_rank_blocks(A)
    ctx = H.Context(blocks)
    out = dict(matrix=name, rows=A.rows, nnz=A.nnz, flags=[k for k, v in ctx.flags().items() if v], device_matrix_bytes=ctx.device_matrix_bytes())
    x = 1.0 + 1e-3 * np.cos(np.arange(A.rows))
    fresh = H.Context(H.single_rank_blocks(A2))
    want = fresh.spmv(x)
    fresh.close()
    dev2, dev1 = torch.from_numpy(val2).cuda(), torch.from_numpy(np.ascontiguousarray(A.val)).cuda()
    ctx.update_values(dev2)                                            # code objects loaded, clocks up
    out["update_device_ms"] = round(1e3 * best(lambda: ctx.update_values(dev2), a.reps), 3)
    assert np.array_equal(ctx.spmv(x), want), "product after the device update differs from a fresh context's"
    ctx.update_values(dev1)
    out["update_host_ms"] = round(1e3 * best(lambda: ctx.update_values(val2), a.reps), 3)
    assert np.array_equal(ctx.spmv(x), want), "product after the host update differs from a fresh context's"
    scratch = torch.empty_like(dev2)
    scratch.copy_(dev2)
    out["copy_d2d_ms"] = round(1e3 * best(lambda: scratch.copy_(dev2), max(a.reps, 5)), 3)
    del scratch, dev1, dev2

    def recreate():
        global ctx
        ctx.close()
        ctx = H.Context(blocks)
    out["recreate_ms"] = round(1e3 * best(recreate, a.reps), 3)
    ctx.close()
    results.append(out)
    print(json.dumps(out), flush=True)

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(cases=results), f, indent=1)
