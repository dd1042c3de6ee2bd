#!/usr/bin/env python3
"""What the block-Jacobi preconditioner (BICG_BICGSTAB_BLOCK) costs on one MI355X, measured on one context
per matrix in one process, for the Transport-shaped matrix (synth.transport_like) and the unstructured FEM matrix in "rcm" numbering
(mpi_bicgstab_amd.mesh, m = 117), both at 1.6 M rows:

  (a) k_bjac_apply back to back (bicg_precond_apply_bench) at bs = 4 and 8, against its byte model -- (bs + 2) * 8 bytes per row:
      bs plane entries, the input once, the output once -- priced at the copy rate bicg_stream_bench measures on the same GPU;
  (b) ms per iteration on the device clock (bicg_run_iterate_timed) of method 5 with identity blocks (bs = 4) against method 4 with
      d = 1 and against method 0. Methods 4 and 5 are then the plain multi-launch iteration bit for bit (tests/test_precond_gpu.py,
      tests/test_block_precond_gpu.py), so all walk through the same unconverged iterates -- tol = 0 on a badly scaled system -- and
      every kernel of every timed iteration does its full work. Per method: --warmup iterations, then the best of --reps regions of
      --steps iterations.
A measuring tool, not a test: no threshold; it asserts only that every timed region ran its --steps iterations and that methods 4 and
5 end on the same bytes.
    python tools/block_precond_probe.py [--matrix transport|mesh|both] [--n ROWS] [--m 117] [--steps 100] [--warmup 20] [--reps 5] [--out FILE.json]"""
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
copy_gbps = H.stream_bench("copy")
print(json.dumps(dict(stream_copy_gbps=round(copy_gbps, 1))), flush=True)


def identity_blocks(n, bs):
    out = np.zeros((-(-n // bs), bs, bs))
    out[:, np.arange(bs), np.arange(bs)] = 1.0
    return out


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
               stream_copy_gbps=round(copy_gbps, 1))
    # ---- (a) the operator back to back
    for bs in (4, 8):
        assert ctx.set_block_diagonal(identity_blocks(n, bs), bs) == 0
        ms = min(ctx.apply_preconditioner_bench(200) for _ in range(a.reps))
        model_bytes = (bs + 2) * 8 * n
        model_ms = model_bytes / (copy_gbps * 1e9) * 1e3
        out[f"apply_bs{bs}"] = dict(ms=round(ms, 5), model_bytes=model_bytes, model_ms=round(model_ms, 5), ratio=round(ms / model_ms, 3),
                                    gbps=round(model_bytes / ms / 1e6, 1))
    # ---- (b) the iteration
    b = ctx.spmv(np.ones(n))
    total = a.warmup + a.steps * a.reps
    final = {}
    for method in ("bicgstab", "bicgstab_diag", "bicgstab_block"):
        if method == "bicgstab_diag":
            assert ctx.set_diagonal(np.ones(n)) == 0
        if method == "bicgstab_block":
            assert ctx.set_block_diagonal(identity_blocks(n, 4), 4) == 0
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
    assert final["bicgstab_diag"] == final["bicgstab_block"], "identity blocks did not reproduce method 4 with d = 1"
    out["plain_same_bytes"] = final["bicgstab"] == final["bicgstab_block"]
    out["block_over_diag"] = round(out["bicgstab_block_ms_per_iteration"] / out["bicgstab_diag_ms_per_iteration"], 4)
    out["block_over_plain"] = round(out["bicgstab_block_ms_per_iteration"] / out["bicgstab_ms_per_iteration"], 4)
    out["two_applies_us"] = round(2e3 * out["apply_bs4"]["ms"], 2)
    ctx.close()
    results.append(out)
    print(json.dumps(out), flush=True)

if a.out:
    with open(a.out, "w") as f:
        json.dump(dict(stream_copy_gbps=copy_gbps, cases=results), f, indent=1)
