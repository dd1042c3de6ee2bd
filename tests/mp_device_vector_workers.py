"""Worker of tests/test_device_vectors_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1, as tests/mp_multi_workers.py). Every rank makes each call twice, on numpy arrays and on CUDA tensors, and
compares what comes back as bytes and what the call added to bicg_comm_counts. A rank reports through the ok<rank> / fail<rank>
files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SOLVE = dict(tol=1e-10, max_iter=300, record_trace=1, check_every=4)


def matrix(name):
    import mp_multi_workers as M
    from mpi_bicgstab_amd import synth
    return synth.transport_like(40000) if name == "transport" else M.matrix(name)


def device_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import torch
        import mp_multi_workers as M
        dist = M._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        A = matrix(kind)
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        lo, nl = int(displs[rank]), int(counts[rank])
        if kind == "six":
            assert (nl == 0) == (rank >= 6)                 # the seventh rank has no rows: it passes no arrays
        ctx = H.Context(H.HostBlocks(diag, offd, A.rows, counts, displs))
        if kind == "transport":
            assert ctx.plan_info()["halo"] > 0
        rng = np.random.default_rng(3)
        x = rng.standard_normal(A.rows)[lo:lo + nl]
        B = np.array([A.matvec(1.0 + 0.5 * rng.random(A.rows)) for _ in range(5)])[:, lo:lo + nl]
        X0 = 0.1 * rng.standard_normal((5, A.rows))[:, lo:lo + nl]
        dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).cuda()
        host = lambda t: t.cpu().numpy() if hasattr(t, "data_ptr") else t

        def counted(call):
            c0 = ctx.comm_counts()
            out = call()
            c1 = ctx.comm_counts()
            return out, {k: c1[k] - c0[k] for k in c1}

        def solve_state(got):
            tr = ctx.trace(got["k"])
            q = got["result"]
            return (got["k"], q.iterations, q.breakdown_iteration, np.float64(q.dot_r).tobytes(), np.float64(q.dot_zero).tobytes(),
                    host(got["x"]).tobytes(), host(got["r"]).tobytes(), tuple(tr[k].tobytes() for k in ("alpha", "omega", "beta", "dotr")))

        def multi_state(got):
            xs, rs = host(got["x"]), host(got["r"])
            assert got["rc"] >= 0 and xs.shape == (5, nl)
            return [(int(got["k"][j]), got["results"][j].iterations, np.float64(got["results"][j].dot_r).tobytes(),
                     np.ascontiguousarray(xs[j]).tobytes(), np.ascontiguousarray(rs[j]).tobytes(),
                     tuple(v.tobytes() for v in ctx.multi_trace(j, int(got["k"][j])).values())) for j in range(5)]

        # ---- the collective product
        y_h, d_h = counted(lambda: ctx.spmv(x))
        y_d, d_d = counted(lambda: ctx.spmv(dev(x)))
        assert y_d.is_cuda and y_d.shape == (nl,)
        assert host(y_d).tobytes() == y_h.tobytes(), "spmv on tensors"
        assert d_d == d_h and (d_h["exchanges"] == 1 or kind == "six"), (d_h, d_d)
        # ---- two solvers
        for method in ("bicgstab", "pipe_bicgstab"):
            want, d_h = counted(lambda: solve_state(ctx.solve(method, B[0], x0=X0[0], **SOLVE)))
            got, d_d = counted(lambda: solve_state(ctx.solve(method, dev(B[0]), x0=dev(X0[0]), **SOLVE)))
            assert got == want, method
            assert d_d == d_h and d_h["allreduces"] > 0, (method, d_h, d_d)
        # ---- load / run / fetch with a warm start
        ctx.load(dev(X0[1]), dev(B[1]))
        ctx.run("bicgstab", **SOLVE)
        ctx.load(None, dev(B[2]))
        res = ctx.run("bicgstab", **SOLVE)
        xw, rw = ctx.fetch(device=True)
        first = ctx.solve("bicgstab", B[1], x0=X0[1], **SOLVE)
        second = ctx.solve("bicgstab", B[2], x0=first["x"], **SOLVE)
        assert (res.iterations, host(xw).tobytes(), host(rw).tobytes()) == (second["result"].iterations, second["x"].tobytes(), second["r"].tobytes())
        # ---- five columns
        want, d_h = counted(lambda: multi_state(ctx.solve_multi(B, X0=X0, nrhs=5, **SOLVE)))
        got, d_d = counted(lambda: multi_state(ctx.solve_multi(dev(B), X0=dev(X0), nrhs=5, **SOLVE)))
        assert got == want, "solve_multi on tensors"
        assert d_d == d_h and d_h["allreduces"] > 0, (d_h, d_d)
        torch.cuda.synchronize()
        assert not ctx.comm_failed()
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
