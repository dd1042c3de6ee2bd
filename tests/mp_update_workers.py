"""Worker of tests/test_update_values_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1, as tests/mp_multi_workers.py), every rank updates the values of its own blocks and compares, as bytes, with
a fresh context on the new values. A rank reports through the ok<rank> / fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SOLVE = dict(tol=1e-10, max_iter=300, record_trace=1)


def matrix(name):
    import mp_multi_workers as M
    from mpi_bicgstab_amd import synth
    return synth.transport_like(40000) if name == "transport" else M.matrix(name)


def update_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import mp_multi_workers as M
        dist = M._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T
        from test_update_values import revalued

        case, name = kind.split(":")
        T.init_host_transport(0)
        if case == "p2p":
            rc = H.lib().bicg_comm_enable_p2p()
            assert rc == 0, f"bicg_comm_enable_p2p() returned {rc}: ranks sharing one device reach each other's memory"
        A = matrix(name)
        A2 = revalued(A, 21)
        x = np.random.default_rng(3).standard_normal(A.rows)
        b = A2.matvec(np.ones(A.rows))

        def blocks(M_):
            diag, offd, counts, displs = synth.split_blocks(M_, world, rank)
            return H.HostBlocks(diag, offd, M_.rows, counts, displs), int(displs[rank]), int(counts[rank])

        def state(ctx, lo, nl):
            out = [ctx.spmv(x[lo:lo + nl]).tobytes()]
            for method in ("bicgstab", "pipe_bicgstab"):
                got = ctx.solve(method, b[lo:lo + nl], **SOLVE)
                tr = ctx.trace(got["k"])
                out.append((got["k"], got["x"].tobytes(), got["r"].tobytes(), tuple(tr[k].tobytes() for k in ("alpha", "omega", "beta", "dotr"))))
            return out

        blk2, lo, nl = blocks(A2)
        fresh = H.Context(blk2)
        persist = fresh.flags()["persist"]
        if case == "p2p":
            assert persist and fresh.flags()["p2p"], fresh.flags()      # the ranks are small enough for the persistent plan
        facts = (fresh.flags(), fresh.plan_info(), fresh.device_matrix_bytes())
        want = state(fresh, lo, nl)
        fresh.close()

        blk, _, _ = blocks(A)
        ctx = H.Context(blk)
        assert (ctx.flags(), ctx.plan_info(), ctx.device_matrix_bytes()) == facts
        if name == "six":
            assert (nl == 0) == (rank >= 6)                             # a rank without rows calls with empty arrays
        assert state(ctx, lo, nl) != want or nl == 0                    # (A and A2 differ: the comparison below means something)
        before, allocs = ctx.comm_counts(), H.device_allocations()
        assert ctx.update_values(blk2) == 0
        assert ctx.comm_counts() == before, "bicg_update_values is local: no transport call"
        assert H.device_allocations() == allocs
        assert (ctx.flags(), ctx.plan_info(), ctx.device_matrix_bytes()) == facts
        got = state(ctx, lo, nl)
        assert got[0] == want[0], "collective spmv after the update"
        assert got[1] == want[1], "bicgstab after the update"
        assert got[2] == want[2], "pipe_bicgstab after the update"
        assert not ctx.comm_failed()
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
