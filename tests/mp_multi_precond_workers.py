"""Worker of tests/test_multi_precond_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1), as in mp_multi_workers.py, and call bicg_solve_multi collectively with the right-preconditioned methods 4
and 5. Every rank builds the same global inputs (deterministic generators) and takes its rows; a rank reports through the ok<rank> /
fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OPTS = dict(tol=1e-10, max_iter=40, record_trace=1)


def matrix(name):
    import mp_multi_workers as W
    from mpi_bicgstab_amd import synth
    return synth.transport_like(40000) if name == "transport40000" else W.matrix(name)


def inputs(A, nrhs):
    """(B, X0, d), global: b_j = A x*_j with x*_0 = 1, x*_1 = 0 and random ones; x0_j without a zero but x0_1 = 0; d powers of two"""
    import numpy as np
    from mpi_bicgstab_amd import synth
    n = A.rows
    idx = np.arange(n, dtype=np.int64)
    xs = np.array([np.ones(n) if j == 0 else np.zeros(n) if j == 1 else 0.5 + synth._uniform(idx, 70 + j) for j in range(nrhs)])
    B = np.array([A.matvec(x) for x in xs])
    X0 = np.array([np.zeros(n) if j == 1 else 0.25 * synth._uniform(idx, 90 + j) - 0.125 for j in range(nrhs)])
    e = np.floor(17.0 * synth._uniform(idx, 31)).astype(np.int64) - 8
    return B, X0, np.ldexp(1.0, e)


def precond_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import mp_multi_workers as W
        dist = W._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        case, name = kind.split(":")
        T.init_host_transport(0)
        A = matrix(name)
        nrhs = 3 if name == "six" else 5
        Bg, X0g, dg = inputs(A, nrhs)
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        lo, nl = int(displs[rank]), int(counts[rank])
        if name == "six":
            assert world == 7 and (nl == 0) == (rank == 6)      # the seventh rank has no rows
        H.switches(persist=0)
        ctx = H.Context(H.HostBlocks(diag, offd, A.rows, counts, displs))
        B, X0, d = (np.ascontiguousarray(a[:, lo:lo + nl]) for a in (Bg, X0g, dg[None, :]))
        d = d[0]
        bs = 4 if rank % 2 == 0 else 3                           # the blocks are a rank's own: they need not agree between ranks
        blocks = H.csr_block_diagonal(H.HostBlocks(diag, offd, A.rows, counts, displs), bs)[0] if nl else None

        def put_diagonal(c, dd):
            assert c.set_diagonal(dd if nl else None) == 0 and c.preconditioner() == "diagonal"

        def put_blocks(c):
            assert c.set_block_diagonal(blocks, bs) == 0 and c.preconditioner() == "block_diagonal"

        def solve(c, b, x0, method, **kw):
            return c.solve_multi(b, X0=x0, nrhs=len(b), method=method, **dict(OPTS, **kw))

        if case == "props":
            # ---- E. every rank holds the same scalars; D. a column is its own one-column collective call, whatever check_every is
            for method, put in (("bicgstab_diag", lambda: put_diagonal(ctx, d)), ("bicgstab_block", lambda: put_blocks(ctx))):
                put()
                got = solve(ctx, B, X0, method)
                assert got["rc"] >= 1 and got["rc"] == max(got["k"]) and got["k"][1] == 0, (method, got["rc"], got["k"])
                state = W.whole_state(ctx, got)
                print(name, method, "rank", rank, "k", [s[0] for s in state], flush=True)
                W.same_on_every_rank(dist, world, W.scalar_state(state), method)
                for j in sorted({0, 1, nrhs - 1}):
                    one = solve(ctx, B[j:j + 1], X0[j:j + 1], method)
                    assert W.column_state(ctx, one, 0) == state[j], (method, j)
                assert W.whole_state(ctx, solve(ctx, B, X0, method, check_every=7)) == state, (method, "check_every")
            # ---- B. powers of two: method 4 on A is the plain call on A D^-1 at the same partition
            As = synth.CSR(A.rows, A.cols, A.ptr, A.col, A.val * (1.0 / dg)[A.col])
            sd, so, _, _ = synth.split_blocks(As, world, rank)
            other = H.Context(H.HostBlocks(sd, so, A.rows, counts, displs))
            assert other.flags() == ctx.flags() and other.plan_info() == ctx.plan_info()
            put_diagonal(ctx, d)
            got = solve(ctx, B, X0, "bicgstab_diag")
            sa = W.whole_state(ctx, got)
            want = solve(other, B, d * X0, "bicgstab")
            sb = W.whole_state(other, want)
            drop_x = lambda st: [s[:5] + s[6:] for s in st]
            assert max(s[0] for s in sa) >= 1
            assert drop_x(sa) == drop_x(sb), "method 4 with powers of two is not the plain call on the scaled columns"
            assert got["x"].tobytes() == (want["x"] / d).tobytes()
            other.close()
        elif case == "cleared":
            # ---- one rank without its preconditioner: -2 there, -1 elsewhere, nothing touched anywhere
            for method, put in (("bicgstab_diag", lambda: put_diagonal(ctx, d)), ("bicgstab_block", lambda: put_blocks(ctx))):
                put()
                want = W.whole_state(ctx, solve(ctx, B, X0, method))      # (everything a multi call allocates is allocated now)
                if rank == 1:
                    assert ctx.clear_preconditioner() == 0
                held = H.device_allocations()
                got = solve(ctx, B, X0, method)
                assert got["rc"] == (-2 if rank == 1 else -1), (method, rank, got["rc"])
                assert got["x"].tobytes() == X0.tobytes() and got["r"].tobytes() == B.tobytes(), method
                assert H.device_allocations() == held
                put()                                                    # ... and the communicator is still in step
                assert W.whole_state(ctx, solve(ctx, B, X0, method)) == want, method
        else:
            raise ValueError(kind)
        H.switches(persist=None)
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
