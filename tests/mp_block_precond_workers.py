"""Worker of tests/test_block_precond_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1, as tests/mp_multi_workers.py). Every rank holds one context on its part of A and compares as bytes:
  refusal        method 5 without a block preconditioner (none at all, then a diagonal one): -2, nothing touched, nothing moved;
  blocks = d     blocks of bs = 4 with d = powers of two on their diagonals and zeros elsewhere: method 5 against method 4 with that
                 d -- k, x, r, the result fields, the traces; the blocks are local to the rank and partial at its last rows;
  counts         method 5 moves bicg_comm_counts by what method 4 moves it, the install by nothing.
A rank reports through the ok<rank> / fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXED = dict(tol=0.0, max_iter=12, record_trace=1, check_every=4)
BS = 4


def matrix(name):
    import mp_multi_workers as M
    from mpi_bicgstab_amd import synth
    return synth.transport_like(40000) if name == "transport" else M.matrix(name)


def diagonal_blocks(d, bs):
    """blocks that hold d on their diagonals and zeros elsewhere, the layout of bicg_precond_block_diagonal (1.0 beyond a partial block:
    ignored by the install)"""
    import numpy as np
    nb = -(-d.size // bs)
    dd = np.ones(nb * bs)
    dd[:d.size] = d
    out = np.zeros((nb, bs, bs))
    out[:, np.arange(bs), np.arange(bs)] = dd.reshape(nb, bs)
    return out


def block_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import mp_multi_workers as M
        dist = M._init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        A = matrix(kind)
        n = A.rows
        idx = np.arange(n, dtype=np.int64)
        d_glob = np.ldexp(1.0, np.floor(17.0 * synth._uniform(idx, 31)).astype(np.int64) - 8)      # 2^e, e in [-8, 8]
        H.switches(persist=0)
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        ca = H.Context(H.HostBlocks(diag, offd, n, counts, displs))
        lo, nl = int(displs[rank]), int(counts[rank])
        if kind == "six":
            assert (nl == 0) == (rank >= 6)                 # the seventh rank has no rows: it passes NULL
        else:
            assert ca.plan_info()["halo"] > 0
            assert [int(c) for c in counts] == [13334, 13333, 13333] and nl % BS != 0      # partial last blocks on every rank
        x0 = (0.25 * synth._uniform(idx, 77) - 0.125)[lo:lo + nl]
        b = A.matvec(1.0 + 0.5 * synth._uniform(idx, 78))[lo:lo + nl]
        d = d_glob[lo:lo + nl]

        def counted(call):
            c0 = ca.comm_counts()
            out = call()
            c1 = ca.comm_counts()
            return out, {k: c1[k] - c0[k] for k in c1}

        def raw(a):      # bytes; neither system breaks down within twelve iterations, so a NaN anywhere is a failure of its own
            a = np.array(a, dtype=np.float64)
            assert not np.isnan(a).any(), "a NaN in what a solve reports"
            return a.tobytes()

        def state(ctx, got):
            tr = ctx.trace(got["k"])
            q = got["result"]
            return (got["k"], q.iterations, q.breakdown_iteration, raw(q.dot_r), raw(q.dot_zero),
                    raw(got["x"]), raw(got["r"]), tuple(raw(tr[k]) for k in ("alpha", "omega", "beta", "dotr")))

        def refused():
            got, moved = counted(lambda: ca.solve("bicgstab_block", b, x0=x0, **FIXED))
            assert got["k"] == -2 and got["x"].tobytes() == x0.tobytes() and got["r"].tobytes() == b.tobytes()
            assert moved == dict(exchanges=0, allreduces=0), moved

        # ---- without a block preconditioner: refused on every rank, nothing moves
        refused()
        rc, moved = counted(lambda: ca.set_diagonal(d if nl else None))
        assert rc == 0 and moved == dict(exchanges=0, allreduces=0), (rc, moved)
        refused()                                           # a diagonal one is not a block one
        want, d_diag = counted(lambda: state(ca, ca.solve("bicgstab_diag", b, x0=x0, **FIXED)))
        assert want[0] == 12 or kind == "six", want[0]
        # ---- blocks that hold d: method 4, bit for bit
        rc, moved = counted(lambda: ca.set_block_diagonal(diagonal_blocks(d, BS) if nl else None, BS))
        assert rc == 0 and moved == dict(exchanges=0, allreduces=0), (rc, moved)
        assert ca.preconditioner() == "block_diagonal"
        got, d_block = counted(lambda: state(ca, ca.solve("bicgstab_block", b, x0=x0, **FIXED)))
        assert got == want, "blocks = d"
        assert d_block == d_diag and d_diag["allreduces"] > 0, (d_diag, d_block)
        M.same_on_every_rank(dist, world, (got[0], got[3], got[4], got[7]), "blocks = d")
        got = ca.solve("bicgstab_diag", b, x0=x0, **FIXED)  # ... and method 4 is refused now
        assert got["k"] == -2
        assert not ca.comm_failed()
        ca.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
