"""Worker of tests/test_shifted_exact_gpu.py::test_two_ranks_persistent: `world` spawned processes share cuda:0 (gloo rendezvous on
127.0.0.1, the peer-to-peer data path set up as in tests/mp_update_workers.py). Every rank holds its rows of the integer system
exact_dots.RANK_SHIFTED, runs shifted_lopbicgstab and shifted_pipe_lopbicgstab for one iteration in the persistent form -- the
helper workgroups add the ranks' sums through the mailboxes -- and must report the WHOLE system's exact first scalars and its rows
of every x_j and of r as the bytes of the CPU oracle at two ranks. A rank reports through the ok<rank> / fail<rank> files of
mp_workers.py; a peer-to-peer path that does not come up is a failure."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def shifted_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import mp_multi_workers as M
        dist = M._init(rank, world, port)
        import exact_dots as E
        from mpi_bicgstab_amd import hipsolver as H
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        rc = H.lib().bicg_comm_enable_p2p()
        assert rc == 0, f"bicg_comm_enable_p2p() returned {rc}: ranks sharing one device reach each other's memory"
        n, lists = E.RANK_SHIFTED
        A, b = E.system(n)
        blk, lo, nl = E.host_blocks(A, world, rank)
        ctx = H.Context(blk)
        fl, info = ctx.flags(), ctx.plan_info()
        assert fl["persist"] and fl["p2p"], fl
        assert info["rows"] == nl and info["halo"] > 0, info
        for i in lists:
            nsig, seed, sg = E.list_case(i)
            sigma = E.shift_list(nsig, seed, sg)
            F = E.shifted_first(n, (), 600, sg)
            for which in ("shifted_lopbicgstab", "shifted_pipe_lopbicgstab"):
                want = F.scalars(which)
                o = E.oracle_shifted(A, b, which, sigma, seed, nranks=world, tol=0.0, max_iter=1)
                got = ctx.solve_shifted(b[lo:lo + nl].astype(np.float64), sigma, seed, which=which, tol=0.0, max_iter=1, check_every=1,
                                        record_trace=1)
                where = (rank, which, nsig, seed, sg)
                assert ctx.last_shifted_persistent() and not ctx.comm_failed(), where
                tr = ctx.trace(1)
                print(where, "alpha", tr["alpha"][0], "omega", tr["omega"][0].hex(), "beta", tr["beta"][0].hex())
                assert got["k"] == o["k"] == 1, where + (got["k"], o["k"])
                assert E.same_bytes(got["result"].dot_zero, want["dot_zero"]), where + (got["result"].dot_zero, want["dot_zero"])
                for key in ("alpha", "omega", "beta", "dotr"):
                    if key in want:
                        assert E.same_bytes(tr[key][0], want[key]), where + (key, tr[key][0], want[key])
                    else:                     # pipe: omega is not dyadic, r is rounded: the rational replay's derived bounds
                        R = F.residual_dots(E.recurrence(which))
                        assert E.within(tr[key][0], R[key], R[key + "_bound"]), where + (key, tr[key][0], float(R[key]), float(R[key + "_bound"]))
                mine = o["x"][:, lo:lo + nl]
                bad = [j for j in range(nsig) if got["x"][j].tobytes() != np.ascontiguousarray(mine[j]).tobytes()]
                assert not bad, where + ("shifts whose rows differ from the oracle's", bad)
                assert got["r"].tobytes() == np.ascontiguousarray(o["r"][lo:lo + nl]).tobytes(), where + ("r",)
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
