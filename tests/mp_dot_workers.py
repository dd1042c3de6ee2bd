"""Worker of tests/test_dot_groups_gpu.py::test_two_ranks: `world` spawned processes share cuda:0 through the host-staged transport
(gloo rendezvous on 127.0.0.1, as tests/mp_update_workers.py). Every rank holds its rows of an integer system of
tests/exact_dots.py, asserts the launch geometry the case is there for -- interior sliced-ELL groups and CSR row blocks, then
one or two halo-touching workgroups in the same dot group -- and must report the WHOLE matrix's exact dot_zero, alpha[0] and
omega[0] as bytes. A rank reports through the ok<rank> / fail<rank> files of mp_workers.py."""
from __future__ import annotations

import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def dot_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        import mp_multi_workers as M
        dist = M._init(rank, world, port)
        import exact_dots as E
        from mpi_bicgstab_amd import hipsolver as H
        from mpi_bicgstab_amd import dist_transport as T

        T.init_host_transport(0)
        n, groups, L, want = E.RANK_SHAPES[kind]
        A, b = E.system(n, groups, L)
        F = E.first(n, groups, L)
        blk, lo, nl = E.host_blocks(A, world, rank)
        H.switches(persist=0)
        ctx = H.Context(blk)
        fl, info = ctx.flags(), ctx.plan_info()
        g_int, g_bnd, b_int, b_bnd = want[rank]
        assert info["rows"] == nl and info["halo"] > 0, info
        assert info["row_blocks"] == g_int + g_bnd + b_int + b_bnd and info["boundary_blocks"] == g_bnd + b_bnd, info
        assert info["sell_rows"] == E.GROUP * (g_int + g_bnd), info
        # host-staged collectives, no peer-to-peer path: the tail finish is on, and a product is interior launches followed by
        # halo-touching ones (CSR row blocks keep the plan from the single merged launch)
        assert not fl["p2p"] and not fl["persist"] and not fl["all_sell"] and fl["tail_finish"] and not fl["handover"], fl
        H.product_kernels()
        got = ctx.solve("bicgstab", b[lo:lo + nl].astype(np.float64), tol=0.0, max_iter=3, check_every=3, record_trace=1)
        assert "csr" in H.product_kernels()
        tr = ctx.trace(got["k"])
        assert got["k"] == 3 and not ctx.comm_failed()
        print(kind, rank, "dot_zero", got["result"].dot_zero, F.dot_zero, "alpha", tr["alpha"][0], "omega", tr["omega"][0].hex(), F.omega.hex())
        assert E.same_bytes(got["result"].dot_zero, F.dot_zero), (got["result"].dot_zero, F.dot_zero)
        assert E.same_bytes(tr["alpha"][0], F.alpha), (tr["alpha"][0], F.alpha)
        assert E.same_bytes(tr["omega"][0], F.omega), (tr["omega"][0], F.omega)
        i = np.arange(lo, lo + nl)
        u, v = 1 + i % 7, 1 + i % 5
        j = np.arange(n)
        assert E.same_bytes(ctx.dot(u.astype(np.float64), v.astype(np.float64)), float(E.isum((1 + j % 7) * (1 + j % 5))))
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
