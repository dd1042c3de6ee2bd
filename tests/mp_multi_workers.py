"""Worker of tests/test_multi_rhs_ranks_gpu.py: `world` spawned processes share cuda:0 through the host-staged transport (gloo
rendezvous on 127.0.0.1) and call bicg_solve_multi collectively. The parent leaves the inputs and the oracle's solves at the same
rank count in <outdir>/oracle.npz (xs, B [nrhs][n]; k [nrhs]; x [nrhs][n]; alpha / omega / beta / dotr [nrhs][max k]); a rank
reports through the ok<rank> / fail<rank> files of mp_workers.py, or skip<rank> with the reason."""
from __future__ import annotations

import os
import sys
import traceback
from datetime import timedelta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TOL = 1e-12


def _init(rank, world, port):
    import torch
    torch.set_num_threads(1)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    # a collective that never completes ends the worker (and with it the test) instead of sitting on the machine
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    return dist


def matrix(kind):
    import mp_workers as W
    from mpi_bicgstab_amd import synth
    if kind == "six":          # the 6-row matrix of mp_workers.empty_rank_worker
        return synth.from_offsets(6, (0, 1, -1, 2), diag_base=5.0, seed=1)
    return W.test_matrix(kind)


def column_state(ctx, got, j):
    """everything bicg_solve_multi reports about column j on this rank, as bytes (tests/test_multi_rhs_gpu.py)"""
    import numpy as np
    q = got["results"][j]
    tr = ctx.multi_trace(j, int(got["k"][j]))
    return (int(got["k"][j]), q.iterations, q.breakdown_iteration, np.float64(q.dot_r).tobytes(), np.float64(q.dot_zero).tobytes(),
            got["x"][j].tobytes(), got["r"][j].tobytes(), tuple(tr[k].tobytes() for k in ("alpha", "omega", "beta", "dotr")))


def whole_state(ctx, got):
    return [column_state(ctx, got, j) for j in range(len(got["k"]))]


def scalar_state(state):
    """the part of a state that every rank must report with the same bytes: all of it but the rank's rows of x and r"""
    return [(s[0], s[1], s[2], s[3], s[4], s[7]) for s in state]


def same_on_every_rank(dist, world, obj, what):
    out = [None] * world
    dist.all_gather_object(out, obj)
    assert all(o == out[0] for o in out), f"{what}: the ranks report different bytes"
    return out[0]


def assert_oracle_bars(ctx, got, ref, lo, nl, what, singular=False, cols=None):
    """the bars of tests/test_multi_rhs_gpu.py against the oracle at the same rank count; singular: x against the oracle's x"""
    import numpy as np
    for j in (range(len(got["k"])) if cols is None else cols):
        k, ko = int(got["k"][j]), int(ref["k"][j])
        xo = ref["x"][j]
        err = np.abs(got["x"][j] - ref["xs"][j, lo:lo + nl]).max() if nl else 0.0
        err_o = np.abs(got["x"][j] - xo[lo:lo + nl]).max() if nl else 0.0
        print(what, "column", j, "k", k, "oracle", ko, "|x - x*|", err, "|x - x_o|", err_o, flush=True)
        assert abs(k - ko) <= 2, (what, j, k, ko)
        if singular:
            assert err_o <= 1e-8 * max(1.0, np.abs(xo).max()), (what, j, err_o)
        else:
            assert err <= 1e-9, (what, j, err)
        tr = ctx.multi_trace(j, k)
        m = min(6, k, ko)
        for name in ("alpha", "omega", "beta", "dotr"):
            assert np.allclose(tr[name][:m], ref[name][j, :m], rtol=1e-8, atol=0.0), (what, j, name, tr[name][:m], ref[name][j, :m])


def _delta(ctx, before):
    now = ctx.comm_counts()
    return {k: now[k] - before[k] for k in now}


def multi_worker(rank, world, port, kind, outdir):
    try:
        import numpy as np
        dist = _init(rank, world, port)
        from mpi_bicgstab_amd import hipsolver as H, synth
        from mpi_bicgstab_amd import dist_transport as T

        case, name = kind.split(":")
        T.init_host_transport(0)
        if case == "p2p":
            rc = H.lib().bicg_comm_enable_p2p()
            if rc != 0:
                open(os.path.join(outdir, f"skip{rank}"), "w").write(f"bicg_comm_enable_p2p() returned {rc}")
                dist.barrier()
                H.lib().bicg_comm_finalize()
                dist.destroy_process_group()
                return
        ref = np.load(os.path.join(outdir, "oracle.npz"))
        A = matrix(name)
        diag, offd, counts, displs = synth.split_blocks(A, world, rank)
        lo, nl = int(displs[rank]), int(counts[rank])
        ctx = H.Context(H.HostBlocks(diag, offd, A.rows, counts, displs))
        B = np.ascontiguousarray(ref["B"][:, lo:lo + nl])
        nrhs = B.shape[0]
        singular = name == "ragged"
        solve = lambda b, **kw: ctx.solve_multi(b, nrhs=len(b), tol=kw.pop("tol", TOL), record_trace=1, **kw)

        if case == "oracle":
            # ---- 1. the oracle's bars, 2. every rank reports the same bytes; a second run gives the bytes of the first
            assert ctx.flags()["spmm"] == (name != "ragged"), ctx.flags()      # ragged: a 700-entry row -> the per-column product
            got = solve(B)
            state = whole_state(ctx, got)
            assert_oracle_bars(ctx, got, ref, lo, nl, f"{name} P={world}", singular)
            assert got["rc"] == max(got["k"])
            assert got["k"][1] == 0 and got["results"][1].iterations == 0
            assert got["x"][1].tobytes() == np.zeros(nl).tobytes()
            if name == "stencil":
                assert len(set(int(k) for k in got["k"])) >= 3, got["k"]      # the columns stop at different iterations
            same_on_every_rank(dist, world, scalar_state(state), "first run")
            again = solve(B)
            assert whole_state(ctx, again) == state, "a second run gives other bytes"
        elif case == "neighbours":
            # ---- 3. a column does not know its neighbours, nor how often the host looked
            got = solve(B)
            state = whole_state(ctx, got)
            ks = [int(k) for k in got["k"]]        # (the same on every rank: every rank picks the same columns)
            running = [j for j in range(nrhs) if ks[j] > 0]
            fast, slow = min(running, key=lambda j: ks[j]), max(running, key=lambda j: ks[j])
            assert nrhs == 21
            for j in sorted({fast, slow, 1, 18}):
                one = solve(B[j:j + 1])
                assert column_state(ctx, one, 0) == state[j], (name, j)
            for every in (1, 7):
                assert whole_state(ctx, solve(B, check_every=every)) == state, every
        elif case == "counts":
            # ---- 4. one exchange per set and product, 5. one all-reduce per dot group of a set
            assert ctx.flags()["spmm"] and nrhs == 16 and ctx.plan_info()["halo"] > 0
            opts = dict(tol=0.0, max_iter=3, check_every=1)
            c0 = ctx.comm_counts()
            state = whole_state(ctx, solve(B, **opts))
            d16 = _delta(ctx, c0)
            assert d16["exchanges"] == 1 + 2 * 3, d16      # s = A x0, then s = A p and y = A q of three iterations
            assert [s[0] for s in state] == [0 if j == 1 else 3 for j in range(16)]
            H.switches(halo_set=0)                         # read at the call
            try:
                c0 = ctx.comm_counts()
                per_column = whole_state(ctx, solve(B, **opts))
                assert _delta(ctx, c0)["exchanges"] == 7 * 16
            finally:
                H.switches(halo_set=None)
            assert per_column == state, "halo-set=0 changes the result"
            H.switches(spmm=0)
            try:
                assert whole_state(ctx, solve(B, **opts)) == state, "spmm=0 changes the result"
            finally:
                H.switches(spmm=None)
            c0 = ctx.comm_counts()
            solve(B[4:5], **opts)
            d1 = _delta(ctx, c0)
            print("all-reduces: 16 columns", d16["allreduces"], "1 column", d1["allreduces"], flush=True)
            assert d16["allreduces"] <= d1["allreduces"], (d16, d1)
            same_on_every_rank(dist, world, (d16["allreduces"], d1["allreduces"]), "all-reduce counts")
            X = np.random.default_rng(17).standard_normal((16, A.rows))[:, lo:lo + nl]
            c0 = ctx.comm_counts()
            Y = ctx.spmm(X)[0]
            assert _delta(ctx, c0)["exchanges"] == 1
            H.switches(halo_set=0)
            try:
                c0 = ctx.comm_counts()
                Y1 = ctx.spmm(X)[0]
                assert _delta(ctx, c0)["exchanges"] == 16
            finally:
                H.switches(halo_set=None)
            assert Y.tobytes() == Y1.tobytes(), "bicg_spmm: halo-set changes the products"
        elif case == "empty":
            # ---- 6. ranks without rows call with nrhs and empty arrays
            assert (nl == 0) == (rank >= 6) and nrhs == 3
            got = solve(B) if nl else ctx.solve_multi(np.zeros((3, 0)), nrhs=3, tol=TOL, record_trace=1)
            assert got["rc"] >= 0 and got["x"].shape == (3, nl) and len(got["k"]) == 3
            if nl:
                assert_oracle_bars(ctx, got, ref, lo, nl, f"six P={world}")
            same_on_every_rank(dist, world, [int(k) for k in got["k"]], "iteration counts")
        elif case == "disagree":
            # ---- 7. different arguments: -1 everywhere, nothing touched, and the communicator stays in step
            mine = 5 if rank == 0 else 3
            X0 = np.full((mine, nl), 0.25)
            got = ctx.solve_multi(B[:mine], X0=X0, tol=TOL)
            assert got["rc"] == -1, got["rc"]
            assert got["x"].tobytes() == X0.tobytes() and got["r"].tobytes() == B[:mine].tobytes()
            X0 = np.full((3, nl), 0.25)
            got = ctx.solve_multi(B[:3], X0=X0, method="ca_bicgstab", tol=TOL)
            assert got["rc"] == -2, got["rc"]
            assert got["x"].tobytes() == X0.tobytes() and got["r"].tobytes() == B[:3].tobytes()
            got = solve(B[:5])
            assert_oracle_bars(ctx, got, ref, lo, nl, "after the refusals")
        elif case == "p2p":
            # ---- 8. a peer-to-peer context: per-column exchanges on its data path, the all-reduces on the transport underneath
            assert H.lib().bicg_comm_p2p_active() > 0 and ctx.flags()["p2p"] and nrhs == 16
            got = solve(B)
            state = whole_state(ctx, got)
            assert_oracle_bars(ctx, got, ref, lo, nl, "p2p")
            one = solve(B[4:5])
            assert column_state(ctx, one, 0) == state[4]
            assert not ctx.comm_failed()
        else:
            raise ValueError(kind)
        ctx.close()
        dist.barrier()
        H.lib().bicg_comm_finalize()
        dist.destroy_process_group()
        open(os.path.join(outdir, f"ok{rank}"), "w").write("ok")
    except Exception:
        open(os.path.join(outdir, f"fail{rank}"), "w").write(traceback.format_exc())
        raise
