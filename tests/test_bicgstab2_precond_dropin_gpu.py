"""`-m gpu`: the callers of the right-preconditioned BiCGStab(2) (methods 7 and 8) that do not go through
Context.solve -- the drop-ins `jacobi_bicgstab2()` / `block_jacobi_bicgstab2()` (csrc/bicg_dropin.cpp) and `bicg_solver_host <matrix>
jacobi_bicgstab2` (host/bicg_main.c).

Systems S2 (scaled convection stencil, Jacobi) and S4 (block-coupled convection stencil, 4 x 4 blocks) of
tests/bicgstab2_precond_ref.py, b = R.rhs(A, 78), x0 = 0, tol 1e-10 and at most 40 steps from the environment as the drop-ins read
them. Context.solve on a context of the same blocks with the same preconditioner is the reference: k, x and r of the drop-in are the
same bytes. What the drop-ins print is what bicgstab() prints on the same matrix at the same step count: the same lines up to their
numbers. What they cannot install ends the process with the lines of jacobi_bicgstab() / block_jacobi_bicgstab(). The drop-in cache
is read once per process, hence children."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mpi_bicgstab_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mpi-bicgstab_amd", "host", "bicg_solver_host")
MPIEXEC = "/opt/conda/bin/mpiexec"
ENV = dict(BICG_MAX_ITER="40", BICG_TOL="1e-10", BICG_OUT_ITER="10")

CHILD = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
from mpi_bicgstab_amd import hipsolver as H, synth
import bicgstab2_ref as R, bicgstab2_precond_ref as Q
L = H.lib()
L.bicg_comm_init_single(0)
name, out = sys.argv[1], sys.argv[2]
A = Q.systems()[name]()
blk = H.single_rank_blocks(A)
b, x0 = R.rhs(A, 78), np.zeros(A.rows)
ctx = H.Context(blk)
if name == "S2":
    assert ctx.set_diagonal(Q.diagonal(A)) == 0
    method, call = "bicgstab2_diag", lambda x, r: L.jacobi_bicgstab2(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r))
else:
    assert ctx.set_block_diagonal(Q.blocks_of(A, 4), 4) == 0
    method, call = "bicgstab2_block", lambda x, r: L.block_jacobi_bicgstab2(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r), 4)
want = ctx.solve(method, b, x0=x0, tol=1e-10, max_iter=40)
ctx.close()
sys.stdout.flush()
print("BEGIN new", flush=True)
x, r = x0.copy(), b.copy()
k = call(x, r)
x2, r2 = x0.copy(), b.copy()       # a second call: the resident context, the preconditioner installed again
k2 = call(x2, r2)
print("BEGIN plain", flush=True)
xp, rp = x0.copy(), b.copy()
kp = L.bicgstab(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(xp), H._d(rp))
print("END", flush=True)
L.bicg_dropin_release()
np.savez(out, k=k, x=x, r=r, k2=k2, x2=x2, r2=r2, kp=kp, want_k=want["k"], want_x=want["x"], want_r=want["r"],
         breakdown=want["result"].breakdown_iteration)
"""


def shape(lines):
    """printed lines with every number replaced"""
    return [re.sub(r"[-+]?\d+(\.\d+)?(e[-+]?\d+)?", "#", ln) for ln in lines]


@pytest.mark.parametrize("name", ["S2", "S4"])
def test_drop_ins_give_the_bytes_of_context_solve_and_print_bicgstabs_lines(name, tmp_path):
    out = str(tmp_path / "child.npz")
    env = {k: v for k, v in os.environ.items() if k not in ("BICG_DROPIN_CACHE", "BICG_QUIET")}
    p = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT), name, out], env=dict(env, **ENV), capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    s = np.load(out)
    assert int(s["breakdown"]) == 0 and int(s["want_k"]) == 40 == int(s["kp"])      # the reduced cap decided, for both
    for tag in ("", "2"):
        assert int(s["k" + tag]) == 40
        assert s["x" + tag].tobytes() == s["want_x"].tobytes() and s["r" + tag].tobytes() == s["want_r"].tobytes()
    lines = p.stdout.splitlines()
    new = lines[lines.index("BEGIN new") + 1:lines.index("BEGIN plain")]
    plain = lines[lines.index("BEGIN plain") + 1:lines.index("END")]
    print("\n".join(new))
    assert len(plain) == 8 and plain[0].startswith("Iteration: 10, Residual: ") and plain[4] == "Total iter   : 40"
    assert shape(new) == shape(plain) + shape(plain)                                  # two calls
    assert new[:6] == new[8:14]                                                       # the same solve twice (the two time lines differ)
    assert new[3].startswith("Iteration: 40, Residual: ") and new[4] == "Total iter   : 40"


REFUSED_CHILD = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %(root)r)
from mpi_bicgstab_amd import hipsolver as H, synth
L = H.lib()
L.bicg_comm_init_single(0)
n = 64
what, fn, bs = sys.argv[1], sys.argv[2], int(sys.argv[3])
if what == "missing":      # row 1 stores no (1,1)
    ptr = np.concatenate([[0, 1, 2], 2 + np.arange(1, n - 1)]).astype(np.uint32)
    col = np.concatenate([[0, 0], np.arange(2, n)]).astype(np.uint32)
    val = np.concatenate([[4.0, 1.0], np.full(n - 2, 4.0)])
else:                      # the first 2 x 2 block is exactly singular
    ptr = np.concatenate([[0, 2, 4], 4 + np.arange(1, n - 1)]).astype(np.uint32)
    col = np.concatenate([[0, 1, 0, 1], np.arange(2, n)]).astype(np.uint32)
    val = np.concatenate([[0.5, 2.0, 0.25, 1.0], np.full(n - 2, 4.0)])
A = synth.CSR(n, n, ptr, col, val)
blk = H.single_rank_blocks(A)
x, r = np.zeros(n), np.ones(n)
if fn == "jacobi":
    L.jacobi_bicgstab2(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r))
else:
    L.block_jacobi_bicgstab2(C.byref(blk.diag), C.byref(blk.offd), C.byref(blk.info), H._d(x), H._d(r), bs)
print("RETURNED")
"""


@pytest.mark.parametrize("what,fn,bs,line", [("missing", "jacobi", 0, "Error: matrix has rows without a diagonal entry."),
                                             ("singular", "block", 2, "Error: matrix has a singular diagonal block."),
                                             ("singular", "block", 17, "Error: block size 17 is outside 1..16."),
                                             ("singular", "block", 0, "Error: block size 0 is outside 1..16.")])
def test_drop_ins_exit_on_what_they_cannot_install(what, fn, bs, line):
    env = dict(os.environ, BICG_QUIET="1", BICG_MAX_ITER="6")
    p = subprocess.run([sys.executable, "-c", REFUSED_CHILD % dict(root=ROOT), what, fn, str(bs)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 1, (p.returncode, p.stderr[-2000:])
    assert line in p.stderr.splitlines() and "RETURNED" not in p.stdout


def test_host_driver_accepts_the_solver_names(tmp_path):
    path = str(tmp_path / "offsets.mtx")
    synth.write_mtx(path, synth.from_offsets(6007, (0, 1, -1, 50, -50, 51, -51, 2000, -2000), diag_base=12.0, seed=8))
    env = dict(os.environ, BICG_QUIET="1", BICG_MAX_ITER="40", BICG_TOL="1e-10")
    for method in (["jacobi_bicgstab2"], ["block_jacobi_bicgstab2"], ["block_jacobi_bicgstab2", "3"]):
        cmd = [HOST, path] + method
        if os.path.exists(MPIEXEC):
            cmd = [MPIEXEC, "-n", "1"] + cmd
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and "Unknown method" not in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    usage = subprocess.run(([MPIEXEC, "-n", "1"] if os.path.exists(MPIEXEC) else []) + [HOST], capture_output=True, text=True, timeout=60)
    assert "  jacobi_bicgstab2\n" in usage.stdout and "  block_jacobi_bicgstab2 [" in usage.stdout
