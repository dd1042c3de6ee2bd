"""Without a GPU: the right-preconditioned BiCGStab(2), methods BICG_BICGSTAB2_DIAG = 7 and BICG_BICGSTAB2_BLOCK = 8 (DESIGN.md
section 4.24).

1. On the numpy restatements alone (tests/bicgstab2_precond_ref.py, tests/bicgstab2_ref.py) -- the claim the methods are there for.
   Systems: S1 = convection(12, 20) and S2 = convection(16, 5), both scaled A <- D A D over four decades, with Jacobi; S3 =
   block_coupled(4096, 4, convection(16, 5), coupling 48, four decades) with its 4 x 4 blocks. b = R.rhs(A, seed), seeds 78..81, x0 = 0,
   tol 1e-10, max_iter 1000. On every seed
     - hat_sweeps does not break down, reaches a true relative residual <= 1e-9 and needs at most 300 / 100 / 200 BiCG steps
       (caps; observed maxima 260 / 78 / 166),
     - plain BiCGStab and unpreconditioned BiCGStab(2) do not reach the tolerance in 1000 steps,
     - plain BiCGStab on A M^-1 (methods 4 / 5) ends with a non-finite recurrence scalar.
   With the identity for M^-1, hat_sweeps is bicgstab2_ref.sweeps bit for bit.
2. The public surface: enum values, drop-in prototypes, the binding's method table, the exported symbols."""
import functools
import os
import re

import numpy as np
import pytest

import bicgstab2_precond_ref as Q
import bicgstab2_ref as R
from mpi_bicgstab_amd import hipsolver as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (78, 79, 80, 81)
TOL = 1e-10
CASES = {"S1": ("jacobi", 300), "S2": ("jacobi", 100), "S3": ("blocks", 200)}


@functools.lru_cache(maxsize=None)
def system(name):
    A = Q.systems()[name]()
    minv = Q.jacobi(A) if CASES[name][0] == "jacobi" else Q.block_inverse(A, 4)
    return A, R.Product(A), minv


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", list(CASES))
def test_converges_where_every_other_method_fails(name, seed):
    A, mul, minv = system(name)
    cap = CASES[name][1]
    b, x0 = R.rhs(A, seed), np.zeros(A.rows)
    got = Q.hat_sweeps(mul, minv, b, x0, 1000, TOL)
    rel = R.true_relres(mul, b, got["x"])
    print(name, "seed", seed, "hat_sweeps k", got["k"], "true relres %.2e" % rel)
    assert got["breakdown"] == 0 and rel <= 1e-9 and got["k"] <= cap, (got["k"], got["breakdown"], rel)
    for label, fn in (("method 0", R.plain), ("method 6", R.sweeps)):
        other = fn(mul, b, x0, 1000, TOL)
        orel = float(np.sqrt(other["dot_r"] / other["dot_zero"]))
        print("  ", label, "k", other["k"], "relres %.2e" % orel)
        assert other["k"] == 1000 and not orel <= TOL, (label, other["k"], orel)
    hat = R.plain(Q.right(mul, minv), b, x0, 1000, TOL)
    print("   plain BiCGStab on A M^-1: k", hat["k"], "finite", hat["finite"])
    assert not hat["finite"], hat["k"]


@pytest.mark.parametrize("name", ["S2", "S3"])
def test_identity_is_the_unpreconditioned_restatement_bit_for_bit(name):
    A, mul, _ = system(name)
    b = R.rhs(A, 78)
    x0 = np.full(A.rows, 0.125)
    for opts in (dict(max_iter=40, tol=0.0), dict(max_iter=7, tol=0.0), dict(max_iter=1000, tol=1e-3)):
        want = R.sweeps(mul, b, x0, opts["max_iter"], opts["tol"])
        got = Q.hat_sweeps(mul, Q.identity, b, x0, opts["max_iter"], opts["tol"])
        assert got["k"] == want["k"] > 0 and got["breakdown"] == want["breakdown"]
        assert got["x"].tobytes() == want["x"].tobytes() and got["r"].tobytes() == want["r"].tobytes()
        for q in want["trace"]:
            assert got["trace"][q].tobytes() == want["trace"][q].tobytes(), q
        assert got["dot_r"] == want["dot_r"] and got["dot_zero"] == want["dot_zero"]


def test_restatement_helpers():
    """scaled is synth.from_offsets' rule; the block inverse of diagonal blocks is Jacobi; a partial last block is its leading part"""
    from mpi_bicgstab_amd import synth
    offs = (0, 1, -1, 37, -37)
    plain, want = synth.from_offsets(1001, offs, 9.0, seed=5), synth.from_offsets(1001, offs, 9.0, seed=5, scale_decades=3.0)
    got = Q.scaled(plain, 3.0)
    assert got.val.tobytes() == want.val.tobytes() and got.col.tobytes() == want.col.tobytes()
    A = synth.block_coupled(1003, 4, gen=lambda n: synth.from_offsets(n, offs, 9.0, seed=5))      # 250 whole blocks and three rows
    v = 1.0 + synth._uniform(np.arange(A.rows, dtype=np.int64), 3)
    z = Q.block_inverse(A, 4)(v)
    B = Q.blocks_of(A, 4)
    np.testing.assert_allclose(np.einsum("kab,kb->ka", B[:-1], z[:1000].reshape(250, 4)).reshape(-1), v[:1000], rtol=1e-12)
    np.testing.assert_allclose(B[-1, :3, :3] @ z[1000:], v[1000:], rtol=1e-12)
    np.testing.assert_allclose(Q.block_inverse(A, 1)(v), Q.jacobi(A)(v), rtol=1e-15)
    assert Q.jacobi(A, reciprocal=True)(v).tobytes() == ((1.0 / Q.diagonal(A)) * v).tobytes()


def test_method_table_and_header():
    assert H.LATER_METHODS["bicgstab2_diag"] == 7 and H.LATER_METHODS["bicgstab2_block"] == 8
    assert H.METHODS["bicgstab2_diag"] == 7 and H.METHODS["bicgstab2_block"] == 8
    assert len(H.METHODS) == 5 and "bicgstab2_diag" not in list(H.METHODS)
    hdr = open(os.path.join(ROOT, "include", "bicgstab_hip.h")).read()
    assert re.search(r"\bBICG_BICGSTAB2_DIAG\s*=\s*7\b", hdr) and re.search(r"\bBICG_BICGSTAB2_BLOCK\s*=\s*8\b", hdr)

    def params(name):
        m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, hdr, re.M)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()
    assert params("jacobi_bicgstab2") == params("bicgstab")
    assert params("block_jacobi_bicgstab2") == params("block_jacobi_bicgstab")


def test_library_exports_the_drop_ins():
    L = H.lib()
    assert hasattr(L, "jacobi_bicgstab2") and hasattr(L, "block_jacobi_bicgstab2")
    assert L.jacobi_bicgstab2.argtypes == L.bicgstab.argtypes
    assert L.block_jacobi_bicgstab2.argtypes == L.block_jacobi_bicgstab.argtypes
