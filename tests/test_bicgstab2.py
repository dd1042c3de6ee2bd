"""Without a GPU: BiCGStab(2) (method BICG_BICGSTAB2 = 6).

1. On the numpy restatements of tests/bicgstab2_ref.py alone -- the claim the method is there for: on the convection-dominated
   stencils synth.stencil7(m, (6.05, -1-c, -1+c, ...)) with b = A (1 + 0.5 u), u = synth._uniform(idx, seed), seeds 78..81, x0 = 0,
   tol 1e-10, BiCGStab(2) needs at most half the BiCG steps of plain BiCGStab at c = 5 (m = 16), and at c = 20 (m = 12 and 16) it
   reaches a true relative residual <= 1e-9 within 300 steps where the plain recurrence ends non-finite or above the tolerance at
   1000 steps on every seed. The GPU tests compare the device with `sweeps`; they do not assert that the device's plain method fails.
2. The public surface: the method table of the binding, the header's enum value and drop-in, the exported symbol."""
import os
import re

import numpy as np
import pytest

import bicgstab2_ref as R
from mpi_bicgstab_amd import hipsolver as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (78, 79, 80, 81)
TOL = 1e-10


def both(m, c, seed):
    A = R.convection(m, c)
    P = R.Product(A)
    b, x0 = R.rhs(A, seed), np.zeros(A.rows)
    s = R.sweeps(P, b, x0, 1000, TOL)
    p = R.plain(P, b, x0, 1000, TOL)
    return P, b, s, p


@pytest.mark.parametrize("seed", SEEDS)
def test_half_the_steps_of_plain_bicgstab_at_c5(seed):
    P, b, s, p = both(16, 5, seed)
    print("m 16 c 5 seed", seed, "BiCGStab(2) k", s["k"], "plain k", p["k"], "ratio %.3f" % (s["k"] / p["k"]))
    assert p["finite"] and p["k"] < 1000 and not s["breakdown"]
    assert R.true_relres(P, b, s["x"]) <= 1e-9
    assert s["k"] <= 0.5 * p["k"], (s["k"], p["k"])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("m", (12, 16))
def test_converges_at_c20_where_plain_bicgstab_does_not(m, seed):
    P, b, s, p = both(m, 20, seed)
    rel = R.true_relres(P, b, s["x"])
    plain_rel = float(np.sqrt(p["dot_r"] / p["dot_zero"]))
    print("m", m, "c 20 seed", seed, "BiCGStab(2) k", s["k"], "true relres %.2e" % rel, "plain k", p["k"], "finite", p["finite"],
          "relres %.2e" % plain_rel)
    assert not p["finite"] or (p["k"] == 1000 and not plain_rel <= TOL), (p["k"], p["finite"], plain_rel)
    assert not s["breakdown"] and s["k"] <= 300 and rel <= 1e-9, (s["k"], rel)


def test_restatement_semantics():
    """k advances by 2, never passes max_iter, the trace is filled pairwise, a 1 x 1 system breaks down in its first sweep"""
    A = R.convection(6, 5)
    b, x0 = R.rhs(A, 78), np.zeros(A.rows)
    assert R.sweeps(A, b, x0, 7, 0.0)["k"] == 6
    for cap in (0, 1):
        got = R.sweeps(A, b, x0, cap, 0.0)
        assert got["k"] == 0 and got["x"].tobytes() == x0.tobytes()
    assert R.sweeps(A, np.zeros(A.rows), x0, 10, 1e-10)["k"] == 0
    got = R.sweeps(A, b, x0, 4, 0.0)
    tr = got["trace"]
    assert all(len(tr[q]) == 4 for q in tr) and tr["dotr"][0] == tr["dotr"][1] == R.sweeps(A, b, x0, 2, 0.0)["dot_r"]
    assert tr["beta"][0] == 0.0 and tr["dotr"][3] == got["dot_r"]
    ext = R.sweeps(A, b, x0, 4, 0.0, extended=True)
    assert 0.0 < R.gap(ext["trace"]["alpha"], tr["alpha"]) < 1e-12
    from mpi_bicgstab_amd import synth
    one = synth.transport_like(1)
    got = R.sweeps(one, one.matvec(np.array([1.25])), np.array([0.1]), 6, 0.0)
    assert got["k"] == 2 and got["breakdown"] == 2


def test_method_table_and_header():
    assert H.METHODS["bicgstab2"] == 6 and H.LATER_METHODS["bicgstab2"] == 6
    assert len(H.METHODS) == 5 and "bicgstab2" not in list(H.METHODS)
    hdr = open(os.path.join(ROOT, "include", "bicgstab_hip.h")).read()
    assert re.search(r"\bBICG_BICGSTAB2\s*=\s*6\b", hdr)

    def params(name):
        m = re.search(r"^int\s+%s\s*\(([^)]*)\)\s*;" % name, hdr, re.M)
        assert m, name
        return re.sub(r"\s+", " ", m.group(1)).strip()
    assert params("bicgstab2") == params("bicgstab")
    for word in ("k + 2 <= max_iter", "ceil(n / 2)", "omega[k-2] = g1", "BICG_GRAPH=1", "return -2", "Out of scope"):
        assert word in hdr, word


def test_library_exports_the_drop_in():
    L = H.lib()
    assert hasattr(L, "bicgstab2")
    assert L.bicgstab2.argtypes == L.bicgstab.argtypes
