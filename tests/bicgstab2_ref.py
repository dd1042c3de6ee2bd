"""Plain numpy restatements of BiCGStab(2) (the sweep in include/bicgstab_hip.h at BICG_BICGSTAB2) and of
plain BiCGStab (the loop of reference src/solver.c:74-120), float64 throughout. No library call: the tests compare the device's
method 6 against `sweeps`, and `sweeps` against `plain` for the claim that it works where the plain method does not.

Every element-wise update is evaluated as the kernels evaluate it: term by term from the left, one multiply and one add each. A row
of a product adds its entries in stored order, each product rounded on its own. What is left open is the association of the dot
sums: numpy's pairwise blocks by default; extended=True accumulates every dot in np.longdouble and rounds once -- the gap between
the two runs is what a different association does to the recurrence, measured on the restatement alone."""
import numpy as np


class Product:
    """y = A x for a synth.CSR, every row summed in stored order (0 + a_0 x_0) + a_1 x_1 + ..."""

    def __init__(self, A):
        ptr = A.ptr.astype(np.int64)
        self.n = A.rows
        length = np.diff(ptr)
        self.steps = []
        for k in range(int(length.max()) if self.n else 0):
            rows = np.nonzero(length > k)[0]
            at = ptr[rows] + k
            self.steps.append((rows, A.val[at], A.col[at].astype(np.int64)))

    def __call__(self, x):
        y = np.zeros(self.n)
        for rows, val, col in self.steps:
            y[rows] += val * x[col]
        return y


def _dot(extended):
    if extended:
        return lambda a, b: np.float64(np.sum(a.astype(np.longdouble) * b.astype(np.longdouble)))
    return lambda a, b: np.float64(np.dot(a, b))      # (numpy scalars: x / 0 is inf or NaN, not an exception)


def sweeps(A, b, x0, max_iter, tol, extended=False):
    """BiCGStab(2). Returns dict(x, r, k, dot_r, dot_zero, breakdown, trace) with trace = dict(alpha, beta, omega, dotr), arrays of
    length k: entries k-2 / k-1 of a sweep hold the alpha and beta of its steps j = 0 / 1, omega holds g1 / g2, dotr the sweep's
    final (r0,r0) twice. k counts BiCG steps; a sweep runs while dot_r > tol^2 dot_zero and k + 2 <= max_iter."""
    mul = A if callable(A) else Product(A)
    dot = _dot(extended)
    x = np.array(x0, dtype=np.float64)
    r0 = b + (-1.0) * mul(x)
    rh = r0.copy()
    n = r0.size
    u0, u1, u2 = np.zeros(n), np.zeros(n), np.zeros(n)
    rho0, alpha, omega = np.float64(1.0), np.float64(0.0), np.float64(1.0)
    dot_zero = dot_r = dot(r0, r0)
    rho1 = dot_r                      # (r#,r0) with r# = r0
    tr = dict(alpha=[], beta=[], omega=[], dotr=[])
    k, breakdown = 0, 0
    with np.errstate(all="ignore"):
        while dot_r > tol * tol * dot_zero and k + 2 <= max_iter:
            rho0 = (-omega) * rho0
            # j = 0
            beta = alpha * (rho1 / rho0); rho0 = rho1
            b_j0 = beta
            u0 = r0 + (-beta) * u0
            u1 = mul(u0)
            alpha = rho0 / dot(rh, u1)
            a_j0 = alpha
            x = x + alpha * u0
            r0 = r0 + (-alpha) * u1
            r1 = mul(r0)
            rho1 = dot(rh, r1)
            # j = 1
            beta = alpha * (rho1 / rho0); rho0 = rho1
            u0 = r0 + (-beta) * u0
            u1 = r1 + (-beta) * u1
            u2 = mul(u1)
            alpha = rho0 / dot(rh, u2)
            x = x + alpha * u0
            r0 = r0 + (-alpha) * u1
            r1 = r1 + (-alpha) * u2
            r2 = mul(r1)
            # MR
            a11, b1, a12, a22, b2 = dot(r1, r1), dot(r0, r1), dot(r1, r2), dot(r2, r2), dot(r0, r2)
            det = a11 * a22 - a12 * a12
            g1 = (b1 * a22 - b2 * a12) / det
            g2 = (a11 * b2 - a12 * b1) / det
            x = (x + g1 * r0) + g2 * r1
            r0 = (r0 + (-g1) * r1) + (-g2) * r2
            u0 = (u0 + (-g1) * u1) + (-g2) * u2
            omega = g2
            dot_r = dot(r0, r0)
            rho1 = dot(rh, r0)
            k += 2
            tr["alpha"] += [a_j0, alpha]; tr["beta"] += [b_j0, beta]; tr["omega"] += [g1, g2]; tr["dotr"] += [dot_r, dot_r]
            if not np.all(np.isfinite([alpha, beta, g1, g2, dot_r])):
                breakdown = k
                break
    return dict(x=x, r=r0, k=k, dot_r=dot_r, dot_zero=dot_zero, breakdown=breakdown, trace={q: np.array(v) for q, v in tr.items()})


def plain(A, b, x0, max_iter, tol):
    """Plain BiCGStab, reference src/solver.c:74-120. Returns dict(x, r, k, dot_r, dot_zero, finite): finite is False once a
    recurrence scalar or (r,r) is not finite (the loop stops there)."""
    mul = A if callable(A) else Product(A)
    dot = _dot(False)
    x = np.array(x0, dtype=np.float64)
    r = b + (-1.0) * mul(x)
    rh, p = r.copy(), r.copy()
    rTr = dot_zero = dot_r = dot(r, r)
    k, finite = 0, True
    with np.errstate(all="ignore"):
        while dot_r > tol * tol * dot_zero and k < max_iter:
            s = mul(p)
            alpha = rTr / dot(rh, s)
            q = r + (-alpha) * s
            y = mul(q)
            omega = dot(q, y) / dot(y, y)
            x = (x + alpha * p) + omega * q
            r = q + (-omega) * y
            dot_r = dot(r, r)
            rTr_old, rTr = rTr, dot(rh, r)
            beta = (alpha / omega) * (rTr / rTr_old)
            p = (beta * p + 1.0 * r) + (-beta * omega) * s
            k += 1
            if not np.all(np.isfinite([alpha, omega, beta, dot_r])):
                finite = False
                break
    return dict(x=x, r=r, k=k, dot_r=dot_r, dot_zero=dot_zero, finite=finite)


def true_relres(A, b, x):
    mul = A if callable(A) else Product(A)
    return float(np.linalg.norm(b - mul(x)) / np.linalg.norm(b))


def convection(m, c):
    """the issue's matrix family: 7-point diffusion 1, central-difference convection c in each direction"""
    from mpi_bicgstab_amd import synth
    return synth.stencil7(m, (6.05, -1 - c, -1 + c, -1 - c, -1 + c, -1 - c, -1 + c))


def rhs(A, seed):
    from mpi_bicgstab_amd import synth
    mul = A if callable(A) else A.matvec
    return mul(1.0 + 0.5 * synth._uniform(np.arange(A.rows, dtype=np.int64), seed))


def gap(a, b):
    """largest |a - b| relative to the largest magnitude of a"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = float(np.max(np.abs(a))) if a.size else 0.0
    return float(np.max(np.abs(a - b))) / scale if scale > 0.0 else 0.0
