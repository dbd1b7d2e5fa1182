"""Extended-precision minimiser of the reference's per-element QP ("truth").

TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).

The QP is the one ``lssvr_primal`` hands to SLSQP (Dual.py:46-78).  Its data are
taken exactly as the reference's float64 arithmetic produces them -- collocation
abscissae ``t_k = off + scl*x_k`` (float64), right-hand side ``f(x_k)`` (float64),
``scl`` (float64) -- and from there on everything is done with ``mpmath`` at
``dps`` significant digits: Legendre values/derivatives, the KKT matrix

    [[I + gamma A^T A, B^T], [B, 0]] [w; mu] = [gamma A^T f; g]      

and its LU solve.  ``mpmath`` ships with sympy in this image; when it is missing
the callers fall back to ``oracle.lssvr_oracle.solve_primal_kkt`` (float64).
"""
from __future__ import annotations

import numpy as np

try:  # pragma: no cover - availability probe
    import mpmath as mp
    HAVE_MP = True
except Exception:  # pragma: no cover
    mp = None
    HAVE_MP = False


def _legendre_tables_mp(t, M):
    L = [mp.mpf(1)] + [mp.mpf(0)] * (M - 1)
    D1 = [mp.mpf(0)] * M
    D2 = [mp.mpf(0)] * M
    if M > 1:
        L[1] = t
        D1[1] = mp.mpf(1)
    for p in range(1, M - 1):
        L[p + 1] = ((2 * p + 1) * t * L[p] - p * L[p - 1]) / (p + 1)
        D1[p + 1] = D1[p - 1] + (2 * p + 1) * L[p]
        D2[p + 1] = D2[p - 1] + (2 * p + 1) * D1[p]
    return L, D1, D2


def solve_truth(s, dps=60):
    """``s`` = ``oracle.lssvr_oracle.ElementSystem``.  The rows of -(a u')' + c u = f,

        A = scl^2 (-a D2 - (a'/scl) D1 + (c/scl^2) L),

    are *defined* by the float64 data ``s`` carries -- t_k, scl, f(x_k), g and the samples a(x_k), a'(x_k)/scl,
    c(x_k)/scl^2 (absent: a = 1, a' = 0, c = 0, whose products are exact) -- and are built and solved in mpmath
    from there."""
    if not HAVE_MP:
        raise RuntimeError("mpmath not available")
    mp.mp.dps = dps
    M, n = s.M, s.n
    scl = mp.mpf(float(s.scl))
    gam = mp.mpf(float(s.gamma))
    A = mp.zeros(n, M)
    for k in range(n):
        tk = mp.mpf(float(s.t[k]))
        L, D1, D2 = _legendre_tables_mp(tk, M)
        ak = mp.mpf(1 if s.ak is None else float(s.ak[k]))
        dak = mp.mpf(0 if s.dak is None else float(s.dak[k]))
        ck = mp.mpf(0 if s.ck is None else float(s.ck[k]))
        if s.ak is not None and s.ck is None:
            # -(a u')' = f keeps the definition its truth values were first computed with: a_k as the rounded
            # float64 row holds it, recovered from column 2 (L_2'' = 3, L_2' = 3t; column 1 is -a'/scl exactly).
            # The carried a(x_k) differs from it by an ulp, which moves float64 truth values.
            ak = (-mp.mpf(float(s.Ahat[k, 2])) - dak * 3 * tk) / 3
        for p in range(M):
            A[k, p] = scl * scl * (-ak * D2[p] - dak * D1[p] + ck * L[p])
    # the reference evaluates u(xmin), u(xmax) through the same float64 mapdomain
    ta = mp.mpf(float(np.float64(s.off) + np.float64(s.scl) * np.float64(s.a)))
    tb = mp.mpf(float(np.float64(s.off) + np.float64(s.scl) * np.float64(s.b)))
    La, _, _ = _legendre_tables_mp(ta, M)
    Lb, _, _ = _legendre_tables_mp(tb, M)
    K = mp.zeros(M + 2, M + 2)
    AtA = A.T * A
    for i in range(M):
        for j in range(M):
            K[i, j] = gam * AtA[i, j] + (1 if i == j else 0)
        K[i, M] = K[M, i] = La[i]
        K[i, M + 1] = K[M + 1, i] = Lb[i]
    Atf = A.T * mp.matrix([mp.mpf(float(v)) for v in s.f])
    rhs = mp.matrix(M + 2, 1)
    for i in range(M):
        rhs[i] = gam * Atf[i]
    rhs[M] = mp.mpf(float(s.g[0]))
    rhs[M + 1] = mp.mpf(float(s.g[1]))
    sol = mp.lu_solve(K, rhs)
    return np.array([float(sol[i]) for i in range(M)])


def truth_all(nodes, values, M, gamma, n, rhs, global_domain=None, elements=None, dps=60,
              coef_a=None, coef_da=None, bc_left=0.0, bc_right=0.0, coef_c=None):
    """Truth coefficients for ``elements`` (default all) of a mesh."""
    from . import lssvr_oracle as orc
    return np.array([solve_truth(s, dps) for s in orc.mesh_element_systems(
        nodes, values, M, gamma, n, rhs, global_domain, elements, coef_a, coef_da, coef_c, bc_left, bc_right)])
