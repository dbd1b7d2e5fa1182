"""numpy statement of DESIGN.md section 25: block inverse iteration with a fixed shift and a Rayleigh-Ritz step for the
k eigenvalues nearest sigma of  -(a u')' + c u = lambda rho u  on a P1 mesh, the Sturm count that certifies them, and
the Rayleigh quotient of the enhanced modes.  The shifted systems go through scipy.linalg.solve_banded (LAPACK's
pivoting banded LU); everything else is numpy.  The device kernels (csrc/eigen.hip) and the facade's solve_eigen
follow this text step by step; tests/eigen_rules.py imports it.

Run as a script it prints, for -u'' = lambda u on (-1, 1) with Dirichlet ends, the P1 and the enhanced eigenvalue
errors at ne = 8, 16, 32 (M = 9), the improvement factors DESIGN.md quotes."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import lssvr_oracle as orc                     # noqa: E402

DIRICHLET, ROBIN = 0, 1
MAX_BLOCK = 8
EPS = 2.0 ** -53


def _zero(x):
    return np.zeros_like(np.asarray(x, dtype=np.float64))


def _one(x):
    return np.ones_like(np.asarray(x, dtype=np.float64))


def pencil(nodes, a=None, c=None, rho=None, nquad=2):
    """(kdiag[ne+1], koff[ne], mdiag[ne+1], moff[ne]): K the P1 bands of -(a u')' + c u, M the consistent mass bands
    weighted by rho -- the reaction assembly with a = 0 and c = rho."""
    nodes = np.asarray(nodes, dtype=np.float64)
    kd, ko = orc.p1_bands(nodes, _zero, a, nquad, _zero if c is None else c)[:2]
    md, mo = orc.p1_bands(nodes, _zero, _zero, nquad, _one if rho is None else rho)[:2]
    return kd, ko, md, mo


def unknowns(ne, kinds):
    """(sh, hi): the unknowns are the nodes sh .. hi-1 (a Dirichlet end is no unknown)."""
    return (0 if kinds[0] == ROBIN else 1), (ne + 1 if kinds[1] == ROBIN else ne)


def reduced(bands, kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0)):
    """(alpha[m], beta[m-1], mu[m], nu[m-1]): the diagonals and off-diagonals of K (kappa on its end diagonal) and M
    over the unknowns."""
    kd, ko, md, mo = (np.asarray(t, dtype=np.float64) for t in bands)
    sh, hi = unknowns(len(ko), kinds)
    al = kd[sh:hi].copy()
    if kinds[0] == ROBIN:
        al[0] += kappa[0]
    if kinds[1] == ROBIN:
        al[-1] += kappa[1]
    return al, ko[sh:hi - 1].copy(), md[sh:hi].copy(), mo[sh:hi - 1].copy()


def dense(bands, kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0)):
    al, be, mu, nu = reduced(bands, kinds, kappa)
    return (np.diag(al) + np.diag(be, 1) + np.diag(be, -1)), (np.diag(mu) + np.diag(nu, 1) + np.diag(nu, -1))


def tri_apply(d, o, Z):
    """(tridiag(o, d, o) Z^T)^T for Z [nb, m]."""
    out = d[None, :] * Z
    out[:, :-1] += o[None, :] * Z[:, 1:]
    out[:, 1:] += o[None, :] * Z[:, :-1]
    return out


def shifted_solve(al, be, mu, nu, sigma, Y):
    """Z [nb, m] with (K - sigma M) Z^T = Y^T, by LAPACK's banded LU with partial pivoting."""
    from scipy.linalg import solve_banded
    m = len(al)
    ab = np.zeros((3, m))
    ab[1] = al - sigma * mu
    ab[0, 1:] = be - sigma * nu
    ab[2, :-1] = be - sigma * nu
    return solve_banded((1, 1), ab, Y.T).T


def ritz(A, B, sigma):
    """(theta[nb] ascending in |theta - sigma|, Q[nb, nb], info): Q^T A Q = diag theta, Q^T B Q = I.  info counts the
    dependent columns of B; LAPACK raises for those, so here it is 0 or an exception."""
    from scipy.linalg import eigh
    th, Q = eigh(0.5 * (A + A.T), 0.5 * (B + B.T))
    order = np.argsort(np.abs(th - sigma), kind="stable")
    return th[order], Q[:, order], 0


def sturm_count(al, be, mu, nu, s, pivmin=None):
    """The number of negative pivots of LDL^T (K - s M): d_i = alpha_i - beta_{i-1}^2 / d_{i-1}, a pivot with
    |d| < pivmin taken as -pivmin (LAPACK dstebz).  By Sylvester's law the number of eigenvalues below s."""
    a = al - s * mu
    b = be - s * nu
    if pivmin is None:
        pivmin = np.finfo(np.float64).tiny * max(1.0, float(np.max(b * b)) if b.size else 1.0)
    cnt, d = 0, 1.0
    for i in range(len(a)):
        d = a[i] - (b[i - 1] * b[i - 1] / d if i else 0.0)
        if abs(d) < pivmin:
            d = -pivmin
        cnt += d < 0.0
    return int(cnt)


def solve(bands, kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), k=1, sigma=0.0, tol=1e-12, max_iter=200,
          check_every=4, solve_fn=shifted_solve, ritz_fn=ritz, count_fn=sturm_count):
    """Block inverse iteration.  Returns dict(theta[k], X[k, ne+1], residuals[k], index[k], iterations, converged,
    counts): theta in the order of |theta - sigma|, X M-orthonormal with a positive value at the first unknown, index
    the position of each value in the ascending spectrum, from 0: the number of eigenvalues below it."""
    al, be, mu, nu = reduced(bands, kinds, kappa)
    ne = len(bands[1])
    sh, hi = unknowns(ne, kinds)
    m = hi - sh
    if not 1 <= k <= 6 or k > m:
        raise ValueError(f"k = {k} must lie in 1 .. min(6, {m})")
    nb = min(MAX_BLOCK, k + 2, m)
    kmax = max(float(np.max(np.abs(al))), float(np.max(np.abs(be))) if m > 1 else 0.0)
    row = mu.copy()
    row[1:] -= np.abs(nu)
    row[:-1] -= np.abs(nu)
    mmin = float(row.min())
    Y = np.random.default_rng(0).standard_normal((nb, m))
    it, converged = 0, False
    while it < max_iter and not converged:
        it += 1
        Z = solve_fn(al, be, mu, nu, sigma, Y)
        MZ, KZ = tri_apply(mu, nu, Z), tri_apply(al, be, Z)
        A, B = Z @ KZ.T, Z @ MZ.T
        theta, Q, info = ritz_fn(A, B, sigma)
        if info:
            raise RuntimeError(f"{info} dependent column(s) in the block")
        X, Y, R = Q.T @ Z, Q.T @ MZ, Q.T @ KZ
        sign = np.where(X[:, 0] < 0.0, -1.0, 1.0)
        X, Y, R = sign[:, None] * X, sign[:, None] * Y, sign[:, None] * R
        if it % check_every and it != max_iter:
            continue
        res = np.sqrt(np.sum((R - theta[:, None] * Y) ** 2, axis=1))
        xn = np.sqrt(np.sum(X * X, axis=1))
        converged = bool(np.all(res[:k] <= tol * kmax * xn[:k]))
    index, counts = None, None
    if converged:
        floor = 64.0 * EPS * kmax / mmin
        order = np.argsort(theta[:k], kind="stable")
        t_lo, t_hi = theta[order[0]], theta[order[-1]]
        below = [t for t in theta[k:] if t < t_lo]
        above = [t for t in theta[k:] if t > t_hi]
        d_lo = max(0.5 * (t_lo - max(below)) if below else 0.0, res[order[0]] / math.sqrt(mmin), floor)
        d_hi = max(0.5 * (min(above) - t_hi) if above else 0.0, res[order[-1]] / math.sqrt(mmin), floor)
        counts = (count_fn(al, be, mu, nu, t_lo - d_lo), count_fn(al, be, mu, nu, t_hi + d_hi))
        if counts[1] - counts[0] != k:
            raise RuntimeError(f"found {k} value(s) in [{t_lo}, {t_hi}], the Sturm counts {counts} say "
                               f"{counts[1] - counts[0]}")
        index = np.empty(k, dtype=np.int64)
        index[order] = counts[0] + np.arange(k)
    full = np.zeros((k, ne + 1))
    full[:, sh:hi] = X[:k]
    return dict(theta=theta[:k].copy(), X=full, residuals=res[:k].copy(), index=index, iterations=it,
                converged=converged, counts=counts)


def rayleigh(nodes, W, nq, a=None, c=None, rho=None, kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0)):
    """(numerator, denominator, sum |terms| of the numerator) of the Rayleigh quotient of the piecewise Legendre
    function W[ne, M] by nq-point Gauss: int (a u'^2 + c u^2) + kappa u(x_end)^2 at the Robin ends, over int rho u^2."""
    nodes = np.asarray(nodes, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    xi, wt = np.polynomial.legendre.leggauss(nq)
    h = np.diff(nodes)
    xq = 0.5 * (nodes[:-1] + nodes[1:])[:, None] + 0.5 * h[:, None] * xi[None, :]
    V = np.polynomial.legendre.legvander(xi, W.shape[1] - 1)                     # [nq, M]
    D = np.stack([np.polynomial.legendre.legval(xi, np.polynomial.legendre.legder(np.eye(W.shape[1])[p]))
                  if p else np.zeros_like(xi) for p in range(W.shape[1])], axis=1)
    u = W @ V.T
    du = (W @ D.T) * (2.0 / h)[:, None]
    aq = np.broadcast_to((_one if a is None else a)(xq), xq.shape)
    cq = np.broadcast_to((_zero if c is None else c)(xq), xq.shape)
    rq = np.broadcast_to((_one if rho is None else rho)(xq), xq.shape)
    half = 0.5 * h
    ta, tc = aq * du * du, cq * u * u
    num = float(np.sum(half * ((ta + tc) @ wt)))
    mag = float(np.sum(half * ((np.abs(ta) + np.abs(tc)) @ wt)))
    den = float(np.sum(half * ((rq * u * u) @ wt)))
    ends = (float(np.sum(W[0] * (-1.0) ** np.arange(W.shape[1]))), float(np.sum(W[-1])))
    for i in range(2):
        if kinds[i] == ROBIN:
            num += kappa[i] * ends[i] ** 2
            mag += abs(kappa[i]) * ends[i] ** 2
    return num, den, mag


def enhanced_value(nodes, u, theta, M, gamma, n_colloc, a=None, da=None, c=None, rho=None, nq=None):
    """The Rayleigh quotient of the mode (u, theta) after the oracle's reaction-row enhancement: the source problem
    -(a u')' + (c - theta rho) u = 0 with the mode's nodal values, zero right-hand side and zero Dirichlet data."""
    cfun = _zero if c is None else c
    rfun = _one if rho is None else rho
    W = orc.enhance_all_vec(nodes, u, M, gamma, n_colloc, rhs=_zero, coef_a=_one if a is None else a,
                            coef_da=_zero if da is None else da, coef_c=lambda x: cfun(x) - theta * rfun(x))
    num, den, _ = rayleigh(nodes, W, max(M, 8) if nq is None else nq, a, c, rho)
    return num / den, W


def improvement_table(sizes=(8, 16, 32), M=9, gamma=1e4, n_colloc=16, modes=(1, 2)):
    """[(ne, j, |P1 - exact|, |enhanced - exact|)] for -u'' = lambda u on (-1, 1), Dirichlet: lambda_j = (j pi / 2)^2."""
    rows = []
    for ne in sizes:
        nodes = np.linspace(-1.0, 1.0, ne + 1)
        r = solve(pencil(nodes), k=max(modes), sigma=0.0)
        order = np.argsort(r["theta"])
        for j in modes:
            col = order[j - 1]
            exact = (j * math.pi / 2.0) ** 2
            val, _ = enhanced_value(nodes, r["X"][col], r["theta"][col], M, gamma, n_colloc)
            rows.append((ne, j, abs(r["theta"][col] - exact), abs(val - exact)))
    return rows


if __name__ == "__main__":
    for ne, j, e_fem, e_enh in improvement_table():
        print(f"ne = {ne:3d}  mode {j}:  |P1 - exact| = {e_fem:.3e}   |enhanced - exact| = {e_enh:.3e}   "
              f"factor {e_fem / e_enh:.1f}")
