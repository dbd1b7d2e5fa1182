"""numpy restatement of the periodic boundary condition (include/lssvr_hip.h: lssvr_tridiag_periodic_solve_multi,
lssvr_tridiag_ns_periodic_solve_multi, lssvr_estimate_seam) on top of oracle/lssvr_oracle.py and
tests/convection_rules.py, with the same Gauss rule, and the problems the tests share.  A plain module: the CPU tests
pin it to manufactured solutions, the GPU tests compare the kernels with it, scripts/proto/periodic_proto.py runs the
adaptive loop on it.

Node ne is node 0: u(x_0) = u(x_ne) = s, and the two half rows of the open bands -- row 0 (diag[0], sup[0], load[0])
and row ne (sub[ne-1], diag[ne], load[ne]) -- add up to the seam row
    (diag[0] + diag[ne]) s + sup[0] u_1 + sub[ne-1] u_{ne-1} = load[0] + load[ne].
The ne unknowns are s = u_0 and u_1 .. u_{ne-1}; every solve here returns u[ne+1] with u[ne] = u[0]."""
import functools
import math

import numpy as np

import convection_rules as cr


# --------------------------------------------------------------------------
# the cyclic system
# --------------------------------------------------------------------------
def cyclic_bands(diag, sub, sup, load, dtype=np.float64):
    """(D, L, U, R), each [ne]: row i is L[i] u[i-1] + D[i] u[i] + U[i] u[i+1] = R[i] with the indices mod ne."""
    diag, sub, sup, load = (np.asarray(t, dtype=dtype) for t in (diag, sub, sup, load))
    D = diag[:-1].copy()
    D[0] = diag[0] + diag[-1]
    R = load[:-1].copy()
    R[0] = load[0] + load[-1]
    return D, np.roll(sub, 1), sup.copy(), R


def dense_system(diag, sub, sup, load):
    """(A[ne, ne], rhs[ne]) of the cyclic system; with two elements both couplings of a row meet in one entry."""
    D, L, U, R = cyclic_bands(diag, sub, sup, load)
    n = len(D)
    A = np.diag(D)
    for i in range(n):
        A[i, (i - 1) % n] += L[i]
        A[i, (i + 1) % n] += U[i]
    return A, R


def _closed(u):
    return np.concatenate([u, u[:1]])


def dense_solve(diag, sub, sup, load):
    """``numpy.linalg.solve`` (LAPACK, partial pivoting) on :func:`dense_system` -> u[ne+1]."""
    return _closed(np.linalg.solve(*dense_system(diag, sub, sup, load)))


def banded_solve(diag, sub, sup, load):
    """The same system by LAPACK's banded LU (partial pivoting) and the Sherman-Morrison formula for the two corner
    entries: the pivoted comparison at sizes a dense matrix does not fit.  Two elements: the dense solve."""
    from scipy.linalg import solve_banded
    D, L, U, R = cyclic_bands(diag, sub, sup, load)
    n = len(D)
    if n < 3:
        return dense_solve(diag, sub, sup, load)
    beta, alpha = L[0], U[-1]               # A[0, n-1] and A[n-1, 0]
    gamma = -D[0]
    ab = np.zeros((3, n))
    ab[1] = D
    ab[1, 0] -= gamma
    ab[1, -1] -= alpha * beta / gamma
    ab[0, 1:] = U[:-1]
    ab[2, :-1] = L[1:]
    w = np.zeros(n)
    w[0], w[-1] = gamma, alpha
    y, q = solve_banded((1, 1), ab, np.stack([R, w], axis=1)).T
    fact = (y[0] + beta * y[-1] / gamma) / (1.0 + q[0] + beta * q[-1] / gamma)
    return _closed(y - fact * q)


def thomas_cyclic_ld(diag, sub, sup, load):
    """The same system in long double without pivoting: the seam eliminated -- u_int = y + s z, y the Dirichlet
    solve with end values (0, 0), z the one with zero load and end values (1, 1), s from the seam row -- then Thomas
    for y and z (``convection_rules.thomas_ns_ld``).  The forward reference of the device solve; long double."""
    ld = np.longdouble
    diag, sub, sup, load = (np.asarray(t, dtype=ld) for t in (diag, sub, sup, load))
    y = cr.thomas_ns_ld(diag, sub, sup, load, 0.0, 0.0)
    z = cr.thomas_ns_ld(diag, sub, sup, np.zeros_like(load), 1.0, 1.0)
    s = ((load[0] + load[-1] - sup[0] * y[1] - sub[-1] * y[-2])
         / (diag[0] + diag[-1] + sup[0] * z[1] + sub[-1] * z[-2]))
    u = y + s * z
    u[0] = u[-1] = s
    return u


def residual(diag, sub, sup, load, u):
    """Residual [ne] of the cyclic system for u[ne+1] (u[ne] is not read)."""
    D, L, U, R = cyclic_bands(diag, sub, sup, load)
    v = np.asarray(u, dtype=np.float64)[:-1]
    return L * np.roll(v, 1) + D * v + U * np.roll(v, -1) - R


def roll_bands(diag, sub, sup, load, k):
    """The open bands of the same cyclic system with the seam moved to node k (0 < k < ne): new node j is old node
    (j + k) mod ne.  The old seam rows are merged into one interior row, the row of old node k is split in two halves
    (x/2 + x/2 == x in floating point, so the cyclic system is the old one, bit for bit, up to the merge's one
    rounding).  u_new[j] = u_old[(j + k) mod ne]."""
    D, L, U, R = cyclic_bands(diag, sub, sup, load)
    D, R = np.roll(D, -k), np.roll(R, -k)
    nd = np.concatenate([D, [0.5 * D[0]]])
    nd[0] = 0.5 * D[0]
    nl = np.concatenate([R, [0.5 * R[0]]])
    nl[0] = 0.5 * R[0]
    return nd, np.roll(np.asarray(sub, dtype=np.float64), -k), np.roll(np.asarray(sup, dtype=np.float64), -k), nl


def roll_solution(u, k):
    return _closed(np.roll(np.asarray(u)[:-1], -k))


def fem_solve_periodic(nodes, f, a=None, b=None, c=None, nquad=2):
    """Nodal values u[ne+1] (u[ne] == u[0]) of the periodic P1 solve of -(a u')' + b u' + c u = f: the bands of
    ``convection_rules.conv_bands`` (the quadrature of the assembly kernels) through :func:`dense_solve`."""
    diag, sub, sup, load, _ = cr.conv_bands(nodes, f, a, b, c, nquad)
    return dense_solve(diag, sub, sup, load)


# --------------------------------------------------------------------------
# the bands the solve tests share: -u'' + b u' + u = pi^2 sin(pi x) on a uniform mesh of (-1, 1)
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solve_case(ne, convection):
    """(bands, u_ld, u_lapack).  ``convection``: b = amp sin(pi x), periodic, with cell Peclet numbers up to 0.5; else
    no b (sub == sup).  Computed once per case and shared: do not write to the arrays."""
    from oracle import lssvr_oracle as orc
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    c = lambda x: 1.0 + 0.0 * x                                       # noqa: E731
    b = None
    if convection:
        amp = 0.5 * ne                    # |b| <= amp and h = 2 / ne: cell Peclet |bbar| h / 2 <= 0.5
        b = lambda x: amp * np.sin(np.pi * np.asarray(x, dtype=np.float64))           # noqa: E731
    bands = cr.conv_bands(nodes, orc.poisson_rhs, None, b, c)[:4]
    return bands, thomas_cyclic_ld(*bands), banded_solve(*bands)


@functools.lru_cache(maxsize=None)
def dirichlet_lapack_distance(ne, convection):
    """max |LAPACK - long double| of the Dirichlet/Dirichlet solve on the bands of :func:`solve_case`, relative to
    max |u|: what the bars of the Dirichlet entries were set beside."""
    bands = solve_case(ne, convection)[0]
    u_ld = cr.thomas_ns_ld(*bands, 0.25, -0.5)
    u_la = cr.banded_ns(*bands, 0.25, -0.5)
    return float(np.max(np.abs(u_la.astype(np.longdouble) - u_ld)) / np.max(np.abs(u_ld)))


# --------------------------------------------------------------------------
# the seam term of the indicator
# --------------------------------------------------------------------------
def seam_jump(x, W, a_seam):
    """J = a_seam[0] u_{ne-1}'(x_ne) - a_seam[1] u_0'(x_0) from the Legendre rows of the last and the first element:
    the flux jump across the seam, a_seam = (a at x_ne seen from element ne-1, a at x_0 seen from element 0).
    P_k'(+-1) = (+-1)^(k+1) k(k+1)/2."""
    M = W.shape[1]
    k = np.arange(M, dtype=np.float64)
    w = k * (k + 1) / 2
    dr = math.fsum(W[-1] * w) * (2.0 / (x[-1] - x[-2]))
    dl = math.fsum(W[0] * w * (-1.0) ** (k + 1)) * (2.0 / (x[1] - x[0]))
    return a_seam[0] * dr - a_seam[1] * dl


def estimate_seam(x, W, a_seam, eta2, out3):
    """(eta2, out3) after the seam term: eta2[ne-1] += h_{ne-1}/2 J^2, then eta2[0] += h_0/2 J^2; out3 = {sum + the
    added terms, max with the new values, non-finite count + 1 for a value that stops being finite}.  The inputs are
    not written."""
    eta2 = np.array(eta2, dtype=np.float64)
    s, mx, cnt = (float(v) for v in out3)
    J = seam_jump(x, W, a_seam)
    for e in (len(x) - 2, 0):
        add = 0.5 * (x[e + 1] - x[e]) * J * J
        old = eta2[e]
        eta2[e] = old + add
        if np.isfinite(old):
            if np.isfinite(eta2[e]):
                s, mx = s + add, max(mx, eta2[e])
            else:
                cnt += 1.0
    return eta2, np.array([s, mx, cnt])


# --------------------------------------------------------------------------
# manufactured problems on (-1, 1), period 2 (each: f, a, da, b, c, exact u)
# --------------------------------------------------------------------------
def _arr(x):
    return np.asarray(x, dtype=np.float64)


def _one(x):
    return 1.0 + 0.0 * _arr(x)


PI = math.pi


def man_u(x):
    x = _arr(x)
    return np.sin(PI * x) + 0.3 * np.cos(2 * PI * x)


def man_du(x):
    x = _arr(x)
    return PI * np.cos(PI * x) - 0.6 * PI * np.sin(2 * PI * x)


def man_d2u(x):
    x = _arr(x)
    return -PI ** 2 * np.sin(PI * x) - 1.2 * PI ** 2 * np.cos(2 * PI * x)


# 1. -u'' + u = f
def const_f(x):
    return -man_d2u(x) + man_u(x)


# 2. -(a u')' + b u' + c u = f with a = 2 + sin(pi x), b = sin(pi x) / 2, c = 1 + cos(pi x) / 2
def var_a(x):
    return 2.0 + np.sin(PI * _arr(x))


def var_da(x):
    return PI * np.cos(PI * _arr(x))


def var_b(x):
    return 0.5 * np.sin(PI * _arr(x))


def var_c(x):
    return 1.0 + 0.5 * np.cos(PI * _arr(x))


def var_f(x):
    return -var_a(x) * man_d2u(x) + (var_b(x) - var_da(x)) * man_du(x) + var_c(x) * man_u(x)


PROBLEMS = {
    "const": dict(f=const_f, a=None, da=None, b=None, c=_one, u=man_u),
    "var": dict(f=var_f, a=var_a, da=var_da, b=var_b, c=var_c, u=man_u),
}


def problem_nodal_error(name, ne, nquad=3):
    """max |u_h - u| at the nodes of a uniform mesh of (-1, 1) with ``ne`` elements."""
    p = PROBLEMS[name]
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    u = fem_solve_periodic(nodes, p["f"], p["a"], p["b"], p["c"], nquad)
    return float(np.max(np.abs(u - p["u"](nodes))))


# 3. the adaptive problem: -u'' + u = f with u = exp(-(1 + cos(pi x)) / 0.05), a peak of width ~0.1 on the seam
PEAK_W = 0.05


def peak_u(x):
    return np.exp(-(1.0 + np.cos(PI * _arr(x))) / PEAK_W)


def peak_f(x):
    x = _arr(x)
    g1 = (PI / PEAK_W) * np.sin(PI * x)               # (log u)'
    g2 = (PI ** 2 / PEAK_W) * np.cos(PI * x)          # (log u)''
    u = peak_u(x)
    return -(g2 + g1 * g1) * u + u
