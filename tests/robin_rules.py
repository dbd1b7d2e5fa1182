"""numpy restatement of the Neumann / Robin boundary conditions (include/lssvr_hip.h: lssvr_tridiag_bc_solve_multi,
lssvr_tridiag_ns_bc_solve_multi, lssvr_estimate_ends) on top of oracle/lssvr_oracle.py and tests/convection_rules.py,
with the same Gauss rule, and the problems the tests share.  A plain module: the CPU tests pin it to manufactured
solutions, the GPU tests compare the kernels with it.

At each end, Dirichlet (u = g, kind 0) or Robin (a du/dn + kappa u = g with the outward normal, kind 1; Neumann is
kappa = 0).  A Robin end adds kappa to the end diagonal and g to the end load and keeps the end row; a Dirichlet end
replaces the row by u = g."""
import functools
import math

import numpy as np

import convection_rules as cr

DIRICHLET, ROBIN = 0, 1
KIND_PAIRS = [(DIRICHLET, DIRICHLET), (DIRICHLET, ROBIN), (ROBIN, DIRICHLET), (ROBIN, ROBIN)]


# --------------------------------------------------------------------------
# the P1 system with Robin ends
# --------------------------------------------------------------------------
def dense_system(diag, sub, sup, load, kinds, kappa, values):
    """(A[ne+1, ne+1], rhs[ne+1]) of the bands with the end conditions applied: a Robin end row keeps its band
    entries, gains kappa on the diagonal and g on the right-hand side; a Dirichlet end row becomes u = g."""
    n = len(diag)
    A = np.diag(np.asarray(diag, dtype=np.float64)) + np.diag(sub, -1) + np.diag(sup, 1)
    r = np.array(load, dtype=np.float64)
    for i, end in ((0, 0), (1, n - 1)):
        if kinds[i] == ROBIN:
            A[end, end] += kappa[i]
            r[end] += values[i]
        else:
            A[end] = 0.0
            A[end, end] = 1.0
            r[end] = values[i]
    return A, r


def dense_solve(diag, sub, sup, load, kinds, kappa, values):
    """``numpy.linalg.solve`` on :func:`dense_system`; a Dirichlet end comes back as its value exactly."""
    u = np.linalg.solve(*dense_system(diag, sub, sup, load, kinds, kappa, values))
    for i, end in ((0, 0), (1, -1)):
        if kinds[i] == DIRICHLET:
            u[end] = values[i]
    return u


def unknown_rows(diag, sub, sup, load, kinds, kappa, values, dtype=np.float64):
    """(d, lo, up, r, first) of the rows that stay unknown -- node ``first`` onwards, a Dirichlet end eliminated into
    its neighbour's right-hand side: lo[k] couples unknown k+1 to k, up[k] unknown k to k+1."""
    n = len(diag)
    d = np.array(diag, dtype=dtype)
    r = np.array(load, dtype=dtype)
    first, last = 0, n - 1
    if kinds[0] == ROBIN:
        d[0] += kappa[0]
        r[0] += values[0]
    else:
        first = 1
        if n > 2 or kinds[1] == ROBIN:
            r[1] -= sub[0] * values[0]
    if kinds[1] == ROBIN:
        d[-1] += kappa[1]
        r[-1] += values[1]
    else:
        last = n - 2
        if last >= first:
            r[last] -= sup[-1] * values[1]
    return d[first:last + 1], np.asarray(sub)[first:last], np.asarray(sup)[first:last], r[first:last + 1], first


def _assemble(x, kinds, values, first, n):
    u = np.zeros(n, dtype=x.dtype)
    u[first:first + len(x)] = x
    if kinds[0] == DIRICHLET:
        u[0] = values[0]
    if kinds[1] == DIRICHLET:
        u[-1] = values[1]
    return u


def banded_solve(diag, sub, sup, load, kinds, kappa, values):
    """The same system by LAPACK's banded LU (partial pivoting): the reference at sizes a dense matrix does not fit."""
    from scipy.linalg import solve_banded
    d, lo, up, r, first = unknown_rows(diag, sub, sup, load, kinds, kappa, values)
    x = np.zeros(0)
    if len(d):
        ab = np.zeros((3, len(d)))
        ab[1] = d
        ab[0, 1:] = up
        ab[2, :-1] = lo
        x = solve_banded((1, 1), ab, r)
    return _assemble(x, kinds, values, first, len(diag))


def thomas_ld(diag, sub, sup, load, kinds, kappa, values):
    """The same system by Thomas elimination in long double (no pivoting): the forward reference of the device solve,
    as ``convection_rules.thomas_ns_ld`` is for the Dirichlet entries.  Returned as long double."""
    ld = np.longdouble
    bands = [np.asarray(t, dtype=ld) for t in (diag, sub, sup, load)]
    d, lo, up, r, first = unknown_rows(*bands, kinds, [ld(k) for k in kappa], [ld(v) for v in values], dtype=ld)
    m = len(d)
    x = np.zeros(m, dtype=ld)
    if m:
        for i in range(1, m):
            w = lo[i - 1] / d[i - 1]
            d[i] -= w * up[i - 1]
            r[i] -= w * r[i - 1]
        x[-1] = r[-1] / d[-1]
        for i in range(m - 2, -1, -1):
            x[i] = (r[i] - up[i] * x[i + 1]) / d[i]
    return _assemble(x, kinds, [ld(v) for v in values], first, len(diag))


def fem_solve(nodes, f, kinds, kappa, values, a=None, b=None, c=None, nquad=2):
    """Nodal values of the P1 solve of -(a u')' + b u' + c u = f with the end conditions: the bands of
    ``convection_rules.conv_bands`` (the quadrature of the assembly kernels) through :func:`dense_solve`."""
    diag, sub, sup, load, _ = cr.conv_bands(nodes, f, a, b, c, nquad)
    return dense_solve(diag, sub, sup, load, kinds, kappa, values)


# --------------------------------------------------------------------------
# the bands the solve tests share: -u'' + b u' + u = pi^2 sin(pi x) on a uniform mesh of (-1, 1)
# --------------------------------------------------------------------------
SOLVE_KAPPA = (0.0, 2.0)          # a Neumann end on the left, a Robin end on the right (where the end is Robin)
SOLVE_VALUES = (0.25, -0.5)


@functools.lru_cache(maxsize=None)
def solve_case(ne, kinds, convection):
    """(bands, u_ld, u_lapack) for the end ``kinds`` with SOLVE_KAPPA and SOLVE_VALUES.  ``convection``: b = amp x
    with cell Peclet numbers up to 0.5 -- outflow at both ends, so kappa + b n / 2 >= 0 holds with kappa = 0 --
    else no b (sub == sup).  c = 1 keeps two Neumann ends regular.  Computed once per case and shared: do not write
    to the arrays."""
    from oracle import lssvr_oracle as orc
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    c = lambda x: 1.0 + 0.0 * x                                       # noqa: E731
    b = None
    if convection:
        amp = 0.5 * ne                    # |b| <= amp and h = 2 / ne: cell Peclet |bbar| h / 2 <= 0.5
        b = lambda x: amp * np.asarray(x, dtype=np.float64)           # noqa: E731
    bands = cr.conv_bands(nodes, orc.poisson_rhs, None, b, c)[:4]
    u_ld = thomas_ld(*bands, kinds, SOLVE_KAPPA, SOLVE_VALUES)
    u_la = banded_solve(*bands, kinds, SOLVE_KAPPA, SOLVE_VALUES)
    return bands, u_ld, u_la


# --------------------------------------------------------------------------
# boundary term of the indicator
# --------------------------------------------------------------------------
def end_residuals(x, W, kinds, kappa, g, a_ends):
    """(J_left, J_right): J = g - kappa u_e(x_end) - a du_e/dn from the end element's Legendre row, du/dn = -u' at the
    left end and +u' at the right one; 0 at a Dirichlet end.  P_k(+-1) = (+-1)^k, P_k'(+-1) = (+-1)^(k+1) k(k+1)/2."""
    M = W.shape[1]
    k = np.arange(M, dtype=np.float64)
    w = k * (k + 1) / 2
    J = [0.0, 0.0]
    for i, (e, sign) in enumerate(((0, -1.0), (len(x) - 2, 1.0))):
        if kinds[i] != ROBIN:
            continue
        scl = 2.0 / (x[e + 1] - x[e])
        val = math.fsum(W[e] * sign ** k)
        der = math.fsum(W[e] * w * sign ** (k + 1)) * scl
        J[i] = g[i] - kappa[i] * val - a_ends[i] * (sign * der)
    return tuple(J)


def estimate_ends(x, W, kinds, kappa, g, a_ends, eta2, out3):
    """(eta2, out3) after the boundary term: eta2[end element] += h/2 J^2; out3 = {sum + the added terms, max with the
    new values, non-finite count + 1 for a value that stops being finite}.  The inputs are not written."""
    eta2 = np.array(eta2, dtype=np.float64)
    s, mx, cnt = (float(v) for v in out3)
    for i, (e, J) in enumerate(zip((0, len(x) - 2), end_residuals(x, W, kinds, kappa, g, a_ends))):
        if kinds[i] != ROBIN:
            continue
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
# manufactured problems (each: f, a, da, b, c, boundary of the facade, exact u, domain)
# --------------------------------------------------------------------------
def _arr(x):
    return np.asarray(x, dtype=np.float64)


def _one(x):
    return 1.0 + 0.0 * _arr(x)


# 1. u = cos(pi x) on (-1, 1), -u'' + u = f, Neumann g = 0 at both ends (u'(+-1) = 0)
def cos_u(x):
    return np.cos(np.pi * _arr(x))


def cos_f(x):
    return (np.pi ** 2 + 1.0) * np.cos(np.pi * _arr(x))


# 2. u = e^x on (-1, 1), -(a u')' = f with a = 1 + x^2/2, Dirichlet left, Robin kappa = 2 right:
#    g = a(1) u'(1) + 2 u(1) = 3.5 e
def exp_u(x):
    return np.exp(_arr(x))


def exp_a(x):
    return 1.0 + 0.5 * _arr(x) ** 2


def exp_da(x):
    return _arr(x)


def exp_f(x):
    x = _arr(x)
    return -(x + exp_a(x)) * np.exp(x)


EXP_KAPPA = 2.0
EXP_G = 3.5 * math.e


# 3. convection with an outflow Neumann end: -u'' + b u' + u = f on (-1, 1), b = 2, u = sin(pi x / 2) + x/2:
#    Dirichlet at the inflow end x = -1, Neumann at the outflow end x = 1, g = u'(1) = 1/2
OUT_B = 2.0


def out_u(x):
    x = _arr(x)
    return np.sin(0.5 * np.pi * x) + 0.5 * x


def out_b(x):
    return OUT_B + 0.0 * _arr(x)


def out_f(x):
    x = _arr(x)
    s, co = np.sin(0.5 * np.pi * x), np.cos(0.5 * np.pi * x)
    return (0.25 * np.pi ** 2) * s + OUT_B * (0.5 * np.pi * co + 0.5) + s + 0.5 * x


PROBLEMS = {
    "cos": dict(f=cos_f, a=None, da=None, b=None, c=_one, u=cos_u, kinds=(ROBIN, ROBIN), kappa=(0.0, 0.0),
                values=(0.0, 0.0), boundary=(("neumann", 0.0), ("neumann", 0.0))),
    "exp": dict(f=exp_f, a=exp_a, da=exp_da, b=None, c=None, u=exp_u, kinds=(DIRICHLET, ROBIN),
                kappa=(0.0, EXP_KAPPA), values=(math.exp(-1.0), EXP_G),
                boundary=(("dirichlet", math.exp(-1.0)), ("robin", EXP_KAPPA, EXP_G))),
    "outflow": dict(f=out_f, a=None, da=None, b=out_b, c=_one, u=out_u, kinds=(DIRICHLET, ROBIN), kappa=(0.0, 0.0),
                    values=(-1.5, 0.5), boundary=(("dirichlet", -1.5), ("neumann", 0.5))),
}


def problem_nodal_error(name, ne, nquad=3):
    """max |u_h - u| at the nodes of a uniform mesh of (-1, 1) with ``ne`` elements."""
    p = PROBLEMS[name]
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    u = fem_solve(nodes, p["f"], p["kinds"], p["kappa"], p["values"], p["a"], p["b"], p["c"], nquad)
    return float(np.max(np.abs(u - p["u"](nodes))))
