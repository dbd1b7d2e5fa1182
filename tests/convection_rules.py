"""numpy restatement of the convection term's P1 half (include/lssvr_hip.h: lssvr_p1_assemble_conv,
lssvr_tridiag_ns_dirichlet_solve) on top of oracle/lssvr_oracle.py, with the same Gauss rule, and the two problems the
tests share.  A plain module: the CPU tests pin it to a manufactured solution, the GPU tests compare the kernels with
it, scripts/proto/conv_adapt.py runs the adaptive loop on it.

The enhancement and indicator rows need no restatement of their own: -(a u')' + b u' = -a u'' - (a' - b) u', so the
oracle's ``coef_da`` / ``da`` argument takes a' - b."""
import functools
import math

import numpy as np

from oracle import lssvr_oracle as orc


# --------------------------------------------------------------------------
# bands of -(a u')' + b u' + c u = f
# --------------------------------------------------------------------------
def conv_halves(nodes, b, nquad=2):
    """(beta0[ne], beta1[ne]): beta_i = sum_q w_q b(x_q) phi_i(xi_q), phi_0 = 1 - xi, phi_1 = xi; the element matrix
    of b u' is [[-beta0, beta0], [-beta1, beta1]] (h phi_j' = -+1, the h of the Jacobian cancels)."""
    xi, wt = orc.gauss_rule01(nquad)
    bq = np.asarray(b(orc.quad_points(nodes, nquad)), dtype=np.float64)
    b0 = np.zeros(len(nodes) - 1)
    b1 = np.zeros(len(nodes) - 1)
    for k in range(len(xi)):
        b0 = b0 + (wt[k] * (1.0 - xi[k])) * bq[:, k]
        b1 = b1 + (wt[k] * xi[k]) * bq[:, k]
    return b0, b1


def conv_bands(nodes, f, a=None, b=None, c=None, nquad=2):
    """(diag[ne+1], sub[ne], sup[ne], load[ne+1], kloc[ne]): sub[i] is the coefficient of u_i in row i+1, sup[i] that
    of u_{i+1} in row i.  Without ``b`` both equal ``off`` of ``orc.p1_bands``."""
    nodes = np.asarray(nodes, dtype=np.float64)
    diag, off, load, kloc = orc.p1_bands(nodes, f, a, nquad, c)
    if b is None:
        return diag, off.copy(), off.copy(), load, kloc
    b0, b1 = conv_halves(nodes, b, nquad)
    diag = diag.copy()
    diag[:-1] -= b0
    diag[1:] += b1
    return diag, off - b1, off + b0, load, kloc


def cell_peclet(nodes, a, b, nquad=2):
    """|bbar_e| h_e / (2 abar_e) per element, bbar and abar the quadrature means (a = None: 1)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    _, wt = orc.gauss_rule01(nquad)
    xq = orc.quad_points(nodes, nquad)
    bbar = np.asarray(b(xq), dtype=np.float64) @ wt
    abar = np.ones(len(nodes) - 1) if a is None else np.asarray(a(xq), dtype=np.float64) @ wt
    return np.abs(bbar) * np.diff(nodes) / (2.0 * abar)


def _interior(diag, sub, sup, load, u0, u1):
    r = np.array(load[1:-1], dtype=np.float64)
    r[0] -= sub[0] * u0
    r[-1] -= sup[-1] * u1
    return r


def banded_ns(diag, sub, sup, load, u0=0.0, u1=0.0):
    """Dirichlet values on both end dofs, the interior by LAPACK's banded LU (partial pivoting)."""
    from scipy.linalg import solve_banded
    n = len(diag)
    u = np.zeros(n)
    u[0], u[-1] = u0, u1
    if n <= 2:
        return u
    ab = np.zeros((3, n - 2))
    ab[1] = diag[1:-1]
    ab[0, 1:] = sup[1:-1]           # row k+1 of the interior couples to its right neighbour by sup[k+1]
    ab[2, :-1] = sub[1:-1]          # and to its left neighbour by sub[k]
    u[1:-1] = solve_banded((1, 1), ab, _interior(diag, sub, sup, load, u0, u1))
    return u


def thomas_ns_ld(diag, sub, sup, load, u0=0.0, u1=0.0):
    """The same system by Thomas elimination in long double (no pivoting; 64-bit mantissa on x86): the forward
    reference of the device solve.  Returned as long double."""
    ld = np.longdouble
    n = len(diag)
    u = np.zeros(n, dtype=ld)
    u[0], u[-1] = ld(u0), ld(u1)
    m = n - 2
    if m <= 0:
        return u
    d = np.asarray(diag[1:-1], dtype=ld).copy()
    lo = np.asarray(sub[1:-1], dtype=ld)            # lo[k]: row k+1 of the interior, column k
    up = np.asarray(sup[1:-1], dtype=ld)            # up[k]: row k, column k+1
    r = np.asarray(load[1:-1], dtype=ld).copy()
    r[0] -= ld(sub[0]) * ld(u0)
    r[-1] -= ld(sup[-1]) * ld(u1)
    for i in range(1, m):
        w = lo[i - 1] / d[i - 1]
        d[i] -= w * up[i - 1]
        r[i] -= w * r[i - 1]
    x = np.zeros(m, dtype=ld)
    x[-1] = r[-1] / d[-1]
    for i in range(m - 2, -1, -1):
        x[i] = (r[i] - up[i] * x[i + 1]) / d[i]
    u[1:-1] = x
    return u


def fem_solve(nodes, f, a=None, b=None, c=None, nquad=2, u0=0.0, u1=0.0):
    """Nodal values of the P1 solve: the bands above through LAPACK."""
    diag, sub, sup, load, _ = conv_bands(nodes, f, a, b, c, nquad)
    return banded_ns(diag, sub, sup, load, u0, u1)


# --------------------------------------------------------------------------
# bands of -u'' + b u' + c u on a uniform mesh of (-1, 1) with a prescribed max cell Peclet number
# --------------------------------------------------------------------------
SHAPES = {"pos": lambda x: 1.0 + 0.0 * x, "neg": lambda x: -1.0 + 0.0 * x, "change": lambda x: -1.0 * x}


@functools.lru_cache(maxsize=None)
def peclet_case(ne, peclet, shape, u0=0.25, u1=-0.5):
    """(bands, u_ld, u_lapack) of -u'' + b u' + u = pi^2 sin(pi x), b = amp * SHAPES[shape] with amp such that the
    largest cell Peclet number |bbar_e| h / 2 is ``peclet``.  Computed once per case and shared: do not write to the
    arrays."""
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    c = lambda x: 1.0 + 0.0 * x                                       # noqa: E731
    b = None
    unit = cell_peclet(nodes, None, SHAPES[shape]).max()
    if peclet > 0 and unit > 0:                                       # (one element and an odd b: bbar = 0, no b)
        b = lambda x: (peclet / unit) * SHAPES[shape](np.asarray(x, dtype=np.float64))    # noqa: E731
    bands = conv_bands(nodes, orc.poisson_rhs, None, b, c)[:4]
    u_ld = thomas_ns_ld(*bands, u0, u1)
    u_la = banded_ns(*bands, u0, u1)
    return bands, u_ld, u_la


# --------------------------------------------------------------------------
# manufactured problem: u = sin(pi x) on (-1, 1), a = 1 + x^2/4, b = 1 + x/2, c = 1
# --------------------------------------------------------------------------
def man_a(x):
    x = np.asarray(x, dtype=np.float64)
    return 1.0 + 0.25 * x * x


def man_da(x):
    return 0.5 * np.asarray(x, dtype=np.float64)


def man_b(x):
    return 1.0 + 0.5 * np.asarray(x, dtype=np.float64)


def man_c(x):
    return 1.0 + 0.0 * np.asarray(x, dtype=np.float64)


def man_u(x):
    return np.sin(np.pi * np.asarray(x, dtype=np.float64))


def man_f(x):
    """-(a u')' + b u' + c u for u = sin(pi x)."""
    x = np.asarray(x, dtype=np.float64)
    s, co = np.sin(np.pi * x), np.cos(np.pi * x)
    return man_a(x) * np.pi ** 2 * s + (man_b(x) - man_da(x)) * np.pi * co + man_c(x) * s


def man_folded(x):
    """a' - b: what the enhancement and indicator tables hold."""
    return man_da(x) - man_b(x)


# --------------------------------------------------------------------------
# boundary layer: -eps u'' + u' = 1 on (0, 1), u(0) = u(1) = 0; the outflow layer is at x = 1
# --------------------------------------------------------------------------
LAYER_EPS = 0.02


def layer_a(x):
    return LAYER_EPS + 0.0 * np.asarray(x, dtype=np.float64)


def layer_da(x):
    return 0.0 * np.asarray(x, dtype=np.float64)


def layer_b(x):
    return 1.0 + 0.0 * np.asarray(x, dtype=np.float64)


layer_f = layer_b


def layer_folded(x):
    return layer_da(x) - layer_b(x)


def layer_exact(x):
    x = np.asarray(x, dtype=np.float64)
    e1 = math.exp(-1.0 / LAYER_EPS)
    return x - (np.exp((x - 1.0) / LAYER_EPS) - e1) / (1.0 - e1)
