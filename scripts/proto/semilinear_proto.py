"""numpy statement of DESIGN.md section 27: a damped Newton iteration for

    -(a u')' + b u' + c u + g(x, u) = f      on a P1 mesh,

each end Dirichlet u = g_end or Robin a du/dn + kappa u = g_end, with g from a tabulated family: POLY
g = sum_k q_k(x) u^k and EXP g = q_0(x) exp(q_1(x) u).  One Newton step from the nodal iterate u is the LINEAR problem
with the reaction c + g_u(x, u_h) and the right-hand side f - g(x, u_h) + g_u(x, u_h) u_h at the quadrature points (u_h:
the P1 interpolant of u), solved for the new iterate itself.  The merit function is |R(v)|_inf, R(v) = K v + G(v) - F.

The module has its own assembly -- the oracle's conventions (Gauss rule on [0, 1], k = abar / h, consistent mass, the
convection halves), written on TABLES at the quadrature points so that c_eff can go in -- and solves through LAPACK's
banded LU in float64 or an unpivoted elimination in any numpy float type (np.longdouble: the reference the float64
bars are measured against).  It does not import the library.  The device kernels (csrc/nonlinear.hip) and the facade's
solve_fem with ``nonlinear=`` follow this text step by step; tests/semilinear_rules.py imports it.

Run as a script it prints the accuracy record DESIGN.md quotes."""
import math

import numpy as np

DIRICHLET, ROBIN = 0, 1
POLY, EXP = 0, 1
MAX_TERMS = 6
ARMIJO = 1e-4


def gauss_rule01(nquad=2):
    xg, wg = np.polynomial.legendre.leggauss(int(nquad))
    return 0.5 * (1.0 + xg), 0.5 * wg


def quad_points(nodes, nquad=2):
    nodes = np.asarray(nodes, dtype=np.float64)
    xi, _ = gauss_rule01(nquad)
    return nodes[:-1, None] + (nodes[1:] - nodes[:-1])[:, None] * xi[None, :]


def table(fn, pts, default=None):
    """float64 table of the callable ``fn`` at ``pts`` (``None``: the constant ``default``, or None)."""
    if fn is None:
        return None if default is None else np.full(pts.shape, float(default))
    return np.array(np.broadcast_to(np.asarray(fn(pts), dtype=np.float64), pts.shape))


def assemble(nodes, aq, bq, cq, fq, nquad=2, dtype=np.float64):
    """(diag[ne+1], sub[ne], sup[ne], load[ne+1]) of -(a u')' + b u' + c u = f from the tables [ne, nquad] at the
    quadrature points (aq None: a = 1; bq, cq None: no such term); sub[i] is the coefficient of u_i in row i+1, sup[i]
    that of u_{i+1} in row i."""
    nodes = np.asarray(nodes, dtype=dtype)
    xi, wt = (np.asarray(v, dtype=dtype) for v in gauss_rule01(nquad))
    h = nodes[1:] - nodes[:-1]
    ne = len(h)
    fq = np.asarray(fq, dtype=dtype)
    sl, sr, am = (np.zeros(ne, dtype=dtype) for _ in range(3))
    for k in range(len(xi)):
        sl = sl + (wt[k] * (1.0 - xi[k])) * fq[:, k]
        sr = sr + (wt[k] * xi[k]) * fq[:, k]
        if aq is not None:
            am = am + wt[k] * np.asarray(aq, dtype=dtype)[:, k]
    kloc = (np.ones(ne, dtype=dtype) if aq is None else am) / h
    diag, load = np.zeros(ne + 1, dtype=dtype), np.zeros(ne + 1, dtype=dtype)
    diag[:-1] += kloc
    diag[1:] += kloc
    load[:-1] += h * sl
    load[1:] += h * sr
    sub, sup = -kloc, -kloc
    if cq is not None:
        cq = np.asarray(cq, dtype=dtype)
        diag[:-1] += h * (cq @ (wt * (1.0 - xi) ** 2))
        diag[1:] += h * (cq @ (wt * xi ** 2))
        m = h * (cq @ (wt * (1.0 - xi) * xi))
        sub, sup = sub + m, sup + m
    if bq is not None:
        bq = np.asarray(bq, dtype=dtype)
        b0, b1 = bq @ (wt * (1.0 - xi)), bq @ (wt * xi)
        diag[:-1] -= b0
        diag[1:] += b1
        sub, sup = sub - b1, sup + b0
    return diag, sub, sup, load


def g_and_gu(kind, q, uh):
    """(g, g_u) at the tables' points, in the kernels' order: Horner for POLY, E = exp(q_1 u) for EXP."""
    if kind == EXP:
        E = np.exp(q[1] * uh)
        return q[0] * E, (q[0] * q[1]) * E
    K = len(q) - 1
    g = q[K] + 0.0 * uh
    d = (float(K) * q[K] if K > 0 else 0.0 * q[K]) + 0.0 * uh
    for k in range(K - 1, -1, -1):
        g = g * uh + q[k]
        if k >= 1:
            d = d * uh + float(k) * q[k]
    return g, d


def linearize(kind, q, u, t, c, f):
    """(c_eff, f_eff, f_res) [ne, n] of lssvr_nl_linearize, element-major: q [nterm, ne, n], c (None: 0) and f [ne, n],
    t [n] local coordinates, u [ne+1]; in the dtype of ``u``."""
    dt = u.dtype
    q = [np.asarray(v, dtype=dt) for v in q]
    uh = u[:-1, None] + (u[1:] - u[:-1])[:, None] * np.asarray(t, dtype=dt)[None, :]
    g, d = g_and_gu(kind, q, uh)
    fr = np.asarray(f, dtype=dt) - g
    c0 = np.zeros_like(fr) if c is None else np.asarray(c, dtype=dt)
    return c0 + d, fr + d * uh, fr


def residual(diag, sub, sup, load, u, kinds, kappa, g):
    """r[ne+1] of lssvr_nl_residual: rows of K u - load, + (kappa u - g) at a Robin end, 0 at a Dirichlet end."""
    r = diag * u
    r[1:] = sub * u[:-1] + r[1:]
    r[:-1] = r[:-1] + sup * u[1:]
    r = r - load
    for i, end in ((0, 0), (1, -1)):
        r[end] = r[end] + (kappa[i] * u[end] - g[i]) if kinds[i] == ROBIN else 0.0
    return r


def lapack_solve(d, lo, up, b):
    from scipy.linalg import solve_banded
    ab = np.zeros((3, len(d)))
    ab[1] = d
    ab[0, 1:] = up
    ab[2, :-1] = lo
    return solve_banded((1, 1), ab, b)


def thomas_solve(d, lo, up, b):
    """Unpivoted elimination in the arrays' own float type (the np.longdouble reference)."""
    d, b = d.copy(), b.copy()
    for i in range(1, len(d)):
        m = lo[i - 1] / d[i - 1]
        d[i] = d[i] - m * up[i - 1]
        b[i] = b[i] - m * b[i - 1]
    x = b
    x[-1] = b[-1] / d[-1]
    for i in range(len(d) - 2, -1, -1):
        x[i] = (b[i] - up[i] * x[i + 1]) / d[i]
    return x


def bc_solve(diag, sub, sup, rhs, kinds, kappa, g):
    """u[ne+1] of the system with the ends of lssvr_tridiag_ns_bc_solve_multi: a Robin end keeps its node, adds kappa to
    its diagonal and g to its row; a Dirichlet end is the value g, taken to the neighbour's right-hand side."""
    ne = len(sub)
    dt = rhs.dtype
    lo, hi = (0 if kinds[0] == ROBIN else 1), (ne + 1 if kinds[1] == ROBIN else ne)
    u = np.zeros(ne + 1, dtype=dt)
    d, b = diag[lo:hi].copy(), rhs[lo:hi].copy()
    if kinds[0] == ROBIN:
        d[0] += dt.type(kappa[0])
        b[0] += dt.type(g[0])
    else:
        u[0] = g[0]
        if hi > lo:
            b[0] -= sub[0] * dt.type(g[0])
    if kinds[1] == ROBIN:
        d[-1] += dt.type(kappa[1])
        b[-1] += dt.type(g[1])
    else:
        u[ne] = g[1]
        if hi > lo:
            b[-1] -= sup[ne - 1] * dt.type(g[1])
    if hi > lo:
        fn = lapack_solve if dt == np.float64 else thomas_solve
        u[lo:hi] = fn(d, sub[lo:hi - 1], sup[lo:hi - 1], b)
    return u


def solve(nodes, kind, q, f, a=None, b=None, c=None, kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0),
          end_values=(0.0, 0.0), u_init=None, tol=1e-12, max_iter=30, max_halvings=8, nquad=2, dtype=np.float64,
          K=None):
    """The Newton loop.  ``q``: the list of callables q_k(x); ``f``, ``a``, ``b``, ``c``: callables (None: 0, a = 1).
    Every callable is tabulated in float64; everything after runs in ``dtype``.  ``K``: (diag, sub, sup) float64 to use
    as the bands of the linear operator in the merit function instead of this module's assembly (the arrays another
    assembly produced).  Returns dict(u, iterations, residuals, steps, lambdas, converged, K=(diag, sub, sup)):
    residuals[i] = |R(u_i)|_inf and steps[i] = |u_new - u_i|_inf of iteration i + 1, lambdas[i] the damping it took."""
    nodes = np.asarray(nodes, dtype=np.float64)
    dt = np.dtype(dtype)
    xq = quad_points(nodes, nquad)
    t = gauss_rule01(nquad)[0]
    aq, bq, cq, fq = table(a, xq), table(b, xq), table(c, xq), table(f, xq, 0.0)
    qq = [table(fn, xq) for fn in q]
    zq = np.zeros_like(xq)
    if K is None:
        K = assemble(nodes, aq, bq, cq, zq, nquad, dt)[:3]
    K = tuple(np.asarray(v, dtype=dt) for v in K)
    g = [dt.type(v) for v in end_values]
    kap = [dt.type(v) for v in kappa]
    u = np.zeros(len(nodes), dtype=dt) if u_init is None else \
        np.array(np.broadcast_to(np.asarray(u_init(nodes), dtype=np.float64), nodes.shape), dtype=dt)
    for i, end in ((0, 0), (1, -1)):
        if kinds[i] == DIRICHLET:
            u[end] = g[i]

    def merit(v):
        fr = linearize(kind, qq, v, t, cq, fq)[2]
        load = assemble(nodes, None, None, None, fr, nquad, dt)[3]
        return float(np.max(np.abs(residual(*K, load, v, kinds, kap, g))))

    rep = dict(iterations=0, residuals=[], steps=[], lambdas=[], converged=False, K=K)
    for it in range(1, int(max_iter) + 1):
        ce, fe, _ = linearize(kind, qq, u, t, cq, fq)
        d_, lo_, up_, load = assemble(nodes, aq, bq, ce, fe, nquad, dt)
        u_new = bc_solve(d_, lo_, up_, load, kinds, kap, g)
        r0 = merit(u)
        step, size = float(np.max(np.abs(u_new - u))), float(np.max(np.abs(u_new)))
        if not all(math.isfinite(v) for v in (r0, step, size)):
            raise RuntimeError(f"Newton iteration {it} produced non-finite values")
        rep["iterations"] = it
        rep["residuals"].append(r0)
        rep["steps"].append(step)
        if step <= tol * max(1.0, size):
            u = u_new
            rep["lambdas"].append(1.0)
            rep["converged"] = True
            break
        lam, tried = 1.0, []
        for _ in range(int(max_halvings) + 1):
            v = u_new if lam == 1.0 else u + dt.type(lam) * (u_new - u)
            rv = merit(v)
            tried.append((rv, lam, v))
            if rv <= (1.0 - ARMIJO * lam) * r0:
                break
            lam *= 0.5
        else:
            rv, lam, v = min(tried, key=lambda p: p[0])
        u = v
        rep["lambdas"].append(lam)
    rep["u"] = u
    return rep


# ---- Bratu: -u'' - lam e^u = 0 on (0, 1), u(0) = u(1) = 0; the lower branch in closed form -------------------------
def bratu_theta(lam=1.0):
    """The smaller root of theta = sqrt(2 lam) cosh(theta / 4), by bisection on [0, 4 asinh-point]."""
    fn = lambda th: th - math.sqrt(2.0 * lam) * math.cosh(th / 4.0)      # noqa: E731
    lo, hi = 0.0, 4.0                     # fn(0) < 0; the lower root lies below the maximum of fn
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if fn(mid) < 0.0 else (lo, mid)
    return 0.5 * (lo + hi)


def bratu_exact(x, lam=1.0):
    th = bratu_theta(lam)
    return -2.0 * np.log(np.cosh((np.asarray(x, dtype=np.float64) - 0.5) * th / 2.0) / math.cosh(th / 4.0))


def bratu(ne, lam=1.0, dtype=np.float64, **kw):
    nodes = np.linspace(0.0, 1.0, ne + 1)
    return solve(nodes, EXP, [lambda x: -lam + 0.0 * x, lambda x: 1.0 + 0.0 * x], None, dtype=dtype, **kw)


# ---- case A: -u'' + u^3 = f, u = sin(pi x) on (-1, 1) -----------------------------------------------------------------
def cubic_f(x):
    s = np.sin(math.pi * x)
    return math.pi ** 2 * s + s ** 3


def cubic_q():
    z = lambda x: 0.0 * x                 # noqa: E731
    return [z, z, z, lambda x: 1.0 + 0.0 * x]


def cubic(ne, dtype=np.float64, **kw):
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    return solve(nodes, POLY, cubic_q(), cubic_f, dtype=dtype, **kw)


def enhance(nodes, u, kind, q, f, M, gamma, n, a=None, da=None, b=None, c=None, kinds=(DIRICHLET, DIRICHLET),
            end_values=(0.0, 0.0)):
    """W [ne, M] of the enhancement: ONE linearisation at the collocation points around the P1 interpolant of ``u``,
    then the oracle's reaction rows with c_values = c_eff, rhs_values = f_eff and the folded a' - b.  (The only use of
    the oracle: the element rows are its own.)"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if root not in sys.path:
        sys.path.insert(0, root)
    from oracle import lssvr_oracle as orc
    nodes = np.asarray(nodes, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    ne = len(nodes) - 1
    xc = np.linspace(nodes[:-1], nodes[1:], n, axis=-1)
    t = np.arange(n, dtype=np.float64) / float(n - 1)
    ce, fe, _ = linearize(kind, [table(fn, xc) for fn in q], u, t, table(c, xc), table(f, xc, 0.0))
    W = np.zeros((ne, M))
    one = lambda x: np.ones_like(x)       # noqa: E731
    for e in range(ne):
        fold = lambda x, e=e: (0.0 * x if da is None else da(x)) - (0.0 * x if b is None else b(x))   # noqa: E731
        gl = end_values[0] if (e == 0 and kinds[0] == DIRICHLET) else u[e]
        gr = end_values[1] if (e == ne - 1 and kinds[1] == DIRICHLET) else u[e + 1]
        s = orc.element_system(nodes[e], nodes[e + 1], gl, gr, M, gamma, n, rhs=None, coef_a=one if a is None else a,
                               coef_da=fold, f_values=fe[e], coef_c=lambda x, e=e: ce[e])
        W[e] = orc.solve_bc_eliminated(s)
    return W


if __name__ == "__main__":
    print("case A, -u'' + u^3 = f, u = sin(pi x): ne, iterations, lambdas, max nodal error")
    for ne in (8, 16, 32):
        r = cubic(ne)
        x = np.linspace(-1.0, 1.0, ne + 1)
        print(ne, r["iterations"], r["lambdas"], f"{np.max(np.abs(r['u'] - np.sin(math.pi * x))):.4e}")
        print("   steps", [f"{s:.2e}" for s in r["steps"]])
    print("Bratu lam = 1: ne, iterations, max nodal error against the closed form")
    for ne in (8, 16, 32):
        r = bratu(ne)
        print(ne, r["iterations"], f"{np.max(np.abs(r['u'] - bratu_exact(np.linspace(0, 1, ne + 1)))):.4e}")
