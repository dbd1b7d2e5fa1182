"""numpy statement of DESIGN.md section 28: BDF1 / BDF2 with a fixed step and a fixed number of Newton iterations for

    rho u_t - (a u')' + c u + g(x, u) = f(x, t) = sum_r phi_r(t) f_r(x)      on a P1 mesh,

each end Dirichlet u = g(t) or Robin a du/dn + kappa u = g(t), g(x, u) from the tabulated families of section 27:
("poly", [q0, q1, ...]) -- sum_k q_k(x) u^k -- or ("exp", q0, q1) -- q0(x) exp(q1(x) u).  Step n+1 solves

    (alpha / dt) M v + K v + G(v) = r,      r = (1/dt) M (beta0 u^n + beta1 u^{n-1}) + load(t_{n+1}),

by newton_iters iterations from v_0 = 2 u^n - u^{n-1} (BDF1 and the first step: u^n): iterate k is the linear problem
with the reaction c + alpha rho / dt + g_u(x, v_k,h) and the right-hand side r + L(-g + g_u v_k,h), solved for v_{k+1}
itself.  After each solve the monitor row (|A_k v_k - b_k|_inf on the free rows, |v_{k+1} - v_k|_inf, |v_{k+1}|_inf, the
count of non-finite entries) is kept: A_k v_k - b_k is the nonlinear residual at v_k.

The module has its own assembly (every sum in the order the device kernel documents), runs in float64 through
scipy.linalg.solve_banded (LAPACK's pivoting banded LU) or in any numpy float type through an unpivoted elimination
(np.longdouble: the reference the float64 bars are measured against), and imports neither the library nor the oracle.
tests/transient_nl_rules.py imports it.

Run as a script it prints, for u_t - u'' + u^3 = f with u = exp(-t) sin(pi x) on (0, 1), the float64 loop's distance
from the np.longdouble loop and the observed temporal orders of BDF1 and BDF2."""
import math

import numpy as np

DIRICHLET, ROBIN = 0, 1
POLY, EXP = 0, 1
SCHEMES = {"bdf1": (1.0, 1.0, 0.0), "bdf2": (1.5, 2.0, -0.5)}      # alpha, beta0, beta1


def _zero(x):
    return np.zeros_like(np.asarray(x, dtype=np.float64))


def _one(x):
    return np.ones_like(np.asarray(x, dtype=np.float64))


def _fn(v):
    return v if callable(v) else (lambda t, v=float(v): v)


def gauss01(nquad):
    """(xi, w) of the Gauss-Legendre rule on [0, 1], float64."""
    xg, wg = np.polynomial.legendre.leggauss(int(nquad))
    return 0.5 * (1.0 + xg), 0.5 * wg


def table(fn, pts):
    """An own float64 array of fn at pts (broadcast)."""
    return np.array(np.broadcast_to(np.asarray(fn(pts), dtype=np.float64), pts.shape))


def quad_points(nodes, xi):
    return nodes[:-1, None] + np.diff(nodes)[:, None] * xi[None, :]


def family(kind, q, uh):
    """(g, g_u) at the points of uh; q [nterm, ...].  POLY by Horner from the highest term, g_u with the factors
    (double)k; EXP: E = exp(q1 uh), g = q0 E, g_u = (q0 q1) E."""
    if kind == EXP:
        E = np.exp(q[1] * uh)
        return q[0] * E, (q[0] * q[1]) * E
    K = len(q) - 1
    g = q[K].copy()
    d = np.zeros_like(g) if K == 0 else float(K) * q[K]
    for j in range(K - 1, -1, -1):
        g = g * uh + q[j]
        if j >= 1:
            d = d * uh + float(j) * q[j]
    return g, d


def p1_system(nodes, a_q, c_q, f_q, rule):
    """(diag, off, load) of -(a u')' + c u = f from the tables [ne, nquad] (a_q None: a = 1), in the arrays' float
    type.  Per element: sl += (w (1 - xi)) f, sr += (w xi) f, am += w a, ll += (w c) ((1 - xi)(1 - xi)), lr, rr likewise,
    k running over the points; k = am / h, fl = h sl, ..., m_ll = h ll, ...  Per node: d = 0; d += k + m_ll (right
    element); d += k + m_rr (left element); l likewise; off = m_lr - k."""
    xi, w = rule
    dt = c_q.dtype
    h = np.diff(nodes).astype(dt)
    ne = len(h)
    sl, sr, am, ll, lr, rr = (np.zeros(ne, dtype=dt) for _ in range(6))
    for k in range(len(xi)):
        x_, w_ = dt.type(xi[k]), dt.type(w[k])
        one = dt.type(1.0)
        sl += (w_ * (one - x_)) * f_q[:, k]
        sr += (w_ * x_) * f_q[:, k]
        if a_q is not None:
            am += w_ * a_q[:, k]
        wc = w_ * c_q[:, k]
        ll += wc * ((one - x_) * (one - x_))
        lr += wc * ((one - x_) * x_)
        rr += wc * (x_ * x_)
    kk = (am if a_q is not None else np.ones(ne, dtype=dt)) / h
    fl, fr, mll, mlr, mrr = h * sl, h * sr, h * ll, h * lr, h * rr
    d, l = np.zeros(ne + 1, dtype=dt), np.zeros(ne + 1, dtype=dt)
    d[:-1] += kk + mll
    l[:-1] += fl
    d[1:] += kk + mrr
    l[1:] += fr
    return d, mlr - kk, l


def newton_system(nodes, v, a_q, cs_q, q_q, r, kind, rule):
    """(diag, off, rhs) of one Newton iteration around the nodal iterate v: u_h = v_e + (v_{e+1} - v_e) xi,
    c_eff = cs + g_u, f_eff = (0 - g) + g_u u_h, the assembly of p1_system, rhs = r + load."""
    dt = v.dtype
    xi = np.asarray(rule[0]).astype(dt)
    uh = v[:-1, None] + (v[1:] - v[:-1])[:, None] * xi[None, :]
    g, d = family(kind, q_q, uh)
    diag, off, load = p1_system(nodes, a_q, cs_q + d, (dt.type(0.0) - g) + d * uh, rule)
    return diag, off, r + load


def tri_apply(d, o, v):
    out = d * v
    out[1:] = o * v[:-1] + out[1:]
    out[:-1] = out[:-1] + o * v[1:]
    return out


def step_rhs(md, mo, u0, u1, beta0, beta1, inv_dt, L, phi):
    v = beta0 * u0 if beta1 == 0.0 else beta0 * u0 + beta1 * u1
    s = inv_dt * tri_apply(md, mo, v)
    for r in range(len(phi)):
        s = s + phi[r] * L[r]
    return s


def lapack_solve(d, o, b):
    from scipy.linalg import solve_banded
    ab = np.zeros((3, len(d)))
    ab[1] = d
    ab[0, 1:] = o
    ab[2, :-1] = o
    return solve_banded((1, 1), ab, b)


def thomas_solve(d, o, b):
    """Unpivoted elimination in the arrays' own float type."""
    d, b = d.copy(), b.copy()
    for i in range(1, len(d)):
        m = o[i - 1] / d[i - 1]
        d[i] = d[i] - m * o[i - 1]
        b[i] = b[i] - m * b[i - 1]
    b[-1] = b[-1] / d[-1]
    for i in range(len(d) - 2, -1, -1):
        b[i] = (b[i] - o[i] * b[i + 1]) / d[i]
    return b


def bc_solve(diag, off, rhs, kinds, kappa, g, solve_fn):
    """The ends of lssvr_tridiag_bc_solve_multi: a Robin end keeps its node, adds kappa to its diagonal and g to its
    row; a Dirichlet end is the value g, taken to the neighbour's right-hand side."""
    ne = len(off)
    sh, hi = (0 if kinds[0] == ROBIN else 1), (ne + 1 if kinds[1] == ROBIN else ne)
    u = np.zeros(ne + 1, dtype=rhs.dtype)
    d, b = diag[sh:hi].copy(), rhs[sh:hi].copy()
    if kinds[0] == ROBIN:
        d[0] += kappa[0]
        b[0] += g[0]
    else:
        u[0] = g[0]
        if hi > sh:
            b[0] -= off[0] * g[0]
    if kinds[1] == ROBIN:
        d[-1] += kappa[1]
        b[-1] += g[1]
    else:
        u[ne] = g[1]
        if hi > sh:
            b[-1] -= off[ne - 1] * g[1]
    if hi > sh:
        u[sh:hi] = solve_fn(d, off[sh:hi - 1], b)
    return u


def monitor(diag, off, rhs, v, v_new, kinds, kappa, g):
    """The four numbers of lssvr_nl_residual: r = (A v - rhs) + (kappa v - g) at a Robin end, 0 at a Dirichlet end."""
    r = tri_apply(diag, off, v) - rhs
    for i, end in ((0, 0), (1, -1)):
        r[end] = r[end] + (kappa[i] * v[end] - g[i]) if kinds[i] == ROBIN else 0.0
    out, bad = [], 0
    for t in (r, v_new - v, v_new):
        fin = np.isfinite(t)
        bad += int(np.sum(~fin))
        out.append(np.max(np.abs(t[fin])) if fin.any() else t.dtype.type(0.0))
    return out + [bad]


def solve(nodes, u0, t_end, nsteps, scheme="bdf2", nonlinear=("poly", [_zero]), a=None, c=None, rho=None, forcing=None,
          kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), end_data=(0.0, 0.0), snapshots=None, nquad=2,
          newton_iters=3, dtype=np.float64, bands=None, rule=None):
    """The time loop.  Returns dict(times, nodal [ns, ne+1], diffs [ns, ne+1] (the nodal BDF differences at the
    snapshots), weights, phi, g, newton [nsteps, newton_iters, 4], dt).  ``dtype`` other than float64 runs the unpivoted
    elimination and every sum in that type on the float64 tables.  ``bands``: dict(mass=(mdiag, moff), loads [R, ne+1])
    to run on instead of this module's assembly (the float64 arrays another assembly produced); ``rule``: (xi, w) on
    [0, 1] instead of gauss01(nquad)."""
    dtype = np.dtype(dtype)
    nodes = np.asarray(nodes, dtype=np.float64)
    ne = len(nodes) - 1
    rule = gauss01(nquad) if rule is None else rule
    kind = {"poly": POLY, "exp": EXP}[nonlinear[0]]
    qf = list(nonlinear[1]) if kind == POLY else list(nonlinear[1:])
    forcing = [(0.0, _zero)] if not forcing else list(forcing)
    snapshots = [nsteps] if snapshots is None else list(snapshots)
    dt = float(t_end) / nsteps
    inv_dt = 1.0 / dt
    solve_fn = lapack_solve if dtype == np.float64 else thomas_solve
    xq = quad_points(nodes, np.asarray(rule[0], dtype=np.float64))
    a_q = None if a is None else table(a, xq).astype(dtype)
    c64, rho64 = table(_zero if c is None else c, xq), table(_one if rho is None else rho, xq)
    q_q = np.stack([table(f, xq) for f in qf]).astype(dtype)
    cs = {al: (c64 + al * rho64 / dt).astype(dtype) for al in {1.0, SCHEMES[scheme][0]}}       # rounded in float64
    if bands is None:
        z = np.zeros_like(c64)
        md, mo, _ = p1_system(nodes, z, rho64, z, rule)
        L = np.stack([p1_system(nodes, None, z, table(f, xq), rule)[2] for _, f in forcing])
    else:
        (md, mo), L = bands["mass"], bands["loads"]
    md, mo, L = (np.asarray(t, dtype=dtype) for t in (md, mo, L))
    phis = [_fn(p) for p, _ in forcing]
    gl, gr = (_fn(v) for v in end_data)
    times = dt * np.arange(nsteps + 1)
    phi = np.array([[p(t) for p in phis] for t in times], dtype=np.float64)
    g = np.array([[gl(t), gr(t)] for t in times], dtype=np.float64)
    cur = table(u0, nodes).astype(dtype)
    for i, end in ((0, 0), (1, ne)):
        if kinds[i] == DIRICHLET:
            cur[end] = g[0, i]
    prev = None
    out = dict(times=[], nodal=[], diffs=[], weights=[], phi=[], g=[], dt=dt)
    newton = np.zeros((nsteps, newton_iters, 4), dtype=dtype)
    for n in range(1, nsteps + 1):
        al, b0, b1 = SCHEMES["bdf1"] if (n == 1 or scheme == "bdf1") else SCHEMES["bdf2"]
        r = step_rhs(md, mo, cur, prev, b0, b1, inv_dt, L, phi[n].astype(dtype))
        gn = g[n].astype(dtype)
        v = cur.copy() if b1 == 0.0 else prev + dtype.type(2.0) * (cur - prev)
        for k in range(newton_iters):
            diag, off, rhs = newton_system(nodes, v, a_q, cs[al], q_q, r, kind, rule)
            v_new = bc_solve(diag, off, rhs, kinds, kappa, gn, solve_fn)
            newton[n - 1, k] = monitor(diag, off, rhs, v, v_new, kinds, kappa, gn)
            v = v_new
        if n in snapshots:
            d = al * v - b0 * cur
            out["times"].append(times[n])
            out["nodal"].append(v.copy())
            out["diffs"].append(inv_dt * (d if b1 == 0.0 else d - b1 * prev))
            out["weights"].append((al, b0, b1))
            out["phi"].append(phi[n])
            out["g"].append(g[n])
        prev, cur = cur, v
    for k in ("times", "nodal", "diffs", "weights", "phi", "g"):
        out[k] = np.array(out[k])
    out["newton"] = newton
    return out


# the manufactured problem of the checks: u_t - u'' + u^3 = f, u = exp(-t) sin(pi x) on (0, 1), zero Dirichlet ends
def cubic_manufactured():
    """(u0, nonlinear, forcing, exact(x, t)):  f = (pi^2 - 1) e^{-t} sin(pi x) + e^{-3t} sin^3(pi x), so R = 2."""
    s = lambda x: np.sin(math.pi * np.asarray(x, dtype=np.float64))       # noqa: E731
    forcing = [(lambda t: (math.pi ** 2 - 1.0) * math.exp(-t), s), (lambda t: math.exp(-3.0 * t), lambda x: s(x) ** 3)]
    return s, ("poly", [_zero, _zero, _zero, _one]), forcing, lambda x, t: math.exp(-t) * s(x)


def temporal_orders(ne=2048, steps=(8, 16, 32), t_end=1.0, newton_iters=3):
    """{scheme: [log2 of the error ratios]} of the nodal max error at t_end against the SPATIALLY discrete limit (the
    same mesh, 1024 BDF2 steps), so that the mesh error cancels."""
    u0, nl, forcing, _ = cubic_manufactured()
    nodes = np.linspace(0.0, 1.0, ne + 1)
    ref = solve(nodes, u0, t_end, 1024, "bdf2", nl, forcing=forcing, newton_iters=newton_iters)["nodal"][-1]
    out = {}
    for scheme in ("bdf1", "bdf2"):
        e = [float(np.max(np.abs(solve(nodes, u0, t_end, n, scheme, nl, forcing=forcing,
                                       newton_iters=newton_iters)["nodal"][-1] - ref))) for n in steps]
        out[scheme] = [math.log2(e[i] / e[i + 1]) for i in range(len(e) - 1)]
    return out


if __name__ == "__main__":
    u0, nl, forcing, exact = cubic_manufactured()
    for scheme in ("bdf1", "bdf2"):
        for ne in (2, 5, 32, 33):
            nodes = np.linspace(0.0, 1.0, ne + 1)
            kw = dict(forcing=forcing, snapshots=list(range(1, 41)))
            r64 = solve(nodes, u0, 0.4, 40, scheme, nl, **kw)
            rld = solve(nodes, u0, 0.4, 40, scheme, nl, dtype=np.longdouble, **kw)
            print(f"{scheme} ne = {ne:3d}: max |float64 - longdouble| = "
                  f"{float(np.max(np.abs(r64['nodal'] - rld['nodal']))):.2e}   last step's monitor "
                  f"{[f'{float(v):.1e}' for v in r64['newton'][-1, :, 0]]}")
    print("temporal orders:", temporal_orders())
