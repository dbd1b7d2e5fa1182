"""numpy prototype of the adjoint sensitivities of the P1 solve of -(a u')' + b u' + c u = f: a
dense restatement of the assembly (the tables a, b, c, f at the Gauss points, csrc/lssvr_p1.hpp and csrc/p1_conv.hip)
and of the solve with Dirichlet, Neumann and Robin ends, the complex-step derivative of a functional J(u) with respect
to every table entry and every end datum (Im J(theta + i 1e-30 delta) / 1e-30: no subtraction, so no cancellation),
and the adjoint formulas that csrc/lssvr_sens.hpp evaluates, in its order of operations.  No GPU, nothing but numpy.

Run as a script it prints what DESIGN.md section 31 records: the deviation of the adjoint gradients from the complex
step on every case of tests/sensitivity_rules.py, the deviation of central differences from it (the tolerances of the
autograd gradcheck), and a small inverse problem -- 20 steps of plain gradient descent on the log of a piecewise-constant
a on 16 elements from exact nodal observations of u."""
import numpy as np

DIRICHLET, ROBIN = 0, 1
CSTEP = 1e-30

# Gauss-Legendre on [0, 1]: the literals of quad_rule (csrc/lssvr_p1.hpp), so that the doubles are the library's
GAUSS01 = {
    1: ([0.5], [1.0]),
    2: ([0.21132486540518711775, 0.78867513459481288225], [0.5, 0.5]),
    3: ([0.11270166537925831148, 0.5, 0.88729833462074168852],
        [0.27777777777777777778, 0.44444444444444444444, 0.27777777777777777778]),
    4: ([0.069431844202973712388, 0.33000947820757186760, 0.66999052179242813240, 0.93056815579702628761],
        [0.17392742256872692869, 0.32607257743127307131, 0.32607257743127307131, 0.17392742256872692869]),
    5: ([0.046910077030668003601, 0.23076534494715845448, 0.5, 0.76923465505284154552, 0.95308992296933199640],
        [0.11846344252809454376, 0.23931433524968323402, 0.28444444444444444444, 0.23931433524968323402,
         0.11846344252809454376]),
}


def gauss01(nq):
    xi, w = GAUSS01[int(nq)]
    return np.array(xi), np.array(w)


def quad_points(x, nq):
    """The Gauss points of every element [ne, nq]: x_e + h_e xi_q."""
    xi, _ = gauss01(nq)
    return x[:-1, None] + np.diff(x)[:, None] * xi[None, :]


# ---- assembly and solve, dense; real or complex ------------------------------------------------------------------------
def assemble(x, f, a=None, b=None, c=None):
    """The raw bands (diag [ne+1], sub [ne], sup [ne], load [ne+1]) of the tables f, a, b, c [ne, nq] (None: a = 1,
    b = 0, c = 0), before any end treatment: sub[i] multiplies u_i in row i+1, sup[i] multiplies u_{i+1} in row i."""
    ne, nq = f.shape
    xi, w = gauss01(nq)
    h = np.diff(x)
    dt = np.result_type(f, *(t for t in (a, b, c) if t is not None))
    one = np.ones((ne, nq)) if a is None else a
    zero = np.zeros((ne, nq))
    b = zero if b is None else b
    c = zero if c is None else c
    k = (one @ w) / h
    mll, mlr, mrr = (h * ((c * w) @ p) for p in ((1 - xi) ** 2, (1 - xi) * xi, xi ** 2))
    b0, b1 = (b * w) @ (1 - xi), (b * w) @ xi
    diag = np.zeros(ne + 1, dtype=dt)
    load = np.zeros(ne + 1, dtype=dt)
    diag[:-1] += k + mll - b0
    diag[1:] += k + mrr + b1
    load[:-1] += h * ((f * w) @ (1 - xi))
    load[1:] += h * ((f * w) @ xi)
    return diag, (mlr - k) - b1, (mlr - k) + b0, load


def dense(diag, sub, sup):
    return np.diag(diag) + np.diag(sub, -1) + np.diag(sup, 1)


def bc_solve(K, load, kinds, kappa, g):
    """u of the full matrix K and the raw load with the ends: a Dirichlet end has u = g, a Robin (Neumann: kappa = 0)
    end stays an unknown with kappa on the diagonal and g on the load.  Dense LU."""
    n = len(load)
    A = np.array(K, dtype=np.result_type(K, load, np.asarray(kappa), np.asarray(g)))
    r = np.array(load, dtype=A.dtype)
    u = np.zeros(n, dtype=A.dtype)
    free = np.ones(n, dtype=bool)
    for s, end in ((0, 0), (1, n - 1)):
        if kinds[s] == ROBIN:
            A[end, end] += kappa[s]
            r[end] += g[s]
        else:
            free[end] = False
            u[end] = g[s]
    r = r - A[:, ~free] @ u[~free]
    u[free] = np.linalg.solve(A[np.ix_(free, free)], r[free])
    return u


def primal(x, tabs, kinds, kappa, g):
    """(u, K, bands) of the tables ``tabs`` = dict(f=, a=, b=, c=)."""
    bands = assemble(x, tabs["f"], tabs.get("a"), tabs.get("b"), tabs.get("c"))
    K = dense(*bands[:3])
    return bc_solve(K, bands[3], kinds, kappa, g), K, bands


def adjoint(K, p, kinds, kappa):
    """z of the TRANSPOSED matrix with load p, zero end data and the primal's kinds and kappa."""
    return bc_solve(K.T, p, kinds, kappa, (0.0, 0.0))


# ---- functionals: J(u), analytic in u, and p = dJ/du ---------------------------------------------------------------------
class Linear:
    """J(u) = p . u for a nodal vector p (the P1 load of a density j: J = int j u_h dx)."""

    def __init__(self, p):
        self.p = np.asarray(p, dtype=np.float64)

    def value(self, x, u):
        return self.p @ u

    def gradient(self, x, u):
        return self.p.copy()


def hat_weights(x, xo):
    """(e, t): the element of every observation point and its local coordinate, u_h(xo) = u_e (1 - t) + u_{e+1} t."""
    e = np.clip(np.searchsorted(x, xo, side="right") - 1, 0, len(x) - 2)
    return e, (xo - x[e]) / (x[e + 1] - x[e])


class Misfit:
    """J(u) = 1/2 sum_i (u_h(x_i) - d_i)^2; p scatters the residuals through the hat functions."""

    def __init__(self, xo, d):
        self.xo, self.d = np.asarray(xo, dtype=np.float64), np.asarray(d, dtype=np.float64)

    def residual(self, x, u):
        e, t = hat_weights(x, self.xo)
        return u[e] * (1 - t) + u[e + 1] * t - self.d

    def value(self, x, u):
        r = self.residual(x, u)
        return 0.5 * (r @ r)          # (no conjugate: analytic, as the complex step needs)

    def gradient(self, x, u):
        e, t = hat_weights(x, self.xo)
        r = self.residual(x, u)
        p = np.zeros(len(x), dtype=r.dtype)
        np.add.at(p, e, r * (1 - t))
        np.add.at(p, e + 1, r * t)
        return p


# ---- the adjoint formulas, in the order of csrc/lssvr_sens.hpp ----------------------------------------------------------
def table_gradients(x, U, Z, nq):
    """(ga, gb, gc, gf), each [nc, ne, nq], of the pairs (U[j], Z[j]); U [nc, ne+1] or [1, ne+1] for all cases.  Every
    operation in the order of sens_entry, one rounding each: bit for bit the library's values."""
    xi, w = gauss01(nq)
    U, Z = np.atleast_2d(U), np.atleast_2d(Z)
    U = np.broadcast_to(U, Z.shape)
    h = (x[1:] - x[:-1])[None, :, None]
    xi, w = xi[None, None, :], w[None, None, :]
    u0, u1, z0, z1 = (t[:, :, None] for t in (U[:, :-1], U[:, 1:], Z[:, :-1], Z[:, 1:]))
    om, wh, hw = 1.0 - xi, w / h, h * w
    du = u1 - u0
    zq = z0 * om + z1 * xi
    ga = -((wh * (z1 - z0)) * du)
    gb = -((w * zq) * du)
    gc = -((hw * zq) * (u0 * om + u1 * xi))
    gf = hw * zq
    return ga, gb, gc, gf


def end_gradients(U, Z, P, band_ends, kinds):
    """out_ends [nc, 4] = (dJ/dg_0, dJ/dg_ne, dJ/dkappa_0, dJ/dkappa_ne) in the order of sens_ends; P None: zero."""
    U, Z = np.atleast_2d(U), np.atleast_2d(Z)
    U = np.broadcast_to(U, Z.shape)
    P = np.zeros_like(Z) if P is None else np.atleast_2d(P)
    ne = Z.shape[1] - 1
    out = np.zeros((Z.shape[0], 4), dtype=Z.dtype)
    for s, (end, inner) in enumerate(((0, 1), (ne, ne - 1))):
        if kinds[s] == ROBIN:
            out[:, s] = Z[:, end]
            out[:, 2 + s] = -(Z[:, end] * U[:, end])
        else:
            out[:, s] = P[:, end] - band_ends[s] * Z[:, inner]
    return out


def adjoint_gradients(x, tabs, kinds, kappa, g, J):
    """dict(a=, b=, c=, f= [ne, nq], ends= [4], value=, u=, z=) by ONE primal and ONE adjoint solve."""
    nq = tabs["f"].shape[1]
    u, K, bands = primal(x, tabs, kinds, kappa, g)
    p = J.gradient(x, u)
    z = adjoint(K, p, kinds, kappa)
    ga, gb, gc, gf = (t[0] for t in table_gradients(x, u, z, nq))
    ends = end_gradients(u, z, p, (bands[1][0], bands[2][-1]), kinds)[0]
    return dict(a=ga, b=gb, c=gc, f=gf, ends=ends, value=J.value(x, u), u=u, z=z, p=p)


# ---- the yardstick: complex step, one solve per parameter ----------------------------------------------------------------
def _full(x, tabs):
    ne, nq = tabs["f"].shape
    return dict(a=np.ones((ne, nq)) if tabs.get("a") is None else tabs["a"],
                b=np.zeros((ne, nq)) if tabs.get("b") is None else tabs["b"],
                c=np.zeros((ne, nq)) if tabs.get("c") is None else tabs["c"], f=tabs["f"])


def complex_step(x, tabs, kinds, kappa, g, J):
    """The same dict as :func:`adjoint_gradients` (a, b, c, f, ends) by Im J(theta + i 1e-30 delta) / 1e-30."""
    full = _full(x, tabs)
    out = {}
    for name in "abcf":
        grad = np.zeros(full[name].shape)
        for idx in np.ndindex(*grad.shape):
            t = {k: v.astype(complex) if k == name else v for k, v in full.items()}
            t[name][idx] += 1j * CSTEP
            grad[idx] = J.value(x, primal(x, t, kinds, kappa, g)[0]).imag / CSTEP
        out[name] = grad
    ends = np.zeros(4)
    for s in range(2):
        gg = np.array(g, dtype=complex)
        gg[s] += 1j * CSTEP
        ends[s] = J.value(x, primal(x, full, kinds, kappa, gg)[0]).imag / CSTEP
        if kinds[s] == ROBIN:
            kk = np.array(kappa, dtype=complex)
            kk[s] += 1j * CSTEP
            ends[2 + s] = J.value(x, primal(x, full, kinds, kk, g)[0]).imag / CSTEP
    out["ends"] = ends
    return out


def central_differences(x, tabs, kinds, kappa, g, J, eps=1e-6):
    """The table gradients by (J(theta + eps) - J(theta - eps)) / (2 eps): what torch.autograd.gradcheck compares with."""
    full = _full(x, tabs)
    out = {}
    for name in "abcf":
        grad = np.zeros(full[name].shape)
        for idx in np.ndindex(*grad.shape):
            v = []
            for sgn in (1.0, -1.0):
                t = {k: v_.copy() for k, v_ in full.items()}
                t[name][idx] += sgn * eps
                v.append(J.value(x, primal(x, t, kinds, kappa, g)[0]))
            grad[idx] = (v[0] - v[1]) / (2.0 * eps)
        out[name] = grad
    return out


GROUPS = ("a", "b", "c", "f", "ends")


def deviation(got, want):
    """The largest deviation of the gradients ``got`` from ``want`` over the groups a, b, c, f, ends (those that ``got``
    holds), each relative to the largest entry of its group in ``want``."""
    worst = 0.0
    for k in GROUPS:
        if got.get(k) is None:
            continue
        scale = float(np.max(np.abs(want[k])))
        err = float(np.max(np.abs(np.asarray(got[k]) - want[k])))
        worst = max(worst, err / scale if scale > 0.0 else err)
    return worst


# ---- the cases: callables, so that the facade can be handed the same problem ----------------------------------------------
def mesh(ne, seed=3):
    """ne non-uniform elements on [-1, 1]: widths between 0.6 and 1.4 of the mean."""
    rng = np.random.default_rng(seed + ne)
    w = 0.6 + 0.8 * rng.random(ne)
    x = np.concatenate([[0.0], np.cumsum(w)])
    return -1.0 + 2.0 * x / x[-1]


def coef_a(x):
    return 1.0 + 0.3 * np.sin(2.0 * x)


def coef_da(x):
    return 0.6 * np.cos(2.0 * x)


def reaction(x):
    return 1.5 + np.cos(3.0 * x)


def helmholtz(x):
    return -15.0 + 0.0 * x


def rhs(x):
    return np.exp(0.5 * x) + np.sin(3.0 * x)


def goal_density(x):
    return 1.0 + x * x


def convection(ne):
    """b(x) = 0.4 ne x: outflow at both ends (every Robin end keeps kappa + b n / 2 >= 0), cell Peclet number about 0.5
    at the ends of the ``ne``-element mesh."""
    return lambda x: 0.4 * ne * np.asarray(x, dtype=np.float64)


KAPPA = (0.7, 1.3)
END_DATA = (0.3, -0.2)
END_COMBOS = ((DIRICHLET, DIRICHLET), (DIRICHLET, ROBIN), (ROBIN, DIRICHLET), (ROBIN, ROBIN))


def case_tables(x, nq, conv, react):
    """The tables of a case at the Gauss points: a always, b with ``conv``, c with ``react`` (True, or "helmholtz")."""
    xq = quad_points(x, nq)
    tabs = dict(f=rhs(xq), a=coef_a(xq))
    if conv:
        tabs["b"] = convection(len(x) - 1)(xq)
    if react:
        tabs["c"] = helmholtz(xq) if react == "helmholtz" else reaction(xq)
    return tabs


def peclet(x, tabs):
    _, w = gauss01(tabs["f"].shape[1])
    return float(np.max(np.abs(tabs["b"] @ w) * np.diff(x) / (2.0 * (tabs["a"] @ w))))


def goal_load(x, nq):
    """p of J(u) = int j u_h dx: the P1 load of the density by the nq-point rule of the assembly."""
    return assemble(x, goal_density(quad_points(x, nq)))[3]


def observations(x, n=9, seed=11):
    """(x_obs, d_obs): points strictly inside the mesh and data of size 1."""
    rng = np.random.default_rng(seed)
    xo = np.sort(-0.95 + 1.9 * rng.random(n))
    return xo, np.cos(2.0 * xo)


def functional(x, kind, nq=2):
    if kind == "goal":
        return Linear(goal_load(x, nq))
    if kind == "observe":
        return Misfit(*observations(x))
    return Linear(np.random.default_rng(5).standard_normal(len(x)))       # "random": any nodal p


def reading(x, tabs, kinds, J, kappa=KAPPA, g=END_DATA):
    """(deviation of the adjoint gradients from the complex step, the adjoint dict, the complex-step dict)."""
    adj = adjoint_gradients(x, tabs, kinds, kappa, g, J)
    cs = complex_step(x, tabs, kinds, kappa, g, J)
    return deviation(adj, cs), adj, cs


# ---- the inverse problem ------------------------------------------------------------------------------------------------
DEMO_NE, DEMO_STEPS, DEMO_RATE = 16, 20, 0.04


def demo_truth(ne=DEMO_NE):
    """(x, a_true [ne], f table [ne, 2], nodal data d): -(a u')' = 1 on [0, 1], u = 0 at both ends."""
    x = np.linspace(0.0, 1.0, ne + 1)
    mid = 0.5 * (x[:-1] + x[1:])
    a_true = 1.0 + 0.5 * np.sin(2.0 * np.pi * mid)
    f = np.ones((ne, 2))
    d = primal(x, dict(f=f, a=np.repeat(a_true[:, None], 2, axis=1)), (DIRICHLET,) * 2, (0.0, 0.0), (0.0, 0.0))[0]
    return x, a_true, f, d


def demo(steps=DEMO_STEPS, rate=DEMO_RATE):
    """Plain gradient descent on theta = log a_e from a = 1, J = 1/2 |u - d|^2 over the nodes, scaled by 1 / J(a = 1)
    so that the rate is a plain number: theta -= rate grad (J / J_0).  Returns the misfits J_0 .. J_steps."""
    x, _, f, d = demo_truth()
    J = Misfit(x, d)
    theta = np.zeros(DEMO_NE)
    hist, j0 = [], None
    for _ in range(steps + 1):
        a = np.repeat(np.exp(theta)[:, None], 2, axis=1)
        r = adjoint_gradients(x, dict(f=f, a=a), (DIRICHLET,) * 2, (0.0, 0.0), (0.0, 0.0), J)
        j0 = r["value"] if j0 is None else j0
        hist.append(float(r["value"]))
        theta = theta - rate * (r["a"].sum(axis=1) * np.exp(theta)) / j0
    return hist


def main():
    print("adjoint gradients against the complex step (largest group-relative deviation)")
    for ne in (7, 33):
        x = mesh(ne)
        for conv, react in ((False, False), (True, True)):
            for nq in (1, 2, 5):
                tabs = case_tables(x, nq, conv, react)
                devs = [reading(x, tabs, kinds, functional(x, "random"))[0] for kinds in END_COMBOS]
                pe = f", Peclet {peclet(x, tabs):.2f}" if conv else ""
                print(f"  ne={ne:2d} nquad={nq} b,c={'yes' if conv else 'no '}: "
                      + " ".join(f"{d:.1e}" for d in devs) + "  (DD DR RD RR)" + pe)
        tabs = case_tables(x, 2, False, "helmholtz")
        print(f"  ne={ne:2d} nquad=2 Helmholtz c=-15, DR: "
              f"{reading(x, tabs, (DIRICHLET, ROBIN), functional(x, 'random'))[0]:.1e}")
        for kind in ("goal", "observe"):
            tabs = case_tables(x, 2, True, True)
            devs = [reading(x, tabs, kinds, functional(x, kind))[0] for kinds in END_COMBOS]
            print(f"  ne={ne:2d} nquad=2 b,c=yes {kind:7s}: " + " ".join(f"{d:.1e}" for d in devs))
    print("central differences (eps = 1e-6) against the complex step, Dirichlet-Robin, b and c, nquad = 2")
    for ne in (6, 33):
        x = mesh(ne)
        tabs = case_tables(x, 2, True, True)
        J = functional(x, "random")
        cs = complex_step(x, tabs, (DIRICHLET, ROBIN), KAPPA, END_DATA, J)
        cd = central_differences(x, tabs, (DIRICHLET, ROBIN), KAPPA, END_DATA, J)
        worst = max(float(np.max(np.abs(cd[k] - cs[k]))) for k in "abcf")
        print(f"  ne={ne:2d}: largest absolute deviation {worst:.1e}, largest gradient entry "
              f"{max(float(np.max(np.abs(cs[k]))) for k in 'abcf'):.2e}")
    hist = demo()
    print(f"inverse problem, {DEMO_NE} elements, {DEMO_STEPS} steps of gradient descent on log a (rate {DEMO_RATE})")
    print("  misfit: " + " ".join(f"{v:.3e}" for v in hist))
    print(f"  monotone: {all(b < a for a, b in zip(hist, hist[1:]))}, final / first = {hist[-1] / hist[0]:.3e}, "
          f"final = {hist[-1]:.6e}")


if __name__ == "__main__":
    main()
