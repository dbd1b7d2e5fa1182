"""numpy prototype of the adjoint sensitivities of the semilinear P1 solve of -(a u')' + b u' + c u + g(x, u) = f
(DESIGN.md section 35), g from the tabulated families of section 27: POLY g = sum_k q_k(x) u^k and EXP
g = q_0(x) exp(q_1(x) u).  On the dense assembly and solve of sensitivity_proto.py (section 31) it states

  the forward solve   the facade's damped Newton iteration in float64, on TABLES at the Gauss points: a step is the
                      linear problem with the reaction c + g_u(x, u_h) and the right-hand side f - g + g_u u_h;
  the adjoint         z of the TRANSPOSED Jacobian K + M(g_u(., u*_h)) at the converged u*, then the formulas of
                      csrc/lssvr_sens.hpp for a, b, c, f and the end data and those of csrc/lssvr_nl_sens.hpp for the
                      q_k, in their order of operations;
  the yardstick       the complex step.  From the converged real u* one datum is perturbed by i 1e-30 and full undamped
                      Newton steps run in complex arithmetic until the increment is below 1e-14 (g is analytic in u and
                      in its tables for both families); dJ/d(datum) = Im J / 1e-30, no subtraction.

Run as a script it prints what DESIGN.md section 35 records: the deviation of the adjoint gradients from the complex
step on the cases of tests/semilinear_sensitivity_rules.py, the control with g_u forgotten in the Jacobian, and a small
inverse problem -- 20 steps of plain gradient descent on the log of a piecewise-constant q_3 of -u'' + q_3 u^3 = f on 16 elements
from 9 observations.  No GPU, nothing but numpy."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sensitivity_proto as sp          # noqa: E402

DIRICHLET, ROBIN = sp.DIRICHLET, sp.ROBIN
POLY, EXP = 0, 1
CSTEP = sp.CSTEP
ARMIJO = 1e-4
KAPPA, END_DATA, END_COMBOS = sp.KAPPA, sp.END_DATA, sp.END_COMBOS


# ---- the family: g and g_u, analytic in u and in the tables ---------------------------------------------------------------
def g_and_gu(kind, q, uh):
    """(g, g_u) at the tables' points in the order of csrc/lssvr_nl_family.hpp: Horner for POLY, E = exp(q_1 u)."""
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


def interpolant(u, nq):
    """u_h at the Gauss points [ne, nq] as lssvr_nl_linearize forms it: u_e + (u_{e+1} - u_e) xi_q."""
    xi, _ = sp.gauss01(nq)
    return u[:-1, None] + (u[1:] - u[:-1])[:, None] * xi[None, :]


def linearize(tabs, kind, u):
    """(c_eff, f_eff, f_res) [ne, nq] of one Newton step around the nodal iterate u."""
    uh = interpolant(u, tabs["f"].shape[1])
    g, d = g_and_gu(kind, tabs["q"], uh)
    fr = tabs["f"] - g
    c = tabs.get("c")
    return (d if c is None else c + d), fr + d * uh, fr


def newton_step(x, tabs, kind, u, kinds, kappa, g):
    """(u_new, the raw bands of the Jacobian at u): the linear solve with c_eff and f_eff."""
    ce, fe, _ = linearize(tabs, kind, u)
    bands = sp.assemble(x, fe, tabs.get("a"), tabs.get("b"), ce)
    return sp.bc_solve(sp.dense(*bands[:3]), bands[3], kinds, kappa, g), bands


def residual(x, tabs, kind, v, kinds, kappa, g):
    """|R(v)|_inf, R(v) = K v + G(v) - F on the free rows (a Robin end row with kappa v - g, a Dirichlet row 0)."""
    fr = linearize(tabs, kind, v)[2]
    diag, sub, sup, load = sp.assemble(x, fr, tabs.get("a"), tabs.get("b"), tabs.get("c"))
    r = sp.dense(diag, sub, sup) @ v - load
    for s, end in ((0, 0), (1, -1)):
        r[end] = r[end] + (kappa[s] * v[end] - g[s]) if kinds[s] == ROBIN else 0.0
    return float(np.max(np.abs(r)))


def solve(x, tabs, kind, kinds, kappa=KAPPA, g=END_DATA, u_init=None, tol=1e-12, max_iter=30, max_halvings=8):
    """The facade's damped Newton iteration in float64 -> (u, dict(iterations, steps, lambdas)):
    the stop test |u_new - u| <= tol max(1, |u_new|) first, else lambda = 1, 1/2, ... until
    |R(u + lambda d)| <= (1 - 1e-4 lambda) |R(u)|, else the tried lambda with the smallest residual."""
    u = np.zeros(len(x)) if u_init is None else np.array(u_init, dtype=np.float64)
    for s, end in ((0, 0), (1, -1)):
        if kinds[s] == DIRICHLET:
            u[end] = g[s]
    rep = dict(iterations=0, steps=[], lambdas=[])
    for it in range(1, max_iter + 1):
        u_new = newton_step(x, tabs, kind, u, kinds, kappa, g)[0]
        step, size = float(np.max(np.abs(u_new - u))), float(np.max(np.abs(u_new)))
        if not (math.isfinite(step) and math.isfinite(size)):
            raise RuntimeError(f"Newton iteration {it} produced non-finite values")
        rep["iterations"] = it
        rep["steps"].append(step)
        if step <= tol * max(1.0, size):
            rep["lambdas"].append(1.0)
            return u_new, rep
        r0 = residual(x, tabs, kind, u, kinds, kappa, g)
        lam, tried = 1.0, []
        for _ in range(max_halvings + 1):
            v = u_new if lam == 1.0 else u + lam * (u_new - u)
            rv = residual(x, tabs, kind, v, kinds, kappa, g)
            tried.append((rv, lam, v))
            if rv <= (1.0 - ARMIJO * lam) * r0:
                break
            lam *= 0.5
        else:
            rv, lam, v = min(tried, key=lambda t: t[0])
        u = v
        rep["lambdas"].append(lam)
    raise RuntimeError(f"the Newton iteration did not converge in {max_iter} iterations: {rep}")


# ---- the adjoint, in the order of csrc/lssvr_sens.hpp and csrc/lssvr_nl_sens.hpp -------------------------------------
def nl_gradients(x, U, Z, nq, kind, nterm, q_tabs=None):
    """gq [nc, nterm, ne, nq] of the pairs (U[j], Z[j]) (U [1, ne+1]: one primal for all cases).  Every operation in the
    order of nl_sens_entry, one rounding each: bit for bit the library's values for POLY, and for EXP up to exp."""
    xi, w = sp.gauss01(nq)
    U, Z = np.atleast_2d(U), np.atleast_2d(Z)
    U = np.broadcast_to(U, Z.shape)
    h = (x[1:] - x[:-1])[None, :, None]
    xi, w = xi[None, None, :], w[None, None, :]
    u0, u1, z0, z1 = (t[:, :, None] for t in (U[:, :-1], U[:, 1:], Z[:, :-1], Z[:, 1:]))
    om, hw = 1.0 - xi, h * w
    s = hw * (z0 * om + z1 * xi)
    uq = u0 * om + u1 * xi
    if kind == EXP:
        E = np.exp(q_tabs[1][None] * uq)
        return np.stack([-(s * E), -(s * ((q_tabs[0][None] * uq) * E))], axis=1)
    out, pk = [-s], np.ones_like(uq)
    for _ in range(1, nterm):
        pk = pk * uq
        out.append(-(s * pk))
    return np.stack(out, axis=1)


def adjoint_gradients(x, tabs, kind, kinds, kappa, g, J, forget_gu=False):
    """dict(a=, b=, c=, f= [ne, nq], q= [nterm, ne, nq], ends= [4], value=, u=, z=, p=, newton=) by ONE Newton solve,
    ONE linearisation at u* and ONE adjoint solve.  ``forget_gu``: the control -- z from K^T alone."""
    nq = tabs["f"].shape[1]
    u, rep = solve(x, tabs, kind, kinds, kappa, g)
    ce = tabs.get("c") if forget_gu else linearize(tabs, kind, u)[0]
    bands = sp.assemble(x, tabs["f"], tabs.get("a"), tabs.get("b"), ce)
    p = J.gradient(x, u)
    z = sp.adjoint(sp.dense(*bands[:3]), p, kinds, kappa)
    ga, gb, gc, gf = (t[0] for t in sp.table_gradients(x, u, z, nq))
    gq = nl_gradients(x, u, z, nq, kind, len(tabs["q"]), tabs["q"])[0]
    ends = sp.end_gradients(u, z, p, (bands[1][0], bands[2][-1]), kinds)[0]
    return dict(a=ga, b=gb, c=gc, f=gf, q=gq, ends=ends, value=J.value(x, u), u=u, z=z, p=p, newton=rep)


# ---- the yardstick ----------------------------------------------------------------------------------------------------
def _full(tabs):
    shape = tabs["f"].shape
    return dict(a=np.ones(shape) if tabs.get("a") is None else tabs["a"],
                b=np.zeros(shape) if tabs.get("b") is None else tabs["b"],
                c=np.zeros(shape) if tabs.get("c") is None else tabs["c"], f=tabs["f"], q=tabs["q"])


def complex_newton(x, tabs, kind, u, kinds, kappa, g, tol=1e-14, max_iter=10):
    """Full undamped Newton steps in complex arithmetic from the (real, converged) u until |u_new - u|_inf < tol."""
    u = np.asarray(u, dtype=complex)
    for _ in range(max_iter):
        u_new = newton_step(x, tabs, kind, u, kinds, kappa, g)[0]
        inc = float(np.max(np.abs(u_new - u)))
        u = u_new
        if inc < tol:
            return u
    raise RuntimeError("the complex Newton steps did not settle")


def complex_step(x, tabs, kind, kinds, kappa, g, J, u):
    """The gradients of :func:`adjoint_gradients` (a, b, c, f, q, ends) by Im J(theta + i 1e-30 delta) / 1e-30, one
    complex Newton run from the converged ``u`` per datum."""
    full = _full(tabs)
    out = {}
    for name in ("a", "b", "c", "f", "q"):
        grad = np.zeros(full[name].shape)
        for idx in np.ndindex(*grad.shape):
            t = {k: v.astype(complex) if k == name else v for k, v in full.items()}
            t[name][idx] += 1j * CSTEP
            grad[idx] = J.value(x, complex_newton(x, t, kind, u, kinds, kappa, g)).imag / CSTEP
        out[name] = grad
    ends = np.zeros(4)
    for s in range(2):
        gg = np.array(g, dtype=complex)
        gg[s] += 1j * CSTEP
        ends[s] = J.value(x, complex_newton(x, full, kind, u, kinds, kappa, gg)).imag / CSTEP
        if kinds[s] == ROBIN:
            kk = np.array(kappa, dtype=complex)
            kk[s] += 1j * CSTEP
            ends[2 + s] = J.value(x, complex_newton(x, full, kind, u, kinds, kk, g)).imag / CSTEP
    out["ends"] = ends
    return out


def groups(grads):
    """The groups of the reading: a, b, c, f, every q_k on its own, the end data (None where ``grads`` has none)."""
    out = {k: grads.get(k) for k in ("a", "b", "c", "f", "ends")}
    if grads.get("q") is not None:
        out.update({f"q{k}": t for k, t in enumerate(grads["q"])})
    return out


def deviation(got, want):
    """The largest deviation of the gradients ``got`` from ``want`` over the groups (those that ``got`` holds), each
    relative to the largest entry of its group in ``want``."""
    worst, want = 0.0, groups(want)
    for k, t in groups(got).items():
        if t is None:
            continue
        scale = float(np.max(np.abs(want[k])))
        err = float(np.max(np.abs(np.asarray(t) - want[k])))
        worst = max(worst, err / scale if scale > 0.0 else err)
    return worst


def reading(x, tabs, kind, kinds, J, kappa=KAPPA, g=END_DATA):
    """(deviation of the adjoint gradients from the complex step, the adjoint dict, the complex-step dict)."""
    adj = adjoint_gradients(x, tabs, kind, kinds, kappa, g, J)
    cs = complex_step(x, tabs, kind, kinds, kappa, g, J, adj["u"])
    return deviation(adj, cs), adj, cs


# ---- the cases: callables, so that the facade can be handed the same problem ----------------------------------------------
def _const(v):
    return lambda x: float(v) + 0.0 * np.asarray(x, dtype=np.float64)


def zero(x):
    return 0.0 * np.asarray(x, dtype=np.float64)


# law -> (kind, [q_k(x)]).  "cubic": q_3 = 1 + x^2 / 2 > 0 carries the problem, q_1 takes both signs; "poly1": g = q_0(x),
# a source (g_u = 0); "poly6": every power up to u^5; "bratu": -u'' - e^u = 0, where c + g_u < 0
LAWS = {
    "cubic": (POLY, [lambda x: 0.2 * np.cos(x), lambda x: 0.4 * np.sin(2.0 * x), lambda x: 0.1 * x,
                     lambda x: 1.0 + 0.5 * x * x]),
    "poly1": (POLY, [lambda x: 0.5 * np.cos(2.0 * x)]),
    "poly6": (POLY, [_const(0.1), lambda x: 0.3 * np.cos(x), lambda x: 0.1 * np.sin(x), _const(0.5),
                     lambda x: 0.05 * x, _const(0.2)]),
    "bratu": (EXP, [_const(-1.0), _const(1.0)]),
}


def mesh(ne, law):
    """The non-uniform meshes of sensitivity_proto on [-1, 1]; Bratu's on (0, 1)."""
    x = sp.mesh(ne)
    return 0.5 * (x + 1.0) if law == "bratu" else x


def case_tables(x, nq, conv, react, law):
    """(kind, tables): f, a, b, c of sensitivity_proto's cases (Bratu: f = 0 and a = 1, no b, no c) and q [nterm, ne,
    nq] of the law at the Gauss points."""
    kind, q = LAWS[law]
    xq = sp.quad_points(x, nq)
    tabs = dict(f=zero(xq)) if law == "bratu" else sp.case_tables(x, nq, conv, react)
    tabs["q"] = np.stack([np.broadcast_to(fn(xq), xq.shape) for fn in q])
    return kind, tabs


def observations(x, n=9, seed=11):
    """(x_obs, d_obs): points strictly inside the mesh (sensitivity_proto's on [-1, 1]) and data of size 1."""
    t = np.sort(np.random.default_rng(seed).random(n))
    xo = x[0] + (x[-1] - x[0]) * (0.025 + 0.95 * t)
    return xo, np.cos(2.0 * xo)


def goal_density(x):
    return sp.goal_density(x)


def functional(x, name, nq=2):
    if name == "goal":
        return sp.Linear(sp.assemble(x, goal_density(sp.quad_points(x, nq)))[3])
    if name == "observe":
        return sp.Misfit(*observations(x))
    return sp.Linear(np.random.default_rng(5).standard_normal(len(x)))       # "random": any nodal p


# ---- the inverse problem ------------------------------------------------------------------------------------------------
DEMO_NE, DEMO_STEPS, DEMO_RATE, DEMO_START = 16, 20, 1.0, 2.0


def demo_q3_true(x):
    return 1.0 + 0.5 * np.sin(math.pi * x)


def demo_rhs(x):
    s = np.sin(math.pi * x)
    return math.pi ** 2 * s + 2.0 * s ** 3


def demo_tables(x, q3):
    """The tables of -u'' + q_3 u^3 = f with q_3 = q3[e] on element e (nquad 2)."""
    xq = sp.quad_points(x, 2)
    q3 = np.broadcast_to(np.asarray(q3, dtype=np.float64)[:, None], xq.shape)
    return dict(f=demo_rhs(xq), q=np.stack([zero(xq), zero(xq), zero(xq), q3]))


def demo_truth(ne=DEMO_NE):
    """(x, q_3 of the truth per element, (x_obs, d_obs)): -u'' + q_3 u^3 = f on [-1, 1], u = 0 at both ends, 9 points
    inside the mesh with the values of the truth's P1 solution there."""
    x = np.linspace(-1.0, 1.0, ne + 1)
    q3 = demo_q3_true(0.5 * (x[:-1] + x[1:]))
    u = solve(x, demo_tables(x, q3), POLY, (DIRICHLET,) * 2, (0.0, 0.0), (0.0, 0.0))[0]
    xo = observations(x)[0]
    e, t = sp.hat_weights(x, xo)
    return x, q3, (xo, u[e] * (1 - t) + u[e + 1] * t)


def demo(steps=DEMO_STEPS, rate=DEMO_RATE):
    """Plain gradient descent on theta_e = log q_3 on element e (so q_3 stays positive and the unpivoted solve applies)
    from q_3 = 2, J = 1/2 sum (u_h(x_i) - d_i)^2, scaled by 1 / J(q_3 = 2) so that the rate is a plain number:
    theta -= rate grad (J / J_0).  Returns the misfits J_0 .. J_steps."""
    x, _, obs = demo_truth()
    J = sp.Misfit(*obs)
    theta = np.full(DEMO_NE, math.log(DEMO_START))
    hist, j0 = [], None
    for _ in range(steps + 1):
        r = adjoint_gradients(x, demo_tables(x, np.exp(theta)), POLY, (DIRICHLET,) * 2, (0.0, 0.0), (0.0, 0.0), J)
        j0 = r["value"] if j0 is None else j0
        hist.append(float(r["value"]))
        theta = theta - rate * (r["q"][3].sum(axis=1) * np.exp(theta)) / j0
    return hist


def main():
    print("adjoint gradients against the complex step (largest group-relative deviation; DD DR RD RR)")
    for ne in (7, 33):
        for conv in (False, True):
            for nq in (1, 2, 5):
                x = mesh(ne, "cubic")
                kind, tabs = case_tables(x, nq, conv, conv, "cubic")
                devs = [reading(x, tabs, kind, kinds, functional(x, "random"))[0] for kinds in END_COMBOS]
                print(f"  cubic ne={ne:2d} nquad={nq} b,c={'yes' if conv else 'no '}: "
                      + " ".join(f"{d:.1e}" for d in devs))
        for law in ("poly1", "poly6", "bratu"):
            x = mesh(ne, law)
            kind, tabs = case_tables(x, 2, False, law != "bratu", law)
            # (Bratu with a Robin end on the left has no solution for this data: DD and DR only)
            combos = END_COMBOS[:2] if law == "bratu" else END_COMBOS
            devs = [reading(x, tabs, kind, kinds, functional(x, "random"))[0] for kinds in combos]
            print(f"  {law} ne={ne:2d} nquad=2: " + " ".join(f"{d:.1e}" for d in devs))
    x = mesh(33, "cubic")
    kind, tabs = case_tables(x, 2, True, True, "cubic")
    J = functional(x, "goal")
    read, _, cs = reading(x, tabs, kind, (DIRICHLET, ROBIN), J)
    wrong = deviation(adjoint_gradients(x, tabs, kind, (DIRICHLET, ROBIN), KAPPA, END_DATA, J, forget_gu=True), cs)
    print(f"control, cubic ne=33 nquad=2 b,c DR goal: the adjoint reads {read:.1e}, with g_u forgotten {wrong:.1e}")
    hist = demo()
    print(f"inverse problem, {DEMO_NE} elements, {DEMO_STEPS} steps of gradient descent on log q_3 (rate {DEMO_RATE})")
    print("  misfit: " + " ".join(f"{v:.3e}" for v in hist))
    print(f"  monotone: {all(b < a for a, b in zip(hist, hist[1:]))}, final / first = {hist[-1] / hist[0]:.3e}, "
          f"final = {hist[-1]:.6e}")


if __name__ == "__main__":
    main()
