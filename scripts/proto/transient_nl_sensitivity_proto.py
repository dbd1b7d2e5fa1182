"""numpy prototype of the adjoint sensitivities of the semilinear BDF loop of rho u_t - (a u')' + c u + g(x, u) = f(x, t)
(DESIGN.md section 36), g from the tabulated families of section 27.  On the dense pieces of
transient_sensitivity_proto.py (section 32) and semilinear_sensitivity_proto.py (section 35) it states

  the forward loop    solve_transient(..., nonlinear=...) in float64: per step ``iters`` Newton iterations from the
                      extrapolation 2 u^n - u^{n-1} (BDF1 and the first step: u^n), each the linear problem with the
                      reaction c + alpha rho / dt + g_u(x, v_h) and the right-hand side r + L(-g + g_u v_h);
  the adjoint         of the CONVERGED implicit step: J_n = K + M(c + alpha_n rho / dt + g_u(., u^n_h)) AT u^n,
                      B_n = p_n + (1/dt) M (beta0_{n+1} lam^{n+1} + beta1_{n+2} lam^{n+2}), J_n lam^n = B_n, and the sums
                      over time in the order of csrc/lssvr_chunk_sens.hpp, those of the q_k included;
  the yardstick       the complex step through the WHOLE loop: one datum perturbed by i 1e-30 and every step's Newton
                      iteration run in complex arithmetic until its increment is below 1e-14 (g is analytic in u and
                      in its tables); dJ/d(datum) = Im J / 1e-30, no subtraction.

Run as a script it prints what DESIGN.md section 36 records: the readings on the cases of
tests/transient_nl_sensitivity_rules.py, the control with g_u left out of J_n, the increment of the non-converging case
and a small inverse problem -- a piecewise-constant q_3 of u_t - u'' + q_3 u^3 = f on 16 elements from observations at
two steps, by 20 steps of gradient descent on log q_3.  No GPU, nothing but numpy."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import semilinear_sensitivity_proto as nlp          # noqa: E402
import transient_sensitivity_proto as tsp           # noqa: E402

sp = tsp.sp
DIRICHLET, ROBIN = sp.DIRICHLET, sp.ROBIN
POLY, EXP = nlp.POLY, nlp.EXP
CSTEP, CHUNK, BDF = sp.CSTEP, tsp.CHUNK, tsp.BDF
coefficients, adjoint_betas = tsp.coefficients, tsp.adjoint_betas
CONVERGED, MAX_NEWTON = 1e-14, 50


class Problem(tsp.Problem):
    """tsp.Problem and the law: ``kind`` (POLY / EXP) and its tables q [nterm, ne, nq] at the Gauss points."""

    def __init__(self, base, kind, q):
        super().__init__(base.x, base.a, base.c, base.rho, base.f, base.phi, base.g, base.kappa, base.kinds, base.u0,
                         base.dt, base.scheme)
        self.kind, self.q = kind, q

    def replace(self, **kw):
        p = Problem(self, self.kind, self.q)
        for k, v in kw.items():
            setattr(p, k, v)
        return p


# ---- the forward loop, dense; real or complex -------------------------------------------------------------------------------
def mass_and_loads(p):
    zero = np.zeros(p.a.shape)
    md, msub, msup, _ = sp.assemble(p.x, zero, zero, None, p.rho)
    return sp.dense(md, msub, msup), np.stack([sp.assemble(p.x, fr)[3] for fr in p.f])


def jacobian(p, al, v, with_gu=True):
    """(dense J, raw bands, g, g_u) of K + M(c + al rho / dt + g_u(., v_h)) at the nodal v."""
    uh = nlp.interpolant(v, p.nq)
    g, d = nlp.g_and_gu(p.kind, p.q, uh)
    cs = p.c + al * p.rho / p.dt
    bands = sp.assemble(p.x, (0.0 - g) + d * uh, p.a, None, cs + d if with_gu else cs)
    return sp.dense(*bands[:3]), bands


def forward(p, iters=None, guess=None):
    """(U [N+1, ne+1], dv [N, iterations run]): the loop of solve_transient(..., nonlinear=...).  ``iters``: the fixed
    Newton count of the facade; None: every step runs until its increment is below 1e-14 (the converged implicit step).
    ``guess`` [N+1, ne+1]: the start of step n is guess[n] instead of the extrapolation."""
    M, loads = mass_and_loads(p)
    dt = np.result_type(M, loads, p.a, p.c, p.q, p.phi, p.g, np.asarray(p.kappa), p.u0)
    U = np.zeros((p.N + 1, len(p.x)), dtype=dt)
    U[0] = p.u0
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == DIRICHLET:
            U[0, end] = p.g[0, s]
    incs = []
    for n in range(1, p.N + 1):
        al, b0, b1 = coefficients(p.scheme, n, p.N)
        w = b0 * U[n - 1] if b1 == 0.0 else b0 * U[n - 1] + b1 * U[n - 2]
        r = (1.0 / p.dt) * (M @ w) + p.phi[n - 1] @ loads
        if guess is not None:
            v = guess[n].astype(dt)
        else:
            v = U[n - 1].copy() if b1 == 0.0 else U[n - 2] + 2.0 * (U[n - 1] - U[n - 2])
        inc = []
        for it in range(MAX_NEWTON if iters is None else iters):
            J, bands = jacobian(p, al, v)
            v_new = sp.bc_solve(J, r + bands[3], p.kinds, p.kappa, p.g[n])
            inc.append(float(np.max(np.abs(v_new - v))))
            v = v_new
            if iters is None and inc[-1] < CONVERGED:
                break
        else:
            if iters is None:
                raise RuntimeError(f"step {n}: the Newton iteration did not settle ({inc})")
        U[n] = v
        incs.append(inc)
    return U, incs


# ---- the backward loop and the sums over time, in the kernels' order --------------------------------------------------------
def backward(p, U, P, with_gu=True):
    """(lam [N+3, ne+1], B [N+1, ne+1], band_ends [N+1, 2]): J_n AT u^n (``with_gu`` False: the control, g_u left out),
    row n of band_ends = {off[0], off[ne-1]} of J_n."""
    M, _ = mass_and_loads(p)
    N = p.N
    lam, B, be = np.zeros((N + 3, len(p.x))), np.zeros((N + 1, len(p.x))), np.zeros((N + 1, 2))
    for n in range(N, -1, -1):
        b0, b1 = adjoint_betas(p.scheme, n, N)
        v = b0 * lam[n + 1] if b1 == 0.0 else b0 * lam[n + 1] + b1 * lam[n + 2]
        B[n] = (1.0 / p.dt) * (M @ v) + 1.0 * P[n]
        if n >= 1:
            J, bands = jacobian(p, coefficients(p.scheme, n, N)[0], U[n], with_gu)
            be[n] = bands[1][0], bands[2][-1]
            lam[n] = sp.bc_solve(J.T, B[n], p.kinds, p.kappa, (0.0, 0.0))
    return lam, B, be


def chunk_gq(x, nq, Utraj, Z, n0, kind, nterm, q_tabs=None, init=None):
    """gq [nterm, ne, nq] of the chunk of m = len(Z) levels n0 .. n0+m-1 (row i of Z: level n0+m-1-i), continued from
    ``init`` or from 0: every operation in the order of ChunkNlGq (csrc/lssvr_chunk_sens.hpp), one rounding each."""
    xi, w = sp.gauss01(nq)
    ne, m = len(x) - 1, len(Z)
    hw = (x[1:] - x[:-1])[:, None] * w[None, :]
    xi = xi[None, :]
    om = 1.0 - xi
    gq = np.zeros((nterm, ne, int(nq))) if init is None else np.array(init, dtype=np.float64)
    for i in range(m):
        u = Utraj[n0 + m - 1 - i]
        s = hw * (Z[i][:-1, None] * om + Z[i][1:, None] * xi)
        uq = u[:-1, None] * om + u[1:, None] * xi
        if kind == EXP:
            E = np.exp(q_tabs[1] * uq)
            gq[0] = gq[0] - (s * E)
            gq[1] = gq[1] - (s * ((q_tabs[0] * uq) * E))
        else:
            gq[0] = gq[0] - s
            pk = np.ones_like(uq)
            for k in range(1, nterm):
                pk = pk * uq
                gq[k] = gq[k] - (s * pk)
    return gq


def sweep_gradients(p, U, lam, B, be, size=CHUNK):
    """The gradient dict of a whole sweep in chunks of ``size`` levels: those of tsp.sweep_gradients with every level's
    own band_ends row, and q [nterm, ne, nq]."""
    N, R, inv_dt = p.N, p.f.shape[0], 1.0 / p.dt
    out_g = np.zeros((N + 1, 2))
    tabs = kap = gq = None
    for n0, m in tsp.chunks(N, size):
        steps = [n0 + m - 1 - i for i in range(m)]
        Z, Br = lam[steps], B[steps]
        coef = np.array([coefficients(p.scheme, n, N) for n in steps])
        tabs = tsp.chunk_tables(p.x, p.nq, U, Z, n0, inv_dt, coef, p.phi, R, tabs)
        gq = chunk_gq(p.x, p.nq, U, Z, n0, p.kind, len(p.q), p.q, gq)
        kap = tsp.chunk_ends(U, Z, Br, n0, be[steps], list(range(m)), p.kinds, out_g, kap)
    gu0 = B[0].copy()
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == DIRICHLET:
            out_g[0, s] = B[0][end]
            gu0[end] = 0.0
    return dict(tabs, q=gq, u0=gu0, g=out_g, kappa=kap)


def adjoint_gradients(p, J, iters=6, size=CHUNK, with_gu=True):
    """The gradient dict by ONE forward loop of ``iters`` Newton iterations per step and ONE backward loop, plus value,
    U, lam, B, P, newton (the increments)."""
    U, incs = forward(p, iters)
    P = J.gradient(p.x, U)
    lam, B, be = backward(p, U, P, with_gu)
    out = sweep_gradients(p, U, lam, B, be, size)
    out.update(value=float(J.value(p.x, U)), U=U, lam=lam, B=B, P=P, band_ends=be, newton=incs)
    return out


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def complex_step(p, J):
    """The same gradient dict by Im J(theta + i 1e-30 delta) / 1e-30: one loop per entry, every step's Newton iteration in
    complex arithmetic until its increment is below 1e-14, started at the converged real state of that step."""
    U = forward(p)[0]

    def run(**kw):
        q = p.replace(**kw)
        return J.value(q.x, forward(q, guess=U)[0]).imag / CSTEP

    out = {}
    for name in ("a", "c", "rho", "f", "q", "u0", "g"):
        base = np.asarray(getattr(p, name), dtype=np.float64)
        grad = np.zeros(base.shape)
        for idx in np.ndindex(*base.shape):
            t = base.astype(complex)
            t[idx] += 1j * CSTEP
            grad[idx] = run(**{name: t})
        out[name] = grad
    gk = np.zeros(2)
    for s in range(2):
        if p.kinds[s] == ROBIN:
            t = np.array(p.kappa, dtype=complex)
            t[s] += 1j * CSTEP
            gk[s] = run(kappa=t)
    out["kappa"] = gk
    for s, end in ((0, 0), (1, -1)):          # (a Dirichlet end starts at g(t_0): u0 does not reach it)
        if p.kinds[s] == DIRICHLET:
            out["u0"][end] = 0.0
    return out


def groups(grads):
    """The groups of the reading: a, c, rho, every f_r and every q_k on its own, u0, the end values g, kappa."""
    out = {k: grads.get(k) for k in ("a", "c", "rho", "u0", "g", "kappa")}
    for name in ("f", "q"):
        if grads.get(name) is not None:
            out.update({f"{name}{k}": t for k, t in enumerate(grads[name])})
    return out


def deviations(got, want):
    """Per group, the largest deviation of ``got`` from ``want`` relative to the group's largest entry in ``want``
    (absolute where that is 0: kappa at two Dirichlet ends)."""
    out, want = {}, groups(want)
    for k, t in groups(got).items():
        if t is None:
            continue
        scale = float(np.max(np.abs(want[k])))
        err = float(np.max(np.abs(np.asarray(t) - want[k])))
        out[k] = err / scale if scale > 0.0 else err
    return out


def reading(case, iters=6):
    """(the reading: the largest group deviation of the adjoint gradients from the complex step; the adjoint dict; the
    complex-step dict) of ``case`` = (Problem, functional)."""
    p, J = case
    adj = adjoint_gradients(p, J, iters)
    cs = complex_step(p, J)
    return max(deviations(adj, cs).values()), adj, cs


# ---- the cases: callables, so that the facade can be handed the same problem ------------------------------------------------
# "cubic", "poly1", "poly6": the laws of section 35; "exp": g = q_0 exp(q_1 u) with q_0 > 0 and q_1 > 0, so g_u > 0 and
# c + alpha rho / dt + g_u >= 0 holds on "bands"; "linear": g = c0(x) u, the linear limit
LAWS = dict(nlp.LAWS)
LAWS["exp"] = (EXP, [lambda x: 0.5 + 0.2 * np.cos(x), lambda x: 0.6 + 0.1 * x])
LAWS["linear"] = (POLY, [nlp.zero, lambda x: 0.5 + 0.25 * x])


def problem(law, ne, nq, kinds, scheme, N, t_end=tsp.T_END):
    """tsp.problem -- rho(x), c(x), a(x), two forcing terms with time-dependent phi, moving end data -- with ``law``."""
    base = tsp.problem(ne, nq, kinds, scheme, N, t_end)
    kind, q = LAWS[law]
    xq = sp.quad_points(base.x, nq)
    return Problem(base, kind, np.stack([np.broadcast_to(fn(xq), xq.shape) for fn in q]))


def functional(p, kind):
    """"goal": int (1 + x^2) u^n dx over the steps max(1, N // 3), max(1, 2 N // 3) and N with the weights 0.5, -1, 2
    (a goal over several steps; fewer where they coincide); "observe": tsp's misfit at 9 points and two steps."""
    if kind == "observe":
        return tsp.MisfitT(*tsp.observations(p.N))
    P = np.zeros((p.N + 1, len(p.x)))
    for n, w in zip(*goal_steps(p.N)):
        P[n] = w * sp.goal_load(p.x, p.nq)
    return tsp.LinearT(P)


def goal_steps(N):
    steps, wts = [], []
    for n, w in ((max(1, N // 3), 0.5), (max(1, 2 * N // 3), -1.0), (N, 2.0)):
        if n not in steps:
            steps.append(n)
            wts.append(w)
    return steps, wts


# ---- a step that does not converge: the cubic, one Newton iteration, a long step ---------------------------------------------
SLOW = dict(law="cubic", ne=33, nq=2, kinds=(DIRICHLET, ROBIN), scheme="bdf2", N=3, t_end=6.0, iters=1, tol=1e-10)


def slow_increment():
    """(step, |dv_last| / (tol max(1, |v|))) of the first step of the SLOW case whose last increment is above tolerance."""
    p = problem(SLOW["law"], SLOW["ne"], SLOW["nq"], SLOW["kinds"], SLOW["scheme"], SLOW["N"], SLOW["t_end"])
    U, incs = forward(p, SLOW["iters"])
    for n, inc in enumerate(incs, 1):
        ratio = inc[-1] / (SLOW["tol"] * max(1.0, float(np.max(np.abs(U[n])))))
        if ratio > 1.0:
            return n, ratio
    return None, 0.0


# ---- the inverse problem: a piecewise-constant q_3 of u_t - u'' + q_3 u^3 = f from observations at two steps ----------------
DEMO_NE, DEMO_N, DEMO_T, DEMO_OBS, DEMO_ITERS, DEMO_RATE, DEMO_START, DEMO_NEWTON = 16, 8, 0.4, (4, 8), 20, 1.0, 2.0, 6


def demo_problem(q3):
    """u_t - u'' + q_3 u^3 = f on [-1, 1], q_3 = q3[e] on element e, u = 0 at both ends, u(x, 0) = sin(pi x), the forcing
    of the steady demo of section 35 (nquad 2, BDF2)."""
    x = np.linspace(-1.0, 1.0, DEMO_NE + 1)
    xq = sp.quad_points(x, 2)
    one, zero = np.ones(xq.shape), np.zeros(xq.shape)
    q3 = np.broadcast_to(np.asarray(q3, dtype=np.float64)[:, None], xq.shape)
    base = tsp.Problem(x, one, zero, one, nlp.demo_rhs(xq)[None], np.ones((DEMO_N, 1)), np.zeros((DEMO_N + 1, 2)),
                       np.zeros(2), (DIRICHLET, DIRICHLET), demo_u0(x), DEMO_T / DEMO_N, "bdf2")
    return Problem(base, POLY, np.stack([zero, zero, zero, q3]))


def demo_u0(x):
    return 0.5 * np.sin(math.pi * x)


def demo_data():
    """(x, x_obs, d [2, nobs]): the values of the truth's trajectory at 9 points inside the mesh, at the steps DEMO_OBS."""
    p = demo_problem(nlp.demo_q3_true(0.5 * (np.linspace(-1.0, 1.0, DEMO_NE + 1)[:-1]
                                             + np.linspace(-1.0, 1.0, DEMO_NE + 1)[1:])))
    U = forward(p, DEMO_NEWTON)[0]
    xo = nlp.observations(p.x)[0]
    e, t = sp.hat_weights(p.x, xo)
    return p.x, xo, np.stack([U[n][e] * (1 - t) + U[n][e + 1] * t for n in DEMO_OBS])


def demo(gradient=None, iters=DEMO_ITERS, rate=DEMO_RATE):
    """Plain gradient descent on theta_e = log q_3 on element e from q_3 = 2, J the misfit, scaled by 1 / J(q_3 = 2) so
    that the rate is a plain number: theta -= rate grad (J / J_0).  ``gradient(q3, x_obs, d)`` -> (J, dJ/dq_3 [ne, nq]):
    the prototype's by default, the facade's in the GPU test.  Returns the misfits J_0 .. J_iters."""
    _, xo, d = demo_data()

    def proto_gradient(q3, xo, d):
        r = adjoint_gradients(demo_problem(q3), tsp.MisfitT(DEMO_OBS, xo, d), DEMO_NEWTON)
        return r["value"], r["q"][3]

    gradient = gradient or proto_gradient
    theta = np.full(DEMO_NE, math.log(DEMO_START))
    hist, j0 = [], None
    for _ in range(iters + 1):
        j, gq3 = gradient(np.exp(theta), xo, d)
        j0 = j if j0 is None else j0
        hist.append(float(j))
        theta = theta - rate * (np.asarray(gq3).sum(axis=1) * np.exp(theta)) / j0
    return hist


def main():
    D, R = DIRICHLET, ROBIN
    print("adjoint gradients of the semilinear BDF loop against the complex step through the whole loop (the reading)")
    rows = [("cubic", 7, 1, (D, D), "bdf1", 3, "goal"), ("cubic", 7, 2, (D, R), "bdf2", 3, "observe"),
            ("cubic", 7, 5, (R, D), "bdf2", 11, "goal"), ("cubic", 7, 2, (R, R), "bdf1", 11, "observe"),
            ("poly1", 7, 2, (D, R), "bdf2", 3, "goal"), ("poly6", 7, 2, (R, D), "bdf2", 3, "observe"),
            ("exp", 7, 2, (R, R), "bdf2", 11, "goal"), ("cubic", 33, 2, (D, R), "bdf2", 11, "goal"),
            ("exp", 33, 2, (R, D), "bdf2", 11, "observe")]
    for law, ne, nq, kinds, scheme, N, fn in rows:
        p = problem(law, ne, nq, kinds, scheme, N)
        read, adj, _ = reading((p, functional(p, fn)))
        print(f"  {law:6s} ne={ne:2d} nquad={nq} {''.join('DR'[k] for k in kinds)} {scheme} N={N:2d} {fn:7s}: {read:.1e}"
              f"   (largest last increment {max(i[-1] for i in adj['newton']):.1e})")
    p = problem("cubic", 33, 2, (D, R), "bdf2", 11)
    J = functional(p, "goal")
    read, _, cs = reading((p, J))
    wrong = max(deviations(adjoint_gradients(p, J, with_gu=False), cs).values())
    print(f"control, cubic ne=33 nquad=2 DR bdf2 N=11 goal: the adjoint reads {read:.1e}, with g_u left out of J_n "
          f"{wrong:.1e}")
    n, ratio = slow_increment()
    print(f"one Newton iteration, t_end = {SLOW['t_end']}, N = {SLOW['N']}: step {n} ends {ratio:.1e} x above "
          f"newton_tol = {SLOW['tol']:g}")
    hist = demo()
    print(f"inverse problem, {DEMO_NE} elements, {DEMO_N} BDF2 steps to t = {DEMO_T}, observations at steps {DEMO_OBS}, "
          f"{DEMO_ITERS} steps of gradient descent on log q_3 (rate {DEMO_RATE})")
    print("  misfit: " + " ".join(f"{v:.3e}" for v in hist))
    print(f"  monotone: {all(b < a for a, b in zip(hist, hist[1:]))}, final / first = {hist[-1] / hist[0]:.3e}, "
          f"final = {hist[-1]:.6e}")


if __name__ == "__main__":
    main()
