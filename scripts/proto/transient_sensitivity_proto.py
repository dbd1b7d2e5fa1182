"""numpy prototype of the adjoint sensitivities of the BDF loop of rho u_t - (a u')' + c u = f(x, t) (DESIGN.md section
32): the dense forward loop of section 26 (real or complex), the complex-step derivative of a functional
J = J(u^1 .. u^N) with respect to every datum -- the tables a, c, rho, f_r at the Gauss points, the initial state and the
end data g(t_n), kappa -- by Im J(theta + i 1e-30 delta) / 1e-30 (no subtraction, so no cancellation), the backward loop
and the sums over time that csrc/lssvr_chunk_sens.hpp evaluates, in its order of operations.  No GPU, nothing but numpy.

Run as a script it prints what DESIGN.md section 32 records: the deviation of the adjoint gradients from the complex
step per group on the cases of tests/transient_sensitivity_rules.py, what a wrong pair of adjoint coefficients reads, and
a small inverse problem -- the initial state of the heat equation from two snapshots by 20 steps of gradient descent."""
import numpy as np

import sensitivity_proto as sp

DIRICHLET, ROBIN = sp.DIRICHLET, sp.ROBIN
CSTEP = sp.CSTEP
BDF = {"bdf1": (1.0, 1.0, 0.0), "bdf2": (1.5, 2.0, -0.5)}
CHUNK = 8


def coefficients(scheme, n, N):
    """(alpha_n, beta0_n, beta1_n) of step n: BDF1 for step 1, the scheme's after it, zeros beyond N (there is no such
    step: the adjoint's lambda^{N+1} = lambda^{N+2} = 0 need no coefficient)."""
    if n > N:
        return 0.0, 0.0, 0.0
    return BDF["bdf1"] if n == 1 else BDF[scheme]


def adjoint_betas(scheme, n, N):
    """(beta0_{n+1}, beta1_{n+2}): the coefficients of the adjoint right-hand side B_n."""
    return coefficients(scheme, n + 1, N)[1], coefficients(scheme, n + 2, N)[2]


# ---- the problem and the forward loop, dense; real or complex --------------------------------------------------------------
class Problem:
    """The data of one loop: x [ne+1], tables a, c, rho [ne, nq] and f [R, ne, nq] at the Gauss points, phi [N, R] (row
    n-1 = phi(t_n): the layout solve_transient uploads), g [N+1, 2] the end data at t_0 .. t_N, kappa [2], kinds, u0
    [ne+1], dt, N, scheme."""

    def __init__(self, x, a, c, rho, f, phi, g, kappa, kinds, u0, dt, scheme):
        self.x, self.a, self.c, self.rho, self.f = x, a, c, rho, f
        self.phi, self.g, self.kappa, self.kinds, self.u0 = phi, g, kappa, tuple(kinds), u0
        self.dt, self.scheme, self.N = dt, scheme, phi.shape[0]
        self.nq = a.shape[1]

    def replace(self, **kw):
        p = Problem(self.x, self.a, self.c, self.rho, self.f, self.phi, self.g, self.kappa, self.kinds, self.u0,
                    self.dt, self.scheme)
        for k, v in kw.items():
            setattr(p, k, v)
        return p


def matrices(p):
    """(M, {alpha: A_alpha}, loads [R, ne+1]) dense: M the mass matrix of rho, A_alpha = K + (alpha / dt) M as ONE
    assembly with the reaction table c + alpha rho / dt (what solve_transient does), L_r the P1 load of f_r."""
    zero = np.zeros(p.a.shape)
    md, msub, msup, _ = sp.assemble(p.x, zero, zero, None, p.rho)
    A = {}
    for al in {BDF["bdf1"][0], BDF[p.scheme][0]}:
        A[al] = sp.dense(*sp.assemble(p.x, zero, p.a, None, p.c + al * p.rho / p.dt)[:3])
    loads = np.stack([sp.assemble(p.x, fr)[3] for fr in p.f])
    return sp.dense(md, msub, msup), A, loads


def forward(p):
    """U [N+1, ne+1]: u^0 = u0 with g(t_0) at a Dirichlet end, then the loop of section 26."""
    M, A, loads = matrices(p)
    dt = np.result_type(M, *A.values(), loads, p.phi, p.g, np.asarray(p.kappa), p.u0)
    U = np.zeros((p.N + 1, len(p.x)), dtype=dt)
    U[0] = p.u0
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == DIRICHLET:
            U[0, end] = p.g[0, s]
    for n in range(1, p.N + 1):
        al, b0, b1 = coefficients(p.scheme, n, p.N)
        v = b0 * U[n - 1] if b1 == 0.0 else b0 * U[n - 1] + b1 * U[n - 2]
        rhs = (1.0 / p.dt) * (M @ v) + p.phi[n - 1] @ loads
        U[n] = sp.bc_solve(A[al], rhs, p.kinds, p.kappa, p.g[n])
    return U


# ---- functionals of the trajectory: J(U), analytic in U, and p_n = dJ/du^n (p_0 = 0) --------------------------------------
class LinearT:
    """J = sum_n P[n] . u^n for nodal rows P [N+1, ne+1], P[0] = 0."""

    def __init__(self, P):
        self.P = np.asarray(P, dtype=np.float64)
        assert not self.P[0].any()

    def value(self, x, U):
        return np.sum(self.P * U)

    def gradient(self, x, U):
        return self.P.copy()


class MisfitT:
    """J = 1/2 sum_k sum_i (u^{n_k}(x_i) - d_ki)^2 at the steps n_k; the residuals scatter through the hat functions."""

    def __init__(self, steps, xo, d):
        self.steps, self.one = list(steps), [sp.Misfit(xo, dk) for dk in np.atleast_2d(d)]

    def value(self, x, U):
        return sum(m.value(x, U[n]) for n, m in zip(self.steps, self.one))

    def gradient(self, x, U):
        P = np.zeros(U.shape, dtype=U.dtype)
        for n, m in zip(self.steps, self.one):
            P[n] = m.gradient(x, U[n])
        return P


# ---- the backward loop --------------------------------------------------------------------------------------------------
def backward(p, P, wrong_betas=False):
    """(lam [N+3, ne+1], B [N+1, ne+1]): lam[N+1] = lam[N+2] = 0, and for n = N .. 1
    B_n = p_n + (1/dt) M (beta0_{n+1} lam^{n+1} + beta1_{n+2} lam^{n+2}),  A_n^T lam^n = B_n with zero end data;
    B_0 likewise, without a solve (lam[0] stays 0: it is not a state).  ``wrong_betas``: the negative control,
    (beta0_n, beta1_n) in the place of (beta0_{n+1}, beta1_{n+2})."""
    M, A, _ = matrices(p)
    N = p.N
    lam = np.zeros((N + 3, len(p.x)))
    B = np.zeros((N + 1, len(p.x)))
    for n in range(N, -1, -1):
        b0, b1 = adjoint_betas(p.scheme, n, N)
        if wrong_betas and n >= 1:
            _, b0, b1 = coefficients(p.scheme, n, N)
        v = b0 * lam[n + 1] if b1 == 0.0 else b0 * lam[n + 1] + b1 * lam[n + 2]
        B[n] = (1.0 / p.dt) * (M @ v) + 1.0 * P[n]
        if n >= 1:
            lam[n] = sp.bc_solve(A[coefficients(p.scheme, n, N)[0]].T, B[n], p.kinds, p.kappa, (0.0, 0.0))
    return lam, B


def band_ends(p):
    """[2, 2]: {sub[0], sup[ne-1]} of the matrix of step 1 (row 0) and of the later steps (row 1)."""
    _, A, _ = matrices(p)
    return np.array([[A[al][1, 0], A[al][-2, -1]] for al in (BDF["bdf1"][0], BDF[p.scheme][0])])


# ---- the sums over time, in the order of csrc/lssvr_chunk_sens.hpp -----------------------------------------------------------
def ts_diff(al, b0, b1, inv_dt, u2, u0, u1):
    d = al * u2 - b0 * u0
    return inv_dt * (d if b1 == 0.0 else d - b1 * u1)


def chunk_tables(x, nq, Utraj, Z, n0, inv_dt, coef, phi, R, init=None):
    """dict(a=, c=, rho= [ne, nq], f= [R, ne, nq]) of the chunk of m = len(Z) steps n0 .. n0+m-1; row i of Z and of coef
    belongs to step n0+m-1-i.  ``init``: the dict the sums continue from (accumulate), else they start from 0.  Every
    operation in the order of chunk_sens_entry, one rounding each: bit for bit the library's values."""
    xi, w = sp.gauss01(nq)
    ne, m = len(x) - 1, len(Z)
    h = (x[1:] - x[:-1])[:, None]
    xi, w = xi[None, :], w[None, :]
    om, wh, hw = 1.0 - xi, w / h, h * w
    zero = np.zeros((ne, int(nq)))
    sa, sc, sr = (zero.copy() if init is None else np.array(init[k]) for k in ("a", "c", "rho"))
    sf = np.zeros((R, ne, int(nq))) if init is None else np.array(init["f"])
    nhi = n0 + m - 1
    for i in range(m):
        n = nhi - i
        u, pv = Utraj[n], Utraj[n - 1]
        qv = Utraj[n - 2] if n >= 2 else np.zeros_like(u)
        u0, u1, p0, p1, q0, q1, z0, z1 = (t[:, None] for t in (u[:-1], u[1:], pv[:-1], pv[1:], qv[:-1], qv[1:],
                                                                Z[i][:-1], Z[i][1:]))
        t = hw * (z0 * om + z1 * xi)
        sa = sa - ((wh * (z1 - z0)) * (u1 - u0))
        sc = sc - (t * (u0 * om + u1 * xi))
        al, b0, b1 = coef[i]
        w0, w1 = ts_diff(al, b0, b1, inv_dt, u0, p0, q0), ts_diff(al, b0, b1, inv_dt, u1, p1, q1)
        sr = sr - (t * (w0 * om + w1 * xi))
        for r in range(R):
            sf[r] = sf[r] + phi[n - 1, r] * t
    return dict(a=sa, c=sc, rho=sr, f=sf)


def chunk_ends(Utraj, Z, Brows, n0, bends, band_row, kinds, out_g, kappa_init=None):
    """The end gradients of the chunk in the order of chunk_sens_ends: rows n0 .. n0+m-1 of ``out_g`` [N+1, 2] are
    written in place; returns kappa [2], continued from ``kappa_init`` (accumulate) or from 0."""
    ne, m = Z.shape[1] - 1, len(Z)
    nhi = n0 + m - 1
    kap = np.zeros(2) if kappa_init is None else np.array(kappa_init, dtype=np.float64)
    for s, (end, inner) in enumerate(((0, 1), (ne, ne - 1))):
        for i in range(m):
            n = nhi - i
            if kinds[s] == ROBIN:
                out_g[n, s] = Z[i][end]
                kap[s] = kap[s] - (Z[i][end] * Utraj[n][end])
            else:
                out_g[n, s] = Brows[i][end] - bends[band_row[i]][s] * Z[i][inner]
    return kap


def chunks(N, size=CHUNK):
    """The chunks of a sweep over the steps N .. 1 -> [(n0, m)], the highest steps first."""
    out, hi = [], N
    while hi >= 1:
        m = min(size, hi)
        out.append((hi - m + 1, m))
        hi -= m
    return out


def sweep_gradients(p, U, lam, B, size=CHUNK, tables=chunk_tables, ends=chunk_ends):
    """The gradient dict of a whole sweep in chunks of ``size`` steps, through ``tables`` / ``ends`` (the numpy
    restatement, or wrappers of the library's host mirror with the same signature): a, c, rho [ne, nq], f [R, ne, nq],
    u0 [ne+1], g [N+1, 2], kappa [2]."""
    N, R = p.N, p.f.shape[0]
    inv_dt = 1.0 / p.dt
    be = band_ends(p)
    out_g = np.zeros((N + 1, 2))
    tabs = kap = None
    for n0, m in chunks(N, size):
        steps = [n0 + m - 1 - i for i in range(m)]
        Z, Br = lam[steps], B[steps]
        coef = np.array([coefficients(p.scheme, n, N) for n in steps])
        tabs = tables(p.x, p.nq, U, Z, n0, inv_dt, coef, p.phi, R, tabs)
        kap = ends(U, Z, Br, n0, be, [0 if n == 1 else 1 for n in steps], p.kinds, out_g, kap)
    gu0 = B[0].copy()
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == DIRICHLET:
            out_g[0, s] = B[0][end]
            gu0[end] = 0.0
    return dict(tabs, u0=gu0, g=out_g, kappa=kap)


def adjoint_gradients(p, J, size=CHUNK, wrong_betas=False):
    """The gradient dict by ONE forward and ONE backward loop, plus value, U, lam, B, P."""
    U = forward(p)
    P = J.gradient(p.x, U)
    lam, B = backward(p, P, wrong_betas)
    out = sweep_gradients(p, U, lam, B, size)
    out.update(value=float(J.value(p.x, U)), U=U, lam=lam, B=B, P=P)
    return out


# ---- the yardstick: complex step, one loop per datum ------------------------------------------------------------------------
def complex_step(p, J):
    """The same gradient dict by Im J(theta + i 1e-30 delta) / 1e-30, one forward loop per entry."""
    def run(**kw):
        q = p.replace(**kw)
        return J.value(q.x, forward(q)).imag / CSTEP

    out = {}
    for name in ("a", "c", "rho", "f"):
        base = getattr(p, name)
        grad = np.zeros(base.shape)
        for idx in np.ndindex(*base.shape):
            t = base.astype(complex)
            t[idx] += 1j * CSTEP
            grad[idx] = run(**{name: t})
        out[name] = grad
    gu0 = np.zeros(len(p.x))
    for i in range(len(p.x)):
        t = p.u0.astype(complex)
        t[i] += 1j * CSTEP
        gu0[i] = run(u0=t)
    out["u0"] = gu0
    gg = np.zeros(p.g.shape)
    for idx in np.ndindex(*p.g.shape):
        t = p.g.astype(complex)
        t[idx] += 1j * CSTEP
        gg[idx] = run(g=t)
    out["g"] = gg
    gk = np.zeros(2)
    for s in range(2):
        if p.kinds[s] == ROBIN:
            t = np.array(p.kappa, dtype=complex)
            t[s] += 1j * CSTEP
            gk[s] = run(kappa=t)
    out["kappa"] = gk
    return out


GROUPS = ("a", "c", "rho", "f", "u0", "g", "kappa")


def deviations(got, want):
    """Per group, the largest deviation of ``got`` from ``want`` relative to the largest entry of the group in ``want``
    (absolute where that is 0: kappa at two Dirichlet ends)."""
    out = {}
    for k in GROUPS:
        if got.get(k) is None:
            continue
        scale = float(np.max(np.abs(want[k])))
        err = float(np.max(np.abs(np.asarray(got[k]) - want[k])))
        out[k] = err / scale if scale > 0.0 else err
    return out


def reading(case):
    """(per-group deviations of the adjoint gradients from the complex step, the adjoint dict, the complex-step dict)
    of ``case`` = (Problem, functional)."""
    p, J = case
    adj = adjoint_gradients(p, J)
    cs = complex_step(p, J)
    return deviations(adj, cs), adj, cs


# ---- the cases: callables, so that the facade can be handed the same problem ------------------------------------------------
def weight(x):
    return 1.0 + 0.5 * x * x


def forcing_x1(x):
    return np.cos(2.0 * x)


def phi0(t):
    return 1.0 + 0.5 * t


def phi1(t):
    return np.sin(3.0 * t) - 0.2


def g_left(t):
    return 0.3 + 0.4 * t


def g_right(t):
    return -0.2 + np.sin(2.0 * t)


def u_init(x):
    return np.cos(1.5 * x) + 0.3 * x


FORCING = ((phi0, sp.rhs), (phi1, forcing_x1))
T_END = 0.6


def problem(ne, nq, kinds, scheme, N, t_end=T_END):
    """The case problem: the non-uniform mesh of ne elements on [-1, 1], a = 1 + 0.3 sin 2x, c = 1.5 + cos 3x,
    rho = 1 + x^2 / 2, R = 2 forcing terms with non-constant phi, moving end data, kappa = (0.7, 1.3)."""
    x = sp.mesh(ne)
    xq = sp.quad_points(x, nq)
    dt = t_end / N
    times = dt * np.arange(N + 1)
    phi = np.array([[float(f(t)) for f, _ in FORCING] for t in times[1:]])
    g = np.array([[float(g_left(t)), float(g_right(t))] for t in times])
    f = np.stack([fx(xq) for _, fx in FORCING])
    return Problem(x, sp.coef_a(xq), sp.reaction(xq), weight(xq), f, phi, g, np.array(sp.KAPPA), kinds, u_init(x), dt,
                   scheme)


def observe_steps(N):
    return [max(1, N // 2), N]


def observations(N):
    """(steps, x_obs [9], d_obs [2, 9]): 9 points strictly inside the mesh, two steps, data of size 1."""
    xo, d = sp.observations(None)
    return observe_steps(N), xo, np.stack([d, 0.5 * d + 0.1])


def functional(p, kind):
    """"random": any nodal p_n, about 40 % of the steps zero; "goal": the terminal int (1 + x^2) u^N dx; "observe": the
    misfit at 9 points and two steps."""
    N, n1 = p.N, len(p.x)
    if kind == "goal":
        P = np.zeros((N + 1, n1))
        P[N] = sp.goal_load(p.x, p.nq)
        return LinearT(P)
    if kind == "observe":
        return MisfitT(*observations(N))
    rng = np.random.default_rng(5 + N)
    P = rng.standard_normal((N + 1, n1)) * (rng.random(N + 1) >= 0.4)[:, None]
    P[0] = 0.0
    if not P[N].any():
        P[N] = rng.standard_normal(n1)
    return LinearT(P)


# ---- the inverse problem: the initial state of u_t = u'' from two snapshots -------------------------------------------------
DEMO_NE, DEMO_N, DEMO_T, DEMO_OBS, DEMO_ITERS, DEMO_RATE = 16, 16, 0.05, (8, 16), 20, 1.0


def demo_truth(x):
    return np.sin(np.pi * x) + 0.5 * np.sin(3.0 * np.pi * x)


def demo_problem(u0):
    x = np.linspace(0.0, 1.0, DEMO_NE + 1)
    one, zero = np.ones((DEMO_NE, 2)), np.zeros((DEMO_NE, 2))
    return Problem(x, one, zero, one, zero[None], np.ones((DEMO_N, 1)), np.zeros((DEMO_N + 1, 2)), np.zeros(2),
                   (DIRICHLET, DIRICHLET), np.asarray(u0, dtype=np.float64), DEMO_T / DEMO_N, "bdf2")


def demo_data():
    """(x, d [2, ne+1]): the exact discrete snapshots of the run from the true initial state, at every node."""
    p = demo_problem(demo_truth(np.linspace(0.0, 1.0, DEMO_NE + 1)))
    return p.x, forward(p)[list(DEMO_OBS)]


def demo(gradient=None, iters=DEMO_ITERS, rate=DEMO_RATE):
    """Plain gradient descent on the nodal u0 from zero with the fixed ``rate``: u0 -= rate dJ/du0.  ``gradient(u0, x,
    d)`` -> (J, dJ/du0): the prototype's by default, the facade's in the GPU test.  Returns the misfits J_0 .. J_iters."""
    x, d = demo_data()

    def proto_gradient(u0, x, d):
        r = adjoint_gradients(demo_problem(u0), MisfitT(DEMO_OBS, x, d))
        return r["value"], r["u0"]

    gradient = gradient or proto_gradient
    u0 = np.zeros(len(x))
    hist = []
    for _ in range(iters + 1):
        j, gr = gradient(u0, x, d)
        hist.append(float(j))
        u0 = u0 - rate * gr
    return hist


def main():
    print("adjoint gradients of the BDF loop against the complex step (per group, relative to the group's largest entry)")
    print("  case                         " + " ".join(f"{k:>8s}" for k in GROUPS))
    D, R = DIRICHLET, ROBIN
    rows = [(1, 1, (D, D), "bdf1", 3), (2, 2, (R, R), "bdf2", 3), (7, 1, (D, R), "bdf2", 3), (7, 2, (R, D), "bdf1", 8),
            (7, 5, (R, R), "bdf2", 9), (33, 2, (D, D), "bdf2", 9), (33, 2, (D, R), "bdf2", 17),
            (33, 2, (R, R), "bdf2", 17), (33, 3, (R, D), "bdf1", 17)]
    for ne, nq, kinds, scheme, N in rows:
        p = problem(ne, nq, kinds, scheme, N)
        dev = reading((p, functional(p, "random")))[0]
        print(f"  ne={ne:2d} nquad={nq} {''.join('DR'[k] for k in kinds)} {scheme} N={N:2d}: "
              + " ".join(f"{dev[k]:8.1e}" for k in GROUPS))
    p = problem(7, 2, (D, R), "bdf2", 3)
    J = functional(p, "random")
    cs = complex_step(p, J)
    good = max(deviations(adjoint_gradients(p, J), cs).values())
    bad = max(deviations(adjoint_gradients(p, J, wrong_betas=True), cs).values())
    print(f"negative control, N = 3 BDF2, (beta0_n, beta1_n) in the adjoint right-hand side: {bad:.2e} against {good:.2e}")
    hist = demo()
    print(f"inverse problem, {DEMO_NE} elements, {DEMO_N} BDF2 steps to t = {DEMO_T}, snapshots at steps {DEMO_OBS}, "
          f"{DEMO_ITERS} steps of gradient descent on u0 (rate {DEMO_RATE})")
    print("  misfit: " + " ".join(f"{v:.3e}" for v in hist))
    print(f"  monotone: {all(b < a for a, b in zip(hist, hist[1:]))}, final / first = {hist[-1] / hist[0]:.3e}, "
          f"final = {hist[-1]:.6e}")


if __name__ == "__main__":
    main()
