"""numpy prototype of the adjoint sensitivities of the Newmark loop of rho u_tt + d u_t - (a u')' + c u = f(x, t) (DESIGN.md
section 34): the dense forward loop of section 29 (real or complex; the scalars are wave_proto.coefficients, the
assembly, the end treatment and the functionals those of sensitivity_proto / transient_sensitivity_proto), the
complex-step derivative of a functional J = sum_n p_n . u^n, n = 0 .. N, with respect to every datum -- the tables a, c,
rho, d, f_r at the Gauss points, the initial state and velocity, the end data g(t_n), kappa and the first acceleration of
a Dirichlet end -- by Im J(theta + i 1e-30 delta) / 1e-30, the backward sweep through the transposed Newmark recurrences
in the order of csrc/lssvr_newmark_adj.hpp, and the sums over time in that of csrc/lssvr_chunk_sens.hpp.  No GPU, nothing
but numpy.

Run as a script it prints what DESIGN.md section 34 records: the deviation of the adjoint gradients from the complex
step per group, with and without damping and for (beta, gamma) = (1/4, 1/2) and (0.3025, 0.6), what the sweep reads
without c_va vbar in abar*, and a small inverse problem -- the initial displacement of u_tt = (a u')' from traces at three
points by 20 steps of gradient descent."""
import numpy as np

import sensitivity_proto as sp
import transient_sensitivity_proto as tsp
import wave_proto as wp

DIRICHLET, ROBIN = sp.DIRICHLET, sp.ROBIN
CSTEP = sp.CSTEP
CHUNK = 8
NEWMARK = ((0.25, 0.5), (0.3025, 0.6))
MisfitT = tsp.MisfitT


# ---- the problem and the forward loop, dense; real or complex --------------------------------------------------------------
class Problem:
    """The data of one loop: x [ne+1], tables a, c, rho, d [ne, nq] (d None: no damping) and f [R, ne, nq] at the Gauss
    points, phi [N+1, R] and g [N+1, 2] (row n: the time t_n, the layout solve_wave uploads), kappa [2], kinds, u0, v0
    [ne+1], accel0 [2] (the first acceleration of a Dirichlet end), dt, beta, gamma."""
    FIELDS = ("x", "a", "c", "rho", "d", "f", "phi", "g", "kappa", "kinds", "u0", "v0", "accel0", "dt", "beta", "gamma")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])
        self.kinds = tuple(self.kinds)
        self.N, self.nq = self.phi.shape[0] - 1, self.a.shape[1]

    def replace(self, **kw):
        return Problem(**{**{k: getattr(self, k) for k in self.FIELDS}, **kw})


def matrices(p):
    """dict(mass, damp (None without d), stiff, step: dense; loads [R, ne+1]).  The step's matrix is ONE assembly with
    the reaction table c + rho / (beta dt^2) + gamma d / (beta dt), what solve_wave does."""
    zero = np.zeros(p.a.shape)
    shift = p.c + p.rho / (p.beta * p.dt ** 2)
    if p.d is not None:
        shift = shift + p.gamma * p.d / (p.beta * p.dt)
    full = lambda a, c: sp.dense(*sp.assemble(p.x, zero, a, None, c)[:3])      # noqa: E731
    return dict(mass=full(zero, p.rho), damp=None if p.d is None else full(zero, p.d), stiff=full(p.a, p.c),
                step=full(p.a, shift), loads=np.stack([sp.assemble(p.x, fr)[3] for fr in p.f]))


def forward(p, mats=None):
    """(U, V, A), each [N+1, ne+1]: the state at t_0 .. t_N by the loop of section 29, every node kept (the end node of
    a Dirichlet end follows the pointwise recurrences like any other)."""
    m = mats or matrices(p)
    Mr, Md, K, S, L = m["mass"], m["damp"], m["stiff"], m["step"], m["loads"]
    typ = np.result_type(Mr, K, S, L, p.phi, p.g, np.asarray(p.kappa), p.u0, p.v0, np.asarray(p.accel0),
                         *(() if Md is None else (Md,)))
    dt, c_u2, c_v1, c_m, c_d, c_va = wp.coefficients(p.dt, p.beta, p.gamma)
    n1 = len(p.x)
    U, V, A = (np.zeros((p.N + 1, n1), dtype=typ) for _ in range(3))
    U[0], V[0] = p.u0, p.v0
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == DIRICHLET:
            U[0, end] = p.g[0, s]
    r0 = p.phi[0] @ L - K @ U[0]
    if Md is not None:
        r0 = r0 - Md @ V[0]
    ga = np.zeros(2, dtype=typ)
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == ROBIN:
            r0[end] = r0[end] + (p.g[0, s] - p.kappa[s] * U[0, end])
        else:
            ga[s] = p.accel0[s]
    A[0] = sp.bc_solve(Mr, r0, p.kinds, (0.0, 0.0), ga)
    for n in range(p.N):
        ut = (U[n] + dt * V[n]) + c_u2 * A[n]
        vt = V[n] + c_v1 * A[n]
        rhs = p.phi[n + 1] @ L + Mr @ (c_m * ut)
        if Md is not None:
            rhs = rhs + Md @ (c_d * ut - vt)
        U[n + 1] = sp.bc_solve(S, rhs, p.kinds, p.kappa, p.g[n + 1])
        A[n + 1] = (U[n + 1] - ut) * c_m
        V[n + 1] = vt + c_va * A[n + 1]
    return U, V, A


# ---- functionals of the trajectory: J(U), analytic in U, and p_n = dJ/du^n, n = 0 .. N -----------------------------------
class LinearW:
    """J = sum_n P[n] . u^n for nodal rows P [N+1, ne+1]; unlike the BDF loop's, P[0] may be anything."""

    def __init__(self, P):
        self.P = np.asarray(P, dtype=np.float64)

    def value(self, x, U):
        return np.sum(self.P * U)

    def gradient(self, x, U):
        return self.P.copy()


# ---- the transposed Newmark recurrences, in the order of csrc/lssvr_newmark_adj.hpp ---------------------------------------
def band_apply(diag, off, lam):
    """(M lam)_i = (off[i-1] lam[i-1] + diag[i] lam[i]) + off[i] lam[i+1]; rows 0 and ne leave the missing term out."""
    y = diag * lam
    y[1:] = off * lam[:-1] + y[1:]
    y[:-1] = y[:-1] + off * lam[1:]
    return y


def adjoint_seed(P, vbar, abar, dt, beta, gamma):
    """The first call of a sweep: B_N = p_N + c_m (abar + c_va vbar) (P None: the second term alone)."""
    _, _, _, c_m, _, c_va = wp.coefficients(dt, beta, gamma)
    t = c_m * (abar + c_va * vbar)
    return t if P is None else P + t


def adjoint_advance(lam, vbar, abar, md, mo, dd, do, P, dt, beta, gamma, wrong=False):
    """One case of lssvr_newmark_adjoint_advance between two backward solves -> (ubar, vbar, abar, B) of level n from
    lam = lambda^{n+1}, the bars (vbar, abar) of level n+1 and the row P = p_n (None: zero).  ``dd`` None: no damping.
    ``wrong``: the negative control, abar* without c_va vbar.  One rounding per operation, bit for bit the library's."""
    dt, c_u2, c_v1, c_m, c_d, c_va = wp.coefficients(dt, beta, gamma)
    ast = abar if wrong else abar + c_va * vbar
    y = band_apply(md, mo, lam)
    if dd is None:
        ut = c_m * y - c_m * ast
        vt = vbar
    else:
        z = band_apply(dd, do, lam)
        ut = (c_m * y + c_d * z) - c_m * ast
        vt = vbar - z
    ub = ut if P is None else P + ut
    vb = dt * ut + vt
    ab = c_u2 * ut + c_v1 * vt
    return ub, vb, ab, ub + c_m * (ab + c_va * vb)


def bands_of(M):
    return np.array(np.diag(M)), np.array(np.diag(M, 1))


def backward(p, P, mats=None, wrong=False):
    """(lam [N+1, ne+1], B [N+1, ne+1], ubar0, vbar0): lam[n], n >= 1, solves A lam = B_n with zero end data; lam[0]
    solves M_rho lam = abar of level 0 (= B[0]), Robin ends as natural rows; (ubar0, vbar0): the bars of level 0
    BEFORE the first acceleration's share."""
    m = mats or matrices(p)
    md, mo = bands_of(m["mass"])
    dd, do = (None, None) if m["damp"] is None else bands_of(m["damp"])
    N, n1 = p.N, len(p.x)
    lam, B = np.zeros((N + 1, n1)), np.zeros((N + 1, n1))
    vb = ab = np.zeros(n1)
    B[N] = adjoint_seed(P[N], vb, ab, p.dt, p.beta, p.gamma)
    ub = P[0]
    for n in range(N - 1, -1, -1):
        lam[n + 1] = sp.bc_solve(m["step"].T, B[n + 1], p.kinds, p.kappa, (0.0, 0.0))
        ub, vb, ab, Bn = adjoint_advance(lam[n + 1], vb, ab, md, mo, dd, do, P[n], p.dt, p.beta, p.gamma, wrong)
        B[n] = Bn if n >= 1 else ab
    if N == 0:
        B[0] = ab
    lam[0] = sp.bc_solve(m["mass"].T, B[0], p.kinds, (0.0, 0.0), (0.0, 0.0))
    return lam, B, ub, vb


# ---- the sums over time, in the order of csrc/lssvr_chunk_sens.hpp ---------------------------------------------------------
TABLES = ("a", "c", "rho", "d", "f")


def chunk_tables(x, nq, Utraj, Vtraj, Atraj, Z, n0, phi, R, want=TABLES, init=None):
    """{table: sums} of the chunk of m = len(Z) levels n0 .. n0+m-1; row i of Z belongs to level n0+m-1-i.  ``init``:
    the dict the sums continue from (accumulate), else from 0.  Every operation in the order of chunk_sens_entry."""
    xi, w = sp.gauss01(nq)
    ne, m = len(x) - 1, len(Z)
    h = (x[1:] - x[:-1])[:, None]
    xi, w = xi[None, :], w[None, :]
    om, wh, hw = 1.0 - xi, w / h, h * w
    s = {k: (np.zeros((R, ne, int(nq))) if k == "f" else np.zeros((ne, int(nq)))) if init is None else np.array(init[k])
         for k in want}
    nhi = n0 + m - 1
    lr = lambda t: (t[:-1, None], t[1:, None])          # noqa: E731
    for i in range(m):
        n = nhi - i
        z0, z1 = lr(Z[i])
        t = hw * (z0 * om + z1 * xi)
        if "a" in want:
            u0, u1 = lr(Utraj[n])
            s["a"] = s["a"] - ((wh * (z1 - z0)) * (u1 - u0))
        for k, traj in (("c", Utraj), ("rho", Atraj), ("d", Vtraj)):
            if k in want:
                u0, u1 = lr(traj[n])
                s[k] = s[k] - (t * (u0 * om + u1 * xi))
        if "f" in want:
            for r in range(R):
                s["f"][r] = s["f"][r] + phi[n, r] * t
    return s


def chunk_ends(Utraj, Z, Brows, n0, bends, kinds, out_g, kappa_init=None):
    """The end gradients of the chunk in the order of chunk_sens_ends: rows n0 .. n0+m-1 of ``out_g`` [N+1, 2] are written
    in place; returns kappa [2], continued from ``kappa_init`` (accumulate) or from 0."""
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
                out_g[n, s] = Brows[i][end] - bends[s] * Z[i][inner]
    return kap


def band_ends(M):
    """{sub[0], sup[ne-1]} of a dense matrix."""
    return np.array([M[1, 0], M[-2, -1]])


def sweep_gradients(p, U, V, A, lam, B, ub, vb, mats=None, size=CHUNK, tables=chunk_tables, ends=chunk_ends):
    """The gradient dict of a whole sweep: levels N .. 1 in chunks of ``size`` and level 0 on its own (its matrix is
    M_rho), through ``tables`` / ``ends`` (the numpy restatement, or wrappers of the library's host mirror)."""
    m = mats or matrices(p)
    N, R = p.N, p.f.shape[0]
    want = tuple(k for k in TABLES if k != "d" or p.d is not None)
    out_g = np.zeros((N + 1, 2))
    tabs = kap = None
    for n0, mm in tsp.chunks(N, size):
        lv = [n0 + mm - 1 - i for i in range(mm)]
        tabs = tables(p.x, p.nq, U, V, A, lam[lv], n0, p.phi, R, want, tabs)
        kap = ends(U, lam[lv], B[lv], n0, band_ends(m["step"]), p.kinds, out_g, kap)
    tabs = tables(p.x, p.nq, U, V, A, lam[:1], 0, p.phi, R, want, tabs)
    kap = ends(U, lam[:1], B[:1], 0, band_ends(m["mass"]), p.kinds, out_g, kap)
    # level 0: u0 and v0 enter the first acceleration's right-hand side with -K (kappa of the Robin ends on its
    # diagonal) and -M_d; a Dirichlet end starts at g(0), and what the pass wrote there is dJ/d end_accel0
    Kk = np.array(m["stiff"])
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == ROBIN:
            Kk[end, end] += p.kappa[s]
    gu0 = ub - Kk @ lam[0]
    gv0 = vb if m["damp"] is None else vb - m["damp"] @ lam[0]
    gacc = np.zeros(2)
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == DIRICHLET:
            gacc[s] = out_g[0, s]
            out_g[0, s] = gu0[end]
            gu0[end] = 0.0
    return dict(tabs, u0=gu0, v0=gv0, g=out_g, kappa=kap, accel0=gacc)


def adjoint_gradients(p, J, size=CHUNK, wrong=False):
    """The gradient dict by ONE forward and ONE backward loop, plus value and the arrays of both."""
    mats = matrices(p)
    U, V, A = forward(p, mats)
    P = J.gradient(p.x, U)
    lam, B, ub, vb = backward(p, P, mats, wrong)
    out = sweep_gradients(p, U, V, A, lam, B, ub, vb, mats, size)
    out.update(value=float(J.value(p.x, U)), U=U, V=V, A=A, lam=lam, B=B, P=P)
    return out


# ---- the yardstick: complex step, one loop per datum ------------------------------------------------------------------------
GROUPS = ("a", "c", "rho", "d", "f", "u0", "v0", "g", "kappa", "accel0")


def complex_step(p, J):
    """The same gradient dict by Im J(theta + i 1e-30 delta) / 1e-30, one forward loop per entry."""
    def run(**kw):
        q = p.replace(**kw)
        return J.value(q.x, forward(q)[0]).imag / CSTEP

    out = {}
    for name in ("a", "c", "rho", "d", "f", "u0", "v0", "g"):
        base = getattr(p, name)
        if base is None:
            continue
        grad = np.zeros(base.shape)
        for idx in np.ndindex(*base.shape):
            t = base.astype(complex)
            t[idx] += 1j * CSTEP
            grad[idx] = run(**{name: t})
        out[name] = grad
    for name in ("kappa", "accel0"):
        grad = np.zeros(2)
        for s in range(2):
            if (p.kinds[s] == ROBIN) == (name == "kappa"):
                t = np.array(getattr(p, name), dtype=complex)
                t[s] += 1j * CSTEP
                grad[s] = run(**{name: t})
        out[name] = grad
    return out


def deviations(got, want):
    """Per group, the largest deviation of ``got`` from ``want`` relative to the largest entry of the group in ``want``
    (absolute where that is 0).  accel0 is measured against the largest entry of g, the other datum of the same ends:
    with (beta, gamma) = (1/4, 1/2) and no damping its own derivative is 0 up to rounding, no scale at all."""
    out = {}
    for k in GROUPS:
        if got.get(k) is None or want.get(k) is None:
            continue
        scale = float(np.max(np.abs(want["g" if k == "accel0" else k])))
        err = float(np.max(np.abs(np.asarray(got[k]) - want[k])))
        out[k] = err / scale if scale > 0.0 else err
    return out


def reading(case, wrong=False):
    """(per-group deviations of the adjoint gradients from the complex step, the adjoint dict, the complex-step dict)
    of ``case`` = (Problem, functional)."""
    p, J = case
    adj = adjoint_gradients(p, J, wrong=wrong)
    cs = complex_step(p, J)
    return deviations(adj, cs), adj, cs


# ---- the cases: callables, so that the facade can be handed the same problem ------------------------------------------------
weight, forcing_x1, phi0, phi1, g_left, g_right, u_init = (tsp.weight, tsp.forcing_x1, tsp.phi0, tsp.phi1, tsp.g_left,
                                                           tsp.g_right, tsp.u_init)
FORCING = tsp.FORCING
T_END = 0.6
ACCEL0 = (0.0, -0.0)        # g_left'' (0) = 0, g_right''(0) = -4 sin 0 = 0


def damping(x):
    return 0.4 + 0.3 * np.cos(x)


def v_init(x):
    """The start velocity; equal to g'(0) = (0.4, 2.0) at the ends x = -1, 1, as a moving Dirichlet end needs."""
    return 1.2 + 0.8 * x + 0.5 * (1.0 - x * x)


def problem(ne, nq, kinds, N, damped, newmark, t_end=T_END):
    """The case problem: the non-uniform mesh of ne elements on [-1, 1], a = 1 + 0.3 sin 2x, c = 1.5 + cos 3x,
    rho = 1 + x^2 / 2, d = 0.4 + 0.3 cos x (``damped``), R = 2 forcing terms with non-constant phi, moving end data,
    kappa = (0.7, 1.3)."""
    x = sp.mesh(ne)
    xq = sp.quad_points(x, nq)
    dt = t_end / N
    times = dt * np.arange(N + 1)
    phi = np.array([[float(f(t)) for f, _ in FORCING] for t in times])
    g = np.array([[float(g_left(t)), float(g_right(t))] for t in times])
    f = np.stack([fx(xq) for _, fx in FORCING])
    return Problem(x=x, a=sp.coef_a(xq), c=sp.reaction(xq), rho=weight(xq), d=damping(xq) if damped else None, f=f,
                   phi=phi, g=g, kappa=np.array(sp.KAPPA), kinds=kinds, u0=u_init(x), v0=v_init(x),
                   accel0=np.array(ACCEL0), dt=dt, beta=newmark[0], gamma=newmark[1])


def observe_steps(N):
    return [0, max(1, N // 2), N]


def observations(N):
    """(steps, x_obs [9], d_obs [3, 9]): 9 points strictly inside the mesh, three steps (the start among them)."""
    xo, d = sp.observations(None)
    return observe_steps(N), xo, np.stack([0.8 * d - 0.1, d, 0.5 * d + 0.1])


def functional(p, kind):
    """"random": any nodal p_n, about 40 % of the levels zero, p_0 != 0; "goal": the terminal int (1 + x^2) u^N dx;
    "observe": the misfit at 9 points and three steps."""
    N, n1 = p.N, len(p.x)
    if kind == "goal":
        P = np.zeros((N + 1, n1))
        P[N] = sp.goal_load(p.x, p.nq)
        return LinearW(P)
    if kind == "observe":
        return MisfitT(*observations(N))
    rng = np.random.default_rng(11 + N)
    P = rng.standard_normal((N + 1, n1)) * (rng.random(N + 1) >= 0.4)[:, None]
    for n in (0, N):
        if not P[n].any():
            P[n] = rng.standard_normal(n1)
    return LinearW(P)


# ---- the inverse problem: the initial displacement of u_tt = (a u')' from traces at three points ----------------------------
DEMO_NE, DEMO_N, DEMO_T, DEMO_X, DEMO_ITERS, DEMO_RATE = 16, 32, 2.0, (0.2, 0.45, 0.7), 20, 0.05


def demo_truth(x):
    return np.sin(np.pi * x) + 0.5 * np.sin(2.0 * np.pi * x)


def demo_coef(x):
    return 1.0 + 0.5 * x


def demo_problem(u0):
    x = np.linspace(0.0, 1.0, DEMO_NE + 1)
    one, zero = np.ones((DEMO_NE, 2)), np.zeros((DEMO_NE, 2))
    return Problem(x=x, a=demo_coef(sp.quad_points(x, 2)), c=zero, rho=one, d=None, f=zero[None],
                   phi=np.ones((DEMO_N + 1, 1)), g=np.zeros((DEMO_N + 1, 2)), kappa=np.zeros(2),
                   kinds=(DIRICHLET, DIRICHLET), u0=np.asarray(u0, dtype=np.float64), v0=np.zeros(DEMO_NE + 1),
                   accel0=np.zeros(2), dt=DEMO_T / DEMO_N, beta=0.25, gamma=0.5)


def demo_data():
    """(steps, x_obs, d [N, 3]): the exact discrete traces of the run from the true start at the three points, every
    step 1 .. N."""
    p = demo_problem(demo_truth(np.linspace(0.0, 1.0, DEMO_NE + 1)))
    U = forward(p)[0]
    xo = np.array(DEMO_X)
    e, t = sp.hat_weights(p.x, xo)
    steps = list(range(1, DEMO_N + 1))
    return steps, xo, (U[:, e] * (1 - t) + U[:, e + 1] * t)[steps]


def demo(gradient=None, iters=DEMO_ITERS, rate=DEMO_RATE):
    """Plain gradient descent on the nodal u0 from zero with the fixed ``rate``: u0 -= rate dJ/du0.  ``gradient(u0,
    steps, xo, d)`` -> (J, dJ/du0): the prototype's by default, the facade's in the GPU test.  Returns J_0 .. J_iters."""
    steps, xo, d = demo_data()

    def proto_gradient(u0, steps, xo, d):
        r = adjoint_gradients(demo_problem(u0), MisfitT(steps, xo, d))
        return r["value"], r["u0"]

    gradient = gradient or proto_gradient
    u0 = np.zeros(DEMO_NE + 1)
    hist = []
    for _ in range(iters + 1):
        j, gr = gradient(u0, steps, xo, d)
        hist.append(float(j))
        u0 = u0 - rate * gr
    return hist


CONTROL = (7, 2, (DIRICHLET, ROBIN), 3, True, NEWMARK[1])


def control():
    """(reading, reading without c_va vbar in abar*) on the control case, the largest group each."""
    p = problem(*CONTROL)
    J = functional(p, "random")
    cs = complex_step(p, J)
    return (max(deviations(adjoint_gradients(p, J), cs).values()),
            max(deviations(adjoint_gradients(p, J, wrong=True), cs).values()))


def main():
    print("adjoint gradients of the Newmark loop against the complex step (per group, relative to the group's largest "
          "entry)")
    print("  case                                      " + " ".join(f"{k:>8s}" for k in GROUPS))
    D, R = DIRICHLET, ROBIN
    rows = [(1, 1, (D, D), 3), (2, 2, (R, R), 3), (7, 1, (D, R), 3), (7, 2, (R, D), 8), (7, 5, (R, R), 9),
            (7, 2, (D, D), 17), (33, 2, (D, D), 9), (33, 2, (D, R), 17), (33, 2, (R, R), 17), (33, 3, (R, D), 17)]
    for damped in (False, True):
        for nm in NEWMARK:
            for ne, nq, kinds, N in rows:
                p = problem(ne, nq, kinds, N, damped, nm)
                dev = reading((p, functional(p, "random")))[0]
                print(f"  ne={ne:2d} nquad={nq} {''.join('DR'[k] for k in kinds)} N={N:2d} d={'yn'[not damped]} "
                      f"({nm[0]:.4f}, {nm[1]:.1f}): " + " ".join(f"{dev[k]:8.1e}" if k in dev else "       -"
                                                                  for k in GROUPS))
    good, bad = control()
    print(f"negative control, 7 elements DR N = 3 damped (0.3025, 0.6), abar* without c_va vbar: {bad:.2e} against "
          f"{good:.2e}")
    hist = demo()
    print(f"inverse problem, {DEMO_NE} elements, {DEMO_N} steps to t = {DEMO_T}, traces at x = {DEMO_X}, "
          f"{DEMO_ITERS} steps of gradient descent on u0 (rate {DEMO_RATE})")
    print("  misfit: " + " ".join(f"{v:.3e}" for v in hist))
    print(f"  monotone: {all(b < a for a, b in zip(hist, hist[1:]))}, final / first = {hist[-1] / hist[0]:.3e}, "
          f"final = {hist[-1]:.6e}")


if __name__ == "__main__":
    main()
