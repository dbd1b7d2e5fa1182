"""float64 numpy restatement of the reaction operator -(a u')' + c u = f, shared by
tests/test_react_cpu.py and tests/test_gpu_react.py.  Built on oracle/lssvr_oracle.py: the per-element system is
``element_system(..., coef_a, coef_da)`` plus (c / scl^2) L in Ahat; the P1 bands are ``p1_assemble_local`` plus
the consistent mass matrix; the indicator adds -c u to the residual.  The 60-digit KKT solve is restated here as
well (closed_form_mp.solve_truth recovers a, a' from columns 1 and 2 of Ahat, which the c term changes)."""
import numpy as np
from numpy.polynomial.legendre import legder, legval

from oracle import closed_form_mp as cf
from oracle import lssvr_oracle as orc

GAMMA = 1e4
SIZES = [(2000, 9, 16), (300, 20, 32), (100, 26, 40), (25, 9, 16)]      # (ne, M, n)
KS = [1.0, 1e4]


def react_functions(k):
    """a, a' of BASELINE config 5, c = k (2 + cos 2 pi x), and f manufactured for u = sin(pi x)."""
    cc, phi = orc.varcoef_params()
    a, da, f_vc = orc.varcoef_functions(cc, phi)

    def c(x):
        x = np.asarray(x, dtype=np.float64)
        return k * (2.0 + np.cos(2.0 * np.pi * x))

    def f(x):
        x = np.asarray(x, dtype=np.float64)
        return f_vc(x) + c(x) * np.sin(np.pi * x)

    return a, da, c, f


def element_system_react(i, nodes, values, M, gamma, n, a, da, c, f, global_domain, bc=(0.0, 0.0)):
    """ElementSystem of element i with Ahat = -a D2 - (a'/scl) D1 + (c/scl^2) L; returns (s, c/scl^2)."""
    ne = len(nodes) - 1
    xa, xb = nodes[i], nodes[i + 1]
    g_l, g_r = orc.boundary_values(i, ne, xa, xb, values[i], values[i + 1], global_domain, bc[0], bc[1])
    s = orc.element_system(xa, xb, g_l, g_r, M, gamma, n, f, a, da)
    L, _, _ = orc.legendre_tables(s.t, M)
    cs = np.asarray(c(s.x), dtype=np.float64) / (s.scl * s.scl)
    s.Ahat = s.Ahat + cs[:, None] * L
    return s, cs


def enhance_all_react(nodes, values, M, gamma, n, a, da, c, f, global_domain=None, bc=(0.0, 0.0), elements=None,
                      solve=orc.solve_bc_eliminated):
    nodes = np.asarray(nodes, dtype=np.float64)
    if global_domain is None:
        global_domain = (nodes[0], nodes[-1])
    if elements is None:
        elements = range(len(nodes) - 1)
    return np.array([solve(element_system_react(i, nodes, values, M, gamma, n, a, da, c, f, global_domain, bc)[0])
                     for i in elements])


def solve_truth_react(s, a, da, cs, dps=60):
    """60-digit minimiser of the element's QP.  The rows are defined by the float64 data the float64 restatement
    uses -- t_k, scl, a(x_k), a'(x_k)/scl, c(x_k)/scl^2, f(x_k), g -- and built and solved in mpmath from there."""
    mp = cf.mp
    mp.mp.dps = dps
    M, n = s.M, s.n
    scl = mp.mpf(float(s.scl))
    gam = mp.mpf(float(s.gamma))
    ak = np.asarray(a(s.x), dtype=np.float64)
    dos = np.asarray(da(s.x), dtype=np.float64) / s.scl
    A = mp.zeros(n, M)
    for k in range(n):
        L, D1, D2 = cf._legendre_tables_mp(mp.mpf(float(s.t[k])), M)
        for p in range(M):
            A[k, p] = scl * scl * (-mp.mpf(float(ak[k])) * D2[p] - mp.mpf(float(dos[k])) * D1[p]
                                   + mp.mpf(float(cs[k])) * L[p])
    ta = mp.mpf(float(np.float64(s.off) + np.float64(s.scl) * np.float64(s.a)))
    tb = mp.mpf(float(np.float64(s.off) + np.float64(s.scl) * np.float64(s.b)))
    La, _, _ = cf._legendre_tables_mp(ta, M)
    Lb, _, _ = cf._legendre_tables_mp(tb, M)
    K = mp.zeros(M + 2, M + 2)
    AtA = A.T * A
    for i in range(M):
        for j in range(M):
            K[i, j] = gam * AtA[i, j] + (1 if i == j else 0)
        K[i, M] = K[M, i] = La[i]
        K[i, M + 1] = K[M + 1, i] = Lb[i]
    Atf = A.T * mp.matrix([mp.mpf(float(v)) for v in s.f])
    rhs = mp.matrix(M + 2, 1)
    for i in range(M):
        rhs[i] = gam * Atf[i]
    rhs[M] = mp.mpf(float(s.g[0]))
    rhs[M + 1] = mp.mpf(float(s.g[1]))
    sol = mp.lu_solve(K, rhs)
    return np.array([float(sol[i]) for i in range(M)])


def truth_all_react(nodes, values, M, gamma, n, a, da, c, f, elements, global_domain=None, bc=(0.0, 0.0)):
    nodes = np.asarray(nodes, dtype=np.float64)
    if global_domain is None:
        global_domain = (nodes[0], nodes[-1])
    out = []
    for i in elements:
        s, cs = element_system_react(i, nodes, values, M, gamma, n, a, da, c, f, global_domain, bc)
        out.append(solve_truth_react(s, a, da, cs))
    return np.array(out)


# ---------------------------------------------------------------------------
# P1 with the consistent mass matrix
# ---------------------------------------------------------------------------
def p1_bands_react(nodes, f, a, c, nquad):
    """(diag, off, load, kloc): p1_assemble_local + m_e[i][j] = h sum_q w_q c(x_q) phi_i phi_j, p1_scatter."""
    nodes = np.asarray(nodes, dtype=np.float64)
    kloc, fl, fr = orc.p1_assemble_local(nodes, f, a, nquad)
    diag, off, load = orc.p1_scatter(kloc, fl, fr)
    xi, wt = orc.gauss_rule01(nquad)
    h = nodes[1:] - nodes[:-1]
    cq = np.asarray(c(orc.quad_points(nodes, nquad)), dtype=np.float64)
    mll = h * (cq @ (wt * (1.0 - xi) ** 2))
    mlr = h * (cq @ (wt * (1.0 - xi) * xi))
    mrr = h * (cq @ (wt * xi ** 2))
    diag = diag.copy()
    diag[:-1] += mll
    diag[1:] += mrr
    return diag, off + mlr, load, kloc


def fem_p1_solve_react(nodes, f, a, c, nquad, u0=0.0, u1=0.0):
    diag, off, load, _ = p1_bands_react(nodes, f, a, c, nquad)
    return orc.thomas_dirichlet(diag, off, load, u0, u1)


# ---------------------------------------------------------------------------
# indicator
# ---------------------------------------------------------------------------
def estimate_react(x, W, xi, wt, a, da, c, f, a_ends):
    """eta2[e] = h^2 int_e (f + a u'' + a' u' - c u)^2 + h/2 (J_e^2 + J_{e+1}^2), J the jump of a u'; the tables
    element-major [ne, nq] at the Gauss points (xi, wt on [-1, 1])."""
    ne, M = W.shape
    nq = len(xi)
    h = x[1:] - x[:-1]
    scl = 2.0 / h
    T = np.zeros((3, nq, M))
    D = np.zeros((2, M))
    for k in range(M):
        ek = np.zeros(M)
        ek[k] = 1.0
        T[0, :, k] = legval(xi, ek)
        T[1, :, k] = legval(xi, legder(ek, 1))
        T[2, :, k] = legval(xi, legder(ek, 2))
        D[:, k] = legval(np.array([-1.0, 1.0]), legder(ek, 1))
    r = f + a * ((W @ T[2].T) * (scl ** 2)[:, None]) + da * ((W @ T[1].T) * scl[:, None]) - c * (W @ T[0].T)
    integ = 0.5 * h * ((r * r) @ wt)
    fl = a_ends[:, 0] * ((W @ D[0]) * scl)
    fr = a_ends[:, 1] * ((W @ D[1]) * scl)
    J = np.zeros(ne + 1)
    J[1:-1] = fr[:-1] - fl[1:]
    return h * h * integ + 0.5 * h * (J[:-1] ** 2 + J[1:] ** 2)


def estimate_points(x, xi):
    a, b = x[:-1, None], x[1:, None]
    return 0.5 * (a + b) + (0.5 * (b - a)) * xi[None, :]
