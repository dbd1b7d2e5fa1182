"""numpy restatement of the goal-oriented (dual-weighted residual) estimator (include/lssvr_hip.h:
lssvr_estimate_goal) from the Legendre tables of oracle/lssvr_oracle.py, plain float64.  A plain module: the CPU tests
pin its signs to an identity that holds to rounding, the GPU tests compare the kernel with it.

For -(a u')' + c u = f, J(u) = int j u, any continuous piecewise polynomial ut with the Dirichlet values and z the
solution of -(a z')' + c z = j (zero at Dirichlet ends, a dz/dn + kappa z = 0 at Neumann or Robin ends):

    J(u) - J(ut) = sum_e eta_e
    eta_e = int_e R z - 1/2 (J_e z(x_e) + J_{e+1} z(x_{e+1})) + [end element] (g - kappa ut - a dut/dn) z(x_end)
    R = f + a ut'' + a' ut' - c ut,   J_i = aR_{i-1} ut_{i-1}'(x_i) - aL_i ut_i'(x_i),  J_0 = J_ne = 0

(integrate a ut' z' by parts on every element: the node terms are the flux jumps times z, split in halves between the
two elements of a node; at a Robin end the boundary form kappa ut z and the load g z join the end term)."""
import numpy as np

from oracle import lssvr_oracle as orc

DIRICHLET, ROBIN = 0, 1


def estimate_goal(x, Wu, Wz, xi, wt, f, j, a=None, da=None, c=None, a_ends=None, kinds=(0, 0), kappa=(0.0, 0.0),
                  g=(0.0, 0.0), a_bnd=(1.0, 1.0), jump_free=False):
    """(eta[ne], q[ne], scale[ne]): the signed indicator, q_e = int_e j ut, and ``scale`` = eta with every term taken
    by its magnitude (sum_q |w R z| h/2 + |jump terms| + |end terms|), which bounds what rounding can do where the
    terms cancel.  ``xi``, ``wt``: Gauss rule on [-1, 1]; ``f``, ``j``, ``a``, ``da``, ``c``: element-major [ne, nq]
    tables at ``orc.estimate_points`` (absent ``a``: 1, absent ``da`` / ``c``: 0); ``a_ends`` [ne, 2]: a at each
    element's two nodes (absent: 1); ``kinds``, ``kappa``, ``g``, ``a_bnd``: the two ends of the domain, g of the
    primal problem and a there.  ``jump_free``: the weight is z minus its linear interpolant at every element's two
    nodes, which vanishes there: no jump and no end terms, eta_e = int_e R (z - I_h z)."""
    ne, M = Wu.shape
    if jump_free:
        sg = (-1.0) ** np.arange(M)
        zl0, zr0 = Wz @ sg, Wz.sum(axis=1)
        Wz = Wz.copy()
        Wz[:, 0] -= 0.5 * (zl0 + zr0)
        if M > 1:
            Wz[:, 1] -= 0.5 * (zr0 - zl0)
    h = x[1:] - x[:-1]
    scl = 2.0 / h
    L, D1, D2 = orc.legendre_tables(xi, M)                 # [nq, M]
    u = Wu @ L.T
    z = Wz @ L.T
    R = f + (1.0 if a is None else a) * ((Wu @ D2.T) * (scl ** 2)[:, None])
    if da is not None:
        R = R + da * ((Wu @ D1.T) * scl[:, None])
    if c is not None:
        R = R - c * u
    k = np.arange(M, dtype=np.float64)
    w = k * (k + 1) / 2
    sgn = (-1.0) ** k                                      # P_k(-1); P_k'(-1) = -sgn * w, P_k'(1) = w
    dl = (Wu @ (-sgn * w)) * scl
    dr = (Wu @ w) * scl
    ae = np.ones((ne, 2)) if a_ends is None else a_ends
    fl, fr = ae[:, 0] * dl, ae[:, 1] * dr
    J = np.zeros(ne + 1)
    J[1:-1] = fr[:-1] - fl[1:]
    zl, zr = Wz @ sgn, Wz.sum(axis=1)
    if jump_free:
        zl, zr = np.zeros(ne), np.zeros(ne)
    ul, ur = Wu @ sgn, Wu.sum(axis=1)
    interior = 0.5 * h * ((R * z) @ wt)
    jump_l = -0.5 * J[:-1] * zl
    jump_r = -0.5 * J[1:] * zr
    eta = interior + jump_l + jump_r
    scale = 0.5 * h * (np.abs(R * z) @ wt) + np.abs(jump_l) + np.abs(jump_r)
    if kinds[0] == ROBIN:                                  # du/dn = -u' at the left end
        t = (g[0] - kappa[0] * ul[0] - a_bnd[0] * (-dl[0])) * zl[0]
        eta[0] += t
        scale[0] += abs(t)
    if kinds[1] == ROBIN:
        t = (g[1] - kappa[1] * ur[-1] - a_bnd[1] * dr[-1]) * zr[-1]
        eta[-1] += t
        scale[-1] += abs(t)
    q = 0.5 * h * ((j * u) @ wt)
    return eta, q, scale


def legendre_rows(x, p, M):
    """W[ne, M]: the polynomial ``p`` (numpy Polynomial) expanded exactly in every element's Legendre basis."""
    from numpy.polynomial.legendre import Legendre
    W = np.zeros((len(x) - 1, M))
    for e in range(len(x) - 1):
        cf = p.convert(domain=[x[e], x[e + 1]], kind=Legendre).coef
        assert cf.size <= M
        W[e, :cf.size] = cf
    return W


def continuous_rows(rng, x, M, end_values=(0.0, 0.0)):
    """W[ne, M] of a random continuous piecewise polynomial of degree M - 1: random nodal values (``end_values`` at the
    two ends of the domain; None leaves an end random), random coefficients from degree 2 up, c_0 and c_1 from the
    element's two nodal values (sum_k c_k = right value, sum_k (-1)^k c_k = left value)."""
    ne = len(x) - 1
    v = rng.uniform(-1.0, 1.0, ne + 1)
    for i, val in ((0, end_values[0]), (-1, end_values[1])):
        if val is not None:
            v[i] = val
    W = np.zeros((ne, M))
    W[:, 2:] = rng.standard_normal((ne, M - 2)) / (1.0 + np.arange(2, M)) ** 2
    sgn = (-1.0) ** np.arange(M)
    s_r, s_l = W.sum(axis=1), W @ sgn
    W[:, 0] = 0.5 * ((v[1:] - s_r) + (v[:-1] - s_l))
    W[:, 1] = 0.5 * ((v[1:] - s_r) - (v[:-1] - s_l))
    return W


# --------------------------------------------------------------------------
# the exact cases: the identity holds to rounding for an arbitrary continuous piecewise polynomial ut
# --------------------------------------------------------------------------
def _mesh7(rng):
    h = rng.uniform(0.3, 1.7, 7)
    return np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])


def exact_case_poisson(seed=1, M=7, nq=8):
    """-u'' = f on (-1, 1), u(+-1) = 0, j = 1, so z = (1 - x^2) / 2: 7 non-uniform elements, ut a random continuous
    piecewise polynomial of degree M - 1 with zero end values, f a cubic.  Returns a dict: x, Wu, Wz (z expanded
    exactly, M >= 3), the Gauss rule, the element-major tables f, j, a, da at the Gauss points, a_ends, and J = J(u)
    from the twice-integrated f."""
    from numpy.polynomial import Polynomial
    rng = np.random.default_rng(seed)
    x = _mesh7(rng)
    fp = Polynomial(rng.uniform(-2.0, 2.0, 4))
    up = -fp.integ(2)                                      # -u'' = f, then the line that zeroes both ends
    lo, hi = up(-1.0), up(1.0)
    up = up - Polynomial([0.5 * (hi + lo), 0.5 * (hi - lo)])
    U = up.integ()
    xi, wt = np.polynomial.legendre.leggauss(nq)
    xq = orc.estimate_points(x, xi)
    return dict(x=x, Wu=continuous_rows(rng, x, M), Wz=legendre_rows(x, Polynomial([0.5, 0.0, -0.5]), M), xi=xi,
                wt=wt, f=fp(xq), j=np.ones_like(xq), a=np.ones_like(xq), da=np.zeros_like(xq), c=None,
                a_ends=np.ones((7, 2)), kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), g=(0.0, 0.0),
                a_bnd=(1.0, 1.0), J=float(U(1.0) - U(-1.0)))


ROBIN_KAPPA = 1.5


def exact_case_robin(seed=2, M=7, nq=8):
    """-(a u')' + 2 u = f with a = 1 + x^2/2, a Neumann left end and a Robin right end (kappa = 1.5), everything
    manufactured from polynomials: z a cubic with z'(-1) = 0 and a(1) z'(1) + kappa z(1) = 0, j := -(a z')' + 2 z;
    u a random quartic, f := -(a u')' + 2 u, g := a du/dn + kappa u at the two ends; ut random continuous piecewise
    of degree M - 1 (free end values).  Same dict as :func:`exact_case_poisson`."""
    from numpy.polynomial import Polynomial
    rng = np.random.default_rng(seed)
    x = _mesh7(rng)
    ap = Polynomial([1.0, 0.0, 0.5])
    cc = 2.0
    # z = z0 + z1 x + z2 x^2 + x^3 with z2, z0 random-free: z'(-1) = z1 - 2 z2 + 3 = 0 and
    # a(1) (z1 + 2 z2 + 3) + kappa (z0 + z1 + z2 + 1) = 0 fix z1 and z0 for a random z2
    z2 = float(rng.uniform(-1.0, 1.0))
    z1 = 2.0 * z2 - 3.0
    z0 = -ap(1.0) * (z1 + 2.0 * z2 + 3.0) / ROBIN_KAPPA - z1 - z2 - 1.0
    zp = Polynomial([z0, z1, z2, 1.0])
    assert abs(zp.deriv()(-1.0)) < 1e-13 and abs(ap(1.0) * zp.deriv()(1.0) + ROBIN_KAPPA * zp(1.0)) < 1e-12
    jp = -(ap * zp.deriv()).deriv() + cc * zp
    up = Polynomial(rng.uniform(-1.0, 1.0, 5))
    fp = -(ap * up.deriv()).deriv() + cc * up
    g = (-ap(-1.0) * up.deriv()(-1.0), ap(1.0) * up.deriv()(1.0) + ROBIN_KAPPA * up(1.0))
    JU = (jp * up).integ()
    xi, wt = np.polynomial.legendre.leggauss(nq)
    xq = orc.estimate_points(x, xi)
    an = ap(x)
    return dict(x=x, Wu=continuous_rows(rng, x, M, end_values=(None, None)), Wz=legendre_rows(x, zp, M), xi=xi, wt=wt,
                f=fp(xq), j=jp(xq), a=ap(xq), da=ap.deriv()(xq), c=np.full_like(xq, cc),
                a_ends=np.stack([an[:-1], an[1:]], axis=1), kinds=(ROBIN, ROBIN), kappa=(0.0, ROBIN_KAPPA),
                g=(float(g[0]), float(g[1])), a_bnd=(float(ap(-1.0)), float(ap(1.0))),
                J=float(JU(1.0) - JU(-1.0)))


def identity_defect(case, eta, q, scale):
    """(|sum eta + sum q - J(u)|, sum_e sum_q |terms|): the defect of the error identity and the magnitude of
    everything that was summed (``scale`` of :func:`estimate_goal` plus the terms of q by magnitude)."""
    import math
    h = np.diff(case["x"])
    L = orc.legendre_tables(case["xi"], case["Wu"].shape[1])[0]
    qabs = 0.5 * h * (np.abs(case["j"] * (case["Wu"] @ L.T)) @ case["wt"])
    total = math.fsum(eta.tolist()) + math.fsum(q.tolist())
    return abs(total - case["J"]), math.fsum(scale.tolist()) + math.fsum(qabs.tolist())


def run_case(case):
    """:func:`estimate_goal` on a case dict."""
    keys = ("x", "Wu", "Wz", "xi", "wt", "f", "j", "a", "da", "c", "a_ends", "kinds", "kappa", "g", "a_bnd")
    return estimate_goal(*(case[k] for k in keys))
