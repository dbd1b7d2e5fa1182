"""numpy prototype of solve_adaptive(mode="h") and (mode="hp") with boundary="periodic"  on -u'' + u = f,
u = exp(-(1 + cos(pi x)) / 0.05) on (-1, 1): a peak that sits on the seam x = -1 ~ x = 1.  The loop of the facade --
periodic P1 solve, per-element solve with the nodal values as constraints at every node (the seam included),
indicator with the seam term, threshold marking, bisection -- on the float64 restatement of oracle/lssvr_oracle.py and
tests/periodic_rules.py, no GPU.  Prints the element count, the max errors on 2001 points of the adapted and of the
uniform periodic solve with the same element count, and their ratio (tests/test_gpu_periodic.py allows the device run
2 x the adapted error printed here).  The hp run raises the degree of a marked element by DM where its coefficients
decay fast enough (tests/hp_rules.py) and bisects it otherwise; every element takes max(N, 2 M) collocation points."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lssvr_oracle as orc              # noqa: E402
import periodic_rules as pr                         # noqa: E402
import hp_rules                                     # noqa: E402

M, N, GAMMA, NQUAD, THETA, NE0, MAXE = 8, 16, 1e8, 5, 0.5, 8, 64
SIGMA_MIN, DM, M_MAX, MAX_ITER = 1.0, 2, 20, 50          # the hp run; M_MAX = min(33, M + 12), the facade's default
one = lambda x: 1.0 + 0.0 * np.asarray(x, dtype=np.float64)        # noqa: E731
zero = lambda x: 0.0 * np.asarray(x, dtype=np.float64)             # noqa: E731
f, c = pr.peak_f, one


def solve(nodes):
    u = pr.fem_solve_periodic(nodes, f, None, None, c, NQUAD)
    # a global domain that no element touches: no Dirichlet value replaces a nodal value, as with the facade's
    # elem_offset = 1, ne_global = ne + 2
    return orc.enhance_all(nodes, u, M, GAMMA, N, rhs=f, global_domain=(-3.0, 3.0), coef_a=one, coef_da=zero,
                           coef_c=c)[0]


def indicator(nodes, W):
    xi, wt = np.polynomial.legendre.leggauss(max(M, 8))
    pts = orc.estimate_points(nodes, xi)
    eta2, _ = orc.estimate_indicator(nodes, W, xi, wt, f(pts), one(pts), zero(pts), c(pts),
                                     np.ones((len(nodes) - 1, 2)))
    return pr.estimate_seam(nodes, W, (1.0, 1.0), eta2, np.array([eta2.sum(), eta2.max(), 0.0]))[0]


def run():
    """(nodes of the adapted mesh, its max error, the max error of the uniform mesh with as many elements, the
    elements marked in the first round)."""
    xq = np.linspace(-1, 1, 2001)
    nodes = np.linspace(-1, 1, NE0 + 1)
    first = None
    while True:
        W = solve(nodes)
        eta2 = indicator(nodes, W)
        mark = eta2 >= THETA * THETA * eta2.max()
        if first is None:
            first = np.nonzero(mark)[0]
        if len(nodes) - 1 + mark.sum() > MAXE or not mark.any():
            break
        mid = 0.5 * (nodes[:-1] + nodes[1:])[mark]
        nodes = np.sort(np.concatenate([nodes, mid]))
    err_a = float(np.max(np.abs(orc.evaluate_solution_vec(nodes, W, xq)[0] - pr.peak_u(xq))))
    un = np.linspace(-1, 1, len(nodes))
    err_u = float(np.max(np.abs(orc.evaluate_solution_vec(un, solve(un), xq)[0] - pr.peak_u(xq))))
    return nodes, err_a, err_u, first


def solve_hp(nodes, deg):
    """Zero-padded W[ne, max M]: every element at its own degree, with its own collocation count."""
    u = pr.fem_solve_periodic(nodes, f, None, None, c, NQUAD)
    W = np.zeros((len(deg), int(deg.max())))
    for i, Mi in enumerate(deg):
        W[i, :Mi] = orc.enhance_all(nodes, u, int(Mi), GAMMA, hp_rules.n_colloc(N, Mi), rhs=f,
                                    global_domain=(-3.0, 3.0), coef_a=one, coef_da=zero, coef_c=c, elements=[i])[0][0]
    return W


def run_hp():
    """(nodes, degrees, max error, max error of the uniform mesh of degree M with as many elements, (bisected, raised)
    element indices of the first round)."""
    xq = np.linspace(-1, 1, 2001)
    nodes, deg = np.linspace(-1, 1, NE0 + 1), np.full(NE0, M, dtype=np.int32)
    first = None
    for it in range(MAX_ITER):
        W = solve_hp(nodes, deg)
        xi, wt = np.polynomial.legendre.leggauss(min(32, max(int(deg.max()), 8)))
        pts = orc.estimate_points(nodes, xi)
        eta2, _ = orc.estimate_indicator(nodes, W, xi, wt, f(pts), one(pts), zero(pts), c(pts),
                                         np.ones((len(deg), 2)))
        eta2 = pr.estimate_seam(nodes, W, (1.0, 1.0), eta2, np.array([eta2.sum(), eta2.max(), 0.0]))[0]
        if it + 1 == MAX_ITER:
            break
        sig = hp_rules.smoothness(W, deg)
        if first is None:
            up, split = hp_rules.actions(nodes, eta2, eta2.max(), THETA, 0.0, sig, deg, SIGMA_MIN, DM, M_MAX)
            first = (np.nonzero(split)[0], np.nonzero(up)[0])
        xn, dn, _, (ns, nr) = hp_rules.refine_hp(nodes, eta2, eta2.max(), THETA, 0.0, sig, deg, SIGMA_MIN, DM, M_MAX)
        if ns + nr == 0 or len(xn) - 1 > MAXE:
            break
        nodes, deg = xn, dn
    err_a = float(np.max(np.abs(orc.evaluate_solution_vec(nodes, W, xq)[0] - pr.peak_u(xq))))
    un = np.linspace(-1, 1, len(nodes))
    err_u = float(np.max(np.abs(orc.evaluate_solution_vec(un, solve(un), xq)[0] - pr.peak_u(xq))))
    return nodes, deg, err_a, err_u, first


def main():
    nodes, err_a, err_u, first = run()
    h = np.diff(nodes)
    print(f"adapted: {len(nodes) - 1} elements, h in [{h.min():.3e}, {h.max():.3e}], max error {err_a:.3e}")
    print(f"uniform {len(nodes) - 1}: max error {err_u:.3e};  ratio {err_u / err_a:.4g}")
    print("first round marks elements", first.tolist(), "of", NE0)
    nodes, deg, err_a, err_u, first = run_hp()
    print(f"hp: {len(deg)} elements, degrees {int(deg.min())}..{int(deg.max())}, sum M = {int(deg.sum())}, "
          f"max error {err_a:.3e}")
    print(f"uniform {len(deg)} of degree {M}: max error {err_u:.3e};  ratio {err_u / err_a:.4g}")
    print("first round bisects", first[0].tolist(), "and raises", first[1].tolist())


if __name__ == "__main__":
    main()
