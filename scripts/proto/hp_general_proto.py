"""numpy prototype of solve_adaptive(mode="hp") against (mode="h") for an operator with coefficients and convection
(DESIGN.md section 23): the outflow layer of section 18, -eps u'' + u' = 1 on (0, 1), u(0) = u(1) = 0, eps = 0.02, from
32 uniform elements (cell Peclet 0.78) of degree M0, both runs under the same budget of sum M_e <= MAX_DOF coefficients
(mode "h": max_elements = MAX_DOF // M0).  The loop of the facade -- non-symmetric P1 bands, banded solve, per-element
solve with each element's own degree and max(N, 2 M) collocation points on the folded table a' - b, indicator, decay
rate, raise or bisect -- on the float64 restatement of oracle/lssvr_oracle.py, tests/convection_rules.py and
tests/hp_rules.py, no GPU.  Prints elements, sum M_e and the max error on 2001 points of both runs
(tests/test_gpu_hp_general.py allows the device runs 2 x the errors printed here).

Why M0 = 2 and M_MAX = 3: every element takes the P1 nodal values as its constraint rows, and with convection those carry
an O(h^2) error that only bisection reduces (for -u'' = f they are exact, which is what section 17's 41 x rests on).  A
higher degree pays until the error inside the elements is down at the nodal error, and no further: from the linear
elements M0 = 2 one more coefficient does that, and the coefficients it saves go into bisection.  From M0 = 5 and the
default M_MAX = 17 the same loop LOSES to bisection alone (1.2e-3 against 8.6e-5 at 600 coefficients): `main` prints
that run too."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lssvr_oracle as orc              # noqa: E402
import convection_rules as cr                       # noqa: E402
import hp_rules                                     # noqa: E402

M0, N, GAMMA, NQUAD, THETA, NE0, MAX_DOF = 2, 16, 1e10, 5, 0.5, 32, 600
SIGMA_MIN, DM, M_MAX, MAX_ITER, GD = 1.0, 1, 3, 50, (0.0, 1.0)
XQ = np.linspace(0.0, 1.0, 2001)


def solve(nodes, deg):
    """Zero-padded W[ne, max M]: every element at its own degree, with its own collocation count."""
    u = cr.fem_solve(nodes, cr.layer_f, cr.layer_a, cr.layer_b, None, NQUAD)
    W = np.zeros((len(deg), int(deg.max())))
    for Mi in np.unique(deg):
        ids = np.nonzero(deg == Mi)[0]
        W[ids, :Mi] = orc.enhance_all(nodes, u, int(Mi), GAMMA, hp_rules.n_colloc(N, Mi), rhs=cr.layer_f,
                                      global_domain=GD, coef_a=cr.layer_a, coef_da=cr.layer_folded, elements=ids)[0]
    return W


def indicator(nodes, W, nq):
    xi, wt = np.polynomial.legendre.leggauss(nq)
    pts = orc.estimate_points(nodes, xi)
    an = cr.layer_a(nodes)
    return orc.estimate_indicator(nodes, W, xi, wt, cr.layer_f(pts), cr.layer_a(pts), cr.layer_folded(pts), None,
                                  np.stack([an[:-1], an[1:]], 1))[0]


def max_error(nodes, W):
    return float(np.max(np.abs(orc.evaluate_solution_vec(nodes, W, XQ)[0] - cr.layer_exact(XQ))))


def run_h():
    """(nodes, max error) of mode "h" at degree M0: stops when the next mesh would exceed MAX_DOF // M0 elements."""
    nodes = np.linspace(GD[0], GD[1], NE0 + 1)
    for it in range(MAX_ITER):
        deg = np.full(len(nodes) - 1, M0, dtype=np.int32)
        W = solve(nodes, deg)
        eta2 = indicator(nodes, W, max(M0, 8))
        mark = eta2 >= THETA * THETA * eta2.max()
        if it + 1 == MAX_ITER or not mark.any() or len(deg) + mark.sum() > MAX_DOF // M0:
            break
        nodes = np.sort(np.concatenate([nodes, 0.5 * (nodes[:-1] + nodes[1:])[mark]]))
    return nodes, max_error(nodes, W)


def run_hp():
    """(nodes, degrees, max error) of mode "hp" from degree M0: stops when the next round would exceed MAX_DOF."""
    nodes, deg = np.linspace(GD[0], GD[1], NE0 + 1), np.full(NE0, M0, dtype=np.int32)
    for it in range(MAX_ITER):
        W = solve(nodes, deg)
        eta2 = indicator(nodes, W, min(32, max(int(deg.max()), 8)))
        if it + 1 == MAX_ITER:
            break
        sig = hp_rules.smoothness(W, deg)
        xn, dn, _, (ns, nr) = hp_rules.refine_hp(nodes, eta2, eta2.max(), THETA, 0.0, sig, deg, SIGMA_MIN, DM, M_MAX)
        if ns + nr == 0 or dn.sum() > MAX_DOF:
            break
        nodes, deg = xn, dn
    return nodes, deg, max_error(nodes, W)


def report():
    print(f"start: {NE0} elements of degree {M0}, cell Peclet "
          f"{cr.cell_peclet(np.linspace(*GD, NE0 + 1), cr.layer_a, cr.layer_b, NQUAD).max():.4g}, budget {MAX_DOF}")
    nodes, err_h = run_h()
    print(f"h : {len(nodes) - 1} elements, sum M = {M0 * (len(nodes) - 1)}, max error {err_h:.3e}")
    nodes, deg, err_hp = run_hp()
    print(f"hp: {len(deg)} elements, degrees {int(deg.min())}..{int(deg.max())}, sum M = {int(deg.sum())}, "
          f"max error {err_hp:.3e}")
    print(f"h / hp max error: {err_h / err_hp:.4g}")


def main():
    global M0, DM, M_MAX
    report()
    M0, DM, M_MAX = 5, 2, 17        # the defaults of section 17: the nodal error of the P1 solve is the floor
    report()


if __name__ == "__main__":
    main()
