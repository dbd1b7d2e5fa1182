"""numpy prototype of solve_adaptive(mode="hp") on the test problem of DESIGN.md section 11, -u'' = f with
u = atan(50 x) - x atan(50): the loop of the facade -- P1 solve, per-element solve with each
element's own degree and max(16, 2 M) collocation points, indicator, decay rate, raise or bisect -- on the float64
restatement of oracle/lssvr_oracle.py and the rules of tests/hp_rules.py, no GPU.  Prints, for the h-only runs from
degree 5 and 9 and the hp run from degree 5, under a budget of sum M_e <= 600 coefficients: elements, sum M_e, the
max error on 20 001 points and the estimate (the bar of tests/test_gpu_hp.py is the h / hp error ratio / 10)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lssvr_oracle as orc              # noqa: E402
import hp_rules                                     # noqa: E402

GAMMA, NQUAD, THETA, N0, BUDGET, GD = 1e10, 5, 0.5, 16, 600, (-1.0, 1.0)
A50 = math.atan(50.0)


def exact(x):
    return np.arctan(50.0 * x) - x * A50


def f(x):
    x = np.asarray(x, dtype=np.float64)
    return 250000.0 * x / (1.0 + 2500.0 * x * x) ** 2


def solve(nodes, deg):
    """Zero-padded W[ne, max M] of the mesh: every element at its own degree."""
    u = orc.fem_p1_solve(nodes, f, None, NQUAD)
    ne = len(nodes) - 1
    W = np.zeros((ne, int(deg.max())))
    for i in range(ne):
        M = int(deg[i])
        gl, gr = orc.boundary_values(i, ne, nodes[i], nodes[i + 1], u[i], u[i + 1], GD)
        W[i, :M] = orc.solve_primal_kkt(orc.element_system(nodes[i], nodes[i + 1], gl, gr, M, GAMMA,
                                                           hp_rules.n_colloc(N0, M), rhs=f))
    return W


def adapt(M0, sigma_min, dM=2, M_max=21, log=False):
    nodes, deg = np.linspace(-1, 1, 9), np.full(8, M0, dtype=np.int32)
    while True:
        W = solve(nodes, deg)
        xi, wt = np.polynomial.legendre.leggauss(min(32, max(int(deg.max()), 8)))
        eta2, _ = orc.estimate_indicator(nodes, W, xi, wt, f(orc.estimate_points(nodes, xi)))
        est = math.sqrt(eta2.sum())
        sig = hp_rules.smoothness(W, deg)
        xn, dn, _, (ns, nr) = hp_rules.refine_hp(nodes, eta2, eta2.max(), THETA, 0.0, sig, deg, sigma_min, dM, M_max)
        if log:
            print(f"  ne {len(deg):4d}  dof {int(deg.sum()):4d}  estimate {est:.3e}  bisected {ns:3d}  raised {nr:3d}")
        if ns + nr == 0 or dn.sum() > BUDGET:
            return nodes, deg, W, est
        nodes, deg = xn, dn


def main():
    xq = np.linspace(-1, 1, 20001)
    out = {}
    for tag, M0, smin in (("h  from 5", 5, np.inf), ("h  from 9", 9, np.inf), ("hp from 5", 5, 1.0)):
        nodes, deg, W, est = adapt(M0, smin, log=tag.startswith("hp"))
        err = np.max(np.abs(orc.evaluate_solution_vec(nodes, W, xq)[0] - exact(xq)))
        out[tag] = err
        print(f"{tag}: {len(deg)} elements, sum M = {int(deg.sum())}, degrees {int(deg.min())}..{int(deg.max())}, "
              f"max error {err:.3e}, estimate {est:.3e}")
    print(f"h / hp max error from degree 5: {out['h  from 5'] / out['hp from 5']:.4g}")


if __name__ == "__main__":
    main()
