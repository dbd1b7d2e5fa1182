"""numpy prototype of solve_adaptive on -eps u'' + u = 1, u(+-1) = 0: the loop of the facade
-- P1 with mass matrix, per-element solve, indicator, threshold marking, bisection -- on the float64 restatement
of oracle/lssvr_oracle.py, no GPU.  Prints the element count, the max errors on 20 001 points of the adapted
and of the uniform 128-element solve, and their ratio (the bar of tests/test_gpu_react.py is this ratio / 5)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import lssvr_oracle as orc              # noqa: E402

EPS, M, N, GAMMA, NQUAD, THETA, MAXE = 1e-4, 9, 16, 1e10, 5, 0.5, 128
a = lambda x: EPS + 0.0 * np.asarray(x, dtype=np.float64)          # noqa: E731
da = lambda x: 0.0 * np.asarray(x, dtype=np.float64)               # noqa: E731
c = lambda x: 1.0 + 0.0 * np.asarray(x, dtype=np.float64)          # noqa: E731
f = c


def exact(x):
    r = 1.0 / math.sqrt(EPS)
    return 1.0 - (np.exp(r * (x - 1.0)) + np.exp(-r * (x + 1.0))) / (1.0 + math.exp(-2.0 * r))


def solve(nodes):
    u = orc.fem_p1_solve(nodes, f, a, NQUAD, c)
    return orc.enhance_all(nodes, u, M, GAMMA, N, rhs=f, global_domain=(-1.0, 1.0), coef_a=a, coef_da=da, coef_c=c)[0]


def main():
    xq = np.linspace(-1, 1, 20001)
    xi, wt = np.polynomial.legendre.leggauss(max(M, 8))
    nodes = np.linspace(-1, 1, 9)
    while True:
        W = solve(nodes)
        pts = orc.estimate_points(nodes, xi)
        an = a(nodes)
        eta2, _ = orc.estimate_indicator(nodes, W, xi, wt, f(pts), a(pts), da(pts), c(pts),
                                         np.stack([an[:-1], an[1:]], 1))
        mark = eta2 >= THETA * THETA * eta2.max()
        if len(nodes) - 1 + mark.sum() > MAXE or not mark.any():
            break
        mid = 0.5 * (nodes[:-1] + nodes[1:])[mark]
        nodes = np.sort(np.concatenate([nodes, mid]))
    err_a = np.max(np.abs(orc.evaluate_solution_vec(nodes, W, xq)[0] - exact(xq)))
    un = np.linspace(-1, 1, 129)
    err_u = np.max(np.abs(orc.evaluate_solution_vec(un, solve(un), xq)[0] - exact(xq)))
    h = np.diff(nodes)
    print(f"adapted: {len(nodes) - 1} elements, h in [{h.min():.3e}, {h.max():.3e}], max error {err_a:.3e}")
    print(f"uniform 128: max error {err_u:.3e};  ratio {err_u / err_a:.4g}")
    print("nodes left of -0.5:", int(np.sum(nodes[1:] <= -0.5)), " right of 0.5:", int(np.sum(nodes[:-1] >= 0.5)))


if __name__ == "__main__":
    main()
