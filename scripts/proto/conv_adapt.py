"""numpy prototype of solve_adaptive on -eps u'' + u' = 1, u(0) = u(1) = 0, eps = 0.02: the loop
of the facade -- non-symmetric P1 bands, banded solve, per-element solve, indicator, threshold marking, bisection -- on
the float64 restatement of oracle/lssvr_oracle.py and tests/convection_rules.py, no GPU.  The enhancement and the
indicator take the folded first-derivative table a' - b.  Prints the element count, the max errors on 20 001 points of
the adapted mesh and of the uniform mesh with the same element count, and their ratio (the bar of
tests/test_gpu_conv.py is this ratio / 10)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lssvr_oracle as orc              # noqa: E402
import convection_rules as cr                       # noqa: E402

M, N, GAMMA, NQUAD, THETA, MAXE, NE0 = 9, 16, 1e10, 5, 0.5, 128, 32


def solve(nodes):
    u = cr.fem_solve(nodes, cr.layer_f, cr.layer_a, cr.layer_b, None, NQUAD)
    return orc.enhance_all(nodes, u, M, GAMMA, N, rhs=cr.layer_f, global_domain=(0.0, 1.0), coef_a=cr.layer_a,
                           coef_da=cr.layer_folded)[0]


def main():
    xq = np.linspace(0, 1, 20001)
    xi, wt = np.polynomial.legendre.leggauss(max(M, 8))
    nodes = np.linspace(0, 1, NE0 + 1)
    print(f"start: {NE0} elements, cell Peclet {cr.cell_peclet(nodes, cr.layer_a, cr.layer_b, NQUAD).max():.4g}")
    while True:
        W = solve(nodes)
        pts = orc.estimate_points(nodes, xi)
        an = cr.layer_a(nodes)
        eta2, _ = orc.estimate_indicator(nodes, W, xi, wt, cr.layer_f(pts), cr.layer_a(pts), cr.layer_folded(pts),
                                         None, np.stack([an[:-1], an[1:]], 1))
        mark = eta2 >= THETA * THETA * eta2.max()
        if len(nodes) - 1 + mark.sum() > MAXE or not mark.any():
            break
        mid = 0.5 * (nodes[:-1] + nodes[1:])[mark]
        nodes = np.sort(np.concatenate([nodes, mid]))
    ne = len(nodes) - 1
    err_a = np.max(np.abs(orc.evaluate_solution_vec(nodes, W, xq)[0] - cr.layer_exact(xq)))
    un = np.linspace(0, 1, ne + 1)
    err_u = np.max(np.abs(orc.evaluate_solution_vec(un, solve(un), xq)[0] - cr.layer_exact(xq)))
    h = np.diff(nodes)
    print(f"adapted: {ne} elements, h in [{h.min():.3e}, {h.max():.3e}], max error {err_a:.3e}")
    print(f"uniform {ne}: max error {err_u:.3e};  ratio {err_u / err_a:.4g}")
    print("nodes right of 0.75:", int(np.sum(nodes[:-1] >= 0.75)), " left of 0.5:", int(np.sum(nodes[1:] <= 0.5)),
          " smallest element touches x = 1:", bool(h[-1] == h.min()))


if __name__ == "__main__":
    main()
