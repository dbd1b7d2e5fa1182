"""numpy prototype of solve_goal and solve_adaptive(goal=j) on the test problem of DESIGN.md section 11, -u'' = f with
u = atan(50 x) - x atan(50), for J(u) = int j u dx with j a Gaussian bump: the loop of the facade
-- P1 solves of the primal and the dual problem, per-element solves, dual-weighted residual, threshold marking from
its jump-free form int_e R (z - I_h z), bisection -- on the float64 restatement of oracle/lssvr_oracle.py and
tests/goal_rules.py, no GPU.  Prints
  1. on uniform meshes of 8 .. 64 elements: |J(u) - J(u_enh)|, |J(u) - corrected| and their ratio (the bar rho of
     tests/test_gpu_goal.py is 10 x the worst ratio),
  2. from the same 8-element start, the goal-oriented and the residual-driven loop stopped at the same max_elements:
     |J(u) - J(u_enh)| of both, their element counts and their ratio, at several values of max_elements (the bar r
     of the test is the ratio at its max_elements / 10).  --split-marking marks from the full eta_e instead, with
     its halves of the jumps: the loop that stalls."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import lssvr_oracle as orc              # noqa: E402
import goal_rules                                   # noqa: E402

M, N, GAMMA, NQUAD, THETA, NQ, GD = 5, 16, 1e10, 5, 0.25, 16, (-1.0, 1.0)
MAXE = 48
JUMP_FREE = "--split-marking" not in sys.argv
A50 = math.atan(50.0)
CENTRE, WIDTH = 0.3, 0.3                            # the bump of the tests: the best of --scan, see main()


def exact(x):
    return np.arctan(50.0 * x) - x * A50


def f(x):
    x = np.asarray(x, dtype=np.float64)
    return 250000.0 * x / (1.0 + 2500.0 * x * x) ** 2


def bump(centre, width):
    def j(x):
        x = np.asarray(x, dtype=np.float64)
        return np.exp(-((x - centre) / width) ** 2)
    return j


def J_exact(j):
    """J(u) by a 200-point Gauss rule per element of a uniform 4096-element mesh."""
    xi, wt = np.polynomial.legendre.leggauss(200)
    nodes = np.linspace(-1.0, 1.0, 4097)
    xq = orc.estimate_points(nodes, xi)
    return math.fsum((0.5 * np.diff(nodes) * ((j(xq) * exact(xq)) @ wt)).tolist())


def solve(nodes, rhs):
    u = orc.fem_p1_solve(nodes, rhs, None, NQUAD)
    return orc.enhance_all_vec(nodes, u, M, GAMMA, N, rhs=rhs, global_domain=GD)


def goal_round(nodes, j):
    """(value, eta, marking eta) of one solve_goal on ``nodes``."""
    Wu, Wz = solve(nodes, f), solve(nodes, j)
    xi, wt = np.polynomial.legendre.leggauss(NQ)
    pts = orc.estimate_points(nodes, xi)
    eta, q, _ = goal_rules.estimate_goal(nodes, Wu, Wz, xi, wt, f(pts), j(pts))
    mark = eta
    if JUMP_FREE:
        mark = goal_rules.estimate_goal(nodes, Wu, Wz, xi, wt, f(pts), j(pts), jump_free=True)[0]
    return math.fsum(q.tolist()), eta, mark


def value_of(nodes, W, j):
    xi, wt = np.polynomial.legendre.leggauss(NQ)
    L = orc.legendre_tables(xi, M)[0]
    return math.fsum((0.5 * np.diff(nodes) * ((j(orc.estimate_points(nodes, xi)) * (W @ L.T)) @ wt)).tolist())


def bisect(nodes, eta2):
    mark = eta2 >= THETA * THETA * eta2.max()
    return np.sort(np.concatenate([nodes, 0.5 * (nodes[:-1] + nodes[1:])[mark]])), int(mark.sum())


def adapt_goal(j, maxe=MAXE):
    nodes = np.linspace(-1, 1, 9)
    while True:
        value, eta, mark = goal_round(nodes, j)
        new, n = bisect(nodes, mark * mark)
        if n == 0 or len(new) - 1 > maxe:
            return nodes, value, eta
        nodes = new


def adapt_residual(j, maxe=MAXE):
    nodes = np.linspace(-1, 1, 9)
    xi, wt = np.polynomial.legendre.leggauss(NQ)
    while True:
        W = solve(nodes, f)
        eta2, _ = orc.estimate_indicator(nodes, W, xi, wt, f(orc.estimate_points(nodes, xi)))
        new, n = bisect(nodes, eta2)
        if n == 0 or len(new) - 1 > maxe:
            return nodes, value_of(nodes, W, j)
        nodes = new


def effectivity(j, Ju, log=False):
    worst = 0.0
    for ne in (8, 16, 32, 64):
        value, eta, _ = goal_round(np.linspace(-1, 1, ne + 1), j)
        corr = math.fsum(eta.tolist())
        e0, e1 = abs(Ju - value), abs(Ju - (value + corr))
        worst = max(worst, e1 / e0)
        if log:
            print(f"  ne {ne:3d}  J(u_enh) {value:+.12e}  |J - value| {e0:.3e}  |J - corrected| {e1:.3e}  "
                  f"ratio {e1 / e0:.3e}  sum|eta| {np.abs(eta).sum():.3e}")
    return worst


def main():
    if "--scan" in sys.argv:                 # how the bump was chosen
        for centre in (0.02, 0.1, 0.2, 0.3, 0.5, 0.9):
            for width in (0.02, 0.05, 0.1, 0.2, 0.3):
                j = bump(centre, width)
                Ju = J_exact(j)
                rho = effectivity(j, Ju)
                _, vg, _ = adapt_goal(j)
                _, vr = adapt_residual(j)
                print(f"centre {centre} width {width}: J {Ju:+.6e} rho {rho:.3e} "
                      f"goal err {abs(Ju - vg):.3e} residual err {abs(Ju - vr):.3e} "
                      f"gain {abs(Ju - vr) / abs(Ju - vg):.4g}")
        return
    j = bump(CENTRE, WIDTH)
    Ju = J_exact(j)
    print(f"bump centre {CENTRE} width {WIDTH}: J(u) = {Ju:+.15e}")
    value8 = goal_round(np.linspace(-1, 1, 9), j)[0]
    print(f"|J(u) - J(u_enh)| at 8 elements / (eps |J|) = {abs(Ju - value8) / (np.finfo(float).eps * abs(Ju)):.3e} "
          "(needs >= 1e6)")
    print("1. uniform meshes")
    rho = effectivity(j, Ju, log=True)
    print(f"   worst |J - corrected| / |J - value| = {rho:.4g}  ->  bar rho = {10 * rho:.4g} (must be < 1)")
    print(f"2. adaptive, theta = {THETA}" + ("" if JUMP_FREE else ", marking from the full eta (split jumps)"))
    for maxe in (32, 48, 64, 80, 100, 128):
        ng, vg, eta = adapt_goal(j, maxe)
        nr, vr = adapt_residual(j, maxe)
        gain = abs(Ju - vr) / abs(Ju - vg)
        print(f"   max_elements {maxe:3d}: goal {len(ng) - 1:3d} elements |J - value| {abs(Ju - vg):.3e} sum|eta| "
              f"{np.abs(eta).sum():.3e};  residual {len(nr) - 1:3d} elements |J - value| {abs(Ju - vr):.3e};  "
              f"residual / goal = {gain:.4g}"
              + (f"  ->  bar r = {gain / 10:.4g} (must be > 1)" if maxe == MAXE else ""))


if __name__ == "__main__":
    main()
