"""Time the parts of one Newton iteration of DESIGN.md section 27 on the GPU: lssvr_nl_linearize at the 2 quadrature
points (c_eff and f_eff) and at 16 collocation points, lssvr_nl_residual, one whole Newton iteration (linearize ->
reaction assembly -> one-case solve -> linearize f_res -> load -> residual, without the read-back) and, beside them in
the same run, the one-case lssvr_tridiag_bc_solve_multi.  Default shape: -u'' + u^3 = f on 1e6 uniform elements, POLY
with four terms.  Device events around ``--reps`` back-to-back launches after ``--warmup`` warm-up launches; the median
of ``--rounds`` such windows.  Prints one JSON line: times in microseconds, the byte model of nl_linearize -- (nterm + 2)
tables in (without c_tab: nterm + 1), the tables written out, plus u -- and the rates and ratios they imply.

    python scripts/time_semilinear.py [--ne 1000000] [--nterm 4] [--n-colloc 16] [--reps 20] [--rounds 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.time_eigen import window         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=1000000)
    ap.add_argument("--nterm", type=int, default=4)
    ap.add_argument("--n-colloc", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("time_semilinear.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, nt, n = a.ne, a.nterm, a.n_colloc
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, 2)
    zq, one = torch.zeros_like(xq), torch.ones_like(xq)
    K = ops.p1_assemble(x, 2, rhs_quad=zq, c_quad=one)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.uniform(0.0, 1.0, shape), device=dev)

    u, u_new = rand(ne + 1), rand(ne + 1)
    tq = ops.quad_points(torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev), 2)[0].contiguous()
    tc = torch.arange(n, dtype=torch.float64, device=dev) / float(n - 1)
    qq, fq, cq = rand(nt, ne, 2), rand(ne, 2), one
    qc, fc, cc = rand(nt, n, ne), rand(n, ne), torch.ones((n, ne), dtype=torch.float64, device=dev)
    ce_q, fe_q, fr_q = (torch.empty_like(fq) for _ in range(3))
    ce_c, fe_c = (torch.empty_like(fc) for _ in range(2))
    bands = ops.p1_assemble(x, 2, rhs_quad=fq, c_quad=cq)
    load = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    out4 = torch.empty(4, dtype=torch.float64, device=dev)
    g = torch.zeros((1, 2), dtype=torch.float64, device=dev)
    sol = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    lib = ops._capi.load()
    swork = ops._scratch(None, lib.lssvr_tridiag_bc_work_bytes(ne, 1), dev)
    rwork = ops._scratch(None, lib.lssvr_nl_residual_work_bytes(ne), dev)
    kinds, kappa = (0, 0), (0.0, 0.0)

    def lin_quad():
        ops.nl_linearize(u, tq, ops.NL_POLY, qq, fq, c_tab=cq, c_eff=ce_q, f_eff=fe_q, f_res=None)

    def lin_colloc():
        ops.nl_linearize(u, tc, ops.NL_POLY, qc, fc, c_tab=cc, point_major=True, c_eff=ce_c, f_eff=fe_c, f_res=None)

    def residual():
        ops.nl_residual(K["diag"], K["off"], K["off"], load[0], u, u_new, kinds, kappa, out4=out4, work=rwork)

    def solve():
        ops.tridiag_bc_solve_multi(bands["diag"], bands["off"], bands["load"].unsqueeze(0), kinds, kappa, g, out=sol,
                                   work=swork)

    def iteration():
        lin_quad()
        ops.p1_assemble(x, 2, rhs_quad=fe_q, c_quad=ce_q, out=bands)
        solve()
        ops.nl_linearize(u, tq, ops.NL_POLY, qq, fq, c_tab=cq, c_eff=None, f_eff=None, f_res=fr_q)
        ops.p1_load_multi(x, fr_q.unsqueeze(0), 2, out=load)
        ops.nl_residual(K["diag"], K["off"], K["off"], load[0], u, sol[0], kinds, kappa, out4=out4, work=rwork)

    parts = {"nl_linearize_quad2": lin_quad, f"nl_linearize_colloc{n}": lin_colloc, "nl_residual": residual,
             "solve_bc": solve, "newton_iteration": iteration}
    out = {"ne": ne, "nterm": nt, "n_colloc": n, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    model = {"nl_linearize_quad2": (nt + 2 + 2) * 8 * ne * 2 + 8 * (ne + 1),
             f"nl_linearize_colloc{n}": (nt + 2 + 2) * 8 * ne * n + 8 * (ne + 1),
             "nl_residual": 6 * 8 * (ne + 1)}
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (out["us"][k] * 1e-6) / 1e12, 3) for k in model}
    out["over_solve"] = {k: round(v / out["us"]["solve_bc"], 3) for k, v in out["us"].items() if k != "solve_bc"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
