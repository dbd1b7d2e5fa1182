"""Time lssvr_semilinear_sensitivity on the GPU beside the entries it runs next to, in one run:
lssvr_p1_sensitivity (all four tables), lssvr_nl_linearize (c_eff alone, as the facade calls it at u*), the one-case
lssvr_tridiag_bc_solve_multi and one whole Newton iteration (linearize -> reaction assembly -> one-case solve ->
linearize f_res -> load -> residual, without the read-back: scripts/time_semilinear.py).  Default shape: 1e6 uniform
elements, nquad = 2, nc = 1, POLY with four terms, all 4 + nterm tables and then gq alone.  Device events around
``--reps`` back-to-back launches after ``--warmup`` warm-up launches; the median of ``--rounds`` such windows.  Prints
one JSON line: times in microseconds, the byte model -- per element 3 * 8 B of x, u, z read and nquad * 8 B written
per table -- the rate it implies, and the ratio to each reference entry.

    python scripts/time_semilinear_sensitivity.py [--ne 1000000] [--nquad 2] [--nterm 4] [--reps 20] [--rounds 5]
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
    ap.add_argument("--nquad", type=int, default=2)
    ap.add_argument("--nterm", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("time_semilinear_sensitivity.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, nq, nt = a.ne, a.nquad, a.nterm
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, nq)
    zq, one = torch.zeros_like(xq), torch.ones_like(xq)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.uniform(0.0, 1.0, shape), device=dev)

    u, z = rand(1, ne + 1), rand(1, ne + 1)
    tq = ops.quad_points(torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev), nq)[0].contiguous()
    qq, fq = rand(nt, ne, nq), rand(ne, nq)
    ce, fe, fr = (torch.empty_like(fq) for _ in range(3))
    K = ops.p1_assemble(x, nq, rhs_quad=zq, c_quad=one)
    bands = ops.p1_assemble(x, nq, rhs_quad=fq, c_quad=one)
    outs = {k: torch.empty((1, ne, nq), dtype=torch.float64, device=dev) for k in ops.SENS_TABLES}
    outs["q"] = torch.empty((1, nt, ne, nq), dtype=torch.float64, device=dev)
    load = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    out4 = torch.empty(4, dtype=torch.float64, device=dev)
    g = torch.zeros((1, 2), dtype=torch.float64, device=dev)
    sol = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    lib = ops._capi.load()
    swork = ops._scratch(None, lib.lssvr_tridiag_bc_work_bytes(ne, 1), dev)
    rwork = ops._scratch(None, lib.lssvr_nl_residual_work_bytes(ne), dev)
    kinds, kappa = (0, 0), (0.0, 0.0)

    def nl_sens(want):
        out = {k: outs[k] for k in want}
        return lambda: ops.nl_sensitivity(x, u, z, nq, ops.NL_POLY, nt, want=want, out=out)

    def p1_sens():
        ops.p1_sensitivity(x, u, z, nq, out={k: outs[k] for k in ops.SENS_TABLES})

    def linearize():
        ops.nl_linearize(u[0], tq, ops.NL_POLY, qq, fq, c_tab=one, c_eff=ce, f_eff=None, f_res=None)

    def solve():
        ops.tridiag_bc_solve_multi(bands["diag"], bands["off"], bands["load"].unsqueeze(0), kinds, kappa, g, out=sol,
                                   work=swork)

    def iteration():
        ops.nl_linearize(u[0], tq, ops.NL_POLY, qq, fq, c_tab=one, c_eff=ce, f_eff=fe, f_res=None)
        ops.p1_assemble(x, nq, rhs_quad=fe, c_quad=ce, out=bands)
        solve()
        ops.nl_linearize(u[0], tq, ops.NL_POLY, qq, fq, c_tab=one, c_eff=None, f_eff=None, f_res=fr)
        ops.p1_load_multi(x, fr.unsqueeze(0), nq, out=load)
        ops.nl_residual(K["diag"], K["off"], K["off"], load[0], u[0], sol[0], kinds, kappa, out4=out4, work=rwork)

    parts = {"nl_sens_all": nl_sens(ops.NL_SENS_TABLES), "nl_sens_gq": nl_sens(("q",)), "p1_sens_all": p1_sens,
             "nl_linearize_c_eff": linearize, "solve_bc": solve, "newton_iteration": iteration}
    model = {"nl_sens_all": 8 * (3 * (ne + 1) + (4 + nt) * ne * nq), "nl_sens_gq": 8 * (3 * (ne + 1) + nt * ne * nq),
             "p1_sens_all": 8 * (3 * (ne + 1) + 4 * ne * nq)}
    out = {"ne": ne, "nquad": nq, "nterm": nt, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (out["us"][k] * 1e-6) / 1e12, 3) for k in model}
    for ref in ("p1_sens_all", "nl_linearize_c_eff", "solve_bc", "newton_iteration"):
        out["over_" + ref] = {k: round(out["us"][k] / out["us"][ref], 3) for k in ("nl_sens_all", "nl_sens_gq")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
