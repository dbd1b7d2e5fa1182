"""Time one BDF2 step of DESIGN.md section 26 on the GPU, split into its two parts: lssvr_ts_rhs and the one-case
lssvr_tridiag_bc_solve_multi, plus the whole step (both, back to back) and one lssvr_ts_source_table.  Default shape:
u_t - u'' = f on 1e6 uniform elements, nc = 1, R = 1.  Device events around ``--reps`` back-to-back launches after
``--warmup`` warm-up launches; the median of ``--rounds`` such windows.  Prints one JSON line: times in microseconds,
the byte models -- (2 + 2 + R + 1) * 8 B per node for the right-hand side, R + 1 tables in and one out for the source
table -- and the rates they imply.

    python scripts/time_transient.py [--ne 1000000] [--R 1] [--n-colloc 16] [--reps 20] [--rounds 5]
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
    ap.add_argument("--R", type=int, default=1)
    ap.add_argument("--n-colloc", type=int, default=16)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("time_transient.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, R, n = a.ne, a.R, a.n_colloc
    al, b0, b1 = ops.BDF["bdf2"]
    inv_dt = 1.0 / a.dt
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, 2)
    zq, one = torch.zeros_like(xq), torch.ones_like(xq)
    Mb = ops.p1_assemble(x, 2, rhs_quad=zq, a_quad=zq, c_quad=one)
    A = ops.p1_assemble(x, 2, rhs_quad=zq, c_quad=(al * inv_dt) * one)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.standard_normal(shape), device=dev)

    U = rand(3, ne + 1)
    loads, phi, g = rand(R, ne + 1), rand(1, R), torch.zeros((1, 2), dtype=torch.float64, device=dev)
    b = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    ftab, rtab = rand(R, n, ne), torch.ones((n, ne), dtype=torch.float64, device=dev)
    src = torch.empty_like(rtab)
    work = ops._scratch(None, ops._capi.load().lssvr_tridiag_bc_work_bytes(ne, 1), dev)
    kinds, kappa = (0, 0), (0.0, 0.0)

    def rhs():
        ops.ts_rhs(Mb["diag"], Mb["off"], U[0:1], U[1:2], loads, phi, b0, b1, inv_dt, out=b)

    def solve():
        ops.tridiag_bc_solve_multi(A["diag"], A["off"], b, kinds, kappa, g, out=U[2:3], work=work)

    def step():
        rhs()
        solve()

    parts = {"ts_rhs": rhs, "solve_bc": solve, "step": step,
             "ts_source_table": lambda: ops.ts_source_table(U[2], U[0], U[1], ftab, rtab, phi[0], al, b0, b1, inv_dt,
                                                            point_major=True, out=src)}
    out = {"ne": ne, "R": R, "n_colloc": n, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    model = {"ts_rhs": (2 + 2 + R + 1) * 8 * (ne + 1), "ts_source_table": (R + 2) * 8 * ne * n}
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (out["us"][k] * 1e-6) / 1e12, 3) for k in model}
    out["rhs_over_solve"] = round(out["us"]["ts_rhs"] / out["us"]["solve_bc"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
