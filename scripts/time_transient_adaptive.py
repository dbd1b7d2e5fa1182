"""Time one attempt of the adaptive loop of DESIGN.md section 30 on the GPU, part by part and whole, next to the
fixed-step step of section 26 in the same run.  Default shape: u_t - u'' = f on 1e6 uniform elements, R = 1.

  ts_step / ts_step_skip   lssvr_ts_step with and without the band writes
  ts_rhs + bands           lssvr_ts_rhs and a separate update of the two bands (two torch.add launches): what ts_step
                           replaces
  ts_error                 lssvr_ts_error (both launches), four vectors
  solve_bc                 the one-case lssvr_tridiag_bc_solve_multi
  attempt                  a whole attempt as solve_transient_adaptive makes it: the upload of the row of R + 2 doubles,
                           ts_step, the solve, ts_error and the read-back of four doubles (a host synchronisation)
  fixed_step               lssvr_ts_rhs + the solve, no copy, no synchronisation: the step of solve_transient

Device events around ``--reps`` back-to-back calls after ``--warmup`` warm-up calls; the median of ``--rounds`` such
windows.  Prints one JSON line: times in microseconds, the byte models -- ts_step reads 4 bands, 2 U rows and R loads and
writes 2 bands and 1 right-hand side, (9 + R) * 8 B per node, (5 + R) * 8 B without the band writes; ts_error reads
4 * 8 B per node (3 * 8 at step 2) -- and the rates they imply.

    python scripts/time_transient_adaptive.py [--ne 1000000] [--R 1] [--reps 20] [--rounds 5]
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
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    from hybrid_fem_lssvr_amd.solver import ts_coefficients, ts_error_weights
    if not torch.cuda.is_available():
        raise SystemExit("time_transient_adaptive.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, R = a.ne, a.R
    h, hp, hpp = a.dt, 0.8 * a.dt, 0.7 * a.dt
    al, b0, b1 = ts_coefficients(h / hp)
    inv_h, s = 1.0 / h, al / h
    w = ts_error_weights(h, hp, hpp, al)
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, 2)
    zq, one = torch.zeros_like(xq), torch.ones_like(xq)
    Mb = ops.p1_assemble(x, 2, rhs_quad=zq, a_quad=zq, c_quad=one)
    Kb = ops.p1_assemble(x, 2, rhs_quad=zq, c_quad=zq)
    md, mo, kd, ko = Mb["diag"], Mb["off"], Kb["diag"], Kb["off"]
    adiag, aoff = torch.empty_like(kd), torch.empty_like(ko)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.standard_normal(shape), device=dev)

    U = rand(4, ne + 1)
    loads = rand(R, ne + 1)
    row = torch.zeros(R + 2, dtype=torch.float64, device=dev)
    phi, g = row[:R].unsqueeze(0), row[R:].unsqueeze(0)
    host_row = np.concatenate([rng.standard_normal(R), np.zeros(2)])
    b = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    out4 = torch.zeros(4, dtype=torch.float64, device=dev)
    work = ops._scratch(None, ops._capi.load().lssvr_tridiag_bc_work_bytes(ne, 1), dev)
    ework = ops._scratch(None, ops._capi.load().lssvr_ts_error_work_bytes(ne), dev)
    kinds, kappa = (0, 0), (0.0, 0.0)

    def step(write=True):
        ops.ts_step(kd, ko, md, mo, U[1:2], U[2:3], loads, phi, s, b0, b1, inv_h, adiag=adiag, aoff=aoff,
                    write_bands=write, out=b)

    def rhs():
        ops.ts_rhs(md, mo, U[1:2], U[2:3], loads, phi, b0, b1, inv_h, out=b)

    def rhs_and_bands():
        rhs()
        torch.add(kd, md, alpha=s, out=adiag)
        torch.add(ko, mo, alpha=s, out=aoff)

    def solve():
        ops.tridiag_bc_solve_multi(adiag, aoff, b, kinds, kappa, g, out=U[0:1], work=work)

    def error():
        ops.ts_error(U[0], U[1], U[2], U[3], w, 1e-6, 1e-6, kinds, out4=out4, work=ework)

    def attempt():
        row.copy_(torch.from_numpy(host_row))
        step()
        solve()
        error()
        return out4.cpu()

    def fixed_step():
        rhs()
        solve()

    step()                                              # the bands of the solve
    parts = {"ts_step": step, "ts_step_skip": lambda: step(False), "ts_rhs": rhs, "ts_rhs+bands": rhs_and_bands,
             "ts_error": error, "solve_bc": solve, "attempt": attempt, "fixed_step": fixed_step}
    out = {"ne": ne, "R": R, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    n = ne + 1
    model = {"ts_step": (9 + R) * 8 * n, "ts_step_skip": (5 + R) * 8 * n, "ts_rhs": (5 + R) * 8 * n,
             "ts_error": 4 * 8 * n}
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (out["us"][k] * 1e-6) / 1e12, 3) for k in model}
    out["attempt_over_fixed_step"] = round(out["us"]["attempt"] / out["us"]["fixed_step"], 3)
    out["ts_step_over_rhs_plus_bands"] = round(out["us"]["ts_step"] / out["us"]["ts_rhs+bands"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
