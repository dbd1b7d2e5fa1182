"""Time one Newmark step of DESIGN.md section 29 on the GPU: the fused lssvr_wave_advance, the same work as two split
calls of the entry (state only, then the first-step mode), the one-case lssvr_tridiag_bc_solve_multi and, for scale,
lssvr_ts_rhs -- all in the same run, with and without damping bands.  Default shape: 1e6 uniform elements, nc = 1,
R = 1.  Device events around ``--reps`` back-to-back launches after ``--warmup`` warm-up launches; the median of
``--rounds`` such windows.  Prints one JSON line: times in microseconds, the byte model -- (4 + 4 + R + 3) * 8 B per node
with damping, (4 + 2 + R + 3) * 8 without -- and the rates it implies.

    python scripts/time_wave.py [--ne 1000000] [--R 1] [--reps 20] [--rounds 5]
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
    if not torch.cuda.is_available():
        raise SystemExit("time_wave.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, R, dt, beta, gamma = a.ne, a.R, a.dt, 0.25, 0.5
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, 2)
    zq, one = torch.zeros_like(xq), torch.ones_like(xq)
    Mb = ops.p1_assemble(x, 2, rhs_quad=zq, a_quad=zq, c_quad=one)
    Db = ops.p1_assemble(x, 2, rhs_quad=zq, a_quad=zq, c_quad=0.5 * one)
    A = ops.p1_assemble(x, 2, rhs_quad=zq, c_quad=(1.0 / (beta * dt * dt) + gamma * 0.5 / (beta * dt)) * one)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.standard_normal(shape), device=dev)

    U, V, Acc = rand(2, 1, ne + 1), rand(2, 1, ne + 1), rand(2, 1, ne + 1)
    loads, phi, g = rand(R, ne + 1), rand(1, R), torch.zeros((1, 2), dtype=torch.float64, device=dev)
    b = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    work = ops._scratch(None, ops._capi.load().lssvr_tridiag_bc_work_bytes(ne, 1), dev)
    kinds, kappa = (0, 0), (0.0, 0.0)
    md, mo = Mb["diag"], Mb["off"]

    def fused(dd, do):
        ops.wave_advance(U[1], U[0], V[0], Acc[0], md, mo, dd, do, loads, phi, dt, beta, gamma, V_out=V[1],
                         Acc_out=Acc[1], rhs_out=b)

    def split(dd, do):
        ops.wave_advance(U[1], U[0], V[0], Acc[0], None, None, None, None, None, None, dt, beta, gamma, V_out=V[1],
                         Acc_out=Acc[1], rhs=False)
        ops.wave_advance(None, U[1], V[1], Acc[1], md, mo, dd, do, loads, phi, dt, beta, gamma, rhs_out=b)

    damp = (Db["diag"], Db["off"])
    parts = {"advance_fused_damped": lambda: fused(*damp), "advance_split_damped": lambda: split(*damp),
             "advance_fused": lambda: fused(None, None), "advance_split": lambda: split(None, None),
             "solve_bc": lambda: ops.tridiag_bc_solve_multi(A["diag"], A["off"], b, kinds, kappa, g, out=U[1], work=work),
             "ts_rhs": lambda: ops.ts_rhs(md, mo, U[0], U[1], loads, phi, 2.0, -0.5, 1.0 / dt, out=b)}
    out = {"ne": ne, "R": R, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    model = {"advance_fused_damped": (4 + 4 + R + 3) * 8 * (ne + 1), "advance_fused": (4 + 2 + R + 3) * 8 * (ne + 1),
             "ts_rhs": (2 + 2 + R + 1) * 8 * (ne + 1)}
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (out["us"][k] * 1e-6) / 1e12, 3) for k in model}
    out["fused_over_split"] = {k: round(out["us"]["advance_fused" + k] / out["us"]["advance_split" + k], 3)
                               for k in ("", "_damped")}
    out["fused_over_solve"] = round(out["us"]["advance_fused_damped"] / out["us"]["solve_bc"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
