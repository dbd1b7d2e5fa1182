"""Time one Newton iteration of a semilinear BDF2 step on the GPU: lssvr_ts_nl_assemble against
the three-call chain it replaces (lssvr_nl_linearize -> lssvr_p1_assemble_react -> r + load) in the same run, plus the
whole iteration (assemble, lssvr_tridiag_bc_solve_multi, lssvr_nl_residual) and the whole step (lssvr_ts_rhs, the
extrapolated start and ``--iters`` iterations).  Default shape: 1e6 uniform elements, nquad 2, POLY with 4 terms.  Device
events around ``--reps`` back-to-back launches after ``--warmup`` warm-up launches; the median of ``--rounds`` such
windows.  Prints one JSON line: times in microseconds, the byte models -- the fused kernel reads x, u, r and nterm + 2
tables and writes three bands; the chain writes and reads two more tables and its add streams three more arrays -- and
the rates they imply.

    python scripts/time_transient_nl.py [--ne 1000000] [--nterm 4] [--nquad 2] [--iters 3] [--reps 20] [--rounds 5]
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
    ap.add_argument("--nquad", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("time_transient_nl.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, nq, nterm = a.ne, a.nquad, a.nterm
    al, b0, b1 = ops.BDF["bdf2"]
    inv_dt = 1.0 / a.dt
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, nq)
    zq, one = torch.zeros_like(xq), torch.ones_like(xq)
    Mb = ops.p1_assemble(x, nq, rhs_quad=zq, a_quad=zq, c_quad=one)
    cs = (al * inv_dt) * one
    t = ops.quad_points(torch.as_tensor([0.0, 1.0], dtype=torch.float64, device=dev), nq)[0].contiguous()
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.uniform(0.0, 1.0, shape), device=dev)

    U, V = rand(3, ne + 1), rand(2, ne + 1)
    q = rand(nterm, ne, nq)
    loads, phi, g = rand(1, ne + 1), rand(1, 1), torch.zeros((1, 2), dtype=torch.float64, device=dev)
    b = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    rhs = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    nb = dict(diag=torch.empty(ne + 1, dtype=torch.float64, device=dev),
              off=torch.empty(ne, dtype=torch.float64, device=dev), rhs=rhs[0])
    c_eff, f_eff = torch.empty_like(xq), torch.empty_like(xq)
    chain_bands, chain_rhs = None, torch.empty(ne + 1, dtype=torch.float64, device=dev)
    out4 = torch.empty(4, dtype=torch.float64, device=dev)
    lib = ops._capi.load()
    work = ops._scratch(None, lib.lssvr_tridiag_bc_work_bytes(ne, 1), dev)
    rwork = ops._scratch(None, lib.lssvr_nl_residual_work_bytes(ne), dev)
    kinds, kappa = (0, 0), (0.0, 0.0)
    ops.ts_rhs(Mb["diag"], Mb["off"], U[0:1], U[1:2], loads, phi, b0, b1, inv_dt, out=b)

    def fused(v=V[0]):
        ops.ts_nl_assemble(x, v, cs, "poly", q, b[0], out=nb)

    def chain():
        nonlocal chain_bands
        ops.nl_linearize(V[0], t, "poly", q, zq, c_tab=cs, c_eff=c_eff, f_eff=f_eff)
        chain_bands = ops.p1_assemble(x, nq, rhs_quad=f_eff, c_quad=c_eff, out=chain_bands)
        torch.add(b[0], chain_bands["load"], out=chain_rhs)

    def iteration(v=V[0], tgt=V[1]):
        fused(v)
        ops.tridiag_bc_solve_multi(nb["diag"], nb["off"], rhs, kinds, kappa, g, out=tgt.unsqueeze(0), work=work)
        ops.nl_residual(nb["diag"], nb["off"], nb["off"], nb["rhs"], v, tgt, kinds, kappa, g[0], out4=out4, work=rwork)

    def step():
        ops.ts_rhs(Mb["diag"], Mb["off"], U[0:1], U[1:2], loads, phi, b0, b1, inv_dt, out=b)
        ops.nl_step(U[1], U[0], 2.0, out=V[0])
        v, spare = V[0], V[1]
        for k in range(a.iters):
            tgt = U[2] if k == a.iters - 1 else spare
            iteration(v, tgt)
            v, spare = tgt, v

    parts = {"ts_nl_assemble": fused, "chain": chain, "iteration": iteration, "step": step}
    out = {"ne": ne, "nterm": nterm, "nquad": nq, "iters": a.iters, "reps": a.reps, "rounds": a.rounds, "us": {},
           "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    fused_bytes = 8 * (3 * (ne + 1) + (nterm + 1) * ne * nq + (2 * (ne + 1) + ne))      # (a_quad NULL: nterm + 1 tables)
    model = {"ts_nl_assemble": fused_bytes, "chain": fused_bytes + 8 * (4 * ne * nq + 3 * (ne + 1))}
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (out["us"][k] * 1e-6) / 1e12, 3) for k in model}
    out["chain_over_fused"] = round(out["us"]["chain"] / out["us"]["ts_nl_assemble"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
