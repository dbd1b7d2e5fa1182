"""Time the two kernels of the semilinear transient sensitivities on the GPU beside what they
replace and what they run next to, all in the same run, at 1e5 and 1e6 uniform elements, nquad = 2, POLY nterm = 4:

  the backward step   lssvr_semilinear_adjoint_step against the chain it replaces: lssvr_ts_rhs + lssvr_ts_nl_assemble
                      (whose Newton load is not needed) + the two slices that fill the band_ends row;
  the chunk pass      lssvr_semilinear_transient_sensitivity, m = 8, R = 1, accumulate, all outputs, with and without gq;
  one backward level  adjoint step + solve + 1/8 of the chunk pass, against one forward step of 3 Newton iterations
                      (ts_rhs + 3 x (ts_nl_assemble + solve + nl_residual)).

Device events around ``--reps`` back-to-back calls after ``--warmup`` warm-up calls; the median of ``--rounds`` such
windows.  Prints one JSON line per size: times in microseconds and the byte models -- the step reads per node x, u, two
mass bands, two adjoint states and the row p_n and per element (2 + nterm) nquad table entries, and writes diag, off, B;
the chunk pass as in scripts/time_transient_sensitivity.py plus nterm nquad 8 B per element written and read again for
gq.  Run it under a time limit of its own:

    timeout -k 10 300 python scripts/time_transient_nl_sensitivity.py [--ne 100000 1000000] [--reps 20] [--rounds 5]
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


def measure(ne, a):
    import torch
    from hybrid_fem_lssvr_amd import ops
    dev = torch.device("cuda:0")
    nq, nterm, R, N, m = 2, 4, 1, 10, 8
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    one = torch.ones((ne, nq), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.standard_normal(shape), device=dev)

    inv_dt = 100.0
    mass = ops.p1_assemble(x, nq, rhs_quad=one, a_quad=0.0 * one, c_quad=one)
    md, mo = mass["diag"], mass["off"]
    cs = (1.0 + 1.5 * inv_dt) * one
    q = torch.stack([0.2 * one, 0.4 * one, 0.1 * one, 1.0 * one])
    Utraj, Z, B, phi = 0.5 * rand(N + 1, ne + 1), rand(m, ne + 1), rand(m, ne + 1), rand(N, R)
    P, ph1 = rand(1, ne + 1), torch.ones((1, 1), dtype=torch.float64, device=dev)
    band_ends = torch.zeros((m, 2), dtype=torch.float64, device=dev)
    jac = dict(diag=torch.empty(ne + 1, dtype=torch.float64, device=dev),
               off=torch.empty(ne, dtype=torch.float64, device=dev))
    nb = dict(jac, rhs=torch.empty(ne + 1, dtype=torch.float64, device=dev))
    b1, u1 = (torch.empty((1, ne + 1), dtype=torch.float64, device=dev) for _ in range(2))
    g = torch.zeros((1, 2), dtype=torch.float64, device=dev)
    work = ops.tridiag_work(u1, ne, 1, "bc")
    rwork = ops._scratch(None, ops._capi.load().lssvr_nl_residual_work_bytes(ne), dev)
    mon = torch.zeros(4, dtype=torch.float64, device=dev)
    outs = {k: torch.zeros((ne, nq), dtype=torch.float64, device=dev) for k in ("a", "c", "rho")}
    outs.update(f=torch.zeros((R, ne, nq), dtype=torch.float64, device=dev),
                q=torch.zeros((nterm, ne, nq), dtype=torch.float64, device=dev),
                g=torch.zeros((N + 1, 2), dtype=torch.float64, device=dev),
                kappa=torch.zeros(2, dtype=torch.float64, device=dev))
    bdf2 = ops.BDF["bdf2"]
    kinds, kappa = (0, 1), (0.0, 1.0)

    def fused():
        ops.ts_nl_adjoint_step(x, Utraj[3], cs, "poly", q, md, mo, Z[0:1], Z[1:2], P, ph1, 2.0, -0.5, inv_dt, a_quad=one,
                               out=dict(jac, B=b1, band_ends=band_ends[0]))

    def chain():
        ops.ts_rhs(md, mo, Z[0:1], Z[1:2], P, ph1, 2.0, -0.5, inv_dt, out=b1)
        ops.ts_nl_assemble(x, Utraj[3], cs, "poly", q, b1[0], a_quad=one, out=nb)
        band_ends[0, 0].copy_(nb["off"][0])
        band_ends[0, 1].copy_(nb["off"][ne - 1])

    def solve():
        ops.tridiag_bc_solve_multi(jac["diag"], jac["off"], b1, kinds, kappa, g, out=u1, work=work)

    def chunk(with_q):
        want = ops.TS_NL_SENS_TABLES if with_q else ops.TS_SENS_TABLES
        return lambda: ops.ts_nl_sensitivity(x, Utraj, Z, 2, [bdf2] * m, inv_dt, nq, "poly", nterm, q_tabs=q, want=want,
                                             phi=phi, Brows=B, band_ends=band_ends, end_kinds=kinds, accumulate=True,
                                             out={k: outs[k] for k in (*want, "g", "kappa")})

    def forward_step():
        ops.ts_rhs(md, mo, Utraj[2:3], Utraj[1:2], P, ph1, 2.0, -0.5, inv_dt, out=b1)
        for _ in range(3):
            ops.ts_nl_assemble(x, Utraj[3], cs, "poly", q, b1[0], a_quad=one, out=nb)
            ops.tridiag_bc_solve_multi(nb["diag"], nb["off"], nb["rhs"].view(1, -1), kinds, kappa, g, out=u1, work=work)
            ops.nl_residual(nb["diag"], nb["off"], nb["off"], nb["rhs"], Utraj[3], u1[0], kinds, kappa, g[0], out4=mon,
                            work=rwork)

    parts = {"adjoint_step_fused": fused, "adjoint_step_chain": chain, "solve_bc": solve,
             "chunk_m8_with_gq": chunk(True), "chunk_m8_without_gq": chunk(False), "forward_step_3_newton": forward_step}
    out = {"ne": ne, "nquad": nq, "nterm": nterm, "R": R, "m": m, "reps": a.reps, "rounds": a.rounds, "us": {},
           "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    us = out["us"]
    base = 8 * ((1 + (m + 2) + m) * (ne + 1) + 2 * (3 + R) * ne * nq)
    model = {"adjoint_step_fused": 8 * (10 * (ne + 1) + (2 + nterm) * ne * nq),
             "chunk_m8_without_gq": base, "chunk_m8_with_gq": base + 8 * 2 * nterm * ne * nq}
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (us[k] * 1e-6) / 1e12, 3) for k in model}
    out["fused_over_chain"] = round(us["adjoint_step_fused"] / us["adjoint_step_chain"], 3)
    out["gq_over_no_gq"] = round(us["chunk_m8_with_gq"] / us["chunk_m8_without_gq"], 3)
    level = us["adjoint_step_fused"] + us["solve_bc"] + us["chunk_m8_with_gq"] / m
    out["backward_level_us"] = round(level, 2)
    out["backward_level_over_forward_step"] = round(level / us["forward_step_3_newton"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_transient_nl_sensitivity.py needs the GPU: there is nothing to time without it")
    for ne in a.ne:
        print(json.dumps(measure(ne, a)), flush=True)


if __name__ == "__main__":
    main()
