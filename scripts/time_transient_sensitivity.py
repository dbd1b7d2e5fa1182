"""Time lssvr_transient_sensitivity on the GPU beside what it replaces and what it runs next to, all in
the same run: m launches of lssvr_p1_sensitivity (ga, gc, gf, nc = 1: the per-step tables a naive sweep would write), the
one-case lssvr_tridiag_bc_solve_multi and lssvr_ts_rhs (the other two calls of an adjoint step, and the whole forward
step).  Default shape: 1e6 uniform elements, nquad = 2, R = 1, chunks of m = 1 and m = 8, all outputs, with and without
accumulate.  Device events around ``--reps`` back-to-back calls after ``--warmup`` warm-up calls; the median of
``--rounds`` such windows.  Prints one JSON line: times in microseconds, the byte model -- per element and chunk 8 B of x,
(m + 2) 8 B of trajectory rows and m 8 B of Z read, (3 + R) nquad 8 B written, and the same again read with accumulate --
the rate it implies, the chunk's time per adjoint step against one lssvr_p1_sensitivity launch and against the solve, and
the whole backward step against the forward step.  Run it under a time limit of its own:

    timeout -k 10 300 python scripts/time_transient_sensitivity.py [--ne 1000000] [--nquad 2] [--reps 20] [--rounds 5]
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("time_transient_sensitivity.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, nq, R, N = a.ne, a.nquad, 1, 10
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    one = torch.ones((ne, nq), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.standard_normal(shape), device=dev)

    inv_dt = 100.0
    mass = ops.p1_assemble(x, nq, rhs_quad=one, a_quad=0.0 * one, c_quad=one)
    step = ops.p1_assemble(x, nq, rhs_quad=one, a_quad=one, c_quad=(1.0 + 1.5 * inv_dt) * one)
    Utraj, Z, B, phi = rand(N + 1, ne + 1), rand(8, ne + 1), rand(8, ne + 1), rand(N, R)
    band_ends = torch.stack([torch.stack((step["off"][0], step["off"][ne - 1]))] * 2)
    outs = {k: torch.zeros((ne, nq), dtype=torch.float64, device=dev) for k in ("a", "c", "rho")}
    outs.update(f=torch.zeros((R, ne, nq), dtype=torch.float64, device=dev),
                g=torch.zeros((N + 1, 2), dtype=torch.float64, device=dev),
                kappa=torch.zeros(2, dtype=torch.float64, device=dev))
    per_step = {k: torch.empty((1, ne, nq), dtype=torch.float64, device=dev) for k in ("a", "c", "f")}
    u1, b1 = (torch.empty((1, ne + 1), dtype=torch.float64, device=dev) for _ in range(2))
    g = torch.zeros((1, 2), dtype=torch.float64, device=dev)
    work = ops.tridiag_work(u1, ne, 1, "bc")
    load, ph1 = step["load"].view(1, -1), torch.ones((1, 1), dtype=torch.float64, device=dev)
    bdf2 = ops.BDF["bdf2"]

    def chunk(m, accumulate):
        return lambda: ops.ts_sensitivity(x, Utraj, Z[:m], 2, [bdf2] * m, inv_dt, nq, phi=phi, Brows=B[:m],
                                          band_ends=band_ends, band_rows=[1] * m, end_kinds=(0, 1),
                                          accumulate=accumulate, out=outs)

    def naive(m):
        def run():
            for i in range(m):
                ops.p1_sensitivity(x, Utraj[i + 1], Z[i], nq, want=("a", "c", "f"), out=per_step)
        return run

    parts = {"solve_bc": lambda: ops.tridiag_bc_solve_multi(step["diag"], step["off"], load, (0, 1), (0.0, 1.0), g,
                                                            out=u1, work=work),
             "ts_rhs": lambda: ops.ts_rhs(mass["diag"], mass["off"], Z[0:1], Z[1:2], load, ph1, 2.0, -0.5, inv_dt,
                                          out=b1),
             "p1_sens_x1": naive(1), "p1_sens_x8": naive(8)}
    model = {}
    for m in (1, 8):
        for acc in (False, True):
            name = f"ts_sens_m{m}{'_acc' if acc else ''}"
            parts[name] = chunk(m, acc)
            model[name] = 8 * ((1 + (m + 2) + m) * (ne + 1) + (2 if acc else 1) * (3 + R) * ne * nq)
    out = {"ne": ne, "nquad": nq, "R": R, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    us = out["us"]
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (us[k] * 1e-6) / 1e12, 3) for k in model}
    out["us_per_adjoint_step"] = {k: round(us[k] / (8 if "_m8" in k else 1), 2) for k in model}
    out["per_step_over_p1_sens"] = {k: round(v / us["p1_sens_x1"], 3) for k, v in out["us_per_adjoint_step"].items()}
    out["per_step_over_solve"] = {k: round(v / us["solve_bc"], 3) for k, v in out["us_per_adjoint_step"].items()}
    out["m8_over_8_launches"] = round(us["ts_sens_m8_acc"] / us["p1_sens_x8"], 3)
    fwd = us["ts_rhs"] + us["solve_bc"]
    out["forward_step_us"] = round(fwd, 2)
    out["backward_step_us"] = {k: round(fwd + v, 2) for k, v in out["us_per_adjoint_step"].items()}
    out["backward_over_forward"] = {k: round((fwd + v) / fwd, 3) for k, v in out["us_per_adjoint_step"].items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
