"""Time lssvr_newmark_sensitivity and lssvr_newmark_adjoint_advance on the GPU beside what they
replace and what they run next to, all in the same run: launches of lssvr_p1_sensitivity that produce the same tables
level by level (ga, gc, gf from (u, lambda), then gc again from (acc, lambda) for dJ/drho and from (v, lambda) for
dJ/dd: they have the form of dJ/dc), lssvr_wave_advance (the forward loop's launch between two solves) and the one-case
lssvr_tridiag_bc_solve_multi.  Default shape: 1e6 uniform elements, nquad = 2, R = 1, chunks of m = 1 and m = 8, with
and without accumulate, with and without damping.  Device events around ``--reps`` back-to-back calls after
``--warmup`` warm-up calls; the median of ``--rounds`` such windows.  Prints one JSON line: times in microseconds, the
byte model -- per element and chunk 8 B of x, T m 8 B of trajectory rows (T = 3 with damping, 2 without) and m 8 B of Z
read, (T + 1 + R) nquad 8 B written, and the same again read with accumulate; the advance (5 + B) 8 B read per node
(lambda, vbar, abar, p and B = 2 or 4 band entries) and 3 8 B written -- the rates they imply, and the ratios.  Run it
under a time limit of its own:

    timeout -k 10 300 python scripts/time_wave_sensitivity.py [--ne 1000000] [--nquad 2] [--reps 20] [--rounds 5]
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
        raise SystemExit("time_wave_sensitivity.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, nq, R, N = a.ne, a.nquad, 1, 10
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    one = torch.ones((ne, nq), dtype=torch.float64, device=dev)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.standard_normal(shape), device=dev)

    def empty(*shape):
        return torch.empty(shape, dtype=torch.float64, device=dev)

    dt, beta, gamma = 0.01, 0.25, 0.5
    mass = ops.p1_assemble(x, nq, rhs_quad=one, a_quad=0.0 * one, c_quad=one)
    damp = ops.p1_assemble(x, nq, rhs_quad=one, a_quad=0.0 * one, c_quad=0.5 * one)
    step = ops.p1_assemble(x, nq, rhs_quad=one, a_quad=one, c_quad=(1.0 + 1.0 / (beta * dt * dt)) * one)
    Ut, Vt, At, Z, B, phi = (rand(N + 1, ne + 1), rand(N + 1, ne + 1), rand(N + 1, ne + 1), rand(8, ne + 1),
                             rand(8, ne + 1), rand(N + 1, R))
    band_ends = torch.stack((step["off"][0], step["off"][ne - 1]))
    outs = {k: torch.zeros((ne, nq), dtype=torch.float64, device=dev) for k in ("a", "c", "rho", "d")}
    outs.update(f=torch.zeros((R, ne, nq), dtype=torch.float64, device=dev),
                g=torch.zeros((N + 1, 2), dtype=torch.float64, device=dev),
                kappa=torch.zeros(2, dtype=torch.float64, device=dev))
    per_level = {k: empty(1, ne, nq) for k in ("a", "c", "f")}
    as_c = dict(c=empty(1, ne, nq))
    u1, g = empty(1, ne + 1), torch.zeros((1, 2), dtype=torch.float64, device=dev)
    work = ops.tridiag_work(u1, ne, 1, "bc")
    load, ph1 = step["load"].view(1, -1), torch.ones((1, 1), dtype=torch.float64, device=dev)
    adv_out = dict(v=empty(ne + 1), a=empty(ne + 1), b=empty(ne + 1))
    wv, wa, wb = empty(1, ne + 1), empty(1, ne + 1), empty(1, ne + 1)

    def chunk(m, accumulate, damped):
        want = ops.NM_SENS_TABLES if damped else tuple(k for k in ops.NM_SENS_TABLES if k != "d")
        out = {k: v for k, v in outs.items() if k != "d" or damped}
        return lambda: ops.newmark_sensitivity(x, Ut, Z[:m], 2, nq, want=want, Vtraj=Vt if damped else None, Atraj=At,
                                               phi=phi, Brows=B[:m], band_ends=band_ends, end_kinds=(0, 1),
                                               accumulate=accumulate, out=out)

    def naive(m, damped):
        def run():
            for i in range(m):
                ops.p1_sensitivity(x, Ut[i + 2], Z[i], nq, want=("a", "c", "f"), out=per_level)
                ops.p1_sensitivity(x, At[i + 2], Z[i], nq, want=("c",), out=as_c)
                if damped:
                    ops.p1_sensitivity(x, Vt[i + 2], Z[i], nq, want=("c",), out=as_c)
        return run

    def advance(damped):
        dd, do = (damp["diag"], damp["off"]) if damped else (None, None)
        return lambda: ops.newmark_adjoint_advance(Z[0], B[0], B[1], mass["diag"], mass["off"], dd, do, dt, beta, gamma,
                                                   P=B[2], out=adv_out)

    def forward_advance(damped):
        dd, do = (damp["diag"], damp["off"]) if damped else (None, None)
        return lambda: ops.wave_advance(Z[0:1], Z[1:2], Z[2:3], Z[3:4], mass["diag"], mass["off"], dd, do, load, ph1, dt,
                                        beta, gamma, V_out=wv, Acc_out=wa, rhs_out=wb)

    parts = {"solve_bc": lambda: ops.tridiag_bc_solve_multi(step["diag"], step["off"], load, (0, 1), (0.0, 1.0), g,
                                                            out=u1, work=work)}
    model = {}
    for damped in (True, False):
        tag = "_damped" if damped else ""
        T = 3 if damped else 2
        parts[f"adjoint_advance{tag}"] = advance(damped)
        parts[f"wave_advance{tag}"] = forward_advance(damped)
        parts[f"p1_sens_x1{tag}"] = naive(1, damped)
        parts[f"p1_sens_x8{tag}"] = naive(8, damped)
        model[f"adjoint_advance{tag}"] = 8 * (5 + (4 if damped else 2) + 3) * (ne + 1)
        for m in (1, 8):
            for acc in (False, True):
                name = f"nm_sens_m{m}{'_acc' if acc else ''}{tag}"
                parts[name] = chunk(m, acc, damped)
                model[name] = 8 * ((1 + T * m + m) * (ne + 1) + (2 if acc else 1) * (T + 1 + R) * ne * nq)
    out = {"ne": ne, "nquad": nq, "R": R, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    us = out["us"]
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (us[k] * 1e-6) / 1e12, 3) for k in model}
    sens = [k for k in model if k.startswith("nm_sens")]
    out["us_per_level"] = {k: round(us[k] / (8 if "_m8" in k else 1), 2) for k in sens}
    out["per_level_over_p1_sens"] = {k: round(out["us_per_level"][k]
                                              / us["p1_sens_x1" + ("_damped" if k.endswith("_damped") else "")], 3)
                                     for k in sens}
    out["m8_over_8_levels_of_p1_sens"] = {tag or "undamped": round(us[f"nm_sens_m8_acc{tag}"] / us[f"p1_sens_x8{tag}"], 3)
                                          for tag in ("_damped", "")}
    out["adjoint_over_forward_advance"] = {tag or "undamped": round(us[f"adjoint_advance{tag}"] / us[f"wave_advance{tag}"], 3)
                                           for tag in ("_damped", "")}
    out["backward_over_forward_step"] = {
        tag or "undamped": round((us["solve_bc"] + us[f"adjoint_advance{tag}"] + out["us_per_level"][f"nm_sens_m8_acc{tag}"])
                                 / (us["solve_bc"] + us[f"wave_advance{tag}"]), 3) for tag in ("_damped", "")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
