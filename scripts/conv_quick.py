"""Timing of the P1 half of the convection term at 1e6 elements on one MI355X:
lssvr_tridiag_ns_dirichlet_solve beside lssvr_tridiag_dirichlet_solve, and lssvr_p1_assemble_conv beside
lssvr_p1_assemble_react, device events around `reps` back-to-back launches after a warm-up, the two members of a
pair alternating over `rounds` rounds.  The bands are those of -u'' + b u' + u = f with cell Peclet number 0.5 on a
uniform mesh; the symmetric solver gets the bands of the same problem without b.  Prints every round, the medians
and the ratio against the byte model (four bands read instead of three: 4/3 for the top level).

    python scripts/conv_quick.py [--ne 1000000] [--reps 50] [--rounds 5] [--json PATH]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hybrid_fem_lssvr_amd import ops  # noqa: E402


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None, help="write the record to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_quick.py needs an MI355X")
    dev = torch.device("cuda:0")
    ne, nquad = args.ne, 2
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, nquad)
    fq = ops.POISSON_AMP * torch.sin(ops.POISSON_OMEGA * xq)
    cq = torch.ones_like(xq)
    bq = torch.full_like(xq, 0.5 * ne)                       # |b| h / 2 = 0.5 with h = 2 / ne, a = 1
    sym = ops.p1_assemble(x, nquad, rhs_quad=fq, c_quad=cq)
    ns = ops.p1_assemble(x, nquad, rhs_quad=fq, c_quad=cq, b_quad=bq)
    u = torch.empty(ne + 1, dtype=torch.float64, device=dev)
    lib = ops._capi.load()
    w_sym = torch.empty(lib.lssvr_tridiag_work_bytes(ne) // 8 + 1, dtype=torch.float64, device=dev)
    w_ns = torch.empty(lib.lssvr_tridiag_ns_work_bytes(ne) // 8 + 1, dtype=torch.float64, device=dev)
    runs = {
        "tridiag": lambda: ops.tridiag_dirichlet_solve(sym["diag"], sym["off"], sym["load"], 0.25, -0.5, out=u,
                                                       work=w_sym),
        "tridiag_ns": lambda: ops.tridiag_ns_dirichlet_solve(ns["diag"], ns["sub"], ns["sup"], ns["load"], 0.25, -0.5,
                                                             out=u, work=w_ns),
        "p1_assemble_react": lambda: ops.p1_assemble(x, nquad, rhs_quad=fq, c_quad=cq, out=sym),
        "p1_assemble_conv": lambda: ops.p1_assemble(x, nquad, rhs_quad=fq, c_quad=cq, b_quad=bq, out=ns),
    }
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            times[k].append(timeit(fn, args.reps) * 1e6)
    rec = {"ne": ne, "reps": args.reps, "rounds": args.rounds}
    for k, v in times.items():
        rec[k] = {"us": v, "median_us": float(np.median(v))}
        print(f"{k:18s}: " + ", ".join(f"{t:7.1f}" for t in v) + f"  us; median {np.median(v):7.1f}")
    r = rec["tridiag_ns"]["median_us"] / rec["tridiag"]["median_us"]
    ra = rec["p1_assemble_conv"]["median_us"] / rec["p1_assemble_react"]["median_us"]
    rec["ns_over_sym"], rec["conv_over_react"] = r, ra
    print(f"tridiag_ns / tridiag = {r:.3f} (byte model of the top level: 4/3 = 1.333)")
    # assembly bytes per element: x, f, c (, b) tables of nquad; diag, off | sub + sup, load
    by_r, by_c = 8 + 2 * nquad * 8 + 3 * 8, 8 + 3 * nquad * 8 + 4 * 8
    print(f"p1_assemble_conv / p1_assemble_react = {ra:.3f} (byte model: {by_c} / {by_r} = {by_c / by_r:.3f})")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
