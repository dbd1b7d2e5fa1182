"""Time one iteration of the block inverse iteration of DESIGN.md section 25 on the GPU, split into its four parts:
the nb-case shifted solve (unpivoted and pivoting), lssvr_eig_apply, lssvr_eig_ritz and lssvr_eig_rotate, plus the Sturm
count of two shifts.  Default shape: -u'' = lambda u on 1e6 uniform elements, k = 4, nb = 6.  Device events around
``--reps`` back-to-back launches after ``--warmup`` warm-up launches; the median of ``--rounds`` such windows.  Prints
one JSON line: times in microseconds, the byte model of the two streaming kernels and the rate it implies.

    python scripts/time_eigen.py [--ne 1000000] [--nb 6] [--reps 20] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def window(fn, reps, warmup, rounds):
    """Median over ``rounds`` of the mean time of ``reps`` back-to-back calls, in microseconds."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=1000000)
    ap.add_argument("--nb", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("time_eigen.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, nb = a.ne, a.nb
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, 2)
    zq, one = torch.zeros_like(xq), torch.ones_like(xq)
    K = ops.p1_assemble(x, 2, rhs_quad=zq, c_quad=zq)
    M = ops.p1_assemble(x, 2, rhs_quad=zq, a_quad=zq, c_quad=one)
    sigma_in = 30.0                                              # between the third and the fourth eigenvalue
    S_spd = K                                                    # sigma = 0
    S_ind = ops.p1_assemble(x, 2, rhs_quad=zq, c_quad=-sigma_in * one)
    kinds, kappa = (0, 0), (0.0, 0.0)
    Y = torch.zeros((nb, ne + 1), dtype=torch.float64, device=dev)
    Y[:, 1:-1] = torch.as_tensor(np.random.default_rng(0).standard_normal((nb, ne - 1)), device=dev)
    Z, X, Y2, MZ, KZ = (torch.empty_like(Y) for _ in range(5))
    gram = torch.empty((2, nb, nb), dtype=torch.float64, device=dev)
    theta = torch.empty(nb, dtype=torch.float64, device=dev)
    Q = torch.empty((nb, nb), dtype=torch.float64, device=dev)
    res2 = torch.empty((2, nb), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = ops._capi.load()
    swork = ops._scratch(None, max(lib.lssvr_tridiag_pivot_work_bytes(ne, nb), lib.lssvr_tridiag_bc_work_bytes(ne, nb)),
                         dev)
    ework = ops._scratch(None, lib.lssvr_eig_work_bytes(ne, nb), dev)
    parts = {
        "solve_bc": lambda: ops.tridiag_bc_solve_multi(S_spd["diag"], S_spd["off"], Y, kinds, kappa, out=Z, work=swork),
        "solve_pivot": lambda: ops.tridiag_pivot_solve_multi(S_ind["diag"], S_ind["off"], S_ind["off"], Y, kinds, kappa,
                                                             out=Z, work=swork),
        "apply": lambda: ops.eig_apply(K["diag"], K["off"], M["diag"], M["off"], Z, kinds, kappa, MZ=MZ, KZ=KZ,
                                       gram=gram, work=ework),
        "ritz": lambda: ops.eig_ritz(gram, 0.0, theta=theta, Q=Q, info=info),
        "rotate": lambda: ops.eig_rotate(Z, MZ, KZ, Q, theta, kinds, X=X, Y=Y2, res2=res2, work=ework),
    }
    out = {"ne": ne, "nb": nb, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    parts["solve_bc"]()                 # Z, then gram, Q and theta hold sensible values for the parts that follow
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    shifts = torch.as_tensor([1.0, 30.0], dtype=torch.float64, device=dev)
    med, lo, hi = window(lambda: ops.eig_count(K["diag"], K["off"], M["diag"], M["off"], shifts, 1e-290), 2, 1, 3)
    out["us"]["count_2_shifts"] = round(med, 1)
    n = ne + 1
    model = {"apply": (3 * nb + 4) * 8 * n, "rotate": 5 * nb * 8 * n}
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (out["us"][k] * 1e-6) / 1e12, 3) for k in model}
    out["iteration_us"] = {"bc": round(sum(out["us"][k] for k in ("solve_bc", "apply", "ritz", "rotate")), 1),
                           "pivot": round(sum(out["us"][k] for k in ("solve_pivot", "apply", "ritz", "rotate")), 1)}
    out["three_kernels_over_solve"] = {s: round((out["us"]["apply"] + out["us"]["ritz"] + out["us"]["rotate"])
                                                / out["us"]["solve_" + s], 3) for s in ("bc", "pivot")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
