"""Time lssvr_p1_sensitivity on the GPU beside the two entries it runs next to: the assembly
lssvr_p1_assemble_conv and the one-case lssvr_tridiag_ns_bc_solve_multi, all in the same run.  Default shape: 1e6
uniform elements, nquad = 2, nc in {1, 8}, all four outputs and then ga alone.  Device events around ``--reps``
back-to-back launches after ``--warmup`` warm-up launches; the median of ``--rounds`` such windows.  Prints one JSON
line: times in microseconds, the byte model -- per element 3 * 8 B of x, U, Z read per case (x once) and nquad * 8 B
written per table and case -- the rate it implies, and the ratio to each reference entry.

    python scripts/time_sensitivity.py [--ne 1000000] [--nquad 2] [--reps 20] [--rounds 5]
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
        raise SystemExit("time_sensitivity.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, nq = a.ne, a.nquad
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, nq)
    one = torch.ones_like(xq)
    rng = np.random.default_rng(0)

    def rand(*shape):
        return torch.as_tensor(rng.standard_normal(shape), device=dev)

    bq = 0.25 * ne * xq          # cell Peclet number <= 0.25: the unpivoted solve is safe
    bands = ops.p1_assemble(x, nq, rhs_quad=one, a_quad=one, c_quad=one, b_quad=bq)
    U, Z = rand(8, ne + 1), rand(8, ne + 1)
    outs = {k: torch.empty((8, ne, nq), dtype=torch.float64, device=dev) for k in ops.SENS_TABLES}
    u1 = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
    g = torch.zeros((1, 2), dtype=torch.float64, device=dev)
    work = ops._scratch(None, ops._capi.load().lssvr_tridiag_bc_work_bytes(ne, 1), dev)
    load = bands["load"].view(1, -1)

    def sens(nc, want):
        out = {k: outs[k][:nc] for k in want}
        return lambda: ops.p1_sensitivity(x, U[:nc], Z[:nc], nq, want=want, out=out)

    parts = {"assemble_conv": lambda: ops.p1_assemble(x, nq, rhs_quad=one, a_quad=one, c_quad=one, b_quad=bq, out=bands),
             "solve_ns_bc": lambda: ops.tridiag_ns_bc_solve_multi(bands["diag"], bands["sub"], bands["sup"], load,
                                                                  (0, 0), (0.0, 0.0), g, out=u1, work=work)}
    model = {}
    for nc in (1, 8):
        for tag, want in (("all", ops.SENS_TABLES), ("ga", ("a",))):
            parts[f"sens_nc{nc}_{tag}"] = sens(nc, want)
            model[f"sens_nc{nc}_{tag}"] = 8 * ((1 + 2 * nc) * (ne + 1) + len(want) * nc * ne * nq)
    out = {"ne": ne, "nquad": nq, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (out["us"][k] * 1e-6) / 1e12, 3) for k in model}
    out["over_assemble_conv"] = {k: round(out["us"][k] / out["us"]["assemble_conv"], 3) for k in model}
    out["over_solve_ns_bc"] = {k: round(out["us"][k] / out["us"]["solve_ns_bc"], 3) for k in model}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
