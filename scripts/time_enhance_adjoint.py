"""Time lssvr_enhance_adjoint on the GPU beside the forward call it differentiates, in the same
run: lssvr_enhance_react_ws on the same element-major tables.  Default shape: 1e6 uniform elements, M = 9, 16 points,
all six outputs and gf + gu alone.  Device events around ``--reps`` back-to-back calls after ``--warmup`` warm-up calls;
the median of ``--rounds`` such windows.  Prints one JSON line: times in microseconds, the byte model -- per element the
forward call moves 4 n 8 + 8 M + 16 B, the adjoint call the four tables, W and Wbar in and up to four tables and the
pair out, and the gather the pair in and 8 B out -- the rate it implies and the ratio to the forward call beside the
ratio of the models.  Run it under a time limit of its own:

    timeout -k 10 300 python scripts/time_enhance_adjoint.py [--ne 1000000] [--M 9] [--n 16] [--reps 20] [--rounds 5]
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
    ap.add_argument("--M", type=int, default=9)
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("time_enhance_adjoint.py needs the GPU: there is nothing to time without it")
    dev = torch.device("cuda:0")
    ne, M, n, gamma = a.ne, a.M, a.n, 1.0e4
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xc = ops.colloc_points(x, n)
    rng = np.random.default_rng(0)
    u = torch.as_tensor(rng.standard_normal(ne + 1), device=dev)
    f = torch.as_tensor(rng.standard_normal((ne, n)), device=dev)
    av, dav, cv = 1.0 + 0.3 * torch.sin(2.0 * xc), 0.6 * torch.cos(2.0 * xc), 1.5 + torch.cos(3.0 * xc)
    W = torch.empty((ne, M), dtype=torch.float64, device=dev)
    st = torch.empty(ne, dtype=torch.int32, device=dev)
    Wbar = torch.as_tensor(rng.standard_normal((ne, M)), device=dev)
    dom = (-1.0, 1.0)

    def forward():
        ops.enhance_varcoef(x, u, M, gamma, n, av, dav, f, c_values=cv, global_domain=dom, out=W, status=st)

    forward()
    shapes = {"u": (ne + 1,), "bc": (2,)}
    bufs = {k: torch.empty(shapes.get(k, (ne, n)), dtype=torch.float64, device=dev) for k in ops.ENH_ADJ_OUTPUTS}
    work = torch.empty((ne, 2), dtype=torch.float64, device=dev)

    def adjoint(want):
        return lambda: ops.enhance_adjoint(x, W, Wbar, M, gamma, n, f, a_values=av, da_values=dav, c_values=cv,
                                           status=st, want=want, global_domain=dom, out=bufs, work=work)

    parts = {"forward_react_ws": forward, "adjoint_all": adjoint(ops.ENH_ADJ_OUTPUTS), "adjoint_f_u": adjoint(("u", "f"))}
    fwd_b = (4 * n * 8 + 8 * M + 16) * ne
    model = {"forward_react_ws": fwd_b,
             "adjoint_all": (4 * n * 8 + 2 * 8 * M + 8) * ne + (4 * n * 8 + 16) * ne + 24 * ne,
             "adjoint_f_u": (4 * n * 8 + 2 * 8 * M + 8) * ne + (n * 8 + 16) * ne + 24 * ne}
    out = {"ne": ne, "M": M, "n": n, "reps": a.reps, "rounds": a.rounds, "us": {}, "us_min_max": {}}
    for name, fn in parts.items():
        med, lo, hi = window(fn, a.reps, a.warmup, a.rounds)
        out["us"][name] = round(med, 2)
        out["us_min_max"][name] = [round(lo, 2), round(hi, 2)]
    us = out["us"]
    out["bytes"] = model
    out["TB_per_s"] = {k: round(model[k] / (us[k] * 1e-6) / 1e12, 3) for k in model}
    out["over_forward"] = {k: round(us[k] / us["forward_react_ws"], 3) for k in model}
    out["model_over_forward"] = {k: round(model[k] / fwd_b, 3) for k in model}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
