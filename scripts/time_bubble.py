"""Time ops.p1_assemble_bubble on the device: 1e6 uniform elements, every order at nquad = 5
and R = 1, beside ops.p1_assemble(b_quad=...) in the same run, alternating between them.

Method: device events around 20 back-to-back calls after 3 warm-ups, the median of 5 windows, the spread as
(max - min) / median.  Each time is set against the byte model of the call -- in (3 + R) nquad 8 B per element,
intermediate (4 + 2R) 8 B per element written and read once, out (3 + R) 8 B per node -- as achieved TB/s.  The
figure is the wrapper's call (two launches and the host code between them), not a kernel time.  There is no CPU path:
without a device the script fails.

    python scripts/time_bubble.py [--ne 1000000] [--calls 20] [--windows 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model_bytes(ne, nquad, R, bubble):
    per_elem_in = (3 + R) * nquad * 8
    out = (3 + R) * 8 * (ne + 1)
    mid = 2 * (4 + 2 * R) * 8 * ne if bubble else 0          # written by the element pass, read by the node pass
    return per_elem_in * ne + mid + out + 8 * (ne + 1)       # (+ the mesh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=1000000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    from hybrid_fem_lssvr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("time_bubble.py needs the MI355X: there is no CPU path")
    dev, ne, nquad, R = torch.device("cuda:0"), args.ne, 5, 1
    x = torch.linspace(-1.0, 1.0, ne + 1, dtype=torch.float64, device=dev)
    xq = ops.quad_points(x, nquad)
    fq, aq = torch.sin(3.0 * xq), 1.3 + 0.3 * torch.sin(2.0 * xq)
    cq, bq = 0.8 + 0.6 * torch.cos(2.0 * xq), 0.3 * torch.sin(5.0 * xq)
    cases = {"p1_assemble(b_quad)": None, **{f"bubble order {p}": p for p in ops.BUBBLE_ORDERS}}
    bufs, work = {}, None

    def call(name):
        p = cases[name]
        if p is None:
            bufs[name] = ops.p1_assemble(x, nquad, rhs_quad=fq, a_quad=aq, c_quad=cq, b_quad=bq, out=bufs.get(name))
        else:
            bufs[name] = ops.p1_assemble_bubble(x, p, nquad, fq, a_quad=aq, c_quad=cq, b_quad=bq, out=bufs.get(name),
                                                work=work)
    work = torch.empty((4 + 2 * R) * ne, dtype=torch.float64, device=dev)
    for name in cases:
        for _ in range(args.warmup):
            call(name)
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(args.windows):                 # alternate: one window of every case per round
        for name in cases:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.calls):
                call(name)
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) * 1e-3 / args.calls)
    out = dict(ne=ne, nquad=nquad, R=R, calls=args.calls, windows=args.windows, cases={})
    for name, t in times.items():
        med = float(np.median(t))
        nbytes = model_bytes(ne, nquad, R, cases[name] is not None)
        out["cases"][name] = dict(median_us=med * 1e6, spread=(max(t) - min(t)) / med, model_MB=nbytes / 1e6,
                                  achieved_TBps=nbytes / med / 1e12)
        print(f"{name:22s} median {med * 1e6:9.1f} us/call  spread {100 * (max(t) - min(t)) / med:5.1f} %  "
              f"model {nbytes / 1e6:7.1f} MB  {nbytes / med / 1e12:6.3f} TB/s")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
