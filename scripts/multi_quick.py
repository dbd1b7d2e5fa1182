"""Several load cases against separate calls: 1e6 elements, degree 8 (M = 9), 16 points, point-major, reaction rows.
For ncases in {1, 4, 8}: ``lssvr_enhance_multi`` (kernel_ms_host: first pass's begin to last pass's end) against
ncases calls of ``lssvr_enhance_react_ws`` (the sum of theirs) in the same process, the two alternating repetition by
repetition; medians of REPS repetitions after a warm-up, with the min-max spread of each.  Byte model per element
(DESIGN.md section 16): R cases in one pass 392 + 208 R (the a, a', c tables once), R separate calls 600 R.
usage: multi_quick.py [ne [M [n_colloc]]] [--json PATH]"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from hybrid_fem_lssvr_amd import ops
import bench

REPS = 15
HBM_PEAK = 8.0e12           # B/s, MI355X
dev = "cuda:0"
argv = sys.argv[1:]
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
ne = int(argv[0]) if argv else 1000000
M = int(argv[1]) if len(argv) > 1 else 9
n = int(argv[2]) if len(argv) > 2 else 16
x = torch.linspace(-1, 1, ne + 1, dtype=torch.float64, device=dev)
xc = ops.colloc_points(x, n, point_major=True)
a, da, f = bench._varcoef_device_tables(xc)
c = 2.0 + torch.cos(2.0 * np.pi * xc)
gd = (-1.0, 1.0)
rows = []
for R in (1, 4, 8):
    U = torch.stack([torch.sin((j + 1) * np.pi * x / 2) + 0.1 * j for j in range(R)])
    F = torch.stack([(1.0 + 0.25 * j) * f + 0.5 * j for j in range(R)])
    bc = torch.tensor([[0.3 + 0.1 * j, -0.2 - 0.05 * j] for j in range(R)], dtype=torch.float64, device=dev)
    W = torch.empty((R, ne, M), dtype=torch.float64, device=dev)
    st = torch.empty((R, ne), dtype=torch.int32, device=dev)
    W1 = torch.empty((R, ne, M), dtype=torch.float64, device=dev)
    st1 = torch.empty((R, ne), dtype=torch.int32, device=dev)
    multi = lambda: ops.enhance_multi(x, U, M, 1e4, n, a, da, F, c_values=c, bc=bc, point_major=True,
                                      global_domain=gd, out=W, status=st, timed=True)
    single = lambda: sum(ops.enhance_varcoef(x, U[j], M, 1e4, n, a, da, F[j], c_values=c, point_major=True,
                                             global_domain=gd, bc=tuple(bc[j].tolist()), out=W1[j], status=st1[j],
                                             profiled=True) for j in range(R))
    for _ in range(3):
        multi(), single()
    tm, ts = [], []
    for _ in range(REPS):
        tm.append(multi())
        ts.append(single())
    tm, ts = np.sort(tm), np.sort(ts)
    mm, ms = float(np.median(tm)), float(np.median(ts))
    model = (392 + 208 * R) / (600.0 * R)
    err = float(((W - W1).abs().amax() / W1.abs().amax()).item())
    row = dict(ne=ne, M=M, n=n, ncases=R, multi_us=mm * 1e6, multi_min_us=tm[0] * 1e6, multi_max_us=tm[-1] * 1e6,
               separate_us=ms * 1e6, separate_min_us=ts[0] * 1e6, separate_max_us=ts[-1] * 1e6, ratio=mm / ms,
               model_ratio=model, multi_hbm_fraction=(392 + 208 * R) * ne / mm / HBM_PEAK,
               separate_hbm_fraction=600.0 * R * ne / ms / HBM_PEAK, max_rel_diff=err,
               fallbacks=int(st.sum()) + int(st1.sum()), reps=REPS)
    rows.append(row)
    print(f"ncases {R}: multi {mm*1e6:.1f} us [{tm[0]*1e6:.1f}, {tm[-1]*1e6:.1f}]  separate {ms*1e6:.1f} us "
          f"[{ts[0]*1e6:.1f}, {ts[-1]*1e6:.1f}]  ratio {mm/ms:.3f} (byte model {model:.3f})  HBM fraction multi "
          f"{row['multi_hbm_fraction']:.2f} separate {row['separate_hbm_fraction']:.2f}  max rel diff {err:.1e}",
          flush=True)
    del U, F, W, st, W1, st1
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(rows, fh, indent=1)
