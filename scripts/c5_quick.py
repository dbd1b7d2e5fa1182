"""BASELINE config 5 timing: variable-coefficient rows, 1e6 elements, degree 8, 16 points, tabulated
a, a', f (16 + 72 + 3*128 = 472 B per element), both table layouts; hipExt-stamped launches.
usage: c5_quick.py [ne [M [n_colloc]]] [--reaction]   (LSSVR_VC_MINW=1: the two-waves-per-SIMD build of the
point-major kernel; M = 9 and 16 points unless given: M > 22, or M > 16 with --reaction, reaches the MFMA kernels)
--reaction: also lssvr_enhance_react_ws on the same mesh (a fourth table, c = 2 + cos 2 pi x: 600 B per element)
and its ratio to the variable-coefficient entry of the same run."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from hybrid_fem_lssvr_amd import ops
import bench
dev = "cuda:0"
reaction = "--reaction" in sys.argv[1:]
argv = [v for v in sys.argv[1:] if v != "--reaction"]
ne = int(argv[0]) if argv else 1000000
M = int(argv[1]) if len(argv) > 1 else 9
n = int(argv[2]) if len(argv) > 2 else 16
vc_bytes = 16 + 8 * M + 3 * 8 * n          # x, u | W row | a, a', f
rx_bytes = vc_bytes + 8 * n                # ... and c
x = torch.linspace(-1, 1, ne + 1, dtype=torch.float64, device=dev)
u = torch.sin(np.pi * x)
W = torch.empty((ne, M), dtype=torch.float64, device=dev)
st = torch.empty(ne, dtype=torch.int32, device=dev)
res, med = {}, {}
for pm in (True, False):
    a, da, f = bench._varcoef_device_tables(ops.colloc_points(x, n, point_major=pm))
    run = lambda: ops.enhance_varcoef(x, u, M, 1e4, n, a, da, f, global_domain=(-1.0, 1.0), out=W, status=st,
                                      point_major=pm, profiled=True)
    run()
    ts = sorted(run() for _ in range(40))
    res[pm] = W.clone()
    med[pm] = ts[20]
    print(f"config 5 {'point' if pm else 'element'}-major: median {ts[20]*1e6:.1f} us  min {ts[0]*1e6:.1f} us -> "
          f"{ne/ts[20]:.3e} el/s, {vc_bytes*ne/ts[20]/1e9:.0f} GB/s, fallback {int(st.sum())}")
print("bit-equal:", bool(torch.equal(res[True], res[False])))
if reaction:
    for pm in (True, False):
        xc = ops.colloc_points(x, n, point_major=pm)
        a, da, f = bench._varcoef_device_tables(xc)
        c = 2.0 + torch.cos(2.0 * np.pi * xc)
        run = lambda: ops.enhance_varcoef(x, u, M, 1e4, n, a, da, f, global_domain=(-1.0, 1.0), out=W, status=st,
                                          point_major=pm, profiled=True, c_values=c)
        run()
        ts = sorted(run() for _ in range(40))
        print(f"reaction {'point' if pm else 'element'}-major: median {ts[20]*1e6:.1f} us  min {ts[0]*1e6:.1f} us -> "
              f"{ne/ts[20]:.3e} el/s, {rx_bytes*ne/ts[20]/1e9:.0f} GB/s, fallback {int(st.sum())}; "
              f"ratio to varcoef {ts[20]/med[pm]:.3f} (bytes {rx_bytes}/{vc_bytes} = {rx_bytes/vc_bytes:.3f})")
