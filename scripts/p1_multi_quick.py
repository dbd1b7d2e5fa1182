"""The P1 half of several load cases against separate calls: 1e6 elements, nquad = 2, reaction bands (symmetric
solve) and cell-Peclet-0.5 convection bands (non-symmetric solve).  For ncases in {1, 4, 8}: one
``lssvr_tridiag(_ns)_dirichlet_solve_multi`` against ncases calls of the single entry, and one ``lssvr_p1_load_multi``
against ncases calls of ``lssvr_p1_assemble_react``, in the same process, the two alternating repetition by repetition
(device time between two events on the stream, every buffer allocated beforehand); medians of REPS repetitions after a
warm-up, with the min-max spread of each.  Byte model per unknown at the top level: separate
calls 9 doubles a case, one pass 6 + 3 R.  Acceptance (the rule of section 16): at 8 cases the multi solve's slowest
repetition is below the separate calls' fastest; at 1 case the multi median lies inside the single entry's
[min, max].
usage: p1_multi_quick.py [ne [ncases ...]] [--json PATH]"""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from hybrid_fem_lssvr_amd import _capi, ops

REPS = 15
dev = "cuda:0"
argv = sys.argv[1:]
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
ne = int(argv[0]) if argv else 1000000
cases = [int(v) for v in argv[1:]] or [1, 4, 8]
nquad = 2
RC = ops.TRIDIAG_MULTI_CASES
lib = _capi.load()
x = torch.linspace(-1, 1, ne + 1, dtype=torch.float64, device=dev)
xq = ops.quad_points(x, nquad)
f0 = float(np.pi ** 2) * torch.sin(np.pi * xq)
cq = 2.0 + torch.cos(2.0 * np.pi * xq)
bq = torch.full_like(xq, 0.5 * ne)                     # |b| h / 2 = 0.5 with h = 2 / ne and a = 1
react = ops.p1_assemble(x, nquad, rhs_quad=f0, c_quad=cq)
conv = ops.p1_assemble(x, nquad, rhs_quad=f0, c_quad=cq, b_quad=bq)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def compare(multi, single):
    for _ in range(3):
        multi(), single()
    torch.cuda.synchronize()
    tm, ts = [], []
    for _ in range(REPS):
        tm.append(timed(multi))
        ts.append(timed(single))
    return np.sort(tm), np.sort(ts)


rows = []
for R in cases:
    FQ = torch.stack([(1.0 + 0.25 * j) * f0 + 0.5 * j for j in range(R)])
    bc = torch.tensor([[0.3 + 0.1 * j, -0.2 - 0.05 * j] for j in range(R)], dtype=torch.float64, device=dev)
    bch = bc.tolist()
    L = ops.p1_load_multi(x, FQ, nquad)
    U = torch.empty((R, ne + 1), dtype=torch.float64, device=dev)
    U1 = torch.empty((R, ne + 1), dtype=torch.float64, device=dev)
    work = torch.empty(lib.lssvr_tridiag_multi_work_bytes(ne, R) // 8 + 1, dtype=torch.float64, device=dev)
    work1 = torch.empty(lib.lssvr_tridiag_work_bytes(ne) // 8 + 1, dtype=torch.float64, device=dev)
    L1 = torch.empty((R, ne + 1), dtype=torch.float64, device=dev)
    scratch = ops.p1_assemble(x, nquad, rhs_quad=f0, c_quad=cq)
    model = (6 + 3 * min(R, RC)) / (9.0 * min(R, RC)) if R % RC == 0 or R < RC else float("nan")
    jobs = {
        "tridiag": (lambda: ops.tridiag_dirichlet_solve_multi(react["diag"], react["off"], L, bc, out=U, work=work),
                    lambda: [ops.tridiag_dirichlet_solve(react["diag"], react["off"], L[j], *bch[j], out=U1[j],
                                                         work=work1) for j in range(R)]),
        "tridiag_ns": (lambda: ops.tridiag_ns_dirichlet_solve_multi(conv["diag"], conv["sub"], conv["sup"], L, bc,
                                                                    out=U, work=work),
                       lambda: [ops.tridiag_ns_dirichlet_solve(conv["diag"], conv["sub"], conv["sup"], L[j], *bch[j],
                                                               out=U1[j], work=work1) for j in range(R)]),
        "p1_load": (lambda: ops.p1_load_multi(x, FQ, nquad, out=L1),
                    lambda: [ops.p1_assemble(x, nquad, rhs_quad=FQ[j], c_quad=cq, out=scratch) for j in range(R)]),
    }
    for name, (multi, single) in jobs.items():
        tm, ts = compare(multi, single)
        mm, ms = float(np.median(tm)), float(np.median(ts))
        same = bool((U == U1).all().item()) if name != "p1_load" else bool((L1 == L).all().item())
        if name == "p1_load":
            ok = None
        elif R == 1:
            ok = bool(ts[0] <= mm <= ts[-1])
        else:
            ok = bool(tm[-1] < ts[0])
        row = dict(what=name, ne=ne, ncases=R, multi_us=mm * 1e6, multi_min_us=tm[0] * 1e6, multi_max_us=tm[-1] * 1e6,
                   separate_us=ms * 1e6, separate_min_us=ts[0] * 1e6, separate_max_us=ts[-1] * 1e6, ratio=mm / ms,
                   model_ratio=None if name == "p1_load" else model, bit_identical=same, accepted=ok, reps=REPS)
        rows.append(row)
        print(f"{name} ncases {R}: multi {mm*1e6:.1f} us [{tm[0]*1e6:.1f}, {tm[-1]*1e6:.1f}]  separate {ms*1e6:.1f} us "
              f"[{ts[0]*1e6:.1f}, {ts[-1]*1e6:.1f}]  ratio {mm/ms:.3f}"
              + ("" if name == "p1_load" else f" (byte model {model:.3f})")
              + f"  bit-identical {same}  accepted {ok}", flush=True)
    del FQ, L, U, U1, work, work1, L1
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(rows, fh, indent=1)
