"""One hp enhancement round with coefficients, reaction and convection, two ways: 1e5 elements
with the seven degree parameters 8, 10, .. 20 in equal shares, a = 2 + sin pi x, b = sin(pi x)/2, c = 1 + cos(pi x)/2,
every table tabulated ON THE DEVICE so that the round holds device work only.
  whole mesh:    per degree ``colloc_points`` of every element, the four tables on them, ``enhance_varcoef`` over the
                 whole mesh, the rows of the degree's own elements copied out (the path before the element lists)
  element lists: ``group_by_degree`` once, per degree ``colloc_points_subset``, the four tables on those points,
                 ``enhance_varcoef_subset`` into the padded rows
Wall time of a round between two device synchronisations, the two alternating repetition by repetition; medians of
REPS rounds after a warm-up, with the min-max spread.  Byte model of the tables: 4 n doubles per element and degree
against 4 n per element, 1/7 with seven degrees.
usage: hp_round_quick.py [ne] [--json PATH]"""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from hybrid_fem_lssvr_amd import ops

REPS, GAMMA, N0 = 30, 1e4, 16
DEGREES = (8, 10, 12, 14, 16, 18, 20)
dev = "cuda:0"
argv = sys.argv[1:]
out_json = None
if "--json" in argv:
    i = argv.index("--json")
    out_json = argv[i + 1]
    del argv[i:i + 2]
ne = int(argv[0]) if argv else 100000
x = torch.linspace(-1, 1, ne + 1, dtype=torch.float64, device=dev)
u = torch.sin(np.pi * x) + 0.3 * torch.cos(2 * np.pi * x)
deg_h = np.random.default_rng(1).permutation(np.resize(np.array(DEGREES), ne))
deg = torch.as_tensor(deg_h.astype(np.int32), device=dev)
Mmax = max(DEGREES)
gd = (-1.0, 1.0)


def tables(pts):
    """(a, a' - b, f, c) at the device points, any layout."""
    s, c = torch.sin(np.pi * pts), torch.cos(np.pi * pts)
    a, b, cc = 2.0 + s, 0.5 * s, 1.0 + 0.5 * c
    uu, du = s + 0.3 * torch.cos(2 * np.pi * pts), np.pi * c - 0.6 * np.pi * torch.sin(2 * np.pi * pts)
    d2u = -np.pi ** 2 * s - 1.2 * np.pi ** 2 * torch.cos(2 * np.pi * pts)
    da = np.pi * c
    return a, da - b, -a * d2u + (b - da) * du + cc * uu, cc


ids_of = {M: torch.as_tensor(np.nonzero(deg_h == M)[0], device=dev) for M in DEGREES}


def whole_mesh():
    W = torch.zeros((ne, Mmax), dtype=torch.float64, device=dev)
    for M in DEGREES:
        n, pm = max(N0, 2 * M), M <= 22
        ta, tda, tf, tc = tables(ops.colloc_points(x, n, point_major=pm))
        Wg, _ = ops.enhance_varcoef(x, u, M, GAMMA, n, ta, tda, tf, c_values=tc, point_major=pm, global_domain=gd)
        W[ids_of[M], :M] = Wg[ids_of[M]]
    return W


def element_lists():
    W = torch.zeros((ne, Mmax), dtype=torch.float64, device=dev)
    ids, offsets = ops.group_by_degree(deg)
    off = offsets.cpu().numpy()
    for M in DEGREES:
        n, pm = max(N0, 2 * M), M <= 22
        sub = ids[off[M]:off[M + 1]]
        ta, tda, tf, tc = tables(ops.colloc_points_subset(x, sub, n, point_major=pm))
        ops.enhance_varcoef_subset(x, u, M, GAMMA, n, W, ta, tda, tf, elem_ids=sub, c_values=tc, point_major=pm,
                                   global_domain=gd)
    return W


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    W = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, W


for _ in range(3):
    whole_mesh(), element_lists()
tw, tl = [], []
for _ in range(REPS):
    t, Ww = timed(whole_mesh)
    tw.append(t)
    t, Wl = timed(element_lists)
    tl.append(t)
tw, tl = np.sort(tw), np.sort(tl)
mw, ml = float(np.median(tw)), float(np.median(tl))
err = float(((Ww - Wl).abs().amax() / Ww.abs().amax()).item())
row = dict(ne=ne, degrees=list(DEGREES), whole_mesh_ms=mw * 1e3, whole_mesh_min_ms=tw[0] * 1e3,
           whole_mesh_max_ms=tw[-1] * 1e3, element_lists_ms=ml * 1e3, element_lists_min_ms=tl[0] * 1e3,
           element_lists_max_ms=tl[-1] * 1e3, ratio=ml / mw, model_ratio=1.0 / len(DEGREES), max_rel_diff=err, reps=REPS)
print(f"ne {ne}, {len(DEGREES)} degrees: whole mesh {mw*1e3:.2f} ms [{tw[0]*1e3:.2f}, {tw[-1]*1e3:.2f}]  element lists "
      f"{ml*1e3:.2f} ms [{tl[0]*1e3:.2f}, {tl[-1]*1e3:.2f}]  ratio {ml/mw:.3f} (table byte model "
      f"{1.0/len(DEGREES):.3f})  max rel diff {err:.1e}", flush=True)
if out_json:
    os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
    with open(out_json, "w") as fh:
        json.dump(row, fh, indent=1)
