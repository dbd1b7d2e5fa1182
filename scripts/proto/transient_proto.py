"""numpy statement of DESIGN.md section 26: BDF1 / BDF2 with a fixed step for

    rho u_t - (a u')' + c u = f(x, t) = sum_r phi_r(t) f_r(x)      on a P1 mesh,

each end Dirichlet u = g(t) or Robin a du/dn + kappa u = g(t), and the enhancement of a snapshot as the elliptic problem
-(a u')' + c u = f(., t) - rho I_h w with w the nodal BDF difference.  Step n+1 solves

    A_alpha u^{n+1} = (1/dt) M (beta0 u^n + beta1 u^{n-1}) + load(t_{n+1}),     A_alpha = K + (alpha / dt) M,

through scipy.linalg.solve_banded (LAPACK's pivoting banded LU) in float64, or through an unpivoted elimination in any
numpy float type (np.longdouble: the reference the float64 bars are measured against).  The element rows of the
enhancement are the oracle's.  The device kernels (csrc/timestep.hip) and the facade's solve_transient follow this text
step by step; tests/transient_rules.py imports it.

Run as a script it prints the accuracy record DESIGN.md quotes: u = exp(-t) cos(pi x / 2) on 8, 16, 32 elements, the
max error of the P1 interpolant and of the enhanced snapshot at t = 1."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import lssvr_oracle as orc                     # noqa: E402

DIRICHLET, ROBIN = 0, 1
SCHEMES = {"bdf1": (1.0, 1.0, 0.0), "bdf2": (1.5, 2.0, -0.5)}      # alpha, beta0, beta1
MAX_TERMS = 8


def _zero(x):
    return np.zeros_like(np.asarray(x, dtype=np.float64))


def _one(x):
    return np.ones_like(np.asarray(x, dtype=np.float64))


def _fn(v):
    """A callable of t from a callable or a constant."""
    return v if callable(v) else (lambda t, v=float(v): v)


def mass_bands(nodes, rho=None, nquad=2):
    """(mdiag[ne+1], moff[ne]): the consistent mass bands weighted by rho -- the reaction assembly with a = 0."""
    return orc.p1_bands(nodes, _zero, _zero, nquad, _one if rho is None else rho)[:2]


def step_bands(nodes, alpha, dt, a=None, c=None, rho=None, nquad=2):
    """(diag, off) of A_alpha = K + (alpha / dt) M: ONE reaction assembly with c_quad = c + alpha rho / dt."""
    cf, rf = (_zero if c is None else c), (_one if rho is None else rho)
    return orc.p1_bands(nodes, _zero, a, nquad, lambda x: cf(x) + alpha * rf(x) / dt)[:2]


def loads(nodes, f_list, nquad=2):
    """[R, ne+1]: the P1 load of every spatial factor f_r."""
    return np.stack([orc.p1_bands(nodes, f, None, nquad)[2] for f in f_list])


def tri_apply(d, o, v):
    """tridiag(o, d, o) v, summed as (o[i-1] v[i-1] + d[i] v[i]) + o[i] v[i+1]."""
    out = d * v
    out[1:] = o * v[:-1] + out[1:]
    out[:-1] = out[:-1] + o * v[1:]
    return out


def step_rhs(md, mo, u0, u1, beta0, beta1, inv_dt, L, phi):
    """inv_dt M (beta0 u0 + beta1 u1) + sum_r phi[r] L[r], in the order of lssvr_ts_rhs (u1 unread when beta1 == 0)."""
    v = beta0 * u0 if beta1 == 0.0 else beta0 * u0 + beta1 * u1
    s = inv_dt * tri_apply(md, mo, v)
    for r in range(len(phi)):
        s = s + phi[r] * L[r]
    return s


def lapack_solve(d, o, b):
    from scipy.linalg import solve_banded
    ab = np.zeros((3, len(d)))
    ab[1] = d
    ab[0, 1:] = o
    ab[2, :-1] = o
    return solve_banded((1, 1), ab, b)


def thomas_solve(d, o, b):
    """Unpivoted elimination in the arrays' own float type (the np.longdouble reference)."""
    d, b = d.copy(), b.copy()
    for i in range(1, len(d)):
        m = o[i - 1] / d[i - 1]
        d[i] = d[i] - m * o[i - 1]
        b[i] = b[i] - m * b[i - 1]
    x = b
    x[-1] = b[-1] / d[-1]
    for i in range(len(d) - 2, -1, -1):
        x[i] = (b[i] - o[i] * x[i + 1]) / d[i]
    return x


def bc_solve(diag, off, rhs, kinds, kappa, g, solve_fn=lapack_solve):
    """u[ne+1] of the step's system with the ends of lssvr_tridiag_bc_solve_multi: a Robin end keeps its node, adds
    kappa to its diagonal and g to its row; a Dirichlet end is the value g, taken to the neighbour's right-hand side."""
    ne = len(off)
    sh, hi = (0 if kinds[0] == ROBIN else 1), (ne + 1 if kinds[1] == ROBIN else ne)
    u = np.zeros(ne + 1, dtype=rhs.dtype)
    d, b = diag[sh:hi].copy(), rhs[sh:hi].copy()
    if kinds[0] == ROBIN:
        d[0] += kappa[0]
        b[0] += g[0]
    else:
        u[0] = g[0]
        if hi > sh:
            b[0] -= off[0] * g[0]
    if kinds[1] == ROBIN:
        d[-1] += kappa[1]
        b[-1] += g[1]
    else:
        u[ne] = g[1]
        if hi > sh:
            b[-1] -= off[ne - 1] * g[1]
    if hi > sh:
        u[sh:hi] = solve_fn(d, off[sh:hi - 1], b)
    return u


def solve(nodes, u0, t_end, nsteps, scheme="bdf2", a=None, c=None, rho=None, forcing=None,
          kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), end_data=(0.0, 0.0), snapshots=None, nquad=2,
          dtype=np.float64, every=False, rhs_fn=None, bands=None):
    """The time loop.  ``forcing``: a list of (phi(t) or a constant, f(x)) pairs (default: no forcing); ``end_data``:
    (g_left, g_right), callables of t or constants.  Returns dict(times, nodal [ns, ne+1], diffs [ns, ne+1] the nodal
    BDF differences w at the snapshots, weights [ns, 3] = (alpha, beta0, beta1) of each snapshot's step, phi [ns, R],
    g [ns, 2], dt); ``every``: all steps 1 .. nsteps are snapshots.  ``dtype`` other than float64 runs the unpivoted
    elimination in that type on the float64 bands and loads.  ``rhs_fn``: a stand-in for :func:`step_rhs` (the
    library's host mirror, in the tests).  ``bands``: dict(mass=(mdiag, moff), step={alpha: (diag, off)}, loads [R, ne+1])
    to run the loop on instead of the oracle's assembly -- the float64 arrays another assembly produced, so that two
    loops can be compared on the same rounded data."""
    nodes = np.asarray(nodes, dtype=np.float64)
    ne = len(nodes) - 1
    if scheme not in SCHEMES:
        raise ValueError(f"scheme must be one of {sorted(SCHEMES)}")
    forcing = [(0.0, _zero)] if not forcing else list(forcing)
    if not 1 <= len(forcing) <= MAX_TERMS:
        raise ValueError(f"forcing must hold 1 .. {MAX_TERMS} terms")
    snapshots = list(range(1, nsteps + 1)) if every else ([nsteps] if snapshots is None else list(snapshots))
    if any(not 1 <= s <= nsteps for s in snapshots):
        raise ValueError("snapshots must lie in 1 .. nsteps")
    dt = float(t_end) / nsteps
    inv_dt = 1.0 / dt
    solve_fn = lapack_solve if dtype == np.float64 else thomas_solve
    if bands is None:
        bands = dict(mass=mass_bands(nodes, rho, nquad), loads=loads(nodes, [f for _, f in forcing], nquad),
                     step={al: step_bands(nodes, al, dt, a, c, rho, nquad)
                           for al in {SCHEMES["bdf1"][0], SCHEMES[scheme][0]}})
    md, mo = (np.asarray(t, dtype=dtype) for t in bands["mass"])
    A = {al: tuple(np.asarray(t, dtype=dtype) for t in v) for al, v in bands["step"].items()}
    L = np.asarray(bands["loads"], dtype=dtype)
    phis = [_fn(p) for p, _ in forcing]
    gl, gr = (_fn(v) for v in end_data)
    times = dt * np.arange(nsteps + 1)
    phi = np.array([[p(t) for p in phis] for t in times], dtype=np.float64)
    g = np.array([[gl(t), gr(t)] for t in times], dtype=np.float64)
    cur = np.asarray(np.broadcast_to(np.asarray(u0(nodes), dtype=np.float64), nodes.shape), dtype=dtype).copy()
    for i, end in ((0, 0), (1, ne)):
        if kinds[i] == DIRICHLET:
            cur[end] = g[0, i]
    prev = None
    out = dict(times=[], nodal=[], diffs=[], weights=[], phi=[], g=[], dt=dt)
    for n in range(1, nsteps + 1):
        al, b0, b1 = SCHEMES["bdf1"] if (n == 1 or scheme == "bdf1") else SCHEMES["bdf2"]
        rhs = (rhs_fn or step_rhs)(md, mo, cur, prev, b0, b1, inv_dt, L, np.asarray(phi[n], dtype=dtype))
        new = bc_solve(*A[al], rhs, kinds, kappa, np.asarray(g[n], dtype=dtype), solve_fn)
        if n in snapshots:
            d = al * new - b0 * cur
            out["times"].append(times[n])
            out["nodal"].append(new.copy())
            out["diffs"].append(inv_dt * (d if b1 == 0.0 else d - b1 * prev))
            out["weights"].append((al, b0, b1))
            out["phi"].append(phi[n])
            out["g"].append(g[n])
        prev, cur = cur, new
    for k in ("times", "nodal", "diffs", "weights", "phi", "g"):
        out[k] = np.array(out[k])
    return out


def enhance_snapshot(nodes, u, w, phi, f_list, M, gamma, n_colloc, a=None, da=None, c=None, rho=None,
                     kinds=(DIRICHLET, DIRICHLET), g=(0.0, 0.0)):
    """W[ne, M]: the oracle's reaction rows for -(a u')' + c u = sum_r phi[r] f_r - rho I_h w with the nodal values u
    (float64).  A Dirichlet end takes g as its constraint, a Robin end the nodal value, like every interior node.  The
    reaction term is c itself: no 1/dt shift."""
    nodes = np.asarray(nodes, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    rf = _one if rho is None else rho

    def rhs(x):
        f = phi[0] * np.asarray(f_list[0](x), dtype=np.float64)
        for r in range(1, len(f_list)):
            f = f + phi[r] * np.asarray(f_list[r](x), dtype=np.float64)
        return f - rf(x) * np.interp(x, nodes, w)

    bl = float(g[0]) if kinds[0] == DIRICHLET else float(u[0])
    br = float(g[1]) if kinds[1] == DIRICHLET else float(u[-1])
    return orc.enhance_all_vec(nodes, u, M, gamma, n_colloc, rhs=rhs, coef_a=_one if a is None else a,
                               coef_da=_zero if da is None else da, coef_c=_zero if c is None else c,
                               bc_left=bl, bc_right=br)


# the accuracy record: u = exp(-t) cos(pi x / 2) on (-1, 1), zero Dirichlet ends
def manufactured():
    """(u0, forcing, exact(x, t)) of rho = a = 1, c = 0: f = (pi^2 / 4 - 1) exp(-t) cos(pi x / 2)."""
    q = math.pi ** 2 / 4.0 - 1.0
    return (lambda x: np.cos(0.5 * math.pi * x), [(lambda t: math.exp(-t), lambda x: q * np.cos(0.5 * math.pi * x))],
            lambda x, t: math.exp(-t) * np.cos(0.5 * math.pi * x))


def accuracy_record(sizes=(8, 16, 32), t_end=1.0, nsteps=64, M=9, gamma=1e4, n_colloc=16, nfine=2001):
    """[(ne, max |I_h u_h - u|, max |enhanced - u|)] at t_end over ``nfine`` points."""
    u0, forcing, exact = manufactured()
    xs = np.linspace(-1.0, 1.0, nfine)
    rows = []
    for ne in sizes:
        nodes = np.linspace(-1.0, 1.0, ne + 1)
        r = solve(nodes, u0, t_end, nsteps, "bdf2", forcing=forcing)
        W = enhance_snapshot(nodes, r["nodal"][-1], r["diffs"][-1], r["phi"][-1], [f for _, f in forcing], M, gamma,
                             n_colloc)
        ue = orc.evaluate_solution_vec(nodes, W, xs)[0]
        ref = exact(xs, t_end)
        rows.append((ne, float(np.max(np.abs(np.interp(xs, nodes, r["nodal"][-1]) - ref))),
                     float(np.max(np.abs(ue - ref)))))
    return rows


if __name__ == "__main__":
    for ne, e_p1, e_enh in accuracy_record():
        print(f"ne = {ne:3d}:  max |P1 interpolant - u| = {e_p1:.3e}   max |enhanced - u| = {e_enh:.3e}   "
              f"factor {e_p1 / e_enh:.2f}")
