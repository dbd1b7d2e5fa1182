"""numpy statement of DESIGN.md section 29: Newmark (beta, gamma) in displacement form with a fixed step for

    rho u_tt + d u_t - (a u')' + c u = f(x, t) = sum_r phi_r(t) f_r(x)      on a P1 mesh,

u(., 0) = u0, u_t(., 0) = v0, each end Dirichlet u = g(t) or Robin a du/dn + kappa u = g(t).  With the predictors
ut = u + dt v + dt^2 (1/2 - beta) acc, vt = v + dt (1 - gamma) acc step n+1 solves

    A u' = load(t_{n+1}) + M_rho (ut / (beta dt^2)) + M_d ((gamma / (beta dt)) ut - vt),
    A = K + M_rho / (beta dt^2) + (gamma / (beta dt)) M_d      (ONE reaction assembly),

then acc' = (u' - ut) / (beta dt^2), v' = vt + gamma dt acc'.  The first acceleration solves
M_rho acc0 = load(0) - M_d v0 - K u0 (Robin end: - (kappa u0 - g(0)) in its row; Dirichlet end: the value g''(0)).
The solves are scipy.linalg.solve_banded (LAPACK) in float64, or an unpivoted elimination in any numpy float type
(np.longdouble: the reference the float64 bars are measured against).  :func:`advance` is the plain restatement of the
kernel lssvr_wave_advance (csrc/wave.hip), every sum in its documented order; the facade's solve_wave follows
:func:`solve` step by step; tests/wave_rules.py imports this file.

Run as a script it prints what DESIGN.md quotes: the temporal orders, the energy readings and the accuracy record of
the standing wave u = cos(pi t / 2) cos(pi x / 2) on 8, 16, 32 elements."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import transient_proto as tp                               # noqa: E402
from oracle import lssvr_oracle as orc                     # noqa: E402

DIRICHLET, ROBIN = tp.DIRICHLET, tp.ROBIN
MAX_TERMS = tp.MAX_TERMS
_zero, _one, _fn = tp._zero, tp._one, tp._fn
mass_bands, loads, tri_apply, bc_solve = tp.mass_bands, tp.loads, tp.tri_apply, tp.bc_solve


def stiff_bands(nodes, a=None, c=None, nquad=2):
    """(kdiag, koff) of K: the reaction assembly of (a, c)."""
    return orc.p1_bands(nodes, _zero, a, nquad, _zero if c is None else c)[:2]


def step_bands(nodes, dt, beta, gamma, a=None, c=None, rho=None, d=None, nquad=2):
    """(diag, off) of A: ONE reaction assembly with c_quad = c + rho / (beta dt^2) + gamma d / (beta dt)."""
    cf, rf, df = (_zero if c is None else c), (_one if rho is None else rho), (_zero if d is None else d)
    return orc.p1_bands(nodes, _zero, a, nquad,
                        lambda x: cf(x) + rf(x) / (beta * dt ** 2) + gamma * df(x) / (beta * dt))[:2]


def coefficients(dt, beta, gamma, dtype=np.float64):
    """(dt, c_u2, c_v1, c_m, c_d, c_va) in ``dtype``, each in the order wave_coefficients computes it."""
    dt, beta, gamma = dtype(dt), dtype(beta), dtype(gamma)
    dt2 = dt * dt
    return (dt, dt2 * (dtype(0.5) - beta), dt * (dtype(1.0) - gamma), dtype(1.0) / (beta * dt2), gamma / (beta * dt),
            gamma * dt)


def advance(U_new, U, V, Acc, md, mo, dd, do, L, phi, dt, beta, gamma, rhs=True):
    """One case of lssvr_wave_advance on vectors [ne+1] of one float type -> (V_out, Acc_out, rhs_out); ``U_new`` None:
    (U, V, Acc) is the state; ``rhs`` False: no right-hand side; ``dd`` None: no damping.  Every sum in the order of
    csrc/wave.hip."""
    dtype = U.dtype.type
    dt, c_u2, c_v1, c_m, c_d, c_va = coefficients(dt, beta, gamma, dtype)
    if U_new is None:
        u, v, acc = U, V, Acc
        V_out = Acc_out = None
    else:
        ut = (U + dt * V) + c_u2 * Acc
        vt = V + c_v1 * Acc
        acc = (U_new - ut) * c_m
        v = vt + c_va * acc
        u, V_out, Acc_out = U_new, v, acc
    if not rhs:
        return V_out, Acc_out, None
    ut = (u + dt * v) + c_u2 * acc
    s = tri_apply(md, mo, c_m * ut)
    if dd is not None:
        s = s + tri_apply(dd, do, c_d * ut - (v + c_v1 * acc))
    for r in range(len(phi)):
        s = s + phi[r] * L[r]
    return V_out, Acc_out, s


def energy(kd, ko, md, mo, u, v, kinds, kappa):
    """E = 1/2 v^T M_rho v + 1/2 u^T K u + 1/2 sum over the Robin ends of kappa u_end^2, over all nodes."""
    e = (v * tri_apply(md, mo, v)).sum() + (u * tri_apply(kd, ko, u)).sum()
    for i, end in ((0, 0), (1, -1)):
        if kinds[i] == ROBIN:
            e = e + kappa[i] * u[end] * u[end]
    return 0.5 * e


def assemble(nodes, dt, beta, gamma, a=None, c=None, rho=None, d=None, f_list=(_zero,), nquad=2):
    """The float64 arrays of the loop, by the oracle's assembly: dict(mass, damp (None without d), stiff, step, loads)."""
    return dict(mass=mass_bands(nodes, rho, nquad), damp=None if d is None else mass_bands(nodes, d, nquad),
                stiff=stiff_bands(nodes, a, c, nquad), step=step_bands(nodes, dt, beta, gamma, a, c, rho, d, nquad),
                loads=loads(nodes, list(f_list), nquad))


def solve(nodes, u0, v0, t_end, nsteps, a=None, c=None, rho=None, d=None, forcing=None,
          kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), end_data=(0.0, 0.0), end_accel0=(0.0, 0.0), snapshots=None,
          beta=0.25, gamma=0.5, nquad=2, dtype=np.float64, every=False, adv_fn=None, bands=None):
    """The time loop.  ``forcing``: a list of (phi(t) or a constant, f(x)) pairs (default: none); ``end_data``:
    (g_left, g_right), callables of t or constants; ``end_accel0`` = (g_left''(0), g_right''(0)), read at a Dirichlet
    end.  u0 and v0 are sampled at the nodes; a Dirichlet end starts at g(0), and with constant data its velocity is 0.
    Returns dict(times, nodal, velocity, accel [ns, ne+1], energy [ns+1] (index 0: t = 0), accel0, phi [ns, R],
    g [ns, 2], dt); ``every``: all steps are snapshots.  ``dtype`` other than float64 runs the unpivoted elimination in
    that type on the float64 bands.  ``adv_fn``: a stand-in for :func:`advance` (the library's host mirror, in the
    tests).  ``bands``: the arrays of :func:`assemble` as another assembly produced them."""
    nodes = np.asarray(nodes, dtype=np.float64)
    ne = len(nodes) - 1
    forcing = [(0.0, _zero)] if not forcing else list(forcing)
    if not 1 <= len(forcing) <= MAX_TERMS:
        raise ValueError(f"forcing must hold 1 .. {MAX_TERMS} terms")
    snapshots = list(range(1, nsteps + 1)) if every else ([nsteps] if snapshots is None else list(snapshots))
    if any(not 1 <= s <= nsteps for s in snapshots):
        raise ValueError("snapshots must lie in 1 .. nsteps")
    dt = float(t_end) / nsteps
    solve_fn = tp.lapack_solve if dtype == np.float64 else tp.thomas_solve
    adv = adv_fn or advance
    if bands is None:
        bands = assemble(nodes, dt, beta, gamma, a, c, rho, d, [f for _, f in forcing], nquad)
    cast = lambda pair: None if pair is None else tuple(np.asarray(t, dtype=dtype) for t in pair)      # noqa: E731
    (md, mo), (kd, ko), (sd, so) = cast(bands["mass"]), cast(bands["stiff"]), cast(bands["step"])
    dd, do = cast(bands["damp"]) or (None, None)
    L = np.asarray(bands["loads"], dtype=dtype)
    phis = [_fn(p) for p, _ in forcing]
    times = dt * np.arange(nsteps + 1)
    phi = np.array([[p(t) for p in phis] for t in times], dtype=np.float64)
    g = np.array([[_fn(v)(t) for v in end_data] for t in times], dtype=np.float64)
    u = np.asarray(np.broadcast_to(np.asarray(u0(nodes), dtype=np.float64), nodes.shape), dtype=dtype).copy()
    v = np.asarray(np.broadcast_to(np.asarray(v0(nodes), dtype=np.float64), nodes.shape), dtype=dtype).copy()
    for i, end in ((0, 0), (1, ne)):
        if kinds[i] == DIRICHLET:
            u[end] = g[0, i]
            if not callable(end_data[i]):
                v[end] = 0.0
    kap = np.asarray(kappa, dtype=dtype)
    # acc0: M_rho acc0 = load(0) - M_d v0 - K u0, all rows; a Robin end's row takes g(0) - kappa u0 and is natural
    r0 = np.zeros(ne + 1, dtype=dtype)
    for r in range(len(phis)):
        r0 = r0 + dtype(phi[0, r]) * L[r]
    if dd is not None:
        r0 = r0 - tri_apply(dd, do, v)
    r0 = r0 - tri_apply(kd, ko, u)
    ga = np.zeros(2, dtype=dtype)
    for i, end in ((0, 0), (1, ne)):
        if kinds[i] == ROBIN:
            r0[end] = r0[end] + (dtype(g[0, i]) - kap[i] * u[end])
        else:
            ga[i] = dtype(end_accel0[i])
    acc = bc_solve(md, mo, r0, kinds, (0.0, 0.0), ga, solve_fn)
    out = dict(times=[], nodal=[], velocity=[], accel=[], energy=[energy(kd, ko, md, mo, u, v, kinds, kap)],
               accel0=acc.copy(), phi=[], g=[], dt=dt)
    rhs = adv(None, u, v, acc, md, mo, dd, do, L, np.asarray(phi[1], dtype=dtype), dt, beta, gamma)[2]
    for n in range(1, nsteps + 1):
        new = bc_solve(sd, so, rhs, kinds, kap, np.asarray(g[n], dtype=dtype), solve_fn)
        last = n == nsteps
        v, acc, rhs = adv(new, u, v, acc, md, mo, dd, do, L, None if last else np.asarray(phi[n + 1], dtype=dtype), dt,
                          beta, gamma, rhs=not last)
        u = new
        if n in snapshots:
            out["times"].append(times[n])
            out["nodal"].append(u.copy())
            out["velocity"].append(v.copy())
            out["accel"].append(acc.copy())
            out["energy"].append(energy(kd, ko, md, mo, u, v, kinds, kap))
            out["phi"].append(phi[n])
            out["g"].append(g[n])
    for k in ("times", "nodal", "velocity", "accel", "energy", "phi", "g"):
        out[k] = np.array(out[k])
    return out


def enhance_snapshot(nodes, u, v, acc, phi, f_list, M, gamma_reg, n_colloc, a=None, da=None, c=None, rho=None, d=None,
                     kinds=(DIRICHLET, DIRICHLET), g=(0.0, 0.0)):
    """W[ne, M]: the oracle's reaction rows for -(a u')' + c u = sum_r phi[r] f_r - rho I_h acc - d I_h v with the nodal
    values u (float64).  A Dirichlet end takes g as its constraint, a Robin end the nodal value."""
    nodes = np.asarray(nodes, dtype=np.float64)
    u, v, acc = (np.asarray(t, dtype=np.float64) for t in (u, v, acc))
    rf = _one if rho is None else rho

    def rhs(x):
        f = phi[0] * np.asarray(f_list[0](x), dtype=np.float64)
        for r in range(1, len(f_list)):
            f = f + phi[r] * np.asarray(f_list[r](x), dtype=np.float64)
        f = f - rf(x) * np.interp(x, nodes, acc)
        return f if d is None else f - d(x) * np.interp(x, nodes, v)

    bl = float(g[0]) if kinds[0] == DIRICHLET else float(u[0])
    br = float(g[1]) if kinds[1] == DIRICHLET else float(u[-1])
    return orc.enhance_all_vec(nodes, u, M, gamma_reg, n_colloc, rhs=rhs, coef_a=_one if a is None else a,
                               coef_da=_zero if da is None else da, coef_c=_zero if c is None else c,
                               bc_left=bl, bc_right=br)


# the standing wave u = cos(pi t / 2) cos(pi x / 2) on (-1, 1): a = rho = 1, c = d = f = 0, zero Dirichlet ends
def standing():
    """(u0, v0, exact(x, t))."""
    return (lambda x: np.where(np.abs(np.asarray(x)) == 1.0, 0.0, np.cos(0.5 * math.pi * np.asarray(x, dtype=np.float64))),
            _zero, lambda x, t: math.cos(0.5 * math.pi * t) * np.cos(0.5 * math.pi * x))


ORDER_NE, ORDER_T, ORDER_STEPS = 2048, 0.8, (8, 16, 32)


def temporal_orders(adv_fn=None, ne=ORDER_NE, t_end=ORDER_T, steps=ORDER_STEPS):
    """(errors, orders): max nodal error at t_end against the exact standing wave, and log2 of successive ratios."""
    u0, v0, exact = standing()
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    errs = [float(np.max(np.abs(solve(nodes, u0, v0, t_end, n, adv_fn=adv_fn)["nodal"][-1] - exact(nodes, t_end))))
            for n in steps]
    return errs, [math.log2(errs[i] / errs[i + 1]) for i in range(len(errs) - 1)]


def accuracy_record(sizes=(8, 16, 32), t_end=0.8, nsteps=64, M=9, gamma_reg=1e4, n_colloc=16, nfine=2001):
    """[(ne, max |I_h u_h - u|, max |enhanced - u|)] at t_end over ``nfine`` points."""
    u0, v0, exact = standing()
    xs = np.linspace(-1.0, 1.0, nfine)
    rows = []
    for ne in sizes:
        nodes = np.linspace(-1.0, 1.0, ne + 1)
        r = solve(nodes, u0, v0, t_end, nsteps)
        W = enhance_snapshot(nodes, r["nodal"][-1], r["velocity"][-1], r["accel"][-1], [0.0], [_zero], M, gamma_reg,
                             n_colloc)
        ue = orc.evaluate_solution_vec(nodes, W, xs)[0]
        ref = exact(xs, t_end)
        rows.append((ne, float(np.max(np.abs(np.interp(xs, nodes, r["nodal"][-1]) - ref))),
                     float(np.max(np.abs(ue - ref)))))
    return rows


if __name__ == "__main__":
    errs, orders = temporal_orders()
    print("temporal order, 2048 elements, 8 / 16 / 32 steps: errors", ", ".join(f"{e:.3e}" for e in errs), " orders",
          ", ".join(f"{o:.3f}" for o in orders))
    for ne, e_p1, e_enh in accuracy_record():
        print(f"ne = {ne:3d}:  max |P1 interpolant - u| = {e_p1:.3e}   max |enhanced - u| = {e_enh:.3e}   "
              f"factor {e_p1 / e_enh:.2f}")
