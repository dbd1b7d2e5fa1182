"""numpy statement of DESIGN.md section 30: variable-step BDF2 with a local error estimate and a step controller for

    rho u_t - (a u')' + c u = f(x, t) = sum_r phi_r(t) f_r(x)      on a P1 mesh,

each end Dirichlet u = g(t) or Robin a du/dn + kappa u = g(t).  With h the trial step, h_p the last accepted one and
omega = h / h_p an attempt solves

    (K + (alpha / h) M) u^{n+1} = (1/h) M (beta0 u^n + beta1 u^{n-1}) + load(t_{n+1}),
    alpha = (1 + 2 omega) / (1 + omega),  beta0 = 1 + omega,  beta1 = -omega^2 / (1 + omega),

(1, 1, 0 at step 1), through scipy.linalg.solve_banded in float64 or through an unpivoted elimination in any numpy
float type (np.longdouble: the reference the float64 bars are measured against).  The estimate is a divided difference
of the nodal vectors, its norm a scaled maximum; the controller, the estimator's weights and the clipping to the output
times are plain float64 functions of scalars, the same in every variant.  The device kernels
(csrc/timestep_adapt.hip) and the facade's solve_transient_adaptive follow this text step by step;
tests/transient_adaptive_rules.py imports it.

Run as a script it prints the record DESIGN.md quotes: attempts, rejections and the global error at t = 1 against the
exact semi-discrete solution for the two-mode decay, and the rejections a short pulse in the forcing causes."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import transient_proto as tp                                # noqa: E402
from oracle import lssvr_oracle as orc                      # noqa: E402

DIRICHLET, ROBIN = tp.DIRICHLET, tp.ROBIN
SAFETY, FAC_MIN, FAC_MAX = 0.9, 0.2, 2.0
OMEGA_MAX = 2.0                 # below the zero-stability limit 1 + sqrt(2) of variable-step BDF2
OUT_SLACK = 1e-9                # a step that ends within this fraction of itself before an output time is stretched to it
MAX_RESTARTS = 8


# ---- the scalar rules: float64, pure ----------------------------------------------------------------------------------
def coefficients(omega):
    """(alpha, beta0, beta1) of variable-step BDF2 at omega = h / h_p; omega = 1 gives (3/2, 2, -1/2) exactly."""
    return (1.0 + 2.0 * omega) / (1.0 + omega), 1.0 + omega, -(omega * omega) / (1.0 + omega)


def weights_bdf2(h, hp, hpp, alpha):
    """(w3, w2, w1, w0) with e = w3 u^{n+1} + w2 u^n + w1 u^{n-1} + w0 u^{n-2} = h^2 (h + h_p) / alpha times the third
    divided difference over t_{n+1}, t_n, t_{n-1}, t_{n-2} (h, hp, hpp: the three steps between them, newest first).
    The differences of the times are sums of steps: nothing cancels."""
    f = h * h * (h + hp) / alpha
    return (f / (h * (h + hp) * (h + hp + hpp)), -f / (h * hp * (hp + hpp)), f / ((h + hp) * hp * hpp),
            -f / ((h + hp + hpp) * (hp + hpp) * hpp))


def weights_bdf1(h, hp):
    """(w3, w2, w1, 0) with e = h^2 times the second divided difference over t_2, t_1, t_0: the backward-Euler error of
    step 1, read at step 2."""
    f = h * h
    return f / (h * (h + hp)), -f / (h * hp), f / ((h + hp) * hp), 0.0


def controller(err, bad, p, after_reject):
    """(accepted, fac) from the scaled estimate ``err``, the count ``bad`` of non-finite rows, the exponent's order
    ``p`` (3: BDF2 estimate, 2: the step-2 estimate) and whether the attempt followed a rejection."""
    grow = 1.0 if after_reject else FAC_MAX
    if bad != 0 or not math.isfinite(err):
        return False, FAC_MIN
    raw = math.inf if err == 0.0 else SAFETY * err ** (-1.0 / p)
    return err <= 1.0, min(max(raw, FAC_MIN), grow)


def raw_factor(err, p):
    """The factor before its clip: what the margins of a test case are measured on."""
    return math.inf if err == 0.0 else SAFETY * err ** (-1.0 / p)


def trial_step(t, dt, dt_max, h_prev, t_target):
    """(h, t_new, short): the step of an attempt that starts at ``t`` with the controller's ``dt``: capped by dt_max
    and by OMEGA_MAX times the last accepted step, then clipped so that ``t_target`` is hit exactly."""
    h = min(dt, dt_max)
    if h_prev is not None:
        h = min(h, OMEGA_MAX * h_prev)
    if t + h * (1.0 + OUT_SLACK) >= t_target:
        return t_target - t, t_target, (t_target - t) < dt
    return h, t + h, h < dt


def next_dt(dt, h, short, accepted, fac):
    """The controller's dt after an attempt of step h: fac h, except that an accepted step that was shortened (to hit
    an output, or by a cap) never shrinks dt when its estimate asks for growth."""
    if accepted and short and fac >= 1.0:
        return max(dt, fac * h)
    return fac * h


# ---- the vector pieces ----------------------------------------------------------------------------------------------
def step_matrix(kd, ko, md, mo, s):
    """(kdiag + s mdiag, koff + s moff): one multiply and one add each, in that order."""
    return kd + s * md, ko + s * mo


def estimate(U3, U2, U1, U0, w, atol, rtol, kinds):
    """(max |e| / sc, max |e|, max |U3|, count of rows not finite) in the order of lssvr_ts_error."""
    e = w[0] * U3 + w[1] * U2
    if w[2] != 0.0:
        e = e + w[2] * U1
    if w[3] != 0.0:
        e = e + w[3] * U0
    a3, a2, ae = np.abs(U3), np.abs(U2), np.abs(e)
    sc = atol + rtol * np.where(a3 > a2, a3, a2)
    keep = np.ones(len(U3), dtype=bool)
    if kinds[0] == DIRICHLET:
        keep[0] = False
    if kinds[1] == DIRICHLET:
        keep[-1] = False
    bad = keep & ~(np.isfinite(ae) & np.isfinite(sc))
    ok = keep & ~bad
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ae[ok] / sc[ok]
    q = q[~np.isnan(q)]
    fin = keep & np.isfinite(a3)
    zero = U3.dtype.type(0.0)
    return (q.max() if q.size else zero, ae[ok].max() if ok.any() else zero, a3[fin].max() if fin.any() else zero,
            float(np.count_nonzero(bad)))


def assembled(nodes, a=None, c=None, rho=None, f_list=(), nquad=2):
    """dict(mass, stiff, loads): the oracle's assembly of M, K = -(a u')' + c u and the R loads."""
    return dict(mass=tp.mass_bands(nodes, rho, nquad),
                stiff=orc.p1_bands(nodes, tp._zero, a, nquad, tp._zero if c is None else c)[:2],
                loads=tp.loads(nodes, list(f_list), nquad))


def solve(nodes, u0, t_end, rtol, atol, dt0, t_out=None, dt_min=None, dt_max=None, max_steps=100000, a=None, c=None,
          rho=None, forcing=None, kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), end_data=(0.0, 0.0), nquad=2,
          dtype=np.float64, bands=None, rhs_fn=None, matrix_fn=None, estimate_fn=None):
    """The adaptive loop.  Returns dict(times, nodal [ns, ne+1], diffs, weights [ns, 3], inv_h [ns], phi, g: as
    transient_proto.solve, per output time; steps [attempts, 4] = (t the attempt starts from, its step, err (nan at
    step 1), accepted); facs: the raw factor of every attempt with an estimate (nan at step 1); n_accepted, n_rejected,
    n_restarts).  ``dtype`` other than float64 runs the linear algebra and the estimate in that type on the float64
    bands; the scalar rules stay float64.  ``bands``: dict(mass, stiff, loads) to run on instead of the oracle's
    assembly.  ``rhs_fn`` / ``matrix_fn`` / ``estimate_fn``: stand-ins for step_rhs / step_matrix / estimate (the
    library's host mirrors, in the tests)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    ne = len(nodes) - 1
    forcing = [(0.0, tp._zero)] if not forcing else list(forcing)
    t_end = float(t_end)
    t_out = [t_end] if t_out is None else [float(t) for t in t_out]
    dt_max = t_end if dt_max is None else float(dt_max)
    dt_min = 16.0 * 2.0 ** -52 * t_end if dt_min is None else float(dt_min)
    solve_fn = tp.lapack_solve if dtype == np.float64 else tp.thomas_solve
    if bands is None:
        bands = assembled(nodes, a, c, rho, [f for _, f in forcing], nquad)
    md, mo = (np.asarray(t, dtype=dtype) for t in bands["mass"])
    kd, ko = (np.asarray(t, dtype=dtype) for t in bands["stiff"])
    L = np.asarray(bands["loads"], dtype=dtype)
    phis = [tp._fn(p) for p, _ in forcing]
    gfn = [tp._fn(v) for v in end_data]
    rhs_fn, matrix_fn, estimate_fn = rhs_fn or tp.step_rhs, matrix_fn or step_matrix, estimate_fn or estimate

    def start():
        u = np.asarray(np.broadcast_to(np.asarray(u0(nodes), dtype=np.float64), nodes.shape), dtype=dtype).copy()
        for i, end in ((0, 0), (1, ne)):
            if kinds[i] == DIRICHLET:
                u[end] = gfn[i](0.0)
        return u

    out = dict(times=[], nodal=[], diffs=[], weights=[], inv_h=[], phi=[], g=[])
    steps, facs = [], []
    U = [start()]                   # accepted vectors, newest first (at most three are read)
    hs = []                         # accepted steps, newest first
    t, dt, k, restarts, after_reject, dt_start = 0.0, float(dt0), 0, 0, False, float(dt0)
    while k < len(t_out):
        if len(steps) >= max_steps:
            raise RuntimeError(f"more than max_steps = {max_steps} attempts at t = {t:.6g}, dt = {dt:.6g}, "
                               f"last err = {steps[-1][2]:.6g}")
        if dt < dt_min:
            raise RuntimeError(f"dt = {dt:.6g} < dt_min = {dt_min:.6g} at t = {t:.6g}, last err = {steps[-1][2]:.6g}")
        n = len(hs) + 1
        h, t_new, short = trial_step(t, dt, dt_max, hs[0] if hs else None, t_out[k])
        al, b0, b1 = (1.0, 1.0, 0.0) if n == 1 else coefficients(h / hs[0])
        inv_h, s = 1.0 / h, al / h
        phi = np.array([float(p(t_new)) for p in phis], dtype=np.float64)
        g = np.array([float(v(t_new)) for v in gfn], dtype=np.float64)
        A = matrix_fn(kd, ko, md, mo, s)
        rhs = rhs_fn(md, mo, U[0], U[1] if b1 != 0.0 else None, b0, b1, inv_h, L, np.asarray(phi, dtype=dtype))
        new = tp.bc_solve(*A, rhs, kinds, kappa, np.asarray(g, dtype=dtype), solve_fn)
        if n == 1:
            err, accepted, fac, raw = math.nan, True, 1.0, math.nan
        else:
            p = 2 if n == 2 else 3
            w = weights_bdf1(h, hs[0]) if n == 2 else weights_bdf2(h, hs[0], hs[1], al)
            r4 = estimate_fn(new, U[0], U[1], U[2] if n > 2 else None, w, atol, rtol, kinds)
            err = float(r4[0])
            accepted, fac = controller(err, float(r4[3]), p, after_reject)
            raw = raw_factor(err, p) if float(r4[3]) == 0 and math.isfinite(err) else math.nan
        steps.append((t, h, err, float(accepted)))
        facs.append(raw)
        if not accepted and n == 2:
            restarts += 1
            if restarts > MAX_RESTARTS:
                raise RuntimeError(f"more than {MAX_RESTARTS} restarts: step 2 rejected at dt = {h:.6g}, "
                                   f"err = {err:.6g}")
            dt_start = fac * dt_start
            U, hs, t, dt, k, after_reject = [start()], [], 0.0, dt_start, 0, True
            for v in out.values():
                del v[:]
            continue
        if n > 1:
            dt = next_dt(dt, h, short, accepted, fac)
            after_reject = not accepted
        if not accepted:
            continue
        if t_new == t_out[k]:
            d = al * new - b0 * U[0]
            out["times"].append(t_new)
            out["nodal"].append(new.copy())
            out["diffs"].append(inv_h * (d if b1 == 0.0 else d - b1 * U[1]))
            out["weights"].append((al, b0, b1))
            out["inv_h"].append(inv_h)
            out["phi"].append(phi)
            out["g"].append(g)
            k += 1
        U, hs, t = [new] + U[:2], [h] + hs[:1], t_new
    res = {key: np.array(v) for key, v in out.items()}
    steps = np.array(steps, dtype=np.float64).reshape(-1, 4)
    res.update(steps=steps, facs=np.array(facs), n_accepted=int(steps[:, 3].sum()),
               n_rejected=int(len(steps) - steps[:, 3].sum()), n_restarts=restarts)
    return res


def margins(res):
    """(min |err - 1|, min relative distance of a raw factor from the clip bounds 0.2 and 2) over the attempts with an
    estimate: how far every decision of the run is from flipping."""
    err, fac = res["steps"][:, 2], res["facs"]
    has = np.isfinite(err) & np.isfinite(fac)
    m_err = float(np.min(np.abs(err[has] - 1.0))) if has.any() else math.inf
    rel = [abs(f - b) / b for f in fac[has] for b in (FAC_MIN, FAC_MAX)]
    # the bound of 1 that follows a rejection
    after = np.concatenate([[False], res["steps"][:-1, 3] == 0.0])
    rel += [abs(f - 1.0) for f in fac[has & after]]
    return m_err, (min(rel) if rel else math.inf)


def exact_semidiscrete(bands, u_init, t):
    """u(t) of M u' = -K u with zero Dirichlet ends from u_init: the generalised eigen-decomposition K v = lambda M v
    of the interior block, dense, in float64."""
    from scipy.linalg import eigh
    (md, mo), (kd, ko) = bands["mass"], bands["stiff"]

    def dense(d, o):
        return np.diag(d[1:-1]) + np.diag(o[1:-1], 1) + np.diag(o[1:-1], -1)
    lam, V = eigh(dense(kd, ko), dense(md, mo))             # V^T M V = I
    u = np.zeros_like(np.asarray(u_init, dtype=np.float64))
    u[1:-1] = V @ (np.exp(-lam * t) * (V.T @ (dense(md, mo) @ u_init[1:-1])))
    return u


# ---- the two cases of the record: -u'' on 32 uniform elements of (-1, 1), zero Dirichlet ends --------------------------
def two_mode(x):
    x = np.asarray(x, dtype=np.float64)
    v = np.cos(0.5 * math.pi * x) + 0.5 * np.cos(2.5 * math.pi * x)
    return np.where(np.abs(x) == 1.0, 0.0, v)


def pulse(t):
    return 50.0 * math.exp(-((t - 0.5) / 0.02) ** 2)


if __name__ == "__main__":
    nodes = np.linspace(-1.0, 1.0, 33)
    B = assembled(nodes, f_list=[tp._zero])
    ref = exact_semidiscrete(B, two_mode(nodes), 1.0)
    print("two-mode decay, dt0 = 1e-4:")
    for tol in (1e-3, 1e-4, 1e-5, 1e-6):
        r = solve(nodes, two_mode, 1.0, tol, tol, 1e-4)
        me, mf = margins(r)
        print(f"  tol {tol:.0e}: accepted {r['n_accepted']:4d} rejected {r['n_rejected']:3d}  dt {r['steps'][:, 1].min():.2e}"
              f" .. {r['steps'][:, 1].max():.2e}  error at t = 1 {np.max(np.abs(r['nodal'][-1] - ref)):.2e}"
              f"  margins {me:.1e} {mf:.1e}")
    print("pulse forcing 50 exp(-((t - 0.5) / 0.02)^2) cos(pi x / 2), dt0 = 1e-3:")
    for tol in (1e-3, 1e-4):
        r = solve(nodes, two_mode, 1.0, tol, tol, 1e-3, t_out=[0.25, 0.5, 1.0],
                  forcing=[(pulse, lambda x: np.cos(0.5 * math.pi * x))])
        me, mf = margins(r)
        print(f"  tol {tol:.0e}: accepted {r['n_accepted']:4d} rejected {r['n_rejected']:3d} restarts "
              f"{r['n_restarts']}  margins {me:.1e} {mf:.1e}")
