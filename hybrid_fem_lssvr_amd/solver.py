"""Host-side mirror of the reference's solve-then-enhance call surface.

Same names, argument meaning and error behaviour as
``1D-Possion/Hybrid-FEM-LSSVR-Dual.py`` ("Dual.py"):

* :func:`lssvr_primal`                 -- Dual.py:20-98
* :class:`FEMLSSVRPrimalSolver`        -- Dual.py:100-203
  (``solve_fem``, ``solve_lssvr_subproblems``, ``solve``, ``evaluate_solution``;
  attributes ``fem_nodes``, ``fem_values``, ``lssvr_functions``)
* :func:`true_solution`, :func:`poisson_rhs`, ``main_boundary_condition_*`` -- Dual.py:8-18

What differs is where the arithmetic runs: every step is a hand-written gfx950
kernel behind ``liblssvr_hip.so``; this module only moves arrays to the device,
chooses the right-hand-side mode and wraps results.  There is no CPU fallback:
without the HIP library or without a GPU every solve raises.

Additions over the reference (all keyword-only, defaults reproduce the reference):
``n_colloc`` (hard-coded 12 at Dual.py:40), ``rhs`` (``poisson_rhs`` at Dual.py:157),
``nquad`` (scikit-fem's default 2-point rule for P1), ``mesh`` (a scikit-fem style
mesh/basis or node array instead of ``np.linspace(a, b, num_fem_nodes)``), ``fem_solver``
(``"bands"``: the assembled float64 tridiagonal system, as ``enforce`` + ``solve`` see it;
``"flux"``: exact-structure prefix-scan solve; ``"pivot"``: the bands through the
pivoting partitioned solve of DESIGN.md section 24 -- it lifts the host checks ``c >= 0``, cell Peclet number <= 1 and
``kappa + b n / 2 >= 0`` of the unpivoted solve, returns the plain Galerkin solution above Peclet 1, raises
``RuntimeError`` for a system that is singular to working precision, and has no periodic form), ``solver``
(``ops.SOLVER_PRIMAL`` default; ``ops.SOLVER_SHARED``: uniform meshes only, one shared operator
applied per element), ``coef`` (a pair ``(a, da)`` of numpy-vectorised callables:
solve, estimate and refine ``-(a u')' = f`` instead of ``-u'' = f``, BASELINE config 5 and DESIGN.md
section 11; ``None`` keeps the Poisson rows), ``reaction`` (a numpy-vectorised callable ``c >= 0``: solve,
estimate and refine ``-(a u')' + c u = f``; without ``coef``, a = 1; ``None``: no such term),
``convection`` (a numpy-vectorised callable ``b``: solve, estimate and refine ``-(a u')' + b u' + c u = f``, DESIGN.md
section 18; the P1 system is then non-symmetric and is solved without stabilisation, so every element must have a cell
Peclet number ``|b| h / (2 a) <= 1``; ``None``: no such term), ``boundary`` (a pair ``(left, right)``, each ``None``,
``("dirichlet", g)``, ``("neumann", g)`` or ``("robin", kappa, g)``: the condition ``a du/dn + kappa u = g`` with the
outward normal at an end instead of a fixed value; or the string ``"periodic"``:
``u(x_0) = u(x_ne)`` and ``a u'(x_0) = a u'(x_ne)``, DESIGN.md section 22 -- it needs a reaction term that is positive
somewhere, coefficients that are periodic on the interval, ``fem_solver="bands"`` and a per-element solver, and has no
``solve_goal``; ``None`` keeps the module's Dirichlet functions), ``element_lists`` (``True``: ``element_degrees`` and
``solve_adaptive(mode="hp")`` work with ``coef``, ``reaction`` and ``convection`` and every ``boundary``, one element-list
launch of the table kernels per degree group; ``False``, the default, keeps every path as it was:
Poisson rows, or ``boundary="periodic"`` through one whole-mesh launch per degree, anything else is refused),
``nonlinear`` (``("poly", [q0, q1, ...])``: g(x, u) = sum_k q_k(x) u^k with 1 .. 6 numpy-vectorised callables, or
``("exp", q0, q1)``: g = q0(x) exp(q1(x) u) -- solve ``-(a u')' + b u' + c u + g(x, u) = f`` by a damped Newton
iteration inside ``solve_fem()``; ``fem_solver`` "bands" or "pivot", Dirichlet or Robin ends, one
degree for all elements, and no ``solve_many`` / ``solve_goal`` / ``solve_adaptive`` / ``solve_eigen`` /
``solve_transient``; the checks of the linear problem hold for a, b, c alone, so two Neumann ends without a ``reaction``
are refused as singular even where g_u > 0 would make every Newton matrix definite -- give such a problem a small
``reaction`` and subtract it in q_1; ``None`` keeps every path as it was).
"""
from __future__ import annotations

import math
import types

import numpy as np
from numpy.polynomial.legendre import Legendre

from . import ops
from .mesh import LineMesh, P1Basis, as_line_mesh


# --------------------------------------------------------------------------
# problem definition (Dual.py:8-18)
# --------------------------------------------------------------------------
def true_solution(x):
    """Dual.py:8-9."""
    return np.sin(np.pi * x)


class SinRHS:
    """f(x) = amp * sin(omega * x): callable like the reference's ``poisson_rhs``
    (numpy arithmetic, Dual.py:11-12) and recognised by the facade, which then
    evaluates it inside the kernels instead of tabulating it on the host."""

    def __init__(self, amp, omega):
        self.amp = float(amp)
        self.omega = float(omega)

    def __call__(self, x):
        return self.amp * np.sin(self.omega * x)

    def __repr__(self):
        return f"SinRHS(amp={self.amp!r}, omega={self.omega!r})"


poisson_rhs = SinRHS(np.pi ** 2, np.pi)          # Dual.py:11-12


def main_boundary_condition_left(x):
    """Dual.py:14-15."""
    return 0.0


def main_boundary_condition_right(x):
    """Dual.py:17-18."""
    return 0.0


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _device(device):
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("hybrid_fem_lssvr_amd needs an MI355X (no GPU visible); "
                           "the HIP path has no CPU fallback")
    return torch.device(device)


def _to_dev(a, device):
    torch = _torch()
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=device)


def _read_back(**tensors):
    """ONE device-to-host copy of all ``tensors`` -> {name: float64 array in the tensor's shape}.  A value may also be a
    tuple of tensors (a pair of bands: a tuple of arrays comes back) or None (None comes back); int32 info words come
    back as float64.  The arrays are views of one host buffer."""
    torch = _torch()
    flat = [t for v in tensors.values() if v is not None for t in (v if isinstance(v, tuple) else (v,))]
    host = torch.cat([t.reshape(-1).double() for t in flat]).cpu().numpy()
    parts = iter(np.split(host, np.cumsum([t.numel() for t in flat])[:-1]))

    def take(t):
        return next(parts).reshape(tuple(t.shape))
    return {k: None if v is None else tuple(take(t) for t in v) if isinstance(v, tuple) else take(v)
            for k, v in tensors.items()}


# ---- what the backward sweeps of solve_transient_sensitivity and solve_wave_sensitivity share -------------------------
def _functional_rows(U, jsteps, rows, functional, zero_rows=0):
    """Upload of the functional's rows after the forward loop: (jidx, P, prow).  ``jidx``: the steps of the functional,
    on the device of the trajectory U; P: the rows p_n = dJ/du^n that are not zero, in the order of ``jsteps``, and
    ``zero_rows`` zero rows after them, in one upload; prow: {step: its row of P}.  ``rows=None`` (a misfit): they are
    formed on the host from the observed steps, the one read-back between the loops."""
    jidx = _torch().as_tensor(jsteps, device=U.device)
    if rows is None:
        _, rows = functional(_read_back(u=U[jidx])["u"])
    P = _to_dev(np.concatenate([rows, np.zeros((zero_rows, U.shape[1]))]), U.device)
    return jidx, P, {n: k for k, n in enumerate(jsteps)}


def _sweep_chunks(nsteps, chunk):
    """The cut of the backward sweep over the levels nsteps .. 1 into chunks of up to ``chunk``: (hi, m, side) with hi the
    highest level of a chunk, m its length and side the one of the two alternating chunk buffers it fills."""
    hi, side = nsteps, 0
    while hi >= 1:
        m = min(chunk, hi)
        yield hi, m, side
        hi, side = hi - m, 1 - side


def _dirichlet_u0(kinds, d_u0, d_g):
    """The fix-up after the read-back: at a Dirichlet end u^0_end is the end value g(t_0), so its derivative moves from
    d_u0[end] into d_g[0, s] and d_u0[end] becomes 0, in place.  Returns [(s, end, what d_g[0, s] held)] of those ends."""
    moved = []
    for s, end in ((0, 0), (1, -1)):
        if kinds[s] == ops.END_DIRICHLET:
            moved.append((s, end, d_g[0, s]))
            d_g[0, s] = d_u0[end]
            d_u0[end] = 0.0
    return moved


# ---- the scalar rules of solve_transient_adaptive: float64, pure --------------------------------
TS_SAFETY, TS_FAC_MIN, TS_FAC_MAX = 0.9, 0.2, 2.0
TS_OMEGA_MAX = 2.0              # below the zero-stability limit 1 + sqrt(2) of variable-step BDF2
TS_OUT_SLACK = 1e-9             # a step that ends within this fraction of itself before an output time is stretched to it
TS_MAX_RESTARTS = 8
TS_MONITOR_ROWS = 1024          # rows of one block of the per-attempt monitor on the device


def ts_coefficients(omega):
    """(alpha, beta0, beta1) of variable-step BDF2 at omega = h / h_p; omega = 1 gives (3/2, 2, -1/2) exactly."""
    return (1.0 + 2.0 * omega) / (1.0 + omega), 1.0 + omega, -(omega * omega) / (1.0 + omega)


def ts_error_weights(h, hp, hpp=None, alpha=None):
    """(w3, w2, w1, w0) of the local error estimate e = w3 u^{n+1} + w2 u^n + w1 u^{n-1} + w0 u^{n-2} for the steps
    h, hp, hpp between those times (newest first).  With ``hpp``: h^2 (h + hp) / alpha times the third divided
    difference, the local error of variable-step BDF2 for a cubic.  Without: h^2 times the second divided difference
    (w0 = 0), the backward-Euler error of step 1 as step 2 reads it.  The differences of the times are sums of steps:
    nothing cancels."""
    if hpp is None:
        f = h * h
        return f / (h * (h + hp)), -f / (h * hp), f / ((h + hp) * hp), 0.0
    f = h * h * (h + hp) / alpha
    return (f / (h * (h + hp) * (h + hp + hpp)), -f / (h * hp * (hp + hpp)), f / ((h + hp) * hp * hpp),
            -f / ((h + hp + hpp) * (hp + hpp) * hpp))


def ts_controller(err, bad, p, after_reject):
    """(accepted, fac): accepted iff err <= 1 and no row was non-finite (``bad`` == 0); fac =
    clip(0.9 err^(-1/p), 0.2, grow) with grow = 2, or 1 for the attempt after a rejection; a non-finite attempt is a
    rejection with fac = 0.2.  ``p``: 3 for the BDF2 estimate, 2 for the step-2 estimate."""
    grow = 1.0 if after_reject else TS_FAC_MAX
    if bad != 0 or not math.isfinite(err):
        return False, TS_FAC_MIN
    raw = math.inf if err == 0.0 else TS_SAFETY * err ** (-1.0 / p)
    return err <= 1.0, min(max(raw, TS_FAC_MIN), grow)


def ts_trial_step(t, dt, dt_max, h_prev, t_target):
    """(h, t_new, short): the step of an attempt that starts at ``t`` with the controller's ``dt`` -- capped by dt_max
    and by omega <= 2 against the last accepted step ``h_prev`` (None at step 1), then, if
    t + h (1 + 1e-9) >= t_target, set to t_target - t so that the output time is hit exactly (t_new IS t_target).
    ``short``: the step is below dt."""
    h = min(dt, dt_max)
    if h_prev is not None:
        h = min(h, TS_OMEGA_MAX * h_prev)
    if t + h * (1.0 + TS_OUT_SLACK) >= t_target:
        return t_target - t, t_target, (t_target - t) < dt
    return h, t + h, h < dt


def ts_next_dt(dt, h, short, accepted, fac):
    """The controller's dt after an attempt of step h: fac h, except that an accepted step that was shortened (to hit
    an output, or by a cap) does not shrink dt when its estimate asks for growth."""
    if accepted and short and fac >= 1.0:
        return max(dt, fac * h)
    return fac * h


def _tabulate(fn, pts, point_major=False):
    """Device table of the callable ``fn`` at the device points ``pts`` [ne, k].  The callable ALWAYS sees the
    element-major host array ``x[e, k]`` -- points along the last axis, as in the reference, where it receives the
    1-D array of one element's n points (Dual.py:40-44): a callable that returns a per-point vector of shape (k,),
    or otherwise relies on the last axis being the points, broadcasts the same at every degree (up to
    M = 22 it used to see the transposed array).  The table is handed over as [ne, k], or transposed to [k, ne]
    with ``point_major``; same values either way."""
    xh = pts.cpu().numpy()
    t = np.asarray(fn(xh), dtype=np.float64)
    if t.shape != xh.shape:
        t = np.broadcast_to(t, xh.shape)
    return _to_dev(t.T if point_major else t, pts.device)


def _point_major(M):
    """The lane-per-element kernels (M <= 22) read point-major tables (``t[k, e]``) at full HBM rate; above, the
    tables stay element-major."""
    return int(M) <= 22


def _rhs_mode(rhs, points, point_major=False):
    """Keyword arguments of the Poisson-row operators for the right-hand side: ``rhs=(amp, omega)`` for the named
    f, evaluated in-kernel, else the callable (Dual.py:20 ``rhs_func``) tabulated at ``points()``."""
    if isinstance(rhs, SinRHS):
        return dict(rhs=(rhs.amp, rhs.omega))
    return dict(rhs_values=_tabulate(rhs, points(), point_major), point_major=point_major)


def _one(x):
    return np.ones_like(np.asarray(x, dtype=np.float64))


def _zero(x):
    return np.zeros_like(np.asarray(x, dtype=np.float64))


class _Equation:
    """-(a u')' + b u' + c u = f as the facade holds it: the callables ``a``, ``da``, ``b``, ``c``, ``f``; ``a`` /
    ``da``, ``b`` and ``c`` are None where the term is absent (a = 1, b = 0, c = 0)."""

    def __init__(self, rhs, coef, reaction, convection=None):
        self.a, self.da = coef if coef is not None else (None, None)
        self.b, self.c, self.f = convection, reaction, rhs
        # the Poisson rows: no table but f's
        self.poisson = coef is None and reaction is None and convection is None

    def tables(self, points, point_major=False):
        """(a, a', f, c | None) tabulated at ``points``; without ``coef``, a = 1 and a' = 0.  With convection the
        second table is the folded first-derivative coefficient a' - b of -(a u')' + b u' = -a u'' - (a' - b) u',
        which is all the enhancement and indicator kernels read it as (without ``coef``: -b)."""
        a, da = (_one, _zero) if self.a is None else (self.a, self.da)
        ta, tda, tf = (_tabulate(fn, points, point_major) for fn in (a, da, self.f))
        if self.b is not None:
            tda = tda - _tabulate(self.b, points, point_major)
        return ta, tda, tf, None if self.c is None else _tabulate(self.c, points, point_major)

    def a_ends(self, x):
        """a at the left and right end of every element [ne, 2]: a callable a is continuous at the nodes."""
        an = np.asarray((_one if self.a is None else self.a)(x.cpu().numpy()), dtype=np.float64)
        an = np.broadcast_to(an, (x.numel(),))
        return _to_dev(np.stack([an[:-1], an[1:]], axis=1), x.device)


class _Boundary:
    """``boundary=(left, right)`` of the facade, parsed: per end ``kinds`` (``ops.END_DIRICHLET`` / ``END_ROBIN``),
    ``kappa`` (0 at a Dirichlet end) and ``values`` -- g of a Robin end, the value of a ``("dirichlet", g)`` end, None
    for an end left to the module's Dirichlet function.  ``ValueError`` for anything else."""

    def __init__(self, boundary):
        if not isinstance(boundary, (tuple, list)) or len(boundary) != 2:
            raise ValueError("boundary must be a pair (left, right)")
        self.kinds, self.kappa, self.values = [], [], []
        for side, spec in zip(("left", "right"), boundary):
            kind, kappa, g = ops.END_DIRICHLET, 0.0, None
            if spec is not None:
                if not isinstance(spec, (tuple, list)) or not spec or spec[0] not in ("dirichlet", "neumann", "robin"):
                    raise ValueError(f"boundary[{side}] must be None, ('dirichlet', g), ('neumann', g) or "
                                     f"('robin', kappa, g), got {spec!r}")
                if len(spec) != (3 if spec[0] == "robin" else 2):
                    raise ValueError(f"boundary[{side}] = {spec!r}: '{spec[0]}' takes "
                                     f"{'kappa and g' if spec[0] == 'robin' else 'g'}")
                g = float(spec[-1])
                if spec[0] != "dirichlet":
                    kind = ops.END_ROBIN
                    kappa = float(spec[1]) if spec[0] == "robin" else 0.0
                if not math.isfinite(g) or not math.isfinite(kappa):
                    raise ValueError(f"boundary[{side}] = {spec!r}: kappa and g must be finite")
                if kappa < 0.0:
                    raise ValueError(f"boundary[{side}]: kappa = {kappa} < 0 (a du/dn + kappa u = g needs kappa >= 0: "
                                     "the solve does not pivot)")
            self.kinds.append(kind)
            self.kappa.append(kappa)
            self.values.append(g)

    @property
    def robin(self):
        return ops.END_ROBIN in self.kinds

    def shard(self, ne):
        """The shard arguments with which the enhancement kernels take the FEM nodal value, not a Dirichlet value, as
        the constraint row at a Robin end: their boundary flags fire for global element 0 and ne_global - 1 only."""
        off = 1 if self.kinds[0] == ops.END_ROBIN else 0
        return dict(elem_offset=off, ne_global=off + ne + (1 if self.kinds[1] == ops.END_ROBIN else 0))


class _Nonlinear:
    """``nonlinear=`` of the facade, parsed: ``("poly", [q0, q1, ...])`` -- g(x, u) = sum_k q_k(x) u^k, 1 .. 6 terms --
    or ``("exp", q0, q1)`` -- g = q0(x) exp(q1(x) u); ``kind`` is the ``ops.NL_*`` id and ``q`` the list of callables.
    ``ValueError`` for anything else."""

    def __init__(self, spec):
        if not isinstance(spec, (tuple, list)) or not spec or spec[0] not in ("poly", "exp"):
            raise ValueError("nonlinear must be ('poly', [q0, q1, ...]) or ('exp', q0, q1), got "
                             f"{spec!r}" if not callable(spec) else "nonlinear must be ('poly', [q0, q1, ...]) or "
                             "('exp', q0, q1): g comes from a tabulated family, not from a callable of u")
        if spec[0] == "poly":
            if len(spec) != 2 or not isinstance(spec[1], (tuple, list)):
                raise ValueError("nonlinear=('poly', [q0, q1, ...]) takes one list of callables q_k(x)")
            q = list(spec[1])
            if not 1 <= len(q) <= 6:
                raise ValueError(f"nonlinear 'poly' takes 1 .. 6 terms (nterm), got {len(q)}")
            self.kind = 0           # ops.NL_POLY (the ids are the header's; ops is not needed to refuse)
        else:
            if len(spec) != 3:
                raise ValueError("nonlinear=('exp', q0, q1) takes the two callables q0(x), q1(x)")
            q = list(spec[1:])
            self.kind = 1           # ops.NL_EXP
        if not all(callable(f) for f in q):
            raise ValueError("every q_k of nonlinear must be a callable q_k(x)")
        self.q = q

    def host_tables(self, pts, what):
        """[nterm, *pts.shape] float64 on the host: every q_k at ``pts``; ``ValueError`` for a q_k that does not return
        one value per point (or one that broadcasts) or is not finite there."""
        out = []
        for k, fn in enumerate(self.q):
            try:
                t = np.broadcast_to(np.asarray(fn(pts), dtype=np.float64), pts.shape)
            except ValueError:
                raise ValueError(f"nonlinear q_{k} must return one value per point ({list(pts.shape)} at the {what} "
                                 "points) or a value that broadcasts to them") from None
            if not np.all(np.isfinite(t)):
                raise ValueError(f"nonlinear q_{k} is not finite at a {what} point")
            out.append(t)
        return np.stack(out)

    def tables(self, pts, what, point_major=False):
        """Device tables [nterm, ne, k] (``point_major``: [nterm, k, ne]) of the q_k at the device points [ne, k],
        after the checks of :meth:`host_tables` at those very points (``what`` names them in the message)."""
        t = self.host_tables(pts.cpu().numpy(), what)
        return _to_dev(np.transpose(t, (0, 2, 1)) if point_major else t, pts.device)


class NewtonReport:
    """What the Newton iteration of ``solve_fem()`` with ``nonlinear=`` leaves in ``solver.newton``: ``iterations``
    (linear solves), ``residuals[i]`` = |R(u_i)|_inf and ``steps[i]`` = |u_new - u_i|_inf of iteration i + 1,
    ``lambdas[i]`` the damping it took, ``converged``.  It is assigned before the first iteration and filled as the
    loop runs, so it also holds the history of a solve that raised."""

    def __init__(self):
        self.iterations, self.residuals, self.steps, self.lambdas, self.converged = 0, [], [], [], False

    def __str__(self):
        return (f"{self.iterations} iteration(s), converged={self.converged}, residuals "
                f"{[f'{v:.3e}' for v in self.residuals]}, steps {[f'{v:.3e}' for v in self.steps]}, lambdas "
                f"{self.lambdas}")


def _enhance(x, u, M, gamma, n_colloc, *, global_domain, bc, solver, uniform_rtol=1e-9, **kw):
    """ops.enhance, or -- for ``solver=ops.SOLVER_SHARED`` -- the uniform-mesh shortcut: checks that
    every element length is within ``uniform_rtol`` of the mean, builds the shared operator with
    the general kernel and applies it (``lssvr_enhance_shared``)."""
    if solver != ops.SOLVER_SHARED:
        return ops.enhance(x, u, M, gamma, n_colloc, global_domain=global_domain, bc=bc, solver=solver, **kw)
    ne = x.numel() - 1
    if ne < 1:
        raise ValueError("need at least one element")
    hs = x[1:] - x[:-1]
    h0 = float(((x[-1] - x[0]) / ne).item())
    dev_rel = float(((hs / h0 - 1.0).abs().max()).item())
    if not dev_rel <= uniform_rtol:
        raise ValueError(f"solver='shared' needs a uniform mesh: element lengths deviate by {dev_rel:.2e} "
                         f"(> uniform_rtol = {uniform_rtol:.1e}); use the general solver")
    op = ops.build_shared_operator(h0, M, gamma, n_colloc, device=x.device)
    return ops.enhance_shared(x, u, op, M, n_colloc, global_domain=global_domain, bc=bc, **kw)


class EnhancedSolution:
    """Per-element Legendre coefficients on the device plus what is needed to use
    them: ``W`` float64[ne, M] (row i = ``lssvr_functions[i].coef``), ``nodes``
    float64[ne+1], ``status`` int32[ne] (1 = linear-interpolant fallback)."""

    def __init__(self, nodes, W, status):
        self.nodes = nodes
        self.W = W
        self.status = status

    @property
    def n_fallback(self):
        return int((self.status != 0).sum().item())

    def evaluate(self, x_points, return_elements=False, deriv=0):
        """``evaluate_solution`` (Dual.py:176-203) on the device; ``deriv`` = 1 / 2: the first /
        second x-derivative of the enhanced solution instead (same element rule)."""
        xq = _to_dev(np.asarray(x_points, dtype=np.float64).reshape(-1), self.W.device)
        u, elem = ops.evaluate(self.nodes, self.W, xq, want_elem=True, deriv=deriv)
        u = u.cpu().numpy()
        if return_elements:
            return u, elem.cpu().numpy()
        return u


class GoalEstimate:
    """What :meth:`FEMLSSVRPrimalSolver.solve_goal` returns for J(u) = int j u dx: ``value`` = J(u_enh),
    ``correction`` = sum eta_e (NaN when an eta_e is not finite), ``corrected`` = value + correction, ``eta`` the
    signed per-element terms as numpy, and the device tensors ``eta2`` [ne] = eta^2 and ``out4`` =
    {sum eta, max eta2, non-finite count, sum q} of ``ops.estimate_goal`` for ``ops.refine``."""

    def __init__(self, eta, eta2, out4):
        self.eta2, self.out4 = eta2, out4
        self.eta = eta.cpu().numpy()
        s = out4.cpu().numpy()
        self.n_nonfinite = int(s[2])
        self.value = float(s[3])
        self.correction = float(s[0]) if self.n_nonfinite == 0 else float("nan")
        self.corrected = self.value + self.correction


class Sensitivity:
    """What :meth:`FEMLSSVRPrimalSolver.solve_sensitivity` returns for a functional J of the P1 solution: ``value`` =
    J(u_h) and its derivatives with respect to the data of the P1 solve, as numpy -- ``d_coef``, ``d_convection``,
    ``d_reaction``, ``d_rhs`` [ne, nquad]: dJ/d(a, b, c, f at quadrature point q of element e), the tables of
    ``ops.p1_assemble`` (``d_convection`` / ``d_reaction`` are None where the solver has no such term; without
    ``coef`` the coefficient is the table a = 1, and ``d_coef`` is the derivative there); ``d_end_values`` [2]: dJ/dg
    of the left and right end datum (the Dirichlet value, or g of a Neumann or Robin end); ``d_kappa`` [2]: dJ/dkappa
    (0 at a Dirichlet end); ``adjoint`` the nodal adjoint solution z (0 at a Dirichlet end) and ``nodes`` the mesh.
    :meth:`FEMLSSVRPrimalSolver.solve_semilinear_sensitivity` adds ``d_nonlinear`` [nterm, ne, nquad]: dJ/dq_k of the
    tables of g(x, u), and ``newton``, the :class:`NewtonReport` of its solve.  The mesh is not differentiated."""

    def __init__(self, value, tables, ends, adjoint, nodes):
        self.value = float(value)
        self.d_coef, self.d_convection, self.d_reaction, self.d_rhs = (tables.get(k) for k in ops.SENS_TABLES)
        self.d_end_values, self.d_kappa = ends[:2].copy(), ends[2:].copy()
        self.adjoint, self.nodes = adjoint, nodes


class TransientSensitivity:
    """What :meth:`FEMLSSVRPrimalSolver.solve_transient_sensitivity` returns for a functional J of the BDF trajectory:
    ``value`` = J and its derivatives with respect to the data of the loop, as numpy -- ``d_coef``, ``d_reaction``,
    ``d_weight`` [ne, nquad]: dJ/d(a, c, rho at quadrature point q of element e) (without ``coef`` / ``reaction`` /
    ``weight`` the derivative at the table a = 1 / c = 0 / rho = 1); ``d_forcing`` [R, ne, nquad]: dJ/df_r there;
    ``d_u0`` [ne+1]: dJ/du0 at the nodes (0 at a Dirichlet end: the start is g(0) there); ``d_end_values``
    [nsteps+1, 2]: dJ/dg(t_n) of the left and right end datum, row n for t_n (row 0: the start of a Dirichlet end);
    ``d_kappa`` [2] (0 at a Dirichlet end); ``times`` [nsteps+1] and ``nodes``.  Neither the mesh nor dt is
    differentiated.  With ``nonlinear=``: ``d_nonlinear`` [nterm, ne, nquad]: dJ/dq_k of the tables of g(x, u), and
    ``newton`` [nsteps, newton_iters, 4]: the monitor of the forward loop (|R|, |dv|, |v|, non-finite count per
    iteration), as ``TransientSolution.newton``; both ``None`` for a linear call."""

    def __init__(self, value, tables, d_u0, d_end_values, d_kappa, times, nodes, d_nonlinear=None, newton=None):
        self.value = float(value)
        self.d_coef, self.d_reaction, self.d_weight, self.d_forcing = (tables[k] for k in ops.TS_SENS_TABLES)
        self.d_u0, self.d_end_values, self.d_kappa = d_u0, d_end_values, d_kappa
        self.times, self.nodes = times, nodes
        self.d_nonlinear, self.newton = d_nonlinear, newton


class WaveSensitivity:
    """What :meth:`FEMLSSVRPrimalSolver.solve_wave_sensitivity` returns for a functional J of the Newmark trajectory:
    ``value`` = J and its derivatives with respect to the data of the loop, as numpy -- ``d_coef``, ``d_reaction``,
    ``d_weight``, ``d_damping`` [ne, nquad]: dJ/d(a, c, rho, d at quadrature point q of element e) (without ``coef`` /
    ``reaction`` / ``weight`` the derivative at the table a = 1 / c = 0 / rho = 1; ``d_damping`` is ``None`` without
    ``damping``: the velocities are then not stored); ``d_forcing`` [R, ne, nquad]: dJ/df_r there; ``d_u0``, ``d_v0``
    [ne+1]: dJ/du0, dJ/dv0 at the nodes (``d_u0`` 0 at a Dirichlet end: the start is g(0) there; ``d_v0`` 0 at a
    Dirichlet end with constant data: its velocity is 0); ``d_end_values`` [nsteps+1, 2]: dJ/dg(t_n) of the left and
    right end datum, row n for t_n; ``d_kappa`` [2] (0 at a Dirichlet end); ``d_end_accel0`` [2]: dJ/d end_accel0 (0
    at a Robin end); ``times`` [nsteps+1] and ``nodes``.  Neither the mesh nor dt, beta, gamma is differentiated."""

    def __init__(self, value, tables, d_u0, d_v0, d_end_values, d_kappa, d_end_accel0, times, nodes):
        self.value = float(value)
        self.d_coef, self.d_reaction, self.d_weight, self.d_damping, self.d_forcing = (tables.get(k) for k in
                                                                                       ops.NM_SENS_TABLES)
        self.d_u0, self.d_v0, self.d_end_values, self.d_kappa = d_u0, d_v0, d_end_values, d_kappa
        self.d_end_accel0, self.times, self.nodes = d_end_accel0, times, nodes


def _evaluate_item(items, method, what, i, x, deriv):
    """``evaluate`` of the solution classes below: item ``i`` of their :class:`EnhancedSolution` list at ``x``."""
    if not items:
        raise RuntimeError(f"{method} ran with enhance=False: there are no enhanced {what} to evaluate")
    x = np.asarray(x, dtype=np.float64)
    return items[i].evaluate(x.reshape(-1), deriv=deriv).reshape(x.shape)


class EigenSolution:
    """What :meth:`FEMLSSVRPrimalSolver.solve_eigen` returns for the k eigenvalues of -(a u')' + c u = lambda rho u
    nearest the shift, in the order of their distance from it:

    * ``values_fem`` float64[k]: the P1 eigenvalues; ``values`` float64[k]: the Rayleigh quotients of the enhanced
      modes (``None`` with ``enhance=False``);
    * ``residuals`` float64[k]: |K x_j - theta_j M x_j|_2; ``index`` int[k]: the position of each mode in the ascending
      discrete spectrum, counted from 0 (the number of eigenvalues below it), by the Sturm count (``None`` when the iteration did not converge);
    * ``iterations``, ``converged``; ``nodal`` float64[k, ne+1]: the modes' nodal values, M-orthonormal, each with a
      positive value at the first unknown; ``modes``: k :class:`EnhancedSolution` (empty with ``enhance=False``)."""

    def __init__(self, values_fem, values, residuals, index, iterations, converged, nodal, modes, sigma):
        self.values_fem, self.values, self.residuals, self.index = values_fem, values, residuals, index
        self.iterations, self.converged, self.nodal, self.modes, self.sigma = iterations, converged, nodal, modes, sigma

    def evaluate(self, j, x, deriv=0):
        """The enhanced mode ``j`` (its ``deriv``-th derivative) at the points ``x``."""
        return _evaluate_item(self.modes, "solve_eigen", "modes", j, x, deriv)


class TransientSolution:
    """What :meth:`FEMLSSVRPrimalSolver.solve_transient` returns for its ``ns`` snapshots, in ascending time:

    * ``times`` float64[ns];
    * ``nodal`` float64[ns, ne+1]: the P1 nodal values;
    * ``enhanced``: ns :class:`EnhancedSolution` (empty with ``enhance=False``);
    * ``bands``, a diagnostic: host copies of what the loop ran on, as the device assembled it --
      dict(mass=(mdiag, moff), step={alpha: (diag, off)}, loads [R, ne+1]); with ``nonlinear=`` the step matrices are
      the LINEAR part K + (alpha / dt) M, to which every Newton iteration adds the mass matrix of g_u;
    * ``newton`` (``None`` without ``nonlinear=``) float64[nsteps, newton_iters, 4]: row [n - 1, k] holds what
      ``ops.nl_residual`` read in iteration k of step n -- |residual at v_k|_inf, |v_{k+1} - v_k|_inf, |v_{k+1}|_inf
      and the count of non-finite entries.

    :meth:`FEMLSSVRPrimalSolver.solve_transient_adaptive` returns the same, one snapshot per output time, with
    ``bands`` = dict(mass, stiff=(kdiag, koff) of -(a u')' + c u, loads), and adds

    * ``steps`` float64[attempts, 4]: every attempt's (t it starts from, its step, the scaled estimate err -- nan at a
      first step, which has none --, 1.0 accepted / 0.0 rejected), in the order they were made, restarts included;
    * ``n_accepted``, ``n_rejected``, ``n_restarts``;
    * ``monitor`` float64[attempts with an estimate, 4]: what ``ops.ts_error`` wrote, as read back after the loop."""

    def __init__(self, times, nodal, enhanced, bands, newton=None, steps=None, n_restarts=0, monitor=None):
        self.times, self.nodal, self.enhanced, self.bands, self.newton = times, nodal, enhanced, bands, newton
        self.steps, self.n_restarts, self.monitor = steps, n_restarts, monitor
        self.n_accepted = None if steps is None else int(np.count_nonzero(steps[:, 3]))
        self.n_rejected = None if steps is None else int(len(steps)) - self.n_accepted

    def evaluate(self, k, x, deriv=0):
        """The enhanced snapshot ``k`` (its ``deriv``-th x-derivative) at the points ``x``."""
        return _evaluate_item(self.enhanced, "solve_transient", "snapshots", k, x, deriv)


class WaveSolution:
    """What :meth:`FEMLSSVRPrimalSolver.solve_wave` returns for its ``ns`` snapshots, in ascending time:

    * ``times`` float64[ns];
    * ``nodal``, ``velocity``, ``accel`` float64[ns, ne+1]: the nodal u, u_t and u_tt of the Newmark rule;
    * ``energy`` float64[ns + 1]: 1/2 v^T M_rho v + 1/2 u^T K u + 1/2 sum over the Robin ends of kappa u_end^2 at
      t = 0 (index 0) and at every snapshot (index k + 1), over all nodes;
    * ``enhanced``: ns :class:`EnhancedSolution` (empty with ``enhance=False``);
    * ``bands``, a diagnostic: host copies of what the loop ran on, as the device assembled it --
      dict(mass=(mdiag, moff), damp=(ddiag, doff) or None, stiff=(kdiag, koff), step=(diag, off), loads [R, ne+1])."""

    def __init__(self, times, nodal, velocity, accel, energy, enhanced, bands):
        self.times, self.nodal, self.velocity, self.accel = times, nodal, velocity, accel
        self.energy, self.enhanced, self.bands = energy, enhanced, bands

    def evaluate(self, k, x, deriv=0):
        """The enhanced snapshot ``k`` (its ``deriv``-th x-derivative) at the points ``x``."""
        return _evaluate_item(self.enhanced, "solve_wave", "snapshots", k, x, deriv)


class _ElementFunctions:
    """``solver.lssvr_functions``: a read-only sequence whose item i is
    ``Legendre(W[i], [x_i, x_{i+1}])`` (Dual.py:95, 163) -- built lazily from the device
    coefficients, so a 1e7-element solve does not create 1e7 Python objects."""

    def __init__(self, nodes_host, W_dev):
        self._nodes = nodes_host
        self._W_dev = W_dev
        self._W = None

    def _host(self):
        if self._W is None:
            self._W = self._W_dev.cpu().numpy()
        return self._W

    def __len__(self):
        return self._W_dev.shape[0]

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return Legendre(self._host()[i], [self._nodes[i], self._nodes[i + 1]])

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]


def enhance_elements(mesh, nodal_values, M, gamma, *, n_colloc=12, rhs=poisson_rhs,
                     global_domain=None, bc=(0.0, 0.0), device="cuda:0", solver=ops.SOLVER_PRIMAL):
    """Batched entry: every element of ``mesh`` (scikit-fem style mesh / basis, or
    node array) gets its LSSVR polynomial in one launch.  Returns EnhancedSolution."""
    dev = _device(device)
    m = as_line_mesh(mesh)
    x = _to_dev(m.nodes, dev)
    u = _to_dev(nodal_values, dev)
    if u.numel() != x.numel():
        raise ValueError("nodal_values must have one value per mesh node")
    if global_domain is None:
        global_domain = (float(m.nodes[0]), float(m.nodes[-1]))
    kw = _rhs_mode(rhs, lambda: ops.colloc_points(x, n_colloc), _point_major(M))
    W, st = _enhance(x, u, int(M), float(gamma), int(n_colloc), global_domain=global_domain,
                     bc=bc, solver=solver, **kw)
    return EnhancedSolution(x, W, st)


def enhance_elements_hetero(mesh, nodal_values, M, gamma, *, n_colloc=12, rhs=poisson_rhs,
                            global_domain=None, bc=(0.0, 0.0), device="cuda:0"):
    """Per-element ``M`` / ``gamma`` / ``n_colloc`` (the reference has one
    ``lssvr_M`` / ``lssvr_gamma`` per mesh, Dual.py:101).  Each of the three is a scalar or an
    array with one entry per element.  Elements are grouped by (M, n_colloc); every group is
    one ``lssvr_enhance_subset`` launch writing straight into the rows of a zero-padded
    ``W[ne, max M]`` (a Legendre series with trailing zeros evaluates identically), so
    ``EnhancedSolution.evaluate`` works unchanged.  ``lssvr_functions``-style access:
    ``Legendre(W[i, :M_i], [x_i, x_{i+1}])``."""
    torch = _torch()
    dev = _device(device)
    m = as_line_mesh(mesh)
    ne = m.nelements
    x = _to_dev(m.nodes, dev)
    u = _to_dev(nodal_values, dev)
    if u.numel() != x.numel():
        raise ValueError("nodal_values must have one value per mesh node")
    if global_domain is None:
        global_domain = (float(m.nodes[0]), float(m.nodes[-1]))
    Ms = np.broadcast_to(np.asarray(M, dtype=np.int64), (ne,))
    ns = np.broadcast_to(np.asarray(n_colloc, dtype=np.int64), (ne,))
    gs = np.array(np.broadcast_to(np.asarray(gamma, dtype=np.float64), (ne,)))
    if np.any(gs <= 0):
        raise ValueError("gamma must be > 0 for every element")
    W = torch.zeros((ne, int(Ms.max())), dtype=torch.float64, device=dev)
    st = torch.zeros((ne,), dtype=torch.int32, device=dev)
    gv = _to_dev(gs, dev)
    for Mg, ng in sorted({(int(a), int(b)) for a, b in zip(Ms, ns)}):
        ids_h = np.nonzero((Ms == Mg) & (ns == ng))[0].astype(np.int64)
        ids = torch.as_tensor(ids_h, device=dev)
        # (a callable f is tabulated at this group's collocation points, np.linspace per element)
        kw = _rhs_mode(rhs, lambda: ops.colloc_points(x, ng)[ids])
        ops.enhance_subset(x, u, Mg, 1.0, ng, W, elem_ids=ids, gamma_values=gv,
                           global_domain=global_domain, bc=bc, status=st, **kw)
    sol = EnhancedSolution(x, W, st)
    sol.degrees = Ms.copy()
    return sol


# --------------------------------------------------------------------------
# lssvr_primal (Dual.py:20-98)
# --------------------------------------------------------------------------
def lssvr_primal(rhs_func, domain_range, u_xmin, u_xmax, M, gamma,
                 is_left_boundary=False, is_right_boundary=False,
                 global_domain_range=(-1, 1), *, n_colloc=12, device="cuda:0"):
    """One element's LSSVR polynomial; same signature as Dual.py:20-22.

    Returns ``numpy.polynomial.legendre.Legendre(coef, domain_range)`` like the
    reference (Dual.py:95-98).  The equality-constrained QP of Dual.py:46-78 is
    solved in closed form on the GPU instead of by SLSQP; a breakdown of the
    factorisation prints the reference's warning (Dual.py:90-92) and returns the
    linear interpolant of the boundary values (Dual.py:164-169)."""
    dev = _device(device)
    xmin, xmax = float(domain_range[0]), float(domain_range[1])
    x = _to_dev([xmin, xmax], dev)
    u = _to_dev([u_xmin, u_xmax], dev)
    # the kernel derives the flags from the element's global index (Dual.py:150-151)
    off = 0 if is_left_boundary else 1
    ne_global = off + 1 if is_right_boundary else off + 2
    kw = _rhs_mode(rhs_func, lambda: ops.colloc_points(x, n_colloc), _point_major(M))
    W, st = ops.enhance(x, u, int(M), float(gamma), int(n_colloc), elem_offset=off,
                        ne_global=ne_global,
                        global_domain=(float(global_domain_range[0]), float(global_domain_range[1])),
                        bc=(main_boundary_condition_left(global_domain_range[0]),
                            main_boundary_condition_right(global_domain_range[1])), **kw)
    if int(st[0].item()) != 0:
        print("Warning: Optimization may not have converged: factorisation breakdown "
              "(linear interpolant returned)")
    return Legendre(W[0].cpu().numpy(), [domain_range[0], domain_range[1]])


# --------------------------------------------------------------------------
# FEMLSSVRPrimalSolver (Dual.py:100-203)
# --------------------------------------------------------------------------
class FEMLSSVRPrimalSolver:
    def __init__(self, num_fem_nodes=5, lssvr_M=12, lssvr_gamma=1e6, global_domain=(-1, 1), *,
                 n_colloc=12, rhs=poisson_rhs, nquad=2, mesh=None, device="cuda:0",
                 solver=ops.SOLVER_PRIMAL, fem_solver="bands", coef=None, reaction=None, convection=None,
                 boundary=None, element_lists=False, nonlinear=None, fem_order=1):
        # Dual.py:101-108
        self.num_fem_nodes = num_fem_nodes
        self.lssvr_M = lssvr_M
        self.lssvr_gamma = lssvr_gamma
        self.global_domain = global_domain
        self.fem_nodes = None
        self.fem_values = None
        self.lssvr_functions = []
        # additions
        self.n_colloc = n_colloc
        self.rhs = rhs
        self.nquad = nquad
        self.mesh = None if mesh is None else as_line_mesh(mesh)
        self.device = device
        self.solver_id = solver
        if fem_solver not in ("bands", "flux", "pivot"):
            raise ValueError("fem_solver must be 'bands', 'flux' or 'pivot'")
        self.fem_solver = fem_solver
        if coef is not None:
            if not (isinstance(coef, (tuple, list)) and len(coef) == 2 and all(callable(c) for c in coef)):
                raise ValueError("coef must be a pair (a, da) of callables")
            # lssvr_enhance_varcoef has no solver selector: it takes its own path by M and n_colloc
            if solver != ops.SOLVER_PRIMAL:
                raise ValueError("coef (variable coefficients) needs solver=ops.SOLVER_PRIMAL"
                                 + (": the shared operator holds the Poisson rows only"
                                    if solver == ops.SOLVER_SHARED else ""))
            coef = tuple(coef)
        self.coef = coef
        if reaction is not None:
            if not callable(reaction):
                raise ValueError("reaction must be a callable c(x)")
            if fem_solver == "flux":
                raise ValueError("reaction needs fem_solver='bands': the flux solve factors A = D^T K D, "
                                 "which a mass matrix breaks")
            if solver != ops.SOLVER_PRIMAL:
                raise ValueError("reaction needs solver=ops.SOLVER_PRIMAL: the reaction rows have a primal "
                                 "solve only")
        self.reaction = reaction
        if convection is not None:
            if not callable(convection):
                raise ValueError("convection must be a callable b(x)")
            if fem_solver == "flux":
                raise ValueError("convection needs fem_solver='bands': the flux solve factors A = D^T K D, "
                                 "which a non-symmetric matrix breaks")
            if solver != ops.SOLVER_PRIMAL:
                raise ValueError("convection needs solver=ops.SOLVER_PRIMAL: the rows with a first-derivative "
                                 "term have a primal solve only")
        self.convection = convection
        if isinstance(boundary, str) and boundary == "periodic":
            if fem_solver == "pivot":
                raise ValueError("boundary='periodic' needs fem_solver='bands': the seam Schur complement is built "
                                 "from two Dirichlet solves, which can be singular where the periodic problem is "
                                 "not; the pivoting solve has no cyclic form yet")
            if fem_solver == "flux":
                raise ValueError("boundary='periodic' needs fem_solver='bands': the flux solve factors "
                                 "A = D^T K D between two Dirichlet values")
            if solver == ops.SOLVER_SHARED:
                raise ValueError("boundary='periodic' needs a per-element solver, not ops.SOLVER_SHARED: the "
                                 "shared operator takes its end rows from the Dirichlet values")
        elif boundary is not None and _Boundary(boundary).robin:
            if fem_solver == "flux":
                raise ValueError("a Neumann or Robin end needs fem_solver='bands': the flux solve factors "
                                 "A = D^T K D between two Dirichlet values")
            if solver == ops.SOLVER_SHARED:
                raise ValueError("a Neumann or Robin end needs a per-element solver, not ops.SOLVER_SHARED: the "
                                 "shared operator takes its end rows from the Dirichlet values")
        self.boundary = boundary
        # one degree per element (element_degrees, solve_adaptive(mode="hp")) for coef / reaction / convection with any
        # boundary, through the element lists of the table kernels; False: every path as it was
        self.element_lists = bool(element_lists)
        # -(a u')' + b u' + c u + g(x, u) = f by a damped Newton iteration; None: every path as
        # it was
        if nonlinear is not None:
            _Nonlinear(nonlinear)
            if fem_solver == "flux":
                raise ValueError("nonlinear needs fem_solver='bands' or 'pivot': every Newton step carries the mass "
                                 "matrix of c + g_u, which the flux solve does not hold")
            if isinstance(boundary, str) and boundary == "periodic":
                raise ValueError("nonlinear has no boundary='periodic': the Newton loop runs the solves with "
                                 "Dirichlet or Robin ends")
            if solver != ops.SOLVER_PRIMAL:
                raise ValueError("nonlinear needs solver=ops.SOLVER_PRIMAL: the linearised rows are reaction rows, "
                                 "which have a primal solve only")
            if self.element_lists:
                raise ValueError("nonlinear has no element_lists / element_degrees: the linearised tables are "
                                 "written for one degree")
        self.nonlinear = nonlinear
        # the degree of the element space of the P1 half: 2 .. 4 add the hierarchic bubbles up
        # to that degree and condense them out, so the nodal values converge like h^(2 fem_order); 1: every path as it
        # was
        self.fem_order = fem_order
        self._check_fem_order()
        self.newton = None              # NewtonReport after solve_fem() with nonlinear
        self.enhanced = None            # EnhancedSolution after solve_lssvr_subproblems
        self.adapt_history = []         # solve_adaptive: one dict(ne, estimate, marked) per round
        self.dual = None                # EnhancedSolution of the dual problem after solve_goal
        self.element_degrees = None     # one M per element (2 .. 33) instead of lssvr_M; solve_adaptive(mode="hp")
        self._x_dev = None
        self._u_dev = None

    def _check_fem_order(self, what=None):
        """``fem_order`` and what it needs of the other (public) attributes, on the host; ``what``: a method that
        assembles for itself and has no ``fem_order > 1`` (``ValueError``)."""
        p = self.fem_order
        if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 1 <= p <= 4:
            raise ValueError(f"fem_order must be an integer in 1 .. 4, got {p!r}")
        if p == 1:
            return
        if what is not None:
            raise ValueError(f"{what} has no fem_order > 1: it assembles the P1 matrices for itself; the "
                             "bubble-condensed bands serve solve(), solve_many(), estimate() and "
                             "solve_adaptive(mode='h')")
        if int(self.nquad) < p + 1 or int(self.nquad) > 5:
            raise ValueError(f"fem_order = {p} needs nquad in fem_order+1 .. 5 = {p + 1} .. 5 (the element matrices "
                             f"hold polynomials of degree 2 fem_order), got nquad = {self.nquad}")
        if self.fem_solver == "flux":
            raise ValueError("fem_order > 1 needs fem_solver='bands' or 'pivot': the flux solve factors "
                             "A = D^T K D, which the condensed element matrices do not have")
        if self.nonlinear is not None:
            raise ValueError("nonlinear has no fem_order > 1: the Newton loop assembles the P1 matrices for itself")

    def _check_bubble_rhs(self, rhs_list):
        """The bubble-condensed entry takes tabulated loads only."""
        self._check_fem_order()
        for f in rhs_list:
            if isinstance(f, SinRHS):
                raise ValueError("fem_order > 1 takes tabulated loads only: a SinRHS right-hand side is evaluated "
                                 "inside the P1 assembly kernel, which the bubble-condensed assembly does not do; "
                                 "pass a callable f(x)")
        if len(rhs_list) > ops.BUBBLE_MAX_CASES:
            raise ValueError(f"fem_order > 1 assembles at most {ops.BUBBLE_MAX_CASES} load cases in one call, "
                             f"got {len(rhs_list)}")

    def _check_bands(self, bands, x):
        """The hypothesis of the unpivoted solve on the condensed ``bands`` (the header of tridiag.hip), in one
        device reduction and one read-back before the solve: every entry finite, every row dominant (kappa joins a
        Robin end row).  ``fem_solver="pivot"`` needs only the first."""
        bnd, pivot = self._bnd, self.fem_solver == "pivot"
        free = (False, False) if bnd is None else tuple(k == ops.END_ROBIN for k in bnd.kinds)
        kappa = (0.0, 0.0) if bnd is None else bnd.kappa
        finite, row, margin = ops.band_dominance(bands["diag"], bands["sub"], bands["sup"], free, kappa,
                                                 self._periodic)
        if finite and (pivot or margin >= 0.0):
            return
        nodes = x.cpu().numpy()
        ne = nodes.size - 1
        lo, hi = nodes[max(row - 1, 0)], nodes[min(row + 1, ne)]
        if not finite:
            msg = (f"the bubble-condensed bands of fem_order = {self.fem_order} are not finite (worst row {row}, "
                   f"elements on [{lo:.6g}, {hi:.6g}]): a bubble pivot was zero or not finite; refine the mesh there")
            if pivot:
                raise RuntimeError(msg)
            raise ValueError(msg + " or check the coefficients")
        raise ValueError(f"row {row} of the bubble-condensed bands (elements on [{lo:.6g}, {hi:.6g}]) is not "
                         f"diagonally dominant: diag - |sub| - |sup| = {margin:.3g} < 0, and the tridiagonal solve "
                         "does not pivot; refine the mesh there or use fem_solver='pivot'")

    @property
    def _eq(self):
        # (from the attributes at the time of use: they are public, and were always read when solving)
        return _Equation(self.rhs, self.coef, self.reaction, self.convection)

    def _default_mesh(self):
        return LineMesh.from_nodes(np.linspace(self.global_domain[0], self.global_domain[1], self.num_fem_nodes))

    @property
    def _bnd(self):
        """The parsed ``boundary`` when an end is Neumann or Robin, else None: ``boundary=None`` and two Dirichlet
        ends take the Dirichlet path."""
        if self.boundary is None or self._periodic:
            return None
        b = _Boundary(self.boundary)
        return b if b.robin else None

    @property
    def _periodic(self):
        """``boundary="periodic"``: u(x_0) = u(x_ne) and a u'(x_0) = a u'(x_ne), DESIGN.md section 22."""
        return isinstance(self.boundary, str) and self.boundary == "periodic"

    def _shard(self, ne):
        """The shard arguments of the enhancement for the configured ends: none with Dirichlet ends, those of
        :meth:`_Boundary.shard` with a Neumann or Robin end; on a periodic domain no Dirichlet flag may fire, so
        elements 0 and ne-1 take the seam value as their nodal constraint like an interior node."""
        if self._periodic:
            return dict(elem_offset=1, ne_global=ne + 2)
        bnd = self._bnd
        return {} if bnd is None else bnd.shard(ne)

    def _gd_bc(self):
        """(global domain, end values at its two ends) as float pairs: the Dirichlet value -- the module's function,
        or g of ``("dirichlet", g)`` -- or, at a Neumann or Robin end, its g."""
        gd = (float(self.global_domain[0]), float(self.global_domain[1]))
        bc = (main_boundary_condition_left(self.global_domain[0]),
              main_boundary_condition_right(self.global_domain[1]))
        if self.boundary is not None and not self._periodic:      # (periodic: no end value is read anywhere)
            bc = tuple(d if g is None else g for d, g in zip(bc, _Boundary(self.boundary).values))
        return gd, bc

    def _reaction_positive(self, eq, nodes, nonzero=False):
        """Whether the reaction term is positive (``nonzero``: not zero) at a quadrature point of the P1 assembly."""
        if eq.c is None:
            return False
        xi = np.polynomial.legendre.leggauss(int(self.nquad))[0]
        xq = 0.5 * (nodes[:-1] + nodes[1:])[:, None] + 0.5 * np.diff(nodes)[:, None] * xi[None, :]
        cq = np.broadcast_to(np.asarray(eq.c(xq), dtype=np.float64), xq.shape)
        return bool(np.any(cq != 0.0 if nonzero else cq > 0.0))

    def _check_periodic(self, m):
        """What the periodic solve needs, on the host and before any launch: the assembled bands and a per-element
        solver, at least two elements, a problem that is not singular, and coefficients that are periodic on this
        interval."""
        if self.fem_solver != "bands" or self.solver_id == ops.SOLVER_SHARED:     # (attributes are public)
            raise ValueError("boundary='periodic' needs fem_solver='bands' and a per-element solver")
        eq = self._eq
        nodes = np.asarray(m.nodes, dtype=np.float64)
        if nodes.size < 3:
            raise ValueError("boundary='periodic' needs at least two elements")
        if not self._reaction_positive(eq, nodes):
            raise ValueError("singular problem: periodic ends and no reaction that is positive at a quadrature point "
                             "leave u determined up to a constant")
        ends = nodes[[0, -1]]
        for name, fn in (("coef a", eq.a), ("coef da", eq.da), ("convection", eq.b), ("reaction", eq.c)):
            if fn is None:
                continue
            v = np.broadcast_to(np.asarray(fn(ends), dtype=np.float64), (2,))
            if not abs(float(v[0]) - float(v[1])) <= 1e-12 * max(1.0, abs(float(v[0])), abs(float(v[1]))):
                raise ValueError(f"{name} is not periodic on [{ends[0]:.6g}, {ends[1]:.6g}]: {float(v[0])!r} at the "
                                 f"left end, {float(v[1])!r} at the right end")

    def _check_boundary(self, m):
        """What makes the unpivoted solve with a Neumann or Robin end safe, on the host and before any launch: the
        matrix is not singular, and with convection the end row keeps its dominance.  ``fem_solver="pivot"`` needs
        only the first: two Neumann ends and a reaction that vanishes at every quadrature point."""
        if self._periodic:
            return self._check_periodic(m)
        bnd = self._bnd
        if bnd is None:
            return
        if self.fem_solver == "flux" or self.solver_id == ops.SOLVER_SHARED:      # (attributes are public)
            raise ValueError("a Neumann or Robin end needs fem_solver='bands' and a per-element solver")
        pivot = self.fem_solver == "pivot"
        eq = self._eq
        nodes = np.asarray(m.nodes, dtype=np.float64)
        if bnd.kinds == [ops.END_ROBIN, ops.END_ROBIN] and bnd.kappa[0] + bnd.kappa[1] == 0.0:
            if not self._reaction_positive(eq, nodes, nonzero=pivot):
                raise ValueError("singular problem: two Neumann ends (kappa_left + kappa_right = 0) and no reaction "
                                 f"that is {'nonzero' if pivot else 'positive'} at a quadrature point leave u "
                                 "determined up to a constant")
        if eq.b is not None and not pivot:
            b_end = np.broadcast_to(np.asarray(eq.b(nodes[[0, -1]]), dtype=np.float64), (2,))
            for i, (side, n) in enumerate((("left", -1.0), ("right", 1.0))):
                if bnd.kinds[i] == ops.END_ROBIN and not bnd.kappa[i] + 0.5 * n * float(b_end[i]) >= 0.0:
                    raise ValueError(f"{side} end: kappa + b n / 2 = {bnd.kappa[i] + 0.5 * n * float(b_end[i]):.3g} "
                                     "< 0 (n the outward normal): an inflow Neumann or Robin end this weak loses "
                                     "coercivity, and the solve does not pivot; raise kappa or fix u there")

    def _fem_setup(self):
        """(mesh, x device, xq device, kw) of a P1 assembly: the nodes, the quadrature points and the coefficient
        tables ``ops.p1_assemble`` takes as keywords, after the checks that make the unpivoted solve safe."""
        m = self._default_mesh() if self.mesh is None else self.mesh
        self._check_boundary(m)
        x = _to_dev(m.nodes, _device(self.device))
        xq = ops.quad_points(x, self.nquad)
        eq, kw = self._eq, {}
        if eq.a is not None:             # kloc = abar / h, abar the quadrature mean of a
            kw["a_quad"] = _tabulate(eq.a, xq)
        if eq.c is not None:             # consistent mass matrix of c in the bands
            cq = _tabulate(eq.c, xq)
            if self.fem_solver != "pivot" and bool((cq < 0).any().item()):
                raise ValueError("reaction is negative at a quadrature point: the tridiagonal solve does not "
                                 "pivot and assumes an SPD matrix (c >= 0)")
            kw["c_quad"] = cq
        if eq.b is not None and self.fem_order > 1:      # (no Peclet bound: _check_bands looks at the bands themselves)
            kw["b_quad"] = _tabulate(eq.b, xq)
        elif eq.b is not None:           # b u' in the bands: sub and sup instead of off
            kw["b_quad"] = self._convection_quad(eq, x, xq)
        return m, x, xq, kw

    def _fem(self, rhs, u0, u1):
        """(mesh, x device, u device, bands) of the P1 solve for the right-hand side ``rhs`` and the end values
        ``u0``, ``u1`` (:meth:`_gd_bc`); no attribute of the solver is written."""
        if self.fem_order != 1:
            return self._fem_bubble(rhs, u0, u1)
        m, x, xq, kw = self._fem_setup()
        if isinstance(rhs, SinRHS):
            bands = ops.p1_assemble(x, self.nquad, rhs=(rhs.amp, rhs.omega), want_local=True, **kw)
        else:
            fq = _to_dev(rhs(xq.cpu().numpy()), x.device)
            bands = ops.p1_assemble(x, self.nquad, rhs_quad=fq, want_local=True, **kw)
        return m, x, self._p1_solve(bands, "b_quad" in kw, u0, u1), bands

    def _bubble_assemble(self, rhs_list):
        """(mesh, x device, bands) of ``fem_order > 1``: ONE ``ops.p1_assemble_bubble`` for all right-hand sides
        (``load`` [ncases, ne+1]), then the check of the bands.  The bands are the non-symmetric ones (sub, sup),
        with or without convection."""
        self._check_bubble_rhs(rhs_list)
        m, x, xq, kw = self._fem_setup()
        xq_host = xq.cpu().numpy()
        fq = [_to_dev(f(xq_host), x.device) for f in rhs_list]
        for j, t in enumerate(fq):
            if t.numel() != xq.numel():
                raise ValueError(f"right-hand side {j} must return one value per quadrature point "
                                 f"({list(xq.shape)}), got {list(t.shape)}")
        fq = _torch().stack([t.reshape(xq.shape) for t in fq])
        bands = ops.p1_assemble_bubble(x, int(self.fem_order), int(self.nquad), fq, want_local=True, **kw)
        self._check_bands(bands, x)
        return m, x, bands

    def _fem_bubble(self, rhs, u0, u1):
        """:meth:`_fem` with ``fem_order > 1``."""
        m, x, bands = self._bubble_assemble([rhs])
        bands = {k: (v[0] if k in ("load", "floc") else v) for k, v in bands.items()}
        return m, x, self._tridiag_solve(bands, bands["load"], True, (u0, u1), False), bands

    def _p1_solve(self, bands, conv, u0, u1):
        """u device [ne+1] of the assembled ``bands`` with the end values ``u0``, ``u1`` for the configured ends and
        ``fem_solver``; ``conv``: the bands are the non-symmetric ones (sub, sup).  The one dispatch behind
        :meth:`_fem` and the Newton steps of :meth:`_solve_fem_newton`."""
        if self.fem_solver == "flux" and not (self._periodic or self._bnd is not None or conv):
            # exact-structure solution of A = D^T K D by the element-flux prefix scan
            return ops.p1_flux_solve(bands["kloc"], bands["load"], u0, u1)
        return self._tridiag_solve(bands, bands["load"], conv, (u0, u1), False)

    def _tridiag_solve(self, bands, load, conv, ends, multi):
        """The tridiagonal solve of ``load`` ([ne+1], or [nc, ne+1] with ``multi``) on the assembled ``bands``: the
        one ladder that picks the ``ops.tridiag_*`` function by ``fem_solver="pivot"``, the configured ends (periodic,
        Neumann or Robin, Dirichlet), ``conv`` (the non-symmetric bands sub, sup) and ``multi``.  ``ends``: the pair
        (u0, u1), with ``multi`` the float64 host array [nc, 2] (uploaded here, where the solve reads it)."""
        bnd = self._bnd
        if self.fem_solver == "pivot":
            return self._pivot_solve(bands, load, _to_dev(ends, load.device) if multi else ends, multi)
        # the families of ops.tridiag_* (none of these pivots or stabilises: with convection, _convection_quad has
        # checked the cell Peclet number):
        #   periodic   node ne is node 0: the cyclic solve reads no end value (_check_periodic has run)
        #   bc         a Neumann or Robin end stays an unknown; kappa and g join its row inside the solve
        #              (_check_boundary has run)
        #   dirichlet  the ASSEMBLED float64 bands (rounded diagonal included) through `enforce` + `solve` semantics
        #              (Dual.py:129-130).  Which matrix scikit-fem itself assembles is an assumption of SURVEY.md
        #              Appendix C -- parity unpinned, the package is not importable here (the reference negates both
        #              forms, Dual.py:117-124: -K u = -b; this code assembles +K u = +b, the same u)
        family = "periodic" if self._periodic else "dirichlet" if bnd is None else "bc"
        fn = getattr(ops, f"tridiag_{'ns_' if conv else ''}{family}_solve{'_multi' if multi else ''}")
        system = (bands["diag"], bands["sub"], bands["sup"], load) if conv else (bands["diag"], bands["off"], load)
        if family == "periodic":
            return fn(*system)
        if multi:
            ends = _to_dev(ends, load.device)
        if family == "bc":
            return fn(*system, bnd.kinds, bnd.kappa, ends)
        return fn(*system, ends) if multi else fn(*system, *ends)

    def _fem_many(self, rhs_list, bc):
        """(x device, U device [ncases, ne+1]) of the P1 solves of :meth:`solve_many`: what ``_fem`` per case returns,
        bit for bit, with the work that does not depend on the load done once -- the coefficient tables and their
        checks, ONE assembly of the bands, the loads of all callable right-hand sides in one ``ops.p1_load_multi``,
        one multi-RHS solve.  A ``SinRHS`` keeps its load from the in-kernel-sin assembly; ``fem_solver="flux"``
        keeps the per-case path.  ``bc``: float64 host array [ncases, 2]."""
        torch = _torch()
        if self.fem_order != 1:
            _, x, bands = self._bubble_assemble(rhs_list)
            return x, self._tridiag_solve(bands, bands["load"], True, bc, True)
        if self.fem_solver == "flux" and self.convection is None:
            x, us = None, []
            for f, (u0, u1) in zip(rhs_list, bc):
                _, x, u, _ = self._fem(f, float(u0), float(u1))
                us.append(u)
            return x, torch.stack(us)
        _, x, xq, kw = self._fem_setup()
        dev = x.device
        load = torch.empty((len(rhs_list), x.numel()), dtype=torch.float64, device=dev)
        tabulated = [j for j, f in enumerate(rhs_list) if not isinstance(f, SinRHS)]
        bands = None
        for j, f in enumerate(rhs_list):
            if isinstance(f, SinRHS):           # its load keeps the bits of the in-kernel sin; the bands come along
                bands = ops.p1_assemble(x, self.nquad, rhs=(f.amp, f.omega), **kw)
                load[j].copy_(bands["load"])
        if tabulated:
            xq_host = xq.cpu().numpy()
            fq = [_to_dev(rhs_list[j](xq_host), dev) for j in tabulated]
            for j, t in zip(tabulated, fq):
                if t.numel() != xq.numel():
                    raise ValueError(f"rhs_list[{j}] must return one value per quadrature point "
                                     f"({list(xq.shape)}), got {list(t.shape)}")
            fq = torch.stack([t.reshape(xq.shape) for t in fq])
            if bands is None:                   # the bands do not depend on the right-hand side
                bands = ops.p1_assemble(x, self.nquad, rhs_quad=fq[0], **kw)
            loads = ops.p1_load_multi(x, fq, self.nquad)
            if len(tabulated) == len(rhs_list):
                load = loads
            else:
                load[torch.as_tensor(tabulated, device=dev)] = loads
        return x, self._tridiag_solve(bands, load, "b_quad" in kw, bc, True)

    def _pivot_solve(self, bands, load, end_values, multi):
        """The P1 solve of ``fem_solver="pivot"`` on the assembled bands -- symmetric (off) or
        not (sub, sup) -- with the configured ends; ``RuntimeError`` when the solve met a pivot that was zero or not
        finite.  Reading that count waits for the solve."""
        sub, sup = (bands["sub"], bands["sup"]) if "sub" in bands else (bands["off"], bands["off"])
        bnd = self._bnd
        kinds, kappa = ((ops.END_DIRICHLET,) * 2, (0.0, 0.0)) if bnd is None else (bnd.kinds, bnd.kappa)
        fn = ops.tridiag_pivot_solve_multi if multi else ops.tridiag_pivot_solve
        u, info = fn(bands["diag"], sub, sup, load, kinds, kappa, end_values, return_info=True)
        bad = int(info.item())
        if bad:
            raise RuntimeError(f"P1 system singular to working precision: the pivoting tridiagonal solve met {bad} "
                               "pivot(s) that were zero or not finite; the problem has no unique discrete solution "
                               "on this mesh (change the mesh, the coefficients or the boundary conditions)")
        return u

    def _convection_quad(self, eq, x, xq):
        """b at the quadrature points ``xq`` [ne, nquad], after the check that makes the unpivoted, unstabilised solve safe:
        the cell Peclet number |bbar_e| h_e / (2 abar_e) <= 1 on every element (bbar, abar: quadrature means).
        Host arithmetic on the tabulated values, before the assembly is launched.  ``fem_solver="pivot"`` tabulates b
        and skips the check: above Peclet 1 it returns the Galerkin solution, oscillations included."""
        xq = xq.cpu().numpy()
        w = 0.5 * np.polynomial.legendre.leggauss(int(self.nquad))[1]
        bq = np.array(np.broadcast_to(np.asarray(eq.b(xq), dtype=np.float64), xq.shape))     # (a writable copy)
        if self.fem_solver == "pivot":
            return _to_dev(bq, x.device)
        abar = 1.0 if eq.a is None else np.broadcast_to(np.asarray(eq.a(xq), dtype=np.float64), xq.shape) @ w
        nodes = x.cpu().numpy()
        pe = np.abs(bq @ w) * np.diff(nodes) / (2.0 * abar)
        worst = int(np.argmax(pe)) if np.all(np.isfinite(pe)) else int(np.argmax(~np.isfinite(pe)))
        if not pe[worst] <= 1.0:
            raise ValueError(f"cell Peclet number |b| h / (2 a) = {pe[worst]:.3g} > 1 on element {worst} "
                             f"[{nodes[worst]:.6g}, {nodes[worst + 1]:.6g}]: the P1 solve of the convection term has "
                             "no stabilisation and does not pivot; refine the mesh there")
        return _to_dev(bq, x.device)

    # ---- Dual.py:110-137 --------------------------------------------------------------
    def solve_fem(self, *, u_init=None, tol=None, max_iter=None):
        """P1 finite-element solve: mesh, element-local assembly, Dirichlet on all
        boundary dofs, tridiagonal solve, nodal values.  Returns ``(u_fem, basis)``
        like the reference (``basis`` is scikit-fem shaped, see ``mesh.py``).

        With ``nonlinear=`` the solve is a damped Newton iteration from ``u_init`` (a callable
        sampled at the nodes; ``None``: zeros; Dirichlet ends start at their values) until
        |u_new - u|_inf <= ``tol`` max(1, |u_new|_inf) (default 1e-12), at most ``max_iter`` (default 30) linear
        solves; ``RuntimeError`` when it does not converge or meets a non-finite value; the report is ``self.newton``.
        Without ``nonlinear`` the three keywords must be left alone."""
        if self.nonlinear is None:
            if u_init is not None or tol is not None or max_iter is not None:
                raise ValueError("u_init, tol and max_iter belong to the Newton iteration of nonlinear=")
            m, x, u, bands = self._fem(self.rhs, *self._gd_bc()[1])
        else:
            m, x, u, bands = self._solve_fem_newton(u_init, 1e-12 if tol is None else tol,
                                                    30 if max_iter is None else max_iter)
        basis = P1Basis(m)
        self.bands = bands
        self._x_dev, self._u_dev = x, u
        u_fem = u.cpu().numpy()
        self.fem_nodes = m.p[0]
        self.fem_values = u_fem.copy()
        return u_fem, basis

    # ---- semilinear problems (no reference counterpart) ----------------------------------
    def _check_nonlinear(self, what=None):
        """The parsed ``nonlinear`` after the checks that need no device; ``what``: a method that has no semilinear
        form (``ValueError``)."""
        if what is not None:
            if self.nonlinear is not None:
                raise ValueError(f"{what} has no semilinear form: nonlinear= is solved by solve_fem() / solve() only")
            return None
        nl = _Nonlinear(self.nonlinear)
        if self.fem_solver == "flux" or self._periodic or self.solver_id != ops.SOLVER_PRIMAL:      # (public attributes)
            raise ValueError("nonlinear needs fem_solver='bands' or 'pivot', Dirichlet or Robin ends and "
                             "solver=ops.SOLVER_PRIMAL")
        if self.element_lists or self.element_degrees is not None:
            raise ValueError("nonlinear has no element_lists / element_degrees: the linearised tables are written for "
                             "one degree")
        return nl

    def _nl_host_points(self, nodes):
        """The host's copy of the points the q_k are checked at before any device call: the Gauss points of the
        assembly and the collocation points."""
        xi = 0.5 * (1.0 + np.polynomial.legendre.leggauss(int(self.nquad))[0])
        xq = nodes[:-1, None] + np.diff(nodes)[:, None] * xi[None, :]
        return xq, np.linspace(nodes[:-1], nodes[1:], int(self.n_colloc), axis=-1)

    def _solve_fem_newton(self, u_init, tol, max_iter, max_halvings=8):
        """(mesh, x device, u device, bands of the last Newton step) of the damped Newton iteration.

        Once: the bands K of a, b, c by the existing assembly, and f, c and the q_k at the quadrature points.  One
        iteration: ``ops.nl_linearize`` -> ONE ``ops.p1_assemble`` with c_quad = c_eff and rhs_quad = f_eff -> the
        solve of :meth:`_p1_solve` gives u_new.  The merit function |R(v)|_inf, R(v) = K v + G(v) - F, costs
        ``ops.nl_linearize`` (f_res only) -> ``ops.p1_load_multi`` -> ``ops.nl_residual``, and reading its four
        numbers is the loop's synchronisation.  The stop test |u_new - u| <= tol max(1, |u_new|) comes first; otherwise
        lambda = 1, 1/2, ... (at most ``max_halvings`` halvings) until |R(u + lambda d)| <= (1 - 1e-4 lambda) |R(u)|,
        else the tried lambda with the smallest residual."""
        self._check_fem_order("nonlinear=")
        torch = _torch()
        nl = self._check_nonlinear()
        if not (float(tol) > 0.0) or not math.isfinite(float(tol)):
            raise ValueError(f"tol must be finite and > 0, got {tol!r}")
        if isinstance(max_iter, bool) or int(max_iter) != max_iter or int(max_iter) < 1:
            raise ValueError(f"max_iter must be an integer >= 1, got {max_iter!r}")
        if u_init is not None and not callable(u_init):
            raise ValueError("u_init must be a callable u_init(x) or None")
        tol, max_iter = float(tol), int(max_iter)
        m = self._default_mesh() if self.mesh is None else self.mesh
        nodes = np.asarray(m.nodes, dtype=np.float64)
        ne = nodes.size - 1
        xq_host, xc_host = self._nl_host_points(nodes)
        nl.host_tables(xq_host, "quadrature")
        if int(self.n_colloc) >= 2:
            nl.host_tables(xc_host, "collocation")
        u0, u1 = self._gd_bc()[1]
        bnd = self._bnd
        kinds, kappa = ((ops.END_DIRICHLET,) * 2, (0.0, 0.0)) if bnd is None else (tuple(bnd.kinds), tuple(bnd.kappa))
        start = np.zeros(ne + 1) if u_init is None else \
            np.array(np.broadcast_to(np.asarray(u_init(nodes), dtype=np.float64), nodes.shape))
        for i, (end, g) in enumerate(((0, u0), (-1, u1))):
            if kinds[i] == ops.END_DIRICHLET:
                start[end] = g
        if not np.all(np.isfinite(start)):
            raise ValueError("u_init is not finite at a node")
        # ---- the device from here on
        _, x, xq, kw = self._fem_setup()
        dev = x.device
        conv = "b_quad" in kw
        eq = self._eq
        fq = _tabulate(eq.f, xq)
        cq = kw.get("c_quad")
        qq = nl.tables(xq, "quadrature")
        zq = torch.zeros_like(xq)
        K = ops.p1_assemble(x, self.nquad, rhs_quad=zq, **kw)
        ksub, ksup = (K["sub"], K["sup"]) if conv else (K["off"], K["off"])
        t = ops.quad_points(_to_dev([0.0, 1.0], dev), self.nquad)[0].contiguous()     # the rule's points on [0, 1]
        ends = _to_dev([u0, u1], dev)
        u = _to_dev(start, dev)
        c_eff, f_eff, f_res = (torch.empty_like(xq) for _ in range(3))
        step_kw = {k: v for k, v in kw.items() if k != "c_quad"}
        bands = None
        load = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
        out4 = torch.empty(4, dtype=torch.float64, device=dev)
        trial = torch.empty_like(u)
        work = ops._scratch(None, ops._capi.load().lssvr_nl_residual_work_bytes(ne), dev)

        def merit(v, v_new):
            """(|R(v)|, |v_new - v|, |v_new|) by one read of out4; ``RuntimeError`` at a non-finite entry."""
            ops.nl_linearize(v, t, nl.kind, qq, fq, c_tab=cq, c_eff=None, f_eff=None, f_res=f_res)
            ops.p1_load_multi(x, f_res.unsqueeze(0), self.nquad, out=load)
            ops.nl_residual(K["diag"], ksub, ksup, load[0], v, v_new, kinds, kappa, ends, out4=out4, work=work)
            r, du, un, bad = (float(w) for w in out4.cpu().numpy())
            if bad:
                raise RuntimeError(f"the Newton iteration met {int(bad)} non-finite value(s) in the residual or the "
                                   f"iterate; so far: {rep}")
            return r, du, un

        rep = self.newton = NewtonReport()
        for it in range(1, max_iter + 1):
            ops.nl_linearize(u, t, nl.kind, qq, fq, c_tab=cq, c_eff=c_eff, f_eff=f_eff, f_res=None)
            if self.fem_solver != "pivot" and bool((c_eff < 0).any().item()):
                raise ValueError(f"c + g_u is negative at a quadrature point in Newton iteration {it}: the tridiagonal "
                                 "solve does not pivot and assumes an SPD matrix; use fem_solver=\"pivot\"")
            bands = ops.p1_assemble(x, self.nquad, rhs_quad=f_eff, c_quad=c_eff, out=bands, **step_kw)
            u_new = self._p1_solve(bands, conv, u0, u1)
            r0, du, un = merit(u, u_new)
            rep.iterations = it
            rep.residuals.append(r0)
            rep.steps.append(du)
            if du <= tol * max(1.0, un):
                u = u_new
                rep.lambdas.append(1.0)
                rep.converged = True
                break
            lam, tried = 1.0, []
            for _ in range(int(max_halvings) + 1):
                v = u_new if lam == 1.0 else ops.nl_step(u, u_new, lam, out=trial)
                rv = merit(v, v)[0]
                tried.append((rv, lam))
                if rv <= (1.0 - 1e-4 * lam) * r0:
                    break
                lam *= 0.5
            else:
                rv, lam = min(tried, key=lambda p: p[0])
                v = u_new if lam == 1.0 else ops.nl_step(u, u_new, lam, out=trial)
            u = v.clone()
            rep.lambdas.append(lam)
        if not rep.converged:
            raise RuntimeError(f"the Newton iteration did not converge in {max_iter} iteration(s) to tol = {tol:g}: "
                               f"{rep}")
        return m, x, u, bands

    def _nl_tables(self, pts, what, t_local, point_major, u):
        """(a, a' - b, f_eff, c_eff) at the device points ``pts`` [ne, k] with the local coordinates ``t_local`` [k]:
        the tables of the LINEAR problem that the enhancement and the indicator see, ONE ``ops.nl_linearize`` around
        the P1 interpolant of the nodal values ``u``."""
        nl = self._check_nonlinear()
        ta, tda, tf, tc = self._eq.tables(pts, point_major)
        lin = ops.nl_linearize(u, t_local, nl.kind, nl.tables(pts, what, point_major), tf, c_tab=tc,
                               point_major=point_major)
        return ta, tda, lin["f_eff"], lin["c_eff"]

    # ---- one degree per element (no reference counterpart: Dual.py:101 has one lssvr_M) ----
    def _check_hp(self, what):
        if self.element_lists:
            # every operator and boundary kind: the Poisson rows run through lssvr_enhance_subset
            # (_enhance_by_degree), coefficients, reaction and convection through the element lists of the table
            # kernels (_enhance_by_degree_lists); both are primal solves
            if self.solver_id != ops.SOLVER_PRIMAL:
                raise ValueError(f"{what} needs solver=ops.SOLVER_PRIMAL")
            return
        if self._periodic:
            # a periodic problem needs a reaction term, which lssvr_enhance_subset does not hold: the degree groups
            # run through the table kernels instead (_enhance_by_degree_tables), with any coefficients
            if self.solver_id != ops.SOLVER_PRIMAL:
                raise ValueError(f"{what} needs solver=ops.SOLVER_PRIMAL")
            return
        if self.coef is not None or self.reaction is not None or self.convection is not None:
            raise ValueError(f"{what} needs the Poisson rows (no coef, no reaction, no convection): "
                             "lssvr_enhance_subset holds those only (element_lists=True runs the others through "
                             "the element lists of the table kernels)")
        if self.solver_id != ops.SOLVER_PRIMAL:
            raise ValueError(f"{what} needs solver=ops.SOLVER_PRIMAL")

    def _check_degrees(self, ne):
        """``element_degrees`` as an int64 host array: one degree in 2 .. 33 per element."""
        self._check_hp("element_degrees")
        deg = np.asarray(self.element_degrees)
        if deg.shape != (ne,) or not np.issubdtype(deg.dtype, np.integer):
            raise ValueError(f"element_degrees must hold one integer per element ({ne}), got shape {deg.shape} "
                             f"of {deg.dtype}")
        if deg.min() < ops.MIN_DEGREE or deg.max() > ops.MAX_DEGREE:
            raise ValueError(f"element_degrees must lie in [2, 33], got [{deg.min()}, {deg.max()}]")
        return deg.astype(np.int64)

    def group_colloc(self, M):
        """Collocation points of the elements of degree ``M`` when ``element_degrees`` is set:
        max(n_colloc, 2 M) -- n >= 2 (M - 2) keeps a raised element in the parity-solve regime and away from
        the near-square one."""
        return max(int(self.n_colloc), 2 * int(M))

    def _enhance_by_degree(self, x, u, degrees, gamma, gd, bc, **shard):
        """Group the elements by degree on the device, read the 35 offsets back once, one ``enhance_subset`` per
        non-empty degree into a zeroed W[ne, max M]."""
        torch = _torch()
        ne = degrees.size
        ids, offsets = ops.group_by_degree(torch.as_tensor(degrees.astype(np.int32), device=x.device))
        off = offsets.cpu().numpy()
        W = torch.zeros((ne, int(degrees.max())), dtype=torch.float64, device=x.device)
        st = torch.zeros((ne,), dtype=torch.int32, device=x.device)
        for Mg in range(ops.MIN_DEGREE, ops.MAX_DEGREE + 1):
            sub = ids[off[Mg]:off[Mg + 1]]
            if sub.numel() == 0:
                continue
            ng = self.group_colloc(Mg)
            # (a callable f is tabulated at this group's collocation points, np.linspace per element)
            kw = _rhs_mode(self.rhs, lambda: ops.colloc_points(x, ng)[sub])
            ops.enhance_subset(x, u, Mg, gamma, ng, W, elem_ids=sub, global_domain=gd, bc=bc, status=st, **kw,
                               **shard)
        return W, st

    def _enhance_by_degree_tables(self, x, u, degrees, gamma, gd, bc, eq=None, **shard):
        """:meth:`_enhance_by_degree` for rows that ``lssvr_enhance_subset`` does not hold, without element lists
        (``boundary="periodic"`` with ``element_lists=False``): every degree that occurs is one ``ops.enhance_varcoef``
        over the whole mesh at that degree's collocation count, and the rows of its own elements are copied into a
        zeroed W[ne, max M].  The cost is one whole-mesh launch per distinct degree; :meth:`_enhance_by_degree_lists`
        removes that factor.  ``eq``: the equation whose rows are fitted (default: the solver's own)."""
        torch = _torch()
        eq = self._eq if eq is None else eq
        W = torch.zeros((degrees.size, int(degrees.max())), dtype=torch.float64, device=x.device)
        st = torch.zeros((degrees.size,), dtype=torch.int32, device=x.device)
        for Mg in np.unique(degrees):
            Mg = int(Mg)
            ng, pm = self.group_colloc(Mg), _point_major(Mg)
            ta, tda, tf, tc = eq.tables(ops.colloc_points(x, ng), pm)
            Wg, sg = ops.enhance_varcoef(x, u, Mg, gamma, ng, ta, tda, tf, global_domain=gd, bc=bc, point_major=pm,
                                         c_values=tc, **shard)
            ids = torch.as_tensor(np.nonzero(degrees == Mg)[0], device=x.device)
            W[ids, :Mg] = Wg[ids]
            st[ids] = sg[ids]
        return W, st

    def _enhance_by_degree_lists(self, x, u, degrees, gamma, gd, bc, eq=None, **shard):
        """:meth:`_enhance_by_degree` for rows that ``lssvr_enhance_subset`` does not hold (coefficients, reaction,
        convection; every ``boundary``; ``element_lists=True``): the same grouping, and per non-empty degree the
        collocation points of its own elements (``ops.colloc_points_subset``), the tables on those points, and one
        ``ops.enhance_varcoef_subset`` into a zeroed W[ne, max M].  Every element is tabulated and solved once.
        ``eq``: the equation whose rows are fitted (default: the solver's own)."""
        torch = _torch()
        eq = self._eq if eq is None else eq
        ne = degrees.size
        ids, offsets = ops.group_by_degree(torch.as_tensor(degrees.astype(np.int32), device=x.device))
        off = offsets.cpu().numpy()
        W = torch.zeros((ne, int(degrees.max())), dtype=torch.float64, device=x.device)
        st = torch.zeros((ne,), dtype=torch.int32, device=x.device)
        for Mg in range(ops.MIN_DEGREE, ops.MAX_DEGREE + 1):
            sub = ids[off[Mg]:off[Mg + 1]]
            if sub.numel() == 0:
                continue
            ng, pm = self.group_colloc(Mg), _point_major(Mg)
            ta, tda, tf, tc = eq.tables(ops.colloc_points_subset(x, sub, ng), pm)
            ops.enhance_varcoef_subset(x, u, Mg, gamma, ng, W, ta, tda, tf, elem_ids=sub, c_values=tc,
                                       point_major=pm, global_domain=gd, bc=bc, status=st, **shard)
        return W, st

    # ---- Dual.py:139-169 --------------------------------------------------------------
    def solve_lssvr_subproblems(self):
        """Solve LSSVR with the primal method in each element (one kernel launch)."""
        if self.fem_nodes is None or self.fem_values is None:
            raise RuntimeError("fem_nodes / fem_values are not set: call solve_fem() first "
                               "or assign them (Dual.py:139 reads only these attributes)")
        dev = _device(self.device)
        nodes = np.asarray(self.fem_nodes, dtype=np.float64)
        x = self._x_dev
        if x is None or x.numel() != nodes.size or not np.array_equal(x.cpu().numpy(), nodes):
            x = _to_dev(nodes, dev)
        u = _to_dev(self.fem_values, dev)       # the attribute is authoritative (may be user-set)
        gd, bc = self._gd_bc()
        M, gamma, n = int(self.lssvr_M), float(self.lssvr_gamma), int(self.n_colloc)
        pm = _point_major(M)
        eq = self._eq
        # at a Neumann or Robin end the end element takes the FEM nodal value as its constraint row, as at every
        # interior node: the enhanced solution meets the flux condition to the accuracy of the element fit only
        bnd = self._bnd
        if bnd is not None and self.solver_id == ops.SOLVER_SHARED:
            raise ValueError("a Neumann or Robin end needs a per-element solver, not ops.SOLVER_SHARED")
        if self._periodic and self.solver_id == ops.SOLVER_SHARED:
            raise ValueError("boundary='periodic' needs a per-element solver, not ops.SOLVER_SHARED")
        shard = self._shard(nodes.size - 1)
        degrees = None
        if self.nonlinear is not None:
            # the linear problem around the P1 interpolant of u: c_eff = c + g_u, f_eff = f - g + g_u u_h
            self._check_nonlinear()
            if n < 2 or n > ops.NL_MAX_POINTS:
                raise ValueError(f"nonlinear needs 2 <= n_colloc <= {ops.NL_MAX_POINTS}, got {n}")
            t = _torch().arange(n, dtype=_torch().float64, device=dev) / float(n - 1)
            ta, tda, tf, tc = self._nl_tables(ops.colloc_points(x, n), "collocation", t, pm, u)
            W, st = ops.enhance_varcoef(x, u, M, gamma, n, ta, tda, tf, global_domain=gd, bc=bc, point_major=pm,
                                        c_values=tc, **shard)
        elif self.element_degrees is not None:
            degrees = self._check_degrees(nodes.size - 1)
            by_degree = self._enhance_by_degree_tables if self._periodic else self._enhance_by_degree
            if self.element_lists and not eq.poisson:
                by_degree = self._enhance_by_degree_lists
            W, st = by_degree(x, u, degrees, gamma, gd, bc, **shard)
        elif eq.poisson:
            kw = _rhs_mode(eq.f, lambda: ops.colloc_points(x, n), pm)
            W, st = _enhance(x, u, M, gamma, n, global_domain=gd, bc=bc, solver=self.solver_id, **kw, **shard)
        else:
            # the varcoef / reaction kernels take tables only (a SinRHS too)
            ta, tda, tf, tc = eq.tables(ops.colloc_points(x, n), pm)
            W, st = ops.enhance_varcoef(x, u, M, gamma, n, ta, tda, tf, global_domain=gd, bc=bc, point_major=pm,
                                        c_values=tc, **shard)
        self.enhanced = EnhancedSolution(x, W, st)
        if degrees is not None:
            self.enhanced.degrees = degrees
        self._report_fallbacks()
        self.lssvr_functions = _ElementFunctions(nodes, W)

    def _report_fallbacks(self):
        nbad = self.enhanced.n_fallback
        if nbad:
            bad = np.nonzero(self.enhanced.status.cpu().numpy())[0]
            for i in bad[:10]:
                print(f"Error in element {i+1}: factorisation breakdown, linear interpolant used")
            if nbad > 10:
                print(f"... and {nbad - 10} more elements")

    # ---- Dual.py:171-174 --------------------------------------------------------------
    def solve(self, **newton):
        """Complete solution: FEM + LSSVR.  ``newton``: the keywords of :meth:`solve_fem` (``nonlinear=`` only)."""
        self.solve_fem(**newton)
        self.solve_lssvr_subproblems()

    def solve_many(self, rhs_list, bc=None):
        """Several load cases on this solver's mesh and operator: for every right-hand side of ``rhs_list`` the P1
        assembly and Dirichlet solve (``coef``, ``reaction``, ``nquad`` and ``fem_solver`` as configured), then ONE
        ``ops.enhance_multi`` over all cases -- the element systems are formed and factored once, not once per case.
        ``bc``: ``None`` (the end values ``solve()`` uses) or one ``(left, right)`` pair per case -- at a Neumann or
        Robin end of ``boundary`` the entry is that case's g; the kinds and kappa belong to the matrix and are shared
        (``boundary="periodic"`` has no end values: ``bc`` must be ``None``).  Returns a list of :class:`EnhancedSolution`, one per case; ``rhs``, ``fem_values``, ``enhanced`` and
        the other attributes of the solver are left as they are.  Without ``coef`` the tables hold a = 1, a' = 0."""
        self._check_nonlinear("solve_many")
        return self._solve_many(rhs_list, bc)[0]

    def _solve_many(self, rhs_list, bc):
        """:meth:`solve_many` -> (its list, x device, U device [ncases, ne+1] the P1 nodal values of the cases)."""
        torch = _torch()
        rhs_list = list(rhs_list)
        if not rhs_list or not all(callable(f) for f in rhs_list):
            raise ValueError("rhs_list must be a non-empty sequence of callables")
        if self.solver_id != ops.SOLVER_PRIMAL:
            raise ValueError("solve_many needs solver=ops.SOLVER_PRIMAL")
        if self._periodic and bc is not None:
            raise ValueError("boundary='periodic' has no end values: bc must be None")
        gd, bc0 = self._gd_bc()
        if bc is None:
            bc = [bc0] * len(rhs_list)
        bc = np.asarray(bc, dtype=np.float64)
        if bc.shape != (len(rhs_list), 2):
            raise ValueError(f"bc must hold one (left, right) pair per case: {(len(rhs_list), 2)}, got {bc.shape}")
        M, gamma, n = int(self.lssvr_M), float(self.lssvr_gamma), int(self.n_colloc)
        pm = int(M) <= 16                    # the lane kernel of lssvr_enhance_multi reads point-major tables
        x, U = self._fem_many(rhs_list, bc)
        pts = ops.colloc_points(x, n)
        ta, tda, _, tc = _Equation(_zero, self.coef, self.reaction, self.convection).tables(pts, pm)
        tf = torch.stack([_tabulate(f, pts, pm) for f in rhs_list])
        W, st = ops.enhance_multi(x, U, M, gamma, n, ta, tda, tf, c_values=tc,
                                  bc=_to_dev(bc, x.device), point_major=pm, global_domain=gd,
                                  **self._shard(x.numel() - 1))
        return [EnhancedSolution(x, W[j], st[j]) for j in range(len(rhs_list))], x, U

    # ---- eigenproblems (no reference counterpart) ------------------------
    def _check_eigen(self, k, sigma, weight, tol, max_iter, check_every):
        """What :meth:`solve_eigen` does not cover, on the host and before any device call -> (mesh, nodes, kinds,
        kappa, number of unknowns)."""
        if self.convection is not None:
            raise ValueError("solve_eigen has no convection term: the pencil of -(a u')' + b u' + c u = lambda rho u "
                             "is not symmetric, and the Rayleigh-Ritz step and the Sturm count need a symmetric one")
        if self._periodic:
            raise ValueError("solve_eigen has no boundary='periodic': a shift inside the spectrum needs the pivoting "
                             "solve, which has no cyclic form")
        if self.fem_solver == "flux":
            raise ValueError("solve_eigen needs fem_solver='bands' or 'pivot': the flux solve factors A = D^T K D, "
                             "which the mass matrix of the shift breaks")
        if self.solver_id != ops.SOLVER_PRIMAL:
            raise ValueError("solve_eigen needs solver=ops.SOLVER_PRIMAL: the modes are enhanced through the "
                             "reaction rows, which have a primal solve only")
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= 6:
            raise ValueError(f"k must be an integer in 1 .. 6 (the block of k + 2 vectors is one pass of the "
                             f"multi-RHS solvers), got {k!r}")
        if not math.isfinite(float(sigma)):
            raise ValueError(f"sigma must be finite, got {sigma!r}")
        if weight is not None and not callable(weight):
            raise ValueError("weight must be a callable rho(x) or None")
        if not (float(tol) > 0.0) or int(max_iter) < 1 or int(check_every) < 1:
            raise ValueError("tol must be > 0, max_iter and check_every >= 1")
        if any(float(v) != 0.0 for v in self._gd_bc()[1]):
            raise ValueError(f"solve_eigen needs homogeneous end data (u = 0 or a du/dn + kappa u = 0), got the end "
                             f"values {self._gd_bc()[1]!r}")
        bnd = self._bnd
        kinds, kappa = ((ops.END_DIRICHLET,) * 2, (0.0, 0.0)) if bnd is None else (tuple(bnd.kinds), tuple(bnd.kappa))
        m = self._default_mesh() if self.mesh is None else self.mesh
        nodes = np.asarray(m.nodes, dtype=np.float64)
        unknowns = nodes.size - 2 + sum(1 for kd in kinds if kd == ops.END_ROBIN)
        if int(k) > unknowns:
            raise ValueError(f"k = {k} > {unknowns}, the number of unknowns of the P1 system")
        xi = np.polynomial.legendre.leggauss(int(self.nquad))[0]
        xq = 0.5 * (nodes[:-1] + nodes[1:])[:, None] + 0.5 * np.diff(nodes)[:, None] * xi[None, :]
        rq = np.broadcast_to(np.asarray((_one if weight is None else weight)(xq), dtype=np.float64), xq.shape)
        if not np.all(rq > 0.0):
            raise ValueError("weight must be positive at every quadrature point (rho > 0): M would not be positive "
                             "definite")
        if self.element_degrees is not None:
            deg = np.asarray(self.element_degrees)
            if deg.shape != (nodes.size - 1,) or not np.issubdtype(deg.dtype, np.integer) or \
                    deg.min() < ops.MIN_DEGREE or deg.max() > ops.MAX_DEGREE:
                raise ValueError(f"element_degrees must hold one integer in [2, 33] per element ({nodes.size - 1})")
        return m, nodes, kinds, kappa, unknowns

    def solve_eigen(self, k=1, sigma=0.0, weight=None, tol=1e-12, max_iter=200, check_every=4, enhance=True, nq=None):
        """The ``k`` <= 6 eigenvalues nearest ``sigma`` of -(a u')' + c u = lambda rho u with the solver's ``mesh``,
        ``coef``, ``reaction`` and ``boundary`` (Dirichlet, Neumann or Robin ends with zero data), ``weight`` = rho (a
        callable, ``None``: 1); ``rhs`` is not read.  Block inverse iteration with the fixed shift and a Rayleigh-Ritz
        step on the device: per iteration one multi-RHS solve of (K - sigma M) Z = Y -- the
        unpivoted solve when c - sigma rho >= 0 at every quadrature point, else the pivoting one --, ``ops.eig_apply``,
        ``ops.eig_ritz`` and ``ops.eig_rotate``; theta, the residuals and the info words are read back every
        ``check_every`` iterations.  It stops when |K x_j - theta_j M x_j|_2 <= tol |K|_max |x_j|_2 for the first k
        columns, or at ``max_iter``.  A Sturm count then certifies that the k values are consecutive and gives their
        positions in the spectrum (``RuntimeError`` with the counts otherwise).  With ``enhance`` every mode is fitted
        per element by the reaction rows with the table c - theta_j rho (``lssvr_M``, ``n_colloc``, ``lssvr_gamma``,
        ``element_degrees``), and its Rayleigh quotient, by ``nq``-point Gauss, is the enhanced eigenvalue.  Returns
        an :class:`EigenSolution`."""
        self._check_fem_order("solve_eigen")
        self._check_nonlinear("solve_eigen")
        torch = _torch()
        m, nodes, kinds, kappa, unknowns = self._check_eigen(k, sigma, weight, tol, max_iter, check_every)
        k, sigma, ne = int(k), float(sigma), nodes.size - 1
        rho = _one if weight is None else weight
        eq = self._eq
        dev = _device(self.device)
        x = _to_dev(nodes, dev)
        xq = ops.quad_points(x, self.nquad)
        zq = torch.zeros_like(xq)
        aq = None if eq.a is None else _tabulate(eq.a, xq)
        cq = zq if eq.c is None else _tabulate(eq.c, xq)
        rq = _tabulate(rho, xq)
        sq = cq - sigma * rq
        K = ops.p1_assemble(x, self.nquad, rhs_quad=zq, a_quad=aq, c_quad=cq)
        Mb = ops.p1_assemble(x, self.nquad, rhs_quad=zq, a_quad=zq, c_quad=rq)
        S = ops.p1_assemble(x, self.nquad, rhs_quad=zq, a_quad=aq, c_quad=sq)
        # one read for the sizes the host needs: the sign of c - sigma rho, |K|_max, |M off|_max and M's Gershgorin floor
        md, mo = Mb["diag"], Mb["off"]
        lo, hi = (0 if kinds[0] == ops.END_ROBIN else 1), (ne + 1 if kinds[1] == ops.END_ROBIN else ne)
        row = md[lo:hi].clone()
        row[1:] -= mo[lo:hi - 1].abs()
        row[:-1] -= mo[lo:hi - 1].abs()
        smin, smax, kmax, komax, momax, mmin = (float(v) for v in torch.stack(
            [sq.min(), sq.max(), torch.maximum(K["diag"].abs().max() + max(kappa), K["off"].abs().max()),
             K["off"].abs().max(), mo.abs().max(), row.min()]).cpu())
        pure_neumann = kinds == (ops.END_ROBIN,) * 2 and kappa[0] + kappa[1] == 0.0
        pivot = self.fem_solver == "pivot" or smin < 0.0 or (pure_neumann and smax == 0.0)
        nb = min(ops.EIG_MAX_BLOCK, k + 2, unknowns)
        y0 = np.zeros((nb, ne + 1))
        y0[:, lo:hi] = np.random.default_rng(0).standard_normal((nb, hi - lo))
        Y = _to_dev(y0, dev)
        Z, X, MZ, KZ = (torch.empty_like(Y) for _ in range(4))
        gram = torch.empty((2, nb, nb), dtype=torch.float64, device=dev)
        theta = torch.empty(nb, dtype=torch.float64, device=dev)
        Q = torch.empty((nb, nb), dtype=torch.float64, device=dev)
        res2 = torch.empty((2, nb), dtype=torch.float64, device=dev)
        rinfo = torch.zeros(1, dtype=torch.int32, device=dev)
        pinfo = rinfo
        swork = ops.tridiag_work(Y, ne, nb, "pivot", "bc")
        ework = ops._scratch(None, ops._capi.load().lssvr_eig_work_bytes(ne, nb), dev)
        it, converged, th, res, xn = 0, False, None, None, None
        while it < int(max_iter) and not converged:
            it += 1
            if pivot:
                _, pinfo = ops.tridiag_pivot_solve_multi(S["diag"], S["off"], S["off"], Y, kinds, kappa, out=Z,
                                                         work=swork, return_info=True)
            else:
                ops.tridiag_bc_solve_multi(S["diag"], S["off"], Y, kinds, kappa, out=Z, work=swork)
            ops.eig_apply(K["diag"], K["off"], md, mo, Z, kinds, kappa, MZ=MZ, KZ=KZ, gram=gram, work=ework)
            ops.eig_ritz(gram, sigma, theta=theta, Q=Q, info=rinfo)
            ops.eig_rotate(Z, MZ, KZ, Q, theta, kinds, X=X, Y=Y, res2=res2, work=ework)
            if it % int(check_every) and it != int(max_iter):
                continue
            host = _read_back(theta=theta, res2=res2, pinfo=pinfo, rinfo=rinfo)                 # one small copy
            th, (res, xn) = host["theta"], np.sqrt(host["res2"])
            if pivot and host["pinfo"][0]:
                raise RuntimeError(f"K - sigma M is singular to working precision at sigma = {sigma!r}: the pivoting "
                                   f"solve met {int(host['pinfo'][0])} pivot(s) that were zero or not finite; sigma is "
                                   "an eigenvalue of the discrete problem, move it")
            if host["rinfo"][0]:
                raise RuntimeError(f"the block of iteration vectors lost {int(host['rinfo'][0])} column(s): their "
                                   "images under the shifted inverse are linearly dependent to working precision "
                                   "(sigma is too close to an eigenvalue for a block of this width)")
            if not all(np.all(np.isfinite(v)) for v in host.values()):
                raise RuntimeError("block inverse iteration produced non-finite values")
            converged = bool(np.all(res[:k] <= float(tol) * kmax * xn[:k]))
        index = None
        if converged:
            # the k values are consecutive eigenvalues: the Sturm counts just outside them differ by k
            eps = 2.0 ** -53
            floor = 64.0 * eps * kmax / mmin
            order = np.argsort(th[:k], kind="stable")
            t_lo, t_hi = th[order[0]], th[order[-1]]
            below = [t for t in th[k:] if t < t_lo]
            above = [t for t in th[k:] if t > t_hi]
            d_lo = max(0.5 * (t_lo - max(below)) if below else 0.0, res[order[0]] / math.sqrt(mmin), floor)
            d_hi = max(0.5 * (min(above) - t_hi) if above else 0.0, res[order[-1]] / math.sqrt(mmin), floor)
            shifts = _to_dev([t_lo - d_lo, t_hi + d_hi], dev)
            pivmin = np.finfo(np.float64).tiny * max(1.0, (komax + max(abs(t_lo - d_lo), abs(t_hi + d_hi)) * momax) ** 2)
            cnt = ops.eig_count(K["diag"], K["off"], md, mo, shifts, pivmin, kinds, kappa).cpu().numpy()
            if int(cnt[1]) - int(cnt[0]) != k:
                raise RuntimeError(f"solve_eigen found {k} value(s) in [{t_lo!r}, {t_hi!r}], but the Sturm counts "
                                   f"{int(cnt[0])} below {t_lo - d_lo!r} and {int(cnt[1])} below {t_hi + d_hi!r} "
                                   f"say the discrete problem has {int(cnt[1]) - int(cnt[0])} there")
            index = np.empty(k, dtype=np.int64)
            index[order] = int(cnt[0]) + np.arange(k)
        nodal = X[:k].cpu().numpy()
        values, modes = None, []
        if enhance:
            M, gamma, n = int(self.lssvr_M), float(self.lssvr_gamma), int(self.n_colloc)
            gd = (float(self.global_domain[0]), float(self.global_domain[1]))
            shard = self._shard(ne)
            degrees = None if self.element_degrees is None else np.asarray(self.element_degrees).astype(np.int64)
            nqe = max(M if degrees is None else int(degrees.max()), 8) if nq is None else int(nq)
            if not 1 <= nqe <= 32:
                raise ValueError(f"nq must be in [1, 32], got {nqe}")
            pts = ops.estimate_points(x, nqe)
            ta, tc, tr = (_tabulate(fn, pts, True) for fn in (_one if eq.a is None else eq.a,
                                                            _zero if eq.c is None else eq.c, rho))
            values = np.empty(k)
            for j in range(k):
                tj = float(th[j])
                c0 = _zero if eq.c is None else eq.c
                eqj = _Equation(_zero, self.coef, lambda t, tj=tj, c0=c0: np.asarray(c0(t), dtype=np.float64)
                                - tj * np.asarray(rho(t), dtype=np.float64), None)
                u = X[j].contiguous()
                if degrees is not None:
                    by_degree = self._enhance_by_degree_lists if self.element_lists else self._enhance_by_degree_tables
                    W, st = by_degree(x, u, degrees, gamma, gd, (0.0, 0.0), eq=eqj, **shard)
                else:
                    pm = _point_major(M)
                    ea, eda, ef, ec = eqj.tables(ops.colloc_points(x, n), pm)
                    W, st = ops.enhance_varcoef(x, u, M, gamma, n, ea, eda, ef, global_domain=gd, bc=(0.0, 0.0),
                                                point_major=pm, c_values=ec, **shard)
                modes.append(EnhancedSolution(x, W, st))
                out3 = ops.eig_rayleigh(x, W, nqe, ta, tc, tr, point_major=True, end_kinds=kinds, kappa=kappa,
                                        work=ework).cpu().numpy()
                values[j] = out3[0] / out3[1]
        return EigenSolution(th[:k].copy(), values, res[:k].copy(), index, it, converged, nodal, modes, sigma)

    # ---- time stepping: what solve_transient and solve_wave share (DESIGN.md sections 26, 28, 29) -------------
    def _check_time(self, me, u0, t_end, nsteps, weight, forcing, end_data, snapshots, enhance, damping=None,
                    phi0=False):
        """What the time loops (``me``: the method's name in the messages) do not cover and what their data must
        satisfy, whatever the rule in time; on the host and before any device call -> a namespace of nodes, kinds,
        kappa, dt, times, steps, u_init, end_data (the pair as given or defaulted), phi [nsteps, R] -- with ``phi0``
        [nsteps + 1, R]: a row for t = 0 first --, g [nsteps + 1, 2], quad, colloc.  Every callable is evaluated here,
        once per kind of point, and ``quad`` / ``colloc`` are its host tables, the ones the device is handed: a, c, rho
        [ne, nquad] and f [R, ne, nquad] at the Gauss points of the assembly; with ``enhance`` a, da, c, rho
        [ne, n_colloc] and f [R, ne, n_colloc] at np.linspace(x_e, x_e+1, n_colloc), the abscissae lssvr_colloc_points
        writes (else None).  ``damping``: one more coefficient d(x), tabulated as "d" in both.  ``nsteps=None`` (with
        ``phi0``) is the caller whose steps are not known beforehand, :meth:`solve_transient_adaptive`: t = 0 is the one
        time tabulated, dt is None, steps is empty and ``snapshots`` is not looked at; phi_fns / g_fns are the callables
        of t that it evaluates as it goes.  The parameters of the
        rule and the definiteness of its step matrix are the caller's: :meth:`_check_transient`,
        :meth:`_check_wave`."""
        if self.convection is not None:
            raise ValueError(f"{me} has no convection term: the step's matrix would need the non-symmetric "
                             "solve and a cell Peclet check per step size")
        if self._periodic:
            raise ValueError(f"{me} has no boundary='periodic': the time loop runs the solve with Dirichlet "
                             "or Robin ends")
        if self.fem_solver != "bands":
            raise ValueError(f"{me} needs fem_solver='bands': the step's matrix carries "
                             "a mass matrix (no flux solve) and is definite (no pivoting)")
        if self.element_degrees is not None:
            raise ValueError(f"{me} has no element_degrees: all snapshots are enhanced as cases of one "
                             "ops.enhance_multi, which has one degree")
        if self.solver_id != ops.SOLVER_PRIMAL:
            raise ValueError(f"{me} needs solver=ops.SOLVER_PRIMAL: the snapshots are enhanced through the "
                             "reaction rows, which have a primal solve only")
        if not callable(u0):
            raise ValueError("u0 must be a callable u0(x)")
        if weight is not None and not callable(weight):
            raise ValueError("weight must be a callable rho(x) or None")
        if damping is not None and not callable(damping):
            raise ValueError("damping must be a callable d(x) or None")
        if nsteps is not None and (isinstance(nsteps, bool) or int(nsteps) != nsteps or int(nsteps) < 1):
            raise ValueError(f"nsteps must be an integer >= 1, got {nsteps!r}")
        nsteps, t_end = None if nsteps is None else int(nsteps), float(t_end)
        if not (math.isfinite(t_end) and t_end > 0.0):
            raise ValueError(f"t_end must be finite and > 0, got {t_end!r}")
        forcing = [(1.0, self.rhs)] if forcing is None else list(forcing)
        if not all(isinstance(p, (tuple, list)) and len(p) == 2 and callable(p[1]) for p in forcing):
            raise ValueError("forcing must be a list of (phi, f_x) pairs: phi a callable of t or a constant, f_x a "
                             "callable of x")
        if not 1 <= len(forcing) <= ops.TS_MAX_TERMS:
            raise ValueError(f"forcing must hold 1 .. {ops.TS_MAX_TERMS} terms (R <= {ops.TS_MAX_TERMS}), got "
                             f"{len(forcing)}")
        if nsteps is None:
            steps = []
        else:
            snapshots = [nsteps] if snapshots is None else list(snapshots)
            if not snapshots or any(isinstance(s, bool) or int(s) != s or not 1 <= int(s) <= nsteps
                                    for s in snapshots):
                raise ValueError(f"snapshots must be step indices in 1 .. nsteps = {nsteps}, got {snapshots!r}")
            steps = sorted({int(s) for s in snapshots})
        bnd = self._bnd
        kinds, kappa = ((ops.END_DIRICHLET,) * 2, (0.0, 0.0)) if bnd is None else (tuple(bnd.kinds), tuple(bnd.kappa))
        if end_data is None:
            end_data = self._gd_bc()[1]
        if not isinstance(end_data, (tuple, list)) or len(end_data) != 2:
            raise ValueError("end_data must be a pair (g_left, g_right) of callables of t or constants")
        gfn = [v if callable(v) else (lambda t, v=float(v): v) for v in end_data]
        pfn = [p if callable(p) else (lambda t, p=float(p): p) for p, _ in forcing]
        m = self._default_mesh() if self.mesh is None else self.mesh
        nodes = np.asarray(m.nodes, dtype=np.float64)
        if nsteps is None:
            dt, times = None, np.zeros(1)
        else:
            dt = t_end / nsteps
            times = dt * np.arange(nsteps + 1)
        phi = np.array([[float(p(t)) for p in pfn] for t in (times if phi0 else times[1:])], dtype=np.float64)
        g = np.array([[float(v(t)) for v in gfn] for t in times], dtype=np.float64)
        # the data at the Gauss points of the assembly, a + h xi on [0, 1] as lssvr_quad_points has them, and at the
        # collocation points: finite, one value per point, rho > 0
        xi = 0.5 * (1.0 + np.polynomial.legendre.leggauss(int(self.nquad))[0])
        xq = nodes[:-1, None] + np.diff(nodes)[:, None] * xi[None, :]
        eq = self._eq
        fns = dict(a=_one if eq.a is None else eq.a, da=_zero if eq.da is None else eq.da,
                   c=_zero if eq.c is None else eq.c, rho=_one if weight is None else weight, d=damping)
        extra = () if damping is None else ("d",)

        def tables(pts, names, what):
            out = {}
            for nm, fn in (*((k, fns[k]) for k in names), *((r, f) for r, (_, f) in enumerate(forcing))):
                label = f"forcing[{nm}] f_x" if isinstance(nm, int) else {"a": "coef a", "da": "coef da",
                                                                          "c": "reaction", "rho": "weight",
                                                                          "d": "damping"}[nm]
                try:
                    t = np.broadcast_to(np.asarray(fn(pts), dtype=np.float64), pts.shape)
                except ValueError:
                    raise ValueError(f"{label} must return one value per point ({list(pts.shape)} at the {what} "
                                     "points) or a value that broadcasts to them") from None
                if not np.all(np.isfinite(t)):
                    raise ValueError(f"{label} is not finite at a {what} point")
                out[nm] = np.array(t)                       # (an own, writable copy: broadcast_to gives a view)
            out["f"] = np.stack([out.pop(r) for r in range(len(forcing))])
            return out

        quad = tables(xq, ("a", "c", "rho") + extra, "quadrature")
        colloc = None
        if enhance:
            n = int(self.n_colloc)
            if n < 2:
                raise ValueError(f"n_colloc must be >= 2, got {n}")
            colloc = tables(np.linspace(nodes[:-1], nodes[1:], n, axis=-1), ("a", "da", "c", "rho") + extra,
                            "collocation")
        u_init = np.array(np.broadcast_to(np.asarray(u0(nodes), dtype=np.float64), nodes.shape))
        for i, end in ((0, 0), (1, -1)):
            if kinds[i] == ops.END_DIRICHLET:
                u_init[end] = g[0, i]
        self._check_finite(("u0", u_init), ("end_data", g), ("forcing phi", phi))
        if not np.all(quad["rho"] > 0.0):
            raise ValueError("weight must be positive at every quadrature point (rho > 0): M would not be positive "
                             "definite")
        return types.SimpleNamespace(nodes=nodes, kinds=kinds, kappa=kappa, dt=dt, times=times, steps=steps,
                                     u_init=u_init, end_data=end_data, phi=phi, g=g, quad=quad, colloc=colloc,
                                     phi_fns=pfn, g_fns=gfn)

    @staticmethod
    def _check_finite(*named):
        for nm, t in named:
            if not np.all(np.isfinite(t)):
                raise ValueError(f"{nm} is not finite where it is tabulated")

    def _time_setup(self, p, enhance, matrices, per_snapshot=False, nbuf=3):
        """The device side that the time loops share, from the plan ``p`` of :meth:`_check_time` -> a namespace of
        dev, x, aq (None without ``coef``), bands {key: (diag, off)} and cq {key: the c table} of every
        (key, with a, host c table) of ``matrices`` -- each ONE ``ops.p1_assemble``, in the order given --, loads
        [R, ne+1], phi and g (every row of the plan's), pm, tab (with ``enhance``: the collocation tables a, da, c,
        rho, f and d, transposed when ``pm``), src [ns, table] (the right-hand sides of the snapshots' elliptic
        problems), U [nbuf, ne+1] with the start in row 0, S [ns, ne+1], b [1, ne+1], work (of the one-case "bc"
        solve) and snap {step: snapshot index}.

        ``pm``, the layout of the collocation tables, follows the kernel that reads them: ``ops.enhance_multi`` (all
        snapshots in one call: solve_transient, solve_wave) takes point-major tables for its lane kernel, M <= 16;
        ``ops.enhance_varcoef`` (``per_snapshot``: one call each, solve_transient with nonlinear=) when
        ``_point_major(M)``."""
        torch = _torch()
        ne, ns, q = p.nodes.size - 1, len(p.steps), p.quad
        dev = _device(self.device)
        x = _to_dev(p.nodes, dev)
        zq = torch.zeros((ne, int(self.nquad)), dtype=torch.float64, device=dev)
        aq = None if self.coef is None else _to_dev(q["a"], dev)
        bands, cq = {}, {}
        for key, with_a, c_host in matrices:
            cq[key] = _to_dev(c_host, dev)
            A = ops.p1_assemble(x, self.nquad, rhs_quad=zq, a_quad=aq if with_a else zq, c_quad=cq[key])
            bands[key] = (A["diag"], A["off"])
        loads = ops.p1_load_multi(x, _to_dev(q["f"], dev), self.nquad)
        pm = _point_major(self.lssvr_M) if per_snapshot else int(self.lssvr_M) <= 16
        tab = src = None
        if enhance:
            c = p.colloc
            tab = {k: _to_dev(np.transpose(c[k], (0, 2, 1)) if k == "f" else c[k].T, dev) if pm else _to_dev(c[k], dev)
                   for k in c}
            src = torch.empty((ns,) + tuple(tab["rho"].shape), dtype=torch.float64, device=dev)
        U = torch.empty((nbuf, ne + 1), dtype=torch.float64, device=dev)
        U[0].copy_(_to_dev(p.u_init, dev))
        S = torch.empty((ns, ne + 1), dtype=torch.float64, device=dev)
        b = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
        return types.SimpleNamespace(dev=dev, x=x, aq=aq, bands=bands, cq=cq, loads=loads, phi=_to_dev(p.phi, dev),
                                     g=_to_dev(p.g, dev), pm=pm, tab=tab, src=src, U=U, S=S, b=b,
                                     work=ops.tridiag_work(b, ne, 1, "bc"), snap={s: k for k, s in enumerate(p.steps)})

    def _enhance_snapshots(self, p, D, nodal):
        """The snapshots ``nodal`` [ns, ne+1] through ONE ``ops.enhance_multi``, on the tables and the right-hand sides
        ``D.src`` of :meth:`_time_setup`, with g at the snapshots' times as the end values -> ns EnhancedSolution."""
        torch = _torch()
        bc = D.g[torch.as_tensor(p.steps, device=D.dev)].contiguous()
        W, st = ops.enhance_multi(D.x, nodal, int(self.lssvr_M), float(self.lssvr_gamma), int(self.n_colloc),
                                  D.tab["a"], D.tab["da"], D.src, c_values=D.tab["c"], bc=bc, point_major=D.pm,
                                  global_domain=(float(self.global_domain[0]), float(self.global_domain[1])),
                                  **self._shard(p.nodes.size - 1))
        return [EnhancedSolution(D.x, W[k], st[k]) for k in range(len(p.steps))]

    # ---- transient problems (no reference counterpart; DESIGN.md sections 26 and 28) ------------------------------
    def _check_transient(self, u0, t_end, nsteps, scheme, weight, forcing, end_data, snapshots, enhance):
        """:meth:`_check_time` for :meth:`solve_transient`, and what belongs to BDF: the scheme's name, and
        c + rho / dt >= 0 at the quadrature points."""
        p = self._check_time("solve_transient", u0, t_end, nsteps, weight, forcing, end_data, snapshots, enhance)
        if scheme not in ops.BDF:
            raise ValueError(f"scheme must be 'bdf1' or 'bdf2', got {scheme!r}")
        if not np.all(p.quad["c"] + p.quad["rho"] / p.dt >= 0.0):
            raise ValueError(f"c + rho / dt < 0 at a quadrature point (dt = {p.dt:.6g}): the step's matrix would not "
                             "be positive definite, and the solve does not pivot; shorten the step")
        return p

    @staticmethod
    def _newton_args(who, nonlinear, newton_iters, newton_tol):
        """The semilinear keywords of :meth:`solve_transient` and :meth:`solve_transient_sensitivity` -> (the parsed
        law or None, newton_iters, newton_tol): ``newton_*`` only come with ``nonlinear``; defaults 3 and 1e-10."""
        if nonlinear is None:
            if newton_iters is not None or newton_tol is not None:
                raise ValueError(f"newton_iters and newton_tol belong to {who}(..., nonlinear=...)")
            return None, None, None
        nl = _Nonlinear(nonlinear)
        newton_iters, newton_tol = 3 if newton_iters is None else newton_iters, 1e-10 if newton_tol is None \
            else newton_tol
        if isinstance(newton_iters, bool) or int(newton_iters) != newton_iters or not 1 <= int(newton_iters) <= 8:
            raise ValueError(f"newton_iters must be an integer in 1 .. 8, got {newton_iters!r}")
        if not (float(newton_tol) > 0.0) or not math.isfinite(float(newton_tol)):
            raise ValueError(f"newton_tol must be finite and > 0, got {newton_tol!r}")
        return nl, int(newton_iters), float(newton_tol)

    @staticmethod
    def _newton_failures(who, newton, iters, tol):
        """The two ``RuntimeError``s of a semilinear loop from its monitor ``newton`` [nsteps, iters, 4] on the host: a
        non-finite value met, or a last increment above ``tol`` max(1, |v|_inf)."""
        def history(i):
            return ", ".join(f"|R| {r:.3e} |dv| {d:.3e}" for r, d, _, _ in newton[i])
        bad = np.nonzero(newton[:, :, 3].sum(axis=1) != 0.0)[0]
        if bad.size:
            i = int(bad[0])
            raise RuntimeError(f"{who}: step {i + 1} met {int(newton[i, :, 3].sum())} non-finite value(s) in "
                               f"its Newton iteration ({history(i)}); shorten the step")
        last = newton[:, -1, :]
        slow = np.nonzero(last[:, 1] > tol * np.maximum(1.0, last[:, 2]))[0]
        if slow.size:
            i = int(slow[0])
            raise RuntimeError(f"{who}: step {i + 1} did not converge in {iters} Newton iteration(s) to "
                               f"newton_tol = {tol:g} ({history(i)}); raise newton_iters or shorten the step")

    def solve_transient(self, u0, t_end, *, nsteps, scheme="bdf2", weight=None, forcing=None, end_data=None,
                        snapshots=None, enhance=True, nonlinear=None, newton_iters=None, newton_tol=None):
        """rho u_t - (a u')' + c u = f(x, t) for 0 < t <= ``t_end`` with u(x, 0) = ``u0(x)``, on the solver's ``mesh``
        with its ``coef``, ``reaction`` and ``boundary`` kinds (each end Dirichlet u = g(t) or Robin
        a du/dn + kappa u = g(t)); ``nsteps`` equal steps of backward Euler (``scheme="bdf1"``) or of BDF2 started by
        one backward-Euler step (``"bdf2"``).  ``weight`` = rho (a callable; ``None``: 1); ``forcing``: a list of at
        most 8 pairs (phi, f_x), f(x, t) = sum phi(t) f_x(x), phi a callable of t or a constant (``None``:
        ``[(1, self.rhs)]``); ``end_data`` = (g_left, g_right), callables of t or constants (``None``: the end values
        ``solve()`` uses); ``snapshots``: the step indices in 1 .. nsteps to keep (``None``: the last).  ``u0`` is
        sampled at the nodes, and a Dirichlet end starts at g(0).

        Per step ``ops.ts_rhs`` and one ``ops.tridiag_bc_solve_multi`` on the bands of
        K + (alpha / dt) M, assembled once per alpha; phi and g of every step are uploaded before the loop, which
        rotates three nodal buffers on one stream and issues no copy from the host and no synchronisation.  At a
        snapshot step ``ops.ts_source_table`` writes the right-hand side f(., t) - rho I_h w of the snapshot's elliptic
        problem (w: the nodal BDF difference); with ``enhance`` all snapshots then go through ONE
        ``ops.enhance_multi`` (``lssvr_M``, ``n_colloc``, ``lssvr_gamma``; c itself, not shifted by 1 / dt).  Two
        Neumann ends without a reaction are fine here: M / dt makes the matrix definite.  Returns a
        :class:`TransientSolution`; the solver's attributes are left as they are.

        ``nonlinear`` = ``("poly", [q0, q1, ...])`` or ``("exp", q0, q1)`` (the specs of the constructor's
        ``nonlinear=``, given HERE, on a solver built without it) adds g(x, u) to the left-hand side (DESIGN.md section
        28): every step then runs ``newton_iters`` Newton iterations (a fixed count, 1 .. 8, default 3; no line
        search) from the extrapolation 2 u^n - u^{n-1} (BDF1 and the first step: u^n), each ONE
        ``ops.ts_nl_assemble`` -> ``ops.tridiag_bc_solve_multi`` -> ``ops.nl_residual``, whose four numbers go to a
        device table that is read once, after the loop, with the snapshots (``TransientSolution.newton``).
        ``RuntimeError`` with the step and its history when a step's last increment exceeds
        ``newton_tol`` max(1, |v|_inf) (default 1e-10) or a non-finite value was met.  The q_k are tabulated and
        checked on the host before any device call; that c + alpha rho / dt + g_u >= 0 holds at the iterates cannot
        be checked without a read-back inside the loop and is not: the solve does not pivot, and the increment test
        after the loop is the net.  A snapshot is enhanced as the linear problem around its own nodal values, one
        ``ops.nl_linearize`` at the collocation points and one ``ops.enhance_varcoef`` each (c_eff differs per
        snapshot).  ``nonlinear=None`` runs exactly the calls above; ``newton_iters`` / ``newton_tol`` then must be
        left alone."""
        self._check_fem_order("solve_transient")
        if self.nonlinear is not None:
            raise ValueError("solve_transient takes the semilinear term as its own keyword: build the solver without "
                             "nonlinear= and call solve_transient(..., nonlinear=...)")
        enhance = bool(enhance)
        nl, iters, tol = self._newton_args("solve_transient", nonlinear, newton_iters, newton_tol)
        p = self._check_transient(u0, t_end, nsteps, scheme, weight, forcing, end_data, snapshots, enhance)
        kinds, kappa, steps, q, n = p.kinds, p.kappa, p.steps, p.quad, int(self.n_colloc)
        if nl is not None:
            if enhance and n > ops.NL_MAX_POINTS:
                raise ValueError(f"nonlinear needs n_colloc <= {ops.NL_MAX_POINTS} for the enhanced snapshots, got {n}")
            xq_host, xc_host = self._nl_host_points(p.nodes)
            qq_host = nl.host_tables(xq_host, "quadrature")
            qc_host = nl.host_tables(xc_host, "collocation") if enhance else None
        # ---- the device from here on
        torch = _torch()
        nsteps, ne, ns, inv_dt = int(nsteps), p.nodes.size - 1, len(steps), 1.0 / p.dt
        # the matrices of the loop: K + (alpha / dt) M as ONE reaction assembly each (with nonlinear= a diagnostic:
        # every Newton iteration assembles its own from the same c table)
        alphas = {ops.BDF["bdf1"][0], ops.BDF[scheme][0]}
        D = self._time_setup(p, enhance, [("mass", False, q["rho"]),
                                          *((al, True, q["c"] + al * q["rho"] / p.dt) for al in alphas)],
                             per_snapshot=nl is not None)
        dev, x, U, S, b, loads, work, snap, pm = D.dev, D.x, D.U, D.S, D.b, D.loads, D.work, D.snap, D.pm
        phi, g = D.phi, D.g[1:]                                        # row n - 1: the step that ends at t_n
        (md, mo), mon = D.bands["mass"], None
        if enhance:
            ftab, rtab, src = D.tab["f"], D.tab["rho"], D.src
        if nl is not None:
            qq = _to_dev(qq_host, dev)
            V = torch.empty((2, ne + 1), dtype=torch.float64, device=dev)         # the Newton iterates of a step
            rhs = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
            nb = dict(diag=torch.empty(ne + 1, dtype=torch.float64, device=dev),
                      off=torch.empty(ne, dtype=torch.float64, device=dev), rhs=rhs[0])
            mon = torch.zeros((nsteps, iters, 4), dtype=torch.float64, device=dev)
            rwork = ops._scratch(None, ops._capi.load().lssvr_nl_residual_work_bytes(ne), dev)
            if enhance:
                qc = _to_dev(np.transpose(qc_host, (0, 2, 1)) if pm else qc_host, dev)
                tloc = torch.arange(n, dtype=torch.float64, device=dev) / float(n - 1)
                c_eff, f_eff = (torch.empty_like(src) for _ in range(2))
        bdf1 = ops.BDF["bdf1"]
        cur, prev, new = 0, 1, 2
        # the loop: launches on the current stream only
        for step in range(1, nsteps + 1):
            al, b0, b1 = bdf1 if step == 1 else ops.BDF[scheme]
            u_prev = None if b1 == 0.0 else U[prev:prev + 1]
            ops.ts_rhs(md, mo, U[cur:cur + 1], u_prev, loads, phi[step - 1:step], b0, b1, inv_dt, out=b)
            if nl is None:
                ops.tridiag_bc_solve_multi(*D.bands[al], b, kinds, kappa, g[step - 1:step], out=U[new:new + 1],
                                           work=work)
            else:
                if b1 == 0.0:
                    V[0].copy_(U[cur])
                else:
                    ops.nl_step(U[prev], U[cur], 2.0, out=V[0])
                v, spare = V[0], V[1]
                for it in range(iters):
                    tgt = U[new] if it == iters - 1 else spare
                    ops.ts_nl_assemble(x, v, D.cq[al], nl.kind, qq, b[0], a_quad=D.aq, out=nb)
                    ops.tridiag_bc_solve_multi(nb["diag"], nb["off"], rhs, kinds, kappa, g[step - 1:step],
                                               out=tgt.unsqueeze(0), work=work)
                    ops.nl_residual(nb["diag"], nb["off"], nb["off"], nb["rhs"], v, tgt, kinds, kappa, g[step - 1],
                                    out4=mon[step - 1, it], work=rwork)
                    v, spare = tgt, v
            k = snap.get(step)
            if k is not None:
                S[k].copy_(U[new])
                if enhance:
                    ops.ts_source_table(U[new], U[cur], None if b1 == 0.0 else U[prev], ftab, rtab, phi[step - 1], al,
                                        b0, b1, inv_dt, point_major=pm, out=src[k])
                    if nl is not None:
                        ops.nl_linearize(U[new], tloc, nl.kind, qc, src[k], c_tab=D.tab["c"], point_major=pm,
                                         c_eff=c_eff[k], f_eff=f_eff[k])
            cur, prev, new = new, cur, prev
        enhanced = []
        if enhance and nl is None:
            enhanced = self._enhance_snapshots(p, D, S)
        elif enhance:
            # a snapshot is the linear problem around its own nodal values: c_eff differs per snapshot
            gd = (float(self.global_domain[0]), float(self.global_domain[1]))
            shard = self._shard(ne)
            for k, s in enumerate(steps):
                W, st = ops.enhance_varcoef(x, S[k], int(self.lssvr_M), float(self.lssvr_gamma), n, D.tab["a"],
                                            D.tab["da"], f_eff[k], global_domain=gd,
                                            bc=(float(p.g[s, 0]), float(p.g[s, 1])), point_major=pm,
                                            c_values=c_eff[k], **shard)
                enhanced.append(EnhancedSolution(x, W, st))
        order = sorted(alphas)
        host = _read_back(nodal=S, mass=D.bands["mass"], loads=loads, newton=mon,      # one copy: snapshots, bands, monitor
                          **{f"step{i}": D.bands[al] for i, al in enumerate(order)})
        bands = dict(mass=host["mass"], loads=host["loads"], step={al: host[f"step{i}"] for i, al in enumerate(order)})
        newton = host["newton"]
        if nl is not None:
            self._newton_failures("solve_transient", newton, iters, tol)
        return TransientSolution(p.times[steps].copy(), host["nodal"], enhanced, bands, newton)

    # ---- adjoint sensitivities of the BDF loop (no reference counterpart) ---------------------
    def _check_transient_sensitivity(self, p, goal, goal_steps, goal_weights, observe, max_state_bytes,
                                     who="solve_transient_sensitivity", first=1, ntraj=1):
        """The functional of :meth:`solve_transient_sensitivity` on the plan ``p`` of :meth:`_check_transient`, on the
        host and before any device call -> (steps, rows, functional): the ascending steps n with p_n != 0, ``rows``
        [len(steps), ne+1] for a goal (None for a misfit, whose rows need the trajectory), and
        ``functional(U_steps)`` -> (J, rows) for the nodal states at those steps.  ``who``, ``first`` and ``ntraj``: the
        caller's name, its first admissible step (0 where u^0 counts) and how many trajectories it stores."""
        nsteps, nodes = len(p.times) - 1, p.nodes
        if (goal is None) == (observe is None):
            raise ValueError(f"{who} needs exactly one of goal (a callable j(x): J = sum_k w_k int "
                             "j u^{n_k} dx) and observe = (steps, x_obs, d_obs) (J = 1/2 sum (u^{n_k}(x_i) - d_ki)^2)")
        need = ntraj * (nsteps + 1) * nodes.size * 8
        if need > max_state_bytes:
            raise ValueError(f"the stored trajectory needs {'' if ntraj == 1 else f'{ntraj} '}(nsteps+1)(ne+1) 8 = "
                             f"{need} bytes > max_state_bytes = "
                             f"{max_state_bytes}: checkpointing (recomputing the trajectory in pieces) is not built")

        def checked_steps(steps, what):
            steps = list(steps)
            if not steps or any(isinstance(s, bool) or int(s) != s or not first <= int(s) <= nsteps for s in steps):
                raise ValueError(f"{what} must be step indices in {first} .. nsteps = {nsteps}, got {steps!r}")
            steps = [int(s) for s in steps]
            if len(set(steps)) != len(steps):
                raise ValueError(f"{what} must not name a step twice, got {steps!r}")
            return steps
        h = np.diff(nodes)
        if goal is not None:
            if not callable(goal):
                raise ValueError("goal must be a callable j(x): the density of J = sum_k w_k int j u^{n_k} dx")
            steps = checked_steps([nsteps] if goal_steps is None else goal_steps, "goal_steps")
            wts = np.ones(len(steps)) if goal_weights is None else np.asarray(goal_weights, dtype=np.float64).reshape(-1)
            if wts.size != len(steps):
                raise ValueError(f"goal_weights must hold one weight per goal step ({len(steps)}), got {wts.size}")
            self._check_finite(("goal_weights", wts))
            xi, w = np.polynomial.legendre.leggauss(int(self.nquad))
            xi, w = 0.5 * (1.0 + xi), 0.5 * w
            xq = nodes[:-1, None] + h[:, None] * xi[None, :]
            try:
                j = np.broadcast_to(np.asarray(goal(xq), dtype=np.float64), xq.shape)
            except ValueError:
                raise ValueError(f"goal must return one value per point ({list(xq.shape)} at the quadrature points) or "
                                 "a value that broadcasts to them") from None
            if not np.all(np.isfinite(j)):
                raise ValueError("goal is not finite at a quadrature point")
            # the P1 load of j by the rule of the assembly: int j u_h dx = load . u
            load = np.zeros(nodes.size)
            load[:-1] += h * ((j * w) @ (1.0 - xi))
            load[1:] += h * ((j * w) @ xi)
            order = np.argsort(steps)
            steps, rows = [steps[i] for i in order], wts[order, None] * load[None, :]
            return steps, rows, lambda U: (float(np.sum(rows * U)), rows)
        if goal_steps is not None or goal_weights is not None:
            raise ValueError("goal_steps and goal_weights belong to goal=")
        if not isinstance(observe, (tuple, list)) or len(observe) != 3:
            raise ValueError("observe must be a triple (steps, x_obs, d_obs)")
        steps = checked_steps(observe[0], "observe steps")
        xo = np.asarray(observe[1], dtype=np.float64).reshape(-1)
        d = np.asarray(observe[2], dtype=np.float64)
        if xo.size < 1 or d.shape != (len(steps), xo.size):
            raise ValueError(f"observe: d_obs must be [len(steps), nobs] = [{len(steps)}, {xo.size}] with at least one "
                             f"point, got {list(d.shape)}")
        self._check_finite(("observe x_obs", xo), ("observe d_obs", d))
        if xo.min() < nodes[0] or xo.max() > nodes[-1]:
            raise ValueError(f"observe: every x_obs must lie in the mesh [{nodes[0]:.6g}, {nodes[-1]:.6g}]")
        order = np.argsort(steps)
        steps, d = [steps[i] for i in order], d[order]
        e = np.clip(np.searchsorted(nodes, xo, side="right") - 1, 0, nodes.size - 2)
        t = (xo - nodes[e]) / h[e]

        def misfit(U):
            r = U[:, e] * (1.0 - t) + U[:, e + 1] * t - d
            rows = np.zeros(U.shape)
            for k in range(len(steps)):
                np.add.at(rows[k], e, r[k] * (1.0 - t))
                np.add.at(rows[k], e + 1, r[k] * t)
            return 0.5 * float(np.sum(r * r)), rows
        return steps, None, misfit

    def solve_transient_sensitivity(self, u0, t_end, *, nsteps, scheme="bdf2", weight=None, forcing=None, end_data=None,
                                    goal=None, goal_steps=None, goal_weights=None, observe=None,
                                    max_state_bytes=2 ** 31, nonlinear=None, newton_iters=None, newton_tol=None):
        """Derivatives of a functional J of the trajectory of :meth:`solve_transient` (same ``u0``, ``t_end``,
        ``nsteps``, ``scheme``, ``weight``, ``forcing``, ``end_data``) with respect to the data of the loop, by the
        discrete adjoint: exact for the discrete scheme, at the cost of one more loop of the same length.  ``goal``: a
        callable j(x), J = sum_k w_k int j u^{n_k} dx by the quadrature rule of the assembly, over ``goal_steps``
        (default ``[nsteps]``) with ``goal_weights`` (default ones); or ``observe=(steps, x_obs, d_obs)`` with d_obs
        [len(steps), nobs]: the misfit J = 1/2 sum_k sum_i (u^{n_k}(x_i) - d_ki)^2 at points inside the mesh.

        The forward loop is :meth:`solve_transient`'s, bit for bit, writing every u^n into a stored trajectory
        [nsteps+1, ne+1].  The rows p_n = dJ/du^n that are not zero are uploaded once (for a misfit they are formed on
        the host from the observed steps, one read-back between the loops).  The backward sweep runs n = nsteps .. 1
        in chunks of up to 8 steps: per step ``ops.ts_rhs`` (U0 = lambda^{n+1}, U1 = lambda^{n+2}, the load p_n,
        phi = 1, coefficients (beta0_{n+1}, beta1_{n+2})) and ``ops.tridiag_bc_solve_multi`` on the forward loop's
        bands with zero end data, into the chunk's rows; then ONE ``ops.ts_sensitivity`` per chunk adds the chunk to
        the tables.  Two chunk buffers alternate, so lambda^{n+1}, lambda^{n+2} of a chunk's first steps are still in
        the other.  One last ``ops.ts_rhs`` gives B_0 = dJ/du0, and one read-back fetches everything.  Neither loop
        synchronises or copies from the host.  Returns a :class:`TransientSensitivity`; the solver's attributes are
        left as they are.

        ``nonlinear`` (with ``newton_iters``, ``newton_tol``; the rules of :meth:`solve_transient`: the term is given
        HERE, on a solver built without it) differentiates the semilinear loop rho u_t - (a u')' + c u + g(x, u) = f
        (DESIGN.md section 36).  The gradient is that of the CONVERGED implicit step: level n counts as the solution of
        F_n(u^n) = 0, which the Newton iteration converges to quadratically, so a state whose last increment is |dv|
        differs from it by O(|dv|^2), and so does the gradient; ``newton`` of the result holds |dv| of every iteration
        (differentiating through a fixed iteration count would need g_uu and is not built).  The forward loop is
        :meth:`solve_transient`'s semilinear loop, call for call, into the stored trajectory; its monitor is read once
        after the loop (with the observed states of a misfit) and the two ``RuntimeError``s of :meth:`solve_transient`
        are raised BEFORE the backward sweep.  Per level the sweep then issues ONE ``ops.ts_nl_adjoint_step`` -- the
        bands of the Jacobian J_n = K + M(c + alpha_n rho / dt + g_u(., u^n_h)) AT u^n (not the forward loop's last
        Newton matrix, linearised one iterate earlier), B_n and the end entries of J_n -- and one
        ``ops.tridiag_bc_solve_multi``, and per chunk ONE ``ops.ts_nl_sensitivity``, which adds ``d_nonlinear``
        [nterm, ne, nquad] = dJ/dq_k at every quadrature point.  ``nonlinear=None`` issues exactly the calls above;
        ``d_nonlinear`` and ``newton`` are then ``None``.

        Refused (``ValueError``, before any device call): what :meth:`solve_transient` refuses (convection,
        ``boundary="periodic"``, a ``fem_solver`` other than "bands", ``element_degrees``, a solver other than
        ``ops.SOLVER_PRIMAL``), a solver built with ``nonlinear=``, both or neither of ``goal`` and ``observe``, a step
        outside 1 .. nsteps or named twice, data of the wrong shape or not finite, and a trajectory of more than
        ``max_state_bytes``: checkpointing is not built."""
        self._check_fem_order("solve_transient_sensitivity")
        self._check_nonlinear("solve_transient_sensitivity")
        nl, iters, tol = self._newton_args("solve_transient_sensitivity", nonlinear, newton_iters, newton_tol)
        p = self._check_transient(u0, t_end, nsteps, scheme, weight, forcing, end_data, None, False)
        jsteps, rows, functional = self._check_transient_sensitivity(p, goal, goal_steps, goal_weights, observe,
                                                                     max_state_bytes)
        kinds, kappa, q = p.kinds, p.kappa, p.quad
        if nl is not None:
            qq_host = nl.host_tables(self._nl_host_points(p.nodes)[0], "quadrature")
        # ---- the device from here on
        torch = _torch()
        nsteps, ne, inv_dt = int(nsteps), p.nodes.size - 1, 1.0 / p.dt
        bdf1, bdf = ops.BDF["bdf1"], ops.BDF[scheme]
        alphas = {bdf1[0], bdf[0]}
        D = self._time_setup(p, False, [("mass", False, q["rho"]),
                                        *((al, True, q["c"] + al * q["rho"] / p.dt) for al in alphas)],
                             nbuf=nsteps + 1)
        dev, x, U, b, loads, work = D.dev, D.x, D.U, D.b, D.loads, D.work
        phi, g = D.phi, D.g[1:]                                        # row n - 1: the step that ends at t_n
        md, mo = D.bands["mass"]

        def coefficients(n):
            """(alpha_n, beta0_n, beta1_n); zeros beyond the last step."""
            return (0.0, 0.0, 0.0) if n > nsteps else bdf1 if n == 1 else bdf

        if nl is not None:
            qq = _to_dev(qq_host, dev)
            V = torch.empty((2, ne + 1), dtype=torch.float64, device=dev)         # the Newton iterates of a step
            rhs = torch.empty((1, ne + 1), dtype=torch.float64, device=dev)
            nb = dict(diag=torch.empty(ne + 1, dtype=torch.float64, device=dev),
                      off=torch.empty(ne, dtype=torch.float64, device=dev), rhs=rhs[0])
            mon = torch.zeros((nsteps, iters, 4), dtype=torch.float64, device=dev)
            rwork = ops._scratch(None, ops._capi.load().lssvr_nl_residual_work_bytes(ne), dev)
        # the forward loop of solve_transient, every state kept: row n of U is u^n
        for n in range(1, nsteps + 1):
            al, b0, b1 = coefficients(n)
            ops.ts_rhs(md, mo, U[n - 1:n], None if b1 == 0.0 else U[n - 2:n - 1], loads, phi[n - 1:n], b0, b1, inv_dt,
                       out=b)
            if nl is None:
                ops.tridiag_bc_solve_multi(*D.bands[al], b, kinds, kappa, g[n - 1:n], out=U[n:n + 1], work=work)
                continue
            if b1 == 0.0:
                V[0].copy_(U[n - 1])
            else:
                ops.nl_step(U[n - 2], U[n - 1], 2.0, out=V[0])
            v, spare = V[0], V[1]
            for it in range(iters):
                tgt = U[n] if it == iters - 1 else spare
                ops.ts_nl_assemble(x, v, D.cq[al], nl.kind, qq, b[0], a_quad=D.aq, out=nb)
                ops.tridiag_bc_solve_multi(nb["diag"], nb["off"], rhs, kinds, kappa, g[n - 1:n], out=tgt.unsqueeze(0),
                                           work=work)
                ops.nl_residual(nb["diag"], nb["off"], nb["off"], nb["rhs"], v, tgt, kinds, kappa, g[n - 1],
                                out4=mon[n - 1, it], work=rwork)
                v, spare = tgt, v
        newton = None
        if nl is not None:
            # the one read-back between the loops: the monitor, and the observed states a misfit forms its rows from
            between = _read_back(newton=mon, u=U[torch.as_tensor(jsteps, device=dev)])
            newton = between["newton"]
            self._newton_failures("solve_transient_sensitivity", newton, iters, tol)
            if rows is None:
                rows = functional(between["u"])[1]
        # the rows p_n that are not zero, and a zero row for every other step (and for lambda^{N+1}, lambda^{N+2})
        jidx, P, prow = _functional_rows(U, jsteps, rows, functional, zero_rows=1)
        zero, one = P[len(jsteps):], torch.ones((1, 1), dtype=torch.float64, device=dev)
        chunk = ops.TS_SENS_CHUNK
        Zb, Bb = (torch.empty((2, chunk, ne + 1), dtype=torch.float64, device=dev) for _ in range(2))
        if nl is not None:
            return self._transient_nl_backward(p, D, nl, qq, U, jidx, P, prow, zero, one, Zb, Bb, coefficients,
                                               functional, newton)
        band_ends = torch.stack([torch.stack((D.bands[al][1][0], D.bands[al][1][ne - 1])) for al in (bdf1[0], bdf[0])])
        out = dict(g=torch.zeros((nsteps + 1, 2), dtype=torch.float64, device=dev))
        lam1, lam2 = zero, zero                                        # lambda^{n+1}, lambda^{n+2}
        # the backward sweep: launches on the current stream only
        for hi, m, side in _sweep_chunks(nsteps, chunk):
            Z, B = Zb[side, :m], Bb[side, :m]
            for i in range(m):
                n = hi - i
                b0, b1 = coefficients(n + 1)[1], coefficients(n + 2)[2]
                k = prow.get(n, len(jsteps))
                ops.ts_rhs(md, mo, lam1, None if b1 == 0.0 else lam2, P[k:k + 1], one, b0, b1, inv_dt, out=B[i:i + 1])
                ops.tridiag_bc_solve_multi(*D.bands[coefficients(n)[0]], B[i:i + 1], kinds, kappa, None,
                                           out=Z[i:i + 1], work=work)
                lam1, lam2 = Z[i:i + 1], lam1
            steps = range(hi, hi - m, -1)
            out = ops.ts_sensitivity(x, U, Z, hi - m + 1, [coefficients(n) for n in steps], inv_dt, self.nquad, phi=phi,
                                     Brows=B, band_ends=band_ends, band_rows=[0 if n == 1 else 1 for n in steps],
                                     end_kinds=kinds, accumulate=hi < nsteps, out=out)
        b0, b1 = coefficients(1)[1], coefficients(2)[2]
        ops.ts_rhs(md, mo, lam1, None if b1 == 0.0 else lam2, zero, one, b0, b1, inv_dt, out=b)       # B_0
        host = _read_back(b0=b, u=U[jidx], **out)
        value, _ = functional(host["u"])
        d_u0, d_g = host["b0"][0].copy(), host["g"].copy()
        _dirichlet_u0(kinds, d_u0, d_g)
        return TransientSensitivity(value, {k: host[k].copy() for k in ops.TS_SENS_TABLES}, d_u0, d_g,
                                    host["kappa"].copy(), p.times.copy(), p.nodes)

    def _transient_nl_backward(self, p, D, nl, qq, U, jidx, P, prow, zero, one, Zb, Bb, coefficients, functional,
                               newton):
        """The backward sweep of :meth:`solve_transient_sensitivity` with ``nonlinear=``, on what
        its forward loop left: per level ONE ``ops.ts_nl_adjoint_step`` (the Jacobian AT u^n, B_n, the end entries) and
        one solve, per chunk ONE ``ops.ts_nl_sensitivity``; launches on the current stream only."""
        torch = _torch()
        dev, x, b, work, kinds, kappa = D.dev, D.x, D.b, D.work, p.kinds, p.kappa
        nsteps, ne, inv_dt, chunk = len(p.times) - 1, p.nodes.size - 1, 1.0 / p.dt, ops.TS_SENS_CHUNK
        md, mo = D.bands["mass"]
        nterm, nzero = int(qq.shape[0]), len(prow)
        jac = dict(diag=torch.empty(ne + 1, dtype=torch.float64, device=dev),
                   off=torch.empty(ne, dtype=torch.float64, device=dev))
        band_ends = torch.empty((chunk, 2), dtype=torch.float64, device=dev)
        out = dict(g=torch.zeros((nsteps + 1, 2), dtype=torch.float64, device=dev))
        lam1, lam2 = zero, zero                                        # lambda^{n+1}, lambda^{n+2}
        for hi, m, side in _sweep_chunks(nsteps, chunk):
            Z, B = Zb[side, :m], Bb[side, :m]
            for i in range(m):
                n = hi - i
                b0, b1 = coefficients(n + 1)[1], coefficients(n + 2)[2]
                k = prow.get(n, nzero)
                ops.ts_nl_adjoint_step(x, U[n], D.cq[coefficients(n)[0]], nl.kind, qq, md, mo, lam1,
                                       None if b1 == 0.0 else lam2, P[k:k + 1], one, b0, b1, inv_dt, a_quad=D.aq,
                                       out=dict(jac, B=B[i:i + 1], band_ends=band_ends[i]))
                ops.tridiag_bc_solve_multi(jac["diag"], jac["off"], B[i:i + 1], kinds, kappa, None, out=Z[i:i + 1],
                                           work=work)
                lam1, lam2 = Z[i:i + 1], lam1
            steps = range(hi, hi - m, -1)
            out = ops.ts_nl_sensitivity(x, U, Z, hi - m + 1, [coefficients(n) for n in steps], inv_dt, self.nquad,
                                        nl.kind, nterm, q_tabs=qq, phi=D.phi, Brows=B, band_ends=band_ends[:m],
                                        end_kinds=kinds, accumulate=hi < nsteps, out=out)
        b0, b1 = coefficients(1)[1], coefficients(2)[2]
        ops.ts_rhs(md, mo, lam1, None if b1 == 0.0 else lam2, zero, one, b0, b1, inv_dt, out=b)       # B_0
        host = _read_back(b0=b, u=U[jidx], **out)
        value, _ = functional(host["u"])
        d_u0, d_g = host["b0"][0].copy(), host["g"].copy()
        _dirichlet_u0(kinds, d_u0, d_g)
        return TransientSensitivity(value, {k: host[k].copy() for k in ops.TS_SENS_TABLES}, d_u0, d_g,
                                    host["kappa"].copy(), p.times.copy(), p.nodes, host["q"].copy(), newton)

    # ---- adaptive time stepping (no reference counterpart) ----------------------------------
    def _check_adaptive(self, u0, t_end, rtol, atol, dt0, t_out, dt_min, dt_max, max_steps, weight, forcing, end_data,
                        enhance):
        """:meth:`_check_time` for :meth:`solve_transient_adaptive`, and what belongs to the controller: the
        tolerances, dt0, dt_min, dt_max, the output times, max_steps, and c + rho / dt_max >= 0 at the quadrature
        points (alpha >= 1 for every omega, so this covers every step).  Returns the plan with rtol, atol, dt0, dt_min,
        dt_max, t_out (a float64 array), max_steps added."""
        if self.nonlinear is not None:
            raise ValueError("solve_transient_adaptive has no nonlinear term: the Newton iteration inside a step has "
                             "no error control yet; use solve_transient(..., nonlinear=...)")
        p = self._check_time("solve_transient_adaptive", u0, t_end, None, weight, forcing, end_data, None, enhance,
                             phi0=True)
        t_end = float(t_end)
        try:
            rtol, atol, dt0 = float(rtol), float(atol), float(dt0)
        except (TypeError, ValueError):
            raise ValueError("rtol, atol and dt0 must be numbers") from None
        if not (math.isfinite(rtol) and math.isfinite(atol)) or rtol < 0.0 or atol < 0.0 or not rtol + atol > 0.0:
            raise ValueError(f"rtol and atol must be finite and >= 0 and rtol + atol > 0, got rtol = {rtol!r}, "
                             f"atol = {atol!r}")
        if not 0.0 < dt0 <= t_end:
            raise ValueError(f"dt0 must lie in (0, t_end = {t_end!r}], got {dt0!r}")
        dt_min = 16.0 * 2.0 ** -52 * t_end if dt_min is None else float(dt_min)
        dt_max = t_end if dt_max is None else float(dt_max)
        if not (math.isfinite(dt_min) and 0.0 <= dt_min <= dt0):
            raise ValueError(f"dt_min must lie in [0, dt0 = {dt0!r}], got {dt_min!r}")
        if not (math.isfinite(dt_max) and dt_max >= dt0):
            raise ValueError(f"dt_max must be finite and >= dt0 = {dt0!r}, got {dt_max!r}")
        if isinstance(max_steps, bool) or int(max_steps) != max_steps or int(max_steps) < 1:
            raise ValueError(f"max_steps must be an integer >= 1, got {max_steps!r}")
        t_out = np.array([t_end] if t_out is None else t_out, dtype=np.float64).reshape(-1)
        if t_out.size < 1 or not np.all(np.isfinite(t_out)) or not np.all(np.diff(t_out) > 0.0) \
                or not (t_out[0] > 0.0 and t_out[-1] <= t_end):
            raise ValueError(f"t_out must be ascending times in (0, t_end = {t_end!r}], got {t_out.tolist()!r}")
        if not np.all(p.quad["c"] + p.quad["rho"] / dt_max >= 0.0):
            raise ValueError(f"c + rho / dt_max < 0 at a quadrature point (dt_max = {dt_max:.6g}): a step's matrix "
                             "would not be positive definite, and the solve does not pivot; give a smaller dt_max")
        p.rtol, p.atol, p.dt0, p.dt_min, p.dt_max, p.t_out, p.max_steps = rtol, atol, dt0, dt_min, dt_max, t_out, \
            int(max_steps)
        return p

    def solve_transient_adaptive(self, u0, t_end, *, rtol, atol, dt0, t_out=None, dt_min=None, dt_max=None,
                                 max_steps=100000, weight=None, forcing=None, end_data=None, enhance=True):
        """The problem of :meth:`solve_transient` with steps chosen by a local error estimate: variable-step BDF2
        (step 1: backward Euler with ``dt0``) and per-step control of
        err = max_i |e_i| / (``atol`` + ``rtol`` max(|u^{n+1}_i|, |u^n_i|)) over all nodes but Dirichlet end nodes, e a
        divided difference of the last nodal vectors.  An attempt is accepted iff err <= 1; the
        next step is the attempt's times clip(0.9 err^(-1/3), 0.2, 2) (no growth right after a rejection).  ``t_out``:
        ascending output times in (0, t_end] (``None``: ``[t_end]``), each hit exactly: ``times`` of the result equals
        it bit for bit.  ``dt_max`` (``None``: t_end) caps the step; c + rho / dt_max >= 0 is required, so a negative
        reaction needs one.  ``RuntimeError`` when the controller's dt falls below ``dt_min`` (``None``:
        16 eps t_end), after ``max_steps`` attempts, or when step 2 -- whose estimate judges step 1 -- is rejected more
        than 8 times (each restarts from u0 with a smaller dt0).

        Per attempt: phi(t) and g(t) of the trial time go up as one row of R + 2 doubles, ``ops.ts_step`` writes
        K + (alpha / h) M and the right-hand side from the bands K and M assembled ONCE before the loop,
        ``ops.tridiag_bc_solve_multi`` solves, ``ops.ts_error`` reduces the estimate and its four doubles come back --
        the one synchronisation of an attempt.  Four nodal buffers rotate on acceptance only (a fifth keeps the start).  At an output step
        ``ops.ts_source_table`` runs with that step's alpha, beta0, beta1 and 1 / h, and with ``enhance`` all snapshots
        go through ONE ``ops.enhance_multi`` after the loop.  Snapshots, bands and the monitor come back in one copy.
        Returns a :class:`TransientSolution` with ``steps``, ``n_accepted``, ``n_rejected``, ``n_restarts``,
        ``monitor``; the solver's attributes are left as they are."""
        self._check_fem_order("solve_transient_adaptive")
        enhance = bool(enhance)
        p = self._check_adaptive(u0, t_end, rtol, atol, dt0, t_out, dt_min, dt_max, max_steps, weight, forcing,
                                 end_data, enhance)
        kinds, kappa, q, t_out = p.kinds, p.kappa, p.quad, p.t_out
        ns, R = t_out.size, p.phi.shape[1]
        p.steps = list(range(ns))                                  # the snapshots index the table of g below
        p.g = np.zeros((ns, 2))
        # ---- the device from here on
        torch = _torch()
        ne = p.nodes.size - 1
        D = self._time_setup(p, enhance, [("mass", False, q["rho"]), ("stiff", True, q["c"])], nbuf=5)
        dev, U, S, b, loads, work, pm, G = D.dev, D.U, D.S, D.b, D.loads, D.work, D.pm, D.g
        (md, mo), (kd, ko) = D.bands["mass"], D.bands["stiff"]
        U[4].copy_(U[0])                                                   # the start, kept for a restart
        adiag, aoff = torch.empty_like(kd), torch.empty_like(ko)
        row = torch.empty(R + 2, dtype=torch.float64, device=dev)          # phi_r(t), then g(t), of the trial time
        phi, g = row[:R].unsqueeze(0), row[R:].unsqueeze(0)
        ework = ops._scratch(None, ops._capi.load().lssvr_ts_error_work_bytes(ne), dev)
        mon = []                                                           # blocks [TS_MONITOR_ROWS, 4] of out4 rows
        if enhance:
            ftab, rtab, src = D.tab["f"], D.tab["rho"], D.src
        steps, hs = [], []                       # every attempt; the accepted steps, newest first
        new, cur, prev, old = 1, 0, 2, 3
        t, dt, k, restarts, after_reject, dt_start, s_last, n_est, err = 0.0, p.dt0, 0, 0, False, p.dt0, None, 0, \
            math.nan
        # the loop: launches on the current stream; per attempt one small upload and one read-back of four doubles
        while k < ns:
            if len(steps) >= p.max_steps:
                raise RuntimeError(f"solve_transient_adaptive: more than max_steps = {p.max_steps} attempts at "
                                   f"t = {t:.6g}, dt = {dt:.6g}, last err = {err:.6g}")
            if dt < p.dt_min:
                raise RuntimeError(f"solve_transient_adaptive: dt = {dt:.6g} < dt_min = {p.dt_min:.6g} at "
                                   f"t = {t:.6g}, last err = {err:.6g}")
            n = len(hs) + 1
            h, t_new, short = ts_trial_step(t, dt, p.dt_max, hs[0] if hs else None, float(t_out[k]))
            al, b0, b1 = ops.BDF["bdf1"] if n == 1 else ts_coefficients(h / hs[0])
            inv_h, s = 1.0 / h, al / h
            host_row = np.array([float(f(t_new)) for f in (*p.phi_fns, *p.g_fns)], dtype=np.float64)
            if not np.all(np.isfinite(host_row)):
                raise ValueError(f"forcing phi or end_data is not finite at t = {t_new!r}")
            row.copy_(torch.from_numpy(host_row))
            ops.ts_step(kd, ko, md, mo, U[cur:cur + 1], None if b1 == 0.0 else U[prev:prev + 1], loads, phi, s, b0, b1,
                        inv_h, adiag=adiag, aoff=aoff, write_bands=s != s_last, out=b)
            s_last = s
            ops.tridiag_bc_solve_multi(adiag, aoff, b, kinds, kappa, g, out=U[new:new + 1], work=work)
            if n == 1:                                       # no estimate: nothing to read, nothing to wait for
                err, accepted, fac = math.nan, True, 1.0
            else:
                w = ts_error_weights(h, hs[0]) if n == 2 else ts_error_weights(h, hs[0], hs[1], al)
                if n_est % TS_MONITOR_ROWS == 0:
                    mon.append(torch.zeros((TS_MONITOR_ROWS, 4), dtype=torch.float64, device=dev))
                out4 = mon[-1][n_est % TS_MONITOR_ROWS]
                n_est += 1
                ops.ts_error(U[new], U[cur], U[prev], U[old] if n > 2 else None, w, p.atol, p.rtol, kinds, out4=out4,
                             work=ework)
                r4 = out4.cpu().numpy()
                err = float(r4[0])
                accepted, fac = ts_controller(err, float(r4[3]), 2 if n == 2 else 3, after_reject)
            steps.append((t, h, err, float(accepted)))
            if not accepted and n == 2:
                # the estimate of step 2 judges step 1, which cannot be retried alone: start again with a smaller dt0
                restarts += 1
                if restarts > TS_MAX_RESTARTS:
                    raise RuntimeError(f"solve_transient_adaptive: step 2 rejected after {TS_MAX_RESTARTS} restarts "
                                       f"(dt = {h:.6g}, err = {err:.6g}); give a smaller dt0")
                dt_start = fac * dt_start
                U[0].copy_(U[4])
                new, cur, prev, old = 1, 0, 2, 3
                hs, t, dt, k, after_reject = [], 0.0, dt_start, 0, True
                continue
            if n > 1:
                dt = ts_next_dt(dt, h, short, accepted, fac)
                after_reject = not accepted
            if not accepted:
                continue
            if t_new == t_out[k]:
                S[k].copy_(U[new])
                G[k].copy_(row[R:])
                if enhance:
                    ops.ts_source_table(U[new], U[cur], None if b1 == 0.0 else U[prev], ftab, rtab, row[:R], al, b0,
                                        b1, inv_h, point_major=pm, out=src[k])
                k += 1
            new, cur, prev, old = old, new, cur, prev
            hs, t = [h] + hs[:1], t_new
        enhanced = self._enhance_snapshots(p, D, S) if enhance else []
        host = _read_back(nodal=S, mass=D.bands["mass"], stiff=D.bands["stiff"], loads=loads,   # one copy
                          monitor=torch.cat(mon)[:n_est] if mon else None)
        bands = dict(mass=host["mass"], stiff=host["stiff"], loads=host["loads"])
        return TransientSolution(t_out.copy(), host["nodal"], enhanced, bands,
                                 steps=np.array(steps, dtype=np.float64).reshape(-1, 4), n_restarts=restarts,
                                 monitor=host["monitor"])

    # ---- wave problems (no reference counterpart) -----------------------------
    def _check_wave(self, u0, v0, t_end, nsteps, damping, weight, forcing, end_data, end_accel0, snapshots, enhance,
                    beta, gamma):
        """:meth:`_check_time` for :meth:`solve_wave` (the tables gain d, phi the row of t = 0), and what belongs to the
        Newmark rule: the plan gains beta, gamma, v_init, accel0 [2] and shift [ne, nquad], the reaction table of the
        step's matrix, which must stay definite."""
        p = self._check_time("solve_wave", u0, t_end, nsteps, weight, forcing, end_data, snapshots, enhance,
                             damping=damping, phi0=True)
        p.beta, p.gamma = float(beta), float(gamma)
        if not (math.isfinite(p.beta) and math.isfinite(p.gamma)):
            raise ValueError(f"beta and gamma must be finite, got {beta!r}, {gamma!r}")
        # (the bound itself is allowed: 0.25 * (0.6 + 0.5) ** 2 rounds one ulp above 0.3025)
        if p.gamma < 0.5 or p.beta * (1.0 + 2.0 ** -50) < 0.25 * (p.gamma + 0.5) ** 2:
            raise ValueError(f"beta = {p.beta!r}, gamma = {p.gamma!r}: the Newmark rule is unconditionally stable for "
                             "gamma >= 1/2 and beta >= (gamma + 1/2)^2 / 4 only, and the step is not checked "
                             "against the mesh")
        if not callable(v0):
            raise ValueError("v0 must be a callable v0(x)")
        p.v_init = np.array(np.broadcast_to(np.asarray(v0(p.nodes), dtype=np.float64), p.nodes.shape))
        for i, end in ((0, 0), (1, -1)):
            if p.kinds[i] == ops.END_DIRICHLET:
                if callable(p.end_data[i]) and end_accel0 is None:
                    raise ValueError("end_accel0 = (g_left''(0), g_right''(0)) is needed when a Dirichlet end has "
                                     "callable end_data: the first acceleration takes that value at the end, and "
                                     "the average-acceleration rule never damps an error in it")
                if not callable(p.end_data[i]):
                    p.v_init[end] = 0.0                       # constant Dirichlet data: the end does not move
        acc0 = (0.0, 0.0) if end_accel0 is None else end_accel0
        if not isinstance(acc0, (tuple, list, np.ndarray)) or len(acc0) != 2:
            raise ValueError("end_accel0 must be a pair (g_left''(0), g_right''(0))")
        p.accel0 = np.array([float(acc0[0]), float(acc0[1])])
        self._check_finite(("v0", p.v_init), ("end_accel0", p.accel0))
        p.shift = p.quad["c"] + p.quad["rho"] / (p.beta * p.dt ** 2)
        if damping is not None:
            p.shift = p.shift + p.gamma * p.quad["d"] / (p.beta * p.dt)
        if not np.all(p.shift >= 0.0):
            raise ValueError(f"c + rho / (beta dt^2) + gamma d / (beta dt) < 0 at a quadrature point "
                             f"(dt = {p.dt:.6g}): the step's matrix would not be positive definite, and the solve "
                             "does not pivot; shorten the step")
        return p

    @staticmethod
    def _wave_energy_ends(p):
        """(kinds, kappa) for ``ops.eig_apply`` on every node of a wave problem: all ends as Robin rows, kappa of the
        problem's Robin ends (eig_apply adds it to K's end diagonal itself, so u^T K u already holds kappa u_end^2)."""
        return ((ops.END_ROBIN, ops.END_ROBIN),
                tuple(kp if kd_ == ops.END_ROBIN else 0.0 for kd_, kp in zip(p.kinds, p.kappa)))

    def _wave_first_accel(self, p, D, damped, sz0, MZ, KZ, gram0, ework, v_out, acc_out):
        """The start of a Newmark loop on the plan ``p`` of :meth:`_check_wave` and the arrays ``D`` of
        :meth:`_time_setup`: sz0 [2, ne+1] receives [u0, v0], one ``ops.eig_apply`` on it fills MZ, KZ [2, ne+1] and
        gram0, and the first acceleration solves M_rho acc0 = load(0) - M_d v0 - K u0, Robin rows with
        g(0) - kappa u0, into ``acc_out`` [1, ne+1]; ``v_out`` [ne+1] receives v0."""
        kinds, ne, phi, g = p.kinds, p.nodes.size - 1, D.phi, D.g
        (kd, ko), (md, mo) = D.bands["stiff"], D.bands["mass"]
        ekinds, ekap = self._wave_energy_ends(p)
        sz0[0].copy_(D.U[0])
        sz0[1].copy_(_to_dev(p.v_init, D.dev))
        ops.eig_apply(kd, ko, md, mo, sz0, ekinds, ekap, MZ=MZ, KZ=KZ, gram=gram0, work=ework)
        r0 = (phi[0][:, None] * D.loads).sum(dim=0)
        if damped:
            dd, do = D.bands["damp"]
            dv = ops.eig_apply(kd, ko, dd, do, sz0[1:2], ekinds, ekap, work=ework)[0]
            r0 = r0 - dv[0]
        r0 = r0 - KZ[0]
        a_ends = [0.0, 0.0]
        for i, end in ((0, 0), (1, ne)):
            if kinds[i] == ops.END_ROBIN:
                r0[end] += g[0, i]
            else:
                a_ends[i] = float(p.accel0[i])
        v_out.copy_(sz0[1])
        ops.tridiag_bc_solve_multi(md, mo, r0.unsqueeze(0).contiguous(), kinds, (0.0, 0.0), [a_ends], out=acc_out,
                                   work=D.work)

    def solve_wave(self, u0, v0, t_end, *, nsteps, damping=None, weight=None, forcing=None, end_data=None,
                   end_accel0=None, snapshots=None, enhance=True, beta=0.25, gamma=0.5):
        """rho u_tt + d u_t - (a u')' + c u = f(x, t) for 0 < t <= ``t_end`` with u(x, 0) = ``u0(x)`` and
        u_t(x, 0) = ``v0(x)``, on the solver's ``mesh`` with its ``coef``, ``reaction`` and ``boundary`` kinds (each end
        Dirichlet u = g(t) or Robin a du/dn + kappa u = g(t), kappa >= 0); ``nsteps`` equal steps of the Newmark rule
        (``beta``, ``gamma``) in displacement form -- the default (1/4, 1/2) is the average-acceleration rule:
        unconditionally stable, second order, and energy conserving for d = 0, f = 0.  ``damping`` = d and ``weight`` =
        rho are callables of x (``None``: 0 and 1); ``forcing``, ``end_data`` and ``snapshots`` as in
        :meth:`solve_transient`.  ``u0`` and ``v0`` are sampled at the nodes; a Dirichlet end starts at g(0), and with
        constant data its velocity is 0 (with callable data ``v0`` must equal g'(0) there).  ``end_accel0`` =
        (g_left''(0), g_right''(0)) is the first acceleration's value at a Dirichlet end: required when such an end
        has callable ``end_data``, zeros otherwise.

        Before the loop the bands of K, M_rho, M_d and of the step's matrix
        K + M_rho / (beta dt^2) + gamma M_d / (beta dt) are assembled once each, phi and g of every step are uploaded,
        and the first acceleration solves M_rho acc0 = load(0) - M_d v0 - K u0 with the products of ``ops.eig_apply``.
        Per step ONE ``ops.tridiag_bc_solve_multi`` and ONE ``ops.wave_advance``, which writes the correctors of the
        step and the right-hand side of the next; two (v, acc) pairs and two nodal buffers alternate on one stream,
        with no copy from the host and no synchronisation.  At a snapshot step one ``ops.eig_apply`` on [u, v] gives
        the energy E = 1/2 v^T M_rho v + 1/2 u^T K u + 1/2 sum over the Robin ends of kappa u_end^2, and
        ``ops.ts_source_table`` the right-hand side f(., t) - rho I_h acc - d I_h v of the snapshot's elliptic
        problem; with ``enhance`` all snapshots then go through ONE ``ops.enhance_multi``.  Returns a
        :class:`WaveSolution`; the solver's attributes are left as they are."""
        self._check_fem_order("solve_wave")
        self._check_nonlinear("solve_wave")
        torch = _torch()
        enhance = bool(enhance)
        p = self._check_wave(u0, v0, t_end, nsteps, damping, weight, forcing, end_data, end_accel0, snapshots, enhance,
                             beta, gamma)
        kinds, kappa, dt, steps, q, beta, gamma = p.kinds, p.kappa, p.dt, p.steps, p.quad, p.beta, p.gamma
        nsteps, ne, ns, damped = int(nsteps), p.nodes.size - 1, len(steps), damping is not None
        # K, M_rho, M_d and the step's matrix K + M_rho / (beta dt^2) + gamma M_d / (beta dt): ONE assembly each
        D = self._time_setup(p, enhance, [("stiff", True, q["c"]), ("mass", False, q["rho"]),
                                          *([("damp", False, q["d"])] if damped else []), ("step", True, p.shift)],
                             nbuf=2)
        dev, U, b, loads, work, snap, pm = D.dev, D.U, D.b, D.loads, D.work, D.snap, D.pm
        phi, g, SA = D.phi, D.g, D.S                      # row n: the time t_n; SA: the accelerations of the snapshots
        (kd, ko), (md, mo), (ad, ao) = D.bands["stiff"], D.bands["mass"], D.bands["step"]
        dd, do = D.bands["damp"] if damped else (None, None)
        if enhance:
            ftab, rtab, src = D.tab["f"], D.tab["rho"], D.src
            if damped:
                tmp = torch.empty((1,) + tuple(rtab.shape), dtype=torch.float64, device=dev)
                one = torch.ones(1, dtype=torch.float64, device=dev)
        ekinds, ekap = self._wave_energy_ends(p)
        VA = torch.empty((2, 2, ne + 1), dtype=torch.float64, device=dev)     # [pair][v, acc]
        SZ = torch.empty((ns + 1, 2, ne + 1), dtype=torch.float64, device=dev)     # [t = 0 and the snapshots][u, v]
        gram = torch.empty((ns + 1, 2, 2, 2), dtype=torch.float64, device=dev)
        MZ, KZ = (torch.empty((2, ne + 1), dtype=torch.float64, device=dev) for _ in range(2))
        ework = ops._scratch(None, ops._capi.load().lssvr_eig_work_bytes(ne, 2), dev)
        self._wave_first_accel(p, D, damped, SZ[0], MZ, KZ, gram[0], ework, VA[0, 0], VA[0, 1:2])
        cur, new, pr = 0, 1, 0
        ops.wave_advance(None, U[cur:cur + 1], VA[pr, 0:1], VA[pr, 1:2], md, mo, dd, do, loads, phi[1:2], dt, beta,
                         gamma, rhs_out=b)
        # the loop: launches on the current stream only
        for step in range(1, nsteps + 1):
            ops.tridiag_bc_solve_multi(ad, ao, b, kinds, kappa, g[step:step + 1], out=U[new:new + 1], work=work)
            last = step == nsteps
            ops.wave_advance(U[new:new + 1], U[cur:cur + 1], VA[pr, 0:1], VA[pr, 1:2], md, mo, dd, do, loads,
                             None if last else phi[step + 1:step + 2], dt, beta, gamma, V_out=VA[1 - pr, 0:1],
                             Acc_out=VA[1 - pr, 1:2], rhs_out=None if last else b, rhs=not last)
            cur, new, pr = new, cur, 1 - pr
            k = snap.get(step)
            if k is not None:
                SZ[k + 1, 0].copy_(U[cur])
                SZ[k + 1, 1].copy_(VA[pr, 0])
                SA[k].copy_(VA[pr, 1])
                ops.eig_apply(kd, ko, md, mo, SZ[k + 1], ekinds, ekap, MZ=MZ, KZ=KZ, gram=gram[k + 1], work=ework)
                if enhance:
                    # f - rho I_h acc: alpha = 1, beta0 = beta1 = 0, inv_dt = 1 leave U2 as it is (U0 is read, times 0)
                    ops.ts_source_table(SA[k], SA[k], None, ftab, rtab, phi[step], 1.0, 0.0, 0.0, 1.0, point_major=pm,
                                        out=tmp[0] if damped else src[k])
                    if damped:           # ... - d I_h v: the table so far is the single term, phi = 1
                        ops.ts_source_table(SZ[k + 1, 1], SZ[k + 1, 1], None, tmp, D.tab["d"], one, 1.0, 0.0, 0.0, 1.0,
                                            point_major=pm, out=src[k])
        enhanced = self._enhance_snapshots(p, D, SZ[1:, 0].contiguous()) if enhance else []
        # one copy: the snapshots, the energies and the bands
        host = _read_back(sz=SZ, accel=SA, gram=gram, loads=loads, damp=D.bands.get("damp"),
                          **{k: D.bands[k] for k in ("mass", "stiff", "step")})
        sz, gr = host["sz"], host["gram"]
        energy = 0.5 * (gr[:, 1, 1, 1] + gr[:, 0, 0, 0])
        return WaveSolution(p.times[steps].copy(), sz[1:, 0].copy(), sz[1:, 1].copy(), host["accel"], energy, enhanced,
                            {k: host[k] for k in ("mass", "stiff", "step", "damp", "loads")})

    # ---- adjoint sensitivities of the Newmark loop (no reference counterpart) -----------------
    def solve_wave_sensitivity(self, u0, v0, t_end, *, nsteps, goal=None, observe=None, goal_steps=None, damping=None,
                               weight=None, forcing=None, end_data=None, end_accel0=None, beta=0.25, gamma=0.5,
                               max_state_bytes=2 ** 31):
        """Derivatives of a functional J of the trajectory of :meth:`solve_wave` (same ``u0``, ``v0``, ``t_end``,
        ``nsteps``, ``damping``, ``weight``, ``forcing``, ``end_data``, ``end_accel0``, ``beta``, ``gamma``) with
        respect to the data of the loop, by the discrete adjoint: exact for the discrete scheme, at the cost of one
        more loop of the same length.  ``goal``: a callable j(x), J = sum_k int j u^{n_k} dx by the quadrature rule of
        the assembly, over ``goal_steps`` (default ``[nsteps]``); or ``observe=(steps, x_obs, d_obs)`` with d_obs
        [len(steps), nobs]: the misfit J = 1/2 sum_k sum_i (u^{n_k}(x_i) - d_ki)^2 at points inside the mesh.  Steps
        are 0 .. nsteps: u^0 counts.

        The forward loop is :meth:`solve_wave`'s, bit for bit, writing every u^n and acc^n (and v^n with ``damping``)
        into stored trajectories [nsteps+1, ne+1].  The rows p_n = dJ/du^n that are not zero are uploaded once (for a
        misfit they are formed on the host from the observed steps, one read-back between the loops).  The backward
        sweep runs the levels nsteps .. 1 in chunks of up to 8: per level ``ops.tridiag_bc_solve_multi`` on the step's
        bands with zero end data into the chunk's rows and ONE ``ops.newmark_adjoint_advance``, which writes the bars
        of the level below and the next right-hand side; then ONE ``ops.newmark_sensitivity`` per chunk adds the chunk
        to the tables.  Two chunk buffers alternate.  Level 0 solves on the M_rho bands and is a chunk of its own; two
        ``ops.eig_apply`` products (one without damping) give K lambda^0 and M_d lambda^0 for dJ/du0 and dJ/dv0, and
        one read-back fetches everything.  Neither loop synchronises or copies from the host.  Returns a
        :class:`WaveSensitivity`; the solver's attributes are left as they are.

        Refused (``ValueError``, before any device call): what :meth:`solve_wave` refuses, both or neither of ``goal``
        and ``observe``, a step outside 0 .. nsteps or named twice, data of the wrong shape or not finite, and
        trajectories of more than ``max_state_bytes``: checkpointing is not built."""
        self._check_fem_order("solve_wave_sensitivity")
        self._check_nonlinear("solve_wave_sensitivity")
        p = self._check_wave(u0, v0, t_end, nsteps, damping, weight, forcing, end_data, end_accel0, None, False, beta,
                             gamma)
        damped = damping is not None
        jsteps, rows, functional = self._check_transient_sensitivity(p, goal, goal_steps, None, observe,
                                                                     max_state_bytes, "solve_wave_sensitivity", 0,
                                                                     3 if damped else 2)
        kinds, kappa, dt, q, beta, gamma = p.kinds, p.kappa, p.dt, p.quad, p.beta, p.gamma
        # ---- the device from here on
        torch = _torch()
        nsteps, ne = int(nsteps), p.nodes.size - 1
        D = self._time_setup(p, False, [("stiff", True, q["c"]), ("mass", False, q["rho"]),
                                        *([("damp", False, q["d"])] if damped else []), ("step", True, p.shift)],
                             nbuf=nsteps + 1)
        dev, x, U, b, loads, work, phi, g = D.dev, D.x, D.U, D.b, D.loads, D.work, D.phi, D.g
        (kd, ko), (md, mo), (ad, ao) = D.bands["stiff"], D.bands["mass"], D.bands["step"]
        dd, do = D.bands["damp"] if damped else (None, None)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)      # noqa: E731
        At = new(nsteps + 1, ne + 1)
        Vt = new(nsteps + 1 if damped else 2, ne + 1)           # without damping two rows alternate
        vrow = (lambda n: n) if damped else (lambda n: n % 2)
        SZ, MZ, KZ, gram = new(2, ne + 1), new(2, ne + 1), new(2, ne + 1), new(2, 2, 2)
        ework = ops._scratch(None, ops._capi.load().lssvr_eig_work_bytes(ne, 2), dev)
        self._wave_first_accel(p, D, damped, SZ, MZ, KZ, gram, ework, Vt[0], At[0:1])
        # the forward loop of solve_wave, every state kept: row n of U, At (and Vt) is the state at t_n
        ops.wave_advance(None, U[0:1], Vt[0:1], At[0:1], md, mo, dd, do, loads, phi[1:2], dt, beta, gamma, rhs_out=b)
        for n in range(1, nsteps + 1):
            ops.tridiag_bc_solve_multi(ad, ao, b, kinds, kappa, g[n:n + 1], out=U[n:n + 1], work=work)
            last, vo, vn = n == nsteps, vrow(n - 1), vrow(n)
            ops.wave_advance(U[n:n + 1], U[n - 1:n], Vt[vo:vo + 1], At[n - 1:n], md, mo, dd, do, loads,
                             None if last else phi[n + 1:n + 2], dt, beta, gamma, V_out=Vt[vn:vn + 1],
                             Acc_out=At[n:n + 1], rhs_out=None if last else b, rhs=not last)
        jidx, P, prow = _functional_rows(U, jsteps, rows, functional)     # the rows p_n that are not zero
        prow = {n: P[k] for n, k in prow.items()}
        chunk = ops.NM_SENS_CHUNK
        Zb, Bb = new(2, chunk, ne + 1), new(2, chunk, ne + 1)
        bars = torch.zeros((2, 2, ne + 1), dtype=torch.float64, device=dev)      # [pair][vbar, abar]; level N: zeros
        ub = new(ne + 1)
        step_ends, mass_ends = (torch.stack((off[0], off[ne - 1])) for off in (ao, mo))
        want = tuple(k for k in ops.NM_SENS_TABLES if k != "d" or damped)
        out = dict(g=torch.zeros((nsteps + 1, 2), dtype=torch.float64, device=dev))
        sens = dict(want=want, Vtraj=Vt if damped else None, Atraj=At, phi=phi, end_kinds=kinds)
        # the backward sweep: launches on the current stream only
        ops.newmark_adjoint_advance(None, bars[0, 0], bars[0, 1], None, None, None, None, dt, beta, gamma,
                                    P=prow.get(nsteps), out=dict(b=Bb[0, 0]))
        pr = 0
        for hi, m, side in _sweep_chunks(nsteps, chunk):
            Z, B = Zb[side, :m], Bb[side, :m]
            for i in range(m):
                n = hi - i - 1                                 # lambda^{n+1} and the bars of level n+1 -> level n
                ops.tridiag_bc_solve_multi(ad, ao, B[i:i + 1], kinds, kappa, None, out=Z[i:i + 1], work=work)
                bufs = dict(v=bars[1 - pr, 0], a=bars[1 - pr, 1])
                if n == 0:
                    bufs["u"] = ub
                else:
                    bufs["b"] = B[i + 1] if i + 1 < m else Bb[1 - side, 0]
                ops.newmark_adjoint_advance(Z[i], bars[pr, 0], bars[pr, 1], md, mo, dd, do, dt, beta, gamma,
                                            P=prow.get(n), want_u=n == 0, want_b=n > 0, out=bufs)
                pr = 1 - pr
            out = ops.newmark_sensitivity(x, U, Z, hi - m + 1, self.nquad, Brows=B, band_ends=step_ends,
                                          accumulate=hi < nsteps, out=out, **sens)
        # level 0: M_rho lambda^0 = abar, a Robin end as a natural row; a chunk of its own, in the other buffer
        Z0, A0 = Zb[1 - side, 0:1], bars[pr, 1:2]
        ops.tridiag_bc_solve_multi(md, mo, A0, kinds, (0.0, 0.0), None, out=Z0, work=work)
        out = ops.newmark_sensitivity(x, U, Z0, 0, self.nquad, Brows=A0, band_ends=mass_ends, accumulate=True, out=out,
                                      **sens)
        ekinds, ekap = self._wave_energy_ends(p)
        ework1 = ops._scratch(None, ops._capi.load().lssvr_eig_work_bytes(ne, 1), dev)
        _, KL, _ = ops.eig_apply(kd, ko, md, mo, Z0, ekinds, ekap, work=ework1)
        DL = ops.eig_apply(kd, ko, dd, do, Z0, ekinds, ekap, work=ework1)[0] if damped else None
        host = _read_back(ub=ub, vb=bars[pr, 0], kl=KL, dl=DL, u=U[jidx], **out)
        value, _ = functional(host["u"])
        d_u0 = host["ub"] - host["kl"][0]
        d_v0 = host["vb"] - host["dl"][0] if damped else host["vb"].copy()
        d_g, d_acc = host["g"].copy(), np.zeros(2)
        for s, end, was in _dirichlet_u0(kinds, d_u0, d_g):
            d_acc[s] = was                                      # what the pass wrote there is dJ/d(acc^0_end)
            if not callable(p.end_data[s]):
                d_v0[end] = 0.0
        return WaveSensitivity(value, {k: host[k].copy() for k in want}, d_u0, d_v0, d_g, host["kappa"].copy(), d_acc,
                               p.times.copy(), p.nodes)

    # ---- Dual.py:176-203 --------------------------------------------------------------
    def evaluate_solution(self, x_points):
        """Evaluate the hybrid solution at given points (float64 result; the
        reference's ``zeros_like`` dtype trap for integer input is not reproduced)."""
        if self.enhanced is None:
            raise RuntimeError("call solve() or solve_lssvr_subproblems() first")
        x_points = np.asarray(x_points)
        out = self.enhanced.evaluate(x_points.reshape(-1))
        return out.reshape(x_points.shape)

    def element_indices(self, x_points):
        """Element each query point is evaluated in (Dual.py:182-201 rule)."""
        _, elem = self.enhanced.evaluate(np.asarray(x_points).reshape(-1), return_elements=True)
        return elem

    # ---- a posteriori error indicator and h-refinement (no reference counterpart) ------------
    def _estimate_dev(self, nq):
        """(eta2 device[ne], out3 device[3]) of the current enhanced solution."""
        if self.enhanced is None:
            raise RuntimeError("call solve() first")
        x, W = self.enhanced.nodes, self.enhanced.W
        eq = self._eq
        if self.nonlinear is not None:
            # the residual of the linear problem around the P1 interpolant of the nodal values
            u = _to_dev(self.fem_values, x.device)
            t = ops.estimate_points(_to_dev([0.0, 1.0], x.device), nq)[0].contiguous()
            ta, tda, tf, tc = self._nl_tables(ops.estimate_points(x, nq), "residual-indicator", t, True, u)
            eta2, _, out3 = ops.estimate_varcoef(x, W, nq, ta, tda, tf, eq.a_ends(x), point_major=True, c_values=tc)
        elif eq.poisson:
            eta2, _, out3 = ops.estimate(x, W, nq, **_rhs_mode(eq.f, lambda: ops.estimate_points(x, nq)))
        else:
            # a, a', f (, c) at the Gauss points, point-major (coalesced); a at the nodes from both sides, aL = aR
            ta, tda, tf, tc = eq.tables(ops.estimate_points(x, nq), True)
            eta2, _, out3 = ops.estimate_varcoef(x, W, nq, ta, tda, tf, eq.a_ends(x), point_major=True,
                                                 c_values=tc)
        bnd = self._bnd
        if bnd is not None:              # the boundary residual of the Neumann / Robin ends joins eta2 and out3
            ends = np.array([float(self.fem_nodes[0]), float(self.fem_nodes[-1])])      # (host copy of the nodes)
            a_ends = (1.0, 1.0) if eq.a is None else np.broadcast_to(np.asarray(eq.a(ends), dtype=np.float64), (2,))
            ops.estimate_ends(x, W, bnd.kinds, bnd.kappa, self._gd_bc()[1], a_ends, eta2, out3)
        if self._periodic:               # the flux jump across the seam joins eta2 and out3
            seam = np.array([float(self.fem_nodes[-1]), float(self.fem_nodes[0])])      # (host copy of the nodes)
            a_seam = (1.0, 1.0) if eq.a is None else np.broadcast_to(np.asarray(eq.a(seam), dtype=np.float64), (2,))
            ops.estimate_seam(x, W, a_seam, eta2, out3)
        return eta2, out3

    def _nq(self, nq):
        nq = max(int(self.lssvr_M), 8) if nq is None else int(nq)
        if not 1 <= nq <= 32:
            raise ValueError(f"nq must be in [1, 32], got {nq}")
        return nq

    def estimate(self, nq=None):
        """Per-element error indicator of the enhanced solution after ``solve()``, as numpy:
        eta_e^2 = h_e^2 int_e (f + u_e'')^2 dx + h_e/2 (J_e^2 + J_{e+1}^2), J = jump of u' at the
        nodes (0 at the Dirichlet ends), ``nq``-point Gauss (default max(lssvr_M, 8)).  With ``coef = (a, da)``
        the residual is f + a u_e'' + a' u_e' and J the jump of the flux a u' (a at the nodes from both sides:
        a callable coefficient is continuous there; ``ops.estimate_varcoef`` takes one-sided values); with
        ``reaction = c`` the residual is f + a u_e'' + a' u_e' - c u_e."""
        nq = self._nq(nq)
        eta2, _ = self._estimate_dev(nq)
        return eta2.cpu().numpy()

    # ---- goal-oriented estimation: the dual-weighted residual (no reference counterpart) ------------
    def _check_goal(self, goal):
        """What :meth:`solve_goal` needs, checked on the host before any GPU use."""
        if not callable(goal):
            raise ValueError("goal must be a callable j(x): the density of J(u) = int j u dx")
        if self._periodic:
            raise ValueError("goal needs Dirichlet, Neumann or Robin ends: the dual-weighted residual has no seam "
                             "term, boundary='periodic' is not supported")
        if self.convection is not None:
            raise ValueError("goal needs an operator without convection: the adjoint of -(a u')' + b u' + c u has "
                             "-b and c - b', another matrix than the primal's")
        if self.solver_id != ops.SOLVER_PRIMAL:
            raise ValueError("goal needs solver=ops.SOLVER_PRIMAL: the primal and the dual solution share one "
                             "factorisation through solve_many")
        if self.fem_solver == "flux" and self._bnd is not None:
            raise ValueError("goal with a Neumann or Robin end needs fem_solver='bands'")
        if self.element_degrees is not None:
            raise ValueError("goal needs one degree for all elements (element_degrees is set, e.g. by "
                             "solve_adaptive(mode='hp')): solve_many and the dual-weighted residual take one lssvr_M")

    def _goal_nq(self, nq):
        """Gauss points of the goal path: min(32, max(2 lssvr_M, 16)) unless given.  More than :meth:`estimate`'s
        max(lssvr_M, 8): eta_e is SIGNED, so the quadrature error of int R z does not hide under a square -- where f
        has a layer that 8 points do not resolve it is as large as the correction itself."""
        return self._nq(min(32, max(2 * int(self.lssvr_M), 16)) if nq is None else nq)

    def solve_goal(self, goal, nq=None):
        """Solve for ``rhs`` and for the dual problem of the quantity of interest J(u) = int ``goal`` u dx in one
        :meth:`solve_many` (same matrix: no convection), then weight the residual of the enhanced primal solution with
        the enhanced dual solution (``ops.estimate_goal``, ``nq``-point Gauss, default min(32, max(2 lssvr_M, 16))).
        The dual case has zero end data: the value 0 at a Dirichlet end, g = 0 at a Neumann or Robin end.  Afterwards
        ``fem_nodes``,
        ``fem_values``, ``enhanced`` and ``lssvr_functions`` hold the primal case as after ``solve()`` and ``dual``
        the dual :class:`EnhancedSolution`.  Returns a :class:`GoalEstimate`: ``value`` = J(u_enh), ``correction`` =
        sum eta_e, ``corrected`` = their sum -- the enhanced solution is continuous and takes the Dirichlet values, so
        sum eta_e = J(u) - J(u_enh) up to the error of the dual solution and of the ``nq``-point rule on R z: the
        correction is only as good as that rule resolves f."""
        self._check_fem_order("solve_goal")
        self._check_nonlinear("solve_goal")
        return self._solve_goal(goal, nq)[0]

    def _solve_goal(self, goal, nq):
        """:meth:`solve_goal` -> (its GoalEstimate, marking): ``marking()`` is a second launch on the same tables in
        the jump-free form -> (eta2 device [ne], out4 device [4]) of eta_e = int_e R (z_e - I_h z_e)."""
        self._check_goal(goal)
        nq = self._goal_nq(nq)
        bc0 = self._gd_bc()[1]
        (primal, dual), x, U = self._solve_many([self.rhs, goal], [bc0, (0.0, 0.0)])
        eq = self._eq
        pts = ops.estimate_points(x, nq)
        ta, tda, tf, tc = eq.tables(pts, True)
        tj = _tabulate(goal, pts, True)
        nodes = x.cpu().numpy()
        kw = {}
        bnd = self._bnd
        if bnd is not None:
            ends = nodes[[0, -1]]
            a_bnd = (1.0, 1.0) if eq.a is None else np.broadcast_to(np.asarray(eq.a(ends), dtype=np.float64), (2,))
            kw = dict(end_kinds=bnd.kinds, kappa=bnd.kappa, g=bc0, a_bnd=a_bnd)
        a_ends = eq.a_ends(x)
        eta, eta2, out4 = ops.estimate_goal(x, primal.W, dual.W, nq, ta, tda, tf, tj, a_ends, c_values=tc,
                                            point_major=True, **kw)

        def marking():
            return ops.estimate_goal(x, primal.W, dual.W, nq, ta, tda, tf, tj, a_ends, c_values=tc,
                                     point_major=True, jump_free=True, **kw)[1:]

        self._x_dev, self._u_dev = x, U[0]
        self.fem_nodes = nodes
        self.fem_values = U[0].cpu().numpy()
        self.enhanced, self.dual = primal, dual
        self._report_fallbacks()
        self.lssvr_functions = _ElementFunctions(nodes, primal.W)
        return GoalEstimate(eta, eta2, out4), marking

    # ---- adjoint sensitivities of the P1 solve (no reference counterpart) ------------------
    def _check_sensitivity(self, goal, observe, what="solve_sensitivity", semilinear=False):
        """What :meth:`solve_sensitivity` needs, on the host and before any device call -> (nodes, functional):
        ``functional(u)`` -> (J, p = dJ/du) for the nodal vector u.  ``what``: the caller's name in the messages;
        ``semilinear``: the caller differentiates the Newton solve, so ``nonlinear=`` is not refused."""
        if self._periodic:
            raise ValueError(f"{what} has no boundary='periodic': the adjoint solve and the end gradients "
                             "are written for Dirichlet, Neumann and Robin ends")
        if self.fem_solver == "flux":
            raise ValueError(f"{what} needs fem_solver='bands' or 'pivot': the adjoint is the transposed "
                             "tridiagonal solve, which the flux solve does not have")
        if not semilinear:
            self._check_nonlinear(what)
        if self.solver_id != ops.SOLVER_PRIMAL:
            raise ValueError(f"{what} needs solver=ops.SOLVER_PRIMAL: the derivatives are those of the P1 "
                             "solve, the enhancement is not differentiated")
        if self.element_degrees is not None:
            raise ValueError(f"{what} has no element_degrees: the derivatives are those of the P1 solve, "
                             "which has no degree")
        if (goal is None) == (observe is None):
            raise ValueError(f"{what} needs exactly one of goal (a callable j(x): J = int j u dx) and "
                             "observe = (x_obs, d_obs) (J = 1/2 sum (u_h(x_i) - d_i)^2)")
        m = self._default_mesh() if self.mesh is None else self.mesh
        nodes = np.asarray(m.nodes, dtype=np.float64)
        h = np.diff(nodes)
        xi, w = np.polynomial.legendre.leggauss(int(self.nquad))
        xi, w = 0.5 * (1.0 + xi), 0.5 * w
        xq = nodes[:-1, None] + h[:, None] * xi[None, :]
        eq = self._eq
        named = [("rhs", eq.f), ("coef a", eq.a), ("convection", eq.b), ("reaction", eq.c)]
        if goal is not None:
            if not callable(goal):
                raise ValueError("goal must be a callable j(x): the density of J(u) = int j u dx")
            named.append(("goal", goal))
        tabs = {}
        for label, fn in named:
            if fn is None:
                continue
            try:
                t = np.broadcast_to(np.asarray(fn(xq), dtype=np.float64), xq.shape)
            except ValueError:
                raise ValueError(f"{label} must return one value per point ({list(xq.shape)} at the quadrature "
                                 "points) or a value that broadcasts to them") from None
            if not np.all(np.isfinite(t)):
                raise ValueError(f"{label} is not finite at a quadrature point")
            tabs[label] = t
        self._check_finite(("the end data", np.asarray(self._gd_bc()[1], dtype=np.float64)))
        if goal is not None:
            # p = the P1 load of j by the rule of the assembly: J = int j u_h dx = p . u
            p = np.zeros(nodes.size)
            p[:-1] += h * ((tabs["goal"] * w) @ (1.0 - xi))
            p[1:] += h * ((tabs["goal"] * w) @ xi)
            return nodes, lambda u: (float(p @ u), p)
        if not isinstance(observe, (tuple, list)) or len(observe) != 2:
            raise ValueError("observe must be a pair (x_obs, d_obs)")
        xo, d = (np.asarray(t, dtype=np.float64).reshape(-1) for t in observe)
        if xo.size < 1 or xo.size != d.size:
            raise ValueError(f"observe must hold as many points as data, at least one, got {xo.size} and {d.size}")
        self._check_finite(("observe x_obs", xo), ("observe d_obs", d))
        if xo.min() < nodes[0] or xo.max() > nodes[-1]:
            raise ValueError(f"observe: every x_obs must lie in the mesh [{nodes[0]:.6g}, {nodes[-1]:.6g}]")
        e = np.clip(np.searchsorted(nodes, xo, side="right") - 1, 0, nodes.size - 2)
        t = (xo - nodes[e]) / h[e]

        def misfit(u):
            r = u[e] * (1.0 - t) + u[e + 1] * t - d
            p = np.zeros(nodes.size)
            np.add.at(p, e, r * (1.0 - t))
            np.add.at(p, e + 1, r * t)
            return 0.5 * float(r @ r), p
        return nodes, misfit

    def _adjoint_solve(self, bands, P, kinds, kappa):
        """Z [nc, ne+1] of the TRANSPOSED bands with the loads P, zero end data and the primal's ends, through the
        solver the primal took."""
        ab = ops.adjoint_bands(bands)
        if self.fem_solver == "pivot":
            sub, sup = (ab["sub"], ab["sup"]) if "sub" in ab else (ab["off"], ab["off"])
            z, info = ops.tridiag_pivot_solve_multi(ab["diag"], sub, sup, P, kinds, kappa, None, return_info=True)
            bad = int(info.item())
            if bad:
                raise RuntimeError(f"adjoint system singular to working precision: the pivoting tridiagonal solve "
                                   f"met {bad} pivot(s) that were zero or not finite")
            return z
        if "sub" in ab:
            return ops.tridiag_ns_bc_solve_multi(ab["diag"], ab["sub"], ab["sup"], P, kinds, kappa, None)
        return ops.tridiag_bc_solve_multi(ab["diag"], ab["off"], P, kinds, kappa, None)

    # ---- sensitivities of the ENHANCED solution ----------------------------------------------
    def _check_sensitivity_enhanced(self, goal, observe):
        """What ``solve_sensitivity(of="enhanced")`` needs beyond :meth:`_check_sensitivity`, on the host and before
        any device call -> (nodes, functional): ``functional(W)`` -> (J, Wbar = dJ/dW) for the coefficients W [ne, M]."""
        nodes, _ = self._check_sensitivity(goal, observe)
        M, n = int(self.lssvr_M), int(self.n_colloc)
        if not ops.ENH_ADJ_MIN_M <= M <= ops.ENH_ADJ_MAX_M:
            raise ValueError(f"solve_sensitivity(of='enhanced') needs {ops.ENH_ADJ_MIN_M} <= lssvr_M <= "
                             f"{ops.ENH_ADJ_MAX_M} (the lane kernel of the adjoint), got {M}")
        if not max(2, M - 2) <= n <= ops.ENH_ADJ_MAX_COLLOC:
            raise ValueError(f"solve_sensitivity(of='enhanced') needs max(2, lssvr_M - 2) <= n_colloc <= "
                             f"{ops.ENH_ADJ_MAX_COLLOC}, got {n}")
        if self.element_lists:
            raise ValueError("solve_sensitivity(of='enhanced') has no element_lists: one degree, one launch")
        h = np.diff(nodes)
        vander = np.polynomial.legendre.legvander

        def local(e, xo):
            """L_p at the local coordinate of the points xo of the elements e [len(xo), M]."""
            return vander((2.0 * xo - nodes[e] - nodes[e + 1]) / h[e], M - 1)

        if goal is not None:
            # J = int j u_enh dx by the Gauss rule of the estimators on every element: linear in W
            xi, w = np.polynomial.legendre.leggauss(self._nq(None))
            xq = 0.5 * (nodes[:-1] + nodes[1:])[:, None] + 0.5 * h[:, None] * xi[None, :]
            try:
                jq = np.broadcast_to(np.asarray(goal(xq), dtype=np.float64), xq.shape)
            except ValueError:
                raise ValueError(f"goal must return one value per point ({list(xq.shape)}) or a value that "
                                 "broadcasts to them") from None
            if not np.all(np.isfinite(jq)):
                raise ValueError("goal is not finite at a quadrature point")
            e = np.repeat(np.arange(h.size), xi.size)
            Wbar = np.einsum("eq,eqm->em", jq * (0.5 * h[:, None] * w[None, :]),
                             local(e, xq.ravel()).reshape(h.size, xi.size, M))
            return nodes, lambda W: (float(np.sum(Wbar * W)), Wbar)
        xo, d = (np.asarray(t, dtype=np.float64).reshape(-1) for t in observe)
        e = np.clip(np.searchsorted(nodes, xo, side="right") - 1, 0, nodes.size - 2)
        P = local(e, xo)

        def misfit(W):
            r = np.sum(P * W[e], axis=1) - d
            Wbar = np.zeros(W.shape)
            np.add.at(Wbar, e, r[:, None] * P)
            return 0.5 * float(r @ r), Wbar
        return nodes, misfit

    def _solve_sensitivity_enhanced(self, goal, observe):
        nodes, functional = self._check_sensitivity_enhanced(goal, observe)
        self.solve_fem()
        x, u, bands = self._x_dev, self._u_dev, self.bands
        M, gamma, n = int(self.lssvr_M), float(self.lssvr_gamma), int(self.n_colloc)
        gd, bc = self._gd_bc()
        shard = self._shard(nodes.size - 1)
        eq = self._eq
        # the forward call on ELEMENT-MAJOR tables (the layout of the adjoint), whatever solve() would take
        ta, tda, tf, tc = eq.tables(ops.colloc_points(x, n), False)
        W, st = ops.enhance_varcoef(x, u, M, gamma, n, ta, tda, tf, global_domain=gd, bc=bc, c_values=tc, **shard)
        Wh = W.cpu().numpy()                    # (a misfit's Wbar depends on W: the one copy besides the results')
        value, Wbar = functional(Wh)
        want = ("u", "bc", "a", "da", "f") + (("c",) if tc is not None else ())
        adj = ops.enhance_adjoint(x, W, _to_dev(Wbar, x.device), M, gamma, n, tf, a_values=ta, da_values=tda,
                                  c_values=tc, status=st, want=want, global_domain=gd, **shard)
        bnd = self._bnd
        kinds, kappa = ((ops.END_DIRICHLET,) * 2, (0.0, 0.0)) if bnd is None else (tuple(bnd.kinds), tuple(bnd.kappa))
        P = adj["u"].view(1, -1)
        Z = self._adjoint_solve(bands, P, kinds, kappa)
        p1want = tuple(k for k, on in zip(ops.SENS_TABLES, (True, eq.b is not None, eq.c is not None, True)) if on)
        res = ops.p1_sensitivity(x, u, Z, self.nquad, want=p1want, P=P, bands=bands, end_kinds=kinds)
        host = _read_back(z=Z, **res, **{"enh_" + k: v for k, v in adj.items()})
        ends = host["ends"][0].copy()
        ends[:2] += host["enh_bc"]
        s = Sensitivity(value, {k: host[k][0] for k in p1want}, ends, host["z"][0], nodes)
        s.d_rhs_colloc, s.d_coef_colloc, s.d_dcoef_colloc = host["enh_f"], host["enh_a"], host["enh_da"]
        s.d_reaction_colloc = host.get("enh_c")
        s.d_convection_colloc = None if eq.b is None else -host["enh_da"]
        s.enhanced = Wh
        return s

    def solve_sensitivity(self, goal=None, *, observe=None, of="p1"):
        """``of="enhanced"``: the functional is one of the ENHANCED solution u_enh = sum_p W[e, p] L_p -- J = int j u_enh
        dx by the Gauss rule of :meth:`estimate` on every element, or the misfit 1/2 sum_i (u_enh(x_i) - d_i)^2 -- and
        the chain runs one stage further: the forward enhancement on element-major tables, Wbar = dJ/dW formed on the
        host and uploaded once, ONE ``ops.enhance_adjoint``, whose nodal gradient is the load of the adjoint solve, then
        ONE ``ops.p1_sensitivity`` and one read-back.  The :class:`Sensitivity` then also holds ``d_rhs_colloc``,
        ``d_coef_colloc``, ``d_dcoef_colloc`` (the first-derivative table a' - b), ``d_reaction_colloc`` and
        ``d_convection_colloc`` = -``d_dcoef_colloc`` [ne, n_colloc] (None where the solver has no such term), and
        ``d_end_values`` of a Dirichlet end is the sum of the P1 part and of the enhancement's own.  Refused besides what
        is refused below: ``lssvr_M`` outside 3 .. 16, ``n_colloc`` outside max(2, lssvr_M - 2) .. 64,
        ``element_lists``.  ``of="p1"`` (the default) is the path below, untouched.

        Derivatives of a functional J of the P1 solution with respect to the data of the solve, by the adjoint
        method: ONE :meth:`solve_fem`, ONE adjoint solve -- the same tridiagonal solver on the transposed bands
        (``ops.adjoint_bands``) with load p = dJ/du, zero end data and the same end kinds and kappa -- and ONE
        ``ops.p1_sensitivity``.  ``goal``: a callable j(x), J(u) = int j u_h dx by the quadrature rule of the assembly;
        or ``observe=(x_obs, d_obs)``: the misfit J = 1/2 sum_i (u_h(x_i) - d_i)^2 at points inside the mesh (p is
        formed on the host: a few hundred points at most).  Convection is handled: the transposed solve is what
        :meth:`solve_goal` lacks.  Returns a :class:`Sensitivity`; ``fem_nodes`` and ``fem_values`` hold the primal
        solution as after :meth:`solve_fem`.  Refused (``ValueError``, before any device call): ``boundary="periodic"``,
        ``fem_solver="flux"``, ``nonlinear=``, a solver other than ``ops.SOLVER_PRIMAL``, ``element_degrees``, both or
        neither of ``goal`` and ``observe``, data that are not finite where they are tabulated.  The mesh is not
        differentiated."""
        self._check_fem_order("solve_sensitivity")
        if of not in ("p1", "enhanced"):
            raise ValueError(f"of must be 'p1' or 'enhanced', got {of!r}")
        if of == "enhanced":
            return self._solve_sensitivity_enhanced(goal, observe)
        nodes, functional = self._check_sensitivity(goal, observe)
        self.solve_fem()
        x, u, bands = self._x_dev, self._u_dev, self.bands
        value, p = functional(self.fem_values)
        bnd = self._bnd
        kinds, kappa = ((ops.END_DIRICHLET,) * 2, (0.0, 0.0)) if bnd is None else (tuple(bnd.kinds), tuple(bnd.kappa))
        P = _to_dev(p[None, :], x.device)
        Z = self._adjoint_solve(bands, P, kinds, kappa)
        eq = self._eq
        want = tuple(k for k, on in zip(ops.SENS_TABLES, (True, eq.b is not None, eq.c is not None, True)) if on)
        res = ops.p1_sensitivity(x, u, Z, self.nquad, want=want, P=P, bands=bands, end_kinds=kinds)
        host = _read_back(z=Z, **res)
        return Sensitivity(value, {k: host[k][0] for k in want}, host["ends"][0], host["z"][0], nodes)

    # ---- adjoint sensitivities of the semilinear P1 solve (no reference counterpart) ----------
    def solve_semilinear_sensitivity(self, goal=None, *, observe=None, u_init=None, tol=None, max_iter=None):
        """:meth:`solve_sensitivity` for a solver with ``nonlinear=``: derivatives of a functional J of the converged
        Newton solution u* of -(a u')' + b u' + c u + g(x, u) = f with respect to the data of the solve, the tables
        q_k(x) of g among them.  ONE :meth:`solve_fem` (``u_init``, ``tol``, ``max_iter`` are its Newton keywords), ONE
        ``ops.nl_linearize`` AT u* for c_eff = c + g_u(x, u*_h), ONE ``ops.p1_assemble`` with it -- the Newton Jacobian;
        ``self.bands`` is not reused, it is linearised at the previous iterate --, ONE adjoint solve on its transposed
        bands, ONE ``ops.nl_sensitivity`` and one read-back.  ``goal`` / ``observe`` as for :meth:`solve_sensitivity`.
        Returns a :class:`Sensitivity` that also holds ``d_nonlinear`` [nterm, ne, nquad] = dJ/dq_k at quadrature point
        q of element e and ``newton``, the :class:`NewtonReport` of the solve; ``d_end_values`` of a Dirichlet end takes
        the Jacobian's band entry.  ``fem_solver="pivot"`` where c + g_u < 0.  Refused (``ValueError``, before any
        device call): a solver without ``nonlinear=``, what :meth:`solve_sensitivity` refuses other than ``nonlinear=``,
        what ``nonlinear=`` refuses, Newton keywords :meth:`solve_fem` refuses.  ``of="enhanced"``, the semilinear
        time loop, periodic ends and the mesh are not differentiated."""
        self._check_fem_order("solve_semilinear_sensitivity")
        what = "solve_semilinear_sensitivity"
        if self.nonlinear is None:
            raise ValueError(f"{what} needs nonlinear=: the linear solve is differentiated by solve_sensitivity")
        nodes, functional = self._check_sensitivity(goal, observe, what, semilinear=True)
        nl = self._check_nonlinear()
        self.solve_fem(u_init=u_init, tol=tol, max_iter=max_iter)
        x, u = self._x_dev, self._u_dev
        value, p = functional(self.fem_values)
        bnd = self._bnd
        kinds, kappa = ((ops.END_DIRICHLET,) * 2, (0.0, 0.0)) if bnd is None else (tuple(bnd.kinds), tuple(bnd.kappa))
        # the Jacobian at u*: the tables of the Newton loop, linearised once more
        _, _, xq, kw = self._fem_setup()
        fq = _tabulate(self._eq.f, xq)
        qq = nl.tables(xq, "quadrature")
        t = ops.quad_points(_to_dev([0.0, 1.0], x.device), self.nquad)[0].contiguous()
        c_eff = ops.nl_linearize(u, t, nl.kind, qq, fq, c_tab=kw.get("c_quad"), f_eff=False)["c_eff"]
        if self.fem_solver != "pivot" and bool((c_eff < 0).any().item()):
            raise ValueError("c + g_u is negative at a quadrature point of the converged solution: the tridiagonal "
                             "solve of the adjoint does not pivot and assumes an SPD matrix; use fem_solver=\"pivot\"")
        jac = ops.p1_assemble(x, self.nquad, rhs_quad=fq, **{**kw, "c_quad": c_eff})
        P = _to_dev(p[None, :], x.device)
        Z = self._adjoint_solve(jac, P, kinds, kappa)
        eq = self._eq
        want = tuple(k for k, on in zip(ops.NL_SENS_TABLES, (True, eq.b is not None, eq.c is not None, True, True))
                     if on)
        res = ops.nl_sensitivity(x, u, Z, self.nquad, nl.kind, len(nl.q), q_tabs=qq, want=want, P=P, bands=jac,
                                 end_kinds=kinds)
        host = _read_back(z=Z, **res)
        s = Sensitivity(value, {k: host[k][0] for k in want}, host["ends"][0], host["z"][0], nodes)
        s.d_nonlinear, s.newton = host["q"][0], self.newton
        return s

    def _adapt_rounds(self, tol, max_elements, max_iter, round_fn, start=None):
        """The round loop of every ``solve_adaptive`` mode; host logic only, so a scripted ``round_fn`` can drive it.
        ``round_fn()`` solves and estimates on ``self.mesh`` -> (ne, estimate, the record's further fields, refine);
        ``refine()`` -> (the new nodes as a host array, what the refinement changes in the record: counts) or
        ``None`` for a veto of the mode's own.  It stops at ``tol``, after ``max_iter`` rounds (neither refines), at
        a veto, when every count is 0, or when the new mesh would exceed ``max_elements``; otherwise the record is
        updated and ``self.mesh`` becomes the new nodes.  ``start(ne)``: the mode's own check of the initial mesh,
        before ``adapt_history`` is reset.  Returns the last estimate."""
        if self.mesh is None:
            self.mesh = self._default_mesh()
        if self.mesh.nelements > max_elements:
            raise ValueError(f"the initial mesh has {self.mesh.nelements} elements > max_elements = {max_elements}")
        if start is not None:
            start(self.mesh.nelements)
        self.adapt_history = []
        est = float("nan")
        for it in range(max_iter):
            ne, est, fields, refine = round_fn()
            rec = dict(ne=ne, estimate=est, **fields)
            self.adapt_history.append(rec)
            if (tol is not None and est <= float(tol)) or it + 1 == max_iter:
                break
            out = refine()
            if out is None:
                break
            nodes, counts = out
            if not any(counts.values()) or len(nodes) - 1 > max_elements:
                break
            rec.update(counts)
            self.mesh = LineMesh.from_nodes(nodes)
        return est

    def _refine_h(self, ne, eta2, eta2_max, theta, h_min):
        """``refine()`` of the modes that only bisect (:meth:`_adapt_rounds`)."""
        x_new, _ = ops.refine(self.enhanced.nodes, eta2, eta2_max, theta, h_min=h_min)
        return x_new.cpu().numpy(), dict(marked=x_new.numel() - 1 - ne)

    def _solve_adaptive_goal(self, goal, tol, theta, max_elements, max_iter, h_min, nq):
        """The rounds of ``solve_adaptive(goal=j)``; the arguments it shares with the residual loop are validated."""
        nq = self._goal_nq(nq)

        def round_fn():
            ge, marking = self._solve_goal(goal, nq)
            ne = int(ge.eta.size)
            est = float(np.abs(ge.eta).sum()) if ge.n_nonfinite == 0 else float("inf")

            def refine():
                # marked from the jump-free form: half a jump at a node shared with a coarse neighbour stays as it is
                # however often the fine element is bisected, and the loop would stall on it
                mark2, mark4 = marking()
                return self._refine_h(ne, mark2, mark4[1:2], theta, h_min)
            return ne, est, dict(correction=ge.correction, value=ge.value, marked=0), refine
        return self._adapt_rounds(tol, max_elements, max_iter, round_fn)

    def solve_adaptive(self, tol=None, theta=0.5, max_elements=100000, max_iter=50, h_min=0.0, nq=None, *,
                       mode="h", M_max=None, dM=2, sigma_min=1.0, max_dof=None, goal=None):
        """Solve, estimate, mark, bisect -- repeated.  Each round runs ``solve()`` on the current mesh
        and the indicator of :meth:`estimate` (for ``-(a u')' = f`` when ``coef`` is set); it stops when
        sqrt(sum eta^2) <= ``tol``, after ``max_iter`` rounds, when nothing is marked, or when the refinement
        would take the mesh above
        ``max_elements`` (the final mesh never exceeds it); otherwise every element with
        eta_e >= ``theta`` * max eta (and at least 2 ``h_min`` long) is bisected and ``self.mesh``
        becomes the new nodes.  Afterwards ``fem_nodes``, ``fem_values``, ``lssvr_functions`` and
        ``enhanced`` describe the final mesh as after ``solve()``; ``adapt_history`` holds one
        dict(ne, estimate, marked) per round (marked = elements bisected after that round).
        Returns the final sqrt(sum eta^2).

        ``mode="hp"`` (``solver=ops.SOLVER_PRIMAL``; Poisson rows, or any rows with ``boundary="periodic"``, where each
        degree group runs through the table kernels over the whole mesh; with ``element_lists=True`` any of ``coef``,
        ``reaction``, ``convection`` and any ``boundary``, each degree group through the element lists of the table
        kernels): every element starts at ``lssvr_M``; a marked
        element whose Legendre coefficients decay at a rate ``ops.smoothness`` >= ``sigma_min`` gets ``dM`` more
        coefficients while that stays <= ``M_max`` (default min(33, lssvr_M + 12)), any other marked element is
        bisected and both halves keep its degree (``ops.refine_hp``).  ``element_degrees`` carries the degrees
        from round to round and describes the final mesh; the indicator takes ``nq`` = min(32, max(max M_e, 8))
        Gauss points unless given; every round records dict(ne, estimate, marked, raised, dof) with marked =
        elements bisected, raised = elements raised after that round and dof = sum of M_e.  It also stops when a
        round neither bisects nor raises, or when the refinement would take sum M_e above ``max_dof`` (hp only).

        ``goal=j`` (a callable; ``mode="h"``, no convection, ``solver=ops.SOLVER_PRIMAL``): refine for the quantity
        J(u) = int j u dx instead.  Each round is :meth:`solve_goal`; the elements are marked by the same rule from the
        square of the jump-free form of the dual-weighted residual, int_e R (z - I_h z) with I_h z the linear
        interpolant of the dual solution at the element's nodes (``ops.estimate_goal(jump_free=True)``: what bisecting
        the element itself reduces); a round's estimate is sum |eta_e| -- an upper bound of the
        correction |sum eta_e|, so cancellation between elements cannot stop the loop early -- and is what ``tol``
        is compared with and what is returned; ``adapt_history`` holds dict(ne, estimate, correction, value, marked)
        per round, value = J(u_enh) and correction = sum eta_e on that round's mesh."""
        self._check_nonlinear("solve_adaptive")
        if mode not in ("h", "hp"):
            raise ValueError(f"mode must be 'h' or 'hp', got {mode!r}")
        if mode != "h" or goal is not None:
            self._check_fem_order("solve_adaptive(mode='hp') / solve_adaptive(goal=)")
        if goal is not None:
            if mode != "h":
                raise ValueError("goal needs mode='h': the dual-weighted residual marks elements for bisection only")
            self._check_goal(goal)
        theta = float(theta)
        if not 0.0 <= theta <= 1.0:
            raise ValueError(f"theta must be in [0, 1], got {theta}")
        if isinstance(max_elements, bool) or int(max_elements) != max_elements or max_elements < 1:
            raise ValueError(f"max_elements must be a positive integer, got {max_elements!r}")
        if int(max_iter) != max_iter or max_iter < 1:
            raise ValueError(f"max_iter must be a positive integer, got {max_iter!r}")
        if tol is not None and not float(tol) >= 0.0:
            raise ValueError(f"tol must be >= 0, got {tol!r}")
        if not float(h_min) >= 0.0:
            raise ValueError(f"h_min must be >= 0, got {h_min!r}")
        if mode == "hp":
            return self._solve_adaptive_hp(tol, theta, max_elements, int(max_iter), float(h_min), nq, M_max, dM,
                                           sigma_min, max_dof)
        if max_dof is not None:
            raise ValueError("max_dof bounds sum M_e of mode='hp'; mode='h' is bounded by max_elements")
        if goal is not None:
            return self._solve_adaptive_goal(goal, tol, theta, int(max_elements), int(max_iter), float(h_min), nq)
        nq = self._nq(nq)

        def round_fn():
            self.solve()
            ne, est, eta2, out3 = self._estimate_round(nq)
            return ne, est, dict(marked=0), lambda: self._refine_h(ne, eta2, out3[1:2], theta, float(h_min))
        return self._adapt_rounds(tol, max_elements, int(max_iter), round_fn)

    def _estimate_round(self, nq):
        """(ne, sqrt(sum eta^2) or inf where an eta^2 is not finite, eta2 device [ne], out3 device [3]) of the
        residual indicator on the current enhanced solution."""
        eta2, out3 = self._estimate_dev(nq)
        s = out3.cpu().numpy()
        return int(eta2.numel()), (float(np.sqrt(s[0])) if s[2] == 0 else float("inf")), eta2, out3

    def _solve_adaptive_hp(self, tol, theta, max_elements, max_iter, h_min, nq, M_max, dM, sigma_min, max_dof):
        """The rounds of ``solve_adaptive(mode="hp")``; the arguments it shares with mode "h" are validated."""
        torch = _torch()
        self._check_hp("mode='hp'")
        M0 = int(self.lssvr_M)
        M_max = min(ops.MAX_DEGREE, M0 + 12) if M_max is None else M_max
        if isinstance(M_max, bool) or int(M_max) != M_max or not M0 <= M_max <= ops.MAX_DEGREE:
            raise ValueError(f"M_max must be an integer in [lssvr_M, 33] = [{M0}, 33], got {M_max!r}")
        if isinstance(dM, bool) or int(dM) != dM or dM < 1:
            raise ValueError(f"dM must be a positive integer, got {dM!r}")
        if math.isnan(float(sigma_min)):
            raise ValueError("sigma_min must not be NaN")
        if max_dof is not None and (isinstance(max_dof, bool) or int(max_dof) != max_dof or max_dof < 1):
            raise ValueError(f"max_dof must be a positive integer, got {max_dof!r}")
        if nq is not None:
            nq = self._nq(nq)
        deg = None                     # int64[ne]: the degrees of the current mesh, carried from round to round

        def start(ne):
            nonlocal deg
            deg = np.full(ne, M0, dtype=np.int64)
            if max_dof is not None and deg.sum() > max_dof:
                raise ValueError(f"the initial mesh has {deg.sum()} coefficients > max_dof = {max_dof}")

        def round_fn():
            self.element_degrees = deg
            self.solve()
            ne, est, eta2, out3 = self._estimate_round(min(32, max(int(deg.max()), 8)) if nq is None else nq)

            def refine():
                nonlocal deg
                x, W = self.enhanced.nodes, self.enhanced.W
                deg_dev = torch.as_tensor(deg.astype(np.int32), device=x.device)
                sigma = ops.smoothness(x, W, deg_dev)
                x_new, deg_new, _, (split, raised) = ops.refine_hp(x, eta2, out3[1:2], theta, sigma, deg_dev,
                                                                   sigma_min=float(sigma_min), dM=int(dM),
                                                                   M_max=int(M_max), h_min=h_min)
                deg_new = deg_new.cpu().numpy().astype(np.int64)
                if max_dof is not None and deg_new.sum() > max_dof:
                    return None
                deg = deg_new          # (read by the next round only: a stop of the loop's leaves element_degrees)
                return x_new.cpu().numpy(), dict(marked=split, raised=raised)
            return ne, est, dict(marked=0, raised=0, dof=int(deg.sum())), refine
        return self._adapt_rounds(tol, max_elements, max_iter, round_fn, start)
