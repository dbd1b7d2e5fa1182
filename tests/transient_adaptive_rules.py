"""Shared cases and bars of the adaptive time-stepping tests: tests/test_transient_adaptive_cpu.py
runs them through the numpy prototype, the library's host mirrors and the facade's scalar rules,
tests/test_gpu_transient_adaptive.py through the device.

The bars.  Every "within rounding" bar is 10x what the float64 prototype (scripts/proto/transient_adaptive_proto.py,
LAPACK's banded LU) itself reads on the SAME case against the same loop in np.longdouble, with a floor of 4 eps; the
reading is taken when the test runs (cached), never from the code under test.  Both prototype loops run on the bands the
device assembled, for the reason tests/transient_rules.py gives.  A comparison of two adaptive loops only makes sense
when they take the same decisions, so every case must keep its decisions away from their thresholds IN THE PROTOTYPE
(condition, not measurement): no attempt with |err - 1| < 1e-3 and no raw factor within 1e-3 relative of a clip bound
(0.2, 2, and 1 after a rejection).  ``MARGINS_READ`` records what the cases had when they were chosen."""
import ctypes
import hashlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import transient_adaptive_proto as proto        # noqa: E402
import transient_proto as tproto                # noqa: E402
import transient_rules as tr                    # noqa: E402

EPS, FLOOR, MARGIN = tr.EPS, tr.FLOOR, tr.MARGIN
DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN
DECISION_MARGIN = 1e-3


class Case:
    """One adaptive problem: what proto.solve takes, and the facade's constructor and call arguments."""

    def __init__(self, name, nodes, u0, t_end, tol, dt0, t_out=None, a=None, da=None, c=None, rho=None, forcing=None,
                 kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), end_data=(0.0, 0.0)):
        self.name, self.nodes, self.u0, self.t_end, self.tol, self.dt0, self.t_out = name, nodes, u0, t_end, tol, dt0, \
            t_out
        self.a, self.da, self.c, self.rho, self.forcing = a, da, c, rho, forcing
        self.kinds, self.kappa, self.end_data = kinds, kappa, end_data
        self.scale = float(np.max(np.abs(u0(nodes))))

    def run(self, dtype=np.float64, **kw):
        return proto.solve(self.nodes, self.u0, self.t_end, self.tol, self.tol, self.dt0, t_out=self.t_out, a=self.a,
                           c=self.c, rho=self.rho, forcing=self.forcing, kinds=self.kinds, kappa=self.kappa,
                           end_data=self.end_data, dtype=dtype, **kw)

    def facade(self, M=9, n_colloc=16, gamma=1e4):
        bnd = tuple(("dirichlet", 0.0) if k == DIRICHLET else ("robin", kp, 0.0)
                    for k, kp in zip(self.kinds, self.kappa))
        ctor = dict(num_fem_nodes=len(self.nodes), lssvr_M=M, lssvr_gamma=gamma, n_colloc=n_colloc, mesh=self.nodes,
                    global_domain=(float(self.nodes[0]), float(self.nodes[-1])), boundary=bnd,
                    coef=None if self.a is None else (self.a, self.da), reaction=self.c)
        call = dict(rtol=self.tol, atol=self.tol, dt0=self.dt0, t_out=self.t_out, weight=self.rho,
                    end_data=self.end_data, forcing=[(0.0, tr._zero)] if not self.forcing else self.forcing)
        return ctor, call


UNIFORM = np.linspace(-1.0, 1.0, 33)


def decay(tol=1e-4):
    """(a): -u'' on 32 uniform elements, u0 = cos(pi x / 2) + cos(5 pi x / 2) / 2, zero Dirichlet ends, to t = 1."""
    return Case(f"decay-{tol:g}", UNIFORM, proto.two_mode, 1.0, tol, 1e-4)


def pulse():
    """(b): the same with the forcing 50 exp(-((t - 0.5) / 0.02)^2) cos(pi x / 2) and three output times.  dt0 = 1e-3
    left a raw factor 6.9e-4 from a clip bound; 2e-3 keeps every decision clear of its threshold (MARGINS_READ)."""
    return Case("pulse", UNIFORM, proto.two_mode, 1.0, 1e-3, PULSE_DT0, t_out=[0.25, 0.5, 1.0],
                forcing=[(proto.pulse, lambda x: np.cos(0.5 * math.pi * x))])


PULSE_DT0 = 2e-3


def general():
    """(c): section 26's non-uniform 33-node mesh with variable a, c, rho, Robin-left and moving Dirichlet-right data
    and R = 2, two output times."""
    g = tr.general()
    return Case("general-33", g.nodes, g.u0, g.t_end, 1e-4, 1e-3, t_out=[0.32, 0.64], a=g.a, da=g.da, c=g.c, rho=g.rho,
                forcing=g.forcing, kinds=g.kinds, kappa=g.kappa, end_data=g.end_data)


CASES = {"decay": decay, "pulse": pulse, "general-33": general}
PROPORTIONAL_TOLS = (1e-3, 1e-4, 1e-5)
# (min |err - 1|, min relative distance of a raw factor from a clip bound), prototype on the oracle's bands
MARGINS_READ = {"decay-0.001": (2.8e-1, 9.2e-2), "decay-0.0001": (2.1e-1, 7.5e-2), "decay-1e-05": (7.2e-2, 7.4e-2),
                "pulse": (8.9e-3, 2.1e-3), "general-33": (7.1e-2, 2.5e-1)}
# (accepted, rejected, restarts) of the prototype
COUNTS_READ = {"decay-0.001": (33, 0, 0), "decay-0.0001": (58, 0, 0), "decay-1e-05": (113, 0, 0), "pulse": (60, 10, 1),
               "general-33": (41, 2, 2)}
# name: ((prototype float64, device) of max relative |dt - dt_longdouble| over the attempts, (prototype float64, device)
# of max |u - u_longdouble|_inf / |u0|_inf over the snapshots), on the device's bands
LOOP_READ = {"decay": ((3.5e-12, 8.8e-12), (2.1e-16, 1.4e-15)), "pulse": ((3.5e-12, 3.9e-12), (5.8e-15, 9.6e-15)),
             "general-33": ((3.8e-12, 4.5e-12), (1.8e-15, 4.0e-15))}
# global error at t = 1 of (a) against the exact semi-discrete solution: tol: (prototype, device)
GLOBAL_READ = {1e-3: (3.285e-3, 3.285e-3), 1e-4: (7.891e-4, 7.891e-4), 1e-5: (1.822e-4, 1.822e-4)}

_REFERENCES = {}


def references(name, bands=None):
    """(case, np.longdouble loop, float64 loop), computed once per (name, bands)."""
    key = (name, None if bands is None else hashlib.sha1(tr._band_bytes(bands)).hexdigest())
    if key not in _REFERENCES:
        case = CASES[name]() if name in CASES else decay(float(name.split("-", 1)[1]))
        _REFERENCES[key] = (case, case.run(np.longdouble, bands=bands), case.run(bands=bands))
    return _REFERENCES[key]


def decisions_clear(res):
    me, mf = proto.margins(res)
    return me >= DECISION_MARGIN and mf >= DECISION_MARGIN, (me, mf)


def dt_reading(name, steps, bands=None):
    """(max relative difference of the attempts' steps from the np.longdouble loop's, bar, the float64 prototype's
    own); the accept / reject sequences must be equal first."""
    case, ref, p64 = references(name, bands)
    err, read = (float(np.max(np.abs(np.asarray(s)[:, 1] - ref["steps"][:, 1]) / ref["steps"][:, 1]))
                 for s in (steps, p64["steps"]))
    return err, max(MARGIN * read, FLOOR), read


def nodal_reading(name, nodal, bands=None):
    case, ref, p64 = references(name, bands)
    err, read = (float(np.max(np.abs(np.asarray(v, dtype=np.longdouble) - ref["nodal"]))) / case.scale
                 for v in (nodal, p64["nodal"]))
    return err, max(MARGIN * read, FLOOR), read


def global_error(case, bands, nodal_end):
    """|u_h(1) - exact semi-discrete u(1)|_inf on the given bands (case (a): no forcing, zero Dirichlet ends)."""
    return float(np.max(np.abs(np.asarray(nodal_end) - proto.exact_semidiscrete(bands, case.u0(case.nodes),
                                                                                case.t_end))))


# ---- the host mirrors -------------------------------------------------------------------------------------------------
_hp, _h = tr._hp, tr._h


def step_host(kd, ko, md, mo, U0, U1, loads, phi, s, beta0, beta1, inv_dt, write_bands=True, sentinel=np.nan,
              check=True):
    """lssvr_ts_step_host -> (rc, adiag, aoff, b); U0 [ne+1], loads [R, ne+1], phi [R]; the bands start as
    ``sentinel``."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    kd, ko, md, mo, U0, loads, phi = (_h(t) for t in (kd, ko, md, mo, U0, loads, phi))
    U1 = None if U1 is None else _h(U1)
    ne = len(mo)
    adiag, aoff, b = np.full(ne + 1, sentinel), np.full(ne, sentinel), np.full(ne + 1, np.nan)
    rc = lib.lssvr_ts_step_host(_hp(kd), _hp(ko), _hp(md), _hp(mo), _hp(U0), None if U1 is None else _hp(U1),
                                _hp(loads), _hp(phi), ne, loads.shape[0], s, beta0, beta1, inv_dt, int(write_bands),
                                _hp(adiag), _hp(aoff), _hp(b))
    if check:
        _capi.check(rc, "lssvr_ts_step_host")
    return rc, adiag, aoff, b


def error_host(U3, U2, U1, U0, w, atol, rtol, kinds, check=True):
    """lssvr_ts_error_host -> (rc, out4)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    U3, U2 = _h(U3), _h(U2)
    U1, U0 = (None if t is None else _h(t) for t in (U1, U0))
    out4 = np.full(4, np.nan)
    rc = lib.lssvr_ts_error_host(_hp(U3), _hp(U2), None if U1 is None else _hp(U1), None if U0 is None else _hp(U0),
                                 int(kinds[0]), int(kinds[1]), len(U3) - 1, *[float(v) for v in w], atol, rtol,
                                 _hp(out4))
    if check:
        _capi.check(rc, "lssvr_ts_error_host")
    return rc, out4


def estimate_host(U3, U2, U1, U0, w, atol, rtol, kinds):
    """proto.estimate through the host mirror: the ``estimate_fn`` of proto.solve."""
    return error_host(U3, U2, U1, U0, w, atol, rtol, kinds)[1]


def matrix_host_and_rhs(kd, ko, md, mo, u0, u1, loads, phi, s, beta0, beta1, inv_dt):
    return step_host(kd, ko, md, mo, u0, u1, loads, phi, s, beta0, beta1, inv_dt)[1:]


def error_numpy(U3, U2, U1, U0, w, atol, rtol, kinds):
    return np.array([float(v) for v in proto.estimate(np.asarray(U3, dtype=np.float64), np.asarray(U2, dtype=np.float64),
                                                      U1, U0, w, atol, rtol, kinds)])


def error_inputs(ne, seed=0):
    """Four smooth-plus-noise nodal vectors and the weights of a non-uniform triple of steps: e is small against u, as
    in a run."""
    rng = np.random.default_rng(77 * seed + ne % 9973)
    x = np.linspace(0.0, 1.0, ne + 1)
    base = np.cos(3.0 * x) + 0.1 * rng.standard_normal(ne + 1)
    h, hp, hpp = 0.013, 0.011, 0.007
    ts = np.array([h + hp + hpp, hp + hpp, hpp, 0.0])
    Us = [base * math.exp(-t) + 1e-6 * rng.standard_normal(ne + 1) for t in ts]
    al = proto.coefficients(h / hp)[0]
    return Us, proto.weights_bdf2(h, hp, hpp, al), proto.weights_bdf1(h, hp)


# ---- what solve_transient_adaptive refuses: (name, constructor kwargs, call kwargs, a fragment of the message) -------------
BASE = dict(rtol=1e-3, atol=1e-3, dt0=0.01)


def refusals():
    u0 = lambda x: 0.0 * x      # noqa: E731
    me = "solve_transient_adaptive "

    def kw(**over):
        return {**BASE, **over}
    return [
        ("convection", dict(convection=lambda x: 0.0 * x), kw(), me + tr.STRUCTURAL[0]),
        ("periodic", dict(boundary="periodic", reaction=lambda x: 1.0 + 0.0 * x), kw(), me + tr.STRUCTURAL[1]),
        ("fem_solver flux", dict(fem_solver="flux"), kw(), me + tr.STRUCTURAL[2]),
        ("fem_solver pivot", dict(fem_solver="pivot"), kw(), me + tr.STRUCTURAL[2]),
        ("element_degrees", dict(_degrees=True), kw(), me + tr.STRUCTURAL[3]),
        ("solver", dict(solver=1), kw(), me + tr.STRUCTURAL[4]),
        ("nonlinear", dict(nonlinear=("poly", [u0, u0])), kw(), me + "has no nonlinear term"),
        ("rho <= 0", {}, kw(weight=lambda x: x), tr.RHO_MSG),
        ("R > 8", {}, kw(forcing=[(1.0, u0)] * 9), "forcing must hold 1 .. 8 terms (R <= 8), got 9"),
        ("non-finite forcing", {}, kw(forcing=[(1.0, lambda x: np.full_like(x, np.nan))]),
         "forcing[0] f_x is not finite at a quadrature point"),
        ("non-finite phi at t = 0", {}, kw(forcing=[(lambda t: math.inf, u0)]),
         "forcing phi is not finite where it is tabulated"),
        ("non-finite u0", {}, kw(_u0=lambda x: np.full_like(x, np.inf)), "u0 is not finite where it is tabulated"),
        ("t_end", {}, kw(_t_end=-1.0), "t_end must be finite and > 0"),
        ("rtol < 0", {}, kw(rtol=-1e-3), "rtol and atol must be finite and >= 0 and rtol + atol > 0"),
        ("atol < 0", {}, kw(atol=-1e-3), "rtol and atol must be finite and >= 0 and rtol + atol > 0"),
        ("rtol + atol = 0", {}, kw(rtol=0.0, atol=0.0), "rtol and atol must be finite and >= 0 and rtol + atol > 0"),
        ("rtol nan", {}, kw(rtol=math.nan), "rtol and atol must be finite and >= 0 and rtol + atol > 0"),
        ("atol inf", {}, kw(atol=math.inf), "rtol and atol must be finite and >= 0 and rtol + atol > 0"),
        ("dt0 = 0", {}, kw(dt0=0.0), "dt0 must lie in (0, t_end = 0.4]"),
        ("dt0 > t_end", {}, kw(dt0=0.5), "dt0 must lie in (0, t_end = 0.4]"),
        ("dt0 nan", {}, kw(dt0=math.nan), "dt0 must lie in (0, t_end = 0.4]"),
        ("dt_min > dt0", {}, kw(dt_min=0.02), "dt_min must lie in [0, dt0 = 0.01]"),
        ("dt_max < dt0", {}, kw(dt_max=0.005), "dt_max must be finite and >= dt0 = 0.01"),
        ("max_steps", {}, kw(max_steps=0), "max_steps must be an integer >= 1"),
        ("t_out unsorted", {}, kw(t_out=[0.3, 0.2]), "t_out must be ascending times in (0, t_end = 0.4]"),
        ("t_out repeated", {}, kw(t_out=[0.2, 0.2]), "t_out must be ascending times in (0, t_end = 0.4]"),
        ("t_out at 0", {}, kw(t_out=[0.0, 0.2]), "t_out must be ascending times in (0, t_end = 0.4]"),
        ("t_out past the end", {}, kw(t_out=[0.2, 0.5]), "t_out must be ascending times in (0, t_end = 0.4]"),
        ("t_out empty", {}, kw(t_out=[]), "t_out must be ascending times in (0, t_end = 0.4]"),
        ("c + rho/dt_max < 0", dict(reaction=lambda x: -5.0 + 0.0 * x), kw(),
         "c + rho / dt_max < 0 at a quadrature point (dt_max = 0.4)"),
    ]


def passing():
    """A mildly negative c with a dt_max that keeps c + rho / dt_max >= 0 gets as far as the device."""
    return [(dict(reaction=lambda x: -5.0 + 0.0 * x), dict(BASE, dt_max=0.1))]


def call_adaptive(s, u0, v0, **kw):
    kw.pop("nsteps", None)                  # tr.check_refusals' default for the fixed-step loops
    return s.solve_transient_adaptive(u0, kw.pop("_t_end", 0.4), **kw)
