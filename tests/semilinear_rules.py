"""Shared cases and bars of the semilinear tests: tests/test_semilinear_cpu.py runs them through
the numpy prototype and the library's host mirrors, tests/test_gpu_semilinear.py through the device.

The bars.  POLY tables, nl_step and out4 of nl_residual are bit-equal to the host mirrors (-ffp-contract=off, one inline
routine behind both), and the host mirrors to the plain numpy restatement below.  EXP differs by the exp itself: the
host mirror's is libm (as numpy's: 0 to 1 ulp apart, EXP_HOST_READ), the device's is the device library's (HIP
documents 1 ulp), so the device bar is 8 eps of |q_0 E| (1 + |q_1 u|) per entry, for every output, on the run in
which the outputs are made of g and g_u alone (f = 0, no c table); with f and c the outputs must be the documented
sums of the device's own g and g_u, bit for bit.  Every
"within rounding" bar of the loop is 10x what the float64 prototype (scripts/proto/semilinear_proto.py, LAPACK's banded
LU) itself reads on the SAME case against the same loop in np.longdouble, with a floor of 4 eps -- the rule of
tests/transient_rules.py.  The reading is taken when the test runs (cached), never from the code under test."""
import ctypes
import functools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import semilinear_proto as proto         # noqa: E402
from oracle import lssvr_oracle as orc   # noqa: E402
import convection_rules as cr            # noqa: E402

EPS = 2.0 ** -52
FLOOR = 4.0 * EPS
MARGIN = 10.0
DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN
POLY, EXP = proto.POLY, proto.EXP
BANDS_BAR = 32.0 * EPS                  # device K against the oracle's assembly: the reasoning of transient_rules.py
ENH_FAMILY_BAR = 1e-11                  # the reaction-row tests' bar against the float64 restatement, M <= 22
# max |np.exp - the host mirror's exp| in ulps of the value, over the EXP cases of the CPU test (both are libm here).
# A record of the reading when the cases were written: no test reads it (the CPU test measures the figure afresh and
# notes it).
EXP_HOST_READ = 0.99


def _zero(x):
    return 0.0 * np.asarray(x, dtype=np.float64)


def _const(v):
    return lambda x: float(v) + 0.0 * np.asarray(x, dtype=np.float64)


# ---- the host mirrors ---------------------------------------------------------------------------------------------------------
def _hp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _h(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def linearize_host(u, t, kind, q, c, f, pm=False, want=(True, True, True), check=True, n=None, nterm=None):
    """lssvr_nl_linearize_host -> (rc, c_eff, f_eff, f_res); the tables in the layout ``pm`` says: q [nterm, ne, n] /
    [nterm, n, ne].  An output not wanted is None."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    u, t, q, c, f = (_h(v) for v in (u, t, q, c, f))
    outs = [np.full(f.shape, np.nan) if w else None for w in want]
    n = (f.shape[0] if pm else f.shape[1]) if n is None else n
    rc = lib.lssvr_nl_linearize_host(_hp(u), _hp(t), _hp(q), _hp(c), _hp(f), len(u) - 1, n, int(pm), kind,
                                     q.shape[0] if nterm is None else nterm, *(_hp(o) for o in outs))
    if check:
        _capi.check(rc, "lssvr_nl_linearize_host")
    return (rc, *outs)


def residual_host(diag, sub, sup, load, u, u_new, kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), g=(0.0, 0.0),
                  check=True):
    """lssvr_nl_residual_host -> (rc, out4)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    diag, sub, sup, load, u, u_new, g = (_h(v) for v in (diag, sub, sup, load, u, u_new, g))
    out4 = np.full(4, np.nan)
    rc = lib.lssvr_nl_residual_host(_hp(diag), _hp(sub), _hp(sup), _hp(load), _hp(u), _hp(u_new), kinds[0], kinds[1],
                                    _hp(g), (ctypes.c_double * 2)(*kappa), len(sub), _hp(out4))
    if check:
        _capi.check(rc, "lssvr_nl_residual_host")
    return rc, out4


def step_host(u, u_new, lam, check=True):
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    u, u_new = _h(u), _h(u_new)
    out = np.full(u.shape, np.nan)
    rc = lib.lssvr_nl_step_host(_hp(u), _hp(u_new), float(lam), len(u) - 1, _hp(out))
    if check:
        _capi.check(rc, "lssvr_nl_step_host")
    return rc, out


# ---- the plain numpy restatement (every sum in the documented order) ---------------------------------------------------
def linearize_numpy(u, t, kind, q, c, f, pm=False):
    """(c_eff, f_eff, f_res) in the layout of the inputs; element-major arithmetic on [ne, n] views."""
    if pm:
        q, f = np.transpose(q, (0, 2, 1)), f.T
        c = None if c is None else c.T
    out = proto.linearize(kind, list(q), np.asarray(u, dtype=np.float64), t, c, f)
    return tuple(np.ascontiguousarray(v.T) if pm else v for v in out)


def residual_numpy(diag, sub, sup, load, u, u_new, kinds, kappa, g):
    """out4 of lssvr_nl_residual: a non-finite entry raises the count and joins no maximum."""
    with np.errstate(all="ignore"):
        r = proto.residual(diag, sub, sup, load, np.asarray(u, dtype=np.float64), kinds, kappa, g)
        vals = [np.abs(r), np.abs(u_new - u), np.abs(u_new)]
    bad = sum(int(np.count_nonzero(~np.isfinite(v))) for v in vals)
    return np.array([max([0.0] + v[np.isfinite(v)].tolist()) for v in vals] + [float(bad)])


def kernel_inputs(ne, n, kind, nterm, seed=0):
    """Seeded inputs of the three kernels: a nodal vector pair, local coordinates, tables [.., ne, n] (element-major)
    and the bands of a random non-symmetric tridiagonal matrix."""
    rng = np.random.default_rng(1000 * seed + ne % 9973 + 17 * n + 31 * nterm + 7 * kind)
    q = rng.uniform(-1.0, 1.0, (nterm, ne, n))
    if kind == EXP:
        q[1] = rng.uniform(-1.5, 1.5, (ne, n))
    return dict(u=rng.uniform(-1.5, 1.5, ne + 1), u_new=rng.uniform(-1.5, 1.5, ne + 1), t=np.sort(rng.uniform(0, 1, n)),
                q=q, c=rng.uniform(0.0, 2.0, (ne, n)), f=rng.standard_normal((ne, n)),
                diag=rng.uniform(2.0, 3.0, ne + 1), sub=rng.uniform(-1.0, -0.5, ne), sup=rng.uniform(-1.0, -0.5, ne),
                load=rng.standard_normal(ne + 1), g=rng.standard_normal(2), kappa=(0.75, 1.25))


def layout(d, pm):
    """(q, c, f) of kernel_inputs in the layout ``pm`` says."""
    if not pm:
        return d["q"], d["c"], d["f"]
    return (np.ascontiguousarray(np.transpose(d["q"], (0, 2, 1))), np.ascontiguousarray(d["c"].T),
            np.ascontiguousarray(d["f"].T))


def exp_bar_scale(d):
    """|q_0 E| (1 + |q_1 u_h|) per entry [ne, n] of kernel_inputs with kind EXP: 8 eps of it is the device bar."""
    uh = d["u"][:-1, None] + (d["u"][1:] - d["u"][:-1])[:, None] * d["t"][None, :]
    q0, q1 = d["q"]
    return np.abs(q0 * np.exp(q1 * uh)) * (1.0 + np.abs(q1 * uh))


def exp_entry_terms(d, with_c=True, with_f=True):
    """Per entry [ne, n] of kernel_inputs with kind EXP, for each of the three outputs (``with_c`` / ``with_f`` False:
    the call without c_tab / with f = 0), the sum of the sizes of the output's terms, |c| + |g_u|,
    |f| + |g| + |g_u u_h|, |f| + |g|: the scale of the host-mirror bar of the CPU test."""
    uh = d["u"][:-1, None] + (d["u"][1:] - d["u"][:-1])[:, None] * d["t"][None, :]
    q0, q1 = d["q"]
    g = np.abs(q0 * np.exp(q1 * uh))
    c = np.abs(d["c"]) if with_c else 0.0
    f = np.abs(d["f"]) if with_f else 0.0
    return dict(c_eff=c + g * np.abs(q1), f_eff=f + g + g * np.abs(q1 * uh), f_res=f + g)


# ---- the cases of the loop -----------------------------------------------------------------------------------------------
class Case:
    """One semilinear problem: what proto.solve takes, and the facade's constructor arguments."""

    def __init__(self, name, nodes, kind, q, f=None, a=None, da=None, b=None, c=None, kinds=(DIRICHLET, DIRICHLET),
                 kappa=(0.0, 0.0), end_values=(0.0, 0.0), fem_solver="bands", exact=None):
        self.name, self.nodes, self.kind, self.q, self.f = name, np.asarray(nodes, dtype=np.float64), kind, q, f
        self.a, self.da, self.b, self.c = a, da, b, c
        self.kinds, self.kappa, self.end_values, self.fem_solver, self.exact = kinds, kappa, end_values, fem_solver, exact

    def run(self, dtype=np.float64, **kw):
        return proto.solve(self.nodes, self.kind, self.q, self.f, a=self.a, b=self.b, c=self.c, kinds=self.kinds,
                           kappa=self.kappa, end_values=self.end_values, dtype=dtype, **kw)

    def facade(self, M=9, n_colloc=16, gamma=1e4, **over):
        bnd = tuple(("dirichlet", g) if k == DIRICHLET else ("robin", kp, g)
                    for k, kp, g in zip(self.kinds, self.kappa, self.end_values))
        nl = ("poly", list(self.q)) if self.kind == POLY else ("exp", *self.q)
        kw = dict(num_fem_nodes=len(self.nodes), lssvr_M=M, lssvr_gamma=gamma, n_colloc=n_colloc, mesh=self.nodes,
                  global_domain=(float(self.nodes[0]), float(self.nodes[-1])), boundary=bnd,
                  rhs=_zero if self.f is None else self.f, coef=None if self.a is None else (self.a, self.da),
                  reaction=self.c, convection=self.b, fem_solver=self.fem_solver, nonlinear=nl)
        kw.update(over)
        return kw

    def oracle_bands(self):
        """(diag, sub, sup) of the LINEAR operator by the oracle's assembly (tests/convection_rules.py for b)."""
        return cr.conv_bands(self.nodes, _zero, self.a, self.b, self.c)[:3]


def case_a(ne):
    """A.  -u'' + u^3 = f, manufactured u = sin(pi x) on (-1, 1), zero Dirichlet ends."""
    return Case(f"A-{ne}", np.linspace(-1.0, 1.0, ne + 1), POLY, proto.cubic_q(), proto.cubic_f,
                exact=lambda x: np.sin(math.pi * x))


A_NE = (2, 5, 32, 33)


def case_b(ne, fem_solver="pivot", lam=1.0):
    """B.  Bratu: -u'' - lam e^u = 0 on (0, 1), zero Dirichlet ends; c_eff = -lam e^u < 0."""
    return Case(f"B-{ne}", np.linspace(0.0, 1.0, ne + 1), EXP, [_const(-lam), _const(1.0)], fem_solver=fem_solver,
                exact=lambda x: proto.bratu_exact(x, lam))


B_NE = (8, 16, 32)


def case_c():
    """C.  Non-uniform 33-node mesh, variable a, b, c (cell Peclet < 1), Robin left / Dirichlet right, POLY with four
    x-dependent terms."""
    w = np.random.default_rng(27).uniform(0.5, 1.5, 32)
    nodes = -1.0 + 2.0 * np.concatenate([[0.0], np.cumsum(w)]) / np.sum(w)
    nodes[-1] = 1.0
    q = [lambda x: 0.2 * np.cos(x), lambda x: 0.5 + 0.25 * x, lambda x: 0.3 * np.sin(2.0 * x),
         lambda x: 1.0 + 0.5 * x * x]
    return Case("C-33", nodes, POLY, q, lambda x: 2.0 * np.sin(math.pi * x) + x, a=lambda x: 1.0 + 0.5 * np.sin(2.0 * x),
                da=lambda x: np.cos(2.0 * x), b=lambda x: 2.0 + np.cos(3.0 * x), c=lambda x: 0.5 + 0.3 * np.cos(3.0 * x),
                kinds=(ROBIN, DIRICHLET), kappa=(2.0, 0.0), end_values=(0.3, -0.4))


def case_d():
    """D.  A stiff cubic from the zero start: -u'' + 1000 u^3 = 1 on (-1, 1), u(-1) = 1.5, u(1) = -0.5, 32 elements.
    The prototype damps iteration 1 (lambda = 1/2: the full step's residual 2.0e1 exceeds |R(u_0)| = 1.2e1, the
    halved step reads 4.8e0) and takes full steps after it: 9 iterations, D_LAMBDAS."""
    return Case("D-32", np.linspace(-1.0, 1.0, 33), POLY, [_zero, _zero, _zero, _const(1000.0)], _const(1.0),
                end_values=(1.5, -0.5))


D_LAMBDAS = [0.5] + [1.0] * 8


def case_e():
    """E.  The linear limit: nterm = 2, g = q_0 + q_1 u, which is the linear problem with reaction c + q_1 and
    right-hand side f - q_0; Newton is exact in one step and stops at the second."""
    q0, q1 = (lambda x: 0.5 * np.cos(2.0 * x)), (lambda x: 1.0 + 0.5 * x)
    c, f = (lambda x: 0.5 + 0.25 * x * x), (lambda x: np.sin(math.pi * x) + 1.0)
    case = Case("E-17", np.linspace(-1.0, 1.0, 18), POLY, [q0, q1], f, c=c, end_values=(0.25, -0.5))
    case.linear = dict(reaction=lambda x: c(x) + q1(x), rhs=lambda x: f(x) - q0(x))
    return case


CASES = {**{f"A-{ne}": functools.partial(case_a, ne) for ne in A_NE},
         **{f"B-{ne}": functools.partial(case_b, ne) for ne in B_NE},
         "C-33": case_c, "D-32": case_d, "E-17": case_e}

# max |u - u_longdouble|_inf / max(1, |u|_inf) on the device's K.  name: (prototype float64, device); written when
# the cases were first run.  A record only: no test reads it -- the bar is taken from the prototype when the test runs,
# and the fresh readings are noted beside it
LOOP_READ = {"A-2": (0.0, 4.4e-16), "A-5": (1.9e-16, 1.7e-16), "A-32": (3.2e-15, 4.0e-15), "A-33": (4.9e-15, 2.7e-15),
             "B-8": (1.3e-16, 7.5e-17), "B-16": (2.0e-16, 1.2e-16), "B-32": (3.3e-16, 1.9e-16), "C-33": (3.0e-15, 2.6e-15),
             "D-32": (8.9e-17, 8.4e-17), "E-17": (3.9e-16, 3.2e-16)}


@functools.lru_cache(maxsize=None)
def _references(name, key):
    case = CASES[name]()
    K = None if key is None else tuple(np.frombuffer(b, dtype=np.float64) for b in key)
    return case, case.run(np.longdouble, K=K), case.run(K=K)


def references(name, K=None):
    """(case, np.longdouble loop, float64 loop), computed once per (name, K); K: the device's (diag, sub, sup)."""
    return _references(name, None if K is None else tuple(np.ascontiguousarray(v).tobytes() for v in K))


def loop_reading(name, u, K=None):
    """(error of the nodal ``u``, bar, the float64 prototype's own error) against the np.longdouble prototype,
    relative to max(1, |u|_inf); the bar is 10x the prototype's, at least 4 eps."""
    case, ref, p64 = references(name, K)
    scale = max(1.0, float(np.max(np.abs(ref["u"]))))
    err, read = (float(np.max(np.abs(np.asarray(v, dtype=np.longdouble) - ref["u"]))) / scale for v in (u, p64["u"]))
    return err, max(MARGIN * read, FLOOR), read


def bands_error(case, K):
    """max |device - oracle| / scale over (diag, sub, sup): the scale of an off-diagonal entry is the larger
    neighbouring diagonal entry (tests/transient_rules.py)."""
    wd, wl, wu = case.oracle_bands()
    gd, gl, gu = K
    assert gd.shape == wd.shape and gl.shape == wl.shape and gu.shape == wu.shape
    sc = np.abs(wd)
    so = np.maximum(sc[:-1], sc[1:])
    return max(float(np.max(np.abs(gd - wd) / sc)), float(np.max(np.abs(gl - wl) / so)),
               float(np.max(np.abs(gu - wu) / so)))


# ---- the accuracy record: case A, M = 9, 16 points, gamma = 1e4 ---------------------------------------------------------
# ne: (max |I_h u_h - u|, max |enhanced - u|) over 2001 points, by the prototype
ACCURACY = {8: (6.2374e-2, 9.6039e-3), 16: (1.6511e-2, 2.4504e-3), 32: (4.1836e-3, 6.1573e-4)}
ACCURACY_POINTS = 2001


def accuracy(nodes, u, W, exact, points=ACCURACY_POINTS):
    """(max |I_h u - exact|, max |enhanced - exact|) over ``points`` equidistant points."""
    xs = np.linspace(nodes[0], nodes[-1], points)
    ue, _ = orc.evaluate_solution(nodes, W, xs)
    return float(np.max(np.abs(np.interp(xs, nodes, u) - exact(xs)))), float(np.max(np.abs(ue - exact(xs))))


# ---- what nonlinear refuses: (name, constructor kwargs or None for the default, what to call) ---------------------------------
def refusals():
    ok = ("poly", [_zero, _zero, _zero, _const(1.0)])
    react = _const(1.0)
    ctor = [
        ("fem_solver flux", dict(nonlinear=ok, fem_solver="flux")),
        ("periodic", dict(nonlinear=ok, boundary="periodic", reaction=react)),
        ("solver", dict(nonlinear=ok, solver=1)),
        ("element_lists", dict(nonlinear=ok, element_lists=True)),
        ("unknown kind", dict(nonlinear=("cubic", [_zero]))),
        ("a callable of u", dict(nonlinear=lambda x, u: u ** 3)),
        ("nterm 0", dict(nonlinear=("poly", []))),
        ("nterm 7", dict(nonlinear=("poly", [_zero] * 7))),
        ("q_k not callable", dict(nonlinear=("poly", [_zero, 1.0]))),
        ("exp with one table", dict(nonlinear=("exp", _zero))),
    ]
    call = [
        ("q_k of the wrong shape", dict(nonlinear=("poly", [lambda x: np.ones(3)])), lambda s: s.solve_fem()),
        ("q_k not finite", dict(nonlinear=("poly", [lambda x: np.full_like(x, np.nan)])), lambda s: s.solve_fem()),
        ("q_k not finite at a node (a collocation point, no quadrature point)",
         dict(nonlinear=("exp", _const(1.0), lambda x: np.where(x == -1.0, np.inf, 1.0))), lambda s: s.solve_fem()),
        ("tol 0", dict(nonlinear=ok), lambda s: s.solve_fem(tol=0.0)),
        ("tol < 0", dict(nonlinear=ok), lambda s: s.solve(tol=-1e-8)),
        ("max_iter 0", dict(nonlinear=ok), lambda s: s.solve_fem(max_iter=0)),
        ("u_init not callable", dict(nonlinear=ok), lambda s: s.solve_fem(u_init=1.0)),
        ("u_init not finite", dict(nonlinear=ok), lambda s: s.solve_fem(u_init=lambda x: np.full_like(x, np.inf))),
        ("element_degrees", dict(nonlinear=ok, _degrees=True), lambda s: s.solve_fem()),
        ("solve_many", dict(nonlinear=ok), lambda s: s.solve_many([_zero])),
        ("solve_goal", dict(nonlinear=ok), lambda s: s.solve_goal(_zero)),
        ("solve_adaptive", dict(nonlinear=ok), lambda s: s.solve_adaptive(tol=1e-3)),
        ("solve_eigen", dict(nonlinear=ok), lambda s: s.solve_eigen()),
        ("solve_transient", dict(nonlinear=ok), lambda s: s.solve_transient(_zero, 0.1, nsteps=2)),
        ("Newton keywords without nonlinear", {}, lambda s: s.solve_fem(tol=1e-10)),
    ]
    return ctor, call


def check_refusals(monkeypatch):
    """Every refusal is a ValueError raised on the host: the library loader and the device lookup are replaced by
    functions that fail the test, so no entry is bound and no kernel can be launched."""
    import pytest
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import _capi, solver

    def forbidden(*a, **k):
        raise AssertionError("a device call was reached before the refusal")
    monkeypatch.setattr(_capi, "load", forbidden)
    monkeypatch.setattr(solver, "_device", forbidden)
    ctor, call = refusals()
    for name, kw in ctor:
        with pytest.raises(ValueError):
            pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, n_colloc=16, **kw)
            raise AssertionError(f"{name}: not refused")
    for name, kw, fn in call:
        kw = dict(kw)
        degrees = kw.pop("_degrees", False)
        s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, n_colloc=16, **kw)
        if degrees:
            s.element_degrees = np.full(8, 9)
        with pytest.raises(ValueError):
            fn(s)
            raise AssertionError(f"{name}: not refused")
    # a well-posed solver gets past the checks: the refusal then comes from the missing device
    s = pkg.FEMLSSVRPrimalSolver(9, nonlinear=ctor[0][1]["nonlinear"])
    with pytest.raises(AssertionError, match="device call"):
        s.solve_fem()
