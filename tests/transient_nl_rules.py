"""Shared cases and bars of the semilinear transient tests: tests/test_transient_nl_cpu.py runs
them through the numpy prototype and the library's host mirror, tests/test_gpu_transient_nl.py through the device.

The bars.  lssvr_ts_nl_assemble is bit-equal to the chain it replaces and, for POLY, to its host mirror and to the plain
numpy restatement (proto.newton_system in float64: every sum in the documented order); EXP differs by the exp itself,
under the bars of tests/semilinear_rules.py.  Every "within rounding" bar of the loop is 10x what the float64 prototype
(scripts/proto/transient_semilinear_proto.py, LAPACK's banded LU) itself reads on the SAME case against the same loop in
np.longdouble, with a floor of 4 eps -- the rule of tests/transient_rules.py.  The reading is taken when the test runs
(cached), never from the code under test."""
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import transient_semilinear_proto as proto   # noqa: E402
import transient_rules as tr                 # noqa: E402
from oracle import lssvr_oracle as orc       # noqa: E402

EPS = 2.0 ** -52
FLOOR = 4.0 * EPS
MARGIN = 10.0
DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN
POLY, EXP = proto.POLY, proto.EXP
BANDS_BAR = tr.BANDS_BAR
ENH_FAMILY_BAR = 1e-11                  # the reaction-row tests' bar against the float64 restatement, M <= 22


_zero, _hp, _h = tr._zero, tr._hp, tr._h


def _const(v):
    return lambda x: float(v) + 0.0 * np.asarray(x, dtype=np.float64)


def kernel_rule(nquad):
    """(xi, w) of the device's rule on [0, 1]: the decimal constants of csrc/lssvr_p1.hpp, rounded as the compiler
    rounds them, so that the numpy restatement and the prototype loops multiply by the very doubles the kernel does."""
    src = open(os.path.join(ROOT, "hybrid_fem_lssvr_amd", "csrc", "lssvr_p1.hpp")).read()
    out = []
    for nm in ("X", "W"):
        m = re.search(r"static const double %s%d\[\] = \{([^}]*)\};" % (nm, nquad), src)
        out.append(np.array([float(t) for t in m.group(1).replace("\n", " ").split(",")]))
    assert len(out[0]) == len(out[1]) == nquad
    return out[0], out[1]


# ---- the host mirror and the numpy restatement of lssvr_ts_nl_assemble ----------------------------------------------------
def assemble_host(x, u, a_q, cs_q, q_q, r, kind, check=True, ne=None, nquad=None, nterm=None, outs=None, drop=()):
    """lssvr_ts_nl_assemble_host -> (rc, diag, off, rhs).  ``drop``: names of pointers handed over as NULL; ``outs``:
    the three output arrays to pass instead of fresh ones (the aliasing refusals)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    v = dict(x=_h(x), u=_h(u), a_q=_h(a_q), cs_q=_h(cs_q), q_q=_h(q_q), r=_h(r))
    n = len(v["x"]) - 1
    o = [np.full(n + 1, np.nan), np.full(n, np.nan), np.full(n + 1, np.nan)] if outs is None else list(outs)
    names = ("diag", "off", "rhs")
    ptr = {k: (None if k in drop else _hp(t)) for k, t in v.items()}
    optr = [None if names[i] in drop else _hp(o[i]) for i in range(3)]
    rc = lib.lssvr_ts_nl_assemble_host(ptr["x"], ptr["u"], ptr["a_q"], ptr["cs_q"], ptr["q_q"], ptr["r"],
                                       n if ne is None else ne, v["cs_q"].shape[1] if nquad is None else nquad, kind,
                                       v["q_q"].shape[0] if nterm is None else nterm, *optr)
    if check:
        _capi.check(rc, "lssvr_ts_nl_assemble_host")
    return (rc, *o)


def assemble_numpy(x, u, a_q, cs_q, q_q, r, kind):
    """(diag, off, rhs) by the prototype's float64 statement of the order of sums, on the kernel's rule."""
    return proto.newton_system(np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64), a_q, cs_q, q_q,
                               np.asarray(r, dtype=np.float64), kind, kernel_rule(cs_q.shape[1]))


def kernel_inputs(ne, nquad, kind, nterm, seed=0):
    """Seeded inputs of the kernel on a non-uniform mesh: x, the iterate u, r, and the tables a (positive), cs
    (positive), q [nterm, ne, nquad]."""
    rng = np.random.default_rng(1000 * seed + ne % 9973 + 17 * nquad + 31 * nterm + 7 * kind)
    q = rng.uniform(-1.0, 1.0, (nterm, ne, nquad))
    if kind == EXP:
        q[1] = rng.uniform(-1.5, 1.5, (ne, nquad))
    return dict(x=np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, ne))]) / ne, u=rng.uniform(-1.5, 1.5, ne + 1),
                r=rng.standard_normal(ne + 1), a=rng.uniform(0.5, 2.0, (ne, nquad)), cs=rng.uniform(1.0, 40.0, (ne, nquad)),
                q=q)


def exp_terms(d, with_a=True):
    """Per entry of (diag [ne+1], off [ne], rhs [ne+1]) of kernel_inputs with kind EXP, the sum of the sizes of the
    entry's terms: the assembly of |a|, |cs| + |g_u| and |g| + |g_u u_h|, plus |r| in rhs -- the scale of the EXP
    bars (a changed exp moves every term it enters by that many ulps of the term, and the sums after it round on the
    same scale)."""
    nquad = d["cs"].shape[1]
    rule = kernel_rule(nquad)
    uh = d["u"][:-1, None] + (d["u"][1:] - d["u"][:-1])[:, None] * rule[0][None, :]
    g, gu = proto.family(EXP, np.abs(d["q"]) * 0 + d["q"], uh)
    dg, of, ld = proto.p1_system(d["x"], np.abs(d["a"]) if with_a else None, np.abs(d["cs"]) + np.abs(gu),
                                 np.abs(g) + np.abs(gu * uh), rule)
    kk = (np.sum(rule[1][None, :] * np.abs(d["a"]), axis=1) if with_a else 1.0) / np.diff(d["x"])
    return dg, of + 2.0 * kk, ld + np.abs(d["r"])          # (p1_system's off is m_lr - k: put |k| back in, twice)


# ---- the cases of the loop ---------------------------------------------------------------------------------------------------
class Case(tr.Case):
    """tr.Case with the semilinear term ``nonlinear`` = ("poly", [q...]) / ("exp", q0, q1) and the iteration count."""

    def __init__(self, name, nodes, u0, t_end, nsteps, nonlinear, scheme="bdf2", newton_iters=3, **kw):
        super().__init__(name, nodes, u0, t_end, nsteps, scheme, **kw)
        self.nonlinear, self.newton_iters = nonlinear, newton_iters

    def run(self, dtype=np.float64, bands=None):
        return proto.solve(self.nodes, self.u0, self.t_end, self.nsteps, self.scheme, self.nonlinear, a=self.a,
                           c=self.c, rho=self.rho, forcing=self.forcing, kinds=self.kinds, kappa=self.kappa,
                           end_data=self.end_data, snapshots=self.snapshots, newton_iters=self.newton_iters,
                           dtype=dtype, bands=bands, rule=kernel_rule(2))

    def facade(self, M=9, n_colloc=16, gamma=1e4):
        ctor, call = super().facade(M, n_colloc, gamma)
        call.update(nonlinear=self.nonlinear, newton_iters=self.newton_iters)
        return ctor, call


CUBIC_NE = (2, 5, 32, 33)
CUBIC_DT, CUBIC_STEPS = 0.01, 40


def cubic(ne, scheme, nsteps=CUBIC_STEPS, t_end=None, snapshots=None, newton_iters=3):
    """Case A: u_t - u'' + u^3 = f with u = exp(-t) sin(pi x) on (0, 1), zero Dirichlet ends, R = 2."""
    u0, nl, forcing, _ = proto.cubic_manufactured()

    def start(x):
        v = u0(x)
        return np.where((np.asarray(x) == 0.0) | (np.asarray(x) == 1.0), 0.0, v)
    return Case(f"cubic-{scheme}-{ne}", np.linspace(0.0, 1.0, ne + 1), start, CUBIC_DT * nsteps if t_end is None
                else t_end, nsteps, nl, scheme, newton_iters, forcing=forcing,
                snapshots=list(range(1, nsteps + 1)) if snapshots is None else snapshots)


def _general(nonlinear, name, nsteps=40, snapshots=(20, 40)):
    g = tr.general(nsteps, snapshots)
    return Case(name, g.nodes, g.u0, 0.4, nsteps, nonlinear, "bdf2", 3, a=g.a, da=g.da, c=g.c, rho=g.rho,
                forcing=g.forcing, kinds=g.kinds, kappa=g.kappa, end_data=g.end_data, snapshots=list(snapshots))


def general_poly(**kw):
    """Case B: the non-uniform 33-node problem of tr.general (variable a, c, rho, Robin left, moving Dirichlet right)
    with four x-dependent POLY terms."""
    return _general(("poly", [lambda x: 0.2 * np.sin(x), lambda x: 0.5 + 0.25 * x, lambda x: 0.3 * np.cos(2.0 * x),
                              lambda x: 1.0 + 0.5 * x * x]), "general-poly-33", **kw)


def general_exp(**kw):
    """Case C: the same problem with g = q0 exp(q1 u), both x-dependent."""
    return _general(("exp", lambda x: 0.5 + 0.2 * np.cos(x), lambda x: 0.8 + 0.1 * x), "general-exp-33", **kw)


CASES = {"general-poly-33": general_poly, "general-exp-33": general_exp,
         **{f"cubic-{s}-{ne}": (lambda s=s, ne=ne: cubic(ne, s)) for s in ("bdf1", "bdf2") for ne in CUBIC_NE}}

# max over the snapshots of |u - u_longdouble|_inf / |u0|_inf, float64 prototype on its own assembly, when the cases
# were written (a record: the tests read the figure afresh).  The device's figures are in DESIGN.md section 28.
LOOP_READ = {"cubic-bdf1-2": 4.6e-16, "cubic-bdf1-5": 9.0e-16, "cubic-bdf1-32": 1.6e-15, "cubic-bdf1-33": 2.8e-15,
             "cubic-bdf2-2": 1.4e-15, "cubic-bdf2-5": 9.6e-16, "cubic-bdf2-32": 1.6e-15, "cubic-bdf2-33": 2.8e-15}

def references(name, bands=None):
    """(case, np.longdouble loop, float64 loop), computed once per (name, bands)."""
    return tr.references(CASES, name, bands)


def loop_reading(name, nodal, bands=None):
    """(error of ``nodal``, bar, the float64 prototype's own error) against the np.longdouble loop, / |u0|_inf."""
    case, ref, p64 = references(name, bands)
    err, read = (float(np.max(np.abs(np.asarray(v, dtype=np.longdouble) - ref["nodal"]))) / case.scale
                 for v in (nodal, p64["nodal"]))
    return err, max(MARGIN * read, FLOOR), read


def monitor_terms(case, ref):
    """[nsteps] the size of the terms of a residual row, per step: max_i (|A| |v|)_i + |b|_i is bounded by the
    prototype's own products on the longdouble iterates; taken as max |diag| max |v| (3 + 1), the three products of a
    row and its right-hand side, from the float64 mass bands and the case's step: a scale, not a reading."""
    dt = case.t_end / case.nsteps
    h = float(np.min(np.diff(case.nodes)))
    amax = 1.0 if case.a is None else float(np.max(np.abs(case.a(case.nodes))))
    rho = 1.0 if case.rho is None else float(np.max(np.abs(case.rho(case.nodes))))
    vmax = float(np.max(np.abs(np.asarray(ref["newton"][:, :, 2], dtype=np.float64))))
    return 4.0 * (2.0 * amax / h + 1.5 * rho * float(np.max(np.diff(case.nodes))) / dt) * max(vmax, 1.0)


def monitor_reading(name, newton, bands=None):
    """(error, bar, prototype's own) of the monitor table [nsteps, iters, 4] against the longdouble loop's: columns 0
    (residual) scaled by the residual's terms (monitor_terms), columns 1 and 2 by |u0|_inf; the count must be equal."""
    case, ref, p64 = references(name, bands)
    sc = np.array([monitor_terms(case, ref), case.scale, case.scale])

    def err(t):
        t = np.asarray(t, dtype=np.longdouble)
        return float(np.max(np.abs(t[:, :, :3] - ref["newton"][:, :, :3]) / sc))
    assert np.array_equal(np.asarray(newton)[:, :, 3], np.asarray(ref["newton"][:, :, 3], dtype=np.float64))
    read = err(p64["newton"])
    return err(newton), max(MARGIN * read, FLOOR), read


def bands_error(case, bands):
    """tr.bands_error: mass, the linear step matrices K + (alpha / dt) M and the loads against the oracle's assembly."""
    return tr.bands_error(case, bands)


# ---- the enhanced snapshots -------------------------------------------------------------------------------------------------
def enhanced_rows(case, r, M, n_colloc, gamma=1e4):
    """W [ns, ne, M]: the oracle's reaction rows fed the restated c_eff = c + g_u(x, I_h u) and
    f_eff = f(., t) - rho I_h w - g + g_u I_h u, on the loop data ``r`` (nodal, diffs, phi, g of the snapshots)."""
    kind = {"poly": POLY, "exp": EXP}[case.nonlinear[0]]
    qf = list(case.nonlinear[1]) if kind == POLY else list(case.nonlinear[1:])
    fl = [f for _, f in case.forcing]
    rho = tr.proto._one if case.rho is None else case.rho
    cf = _zero if case.c is None else case.c
    out = []
    for k in range(len(case.snapshots)):
        u, w = (np.asarray(r[nm][k], dtype=np.float64) for nm in ("nodal", "diffs"))

        def parts(x, u=u):
            x = np.asarray(x, dtype=np.float64)
            uh = np.interp(x, case.nodes, u)
            g, gu = proto.family(kind, np.stack([proto.table(f, x) for f in qf]), uh)
            return uh, g, gu

        def rhs(x, k=k, w=w):
            uh, g, gu = parts(x)
            f = sum(r["phi"][k][i] * np.asarray(fl[i](x), dtype=np.float64) for i in range(len(fl)))
            return (f - rho(x) * np.interp(x, case.nodes, w) - g) + gu * uh

        gk = r["g"][k]
        bl = float(gk[0]) if case.kinds[0] == DIRICHLET else float(u[0])
        br = float(gk[1]) if case.kinds[1] == DIRICHLET else float(u[-1])
        out.append(orc.enhance_all_vec(case.nodes, u, M, gamma, n_colloc, rhs=rhs,
                                       coef_a=tr.proto._one if case.a is None else case.a,
                                       coef_da=tr.proto._zero if case.da is None else case.da,
                                       coef_c=lambda x: cf(x) + parts(x)[2], bc_left=bl, bc_right=br))
    return np.stack(out)


def enhanced_reference(name, M, n_colloc, bands=None):
    """(W on the np.longdouble loop's data, bar, noise): the bar is the larger of the family's 1e-11 and 10x the noise
    that the float64 loop's own rounding -- amplified by 1 / dt in w -- puts into W (the rule of tr.enhanced_reference)."""
    case, ref, p64 = references(name, bands)
    Wl, W64 = enhanced_rows(case, ref, M, n_colloc), enhanced_rows(case, p64, M, n_colloc)
    noise = max(float(orc.rel_l2_coef(W64[k], Wl[k]).max()) for k in range(len(Wl)))
    return Wl, max(ENH_FAMILY_BAR, MARGIN * noise), noise


# ---- what solve_transient(..., nonlinear=...) refuses: (name, constructor kwargs, call kwargs, a fragment of the message) ---
def refusals():
    ok = ("poly", [_zero, _zero, _zero, _const(1.0)])
    nl = dict(nsteps=4, nonlinear=ok)
    nan_q = ("poly", [lambda x: np.full_like(np.asarray(x, dtype=np.float64), np.nan)])
    node_q = ("poly", [lambda x: np.where(np.asarray(x) == -1.0, np.inf, 1.0)])      # a collocation point only
    me = "solve_transient "
    # the message of a solver built with nonlinear= points at the keyword of the call
    own = "build the solver without nonlinear= and call solve_transient(..., nonlinear=...)"
    family = "nonlinear must be ('poly', [q0, q1, ...]) or ('exp', q0, q1)"
    return [
        ("nonlinear on the solver", dict(nonlinear=ok), dict(nsteps=4), own),
        ("nonlinear on the solver and the call", dict(nonlinear=ok), nl, own),
        ("newton_iters without nonlinear", {}, dict(nsteps=4, newton_iters=3),
         "newton_iters and newton_tol belong to solve_transient(..., nonlinear=...)"),
        ("newton_tol without nonlinear", {}, dict(nsteps=4, newton_tol=1e-8),
         "newton_iters and newton_tol belong to solve_transient(..., nonlinear=...)"),
        ("a callable of u", {}, dict(nsteps=4, nonlinear=lambda x, u: u ** 3),
         family + ": g comes from a tabulated family, not from a callable of u"),
        ("unknown family", {}, dict(nsteps=4, nonlinear=("cubic", [_zero])), family + ", got ('cubic', ["),
        ("7 terms", {}, dict(nsteps=4, nonlinear=("poly", [_zero] * 7)), "nonlinear 'poly' takes 1 .. 6 terms (nterm), got 7"),
        ("exp with one table", {}, dict(nsteps=4, nonlinear=("exp", _zero)),
         "nonlinear=('exp', q0, q1) takes the two callables q0(x), q1(x)"),
        ("newton_iters 0", {}, dict(newton_iters=0, **nl), "newton_iters must be an integer in 1 .. 8, got 0"),
        ("newton_iters 9", {}, dict(newton_iters=9, **nl), "newton_iters must be an integer in 1 .. 8, got 9"),
        ("newton_iters 2.5", {}, dict(newton_iters=2.5, **nl), "newton_iters must be an integer in 1 .. 8, got 2.5"),
        ("newton_tol 0", {}, dict(newton_tol=0.0, **nl), "newton_tol must be finite and > 0, got 0.0"),
        ("newton_tol nan", {}, dict(newton_tol=math.nan, **nl), "newton_tol must be finite and > 0, got nan"),
        ("q not finite", {}, dict(nsteps=4, nonlinear=nan_q), "nonlinear q_0 is not finite at a quadrature point"),
        ("q not finite at a node", {}, dict(nsteps=4, nonlinear=node_q),
         "nonlinear q_0 is not finite at a collocation point"),
        ("q of the wrong shape", {}, dict(nsteps=4, nonlinear=("poly", [lambda x: np.ones(3)])),
         "nonlinear q_0 must return one value per point ([8, 2] at the quadrature points)"),
        ("n_colloc > 64 with enhance", dict(n_colloc=65, lssvr_M=9), nl,
         "nonlinear needs n_colloc <= 64 for the enhanced snapshots, got 65"),
        ("convection", dict(convection=lambda x: 0.0 * x), nl, me + tr.STRUCTURAL[0]),
        ("periodic", dict(boundary="periodic", reaction=lambda x: 1.0 + 0.0 * x), nl, me + tr.STRUCTURAL[1]),
        ("fem_solver flux", dict(fem_solver="flux"), nl, me + tr.STRUCTURAL[2]),
        ("fem_solver pivot", dict(fem_solver="pivot"), nl, me + tr.STRUCTURAL[2]),
        ("element_degrees", dict(_degrees=True), nl, me + tr.STRUCTURAL[3]),
        ("solver", dict(solver=1), nl, me + tr.STRUCTURAL[4]),
        ("rho <= 0", {}, dict(weight=lambda x: x, **nl), tr.RHO_MSG),
        ("c + rho/dt < 0", dict(reaction=lambda x: -100.0 + 0.0 * x), nl,
         "c + rho / dt < 0 at a quadrature point (dt = 0.1)"),
        ("snapshot past the end", {}, dict(snapshots=[2, 5], **nl),
         "snapshots must be step indices in 1 .. nsteps = 4, got [2, 5]"),
        ("scheme", {}, dict(scheme="bdf3", **nl), "scheme must be 'bdf1' or 'bdf2', got 'bdf3'"),
    ]


def passing():
    """A well-formed call gets as far as the device."""
    return [(dict(lssvr_M=9, n_colloc=16), dict(nsteps=4, nonlinear=refusals()[1][2]["nonlinear"]))]
