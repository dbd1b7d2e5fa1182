"""Shared cases, restatement and bars of the semilinear sensitivity tests:
tests/test_semilinear_sensitivity_cpu.py runs them through the numpy prototype and the library's host mirror,
tests/test_gpu_semilinear_sensitivity.py through the device.

The restatement is scripts/proto/semilinear_sensitivity_proto.py: the dense assembly, the facade's damped Newton
iteration in float64, the complex-step derivative (from the converged u*, full Newton steps in complex arithmetic: no
subtraction) and the adjoint formulas in the order of csrc/lssvr_sens.hpp and csrc/lssvr_nl_sens.hpp.  As in
tests/sensitivity_rules.py the bar of a case is MARGIN = 10x what the float64 prototype itself reads on the SAME case --
the deviation of its adjoint gradients from the complex step, the largest over the groups (the tables a, b, c, f, every
q_k, the end data), each relative to the largest entry of its group.  The reading is taken when the test runs (cached),
never from the code under test; READ records what it was when the cases were written."""
import ctypes
import functools

import numpy as np

import sensitivity_rules as sr          # (puts the repository and scripts/proto on sys.path)

import semilinear_sensitivity_proto as proto         # noqa: E402

MARGIN, READ_SLACK = sr.MARGIN, sr.READ_SLACK
D, R = sr.D, sr.R
POLY, EXP = proto.POLY, proto.EXP
TABLES = ("a", "b", "c", "f", "q")
CANARY = sr.CANARY
EPS = 2.0 ** -52
# the largest reading of the prototype over the cases of each mesh, when they were written; the prototype must stay
# within READ_SLACK of it (another LAPACK build may round otherwise; the control, g_u forgotten, reads 2.5e-1)
READ = {7: 1.1e-14, 33: 2.0e-13}
# the control: z from K^T alone must read above this multiple of the case's bar
CONTROL_FACTOR = 100.0

# the linear limit (test 8): g = c0(x) u
proto.LAWS.setdefault("linear", (POLY, [proto.zero, lambda x: 0.5 + 0.25 * x]))


class Case:
    """One problem: the law (a key of proto.LAWS), ``ne`` non-uniform elements, ``nq`` points, with or without b and c,
    the end kinds and the functional ("random": any nodal p; "goal": int (1 + x^2) u; "observe": the misfit at 9
    points)."""

    def __init__(self, law, ne, nq, conv, react, kinds, functional="random"):
        self.law, self.ne, self.nq, self.conv, self.react = law, ne, nq, conv, react
        self.kinds, self.functional = tuple(kinds), functional
        self.x = proto.mesh(ne, law)
        self.kind, self.tabs = proto.case_tables(self.x, nq, conv, react, law)
        self.nterm = len(self.tabs["q"])
        self.J = proto.functional(self.x, functional, nq)
        self.kappa, self.g = proto.KAPPA, proto.END_DATA

    @property
    def id(self):
        return (f"{self.law}-ne{self.ne}-q{self.nq}-{'b' if self.conv else ''}{'c' if self.react else ''}-"
                f"{''.join('DR'[k] for k in self.kinds)}-{self.functional}")

    @functools.cached_property
    def reference(self):
        """(reading, adjoint dict, complex-step dict) of the prototype."""
        return proto.reading(self.x, self.tabs, self.kind, self.kinds, self.J, self.kappa, self.g)

    @property
    def bar(self):
        return MARGIN * self.reference[0]

    def forgotten_gu(self):
        """The gradients of the control: z from K^T alone, g_u forgotten in the Jacobian."""
        return proto.adjoint_gradients(self.x, self.tabs, self.kind, self.kinds, self.kappa, self.g, self.J,
                                       forget_gu=True)


@functools.lru_cache(maxsize=None)
def case(*key):
    return Case(*key)


def cpu_cases():
    """Test 1, per mesh (7 and 33 elements): the cubic with and without b and c, nquad 1, 2, 5, the four end
    combinations; the cubic with "goal" and "observe"; POLY nterm 1 and 6; Bratu (Dirichlet-Dirichlet and
    Dirichlet-Robin: with a Robin end on the left this data has no solution) with nquad 1, 2, 5."""
    out = []
    for ne in (7, 33):
        for conv in (False, True):
            for nq in (1, 2, 5):
                out += [case("cubic", ne, nq, conv, conv, kinds) for kinds in proto.END_COMBOS]
        out += [case("cubic", ne, 2, True, True, (D, R), fn) for fn in ("goal", "observe")]
        out += [case(law, ne, 2, conv, True, kinds) for law in ("poly1", "poly6") for conv, kinds in
                ((False, (R, D)), (True, (D, R)))]
        out += [case("bratu", ne, nq, False, False, (D, D)) for nq in (1, 2, 5)]
        out += [case("bratu", ne, 2, False, False, (D, R), fn) for fn in ("random", "observe")]
    return out


def control_case():
    return case("cubic", 33, 2, True, True, (D, R), "goal")


def facade_cases():
    """Test 7, 33 elements, nquad 2 -> (case, fem_solver): the cubic on "bands" (with c: c + g_u > 0) with the four end
    combinations, goal and observe; the cubic with convection on "pivot"; Bratu on "pivot", Dirichlet-Robin."""
    out = []
    for kinds in proto.END_COMBOS:
        out += [(case("cubic", 33, 2, False, True, kinds, fn), "bands") for fn in ("goal", "observe")]
    out.append((control_case(), "pivot"))
    out += [(case("bratu", 33, 2, False, False, (D, R), fn), "pivot") for fn in ("goal", "observe")]
    return out


def facade_solver(c, fem_solver, nonlinear=True, reaction=None, **kw):
    """The facade configured for the case ``c`` (``nonlinear`` False: the linear solver with ``reaction``)."""
    import hybrid_fem_lssvr_amd as pkg
    sp = proto.sp
    ends = tuple(("robin", c.kappa[s], c.g[s]) if c.kinds[s] == R else ("dirichlet", c.g[s]) for s in range(2))
    kind, q = proto.LAWS[c.law]
    bratu = c.law == "bratu"
    if nonlinear:
        kw["nonlinear"] = ("poly", list(q)) if kind == POLY else ("exp", *q)
    if reaction is None:
        reaction = sp.reaction if c.react else None
    return pkg.FEMLSSVRPrimalSolver(mesh=c.x, nquad=c.nq, rhs=proto.zero if bratu else sp.rhs,
                                    coef=None if bratu else (sp.coef_a, sp.coef_da),
                                    convection=sp.convection(c.ne) if c.conv else None, reaction=reaction,
                                    boundary=ends, fem_solver=fem_solver, lssvr_M=9, n_colloc=16, **kw)


def functional_kw(c):
    return dict(goal=proto.goal_density) if c.functional == "goal" else dict(observe=proto.observations(c.x))


def facade_gradients(s, nonlinear=True):
    """The gradient dict (the groups of proto.deviation) of a Sensitivity ``s``."""
    return dict(a=s.d_coef, b=s.d_convection, c=s.d_reaction, f=s.d_rhs, q=s.d_nonlinear if nonlinear else None,
                ends=np.concatenate([s.d_end_values, s.d_kappa]))


# ---- the kernel's inputs and the host mirror ---------------------------------------------------------------------------------
def kernel_inputs(ne, nq, nc, nu, nterm, seed=0):
    """sensitivity_rules.kernel_inputs and q_tabs [nterm, ne, nq], random, of size 1."""
    d = sr.kernel_inputs(ne, nc, nu, seed)
    d["q"] = np.random.default_rng(7 * ne + 13 * nq + nterm + seed).standard_normal((nterm, ne, nq))
    return d


_hp = sr._hp


def nl_host(x, nq, U, Z, kind, nterm, q_tabs=None, want=TABLES, P=None, band_ends=None, kinds=(D, D), ends=False,
            check=True):
    """lssvr_semilinear_sensitivity_host -> (rc, dict): the tables a, b, c, f [nc, ne, nq] and q [nc, nterm, ne, nq],
    canary-filled where they are not in ``want`` (and then not handed over), and "ends" [nc, 4] likewise with
    ``ends``."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    x, U, Z, P, band_ends, q_tabs = (None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.float64))
                                     for t in (x, U, Z, P, band_ends, q_tabs))
    nc, ne = Z.shape[0], len(x) - 1
    out = {k: np.full((nc, ne, int(nq)), CANARY) for k in TABLES[:4]}
    out["q"] = np.full((nc, max(int(nterm), 1), ne, int(nq)), CANARY)
    out["ends"] = np.full((nc, 4), CANARY)
    rc = lib.lssvr_semilinear_sensitivity_host(
        _hp(x), ne, int(nq), _hp(U), U.shape[0], _hp(Z), nc, _hp(q_tabs), int(kind), int(nterm),
        *(_hp(out[k]) if k in want else None for k in TABLES), _hp(P), _hp(band_ends), int(kinds[0]), int(kinds[1]),
        _hp(out["ends"]) if ends else None)
    if check:
        _capi.check(rc, "lssvr_semilinear_sensitivity_host")
    return rc, out


def nl_numpy(x, nq, U, Z, kind, nterm, q_tabs=None, P=None, band_ends=None, kinds=(D, D)):
    """The same dict from the numpy restatement of the formulas, in the order of the two headers."""
    out = sr.sens_numpy(x, nq, U, Z, P, band_ends, kinds)
    out["q"] = proto.nl_gradients(x, U, Z, nq, kind, nterm, q_tabs)
    return out


WANTS = (TABLES, ("q",), ("a",), ("f", "q"), ("b", "c"), ("c", "q"), ("a", "b", "c", "f"))


def exp_bars(x, nq, U, Z, q_tabs):
    """The per-entry bars [nc, 2, ne, nq] of gq for EXP: 8 eps |s E| (1 + |q_1 u_q|) for gq_0 and
    8 eps |s q_0 u_q E| (1 + |q_1 u_q|) for gq_1 -- the two exp implementations differ by an ulp or so of E, whose
    argument q_1 u_q is itself rounded (exp_bar_scale of tests/semilinear_rules.py, through one more product)."""
    xi, w = proto.sp.gauss01(nq)
    U, Z = np.atleast_2d(U), np.atleast_2d(Z)
    U = np.broadcast_to(U, Z.shape)
    h = np.diff(x)[None, :, None]
    om = 1.0 - xi
    s = (h * w) * (Z[:, :-1, None] * om + Z[:, 1:, None] * xi)
    uq = U[:, :-1, None] * om + U[:, 1:, None] * xi
    E = np.exp(q_tabs[1][None] * uq)
    amp = 1.0 + np.abs(q_tabs[1][None] * uq)
    return 8.0 * EPS * np.stack([np.abs(s * E) * amp, np.abs(s * q_tabs[0][None] * uq * E) * amp], axis=1)


def check_against(got, want_tables, ref, ends, kind=POLY, qbar=None):
    """``got`` (canary-prefilled) equals ``ref`` bit for bit in every table of ``want_tables`` (and in the ends with
    ``ends``) -- "q" of EXP within ``qbar`` per entry -- and holds its canaries everywhere else; for POLY gq_0 is -gf
    and gq_1 is gc, bit for bit, where both were asked for."""
    for k in TABLES:
        if k not in want_tables:
            assert np.all(got[k] == CANARY), f"{k} was written though it was not asked for"
        elif k == "q" and kind == EXP:
            assert np.all(np.abs(got[k] - ref[k]) <= qbar), "q"
        else:
            assert np.array_equal(got[k], ref[k]), k
    if ends:
        assert np.array_equal(got["ends"], ref["ends"])
    else:
        assert np.all(got["ends"] == CANARY)
    if kind == POLY and "q" in want_tables:
        if "f" in want_tables:
            assert np.array_equal(got["q"][:, 0], -got["f"])
        if "c" in want_tables and got["q"].shape[1] > 1:
            assert np.array_equal(got["q"][:, 1], got["c"])


# ---- the inverse problem of the prototype --------------------------------------------------------------------------------
DEMO_FINAL = 8.635556e-05       # the misfit after 20 steps, as the prototype prints it
DEMO_RTOL = 1e-6                   # (the agreement tests/test_sensitivity_cpu.py asks of sensitivity_rules.DEMO_FINAL)
