"""Shared cases, restatement and bars of the semilinear transient sensitivity tests:
tests/test_transient_nl_sensitivity_cpu.py runs them through the numpy prototype and the library's host mirrors,
tests/test_gpu_transient_nl_sensitivity.py through the device.

The restatement is scripts/proto/transient_nl_sensitivity_proto.py: the facade's semilinear BDF loop in float64, the
adjoint of the converged implicit step in the kernels' order of operations, and the complex step through the whole loop
(one datum perturbed by i 1e-30, every step's Newton iteration in complex arithmetic until its increment is below 1e-14:
no subtraction).  As in section 35 the bar of a case is MARGIN = 10x what the float64 prototype itself reads on the SAME
case -- the largest deviation of its adjoint gradients from the complex step over the groups a, c, rho, each f_r, each
q_k, u0, the end values and kappa, each relative to its own largest entry.  The reading is taken when the test runs
(cached), never from the code under test; READ records what it was when the cases were written."""
import ctypes
import functools

import numpy as np

import transient_sensitivity_rules as tr          # (puts the repository and scripts/proto on sys.path)
import semilinear_sensitivity_rules as nr

import transient_nl_sensitivity_proto as proto         # noqa: E402

tsp, sp = proto.tsp, proto.sp
MARGIN, READ_SLACK = 10.0, 4.0
D, R = tr.D, tr.R
POLY, EXP = proto.POLY, proto.EXP
END_COMBOS = sp.END_COMBOS
TABLES = ("a", "c", "rho", "f", "q")
CANARY = tr.CANARY
_hp, _c = tr._hp, tr._c
NEWTON_ITERS = 6          # the last increment is then at rounding level: the converged-step assumption costs nothing
# the largest reading of the prototype over the cases of each mesh, when they were written; the prototype must stay
# within READ_SLACK of it (another LAPACK build may round otherwise; the control, g_u left out of J_n, reads 1e-2 and more)
READ = {7: 7.1e-15, 33: 3.8e-14}
# the control: lambda from K + M(c + alpha rho / dt) alone must read above this multiple of the case's bar
CONTROL_FACTOR = 100.0


class Case:
    """One loop: the law (a key of proto.LAWS), ``ne`` non-uniform elements, ``nq`` points, the end kinds, the scheme,
    ``N`` steps and the functional ("goal": over several steps; "observe": the misfit at 9 points and two steps)."""

    def __init__(self, law, ne, nq, kinds, scheme, N, functional="goal"):
        self.law, self.ne, self.nq, self.kinds, self.scheme, self.N = law, ne, nq, tuple(kinds), scheme, N
        self.kind = functional
        self.p = proto.problem(law, ne, nq, kinds, scheme, N)
        self.J = proto.functional(self.p, functional)

    @property
    def id(self):
        return (f"{self.law}-ne{self.ne}-q{self.nq}-{''.join('DR'[k] for k in self.kinds)}-{self.scheme}-N{self.N}-"
                f"{self.kind}")

    @functools.cached_property
    def reference(self):
        """(reading, adjoint dict, complex-step dict) of the prototype with NEWTON_ITERS iterations per step."""
        return proto.reading((self.p, self.J), NEWTON_ITERS)

    @property
    def read(self):
        return self.reference[0]

    @property
    def bar(self):
        return MARGIN * self.read

    def deviation(self, grads):
        """The largest group deviation of ``grads`` from the complex step."""
        return max(proto.deviations(grads, self.reference[2]).values())


@functools.lru_cache(maxsize=None)
def case(*key):
    return Case(*key)


def cpu_cases():
    """7 elements: the cubic with the four end combinations x N = 3, 11, while nquad 1, 2, 5, the two schemes and the two
    functionals rotate; POLY nterm 1 and 6 and EXP with N = 3 and 11; 33 elements: the control case."""
    out = []
    for ki, kinds in enumerate(END_COMBOS):
        for j, N in enumerate((3, 11)):
            r = ki + j
            out.append(case("cubic", 7, (1, 2, 5)[r % 3], kinds, ("bdf2", "bdf1")[(ki // 2 + j) % 2], N,
                            ("goal", "observe")[r % 2]))
    for law in ("poly1", "poly6", "exp"):
        out += [case(law, 7, 2, (D, R), "bdf2", 3, "goal"), case(law, 7, 5, (R, D), "bdf1", 11, "observe")]
    out.append(control_case())
    return out


def control_case():
    return case("cubic", 33, 2, (D, R), "bdf2", 11, "goal")


def facade_cases():
    """33 elements, nquad 2, N = 11 (chunks 8 + 3): the cubic with the four end combinations on BDF2, goal and observe
    alternating; the cubic on BDF1; EXP with goal and with observe."""
    out = [case("cubic", 33, 2, kinds, "bdf2", 11, ("goal", "observe")[ki % 2]) for ki, kinds in enumerate(END_COMBOS)]
    out.append(case("cubic", 33, 2, (R, D), "bdf1", 11, "goal"))
    out += [case("exp", 33, 2, (D, R), "bdf2", 11, "observe"), case("exp", 33, 2, (R, R), "bdf2", 11, "goal")]
    return list(dict.fromkeys(out))


def law_spec(law):
    kind, q = proto.LAWS[law]
    return ("poly", list(q)) if kind == POLY else ("exp", *q)


def facade_solver(c, reaction=None, **kw):
    """The facade configured for the case ``c``."""
    import hybrid_fem_lssvr_amd as pkg
    ends = [("robin", float(c.p.kappa[s]), 0.0) if c.kinds[s] == R else ("dirichlet", 0.0) for s in range(2)]
    return pkg.FEMLSSVRPrimalSolver(mesh=c.p.x, nquad=c.nq, coef=(sp.coef_a, sp.coef_da),
                                    reaction=sp.reaction if reaction is None else reaction, boundary=tuple(ends),
                                    lssvr_M=9, n_colloc=16, **kw)


def facade_args(c, nonlinear=True):
    """The keywords of solve_transient / solve_transient_sensitivity for the loop of ``c`` (without the functional)."""
    kw = dict(nsteps=c.N, scheme=c.scheme, weight=tsp.weight, forcing=[(f, fx) for f, fx in tsp.FORCING],
              end_data=(tsp.g_left, tsp.g_right))
    if nonlinear:
        kw.update(nonlinear=law_spec(c.law), newton_iters=NEWTON_ITERS)
    return kw


def facade_functional(c):
    if c.kind == "goal":
        steps, wts = proto.goal_steps(c.N)
        return dict(goal=sp.goal_density, goal_steps=steps, goal_weights=wts)
    return dict(observe=tsp.observations(c.N))


def facade_gradients(s, nonlinear=True):
    """The gradient dict (the groups of proto.deviations) of a TransientSensitivity ``s``."""
    return dict(a=s.d_coef, c=s.d_reaction, rho=s.d_weight, f=s.d_forcing, q=s.d_nonlinear if nonlinear else None,
                u0=s.d_u0, g=s.d_end_values, kappa=s.d_kappa)


# ---- the chunk pass: inputs, host mirror, numpy restatement ----------------------------------------------------------------
def kernel_inputs(ne, nq, m, nR, nterm, n0=None, bdf1=False, seed=0):
    """tr.kernel_inputs (``bdf1``: every coefficient row BDF1) with band_ends [m, 2], one row per level, and q [nterm, ne,
    nq], random, of size 1."""
    d = tr.kernel_inputs(ne, m, nR, n0, seed)
    rng = np.random.default_rng(77 * ne + 5 * m + nterm + nq + seed)
    d["band_ends"] = rng.standard_normal((m, 2))
    d["band_rows"] = list(range(m))
    d["q"] = rng.standard_normal((nterm, ne, nq))
    if bdf1:
        d["coef"] = np.array([tsp.BDF["bdf1"]] * m)
    return d


def blank(d, nq, nterm, init=None):
    out = tr.blank(d, nq, None if init is None else {k: v for k, v in init.items() if k != "q"})
    out["q"] = np.full((nterm, d["ne"], nq), CANARY) if init is None else np.array(init["q"], dtype=np.float64)
    return out


def initial(d, nq, nterm, seed=1):
    out = tr.initial(d, nq, seed)
    out["q"] = np.random.default_rng(seed + 3 * d["ne"]).standard_normal((nterm, d["ne"], nq))
    return out


def nl_sens_args(d, nq, kind, nterm, out, want, kinds, ends, acc, ptr=_hp, keep=None):
    """The argument list of lssvr_semilinear_transient_sensitivity(_host) on the inputs ``d`` and the outputs ``out``;
    ``keep`` receives the contiguous inputs so that they outlive the call."""
    ins = [_c(d[k]) for k in ("x", "Utraj", "Z", "coef", "phi", "q", "Brows", "band_ends")]
    if keep is not None:
        keep.extend(ins)
    x, U, Z, coef, phi, q, B, be = ins
    return [ptr(x), d["ne"], int(nq), ptr(U), ptr(Z), d["n0"], d["m"], d["inv_dt"], _hp(coef), ptr(phi), d["R"], ptr(q),
            int(kind), int(nterm), *(ptr(out[k]) if k in want else None for k in TABLES), int(acc), ptr(B), ptr(be),
            int(kinds[0]), int(kinds[1]), ptr(out["g"]) if ends else None, ptr(out["kappa"]) if ends else None]


def nl_sens_host(d, nq, kind, nterm, want=TABLES, kinds=(D, D), ends=False, init=None, check=True):
    """lssvr_semilinear_transient_sensitivity_host -> (rc, dict): every table of TABLES, canary-filled where it is not in
    ``want`` (and then not handed over), and "g", "kappa" likewise with ``ends``.  ``init``: accumulate = 1 onto it."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    out, keep = blank(d, nq, nterm, init), []
    rc = lib.lssvr_semilinear_transient_sensitivity_host(
        *nl_sens_args(d, nq, kind, nterm, out, want, kinds, ends, init is not None, keep=keep))
    if check:
        _capi.check(rc, "lssvr_semilinear_transient_sensitivity_host")
    return rc, out


def nl_sens_numpy(d, nq, kind, nterm, kinds=(D, D), init=None):
    """The same dict from the numpy restatement, in the order of csrc/lssvr_chunk_sens.hpp."""
    out = tr.ts_sens_numpy(d, nq, kinds, init)
    out["q"] = proto.chunk_gq(d["x"], nq, d["Utraj"], d["Z"], d["n0"], kind, nterm, d["q"],
                              None if init is None else init["q"])
    return out


def exp_bar(d, nq):
    """The per-entry bar [2, ne, nq] of gq for EXP: that of section 35 (nr.exp_bars) summed over the chunk's levels."""
    nhi = d["n0"] + d["m"] - 1
    return sum(nr.exp_bars(d["x"], nq, d["Utraj"][nhi - i], d["Z"][i], d["q"])[0] for i in range(d["m"]))


def check_against(got, want, ref, ends, init=None, kind=POLY, qbar=None, nterm=None):
    """``got`` equals ``ref`` bit for bit in every table of ``want`` (and in g, kappa with ``ends``) -- "q" of EXP within
    ``qbar`` per entry -- and holds what it was prefilled with everywhere else."""
    for k in TABLES:
        if k not in want:
            assert np.array_equal(got[k], np.full(got[k].shape, CANARY) if init is None else init[k]), \
                f"{k} was written though it was not asked for"
        elif k == "q" and kind == EXP:
            assert np.all(np.abs(got[k] - ref[k]) <= qbar), "q"
        else:
            assert np.array_equal(got[k], ref[k]), k
    if ends:
        assert np.array_equal(got["g"], ref["g"]) and np.array_equal(got["kappa"], ref["kappa"])
    else:
        assert np.all(got["g"] == CANARY)
        assert np.array_equal(got["kappa"], np.full(2, CANARY) if init is None else init["kappa"])
    if kind == POLY and init is None and "q" in want and "c" in want and got["q"].shape[0] > 1:
        assert np.array_equal(got["q"][1], got["c"])          # (both from 0: the same chain of operations)


WANTS = (TABLES, ("q",), ("a",), ("f", "q"), ("c", "rho"), ("c", "q"), ("a", "c", "rho", "f"), ())


def host_sweep(p, U, lam, B, be, size):
    """proto.sweep_gradients through the library's host mirror, in chunks of ``size`` levels."""
    N, nR, nterm = p.N, p.f.shape[0], len(p.q)
    acc = None
    for n0, m in tsp.chunks(N, size):
        steps = [n0 + m - 1 - i for i in range(m)]
        d = dict(x=p.x, Utraj=U, Z=lam[steps], Brows=B[steps], phi=p.phi, band_ends=be[steps], q=p.q,
                 coef=np.array([tsp.coefficients(p.scheme, n, N) for n in steps]), n0=n0, inv_dt=1.0 / p.dt, R=nR, m=m,
                 ne=len(p.x) - 1)
        if acc is None:
            got = nl_sens_host(d, p.nq, p.kind, nterm, kinds=p.kinds, ends=True)[1]
            got["g"][:n0] = 0.0
        else:
            got = nl_sens_host(d, p.nq, p.kind, nterm, kinds=p.kinds, ends=True, init=acc)[1]
        acc = got
    gu0 = B[0].copy()
    for s, end in ((0, 0), (1, -1)):
        if p.kinds[s] == D:
            acc["g"][0, s] = B[0][end]
            gu0[end] = 0.0
        else:
            acc["g"][0, s] = 0.0
    return dict(acc, u0=gu0)


# ---- the backward step: inputs, host mirror, the chain it replaces ------------------------------------------------------------
def step_inputs(ne, nq, kind, nterm, nR=1, seed=0):
    """Random inputs of one backward step: x non-uniform, u, the tables a > 0, cs, q [nterm] (EXP: moderate arguments),
    the mass bands, U0, U1 [1, ne+1], loads [nR, ne+1], phi [1, nR]."""
    rng = np.random.default_rng(31 * ne + 7 * nq + nterm + 100 * kind + seed)
    x = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(ne))]) / ne - 0.3
    return dict(x=x, u=rng.standard_normal(ne + 1), a=0.5 + rng.random((ne, nq)), cs=rng.standard_normal((ne, nq)),
                q=rng.standard_normal((nterm, ne, nq)) * (0.5 if kind == EXP else 1.0), mdiag=rng.random(ne + 1) + 1.0,
                moff=rng.random(ne), U0=rng.standard_normal((1, ne + 1)), U1=rng.standard_normal((1, ne + 1)),
                loads=rng.standard_normal((nR, ne + 1)), phi=rng.standard_normal((1, nR)), inv_dt=3.0 + rng.random(),
                ne=ne, nq=nq, kind=kind, nterm=nterm, R=nR)


def step_args(d, b0, b1, out, ptr=_hp, with_a=True, keep=None, **change):
    """The argument list of lssvr_semilinear_adjoint_step(_host); ``change`` replaces entries by name."""
    ins = {k: _c(d[k]) for k in ("x", "u", "a", "cs", "q", "mdiag", "moff", "U0", "U1", "loads", "phi")}
    if keep is not None:
        keep.append(ins)
    a = dict(x=ptr(ins["x"]), u=ptr(ins["u"]), a=ptr(ins["a"]) if with_a else None, cs=ptr(ins["cs"]), q=ptr(ins["q"]),
             ne=d["ne"], nq=d["nq"], kind=d["kind"], nterm=d["nterm"], mdiag=ptr(ins["mdiag"]), moff=ptr(ins["moff"]),
             U0=ptr(ins["U0"]), U1=ptr(ins["U1"]), loads=ptr(ins["loads"]), phi=ptr(ins["phi"]), R=d["R"],
             beta0=float(b0), beta1=float(b1), inv_dt=d["inv_dt"], diag=ptr(out["diag"]), off=ptr(out["off"]),
             B=ptr(out["B"]), be=ptr(out["band_ends"]))
    assert set(change) <= set(a)
    a.update(change)
    return list(a.values())


def step_blank(ne):
    return dict(diag=np.full(ne + 1, CANARY), off=np.full(ne, CANARY), B=np.full((1, ne + 1), CANARY),
                band_ends=np.full(2, CANARY))


def step_host(d, beta0, beta1, with_a=True):
    """lssvr_semilinear_adjoint_step_host -> dict(diag, off, B, band_ends)."""
    from hybrid_fem_lssvr_amd import _capi
    out, keep = step_blank(d["ne"]), []
    _capi.check(_capi.load().lssvr_semilinear_adjoint_step_host(*step_args(d, beta0, beta1, out, with_a=with_a,
                                                                           keep=keep)),
                "lssvr_semilinear_adjoint_step_host")
    return out


def step_chain(d, beta0, beta1, with_a=True):
    """The same dict from the chain the step replaces: lssvr_ts_rhs_host, lssvr_ts_nl_assemble_host at v = u (its
    right-hand side dropped) and the two slices."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    ne = d["ne"]
    x, u, a, cs, q, md, mo, U0, U1, loads, phi = (_c(d[k]) for k in ("x", "u", "a", "cs", "q", "mdiag", "moff", "U0",
                                                                   "U1", "loads", "phi"))
    out = step_blank(ne)
    _capi.check(lib.lssvr_ts_rhs_host(_hp(md), _hp(mo), _hp(U0), _hp(U1), _hp(loads), _hp(phi), ne, 1, d["R"],
                                      float(beta0), float(beta1), d["inv_dt"], _hp(out["B"])), "lssvr_ts_rhs_host")
    r, rhs = np.zeros(ne + 1), np.zeros(ne + 1)
    _capi.check(lib.lssvr_ts_nl_assemble_host(_hp(x), _hp(u), _hp(a) if with_a else None, _hp(cs), _hp(q), _hp(r), ne,
                                              d["nq"], d["kind"], d["nterm"], _hp(out["diag"]), _hp(out["off"]),
                                              _hp(rhs)), "lssvr_ts_nl_assemble_host")
    out["band_ends"] = np.array([out["off"][0], out["off"][ne - 1]])
    return out


# ---- the inverse problem of the prototype and the step that does not converge ------------------------------------------------
DEMO_FINAL = 4.305177e-05         # the misfit after 20 steps, as the prototype prints it
DEMO_RTOL = 1e-6
SLOW_FACTOR = 100.0                # the prototype shows the last increment of the SLOW case this far above tolerance
