"""CPU: adjoint sensitivities of the semilinear BDF loop where there is no GPU -- the two host
mirrors against their numpy restatement and the chain they replace, bit for bit; the prototype's adjoint against its own
complex step through the whole loop; chunk independence; the control with g_u left out; the argument errors of the four
entries and the facade's refusals."""
import ctypes
import re

import numpy as np
import pytest

import transient_nl_sensitivity_rules as ns

proto, tr = ns.proto, ns.tr
D, R, POLY, EXP = ns.D, ns.R, ns.POLY, ns.EXP
KINDS4 = ((D, D), (D, R), (R, D), (R, R))


@pytest.mark.parametrize("nterm", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("m", [1, 2, 8])
@pytest.mark.parametrize("ne", [1, 2, 7, 33])
def test_chunk_mirror_is_the_numpy_restatement(ne, m, nterm):
    """POLY: every output is bit-equal -- each sum is a chain of single IEEE operations in a written order.  n0 = 1 (no
    row n-2) and 4, BDF1 and mixed BDF2 coefficient rows, R = 1 and 3, nquad 1, 2, 5, the four end pairs; every ``want``
    subset leaves canaries (or what an accumulating call started from) in what it was not asked for."""
    for ci, (n0, bdf1, nR) in enumerate(((1, False, 3), (4, True, 1), (4, False, 3))):
        for nq in (1, 2, 5):
            d = ns.kernel_inputs(ne, nq, m, nR, nterm, n0, bdf1)
            for kinds in KINDS4:
                ref = ns.nl_sens_numpy(d, nq, POLY, nterm, kinds)
                got = ns.nl_sens_host(d, nq, POLY, nterm, ns.TABLES, kinds, ends=True)[1]
                ns.check_against(got, ns.TABLES, ref, True)
            init = ns.initial(d, nq, nterm)
            ref0, ref1 = ns.nl_sens_numpy(d, nq, POLY, nterm), ns.nl_sens_numpy(d, nq, POLY, nterm, (R, D), init)
            for want in ns.WANTS:
                if want:
                    ns.check_against(ns.nl_sens_host(d, nq, POLY, nterm, want)[1], want, ref0, False)
                ns.check_against(ns.nl_sens_host(d, nq, POLY, nterm, want, (R, D), ends=True, init=init)[1], want, ref1,
                                 True, init)


@pytest.mark.parametrize("m", [1, 2, 8])
@pytest.mark.parametrize("ne", [1, 2, 7, 33])
def test_chunk_mirror_exp_within_its_bar(ne, m):
    """EXP: gq within the per-entry bar of section 35 summed over the chunk's levels (numpy's exp against libm's), every
    other output bit-equal."""
    for n0 in (1, 4):
        for nq in (1, 2, 5):
            d = ns.kernel_inputs(ne, nq, m, 2, 2, n0)
            d["q"] *= 0.5
            ref = ns.nl_sens_numpy(d, nq, EXP, 2, (D, R))
            got = ns.nl_sens_host(d, nq, EXP, 2, ns.TABLES, (D, R), ends=True)[1]
            ns.check_against(got, ns.TABLES, ref, True, kind=EXP, qbar=ns.exp_bar(d, nq))


@pytest.mark.parametrize("kind,nterm", [(POLY, 4), (EXP, 2)])
def test_cut_of_a_sweep_does_not_change_a_bit(kind, nterm):
    """11 levels as 8 + 3, as 3 + 8 and as eleven chunks of 1: identical bits in every output (the same libm on every
    path, so EXP too)."""
    ne, nq, N, nR = 7, 2, 11, 2
    rng = np.random.default_rng(4)
    base = ns.kernel_inputs(ne, nq, 1, nR, nterm, 1)
    U, Z, B = (rng.standard_normal((N + 1, ne + 1)) for _ in range(3))
    be, phi = rng.standard_normal((N + 1, 2)), rng.standard_normal((N, nR))
    q = 0.5 * rng.standard_normal((nterm, ne, nq))

    def sweep(cuts):
        acc, hi = None, N
        for m in cuts:
            steps = [hi - i for i in range(m)]
            d = dict(base, Utraj=U, Z=Z[steps], Brows=B[steps], band_ends=be[steps], phi=phi, q=q, n0=hi - m + 1, m=m,
                     coef=np.array([proto.coefficients("bdf2", n, N) for n in steps]))
            got = ns.nl_sens_host(d, nq, kind, nterm, kinds=(R, D), ends=True, init=acc)[1]
            if acc is None:
                got["g"][:hi - m + 1] = 0.0
            acc, hi = got, hi - m
        assert hi == 0
        return acc

    ref = sweep((8, 3))
    for cuts in ((3, 8), (1,) * 11):
        got = sweep(cuts)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (cuts, k)


@pytest.mark.parametrize("ne,nq,m", [(1, 1, 1), (7, 2, 8), (33, 5, 2)])
def test_without_gq_it_is_the_linear_chunk_pass(ne, nq, m):
    """gq NULL: every other output equals lssvr_transient_sensitivity_host bit for bit, given the same band_ends rows
    (the linear entry picks each level's row from two matrices, here every level has its copy)."""
    lin = tr.kernel_inputs(ne, m, 2, 2)          # band_ends [2, 2] and band_rows: which of the two is step row i's
    d = ns.kernel_inputs(ne, nq, m, 2, 4, 2)
    d["band_ends"] = lin["band_ends"][np.array(lin["band_rows"])]
    for kinds in KINDS4:
        ref = tr.ts_sens_host(lin, nq, tr.TABLES, kinds, ends=True)[1]
        got = ns.nl_sens_host(d, nq, POLY, 4, tr.TABLES, kinds, ends=True)[1]
        for k in (*tr.TABLES, "g", "kappa"):
            assert np.array_equal(got[k], ref[k]), (kinds, k)
        assert np.all(got["q"] == ns.CANARY)


@pytest.mark.parametrize("kind,nterm", [(POLY, 1), (POLY, 4), (POLY, 6), (EXP, 2)])
@pytest.mark.parametrize("ne", [1, 2, 7, 33])
def test_backward_step_mirror_is_the_chain(ne, kind, nterm):
    """The bands are bit-equal to lssvr_ts_nl_assemble_host at v = u^n, B to lssvr_ts_rhs_host, and the band_ends row is
    {off[0], off[ne-1]} (the same libm on both sides, so EXP too); with and without a_quad, beta1 zero and not."""
    for nq in (1, 2, 5):
        for nR, (b0, b1), with_a in ((1, (2.0, -0.5), True), (3, (1.0, 0.0), False)):
            d = ns.step_inputs(ne, nq, kind, nterm, nR)
            got, ref = ns.step_host(d, b0, b1, with_a), ns.step_chain(d, b0, b1, with_a)
            for k in ref:
                assert np.array_equal(got[k], ref[k]), (nq, nR, k)
            assert got["band_ends"][0] == got["off"][0] and got["band_ends"][1] == got["off"][ne - 1]


@pytest.mark.parametrize("c", ns.cpu_cases(), ids=lambda c: c.id)
def test_adjoint_against_complex_step(c):
    """The prototype's (u, lambda, B, band_ends) through the library's chunk mirror in chunks of 8, against the complex
    step through the whole loop on every datum: within 10x the prototype's own reading, which stays where it was."""
    read, adj, cs = c.reference
    got = ns.host_sweep(c.p, adj["U"], adj["lam"], adj["B"], adj["band_ends"], 8)
    dev = c.deviation(got)
    print(f"{c.id}: host mirror {dev:.2e}, prototype {read:.2e}, bar {c.bar:.2e}, last increment "
          f"{max(i[-1] for i in adj['newton']):.1e}")
    assert dev <= c.bar
    assert read <= ns.READ_SLACK * ns.READ[c.ne]
    if c.p.kind == POLY:
        for k in ("a", "c", "rho", "f", "q", "u0", "g", "kappa"):
            assert np.array_equal(got[k], adj[k]), k          # the numpy restatement, bit for bit


def test_control_without_gu_in_the_jacobian():
    """lambda from K + M(c + alpha rho / dt) alone, g_u left out of J_n: the cubic on 33 elements reads far above its
    bar."""
    c = ns.control_case()
    wrong = proto.adjoint_gradients(c.p, c.J, ns.NEWTON_ITERS, with_gu=False)
    dev = c.deviation(wrong)
    print(f"g_u left out reads {dev:.2e}, the bar is {c.bar:.2e}: factor {dev / c.bar:.2e}")
    assert dev > ns.CONTROL_FACTOR * c.bar


def test_prototype_demo_and_the_step_that_does_not_converge():
    """The inverse problem of the prototype: the misfit falls monotonically, to the recorded value; and the SLOW case
    ends a step at least 100x above its tolerance."""
    hist = proto.demo()
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] - ns.DEMO_FINAL) <= ns.DEMO_RTOL * ns.DEMO_FINAL
    n, ratio = proto.slow_increment()
    print(f"SLOW: step {n} ends {ratio:.2e} x above tolerance")
    assert n is not None and ratio >= ns.SLOW_FACTOR


def _device_form(a, host_index):
    return [v if v is None or isinstance(v, (int, float)) or i in host_index else ctypes.cast(v, ctypes.c_void_p).value
            for i, v in enumerate(a)]


def test_argument_errors_of_the_chunk_pass():
    """Each single wrong argument returns the code of lssvr_transient_sensitivity, or of lssvr_semilinear_sensitivity for
    the law, on the host; the device entry validates before it launches, so host addresses stand in."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    nq, nterm = 2, 4
    d = ns.kernel_inputs(4, nq, 3, 2, nterm, 2)
    o, keep = ns.blank(d, nq, nterm), []
    names = ("x", "ne", "nq", "U", "Z", "n0", "m", "inv_dt", "coef", "phi", "R", "q", "kind", "nterm", "ga", "gc", "grho",
             "gf", "gq", "acc", "B", "be", "k0", "k1", "g", "kap")
    base = ns.nl_sens_args(d, nq, POLY, nterm, o, ns.TABLES, (D, R), True, 0, keep=keep)
    assert len(base) == len(names)
    hp = ns._hp

    def args(**change):
        a = dict(zip(names, base))
        assert set(change) <= set(a)
        a.update(change)
        return list(a.values())

    none5 = dict(ga=None, gc=None, grho=None, gf=None, gq=None)
    broken = ((dict(ne=0), -2, b"ne = 0"), (dict(m=0), -2, b"m = 0"), (dict(m=9), -2, b"m = 9"),
              (dict(n0=0), -2, b"n0 = 0"), (dict(R=-1), -2, b"R = -1"), (dict(R=9), -2, b"R = 9"),
              (dict(R=0), -2, b"R = 0 is allowed only with gf NULL"), (dict(k1=2), -2, b"end kinds"),
              (dict(nq=0), -7, b"nquad = 0"), (dict(nq=6), -7, b"nquad = 6"),
              (dict(x=None), -1, b"x, Utraj, Z"), (dict(U=None), -1, b"x, Utraj, Z"), (dict(Z=None), -1, b"x, Utraj, Z"),
              (dict(coef=None), -1, b"coef_host"), (dict(none5, g=None, kap=None), -1, b"one of ga, gc, grho, gf, gq, out_g"),
              (dict(B=None), -1, b"Brows and band_ends"), (dict(be=None), -1, b"Brows and band_ends"),
              (dict(phi=None), -1, b"phi must be non-NULL with gf"), (dict(kap=None), -1, b"out_g and out_kappa"),
              (dict(gq=hp(keep[2])), -2, b"none of them an input"), (dict(gq=hp(keep[5])), -2, b"none of them an input"),
              (dict(gc=hp(o["q"])), -2, b"must be distinct"),
              (dict(kind=EXP, nterm=2, q=None), -1, b"q_tabs must be non-NULL with LSSVR_NL_EXP"),
              (dict(nterm=0), -2, b"nterm"), (dict(nterm=7), -2, b"nterm"), (dict(kind=EXP, nterm=3), -2, b"nterm"))
    unknown_kind = lib.lssvr_semilinear_sensitivity_host(hp(keep[0]), 4, nq, hp(keep[1]), 1, hp(keep[2]), 1, hp(keep[5]),
                                                         7, 2, hp(o["a"]), None, None, None, None, None, None, 0, 0, None)
    broken += ((dict(kind=7), unknown_kind, b"kind"),)
    assert unknown_kind < 0
    assert lib.lssvr_semilinear_transient_sensitivity_host(*args()) == 0
    for change, code, word in broken:
        rc = lib.lssvr_semilinear_transient_sensitivity_host(*args(**change))
        assert rc == code and word in lib.lssvr_last_error(), (change, rc, lib.lssvr_last_error())
        rc = lib.lssvr_semilinear_transient_sensitivity(*_device_form(args(**change), (8,)), None)
        assert rc == code and word in lib.lssvr_last_error(), ("device", change, rc, lib.lssvr_last_error())
    # what is allowed: the ends alone; POLY without q_tabs; EXP without q_tabs when gq is not asked for
    assert lib.lssvr_semilinear_transient_sensitivity_host(*args(**none5)) == 0
    assert lib.lssvr_semilinear_transient_sensitivity_host(*args(q=None)) == 0
    assert lib.lssvr_semilinear_transient_sensitivity_host(*args(kind=EXP, nterm=2, q=None, gq=None)) == 0


def test_argument_errors_of_the_backward_step():
    """Each single wrong argument returns the code of the neighbour it is taken from: lssvr_ts_nl_assemble for the
    Jacobian's side, lssvr_ts_rhs for the right-hand side's."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    d = ns.step_inputs(5, 2, POLY, 4, 2)
    out, keep = ns.step_blank(5), []
    hp = ns._hp

    def args(**change):
        return ns.step_args(d, 2.0, -0.5, out, keep=keep, **change)

    assert lib.lssvr_semilinear_adjoint_step_host(*args()) == 0
    x = args()[0]
    broken = ((dict(ne=0), -2, b"ne = 0"), (dict(nq=0), -7, b"nquad = 0"), (dict(nq=6), -7, b"nquad = 6"),
              (dict(nterm=0), -2, b"nterm"), (dict(nterm=7), -2, b"nterm"), (dict(kind=EXP), -2, b"nterm"),
              (dict(R=0), -2, b"R = 0"), (dict(R=9), -2, b"R = 9"), (dict(beta0=np.inf), -2, b"must be finite"),
              (dict(inv_dt=np.nan), -2, b"must be finite"),
              *((dict({k: None}), -1, b"must be non-NULL") for k in ("x", "u", "cs", "q", "mdiag", "moff", "U0", "loads",
                                                                      "phi", "diag", "off", "B", "be")),
              (dict(U1=None), -1, b"U1 must be non-NULL when beta1 != 0"),
              (dict(diag=x), -2, b"none of them an input"), (dict(B=hp(out["diag"])), -2, b"must be distinct"),
              (dict(B=args()[11]), -2, b"none of them an input"))
    for change, code, word in broken:
        rc = lib.lssvr_semilinear_adjoint_step_host(*args(**change))
        assert rc == code and word in lib.lssvr_last_error(), (change, rc, lib.lssvr_last_error())
        rc = lib.lssvr_semilinear_adjoint_step(*_device_form(args(**change), ()), None)
        assert rc == code and word in lib.lssvr_last_error(), ("device", change, rc, lib.lssvr_last_error())
    # what is allowed: a = 1 without a_quad; no U1 with beta1 == 0
    assert lib.lssvr_semilinear_adjoint_step_host(*args(a=None)) == 0
    assert lib.lssvr_semilinear_adjoint_step_host(*args(U1=None, beta1=0.0)) == 0


def test_ops_wrappers_check_on_the_host():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.ts_nl_sensitivity(t, t.view(1, 5), t.view(1, 5), 1, [(1.0, 1.0, 0.0)], 1.0, 2, "poly", 4)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.ts_nl_adjoint_step(t, t, torch.zeros((4, 1), dtype=torch.float64), "poly",
                               torch.zeros((1, 4, 1), dtype=torch.float64), t, t[:4], t.view(1, 5), None, t.view(1, 5),
                               torch.ones((1, 1), dtype=torch.float64), 1.0, 0.0, 1.0)
    assert ops.TS_NL_SENS_TABLES == ops.TS_SENS_TABLES + ("q",)


def _one(x):
    return 1.0 + 0.0 * x


_CUBIC = ("poly", [_one, _one, _one, _one])
REFUSALS = [
    ("solver built with the term", dict(nonlinear=("poly", [_one])), dict(nonlinear=_CUBIC),
     "solve_transient_sensitivity has no semilinear form"),
    ("newton_iters alone", {}, dict(newton_iters=3), "newton_iters and newton_tol belong to solve_transient_sensitivity"),
    ("newton_tol alone", {}, dict(newton_tol=1e-8), "newton_iters and newton_tol belong to solve_transient_sensitivity"),
    ("newton_iters 0", {}, dict(nonlinear=_CUBIC, newton_iters=0), "newton_iters must be an integer in 1 .. 8"),
    ("newton_iters 9", {}, dict(nonlinear=_CUBIC, newton_iters=9), "newton_iters must be an integer in 1 .. 8"),
    ("newton_iters bool", {}, dict(nonlinear=_CUBIC, newton_iters=True), "newton_iters must be an integer in 1 .. 8"),
    ("newton_tol 0", {}, dict(nonlinear=_CUBIC, newton_tol=0.0), "newton_tol must be finite and > 0"),
    ("a callable of u", {}, dict(nonlinear=lambda u: u ** 3), "g comes from a tabulated family"),
    ("seven terms", {}, dict(nonlinear=("poly", [_one] * 7)), "takes 1 .. 6 terms"),
    ("exp arity", {}, dict(nonlinear=("exp", _one)), "takes the two callables"),
    ("q not finite", {}, dict(nonlinear=("poly", [lambda x: np.full_like(x, np.nan)])), "nonlinear q_0 is not finite"),
    ("convection", dict(convection=_one, fem_solver="pivot"), dict(nonlinear=_CUBIC), "has no convection term"),
    ("periodic", dict(boundary="periodic", reaction=_one), dict(nonlinear=_CUBIC), "has no boundary='periodic'"),
    ("pivot", dict(fem_solver="pivot"), dict(nonlinear=_CUBIC), "needs fem_solver='bands'"),
    ("neither", {}, dict(nonlinear=_CUBIC, goal=None), "exactly one of goal"),
    ("goal step beyond", {}, dict(nonlinear=_CUBIC, goal_steps=[2, 5]), "goal_steps must be step indices"),
    ("too large", {}, dict(nonlinear=_CUBIC, max_state_bytes=5 * 9 * 8 - 1), "checkpointing"),
    ("scheme", {}, dict(nonlinear=_CUBIC, scheme="bdf3"), "scheme must be 'bdf1' or 'bdf2'"),
]


def test_facade_refusals(monkeypatch):
    """Every refusal is a ValueError with its reason, raised before the library is loaded or a device looked up."""
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import _capi, solver

    def forbidden(*a, **k):
        raise AssertionError("a device call was reached before the refusal")
    monkeypatch.setattr(_capi, "load", forbidden)
    monkeypatch.setattr(solver, "_device", forbidden)
    for name, ctor, kw, match in REFUSALS:
        kw = {"goal": _one, "nsteps": 4, **kw}
        s = pkg.FEMLSSVRPrimalSolver(9, **ctor)
        with pytest.raises(ValueError, match=re.escape(match)):
            s.solve_transient_sensitivity(_one, 0.1, **kw)
            raise AssertionError(f"{name}: not refused")
    # what is not refused reaches the device
    with pytest.raises(AssertionError, match="device call"):
        pkg.FEMLSSVRPrimalSolver(9).solve_transient_sensitivity(_one, 0.1, nsteps=4, goal=_one, nonlinear=_CUBIC,
                                                                newton_iters=8, newton_tol=1e-12)
