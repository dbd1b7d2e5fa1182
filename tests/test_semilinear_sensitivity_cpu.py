"""CPU: adjoint sensitivities of the semilinear P1 solve where there is no GPU -- the prototype
against the complex step, the control with g_u forgotten, the library's host mirror against the numpy restatement, the
argument errors of the two entries, the facade's refusals and the record of the inverse problem."""
import re

import numpy as np
import pytest

import semilinear_sensitivity_rules as nr

proto = nr.proto
D, R, POLY, EXP = nr.D, nr.R, nr.POLY, nr.EXP


@pytest.mark.parametrize("c", nr.cpu_cases(), ids=lambda c: c.id)
def test_prototype_against_complex_step(c):
    """Newton, ONE linearisation at u*, the adjoint solve (numpy, dense) and the formulas through the library's host
    mirror, against the complex-step derivative of every table entry -- the q_k among them -- and end datum."""
    read, adj, cs = c.reference
    bands = proto.newton_step(c.x, c.tabs, c.kind, adj["u"], c.kinds, c.kappa, c.g)[1]
    got = nr.nl_host(c.x, c.nq, adj["u"][None, :], adj["z"][None, :], c.kind, c.nterm, c.tabs["q"], nr.TABLES,
                     adj["p"][None, :], np.array([bands[1][0], bands[2][-1]]), c.kinds, ends=True)[1]
    dev = proto.deviation({k: got[k][0] for k in (*nr.TABLES, "ends")}, cs)
    print(f"{c.id}: host mirror {dev:.2e}, prototype {read:.2e}, bar {c.bar:.2e}, Newton {adj['newton']['iterations']}")
    assert read <= nr.READ_SLACK * nr.READ[c.ne]          # the prototype itself stays where it was measured
    assert dev <= c.bar
    assert np.all(adj["z"][[0, -1]][np.array(c.kinds) == D] == 0.0)
    assert set(proto.groups(cs)) == {"a", "b", "c", "f", "ends", *(f"q{k}" for k in range(c.nterm))}


def test_control_forgotten_gu():
    """z from K^T alone -- g_u forgotten in the Jacobian -- is far off: the tests above have teeth."""
    c = nr.control_case()
    wrong = proto.deviation(c.forgotten_gu(), c.reference[2])
    print(f"{c.id}: g_u forgotten reads {wrong:.2e}, bar {c.bar:.2e}")
    assert wrong > nr.CONTROL_FACTOR * c.bar


@pytest.mark.parametrize("nc,nu", [(1, 1), (3, 1), (3, 3), (8, 1), (8, 8)])
@pytest.mark.parametrize("ne", [1, 2, 7, 33])
def test_host_mirror_is_the_numpy_restatement(ne, nc, nu):
    """POLY nterm 1 .. 6: every output bit-equal to the numpy restatement; a, b, c, f and the ends bit-equal to
    lssvr_p1_sensitivity_host; gq_0 == -gf and gq_1 == gc; every want subset leaves its canaries.  EXP: gq within the
    per-entry bars of the two exp implementations, everything else bit-equal."""
    sr = nr.sr
    for nq in (1, 2, 5):
        kinds = ((D, D), (R, D), (D, R), (R, R))[nq % 4]
        for kind, nterm in [(POLY, k) for k in range(1, 7)] + [(EXP, 2)]:
            d = nr.kernel_inputs(ne, nq, nc, nu, nterm)
            ref = nr.nl_numpy(d["x"], nq, d["U"], d["Z"], kind, nterm, d["q"], d["P"], d["band_ends"], kinds)
            qbar = nr.exp_bars(d["x"], nq, d["U"], d["Z"], d["q"]) if kind == EXP else None
            got = nr.nl_host(d["x"], nq, d["U"], d["Z"], kind, nterm, d["q"], nr.TABLES, d["P"], d["band_ends"], kinds,
                             ends=True)[1]
            nr.check_against(got, nr.TABLES, ref, True, kind, qbar)
            p1 = sr.sens_host(d["x"], nq, d["U"], d["Z"], sr.TABLES, d["P"], d["band_ends"], kinds, ends=True)[1]
            assert all(np.array_equal(got[k], p1[k]) for k in (*sr.TABLES, "ends"))
            if kind == POLY:          # q_tabs is not read
                again = nr.nl_host(d["x"], nq, d["U"], d["Z"], kind, nterm, None, ("q",))[1]
                assert np.array_equal(again["q"], got["q"])
            if nterm in (2, 4):
                for want in nr.WANTS:
                    got = nr.nl_host(d["x"], nq, d["U"], d["Z"], kind, nterm, d["q"], want)[1]
                    nr.check_against(got, want, ref, False, kind, qbar)
                got = nr.nl_host(d["x"], nq, d["U"], d["Z"], kind, nterm, d["q"], (), d["P"], d["band_ends"], kinds,
                                 ends=True)[1]                  # the end gradients alone
                nr.check_against(got, (), ref, True, kind, qbar)


def test_argument_errors():
    """Each broken argument of the two entries is refused with its code, on the host (the device entry validates
    before it launches, so it can be called here with host addresses standing in)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    d = nr.kernel_inputs(4, 2, 3, 3, 4)
    g, gq, e = np.zeros((3, 4, 2)), np.zeros((3, 6, 4, 2)), np.zeros((3, 4))

    def args(pointer, **change):
        a = dict(x=d["x"], ne=4, nq=2, U=d["U"], nu=3, Z=d["Z"], nc=3, q=d["q"], kind=POLY, nterm=4, ga=g, gb=None,
                 gc=None, gf=None, gq=gq, P=d["P"], band_ends=d["band_ends"], k0=D, k1=R, ends=e)
        assert set(change) <= set(a)
        a.update(change)
        return [pointer(v) if isinstance(v, np.ndarray) else v for v in a.values()]

    def host(**change):
        return lib.lssvr_semilinear_sensitivity_host(*args(nr._hp, **change))

    def device(**change):
        return lib.lssvr_semilinear_sensitivity(*args(lambda t: t.ctypes.data, **change), None)

    assert host() == 0
    none = dict(ga=None, gq=None, ends=None)
    for change, code, word in ((dict(x=None), -1, b"x, U, Z"), (dict(U=None), -1, b"x, U, Z"),
                               (dict(Z=None), -1, b"x, U, Z"), (dict(ne=0), -2, b"ne = 0"),
                               (dict(nc=0), -2, b"nc = 0"), (dict(nc=9), -2, b"nc = 9"), (dict(nu=2), -2, b"nu = 2"),
                               (dict(nq=0), -7, b"nquad = 0"), (dict(nq=6), -7, b"nquad = 6"),
                               (dict(nterm=0), -2, b"nterm = 0"), (dict(nterm=7), -2, b"nterm = 7"),
                               (dict(kind=EXP, nterm=3), -2, b"nterm = 3"), (dict(kind=EXP, nterm=2, q=None), -1,
                                                                            b"q_tabs"),
                               (dict(kind=2), -4, b"unknown kind"),
                               (none, -1, b"ga, gb, gc, gf, gq, out_ends"),
                               (dict(band_ends=None), -1, b"band_ends"), (dict(k1=2), -2, b"end kinds")):
        for fn in (host, device):
            rc = fn(**change)
            assert rc == code and word in lib.lssvr_last_error(), (fn.__name__, change, rc, lib.lssvr_last_error())
    # q_tabs may be NULL for POLY, P may be NULL; one output of any kind is enough; without out_ends neither band_ends
    # nor the kinds are read
    assert host(q=None) == 0 and host(P=None) == 0 and host(kind=EXP, nterm=2) == 0
    assert host(ga=None) == 0 and host(gq=None) == 0 and host(ga=None, gq=None) == 0
    assert host(band_ends=None, k0=7, k1=7, ends=None) == 0


def test_ops_wrapper_checks_on_the_host():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.nl_sensitivity(t, t, t, 2, "poly", 4)
    assert ops.NL_SENS_TABLES == nr.TABLES


def _one(x):
    return 1.0 + 0.0 * x


CUBIC = ("poly", [proto.zero, proto.zero, proto.zero, _one])
NAME = "solve_semilinear_sensitivity"
REFUSALS = [
    ("no nonlinear", dict(nonlinear=None), {}, f"{NAME} needs nonlinear="),
    # (the constructor refuses these with nonlinear=; the attributes are public, so the method checks them again)
    ("periodic", dict(_set=dict(boundary="periodic")), {}, f"{NAME} has no boundary='periodic'"),
    ("flux", dict(_set=dict(fem_solver="flux")), {}, f"{NAME} needs fem_solver='bands' or 'pivot'"),
    ("solver", dict(_set=dict(solver_id=1)), {}, f"{NAME} needs solver=ops.SOLVER_PRIMAL"),
    ("element_degrees", dict(_set=dict(element_degrees=np.full(8, 9))), {}, f"{NAME} has no element_degrees"),
    ("element_lists", dict(_set=dict(element_lists=True)), {}, "nonlinear has no element_lists / element_degrees"),
    ("family", dict(_set=dict(nonlinear=("cubic", _one))), {},
     "nonlinear must be ('poly', [q0, q1, ...]) or ('exp', q0, q1)"),
    ("seven terms", dict(_set=dict(nonlinear=("poly", [_one] * 7))), {}, "nonlinear 'poly' takes 1 .. 6 terms"),
    ("neither", {}, dict(goal=None), f"{NAME} needs exactly one of goal"),
    ("both", {}, dict(observe=([0.0], [1.0])), f"{NAME} needs exactly one of goal"),
    ("goal not callable", {}, dict(goal=3.0), "goal must be a callable j(x)"),
    ("non-finite rhs", dict(rhs=lambda x: np.full_like(x, np.nan)), {}, "rhs is not finite at a quadrature point"),
    ("non-finite goal", {}, dict(goal=lambda x: np.full_like(x, np.nan)), "goal is not finite at a quadrature point"),
    ("non-finite q", dict(nonlinear=("poly", [lambda x: np.full_like(x, np.inf)])), {},
     "nonlinear q_0 is not finite at a quadrature point"),
    ("observation outside", {}, dict(goal=None, observe=([1.5], [0.0])), "every x_obs must lie in the mesh"),
    ("tol", {}, dict(tol=0.0), "tol must be finite and > 0"),
    ("max_iter", {}, dict(max_iter=0), "max_iter must be an integer >= 1"),
    ("max_iter kind", {}, dict(max_iter=2.5), "max_iter must be an integer >= 1"),
    ("u_init", {}, dict(u_init=3.0), "u_init must be a callable u_init(x) or None"),
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
        ctor, kw = {"nonlinear": CUBIC, **ctor}, {"goal": _one, **kw}
        attrs = ctor.pop("_set", {})
        s = pkg.FEMLSSVRPrimalSolver(9, **ctor)
        for k, v in attrs.items():
            setattr(s, k, v)
        with pytest.raises(ValueError, match=re.escape(match)):
            s.solve_semilinear_sensitivity(**kw)
            raise AssertionError(f"{name}: not refused")
    for ctor, kw in ((dict(nonlinear=CUBIC), dict(goal=_one)),
                     (dict(nonlinear=("exp", _one, _one), fem_solver="pivot"), dict(observe=([0.0], [1.0]), tol=1e-10))):
        with pytest.raises(AssertionError, match="device call"):
            pkg.FEMLSSVRPrimalSolver(9, **ctor).solve_semilinear_sensitivity(**kw)
    # solve_sensitivity keeps its refusal and its wording
    with pytest.raises(ValueError, match="solve_sensitivity has no semilinear form"):
        pkg.FEMLSSVRPrimalSolver(9, nonlinear=CUBIC).solve_sensitivity(_one)


def test_demo_record_of_the_prototype():
    """The inverse problem of the prototype: the misfit falls monotonically, to the recorded value."""
    hist = proto.demo()
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] - nr.DEMO_FINAL) <= nr.DEMO_RTOL * nr.DEMO_FINAL
