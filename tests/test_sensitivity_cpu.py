"""CPU: adjoint sensitivities of the P1 solve where there is no GPU -- the library's host mirror
against the numpy restatement bit for bit, the adjoint identity against the complex step, the argument errors of the
two entries, the facade's refusals and the band transposition."""
import numpy as np
import pytest

import sensitivity_rules as sr

proto = sr.proto
D, R = sr.D, sr.R


@pytest.mark.parametrize("nc,nu", [(1, 1), (3, 1), (3, 3), (8, 1), (8, 8)])
@pytest.mark.parametrize("ne", [1, 2, 5, 33])
def test_host_mirror_is_the_numpy_restatement(ne, nc, nu):
    """Every output is bit-equal: each formula is a chain of single IEEE operations in a written order, which numpy
    reproduces; the NULL-output combinations leave the tables that were not asked for untouched."""
    d = sr.kernel_inputs(ne, nc, nu)
    for nq in (1, 2, 3, 4, 5):
        for kinds in ((D, D), (R, D), (D, R), (R, R)):
            ref = sr.sens_numpy(d["x"], nq, d["U"], d["Z"], d["P"], d["band_ends"], kinds)
            got = sr.sens_host(d["x"], nq, d["U"], d["Z"], sr.TABLES, d["P"], d["band_ends"], kinds, ends=True)[1]
            sr.check_against(got, sr.TABLES, ref, True)
        ref0 = sr.sens_numpy(d["x"], nq, d["U"], d["Z"], None, d["band_ends"], (D, D))
        for want in sr.WANTS:
            got = sr.sens_host(d["x"], nq, d["U"], d["Z"], want)[1]
            sr.check_against(got, want, ref0, False)
        got = sr.sens_host(d["x"], nq, d["U"], d["Z"], ("f",), None, d["band_ends"], (D, D), ends=True)[1]      # P NULL
        sr.check_against(got, ("f",), ref0, True)


@pytest.mark.parametrize("c", sr.cpu_cases(), ids=lambda c: c.id)
def test_adjoint_against_complex_step(c):
    """Assembly, solve, adjoint solve (numpy, dense) and the formulas through the library's host mirror, against the
    complex-step derivative of every table entry and end datum: within 10x the prototype's own reading."""
    read, adj, cs = c.reference
    got = sr.sens_host(c.x, c.nq, adj["u"][None, :], adj["z"][None, :], sr.TABLES, adj["p"][None, :],
                       np.array([proto.assemble(c.x, c.tabs["f"], c.tabs.get("a"), c.tabs.get("b"),
                                                c.tabs.get("c"))[k][i] for k, i in ((1, 0), (2, -1))]),
                       c.kinds, ends=True)[1]
    grads = {k: got[k][0] for k in (*sr.TABLES, "ends")}
    dev = proto.deviation(grads, cs)
    print(f"{c.id}: host mirror {dev:.2e}, prototype {read:.2e}, bar {c.bar:.2e}")
    assert dev <= c.bar
    assert read <= sr.READ_SLACK * sr.READ[c.ne]          # the prototype itself stays where it was measured
    assert np.all(adj["z"][[0, -1]][np.array(c.kinds) == D] == 0.0)
    if c.conv:          # the test has teeth: the untransposed adjoint is far off
        assert proto.deviation(c.wrong_adjoint(), cs) > 1e6 * c.bar


def test_argument_errors():
    """Each broken argument of the two entries is refused with its code, on the host (the device entry validates
    before it launches, so it can be called here with host addresses standing in)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    d = sr.kernel_inputs(4, 3, 3)
    g, e = np.zeros((3, 4, 2)), np.zeros((3, 4))

    def host(**change):
        a = dict(x=sr._hp(d["x"]), ne=4, nq=2, U=sr._hp(d["U"]), nu=3, Z=sr._hp(d["Z"]), nc=3, ga=sr._hp(g), gb=None,
                 gc=None, gf=None, P=sr._hp(d["P"]), band_ends=sr._hp(d["band_ends"]), k0=D, k1=R, ends=sr._hp(e))
        assert set(change) <= set(a)
        a.update(change)
        return lib.lssvr_p1_sensitivity_host(*a.values())

    assert host() == 0
    for change, code, word in ((dict(x=None), -1, b"x, U, Z"), (dict(U=None), -1, b"x, U, Z"),
                               (dict(Z=None), -1, b"x, U, Z"), (dict(ga=None), -1, b"ga, gb, gc, gf"),
                               (dict(ne=0), -2, b"ne = 0"), (dict(ne=-3), -2, b"ne"), (dict(nc=0), -2, b"nc = 0"),
                               (dict(nc=9), -2, b"nc = 9"), (dict(nu=2), -2, b"nu = 2"), (dict(nu=0), -2, b"nu = 0"),
                               (dict(nq=0), -7, b"nquad = 0"), (dict(nq=6), -7, b"nquad = 6"),
                               (dict(band_ends=None), -1, b"band_ends"), (dict(k1=2), -2, b"end kinds"),
                               (dict(k0=-1), -2, b"end kinds")):
        rc = host(**change)
        assert rc == code and word in lib.lssvr_last_error(), (change, rc, lib.lssvr_last_error())
    # P may be NULL; without out_ends neither band_ends nor the kinds are read; one output of any kind is enough
    assert host(P=None) == 0
    assert host(band_ends=None, k0=7, k1=7, ends=None) == 0
    assert host(ga=None, gc=sr._hp(g)) == 0
    # the device entry: the same checks, before any launch
    a = [t.ctypes.data for t in (d["x"], d["U"], d["Z"], g, d["band_ends"], e)]
    dev = lambda ne, nq, nu, nc, ga, be, k0, ends: lib.lssvr_p1_sensitivity(      # noqa: E731
        a[0], ne, nq, a[1], nu, a[2], nc, ga, None, None, None, None, be, k0, 0, ends, None)
    assert dev(0, 2, 3, 3, a[3], None, 0, None) == -2
    assert dev(4, 6, 3, 3, a[3], None, 0, None) == -7
    assert dev(4, 2, 2, 3, a[3], None, 0, None) == -2
    assert dev(4, 2, 3, 9, a[3], None, 0, None) == -2
    assert dev(4, 2, 3, 3, None, None, 0, None) == -1
    assert dev(4, 2, 3, 3, a[3], None, 0, a[5]) == -1 and b"band_ends" in lib.lssvr_last_error()
    assert dev(4, 2, 3, 3, a[3], a[4], 5, a[5]) == -2
    assert lib.lssvr_p1_sensitivity(None, 4, 2, a[1], 3, a[2], 3, a[3], None, None, None, None, None, 0, 0, None,
                                    None) == -1


def test_ops_wrapper_checks_on_the_host():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.p1_sensitivity(t, t, t)


REFUSALS = [
    ("periodic", dict(boundary="periodic", reaction=lambda x: 1.0 + 0.0 * x), {}, "solve_sensitivity has no "
     "boundary='periodic'"),
    ("flux", dict(fem_solver="flux"), {}, "solve_sensitivity needs fem_solver='bands' or 'pivot'"),
    ("nonlinear", dict(nonlinear=("poly", [lambda x: 1.0 + 0.0 * x])), {}, "solve_sensitivity has no semilinear form"),
    ("solver", dict(solver=1), {}, "solve_sensitivity needs solver=ops.SOLVER_PRIMAL"),
    ("element_degrees", dict(_degrees=True), {}, "solve_sensitivity has no element_degrees"),
    ("neither", {}, dict(goal=None), "exactly one of goal"),
    ("both", {}, dict(observe=([0.0], [1.0])), "exactly one of goal"),
    ("goal not callable", {}, dict(goal=3.0), "goal must be a callable j(x)"),
    ("non-finite rhs", dict(rhs=lambda x: np.full_like(x, np.nan)), {}, "rhs is not finite at a quadrature point"),
    ("non-finite coef", dict(coef=(lambda x: np.full_like(x, np.inf), lambda x: 0.0 * x)), {},
     "coef a is not finite at a quadrature point"),
    ("non-finite convection", dict(convection=lambda x: np.where(x > 0.9, np.nan, 0.0)), {},
     "convection is not finite at a quadrature point"),
    ("non-finite reaction", dict(reaction=lambda x: np.full_like(x, np.inf)), {},
     "reaction is not finite at a quadrature point"),
    ("non-finite goal", {}, dict(goal=lambda x: np.full_like(x, np.nan)), "goal is not finite at a quadrature point"),
    ("rhs of the wrong shape", dict(rhs=lambda x: np.ones(3)), {}, "rhs must return one value per point ([8, 2]"),
    ("non-finite data", {}, dict(goal=None, observe=([0.0], [np.nan])), "observe d_obs is not finite"),
    ("observation outside", {}, dict(goal=None, observe=([1.5], [0.0])), "every x_obs must lie in the mesh"),
    ("observe sizes", {}, dict(goal=None, observe=([0.0, 0.1], [0.0])), "as many points as data"),
    ("non-finite end data", dict(boundary=(("dirichlet", 0.0), ("neumann", 1.0)), _g=np.inf), {},
     "the end data is not finite"),
]


def test_facade_refusals(monkeypatch):
    """Every refusal is a ValueError with its reason, raised before the library is loaded or a device looked up."""
    import re
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import _capi, solver

    def forbidden(*a, **k):
        raise AssertionError("a device call was reached before the refusal")
    monkeypatch.setattr(_capi, "load", forbidden)
    monkeypatch.setattr(solver, "_device", forbidden)
    one = lambda x: 1.0 + 0.0 * x      # noqa: E731
    for name, ctor, kw, match in REFUSALS:
        ctor, kw = dict(ctor), {"goal": one, **kw}
        degrees, g = ctor.pop("_degrees", False), ctor.pop("_g", None)
        s = pkg.FEMLSSVRPrimalSolver(9, **ctor)
        if degrees:
            s.element_degrees = np.full(8, 9)
        if g is not None:
            s.boundary = (("dirichlet", 0.0), ("neumann", 1.0))
            monkeypatch.setattr(s, "_gd_bc", lambda: ((-1.0, 1.0), (0.0, g)))
        with pytest.raises(ValueError, match=re.escape(match)):
            s.solve_sensitivity(**kw)
            raise AssertionError(f"{name}: not refused")
    for ctor, kw in (({}, dict(goal=one)), (dict(convection=one, fem_solver="pivot"), dict(observe=([0.0], [1.0])))):
        with pytest.raises(AssertionError, match="device call"):
            pkg.FEMLSSVRPrimalSolver(9, **ctor).solve_sensitivity(**kw)


def test_adjoint_bands():
    """sub and sup exchanged, off left alone, nothing copied, the argument untouched."""
    from hybrid_fem_lssvr_amd import ops
    diag, sub, sup, load, off = (np.arange(n, dtype=np.float64) for n in (5, 4, 4, 5, 4))
    ns = dict(diag=diag, sub=sub, sup=sup, load=load)
    t = ops.adjoint_bands(ns)
    assert t is not ns and t["sub"] is sup and t["sup"] is sub and t["diag"] is diag and t["load"] is load
    assert ns["sub"] is sub and ns["sup"] is sup and set(t) == set(ns)
    sym = dict(diag=diag, off=off, load=load, kloc=off)
    t = ops.adjoint_bands(sym)
    assert t is not sym and set(t) == set(sym) and all(t[k] is sym[k] for k in sym)
    assert ops.adjoint_bands(ops.adjoint_bands(ns))["sub"] is sub
    with pytest.raises(ValueError, match="both sub and sup"):
        ops.adjoint_bands(dict(diag=diag, sub=sub))


def test_demo_record_of_the_prototype():
    """The inverse problem of the prototype: the misfit falls monotonically, to the recorded value."""
    hist = proto.demo()
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] - sr.DEMO_FINAL) <= 1e-6 * sr.DEMO_FINAL
