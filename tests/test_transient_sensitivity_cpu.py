"""CPU: adjoint sensitivities of the BDF loop where there is no GPU -- the library's host mirror
against the numpy restatement bit for bit, the backward loop and the sums against the complex step, chunk independence,
the negative control, the argument errors of the two entries and the facade's refusals."""
import ctypes
import re

import numpy as np
import pytest

import transient_sensitivity_rules as tr

proto = tr.proto
D, R = tr.D, tr.R


@pytest.mark.parametrize("nR", [0, 1, 8])
@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("ne", [1, 2, 5, 33])
def test_host_mirror_is_the_numpy_restatement(ne, m, nR):
    """Every output is bit-equal, with no ulp allowance: each sum is a chain of single IEEE operations in a written
    order, which numpy reproduces; every NULL-output combination leaves what was not asked for untouched; an
    accumulating call continues from what the outputs hold."""
    for n0 in (1, 2, 4):          # a chunk that ends at step 1 (no row n-2), at step 2 (row 0), and further in
        d = tr.kernel_inputs(ne, m, nR, n0)
        for nq in (1, 2, 3, 4, 5):
            for kinds in ((D, D), (R, D), (D, R), (R, R)):
                ref = tr.ts_sens_numpy(d, nq, kinds)
                got = tr.ts_sens_host(d, nq, tr.TABLES if nR else tr.TABLES[:3], kinds, ends=True)[1]
                tr.check_against(got, tr.TABLES if nR else tr.TABLES[:3], ref, True)
            init = tr.initial(d, nq)
            ref1 = tr.ts_sens_numpy(d, nq, (R, D), init)
            for want in tr.wants(nR):
                if want:
                    tr.check_against(tr.ts_sens_host(d, nq, want)[1], want, tr.ts_sens_numpy(d, nq), False)
                    tr.check_against(tr.ts_sens_host(d, nq, want, init=init)[1], want, ref1, False, init)
                tr.check_against(tr.ts_sens_host(d, nq, want, (R, D), ends=True, init=init)[1], want, ref1, True, init)


@pytest.mark.parametrize("c", tr.cpu_cases(), ids=lambda c: c.id)
def test_adjoint_against_complex_step(c):
    """The prototype's (u, lambda, B) through the library's host mirror in chunks of 8, against the complex-step
    derivative of every table entry, initial value and end datum: within 10x the prototype's own reading."""
    dev_by_group, adj, cs = c.reference
    got = tr.host_sweep(c.p, adj["U"], adj["lam"], adj["B"], 8)
    dev = c.deviation(got)
    print(f"{c.id}: host mirror {dev:.2e}, prototype {c.read:.2e}, bar {c.bar:.2e}; "
          + " ".join(f"{k} {v:.1e}" for k, v in dev_by_group.items()))
    assert dev <= c.bar
    assert c.read <= tr.READ_SLACK * tr.READ[c.ne]          # the prototype itself stays where it was measured
    for s, end in ((0, 0), (1, -1)):
        if c.kinds[s] == D:
            assert np.all(adj["lam"][:, end] == 0.0) and got["u0"][end] == 0.0 and got["kappa"][s] == 0.0
        else:
            assert got["g"][0, s] == 0.0


@pytest.mark.parametrize("c", [tr.case(33, 2, (D, R), "bdf2", 17, "random"), tr.case(7, 5, (R, R), "bdf1", 9, "observe")],
                         ids=lambda c: c.id)
def test_chunking_does_not_change_a_bit(c):
    """A sweep in chunks of 8, 3 and 1 gives the same tables and end gradients bit for bit: every sum continues from
    the stored value, so the order of the additions does not depend on the cut."""
    _, adj, _ = c.reference
    ref = tr.host_sweep(c.p, adj["U"], adj["lam"], adj["B"], 8)
    for size in (3, 1):
        got = tr.host_sweep(c.p, adj["U"], adj["lam"], adj["B"], size)
        for k in proto.GROUPS:
            assert np.array_equal(got[k], ref[k]), (size, k)
    num = proto.sweep_gradients(c.p, adj["U"], adj["lam"], adj["B"], 8)
    for k in proto.GROUPS:
        assert np.array_equal(num[k], ref[k]), k


NEGATIVE_CONTROL_FACTOR = 1e12          # the prototype reads 6.8e-01 against a bar of 2.0e-14: 3.4e13


def test_negative_control_wrong_adjoint_coefficients():
    """(beta0_n, beta1_n) in the place of (beta0_{n+1}, beta1_{n+2}) in the adjoint right-hand side: on the N = 3 BDF2
    case, where the BDF1 start and the end of the sweep both matter, the gradients are far off."""
    c = tr.case(7, 2, (D, R), "bdf2", 3, "random")
    wrong = proto.adjoint_gradients(c.p, c.J, wrong_betas=True)
    got = tr.host_sweep(c.p, wrong["U"], wrong["lam"], wrong["B"], 8)
    dev = c.deviation(got)
    print(f"wrong coefficients read {dev:.2e}, the bar is {c.bar:.2e}: factor {dev / c.bar:.2e}")
    assert dev > NEGATIVE_CONTROL_FACTOR * c.bar


def test_argument_errors():
    """Each broken argument of the two entries is refused with its code, on the host (the device entry validates
    before it launches, so it can be called here with host addresses standing in)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    d = tr.kernel_inputs(4, 3, 2, 2)
    nq = 2
    o = tr.blank(d, nq)
    keep = [tr._c(d[k]) for k in ("x", "Utraj", "Z", "Brows", "phi", "band_ends", "coef")]
    hp = tr._hp

    def args(**change):
        a = dict(x=hp(keep[0]), ne=4, nq=nq, U=hp(keep[1]), Z=hp(keep[2]), n0=2, m=3, inv_dt=3.0, coef=hp(keep[6]),
                 phi=hp(keep[4]), R=2, ga=hp(o["a"]), gc=hp(o["c"]), grho=hp(o["rho"]), gf=hp(o["f"]), acc=0,
                 B=hp(keep[3]), be=hp(keep[5]), mask=0b011, k0=D, k1=R, g=hp(o["g"]), kap=hp(o["kappa"]))
        assert set(change) <= set(a)
        a.update(change)
        return list(a.values())

    def host(**change):
        return lib.lssvr_transient_sensitivity_host(*args(**change))

    assert host() == 0
    none4 = dict(ga=None, gc=None, grho=None, gf=None)
    broken = ((dict(ne=0), -2, b"ne = 0"), (dict(ne=-3), -2, b"ne"), (dict(m=0), -2, b"m = 0"), (dict(m=9), -2, b"m = 9"),
              (dict(n0=0), -2, b"n0 = 0"), (dict(n0=-1), -2, b"n0"), (dict(R=-1), -2, b"R = -1"), (dict(R=9), -2, b"R = 9"),
              (dict(R=0), -2, b"R = 0 is allowed only with gf NULL"), (dict(k1=2), -2, b"end kinds"),
              (dict(k0=-1), -2, b"end kinds"), (dict(mask=0b1000), -2, b"band_mask"), (dict(mask=-1), -2, b"band_mask"),
              (dict(nq=0), -7, b"nquad = 0"), (dict(nq=6), -7, b"nquad = 6"),
              (dict(x=None), -1, b"x, Utraj, Z"), (dict(U=None), -1, b"x, Utraj, Z"), (dict(Z=None), -1, b"x, Utraj, Z"),
              (dict(coef=None), -1, b"coef_host"), (dict(none4, g=None, kap=None), -1, b"one of ga, gc, grho, gf, out_g"),
              (dict(B=None), -1, b"Brows and band_ends"), (dict(be=None), -1, b"Brows and band_ends"),
              (dict(phi=None), -1, b"phi must be non-NULL with gf"), (dict(kap=None), -1, b"out_g and out_kappa"),
              (dict(g=None), -1, b"out_g and out_kappa"), (dict(ga=hp(keep[2])), -2, b"none of them an input"),
              (dict(gc=hp(o["a"])), -2, b"must be distinct"), (dict(g=hp(keep[3])), -2, b"none of them an input"))
    for change, code, word in broken:
        rc = host(**change)
        assert rc == code and word in lib.lssvr_last_error(), (change, rc, lib.lssvr_last_error())
    # what is allowed: the ends alone; R = 0 and no phi without gf; without out_g neither Brows, band_ends, the mask nor
    # the kinds are read
    assert host(**none4) == 0
    assert host(gf=None, R=0, phi=None) == 0
    assert host(g=None, kap=None, B=None, be=None, mask=99, k0=7, k1=7) == 0
    # the device entry: the same checks, before any launch (the pointers are host addresses: nothing may be launched)
    for change, code, word in broken:
        a = args(**change)
        a = [v if v is None or isinstance(v, (int, float)) or i == 8 else ctypes.cast(v, ctypes.c_void_p).value
             for i, v in enumerate(a)]          # (index 8: coef_host, a host array in the device entry too)
        rc = lib.lssvr_transient_sensitivity(*a, None)
        assert rc == code and word in lib.lssvr_last_error(), ("device", change, rc, lib.lssvr_last_error())


def test_ops_wrapper_checks_on_the_host():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.ts_sensitivity(t, t.view(1, 5), t.view(1, 5), 1, [(1.0, 1.0, 0.0)], 1.0)


def _one(x):
    return 1.0 + 0.0 * x


_OBS = dict(goal=None, observe=([2], [0.0], [[1.0]]))
REFUSALS = [
    ("convection", dict(convection=_one, fem_solver="pivot"), {}, "has no convection term"),
    ("periodic", dict(boundary="periodic", reaction=_one), {}, "has no boundary='periodic'"),
    ("flux", dict(fem_solver="flux"), {}, "needs fem_solver='bands'"),
    ("pivot", dict(fem_solver="pivot"), {}, "needs fem_solver='bands'"),
    ("nonlinear", dict(nonlinear=("poly", [_one])), {}, "solve_transient_sensitivity has no semilinear form"),
    ("element_degrees", dict(_degrees=True), {}, "has no element_degrees"),
    ("solver", dict(solver=1), {}, "needs solver=ops.SOLVER_PRIMAL"),
    ("neither", {}, dict(goal=None), "exactly one of goal"),
    ("both", {}, dict(observe=_OBS["observe"]), "exactly one of goal"),
    ("goal not callable", {}, dict(goal=3.0), "goal must be a callable j(x)"),
    ("goal step 0", {}, dict(goal_steps=[0]), "goal_steps must be step indices in 1 .. nsteps = 4"),
    ("goal step beyond", {}, dict(goal_steps=[2, 5]), "goal_steps must be step indices"),
    ("goal step twice", {}, dict(goal_steps=[2, 2]), "goal_steps must not name a step twice"),
    ("goal steps empty", {}, dict(goal_steps=[]), "goal_steps must be step indices"),
    ("goal weights count", {}, dict(goal_steps=[1, 2], goal_weights=[1.0]), "one weight per goal step"),
    ("goal weights finite", {}, dict(goal_weights=[np.inf]), "goal_weights is not finite"),
    ("non-finite goal", {}, dict(goal=lambda x: np.full_like(x, np.nan)), "goal is not finite at a quadrature point"),
    ("goal shape", {}, dict(goal=lambda x: np.ones(3)), "goal must return one value per point ([8, 2]"),
    ("goal_steps with observe", {}, dict(_OBS, goal_steps=[1]), "goal_steps and goal_weights belong to goal="),
    ("observe not a triple", {}, dict(goal=None, observe=([0.0], [1.0])), "observe must be a triple"),
    ("observe step", {}, dict(goal=None, observe=([5], [0.0], [[1.0]])), "observe steps must be step indices"),
    ("observe step twice", {}, dict(goal=None, observe=([1, 1], [0.0], [[1.0], [1.0]])), "must not name a step twice"),
    ("observe shape", {}, dict(goal=None, observe=([1, 2], [0.0], [[1.0]])), "d_obs must be [len(steps), nobs] = [2, 1]"),
    ("observe non-finite", {}, dict(goal=None, observe=([2], [0.0], [[np.nan]])), "observe d_obs is not finite"),
    ("observe outside", {}, dict(goal=None, observe=([2], [1.5], [[0.0]])), "every x_obs must lie in the mesh"),
    ("too large", {}, dict(max_state_bytes=5 * 9 * 8 - 1), "checkpointing"),
    ("non-finite weight", {}, dict(weight=lambda x: np.full_like(x, np.inf)), "weight is not finite"),
    ("scheme", {}, dict(scheme="bdf3"), "scheme must be 'bdf1' or 'bdf2'"),
    ("nsteps", {}, dict(nsteps=0), "nsteps must be an integer >= 1"),
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
        ctor, kw = dict(ctor), {"goal": _one, "nsteps": 4, **kw}
        degrees = ctor.pop("_degrees", False)
        s = pkg.FEMLSSVRPrimalSolver(9, **ctor)
        if degrees:
            s.element_degrees = np.full(8, 9)
        with pytest.raises(ValueError, match=re.escape(match)):
            s.solve_transient_sensitivity(_one, 0.1, **kw)
            raise AssertionError(f"{name}: not refused")
    # what is not refused reaches the device: the same size as the "too large" case, to the byte
    for kw in (dict(goal=_one, max_state_bytes=5 * 9 * 8), dict(_OBS)):
        with pytest.raises(AssertionError, match="device call"):
            pkg.FEMLSSVRPrimalSolver(9).solve_transient_sensitivity(_one, 0.1, nsteps=4, **kw)


def test_demo_record_of_the_prototype():
    """The inverse problem of the prototype: the misfit falls monotonically, to the recorded value."""
    hist = proto.demo()
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] - tr.DEMO_FINAL) <= 1e-6 * tr.DEMO_FINAL
