"""CPU: semilinear problems -- the host mirrors of csrc/nonlinear.hip against the plain numpy
restatement, the ABI and argument refusals of the new entries, the facade's refusals (before any device call) and the
numpy prototype against itself.  Cases and bars: tests/semilinear_rules.py."""
import ctypes
import math

import numpy as np
import pytest

import semilinear_rules as sr

proto = sr.proto
KINDS = [(sr.POLY, 1), (sr.POLY, 2), (sr.POLY, 4), (sr.POLY, 6), (sr.EXP, 2)]


@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("kind,nterm", KINDS)
@pytest.mark.parametrize("ne,n", [(1, 1), (3, 2), (17, 5), (64, 16), (5, 64)])
def test_linearize_host_is_the_numpy_restatement(note, ne, n, kind, nterm, pm):
    d = sr.kernel_inputs(ne, n, kind, nterm)
    q, c, f = sr.layout(d, pm)
    for with_c in (True, False):
        got = sr.linearize_host(d["u"], d["t"], kind, q, c if with_c else None, f, pm)[1:]
        want = sr.linearize_numpy(d["u"], d["t"], kind, q, c if with_c else None, f, pm)
        if kind == sr.POLY:
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
            continue
        # EXP: the bar is 4x the largest difference this test measures between np.exp and the mirror's exp on the same
        # arguments (in ulps), scaled by the entry's terms -- the sum of their sizes, which bounds both what a changed
        # E does to the entry and the rounding of the entry's own sums after it.  The mirror's E is read back from
        # f_res = f - q_0 E with f = 0 and q_0 = 1.
        uh = d["u"][:-1, None] + (d["u"][1:] - d["u"][:-1])[:, None] * d["t"][None, :]
        q_em = d["q"]
        ones = np.ones_like(uh)
        E_host = -sr.linearize_host(d["u"], d["t"], kind, np.stack([ones, q_em[1]]), None, 0.0 * ones, False,
                                    (False, False, True))[3]
        E_np = np.exp(q_em[1] * uh)
        ulps = float(np.max(np.abs(E_host - E_np) / (sr.EPS * E_np)))
        note(f"np.exp vs the host mirror's exp, ulps (ne={ne}, n={n})", ulps, 1.0)
        assert ulps <= 1.0
        scale = sr.exp_entry_terms(d, with_c)
        for nm, g, w in zip(("c_eff", "f_eff", "f_res"), got, want):
            s = scale[nm].T if pm else scale[nm]
            assert np.all(np.abs(g - w) <= 4.0 * ulps * sr.EPS * s), nm


@pytest.mark.parametrize("want", [(True, False, False), (False, True, False), (False, False, True), (True, True, False),
                                  (True, False, True), (False, True, True)])
def test_linearize_host_skips_a_null_output(want):
    d = sr.kernel_inputs(9, 3, sr.POLY, 4)
    full = sr.linearize_host(d["u"], d["t"], sr.POLY, d["q"], d["c"], d["f"])[1:]
    got = sr.linearize_host(d["u"], d["t"], sr.POLY, d["q"], d["c"], d["f"], want=want)[1:]
    for w, g, f in zip(want, got, full):
        assert (g is None) if not w else np.array_equal(g, f)


@pytest.mark.parametrize("kinds", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("ne", [1, 2, 3, 40, 257])
def test_residual_and_step_host_are_the_numpy_restatement(ne, kinds):
    d = sr.kernel_inputs(ne, 2, sr.POLY, 1)
    args = (d["diag"], d["sub"], d["sup"], d["load"], d["u"], d["u_new"], kinds, d["kappa"], d["g"])
    got = sr.residual_host(*args)[1]
    assert np.array_equal(got, sr.residual_numpy(*args)) and got[3] == 0.0
    # non-finite entries are counted and join no maximum
    u_bad = d["u_new"].copy()
    u_bad[ne // 2] = np.nan
    args_bad = (*args[:5], u_bad, *args[6:])
    got = sr.residual_host(*args_bad)[1]
    assert np.array_equal(got, sr.residual_numpy(*args_bad)) and got[3] == 2.0 and np.all(np.isfinite(got))
    for lam in (1.0, 0.5, 2.0 ** -8):
        assert np.array_equal(sr.step_host(d["u"], d["u_new"], lam)[1], d["u"] + lam * (d["u_new"] - d["u"]))


def test_abi_exports_and_argument_refusals():
    from hybrid_fem_lssvr_amd import _capi, ops
    lib = _capi.load()
    assert lib.lssvr_version() == 7 and (_capi.NL_POLY, _capi.NL_EXP) == (0, 1) == (ops.NL_POLY, ops.NL_EXP)
    for nm in ("lssvr_nl_linearize", "lssvr_nl_linearize_host", "lssvr_nl_residual_work_bytes", "lssvr_nl_residual",
               "lssvr_nl_residual_host", "lssvr_nl_step", "lssvr_nl_step_host"):
        assert hasattr(lib, nm)
    assert lib.lssvr_nl_residual_work_bytes(1) == 32 and lib.lssvr_nl_residual_work_bytes(300000) == 32 * 1024
    assert lib.lssvr_nl_residual_work_bytes(256) == 64 and lib.lssvr_nl_residual_work_bytes(0) == 0
    d = sr.kernel_inputs(4, 3, sr.POLY, 2)
    ok = dict(u=d["u"], t=d["t"], kind=sr.POLY, q=d["q"], c=d["c"], f=d["f"])
    assert sr.linearize_host(**ok, check=False)[0] == 0
    for change, code in ((dict(kind=2), -4), (dict(kind=-1), -4), (dict(nterm=0), -2), (dict(nterm=7), -2),
                         (dict(kind=sr.EXP, nterm=3), -2), (dict(pm=5), -2), (dict(n=0), -2), (dict(n=65), -2),
                         (dict(want=(False, False, False)), -1)):
        assert sr.linearize_host(**{**ok, **change}, check=False)[0] == code, change
    p = sr._hp
    out = np.zeros_like(d["f"])
    u, t, q, f = (sr._h(d[k]) for k in ("u", "t", "q", "f"))
    assert lib.lssvr_nl_linearize_host(None, p(t), p(q), None, p(f), 4, 3, 0, 0, 2, p(out), None, None) == -1
    assert lib.lssvr_nl_linearize_host(p(u), p(t), p(q), None, p(f), 0, 3, 0, 0, 2, p(out), None, None) == -2
    assert lib.lssvr_nl_linearize_host(p(u), p(t), p(q), None, p(f), 4, 3, 0, 0, 2, p(f), None, None) == -2   # aliased
    assert lib.lssvr_nl_linearize_host(p(u), p(t), p(q), None, p(f), 4, 3, 0, 0, 2, p(out), p(out), None) == -2
    # the device entries validate before any launch: safe without a GPU
    fake = ctypes.c_void_p(4096)
    assert lib.lssvr_nl_linearize(fake, fake, fake, None, fake, 4, 3, 0, 9, 2, fake, None, None, None) == -4
    assert lib.lssvr_nl_linearize(fake, fake, fake, None, fake, 4, 3, 0, 0, 2, None, None, None, None) == -1
    kap = (ctypes.c_double * 2)(0.0, 0.0)
    assert lib.lssvr_nl_residual(fake, fake, fake, fake, fake, fake, 0, 3, None, kap, 4, fake, fake, 64, None) == -2
    assert lib.lssvr_nl_residual(fake, fake, fake, fake, fake, fake, 0, 1, None, kap, 4, fake, fake, 64, None) == -1
    assert lib.lssvr_nl_residual(fake, fake, fake, fake, fake, fake, 0, 0, None, kap, 4, fake, None, 64, None) == -1
    assert lib.lssvr_nl_residual(fake, fake, fake, fake, fake, fake, 0, 0, None, kap, 4, fake, fake, 8, None) == -2
    assert lib.lssvr_nl_residual(fake, fake, fake, fake, fake, fake, 0, 0, None, None, 4, fake, fake, 64, None) == -1
    assert lib.lssvr_nl_step(fake, fake, math.inf, 4, ctypes.c_void_p(8192), None) == -2
    assert lib.lssvr_nl_step(fake, fake, 0.5, 4, fake, None) == -2                                    # out is u
    assert lib.lssvr_nl_step(fake, None, 0.5, 4, ctypes.c_void_p(8192), None) == -1
    assert sr.residual_host(d["diag"], d["sub"], d["sup"], d["load"], d["u"], d["u_new"], kinds=(0, 2),
                            check=False)[0] == -2
    assert sr.step_host(d["u"], d["u_new"], math.nan, check=False)[0] == -2


def test_ops_wrappers_reject_host_tensors():
    import torch
    from hybrid_fem_lssvr_amd import ops
    z = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.nl_step(z, z, 0.5)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.nl_linearize(z, z[:2], "poly", torch.zeros(1, 4, 2, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="device memory"):
        ops.nl_residual(z, z[:4], z[:4], z, z, z)
    for kind, nterm in (("cubic", 1), ("poly", 0), ("poly", 7), ("exp", 1), (True, 1)):
        with pytest.raises(ValueError):
            ops.nl_kind(kind, nterm)


def test_facade_refusals_come_before_any_device_call(monkeypatch):
    sr.check_refusals(monkeypatch)


def test_prototype_converges_quadratically_on_case_a(note):
    """Case A from the zero start: full steps only, and the step norms fall quadratically -- s_{k+1} <= C s_k^2 with
    C = 2 |g_uu| / (2 lambda_min) taken generously as 1 (g_uu = 6 u <= 6, lambda_min(K) ~ pi^2 / 4 ... the readings are
    0.06 s_k^2-ish) -- until the rounding floor."""
    for ne in sr.A_NE[2:]:
        r = sr.case_a(ne).run()
        assert r["converged"] and r["lambdas"] == [1.0] * r["iterations"] and r["iterations"] <= 6
        s = r["steps"]
        for k in range(1, len(s) - 1):
            note(f"case A ne={ne} step ratio s_{k + 1} / s_{k}^2", s[k + 1] / s[k] ** 2, 1.0)
            assert s[k + 1] <= max(s[k] ** 2, 1e-13)
        rl = sr.case_a(ne).run(np.longdouble)
        assert rl["iterations"] == r["iterations"] and rl["lambdas"] == r["lambdas"]


def test_prototype_bratu_is_second_order(note):
    errs = []
    for ne in sr.B_NE:
        case = sr.case_b(ne)
        r = case.run()
        assert r["converged"] and r["lambdas"] == [1.0] * r["iterations"]
        errs.append(float(np.max(np.abs(r["u"] - case.exact(case.nodes)))))
    for e0, e1 in zip(errs, errs[1:]):
        note("Bratu nodal error ratio on halving h", e0 / e1, 4.0)
        assert 3.8 <= e0 / e1 <= 4.2
    assert abs(proto.bratu_theta(1.0) - math.sqrt(2.0) * math.cosh(proto.bratu_theta(1.0) / 4.0)) <= 4 * sr.EPS


def test_prototype_damps_case_d_and_is_exact_on_case_e():
    for dtype in (np.float64, np.longdouble):
        r = sr.case_d().run(dtype)
        assert r["converged"] and r["lambdas"] == sr.D_LAMBDAS and r["iterations"] == len(sr.D_LAMBDAS)
    case = sr.case_e()
    r = case.run()
    assert r["converged"] and r["iterations"] == 2 and r["lambdas"] == [1.0, 1.0]
    lin = sr.cr.fem_solve(case.nodes, case.linear["rhs"], None, None, case.linear["reaction"], 2, *case.end_values)
    assert np.max(np.abs(r["u"] - lin)) <= sr.loop_reading("E-17", r["u"])[1]
