"""CPU: semilinear transient problems where there is no GPU -- the host mirror of
lssvr_ts_nl_assemble against the plain numpy restatement of its order of sums (POLY bit for bit, EXP within the measured
libm-vs-np.exp bar of section 27), the exports and return codes of the two entries, the facade's refusals with the
loader replaced, and the prototype's float64 loop against its np.longdouble loop."""
import numpy as np
import pytest

import transient_nl_rules as nr

proto = nr.proto


@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("nquad", [1, 2, 5])
@pytest.mark.parametrize("nterm", [1, 4, 6])
@pytest.mark.parametrize("ne", [1, 2, 3, 33])
def test_poly_host_mirror_is_the_numpy_restatement(ne, nterm, nquad, with_a):
    d = nr.kernel_inputs(ne, nquad, nr.POLY, nterm)
    a = d["a"] if with_a else None
    got = nr.assemble_host(d["x"], d["u"], a, d["cs"], d["q"], d["r"], nr.POLY)[1:]
    want = nr.assemble_numpy(d["x"], d["u"], a, d["cs"], d["q"], d["r"], nr.POLY)
    for nm, g, w in zip(("diag", "off", "rhs"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), nm


@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("nquad", [1, 2, 5])
@pytest.mark.parametrize("ne", [1, 2, 3, 33])
def test_exp_host_mirror_within_the_measured_exp_bar(note, ne, nquad, with_a):
    """The bar of section 27: 4x the largest difference this test measures between np.exp and the host library's exp
    on the case's own arguments (in ulps), scaled by the entry's terms (nr.exp_terms).  The library's E is read back as
    section 27's test reads it, from f_res = f - q_0 E of lssvr_nl_linearize_host with f = 0 and q_0 = 1: both host
    entries call the one family routine."""
    import semilinear_rules as sr
    d = nr.kernel_inputs(ne, nquad, nr.EXP, 2)
    a = d["a"] if with_a else None
    rule = nr.kernel_rule(nquad)
    uh = d["u"][:-1, None] + (d["u"][1:] - d["u"][:-1])[:, None] * rule[0][None, :]
    ones = np.ones_like(uh)
    E_host = -sr.linearize_host(d["u"], rule[0], nr.EXP, np.stack([ones, d["q"][1]]), None, 0.0 * ones, False,
                                (False, False, True))[3]
    E_np = np.exp(d["q"][1] * uh)
    ulps = float(np.max(np.abs(E_host - E_np) / (nr.EPS * E_np)))
    note(f"np.exp vs the host library's exp, ulps (ne={ne}, nquad={nquad})", ulps, 1.0)
    assert ulps <= 1.0
    got = nr.assemble_host(d["x"], d["u"], a, d["cs"], d["q"], d["r"], nr.EXP)[1:]
    want = nr.assemble_numpy(d["x"], d["u"], a, d["cs"], d["q"], d["r"], nr.EXP)
    for nm, g, w, s in zip(("diag", "off", "rhs"), got, want, nr.exp_terms(d, with_a)):
        assert np.all(np.abs(g - w) <= 4.0 * ulps * nr.EPS * s), nm


def test_abi_exports_and_return_codes():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    assert lib.lssvr_version() == 7
    for nm in ("lssvr_ts_nl_assemble", "lssvr_ts_nl_assemble_host"):
        assert hasattr(lib, nm) and nm in _capi.SIGNATURES
    d = nr.kernel_inputs(5, 2, nr.POLY, 3)
    ok = dict(x=d["x"], u=d["u"], a_q=d["a"], cs_q=d["cs"], q_q=d["q"], r=d["r"], kind=nr.POLY)
    assert nr.assemble_host(**ok, check=False)[0] == 0
    assert nr.assemble_host(**{**ok, "a_q": None}, check=False)[0] == 0           # a_quad NULL: a = 1
    NULL, SIZE, RHS, QUAD = -1, -2, -4, -7
    for change, code in ((dict(kind=2), RHS), (dict(kind=-1), RHS), (dict(nterm=0), SIZE), (dict(nterm=7), SIZE),
                         (dict(kind=nr.EXP, nterm=3), SIZE), (dict(ne=0), SIZE), (dict(ne=-3), SIZE),
                         (dict(nquad=0), QUAD), (dict(nquad=6), QUAD),
                         *((dict(drop=(nm,)), NULL) for nm in ("x", "u", "cs_q", "q_q", "r", "diag", "off", "rhs"))):
        assert nr.assemble_host(**{**ok, **change}, check=False)[0] == code, change
    n = len(d["x"])
    fresh = lambda: [np.zeros(n), np.zeros(n - 1), np.zeros(n)]        # noqa: E731
    for i, src in ((0, "x"), (0, "u"), (2, "r"), (2, "u"), (1, "cs_q"), (0, "q_q"), (2, "a_q")):
        outs = fresh()
        args = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v) for k, v in ok.items()}
        outs[i] = args[src]
        assert nr.assemble_host(**args, outs=outs, check=False)[0] == SIZE, (i, src)
    same = np.zeros(n)
    assert nr.assemble_host(**ok, outs=[same, np.zeros(n - 1), same], check=False)[0] == SIZE
    assert b"distinct" in lib.lssvr_last_error()


def test_ops_refuses_host_tensors_and_shapes():
    import torch
    from hybrid_fem_lssvr_amd import ops
    z = torch.zeros(5, dtype=torch.float64)
    t = torch.zeros(4, 2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.ts_nl_assemble(z, z, t, "poly", t.unsqueeze(0), z)


def test_refusals_launch_nothing(monkeypatch):
    nr.tr.check_refusals(monkeypatch, nr.tr.call_transient, nr.refusals(), nr.passing())


def test_linear_keywords_are_untouched():
    """nonlinear=None: solve_transient keeps its signature's defaults (None: the linear calls)."""
    import inspect
    import hybrid_fem_lssvr_amd as pkg
    p = inspect.signature(pkg.FEMLSSVRPrimalSolver.solve_transient).parameters
    assert [p[k].default for k in ("nonlinear", "newton_iters", "newton_tol")] == [None, None, None]
    assert pkg.TransientSolution(0, 0, [], {}).newton is None if hasattr(pkg, "TransientSolution") else True


@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_prototype_float64_agrees_with_longdouble(name):
    """The sanity of the reference itself: the float64 loop stays within 100 eps of the np.longdouble loop, relative to
    |u0|_inf, on every case; the monitor's last residual sits at the rounding floor and its count is zero."""
    case, ref, p64 = nr.references(name)
    err, bar, read = nr.loop_reading(name, p64["nodal"])
    print(f"{name}: float64 vs longdouble {read:.2e}")
    assert err == read and read <= 100.0 * nr.EPS
    assert not np.any(p64["newton"][:, :, 3])
    merr, mbar, mread = nr.monitor_reading(name, p64["newton"])
    assert merr == mread and mread <= 100.0 * nr.EPS
    # quadratic convergence in the prototype: r_{k+1} <= C r_k^2 until the floor
    r = np.asarray(p64["newton"][:, :, 0], dtype=np.float64)
    floor = 1e3 * nr.EPS * nr.monitor_terms(case, ref)
    C = 10.0
    assert np.all((r[:, 1:] <= C * r[:, :-1] ** 2) | (r[:, 1:] <= floor))


@pytest.mark.parametrize("scheme,lo,hi", [("bdf1", 0.8, 1.2), ("bdf2", 1.7, 2.3)])
def test_prototype_temporal_order(scheme, lo, hi):
    """The windows of tests/test_transient_cpu.py for the linear case, on the cubic problem (prototype: 1.03, 1.02 and
    2.15, 2.04)."""
    orders = proto.temporal_orders()[scheme]
    print(f"{scheme}: orders {orders}")
    assert all(lo <= o <= hi for o in orders)
