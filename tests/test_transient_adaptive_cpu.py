"""CPU: adaptive time stepping through the host mirrors lssvr_ts_step_host / lssvr_ts_error_host,
the facade's scalar rules and the numpy prototype; the refusals of the facade and of both entries.  No device."""
import math

import numpy as np
import pytest

import transient_adaptive_rules as R
import transient_rules as tr

proto = R.proto


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


# ---- lssvr_ts_step_host ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta1", [0.0, -0.37])
@pytest.mark.parametrize("nR", [1, 3])
@pytest.mark.parametrize("ne", [1, 2, 5, 257])
def test_step_host_bits(ne, nR, beta1):
    d = tr.kernel_inputs(ne, 1, nR, 4, seed=30)
    rng = np.random.default_rng(ne + nR)
    kd, ko = rng.uniform(1.0, 3.0, ne + 1), -rng.uniform(0.2, 1.0, ne)
    s, b0, inv_dt = 1.4321 / 0.0173, 1.63, 1.0 / 0.0173
    U1 = None if beta1 == 0.0 else d["U1"][0]
    _, adiag, aoff, b = R.step_host(kd, ko, d["md"], d["mo"], d["U0"][0], U1, d["loads"], d["phi"][0], s, b0, beta1,
                                    inv_dt)
    assert _bits(adiag, kd + s * d["md"]) and _bits(aoff, ko + s * d["mo"])
    _, want = tr.rhs_host(d["md"], d["mo"], d["U0"], None if U1 is None else d["U1"], d["loads"], d["phi"], b0, beta1,
                          inv_dt)
    assert _bits(b, want[0])
    assert _bits(b, tr.rhs_numpy(d["md"], d["mo"], d["U0"], None if U1 is None else d["U1"], d["loads"], d["phi"], b0,
                                 beta1, inv_dt)[0])
    # the skip flag: the bands keep the sentinel, b is the same, and K may be missing
    _, adiag, aoff, b2 = R.step_host(kd, ko, d["md"], d["mo"], d["U0"][0], U1, d["loads"], d["phi"][0], s, b0, beta1,
                                     inv_dt, write_bands=False, sentinel=-7.25)
    assert np.all(adiag == -7.25) and np.all(aoff == -7.25) and _bits(b2, b)


# ---- lssvr_ts_error_host --------------------------------------------------------------------------------------------
KINDS = [(0, 0), (1, 0), (0, 1), (1, 1)]


@pytest.mark.parametrize("kinds", KINDS)
@pytest.mark.parametrize("ne", [1, 2, 5, 257])
def test_error_host_bits(ne, kinds):
    Us, w4, w3 = R.error_inputs(ne)
    for w, U0 in ((w4, Us[3]), (w3, None)):
        got = R.error_host(Us[0], Us[1], Us[2], U0, w, 1e-6, 1e-4, kinds)[1]
        want = R.error_numpy(Us[0], Us[1], Us[2], U0, w, 1e-6, 1e-4, kinds)
        assert _bits(got, want), (got, want)
        assert got[3] == 0.0 and (got[0] > 0.0 or kinds == (0, 0) and ne == 1)


def test_error_host_skips_dirichlet_ends():
    Us, w4, _ = R.error_inputs(40)
    base = R.error_host(*Us, w4, 1e-6, 1e-4, (0, 0))[1]
    Us[0] = Us[0].copy()
    Us[0][0], Us[0][-1] = 1e30, -1e30
    assert _bits(R.error_host(*Us, w4, 1e-6, 1e-4, (0, 0))[1], base)
    robin = R.error_host(*Us, w4, 1e-6, 1e-4, (1, 0))[1]
    assert robin[2] == 1e30 and robin[1] > 1e20 and robin[0] != base[0]


def test_error_host_nan_counts_once_and_leaves_the_maxima():
    Us, w4, _ = R.error_inputs(40)
    base = R.error_host(*Us, w4, 1e-6, 1e-4, (0, 0))[1]
    e = np.abs(sum(w * u for w, u in zip(w4, Us)))
    q = e / (1e-6 + 1e-4 * np.maximum(np.abs(Us[0]), np.abs(Us[1])))
    holders = {int(np.argmax(v[1:-1])) + 1 for v in (q, e, np.abs(Us[0]))}
    i = next(j for j in range(1, 39) if j not in holders and j + 1 not in holders)   # rows that hold no maximum
    Us[0] = Us[0].copy()
    Us[0][i] = math.nan
    got = R.error_host(*Us, w4, 1e-6, 1e-4, (0, 0))[1]
    assert got[3] == 1.0 and _bits(got[:3], base[:3])
    Us[1] = Us[1].copy()
    Us[1][i + 1 if i + 1 < 40 else i - 1] = math.inf         # sc is not finite there: a second row
    assert R.error_host(*Us, w4, 1e-6, 1e-4, (0, 0))[1][3] == 2.0


def test_error_host_zero_weights_read_nothing():
    Us, _, w3 = R.error_inputs(40)
    want = R.error_host(Us[0], Us[1], Us[2], None, w3, 1e-6, 1e-4, (1, 1))[1]
    got = R.error_host(Us[0], Us[1], Us[2], np.full(41, math.nan), w3, 1e-6, 1e-4, (1, 1))[1]
    assert np.all(np.isfinite(got)) and _bits(got, want)
    w = (w3[0], w3[1], 0.0, 0.0)
    got = R.error_host(Us[0], Us[1], np.full(41, math.nan), None, w, 1e-6, 1e-4, (1, 1))[1]
    assert np.all(np.isfinite(got)) and _bits(got, R.error_numpy(Us[0], Us[1], None, None, w, 1e-6, 1e-4, (1, 1)))


# ---- coefficients, weights, controller: the facade's functions and the prototype's, on literal cases ---------------------
def _rules():
    from hybrid_fem_lssvr_amd import solver
    return [(proto.coefficients, lambda h, hp, hpp=None, al=None: proto.weights_bdf1(h, hp) if hpp is None
             else proto.weights_bdf2(h, hp, hpp, al), proto.controller, proto.trial_step, proto.next_dt),
            (solver.ts_coefficients, solver.ts_error_weights, solver.ts_controller, solver.ts_trial_step,
             solver.ts_next_dt)]


def test_coefficients_and_weights():
    for coef, weights, _, _, _ in _rules():
        assert coef(1.0) == (1.5, 2.0, -0.5)
        for om in (0.2, 0.7, 2.0):
            al, b0, b1 = coef(om)
            assert 1.0 <= al < 2.0 and abs(al - b0 - b1) < 4 * R.EPS        # consistency: constants are reproduced
        # y = t^3 through one variable-step BDF2 step from exact data, steps 0.013 / 0.011 / 0.007
        h, hp, hpp = 0.013, 0.011, 0.007
        t = np.array([0.4 + hpp + hp + h, 0.4 + hpp + hp, 0.4 + hpp, 0.4])
        y, dy = t ** 3, 3.0 * t[0] ** 2
        al, b0, b1 = coef(h / hp)
        u_new = (b0 * y[1] + b1 * y[2] + h * dy) / al
        e = float(np.dot(weights(h, hp, hpp, al), y))
        assert abs(e - (u_new - y[0])) < 64 * R.EPS * abs(y[0]) and abs(e) > 1e-7
        # y = t^2 through one backward-Euler step, read over the next (different) step
        t = np.array([0.4 + hp + h, 0.4 + hp, 0.4])
        u1 = t[2] ** 2 + hp * 2.0 * t[1]
        w = weights(h, hp)
        assert w[3] == 0.0
        e = float(np.dot(w[:3], t ** 2))
        assert abs(e - h * h) < 64 * R.EPS and abs((u1 - t[1] ** 2) - hp * hp) < 64 * R.EPS


def test_controller_literal_cases():
    for _, _, ctl, trial, nxt in _rules():
        assert ctl(1e-9, 0.0, 3, False) == (True, 2.0)                      # clip at 2
        assert ctl(0.0, 0.0, 3, False) == (True, 2.0)
        assert ctl(1e9, 0.0, 3, False) == (False, 0.2)                      # clip at 0.2
        assert ctl(1e-9, 0.0, 3, True) == (True, 1.0)                       # no growth after a rejection
        assert ctl(8.0, 0.0, 3, True) == (False, 0.9 * 8.0 ** (-1.0 / 3.0))
        assert ctl(0.5, 0.0, 2, False) == (True, 0.9 * 0.5 ** -0.5)         # step 2: p = 2
        assert ctl(1.0, 0.0, 3, False) == (True, 0.9)
        assert ctl(math.nextafter(1.0, 2.0), 0.0, 3, False)[0] is False
        assert ctl(0.1, 1.0, 3, False) == (False, 0.2)                      # a non-finite count rejects
        assert ctl(math.nan, 0.0, 3, False) == (False, 0.2) and ctl(math.inf, 0.0, 3, False) == (False, 0.2)
        # output clipping: the output time is hit exactly, also when the step falls just short of it
        assert trial(0.3, 0.05, 1.0, None, 0.5) == (0.05, 0.35, False)
        h, t_new, short = trial(0.3, 0.25, 1.0, None, 0.5)
        assert t_new == 0.5 and h == 0.5 - 0.3 and short
        h, t_new, short = trial(0.3, 0.2 * (1.0 - 1e-10), 1.0, None, 0.5)
        assert t_new == 0.5 and h == 0.5 - 0.3 and not short
        assert trial(0.3, 0.5, 0.1, None, 1.0) == (0.1, 0.4, True)          # dt_max
        assert trial(0.3, 0.5, 1.0, 0.04, 1.0) == (0.08, 0.38, True)        # omega <= 2
        # a shortened, accepted step does not shrink the controller's dt; a rejection and a full step do set it
        assert nxt(0.25, 0.2, True, True, 1.1) == 0.25 and nxt(0.25, 0.2, True, True, 2.0) == 0.4
        assert nxt(0.25, 0.2, True, True, 0.8) == 0.8 * 0.2 and nxt(0.25, 0.2, True, False, 0.5) == 0.1
        assert nxt(0.25, 0.25, False, True, 1.5) == 0.375


# ---- the prototype loop, the conditions on the cases, and the loop through the host mirrors -----------------------------------
def _all_cases():
    return [R.decay(t) for t in R.PROPORTIONAL_TOLS] + [R.pulse(), R.general()]


def test_cases_keep_their_decisions_clear_of_the_thresholds():
    for case in _all_cases():
        res = case.run()
        ok, (me, mf) = R.decisions_clear(res)
        print(f"{case.name}: margins |err - 1| {me:.2e}, factor {mf:.2e}; accepted {res['n_accepted']} rejected "
              f"{res['n_rejected']} restarts {res['n_restarts']}")
        assert ok, (case.name, me, mf)
        assert np.array_equal(res["times"], np.asarray(case.t_out if case.t_out else [case.t_end]))
        assert np.all(res["steps"][1:, 1] <= 2.0 * np.maximum.accumulate(res["steps"][:, 1])[:-1] * (1 + 1e-12))
    assert R.pulse().run()["n_rejected"] > 0 and R.pulse().run()["n_restarts"] > 0


def test_prototype_matches_the_issue_table_and_its_slope():
    errs = []
    for tol, accepted in zip(R.PROPORTIONAL_TOLS, (33, 58, 113)):
        case = R.decay(tol)
        res = case.run()
        assert res["n_accepted"] == accepted and res["n_rejected"] == 0
        errs.append(R.global_error(case, proto.assembled(case.nodes, f_list=[tr._zero]), res["nodal"][-1]))
    print("global error at t = 1:", errs)
    assert errs[0] > errs[1] > errs[2]
    slopes = [math.log10(errs[i] / errs[i + 1]) for i in range(2)]
    assert all(abs(s - 2.0 / 3.0) < 0.1 for s in slopes), slopes            # per-step control at order 2


@pytest.mark.parametrize("name", ["pulse", "general-33"])
def test_loop_through_host_mirrors_equals_the_prototype(name):
    """The loop with lssvr_ts_step_host and lssvr_ts_error_host in place of the numpy statements: the same bits, so
    the same decisions, steps and snapshots."""
    case, _, want = R.references(name)
    hold = {}

    def matrix_fn(kd, ko, md, mo, s):
        hold["s"] = s
        return kd + s * md, ko + s * mo

    def rhs_fn(md, mo, u0, u1, b0, b1, inv_h, L, phi):
        kd, ko = proto.assembled(case.nodes, case.a, case.c, case.rho,
                                 [f for _, f in case.forcing])["stiff"] if "K" not in hold else hold["K"]
        hold["K"] = (kd, ko)
        adiag, aoff, b = R.matrix_host_and_rhs(kd, ko, md, mo, u0, u1, L, phi, hold["s"], b0, b1, inv_h)
        assert _bits(adiag, kd + hold["s"] * md) and _bits(aoff, ko + hold["s"] * mo)
        return b
    got = case.run(matrix_fn=matrix_fn, rhs_fn=rhs_fn, estimate_fn=R.estimate_host)
    assert _bits(got["steps"], want["steps"]) and _bits(got["nodal"], want["nodal"])


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_facade_refusals(monkeypatch):
    tr.check_refusals(monkeypatch, R.call_adaptive, R.refusals(), R.passing())


def test_entry_refusals():
    from hybrid_fem_lssvr_amd import _capi
    NULL, SIZE = -1, -2
    d = tr.kernel_inputs(5, 1, 2, 4, seed=3)
    kd, ko = np.ones(6), -np.ones(5)
    args = [kd, ko, d["md"], d["mo"], d["U0"][0], d["U1"][0], d["loads"], d["phi"][0], 2.0, 1.5, -0.5, 3.0]

    def step(i=None, v=None, **kw):
        a = list(args)
        if i is not None:
            a[i] = v
        return R.step_host(*a, check=False, **kw)[0]
    assert step() == 0
    assert step(8, math.nan) == SIZE and step(9, math.inf) == SIZE and step(10, math.nan) == SIZE
    assert step(11, -math.inf) == SIZE
    assert step(6, np.ones((9, 6))) == SIZE                                  # R = 9
    assert step(5, None) == NULL                                             # beta1 != 0 needs U1
    lib = _capi.load()
    hp = tr._hp
    out = np.zeros(6)
    o5 = np.zeros(5)

    def raw(**over):
        a = dict(kd=hp(kd), ko=hp(ko), md=hp(d["md"]), mo=hp(d["mo"]), U0=hp(d["U0"][0]), U1=hp(d["U1"][0]),
                 loads=hp(d["loads"]), phi=hp(d["phi"][0]), ne=5, R=2, s=2.0, b0=1.5, b1=-0.5, inv=3.0, wb=1,
                 adiag=hp(out), aoff=hp(o5), b=hp(np.zeros(6)))
        a.update(over)
        return lib.lssvr_ts_step_host(*a.values())
    assert raw() == 0
    assert raw(ne=0) == SIZE and raw(R=0) == SIZE and raw(wb=2) == SIZE
    for nm in ("md", "mo", "U0", "loads", "phi", "b", "kd", "ko", "adiag", "aoff"):
        assert raw(**{nm: None}) == NULL, nm
    assert raw(wb=0, kd=None, ko=None, adiag=None, aoff=None) == 0           # K is not read without the band writes
    assert raw(adiag=hp(kd)) == SIZE and raw(b=hp(d["md"])) == SIZE and raw(b=hp(d["U0"][0])) == SIZE   # aliases
    assert raw(adiag=hp(out), b=hp(out)) == SIZE
    buf = np.zeros(7 * 8 + 8, dtype=np.uint8)
    off = (-buf.ctypes.data) % 8 + 4                                         # 4 bytes past an 8-byte boundary
    mis = buf[off:off + 48].view(np.float64)
    assert mis.ctypes.data % 8 == 4 and raw(b=hp(mis)) == SIZE
    assert b"aligned" in lib.lssvr_last_error()

    Us, w4, _ = R.error_inputs(5)

    def err(kinds=(0, 0), w=w4, atol=1e-6, rtol=1e-4, U=Us):
        return R.error_host(U[0], U[1], U[2], U[3], w, atol, rtol, kinds, check=False)[0]
    assert err() == 0
    assert err(kinds=(2, 0)) == SIZE and err(kinds=(0, -1)) == SIZE
    assert err(w=(math.nan, 1.0, 1.0, 1.0)) == SIZE and err(w=(1.0, 1.0, 1.0, math.inf)) == SIZE
    assert err(atol=-1.0) == SIZE and err(rtol=-1.0) == SIZE and err(atol=0.0, rtol=0.0) == SIZE
    assert err(atol=math.nan) == SIZE and err(rtol=math.inf) == SIZE
    assert err(U=[Us[0], Us[1], None, Us[3]]) == NULL and err(U=[Us[0], Us[1], Us[2], None]) == NULL
    assert err(U=[Us[0], Us[1], None, None], w=(1.0, -1.0, 0.0, 0.0)) == 0
    o4 = np.zeros(4)
    assert lib.lssvr_ts_error_host(None, hp(Us[1]), None, None, 0, 0, 5, 1.0, 1.0, 0.0, 0.0, 1e-6, 1e-6, hp(o4)) == NULL
    assert lib.lssvr_ts_error_host(hp(Us[0]), hp(Us[1]), None, None, 0, 0, 0, 1.0, 1.0, 0.0, 0.0, 1e-6, 1e-6,
                                   hp(o4)) == SIZE
    assert lib.lssvr_ts_error_host(hp(Us[0]), hp(Us[1]), None, None, 0, 0, 5, 1.0, 1.0, 0.0, 0.0, 1e-6, 1e-6,
                                   None) == NULL
    assert lib.lssvr_ts_error_work_bytes(0) == 0 and lib.lssvr_ts_error_work_bytes(1) == 32
    assert lib.lssvr_ts_error_work_bytes(300000) == 1024 * 32


def test_transient_solution_keeps_its_constructor():
    from hybrid_fem_lssvr_amd.solver import TransientSolution
    s = TransientSolution(np.zeros(1), np.zeros((1, 3)), [], {}, None)
    assert s.steps is None and s.n_accepted is None and s.n_rejected is None and s.n_restarts == 0
    s = TransientSolution(np.zeros(1), np.zeros((1, 3)), [], {}, steps=np.array([[0, .1, math.nan, 1], [.1, .1, 2, 0]]))
    assert (s.n_accepted, s.n_rejected) == (1, 1)
