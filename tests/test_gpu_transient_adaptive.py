"""GPU: adaptive time stepping -- the two kernels against their host mirrors, the facade's loop
against the numpy prototype on the bands the device assembled, tolerance proportionality, the enhanced snapshots against
the oracle's rows, the sequence of ``ops`` calls, and the efficiency record."""
import functools
import math
import types

import numpy as np
import pytest

import transient_adaptive_rules as R
import transient_rules as tr

pytestmark = pytest.mark.gpu
proto = R.proto
SIZES = [1, 2, 255, 256, 257, 300000]          # 300000 nodes exceed the 1024 x 256 grid: the grid-stride loop runs


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("beta1", [0.0, -0.37])
@pytest.mark.parametrize("ne", SIZES)
def test_step_kernel_is_the_host_mirror(dev, ne, beta1):
    import torch
    from hybrid_fem_lssvr_amd import ops
    d = tr.kernel_inputs(ne, 1, 2, 2, seed=30)
    rng = np.random.default_rng(ne)
    kd, ko = rng.uniform(1.0, 3.0, ne + 1), -rng.uniform(0.2, 1.0, ne)
    s, b0, inv_dt = 1.4321 / 0.0173, 1.63, 1.0 / 0.0173
    U1 = None if beta1 == 0.0 else d["U1"]
    _, adiag_h, aoff_h, b_h = R.step_host(kd, ko, d["md"], d["mo"], d["U0"][0], None if U1 is None else U1[0],
                                          d["loads"], d["phi"][0], s, b0, beta1, inv_dt)
    T = {k: _t(v, dev) for k, v in dict(kd=kd, ko=ko, md=d["md"], mo=d["mo"], U0=d["U0"], U1=d["U1"],
                                        loads=d["loads"], phi=d["phi"]).items()}
    adiag, aoff = torch.full((ne + 1,), -7.25, dtype=torch.float64, device=dev), \
        torch.full((ne,), -7.25, dtype=torch.float64, device=dev)
    u1 = None if U1 is None else T["U1"]
    args = (T["kd"], T["ko"], T["md"], T["mo"], T["U0"], u1, T["loads"], T["phi"], s, b0, beta1, inv_dt)
    b = ops.ts_step(*args, adiag=adiag, aoff=aoff, write_bands=False)
    assert torch.all(adiag == -7.25) and torch.all(aoff == -7.25)           # the skip flag leaves the bands alone
    assert _bits(b.cpu().numpy()[0], b_h)
    b = ops.ts_step(*args, adiag=adiag, aoff=aoff)
    assert _bits(adiag.cpu().numpy(), adiag_h) and _bits(aoff.cpu().numpy(), aoff_h)
    assert _bits(b.cpu().numpy()[0], b_h)
    want = ops.ts_rhs(T["md"], T["mo"], T["U0"], u1, T["loads"], T["phi"], b0, beta1, inv_dt)
    assert torch.equal(b, want)                                             # b is ops.ts_rhs, bit for bit


@pytest.mark.parametrize("kinds", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("ne", SIZES)
def test_error_kernel_is_the_host_mirror(dev, ne, kinds):
    from hybrid_fem_lssvr_amd import ops
    Us, w4, w3 = R.error_inputs(ne)
    Us = [u.copy() for u in Us]
    if ne >= 255:                                   # non-finite rows in the first and the last workgroup's range
        Us[0][3], Us[1][ne - 2] = math.nan, math.inf
    T = [_t(u, dev) for u in Us]
    for w, k in ((w4, 3), (w3, None)):
        got = ops.ts_error(T[0], T[1], T[2], None if k is None else T[3], w, 1e-6, 1e-4, kinds).cpu().numpy()
        want = R.error_host(Us[0], Us[1], Us[2], None if k is None else Us[3], w, 1e-6, 1e-4, kinds)[1]
        assert _bits(got, want), (got, want)
        assert got[3] == (2.0 if ne >= 255 else 0.0)


def _solve(case, enhance=False, **kw):
    import hybrid_fem_lssvr_amd as pkg
    ctor, call = case.facade(**kw)
    return pkg.FEMLSSVRPrimalSolver(**ctor).solve_transient_adaptive(case.u0, case.t_end, enhance=enhance, **call)


def _checked_bands(case, sol):
    """sol.bands after each array has been held against the oracle's assembly (tr.BANDS_BAR, section 26)."""
    want = proto.assembled(case.nodes, case.a, case.c, case.rho, [f for _, f in case.forcing] if case.forcing
                           else [tr._zero])
    for key in ("mass", "stiff"):
        (gd, go), (wd, wo) = sol.bands[key], want[key]
        sc = np.abs(wd)
        assert np.max(np.abs(gd - wd) / sc) <= tr.BANDS_BAR
        assert np.max(np.abs(go - wo) / np.maximum(sc[:-1], sc[1:])) <= tr.BANDS_BAR
    for got_r, want_r in zip(sol.bands["loads"], want["loads"]):
        sc = float(np.max(np.abs(want_r)))
        assert (np.max(np.abs(got_r - want_r)) / sc if sc > 0.0 else np.max(np.abs(got_r))) <= tr.BANDS_BAR
    return sol.bands


@pytest.mark.parametrize("name", ["decay", "pulse", "general-33"])
def test_loop_against_the_prototype(dev, note, name):
    """The same accept / reject sequence as the prototype, every attempt's step and the nodal snapshots within 10x the
    float64 prototype's own distance from the np.longdouble loop, all on the bands the device assembled."""
    case = R.CASES[name]()
    sol = _solve(case)
    bands = _checked_bands(case, sol)
    _, ref, p64 = R.references(name, bands)
    ok, margins = R.decisions_clear(p64)
    assert ok, margins
    assert np.array_equal(ref["steps"][:, 3], p64["steps"][:, 3])
    assert np.array_equal(sol.steps[:, 3], p64["steps"][:, 3])              # the same decisions, in the same order
    assert (sol.n_accepted, sol.n_rejected, sol.n_restarts) == (p64["n_accepted"], p64["n_rejected"],
                                                                p64["n_restarts"])
    if name == "pulse":
        assert sol.n_rejected > 0 and sol.n_restarts > 0
    assert sol.times.dtype == np.float64 and _bits(sol.times, np.asarray(case.t_out or [case.t_end], dtype=np.float64))
    assert sol.monitor.shape == (int(np.count_nonzero(np.isfinite(sol.steps[:, 2]))), 4)
    assert _bits(sol.monitor[:, 0], sol.steps[np.isfinite(sol.steps[:, 2]), 2]) and not sol.monitor[:, 3].any()
    e_dt, bar_dt, read_dt = R.dt_reading(name, sol.steps, bands)
    e_u, bar_u, read_u = R.nodal_reading(name, sol.nodal, bands)
    note(f"adaptive {name} dt vs longdouble loop", e_dt, bar_dt)
    note(f"adaptive {name} nodal vs longdouble loop", e_u, bar_u)
    print(f"{name}: attempts {len(sol.steps)} rejected {sol.n_rejected} restarts {sol.n_restarts}; dt: device {e_dt:.2e} "
          f"prototype {read_dt:.2e} bar {bar_dt:.2e}; nodal: device {e_u:.2e} prototype {read_u:.2e} bar {bar_u:.2e}; "
          f"margins {margins[0]:.2e} {margins[1]:.2e}")
    assert e_dt <= bar_dt and e_u <= bar_u


def test_tolerance_proportionality(dev, note):
    """Case (a) at three tolerances: the global error at t = 1 against the exact semi-discrete solution falls
    monotonically, each within 1.5x of the prototype's own, with the prototype's accepted-step counts."""
    errs = []
    for tol in R.PROPORTIONAL_TOLS:
        case = R.decay(tol)
        sol = _solve(case)
        bands = _checked_bands(case, sol)
        _, _, p64 = R.references(f"decay-{tol:g}", bands)
        assert R.decisions_clear(p64)[0]
        got, want = R.global_error(case, bands, sol.nodal[-1]), R.global_error(case, bands, p64["nodal"][-1])
        note(f"adaptive decay tol={tol:g} global error at t=1", got)
        print(f"tol {tol:g}: accepted {sol.n_accepted} (prototype {p64['n_accepted']}), global error device {got:.3e} "
              f"prototype {want:.3e}")
        assert sol.n_accepted == p64["n_accepted"] and sol.n_rejected == p64["n_rejected"]
        assert want / 1.5 <= got <= 1.5 * want
        errs.append(got)
    assert errs[0] > errs[1] > errs[2]


def test_enhanced_snapshots_against_the_oracle_rows(dev, note):
    """W of case (c)'s two snapshots against the oracle's reaction rows fed the same right-hand-side table (the
    np.longdouble loop's u and w, the step's own alpha, beta0, beta1, 1 / h in w), rel-L2, the reaction family's bar."""
    M, n = 9, 16
    case = R.general()
    sol = _solve(case, enhance=True, M=M, n_colloc=n)
    bands = _checked_bands(case, sol)
    _, ref, p64 = R.references("general-33", bands)
    assert np.array_equal(sol.steps[:, 3], p64["steps"][:, 3]) and len(sol.enhanced) == 2

    def rows(r, k):
        return R.tproto.enhance_snapshot(case.nodes, np.asarray(r["nodal"][k], dtype=np.float64),
                                         np.asarray(r["diffs"][k], dtype=np.float64), r["phi"][k],
                                         [f for _, f in case.forcing], M, 1e4, n, a=case.a, da=case.da, c=case.c,
                                         rho=case.rho, kinds=case.kinds, g=r["g"][k])
    worst = noise = 0.0
    for k, e in enumerate(sol.enhanced):
        assert int(e.status.sum().item()) == 0
        Wl = rows(ref, k)
        worst = max(worst, float(tr.orc.rel_l2_coef(e.W.cpu().numpy(), Wl).max()))
        noise = max(noise, float(tr.orc.rel_l2_coef(rows(p64, k), Wl).max()))
    bar = max(tr.ENH_FAMILY_BAR, R.MARGIN * noise)
    note("adaptive enhanced M=9 vs oracle rows", worst, bar)
    print(f"enhanced snapshots: device {worst:.2e}, prototype noise {noise:.2e}, bar {bar:.2e}")
    assert worst <= bar
    x = np.linspace(-1.0, 1.0, 41)
    assert np.all(np.isfinite(sol.evaluate(1, x)))


CPU = "Tensor.cpu"


def test_call_sequence_and_copies(dev, monkeypatch):
    """Before the loop ``p1_assemble`` exactly twice; per attempt ``ts_step`` and ``tridiag_bc_solve_multi``, and for
    every attempt with an estimate (all but a first step) ``ts_error`` and one ``Tensor.cpu`` of four doubles; at an
    accepted output step ``ts_source_table``; one ``enhance_multi`` and one final read-back."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    calls = []

    def logged(label, fn):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            calls.append((label, a[0].numel()) if label == CPU else label)
            return fn(*a, **k)
        return wrapper
    for nm, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not nm.startswith("_") and fn.__module__ == ops.__name__:
            monkeypatch.setattr(ops, nm, logged(nm, fn))
    monkeypatch.setattr(torch.Tensor, "cpu", logged(CPU, torch.Tensor.cpu))
    case = R.pulse()
    sol = _solve(case, enhance=True)
    monkeypatch.undo()
    start = calls.index("ts_step")
    assert [c for c in calls[:start] if not isinstance(c, tuple)] == ["p1_assemble", "p1_assemble", "p1_load_multi",
                                                                      "tridiag_work"]
    expected, k = [], 0
    t_out = np.asarray(case.t_out)
    for t, h, err, acc in sol.steps:
        expected += ["ts_step", "tridiag_bc_solve_multi"]
        if math.isfinite(err):
            expected += ["ts_error", (CPU, 4)]
        if t == 0.0 and not math.isfinite(err):
            k = 0                                                           # a (re)start
        if acc and k < len(t_out) and abs(t + h - t_out[k]) <= 1e-12:      # (no other step ends within 1e-9 h of it)
            expected.append("ts_source_table")
            k += 1
    loop = calls[start:]
    assert loop[:len(expected)] == expected
    tail = loop[len(expected):]
    assert tail[0] == "enhance_multi" and [c for c in tail if isinstance(c, tuple)][-1][1] > 4
    assert sum(1 for c in tail if isinstance(c, tuple)) == 1               # the one read-back after the loop
    assert calls.count("p1_assemble") == 2


def test_efficiency_record(dev, note):
    """A record, not a bar on speed: on case (b), the number of equal BDF2 steps solve_transient needs for the error
    the adaptive run has at t = 1 (against 8192 equal steps of solve_transient itself), next to the
    adaptive run's attempts."""
    import hybrid_fem_lssvr_amd as pkg
    case = R.pulse()
    sol = _solve(case)
    ctor, call = case.facade()
    fixed = dict(weight=None, forcing=case.forcing, end_data=case.end_data, enhance=False)
    fine = pkg.FEMLSSVRPrimalSolver(**ctor).solve_transient(case.u0, case.t_end, nsteps=8192, **fixed).nodal[-1]
    e_adapt = float(np.max(np.abs(sol.nodal[-1] - fine)))
    nsteps, e_fixed = 4, math.inf
    while nsteps < 4096:
        nsteps *= 2
        e_fixed = float(np.max(np.abs(pkg.FEMLSSVRPrimalSolver(**ctor).solve_transient(
            case.u0, case.t_end, nsteps=nsteps, **fixed).nodal[-1] - fine)))
        if e_fixed <= e_adapt:
            break
    note("adaptive pulse error at t=1", e_adapt)
    print(f"pulse: adaptive {len(sol.steps)} attempts ({sol.n_accepted} accepted) reach {e_adapt:.3e} at t = 1; "
          f"equal BDF2 steps need {nsteps} (power of two) for {e_fixed:.3e}")
    assert e_fixed <= e_adapt and math.isfinite(e_adapt)


def test_refusals_launch_nothing(dev, monkeypatch):
    tr.check_refusals(monkeypatch, R.call_adaptive, R.refusals(), R.passing())
