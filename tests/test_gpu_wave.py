"""GPU: wave problems -- the kernel of csrc/wave.hip bit for bit against its host mirror, the time
loop of solve_wave against the numpy prototype (discrete mode, energy, fixed point, temporal order, the np.longdouble
loop), the enhanced snapshots against the oracle's rows and the refusals.  Cases and bars: tests/wave_rules.py."""
import numpy as np
import pytest

import wave_rules as wr

pytestmark = pytest.mark.gpu

proto = wr.proto
# the workgroup edge and the neighbour across it; 300000 is past the 1024 x 256 threads of the largest grid, so the
# grid-stride loop runs a second pass
KERNEL_NE = (1, 2, 255, 256, 257, 300000)


def _t(a, dev):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=dev)


@pytest.mark.parametrize("nc", [1, 8])
@pytest.mark.parametrize("ne", KERNEL_NE)
def test_advance_kernel_is_the_host_mirror(dev, ne, nc):
    """All three modes, with and without damping bands, both Newmark pairs, R = 2: bit for bit; and the fused launch
    equals the split pair of launches."""
    from hybrid_fem_lssvr_amd import ops
    d = wr.kernel_inputs(ne, nc, 2)
    t = {k: _t(v, dev) for k, v in d.items()}
    for damped in (False, True):
        dd, do = (t["dd"], t["do"]) if damped else (None, None)
        for beta, gamma in wr.NEWMARK:
            got = {}
            for label, kw in wr.modes_of(d, damped):
                want = wr.advance_host(dt=wr.KERNEL_DT, beta=beta, gamma=gamma, **kw)[1:]
                res = ops.wave_advance(None if kw["U_new"] is None else t["U_new"], t["U"], t["V"], t["Acc"], t["md"],
                                       t["mo"], dd, do, t["loads"], t["phi"], wr.KERNEL_DT, beta, gamma, rhs=kw["rhs"])
                got[label] = res
                for g, w, nm in zip(res, want, ("V_out", "Acc_out", "rhs_out")):
                    if g is None:
                        assert (label, nm) in (("state", "rhs_out"), ("first", "V_out"), ("first", "Acc_out"))
                    else:
                        assert np.array_equal(g.cpu().numpy(), w), (label, nm, damped, beta)
            v, acc, _ = got["state"]
            split = ops.wave_advance(None, t["U_new"], v, acc, t["md"], t["mo"], dd, do, t["loads"], t["phi"],
                                     wr.KERNEL_DT, beta, gamma)[2]
            assert bool((split == got["fused"][2]).all())


def test_ops_wrapper_refuses_aliasing(dev):
    from hybrid_fem_lssvr_amd import ops
    d = wr.kernel_inputs(5, 1, 1)
    t = {k: _t(v, dev) for k, v in d.items()}
    args = (t["U_new"], t["U"], t["V"], t["Acc"], t["md"], t["mo"], None, None, t["loads"], t["phi"], 0.1, 0.25, 0.5)
    for bad in (dict(V_out=t["V"]), dict(Acc_out=t["Acc"]), dict(V_out=t["Acc"]), dict(rhs_out=t["U"])):
        with pytest.raises(ValueError, match="distinct"):
            ops.wave_advance(*args, **bad)


def _solve(case, enhance=False, **kw):
    import hybrid_fem_lssvr_amd as pkg
    ctor, call = case.facade(**kw)
    return pkg.FEMLSSVRPrimalSolver(**ctor).solve_wave(case.u0, case.v0, case.t_end, enhance=enhance, **call)


def _checked_bands(case, sol, note):
    """sol.bands, after every array in it has been held against the oracle's assembly of the case (wr.BANDS_BAR)."""
    err = wr.bands_error(case, sol.bands)
    note(f"wave bands {case.name} device vs oracle assembly, scaled", err, wr.BANDS_BAR)
    print(f"{case.name}: bands device vs oracle {err:.2e}, bar {wr.BANDS_BAR:.2e}")
    assert err <= wr.BANDS_BAR
    return sol.bands


@pytest.mark.parametrize("ne", wr.MODE_NE)
def test_discrete_mode_on_the_device(dev, note, ne):
    case = wr.mode(ne)
    sol = _solve(case)
    assert sol.nodal.shape == sol.velocity.shape == sol.accel.shape == (wr.MODE_STEPS, ne + 1)
    assert sol.energy.shape == (wr.MODE_STEPS + 1,)
    np.testing.assert_allclose(sol.times, wr.MODE_DT * np.arange(1, wr.MODE_STEPS + 1), rtol=1e-15)
    err, bar = wr.mode_error(case, ne, sol.nodal), wr.mode_bar(ne)
    note(f"wave mode ne={ne}", err, bar)
    print(f"mode ne={ne}: device {err:.2e}, prototype {bar / wr.MARGIN:.2e}, bar {bar:.2e}")
    assert err <= bar


def test_energy_on_the_device(dev, note):
    """d = 0: |E^n - E^0| / E^0 over 64 steps within the bar; d > 0: non-increasing up to the bar; gamma = 0.6: E
    decays with d = 0.  E^0 itself is held against the prototype's."""
    bar = wr.energy_bar()
    case = wr.energy_case()
    sol = _solve(case)
    e_ref = case.run()["energy"]
    assert abs(sol.energy[0] - e_ref[0]) <= 64.0 * wr.EPS * e_ref[0]
    drift = wr.energy_drift(sol.energy)
    note("wave energy drift", drift, bar)
    print(f"energy drift: device {drift:.2e}, prototype {bar / wr.MARGIN:.2e}, bar {bar:.2e}")
    assert drift <= bar
    damped = _solve(wr.energy_case(d=wr.damping)).energy
    rise = wr.energy_rise(damped)
    note("wave energy rise with damping", rise, bar)
    assert rise <= bar and damped[-1] < 0.9 * damped[0]
    lossy = _solve(wr.energy_case(beta=0.3025, gamma=0.6)).energy
    rise = wr.energy_rise(lossy)
    note("wave energy rise with gamma = 0.6", rise, bar)
    assert rise <= bar and lossy[-1] < lossy[0] * (1.0 - 1e-3)


@pytest.mark.parametrize("damped", [False, True])
def test_stationary_solution_is_a_fixed_point(dev, note, damped):
    case, ustat = wr.stationary(wr.damping if damped else None)
    sol = _solve(case)
    err, bar = wr.stationary_error(ustat, sol.nodal), wr.stationary_bar(damped)
    note(f"wave fixed point damped={damped}", err, bar)
    print(f"fixed point damped={damped}: device {err:.2e}, prototype {bar / wr.MARGIN:.2e}, bar {bar:.2e}")
    assert err <= bar


def test_temporal_order_on_the_device(dev, note):
    import hybrid_fem_lssvr_amd as pkg
    u0, v0, exact = proto.standing()
    nodes = np.linspace(-1.0, 1.0, proto.ORDER_NE + 1)
    ref = exact(nodes, proto.ORDER_T)
    errs = []
    for nsteps in proto.ORDER_STEPS:
        s = pkg.FEMLSSVRPrimalSolver(proto.ORDER_NE + 1)
        sol = s.solve_wave(u0, v0, proto.ORDER_T, nsteps=nsteps, forcing=[(0.0, wr._zero)], end_data=(0.0, 0.0),
                           enhance=False)
        errs.append(float(np.max(np.abs(sol.nodal[-1] - ref))))
    orders = [float(np.log2(errs[i] / errs[i + 1])) for i in range(2)]
    bar = wr.order_bar()
    for o in orders:
        note("wave temporal order", o, bar)
    print(f"errors {errs}, orders {orders}, bar {bar:.3f}")
    assert all(o >= bar for o in orders)


@pytest.mark.parametrize("name", sorted(wr.CASES))
def test_loop_against_the_prototype(dev, note, name):
    """u, v and acc of solve_wave against the np.longdouble prototype, each within 10x the float64 prototype's own
    distance from it, on the bands the device assembled -- first held against the oracle's assembly."""
    case = wr.CASES[name]()
    sol = _solve(case)
    got = dict(nodal=sol.nodal, velocity=sol.velocity, accel=sol.accel)
    for k, (err, bar, read) in wr.loop_reading(name, got, _checked_bands(case, sol, note)).items():
        note(f"wave loop {name} {k} vs longdouble", err, bar)
        print(f"{name} {k}: device {err:.2e}, prototype {read:.2e}, bar {bar:.2e}")
        assert err <= bar


@pytest.mark.parametrize("name", sorted(wr.CASES))
@pytest.mark.parametrize("M,n", wr.ENH_CASES)
def test_enhanced_snapshots_against_the_oracle_rows(dev, note, M, n, name):
    """W of the snapshots (two at M = 9, the lane kernel of enhance_multi; M = 20, its per-case path), with and without
    damping (the second ts_source_table call), against the oracle's rows on the longdouble loop's data."""
    full = wr.CASES[name]()
    case = full if M <= 16 else wr.general(snapshots=(64,), d=full.d)
    sol = _solve(case, enhance=True, M=M, n_colloc=n)
    Wref, bar, noise = wr.enhanced_reference(name, M, n, _checked_bands(case, sol, note))
    if M > 16:
        Wref = Wref[-1:]
    assert len(sol.enhanced) == len(case.snapshots)
    worst = 0.0
    for k, e in enumerate(sol.enhanced):
        assert e.n_fallback == 0
        worst = max(worst, float(wr.orc.rel_l2_coef(e.W.cpu().numpy(), Wref[k]).max()))
    note(f"wave enhanced {name} M={M} vs oracle rows", worst, bar)
    print(f"{name} M={M}: device {worst:.2e}, prototype noise {noise:.2e}, bar {bar:.2e}")
    assert worst <= bar
    g_right = case.end_data[1](sol.times[-1])
    assert abs(float(sol.evaluate(len(sol.enhanced) - 1, np.array([1.0]))[0]) - g_right) <= 1e-9


def test_refusals_launch_nothing(dev, monkeypatch):
    wr.tr.check_refusals(monkeypatch, wr.call_wave, wr.refusals(), wr.passing())
