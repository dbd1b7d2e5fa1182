"""GPU: transient problems -- the two kernels of csrc/timestep.hip bit for bit against their host
mirrors, the time loop of solve_transient against the numpy prototype, the enhanced snapshots against the oracle's
rows, the accuracy record and the refusals.  Cases and bars: tests/transient_rules.py."""
import numpy as np
import pytest

import transient_rules as tr

pytestmark = pytest.mark.gpu

proto = tr.proto
# the sizes of the issue (workgroup edges, the 512-unknown level of the solver, one table that is grid-strided) and one
# more, past the 262144 threads of the largest grid, so that the per-node kernel is grid-strided too
KERNEL_NE = (1, 2, 3, 254, 255, 256, 257, 600, 100000, 300000)


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=dev)


@pytest.mark.parametrize("nc,R", [(1, 1), (3, 8), (1, 8), (3, 1)])
@pytest.mark.parametrize("ne", KERNEL_NE)
def test_rhs_kernel_is_the_host_mirror(dev, ne, nc, R):
    from hybrid_fem_lssvr_amd import ops
    d = tr.kernel_inputs(ne, nc, R, 2)
    md, mo, U0, U1, loads, phi = (_t(d[k], dev) for k in ("md", "mo", "U0", "U1", "loads", "phi"))
    for b0, b1, with_u1 in ((1.0, 0.0, False), (2.0, -0.5, True)):
        got = ops.ts_rhs(md, mo, U0, U1 if with_u1 else None, loads, phi, b0, b1, 37.0).cpu().numpy()
        want = tr.rhs_host(d["md"], d["mo"], d["U0"], d["U1"] if with_u1 else None, d["loads"], d["phi"], b0, b1,
                           37.0)[1]
        assert np.array_equal(got, want)


@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("n", [2, 16])
@pytest.mark.parametrize("R", [1, 8])
@pytest.mark.parametrize("ne", KERNEL_NE[:-1])
def test_source_table_kernel_is_the_host_mirror(dev, ne, R, n, pm):
    from hybrid_fem_lssvr_amd import ops
    d = tr.kernel_inputs(ne, 1, R, n)
    ftab = np.ascontiguousarray(np.transpose(d["ftab"], (0, 2, 1))) if pm else d["ftab"]
    rtab = np.ascontiguousarray(d["rho_tab"].T) if pm else d["rho_tab"]
    U2, U0, U1, ft, rt, phi = (_t(a, dev) for a in (d["U2"], d["U0"][0], d["U1"][0], ftab, rtab, d["phi"][0]))
    for al, b0, b1, with_u1 in ((1.0, 1.0, 0.0, False), (1.5, 2.0, -0.5, True)):
        got = ops.ts_source_table(U2, U0, U1 if with_u1 else None, ft, rt, phi, al, b0, b1, 100.0,
                                  point_major=pm).cpu().numpy()
        want = tr.source_host(d["U2"], d["U0"][0], d["U1"][0] if with_u1 else None, ftab, rtab, d["phi"][0], al, b0,
                              b1, 100.0, pm)[1]
        assert got.shape == rtab.shape and np.array_equal(got, want)


def _solve(case, enhance=False, **kw):
    import hybrid_fem_lssvr_amd as pkg
    ctor, call = case.facade(**kw)
    return pkg.FEMLSSVRPrimalSolver(**ctor).solve_transient(case.u0, case.t_end, enhance=enhance, **call)


def _checked_bands(case, sol, note):
    """sol.bands, after every array in it has been held against the oracle's assembly of the case (tr.BANDS_BAR)."""
    err = tr.bands_error(case, sol.bands)
    note(f"transient bands {case.name} device vs oracle assembly, scaled", err, tr.BANDS_BAR)
    print(f"{case.name}: bands device vs oracle {err:.2e}, bar {tr.BANDS_BAR:.2e}")
    assert err <= tr.BANDS_BAR
    return sol.bands


@pytest.mark.parametrize("name", sorted(tr.CASES))
def test_loop_against_the_prototype(dev, note, name):
    """The nodal snapshots of solve_transient against the np.longdouble prototype, within 10x the float64 prototype's
    own distance from it, both on the bands the device assembled -- which are first held, array by array, against the
    oracle's assembly of the same problem (tr.LOOP_READ, tr.BANDS_READ record the readings)."""
    case = tr.CASES[name]()
    sol = _solve(case)
    assert sol.nodal.shape == (len(case.snapshots), len(case.nodes))
    np.testing.assert_allclose(sol.times, case.t_end / case.nsteps * np.asarray(case.snapshots), rtol=1e-15)
    err, bar, read = tr.loop_reading(name, sol.nodal, _checked_bands(case, sol, note))
    err_o, bar_o, read_o = tr.loop_reading(name, sol.nodal)
    note(f"transient loop {name} vs longdouble", err, bar)
    note(f"transient loop {name} vs longdouble on the oracle's bands (no bar)", err_o)
    print(f"{name}: device {err:.2e}, prototype {read:.2e}, bar {bar:.2e}; on the oracle's bands {err_o:.2e}, "
          f"{read_o:.2e}")
    assert err <= bar


@pytest.mark.parametrize("scheme", ["bdf1", "bdf2"])
@pytest.mark.parametrize("ne", tr.DECAY_NE)
def test_mode_decay_on_the_device(dev, note, ne, scheme):
    case = tr.decay(ne, scheme)
    sol = _solve(case)
    err, bar = tr.decay_error(case, ne, sol.nodal), tr.decay_bar(ne, scheme)
    note(f"transient decay {scheme} ne={ne}", err, bar)
    print(f"decay {scheme} ne={ne}: device {err:.2e}, prototype {bar / tr.MARGIN:.2e}, bar {bar:.2e}")
    assert err <= bar


@pytest.mark.parametrize("ne,scheme", [(5, "bdf1"), (33, "bdf2")])
def test_bands_of_the_decay_cases(dev, note, ne, scheme):
    case = tr.decay(ne, scheme)
    _checked_bands(case, _solve(case), note)


def test_conservation_on_the_device(dev, note):
    case = tr.neumann()
    sol = _solve(case)
    drift, bar = tr.mass_drift(case, sol.nodal), tr.mass_bar()
    note("transient mass drift", drift, bar)
    print(f"mass drift: device {drift:.2e}, prototype {bar / tr.MARGIN:.2e}, bar {bar:.2e}")
    assert drift <= bar


@pytest.mark.parametrize("M,n", sorted(tr.ENH_READ))
def test_enhanced_snapshots_against_the_oracle_rows(dev, note, M, n):
    """W of the snapshots (two at M = 9, the lane kernel of enhance_multi; M = 20, its per-case path) against the
    oracle's rows on the prototype's data, rel-L2 as in the reaction tests."""
    name = "general-33"
    case = tr.CASES[name]() if M <= 16 else tr.general(snapshots=(64,))
    sol = _solve(case, enhance=True, M=M, n_colloc=n)
    Wref, bar, noise = tr.enhanced_reference(name, M, n, _checked_bands(case, sol, note))
    if M > 16:
        Wref = Wref[-1:]
    assert len(sol.enhanced) == len(case.snapshots)
    worst = 0.0
    for k, e in enumerate(sol.enhanced):
        assert e.n_fallback == 0
        worst = max(worst, float(tr.orc.rel_l2_coef(e.W.cpu().numpy(), Wref[k]).max()))
    note(f"transient enhanced M={M} vs oracle rows", worst, bar)
    print(f"M={M}: device {worst:.2e}, prototype noise {noise:.2e}, bar {bar:.2e}")
    assert worst <= bar
    # evaluate(): the enhanced snapshot meets the moving Dirichlet value at the right end
    g_right = case.end_data[1](sol.times[-1])
    assert abs(float(sol.evaluate(len(sol.enhanced) - 1, np.array([1.0]))[0]) - g_right) <= 1e-9


def test_accuracy_record(dev, note):
    """u = exp(-t) cos(pi x / 2): the device's max errors of the P1 interpolant and of the enhanced snapshot equal the
    prototype's to 3 digits, and the enhanced one is the smaller (the prototype confirms it on the CPU)."""
    import hybrid_fem_lssvr_amd as pkg
    u0, forcing, exact = proto.manufactured()
    xs = np.linspace(-1.0, 1.0, tr.ACCURACY_POINTS)
    ref = exact(xs, tr.ACCURACY_T)
    for ne, (want_p1, want_enh) in tr.ACCURACY.items():
        s = pkg.FEMLSSVRPrimalSolver(ne + 1, lssvr_M=9, lssvr_gamma=1e4, n_colloc=16)
        sol = s.solve_transient(u0, tr.ACCURACY_T, nsteps=tr.ACCURACY_STEPS, forcing=forcing, end_data=(0.0, 0.0))
        e_p1 = float(np.max(np.abs(np.interp(xs, np.linspace(-1.0, 1.0, ne + 1), sol.nodal[-1]) - ref)))
        e_enh = float(np.max(np.abs(sol.evaluate(0, xs) - ref)))
        note(f"transient accuracy ne={ne} interpolant", e_p1)
        note(f"transient accuracy ne={ne} enhanced", e_enh)
        print(f"ne={ne}: interpolant {e_p1:.4e} (prototype {want_p1:.4e}), enhanced {e_enh:.4e} ({want_enh:.4e})")
        assert abs(e_p1 - want_p1) <= 5e-4 * want_p1 and abs(e_enh - want_enh) <= 5e-4 * want_enh
        assert e_enh < e_p1


def test_refusals_launch_nothing(dev, monkeypatch):
    tr.check_refusals(monkeypatch, tr.call_transient, tr.refusals(), tr.passing())
