"""GPU: semilinear transient problems -- lssvr_ts_nl_assemble bit for bit against the chain of
existing entries it replaces and against its host mirror, the time loop of solve_transient(..., nonlinear=...) and its
monitor table against the np.longdouble prototype, the temporal orders, the linear limit, the stationary fixed point, the
monitor's behaviour and the enhanced snapshots against the oracle's rows.  Cases and bars: tests/transient_nl_rules.py."""
import math

import numpy as np
import pytest

import transient_nl_rules as nr

pytestmark = pytest.mark.gpu

proto = nr.proto
KINDS = [(nr.POLY, 1), (nr.POLY, 4), (nr.POLY, 6), (nr.EXP, 2)]
# one, two and three elements (end rows only, one interior row), the edges of a 256-thread workgroup, many workgroups
KERNEL_NE = (1, 2, 3, 255, 256, 257, 300000)


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float64)), device=dev)


@pytest.mark.parametrize("kind,nterm", KINDS)
@pytest.mark.parametrize("nquad", [1, 2, 5])
@pytest.mark.parametrize("ne", KERNEL_NE)
def test_fused_kernel_is_the_chain_and_the_host_mirror(dev, note, ne, nquad, kind, nterm):
    """diag, off, rhs of ops.ts_nl_assemble are BIT-EQUAL to nl_linearize (f_tab = 0, c_tab = cs) -> p1_assemble (react)
    -> r + load on the device, with and without a_quad, EXP included (one device routine behind both); against the host
    mirror POLY is bit-equal and EXP within 8 eps of the entry's terms (section 27's device bar: the device library's
    exp against libm)."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    d = nr.kernel_inputs(ne, nquad, kind, nterm)
    x, u, r, aq, cs, q = (_t(d[k], dev) for k in ("x", "u", "r", "a", "cs", "q"))
    t = ops.quad_points(_t([0.0, 1.0], dev), nquad)[0].contiguous()
    for a_dev, a_host in ((aq, d["a"]), (None, None)):
        got = ops.ts_nl_assemble(x, u, cs, kind, q, r, a_quad=a_dev)
        lin = ops.nl_linearize(u, t, kind, q, torch.zeros_like(cs), c_tab=cs)
        chain = ops.p1_assemble(x, nquad, rhs_quad=lin["f_eff"], a_quad=a_dev, c_quad=lin["c_eff"])
        want = dict(diag=chain["diag"], off=chain["off"], rhs=r + chain["load"])
        for nm in ("diag", "off", "rhs"):
            assert torch.equal(got[nm], want[nm]), (nm, a_dev is not None)
        host = nr.assemble_host(d["x"], d["u"], a_host, d["cs"], d["q"], d["r"], kind)[1:]
        if kind == nr.POLY:
            for nm, h in zip(("diag", "off", "rhs"), host):
                assert np.array_equal(got[nm].cpu().numpy(), h), nm
        else:
            worst = 0.0
            for nm, h, s in zip(("diag", "off", "rhs"), host, nr.exp_terms(d, a_host is not None)):
                worst = max(worst, float(np.max(np.abs(got[nm].cpu().numpy() - h) / (nr.EPS * s))))
            note(f"ts_nl_assemble EXP device vs host mirror, eps of the terms (ne={ne}, nquad={nquad})", worst, 8.0)
            assert worst <= 8.0


def test_out_buffers_and_aliasing(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    d = nr.kernel_inputs(7, 2, nr.POLY, 4)
    x, u, r, cs, q = (_t(d[k], dev) for k in ("x", "u", "r", "cs", "q"))
    out = dict(diag=torch.empty_like(x), off=torch.empty(7, dtype=torch.float64, device=dev), rhs=torch.empty_like(x))
    got = ops.ts_nl_assemble(x, u, cs, "poly", q, r, out=out)
    assert all(got[k] is out[k] for k in out)
    ref = ops.ts_nl_assemble(x, u, cs, nr.POLY, q, r)
    assert all(torch.equal(ref[k], out[k]) for k in out)
    with pytest.raises(ValueError, match="distinct"):
        ops.ts_nl_assemble(x, u, cs, "poly", q, r, out=dict(out, rhs=r))
    with pytest.raises(ValueError):
        ops.ts_nl_assemble(x, u[:-1], cs, "poly", q, r)
    with pytest.raises(ValueError):
        ops.ts_nl_assemble(x, u, cs, "exp", q, r)


def _solve(case, enhance=False, **kw):
    import hybrid_fem_lssvr_amd as pkg
    ctor, call = case.facade(**kw)
    return pkg.FEMLSSVRPrimalSolver(**ctor).solve_transient(case.u0, case.t_end, enhance=enhance, **call)


def _checked_bands(case, sol, note):
    """sol.bands, after every array in it has been held against the oracle's assembly of the case (32 eps)."""
    err = nr.bands_error(case, sol.bands)
    note(f"transient-nl bands {case.name} device vs oracle assembly, scaled", err, nr.BANDS_BAR)
    print(f"{case.name}: bands device vs oracle {err:.2e}, bar {nr.BANDS_BAR:.2e}")
    assert err <= nr.BANDS_BAR
    return sol.bands


@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_loop_and_monitor_against_the_prototype(dev, note, name):
    """The nodal snapshots and the monitor table against the np.longdouble prototype on the device's own mass bands and
    loads (first held against the oracle's assembly), within 10x the float64 prototype's own distance from it."""
    case = nr.CASES[name]()
    sol = _solve(case)
    assert sol.nodal.shape == (len(case.snapshots), len(case.nodes))
    assert sol.newton.shape == (case.nsteps, case.newton_iters, 4)
    bands = _checked_bands(case, sol, note)
    err, bar, read = nr.loop_reading(name, sol.nodal, bands)
    merr, mbar, mread = nr.monitor_reading(name, sol.newton, bands)
    note(f"transient-nl loop {name} vs longdouble", err, bar)
    note(f"transient-nl monitor {name} vs longdouble", merr, mbar)
    print(f"{name}: device {err:.2e}, prototype {read:.2e}, bar {bar:.2e}; monitor {merr:.2e}, {mread:.2e}, {mbar:.2e}")
    assert err <= bar
    assert merr <= mbar


@pytest.mark.parametrize("scheme,lo,hi", [("bdf1", 0.8, 1.2), ("bdf2", 1.7, 2.3)])
def test_temporal_order(dev, scheme, lo, hi):
    """The cubic problem on 2048 elements, 8 / 16 / 32 steps to t = 1, against the spatially discrete limit (the
    prototype's 1024 BDF2 steps on the same mesh); the windows of the linear case (tests/test_transient_cpu.py).  Steps
    of 1/8 need more than the default three iterations to meet the increment test (the third increment of the first
    step reads 2.3e-7): six here."""
    u0, nl, forcing, _ = proto.cubic_manufactured()
    nodes = np.linspace(0.0, 1.0, 2049)
    ref = proto.solve(nodes, u0, 1.0, 1024, "bdf2", nl, forcing=forcing)["nodal"][-1]
    errs = []
    for nsteps in (8, 16, 32):
        sol = _solve(nr.cubic(2048, scheme, nsteps, 1.0, [nsteps], newton_iters=6))
        errs.append(float(np.max(np.abs(sol.nodal[-1] - ref))))
    orders = [math.log2(errs[i] / errs[i + 1]) for i in range(2)]
    print(f"{scheme}: errors {errs}, orders {orders}")
    assert all(lo <= o <= hi for o in orders)


def test_linear_limit(dev, note):
    """("poly", [0, q1]) with newton_iters=1 is the linear problem with the reaction c + q1: one Newton iteration solves
    it exactly, so the snapshots equal linear solve_transient's within the loop bar of the linear case.  The increment
    of the one iteration is the distance from the extrapolated start, not an error: newton_tol is set out of its way."""
    import hybrid_fem_lssvr_amd as pkg
    import transient_rules as tr
    q1 = lambda x: 0.7 + 0.2 * np.sin(2.0 * x)       # noqa: E731
    base = tr.general(40, (20, 40))
    ctor, call = base.facade()
    nl_sol = pkg.FEMLSSVRPrimalSolver(**ctor).solve_transient(
        base.u0, base.t_end, enhance=False, nonlinear=("poly", [nr._zero, q1]), newton_iters=1, newton_tol=1.0, **call)
    ctor["reaction"] = lambda x: base.c(x) + q1(x)
    lin_sol = pkg.FEMLSSVRPrimalSolver(**ctor).solve_transient(base.u0, base.t_end, enhance=False, **call)
    # the bar: 10x the float64 prototype's distance from its longdouble loop on the linear problem, twice (two loops)
    case = tr.Case("limit", base.nodes, base.u0, base.t_end, 40, "bdf2", a=base.a, da=base.da, c=ctor["reaction"],
                   rho=base.rho, forcing=base.forcing, kinds=base.kinds, kappa=base.kappa, end_data=base.end_data,
                   snapshots=[20, 40])
    read = float(np.max(np.abs(case.run()["nodal"] - case.run(np.longdouble)["nodal"]))) / case.scale
    bar = 2.0 * max(nr.MARGIN * read, nr.FLOOR)
    err = float(np.max(np.abs(nl_sol.nodal - lin_sol.nodal))) / case.scale
    note("transient-nl linear limit vs linear solve_transient", err, bar)
    print(f"linear limit: {err:.2e}, prototype {read:.2e}, bar {bar:.2e}")
    assert err <= bar


def test_stationary_solution_is_a_fixed_point(dev, note):
    """The stationary nonlinear= solution of solve_fem() (-u'' + u + u^3 = f, Robin left, Dirichlet right) started as
    u0 stays where it is for 5 steps: its discrete residual is the Newton tolerance of solve_fem, and a step maps a
    perturbation e of the stationary point to (M / dt + J)^{-1} (M / dt) e, a contraction; the bar is 10x the larger of
    solve_fem's stop test (1e-12 max(1, |u|)) and the loop's rounding (the FLOOR rule on 5 steps)."""
    import hybrid_fem_lssvr_amd as pkg
    nodes = nr.tr.general().nodes
    f = lambda x: np.cos(2.0 * x) + 0.5          # noqa: E731
    nl = ("poly", [nr._zero, nr._zero, nr._zero, nr._const(1.0)])
    common = dict(num_fem_nodes=len(nodes), lssvr_M=9, n_colloc=16, mesh=nodes, global_domain=(-1.0, 1.0),
                  rhs=f, reaction=nr._const(1.0), boundary=(("robin", 2.0, 0.3), ("dirichlet", 0.2)))
    u_st = pkg.FEMLSSVRPrimalSolver(nonlinear=nl, **common).solve_fem()[0]
    sol = pkg.FEMLSSVRPrimalSolver(**common).solve_transient(
        lambda x: np.interp(x, nodes, u_st), 0.5, nsteps=5, enhance=False, nonlinear=nl, snapshots=[1, 2, 3, 4, 5],
        end_data=(0.3, 0.2))
    scale = float(np.max(np.abs(u_st)))
    err = float(np.max(np.abs(sol.nodal - u_st[None, :]))) / scale
    bar = 10.0 * max(1e-12 * max(1.0, scale) / scale, 5 * nr.FLOOR)
    note("transient-nl fixed point drift", err, bar)
    print(f"fixed point: drift {err:.2e}, bar {bar:.2e}; first step's monitor {sol.newton[0, :, 0]}")
    assert err <= bar


def test_monitor_behaviour(dev):
    import hybrid_fem_lssvr_amd as pkg
    # quadratic convergence until the rounding floor, on the device's own table
    name = "cubic-bdf1-33"
    case = nr.CASES[name]()
    sol = _solve(case)
    assert sol.newton.shape == (case.nsteps, 3, 4) and not np.any(sol.newton[:, :, 3])
    r = sol.newton[:, :, 0]
    floor = 1e3 * nr.EPS * nr.monitor_terms(case, nr.references(name)[1])
    print("monitor, step 1:", r[0], "floor", floor)
    assert np.all((r[:, 1:] <= 10.0 * r[:, :-1] ** 2) | (r[:, 1:] <= floor))
    assert np.all(r[:, 0] > 1e3 * floor)                        # (the first residual of a step is not at the floor)
    # one iteration on the stiff cubic with a large step does not meet the increment test
    s = pkg.FEMLSSVRPrimalSolver(33, lssvr_M=9, n_colloc=16, global_domain=(0.0, 1.0))
    stiff = ("poly", [nr._zero, nr._zero, nr._zero, nr._const(1000.0)])
    with pytest.raises(RuntimeError, match=r"step 1 did not converge in 1 Newton iteration"):
        s.solve_transient(lambda x: np.sin(math.pi * x), 2.0, nsteps=2, forcing=[(0.0, nr._zero)], end_data=(0.0, 0.0),
                          enhance=False, nonlinear=stiff, newton_iters=1)


@pytest.mark.parametrize("M,n", [(9, 16), (20, 24)])
def test_enhanced_snapshots_against_the_oracle_rows(dev, note, M, n):
    """W of the snapshots (M = 9: the lane kernel of the reaction rows; M = 20: the wave kernel) against the oracle's
    reaction rows fed the restated c_eff and f_eff on the longdouble loop's data, rel-L2 under the family's 1e-11."""
    name = "general-poly-33"
    case = nr.CASES[name]()
    sol = _solve(case, enhance=True, M=M, n_colloc=n)
    Wref, bar, noise = nr.enhanced_reference(name, M, n, _checked_bands(case, sol, note))
    assert len(sol.enhanced) == len(case.snapshots)
    worst = 0.0
    for k, e in enumerate(sol.enhanced):
        assert e.n_fallback == 0
        worst = max(worst, float(nr.orc.rel_l2_coef(e.W.cpu().numpy(), Wref[k]).max()))
    note(f"transient-nl enhanced M={M} vs oracle rows", worst, nr.ENH_FAMILY_BAR)
    print(f"M={M}: device {worst:.2e}, prototype noise {noise:.2e}, bar {nr.ENH_FAMILY_BAR:.2e}")
    assert worst <= nr.ENH_FAMILY_BAR
    g_right = case.end_data[1](sol.times[-1])
    assert abs(float(sol.evaluate(len(sol.enhanced) - 1, np.array([1.0]))[0]) - g_right) <= 1e-9
