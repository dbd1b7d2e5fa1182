"""CPU: transient problems where there is no GPU -- the numpy prototype with the library's host
mirror of the step's right-hand side in its loop against closed forms and invariants, the two host mirrors against a
plain numpy restatement bit for bit, the argument errors of the new entries and the facade's refusals."""
import math

import numpy as np
import pytest

import transient_rules as tr

proto = tr.proto


@pytest.mark.parametrize("scheme", ["bdf1", "bdf2"])
@pytest.mark.parametrize("ne", tr.DECAY_NE)
def test_discrete_mode_decay(ne, scheme):
    """The nodal vector after n steps is s_n u0, s_n the scalar recurrence of the discrete mode; the error is measured
    against |u0|_inf and the bar is 10x the prototype's own reading (tr.DECAY_READ records both)."""
    case = tr.decay(ne, scheme)
    r = case.run(rhs_fn=tr.step_rhs_host)
    err, bar = tr.decay_error(case, ne, r["nodal"]), tr.decay_bar(ne, scheme)
    print(f"decay {scheme} ne={ne}: host mirrors {err:.2e}, prototype {bar / tr.MARGIN:.2e}, bar {bar:.2e}")
    assert err <= bar
    assert bar <= tr.MARGIN * 1.5e-14          # the prototype itself stays where it was measured


@pytest.mark.parametrize("scheme,lo,hi", [("bdf1", 0.8, 1.2), ("bdf2", 1.7, 2.3)])
def test_temporal_order(scheme, lo, hi):
    """u0 = cos(pi x / 2), exact exp(-pi^2 t / 4) cos(pi x / 2), T = 0.4 on 2048 elements: the observed orders between
    8, 16 and 32 steps (prototype: 0.96, 0.98 for BDF1 and 2.10, 2.04 for BDF2)."""
    nodes = np.linspace(-1.0, 1.0, 2049)
    exact = math.exp(-math.pi ** 2 * 0.4 / 4.0) * np.cos(0.5 * math.pi * nodes)
    errs = []
    for nsteps in (8, 16, 32):
        r = proto.solve(nodes, lambda x: np.cos(0.5 * math.pi * x), 0.4, nsteps, scheme, rhs_fn=tr.step_rhs_host)
        errs.append(float(np.max(np.abs(r["nodal"][-1] - exact))))
    orders = [math.log2(errs[i] / errs[i + 1]) for i in range(2)]
    print(f"{scheme}: errors {errs}, orders {orders}")
    assert all(lo <= o <= hi for o in orders)


def test_conservation_with_two_neumann_ends():
    """c = f = g = 0, two Neumann ends, non-uniform mesh, variable rho: sum_i (M u^n)_i stays what it was."""
    case = tr.neumann()
    r = case.run(rhs_fn=tr.step_rhs_host)
    drift, bar = tr.mass_drift(case, r["nodal"]), tr.mass_bar()
    print(f"mass drift {drift:.2e}, prototype {bar / tr.MARGIN:.2e}, bar {bar:.2e}")
    assert drift <= bar
    # and the solution does move: this is no test of a frozen vector
    assert np.max(np.abs(r["nodal"][-1] - case.u0(case.nodes))) > 0.1


def test_stationary_solution_is_a_fixed_point():
    """Start at the stationary P1 solution of a Robin / Dirichlet reaction problem with static data: five steps leave it
    where it is, within 10x what the prototype's own loop reads (floor 4 eps)."""
    g = tr.general()
    kinds, kappa, gl, gr = g.kinds, g.kappa, 0.3, -0.2
    f = lambda x: np.sin(math.pi * x) + x * x      # noqa: E731
    kd, ko, load, _ = tr.orc.p1_bands(g.nodes, f, g.a, 2, g.c)
    ustat = proto.bc_solve(kd, ko, load, kinds, kappa, (gl, gr))
    kw = dict(a=g.a, c=g.c, rho=g.rho, forcing=[(1.0, f)], kinds=kinds, kappa=kappa, end_data=(gl, gr), every=True)
    for scheme in ("bdf1", "bdf2"):
        ref = proto.solve(g.nodes, lambda x: ustat, 0.05, 5, scheme, **kw)
        r = proto.solve(g.nodes, lambda x: ustat, 0.05, 5, scheme, rhs_fn=tr.step_rhs_host, **kw)
        scale = float(np.max(np.abs(ustat)))
        read = float(np.max(np.abs(ref["nodal"] - ustat[None, :]))) / scale
        err = float(np.max(np.abs(r["nodal"] - ustat[None, :]))) / scale
        print(f"fixed point {scheme}: host mirrors {err:.2e}, prototype {read:.2e}")
        assert err <= max(tr.MARGIN * read, tr.FLOOR)
        assert read <= 1e-13


@pytest.mark.parametrize("ne", [1, 2, 3, 64, 257])
@pytest.mark.parametrize("nc,R", [(1, 1), (3, 8), (1, 8), (3, 1)])
def test_rhs_host_is_the_numpy_restatement(ne, nc, R):
    d = tr.kernel_inputs(ne, nc, R, 2)
    for b0, b1, U1 in ((1.0, 0.0, None), (2.0, -0.5, d["U1"]), (1.0, 0.0, d["U1"])):
        got = tr.rhs_host(d["md"], d["mo"], d["U0"], U1, d["loads"], d["phi"], b0, b1, 37.0)[1]
        want = tr.rhs_numpy(d["md"], d["mo"], d["U0"], U1, d["loads"], d["phi"], b0, b1, 37.0)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("ne,n", [(1, 2), (2, 16), (3, 5), (64, 16), (257, 2)])
@pytest.mark.parametrize("R", [1, 8])
def test_source_table_host_is_the_numpy_restatement(ne, n, R, pm):
    d = tr.kernel_inputs(ne, 1, R, n)
    ftab = np.ascontiguousarray(np.transpose(d["ftab"], (0, 2, 1))) if pm else d["ftab"]
    rtab = np.ascontiguousarray(d["rho_tab"].T) if pm else d["rho_tab"]
    for al, b0, b1, U1 in ((1.0, 1.0, 0.0, None), (1.5, 2.0, -0.5, d["U1"][0])):
        got = tr.source_host(d["U2"], d["U0"][0], U1, ftab, rtab, d["phi"][0], al, b0, b1, 100.0, pm)[1]
        want = tr.source_numpy(d["U2"], d["U0"][0], U1, ftab, rtab, d["phi"][0], al, b0, b1, 100.0, pm)
        assert got.shape == rtab.shape and np.array_equal(got, want)


def test_argument_errors():
    """Each broken argument of the two entry pairs is refused with its code, on the host (the device entries validate
    before they launch, so they can be called here with host addresses standing in)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    d = tr.kernel_inputs(4, 2, 2, 3)
    ok = dict(md=d["md"], mo=d["mo"], U0=d["U0"], U1=d["U1"], loads=d["loads"], phi=d["phi"], beta0=2.0, beta1=-0.5,
              inv_dt=10.0)
    assert tr.rhs_host(**ok, check=False)[0] == 0
    z = np.zeros((0, 5))
    for change, code in ((dict(U1=None), -1), (dict(beta0=math.inf), -2), (dict(inv_dt=math.nan), -2),
                         (dict(U0=z, U1=z, phi=np.zeros((0, 2))), -2), (dict(loads=np.zeros((9, 5))), -2),
                         (dict(loads=np.zeros((0, 5))), -2), (dict(U0=np.zeros((9, 5)), U1=np.zeros((9, 5))), -2)):
        assert tr.rhs_host(**{**ok, **change}, check=False)[0] == code, change
    p = tr._hp
    args = [p(d["md"]), p(d["mo"]), p(d["U0"]), p(d["U1"]), p(d["loads"]), p(d["phi"])]
    out = np.zeros((2, 5))
    assert lib.lssvr_ts_rhs_host(*args, 0, 2, 2, 1.0, 0.0, 1.0, p(out)) == -2           # ne < 1
    assert lib.lssvr_ts_rhs_host(*args, 4, 2, 2, 1.0, 0.0, 1.0, None) == -1             # out NULL
    assert lib.lssvr_ts_rhs_host(*args, 4, 2, 2, 1.0, 0.0, 1.0, p(d["U0"])) == -2       # out is U0
    assert b"U0" in lib.lssvr_last_error()
    addr = [a.ctypes.data for a in (d["md"], d["mo"], d["U0"], d["U1"], d["loads"], d["phi"])]
    assert lib.lssvr_ts_rhs(*addr, 4, 0, 2, 1.0, 0.0, 1.0, out.ctypes.data, None) == -2          # nc < 1, no launch
    assert lib.lssvr_ts_rhs(*addr, 4, 2, 2, 1.0, 0.0, 1.0, None, None) == -1
    so = dict(U2=d["U2"], U0=d["U0"][0], U1=d["U1"][0], ftab=d["ftab"], rho_tab=d["rho_tab"], phi=d["phi"][0],
              alpha=1.5, beta0=2.0, beta1=-0.5, inv_dt=10.0, pm=False)
    assert tr.source_host(**so, check=False)[0] == 0
    for change, code in ((dict(U1=None), -1), (dict(alpha=math.inf), -2), (dict(pm=7), -2),
                         (dict(ftab=np.zeros((9, 4, 3))), -2), (dict(rho_tab=np.ones((4, 1)), ftab=np.ones((2, 4, 1))), -2)):
        assert tr.source_host(**{**so, **change}, check=False)[0] == code, change
    sa = [d["U2"].ctypes.data, d["U0"].ctypes.data, d["U1"].ctypes.data, d["ftab"].ctypes.data,
          d["rho_tab"].ctypes.data, d["phi"].ctypes.data]
    assert lib.lssvr_ts_source_table(*sa, 4, 3, 0, 0, 1.0, 1.0, 0.0, 1.0, out.ctypes.data, None) == -2      # R < 1
    assert lib.lssvr_ts_source_table(*sa, 4, 3, 2, 0, 1.0, 1.0, 0.0, 1.0, None, None) == -1


def test_ops_wrappers_reject_host_tensors():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.ts_rhs(t, t[:4], t[None, :], None, t[None, :], torch.zeros((1, 1), dtype=torch.float64), 1.0, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.ts_source_table(t, t, None, torch.zeros((1, 4, 2), dtype=torch.float64),
                            torch.zeros((4, 2), dtype=torch.float64), t[:1], 1.0, 1.0, 0.0, 1.0)


def test_facade_refusals(monkeypatch):
    tr.check_refusals(monkeypatch, tr.call_transient, tr.refusals(), tr.passing())


def test_accuracy_record_of_the_prototype():
    """The manufactured solution on 8, 16, 32 elements: the recorded figures, and the enhanced snapshot is closer to u
    than the P1 interpolant."""
    for ne, e_p1, e_enh in proto.accuracy_record():
        want = tr.ACCURACY[ne]
        assert abs(e_p1 - want[0]) <= 5e-4 * want[0] and abs(e_enh - want[1]) <= 5e-4 * want[1]
        assert e_enh < e_p1
