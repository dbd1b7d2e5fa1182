"""GPU: adjoint sensitivities of the BDF loop -- the device kernel against the host mirror bit for
bit, the facade against the complex step, its forward loop against solve_transient, the inverse problem and the
sequence of calls of the backward sweep."""
import functools
import types

import numpy as np
import pytest
import torch

import transient_sensitivity_rules as tr

pytestmark = pytest.mark.gpu
proto = tr.proto
D, R = tr.D, tr.R


def _device(dev, d, nq, want, kinds=(D, D), ends=False, init=None):
    """ops.ts_sensitivity into canary-filled (or ``init``-filled) buffers -> the dict of tr.ts_sens_host."""
    from hybrid_fem_lssvr_amd import ops
    t = {k: torch.as_tensor(np.ascontiguousarray(d[k]), device=dev) for k in ("x", "Utraj", "Z", "Brows", "phi", "band_ends")}
    full = {k: torch.as_tensor(v, device=dev) for k, v in tr.blank(d, nq, init).items()}
    out = {k: full[k] for k in want}
    if ends:
        out.update(g=full["g"], kappa=full["kappa"])
    res = ops.ts_sensitivity(t["x"], t["Utraj"], t["Z"], d["n0"], d["coef"], d["inv_dt"], nq, want=want,
                             phi=t["phi"] if "f" in want else None, Brows=t["Brows"] if ends else None,
                             band_ends=t["band_ends"] if ends else None, band_rows=d["band_rows"], end_kinds=kinds,
                             accumulate=init is not None, out=out)
    assert set(res) == set(out) and all(res[k] is out[k] for k in out)
    return {k: v.cpu().numpy() for k, v in full.items()}


@pytest.mark.parametrize("m,nR", [(1, 0), (3, 1), (8, 2), (8, 8)])
@pytest.mark.parametrize("ne", [1, 2, 255, 256, 257])
def test_device_is_the_host_mirror(dev, ne, m, nR):
    """Every output bit for bit, accumulate 0 and 1, the NULL-output combinations with their canaries untouched."""
    tabs = tr.TABLES if nR else tr.TABLES[:3]
    for n0 in (1, 3):
        d = tr.kernel_inputs(ne, m, nR, n0)
        for nq in (1, 2, 3, 4, 5):
            kinds = ((D, D), (R, D), (D, R), (R, R))[(nq + n0) % 4]
            ref = tr.ts_sens_host(d, nq, tabs, kinds, ends=True)[1]
            tr.check_against(_device(dev, d, nq, tabs, kinds, ends=True), tabs, ref, True)
            init = tr.initial(d, nq)
            ref1 = tr.ts_sens_host(d, nq, tabs, kinds, ends=True, init=init)[1]
            tr.check_against(_device(dev, d, nq, tabs, kinds, ends=True, init=init), tabs, ref1, True, init)
        nq = 1 + (ne + m) % 5
        init = tr.initial(d, nq)
        ref0 = tr.ts_sens_host(d, nq, tabs, (R, D), ends=True)[1]
        ref1 = tr.ts_sens_host(d, nq, tabs, (R, D), ends=True, init=init)[1]
        for want in tr.wants(nR):
            if want:
                tr.check_against(_device(dev, d, nq, want), want, ref0, False)
            tr.check_against(_device(dev, d, nq, want, (R, D), ends=True, init=init), want, ref1, True, init)


def test_device_past_one_grid_pass(dev):
    """300000 elements, nquad 2, m = 8, R = 2: more table entries than 1024 x 256 threads, so the grid-stride loop takes
    a second pass.  Bit-equal to the host mirror, and a few hundred entries against the numpy formulas, so that a
    stride error that hits mirror and device alike cannot hide."""
    ne, nq, m, nR = 300000, 2, 8, 2
    d = tr.kernel_inputs(ne, m, nR, 2)
    assert ne * nq > 1024 * 256
    ref = tr.ts_sens_host(d, nq, tr.TABLES, (R, D), ends=True)[1]
    got = _device(dev, d, nq, tr.TABLES, (R, D), ends=True)
    tr.check_against(got, tr.TABLES, ref, True)
    rng = np.random.default_rng(7)
    pick = np.unique(np.concatenate([[0, 1, ne - 2, ne - 1, 1024 * 256 // nq - 1, 1024 * 256 // nq, 1024 * 256 // nq + 1],
                                     rng.integers(0, ne, 300)]))
    for e in pick:          # one element at a time: a mesh of one element each
        one = proto.chunk_tables(d["x"][e:e + 2], nq, d["Utraj"][:, e:e + 2], d["Z"][:, e:e + 2], d["n0"], d["inv_dt"],
                                 d["coef"], d["phi"], nR)
        for k in tr.TABLES:
            assert np.array_equal(got[k][..., e, :], one[k][..., 0, :]), (k, e)


@pytest.mark.parametrize("c", tr.facade_cases(), ids=lambda c: c.id)
def test_facade_against_complex_step(dev, note, c, monkeypatch):
    """solve_transient_sensitivity within the bar of the complex step on every group; its forward loop is
    solve_transient's bit for bit, and ``value`` is J of that trajectory."""
    from hybrid_fem_lssvr_amd import ops
    states = []
    solve = ops.tridiag_bc_solve_multi

    @functools.wraps(solve)
    def spy(*a, **k):
        states.append(k["out"])
        return solve(*a, **k)
    monkeypatch.setattr(ops, "tridiag_bc_solve_multi", spy)
    r = tr.facade_solver(c).solve_transient_sensitivity(proto.u_init, proto.T_END, **tr.facade_args(c),
                                                        **tr.facade_functional(c))
    monkeypatch.undo()
    assert len(states) == 2 * c.N
    got = tr.facade_gradients(r)
    by_group = proto.deviations(got, c.reference[2])
    devn = max(by_group.values())
    print(f"{c.id}: device {devn:.2e}, prototype {c.read:.2e}, bar {c.bar:.2e}; "
          + " ".join(f"{k} {v:.1e}" for k, v in by_group.items()))
    note("deviation from the complex step", devn, c.bar)
    assert devn <= c.bar
    assert c.read <= tr.READ_SLACK * tr.READ[c.ne]
    traj = torch.cat(states[:c.N]).cpu().numpy()
    sol = tr.facade_solver(c).solve_transient(proto.u_init, proto.T_END, snapshots=range(1, c.N + 1), enhance=False,
                                              **tr.facade_args(c))
    assert np.array_equal(traj, sol.nodal)
    U = np.concatenate([np.zeros((1, c.ne + 1)), sol.nodal])          # (no functional here looks at u^0)
    assert abs(r.value - c.J.value(c.p.x, U)) <= 1e-13 * max(1.0, abs(r.value))
    assert np.array_equal(r.times, c.p.dt * np.arange(c.N + 1)) and np.array_equal(r.nodes, c.p.x)


def test_inverse_problem(dev, note):
    """The initial state of u_t = u'' from two snapshots: 20 steps of gradient descent with the facade's dJ/du0 end at
    the prototype's misfit within 1.5x."""
    import hybrid_fem_lssvr_amd as pkg

    def gradient(u0, x, d):
        s = pkg.FEMLSSVRPrimalSolver(mesh=x, nquad=2, boundary=(("dirichlet", 0.0), ("dirichlet", 0.0)), lssvr_M=9,
                                     n_colloc=16)
        r = s.solve_transient_sensitivity(lambda t: np.interp(t, x, u0), proto.DEMO_T, nsteps=proto.DEMO_N,
                                          forcing=[(1.0, lambda t: 0.0 * t)], end_data=(0.0, 0.0),
                                          observe=(list(proto.DEMO_OBS), x, d))
        return r.value, r.d_u0
    hist = proto.demo(gradient)
    ref = proto.demo()
    print(f"device {hist[-1]:.6e}, prototype {ref[-1]:.6e}")
    note("inverse problem: final misfit", hist[-1], tr.DEMO_WITHIN * ref[-1])
    assert abs(ref[-1] - tr.DEMO_FINAL) <= 1e-6 * tr.DEMO_FINAL
    assert ref[-1] / tr.DEMO_WITHIN <= hist[-1] <= tr.DEMO_WITHIN * ref[-1]
    assert all(b < a for a, b in zip(hist, hist[1:]))


CPU = "Tensor.cpu"


def test_call_sequence_of_the_backward_sweep(dev, monkeypatch):
    """N = 9: after the 9 forward steps the sweep issues exactly 9 x (ts_rhs, tridiag_bc_solve_multi) with ONE
    ts_sensitivity after the 8th and one after the 9th (chunks of 8 and 1), the final ts_rhs for B_0, and one
    device-to-host copy."""
    from hybrid_fem_lssvr_amd import ops
    c = tr.case(33, 2, (D, R), "bdf2", 9, "goal")
    calls = []

    def logged(label, fn):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            calls.append(label)
            return fn(*a, **k)
        return wrapper
    for nm, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not nm.startswith("_") and fn.__module__ == ops.__name__:
            monkeypatch.setattr(ops, nm, logged(nm, fn))
    monkeypatch.setattr(torch.Tensor, "cpu", logged(CPU, torch.Tensor.cpu))
    tr.facade_solver(c).solve_transient_sensitivity(proto.u_init, proto.T_END, **tr.facade_args(c), goal=tr.sp.goal_density)
    monkeypatch.undo()
    print(calls)
    step = ["ts_rhs", "tridiag_bc_solve_multi"]
    setup = ["p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work"]
    assert calls == setup + 9 * step + 8 * step + ["ts_sensitivity"] + step + ["ts_sensitivity", "ts_rhs", CPU]
