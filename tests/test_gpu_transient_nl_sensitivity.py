"""GPU: adjoint sensitivities of the semilinear BDF loop -- the two device kernels against their
host mirrors, the grid-stride seam, the facade against the prototype's complex step through the whole loop, its value
against solve_transient, the linear limit, the step that does not converge and the inverse problem."""
import numpy as np
import pytest
import torch

import transient_nl_sensitivity_rules as ns

pytestmark = pytest.mark.gpu
proto, tr, tsp, sp = ns.proto, ns.tr, ns.tsp, ns.sp
D, R, POLY, EXP = ns.D, ns.R, ns.POLY, ns.EXP
EPS = 2.0 ** -52
# table sizes 1, 2, 63, 64, 65 and 514 entries
SIZES = [(1, 1), (1, 2), (63, 1), (64, 1), (32, 2), (65, 1), (13, 5), (257, 2)]


def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _chunk_device(dev, d, nq, kind, nterm, want, kinds=(D, D), ends=False, init=None):
    """ops.ts_nl_sensitivity into canary-filled (or ``init``-filled) buffers -> the dict of ns.nl_sens_host."""
    from hybrid_fem_lssvr_amd import ops
    t = {k: _t(d[k], dev) for k in ("x", "Utraj", "Z", "Brows", "phi", "band_ends", "q")}
    full = {k: _t(v, dev) for k, v in ns.blank(d, nq, nterm, init).items()}
    out = {k: full[k] for k in want}
    if ends:
        out.update(g=full["g"], kappa=full["kappa"])
    res = ops.ts_nl_sensitivity(t["x"], t["Utraj"], t["Z"], d["n0"], d["coef"], d["inv_dt"], nq, kind, nterm,
                                q_tabs=t["q"], want=want, phi=t["phi"] if "f" in want else None,
                                Brows=t["Brows"] if ends else None, band_ends=t["band_ends"] if ends else None,
                                end_kinds=kinds, accumulate=init is not None, out=out)
    assert set(res) == set(out) and all(res[k] is out[k] for k in out)
    return {k: v.cpu().numpy() for k, v in full.items()}


@pytest.mark.parametrize("kind,nterm", [(POLY, 1), (POLY, 4), (POLY, 6), (EXP, 2)])
@pytest.mark.parametrize("m", [1, 8])
@pytest.mark.parametrize("ne,nq", SIZES)
def test_chunk_device_is_the_host_mirror(dev, ne, nq, m, kind, nterm):
    """POLY: every output bit for bit; EXP: gq within the per-entry bar of section 35 summed over the levels (the device
    library's exp against libm's), everything else bit for bit.  accumulate 0, and then 1 onto the result."""
    d = ns.kernel_inputs(ne, nq, m, 2, nterm, 1 + (ne + m) % 3)
    if kind == EXP:
        d["q"] *= 0.5
    kinds = ((D, D), (R, D), (D, R), (R, R))[(ne + nq + m) % 4]
    qbar = ns.exp_bar(d, nq) if kind == EXP else None
    ref = ns.nl_sens_host(d, nq, kind, nterm, ns.TABLES, kinds, ends=True)[1]
    got = _chunk_device(dev, d, nq, kind, nterm, ns.TABLES, kinds, ends=True)
    ns.check_against(got, ns.TABLES, ref, True, kind=kind, qbar=qbar)
    init = {k: got[k] for k in (*ns.TABLES, "kappa")}
    ref1 = ns.nl_sens_host(d, nq, kind, nterm, ns.TABLES, kinds, ends=True, init=init)[1]
    got1 = _chunk_device(dev, d, nq, kind, nterm, ns.TABLES, kinds, ends=True, init=init)
    ns.check_against(got1, ns.TABLES, ref1, True, init, kind=kind, qbar=qbar)
    want = (("q",), ("a", "q"), ("c", "rho"), ())[(ne + m) % 4]          # what is not asked for keeps its canaries
    ns.check_against(_chunk_device(dev, d, nq, kind, nterm, want, kinds, ends=True), want, ref, True, kind=kind,
                     qbar=qbar)


def _step_device(dev, d, b0, b1, with_a=True):
    from hybrid_fem_lssvr_amd import ops
    t = {k: _t(d[k], dev) for k in ("x", "u", "a", "cs", "q", "mdiag", "moff", "U0", "U1", "loads", "phi")}
    out = {k: _t(v, dev) for k, v in ns.step_blank(d["ne"]).items()}
    res = ops.ts_nl_adjoint_step(t["x"], t["u"], t["cs"], d["kind"], t["q"], t["mdiag"], t["moff"], t["U0"],
                                 None if b1 == 0.0 else t["U1"], t["loads"], t["phi"], b0, b1, d["inv_dt"],
                                 a_quad=t["a"] if with_a else None, out=out)
    assert all(res[k] is out[k] for k in out)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _exp_band_bars(d):
    """Per-entry bars (diag [ne+1], off [ne]) of the bands for EXP.  g_u = (q_0 q_1) E enters an element's three mass
    sums with the weights h w phi_i phi_j <= h w; the two exp implementations differ by an ulp or so of E, whose argument
    q_1 u_h is itself rounded: 8 eps h w |g_u| (1 + |q_1 u_h|) per point as in section 35, summed over the points of the
    one (off) or two (diag) elements of the entry; plus 4 eps of the entry itself for sums that round differently once
    their terms differ."""
    xi, w = sp.gauss01(d["nq"])
    uh = d["u"][:-1, None] + np.diff(d["u"])[:, None] * xi[None, :]
    arg = d["q"][1] * uh
    s = 8.0 * EPS * (np.diff(d["x"])[:, None] * w[None, :] * np.abs(d["q"][0] * d["q"][1] * np.exp(arg))
                     * (1.0 + np.abs(arg))).sum(axis=1)
    both = np.zeros(d["ne"] + 1)
    both[:-1] += s
    both[1:] += s
    return both, s


@pytest.mark.parametrize("kind,nterm", [(POLY, 1), (POLY, 4), (POLY, 6), (EXP, 2)])
@pytest.mark.parametrize("ne,nq", SIZES)
def test_step_device_is_the_host_mirror(dev, ne, nq, kind, nterm):
    """POLY: the bands, B and the band_ends row bit for bit; EXP: B bit for bit, the bands within their bar and the
    band_ends row the device's own {off[0], off[ne-1]}."""
    for nR, (b0, b1), with_a in ((1, (2.0, -0.5), True), (3, (1.0, 0.0), False)):
        d = ns.step_inputs(ne, nq, kind, nterm, nR)
        ref, got = ns.step_host(d, b0, b1, with_a), _step_device(dev, d, b0, b1, with_a)
        assert np.array_equal(got["B"], ref["B"])
        assert got["band_ends"][0] == got["off"][0] and got["band_ends"][1] == got["off"][ne - 1]
        if kind == POLY:
            for k in ("diag", "off", "band_ends"):
                assert np.array_equal(got[k], ref[k]), k
        else:
            bd, bo = _exp_band_bars(d)
            assert np.all(np.abs(got["diag"] - ref["diag"]) <= bd + 4.0 * EPS * np.abs(ref["diag"]))
            assert np.all(np.abs(got["off"] - ref["off"]) <= bo + 4.0 * EPS * np.abs(ref["off"]))


def test_chunk_device_past_one_grid_pass(dev):
    """131073 elements, nquad 2, m = 2: two table entries past 1024 x 256 threads, so the grid-stride loop takes a second
    pass for them.  Bit-equal to the host mirror, and the elements around the seam (and the first) against the numpy
    formulas, so that a stride error that hits mirror and device alike cannot hide."""
    ne, nq, m, nterm = 131073, 2, 2, 4
    assert ne * nq == 1024 * 256 + 2
    d = ns.kernel_inputs(ne, nq, m, 2, nterm, 2)
    ref = ns.nl_sens_host(d, nq, POLY, nterm, ns.TABLES, (R, D), ends=True)[1]
    got = _chunk_device(dev, d, nq, POLY, nterm, ns.TABLES, (R, D), ends=True)
    ns.check_against(got, ns.TABLES, ref, True)
    for e in (0, 1, ne - 5, ne - 4, ne - 3, ne - 2, ne - 1):          # one element at a time: a mesh of one element each
        one = dict(d, x=d["x"][e:e + 2], Utraj=d["Utraj"][:, e:e + 2], Z=d["Z"][:, e:e + 2], Brows=d["Brows"][:, e:e + 2],
                   q=d["q"][:, e:e + 1], ne=1)
        num = ns.nl_sens_numpy(one, nq, POLY, nterm)
        for k in ns.TABLES:
            assert np.array_equal(got[k][..., e, :], num[k][..., 0, :]), (k, e)


def _facade_value(c, sol_nodal, steps):
    """J of the case on the snapshots ``sol_nodal`` at ``steps``, by the facade's own formulas."""
    U = np.zeros((c.N + 1, c.ne + 1))
    U[steps] = sol_nodal
    return float(c.J.value(c.p.x, U))


@pytest.mark.parametrize("c", ns.facade_cases(), ids=lambda c: c.id)
def test_facade_against_complex_step(dev, note, c):
    """solve_transient_sensitivity(..., nonlinear=...) with 6 Newton iterations per step within 10x the prototype's
    reading of the same case on every group; ``value`` is J of solve_transient's trajectory."""
    kw = ns.facade_functional(c)
    r = ns.facade_solver(c).solve_transient_sensitivity(tsp.u_init, tsp.T_END, **ns.facade_args(c), **kw)
    by_group = proto.deviations(ns.facade_gradients(r), c.reference[2])
    devn = max(by_group.values())
    print(f"{c.id}: device {devn:.2e}, prototype {c.read:.2e}, bar {c.bar:.2e}, last increment "
          f"{r.newton[:, -1, 1].max():.1e}; " + " ".join(f"{k} {v:.1e}" for k, v in by_group.items()))
    note("deviation from the complex step", devn, c.bar)
    note("prototype reading", c.read)
    assert devn <= c.bar
    assert r.d_nonlinear.shape == (len(c.p.q), c.ne, c.nq) and r.newton.shape == (c.N, ns.NEWTON_ITERS, 4)
    steps = sorted(kw["goal_steps"] if c.kind == "goal" else kw["observe"][0])
    sol = ns.facade_solver(c).solve_transient(tsp.u_init, tsp.T_END, snapshots=steps, enhance=False,
                                              **ns.facade_args(c))
    J = _facade_value(c, sol.nodal, steps)
    print(f"value {r.value!r}, J of solve_transient {J!r}")
    assert abs(r.value - J) <= 64.0 * EPS * max(1.0, abs(J))
    assert np.array_equal(r.times, c.p.dt * np.arange(c.N + 1)) and np.array_equal(r.nodes, c.p.x)


def test_linear_limit(dev, note):
    """nonlinear=("poly", [0, c0]) with the default forcing against the linear method with the reaction c + c0: within
    the bar of the linear-law case on the same mesh and steps; dJ/dq_1 is dJ/dc and dJ/dq_0 is -dJ/df_0, bit for bit."""
    c = ns.case("linear", 33, 2, (D, R), "bdf2", 11, "goal")
    c0 = proto.LAWS["linear"][1][1]
    kw = dict(ns.facade_args(c, nonlinear=False), forcing=None, **ns.facade_functional(c))
    r = ns.facade_solver(c).solve_transient_sensitivity(tsp.u_init, tsp.T_END, nonlinear=ns.law_spec("linear"),
                                                        newton_iters=ns.NEWTON_ITERS, **kw)
    lin = ns.facade_solver(c, reaction=lambda x: sp.reaction(x) + c0(x)).solve_transient_sensitivity(
        tsp.u_init, tsp.T_END, **kw)
    assert lin.d_nonlinear is None and lin.newton is None
    devn = max(proto.deviations(ns.facade_gradients(r, nonlinear=False), ns.facade_gradients(lin, False)).values())
    print(f"linear limit: {devn:.2e}, bar {c.bar:.2e}")
    note("linear limit: deviation from the linear method", devn, c.bar)
    assert devn <= c.bar
    assert abs(r.value - lin.value) <= c.bar * max(1.0, abs(lin.value))
    assert np.array_equal(r.d_nonlinear[1], r.d_reaction)
    assert np.array_equal(r.d_nonlinear[0], -r.d_forcing[0])


def test_a_step_that_does_not_converge(dev, monkeypatch):
    """newton_iters = 1 on the cubic with a long step: RuntimeError naming the step, and nothing of the backward sweep
    has been launched (the prototype shows the increment 1e10 x above tolerance)."""
    from hybrid_fem_lssvr_amd import ops
    S = proto.SLOW
    c = ns.case(S["law"], S["ne"], S["nq"], S["kinds"], S["scheme"], S["N"])
    launched = []
    for nm in ("ts_nl_adjoint_step", "ts_nl_sensitivity"):
        monkeypatch.setattr(ops, nm, lambda *a, _nm=nm, **k: launched.append(_nm))
    kw = dict(ns.facade_args(c), newton_iters=S["iters"], newton_tol=S["tol"])
    with pytest.raises(RuntimeError, match=r"solve_transient_sensitivity: step 1 did not converge in 1 Newton iteration"):
        ns.facade_solver(c).solve_transient_sensitivity(tsp.u_init, S["t_end"], goal=sp.goal_density, **kw)
    assert launched == []


def test_inverse_problem(dev, note):
    """A piecewise-constant q_3 of u_t - u'' + q_3 u^3 = f on 16 elements, 8 steps, from observations at two steps: 20
    steps of gradient descent on log q_3 with the facade's dJ/dq_3 -- the misfit falls monotonically and ends within 1e-6
    relative of the prototype's final value."""
    import hybrid_fem_lssvr_amd as pkg
    nlp = proto.nlp
    x = np.linspace(-1.0, 1.0, proto.DEMO_NE + 1)

    def gradient(q3, xo, d):
        def q3_of(pts):
            return q3[np.clip(np.searchsorted(x, pts, side="right") - 1, 0, proto.DEMO_NE - 1)]
        s = pkg.FEMLSSVRPrimalSolver(mesh=x, nquad=2, boundary=(("dirichlet", 0.0), ("dirichlet", 0.0)), lssvr_M=9,
                                     n_colloc=16)
        r = s.solve_transient_sensitivity(proto.demo_u0, proto.DEMO_T, nsteps=proto.DEMO_N,
                                          forcing=[(1.0, nlp.demo_rhs)], end_data=(0.0, 0.0),
                                          observe=(list(proto.DEMO_OBS), xo, d),
                                          nonlinear=("poly", [nlp.zero, nlp.zero, nlp.zero, q3_of]),
                                          newton_iters=proto.DEMO_NEWTON)
        return r.value, r.d_nonlinear[3]
    hist = proto.demo(gradient)
    print("device misfits: " + " ".join(f"{v:.6e}" for v in hist))
    note("inverse problem: final misfit", hist[-1], ns.DEMO_FINAL)
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] - ns.DEMO_FINAL) <= ns.DEMO_RTOL * ns.DEMO_FINAL
