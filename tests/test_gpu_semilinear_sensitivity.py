"""GPU: adjoint sensitivities of the semilinear P1 solve -- the device kernel against the host
mirror, the facade against the prototype's complex step, the linear limit against solve_sensitivity, and the inverse
problem."""
import numpy as np
import pytest
import torch

import semilinear_sensitivity_rules as nr

pytestmark = pytest.mark.gpu
proto = nr.proto
D, R, POLY, EXP = nr.D, nr.R, nr.POLY, nr.EXP


def _device_tables(dev, d, nq, kind, nterm, want, P=None, band_ends=None, kinds=(D, D), q_tabs=True):
    """ops.nl_sensitivity into canary-filled buffers -> the dict of nr.nl_host."""
    from hybrid_fem_lssvr_amd import ops
    t = {k: torch.as_tensor(d[k], device=dev) for k in ("x", "U", "Z", "q")}
    nc, ne = d["Z"].shape[0], len(d["x"]) - 1
    full = {k: torch.full((nc, ne, nq), nr.CANARY, dtype=torch.float64, device=dev) for k in nr.TABLES[:4]}
    full["q"] = torch.full((nc, nterm, ne, nq), nr.CANARY, dtype=torch.float64, device=dev)
    full["ends"] = torch.full((nc, 4), nr.CANARY, dtype=torch.float64, device=dev)
    bands = None
    if band_ends is not None:          # any bands whose sub[0] and sup[ne-1] are the pair
        sub, sup = np.zeros(ne), np.zeros(ne)
        sub[0], sup[ne - 1] = band_ends
        bands = dict(sub=torch.as_tensor(sub, device=dev), sup=torch.as_tensor(sup, device=dev))
    out = {k: full[k] for k in want}
    if bands is not None:
        out["ends"] = full["ends"]
    res = ops.nl_sensitivity(t["x"], t["U"], t["Z"], nq, kind, nterm, q_tabs=t["q"] if q_tabs else None, want=want,
                             P=None if P is None else torch.as_tensor(P, device=dev), bands=bands, end_kinds=kinds,
                             out=out)
    assert set(res) == set(out) and all(res[k] is out[k] for k in out)
    return {k: v.cpu().numpy() for k, v in full.items()}


def _compare(dev, ne, nq, nc, nu, kind, nterm, kinds=(R, D), subsets=False):
    """The device against the host mirror on one set of inputs: all outputs, and with ``subsets`` every want subset
    and the end gradients alone."""
    d = nr.kernel_inputs(ne, nq, nc, nu, nterm)
    ref = nr.nl_host(d["x"], nq, d["U"], d["Z"], kind, nterm, d["q"], nr.TABLES, d["P"], d["band_ends"], kinds,
                     ends=True)[1]
    qbar = nr.exp_bars(d["x"], nq, d["U"], d["Z"], d["q"]) if kind == EXP else None
    got = _device_tables(dev, d, nq, kind, nterm, nr.TABLES, d["P"], d["band_ends"], kinds)
    nr.check_against(got, nr.TABLES, ref, True, kind, qbar)
    if subsets:
        for want in nr.WANTS[1:]:
            nr.check_against(_device_tables(dev, d, nq, kind, nterm, want), want, ref, False, kind, qbar)
        only = _device_tables(dev, d, nq, kind, nterm, (), d["P"], d["band_ends"], kinds)
        nr.check_against(only, (), ref, True, kind, qbar)
        if kind == POLY:          # q_tabs is not read
            only = _device_tables(dev, d, nq, kind, nterm, ("q",), q_tabs=False)
            nr.check_against(only, ("q",), ref, False)
    return d, got


@pytest.mark.parametrize("nc,nu", [(1, 1), (3, 1), (3, 3)])
@pytest.mark.parametrize("ne,nq", [(1, 1), (1, 2), (63, 1), (64, 1), (32, 2), (65, 1), (13, 5), (257, 2)])
def test_device_is_the_host_mirror(dev, ne, nq, nc, nu):
    """Tables of 1, 2, 63, 64, 65 and 514 entries -- on both sides of a wave --: POLY nterm 1 .. 6 bit-equal in every
    output, gq_0 == -gf, gq_1 == gc, every want subset leaves its canaries; EXP within the bars of the two exps."""
    for kind, nterm in [(POLY, k) for k in range(1, 7)] + [(EXP, 2)]:
        _compare(dev, ne, nq, nc, nu, kind, nterm, ((D, D), (R, D), (D, R), (R, R))[nterm % 4], subsets=nterm in (2, 4))


def test_device_past_one_grid_pass(dev):
    """131073 elements, nquad 2: 262146 entries, two more than 1024 x 256 threads, so the grid-stride loop takes a
    second trip in two threads only.  Bit-equal to the host mirror, and the entries around the seam against the numpy
    formulas, so that a stride error that hits mirror and device alike cannot hide."""
    ne, nq, nc, nterm = 131073, 2, 2, 4
    assert ne * nq == 1024 * 256 + 2
    d, got = _compare(dev, ne, nq, nc, nc, POLY, nterm)
    for e in (0, 1, ne // 2 - 1, ne // 2, ne - 2, ne - 1):          # one element at a time: a mesh of one element each
        for j in range(nc):
            one = nr.nl_numpy(d["x"][e:e + 2], nq, d["U"][j:j + 1, e:e + 2], d["Z"][j:j + 1, e:e + 2], POLY, nterm)
            for k in nr.TABLES:
                assert np.array_equal(got[k][j][..., e, :], one[k][0][..., 0, :]), (k, j, e)


@pytest.mark.parametrize("kind,nterm", [(POLY, 6), (EXP, 2)])
def test_device_eight_cases(dev, kind, nterm):
    _compare(dev, 33, 2, 8, 8, kind, nterm, subsets=True)
    _compare(dev, 33, 5, 8, 1, kind, nterm)


@pytest.mark.parametrize("c,fem_solver", nr.facade_cases(), ids=lambda v: v.id if isinstance(v, nr.Case) else v)
def test_facade_against_complex_step(dev, note, c, fem_solver):
    """Every group -- a, b, c, f, each q_k, the end data -- within 10x the prototype's own reading of the same case."""
    read, adj, cs = c.reference
    s = nr.facade_solver(c, fem_solver)
    r = s.solve_semilinear_sensitivity(**nr.functional_kw(c))
    devn = proto.deviation(nr.facade_gradients(r), cs)
    print(f"{c.id} {fem_solver}: device {devn:.2e}, prototype {read:.2e}, bar {c.bar:.2e}, Newton: {r.newton}")
    note(f"{c.id} {fem_solver} deviation from the complex step", devn, c.bar)
    assert (r.d_convection is None) == (not c.conv) and (r.d_reaction is None) == (not c.react)
    assert r.d_coef.shape == r.d_rhs.shape == (c.ne, c.nq) and r.d_nonlinear.shape == (c.nterm, c.ne, c.nq)
    assert r.newton is s.newton and r.newton.converged
    assert devn <= c.bar
    # (J of the nodal solution: a sum of some 34 products of rounded factors, each of size 1 at most)
    assert abs(r.value - float(c.J.value(c.x, s.fem_values))) <= 64 * nr.EPS * max(1.0, abs(r.value))
    assert abs(r.value - float(adj["value"])) <= c.bar * max(1.0, abs(float(adj["value"])))
    assert np.array_equal(r.nodes, c.x) and r.adjoint.shape == c.x.shape
    assert np.all(r.adjoint[[0, -1]][np.array(c.kinds) == D] == 0.0)
    assert np.all(r.d_kappa[np.array(c.kinds) == D] == 0.0)


@pytest.mark.parametrize("fem_solver", ["bands", "pivot"])
def test_linear_limit(dev, note, fem_solver):
    """nonlinear=("poly", [0, c0]) is the linear problem with the reaction c + c0: tables and ends agree with
    solve_sensitivity on that solver within the bar of the case; d_nonlinear[1] is d_reaction and d_nonlinear[0] is
    -d_rhs, bit for bit."""
    c = nr.case("linear", 33, 2, False, True, (D, R), "goal")
    c0 = proto.LAWS["linear"][1][1]
    r = nr.facade_solver(c, fem_solver).solve_semilinear_sensitivity(**nr.functional_kw(c))
    lin = nr.facade_solver(c, fem_solver, nonlinear=False, reaction=lambda x: proto.sp.reaction(x) + c0(x)) \
        .solve_sensitivity(**nr.functional_kw(c))
    devn = proto.deviation(nr.facade_gradients(r, False), nr.facade_gradients(lin, False))
    print(f"linear limit {fem_solver}: {devn:.2e}, bar {c.bar:.2e}, Newton: {r.newton}")
    note(f"linear limit {fem_solver}", devn, c.bar)
    assert devn <= c.bar and abs(r.value - lin.value) <= c.bar * max(1.0, abs(lin.value))
    assert np.array_equal(r.d_nonlinear[1], r.d_reaction) and np.array_equal(r.d_nonlinear[0], -r.d_rhs)
    assert proto.deviation(dict(c=r.d_nonlinear[1], f=-r.d_nonlinear[0]), nr.facade_gradients(lin, False)) <= c.bar


def test_inverse_problem(dev, note):
    """The prototype's demo through the facade: 20 steps of plain gradient descent on the log of the piecewise-constant
    q_3."""
    import math
    import hybrid_fem_lssvr_amd as pkg
    x, _, obs = proto.demo_truth()
    theta = np.full(proto.DEMO_NE, math.log(proto.DEMO_START))
    s = pkg.FEMLSSVRPrimalSolver(mesh=x, nquad=2, rhs=proto.demo_rhs, lssvr_M=9, n_colloc=16,
                                 nonlinear=("poly", [proto.zero, proto.zero, proto.zero,
                                                     lambda pts: np.broadcast_to(np.exp(theta)[:, None], np.shape(pts))]))
    hist = []
    for _ in range(proto.DEMO_STEPS + 1):
        r = s.solve_semilinear_sensitivity(observe=obs)
        hist.append(r.value)
        theta = theta - proto.DEMO_RATE * (r.d_nonlinear[3].sum(axis=1) * np.exp(theta)) / hist[0]
    print("misfit:", " ".join(f"{v:.3e}" for v in hist))
    note("inverse problem, final misfit", hist[-1], nr.DEMO_FINAL)
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] - nr.DEMO_FINAL) <= nr.DEMO_RTOL * nr.DEMO_FINAL
