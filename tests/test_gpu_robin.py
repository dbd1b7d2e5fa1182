"""GPU: Neumann and Robin boundary conditions through every layer -- the tridiagonal solves with free ends and the
boundary term of the indicator against their numpy restatement (tests/robin_rules.py), and the facade's ``boundary``
keyword through solve / solve_many / solve_adaptive."""
import os
import re

import numpy as np
import pytest

import convection_rules as cr
import robin_rules as rr

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hybrid_fem_lssvr_amd", "csrc")


def _constant(path, name):
    return int(re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, path)).read()).group(1))


# rows of a level that one workgroup of the condensation kernel owns: a thread per chunk of kLc rows
T = _constant("lssvr_device.hpp", "kBlock") * _constant("tridiag.hip", "kLc")
K_BASE = _constant("tridiag.hip", "kBase")          # unknowns at or below which one workgroup solves the level alone
# ne: an end row that neighbours the other end; the base-level threshold (the unknowns are ne - 1, ne or ne + 1 by the
# kinds); one workgroup of the condensation kernel short of, at and past its rows; many workgroups
SIZES = [1, 2, 3, K_BASE, T - 1, T, T + 1, 2 * T + 1, 100000]

# The bars of test_tridiag_ns_dirichlet_solve (tests/test_gpu_conv.py), copied as numbers; a size between two listed
# ones takes the bar of the next listed size.
TRIDIAG_FORWARD_BAR = {1: 0.0, 2: 1e-15, 3: 1e-15, 24: 1e-14, 511: 2.5e-12, 512: 2.5e-12, 513: 2.5e-12,
                       514: 2.5e-12, 1025: 4e-12, 16385: 2e-9, 100000: 7e-8, 1234567: 2e-6}


def _forward_bar(ne):
    return TRIDIAG_FORWARD_BAR[min(k for k in TRIDIAG_FORWARD_BAR if k >= ne)]


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _solve(ops, conv, bands, kinds, dev, load=None, values=rr.SOLVE_VALUES):
    diag, sub, sup, ld = (_t(b, dev) for b in bands)
    ld = ld if load is None else load
    multi = ld.dim() == 2
    if conv:
        fn = ops.tridiag_ns_bc_solve_multi if multi else ops.tridiag_ns_bc_solve
        return fn(diag, sub, sup, ld, kinds, rr.SOLVE_KAPPA, values)
    fn = ops.tridiag_bc_solve_multi if multi else ops.tridiag_bc_solve
    return fn(diag, sub, ld, kinds, rr.SOLVE_KAPPA, values)


# ---------------------------------------------------------------------------
# 1. the solves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("conv", [False, True], ids=["sym", "ns"])
@pytest.mark.parametrize("kinds", rr.KIND_PAIRS, ids=["DD", "DR", "RD", "RR"])
@pytest.mark.parametrize("ne", SIZES)
def test_bc_solve_vs_rules(dev, note, ne, kinds, conv):
    """A Dirichlet end comes back exact; every unknown row (the Robin end rows included) has a residual at rounding
    level of |A| |u|; the forward error against the long-double Thomas solve of the same system is within max(10 x
    LAPACK's own distance from it, the bar of the Dirichlet entries at that size) -- the test of the Dirichlet
    entries (tests/test_gpu_conv.py), bar for bar.  At up to 3 elements the dense numpy.linalg.solve is compared too."""
    from hybrid_fem_lssvr_amd import ops
    bands, u_ld, u_la = rr.solve_case(ne, kinds, conv)
    before = [b.copy() for b in bands]
    dev_bands = [_t(b, dev) for b in bands]
    args = dev_bands if conv else [dev_bands[0], dev_bands[1], dev_bands[3]]
    fn = ops.tridiag_ns_bc_solve if conv else ops.tridiag_bc_solve
    u = fn(*args, kinds, rr.SOLVE_KAPPA, rr.SOLVE_VALUES).cpu().numpy()
    # the caller's bands are read only
    for b, d in zip(before, dev_bands):
        assert np.array_equal(b, d.cpu().numpy())
    assert u.shape == (ne + 1,)
    for i, end in ((0, 0), (1, -1)):
        if kinds[i] == rr.DIRICHLET:
            assert u[end] == rr.SOLVE_VALUES[i]
    scale = float(np.max(np.abs(u_ld)))
    A_d, A_lo, A_up, A_r, first = rr.unknown_rows(*bands, kinds, rr.SOLVE_KAPPA, rr.SOLVE_VALUES)
    if len(A_d):
        x = u[first:first + len(A_d)]
        r = A_d * x - A_r
        r[1:] += A_lo * x[:-1]
        r[:-1] += A_up * x[1:]
        res, res_bar = np.max(np.abs(r)), 1e-13 * np.max(np.abs(A_d)) * scale * max(1.0, np.log2(ne))
        note(f"bc_solve ne={ne} {kinds} conv={conv}: residual", res, res_bar)
        assert res <= res_bar
    lapack = float(np.max(np.abs(u_la.astype(np.longdouble) - u_ld)))
    fwd = float(np.max(np.abs(u.astype(np.longdouble) - u_ld)))
    bar = max(10.0 * lapack, _forward_bar(ne)) * scale
    note(f"bc_solve ne={ne} {kinds} conv={conv}: forward error (LAPACK {lapack:.1e})", fwd, bar)
    print(f"ne={ne} {kinds} conv={conv}: forward {fwd:.2e}, LAPACK {lapack:.2e}, bar {bar:.2e}")
    assert fwd <= bar
    if ne <= 3:
        dense = rr.dense_solve(*bands, kinds, rr.SOLVE_KAPPA, rr.SOLVE_VALUES)
        assert np.max(np.abs(u - dense)) <= max(10.0 * lapack, 1e-15) * scale


@pytest.mark.parametrize("conv", [False, True], ids=["sym", "ns"])
@pytest.mark.parametrize("ne", SIZES)
def test_two_dirichlet_ends_are_the_dirichlet_entries_bit_for_bit(dev, ne, conv):
    import torch
    from hybrid_fem_lssvr_amd import ops
    bands, _, _ = rr.solve_case(ne, (rr.DIRICHLET, rr.DIRICHLET), conv)
    diag, sub, sup, load = (_t(b, dev) for b in bands)
    rng = np.random.default_rng(ne)
    loads = torch.stack([load] + [_t(rng.standard_normal(ne + 1), dev) for _ in range(2)])
    bc = _t(np.array([[0.25, -0.5], [1.0, 2.0], [-3.0, 0.5]]), dev)
    if conv:
        old = ops.tridiag_ns_dirichlet_solve_multi(diag, sub, sup, loads, bc)
        new = ops.tridiag_ns_bc_solve_multi(diag, sub, sup, loads, (0, 0), (5.0, 7.0), bc)      # kappa is not read
        one = ops.tridiag_ns_dirichlet_solve(diag, sub, sup, load, 0.25, -0.5)
        one_new = ops.tridiag_ns_bc_solve(diag, sub, sup, load, (0, 0), (0.0, 0.0), (0.25, -0.5))
    else:
        old = ops.tridiag_dirichlet_solve_multi(diag, sub, loads, bc)
        new = ops.tridiag_bc_solve_multi(diag, sub, loads, (0, 0), (5.0, 7.0), bc)
        one = ops.tridiag_dirichlet_solve(diag, sub, load, 0.25, -0.5)
        one_new = ops.tridiag_bc_solve(diag, sub, load, (0, 0), (0.0, 0.0), (0.25, -0.5))
    assert torch.equal(old, new) and torch.equal(one, one_new) and torch.equal(one, new[0])


@pytest.mark.parametrize("conv", [False, True], ids=["sym", "ns"])
@pytest.mark.parametrize("kinds", rr.KIND_PAIRS[1:], ids=["DR", "RD", "RR"])
@pytest.mark.parametrize("nc", [1, 3, 8, 9])
@pytest.mark.parametrize("ne", [3, K_BASE, T + 1])
def test_multi_rows_are_the_single_calls_bit_for_bit(dev, ne, nc, kinds, conv):
    """One pass, a full pass of eight, and eight plus one: every row equals the nc = 1 call on that case; ``out`` rows
    past nc and the caller's bands stay as they were."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    bands, _, _ = rr.solve_case(ne, kinds, conv)
    rng = np.random.default_rng(100 * ne + nc)
    loads = _t(rng.standard_normal((nc, ne + 1)), dev)
    values = _t(rng.standard_normal((nc, 2)), dev)
    keep = (loads.clone(), values.clone())
    out = torch.full((nc + 1, ne + 1), -777.0, dtype=torch.float64, device=dev)
    diag, sub, sup, _ = (_t(b, dev) for b in bands)
    if conv:
        U = ops.tridiag_ns_bc_solve_multi(diag, sub, sup, loads, kinds, rr.SOLVE_KAPPA, values, out=out)
    else:
        U = ops.tridiag_bc_solve_multi(diag, sub, loads, kinds, rr.SOLVE_KAPPA, values, out=out)
    assert U.shape == (nc, ne + 1) and bool((out[nc] == -777.0).all())
    assert torch.equal(loads, keep[0]) and torch.equal(values, keep[1])
    for b, d in zip(bands[:3], (diag, sub, sup)):
        assert np.array_equal(b, d.cpu().numpy())
    vh = values.cpu().numpy()
    for q in range(nc):
        one = _solve(ops, conv, bands, kinds, dev, load=loads[q].clone(), values=(vh[q, 0], vh[q, 1]))
        assert torch.equal(U[q], one), (q, float((U[q] - one).abs().max()))


def test_bc_solve_rejects_bad_arguments(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    d, o, ld = (torch.ones(n, dtype=torch.float64, device=dev) for n in (6, 5, 6))
    for kinds, kappa in (((0, 2), (0.0, 0.0)), ((0, 1), (0.0, -1.0)), ((0, 1), (float("nan"), 0.0))):
        with pytest.raises(ValueError):
            ops.tridiag_bc_solve(d, o, ld, kinds, kappa)
    with pytest.raises(ValueError, match="band lengths"):
        ops.tridiag_bc_solve(d, o[:4], ld, (0, 1), (0.0, 0.0))
    with pytest.raises(ValueError, match="end_values"):
        ops.tridiag_bc_solve_multi(d, o, ld.reshape(1, 6), (0, 1), (0.0, 0.0), torch.zeros(2, 2, dtype=torch.float64,
                                                                                          device=dev))
    with pytest.raises(ValueError, match="work holds"):
        ops.tridiag_bc_solve_multi(d, o, ld.reshape(1, 6), (0, 1), (0.0, 0.0),
                                   work=torch.zeros(1, dtype=torch.float64, device=dev))
    with pytest.raises(TypeError):
        ops.tridiag_ns_bc_solve(d, o, o.float(), ld, (0, 1), (0.0, 0.0))


# ---------------------------------------------------------------------------
# 2. the boundary term of the indicator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", rr.KIND_PAIRS, ids=["DD", "DR", "RD", "RR"])
@pytest.mark.parametrize("ne,M", [(1, 9), (2, 2), (37, 12), (300, 33)])
def test_estimate_ends_vs_rules(dev, ne, M, kinds):
    """eta2 of the two end elements and out3 to 1e-12 relative, everything between untouched; two Dirichlet ends
    change nothing, bit for bit."""
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(1000 * ne + M)
    h = rng.uniform(0.5, 1.5, ne)
    x = np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])
    W = rng.standard_normal((ne, M)) / (1.0 + np.arange(M)) ** 2
    eta2 = rng.uniform(0.1, 1.0, ne)
    out3 = np.array([eta2.sum(), eta2.max(), 0.0])
    kappa, g, a_ends = (0.7, 2.0), (0.3, -1.1), (1.5, 0.8)
    ref_eta2, ref_out3 = rr.estimate_ends(x, W, kinds, kappa, g, a_ends, eta2, out3)
    e_dev, o_dev = _t(eta2, dev), _t(out3, dev)
    got_e, got_o = ops.estimate_ends(_t(x, dev), _t(W, dev), kinds, kappa, g, a_ends, e_dev, o_dev)
    assert got_e is e_dev and got_o is o_dev
    got_e, got_o = got_e.cpu().numpy(), got_o.cpu().numpy()
    if kinds == (rr.DIRICHLET, rr.DIRICHLET):
        assert np.array_equal(got_e, eta2) and np.array_equal(got_o, out3)
        return
    assert np.array_equal(got_e[1:-1], eta2[1:-1])
    for e in (0, ne - 1):
        assert abs(got_e[e] - ref_eta2[e]) <= 1e-12 * abs(ref_eta2[e])
    assert np.all(np.abs(got_o - ref_out3) <= 1e-12 * np.abs(ref_out3))
    assert got_o[2] == 0.0 and got_o[1] == max(out3[1], got_e[0], got_e[-1])


def test_estimate_ends_counts_a_nan_row(dev):
    from hybrid_fem_lssvr_amd import ops
    x = np.linspace(0.0, 1.0, 6)
    W = np.ones((5, 7))
    W[4, 3] = np.nan
    eta2 = np.full(5, 0.5)
    out3 = np.array([2.5, 0.5, 0.0])
    e, o = ops.estimate_ends(_t(x, dev), _t(W, dev), (1, 1), (0.0, 1.0), (0.0, 0.0), (1.0, 1.0), _t(eta2, dev),
                             _t(out3, dev))
    e, o = e.cpu().numpy(), o.cpu().numpy()
    ref_e, ref_o = rr.estimate_ends(x, W, (1, 1), (0.0, 1.0), (0.0, 0.0), (1.0, 1.0), eta2, out3)
    assert np.isnan(e[4]) and o[2] == 1.0 == ref_o[2]
    assert abs(e[0] - ref_e[0]) <= 1e-12 * ref_e[0] and abs(o[0] - ref_o[0]) <= 1e-12 * ref_o[0] and o[1] == e[0]


# ---------------------------------------------------------------------------
# 3. the facade
# ---------------------------------------------------------------------------
def _solver(name, boundary, nodes=25, **kw):
    import hybrid_fem_lssvr_amd as pkg
    p = rr.PROBLEMS[name]
    eq = {}
    if p["a"] is not None:
        eq["coef"] = (p["a"], p["da"])
    if p["b"] is not None:
        eq["convection"] = p["b"]
    if p["c"] is not None:
        eq["reaction"] = p["c"]
    return pkg.FEMLSSVRPrimalSolver(nodes, lssvr_M=8, lssvr_gamma=1e8, n_colloc=16, nquad=3, rhs=p["f"],
                                    global_domain=(-1, 1), boundary=boundary, **eq, **kw)


@pytest.mark.parametrize("name", sorted(rr.PROBLEMS))
def test_facade_manufactured_problems(dev, note, name):
    """24 elements, M = 8, 16 collocation points: fem_values within 1e-12 of the restatement, and the max error of
    evaluate_solution on 2001 points below 10 x the error of the same solver on the Dirichlet version of the problem
    (the same u, exact values at both ends), computed here."""
    p = rr.PROBLEMS[name]
    xq = np.linspace(-1.0, 1.0, 2001)
    s = _solver(name, p["boundary"])
    s.solve()
    ref = rr.fem_solve(np.linspace(-1.0, 1.0, 25), p["f"], p["kinds"], p["kappa"], p["values"], p["a"], p["b"],
                       p["c"], 3)
    assert np.max(np.abs(s.fem_values - ref)) <= 1e-12
    assert s.enhanced.n_fallback == 0
    err = float(np.max(np.abs(s.evaluate_solution(xq) - p["u"](xq))))
    d = _solver(name, (("dirichlet", float(p["u"](-1.0))), ("dirichlet", float(p["u"](1.0)))))
    d.solve()
    err_d = float(np.max(np.abs(d.evaluate_solution(xq) - p["u"](xq))))
    note(f"facade {name}: max error with the Neumann / Robin ends", err, 10.0 * err_d)
    note(f"facade {name}: max error of the Dirichlet version", err_d)
    print(f"{name}: error {err:.3e}, Dirichlet version {err_d:.3e}")
    assert err <= 10.0 * err_d
    # the indicator carries the boundary term: the end elements' eta2 exceed the Dirichlet-end indicator by h/2 J^2
    eta2 = s.estimate()
    assert eta2.shape == (24,) and np.all(np.isfinite(eta2)) and np.all(eta2 >= 0.0)


def test_facade_solve_many_equals_single_solves(dev):
    """Three cases that differ in g at the Robin end: U of solve_many equals three solve() calls bit for bit."""
    p = rr.PROBLEMS["exp"]
    gs = (rr.EXP_G, 0.0, -2.5)
    s = _solver("exp", p["boundary"])
    sols = s.solve_many([p["f"]] * 3, bc=[(p["values"][0], g) for g in gs])
    for g, sol in zip(gs, sols):
        one = _solver("exp", (p["boundary"][0], ("robin", rr.EXP_KAPPA, g)))
        one.solve()
        nodes = np.asarray(one.fem_nodes)
        many_nodal = sol.evaluate(nodes)
        assert np.array_equal(sol.nodes.cpu().numpy(), nodes)
        # U itself: the multi solve's row against the single solve's nodal values
        U = s._fem_many([p["f"]], np.array([[p["values"][0], g]]))[1][0].cpu().numpy()
        assert np.array_equal(U, one.fem_values)
        assert np.max(np.abs(many_nodal - one.evaluate_solution(nodes))) <= 1e-10
    # ... and the three rows of one multi call, bit for bit
    U3 = s._fem_many([p["f"]] * 3, np.array([(p["values"][0], g) for g in gs]))[1].cpu().numpy()
    for g, row in zip(gs, U3):
        one = _solver("exp", (p["boundary"][0], ("robin", rr.EXP_KAPPA, g)))
        one.solve_fem()
        assert np.array_equal(row, one.fem_values)


def test_adaptive_outflow_layer_with_neumann_outflow_end(dev, note):
    """-eps u'' + u' = 1 on (0, 1), eps = 0.02 (the layer problem of tests/test_gpu_conv.py), u(0) = 0 and the
    Neumann end eps u'(1) = 0 at the outflow: solve_adaptive(mode="h") lowers the estimate monotonically over its
    first four rounds and ends without a fallback element."""
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(33, lssvr_M=9, lssvr_gamma=1e10, n_colloc=16, nquad=5, rhs=cr.layer_f,
                                 mesh=np.linspace(0, 1, 33), global_domain=(0, 1), coef=(cr.layer_a, cr.layer_da),
                                 convection=cr.layer_b, boundary=(None, ("neumann", 0.0)))
    est = s.solve_adaptive(tol=1e-12, theta=0.5, max_elements=256, max_iter=5, mode="h")
    hist = [r["estimate"] for r in s.adapt_history]
    for i, v in enumerate(hist):
        note(f"adaptive Neumann outflow: estimate of round {i}", v)
    print("estimates", hist, "elements", [r["ne"] for r in s.adapt_history])
    assert len(hist) >= 4 and np.all(np.isfinite(hist)) and est == hist[-1]
    assert all(b < a for a, b in zip(hist[:3], hist[1:4])), hist
    assert s.enhanced.n_fallback == 0
