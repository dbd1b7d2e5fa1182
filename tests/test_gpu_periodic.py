"""GPU: periodic boundary conditions through every layer -- the cyclic tridiagonal solves and the seam term of the
indicator against their numpy restatement (tests/periodic_rules.py), and the facade's ``boundary="periodic"`` through
solve / solve_many / solve_adaptive."""
import importlib.util
import os

import numpy as np
import pytest

import periodic_rules as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ne: the smallest cyclic system (one interior unknown), three unknowns, a small odd one; 513 has 512 interior unknowns,
# the base level alone, 514 the first condensed level; one workgroup of the condensation kernel (256 threads x 8 rows =
# 2048 rows) and two of them just exceeded; many workgroups
SIZES = [2, 3, 9, 513, 514, 2049, 4097, 100000]

# The bars of the Dirichlet/Dirichlet case of tests/test_gpu_robin.py, copied as numbers; a size between two listed
# ones takes the bar of the next listed size.
TRIDIAG_FORWARD_BAR = {1: 0.0, 2: 1e-15, 3: 1e-15, 24: 1e-14, 511: 2.5e-12, 512: 2.5e-12, 513: 2.5e-12,
                       514: 2.5e-12, 1025: 4e-12, 16385: 2e-9, 100000: 7e-8, 1234567: 2e-6}


def _forward_bar(ne, lapack):
    """The forward bar of tests/test_gpu_robin.py, relative to max |u|: max(10 x the distance of the pivoted LAPACK
    solve from the same long-double reference, the bar of the Dirichlet entries at that size)."""
    return max(10.0 * lapack, TRIDIAG_FORWARD_BAR[min(k for k in TRIDIAG_FORWARD_BAR if k >= ne)])


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _solve(ops, conv, bands, dev, load=None, **kw):
    diag, sub, sup, ld = (_t(b, dev) for b in bands)
    ld = ld if load is None else load
    multi = ld.dim() == 2
    if conv:
        fn = ops.tridiag_ns_periodic_solve_multi if multi else ops.tridiag_ns_periodic_solve
        return fn(diag, sub, sup, ld, **kw)
    fn = ops.tridiag_periodic_solve_multi if multi else ops.tridiag_periodic_solve
    return fn(diag, sub, ld, **kw)


def _lapack_distance(u_la, u_ld):
    scale = float(np.max(np.abs(u_ld)))
    return (float(np.max(np.abs(u_la.astype(np.longdouble) - u_ld))) / scale if scale > 0 else 0.0), scale


# ---------------------------------------------------------------------------
# 1. the solves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("conv", [False, True], ids=["sym", "ns"])
@pytest.mark.parametrize("ne", SIZES)
def test_periodic_solve_vs_rules(dev, note, ne, conv):
    """u[0] == u[ne] exactly; every row of the cyclic system (the seam row included) has a residual at rounding level
    of |A| |u|; the forward error against the long-double cyclic Thomas solve is within max(10 x LAPACK's own distance
    from it, the bar of the Dirichlet entries at that size), relative to max |u|.  Measured on an MI355X, with the
    factor by which LAPACK's distance exceeds its Dirichlet/Dirichlet one: DESIGN.md section 22.  At up to 9 elements
    the dense numpy.linalg.solve is compared too."""
    from hybrid_fem_lssvr_amd import ops
    bands, u_ld, u_la = pr.solve_case(ne, conv)
    before = [b.copy() for b in bands]
    dev_bands = [_t(b, dev) for b in bands]
    args = dev_bands if conv else [dev_bands[0], dev_bands[1], dev_bands[3]]
    fn = ops.tridiag_ns_periodic_solve if conv else ops.tridiag_periodic_solve
    u = fn(*args).cpu().numpy()
    for b, d in zip(before, dev_bands):          # the caller's bands and load are read only
        assert np.array_equal(b, d.cpu().numpy())
    assert u.shape == (ne + 1,) and u[0] == u[-1] and np.all(np.isfinite(u))
    lapack, scale = _lapack_distance(u_la, u_ld)
    D = pr.cyclic_bands(*bands)[0]
    res = float(np.max(np.abs(pr.residual(*bands, u))))
    res_bar = 1e-13 * np.max(np.abs(D)) * scale * max(1.0, np.log2(ne))
    note(f"periodic_solve ne={ne} conv={conv}: residual", res, res_bar)
    fwd = float(np.max(np.abs(u.astype(np.longdouble) - u_ld)))
    bar = _forward_bar(ne, lapack) * scale
    lapack_dd = pr.dirichlet_lapack_distance(ne, conv)
    note(f"periodic_solve ne={ne} conv={conv}: forward error (LAPACK {lapack * scale:.1e}, Dirichlet LAPACK rel "
         f"{lapack_dd:.1e}, scale {scale:.2e})", fwd, bar)
    print(f"ne={ne} conv={conv}: residual {res:.2e} (bar {res_bar:.2e}), forward {fwd:.2e}, LAPACK {lapack * scale:.2e},"
          f" bar {bar:.2e}; LAPACK rel periodic {lapack:.2e} / Dirichlet {lapack_dd:.2e}")
    assert res <= res_bar
    assert fwd <= bar
    if ne <= 9:
        dense = pr.dense_solve(*bands)
        assert np.max(np.abs(u - dense)) <= bar + float(np.max(np.abs(dense - u_ld)))


@pytest.mark.parametrize("conv", [False, True], ids=["sym", "ns"])
@pytest.mark.parametrize("ne", SIZES)
def test_seam_invariance(dev, note, ne, conv):
    """The same cyclic system with the seam at node k (rows split and merged by ``periodic_rules.roll_bands``): the
    rolled solution agrees with the rolled original within the forward bar.  A solve that treats x_0 as a Dirichlet
    end cannot pass this."""
    from hybrid_fem_lssvr_amd import ops
    bands, u_ld, u_la = pr.solve_case(ne, conv)
    lapack, scale = _lapack_distance(u_la, u_ld)
    bar = _forward_bar(ne, lapack) * scale
    u = _solve(ops, conv, bands, dev).cpu().numpy()
    for k in sorted({1, ne // 2}):
        uk = _solve(ops, conv, pr.roll_bands(*bands, k), dev).cpu().numpy()
        diff = float(np.max(np.abs(uk - pr.roll_solution(u, k))))
        note(f"seam invariance ne={ne} conv={conv} k={k}", diff, bar)
        print(f"ne={ne} conv={conv} k={k}: {diff:.2e} (bar {bar:.2e})")
        assert uk[0] == uk[-1] and diff <= bar


@pytest.mark.parametrize("conv", [False, True], ids=["sym", "ns"])
@pytest.mark.parametrize("nc", [1, 3, 7, 8, 9])
@pytest.mark.parametrize("ne", [2, 513, 2049])
def test_multi_rows_are_the_single_calls_bit_for_bit(dev, ne, nc, conv):
    """One case, a few, seven (with z: eight solves), a full pass of eight, eight plus one: every row equals the
    nc = 1 call on that case and closes exactly; ``out`` rows past nc and the caller's arrays stay as they were.  With
    random loads -- no symmetry that could hide a wrong corner entry -- the residual of the cyclic system is at
    rounding level of |A| |u|."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    bands = pr.solve_case(ne, conv)[0]
    rng = np.random.default_rng(100 * ne + nc)
    loads_h = rng.standard_normal((nc, ne + 1))
    loads = _t(loads_h, dev)
    out = torch.full((nc + 1, ne + 1), -777.0, dtype=torch.float64, device=dev)
    U = _solve(ops, conv, bands, dev, load=loads, out=out)
    assert U.shape == (nc, ne + 1) and bool((out[nc] == -777.0).all())
    assert np.array_equal(loads.cpu().numpy(), loads_h)
    assert bool((U[:, 0] == U[:, ne]).all())
    Uh = U.cpu().numpy()
    D = pr.cyclic_bands(*bands)[0]
    for q in range(nc):
        one = _solve(ops, conv, bands, dev, load=loads[q].clone())
        assert torch.equal(U[q], one), (q, float((U[q] - one).abs().max()))
        res = np.max(np.abs(pr.residual(bands[0], bands[1], bands[2], loads_h[q], Uh[q])))
        assert res <= 1e-13 * np.max(np.abs(D)) * np.max(np.abs(Uh[q])) * max(1.0, np.log2(ne))


def test_periodic_solve_rejects_bad_arguments(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    d, o, ld = (torch.ones(n, dtype=torch.float64, device=dev) for n in (6, 5, 6))
    with pytest.raises(ValueError, match="band lengths"):
        ops.tridiag_periodic_solve(d, o[:4], ld)
    with pytest.raises(ValueError, match="band lengths"):
        ops.tridiag_periodic_solve_multi(d, o, ld)
    with pytest.raises(ValueError, match="two elements"):
        ops.tridiag_periodic_solve(d[:2], o[:1], ld[:2])
    with pytest.raises(ValueError, match="work holds"):
        ops.tridiag_periodic_solve_multi(d, o, ld.reshape(1, 6), work=torch.zeros(1, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="out must"):
        ops.tridiag_ns_periodic_solve_multi(d, o, o, ld.reshape(1, 6),
                                            out=torch.zeros(1, 5, dtype=torch.float64, device=dev))
    with pytest.raises(TypeError):
        ops.tridiag_ns_periodic_solve(d, o, o.float(), ld)
    with pytest.raises(ValueError, match="three nodes"):
        ops.estimate_seam(d[:2], d[:2].reshape(1, 2), (1.0, 1.0), d[:1], d[:3])


# ---------------------------------------------------------------------------
# 2. the seam term of the indicator
# ---------------------------------------------------------------------------
def _mesh_and_rows(ne, M):
    rng = np.random.default_rng(1000 * ne + M)
    h = rng.uniform(0.5, 1.5, ne)
    x = np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])
    return x, rng.standard_normal((ne, M)) / (1.0 + np.arange(M)) ** 2


@pytest.mark.parametrize("M", [2, 9, 33])
@pytest.mark.parametrize("ne", [2, 3, 129])
def test_estimate_seam_vs_rules(dev, ne, M):
    """After ``ops.estimate``: eta2 of the two end elements and out3 to 1e-12 relative, everything between
    untouched."""
    from hybrid_fem_lssvr_amd import ops
    x, W = _mesh_and_rows(ne, M)
    a_seam = (1.5, 0.8)
    x_dev, W_dev = _t(x, dev), _t(W, dev)
    e_dev, _, o_dev = ops.estimate(x_dev, W_dev, 8)
    eta2, out3 = e_dev.cpu().numpy().copy(), o_dev.cpu().numpy().copy()
    assert out3[2] == 0.0
    ref_eta2, ref_out3 = pr.estimate_seam(x, W, a_seam, eta2, out3)
    got_e, got_o = ops.estimate_seam(x_dev, W_dev, a_seam, e_dev, o_dev)
    assert got_e is e_dev and got_o is o_dev
    got_e, got_o = got_e.cpu().numpy(), got_o.cpu().numpy()
    assert np.array_equal(got_e[1:-1], eta2[1:-1])
    for e in (0, ne - 1):
        assert got_e[e] > eta2[e] and abs(got_e[e] - ref_eta2[e]) <= 1e-12 * abs(ref_eta2[e])
    assert np.all(np.abs(got_o - ref_out3) <= 1e-12 * np.abs(ref_out3))
    assert got_o[2] == 0.0 and got_o[1] == max(out3[1], got_e[0], got_e[-1])


def test_estimate_seam_counts_a_nan_row(dev):
    """A NaN row in element 0: the estimator has counted elements 0 and 1 already; the seam term makes element ne-1
    non-finite, which raises the count once and leaves the sum."""
    from hybrid_fem_lssvr_amd import ops
    x = np.linspace(0.0, 1.0, 6)
    W = np.ones((5, 7))
    W[0, 3] = np.nan
    x_dev, W_dev = _t(x, dev), _t(W, dev)
    e_dev, _, o_dev = ops.estimate(x_dev, W_dev, 8)
    eta2, out3 = e_dev.cpu().numpy().copy(), o_dev.cpu().numpy().copy()
    assert np.isnan(eta2[0]) and np.isfinite(eta2[4])
    e, o = ops.estimate_seam(x_dev, W_dev, (1.0, 1.0), e_dev, o_dev)
    e, o = e.cpu().numpy(), o.cpu().numpy()
    ref_e, ref_o = pr.estimate_seam(x, W, (1.0, 1.0), eta2, out3)
    assert np.isnan(e[4]) and np.isnan(e[0]) and np.array_equal(e[1:4], eta2[1:4], equal_nan=True)
    assert o[2] == out3[2] + 1.0 == ref_o[2] and o[0] == out3[0] == ref_o[0] and o[1] == out3[1]


# ---------------------------------------------------------------------------
# 3. the facade
# ---------------------------------------------------------------------------
def _solver(name, boundary, nodes=25, **kw):
    import hybrid_fem_lssvr_amd as pkg
    p = pr.PROBLEMS[name]
    eq = {}
    if p["a"] is not None:
        eq["coef"] = (p["a"], p["da"])
    if p["b"] is not None:
        eq["convection"] = p["b"]
    if p["c"] is not None:
        eq["reaction"] = p["c"]
    eq.update(kw)
    return pkg.FEMLSSVRPrimalSolver(nodes, lssvr_M=8, lssvr_gamma=1e8, n_colloc=16, nquad=3, rhs=p["f"],
                                    global_domain=(-1, 1), boundary=boundary, **eq)


@pytest.mark.parametrize("name", sorted(pr.PROBLEMS))
def test_facade_manufactured_problems(dev, note, name):
    """24 elements, M = 8, 16 collocation points: fem_values within 1e-12 of the restatement and closed exactly, no
    fallback element, and the max error of evaluate_solution on 2001 points below 10 x the error of the same solver
    on the Dirichlet version of the problem (the same u, exact values at both ends), computed here.  u_h(x_0) and
    u_h(x_ne) come from two different elements, each held to the seam value by its constraint row: they agree to
    1e-12 max |u| (the oracle's float64 solve of these elements meets its constraint rows to 1e-15; the bar leaves the
    device solve the room its other nodal-interpolation checks take)."""
    p = pr.PROBLEMS[name]
    xq = np.linspace(-1.0, 1.0, 2001)
    s = _solver(name, "periodic")
    s.solve()
    ref = pr.fem_solve_periodic(np.linspace(-1.0, 1.0, 25), p["f"], p["a"], p["b"], p["c"], 3)
    assert s.fem_values[0] == s.fem_values[-1]
    assert np.max(np.abs(s.fem_values - ref)) <= 1e-12
    assert s.enhanced.n_fallback == 0
    uq = s.evaluate_solution(xq)
    err = float(np.max(np.abs(uq - p["u"](xq))))
    d = _solver(name, (("dirichlet", float(p["u"](-1.0))), ("dirichlet", float(p["u"](1.0)))))
    d.solve()
    err_d = float(np.max(np.abs(d.evaluate_solution(xq) - p["u"](xq))))
    gap = abs(float(uq[0] - uq[-1]))
    note(f"facade periodic {name}: max error", err, 10.0 * err_d)
    note(f"facade periodic {name}: max error of the Dirichlet version", err_d)
    note(f"facade periodic {name}: |u_h(x_0) - u_h(x_ne)|", gap, 1e-12 * np.max(np.abs(uq)))
    print(f"{name}: error {err:.3e}, Dirichlet version {err_d:.3e}, seam gap {gap:.3e}")
    assert err <= 10.0 * err_d
    assert gap <= 1e-12 * np.max(np.abs(uq))
    # the indicator carries the seam term
    eta2 = s.estimate()
    assert eta2.shape == (24,) and np.all(np.isfinite(eta2)) and np.all(eta2 >= 0.0)


def test_facade_solve_many_equals_single_solves(dev):
    """Three loads: U of solve_many equals three solve() calls bit for bit, and the enhanced solutions agree at the
    nodes."""
    p = pr.PROBLEMS["var"]
    fs = [p["f"], pr.const_f, lambda x: 1.0 + np.sin(np.pi * np.asarray(x, dtype=np.float64))]
    s = _solver("var", "periodic")
    sols = s.solve_many(fs)
    U3 = s._fem_many(fs, np.zeros((3, 2)))[1].cpu().numpy()
    for f, sol, row in zip(fs, sols, U3):
        one = _solver("var", "periodic")
        one.rhs = f
        one.solve()
        nodes = np.asarray(one.fem_nodes)
        assert np.array_equal(sol.nodes.cpu().numpy(), nodes)
        assert np.array_equal(row, one.fem_values) and row[0] == row[-1]
        assert np.max(np.abs(sol.evaluate(nodes) - one.evaluate_solution(nodes))) <= 1e-10
    with pytest.raises(ValueError, match="bc must be None"):
        s.solve_many(fs, bc=[(0.0, 0.0)] * 3)


def _proto():
    spec = importlib.util.spec_from_file_location("periodic_proto",
                                                  os.path.join(ROOT, "scripts", "proto", "periodic_proto.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_adaptive_peak_on_the_seam(dev, note):
    """-u'' + u = f, u = exp(-(1 + cos(pi x)) / 0.05): the peak sits on the seam.  solve_adaptive(mode="h") from 8
    elements with max_elements = 64: the first round bisects both end elements, the final max error on 2001 points is
    below that of the uniform periodic solve with the same element count and within 2 x what the numpy prototype
    (scripts/proto/periodic_proto.py, run here) reaches; no fallback element."""
    import hybrid_fem_lssvr_amd as pkg
    proto = _proto()
    kw = dict(lssvr_M=proto.M, lssvr_gamma=proto.GAMMA, n_colloc=proto.N, nquad=proto.NQUAD, rhs=pr.peak_f,
              global_domain=(-1, 1), reaction=pr._one, boundary="periodic")
    xq = np.linspace(-1.0, 1.0, 2001)
    first = pkg.FEMLSSVRPrimalSolver(mesh=np.linspace(-1, 1, proto.NE0 + 1), **kw)
    first.solve_adaptive(theta=proto.THETA, max_elements=proto.MAXE, max_iter=2)
    n1 = np.asarray(first.mesh.nodes)
    assert first.adapt_history[0]["marked"] >= 2 and -0.875 in n1 and 0.875 in n1
    s = pkg.FEMLSSVRPrimalSolver(mesh=np.linspace(-1, 1, proto.NE0 + 1), **kw)
    s.solve_adaptive(theta=proto.THETA, max_elements=proto.MAXE)
    ne = len(s.fem_nodes) - 1
    assert ne <= proto.MAXE and s.enhanced.n_fallback == 0
    err = float(np.max(np.abs(s.evaluate_solution(xq) - pr.peak_u(xq))))
    u = pkg.FEMLSSVRPrimalSolver(mesh=np.linspace(-1, 1, ne + 1), **kw)
    u.solve()
    err_u = float(np.max(np.abs(u.evaluate_solution(xq) - pr.peak_u(xq))))
    _, err_p, err_pu, _ = proto.run()
    note("adaptive periodic: max error", err, min(err_u, 2.0 * err_p))
    note("adaptive periodic: uniform mesh with the same element count", err_u)
    note("adaptive periodic: prototype", err_p)
    print(f"adaptive: {ne} elements, error {err:.3e}; uniform {err_u:.3e}; prototype {err_p:.3e} (uniform {err_pu:.3e})")
    assert err < err_u
    assert err <= 2.0 * err_p


def test_adaptive_hp_peak_on_the_seam(dev, note):
    """The same problem with solve_adaptive(mode="hp"), every element starting at degree 8: the first round refines
    both end elements (bisected or raised), the final max error on 2001 points is below that of the uniform periodic
    solve of degree 8 with the same element count and within 2 x what the prototype's hp run reaches; no fallback
    element.  The degree groups run through the table kernels (the reaction rows), not lssvr_enhance_subset."""
    import hybrid_fem_lssvr_amd as pkg
    proto = _proto()
    kw = dict(lssvr_M=proto.M, lssvr_gamma=proto.GAMMA, n_colloc=proto.N, nquad=proto.NQUAD, rhs=pr.peak_f,
              global_domain=(-1, 1), reaction=pr._one, boundary="periodic")
    hp = dict(mode="hp", theta=proto.THETA, max_elements=proto.MAXE, sigma_min=proto.SIGMA_MIN, dM=proto.DM,
              M_max=proto.M_MAX)
    xq = np.linspace(-1.0, 1.0, 2001)
    first = pkg.FEMLSSVRPrimalSolver(mesh=np.linspace(-1, 1, proto.NE0 + 1), **kw)
    first.solve_adaptive(max_iter=2, **hp)
    n1, d1 = np.asarray(first.mesh.nodes), np.asarray(first.element_degrees)
    rec = first.adapt_history[0]
    assert rec["marked"] + rec["raised"] >= 2
    assert (-0.875 in n1 or d1[0] > proto.M) and (0.875 in n1 or d1[-1] > proto.M)
    s = pkg.FEMLSSVRPrimalSolver(mesh=np.linspace(-1, 1, proto.NE0 + 1), **kw)
    s.solve_adaptive(max_iter=proto.MAX_ITER, **hp)
    ne = len(s.fem_nodes) - 1
    deg = np.asarray(s.element_degrees)
    assert ne <= proto.MAXE and deg.shape == (ne,) and s.enhanced.n_fallback == 0
    assert s.fem_values[0] == s.fem_values[-1]
    err = float(np.max(np.abs(s.evaluate_solution(xq) - pr.peak_u(xq))))
    u = pkg.FEMLSSVRPrimalSolver(mesh=np.linspace(-1, 1, ne + 1), **kw)
    u.solve()
    err_u = float(np.max(np.abs(u.evaluate_solution(xq) - pr.peak_u(xq))))
    _, deg_p, err_p, err_pu, _ = proto.run_hp()
    note("adaptive periodic hp: max error", err, min(err_u, 2.0 * err_p))
    note("adaptive periodic hp: uniform mesh with the same element count", err_u)
    note("adaptive periodic hp: prototype", err_p)
    print(f"adaptive hp: {ne} elements, degrees {deg.min()}..{deg.max()}, sum M {deg.sum()}, error {err:.3e}; uniform "
          f"{err_u:.3e}; prototype {err_p:.3e} ({len(deg_p)} elements, sum M {int(deg_p.sum())}, uniform {err_pu:.3e})")
    assert err < err_u
    assert err <= 2.0 * err_p
