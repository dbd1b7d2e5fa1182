"""GPU: the convection term -(a u')' + b u' + c u = f through every layer -- the non-symmetric P1 assembly and the
unpivoted tridiagonal solve against their numpy restatement (tests/convection_rules.py), the enhancement and indicator
kernels with the folded table a' - b against the oracle, and the facade's ``convection`` keyword through solve /
solve_many / solve_adaptive."""
import math

import numpy as np
import pytest

import convection_rules as cr
from oracle import closed_form_mp as cf
from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu

GAMMA = 1e4


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


# ---------------------------------------------------------------------------
# 1. assembly
# ---------------------------------------------------------------------------
def _mesh(ne, nquad):
    rng = np.random.default_rng(1000 * ne + nquad)
    h = rng.uniform(0.5, 1.5, ne)
    return np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])


# b = amp * shape with amp = 0.4 / mean h: |shape| <= 1.3, a >= 1 and h <= 1.5 mean h keep the cell Peclet number
# below 0.39, so the convection part is a sizeable share of every band entry and no entry is a difference of nearly
# equal numbers
B_SHAPES = {"pos": lambda x: 1.0 + 0.3 * np.sin(2.0 * x), "neg": lambda x: -1.0 + 0.3 * np.cos(3.0 * x),
            "change": lambda x: np.sin(2.5 * x + 0.4)}


@pytest.mark.parametrize("shape", ["pos", "neg", "change"])
@pytest.mark.parametrize("nquad", [2, 3, 5])
@pytest.mark.parametrize("ne", [1, 37, 255, 256, 257, 5000])
def test_p1_assemble_conv_vs_restatement(dev, ne, nquad, shape):
    from hybrid_fem_lssvr_amd import ops
    nodes = _mesh(ne, nquad)
    amp = 0.4 * ne / 2.0
    b = lambda x: amp * B_SHAPES[shape](np.asarray(x, dtype=np.float64))          # noqa: E731
    assert cr.cell_peclet(nodes, cr.man_a, b, nquad).max() <= 0.5
    x = _t(nodes, dev)
    xq = ops.quad_points(x, nquad).cpu().numpy()
    fq, aq, cq, bq = (_t(fn(xq), dev) for fn in (cr.man_f, cr.man_a, cr.man_c, b))
    got = ops.p1_assemble(x, nquad, rhs_quad=fq, a_quad=aq, c_quad=cq, b_quad=bq, want_local=True)
    assert "off" not in got
    diag, sub, sup, load, kloc = cr.conv_bands(nodes, cr.man_f, cr.man_a, b, cr.man_c, nquad)
    np.testing.assert_allclose(got["diag"].cpu().numpy(), diag, rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["sub"].cpu().numpy(), sub, rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["sup"].cpu().numpy(), sup, rtol=1e-13, atol=0)
    np.testing.assert_allclose(got["load"].cpu().numpy(), load, rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(got["kloc"].cpu().numpy(), kloc, rtol=1e-15, atol=0)
    # the convection part on its own: sup - sub = beta0 + beta1 = the quadrature mean of b
    b0, b1 = cr.conv_halves(nodes, b, nquad)
    # (a difference of two entries of size k = abar / h: absolute bar at rounding level of the largest k)
    np.testing.assert_allclose((got["sup"] - got["sub"]).cpu().numpy(), b0 + b1, rtol=0, atol=1e-13 * kloc.max())
    # repeatable
    again = ops.p1_assemble(x, nquad, rhs_quad=fq, a_quad=aq, c_quad=cq, b_quad=bq, want_local=True)
    for key in ("diag", "sub", "sup", "load", "kloc", "floc"):
        assert np.array_equal(again[key].cpu().numpy(), got[key].cpu().numpy()), key


@pytest.mark.parametrize("nquad", [2, 3, 5])
@pytest.mark.parametrize("ne", [1, 37, 255, 256, 257, 5000])
def test_p1_assemble_conv_without_b_is_react_bit_for_bit(dev, ne, nquad):
    """b_quad == NULL at the C entry: sub == sup == off of lssvr_p1_assemble_react, diag, load, kloc and floc its own,
    with and without c_quad and a_quad, for a tabulated and for the in-kernel right-hand side."""
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    lib = _capi.load()
    nodes = _mesh(ne, nquad)
    x = _t(nodes, dev)
    xq = ops.quad_points(x, nquad).cpu().numpy()
    fq, aq, cq = (_t(fn(xq), dev) for fn in (cr.man_f, cr.man_a, cr.man_c))
    for a_quad, c_quad, rhs_quad in ((aq, cq, fq), (aq, None, fq), (None, cq, fq), (None, None, None)):
        kw = {} if rhs_quad is None else {"rhs_quad": rhs_quad}
        ref = ops.p1_assemble(x, nquad, a_quad=a_quad, c_quad=c_quad, want_local=True, **kw)
        out = {k: torch.full_like(ref[k], -777.0) for k in ("diag", "load", "kloc", "floc")}
        out["sub"], out["sup"] = torch.full_like(ref["off"], -777.0), torch.full_like(ref["off"], -777.0)
        ptr = lambda t: None if t is None else t.data_ptr()                      # noqa: E731
        rc = lib.lssvr_p1_assemble_conv(ptr(x), ne, nquad, _capi.RHS_SIN if rhs_quad is None else _capi.RHS_ARRAY,
                                        _capi.rhs_params(ops.POISSON_AMP, ops.POISSON_OMEGA), ptr(rhs_quad),
                                        ptr(a_quad), ptr(c_quad), None, ptr(out["diag"]), ptr(out["sub"]),
                                        ptr(out["sup"]), ptr(out["load"]), ptr(out["kloc"]), ptr(out["floc"]),
                                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.lssvr_last_error()
        for key, want in (("diag", "diag"), ("sub", "off"), ("sup", "off"), ("load", "load"), ("kloc", "kloc"),
                          ("floc", "floc")):
            assert np.array_equal(out[key].cpu().numpy(), ref[want].cpu().numpy()), (key, a_quad is None,
                                                                                   c_quad is None)


# ---------------------------------------------------------------------------
# 2. non-symmetric solve
# ---------------------------------------------------------------------------
# The bars of test_tridiag_dirichlet_solve (tests/test_gpu_fem_eval.py), copied as numbers; a size between two listed
# ones takes the bar of the next listed size.
TRIDIAG_FORWARD_BAR = {1: 0.0, 2: 1e-15, 3: 1e-15, 24: 1e-14, 511: 2.5e-12, 512: 2.5e-12, 513: 2.5e-12,
                       514: 2.5e-12, 1025: 4e-12, 16385: 2e-9, 100000: 7e-8, 1234567: 2e-6}
NS_SIZES = [1, 2, 3, 9, 24, 511, 512, 513, 514, 4097, 100000]
# max cell Peclet 0 (no b: one case) and 0.5, 0.95 for b > 0, b < 0 and b changing sign
NS_CASES = [(0.0, "pos")] + [(pe, sh) for pe in (0.5, 0.95) for sh in ("pos", "neg", "change")]


def _forward_bar(ne):
    return TRIDIAG_FORWARD_BAR[min(k for k in TRIDIAG_FORWARD_BAR if k >= ne)]


@pytest.mark.parametrize("peclet,shape", NS_CASES)
@pytest.mark.parametrize("ne", NS_SIZES)
def test_tridiag_ns_dirichlet_solve(dev, note, ne, peclet, shape):
    """End values exact; residual at rounding level of |A| |u| (the bar of test_tridiag_dirichlet_solve); forward error
    against the long-double Thomas solve within max(10 x LAPACK's own distance from it, the symmetric solver's bar).
    Measured on an MI355X (largest of the seven cases per size, relative to max |u|; LAPACK's own distance beside it):
    0 (1), 5e-17 (2), 1e-16 (3), 3.5e-16 (9), 3.7e-16 (24), 4.9e-14 (511; LAPACK 7.8e-14), 4.6e-14 (512), 1.2e-13
    (513), 3.6e-13 (514), 1.3e-12 (4097; LAPACK 1.1e-12), 4.6e-9 (100000; LAPACK 9.9e-11) -- from three elements on the
    Peclet-0 case; the residual is at most 0.001 of its bar everywhere."""
    from hybrid_fem_lssvr_amd import ops
    (diag, sub, sup, load), u_ld, u_la = cr.peclet_case(ne, peclet, shape)
    u = ops.tridiag_ns_dirichlet_solve(_t(diag, dev), _t(sub, dev), _t(sup, dev), _t(load, dev), 0.25,
                                       -0.5).cpu().numpy()
    assert u.shape == (ne + 1,) and u[0] == 0.25 and u[-1] == -0.5
    scale = float(np.max(np.abs(u_ld)))
    if ne > 1:
        r = diag[1:-1] * u[1:-1] + sub[:-1] * u[:-2] + sup[1:] * u[2:] - load[1:-1]
        res, res_bar = np.max(np.abs(r)), 1e-13 * np.max(np.abs(diag)) * scale * max(1.0, np.log2(ne))
        note(f"tridiag_ns ne={ne} Pe={peclet} {shape}: residual", res, res_bar)
        print(f"ne={ne} Pe={peclet} {shape}: residual {res:.2e} (bar {res_bar:.2e})")
        assert res <= res_bar
    lapack = float(np.max(np.abs(u_la.astype(np.longdouble) - u_ld)))
    fwd = float(np.max(np.abs(u.astype(np.longdouble) - u_ld)))
    bar = max(10.0 * lapack, _forward_bar(ne)) * scale
    note(f"tridiag_ns ne={ne} Pe={peclet} {shape}: forward error (LAPACK {lapack:.1e})", fwd, bar)
    print(f"ne={ne} Pe={peclet} {shape}: forward {fwd:.2e}, LAPACK {lapack:.2e}, bar {bar:.2e}")
    assert fwd <= bar


@pytest.mark.parametrize("ne", NS_SIZES)
def test_tridiag_ns_on_symmetric_bands_and_repeatable(dev, note, ne):
    """sub == sup from the symmetric assembly: within the same bars of ops.tridiag_dirichlet_solve; a second call is
    bit-equal to the first."""
    from hybrid_fem_lssvr_amd import ops
    nodes = np.linspace(-1, 1, ne + 1)
    diag, off, load, _ = orc.p1_bands(nodes)
    d, o, l = _t(diag, dev), _t(off, dev), _t(load, dev)
    u_sym = ops.tridiag_dirichlet_solve(d, o, l, 0.25, -0.5).cpu().numpy()
    u1 = ops.tridiag_ns_dirichlet_solve(d, o, o.clone(), l, 0.25, -0.5).cpu().numpy()
    u2 = ops.tridiag_ns_dirichlet_solve(d, o, o.clone(), l, 0.25, -0.5).cpu().numpy()
    assert np.array_equal(u1, u2)
    u_ld = cr.thomas_ns_ld(diag, off, off, load, 0.25, -0.5)
    u_la = cr.banded_ns(diag, off, off, load, 0.25, -0.5)
    scale = float(np.max(np.abs(u_ld)))
    lapack = float(np.max(np.abs(u_la.astype(np.longdouble) - u_ld)))
    bar = max(10.0 * lapack, _forward_bar(ne)) * scale
    diff = float(np.max(np.abs(u1 - u_sym)))
    note(f"tridiag_ns vs tridiag ne={ne}: max difference", diff, bar)
    note(f"tridiag_ns vs tridiag ne={ne}: bit for bit (1 = yes)", float(np.array_equal(u1, u_sym)))
    assert diff <= bar


def test_tridiag_ns_rejects_wrong_sizes(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    z = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)                # noqa: E731
    for sizes in ((6, 5, 4, 6), (5, 5, 5, 6), (6, 5, 5, 5)):
        with pytest.raises(ValueError, match="band lengths"):
            ops.tridiag_ns_dirichlet_solve(*(z(n) for n in sizes))
    with pytest.raises(ValueError, match="out must hold"):
        ops.tridiag_ns_dirichlet_solve(z(6), z(5), z(5), z(6), out=z(5))
    with pytest.raises(ValueError, match="b_quad"):
        ops.p1_assemble(z(6), 2, b_quad=z(9))


# ---------------------------------------------------------------------------
# 3. enhancement: b_values given
# ---------------------------------------------------------------------------
def _enh_b(x):
    return 3.0 * (1.0 + 0.5 * np.asarray(x, dtype=np.float64))


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("ne,M,n", [(65, 9, 16), (129, 16, 24), (65, 17, 24), (33, 26, 40)])
def test_enhance_with_b_values(dev, note, ne, M, n, with_c):
    """b_values: bit for bit the call with the pre-subtracted table; 1e-13 from the 60-digit minimiser with
    coef_da = a' - b on elements 0, ne/3, ne-1; 1e-11 (1e-10 above M = 22) from the float64 restatement -- the bars of
    tests/test_gpu_react.py -- in both table layouts."""
    from hybrid_fem_lssvr_amd import ops
    a, da, c, f = orc.react_functions(1.0)
    c = c if with_c else None
    folded = lambda x: da(x) - _enh_b(x)                                          # noqa: E731
    nodes = np.linspace(-1, 1, ne + 1)
    values = np.sin(np.pi * nodes)
    Wo = orc.enhance_all(nodes, values, M, GAMMA, n, rhs=f, coef_a=a, coef_da=folded, coef_c=c)[0]
    sel = [0, ne // 3, ne - 1]
    tr = (cf.truth_all(nodes, values, M, GAMMA, n, f, elements=sel, coef_a=a, coef_da=folded, coef_c=c)
          if cf.HAVE_MP else None)
    x, u = _t(nodes, dev), _t(values, dev)
    xc = ops.colloc_points(x, n).cpu().numpy()
    bar = 1e-11 if M <= 22 else 1e-10
    for pm in (False, True):
        def tab(fn):
            return None if fn is None else _t(np.asarray(fn(xc), dtype=np.float64).T if pm else fn(xc), dev)
        ta, tda, tf, tc, tb = tab(a), tab(da), tab(f), tab(c), tab(_enh_b)
        W, st = ops.enhance_varcoef(x, u, M, GAMMA, n, ta, tda, tf, point_major=pm, c_values=tc, b_values=tb,
                                    global_domain=(-1.0, 1.0))
        W0, st0 = ops.enhance_varcoef(x, u, M, GAMMA, n, ta, tda - tb, tf, point_major=pm, c_values=tc,
                                      global_domain=(-1.0, 1.0))
        W, W0 = W.cpu().numpy(), W0.cpu().numpy()
        assert np.all(st.cpu().numpy() == 0) and np.array_equal(W, W0)
        Wn, _ = ops.enhance_varcoef(x, u, M, GAMMA, n, ta, tda, tf, point_major=pm, c_values=tc,
                                    global_domain=(-1.0, 1.0))
        assert not np.array_equal(W, Wn.cpu().numpy())                           # b is not ignored
        e64 = orc.rel_l2_coef(W, Wo).max()
        note(f"conv enhance ne={ne} M={M} c={with_c} pm={pm} vs float64", e64, bar)
        assert e64 <= bar
        if tr is not None:
            emp = orc.rel_l2_coef(W[sel], tr).max()
            note(f"conv enhance ne={ne} M={M} c={with_c} pm={pm} vs 60 digits", emp, 1e-13)
            assert emp <= 1e-13
        # several load cases: the same fold
        U = _t(np.stack([values, 0.5 * values]), dev)
        TF = _t(np.stack([tf.cpu().numpy(), 2.0 * tf.cpu().numpy()]), dev)
        Wm, _ = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda, TF, c_values=tc, b_values=tb, point_major=pm,
                                  global_domain=(-1.0, 1.0))
        Wm0, _ = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda - tb, TF, c_values=tc, point_major=pm,
                                   global_domain=(-1.0, 1.0))
        assert np.array_equal(Wm.cpu().numpy(), Wm0.cpu().numpy())
        assert orc.rel_l2_coef(Wm[0].cpu().numpy(), Wo).max() <= bar


def test_b_values_must_match_da_values(dev):
    from hybrid_fem_lssvr_amd import ops
    nodes = np.linspace(-1, 1, 11)
    x, u = _t(nodes, dev), _t(np.sin(nodes), dev)
    tab = _t(np.ones((10, 16)), dev)
    with pytest.raises(ValueError, match="b_values"):
        ops.enhance_varcoef(x, u, 9, GAMMA, 16, tab, tab, tab, b_values=_t(np.ones((16, 10)), dev))
    with pytest.raises(TypeError, match="b_values"):
        ops.enhance_varcoef(x, u, 9, GAMMA, 16, tab, tab, tab, b_values=np.ones((10, 16)))


# ---------------------------------------------------------------------------
# 4. indicator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [4, 16])
@pytest.mark.parametrize("M", [9, 22, 33])
def test_estimate_with_b_values_vs_numpy(dev, M, nq):
    """ops.estimate_varcoef(b_values=...) against orc.estimate_indicator(da = a' - b), 1e-12 relative (the bar of
    test_estimate_react_vs_numpy), with and without c, both layouts; bit for bit the pre-subtracted call."""
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(3000 * M + nq)
    for ne in (1, 129, 3001):
        h = rng.uniform(0.3, 1.7, ne)
        x = np.concatenate([[-3.0], -3.0 + 6.0 * np.cumsum(h) / h.sum()])
        W = rng.standard_normal((ne, M)) / (1.0 + np.arange(M)) ** 2
        xi, wt = ops.gauss_rule(nq)
        xq = orc.estimate_points(x, xi)
        a, da = 1.0 + 0.5 * np.sin(1.3 * xq), 0.65 * np.cos(1.3 * xq)
        b = 2.0 * np.cos(0.9 * xq) + 0.5
        c, f = 3.0 + 2.0 * np.cos(0.7 * xq), 2.5 * np.sin(1.7 * xq) + 0.3
        a_ends = rng.uniform(0.5, 1.5, (ne, 2))
        for cc in (c, None):
            ref = orc.estimate_indicator(x, W, xi, wt, f, a, da - b, cc, a_ends)[0]
            for pm in (False, True):
                tab = lambda t: None if t is None else _t(t.T if pm else t, dev)  # noqa: E731
                args = (_t(x, dev), _t(W, dev), nq, tab(a))
                eta2, _, o3 = ops.estimate_varcoef(*args, tab(da), tab(f), _t(a_ends, dev), point_major=pm,
                                                   c_values=tab(cc), b_values=tab(b))
                eta0, _, o30 = ops.estimate_varcoef(*args, tab(da - b), tab(f), _t(a_ends, dev), point_major=pm,
                                                    c_values=tab(cc))
                eta2 = eta2.cpu().numpy()
                assert np.array_equal(eta2, eta0.cpu().numpy()) and np.array_equal(o3.cpu().numpy(), o30.cpu().numpy())
                assert np.all(np.abs(eta2 - ref) <= 1e-12 * np.abs(ref) + 1e-300), np.max(np.abs(eta2 - ref) / ref)
                s = math.fsum(eta2.tolist())
                o3 = o3.cpu().numpy()
                assert o3[2] == 0.0 and o3[1] == np.max(eta2) and abs(o3[0] - s) <= 1e-14 * s


# ---------------------------------------------------------------------------
# 5. facade
# ---------------------------------------------------------------------------
def _man_solver(ne, M, n, **kw):
    import hybrid_fem_lssvr_amd as pkg
    kw.setdefault("rhs", cr.man_f)
    kw.setdefault("convection", cr.man_b)
    return pkg.FEMLSSVRPrimalSolver(ne + 1, lssvr_M=M, lssvr_gamma=GAMMA, n_colloc=n, nquad=3,
                                    coef=(cr.man_a, cr.man_da), reaction=cr.man_c, **kw)


@pytest.mark.parametrize("M,n", [(9, 16), (20, 32)])
@pytest.mark.parametrize("ne", [200, 60])
def test_facade_solve_with_convection(dev, note, ne, M, n):
    """Manufactured u = sin(pi x) on (-1, 1): fem_values within 1e-12 of the helper's banded solve, and the L2 error of
    solve() within 1e-10 ||u|| of the numpy restatement of the whole pipeline."""
    s = _man_solver(ne, M, n)
    s.solve()
    nodes = np.linspace(-1, 1, ne + 1)
    uo = cr.fem_solve(nodes, cr.man_f, cr.man_a, cr.man_b, cr.man_c, 3)
    assert np.max(np.abs(s.fem_values - uo)) <= 1e-12
    assert set(s.bands) >= {"diag", "sub", "sup", "load"} and "off" not in s.bands
    Wo = orc.enhance_all(nodes, uo, M, GAMMA, n, rhs=cr.man_f, coef_a=cr.man_a, coef_da=cr.man_folded,
                         coef_c=cr.man_c)[0]
    xq = np.linspace(-1, 1, 4001)
    ex = cr.man_u(xq)
    e_gpu = np.linalg.norm(s.evaluate_solution(xq) - ex)
    e_ref = np.linalg.norm(orc.evaluate_solution_vec(nodes, Wo, xq)[0] - ex)
    note(f"facade conv ne={ne} M={M}: |L2 err - restatement| / ||u||", abs(e_gpu - e_ref) / np.linalg.norm(ex), 1e-10)
    assert abs(e_gpu - e_ref) <= 1e-10 * np.linalg.norm(ex)
    assert np.all(s.enhanced.status.cpu().numpy() == 0)
    # the indicator runs and is finite
    eta2 = s.estimate()
    assert eta2.shape == (ne,) and np.all(np.isfinite(eta2)) and np.all(eta2 >= 0)


def test_facade_without_convection_is_the_old_path(dev):
    """convection=None: the same nodal values and W as the solver without the keyword, and as the direct ops calls
    on the same inputs, bit for bit."""
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    s0 = _man_solver(120, 9, 16, convection=None)
    s0.solve()
    s1 = pkg.FEMLSSVRPrimalSolver(121, lssvr_M=9, lssvr_gamma=GAMMA, n_colloc=16, nquad=3, rhs=cr.man_f,
                                  coef=(cr.man_a, cr.man_da), reaction=cr.man_c)
    s1.solve()
    assert np.array_equal(s0.fem_values, s1.fem_values)
    assert np.array_equal(s0.enhanced.W.cpu().numpy(), s1.enhanced.W.cpu().numpy())
    assert "off" in s0.bands and "sub" not in s0.bands
    x = _t(s0.fem_nodes, dev)
    xq = ops.quad_points(x, 3).cpu().numpy()
    b = ops.p1_assemble(x, 3, rhs_quad=_t(cr.man_f(xq), dev), a_quad=_t(cr.man_a(xq), dev),
                        c_quad=_t(cr.man_c(xq), dev))
    u = ops.tridiag_dirichlet_solve(b["diag"], b["off"], b["load"], 0.0, 0.0)
    assert np.array_equal(u.cpu().numpy(), s0.fem_values)
    xc = ops.colloc_points(x, 16).cpu().numpy()
    tabs = [_t(np.asarray(fn(xc)).T, dev) for fn in (cr.man_a, cr.man_da, cr.man_f, cr.man_c)]
    W, _ = ops.enhance_varcoef(x, u, 9, GAMMA, 16, *tabs[:3], point_major=True, c_values=tabs[3],
                               global_domain=(-1.0, 1.0))
    assert np.array_equal(W.cpu().numpy(), s0.enhanced.W.cpu().numpy())


def test_facade_refuses_peclet_above_one(dev):
    """h = 0.2, b = 1, a = h/3: cell Peclet 1.5 -- refused with the number and the worst element, nothing solved."""
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(11, lssvr_M=9, n_colloc=16, rhs=lambda x: 1.0 + 0.0 * x,
                                 coef=(lambda x: 0.2 / 3.0 + 0.0 * x, lambda x: 0.0 * x),
                                 convection=lambda x: 1.0 + 0.0 * x)
    with pytest.raises(ValueError, match=r"Peclet number .* = 1\.5 > 1 on element \d+"):
        s.solve()
    assert s.fem_values is None and s.enhanced is None
    # the worst element is named: refine only the right half, the left half still fails
    s.mesh = pkg.mesh.LineMesh.from_nodes(np.concatenate([np.linspace(-1, 0, 6), np.linspace(0, 1, 11)[1:]]))
    with pytest.raises(ValueError, match=r"on element [0-4] "):
        s.solve_fem()
    s.mesh = pkg.mesh.LineMesh.from_nodes(np.linspace(-1, 1, 21))
    s.solve_fem()                                                                # Peclet 0.75


def test_facade_solve_many_with_convection(dev):
    """Two right-hand sides in one call equal two single solves to 1e-12 relative."""
    f2 = lambda x: np.cos(2.0 * x) + 0.5                                        # noqa: E731
    s = _man_solver(90, 9, 16)
    sols = s.solve_many([cr.man_f, f2])
    assert len(sols) == 2 and s.enhanced is None
    for sol, f in zip(sols, (cr.man_f, f2)):
        one = _man_solver(90, 9, 16, rhs=f)
        one.solve()
        W1 = one.enhanced.W.cpu().numpy()
        assert np.all(sol.status.cpu().numpy() == 0)
        assert orc.rel_l2_coef(sol.W.cpu().numpy(), W1).max() <= 1e-12


# ---------------------------------------------------------------------------
# 6. adaptivity on the outflow boundary layer of -eps u'' + u' = 1
# ---------------------------------------------------------------------------
# numpy prototype of the same loop on the restatement (scripts/proto/conv_adapt.py): 127 elements, max error 6.448e-5
# against 4.757e-3 on 127 uniform elements
PROTO_RATIO = 73.78
PROTO_NE = 127


def _layer_solver(nodes):
    import hybrid_fem_lssvr_amd as pkg
    return pkg.FEMLSSVRPrimalSolver(len(nodes), lssvr_M=9, lssvr_gamma=1e10, n_colloc=16, nquad=5, rhs=cr.layer_f,
                                    mesh=nodes, global_domain=(0, 1), coef=(cr.layer_a, cr.layer_da),
                                    convection=cr.layer_b)


def test_adaptive_outflow_layer(dev, note):
    """-eps u'' + u' = 1 on (0, 1), u(0) = u(1) = 0, eps = 0.02, 32 uniform elements to start (cell Peclet 0.78):
    solve_adaptive(max_elements=128) refines towards the outflow layer at x = 1, and the adapted mesh beats the
    uniform mesh with the same element count in the max norm on 20 001 points by at least the prototype's ratio / 10.
    Prototype (scripts/proto/conv_adapt.py): 127 elements, ratio 73.78, so the bar is 7.378."""
    xq = np.linspace(0, 1, 20001)
    ex = cr.layer_exact(xq)
    s = _layer_solver(np.linspace(0, 1, 33))
    s.solve_adaptive(theta=0.5, max_elements=128)
    nodes = np.asarray(s.fem_nodes)
    ne = len(nodes) - 1
    err_a = np.max(np.abs(s.evaluate_solution(xq) - ex))
    u = _layer_solver(np.linspace(0, 1, ne + 1))
    u.solve()
    err_u = np.max(np.abs(u.evaluate_solution(xq) - ex))
    ratio = err_u / err_a
    note("adaptive outflow layer: elements", ne)
    note("adaptive outflow layer: uniform max error", err_u)
    note("adaptive outflow layer: adapted max error", err_a)
    note("adaptive outflow layer: ratio (prototype %.4g on %d elements)" % (PROTO_RATIO, PROTO_NE), ratio,
         PROTO_RATIO / 10.0)
    print(f"adapted ne={ne} err {err_a:.3e}, uniform-{ne} err {err_u:.3e}, ratio {ratio:.4g}")
    assert 32 < ne <= 128
    h = np.diff(nodes)
    mid = 0.5 * (nodes[1:] + nodes[:-1])
    # refined towards x = 1: most elements sit in the last quarter, the smallest ones inside the layer (a few eps
    # wide), and the inflow half keeps elements at least 16 times longer
    assert np.sum(nodes[:-1] >= 0.75) > ne / 2
    assert mid[np.argmin(h)] > 1.0 - 5.0 * cr.LAYER_EPS
    assert h[mid < 0.5].min() >= 16 * h.min()
    assert ratio >= PROTO_RATIO / 10.0
