"""GPU: the reaction term -(a u')' + c u = f through every layer -- enhancement kernels (lane and MFMA) against the
float64 restatement (oracle/lssvr_oracle.py, ``coef_c``) and its 60-digit solve, the P1 bands with the mass matrix, the
indicator, and the facade's ``reaction`` keyword through solve / estimate / solve_adaptive."""
import math

import numpy as np
import pytest

from oracle import closed_form_mp as cf
from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu

GAMMA = 1e4
SIZES = [(2000, 9, 16), (300, 20, 32), (100, 26, 40), (25, 9, 16)]      # (ne, M, n)
KS = [1.0, 1e4]


def _oracle_W(nodes, values, M, n, a, da, c, f, **kw):
    return orc.enhance_all(nodes, values, M, GAMMA, n, rhs=f, coef_a=a, coef_da=da, coef_c=c, **kw)[0]


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _tables(x, n, funcs, pm, dev):
    from hybrid_fem_lssvr_amd import ops
    xc = ops.colloc_points(x, n).cpu().numpy()
    return [_t(np.asarray(fn(xc), dtype=np.float64).T if pm else fn(xc), dev) for fn in funcs]


def _enhance(dev, nodes, values, M, n, a, da, c, f, pm, **kw):
    from hybrid_fem_lssvr_amd import ops
    x = _t(nodes, dev)
    ta, tda, tf, tc = _tables(x, n, (a, da, f, c), pm, dev)
    kw.setdefault("global_domain", (float(nodes[0]), float(nodes[-1])))
    W, st = ops.enhance_varcoef(x, _t(values, dev), M, GAMMA, n, ta, tda, tf, point_major=pm, c_values=tc, **kw)
    return W.cpu().numpy(), st.cpu().numpy()


# ---------------------------------------------------------------------------
# 1. enhancement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ne,M,n", SIZES)
def test_enhance_react_vs_restatement_and_60_digits(dev, note, ne, M, n, k):
    """1e-11 against the float64 restatement (1e-10 above M = 22, as the project has it), 1e-13 against the
    60-digit minimiser on elements 0, ne/3, ne-1, both table layouts, which agree to 1e-12."""
    a, da, c, f = orc.react_functions(k)
    nodes = np.linspace(-1, 1, ne + 1)
    values = np.sin(np.pi * nodes)
    Wo = _oracle_W(nodes, values, M, n, a, da, c, f)
    sel = [0, ne // 3, ne - 1]
    tr = (cf.truth_all(nodes, values, M, GAMMA, n, f, elements=sel, coef_a=a, coef_da=da, coef_c=c)
          if cf.HAVE_MP else None)
    got = {}
    for pm in (False, True):
        W, st = _enhance(dev, nodes, values, M, n, a, da, c, f, pm)
        got[pm] = W
        assert np.all(st == 0)
        e64 = orc.rel_l2_coef(W, Wo).max()
        note(f"react ne={ne} M={M} k={k:g} pm={pm} vs float64", e64, 1e-11 if M <= 22 else 1e-10)
        print(f"ne={ne} M={M} n={n} k={k:g} pm={pm}: vs float64 {e64:.2e}")
        if tr is not None:
            emp = orc.rel_l2_coef(W[sel], tr).max()
            note(f"react ne={ne} M={M} k={k:g} pm={pm} vs 60 digits", emp, 1e-13)
            print(f"    vs 60 digits {emp:.2e}")
        assert e64 <= (1e-11 if M <= 22 else 1e-10)
        if tr is not None:
            assert emp <= 1e-13
    assert orc.rel_l2_coef(got[True], got[False]).max() <= 1e-12


@pytest.mark.parametrize("ne,M,n", SIZES)
def test_enhance_react_with_zero_c_is_varcoef(dev, note, ne, M, n):
    from hybrid_fem_lssvr_amd import ops
    a, da, _, _ = orc.react_functions(1.0)
    f = orc.varcoef_functions(*orc.varcoef_params())[2]
    nodes = np.linspace(-1, 1, ne + 1)
    values = np.sin(np.pi * nodes)
    for pm in (False, True):
        W, st = _enhance(dev, nodes, values, M, n, a, da, lambda x: 0.0 * x, f, pm)
        x = _t(nodes, dev)
        ta, tda, tf = _tables(x, n, (a, da, f), pm, dev)
        W0, st0 = ops.enhance_varcoef(x, _t(values, dev), M, GAMMA, n, ta, tda, tf, point_major=pm,
                                      global_domain=(-1.0, 1.0))
        W0 = W0.cpu().numpy()
        assert np.all(st == 0) and np.all(st0.cpu().numpy() == 0)
        err = orc.rel_l2_coef(W, W0).max()
        note(f"react c=0 vs varcoef ne={ne} M={M} pm={pm}", err, 1e-12)
        note(f"react c=0 vs varcoef ne={ne} M={M} pm={pm} bit for bit (1 = yes)", float(np.array_equal(W, W0)))
        assert err <= 1e-12


@pytest.mark.parametrize("M,n", [(9, 16), (16, 24), (17, 24), (26, 40)])
@pytest.mark.parametrize("ne", [1, 63, 65, 129, 257])
def test_enhance_react_odd_sizes_and_shard(dev, ne, M, n):
    """Element counts off the wave / workgroup multiples, as a shard of a larger mesh (elem_offset > 0,
    ne_global > ne: no end element is a global-boundary one)."""
    a, da, c, f = orc.react_functions(1e4)
    nodes = np.linspace(-0.7, 0.9, ne + 1)
    values = np.sin(np.pi * nodes)
    bar = 1e-11 if M <= 22 else 1e-10
    for pm in (False, True):
        W, st = _enhance(dev, nodes, values, M, n, a, da, c, f, pm)
        assert np.all(st == 0)
        Wo = _oracle_W(nodes, values, M, n, a, da, c, f)
        assert orc.rel_l2_coef(W, Wo).max() <= bar
        # shard: the same elements as the interior of a mesh of ne + 5 elements; the Dirichlet values do not apply
        W, st = _enhance(dev, nodes, values, M, n, a, da, c, f, pm, elem_offset=3, ne_global=ne + 5,
                         global_domain=(-1.0, 1.0), bc=(7.0, -3.0))
        assert np.all(st == 0)
        Wo = _oracle_W(np.concatenate([[-9.0], nodes, [9.0]]), np.concatenate([[0.0], values, [0.0]]), M, n, a, da,
                       c, f, global_domain=(-9.0, 9.0), elements=range(1, ne + 1))
        assert orc.rel_l2_coef(W, Wo).max() <= bar


@pytest.mark.parametrize("M,n", [(9, 16), (20, 32)])
def test_enhance_react_leaves_pad_columns_alone(dev, M, n):
    """``out`` wider than M is not a form of this entry (W is [ne, M]); what must hold is that a caller's buffer
    behind the ne*M doubles is untouched: a sentinel row after the last element survives."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    a, da, c, f = orc.react_functions(1.0)
    ne = 130
    nodes = np.linspace(-1, 1, ne + 1)
    values = np.sin(np.pi * nodes)
    x = _t(nodes, dev)
    for pm in (False, True):
        buf = torch.full(((ne + 2) * M,), -777.0, dtype=torch.float64, device=dev)
        ta, tda, tf, tc = _tables(x, n, (a, da, f, c), pm, dev)
        ops.enhance_varcoef(x, _t(values, dev), M, GAMMA, n, ta, tda, tf, point_major=pm, c_values=tc,
                            out=buf[: ne * M], global_domain=(-1.0, 1.0))
        h = buf.cpu().numpy()
        assert np.all(h[ne * M:] == -777.0) and not np.any(h[: ne * M] == -777.0)


def test_enhance_react_rejects_fewer_points_than_bubbles(dev):
    from hybrid_fem_lssvr_amd import _capi
    a, da, c, f = orc.react_functions(1.0)
    nodes = np.linspace(-1, 1, 11)
    with pytest.raises(_capi.LssvrHipError, match="M-2"):
        _enhance(dev, nodes, np.sin(np.pi * nodes), 22, 19, a, da, c, f, True)


# ---------------------------------------------------------------------------
# 2. P1 bands with the mass matrix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nquad", [2, 3, 5])
@pytest.mark.parametrize("ne", [1, 37, 255, 256, 5000])
def test_p1_assemble_react_vs_restatement(dev, ne, nquad):
    from hybrid_fem_lssvr_amd import ops
    a, da, c, f = orc.react_functions(1e4)
    rng = np.random.default_rng(ne + nquad)
    h = rng.uniform(0.5, 1.5, ne)
    nodes = np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])
    x = _t(nodes, dev)
    xq = ops.quad_points(x, nquad).cpu().numpy()
    fq, aq, cq = _t(f(xq), dev), _t(a(xq), dev), _t(c(xq), dev)
    b = ops.p1_assemble(x, nquad, rhs_quad=fq, a_quad=aq, c_quad=cq, want_local=True)
    diag, off, load, kloc = orc.p1_bands(nodes, f, a, nquad, c)
    np.testing.assert_allclose(b["diag"].cpu().numpy(), diag, rtol=1e-13, atol=0)
    np.testing.assert_allclose(b["off"].cpu().numpy(), off, rtol=1e-13, atol=0)
    np.testing.assert_allclose(b["load"].cpu().numpy(), load, rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(b["kloc"].cpu().numpy(), kloc, rtol=1e-15, atol=0)
    # c_quad = None is the old call, bit for bit
    b0 = ops.p1_assemble(x, nquad, rhs_quad=fq, a_quad=aq, want_local=True)
    b1 = ops.p1_assemble(x, nquad, rhs_quad=fq, a_quad=aq, want_local=True, c_quad=None)
    for key in ("diag", "off", "load", "kloc", "floc"):
        assert np.array_equal(b0[key].cpu().numpy(), b1[key].cpu().numpy()), key
    assert np.array_equal(b0["load"].cpu().numpy(), b["load"].cpu().numpy())
    assert np.array_equal(b0["kloc"].cpu().numpy(), b["kloc"].cpu().numpy())
    # the tridiagonal solve of the new bands
    u = ops.tridiag_dirichlet_solve(b["diag"], b["off"], b["load"], 0.0, 0.0).cpu().numpy()
    uo = orc.thomas_dirichlet(diag, off, load)
    assert np.max(np.abs(u - uo)) <= 1e-12 * max(1.0, np.max(np.abs(uo)))


# ---------------------------------------------------------------------------
# 3. indicator
# ---------------------------------------------------------------------------
def _est_case(rng, ne, M, nq):
    from hybrid_fem_lssvr_amd import ops
    h = rng.uniform(0.3, 1.7, ne)
    x = np.concatenate([[-3.0], -3.0 + 6.0 * np.cumsum(h) / h.sum()])
    W = rng.standard_normal((ne, M)) / (1.0 + np.arange(M)) ** 2
    xi, wt = ops.gauss_rule(nq)
    xq = orc.estimate_points(x, xi)
    a = 1.0 + 0.5 * np.sin(1.3 * xq)
    da = 0.65 * np.cos(1.3 * xq)
    c = 3.0 + 2.0 * np.cos(0.7 * xq)
    f = 2.5 * np.sin(1.7 * xq) + 0.3
    a_ends = rng.uniform(0.5, 1.5, (ne, 2))
    return x, W, xi, wt, a, da, c, f, a_ends


def _run_est(dev, x, W, nq, a, da, c, f, a_ends, pm):
    from hybrid_fem_lssvr_amd import ops
    tabs = [_t(t.T if pm else t, dev) for t in (a, da, f)]
    cv = None if c is None else _t(c.T if pm else c, dev)
    eta2, _, out3 = ops.estimate_varcoef(_t(x, dev), _t(W, dev), nq, *tabs, _t(a_ends, dev), point_major=pm,
                                         c_values=cv)
    return eta2.cpu().numpy(), out3.cpu().numpy()


@pytest.mark.parametrize("nq", [1, 4, 16, 32])
@pytest.mark.parametrize("M", [1, 2, 9, 12, 13, 22, 23, 33])
def test_estimate_react_vs_numpy(dev, M, nq):
    rng = np.random.default_rng(2000 * M + nq)
    for ne in (1, 127, 128, 129, 3001):
        x, W, xi, wt, a, da, c, f, a_ends = _est_case(rng, ne, M, nq)
        ref = orc.estimate_indicator(x, W, xi, wt, f, a, da, c, a_ends)[0]
        for pm in (False, True):
            eta2, o3 = _run_est(dev, x, W, nq, a, da, c, f, a_ends, pm)
            assert np.all(np.abs(eta2 - ref) <= 1e-12 * np.abs(ref) + 1e-300), np.max(np.abs(eta2 - ref) / ref)
            s = math.fsum(eta2.tolist())
            assert o3[2] == 0.0 and o3[1] == np.max(eta2) and abs(o3[0] - s) <= 1e-14 * s


@pytest.mark.parametrize("M,nq,ne", [(9, 16, 3001), (22, 8, 700), (33, 32, 257), (9, 16, 600_001)])
def test_estimate_react_zero_c_and_repeatable(dev, M, nq, ne):
    rng = np.random.default_rng(M + nq + ne)
    x, W, xi, wt, a, da, c, f, a_ends = _est_case(rng, ne, M, nq)
    for pm in (False, True):
        e0, o0 = _run_est(dev, x, W, nq, a, da, None, f, a_ends, pm)
        ez, oz = _run_est(dev, x, W, nq, a, da, np.zeros_like(c), f, a_ends, pm)
        assert np.all(np.abs(ez - e0) <= 1e-14 * np.abs(e0)) and abs(oz[0] - o0[0]) <= 1e-14 * o0[0]
        e1, o1 = _run_est(dev, x, W, nq, a, da, c, f, a_ends, pm)
        e2, o2 = _run_est(dev, x, W, nq, a, da, c, f, a_ends, pm)
        assert np.array_equal(e1, e2) and np.array_equal(o1, o2)
        assert not np.array_equal(e1, e0)


# ---------------------------------------------------------------------------
# 4. facade
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ne,M,n", [(200, 9, 16), (60, 20, 32), (40, 26, 40)])
def test_facade_solve_with_coef_and_reaction(dev, note, ne, M, n):
    """Manufactured u = sin(pi x): the L2 error of solve() is that of the numpy restatement of the whole pipeline
    (P1 with mass matrix -> Thomas -> per-element solve) within 1e-10 ||u||."""
    import hybrid_fem_lssvr_amd as pkg
    a, da, c, f = orc.react_functions(1e4)
    s = pkg.FEMLSSVRPrimalSolver(ne + 1, lssvr_M=M, lssvr_gamma=GAMMA, n_colloc=n, rhs=f, nquad=3,
                                 coef=(a, da), reaction=c)
    s.solve()
    nodes = np.linspace(-1, 1, ne + 1)
    uo = orc.fem_p1_solve(nodes, f, a, 3, c)
    assert np.max(np.abs(s.fem_values - uo)) <= 1e-12
    Wo = _oracle_W(nodes, uo, M, n, a, da, c, f)
    xq = np.linspace(-1, 1, 4001)
    ex = np.sin(np.pi * xq)
    e_gpu = np.linalg.norm(s.evaluate_solution(xq) - ex)
    e_ref = np.linalg.norm(orc.evaluate_solution_vec(nodes, Wo, xq)[0] - ex)
    note(f"facade react ne={ne} M={M}: |L2 err - restatement| / ||u||", abs(e_gpu - e_ref) / np.linalg.norm(ex), 1e-10)
    assert abs(e_gpu - e_ref) <= 1e-10 * np.linalg.norm(ex)
    assert np.all(s.enhanced.status.cpu().numpy() == 0)
    # the indicator runs and is finite
    eta2 = s.estimate()
    assert eta2.shape == (ne,) and np.all(np.isfinite(eta2)) and np.all(eta2 >= 0)


def test_facade_reaction_without_coef_is_unit_a(dev):
    import hybrid_fem_lssvr_amd as pkg
    _, _, c, _ = orc.react_functions(1.0)
    f = lambda x: (np.pi ** 2 + c(x)) * np.sin(np.pi * x)          # noqa: E731
    one, zero = (lambda x: 1.0 + 0.0 * x), (lambda x: 0.0 * x)
    s1 = pkg.FEMLSSVRPrimalSolver(41, lssvr_M=9, lssvr_gamma=GAMMA, n_colloc=16, rhs=f, reaction=c)
    s2 = pkg.FEMLSSVRPrimalSolver(41, lssvr_M=9, lssvr_gamma=GAMMA, n_colloc=16, rhs=f, reaction=c,
                                  coef=(one, zero))
    s1.solve()
    s2.solve()
    assert np.array_equal(s1.fem_values, s2.fem_values)
    assert np.array_equal(s1.enhanced.W.cpu().numpy(), s2.enhanced.W.cpu().numpy())
    xq = np.linspace(-1, 1, 2001)
    assert np.max(np.abs(s1.evaluate_solution(xq) - np.sin(np.pi * xq))) < 2e-3


def test_facade_without_reaction_is_the_old_path(dev):
    """reaction=None: the same W as the direct ops call on the same inputs, bit for bit."""
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    a, da, _, _ = orc.react_functions(1.0)
    f = orc.varcoef_functions(*orc.varcoef_params())[2]
    s = pkg.FEMLSSVRPrimalSolver(301, lssvr_M=9, lssvr_gamma=GAMMA, n_colloc=16, rhs=f, coef=(a, da),
                                 reaction=None)
    s.solve()
    x = _t(s.fem_nodes, dev)
    ta, tda, tf = _tables(x, 16, (a, da, f), True, dev)
    W, _ = ops.enhance_varcoef(x, _t(s.fem_values, dev), 9, GAMMA, 16, ta, tda, tf, point_major=True,
                               global_domain=(-1.0, 1.0))
    assert np.array_equal(W.cpu().numpy(), s.enhanced.W.cpu().numpy())
    s = pkg.FEMLSSVRPrimalSolver(301, lssvr_M=9, lssvr_gamma=GAMMA, n_colloc=16)
    s.solve()
    W, _ = ops.enhance(_t(s.fem_nodes, dev), _t(s.fem_values, dev), 9, GAMMA, 16, global_domain=(-1.0, 1.0))
    assert np.array_equal(W.cpu().numpy(), s.enhanced.W.cpu().numpy())


def test_facade_negative_reaction_is_refused(dev):
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(21, lssvr_M=9, n_colloc=16, reaction=lambda x: np.cos(3.0 * x))
    with pytest.raises(ValueError, match="SPD"):
        s.solve_fem()


# ---------------------------------------------------------------------------
# 5. adaptivity on the singularly perturbed problem -eps u'' + u = 1
# ---------------------------------------------------------------------------
EPS = 1e-4
# numpy prototype of the same loop on the restatement (scripts/proto/react_adapt.py): see DESIGN.md section 12
PROTO_RATIO = 265.8
PROTO_NE = 112


def _layer_exact(x):
    r = 1.0 / math.sqrt(EPS)
    # 1 - cosh(r x) / cosh(r), without overflow
    return 1.0 - (np.exp(r * (x - 1.0)) + np.exp(-r * (x + 1.0))) / (1.0 + math.exp(-2.0 * r))


def _layer_solver(nodes):
    import hybrid_fem_lssvr_amd as pkg
    return pkg.FEMLSSVRPrimalSolver(len(nodes), lssvr_M=9, lssvr_gamma=1e10, n_colloc=16, nquad=5,
                                    rhs=lambda x: 1.0 + 0.0 * x, mesh=nodes,
                                    coef=(lambda x: EPS + 0.0 * x, lambda x: 0.0 * x), reaction=lambda x: 1.0 + 0.0 * x)


def test_adaptive_boundary_layers(dev, note):
    """-eps u'' + u = 1, u(+-1) = 0, eps = 1e-4: the marked elements gather at both ends and the adapted mesh
    (<= 128 elements) beats the uniform 128-element solve in the max norm on 20 001 points by at least the
    prototype's ratio / 5 (the margin covers marking ties at the threshold), and at least 1."""
    assert PROTO_RATIO is not None, "prototype ratio not recorded"
    xq = np.linspace(-1, 1, 20001)
    ex = _layer_exact(xq)
    s = _layer_solver(np.linspace(-1, 1, 9))
    s.solve_adaptive(theta=0.5, max_elements=128, max_iter=60)
    nodes = np.asarray(s.fem_nodes)
    ne = len(nodes) - 1
    err_a = np.max(np.abs(s.evaluate_solution(xq) - ex))
    u = _layer_solver(np.linspace(-1, 1, 129))
    u.solve()
    err_u = np.max(np.abs(u.evaluate_solution(xq) - ex))
    ratio = err_u / err_a
    note("adaptive layers: elements", ne)
    note("adaptive layers: uniform-128 max error", err_u)
    note("adaptive layers: adapted max error", err_a)
    note("adaptive layers: ratio (prototype %.3g on %d elements)" % (PROTO_RATIO, PROTO_NE), ratio,
         max(PROTO_RATIO / 5.0, 1.0))
    print(f"adapted ne={ne} err {err_a:.3e}, uniform-128 err {err_u:.3e}, ratio {ratio:.3g}")
    assert ne <= 128
    h = np.diff(nodes)
    # both ends refined, the middle not: the smallest elements touch x = -1 and x = +1, the largest sit inside
    assert h[0] == h.min() and h[-1] == h.min()
    assert h.max() == h[np.argmin(np.abs(0.5 * (nodes[1:] + nodes[:-1])))] and h.max() >= 16 * h.min()
    left = np.sum(nodes[1:] <= -0.5)
    right = np.sum(nodes[:-1] >= 0.5)
    assert left > ne / 3 and right > ne / 3
    assert ratio >= max(PROTO_RATIO / 5.0, 1.0)
