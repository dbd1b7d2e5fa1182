"""GPU: derivatives of the enhanced solution, the a posteriori indicator, marking + bisection and the
adaptive facade (ABI 6), each against a numpy restatement of its definition."""
import math

import numpy as np
import pytest
from numpy.polynomial.legendre import Legendre

from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _mesh(rng, ne, lo=-1.0, span=2.0):
    h = rng.uniform(0.3, 1.7, ne)
    return np.concatenate([[lo], lo + span * np.cumsum(h) / h.sum()])


# ---------------------------------------------------------------------------
# numpy restatements
# ---------------------------------------------------------------------------
def _points(x, nq):
    from hybrid_fem_lssvr_amd import ops
    return orc.estimate_points(x, ops.gauss_rule(nq)[0])


def _estimate(x, W, nq, f):
    """The oracle's Poisson indicator (eta2, J, scale of J); f [ne, nq].  The nodes come from numpy, the
    weights from the library."""
    from hybrid_fem_lssvr_amd import ops
    return orc.estimate_indicator(x, W, np.polynomial.legendre.leggauss(nq)[0], ops.gauss_rule(nq)[1], f,
                                  scales=True)[:3]


def _ref_refine(x, eta2, mx, theta, h_min):
    with np.errstate(invalid="ignore"):
        big = ~np.isfinite(eta2) | ((mx > 0) & (eta2 >= (theta * theta) * mx))
    m = big & ((x[1:] - x[:-1]) >= 2.0 * h_min)
    ne = eta2.size
    counts = 1 + m.astype(np.int64)
    pos = np.concatenate([[0], np.cumsum(counts)[:-1]])
    x_new = np.empty(ne + int(m.sum()) + 1)
    x_new[pos] = x[:-1]
    x_new[pos[m] + 1] = 0.5 * (x[:-1][m] + x[1:][m])
    x_new[-1] = x[-1]
    return x_new, np.repeat(np.arange(ne, dtype=np.int64), counts)


# ---------------------------------------------------------------------------
# lssvr_eval_deriv
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 9, 22, 33])
def test_eval_deriv_vs_legendre(dev, M):
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(100 + M)
    ne = 300
    x = _mesh(rng, ne)
    W = rng.standard_normal((ne, M)) / (1.0 + np.arange(M)) ** 2
    xq = np.concatenate([rng.uniform(-1, 1, 2000), x, [-1.3, -1.0000001, 1.0000001, 1.2, np.nan, np.nan]])
    xd, Wd, qd = _t(x, dev), _t(W, dev), _t(xq, dev)
    u0, e0 = ops.evaluate(xd, Wd, qd)
    ud, ed = ops.evaluate(xd, Wd, qd, deriv=0)
    assert np.array_equal(u0.cpu().numpy().view(np.int64), ud.cpu().numpy().view(np.int64))
    e_ref = e0.cpu().numpy()
    for k in (1, 2):
        d, e = ops.evaluate(xd, Wd, qd, deriv=k)
        d, e = d.cpu().numpy(), e.cpu().numpy()
        assert np.array_equal(e, e_ref)
        ref = np.zeros_like(xq)
        for i, (pt, el) in enumerate(zip(xq, e)):
            if el >= 0:
                ref[i] = Legendre(W[el], [x[el], x[el + 1]]).deriv(k)(pt)
        nan = np.isnan(xq)
        assert np.all(e[nan] == -1) and np.all(d[nan] == 0.0)
        scale = max(np.max(np.abs(ref)), 1e-300)
        assert np.max(np.abs(d - ref)) <= 1e-12 * scale, (k, np.max(np.abs(d - ref)) / scale)


def test_enhanced_solution_evaluate_deriv(dev):
    import hybrid_fem_lssvr_amd as pkg
    nodes = np.linspace(-1, 1, 25)
    s = pkg.FEMLSSVRPrimalSolver(25, lssvr_M=9, lssvr_gamma=1e4, n_colloc=16)
    s.solve()
    xq = np.linspace(-0.99, 0.99, 101)
    assert np.array_equal(s.enhanced.evaluate(xq, deriv=0), s.evaluate_solution(xq))
    # the enhanced solution approximates sin(pi x): u' ~ pi cos(pi x), u'' ~ -pi^2 sin(pi x)
    d1 = s.enhanced.evaluate(xq, deriv=1)
    d2 = s.enhanced.evaluate(xq, deriv=2)
    assert np.max(np.abs(d1 - np.pi * np.cos(np.pi * xq))) < 1e-3
    assert np.max(np.abs(d2 + np.pi ** 2 * np.sin(np.pi * xq))) < 1e-1
    assert nodes.size == 25


# ---------------------------------------------------------------------------
# lssvr_estimate
# ---------------------------------------------------------------------------
CASES = [(M, ne) for M in (2, 9, 22, 33) for ne in (1, 2, 129, 5000)] + [(9, 1_000_000), (33, 600_000)]


@pytest.mark.parametrize("layout", ["sin", "array", "array_pm"])
@pytest.mark.parametrize("M,ne", CASES)
def test_estimate_vs_numpy(dev, M, ne, layout):
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(M * 7919 + ne + len(layout))
    nq = 16 if ne >= 100_000 else int(rng.integers(1, 33))
    x = _mesh(rng, ne, lo=-3.0, span=6.0)
    W = rng.standard_normal((ne, M)) / (1.0 + np.arange(M)) ** 2
    xd, Wd = _t(x, dev), _t(W, dev)
    pts = ops.estimate_points(xd, nq).cpu().numpy()
    xq = _points(x, nq)
    assert np.array_equal(pts, xq)
    amp, omega = 2.5, 1.7
    f = amp * np.sin(omega * xq)
    if layout == "sin":
        kw = dict(rhs=(amp, omega))
    elif layout == "array":
        kw = dict(rhs_values=_t(f, dev))
    else:
        kw = dict(rhs_values=_t(f.T, dev), point_major=True)
    eta2, jump, out3 = ops.estimate(xd, Wd, nq, want_jump=True, **kw)
    eta2, jump, o3 = eta2.cpu().numpy(), jump.cpu().numpy(), out3.cpu().numpy()
    e_ref, j_ref, jscale = _estimate(x, W, nq, f)
    assert np.all(np.abs(eta2 - e_ref) <= 1e-12 * np.abs(e_ref) + 1e-300)
    assert jump[0] == 0.0 and jump[-1] == 0.0
    assert np.all(np.abs(jump - j_ref) <= 1e-12 * jscale)
    assert o3[2] == 0.0 and o3[1] == np.max(eta2)
    s = math.fsum(eta2.tolist())
    assert abs(o3[0] - s) <= 1e-14 * s
    eta2b, jumpb, out3b = ops.estimate(xd, Wd, nq, want_jump=True, **kw)
    assert np.array_equal(eta2b.cpu().numpy().view(np.int64), eta2.view(np.int64))
    assert np.array_equal(out3b.cpu().numpy().view(np.int64), o3.view(np.int64))


def test_estimate_non_finite_entries(dev):
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(5)
    ne, M, nq = 70_000, 9, 12
    x = _mesh(rng, ne)
    W = rng.standard_normal((ne, M))
    bad = rng.choice(ne, 40, replace=False)
    W[bad[:20], 3] = np.nan
    W[bad[20:], 5] = np.inf
    eta2, _, out3 = ops.estimate(_t(x, dev), _t(W, dev), nq, rhs=(1.0, 2.0))
    eta2, o3 = eta2.cpu().numpy(), out3.cpu().numpy()
    e_ref, _, _ = _estimate(x, W, nq, np.sin(2.0 * _points(x, nq)))
    fin = np.isfinite(eta2)
    assert np.array_equal(fin, np.isfinite(e_ref))
    assert o3[2] == float(np.count_nonzero(~fin)) and o3[2] >= 40
    assert o3[1] == np.max(eta2[fin])
    s = math.fsum(eta2[fin].tolist())
    assert abs(o3[0] - s) <= 1e-14 * s


@pytest.mark.parametrize("M", [9, 22])
def test_estimate_exact_polynomial_is_rounding_only(dev, M):
    """W sampled from ONE global polynomial u with f = -u'': residual and jumps vanish up to rounding."""
    from hybrid_fem_lssvr_amd import ops
    from numpy.polynomial import Polynomial
    rng = np.random.default_rng(11 + M)
    ne, nq = 16, 12
    x = _mesh(rng, ne)
    p = Polynomial(rng.uniform(-1, 1, 8))
    W = np.zeros((ne, M))
    for e in range(ne):
        c = p.convert(domain=[x[e], x[e + 1]], kind=Legendre).coef
        W[e, :c.size] = c
    xq = _points(x, nq)
    f = -p.deriv(2)(xq)
    eta2, _, _ = ops.estimate(_t(x, dev), _t(W, dev), nq, rhs_values=_t(f, dev))
    eta2 = eta2.cpu().numpy()
    h = x[1:] - x[:-1]
    _, wt = ops.gauss_rule(nq)
    bound = h * h * (0.5 * h * ((f * f) @ wt)) + h * p.deriv(1)(x[:-1]) ** 2
    assert np.all(eta2 <= 1e-24 * bound), np.max(eta2 / bound)


# ---------------------------------------------------------------------------
# lssvr_refine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ne,theta,h_min", [(1, 0.5, 0.0), (1, 1.0, 0.0), (1, 0.0, 0.0), (2, 0.5, 0.0),
                                            (255, 0.5, 0.0), (256, 0.5, 0.0), (257, 0.5, 0.0),
                                            (1000, 0.0, 0.0), (1000, 1.0, 0.0), (1000, 0.5, 0.0),
                                            (4099, 0.3, 3e-4), (256 * 256 + 1, 0.5, 0.0), (2_000_000, 0.5, 0.0),
                                            (2_000_000, 0.7, 4e-7)])
def test_refine_vs_numpy(dev, ne, theta, h_min):
    import torch
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(ne + int(theta * 100))
    x = _mesh(rng, ne)
    eta2 = rng.choice([0.25, 0.5, 1.0, 2.0], ne) * rng.integers(0, 3, ne)   # many ties
    if ne > 10:
        eta2[rng.choice(ne, 3, replace=False)] = [np.nan, np.inf, -np.inf]
    fin = np.isfinite(eta2)
    mx = float(np.max(eta2[fin])) if fin.any() else 0.0
    if ne > 10 and mx > 0:
        eta2[rng.choice(np.nonzero(fin)[0], 5, replace=False)] = (theta * theta) * mx   # exactly at the bar
    xd = _t(x, dev)
    x_new, parent = ops.refine(xd, _t(eta2, dev), _t(np.array([mx]), dev), theta, h_min=h_min,
                               want_parent=True)
    x_ref, p_ref = _ref_refine(x, eta2, mx, theta, h_min)
    assert np.array_equal(x_new.cpu().numpy().view(np.int64), x_ref.view(np.int64))
    assert np.array_equal(parent.cpu().numpy(), p_ref)
    x2, _ = ops.refine(xd, _t(eta2, dev), _t(np.array([mx]), dev), theta, h_min=h_min)
    assert torch.equal(x2, x_new)


def test_refine_with_all_zero_indicator_marks_nothing(dev):
    from hybrid_fem_lssvr_amd import ops
    x = np.linspace(0, 1, 11)
    x_new, parent = ops.refine(_t(x, dev), _t(np.zeros(10), dev), _t(np.zeros(1), dev), 0.0, want_parent=True)
    assert np.array_equal(x_new.cpu().numpy(), x) and np.array_equal(parent.cpu().numpy(), np.arange(10))


def test_estimate_then_refine_on_device(dev):
    """eta2_max straight from out3[1] (no host round trip)."""
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(3)
    ne = 3000
    x = _mesh(rng, ne)
    W = rng.standard_normal((ne, 9))
    eta2, _, out3 = ops.estimate(_t(x, dev), _t(W, dev), 10)
    x_new, _ = ops.refine(_t(x, dev), eta2, out3[1:2], 0.5)
    e = eta2.cpu().numpy()
    x_ref, _ = _ref_refine(x, e, float(np.max(e)), 0.5, 0.0)
    assert np.array_equal(x_new.cpu().numpy(), x_ref)


# ---------------------------------------------------------------------------
# facade
# ---------------------------------------------------------------------------
A50 = math.atan(50.0)


def _u_atan(x):
    return np.arctan(50.0 * x) - x * A50


def _f_atan(x):          # -u''
    return 250000.0 * x / (1.0 + 2500.0 * x * x) ** 2


def _atan_solver(nodes):
    import hybrid_fem_lssvr_amd as pkg
    return pkg.FEMLSSVRPrimalSolver(len(nodes), lssvr_M=9, lssvr_gamma=1e10, global_domain=(-1, 1),
                                    n_colloc=16, nquad=5, rhs=_f_atan, mesh=nodes)


def test_solve_adaptive_beats_uniform(dev, note):
    xt = np.linspace(-1, 1, 20001)
    uni = _atan_solver(np.linspace(-1, 1, 129))
    uni.solve()
    err_uni = np.max(np.abs(uni.evaluate_solution(xt) - _u_atan(xt)))
    runs = []
    for _ in range(2):
        s = _atan_solver(np.linspace(-1, 1, 9))
        est = s.solve_adaptive(theta=0.5, max_elements=128)
        runs.append(s)
    s = runs[0]
    ne = len(s.fem_nodes) - 1
    assert ne <= 128 and s.adapt_history[-1]["ne"] == ne
    err = np.max(np.abs(s.evaluate_solution(xt) - _u_atan(xt)))
    note("uniform128_over_adaptive_max_error", err_uni / err, bar=1e3)
    note("adaptive_elements", ne)
    assert err_uni / err >= 1e3, (err_uni, err, ne)
    assert np.array_equal(runs[0].fem_nodes, runs[1].fem_nodes)
    assert np.array_equal(runs[0].enhanced.W.cpu().numpy(), runs[1].enhanced.W.cpu().numpy())
    ests = [r["estimate"] for r in s.adapt_history]
    assert est == ests[-1]
    tail = ests[-5:]
    assert all(b <= a for a, b in zip(tail, tail[1:])), ests
    assert all(r["marked"] > 0 for r in s.adapt_history[:-1])
    # the state describes the final mesh, as after solve()
    assert len(s.lssvr_functions) == ne and s.fem_values.size == ne + 1
    assert np.array_equal(s.fem_nodes, s.mesh.nodes)


def test_solve_adaptive_stops_at_tol(dev):
    s = _atan_solver(np.linspace(-1, 1, 9))
    s.solve_adaptive(tol=1e-3, max_elements=4096)
    h = s.adapt_history
    assert h[-1]["estimate"] <= 1e-3 and all(r["estimate"] > 1e-3 for r in h[:-1])


def test_estimate_leaves_solution_untouched(dev):
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(25, lssvr_M=9, lssvr_gamma=1e4, global_domain=(-1, 1), n_colloc=16)
    s.solve()
    W0 = s.enhanced.W.cpu().numpy().copy()
    u0 = s.fem_values.copy()
    c0 = [f.coef.copy() for f in s.lssvr_functions]
    eta2 = s.estimate()
    assert eta2.shape == (24,) and np.all(np.isfinite(eta2)) and np.all(eta2 >= 0)
    assert np.array_equal(s.enhanced.W.cpu().numpy().view(np.int64), W0.view(np.int64))
    assert np.array_equal(s.fem_values.view(np.int64), u0.view(np.int64))
    assert all(np.array_equal(f.coef, c) for f, c in zip(s.lssvr_functions, c0))
    assert np.array_equal(s.estimate(nq=9), s.estimate(nq=9))
