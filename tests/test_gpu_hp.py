"""GPU: hp-adaptive refinement -- lssvr_smoothness, lssvr_refine_hp and
lssvr_group_by_degree against the numpy restatement of their rules (tests/hp_rules.py), the facade's per-element
degrees against the float64 oracle of every element's own problem, and solve_adaptive(mode="hp") against the
h-only loop on the test problem of section 11."""
import math

import numpy as np
import pytest

import hp_rules
from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu

NE_SET = [1, 255, 256, 257, 256 * 256 + 1]      # one block, both sides of a block edge, more blocks than the scan has lanes


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---------------------------------------------------------------------------
# lssvr_smoothness
# ---------------------------------------------------------------------------
def _decay_rows(rng, ne, ldw):
    """w_p = +-A exp(-s p), s in [0.05, 3], A in [e^-3, e^3]: |ln env| <= 3 + 3 * 32 < 100.  A third of the rows lose
    one parity, some lose single coefficients; then the special rows.  deg is mixed over [2, ldw]."""
    p = np.arange(ldw)
    s = rng.uniform(0.05, 3.0, ne)
    W = np.exp(rng.uniform(-3, 3, ne))[:, None] * np.exp(-s[:, None] * p[None, :]) * rng.choice([-1.0, 1.0], (ne, ldw))
    par = rng.integers(0, 3, ne)
    W[(par[:, None] == 1) & (p[None, :] % 2 == 0)] = 0.0
    W[(par[:, None] == 2) & (p[None, :] % 2 == 1)] = 0.0
    W[rng.random((ne, ldw)) < 0.05] = 0.0
    deg = rng.integers(2, ldw + 1, ne).astype(np.int32)
    special = [("zero", 0.0), ("nan", np.nan), ("inf", np.inf), ("ninf", -np.inf), ("m2", None), ("one", None)]
    for k, (tag, v) in enumerate(special):
        for e in range(k, ne, 41):
            if tag == "zero":
                W[e] = 0.0
            elif tag == "m2":
                deg[e] = 2
            elif tag == "one":
                W[e, 1:] = 0.0
                W[e, 0] = 3.0
            else:
                W[e, rng.integers(0, ldw)] = v
    for e in range(ne):                       # zero padding beyond the element's own degree
        W[e, deg[e]:] = 0.0
    return W, deg


def _check_sigma(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and not np.any(np.isneginf(got))
    fin = np.isfinite(ref)
    if fin.any():
        # one ulp of ln at |ln env| <= 100 is 1.4e-14; two-ulp logs move a two-point slope by at most 6e-14
        assert np.max(np.abs(got[fin] - ref[fin]) / np.maximum(1.0, np.abs(ref[fin]))) <= 1e-12


@pytest.mark.parametrize("ldw", [2, 12, 13, 22, 23, 33])
def test_smoothness_vs_rule(dev, ldw):
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(1700 + ldw)
    for ne in (1, 127, 128, 129):
        W, deg = _decay_rows(rng, ne, ldw)
        x = _t(np.linspace(0.0, 1.0, ne + 1), dev)
        got = ops.smoothness(x, _t(W, dev), _t(deg, dev))
        again = ops.smoothness(x, _t(W, dev), _t(deg, dev))
        got = got.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(again.cpu().numpy()))
        ref = hp_rules.smoothness(W, deg)
        if ldw >= 12 and ne >= 127:
            assert np.isnan(ref).any() and np.isposinf(ref).any() and np.isfinite(ref).sum() > ne // 2
        _check_sigma(got, ref)


def test_smoothness_grid_stride(dev):
    """One element past grid cap x block (4096 workgroups of 128 elements): the second pass of the loop runs.
    The rows repeat with a period that is no multiple of the block, so the reference is computed once per row."""
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(1777)
    ne, period, ldw = 4096 * 128 + 1, 1031, 12
    Wp, dp = _decay_rows(rng, period, ldw)
    idx = np.arange(ne) % period
    x = _t(np.linspace(0.0, 1.0, ne + 1), dev)
    got = ops.smoothness(x, _t(Wp[idx], dev), _t(dp[idx], dev)).cpu().numpy()
    _check_sigma(got, hp_rules.smoothness(Wp, dp)[idx])
    # independent of the element's length and position
    x2 = _t(np.cumsum(np.concatenate([[-3.0], rng.uniform(0.1, 2.0, period)])), dev)
    a = ops.smoothness(x2, _t(Wp, dev), _t(dp, dev)).cpu().numpy()
    assert np.array_equal(_bits(a), _bits(got[:period]))


def test_smoothness_rejects_wrong_buffers(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    x = _t(np.linspace(0, 1, 11), dev)
    W = torch.zeros((10, 9), dtype=torch.float64, device=dev)
    deg = torch.full((10,), 9, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.smoothness(x, W[:9], deg)
    with pytest.raises(ValueError):
        ops.smoothness(x, W, deg[:9])
    with pytest.raises(TypeError):
        ops.smoothness(x, W, deg.to(torch.int64))
    with pytest.raises(ValueError):
        ops.smoothness(x, torch.zeros((10, 34), dtype=torch.float64, device=dev), deg)
    with pytest.raises(ValueError):
        ops.smoothness(x, W, deg, out=torch.zeros(9, dtype=torch.float64, device=dev))
    # a degree the row cannot hold reads nothing and gives NaN
    s = ops.smoothness(x, W + 1.0, _t(np.array([9, 10, 1, 0, -4, 9, 9, 9, 9, 9], dtype=np.int32), dev)).cpu().numpy()
    assert list(np.isnan(s)) == [False, True, True, True, True] + [False] * 5


# ---------------------------------------------------------------------------
# lssvr_refine_hp
# ---------------------------------------------------------------------------
THETA, SIGMA_MIN = 0.5, 1.0


def _hp_case(rng, ne):
    """Inputs none of whose decisions rests on a rounding: eta2 at least 1 % away from theta^2 max or exactly on it,
    sigma at least 0.05 away from sigma_min (or NaN / inf), lengths 0.01 or 1 against 2 h_min = 0.1."""
    mx = 7.0
    thr = (THETA * THETA) * mx
    kind = rng.integers(0, 6, ne)
    eta2 = np.where(kind == 0, thr * rng.uniform(1.01, 3.9, ne), thr * rng.uniform(0.0, 0.99, ne))
    eta2[kind == 1] = thr                      # exact ties: marked
    eta2[kind == 2] = np.nan
    eta2[kind == 3] = rng.choice([np.inf, -np.inf], int((kind == 3).sum()))
    eta2[rng.integers(0, ne)] = mx
    sigma = np.where(rng.random(ne) < 0.5, rng.uniform(1.05, 6.0, ne), rng.uniform(-1.0, 0.95, ne))
    odd = rng.integers(0, 12, ne)
    sigma[odd == 0] = np.nan
    sigma[odd == 1] = np.inf
    sigma[odd == 2] = SIGMA_MIN                # exactly on it: smooth
    deg = rng.integers(2, 24, ne).astype(np.int32)
    h = np.where(rng.random(ne) < 0.25, 0.01, 1.0) * rng.uniform(1.0, 1.5, ne)
    x = np.concatenate([[-2.0], -2.0 + np.cumsum(h)])
    fin = np.isfinite(eta2) & (eta2 != thr)
    near = int(np.sum(np.abs(eta2[fin] / thr - 1.0) < 0.01))
    sf = np.isfinite(sigma) & (sigma != SIGMA_MIN)
    near += int(np.sum(np.abs(sigma[sf] - SIGMA_MIN) < 0.05))
    hh = x[1:] - x[:-1]
    near += int(np.sum(np.abs(hh / 0.1 - 1.0) < 0.01))
    return x, eta2, mx, sigma, deg, near


def _run_hp(dev, x, eta2, mx, sigma, deg, **kw):
    from hybrid_fem_lssvr_amd import ops
    xn, dn, par, cnt = ops.refine_hp(_t(x, dev), _t(eta2, dev), _t(np.array([mx]), dev), THETA, _t(sigma, dev),
                                     _t(deg, dev), want_parent=True, **kw)
    return xn.cpu().numpy(), dn.cpu().numpy(), par.cpu().numpy(), cnt


def _same(got, ref):
    assert got[3] == ref[3]
    assert got[0].shape == ref[0].shape and np.array_equal(_bits(got[0]), _bits(ref[0]))
    assert got[1].dtype == np.int32 and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2], ref[2])


@pytest.mark.parametrize("ne", NE_SET)
def test_refine_hp_vs_rule(dev, ne):
    rng = np.random.default_rng(1800 + ne)
    x, eta2, mx, sigma, deg, near = _hp_case(rng, ne)
    assert near == 0                           # no element was left out, none sits near a threshold
    got = _run_hp(dev, x, eta2, mx, sigma, deg, sigma_min=SIGMA_MIN, dM=2, M_max=21, h_min=0.05)
    ref = hp_rules.refine_hp(x, eta2, mx, THETA, 0.05, sigma, deg, SIGMA_MIN, 2, 21)
    _same(got, ref)
    if ne >= 255:
        up, split = hp_rules.actions(x, eta2, mx, THETA, 0.05, sigma, deg, SIGMA_MIN, 2, 21)
        m = hp_rules.marked(eta2, mx, THETA)
        # every branch of the rule is taken: raised, no room, rough, blocked by h_min, unmarked
        assert up.any() and split.any() and (m & ~up & ~split).any() and (~m).any()
        assert (m & (deg + 2 > 21) & (sigma >= SIGMA_MIN) & split).any()
    assert np.all(np.diff(got[0]) > 0)
    again = _run_hp(dev, x, eta2, mx, sigma, deg, sigma_min=SIGMA_MIN, dM=2, M_max=21, h_min=0.05)
    _same(again, got)


@pytest.mark.parametrize("ne", [1, 257, 256 * 256 + 1])
def test_refine_hp_without_raising_is_refine(dev, ne):
    """sigma_min = +inf (and no sigma = +inf): nothing is raised, and the nodes and parents are lssvr_refine's."""
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(1900 + ne)
    x, eta2, mx, sigma, deg, _ = _hp_case(rng, ne)
    sigma[np.isposinf(sigma)] = 50.0
    got = _run_hp(dev, x, eta2, mx, sigma, deg, sigma_min=np.inf, dM=2, M_max=21, h_min=0.05)
    xr, pr = ops.refine(_t(x, dev), _t(eta2, dev), _t(np.array([mx]), dev), THETA, h_min=0.05, want_parent=True)
    assert np.array_equal(_bits(got[0]), _bits(xr.cpu().numpy())) and np.array_equal(got[2], pr.cpu().numpy())
    assert np.array_equal(got[1], deg[got[2]])             # children inherit the degree
    assert got[3] == (len(got[1]) - ne, 0)


def test_refine_hp_all_raised_all_split_blocked(dev):
    rng = np.random.default_rng(1999)
    ne = 600
    x = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.0, ne))])
    eta2 = rng.uniform(1.0, 2.0, ne)
    deg = rng.integers(2, 10, ne).astype(np.int32)
    smooth, rough = np.full(ne, 3.0), np.full(ne, 0.1)
    # theta = 0 marks everything (max > 0)
    from hybrid_fem_lssvr_amd import ops
    one = _t(np.array([2.0]), dev)

    def run(sigma, **kw):
        xn, dn, par, cnt = ops.refine_hp(_t(x, dev), _t(eta2, dev), one, 0.0, _t(sigma, dev), _t(deg, dev),
                                         want_parent=True, **kw)
        return xn.cpu().numpy(), dn.cpu().numpy(), par.cpu().numpy(), cnt

    xn, dn, par, cnt = run(smooth, dM=3, M_max=33)
    assert cnt == (0, ne) and np.array_equal(_bits(xn), _bits(x)) and np.array_equal(dn, deg + 3)
    assert np.array_equal(par, np.arange(ne))
    xn, dn, par, cnt = run(rough, dM=3, M_max=33)
    assert cnt == (ne, 0) and np.array_equal(par, np.repeat(np.arange(ne), 2)) and np.array_equal(dn, deg[par])
    assert np.array_equal(_bits(xn[0::2]), _bits(x)) and np.array_equal(_bits(xn[1::2]), _bits(0.5 * (x[:-1] + x[1:])))
    # M_max leaves no room: smooth elements are bisected instead
    _, _, _, cnt = run(smooth, dM=3, M_max=8)
    assert cnt == (int(np.sum(deg + 3 > 8)), int(np.sum(deg + 3 <= 8))) and min(cnt) > 0
    # h_min blocks every split: rough elements stay as they are
    xn, dn, par, cnt = run(rough, dM=3, M_max=33, h_min=0.6)
    assert cnt == (0, 0) and np.array_equal(_bits(xn), _bits(x)) and np.array_equal(dn, deg)


def test_refine_hp_rejects_wrong_buffers(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    x = _t(np.linspace(0, 1, 11), dev)
    e = torch.ones(10, dtype=torch.float64, device=dev)
    d = torch.full((10,), 5, dtype=torch.int32, device=dev)
    for bad in (dict(eta2=e[:9]), dict(sigma=e[:9]), dict(deg=d[:9]), dict(deg=d.to(torch.int64)),
                dict(mx=e[:0]), dict(work=torch.empty(1, dtype=torch.float64, device=dev))):
        a = dict(eta2=e, mx=e[:1], sigma=e, deg=d, work=None)
        a.update(bad)
        with pytest.raises((ValueError, TypeError)):
            ops.refine_hp(x, a["eta2"], a["mx"], 0.5, a["sigma"], a["deg"], work=a["work"])
    for kw in (dict(dM=0), dict(M_max=34), dict(M_max=1)):
        with pytest.raises(ValueError):
            ops.refine_hp(x, e, e[:1], 0.5, e, d, **kw)


# ---------------------------------------------------------------------------
# lssvr_group_by_degree
# ---------------------------------------------------------------------------
def _check_groups(dev, deg):
    from hybrid_fem_lssvr_amd import ops
    deg = np.asarray(deg, dtype=np.int32)
    ids, off = ops.group_by_degree(_t(deg, dev))
    ids, off = ids.cpu().numpy(), off.cpu().numpy()
    ref_ids, ref_off = hp_rules.group_by_degree(deg)
    assert ids.dtype == np.int64 and off.shape == (35,)
    assert np.array_equal(off, ref_off)
    assert np.array_equal(ids[:off[34]], ref_ids)
    valid = (deg >= 2) & (deg <= 33)
    if valid.all():                             # the statement of the contract
        order = np.argsort(deg, kind="stable")
        assert np.array_equal(ids, order)
        assert np.array_equal(off, np.searchsorted(deg[order], np.arange(35)))
        assert off[34] == deg.size
    return ids, off


@pytest.mark.parametrize("ne", NE_SET)
def test_group_by_degree_vs_stable_argsort(dev, ne):
    rng = np.random.default_rng(2000 + ne)
    _check_groups(dev, rng.integers(2, 34, ne))                       # all 32 degrees (from 255 elements on)
    _check_groups(dev, np.full(ne, 9))                                # a single degree
    _check_groups(dev, rng.choice([5, 7, 33], ne, p=[0.9, 0.09, 0.01]))
    deg = rng.integers(2, 34, ne)
    out = rng.random(ne) < 0.1                                        # in no group, and nothing written for them
    deg[out] = rng.choice([0, 1, 34, -5, 1 << 20], int(out.sum()))
    deg[0] = 34
    ids, off = _check_groups(dev, deg)
    assert off[34] == int(np.sum((deg >= 2) & (deg <= 33))) < ne


def test_group_by_degree_every_degree_once(dev):
    ids, off = _check_groups(dev, np.arange(33, 1, -1))
    assert np.array_equal(ids, np.arange(31, -1, -1)) and np.array_equal(off[2:], np.arange(33))


def test_group_by_degree_past_the_grid_cap(dev):
    """More tiles of 256 elements than the 1024 workgroups of the grid: every workgroup sorts a run of tiles."""
    rng = np.random.default_rng(2100)
    _check_groups(dev, rng.integers(2, 34, 1024 * 256 * 2 + 77))


# ---------------------------------------------------------------------------
# facade: element_degrees
# ---------------------------------------------------------------------------
def _hetero_solver(rhs=None):
    import hybrid_fem_lssvr_amd as pkg
    rng = np.random.default_rng(2200)
    ne = 200
    h = rng.uniform(0.3, 1.7, ne)
    nodes = np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])
    nodes[-1] = 1.0
    kw = {} if rhs is None else dict(rhs=rhs)
    s = pkg.FEMLSSVRPrimalSolver(ne + 1, lssvr_M=9, lssvr_gamma=1e4, global_domain=(-1, 1), n_colloc=12, mesh=nodes,
                                 **kw)
    return s, nodes, rng.choice([5, 9, 14, 23, 33], ne)


@pytest.mark.parametrize("callable_rhs", [False, True])
def test_element_degrees_vs_oracle_per_element(dev, callable_rhs):
    s, nodes, deg = _hetero_solver(orc.poisson_rhs if callable_rhs else None)
    ne = len(deg)
    s.element_degrees = deg
    s.solve()
    W = s.enhanced.W.cpu().numpy()
    assert W.shape == (ne, 33) and s.enhanced.n_fallback == 0
    assert np.array_equal(s.enhanced.degrees, deg)
    u = s.fem_values
    worst = {}
    for i in range(ne):
        M = int(deg[i])
        n = hp_rules.n_colloc(12, M)
        assert n == s.group_colloc(M)
        gl, gr = orc.boundary_values(i, ne, nodes[i], nodes[i + 1], u[i], u[i + 1], (-1.0, 1.0))
        wo = orc.solve_primal_kkt(orc.element_system(nodes[i], nodes[i + 1], gl, gr, M, 1e4, n))
        assert np.all(W[i, M:] == 0.0)                        # padding columns are exactly zero
        err = orc.rel_l2_coef(W[i, :M][None], wo[None]).max()
        worst[M] = max(worst.get(M, 0.0), err)
        assert err <= (1e-12 if M <= 22 else 1e-11), (i, M, err)     # test_gpu_hetero.py's bars
    assert sorted(worst) == [5, 9, 14, 23, 33]
    # the estimator and the evaluation take the padded rows as they are
    assert np.all(np.isfinite(s.estimate()))
    assert np.all(np.isfinite(s.evaluate_solution(np.linspace(-1, 1, 501))))


def test_element_degrees_none_is_the_old_solve(dev):
    import hybrid_fem_lssvr_amd as pkg
    s, nodes, deg = _hetero_solver()
    assert s.element_degrees is None
    s.solve()
    W0 = s.enhanced.W.cpu().numpy()
    assert not hasattr(s.enhanced, "degrees")
    ref = pkg.enhance_elements(nodes, s.fem_values, 9, 1e4, n_colloc=12, global_domain=(-1.0, 1.0))
    assert np.array_equal(_bits(W0), _bits(ref.W.cpu().numpy()))
    # ... and a uniform element_degrees is the same problem element by element (another kernel entry: rounding only)
    s.element_degrees = np.full(len(deg), 9)
    s.n_colloc = 18
    s.solve()
    ref18 = pkg.enhance_elements(nodes, s.fem_values, 9, 1e4, n_colloc=18, global_domain=(-1.0, 1.0))
    assert orc.rel_l2_coef(s.enhanced.W.cpu().numpy(), ref18.W.cpu().numpy()).max() <= 1e-12


# ---------------------------------------------------------------------------
# end to end: the problem and the settings of DESIGN.md section 17
# ---------------------------------------------------------------------------
A50 = math.atan(50.0)


def _u_atan(x):
    return np.arctan(50.0 * x) - x * A50


def _f_atan(x):          # -u''
    return 250000.0 * x / (1.0 + 2500.0 * x * x) ** 2


def _atan_solver(M):
    import hybrid_fem_lssvr_amd as pkg
    return pkg.FEMLSSVRPrimalSolver(9, lssvr_M=M, lssvr_gamma=1e10, global_domain=(-1, 1), n_colloc=16, nquad=5,
                                    rhs=_f_atan, mesh=np.linspace(-1, 1, 9))


def test_solve_adaptive_hp_beats_h_from_the_same_degree(dev, note):
    """Budget sum M_e <= 600 from degree 5: the numpy prototype (scripts/proto/hp_adapt.py) reads h: 120 elements,
    max error 2.56e-8; hp: 28 elements, sum M = 544, max error 6.17e-10 -- 41x.  The bar is 4x: the 10x slack of
    section 11.1."""
    xt = np.linspace(-1, 1, 20001)
    h = _atan_solver(5)
    h.solve_adaptive(theta=0.5, max_elements=120)
    h2 = _atan_solver(5)
    h2.solve_adaptive(theta=0.5, max_elements=120, mode="h")
    assert h2.adapt_history == h.adapt_history and h.adapt_history
    assert all(sorted(r) == ["estimate", "marked", "ne"] for r in h.adapt_history)
    assert h.element_degrees is None
    err_h = np.max(np.abs(h.evaluate_solution(xt) - _u_atan(xt)))
    ne_h = len(h.fem_nodes) - 1

    s = _atan_solver(5)
    est = s.solve_adaptive(theta=0.5, mode="hp", M_max=21, dM=2, sigma_min=1.0, max_dof=600)
    hist = s.adapt_history
    err = np.max(np.abs(s.evaluate_solution(xt) - _u_atan(xt)))
    ne = len(s.fem_nodes) - 1
    for what, v in (("h_max_error", err_h), ("hp_max_error", err), ("h_over_hp_max_error", err_h / err),
                    ("h_elements", ne_h), ("hp_elements", ne), ("hp_dof", hist[-1]["dof"]), ("hp_estimate", est),
                    ("hp_rounds", len(hist))):
        note(what, v)
        print(what, v)
    assert all(sorted(r) == ["dof", "estimate", "marked", "ne", "raised"] for r in hist)
    deg = np.asarray(s.element_degrees)
    assert deg.shape == (ne,) and hist[-1]["ne"] == ne and hist[-1]["dof"] == int(deg.sum()) <= 600
    assert deg.min() >= 5 and deg.max() <= 21 and np.array_equal(s.enhanced.degrees, deg)
    assert s.enhanced.W.shape == (ne, int(deg.max()))
    assert ne < ne_h
    assert sum(r["raised"] for r in hist) > 0 and sum(r["marked"] for r in hist) > 0
    assert hist[-1]["estimate"] == est and hist[-1]["marked"] == 0 and hist[-1]["raised"] == 0
    for a, b in zip(hist[:-1], hist[1:]):
        assert b["ne"] == a["ne"] + a["marked"] and b["dof"] > a["dof"]
    assert err <= 0.25 * err_h, (err, err_h)
