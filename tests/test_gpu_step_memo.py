"""GPU: the step memo (ops.StepPlan(memo=True), lssvr_step_plan_memo_*).  A launch with the memo bound must give
the BITS of a launch without it and of ops.enhance + ops.p1_assemble on the same inputs -- for a valid memo, a
stale one and one that cannot match (NaN, signed zeros).  The references are today's paths and the float64 oracle,
never the memo path itself.  Bars against oracle.solve_primal_kkt: the ones tests/test_gpu_enhance.py uses for the
same regimes (1e-12 against the float64 oracle on ordinary meshes; 1e-13 where the ridge dominates, where the
float64 KKT solve is itself at 1e-15 of the 60-digit minimiser)."""
import numpy as np
import pytest

from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu

GAMMA = 1e4


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _bits(a, b):
    """bit-for-bit equality (torch.equal on the integer view: NaN rows and signed zeros count as what they are)"""
    import torch
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return a.shape == b.shape and torch.equal(a, b)


def _mesh(ne, seed, lo=-1.3, hmin=0.002, hmax=0.05):
    rng = np.random.default_rng(seed)
    nodes = np.cumsum(np.concatenate([[lo], rng.uniform(hmin, hmax, ne)]))
    values = np.sin(np.pi * nodes) + 0.01 * rng.standard_normal(ne + 1)
    return nodes, values


def _kkt_rows(nodes, values, M, gamma, n, gd, sel, elem_offset=0, ne_global=None, bc=(0.0, 0.0)):
    ne_global = len(nodes) - 1 if ne_global is None else ne_global
    rows = []
    for i in sel:
        gl, gr = orc.boundary_values(i + elem_offset, ne_global, nodes[i], nodes[i + 1], values[i], values[i + 1], gd,
                                     *bc)
        rows.append(orc.solve_primal_kkt(orc.element_system(nodes[i], nodes[i + 1], gl, gr, M, gamma, n)))
    return np.array(rows)


def _three_ways(dev, nodes, values, M, gamma, n, *, expect_memo=True, **kw):
    """(plan with memo, W) after checking memo on == memo off == enhance + p1_assemble, bit for bit."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    x, u = _t(nodes, dev), _t(values, dev)
    gd = kw.pop("global_domain", (nodes[0], nodes[-1]))
    on = ops.StepPlan(x, u, M, gamma, n, global_domain=gd, memo=True, **kw)
    off = ops.StepPlan(x, u, M, gamma, n, global_domain=gd, memo=False, **kw)
    assert off.memo_bytes == 0 and (on.memo_bytes > 0) == expect_memo
    W1, s1 = on.launch()
    W0, s0 = off.launch()
    We, se = ops.enhance(x, u, M, gamma, n, global_domain=gd, **kw)
    bands = ops.p1_assemble(x, 2)
    torch.cuda.synchronize()
    assert _bits(W1, W0) and _bits(W1, We), (M, n, len(nodes) - 1)
    assert torch.equal(s1, s0) and torch.equal(s1, se)
    for k in ("diag", "off", "load"):
        assert _bits(on.bands[k], off.bands[k]) and _bits(on.bands[k], bands[k]), k
    return on, W1, s1


def _n_odd(M):
    return M + 2 if M % 2 else M + 3


# n = 70 crosses the kReseed boundary; the odd n exercises the pair loop's tail.  (22, 16) is left out: n < M - 2
# is the rank-deficient primal system, which lssvr_step refuses.  (22, 25) is the near-square regime with
# refinement steps: no memo, the plan falls back silently -- the comparison still holds.
MN = [(M, n) for M in (2, 3, 4, 5, 9, 12, 13, 22) for n in (_n_odd(M), 16, 70) if n >= M - 2]


@pytest.mark.parametrize("M,n", MN)
def test_memo_equals_plain_step_and_enhance(dev, M, n):
    for ne in (1, 63, 257, 5003):       # one element; a partial wave; a partial block; many blocks, partial last wave
        nodes, values = _mesh(ne, 1000 * M + n + ne)
        gd = (nodes[0], nodes[-1])
        bc = (0.3, -0.7)                # (non-zero: with zero data the one-element mesh has the zero solution at M = 2)
        _, W, st = _three_ways(dev, nodes, values, M, GAMMA, n, expect_memo=not (M == 22 and n == 25), bc=bc)
        assert int(st.sum()) == 0
        sel = sorted({0, ne // 2, ne - 1})
        err = orc.rel_l2_coef(W.cpu().numpy()[sel], _kkt_rows(nodes, values, M, GAMMA, n, gd, sel, bc=bc)).max()
        print("M=%d n=%d ne=%d vs solve_primal_kkt: %.2e" % (M, n, ne, err))
        assert err <= 1e-12, (M, n, ne, err)


def test_memo_shards_and_boundary_values(dev):
    """An interior shard (elem_offset > 0, ne_global > ne: no Dirichlet value anywhere) and a shard whose ends are the
    global ends with non-zero boundary values."""
    M, n, ne = 9, 16, 257
    nodes, values = _mesh(ne, 7)
    gd_wide = (nodes[0] - 1.0, nodes[-1] + 1.0)
    _, W, _ = _three_ways(dev, nodes, values, M, GAMMA, n, global_domain=gd_wide, elem_offset=40, ne_global=ne + 90)
    sel = [0, ne - 1]
    ref = _kkt_rows(nodes, values, M, GAMMA, n, gd_wide, sel, elem_offset=40, ne_global=ne + 90)
    assert orc.rel_l2_coef(W.cpu().numpy()[sel], ref).max() <= 1e-12
    _, W, _ = _three_ways(dev, nodes, values, M, GAMMA, n, bc=(0.3, -0.7))
    W = W.cpu().numpy()
    assert abs(orc.clenshaw(-1.0, W[0]) - 0.3) < 1e-12 and abs(orc.clenshaw(1.0, W[-1]) + 0.7) < 1e-12


def test_memo_far_from_origin_cold_path(dev):
    """|x| / h ~ 1e9: every wave takes any_slow (exact boundary rows, after the loop -- unchanged by the memo)."""
    ne, h = 200, 0.7
    nodes = 7.0e8 + h * np.arange(ne + 1)
    values = np.sin(0.01 * np.arange(ne + 1))
    _three_ways(dev, nodes, values, 9, GAMMA, 16)
    _three_ways(dev, nodes, values, 13, GAMMA, 16)


@pytest.mark.parametrize("M,n,g4", [(9, 16, 1e-6), (9, 16, 1e-12), (5, 5, 1e-9)])
def test_memo_ridge_dominated_lanes(dev, M, n, g4):
    """tests/test_gpu_enhance.py::test_ridge_dominated_sweep's mesh and penalties, with every third element fine
    enough to leave the ridge regime: some lanes of each wave take cheb_ridge_solve, the others do not."""
    ne, h = 150, 0.5
    gamma = g4 / (2.0 / h) ** 4
    rng = np.random.default_rng(M * 1000 + n)
    widths = np.full(ne, h)
    widths[::3] = 1e-3
    nodes = -1.0 + np.concatenate([[0.0], np.cumsum(widths)])
    values = np.sin(np.pi * nodes) + 0.01 * rng.standard_normal(ne + 1)
    gd = (nodes[0], nodes[-1])
    _, W, st = _three_ways(dev, nodes, values, M, gamma, n)
    assert int(st.sum()) == 0
    sel = [1, 64, 127, ne - 1]                         # coarse (ridge-dominated) elements
    err = orc.rel_l2_coef(W.cpu().numpy()[sel], _kkt_rows(nodes, values, M, gamma, n, gd, sel)).max()
    print("ridge M=%d n=%d g4=%.0e vs solve_primal_kkt: %.2e" % (M, n, g4, err))
    assert err <= 1e-13, err


def test_memo_degenerate_element(dev):
    ne, M, n = 300, 9, 16
    nodes = np.linspace(0, 3, ne + 1)
    nodes[100] = nodes[99]                 # element 99 has h = 0
    values = np.sin(nodes)
    _, W, st = _three_ways(dev, nodes, values, M, GAMMA, n, global_domain=(0.0, 3.0))
    W, st = W.cpu().numpy(), st.cpu().numpy()
    assert list(np.nonzero(st)[0]) == [99]
    assert np.allclose(W[99, :2], [0.5 * (values[99] + values[100]), 0.5 * (values[100] - values[99])])
    assert np.all(W[99, 2:] == 0)


def test_memo_is_validated_against_the_live_mesh(dev):
    """x rewritten in place behind the memo's back (elements 99 .. 139: two waves partially), then refreshed; u
    rewritten; a -0.0 / +0.0 node pair and a NaN node."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    M, n, ne = 9, 16, 700
    nodes, values = _mesh(ne, 11)
    gd = (nodes[0], nodes[-1])
    x, u = _t(nodes, dev), _t(values, dev)
    plan = ops.StepPlan(x, u, M, GAMMA, n, global_domain=gd, memo=True)
    assert plan.memo_bytes == 8 * (19 * 704 + ne + 1)

    def check(what):
        W, st = plan.launch()
        We, se = ops.enhance(x, u, M, GAMMA, n, global_domain=gd)
        torch.cuda.synchronize()
        assert _bits(W, We) and torch.equal(st, se), what
        return W.clone()

    W0 = check("fresh memo")
    x[100:140] += 1.0e-4                        # (spacings >= 2e-3: the mesh stays ordered)
    W1 = check("stale memo, no refresh")
    assert not _bits(W0[99:140], W1[99:140]) and _bits(W0[:99], W1[:99]) and _bits(W0[140:], W1[140:])
    sel = [99, 120, 139]
    ref = _kkt_rows(x.cpu().numpy(), values, M, GAMMA, n, gd, sel)
    assert orc.rel_l2_coef(W1.cpu().numpy()[sel], ref).max() <= 1e-12
    plan.refresh_memo()
    assert _bits(check("after refresh_memo"), W1)
    u.copy_(_t(np.cos(nodes), dev))
    W2 = check("u rewritten")
    assert not _bits(W1, W2)
    # signed zeros: x = -0.0 where the memo's key holds +0.0 is a different key (and the same arithmetic value)
    x.copy_(_t(nodes - nodes[300], dev))
    assert float(x[300]) == 0.0
    plan2 = ops.StepPlan(x, u, M, GAMMA, n, global_domain=(float(x[0]), float(x[-1])), memo=True)
    x[300] = -0.0
    W, st = plan2.launch()
    We, se = ops.enhance(x, u, M, GAMMA, n, global_domain=(float(x[0]), float(x[-1])))
    torch.cuda.synchronize()
    assert _bits(W, We) and torch.equal(st, se)
    # a NaN node differs from its finite key (the loop runs); after a refresh the key holds the same NaN bits and
    # matches -- and the memo then holds what the loop makes of that NaN
    x[500] = float("nan")
    for refresh in (False, True):
        if refresh:
            plan2.refresh_memo()
        W, st = plan2.launch()
        We, se = ops.enhance(x, u, M, GAMMA, n, global_domain=(float(x[0]), float(x[-1])))
        torch.cuda.synchronize()
        assert _bits(W, We) and torch.equal(st, se), refresh
        assert sorted(np.nonzero(st.cpu().numpy())[0]) == [499, 500]


def test_memo_in_a_captured_graph(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    M, n, ne = 9, 16, 1000
    nodes, values = _mesh(ne, 21)
    gd = (nodes[0], nodes[-1])
    x, u = _t(nodes, dev), _t(values, dev)
    plan = ops.StepPlan(x, u, M, GAMMA, n, global_domain=gd, memo=True)
    assert plan.memo_bytes > 0
    graph = ops.StepGraph(plan, steps=3)
    u.copy_(_t(np.cos(nodes), dev))
    W, st = graph.replay()
    torch.cuda.synchronize()
    Wg = W.clone()
    We, se = ops.StepPlan(x, u, M, GAMMA, n, global_domain=gd, memo=False).launch()
    torch.cuda.synchronize()
    assert _bits(Wg, We) and torch.equal(st, se)


def test_two_plans_on_two_streams(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    M, n = 9, 16
    meshes = [_mesh(3001, 31), _mesh(2777, 32)]
    xs = [(_t(a, dev), _t(b, dev), (a[0], a[-1])) for a, b in meshes]
    plans = [ops.StepPlan(x, u, M, GAMMA, n, global_domain=gd, memo=True) for x, u, gd in xs]
    seq = []
    for p in plans:
        W, _ = p.launch()
        torch.cuda.synchronize()
        seq.append(W.clone())
        W.zero_()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in plans]
    for _ in range(4):
        for p, s in zip(plans, streams):
            p.launch(s)
    torch.cuda.synchronize()
    for p, W in zip(plans, seq):
        assert _bits(p.W, W)


@pytest.mark.parametrize("M,n", [(33, 64), (14, 12)])
def test_plans_without_a_memo_fall_back_silently(dev, M, n):
    """M = 33 (MFMA kernels) and the near-square regime at M = 14 have no memo: memo=True is accepted and ignored."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    nodes, values = _mesh(130, 41)
    gd = (nodes[0], nodes[-1])
    x, u = _t(nodes, dev), _t(values, dev)
    plan = ops.StepPlan(x, u, M, GAMMA, n, global_domain=gd, memo=True)
    assert plan.memo_bytes == 0
    plan.refresh_memo()
    W, st = plan.launch()
    W0, st0 = ops.StepPlan(x, u, M, GAMMA, n, global_domain=gd, memo=False).launch()
    torch.cuda.synchronize()
    assert _bits(W, W0) and torch.equal(st, st0)
