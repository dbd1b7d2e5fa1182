"""GPU: the dual Gram solver (csrc/enhance_dual.hip) across its (M, n) range, in all three kernels and all three
instantiations of each.  Grid, mesh, reference and bars: tests/dual_rules.py; the 60-digit truths and the float64
restatement's own error come from tests/golden/G9_dual_grid.npz (no mpmath here).

What each test is there to catch:
  (a) grid            a live-row mask off by one at n = LPE or M = LPE, padding rows or columns that are not exact
                      zeros / unit diagonal, a pivot ring one slot short (the right-hand side rides in slot LPE),
                      the 64-row kernel with idle rows (M = 33, few points), M = 2 and 3 (no / one bubble column);
  (b) instantiations  the tabulated and the variable-coefficient bodies of every kernel at the class corners, the
                      table strides of both layouts;
  (c) routing         ``lssvr_enhance`` taking n < M - 2 to this solver by itself;
  (d) shards          ``elem_offset`` / ``ne_global`` in the Dirichlet replacement of both kernel families, and an
                      element's row not depending on the lane group (LDS slice, shuffle base) it runs in;
  (e) fallback        a degenerate element beside good ones in one wave: its NaNs stay in its own LDS slice and
                      lanes, the idle groups of the last wave (duplicates of a FAILING last element) count nothing;
  (f) stores          nothing outside W[:ne, :M] and status[:ne] is written, everything inside is."""
import numpy as np
import pytest

import dual_rules as dr
from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu

NE = dr.NE
SEL = list(dr.SEL)


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


@pytest.fixture(scope="module")
def gm(dev):
    """The shared mesh on the device (read-only): x, u, global_domain and the host copies."""
    nodes, values, gd = dr.mesh()
    return dict(nodes=nodes, values=values, gd=gd, x=_t(np.array(nodes), dev), u=_t(np.array(values), dev))


def _dual(x, u, M, n, gd, **kw):
    import torch
    from hybrid_fem_lssvr_amd import ops
    W, st = ops.enhance(x, u, M, dr.GAMMA, n, global_domain=gd, solver=ops.SOLVER_DUAL, **kw)
    torch.cuda.synchronize()
    return W, st


def _boundary_rows(W, gl, gr):
    """max |B w - g| over the rows of W: L_p(-1) = (-1)^p, L_p(1) = 1."""
    sgn = (-1.0) ** np.arange(W.shape[1])
    return max(np.max(np.abs(W @ sgn - gl)), np.max(np.abs(W.sum(1) - gr)))


def _ends(values, first_is_global=True, last_is_global=True):
    gl = np.array(values[:-1])
    gr = np.array(values[1:])
    if first_is_global:
        gl[0] = 0.0
    if last_is_global:
        gr[-1] = 0.0
    return gl, gr


# ---- (a) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", dr.CLASSES)
def test_grid_against_truth(gm, note, cls):
    """Every GRID pair of one kernel class, one launch each: no fallback, all finite, the boundary rows to 1e-12 on
    every element, the elements SEL within bar = max(floor, 10 x proto_err) of the 60-digit minimiser.  (Every pair
    is inside the envelope in the committed fixture; one that were not would keep the first three checks.)"""
    fx = dr.fixture()
    gl, gr = _ends(gm["values"])
    bad, worst = [], (0.0, None)
    pairs = [p for p in dr.GRID if dr.kernel_class(*p) == cls]
    assert len(pairs) == {"g16": 30, "g32": 70, "w64": 65}[cls]
    for M, n in pairs:
        W, st = _dual(gm["x"], gm["u"], M, n, gm["gd"])
        W, st = W.cpu().numpy(), st.cpu().numpy()
        truth, case = fx.grid(M, n)
        if st.any() or not np.all(np.isfinite(W)):
            bad.append((M, n, "status / non-finite", st.tolist()))
            continue
        rows = _boundary_rows(W, gl, gr)
        if not rows <= 1e-12:
            bad.append((M, n, "boundary rows", rows))
        if dr.in_envelope(case):
            err = orc.rel_l2_coef(W[SEL], truth).max()
            ratio = err / dr.bar(case)
            note("dual grid %s M=%d n=%d err/bar" % (cls, M, n), ratio, dr.bar(case))
            if ratio > worst[0]:
                worst = (ratio, (M, n))
            if not err <= dr.bar(case):
                bad.append((M, n, "truth", err, dr.bar(case)))
    note("dual grid %s worst err/bar (M=%s n=%s)" % ((cls,) + worst[1]), worst[0])
    assert not bad, "\n".join(map(repr, bad))


# ---- (b) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", dr.CORNERS)
def test_instantiations_at_the_class_corners(dev, gm, note, M, n):
    """RHS_ARRAY against the in-kernel sin and against the truth, point-major bit-equal to element-major; where
    n < M - 2 (the only route to it) the variable-coefficient body with a = 1, a' = 0 against the Poisson body, and
    with a non-trivial a against its own 60-digit truth, both layouts."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    fx = dr.fixture()
    x, u, gd = gm["x"], gm["u"], gm["gd"]
    truth, case = fx.corner(M, n)
    bar = dr.bar(case)
    xc = ops.colloc_points(x, n).cpu().numpy()
    f_em = _t(orc.poisson_rhs(xc), dev)
    W0, s0 = _dual(x, u, M, n, gd)
    W1, s1 = _dual(x, u, M, n, gd, rhs_values=f_em)
    W2, s2 = _dual(x, u, M, n, gd, rhs_values=f_em.t().contiguous(), point_major=True)
    assert int(s0.sum()) == 0 and int(s1.sum()) == 0 and int(s2.sum()) == 0
    assert torch.equal(W1, W2)
    e_tab = orc.rel_l2_coef(W1.cpu().numpy(), W0.cpu().numpy()).max()
    e_tru = orc.rel_l2_coef(W1.cpu().numpy()[SEL], truth).max()
    note("dual corner M=%d n=%d tabulated vs sin / bar" % (M, n), e_tab / bar, bar)
    note("dual corner M=%d n=%d tabulated vs truth / bar" % (M, n), e_tru / bar, bar)
    assert e_tab <= bar and e_tru <= bar
    if n >= M - 2:
        return                                            # lssvr_enhance_varcoef takes these to the primal kernels
    one, zero = torch.ones_like(f_em), torch.zeros_like(f_em)
    Wv, sv = ops.enhance_varcoef(x, u, M, dr.GAMMA, n, one, zero, f_em, global_domain=gd)
    torch.cuda.synchronize()
    assert int(sv.sum()) == 0
    e_one = orc.rel_l2_coef(Wv.cpu().numpy(), W0.cpu().numpy()).max()
    note("dual corner M=%d n=%d varcoef a=1 vs Poisson / bar" % (M, n), e_one / bar, bar)
    assert e_one <= bar
    a, da, fv = dr.varcoef()
    tabs = [_t(fn(xc), dev) for fn in (a, da, fv)]
    Wa, sa = ops.enhance_varcoef(x, u, M, dr.GAMMA, n, *tabs, global_domain=gd)
    Wp, sp = ops.enhance_varcoef(x, u, M, dr.GAMMA, n, *[t.t().contiguous() for t in tabs], global_domain=gd,
                                 point_major=True)
    torch.cuda.synchronize()
    assert int(sa.sum()) == 0 and int(sp.sum()) == 0
    assert torch.equal(Wa, Wp)
    tv, cv = fx.corner(M, n, vc=True)
    e_vc = orc.rel_l2_coef(Wa.cpu().numpy()[SEL], tv).max()
    note("dual corner M=%d n=%d varcoef vs truth / bar" % (M, n), e_vc / dr.bar(cv), dr.bar(cv))
    assert e_vc <= dr.bar(cv)
    assert _boundary_rows(Wa.cpu().numpy(), *_ends(gm["values"])) <= 1e-12


# ---- (c) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(17, 12), (33, 20), (6, 2)])
def test_default_solver_routes_rank_deficient_calls_here(gm, M, n):
    import torch
    from hybrid_fem_lssvr_amd import ops
    Wd, sd = _dual(gm["x"], gm["u"], M, n, gm["gd"])
    W, st = ops.enhance(gm["x"], gm["u"], M, dr.GAMMA, n, global_domain=gm["gd"])
    torch.cuda.synchronize()
    assert torch.equal(W, Wd) and torch.equal(st, sd) and int(sd.sum()) == 0


# ---- (d) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", dr.SHARD_CORNERS)
def test_shards_and_lane_groups(gm, note, M, n):
    """The mesh without its first k = 1, 2, 3 elements (elem_offset = k, ne_global = 9): rows bit-equal to rows k: of
    the full launch -- every element visits every group position of a wave, the last one keeps its Dirichlet value,
    element k gets none.  The same without the LAST k elements.  Then the whole mesh as a window of a 12-element
    one: neither end is replaced, against the truth of the same elements treated as interior."""
    x, u, gd = gm["x"], gm["u"], gm["gd"]
    Wf, sf = _dual(x, u, M, n, gd)
    assert int(sf.sum()) == 0
    Wf = Wf.cpu().numpy()
    for k in (1, 2, 3):
        Wk, sk = _dual(x[k:], u[k:], M, n, gd, elem_offset=k, ne_global=NE)
        assert int(sk.sum()) == 0
        assert np.array_equal(Wk.cpu().numpy(), Wf[k:]), ("head cut", k)
        Wk, sk = _dual(x[:NE + 1 - k], u[:NE + 1 - k], M, n, gd, elem_offset=0, ne_global=NE)
        assert int(sk.sum()) == 0
        assert np.array_equal(Wk.cpu().numpy(), Wf[:NE - k]), ("tail cut", k)
    Ww, sw = _dual(x, u, M, n, dr.wide_domain(), elem_offset=2, ne_global=12)
    assert int(sw.sum()) == 0
    Ww = Ww.cpu().numpy()
    assert _boundary_rows(Ww, *_ends(gm["values"], False, False)) <= 1e-12
    assert np.array_equal(Ww[1:-1], Wf[1:-1])
    truth, case = dr.fixture().window(M, n)
    err = orc.rel_l2_coef(Ww[SEL], truth).max()
    note("dual window M=%d n=%d err/bar" % (M, n), err / dr.bar(case), dr.bar(case))
    assert err <= dr.bar(case)
    # exact ends decide, not the indices alone: the mesh's own indices with a wider domain replace nothing either
    Wx, _ = _dual(x, u, M, n, dr.wide_domain())
    assert np.array_equal(Wx.cpu().numpy(), Ww)


# ---- (e) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(5, 16), (32, 17), (20, 64)])
def test_fallback_inside_a_shared_wave(dev, gm, M, n):
    """A zero-length element (2), a NaN node inside (elements 5, 6) and a NaN last node (element 8): status 1 and the
    linear interpolant there, fail_count = 4 = sum(status) -- the idle groups of the last wave repeat the FAILING
    element 8 and must count nothing -- and every good element bit-equal to its own single-element shard launch,
    where no degenerate element is anywhere near it."""
    import torch
    assert dr.kernel_class(M, n) in ("g16", "g32", "w64") and (M, n) != (9, 16)
    nodes = np.array(gm["nodes"])
    values = gm["values"]
    gd = gm["gd"]
    nodes[3] = nodes[2]
    nodes[6] = np.nan
    nodes[9] = np.nan
    degenerate, good = [2, 5, 6, 8], [0, 1, 3, 4, 7]
    fc = torch.zeros(1, dtype=torch.int32, device=dev)
    x, u = _t(nodes, dev), gm["u"]
    W, st = _dual(x, u, M, n, gd, fail_count=fc)
    W, st = W.cpu().numpy(), st.cpu().numpy()
    assert st.tolist() == [1 if e in degenerate else 0 for e in range(NE)]
    assert int(fc.item()) == int(st.sum()) == 4
    for e in degenerate:
        g = orc.boundary_values(e, NE, nodes[e], nodes[e + 1], values[e], values[e + 1], gd)
        assert np.array_equal(W[e], orc.linear_fallback_coef(g[0], g[1], M)), e
    assert np.all(np.isfinite(W[good]))
    gl, gr = _ends(values, True, False)
    assert _boundary_rows(W[good], gl[good], gr[good]) <= 1e-12
    for e in good:
        We, se = _dual(x[e:e + 2], u[e:e + 2], M, n, gd, elem_offset=e, ne_global=NE)
        assert int(se.sum()) == 0
        assert np.array_equal(We.cpu().numpy()[0], W[e]), e


# ---- (f) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(5, 16), (16, 16), (17, 32), (32, 32), (33, 12), (33, 64)])
def test_stores_stay_inside_the_output(dev, gm, M, n):
    """``out`` and ``status`` as exact-size views inside larger buffers filled with sentinels: every status is
    written 0, no coefficient keeps the sentinel, the guard bands on both sides are untouched (the idle groups of the
    last wave run element ne - 1 again with their stores masked; M = LPE: every lane of a group stores)."""
    import torch
    guard, sguard = 4 * 64, 64
    big = torch.full((NE * M + 2 * guard,), 7.25, dtype=torch.float64, device=dev)
    sbig = torch.full((NE + 2 * sguard,), -7, dtype=torch.int32, device=dev)
    out, status = big[guard:guard + NE * M], sbig[sguard:sguard + NE]
    W, st = _dual(gm["x"], gm["u"], M, n, gm["gd"], out=out, status=status)
    assert W.data_ptr() == out.data_ptr() and st.data_ptr() == status.data_ptr()
    assert torch.all((st == 0) | (st == 1)) and int(st.sum()) == 0
    assert not bool((out == 7.25).any()) and bool(torch.isfinite(out).all())
    assert bool((big[:guard] == 7.25).all()) and bool((big[guard + NE * M:] == 7.25).all())
    assert bool((sbig[:sguard] == -7).all()) and bool((sbig[sguard + NE:] == -7).all())
    Wr, _ = _dual(gm["x"], gm["u"], M, n, gm["gd"])
    assert torch.equal(out.view(NE, M), Wr)
