"""GPU: several load cases on one mesh (``lssvr_enhance_multi`` / ``ops.enhance_multi`` / ``solve_many``) -- one
factorisation per element, many right-hand sides.  Every case has its own right-hand side, nodal values and non-zero
Dirichlet pair, so a mix-up of case indices shows; every expected value is the existing oracle's, called once per
case."""
import functools

import numpy as np
import pytest

from oracle import closed_form_mp as cf
from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu

GAMMA = 1e4
SHAPES = [(257, 9, 16), (130, 16, 24), (65, 4, 8), (65, 2, 4)]      # (ne, M, n)
NCASES = [1, 2, 7, 19]                                              # 19 > every RC(M) (at most 8)
KS = [1.0, 1e4]


def _case_f(f, j):
    return lambda x: (1.0 + 0.25 * j) * f(x) + 0.5 * j


def _case_u(nodes, j):
    return np.sin((j + 1) * np.pi * nodes / 2.0) + 0.1 * j


def _case_bc(j):
    return (0.3 + 0.1 * j, -0.2 - 0.05 * j)


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _tab(fn, xc, pm):
    v = np.broadcast_to(np.asarray(fn(xc), dtype=np.float64), xc.shape)
    return np.array(v.T if pm else v, order="C")


def _inputs(dev, nodes, n, a, da, c, f, ncases, pm):
    """Device inputs of ops.enhance_multi for the first ``ncases`` cases: x, U, a, a', f, c | None, bc."""
    from hybrid_fem_lssvr_amd import ops
    x = _t(nodes, dev)
    xc = ops.colloc_points(x, n).cpu().numpy()
    U = _t(np.stack([_case_u(nodes, j) for j in range(ncases)]), dev)
    F = _t(np.stack([_tab(_case_f(f, j), xc, pm) for j in range(ncases)]), dev)
    bc = _t(np.array([_case_bc(j) for j in range(ncases)]), dev)
    tc = None if c is None else _t(_tab(c, xc, pm), dev)
    return x, U, _t(_tab(a, xc, pm), dev), _t(_tab(da, xc, pm), dev), F, tc, bc


def _multi(dev, nodes, M, n, a, da, c, f, ncases, pm, **kw):
    from hybrid_fem_lssvr_amd import ops
    x, U, ta, tda, F, tc, bc = _inputs(dev, nodes, n, a, da, c, f, ncases, pm)
    kw.setdefault("global_domain", (float(nodes[0]), float(nodes[-1])))
    W, st = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda, F, c_values=tc, bc=bc, point_major=pm, **kw)
    return W.cpu().numpy(), st.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _reference(ne, M, n, k, with_c, ncases, lo=-1.0, hi=1.0):
    """(nodes, [oracle W of case j], [60-digit rows of elements 0, ne//3, ne-1 of case j] | None): computed once,
    shared, never written."""
    a, da, c, f = orc.react_functions(k)
    nodes = np.linspace(lo, hi, ne + 1)
    sel = [0, ne // 3, ne - 1]
    Wo, tr = [], []
    for j in range(ncases):
        bl, br = _case_bc(j)
        kw = dict(coef_a=a, coef_da=da, coef_c=c if with_c else None, bc_left=bl, bc_right=br)
        Wo.append(orc.enhance_all(nodes, _case_u(nodes, j), M, GAMMA, n, rhs=_case_f(f, j), **kw)[0])
        # (M = 2 without c: the 60-digit solve reads a_k back from the column of L_2, which such a system lacks)
        if cf.HAVE_MP and (M > 2 or with_c):
            tr.append(cf.truth_all(nodes, _case_u(nodes, j), M, GAMMA, n, _case_f(f, j), elements=sel, **kw))
    for w in Wo + tr:
        w.setflags(write=False)
    return nodes, Wo, (tr or None)


# ---------------------------------------------------------------------------
# 1. against the restatement, 2. against the single-case entry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ne,M,n", SHAPES)
def test_multi_vs_restatement_and_60_digits(dev, note, ne, M, n, k, with_c):
    """Every case within 1e-11 of the float64 restatement called with that case's f, u and Dirichlet pair (the
    project's bar for M <= 22) and within 1e-13 of the 60-digit minimiser on elements 0, ne//3, ne-1; the two table
    layouts agree to 1e-12.  1, 2, 7 and 19 cases: one pass, a partly filled pass, several passes."""
    a, da, c, f = orc.react_functions(k)
    nodes, Wo, tr = _reference(ne, M, n, k, with_c, max(NCASES))
    sel = [0, ne // 3, ne - 1]
    for nc in NCASES:
        got = {}
        for pm in (False, True):
            W, st = _multi(dev, nodes, M, n, a, da, c if with_c else None, f, nc, pm)
            got[pm] = W
            assert W.shape == (nc, ne, M) and st.shape == (nc, ne) and np.all(st == 0)
            e64 = max(orc.rel_l2_coef(W[j], Wo[j]).max() for j in range(nc))
            note(f"multi ne={ne} M={M} k={k:g} c={with_c} nc={nc} pm={pm} vs float64", e64, 1e-11)
            print(f"ne={ne} M={M} k={k:g} c={with_c} nc={nc} pm={pm}: vs float64 {e64:.2e}")
            assert e64 <= 1e-11
            if tr is not None:
                emp = max(orc.rel_l2_coef(W[j][sel], tr[j]).max() for j in range(nc))
                note(f"multi ne={ne} M={M} k={k:g} c={with_c} nc={nc} pm={pm} vs 60 digits", emp, 1e-13)
                print(f"    vs 60 digits {emp:.2e}")
                assert emp <= 1e-13
        assert max(orc.rel_l2_coef(got[True][j], got[False][j]).max() for j in range(nc)) <= 1e-12


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("ne,M,n", SHAPES)
def test_multi_vs_single_case_entry(dev, note, ne, M, n, with_c):
    """Each case within 1e-12 of ops.enhance_varcoef(..., c_values=...) run on that case alone (the bar
    test_gpu_react.py holds between variants)."""
    from hybrid_fem_lssvr_amd import ops
    a, da, c, f = orc.react_functions(1e4)
    nodes = np.linspace(-1, 1, ne + 1)
    nc = 7
    for pm in (False, True):
        x, U, ta, tda, F, tc, bc = _inputs(dev, nodes, n, a, da, c if with_c else None, f, nc, pm)
        W, st = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda, F, c_values=tc, bc=bc, point_major=pm,
                                  global_domain=(-1.0, 1.0))
        assert np.all(st.cpu().numpy() == 0)
        for j in range(nc):
            W1, st1 = ops.enhance_varcoef(x, U[j].contiguous(), M, GAMMA, n, ta, tda, F[j].contiguous(),
                                          c_values=tc, point_major=pm, global_domain=(-1.0, 1.0), bc=_case_bc(j))
            err = orc.rel_l2_coef(W[j].cpu().numpy(), W1.cpu().numpy()).max()
            note(f"multi vs single ne={ne} M={M} c={with_c} pm={pm} case {j}", err, 1e-12)
            assert err <= 1e-12 and np.all(st1.cpu().numpy() == 0)


# ---------------------------------------------------------------------------
# 3. odd sizes and shards
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,n", [(9, 16), (5, 8), (16, 24)])
@pytest.mark.parametrize("ne", [1, 63, 65, 129])
def test_multi_odd_sizes_and_shards(dev, ne, M, n):
    """Element counts off the wave / workgroup multiples; the same elements as an interior shard (no Dirichlet value
    may be used) and as the shard that holds only the right end (the right value of every case, no left one)."""
    a, da, c, f = orc.react_functions(1e4)
    nodes = np.linspace(-0.7, 0.9, ne + 1)
    nc = 3
    kw = dict(coef_a=a, coef_da=da, coef_c=c)
    for pm in (False, True):
        W, st = _multi(dev, nodes, M, n, a, da, c, f, nc, pm)
        Wi, sti = _multi(dev, nodes, M, n, a, da, c, f, nc, pm, elem_offset=3, ne_global=ne + 5,
                         global_domain=(-1.0, 1.0))
        Wr, str_ = _multi(dev, nodes, M, n, a, da, c, f, nc, pm, elem_offset=3, ne_global=ne + 3,
                          global_domain=(-9.0, float(nodes[-1])))
        assert np.all(st == 0) and np.all(sti == 0) and np.all(str_ == 0)
        for j in range(nc):
            bl, br = _case_bc(j)
            u, fj = _case_u(nodes, j), _case_f(f, j)
            Wo = orc.enhance_all(nodes, u, M, GAMMA, n, rhs=fj, bc_left=bl, bc_right=br, **kw)[0]
            assert orc.rel_l2_coef(W[j], Wo).max() <= 1e-11
            Wo = orc.enhance_all(np.concatenate([[-9.0], nodes, [9.0]]), np.concatenate([[0.0], u, [0.0]]), M, GAMMA,
                                 n, rhs=fj, global_domain=(-9.0, 9.0), elements=range(1, ne + 1), bc_left=bl,
                                 bc_right=br, **kw)[0]
            assert orc.rel_l2_coef(Wi[j], Wo).max() <= 1e-11
            Wo = orc.enhance_all(np.concatenate([[-9.0], nodes]), np.concatenate([[0.0], u]), M, GAMMA, n, rhs=fj,
                                 global_domain=(-9.0, float(nodes[-1])), elements=range(1, ne + 1), bc_left=bl,
                                 bc_right=br, **kw)[0]
            assert orc.rel_l2_coef(Wr[j], Wo).max() <= 1e-11
            if ne > 1:      # the right end took the case's Dirichlet value, not the nodal one
                assert not np.allclose(Wr[j][-1], Wi[j][-1], rtol=1e-9, atol=0.0)


# ---------------------------------------------------------------------------
# 4. degrees above the lane kernel: the single-case kernel once per case
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("ne,M,n,bar", [(40, 17, 24, 1e-11), (20, 26, 40, 1e-10)])
def test_multi_degrees_17_and_26(dev, note, ne, M, n, bar, with_c):
    a, da, c, f = orc.react_functions(1e4)
    nodes, Wo, _ = _reference(ne, M, n, 1e4, with_c, 3)
    for pm in (False, True):
        W, st = _multi(dev, nodes, M, n, a, da, c if with_c else None, f, 3, pm)
        assert np.all(st == 0)
        err = max(orc.rel_l2_coef(W[j], Wo[j]).max() for j in range(3))
        note(f"multi ne={ne} M={M} c={with_c} pm={pm} vs float64", err, bar)
        assert err <= bar


# ---------------------------------------------------------------------------
# 5. per-case fallback
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("ne,M,n", [(257, 9, 16), (130, 16, 24)])
def test_multi_fallback_of_an_element_hits_every_case(dev, ne, M, n, pm):
    """NaN in a_values of two elements: the factorisation breaks down, every case of those elements gets the linear
    interpolant of its own (g_l, g_r) and status 1, fail_count = 2 ncases; every other row is as without the NaN."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    a, da, c, f = orc.react_functions(1e4)
    nc, bad = 7, [3, ne - 2]
    nodes, Wo, _ = _reference(ne, M, n, 1e4, True, max(NCASES))
    x, U, ta, tda, F, tc, bc = _inputs(dev, nodes, n, a, da, c, f, nc, pm)
    for e in bad:
        if pm:
            ta[n // 2, e] = float("nan")
        else:
            ta[e, n // 2] = float("nan")
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    W, st = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda, F, c_values=tc, bc=bc, point_major=pm,
                              global_domain=(-1.0, 1.0), fail_count=cnt)
    W, st = W.cpu().numpy(), st.cpu().numpy()
    want = np.zeros((nc, ne), dtype=np.int32)
    want[:, bad] = 1
    assert np.array_equal(st, want) and int(cnt.item()) == 2 * nc
    good = np.setdiff1d(np.arange(ne), bad)
    for j in range(nc):
        u = _case_u(nodes, j)
        for e in bad:
            assert np.array_equal(W[j, e], orc.linear_fallback_coef(u[e], u[e + 1], M))
        assert orc.rel_l2_coef(W[j][good], Wo[j][good]).max() <= 1e-11


@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("ne,M,n", [(257, 9, 16), (130, 16, 24)])
def test_multi_fallback_of_one_case_stays_with_it(dev, ne, M, n, pm):
    """NaN in f of case 1, element 5: only (1, 5) falls back, fail_count = 1, every other row is untouched."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    a, da, c, f = orc.react_functions(1e4)
    nc = 7
    nodes, Wo, _ = _reference(ne, M, n, 1e4, True, max(NCASES))
    x, U, ta, tda, F, tc, bc = _inputs(dev, nodes, n, a, da, c, f, nc, pm)
    if pm:
        F[1, 2, 5] = float("nan")
    else:
        F[1, 5, 2] = float("nan")
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    W, st = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda, F, c_values=tc, bc=bc, point_major=pm,
                              global_domain=(-1.0, 1.0), fail_count=cnt)
    W, st = W.cpu().numpy(), st.cpu().numpy()
    want = np.zeros((nc, ne), dtype=np.int32)
    want[1, 5] = 1
    assert np.array_equal(st, want) and int(cnt.item()) == 1
    u = _case_u(nodes, 1)
    assert np.array_equal(W[1, 5], orc.linear_fallback_coef(u[5], u[6], M))
    for j in range(nc):
        keep = np.arange(ne) != 5 if j == 1 else np.ones(ne, dtype=bool)
        assert orc.rel_l2_coef(W[j][keep], Wo[j][keep]).max() <= 1e-11


# ---------------------------------------------------------------------------
# 6. no stray writes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("ne,M,n", [(130, 9, 16), (65, 16, 24), (63, 2, 4), (40, 17, 24)])
def test_multi_writes_only_its_rows(dev, ne, M, n, pm):
    """W and status carved out of sentinel-filled buffers with guard rows before and after: the guards survive, every
    row inside is written; NULL status and NULL fail_count both run and give the same W."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    a, da, c, f = orc.react_functions(1.0)
    nc, g = 5, 3
    nodes = np.linspace(-1, 1, ne + 1)
    x, U, ta, tda, F, tc, bc = _inputs(dev, nodes, n, a, da, c, f, nc, pm)
    wbuf = torch.full(((nc * ne + 2 * g) * M,), -777.0, dtype=torch.float64, device=dev)
    sbuf = torch.full((nc * ne + 2 * g,), -7, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    W, st = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda, F, c_values=tc, bc=bc, point_major=pm,
                              global_domain=(-1.0, 1.0), out=wbuf[g * M:(g + nc * ne) * M],
                              status=sbuf[g:g + nc * ne], fail_count=cnt)
    hw, hs = wbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert np.all(hw[:g * M] == -777.0) and np.all(hw[(g + nc * ne) * M:] == -777.0)
    assert np.all(hs[:g] == -7) and np.all(hs[g + nc * ne:] == -7)
    assert not np.any(hw[g * M:(g + nc * ne) * M] == -777.0) and np.all(hs[g:g + nc * ne] == 0)
    assert int(cnt.item()) == 0
    W2, st2 = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda, F, c_values=tc, bc=bc, point_major=pm,
                                global_domain=(-1.0, 1.0), status=False, fail_count=None)
    assert st2 is None and np.array_equal(W2.cpu().numpy().ravel(), hw[g * M:(g + nc * ne) * M])


# ---------------------------------------------------------------------------
# 7. facade
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("plain", [False, True])
def test_facade_solve_many(dev, note, plain):
    """Three right-hand sides on 60 elements, degree 8: each returned solution, on 201 points, within 1e-10 ||u|| of
    a separate solve() with that rhs (the bar of test_facade_solve_with_coef_and_reaction); the solver's own state is
    what it was."""
    import hybrid_fem_lssvr_amd as pkg
    a, da, c, f = orc.react_functions(1e4)
    kw = dict(lssvr_M=9, lssvr_gamma=GAMMA, n_colloc=16, nquad=3)
    if not plain:
        kw.update(coef=(a, da), reaction=c)
    fs = [_case_f(f, j) for j in range(3)]
    s = pkg.FEMLSSVRPrimalSolver(61, rhs=fs[1], **kw)
    s.solve()
    state = (s.rhs, s.fem_values.copy(), s.enhanced, s.enhanced.W.clone(), s.lssvr_functions, s.bands)
    sols = s.solve_many(fs)
    assert len(sols) == 3 and all(isinstance(v, pkg.solver.EnhancedSolution) for v in sols)
    assert s.rhs is state[0] and np.array_equal(s.fem_values, state[1]) and s.enhanced is state[2]
    assert bool((s.enhanced.W == state[3]).all().item()) and s.lssvr_functions is state[4] and s.bands is state[5]
    xq = np.linspace(-1, 1, 201)
    for j, sol in enumerate(sols):
        one = pkg.FEMLSSVRPrimalSolver(61, rhs=fs[j], **kw)
        one.solve()
        ref = one.evaluate_solution(xq)
        err = np.linalg.norm(sol.evaluate(xq) - ref) / np.linalg.norm(ref)
        note(f"solve_many plain={plain} case {j}: distance to solve() / ||u||", err, 1e-10)
        assert err <= 1e-10 and sol.n_fallback == 0
    # one Dirichlet pair per case: the end elements take them
    sols = s.solve_many(fs[:2], bc=[(0.25, -0.5), (0.0, 1.0)])
    for sol, (bl, br) in zip(sols, [(0.25, -0.5), (0.0, 1.0)]):
        ends = sol.evaluate(np.array([-1.0, 1.0]))
        assert abs(ends[0] - bl) <= 1e-6 and abs(ends[1] - br) <= 1e-6


# ---------------------------------------------------------------------------
# 8. validation on the device path
# ---------------------------------------------------------------------------
def test_multi_rejects_fewer_points_than_bubbles(dev):
    from hybrid_fem_lssvr_amd import _capi
    a, da, c, f = orc.react_functions(1.0)
    nodes = np.linspace(-1, 1, 11)
    for M, n in ((9, 6), (22, 19)):
        with pytest.raises(_capi.LssvrHipError, match="M-2") as ei:
            _multi(dev, nodes, M, n, a, da, c, f, 2, True)
        assert "(-5)" in str(ei.value)          # LSSVR_ERR_SOLVER
