"""GPU: every degree of the three lane-per-element kernels that read coefficient tables -- the several-load-case one
(``enhance_multi_kernel``, M = 2 .. 16), the reaction one (``enhance_small_react_kernel``, M = 2 .. 16) and the
variable-coefficient one (``enhance_small_body<M, RHS, VC = true>``, M = 2 .. 22) -- each its own template
instantiation with its own unrolling and register allocation.

Inputs under which a single wrong degree, a wrong tail of a prefetch / staging loop or a mix-up of per-element
quantities shows: a graded mesh of 70 elements (element length 1.5e-3 .. 4.8e-2, about 33x; two waves, the second with
6 live lanes), an odd collocation count n = 2M - 1 that no prefetch or staging depth divides (M = 10 also with n = 18
and n = 20: residues 2 and 0 mod 4), nodal values that are not zero at the ends and a non-zero Dirichlet pair, for the
several-case kernel one per case.  Every expected value is the float64 restatement's (oracle/lssvr_oracle.py) or the
60-digit solve's (oracle/closed_form_mp.py) under the project's own bars: 1e-11, 1e-13, 1e-12 between layouts and
between entries."""
import functools

import numpy as np
import pytest

from oracle import closed_form_mp as cf
from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu

GAMMA = 1e4
NE = 70
SEL = [0, NE // 3, NE - 1]
NCASES = [1, 2, 3, 5, 9]    # for every cases-per-pass count 1, 2, 3, 4, 8: a full pass, a partly filled one, and a
#                             trailing pass of one case (the NC = 1 instantiation)
KS = [1e4, 1.0]
LARGE_NE = 233_100          # at M = 9: 2 097 900 doubles per case, above the 2^21 up to which W is written through
assert LARGE_NE * 9 > 2 ** 21 and LARGE_NE % 64 == 12


def _n_of(M):
    return max(3, 2 * M - 1)


def _degrees(top):
    """(M, n) of the sweep: n = 2M - 1, and M = 10 also with n = 18, 20."""
    return [(M, _n_of(M)) for M in range(2, top + 1)] + [(10, 18), (10, 20)]


def _graded(ne):
    s = np.arange(ne + 1) / ne
    nodes = -1.0 + 2.0 * s ** 1.7
    nodes[-1] = 1.0
    return nodes


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


def _single(dev, nodes, M, n, a, da, c, f, pm, j=0, **kw):
    """Case ``j`` alone through the single-case entry (the reaction kernel with ``c``, the variable-coefficient one
    without); returns device tensors."""
    from hybrid_fem_lssvr_amd import ops
    x = _t(nodes, dev)
    xc = ops.colloc_points(x, n).cpu().numpy()
    ta, tda, tf = (_t(_tab(fn, xc, pm), dev) for fn in (a, da, _case_f(f, j)))
    tc = None if c is None else _t(_tab(c, xc, pm), dev)
    kw.setdefault("global_domain", (float(nodes[0]), float(nodes[-1])))
    kw.setdefault("bc", _case_bc(j))
    return ops.enhance_varcoef(x, _t(_case_u(nodes, j), dev), M, GAMMA, n, ta, tda, tf, c_values=tc, point_major=pm,
                               **kw)


@functools.lru_cache(maxsize=None)
def _reference(M, n, k, with_c, j):
    """(oracle W of case j on the graded mesh, 60-digit rows of elements SEL | None): computed once, shared by the
    several-case and the single-case tests (the latter run case 0), never written."""
    a, da, c, f = orc.react_functions(k)
    nodes = _graded(NE)
    bl, br = _case_bc(j)
    kw = dict(coef_a=a, coef_da=da, coef_c=c if with_c else None, bc_left=bl, bc_right=br)
    Wo, st = orc.enhance_all(nodes, _case_u(nodes, j), M, GAMMA, n, rhs=_case_f(f, j), **kw)
    assert np.all(st == 0)
    Wo.setflags(write=False)
    tr = None
    # (M = 2 without c: the 60-digit solve reads a_k back from the column of L_2, which such a system lacks)
    if cf.HAVE_MP and (M > 2 or with_c):
        tr = cf.truth_all(nodes, _case_u(nodes, j), M, GAMMA, n, _case_f(f, j), elements=SEL, **kw)
        tr.setflags(write=False)
    return Wo, tr


@functools.lru_cache(maxsize=None)
def _shard_reference(M, n, k):
    """Oracle W of case 0's elements as the interior of a longer mesh: no Dirichlet value applies."""
    a, da, c, f = orc.react_functions(k)
    nodes = _graded(NE)
    Wo, st = orc.enhance_all(np.concatenate([[-9.0], nodes, [9.0]]), np.concatenate([[0.0], _case_u(nodes, 0), [0.0]]),
                             M, GAMMA, n, rhs=_case_f(f, 0), global_domain=(-9.0, 9.0), elements=range(1, NE + 1),
                             coef_a=a, coef_da=da, coef_c=c)
    assert np.all(st == 0)
    Wo.setflags(write=False)
    return Wo


def _check(note, what, W, Wo, tr):
    """1e-11 against the restatement, 1e-13 against 60 digits on SEL; each distance recorded first."""
    e64 = orc.rel_l2_coef(W, Wo).max()
    note(f"{what} vs float64", e64, 1e-11)
    print(f"{what}: vs float64 {e64:.2e}")
    emp = None
    if tr is not None:
        emp = orc.rel_l2_coef(W[SEL], tr).max()
        note(f"{what} vs 60 digits", emp, 1e-13)
        print(f"    vs 60 digits {emp:.2e}")
    assert e64 <= 1e-11
    assert emp is None or emp <= 1e-13


# ---------------------------------------------------------------------------
# 1. several load cases: every degree, every pass shape
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("M,n", _degrees(16))
def test_multi_every_degree(dev, note, M, n, with_c):
    """1, 2, 3, 5 and 9 cases in both table layouts: every case within 1e-11 of the restatement called with that
    case's own f, u and Dirichlet pair and within 1e-13 of the 60-digit solve; the layouts within 1e-12 of each other;
    at 5 cases each case within 1e-12 of the single-case entry run on it alone.  (k = 1e4 only: nine references per
    degree are what this test costs.)"""
    from hybrid_fem_lssvr_amd import ops
    k = 1e4
    a, da, c, f = orc.react_functions(k)
    if not with_c:
        c = None
    nodes = _graded(NE)
    ref = [_reference(M, n, k, with_c, j) for j in range(max(NCASES))]
    for nc in NCASES:
        got = {}
        for pm in (False, True):
            x, U, ta, tda, F, tc, bc = _inputs(dev, nodes, n, a, da, c, f, nc, pm)
            W, st = ops.enhance_multi(x, U, M, GAMMA, n, ta, tda, F, c_values=tc, bc=bc, point_major=pm,
                                      global_domain=(-1.0, 1.0))
            W, st = W.cpu().numpy(), st.cpu().numpy()
            got[pm] = W
            assert W.shape == (nc, NE, M) and st.shape == (nc, NE) and np.all(st == 0)
            for j in range(nc):
                _check(note, f"multi M={M} n={n} c={with_c} nc={nc} pm={pm} case {j}", W[j], *ref[j])
            if nc == 5:
                for j in range(nc):
                    W1, st1 = _single(dev, nodes, M, n, a, da, c, f, pm, j)
                    err = orc.rel_l2_coef(W[j], W1.cpu().numpy()).max()
                    note(f"multi vs single M={M} n={n} c={with_c} pm={pm} case {j}", err, 1e-12)
                    assert err <= 1e-12 and np.all(st1.cpu().numpy() == 0)
        err = max(orc.rel_l2_coef(got[True][j], got[False][j]).max() for j in range(nc))
        note(f"multi M={M} n={n} c={with_c} nc={nc} between layouts", err, 1e-12)
        assert err <= 1e-12


# ---------------------------------------------------------------------------
# 2. reaction rows, one case: every lane degree
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("M,n", _degrees(16))
def test_react_every_lane_degree(dev, note, M, n, k):
    """Both layouts within 1e-11 of the restatement, 1e-13 of the 60-digit solve and 1e-12 of each other; the same
    elements as an interior shard (elem_offset > 0, ne_global > ne, a wider global domain: the Dirichlet pair that is
    passed must not be used) within 1e-11 of the restatement of that longer mesh."""
    a, da, c, f = orc.react_functions(k)
    nodes = _graded(NE)
    Wo, tr = _reference(M, n, k, True, 0)
    Ws = _shard_reference(M, n, k)
    got, gots = {}, {}
    for pm in (False, True):
        W, st = _single(dev, nodes, M, n, a, da, c, f, pm)
        got[pm] = W.cpu().numpy()
        assert np.all(st.cpu().numpy() == 0)
        _check(note, f"react M={M} n={n} k={k:g} pm={pm}", got[pm], Wo, tr)
        W, st = _single(dev, nodes, M, n, a, da, c, f, pm, elem_offset=3, ne_global=NE + 5,
                        global_domain=(-9.0, 9.0), bc=(7.0, -3.0))
        gots[pm] = W.cpu().numpy()
        assert np.all(st.cpu().numpy() == 0)
        err = orc.rel_l2_coef(gots[pm], Ws).max()
        note(f"react shard M={M} n={n} k={k:g} pm={pm} vs float64", err, 1e-11)
        assert err <= 1e-11
    for what, g in (("", got), (" shard", gots)):
        err = orc.rel_l2_coef(g[True], g[False]).max()
        note(f"react{what} M={M} n={n} k={k:g} between layouts", err, 1e-12)
        assert err <= 1e-12
    # the end elements took the Dirichlet pair in the first run and the nodal values in the shard
    assert not np.allclose(got[True][0], gots[True][0], rtol=1e-9, atol=0.0)
    assert not np.allclose(got[True][-1], gots[True][-1], rtol=1e-9, atol=0.0)


# ---------------------------------------------------------------------------
# 3. variable coefficient, one case: every lane degree
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("M,n", _degrees(22))
def test_varcoef_every_lane_degree(dev, note, M, n, k):
    """c_values = None, M = 2 .. 22: within 1e-11 of the restatement and 1e-13 of the 60-digit solve; the two layouts
    bit-equal, as test_varcoef_table_layouts_agree holds them.  (k enters through the right-hand side only.)"""
    import torch
    a, da, _, f = orc.react_functions(k)
    nodes = _graded(NE)
    Wo, tr = _reference(M, n, k, False, 0)
    got = {}
    for pm in (False, True):
        got[pm], st = _single(dev, nodes, M, n, a, da, None, f, pm)
        assert np.all(st.cpu().numpy() == 0)
        _check(note, f"varcoef M={M} n={n} k={k:g} pm={pm}", got[pm].cpu().numpy(), Wo, tr)
    assert torch.equal(got[True], got[False])


# ---------------------------------------------------------------------------
# 4. outputs above 2^21 doubles per case: the non-temporal store branch
# ---------------------------------------------------------------------------
def test_multi_and_react_large_output(dev, note):
    """M = 9, n = 16, 233 100 elements (ne M = 2 097 900 > 2^21), 5 cases with c on a graded mesh (element length
    1 : 60, linear in the element index, so the smallest element is about as long as those of a uniform mesh of 1e7
    elements): status all zero, every case within 1e-12 of the single-case reaction entry at the same size, both
    within 1e-11 of the restatement on about 200 elements -- the ends, both sides of wave and workgroup boundaries,
    the whole last wave and a random rest; guard rows before and after W and status survive."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    M, n, ne, nc, g = 9, 16, LARGE_NE, 5, 3
    a, da, c, f = orc.react_functions(1e4)
    s = np.arange(ne + 1) / ne
    nodes = -1.0 + 2.0 * (s + 29.5 * s * s) / 30.5
    nodes[-1] = 1.0
    last = 64 * (ne // 64)                                  # the last wave: 12 live lanes
    bounds = [64, 128, 256, 512, 256 * (ne // 512), 256 * (ne // 512) + 64, 256 * (ne // 256), last - 64, last]
    sel = {0, 1, ne - 1} | {b + d for b in bounds for d in (-1, 0)} | set(range(last, ne))
    sel |= set(np.random.default_rng(9).integers(0, ne, 170).tolist())
    sel = np.array(sorted(sel))
    assert 150 <= len(sel) <= 220
    x = _t(nodes, dev)
    xc = ops.colloc_points(x, n).cpu().numpy()
    ta, tda, tc, f0 = (np.asarray(fn(xc), dtype=np.float64) for fn in (a, da, c, f))
    Fh = np.stack([(1.0 + 0.25 * j) * f0 + 0.5 * j for j in range(nc)])          # _case_f on the table
    Uh = np.stack([_case_u(nodes, j) for j in range(nc)])
    U, bc = _t(Uh, dev), _t(np.array([_case_bc(j) for j in range(nc)]), dev)
    Wo = []
    for j in range(nc):
        bl, br = _case_bc(j)
        w, st = orc.enhance_all(nodes, Uh[j], M, GAMMA, n, rhs=_case_f(f, j), elements=sel, coef_a=a, coef_da=da,
                                coef_c=c, bc_left=bl, bc_right=br)
        assert np.all(st == 0)
        Wo.append(w)
    got = {}
    for pm in (False, True):
        lay = (lambda t: t.T) if pm else (lambda t: t)
        da_, dda, dc = (_t(lay(t), dev) for t in (ta, tda, tc))
        F = _t(np.stack([lay(Fh[j]) for j in range(nc)]), dev)
        wbuf = torch.full(((nc * ne + 2 * g) * M,), -777.0, dtype=torch.float64, device=dev)
        sbuf = torch.full((nc * ne + 2 * g,), -7, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        W, st = ops.enhance_multi(x, U, M, GAMMA, n, da_, dda, F, c_values=dc, bc=bc, point_major=pm,
                                  global_domain=(-1.0, 1.0), out=wbuf[g * M:(g + nc * ne) * M],
                                  status=sbuf[g:g + nc * ne], fail_count=cnt)
        hw, hs = wbuf.cpu().numpy(), sbuf.cpu().numpy()
        assert np.all(hw[:g * M] == -777.0) and np.all(hw[(g + nc * ne) * M:] == -777.0)
        assert np.all(hs[:g] == -7) and np.all(hs[g + nc * ne:] == -7)
        assert np.all(hs[g:g + nc * ne] == 0) and int(cnt.item()) == 0
        W = hw[g * M:(g + nc * ne) * M].reshape(nc, ne, M)
        assert not np.any(W == -777.0)
        got[pm] = W
        for j in range(nc):
            wb1 = torch.full(((ne + 2 * g) * M,), -777.0, dtype=torch.float64, device=dev)
            sb1 = torch.full((ne + 2 * g,), -7, dtype=torch.int32, device=dev)
            ops.enhance_varcoef(x, U[j].contiguous(), M, GAMMA, n, da_, dda, F[j].contiguous(), c_values=dc,
                                point_major=pm, global_domain=(-1.0, 1.0), bc=_case_bc(j), out=wb1[g * M:(g + ne) * M],
                                status=sb1[g:g + ne])
            h1, s1 = wb1.cpu().numpy(), sb1.cpu().numpy()
            assert np.all(h1[:g * M] == -777.0) and np.all(h1[(g + ne) * M:] == -777.0)
            assert np.all(s1[:g] == -7) and np.all(s1[g + ne:] == -7) and np.all(s1[g:g + ne] == 0)
            W1 = h1[g * M:(g + ne) * M].reshape(ne, M)
            err = orc.rel_l2_coef(W[j], W1).max()
            e64 = orc.rel_l2_coef(W[j][sel], Wo[j]).max()
            e641 = orc.rel_l2_coef(W1[sel], Wo[j]).max()
            note(f"large multi vs single pm={pm} case {j}", err, 1e-12)
            note(f"large multi pm={pm} case {j} vs float64 ({len(sel)} elements)", e64, 1e-11)
            note(f"large react pm={pm} case {j} vs float64 ({len(sel)} elements)", e641, 1e-11)
            print(f"pm={pm} case {j}: multi vs single {err:.2e}, vs float64 {e64:.2e} / {e641:.2e}")
            assert err <= 1e-12 and e64 <= 1e-11 and e641 <= 1e-11
    err = max(orc.rel_l2_coef(got[True][j], got[False][j]).max() for j in range(nc))
    note("large multi between layouts", err, 1e-12)
    assert err <= 1e-12
