"""GPU: hp refinement for coefficient, reaction and convection problems -- the element-list
entries ``lssvr_colloc_points_subset`` and ``lssvr_enhance_react_subset`` on a graded mesh of 131 elements (odd: three
waves with a partial last one, an MFMA pair whose second half idles) with a shuffled list of 67 of them, against the
whole-mesh entries (bit for bit where the kernel is lane-per-element) and the float64 restatement
(oracle/lssvr_oracle.py) under the bars of tests/test_gpu_react.py; then ``element_degrees`` and
``solve_adaptive(mode="hp")`` through the facade."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import convection_rules as cr
import periodic_rules as pr
from oracle import lssvr_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA, NE, NSUB, LDW = 1e4, 131, 67, 33
BC = (0.3, -0.7)
SENT = -777.25                      # rows that are not listed keep this bit pattern
LANE_M, MFMA_M = (2, 3, 8, 16), (17, 23, 33)
A, DA, C, F = orc.react_functions(1e4)


def _n(M):
    return max(12, 2 * M)


def _bar(M):
    """tests/test_gpu_react.py's bars against the float64 restatement."""
    return 1e-11 if M <= 22 else 1e-10


def _lane(M, with_c):
    """Whether (M, c table or not) runs the lane-per-element kernel: up to kReactSmallMaxM = 16 with a c table, up to
    kSmallMaxM = 22 without.  Its rows do not depend on what else is in the launch."""
    return M <= (16 if with_c else 22)


@functools.lru_cache(maxsize=None)
def _mesh():
    """(nodes[132], nodal values, ids[67]): element lengths random within a factor 3 and graded by another factor 8
    from left to right; a shuffled strict subset of the elements that holds both end elements."""
    rng = np.random.default_rng(23)
    h = rng.uniform(0.5, 1.5, NE) * 8.0 ** np.linspace(0.0, 1.0, NE)
    nodes = np.concatenate([[-1.0], -1.0 + 2.0 * np.cumsum(h) / h.sum()])
    nodes[-1] = 1.0
    values = np.sin(np.pi * nodes) + 0.25 * np.cos(3.0 * nodes)
    ids = np.concatenate([[0, NE - 1], 1 + rng.choice(NE - 2, NSUB - 2, replace=False)])
    ids = rng.permutation(ids).astype(np.int64)
    assert len(set(ids.tolist())) == NSUB and 0 in ids and NE - 1 in ids and ids[0] not in (0, NE - 1)
    return nodes, values, ids


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _full_tables(dev, M, pm, with_c):
    """The whole-mesh tables (a, a', f, c | None) in the given layout, and the element-major host copies."""
    from hybrid_fem_lssvr_amd import ops
    xc = ops.colloc_points(_t(_mesh()[0], dev), _n(M)).cpu().numpy()
    host = [np.asarray(fn(xc), dtype=np.float64) for fn in ((A, DA, F, C) if with_c else (A, DA, F))]
    devt = [_t(t.T if pm else t, dev) for t in host] + ([] if with_c else [None])
    return devt, host + ([] if with_c else [None])


def _sub_tables(dev, host, ids, pm):
    return [None if t is None else _t(t[ids].T if pm else t[ids], dev) for t in host]


@functools.lru_cache(maxsize=None)
def _oracle(M, with_c, silent=False):
    """Rows of the listed elements by ``element_system`` + ``solve_bc_eliminated``; ``silent``: no Dirichlet flag
    fires (the global domain touches no element)."""
    nodes, values, ids = _mesh()
    gd = (-9.0, 9.0) if silent else (nodes[0], nodes[-1])
    return orc.enhance_all(nodes, values, M, GAMMA, _n(M), rhs=F, global_domain=gd, coef_a=A, coef_da=DA,
                           coef_c=C if with_c else None, bc_left=BC[0], bc_right=BC[1], elements=ids)[0]


def _outputs(dev, ldw=LDW):
    import torch
    W = torch.full((NE, ldw), SENT, dtype=torch.float64, device=dev)
    st = torch.full((NE,), -5, dtype=torch.int32, device=dev)
    return W, st, torch.zeros(1, dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------------
# 1. lssvr_colloc_points_subset
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("nsub", [1, 64, 65, 131])
def test_colloc_points_subset_is_the_gathered_whole_mesh_table(dev, nsub, pm):
    from hybrid_fem_lssvr_amd import ops
    nodes = _mesh()[0]
    ids = np.random.default_rng(nsub).permutation(NE)[:nsub].astype(np.int64)
    x = _t(nodes, dev)
    for n in (2, 12, 46):
        want = ops.colloc_points(x, n).cpu().numpy()[ids]
        got = ops.colloc_points_subset(x, _t(ids, dev), n, point_major=pm).cpu().numpy()
        assert got.shape == ((n, nsub) if pm else (nsub, n))
        assert np.array_equal(_bits(got.T if pm else got), _bits(want))
    # no list: every element in order
    got = ops.colloc_points_subset(x, None, 12, point_major=pm).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(ops.colloc_points(x, 12, point_major=pm).cpu().numpy()))


def test_colloc_points_subset_skips_ids_outside_the_mesh(dev):
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    nodes = _mesh()[0]
    x = _t(nodes, dev)
    ids = _t(np.array([5, -1, 7, NE], dtype=np.int64), dev)
    want = ops.colloc_points(x, 12).cpu().numpy()
    for layout in (0, 1):
        xc = torch.full((4 * 12,), SENT, dtype=torch.float64, device=dev)
        rc = _capi.load().lssvr_colloc_points_subset(x.data_ptr(), NE, ids.data_ptr(), 4, 12, layout, xc.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        got = xc.cpu().numpy().reshape((12, 4) if layout else (4, 12))
        got = got.T if layout else got
        assert np.array_equal(_bits(got[[0, 2]]), _bits(want[[5, 7]])) and np.all(got[[1, 3]] == SENT)


# ---------------------------------------------------------------------------
# 2. lssvr_enhance_react_subset against the whole-mesh entry and the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("pm", [False, True])
@pytest.mark.parametrize("M", LANE_M + MFMA_M)
def test_subset_rows_against_whole_mesh_and_restatement(dev, note, M, pm, with_c):
    """Listed rows: the rows of the whole-mesh entry on the same data, bit for bit for the lane kernels; for the MFMA
    kernel (its boundary rows take the series or the recurrence per PAIR of launch neighbours, ``__all(series_ok)``)
    and for the lane kernels as well, the restatement under tests/test_gpu_react.py's bar.  Everything that is not
    listed keeps its sentinel; status is written by mesh index."""
    from hybrid_fem_lssvr_amd import ops
    nodes, values, ids = _mesh()
    n = _n(M)
    x, u, idt = _t(nodes, dev), _t(values, dev), _t(ids, dev)
    gd = (nodes[0], nodes[-1])
    (ta, tda, tf, tc), host = _full_tables(dev, M, pm, with_c)
    Wf, stf = ops.enhance_varcoef(x, u, M, GAMMA, n, ta, tda, tf, point_major=pm, c_values=tc, global_domain=gd, bc=BC)
    Wf, stf = Wf.cpu().numpy(), stf.cpu().numpy()
    sa, sda, sf, sc = _sub_tables(dev, host, ids, pm)
    W, st, fc = _outputs(dev)
    out = ops.enhance_varcoef_subset(x, u, M, GAMMA, n, W, sa, sda, sf, elem_ids=idt, c_values=sc, point_major=pm,
                                     global_domain=gd, bc=BC, status=st, fail_count=fc)
    assert out is W
    W, st = W.cpu().numpy(), st.cpu().numpy()
    rest = np.setdiff1d(np.arange(NE), ids)
    assert np.all(_bits(W[rest]) == _bits(np.float64(SENT))) and np.all(_bits(W[ids, M:]) == _bits(np.float64(SENT)))
    assert np.all(st[rest] == -5) and np.all(st[ids] == 0) and np.all(stf == 0) and int(fc.item()) == 0
    same = np.array_equal(_bits(W[ids, :M]), _bits(Wf[ids]))
    err_full = orc.rel_l2_coef(W[ids, :M], Wf[ids]).max()
    err = orc.rel_l2_coef(W[ids, :M], _oracle(M, with_c)).max()
    tag = f"M={M} pm={pm} c={with_c}"
    note(f"subset {tag} vs restatement", err, _bar(M))
    note(f"subset {tag} vs whole mesh (bit for bit = {int(same)})", err_full)
    print(f"{tag}: vs restatement {err:.2e} (bar {_bar(M):.0e}), vs whole mesh {err_full:.2e}, bits equal {same}")
    if _lane(M, with_c):
        assert same
    assert err <= _bar(M)
    assert orc.rel_l2_coef(Wf[ids], _oracle(M, with_c)).max() <= _bar(M)


@pytest.mark.parametrize("M", [8, 23])
def test_dirichlet_flags_follow_the_mesh_index(dev, M):
    """Elements 0 and 130 take the Dirichlet values wherever they stand in the list (neither is first or last here);
    elem_offset = 1, ne_global = ne + 2 -- the periodic convention -- silences both."""
    from hybrid_fem_lssvr_amd import ops
    from numpy.polynomial import legendre as L
    nodes, values, ids = _mesh()
    pm, n = M <= 22, _n(M)
    x, u, idt = _t(nodes, dev), _t(values, dev), _t(ids, dev)
    tabs = _sub_tables(dev, _full_tables(dev, M, pm, True)[1], ids, pm)
    rows = {}
    for silent, kw in ((False, {}), (True, dict(elem_offset=1, ne_global=NE + 2))):
        W, st, fc = _outputs(dev)
        ops.enhance_varcoef_subset(x, u, M, GAMMA, n, W, *tabs[:3], elem_ids=idt, c_values=tabs[3], point_major=pm,
                                   global_domain=(nodes[0], nodes[-1]), bc=BC, status=st, fail_count=fc, **kw)
        W = W.cpu().numpy()[:, :M]
        assert int(fc.item()) == 0
        assert orc.rel_l2_coef(W[ids], _oracle(M, True, silent)).max() <= _bar(M)
        rows[silent] = W
    ends = lambda W: (L.legval(-1.0, W[0]), L.legval(1.0, W[NE - 1]))               # noqa: E731
    assert np.allclose(ends(rows[False]), BC, rtol=0, atol=1e-12)
    assert np.allclose(ends(rows[True]), (values[0], values[-1]), rtol=0, atol=1e-12)
    if _lane(M, True):                   # an element away from the ends does not see the flags of its launch neighbours
        inner = ids[(ids != 0) & (ids != NE - 1)]
        assert np.array_equal(_bits(rows[False][inner]), _bits(rows[True][inner]))


@pytest.mark.parametrize("M", [8, 23])
def test_per_element_gamma(dev, note, M):
    """gamma_values[mesh index] spanning 1e2 .. 1e8 replaces the scalar: every listed row matches the restatement at
    its own gamma."""
    from hybrid_fem_lssvr_amd import ops
    nodes, values, ids = _mesh()
    pm, n = M <= 22, _n(M)
    gam = 10.0 ** np.random.default_rng(5).uniform(2.0, 8.0, NE)
    gam[[0, NE - 1]] = (1e2, 1e8)
    x, u, idt = _t(nodes, dev), _t(values, dev), _t(ids, dev)
    tabs = _sub_tables(dev, _full_tables(dev, M, pm, True)[1], ids, pm)
    W, st, fc = _outputs(dev)
    ops.enhance_varcoef_subset(x, u, M, 1.0, n, W, *tabs[:3], elem_ids=idt, c_values=tabs[3], point_major=pm,
                               gamma_values=_t(gam, dev), global_domain=(nodes[0], nodes[-1]), bc=BC, status=st,
                               fail_count=fc)
    W = W.cpu().numpy()
    want = np.array([orc.enhance_all(nodes, values, M, gam[i], n, rhs=F, global_domain=(nodes[0], nodes[-1]), coef_a=A,
                                     coef_da=DA, coef_c=C, bc_left=BC[0], bc_right=BC[1], elements=[i])[0][0]
                     for i in ids])
    err = orc.rel_l2_coef(W[ids, :M], want).max()
    note(f"per-element gamma M={M} vs restatement", err, _bar(M))
    print(f"per-element gamma M={M}: {err:.2e}")
    assert int(fc.item()) == 0 and np.all(st.cpu().numpy()[ids] == 0)
    assert err <= _bar(M)


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("M", [8, 23])
def test_ids_outside_the_mesh_touch_nothing(dev, M, with_c):
    """Ids -1 and ne_mesh: their rows, their status and the mesh are left alone, fail_count counts both; the two valid
    ids of the same launch (one of them the pair neighbour of a skipped id in the MFMA kernel) get their rows."""
    from hybrid_fem_lssvr_amd import ops
    nodes, values, _ = _mesh()
    pm, n = M <= 22, _n(M)
    ids = np.array([5, -1, 7, NE], dtype=np.int64)
    x, u = _t(nodes, dev), _t(values, dev)
    host = _full_tables(dev, M, pm, with_c)[1]
    tabs = _sub_tables(dev, host, np.array([5, 0, 7, 0]), pm)
    W, st, fc = _outputs(dev)
    ops.enhance_varcoef_subset(x, u, M, GAMMA, n, W, *tabs[:3], elem_ids=_t(ids, dev), c_values=tabs[3],
                               point_major=pm, global_domain=(nodes[0], nodes[-1]), bc=BC, status=st, fail_count=fc)
    W, st = W.cpu().numpy(), st.cpu().numpy()
    assert int(fc.item()) == 2
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(nodes)) and np.array_equal(_bits(u.cpu().numpy()), _bits(values))
    rest = np.setdiff1d(np.arange(NE), [5, 7])
    assert np.all(W[rest] == SENT) and np.all(W[[5, 7], M:] == SENT) and np.all(st[rest] == -5)
    assert np.all(st[[5, 7]] == 0)
    want = orc.enhance_all(nodes, values, M, GAMMA, n, rhs=F, global_domain=(nodes[0], nodes[-1]), coef_a=A,
                           coef_da=DA, coef_c=C if with_c else None, elements=[5, 7])[0]
    assert orc.rel_l2_coef(W[[5, 7], :M], want).max() <= _bar(M)


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("M", [8, 23])
def test_no_list_and_no_pitch_is_the_existing_entry(dev, M, with_c):
    """elem_ids = NULL, gamma_values = NULL and ldw = 0 (and ldw = M): the launch of ``ops.enhance_varcoef``, bit for
    bit, status included."""
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    nodes, values, _ = _mesh()
    pm, n = M <= 22, _n(M)
    x, u = _t(nodes, dev), _t(values, dev)
    gd = (nodes[0], nodes[-1])
    (ta, tda, tf, tc), _ = _full_tables(dev, M, pm, with_c)
    Wf, stf = ops.enhance_varcoef(x, u, M, GAMMA, n, ta, tda, tf, point_major=pm, c_values=tc, global_domain=gd, bc=BC)
    W, st, fc = _outputs(dev, M)
    ops.enhance_varcoef_subset(x, u, M, GAMMA, n, W, ta, tda, tf, c_values=tc, point_major=pm, global_domain=gd,
                               bc=BC, status=st, fail_count=fc)                          # (ldw = M)
    assert np.array_equal(_bits(W.cpu().numpy()), _bits(Wf.cpu().numpy())) and torch.equal(st, stf)
    W0, st0, _ = _outputs(dev, M)
    rc = _capi.load().lssvr_enhance_react_subset(
        x.data_ptr(), u.data_ptr(), NE, None, NE, 0, NE, gd[0], gd[1], BC[0], BC[1], M, n, GAMMA, None,
        ta.data_ptr(), tda.data_ptr(), None if tc is None else tc.data_ptr(), tf.data_ptr(), int(pm), W0.data_ptr(), 0,
        st0.data_ptr(), fc.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and int(fc.item()) == 0
    assert np.array_equal(_bits(W0.cpu().numpy()), _bits(Wf.cpu().numpy())) and torch.equal(st0, stf)


def test_ops_check_shapes_dtypes_and_devices(dev):
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    nodes, values, ids = _mesh()
    x, u, idt = _t(nodes, dev), _t(values, dev), _t(ids, dev)
    tab = torch.zeros((NSUB, 12), dtype=torch.float64, device=dev)
    W = torch.zeros((NE, 9), dtype=torch.float64, device=dev)
    kw = dict(elem_ids=idt, global_domain=(-1.0, 1.0))
    with pytest.raises(ValueError, match="W must be"):
        ops.enhance_varcoef_subset(x, u, 9, GAMMA, 12, W[:, :8].contiguous(), tab, tab, tab, **kw)
    with pytest.raises(ValueError, match="a_values must hold"):
        ops.enhance_varcoef_subset(x, u, 9, GAMMA, 12, W, tab[:5], tab, tab, **kw)
    with pytest.raises(ValueError, match="c_values must hold"):
        ops.enhance_varcoef_subset(x, u, 9, GAMMA, 12, W, tab, tab, tab, c_values=tab[:5], **kw)
    with pytest.raises(TypeError, match="elem_ids"):
        ops.enhance_varcoef_subset(x, u, 9, GAMMA, 12, W, tab, tab, tab, elem_ids=idt.to(torch.int32),
                                   global_domain=(-1.0, 1.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.colloc_points_subset(x, idt.cpu(), 12)
    with pytest.raises(ValueError, match="status is indexed by mesh element"):
        ops.enhance_varcoef_subset(x, u, 9, GAMMA, 12, W, tab, tab, tab, status=torch.zeros(NSUB, dtype=torch.int32,
                                                                                            device=dev), **kw)
    with pytest.raises(ValueError, match="elem_ids must be"):
        ops.colloc_points_subset(x, torch.zeros(NE + 1, dtype=torch.int64, device=dev), 12)
    with pytest.raises(_capi.LssvrHipError, match="M-2"):
        ops.enhance_varcoef_subset(x, u, 9, GAMMA, 6, W, tab[:, :6].contiguous(), tab[:, :6].contiguous(),
                                   tab[:, :6].contiguous(), **kw)
    assert float(W.abs().sum().item()) == 0.0


# ---------------------------------------------------------------------------
# 3. the facade: element_degrees with coefficients, reaction and convection
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("right", ["dirichlet", "robin"])
def test_facade_mixed_degrees_rows_against_restatement(dev, note, right):
    """24 elements with degrees from {6, 9, 12, 18}, a = 2 + sin pi x, b = sin(pi x)/2, c = 1 + cos(pi x)/2: every row
    is the restatement's element solve on the facade's own nodal values with the folded table a' - b, at
    max(n_colloc, 2 M) points.  With a Robin end on the right the last element takes its nodal value, not g."""
    import hybrid_fem_lssvr_amd as pkg
    p = pr.PROBLEMS["var"]
    deg = np.random.default_rng(11).permutation(np.repeat([6, 9, 12, 18], 6))
    bnd = (("dirichlet", 0.3), ("dirichlet", 0.3) if right == "dirichlet" else ("robin", 1.0, 0.5))
    s = pkg.FEMLSSVRPrimalSolver(mesh=np.linspace(-1, 1, 25), lssvr_M=6, lssvr_gamma=GAMMA, n_colloc=16, nquad=3,
                                 rhs=p["f"], global_domain=(-1, 1), coef=(p["a"], p["da"]), reaction=p["c"],
                                 convection=p["b"], boundary=bnd, element_lists=True)
    s.element_degrees = deg
    s.solve()
    W = s.enhanced.W.cpu().numpy()
    assert W.shape == (24, 18) and s.enhanced.n_fallback == 0 and np.array_equal(s.enhanced.degrees, deg)
    nodes, vals = np.asarray(s.fem_nodes), np.asarray(s.fem_values)
    gd = (-1.0, 1.0 if right == "dirichlet" else 9.0)
    folded = lambda x: p["da"](x) - p["b"](x)                                    # noqa: E731
    worst = {}
    for M in (6, 9, 12, 18):
        ids = np.nonzero(deg == M)[0]
        want = orc.enhance_all(nodes, vals, M, GAMMA, s.group_colloc(M), rhs=p["f"], global_domain=gd, coef_a=p["a"],
                               coef_da=folded, coef_c=p["c"], bc_left=0.3, bc_right=0.3, elements=ids)[0]
        worst[M] = orc.rel_l2_coef(W[ids, :M], want).max()
        note(f"facade mixed degrees ({right}) M={M}", worst[M], _bar(M))
        assert np.all(W[ids, M:] == 0.0)
    print(right, {M: f"{e:.2e}" for M, e in worst.items()})
    assert all(e <= _bar(M) for M, e in worst.items()), worst
    # the indicator and the evaluation take the padded rows as they are
    assert np.all(np.isfinite(s.estimate())) and np.all(np.isfinite(s.evaluate_solution(np.linspace(-1, 1, 501))))


def _module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", "proto", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_facade_periodic_hp_on_the_element_lists(dev, note):
    """tests/test_gpu_periodic.py's hp run (the peak on the seam, -u'' + u = f from 8 elements of degree 8) with
    ``element_lists=True``: the same rounds as the whole-mesh launch per degree of the default path -- the same final
    mesh and degrees -- and a max error on 2001 points within 2 x the numpy prototype's
    (scripts/proto/periodic_proto.py, run here; 1.502e-5 on 64 elements)."""
    import hybrid_fem_lssvr_amd as pkg
    proto = _module("periodic_proto")
    xq = np.linspace(-1.0, 1.0, 2001)
    runs = {}
    for lists in (False, True):
        s = pkg.FEMLSSVRPrimalSolver(mesh=np.linspace(-1, 1, proto.NE0 + 1), lssvr_M=proto.M, lssvr_gamma=proto.GAMMA,
                                     n_colloc=proto.N, nquad=proto.NQUAD, rhs=pr.peak_f, global_domain=(-1, 1),
                                     reaction=pr._one, boundary="periodic", element_lists=lists)
        s.solve_adaptive(mode="hp", theta=proto.THETA, max_elements=proto.MAXE, sigma_min=proto.SIGMA_MIN,
                         dM=proto.DM, M_max=proto.M_MAX, max_iter=proto.MAX_ITER)
        assert s.enhanced.n_fallback == 0 and s.fem_values[0] == s.fem_values[-1]
        runs[lists] = (np.asarray(s.fem_nodes), np.asarray(s.element_degrees),
                       float(np.max(np.abs(s.evaluate_solution(xq) - pr.peak_u(xq)))))
    err_p = proto.run_hp()[2]
    (n0, d0, e0), (n1, d1, e1) = runs[False], runs[True]
    note("periodic hp on the element lists: max error", e1, 2.0 * err_p)
    print(f"periodic hp: lists {e1:.3e} on {len(d1)} elements, whole mesh per degree {e0:.3e}, prototype {err_p:.3e}")
    assert np.array_equal(n0, n1) and np.array_equal(d0, d1)
    assert e1 <= 2.0 * err_p


def _proto():
    spec = importlib.util.spec_from_file_location("hp_general_proto",
                                                  os.path.join(ROOT, "scripts", "proto", "hp_general_proto.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_adaptive_hp_against_h_on_the_outflow_layer(dev, note):
    """-eps u'' + u' = 1 on (0, 1), eps = 0.02, from 32 elements (cell Peclet 0.78) of degree parameter 2, budget
    sum M_e <= 600: ``mode="hp"`` against ``mode="h"`` with max_elements = 600 // 2.  Both max errors on 2001 points
    are within 2 x the numpy prototype's (scripts/proto/hp_general_proto.py, run here: h 6.578e-5 on 194 elements, hp
    1.865e-5 on 171 elements with sum M = 488), and hp is below h."""
    import hybrid_fem_lssvr_amd as pkg
    proto = _proto()
    xq = proto.XQ
    kw = dict(lssvr_M=proto.M0, lssvr_gamma=proto.GAMMA, n_colloc=proto.N, nquad=proto.NQUAD, rhs=cr.layer_f,
              global_domain=proto.GD, coef=(cr.layer_a, cr.layer_da), convection=cr.layer_b, element_lists=True)
    start = np.linspace(*proto.GD, proto.NE0 + 1)
    h = pkg.FEMLSSVRPrimalSolver(mesh=start, **kw)
    h.solve_adaptive(theta=proto.THETA, max_elements=proto.MAX_DOF // proto.M0, max_iter=proto.MAX_ITER)
    err_h = float(np.max(np.abs(h.evaluate_solution(xq) - cr.layer_exact(xq))))
    s = pkg.FEMLSSVRPrimalSolver(mesh=start, **kw)
    s.solve_adaptive(mode="hp", theta=proto.THETA, sigma_min=proto.SIGMA_MIN, dM=proto.DM, M_max=proto.M_MAX,
                     max_dof=proto.MAX_DOF, max_iter=proto.MAX_ITER)
    err_hp = float(np.max(np.abs(s.evaluate_solution(xq) - cr.layer_exact(xq))))
    deg = np.asarray(s.element_degrees)
    _, perr_h = proto.run_h()
    _, pdeg, perr_hp = proto.run_hp()
    note("adaptive outflow layer h: max error", err_h, 2.0 * perr_h)
    note("adaptive outflow layer hp: max error", err_hp, min(2.0 * perr_hp, err_h))
    print(f"h: {len(h.fem_nodes) - 1} elements, error {err_h:.3e} (prototype {perr_h:.3e}); hp: {len(deg)} elements, "
          f"degrees {deg.min()}..{deg.max()}, sum M {deg.sum()}, error {err_hp:.3e} (prototype {perr_hp:.3e}, "
          f"{len(pdeg)} elements, sum M {int(pdeg.sum())})")
    assert h.enhanced.n_fallback == 0 and s.enhanced.n_fallback == 0
    assert deg.sum() <= proto.MAX_DOF and proto.M0 <= deg.min() and deg.max() <= proto.M_MAX
    assert sum(r["raised"] for r in s.adapt_history) > 0 and sum(r["marked"] for r in s.adapt_history) > 0
    assert err_h <= 2.0 * perr_h
    assert err_hp <= 2.0 * perr_hp
    assert err_hp < err_h
