"""CPU: the host side of hp refinement for coefficient, reaction and convection problems --
the two element-list entries are exported and bound and return their argument errors before any HIP call, the facade
accepts one degree per element for every operator and boundary kind with ``element_lists=True`` and keeps every path
and refusal it had without, a Poisson hp solve still makes the calls it made, and the numpy prototype of the adaptive
run (scripts/proto/hp_general_proto.py) has hp below h."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import hp_rules
import test_capi_cpu as capi_test
from test_periodic_cpu import _FakeAllOps, _names, _one, _per

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(4096)       # never dereferenced: every call below fails validation first, or launches nothing
NAMES = ("lssvr_enhance_react_subset", "lssvr_colloc_points_subset")
OK, ERR_NULL, ERR_SIZE, ERR_DEGREE, ERR_SOLVER = 0, -1, -2, -3, -5


def _lib():
    from hybrid_fem_lssvr_amd import _capi
    return _capi.load()


def test_symbols_in_header_binding_and_library():
    from hybrid_fem_lssvr_amd import _capi
    lib = _lib()
    protos = dict((name, (ret, " ".join(params.split()).split(",")))
                  for ret, name, params in re.findall(r"^(int|int64_t)\s+(lssvr_\w+)\s*\(([^)]*)\)\s*;",
                                                      capi_test._uncommented(capi_test.HEADER), flags=re.M))
    for nm in NAMES:
        assert nm in _capi.SIGNATURES and nm in protos
        fn = getattr(lib, nm)
        assert fn.argtypes == _capi.SIGNATURES[nm][1] and fn.restype is _capi.SIGNATURES[nm][0]
        ret, params = protos[nm]
        assert ret == "int" and [capi_test._ctype_of(d) for d in params] == _capi.SIGNATURES[nm][1], nm
    assert len(_capi.SIGNATURES["lssvr_enhance_react_subset"][1]) == 25
    assert lib.lssvr_version() == 7 == _capi.ABI_VERSION


def _react_subset(lib, *, x=FAKE, u=FAKE, ne_mesh=10, ids=FAKE, nsub=4, off=0, ne_global=10, M=9, n=16, gamma=1e4,
                  gv=None, a=FAKE, da=FAKE, c=FAKE, f=FAKE, layout=0, W=FAKE, ldw=0):
    return lib.lssvr_enhance_react_subset(x, u, ne_mesh, ids, nsub, off, ne_global, 0.0, 1.0, 0.0, 0.0, M, n, gamma,
                                          gv, a, da, c, f, layout, W, ldw, None, None, None)


def test_enhance_react_subset_argument_errors_without_gpu():
    lib = _lib()
    call = lambda **kw: _react_subset(lib, **kw)                          # noqa: E731
    # no dual route: with and without the c table
    for c in (FAKE, None):
        assert call(c=c, M=9, n=6) == ERR_SOLVER and b"M-2" in lib.lssvr_last_error()
        assert call(c=c, M=33, n=30) == ERR_SOLVER
        assert call(c=c, M=9, n=7, nsub=0) == OK                          # n = M - 2 is the primal regime
    # the element list
    assert call(ids=None, nsub=4) == ERR_SIZE and b"nsub must equal ne_mesh" in lib.lssvr_last_error()
    assert call(ids=None, nsub=11) == ERR_SIZE
    assert call(nsub=11) == ERR_SIZE and b"nsub = 11 > ne_mesh = 10" in lib.lssvr_last_error()
    assert call(nsub=-1) == ERR_SIZE and call(ne_mesh=-1, nsub=0) == ERR_SIZE
    # the row pitch
    for ldw in (1, 8, -3):
        assert call(ldw=ldw) == ERR_SIZE and b"ldw" in lib.lssvr_last_error()
    # nothing to do: success, nothing launched -- no device pointer is needed at all
    for c in (FAKE, None):
        assert call(nsub=0, c=c) == OK
        assert call(nsub=0, c=c, x=None, u=None, W=None, a=None, da=None, f=None, ids=None, ne_mesh=0,
                    ne_global=0) == OK
        assert call(nsub=0, c=c, ldw=33, layout=1, gv=FAKE) == OK
    # ... and the one validation path of lssvr_enhance_react_ws / lssvr_enhance_varcoef_ws behind it
    assert call(M=34) == ERR_DEGREE and call(M=1) == ERR_DEGREE
    assert call(n=1) == ERR_SIZE and call(layout=2) == ERR_SIZE and call(gamma=0.0) == ERR_SIZE
    assert call(off=1, ne_global=10) == ERR_SIZE and b"shard" in lib.lssvr_last_error()
    for kw in (dict(x=None), dict(u=None), dict(W=None), dict(a=None), dict(da=None), dict(f=None)):
        assert call(**kw) == ERR_NULL, kw
        assert call(c=None, **kw) == ERR_NULL, kw


def test_colloc_points_subset_argument_errors_without_gpu():
    lib = _lib()

    def call(x=FAKE, ne_mesh=10, ids=FAKE, nsub=4, n=16, layout=0, xc=FAKE):
        return lib.lssvr_colloc_points_subset(x, ne_mesh, ids, nsub, n, layout, xc, None)

    assert call(ids=None, nsub=4) == ERR_SIZE and b"nsub must equal ne_mesh" in lib.lssvr_last_error()
    assert call(nsub=11) == ERR_SIZE and call(nsub=-1) == ERR_SIZE and call(ne_mesh=-2, nsub=0) == ERR_SIZE
    assert call(n=1) == ERR_SIZE and call(layout=2) == ERR_SIZE and call(layout=-1) == ERR_SIZE
    assert call(x=None) == ERR_NULL and call(xc=None) == ERR_NULL
    assert call(nsub=0) == OK and call(nsub=0, x=None, xc=None, ids=None, ne_mesh=0) == OK


def test_ops_validate_before_the_library():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    ids = torch.zeros(2, dtype=torch.int64)
    W = torch.zeros((4, 9), dtype=torch.float64)
    tab = torch.zeros((2, 16), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.colloc_points_subset(t, ids, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.enhance_varcoef_subset(t, t, 9, 1e4, 16, W, tab, tab, tab, elem_ids=ids, global_domain=(0.0, 1.0))
    with pytest.raises(TypeError):
        ops.colloc_points_subset([0.0, 1.0], ids, 16)


# ---------------------------------------------------------------------------
# facade
# ---------------------------------------------------------------------------
def _b(x):
    return 0.25 * (_per(x) - 1.0)          # periodic on (-1, 1), |b| <= 1/8: cell Peclet far below 1 on 8 elements


BOUNDARIES = (None, (None, None), (("dirichlet", 0.25), ("dirichlet", -0.5)), (("neumann", 0.5), None),
              (None, ("robin", 2.0, -0.5)), (("robin", 1.0, 0.0), ("robin", 2.0, 1.0)), "periodic")
OPERATORS = ({"coef": (_per, lambda x: 0.0 * _per(x))}, {"reaction": _one}, {"convection": _b},
             {"coef": (_per, lambda x: 0.0 * _per(x)), "reaction": _one, "convection": _b})


def test_check_hp_accepts_every_operator_and_boundary():
    """Fails on the commit before section 23: there was no ``element_lists``, and ``_check_hp`` refused coef, reaction
    and convection unless the boundary was periodic."""
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    for boundary in BOUNDARIES:
        for kw in OPERATORS:
            s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=6, boundary=boundary, element_lists=True, **kw)
            assert s._check_hp("mode='hp'") is None
            s.element_degrees = np.array([6, 9, 12, 18, 6, 9, 12, 18])
            assert list(s._check_degrees(8)) == [6, 9, 12, 18, 6, 9, 12, 18]
            s.solver_id = ops.SOLVER_DUAL
            with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
                s._check_hp("mode='hp'")
            with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
                s._check_degrees(8)
            with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
                s.solve_adaptive(mode="hp")
    for sid in (ops.SOLVER_DUAL, ops.SOLVER_PRIMAL_WAVE, ops.SOLVER_PRIMAL_MOMENT, ops.SOLVER_SHARED):
        with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
            pkg.FEMLSSVRPrimalSolver(9, lssvr_M=6, solver=sid, element_lists=True).solve_adaptive(mode="hp")


def test_without_element_lists_every_refusal_is_the_old_one():
    """``element_lists`` defaults to False, and then one degree per element is what it was: refused with a coefficient,
    a reaction or convection unless the boundary is periodic, before any GPU use."""
    import hybrid_fem_lssvr_amd as pkg
    assert pkg.FEMLSSVRPrimalSolver(9).element_lists is False
    for boundary in BOUNDARIES:
        for kw in OPERATORS:
            s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=6, boundary=boundary, **kw)
            s.element_degrees = np.full(8, 6)
            if boundary == "periodic":
                assert s._check_hp("mode='hp'") is None and list(s._check_degrees(8)) == [6] * 8
                continue
            with pytest.raises(ValueError, match="Poisson rows.*element_lists=True"):
                s._check_degrees(8)
            with pytest.raises(ValueError, match="Poisson rows"):
                s.solve_adaptive(mode="hp")


def test_goal_and_solve_many_scope_is_unchanged():
    """Out of scope, as before: ``goal=`` refuses ``element_degrees``, and ``solve_many`` takes ``lssvr_M``."""
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=6, reaction=_one, element_lists=True)
    s.element_degrees = np.full(8, 6)
    with pytest.raises(ValueError, match="element_degrees"):
        s.solve_goal(_one)
    with pytest.raises(ValueError, match="mode='h'"):
        s.solve_adaptive(goal=_one, mode="hp")


@pytest.fixture
def fake_ops(monkeypatch):
    import torch
    from hybrid_fem_lssvr_amd import ops, solver

    class Fake(_FakeAllOps):
        """With stand-ins for ``enhance_subset`` and the element-list operators (the grouping of tests/hp_rules.py)."""

        def __getattr__(self, name):
            stubs = {
                "enhance_subset": lambda x, u, M, g, n, W, **kw: W,
                "group_by_degree": lambda deg, **kw: tuple(torch.as_tensor(np.asarray(t, dtype=np.int64))
                                                           for t in hp_rules.group_by_degree(deg.numpy())),
                "colloc_points_subset": lambda x, ids, n, **kw: torch.zeros((ids.numel(), n), dtype=torch.float64)
                + x[ids][:, None],
                "enhance_varcoef_subset": lambda x, u, M, g, n, W, *a, **kw: W,
            }
            if name not in stubs:
                return super().__getattr__(name)

            def op(*args, **kw):
                self.calls.append((name, args, kw))
                return stubs[name](*args, **kw)
            return op

    fake = Fake(ops)
    monkeypatch.setattr(solver, "ops", fake)
    monkeypatch.setattr(solver, "_device", lambda device: torch.device("cpu"))
    return fake


def test_poisson_hp_solve_makes_the_calls_it_made(fake_ops):
    """No coef, reaction or convection: ``element_degrees`` still runs one grouping, then per degree the whole-mesh
    ``colloc_points`` (a callable f) and one ``ops.enhance_subset`` -- none of the new operators -- with Dirichlet and
    with Robin ends, with ``element_lists`` or without; a named right-hand side tabulates nothing."""
    import hybrid_fem_lssvr_amd as pkg
    deg = np.array([8, 8, 10, 12, 12, 10, 8, 8])
    robin = (("dirichlet", 0.25), ("robin", 2.0, -0.5))
    cases = [(b, sh, rhs, nt, el) for b, sh in ((None, {}), (robin, dict(elem_offset=0, ne_global=9)))
             for rhs, nt in ((lambda x: np.cos(x), 3), (pkg.solver.poisson_rhs, 0)) for el in (False, True)]
    for boundary, shard, rhs, n_tab, el in cases:
        fake_ops.calls.clear()
        s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=8, n_colloc=16, boundary=boundary, rhs=rhs, element_lists=el)
        s.element_degrees = deg
        s.solve()
        names = _names(fake_ops)
        assert not {"enhance_varcoef_subset", "colloc_points_subset", "enhance_varcoef", "enhance"} & set(names)
        assert names.count("group_by_degree") == 1 and names.count("colloc_points") == n_tab
        calls = [c for c in fake_ops.calls if c[0] == "enhance_subset"]
        assert [(c[1][2], c[1][4]) for c in calls] == [(8, 16), (10, 20), (12, 24)]
        assert [c[2]["elem_ids"].tolist() for c in calls] == [[0, 1, 6, 7], [2, 5], [3, 4]]
        for c in calls:
            assert {k: v for k, v in c[2].items() if k in ("elem_offset", "ne_global")} == shard
        # the order of the whole round: P1 solve, grouping, then (tabulate,) enhance per degree
        enh = [n for n in names if n in ("group_by_degree", "colloc_points", "enhance_subset")]
        per = ["colloc_points", "enhance_subset"] if n_tab else ["enhance_subset"]
        assert enh == ["group_by_degree"] + per * 3


def test_periodic_without_element_lists_keeps_its_whole_mesh_launches(fake_ops):
    """``boundary="periodic"`` without the keyword is call for call what it was: one ``ops.enhance_varcoef`` over the
    whole mesh per distinct degree, no grouping and none of the new operators."""
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=8, n_colloc=16, boundary="periodic", reaction=_one)
    s.element_degrees = np.array([8, 8, 10, 12, 12, 10, 8, 8])
    s.solve()
    names = _names(fake_ops)
    assert not {"group_by_degree", "enhance_varcoef_subset", "colloc_points_subset", "enhance_subset"} & set(names)
    calls = [c for c in fake_ops.calls if c[0] == "enhance_varcoef"]
    assert [(c[1][2], c[1][4]) for c in calls] == [(8, 16), (10, 20), (12, 24)] and names.count("colloc_points") == 3


def test_general_hp_solve_touches_every_element_once(fake_ops):
    """With a coefficient, a reaction or convection, for every boundary kind: one grouping, and per degree one
    ``colloc_points_subset`` and one ``enhance_varcoef_subset`` on that degree's own elements with the tables of those
    elements only; the lists partition the mesh."""
    import hybrid_fem_lssvr_amd as pkg
    deg = np.array([6, 9, 12, 23, 23, 9, 6, 6])
    for boundary in BOUNDARIES:
        for kw in OPERATORS:
            if boundary == "periodic" and "reaction" not in kw:
                continue                                     # (singular: refused by _check_periodic)
            fake_ops.calls.clear()
            s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=6, n_colloc=16, boundary=boundary, element_lists=True, **kw)
            s.element_degrees = deg
            s.solve()
            names = _names(fake_ops)
            assert not {"enhance_subset", "colloc_points", "enhance_varcoef", "enhance"} & set(names)
            assert names.count("group_by_degree") == 1
            pts = [c for c in fake_ops.calls if c[0] == "colloc_points_subset"]
            enh = [c for c in fake_ops.calls if c[0] == "enhance_varcoef_subset"]
            assert [(c[1][2], c[1][4]) for c in enh] == [(6, 16), (9, 18), (12, 24), (23, 46)]
            assert [c[1][2] for c in pts] == [16, 18, 24, 46]
            lists = [c[2]["elem_ids"].tolist() for c in enh]
            assert lists == [[0, 6, 7], [1, 5], [2], [3, 4]] and [c[1][1].tolist() for c in pts] == lists
            for c, ids in zip(enh, lists):
                M, n = c[1][2], c[1][4]
                pm = M <= 22
                assert c[2]["point_major"] is pm
                tabs = list(c[1][6:9]) + [c[2]["c_values"]]
                assert (tabs[3] is None) == ("reaction" not in kw)
                for t in tabs:
                    assert t is None or tuple(t.shape) == ((n, len(ids)) if pm else (len(ids), n))
                assert {k: v for k, v in c[2].items() if k in ("elem_offset", "ne_global")} == s._shard(8)
            assert tuple(s.enhanced.W.shape) == (8, 23) and list(s.enhanced.degrees) == list(deg)


# ---------------------------------------------------------------------------
# the prototype of the adaptive run
# ---------------------------------------------------------------------------
def _proto():
    spec = importlib.util.spec_from_file_location("hp_general_proto",
                                                  os.path.join(ROOT, "scripts", "proto", "hp_general_proto.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_prototype_hp_beats_h_at_equal_budget():
    """The outflow layer of DESIGN.md section 18 from 32 elements (cell Peclet <= 1): under the same coefficient
    budget the hp run's max error on 2001 points is below the h run's, and both stay inside the budget."""
    import convection_rules as cr
    proto = _proto()
    start = np.linspace(*proto.GD, proto.NE0 + 1)
    assert cr.cell_peclet(start, cr.layer_a, cr.layer_b, proto.NQUAD).max() <= 1.0 and cr.LAYER_EPS == 0.02
    nodes_h, err_h = proto.run_h()
    nodes, deg, err_hp = proto.run_hp()
    print(f"h: {len(nodes_h) - 1} elements, {err_h:.3e}; hp: {len(deg)} elements, sum M {int(deg.sum())}, {err_hp:.3e}")
    assert proto.M0 * (len(nodes_h) - 1) <= proto.MAX_DOF and deg.sum() <= proto.MAX_DOF
    assert deg.min() >= proto.M0 and proto.M0 < deg.max() <= proto.M_MAX and len(deg) > proto.NE0
    assert err_hp < err_h
