"""CPU: the host side of the periodic boundary condition -- the new C entries are exported and bound and reject bad
arguments before any HIP call, the numpy restatement (tests/periodic_rules.py) converges on manufactured problems, and
the facade validates ``boundary="periodic"`` before it touches a GPU and leaves every other ``boundary`` on the
operators it had."""
import ctypes
import os
import re

import numpy as np
import pytest

import periodic_rules as pr
import test_capi_cpu as capi_test
from test_robin_cpu import _FakeOps, _one, _solves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(4096)       # never dereferenced: every call below fails validation first
NAMES = ("lssvr_tridiag_periodic_work_bytes", "lssvr_tridiag_periodic_solve_multi",
         "lssvr_tridiag_ns_periodic_solve_multi", "lssvr_estimate_seam")


def _lib():
    from hybrid_fem_lssvr_amd import _capi
    return _capi.load()


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def test_symbols_in_header_binding_and_library():
    from hybrid_fem_lssvr_amd import _capi
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "lssvr_hip.h")).read()
    for nm in NAMES:
        assert re.search(r"\b%s\s*\(" % nm, header), nm
        assert nm in _capi.SIGNATURES
        fn = getattr(lib, nm)
        assert fn.argtypes == _capi.SIGNATURES[nm][1] and fn.restype is _capi.SIGNATURES[nm][0]
    assert lib.lssvr_version() == 7 == _capi.ABI_VERSION
    # the prototypes against the binding, by the parsing of test_capi_cpu.py
    protos = dict((name, (ret, " ".join(params.split()).split(",")))
                  for ret, name, params in re.findall(r"^(int|int64_t)\s+(lssvr_\w+)\s*\(([^)]*)\)\s*;",
                                                      capi_test._uncommented(capi_test.HEADER), flags=re.M))
    for nm in NAMES:
        ret, params = protos[nm]
        res, argtypes = _capi.SIGNATURES[nm]
        assert res is {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[ret]
        assert [capi_test._ctype_of(d) for d in params] == argtypes, nm


def test_work_bytes_is_monotone_and_holds_z():
    lib = _lib()
    sizes, cases = (2, 3, 9, 513, 514, 2049, 4097, 100000, 1000000), (1, 2, 3, 7, 8, 9, 64)
    for ne in sizes:
        for nc in cases:
            w = lib.lssvr_tridiag_periodic_work_bytes(ne, nc)
            assert w >= lib.lssvr_tridiag_multi_work_bytes(ne, nc) + 16 * (ne + 1)
    for nc in cases:
        ws = [lib.lssvr_tridiag_periodic_work_bytes(ne, nc) for ne in sizes]
        assert all(a < b for a, b in zip(ws, ws[1:]))
    for ne in sizes:
        ws = [lib.lssvr_tridiag_periodic_work_bytes(ne, nc) for nc in cases]
        assert all(a <= b for a, b in zip(ws, ws[1:])) and ws[0] < ws[-1]


def test_argument_errors_without_gpu():
    lib = _lib()
    big = 1 << 30

    def sym(ne=10, nc=1, diag=FAKE, load=FAKE, u=FAKE, work=FAKE, wb=big):
        return lib.lssvr_tridiag_periodic_solve_multi(diag, FAKE, load, ne, nc, u, work, wb, None)

    def ns(ne=10, nc=1, diag=FAKE, sup=FAKE, load=FAKE, u=FAKE, work=FAKE, wb=big):
        return lib.lssvr_tridiag_ns_periodic_solve_multi(diag, FAKE, sup, load, ne, nc, u, work, wb, None)

    for fn in (sym, ns):
        for ne in (0, 1, -3):
            assert fn(ne=ne) == -2 and b"ne" in lib.lssvr_last_error()
        assert fn(nc=0) == -2 and b"nc" in lib.lssvr_last_error()
        assert fn(wb=8) == -2 and b"lssvr_tridiag_periodic_work_bytes" in lib.lssvr_last_error()
        assert fn(wb=lib.lssvr_tridiag_periodic_work_bytes(10, 1) - 1) == -2
        for arg in ("diag", "load", "u", "work"):
            assert fn(**{arg: None}) == -1, arg
    assert ns(sup=None) == -1
    # the off-diagonal band too, the words of each message, and the order of the checks: ne, nc, NULL, work_bytes
    assert lib.lssvr_tridiag_periodic_solve_multi(FAKE, None, FAKE, 10, 1, FAKE, FAKE, big, None) == -1
    assert b"diag, off, load, u, work must be non-NULL" in lib.lssvr_last_error()
    assert lib.lssvr_tridiag_ns_periodic_solve_multi(FAKE, None, FAKE, FAKE, 10, 1, FAKE, FAKE, big, None) == -1
    assert b"diag, sub, sup, load, u, work must be non-NULL" in lib.lssvr_last_error()
    for fn in (sym, ns):
        assert fn(ne=1, nc=0) == -2
        assert b"ne = 1 < 2: a periodic mesh has at least two elements" in lib.lssvr_last_error()
        assert fn(nc=0, diag=None) == -2 and b"nc = 0 < 1" in lib.lssvr_last_error()
        assert fn(diag=None, wb=8) == -1
        need = lib.lssvr_tridiag_periodic_work_bytes(10, 1)
        assert fn(wb=need - 1) == -2 and b"work holds %d bytes, lssvr_tridiag_periodic_work_bytes(10, 1) = %d" % (
            need - 1, need) in lib.lssvr_last_error()
    a = (ctypes.c_double * 2)(1.0, 1.0)

    def seam(M=9, ne=10, x=FAKE, W=FAKE, ah=a, eta2=FAKE, out3=FAKE):
        return lib.lssvr_estimate_seam(x, W, M, ne, ah, eta2, out3, None)

    assert seam(ne=0) == -2 and seam(ne=1) == -2 and b"ne" in lib.lssvr_last_error()
    assert seam(M=0) == -3 and seam(M=34) == -3
    for arg in ("x", "W", "ah", "eta2", "out3"):
        assert seam(**{arg: None}) == -1, arg


def test_ops_validate_before_the_library():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tridiag_periodic_solve(t, t[:4], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tridiag_ns_periodic_solve_multi(t, t[:4], t[:4], t.reshape(1, 5))
    with pytest.raises(TypeError):
        ops.tridiag_periodic_solve([0.0] * 5, t[:4], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.estimate_seam(t, t[:4].reshape(4, 1), (1.0, 1.0), t[:4], t[:3])


# ---------------------------------------------------------------------------
# the restatement on manufactured problems
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pr.PROBLEMS))
def test_rules_converge_on_manufactured_problems(name):
    """Nodal max error of the periodic P1 solve on (-1, 1): a factor 3.5 .. 4.5 per halving of h over 16 .. 256
    elements (the asymptotic factor is 4)."""
    errs = [pr.problem_nodal_error(name, ne) for ne in (16, 32, 64, 128, 256)]
    assert errs[0] < 1e-2
    for coarse, fine in zip(errs, errs[1:]):
        assert 3.5 <= coarse / fine <= 4.5, errs


def test_rules_manufactured_right_hand_sides():
    """f of both problems against a central difference of the flux at random points."""
    x = np.random.default_rng(3).uniform(-1.0, 1.0, 50)
    h = 1e-5
    for p in pr.PROBLEMS.values():
        a = p["a"] or _one
        flux = lambda t: a(t) * pr.man_du(t)                      # noqa: E731
        f = -(flux(x + h) - flux(x - h)) / (2 * h) + (0.0 if p["b"] is None else p["b"](x) * pr.man_du(x)) \
            + p["c"](x) * p["u"](x)
        assert np.max(np.abs(f - p["f"](x))) <= 1e-6 * np.max(np.abs(f))
    d2 = (pr.peak_u(x + h) - 2 * pr.peak_u(x) + pr.peak_u(x - h)) / (h * h)
    assert np.max(np.abs(-d2 + pr.peak_u(x) - pr.peak_f(x))) <= 1e-4 * np.max(np.abs(pr.peak_f(x)))


def test_rules_three_solves_agree():
    """Dense LAPACK, banded LAPACK + Sherman-Morrison and the long-double seam elimination, to 1e-10; the rolled
    system has the rolled solution."""
    for conv in (False, True):
        for ne in (2, 3, 9, 40, 513):
            bands, u_ld, u_la = pr.solve_case(ne, conv)
            u_de = pr.dense_solve(*bands)
            assert u_ld[0] == u_ld[-1] and u_la[0] == u_la[-1] and len(u_ld) == ne + 1
            assert np.max(np.abs(u_de - u_ld)) <= 1e-10 and np.max(np.abs(u_la - u_ld)) <= 1e-10
            assert np.max(np.abs(pr.residual(*bands, u_de))) <= 1e-10
            for k in {1, ne // 2}:
                rolled = pr.roll_bands(*bands, k)
                assert np.max(np.abs(pr.thomas_cyclic_ld(*rolled) - pr.roll_solution(u_ld, k))) <= 1e-10
    # a random non-symmetric dominant system, where no symmetry of the load hides a wrong corner entry
    rng = np.random.default_rng(7)
    for ne in (2, 3, 17):
        sub, sup = -rng.uniform(0.5, 1.0, ne), -rng.uniform(0.5, 1.0, ne)
        diag = rng.uniform(2.5, 3.0, ne + 1)
        load = rng.standard_normal(ne + 1)
        u_de, u_ld, u_la = (fn(diag, sub, sup, load) for fn in (pr.dense_solve, pr.thomas_cyclic_ld, pr.banded_solve))
        assert np.max(np.abs(u_de - u_ld)) <= 1e-10 and np.max(np.abs(u_la - u_ld)) <= 1e-10
        # the seam row itself
        s = u_de[0]
        assert abs((diag[0] + diag[-1]) * s + sup[0] * u_de[1] + sub[-1] * u_de[-2] - load[0] - load[-1]) <= 1e-12


def test_rules_seam_term():
    """Zero to rounding when the first and the last row hold the same smooth periodic function; a hand-computed value
    for two elements; out3 follows."""
    from numpy.polynomial import legendre as L
    x = np.linspace(-1.0, 1.0, 5)
    W = np.array([L.Legendre.fit(np.linspace(a, b, 60), pr.man_u(np.linspace(a, b, 60)), 14, domain=[a, b]).coef
                  for a, b in zip(x[:-1], x[1:])])
    J = pr.seam_jump(x, W, (1.0, 1.0))
    assert abs(J) <= 1e-9 * np.pi              # |u'| ~ pi
    assert abs(pr.seam_jump(x, W, (2.0, 1.0)) - pr.man_du(1.0)) <= 1e-9 * np.pi
    # two elements [0, 1], [1, 3]: u_0 = 1 + 2 P_1 + 3 P_2 on [0, 1], u_1 = 4 P_1 - P_2 on [1, 3]
    # u_0'(0) = (2 - 3 * 3) * 2 = -14, u_1'(3) = (4 - 3) * 1 = 1; a_seam = (2, 0.5): J = 2 * 1 - 0.5 * (-14) = 9
    x2 = np.array([0.0, 1.0, 3.0])
    W2 = np.array([[1.0, 2.0, 3.0], [0.0, 4.0, -1.0]])
    assert pr.seam_jump(x2, W2, (2.0, 0.5)) == 9.0
    eta2, out3 = np.array([1.0, 4.0]), np.array([5.0, 4.0, 0.0])
    new, o3 = pr.estimate_seam(x2, W2, (2.0, 0.5), eta2, out3)
    assert eta2[0] == 1.0                                   # the inputs are not written
    assert new[0] == 1.0 + 0.5 * 81.0 and new[1] == 4.0 + 1.0 * 81.0
    assert o3[0] == 5.0 + 1.5 * 81.0 and o3[1] == 85.0 and o3[2] == 0.0
    W2[0, 1] = np.nan
    new, o3 = pr.estimate_seam(x2, W2, (2.0, 0.5), eta2, out3)
    assert np.all(np.isnan(new)) and o3[2] == 2.0 and o3[0] == 5.0 and o3[1] == 4.0


def test_prototype_refines_the_seam():
    """scripts/proto/periodic_proto.py: both end elements are marked first, and the adapted mesh beats the uniform
    one with the same element count."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("periodic_proto",
                                                  os.path.join(ROOT, "scripts", "proto", "periodic_proto.py"))
    proto = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(proto)
    nodes, err_a, err_u, first = proto.run()
    assert 0 in first and proto.NE0 - 1 in first
    assert len(nodes) - 1 <= proto.MAXE and err_a < err_u


# ---------------------------------------------------------------------------
# facade
# ---------------------------------------------------------------------------
def _per(x):
    return 1.0 + 0.5 * np.cos(np.pi * np.asarray(x, dtype=np.float64))


def _ramp(x):
    return 2.0 + np.asarray(x, dtype=np.float64)


def _zero(x):
    return 0.0 * np.asarray(x, dtype=np.float64)


def test_facade_refuses_before_any_gpu_use():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    S = pkg.FEMLSSVRPrimalSolver
    with pytest.raises(ValueError, match="flux"):
        S(9, boundary="periodic", fem_solver="flux", reaction=_one)
    with pytest.raises(ValueError, match="SOLVER_SHARED"):
        S(9, boundary="periodic", solver=ops.SOLVER_SHARED)
    for bad in ("Periodic", "neumann", ("periodic",), ("periodic", "periodic")):
        with pytest.raises(ValueError, match="boundary"):
            S(9, boundary=bad)
    # attributes are public: switched after construction
    s = S(9, boundary="periodic", reaction=_one)
    s.fem_solver = "flux"
    with pytest.raises(ValueError, match="bands"):
        s.solve()
    s = S(9, boundary="periodic", reaction=_one)
    s.solver_id = ops.SOLVER_SHARED
    with pytest.raises(ValueError, match="per-element"):
        s.solve()
    # singular: no reaction that is positive at a quadrature point, with or without convection
    for kw in ({}, {"reaction": _zero}, {"convection": lambda x: 0.1 + _zero(x)}, {"coef": (_one, _zero)},
               {"reaction": _zero, "convection": lambda x: 0.1 + _zero(x)}):
        s = S(9, boundary="periodic", **kw)
        with pytest.raises(ValueError, match="singular"):
            s.solve()
        with pytest.raises(ValueError, match="singular"):
            s.solve_many([_one])
        with pytest.raises(ValueError, match="singular"):
            s.solve_adaptive(max_iter=1)
    # coefficients that are not periodic on the interval
    for kw, what in (({"coef": (_ramp, _one)}, "coef a"), ({"coef": (_per, _ramp)}, "coef da"),
                     ({"convection": lambda x: 0.1 * _ramp(x)}, "convection"), ({"reaction": _ramp}, "reaction")):
        kw.setdefault("reaction", _one)
        with pytest.raises(ValueError, match=what + " is not periodic"):
            S(9, boundary="periodic", **kw).solve()
    # a difference within 1e-12 max(1, |v|) is rounding, not a refusal
    near = lambda x: 1.0 + 4e-13 * np.asarray(x, dtype=np.float64)       # noqa: E731
    s = S(9, boundary="periodic", reaction=near)
    assert s._check_periodic(s._default_mesh()) is None
    # one element is no periodic mesh
    with pytest.raises(ValueError, match="two elements"):
        S(2, boundary="periodic", reaction=_one).solve()
    # out of scope: goal, end values
    s = S(9, boundary="periodic", reaction=_one)
    with pytest.raises(ValueError, match="periodic"):
        s.solve_goal(_one)
    with pytest.raises(ValueError, match="periodic"):
        s.solve_adaptive(goal=_one)
    # mode="hp" is in scope: what stops it without a reaction is the singular problem, nothing about the mode
    with pytest.raises(ValueError, match="singular"):
        S(9, boundary="periodic").solve_adaptive(mode="hp", max_iter=1)
    with pytest.raises(ValueError, match="bc must be None"):
        s.solve_many([_one, _one], bc=[(0.0, 0.0), (0.0, 0.0)])


class _FakeAllOps(_FakeOps):
    """``_FakeOps`` with stand-ins for the enhancement and indicator operators too, so that ``solve()`` and
    ``estimate()`` run on host tensors and every call is recorded."""

    def __getattr__(self, name):
        import torch
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype)         # noqa: E731
        stubs = {
            "colloc_points": lambda x, n, **kw: z(x.numel() - 1, n) + x[:-1, None],
            "estimate_points": lambda x, nq, **kw: z(x.numel() - 1, nq) + x[:-1, None],
            "enhance": lambda x, u, M, *a, **kw: (z(x.numel() - 1, M), z(x.numel() - 1, dtype=torch.int32)),
            "enhance_varcoef": lambda x, u, M, *a, **kw: (z(x.numel() - 1, M), z(x.numel() - 1, dtype=torch.int32)),
            "estimate": lambda x, W, nq, **kw: (z(x.numel() - 1), None, z(3)),
            "estimate_varcoef": lambda x, W, nq, *a, **kw: (z(x.numel() - 1), None, z(3)),
            "estimate_ends": lambda x, W, *a, **kw: a[-2:],
            "estimate_seam": lambda x, W, a_seam, eta2, out3, **kw: (eta2, out3),
        }
        if name not in stubs:
            return super().__getattr__(name)

        def op(*args, **kw):
            self.calls.append((name, args, kw))
            return stubs[name](*args, **kw)
        return op


def _names(fake):
    return [c[0] for c in fake.calls]


@pytest.fixture
def fake_ops(monkeypatch):
    import torch
    from hybrid_fem_lssvr_amd import ops, solver
    fake = _FakeAllOps(ops)
    monkeypatch.setattr(solver, "ops", fake)
    monkeypatch.setattr(solver, "_device", lambda device: torch.device("cpu"))
    return fake


def test_periodic_routes_to_the_periodic_operators(fake_ops):
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(9, boundary="periodic", reaction=_one)
    assert s._periodic and s._bnd is None and s._gd_bc()[1] == (0.0, 0.0)
    assert s._shard(8) == dict(elem_offset=1, ne_global=10)
    s._fem(s.rhs, *s._gd_bc()[1])
    assert _solves(fake_ops) == ["tridiag_periodic_solve"]
    assert len(fake_ops.calls[-1][1]) == 3 and not fake_ops.calls[-1][2]          # diag, off, load: no end value
    fake_ops.calls.clear()
    s._fem_many([_one, _one, _one], np.zeros((3, 2)))
    assert _solves(fake_ops) == ["tridiag_periodic_solve_multi"]
    assert tuple(fake_ops.calls[-1][1][2].shape) == (3, 9)
    fake_ops.calls.clear()
    s = pkg.FEMLSSVRPrimalSolver(9, boundary="periodic", reaction=_one, convection=lambda x: 0.5 * _per(x))
    s._fem(s.rhs, *s._gd_bc()[1])
    s._fem_many([_one, _one], np.zeros((2, 2)))
    assert _solves(fake_ops) == ["tridiag_ns_periodic_solve", "tridiag_ns_periodic_solve_multi"]


def test_other_boundaries_keep_their_operators(fake_ops):
    """Without ``boundary="periodic"`` every path is call for call the one it was: the Dirichlet and the Neumann / Robin
    operators with their end values, and no periodic operator among the calls."""
    import hybrid_fem_lssvr_amd as pkg
    b = lambda x: 0.5 + 0.0 * np.asarray(x)                 # noqa: E731
    robin = (("dirichlet", 0.25), ("robin", 2.0, -0.5))
    want = {None: "tridiag_dirichlet_solve", robin: "tridiag_bc_solve"}
    for boundary in (None, (None, None), (("dirichlet", 0.25), ("dirichlet", -0.5)), robin):
        for kw in ({}, {"reaction": _one}, {"reaction": _one, "convection": b}):
            s = pkg.FEMLSSVRPrimalSolver(9, boundary=boundary, **kw)
            assert not s._periodic
            assert s._shard(8) == ({} if s._bnd is None else s._bnd.shard(8))
            fake_ops.calls.clear()
            s._fem(s.rhs, *s._gd_bc()[1])
            s._fem_many([_one, _one], np.array([[0.25, 1.0], [0.25, 2.0]]))
            names = _solves(fake_ops)
            assert not any("periodic" in n for n in [c[0] for c in fake_ops.calls])
            stem = want[robin if boundary is robin else None]
            if "convection" in kw:
                stem = stem.replace("tridiag_", "tridiag_ns_")
            assert names == [stem, stem + "_multi"]
            single, multi = (c for c in fake_ops.calls if c[0].startswith("tridiag"))
            if boundary is robin:
                assert single[1][-3:] == ([0, 1], [0.0, 2.0], (0.25, -0.5))
                assert multi[1][-1].tolist() == [[0.25, 1.0], [0.25, 2.0]]
            else:
                assert single[1][-2:] == s._gd_bc()[1]
                assert multi[1][-1].tolist() == [[0.25, 1.0], [0.25, 2.0]]


def test_other_boundaries_keep_their_enhancement_and_indicator(fake_ops):
    """``solve()`` and ``estimate()`` without the new spelling: the enhancement gets the shard arguments it got (none
    with Dirichlet ends, those of ``_Boundary.shard`` with a Robin end), and the indicator never reaches
    ``ops.estimate_seam``."""
    import hybrid_fem_lssvr_amd as pkg
    robin = (("dirichlet", 0.25), ("robin", 2.0, -0.5))
    for boundary, shard in ((None, {}), ((None, None), {}), (robin, dict(elem_offset=0, ne_global=9))):
        for kw, enh, est in (({}, "enhance", "estimate"), ({"reaction": _one}, "enhance_varcoef", "estimate_varcoef")):
            fake_ops.calls.clear()
            s = pkg.FEMLSSVRPrimalSolver(9, boundary=boundary, **kw)
            s.solve()
            s.estimate()
            names = _names(fake_ops)
            assert "estimate_seam" not in names and not any("periodic" in n for n in names)
            assert names.count(enh) == 1 and names.count(est) == 1
            assert names.count("estimate_ends") == (1 if boundary is robin else 0)
            call = fake_ops.calls[names.index(enh)]
            assert {k: v for k, v in call[2].items() if k in ("elem_offset", "ne_global")} == shard


def test_periodic_enhancement_and_indicator(fake_ops):
    """``solve()`` and ``estimate()`` with ``boundary="periodic"``: the table kernels with elem_offset = 1 and
    ne_global = ne + 2, then the estimator and ``ops.estimate_seam`` with a at x_ne and at x_0."""
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(9, boundary="periodic", reaction=_one, coef=(_per, lambda x: 0.0 * _per(x)))
    s.solve()
    s.estimate()
    names = _names(fake_ops)
    assert "estimate_ends" not in names and "enhance" not in names
    call = fake_ops.calls[names.index("enhance_varcoef")]
    assert call[2]["elem_offset"] == 1 and call[2]["ne_global"] == 10
    assert names.index("estimate_seam") == names.index("estimate_varcoef") + 1 and names.count("estimate_seam") == 1
    seam = fake_ops.calls[names.index("estimate_seam")]
    assert tuple(seam[1][2]) == (float(_per(1.0)), float(_per(-1.0)))
    est = fake_ops.calls[names.index("estimate_varcoef")]
    assert seam[1][0] is est[1][0] and seam[1][1] is est[1][1]            # the same x and W


def test_periodic_hp_runs_the_degree_groups_through_the_table_kernels(fake_ops):
    """``element_degrees`` with ``boundary="periodic"``: one ``ops.enhance_varcoef`` per distinct degree, at
    max(n_colloc, 2 M) points and with the periodic shard arguments; ``lssvr_enhance_subset`` holds no reaction rows
    and is not reached.  Without the spelling the degrees still refuse a reaction."""
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=8, n_colloc=16, boundary="periodic", reaction=_one)
    s.element_degrees = np.array([8, 8, 10, 12, 12, 10, 8, 8])
    s.solve()
    names = _names(fake_ops)
    assert "enhance_subset" not in names and "group_by_degree" not in names
    calls = [c for c in fake_ops.calls if c[0] == "enhance_varcoef"]
    assert [(c[1][2], c[1][4]) for c in calls] == [(8, 16), (10, 20), (12, 24)]
    assert all(c[2]["elem_offset"] == 1 and c[2]["ne_global"] == 10 and c[2]["c_values"] is not None for c in calls)
    assert tuple(s.enhanced.W.shape) == (8, 12) and list(s.enhanced.degrees) == [8, 8, 10, 12, 12, 10, 8, 8]
    d = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=8, reaction=_one)
    d.element_degrees = np.full(8, 8)
    with pytest.raises(ValueError, match="Poisson rows"):
        d.solve()
