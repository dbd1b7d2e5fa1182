"""CPU: the host side of the Neumann / Robin boundary conditions -- the new C entries are exported and bound and
reject bad arguments before any HIP call, the numpy restatement (tests/robin_rules.py) converges on manufactured
problems, and the facade validates ``boundary`` before it touches a GPU and leaves ``boundary=None`` on the Dirichlet
operators."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import robin_rules as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(4096)       # never dereferenced: every call below fails validation first
NAMES = ("lssvr_tridiag_bc_work_bytes", "lssvr_tridiag_bc_solve_multi", "lssvr_tridiag_ns_bc_solve_multi",
         "lssvr_estimate_ends")


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
    for c_name, val in (("LSSVR_END_DIRICHLET", _capi.END_DIRICHLET), ("LSSVR_END_ROBIN", _capi.END_ROBIN)):
        assert int(re.search(r"#define %s\s+(\d+)" % c_name, header).group(1)) == val
    # the new block follows the convection block and the load cases
    assert header.index("lssvr_tridiag_bc_solve_multi") > header.index("lssvr_tridiag_ns_dirichlet_solve_multi(")


def test_work_bytes_covers_two_free_ends():
    lib = _lib()
    for ne in (1, 511, 512, 4096, 100000):
        for nc in (1, 3, 8, 9):
            assert lib.lssvr_tridiag_bc_work_bytes(ne, nc) >= lib.lssvr_tridiag_multi_work_bytes(ne + 2, nc)
    assert lib.lssvr_tridiag_bc_work_bytes(1000, 9) == lib.lssvr_tridiag_bc_work_bytes(1000, 8)


def test_argument_errors_without_gpu():
    lib = _lib()
    kap = (ctypes.c_double * 2)(0.0, 2.0)
    big = 1 << 30

    def sym(ne=10, nc=1, kl=1, kr=0, kappa=kap, diag=FAKE, work=FAKE, wb=big):
        return lib.lssvr_tridiag_bc_solve_multi(diag, FAKE, FAKE, kl, kr, FAKE, kappa, ne, nc, FAKE, work, wb, None)

    def ns(ne=10, nc=1, kl=1, kr=0, kappa=kap, sup=FAKE, wb=big):
        return lib.lssvr_tridiag_ns_bc_solve_multi(FAKE, FAKE, sup, FAKE, kl, kr, FAKE, kappa, ne, nc, FAKE, FAKE, wb,
                                                   None)

    for fn in (sym, ns):
        assert fn(ne=0) == -2 and b"ne" in lib.lssvr_last_error()
        assert fn(nc=0) == -2 and b"nc" in lib.lssvr_last_error()
        assert fn(kl=2) == -2 and b"end kinds" in lib.lssvr_last_error()
        assert fn(kr=-1) == -2 and b"end kinds" in lib.lssvr_last_error()
        assert fn(kappa=None) == -1 and b"kappa" in lib.lssvr_last_error()
        assert fn(kappa=(ctypes.c_double * 2)(-1.0, 0.0)) == -2 and b"kappa[0]" in lib.lssvr_last_error()
        assert fn(kr=1, kappa=(ctypes.c_double * 2)(0.0, math.inf)) == -2 and b"kappa[1]" in lib.lssvr_last_error()
        assert fn(kr=1, kappa=(ctypes.c_double * 2)(0.0, math.nan)) == -2
        assert fn(wb=8) == -2 and b"lssvr_tridiag_bc_work_bytes" in lib.lssvr_last_error()
    assert sym(diag=None) == -1 and sym(work=None) == -1 and ns(sup=None) == -1
    # each NULL of both entries (end_values may be NULL: zeros), with the list of its bands in the message
    for entry, nargs, bands, words in ((lib.lssvr_tridiag_bc_solve_multi, 13, (0, 1, 2), b"diag, off, load, u, work"),
                                       (lib.lssvr_tridiag_ns_bc_solve_multi, 14, (0, 1, 2, 3),
                                        b"diag, sub, sup, load, u, work")):
        args = [FAKE] * len(bands) + [1, 0, None, kap, 10, 1, FAKE, FAKE, big, None]
        assert len(args) == nargs
        for i in bands + (nargs - 4, nargs - 3):
            assert entry(*(None if j == i else a for j, a in enumerate(args))) == -1, i
            assert words in lib.lssvr_last_error(), i
    # the order of the checks: ne, nc, NULL, end kinds, work_bytes
    assert sym(ne=0, nc=0) == -2 and b"ne = 0 < 1" in lib.lssvr_last_error()
    assert sym(nc=0, diag=None) == -2 and b"nc = 0 < 1" in lib.lssvr_last_error()
    assert sym(diag=None, kl=2) == -1 and sym(kl=2, wb=8) == -2 and b"end kinds" in lib.lssvr_last_error()
    need = lib.lssvr_tridiag_bc_work_bytes(10, 1)
    assert sym(wb=need - 1) == -2 and b"work holds %d bytes, lssvr_tridiag_bc_work_bytes(10, 1) = %d" % (
        need - 1, need) in lib.lssvr_last_error()
    # kappa of a Dirichlet end is not read
    g = (ctypes.c_double * 2)(0.0, 0.0)

    def ends(M=9, ne=10, kl=1, kr=1, kappa=kap, gh=g, ah=g, W=FAKE):
        return lib.lssvr_estimate_ends(FAKE, W, M, ne, kl, kr, kappa, gh, ah, FAKE, FAKE, None)

    assert ends(ne=0) == -2 and ends(M=0) == -3 and ends(M=34) == -3 and ends(W=None) == -1
    assert ends(kl=3) == -2 and b"end kinds" in lib.lssvr_last_error()
    assert ends(kappa=(ctypes.c_double * 2)(0.0, -2.0)) == -2 and b"kappa[1]" in lib.lssvr_last_error()
    assert ends(gh=None) == -1 and ends(ah=None) == -1
    # two Dirichlet ends add nothing: success without a launch
    assert ends(kl=0, kr=0) == 0


def test_ops_validate_before_the_library():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tridiag_bc_solve(t, t[:4], t, (0, 1), (0.0, 0.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tridiag_ns_bc_solve_multi(t, t[:4], t[:4], t.reshape(1, 5), (0, 1), (0.0, 0.0))
    with pytest.raises(TypeError):
        ops.tridiag_bc_solve([0.0] * 5, t[:4], t, (0, 1), (0.0, 0.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.estimate_ends(t, t[:4].reshape(4, 1), (0, 1), (0.0, 0.0), (0.0, 0.0), (1.0, 1.0), t[:4], t[:3])
    for kinds, kappa in (((0, 2), (0.0, 0.0)), ((0, 1, 1), (0.0, 0.0)), ((True, 0), (0.0, 0.0)), ((0, 1), (0.0, -1.0)),
                         ((0, 1), (math.nan, 0.0)), ((0, 1), (0.0, math.inf)), ((0, 1), (0.0,))):
        with pytest.raises(ValueError):
            ops._end_kinds(kinds, kappa)
    with pytest.raises(TypeError):
        ops._end_kinds(1, (0.0, 0.0))
    assert ops._end_kinds((0, 1), (0.0, 2.0))[0] == (0, 1)


# ---------------------------------------------------------------------------
# the restatement on manufactured problems
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rr.PROBLEMS))
def test_rules_converge_on_manufactured_problems(name):
    """Nodal max error of the P1 solve with the end conditions: a factor >= 3 per halving of h over three halvings
    (the asymptotic factor is 4)."""
    errs = [rr.problem_nodal_error(name, ne) for ne in (12, 24, 48, 96)]
    assert errs[0] < 1e-2
    for coarse, fine in zip(errs, errs[1:]):
        assert coarse / fine >= 3.0, errs


def test_rules_three_solves_agree_and_dirichlet_is_the_old_system():
    import convection_rules as cr
    for conv in (False, True):
        for kinds in rr.KIND_PAIRS:
            for ne in (1, 2, 3, 40):
                bands, u_ld, u_la = rr.solve_case(ne, kinds, conv)
                u_de = rr.dense_solve(*bands, kinds, rr.SOLVE_KAPPA, rr.SOLVE_VALUES)
                assert np.max(np.abs(u_de - u_ld)) <= 1e-13 and np.max(np.abs(u_la - u_ld)) <= 1e-13
        bands, u_ld, _ = rr.solve_case(40, (rr.DIRICHLET, rr.DIRICHLET), conv)
        assert np.array_equal(u_ld, cr.thomas_ns_ld(*bands, *rr.SOLVE_VALUES))


def test_rules_boundary_residual_vanishes_for_the_exact_solution():
    """J of the indicator's boundary term for Legendre rows that interpolate the exact solution: at rounding level of
    the terms; and h/2 J^2 joins eta2 and out3 as stated."""
    from numpy.polynomial import legendre as L
    p = rr.PROBLEMS["exp"]
    x = np.linspace(-1.0, 1.0, 5)
    W = np.array([L.Legendre.fit(np.linspace(a, b, 60), p["u"](np.linspace(a, b, 60)), 14, domain=[a, b]).coef
                  for a, b in zip(x[:-1], x[1:])])
    a_ends = (float(p["a"](x[0])), float(p["a"](x[-1])))
    J = rr.end_residuals(x, W, p["kinds"], p["kappa"], p["values"], a_ends)
    assert J[0] == 0.0 and abs(J[1]) <= 1e-10 * rr.EXP_G
    eta2 = np.array([1.0, 4.0, 2.0, 3.0])
    out3 = np.array([10.0, 4.0, 0.0])
    new, o3 = rr.estimate_ends(x, W, (rr.ROBIN, rr.ROBIN), (1.0, 0.0), (0.5, 2.0), a_ends, eta2, out3)
    Jl, Jr = rr.end_residuals(x, W, (rr.ROBIN, rr.ROBIN), (1.0, 0.0), (0.5, 2.0), a_ends)
    assert np.array_equal(new[1:3], eta2[1:3]) and eta2[0] == 1.0          # the inputs are not written
    assert new[0] == 1.0 + 0.25 * Jl * Jl and new[3] == 3.0 + 0.25 * Jr * Jr
    assert o3[0] == 10.0 + 0.25 * Jl * Jl + 0.25 * Jr * Jr and o3[1] == max(4.0, new[0], new[3]) and o3[2] == 0.0
    Wn = W.copy()
    Wn[0, 3] = np.nan
    new, o3 = rr.estimate_ends(x, Wn, (rr.ROBIN, rr.DIRICHLET), (1.0, 0.0), (0.5, 2.0), a_ends, eta2, out3)
    assert np.isnan(new[0]) and o3[2] == 1.0 and o3[0] == 10.0 and o3[1] == 4.0


# ---------------------------------------------------------------------------
# facade
# ---------------------------------------------------------------------------
def _one(x):
    return 1.0 + 0.0 * np.asarray(x, dtype=np.float64)


def test_facade_validates_boundary_before_any_gpu_use():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    S = pkg.FEMLSSVRPrimalSolver
    neu, rob = ("neumann", 0.0), ("robin", 2.0, 1.0)
    with pytest.raises(ValueError, match="flux"):
        S(9, boundary=(None, neu), fem_solver="flux")
    with pytest.raises(ValueError, match="SOLVER_SHARED"):
        S(9, boundary=(rob, None), solver=ops.SOLVER_SHARED)
    # two Dirichlet ends are the old path: both stay available
    S(9, boundary=(("dirichlet", 1.0), None), fem_solver="flux")
    S(9, boundary=(None, None), solver=ops.SOLVER_SHARED)
    for bad in (("robin", -1.0, 0.0), ("robin", math.nan, 0.0), ("robin", math.inf, 0.0), ("robin", 1.0, math.inf),
                ("neumann", math.nan), ("dirichlet", math.inf)):
        with pytest.raises(ValueError, match="kappa"):
            S(9, boundary=(None, bad))
    for bad in ("neumann", (neu,), (neu, neu, neu), (("flux", 1.0), None), (("robin", 1.0), None),
                (("neumann", 1.0, 2.0), None), (None, 3.0)):
        with pytest.raises(ValueError, match="boundary"):
            S(9, boundary=bad)
    # singular: two Neumann ends and no reaction that is positive somewhere -- raised by solve() before any launch
    for kw in ({}, {"reaction": lambda x: 0.0 * np.asarray(x)}, {"convection": lambda x: 0.1 + 0.0 * np.asarray(x)},
               {"coef": (_one, lambda x: 0.0 * np.asarray(x))}):
        s = S(9, boundary=(neu, ("robin", 0.0, 1.0)), **kw)
        with pytest.raises(ValueError, match="singular"):
            s.solve()
        with pytest.raises(ValueError, match="singular"):
            s.solve_many([_one])
        with pytest.raises(ValueError, match="singular"):
            s.solve_adaptive(max_iter=1)
    # convection: an inflow end with kappa + b n / 2 < 0 loses coercivity
    b_pos = lambda x: 1.0 + 0.0 * np.asarray(x)             # noqa: E731  (flows to the right: inflow at the left end)
    with pytest.raises(ValueError, match="left end"):
        S(9, boundary=(neu, None), convection=b_pos, reaction=_one).solve()
    with pytest.raises(ValueError, match="left end"):
        S(9, boundary=(("robin", 0.49, 0.0), None), convection=b_pos, reaction=_one).solve()
    with pytest.raises(ValueError, match="right end"):
        S(9, boundary=(None, neu), convection=lambda x: -1.0 + 0.0 * np.asarray(x), reaction=_one).solve()
    # attributes are public: a solver switched to the flux solve after construction is refused as well
    s = S(9, boundary=(None, neu))
    s.fem_solver = "flux"
    with pytest.raises(ValueError, match="bands"):
        s.solve()


def test_facade_parses_boundary():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops, solver
    s = pkg.FEMLSSVRPrimalSolver(9, boundary=(("dirichlet", 0.5), ("robin", 2.0, -1.0)))
    b = s._bnd
    assert b.kinds == [ops.END_DIRICHLET, ops.END_ROBIN] and b.kappa == [0.0, 2.0] and b.values == [0.5, -1.0]
    assert s._gd_bc()[1] == (0.5, -1.0)
    assert b.shard(8) == dict(elem_offset=0, ne_global=9)
    b = solver._Boundary((("neumann", 1.0), None))
    assert b.kinds == [ops.END_ROBIN, ops.END_DIRICHLET] and b.values == [1.0, None]
    assert b.shard(8) == dict(elem_offset=1, ne_global=9)
    assert solver._Boundary((("neumann", 1.0), ("neumann", 2.0))).shard(8) == dict(elem_offset=1, ne_global=10)
    # no Neumann or Robin end: the Dirichlet path, with the module's functions where an end is None
    for boundary in (None, (None, None), (("dirichlet", 0.25), None)):
        s = pkg.FEMLSSVRPrimalSolver(9, boundary=boundary)
        assert s._bnd is None
    assert pkg.FEMLSSVRPrimalSolver(9)._gd_bc()[1] == (0.0, 0.0)
    assert pkg.FEMLSSVRPrimalSolver(9, boundary=(("dirichlet", 0.25), None))._gd_bc()[1] == (0.25, 0.0)


class _FakeOps:
    """Stands in for ``ops`` inside solver.py: records which solve operator ``_fem`` / ``_fem_many`` reach, on host
    tensors."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("END_") or name.startswith("SOLVER_") or name in ("MIN_DEGREE", "MAX_DEGREE"):
            return getattr(self._real, name)
        import torch

        def op(*args, **kw):
            self.calls.append((name, args, kw))
            if name == "quad_points":
                x, nq = args[0], args[1]
                return x[:-1, None] + (x[1:] - x[:-1])[:, None] * torch.linspace(0.2, 0.8, nq, dtype=x.dtype)[None, :]
            if name == "p1_assemble":
                n = args[0].numel()
                z = torch.zeros(n, dtype=torch.float64)
                return dict(diag=z, off=z[:-1], sub=z[:-1], sup=z[:-1], load=z, kloc=z[:-1], floc=z[:-1])
            if name == "p1_load_multi":
                return torch.zeros((args[1].shape[0], args[0].numel()), dtype=torch.float64)
            if name.startswith("tridiag"):
                load = args[-4] if "bc_solve" in name else (args[2] if "ns" not in name else args[3])
                return torch.zeros_like(load)
            raise AssertionError(name)
        return op


@pytest.fixture
def fake_ops(monkeypatch):
    import torch
    from hybrid_fem_lssvr_amd import ops, solver
    fake = _FakeOps(ops)
    monkeypatch.setattr(solver, "ops", fake)
    monkeypatch.setattr(solver, "_device", lambda device: torch.device("cpu"))
    return fake


def _solves(fake):
    return [c[0] for c in fake.calls if c[0].startswith("tridiag")]


def test_boundary_none_keeps_the_dirichlet_operators(fake_ops):
    import hybrid_fem_lssvr_amd as pkg
    b = lambda x: 0.5 + 0.0 * np.asarray(x)                 # noqa: E731
    for boundary in (None, (None, None), (("dirichlet", 0.25), ("dirichlet", -0.5))):
        want = (0.0, 0.0) if boundary is None or boundary[0] is None else (0.25, -0.5)
        fake_ops.calls.clear()
        s = pkg.FEMLSSVRPrimalSolver(9, boundary=boundary)
        s._fem(s.rhs, *s._gd_bc()[1])
        assert _solves(fake_ops) == ["tridiag_dirichlet_solve"]
        assert fake_ops.calls[-1][1][3:] == want
        fake_ops.calls.clear()
        s = pkg.FEMLSSVRPrimalSolver(9, boundary=boundary, convection=b)
        s._fem(s.rhs, *s._gd_bc()[1])
        assert _solves(fake_ops) == ["tridiag_ns_dirichlet_solve"]
        fake_ops.calls.clear()
        s._fem_many([_one, _one], np.zeros((2, 2)))
        assert _solves(fake_ops) == ["tridiag_ns_dirichlet_solve_multi"]
        fake_ops.calls.clear()
        pkg.FEMLSSVRPrimalSolver(9, boundary=boundary)._fem_many([_one, _one], np.zeros((2, 2)))
        assert _solves(fake_ops) == ["tridiag_dirichlet_solve_multi"]


def test_robin_end_routes_to_the_bc_operators(fake_ops):
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    boundary = (("dirichlet", 0.25), ("robin", 2.0, -0.5))
    s = pkg.FEMLSSVRPrimalSolver(9, boundary=boundary, reaction=_one)
    s._fem(s.rhs, *s._gd_bc()[1])
    assert _solves(fake_ops) == ["tridiag_bc_solve"]
    name, args, _ = fake_ops.calls[-1]
    assert args[3:] == ([ops.END_DIRICHLET, ops.END_ROBIN], [0.0, 2.0], (0.25, -0.5))
    fake_ops.calls.clear()
    s._fem_many([_one, _one, _one], np.array([[0.25, 1.0], [0.25, 2.0], [0.25, 3.0]]))
    assert _solves(fake_ops) == ["tridiag_bc_solve_multi"]
    assert fake_ops.calls[-1][1][5].tolist() == [[0.25, 1.0], [0.25, 2.0], [0.25, 3.0]]
    fake_ops.calls.clear()
    s = pkg.FEMLSSVRPrimalSolver(9, boundary=boundary, convection=lambda x: 0.5 + 0.0 * np.asarray(x))
    s._fem(s.rhs, *s._gd_bc()[1])
    s._fem_many([_one, _one], np.zeros((2, 2)))
    assert _solves(fake_ops) == ["tridiag_ns_bc_solve", "tridiag_ns_bc_solve_multi"]
