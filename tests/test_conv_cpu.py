"""CPU: the convection term -(a u')' + b u' + c u = f without a device -- the three new C entries are exported, bound
and reject bad arguments on the host; the facade validates ``convection``; the numpy restatement of the non-symmetric
bands (tests/convection_rules.py) reproduces a manufactured solution at P1 order; and the oracle's ``coef_da`` taking
a' - b gives the rows the identity -(a u')' + b u' = -a u'' - (a' - b) u' promises."""
import ctypes

import numpy as np
import pytest

import convection_rules as cr
from oracle import lssvr_oracle as orc

NEW = ("lssvr_p1_assemble_conv", "lssvr_tridiag_ns_work_bytes", "lssvr_tridiag_ns_dirichlet_solve")


def test_conv_symbols_exported_and_bound():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    for nm in NEW:
        assert hasattr(lib, nm), nm
        res, args = _capi.SIGNATURES[nm]
        fn = getattr(lib, nm)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert lib.lssvr_version() == 7 == _capi.ABI_VERSION
    assert len(_capi.SIGNATURES["lssvr_p1_assemble_conv"][1]) == len(_capi.SIGNATURES["lssvr_p1_assemble_react"][1]) + 2
    assert len(_capi.SIGNATURES["lssvr_tridiag_ns_dirichlet_solve"][1]) == \
        len(_capi.SIGNATURES["lssvr_tridiag_dirichlet_solve"][1]) + 1


def test_conv_argument_errors_without_gpu():
    """Validation happens on the host, before any launch: safe to call on a CPU-only box."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    p = _capi.rhs_params(1.0, 1.0)
    F = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]        # never dereferenced

    def asm(x=F[0], ne=10, nquad=2, rhs_id=1, params=p, rhs_quad=None, a=None, c=None, b=F[1], diag=F[2], sub=F[3],
            sup=F[4], load=F[5]):
        rc = lib.lssvr_p1_assemble_conv(x, ne, nquad, rhs_id, params, rhs_quad, a, c, b, diag, sub, sup, load, None,
                                        None, None)
        return rc, lib.lssvr_last_error().decode()

    for kw, rc_want, sub in (({"ne": 0}, -2, "ne"), ({"ne": -1}, -2, "ne"), ({"x": None}, -1, "non-NULL"),
                             ({"diag": None}, -1, "non-NULL"), ({"sub": None}, -1, "sub"),
                             ({"sup": None}, -1, "sup"), ({"load": None}, -1, "non-NULL"),
                             ({"nquad": 0}, -7, "nquad"), ({"nquad": 6}, -7, "nquad"),
                             ({"rhs_id": 7}, -4, "unknown rhs_id"), ({"params": None}, -4, "rhs_params"),
                             ({"rhs_id": 0}, -4, "rhs_quad")):
        rc, msg = asm(**kw)
        assert rc == rc_want and sub in msg, (kw, rc, msg)

    def solve(diag=F[0], sub=F[1], sup=F[2], load=F[3], ne=10, u=F[4], work=F[5]):
        rc = lib.lssvr_tridiag_ns_dirichlet_solve(diag, sub, sup, load, ne, 0.0, 0.0, u, work, None)
        return rc, lib.lssvr_last_error().decode()

    for kw, rc_want, sub in (({"ne": 0}, -2, "ne"), ({"ne": -3}, -2, "ne"), ({"diag": None}, -1, "non-NULL"),
                             ({"sub": None}, -1, "non-NULL"), ({"sup": None}, -1, "non-NULL"),
                             ({"load": None}, -1, "non-NULL"), ({"u": None}, -1, "non-NULL"),
                             ({"work": None}, -1, "non-NULL")):
        rc, msg = solve(**kw)
        assert rc == rc_want and sub in msg, (kw, rc, msg)
    # the workspace is host arithmetic: nothing at or below the 512-unknown base level but the slack, and less than
    # two doubles per unknown above it (6/8 + 5/8 per level, levels shrink eightfold)
    wb = lib.lssvr_tridiag_ns_work_bytes
    assert wb(1) == wb(2) == wb(513) and 0 < wb(513) <= 1024
    assert 8 * 100000 < wb(100000) < 2 * 8 * 100000
    assert wb(10_000_000) < 2 * 8 * 10_000_000
    # one solver, one workspace formula: the symmetric entry asks for the same bytes
    for ne in (1, 2, 513, 514, 4097, 100000, 10_000_000):
        assert lib.lssvr_tridiag_work_bytes(ne) == wb(ne), ne


def test_ops_reject_host_tensors():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tridiag_ns_dirichlet_solve(t, t[:4], t[:4], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.p1_assemble(t, 2, b_quad=t)
    with pytest.raises(TypeError):
        ops.tridiag_ns_dirichlet_solve([0.0] * 5, t[:4], t[:4], t)


def test_facade_validates_convection():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    b = lambda x: 1.0 + 0.0 * x                                       # noqa: E731
    with pytest.raises(ValueError, match="flux"):
        pkg.FEMLSSVRPrimalSolver(9, convection=b, fem_solver="flux")
    for sid in (ops.SOLVER_DUAL, ops.SOLVER_SHARED, ops.SOLVER_PRIMAL_WAVE):
        with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
            pkg.FEMLSSVRPrimalSolver(9, convection=b, solver=sid)
    with pytest.raises(ValueError, match="callable"):
        pkg.FEMLSSVRPrimalSolver(9, convection=1.0)
    s = pkg.FEMLSSVRPrimalSolver(9, convection=b)
    assert s.convection is b and not s._eq.poisson and s._eq.b is b
    with pytest.raises(ValueError, match="convection"):
        s.solve_adaptive(mode="hp")
    s.element_degrees = np.full(8, 6)
    with pytest.raises(ValueError, match="convection"):
        s._check_degrees(8)
    # convection=None is the solver as it was
    s0 = pkg.FEMLSSVRPrimalSolver(9)
    assert s0.convection is None and s0._eq.poisson and s0._eq.b is None


def _nodal_error(ne, nquad=3):
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    u = cr.fem_solve(nodes, cr.man_f, cr.man_a, cr.man_b, cr.man_c, nquad)
    return np.max(np.abs(u - cr.man_u(nodes)))


def test_helper_bands_reproduce_manufactured_solution_at_p1_order():
    """u = sin(pi x), a = 1 + x^2/4, b = 1 + x/2, c = 1: halving h quarters the nodal error to within 20 %."""
    errs = [_nodal_error(ne) for ne in (40, 80, 160, 320)]
    assert errs[0] < 5e-3
    for coarse, fine in zip(errs, errs[1:]):
        assert 0.8 * 4.0 <= coarse / fine <= 1.2 * 4.0, errs
    # the three solves of the helper agree: LAPACK with pivoting, long-double Thomas without
    nodes = np.linspace(-1.0, 1.0, 81)
    bands = cr.conv_bands(nodes, cr.man_f, cr.man_a, cr.man_b, cr.man_c, 3)[:4]
    u_la, u_ld = cr.banded_ns(*bands, 0.25, -0.5), cr.thomas_ns_ld(*bands, 0.25, -0.5)
    assert np.max(np.abs(u_la - u_ld)) <= 1e-13
    dense = np.diag(bands[0]) + np.diag(bands[1], -1) + np.diag(bands[2], 1)
    rhs = bands[3].copy()
    dense[0], dense[-1] = 0.0, 0.0
    dense[0, 0] = dense[-1, -1] = 1.0
    rhs[0], rhs[-1] = 0.25, -0.5
    assert np.max(np.abs(np.linalg.solve(dense, rhs) - u_la)) <= 1e-13


def test_helper_bands_constant_coefficients_and_dominance():
    """Uniform mesh, constant a, b, c: sub, sup = -a/h -+ b/2 + c h/6, diag = 2a/h + 2ch/3; the rows are diagonally
    dominant exactly up to cell Peclet 1; without b the bands are the symmetric ones."""
    ne, a0, c0 = 16, 0.3, 2.0
    nodes = np.linspace(0.0, 2.0, ne + 1)
    h = 2.0 / ne
    a, c, f = (lambda x: a0 + 0.0 * x), (lambda x: c0 + 0.0 * x), (lambda x: 1.0 + 0.0 * x)
    for pe in (-1.0, -0.5, 0.5, 1.0, 1.2):
        b0 = pe * 2.0 * a0 / h
        diag, sub, sup, load, kloc = cr.conv_bands(nodes, f, a, lambda x: b0 + 0.0 * x, c, 3)
        np.testing.assert_allclose(sub, -a0 / h - b0 / 2 + c0 * h / 6, rtol=1e-13)
        np.testing.assert_allclose(sup, -a0 / h + b0 / 2 + c0 * h / 6, rtol=1e-13)
        np.testing.assert_allclose(diag[1:-1], 2 * a0 / h + 2 * c0 * h / 3, rtol=1e-13)
        np.testing.assert_allclose(cr.cell_peclet(nodes, a, lambda x: b0 + 0.0 * x, 3), abs(pe), rtol=1e-13)
        dominant = np.all(np.abs(sub[:-1]) + np.abs(sup[1:]) <= diag[1:-1])
        assert dominant == (abs(pe) <= 1.0), pe
    d0, off, load0, _ = orc.p1_bands(nodes, f, a, 3, c)
    diag, sub, sup, load, _ = cr.conv_bands(nodes, f, a, None, c, 3)
    assert all(np.array_equal(x, y) for x, y in ((diag, d0), (sub, off), (sup, off), (load, load0)))


def test_element_system_rows_with_folded_table():
    """orc.element_system(coef_da = a' - b) has the rows -a D2 - ((a' - b)/scl) D1 + (c/scl^2) L, built by hand on
    three elements, and they are the rows of the operator: applied to the Legendre coefficients of a polynomial they
    give -(a p')' + b p' + c p at the collocation points."""
    M, n = 7, 12
    nodes = np.array([-1.0, -0.4, 0.1, 1.0])
    for e in range(3):
        lo, hi = nodes[e], nodes[e + 1]
        s = orc.element_system(lo, hi, 0.0, 0.0, M, 1e6, n, rhs=cr.man_f, coef_a=cr.man_a, coef_da=cr.man_folded,
                               coef_c=cr.man_c)
        L, D1, D2 = orc.legendre_tables(s.t, M)
        x = s.x
        hand = (-(cr.man_a(x)[:, None] * D2) - ((cr.man_da(x) - cr.man_b(x)) / s.scl)[:, None] * D1
                + (cr.man_c(x) / (s.scl * s.scl))[:, None] * L)
        assert np.array_equal(s.Ahat, hand)
        # against the operator itself on p(x) = sum_k w_k P_k(t(x)) (derivatives by numpy's Legendre class)
        w = 1.0 / (1.0 + np.arange(M)) ** 2
        p = np.polynomial.legendre.Legendre(w, [lo, hi])
        op = -(cr.man_a(x) * p.deriv(2)(x) + cr.man_da(x) * p.deriv(1)(x)) + cr.man_b(x) * p.deriv(1)(x) \
            + cr.man_c(x) * p(x)
        got = (s.scl * s.scl) * (s.Ahat @ w)
        assert np.max(np.abs(got - op)) <= 1e-11 * np.max(np.abs(op))


def test_boundary_layer_problem_is_consistent():
    """The exact solution of the end-to-end problem satisfies -eps u'' + u' = 1 and the boundary values, and 32
    uniform elements have the cell Peclet number 0.78 the issue names."""
    x = np.linspace(0.0, 1.0, 2001)
    u = cr.layer_exact(x)
    assert abs(u[0]) < 1e-15 and abs(u[-1]) < 1e-15
    e1 = np.exp(-1.0 / cr.LAYER_EPS)
    du = 1.0 - np.exp((x - 1.0) / cr.LAYER_EPS) / (cr.LAYER_EPS * (1.0 - e1))
    d2u = -np.exp((x - 1.0) / cr.LAYER_EPS) / (cr.LAYER_EPS ** 2 * (1.0 - e1))
    assert np.max(np.abs(-cr.LAYER_EPS * d2u + du - 1.0)) < 1e-12
    pe = cr.cell_peclet(np.linspace(0.0, 1.0, 33), cr.layer_a, cr.layer_b, 5)
    np.testing.assert_allclose(pe, 0.78125, rtol=1e-13)
