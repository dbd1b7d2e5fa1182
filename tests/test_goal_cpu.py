"""CPU: the host side of goal-oriented error estimation -- the numpy restatement (tests/goal_rules.py) satisfies the
error identity J(u) - J(ut) = sum eta to rounding on two exact cases (any wrong sign or a wrong split of the jumps
breaks it), the new C entries are exported and bound and reject bad arguments before any HIP call, and the facade
raises its ``ValueError``s without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import goal_rules as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(4096)       # never dereferenced: every call below fails validation first
NAMES = ("lssvr_goal_work_bytes", "lssvr_estimate_goal")


# ---------------------------------------------------------------------------
# the identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("make", [gr.exact_case_poisson, gr.exact_case_robin])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_error_identity_holds_to_rounding(make, seed):
    """7 non-uniform elements, ut a random continuous piecewise polynomial of degree 6, z expanded exactly:
    |sum eta + sum q - J(u)| <= 1e-12 * (everything that was summed, by magnitude)."""
    case = make(seed)
    eta, q, scale = gr.run_case(case)
    defect, total = gr.identity_defect(case, eta, q, scale)
    assert defect <= 1e-12 * total, (defect, total)
    # the identity is not vacuous: the correction is of the size of J itself
    assert abs(eta.sum()) > 1e-3 * abs(case["J"])


@pytest.mark.parametrize("make", [gr.exact_case_poisson, gr.exact_case_robin])
def test_identity_detects_a_wrong_sign_or_split(make):
    """Flipping the jump terms, the end terms or the split of a jump between its two elements breaks the identity by
    many orders of magnitude more than the bar."""
    case = make(1)
    eta, q, scale = gr.run_case(case)
    _, total = gr.identity_defect(case, eta, q, scale)
    flipped = dict(case, a_ends=-case["a_ends"])                  # J -> -J: the jump terms change sign
    eta_f, q_f, scale_f = gr.run_case(flipped)
    assert gr.identity_defect(case, eta_f, q_f, scale_f)[0] > 1e-3 * total
    if case["kinds"] != (gr.DIRICHLET, gr.DIRICHLET):
        noend = dict(case, kinds=(gr.DIRICHLET, gr.DIRICHLET))    # the end terms dropped
        eta_n, q_n, scale_n = gr.run_case(noend)
        assert gr.identity_defect(case, eta_n, q_n, scale_n)[0] > 1e-3 * total


def test_jump_free_form_drops_jumps_and_keeps_the_sum_where_the_residual_is_p1_orthogonal():
    """z - I_h z vanishes at the nodes: the jump-free eta does not depend on a_ends or on the end terms.  Its sum
    differs from the full sum by the residual applied to I_h z -- here, with a = 1, by
    sum_i z(x_i) (int f phi_i - int ut' phi_i'), which is evaluated directly."""
    case = gr.exact_case_poisson(3)
    keys = ("x", "Wu", "Wz", "xi", "wt", "f", "j", "a", "da", "c", "a_ends", "kinds", "kappa", "g", "a_bnd")
    full = gr.estimate_goal(*(case[k] for k in keys))[0]
    free = gr.estimate_goal(*(case[k] for k in keys), jump_free=True)[0]
    other = gr.estimate_goal(*(dict(case, a_ends=3.0 * case["a_ends"])[k] for k in keys), jump_free=True)[0]
    assert np.array_equal(free, other)
    # the residual on I_h z, element by element: int_e f I_h z - ut' (I_h z)' h,
    # with ut' (I_h z)' h = (ur - ul)(zr - zl) / h
    x, Wu, Wz, xi, wt = (case[k] for k in ("x", "Wu", "Wz", "xi", "wt"))
    h = np.diff(x)
    sgn = (-1.0) ** np.arange(Wu.shape[1])
    zl, zr, ul, ur = Wz @ sgn, Wz.sum(axis=1), Wu @ sgn, Wu.sum(axis=1)
    Iz = 0.5 * (zl + zr)[:, None] + 0.5 * (zr - zl)[:, None] * xi[None, :]
    on_p1 = 0.5 * h * ((case["f"] * Iz) @ wt) - (ur - ul) * (zr - zl) / h
    assert abs((full.sum() - free.sum()) - on_p1.sum()) <= 1e-12 * (np.abs(full).sum() + np.abs(on_p1).sum())


def test_exact_solution_has_zero_correction():
    """ut = u itself (a global polynomial): residual, jumps and end terms vanish, eta is rounding, sum q = J(u)."""
    from numpy.polynomial import Polynomial
    case = gr.exact_case_robin(4)
    ap, cc = Polynomial([1.0, 0.0, 0.5]), 2.0
    rng = np.random.default_rng(4)
    up = Polynomial(rng.uniform(-1.0, 1.0, 5))
    x = case["x"]
    from oracle import lssvr_oracle as orc
    xq = orc.estimate_points(x, case["xi"])
    g = (-ap(-1.0) * up.deriv()(-1.0), ap(1.0) * up.deriv()(1.0) + gr.ROBIN_KAPPA * up(1.0))
    fp = -(ap * up.deriv()).deriv() + cc * up
    exact = dict(case, Wu=gr.legendre_rows(x, up, 7), f=fp(xq), g=g)
    eta, q, scale = gr.run_case(exact)
    assert np.all(np.abs(eta) <= 1e-12 * np.maximum(scale, 1.0))
    # J(u) for this u by the same Gauss rule (j u has degree 7: exact with 8 points)
    JU = 0.5 * np.diff(x) * ((case["j"] * up(xq)) @ case["wt"])
    assert abs(q.sum() - JU.sum()) <= 1e-13 * np.abs(JU).sum()


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
def _lib():
    from hybrid_fem_lssvr_amd import _capi
    return _capi.load()


def test_symbols_in_header_binding_and_library():
    from hybrid_fem_lssvr_amd import _capi
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "lssvr_hip.h")).read()
    for nm in NAMES:
        assert re.search(r"\b%s\s*\(" % nm, header), nm
        assert nm in _capi.SIGNATURES
        fn = getattr(lib, nm)
        assert fn.argtypes == _capi.SIGNATURES[nm][1] and fn.restype is _capi.SIGNATURES[nm][0]
    assert lib.lssvr_version() == 7 == _capi.ABI_VERSION          # additive: the version does not move
    assert header.index("lssvr_estimate_goal(") > header.index("lssvr_estimate_ends(")


def test_goal_work_bytes_is_host_arithmetic():
    """Four doubles per block of 64 elements, at most 4096 blocks."""
    wb = _lib().lssvr_goal_work_bytes
    assert wb(1) == 32 and wb(64) == 32 and wb(65) == 64
    assert wb(64 * 4096) == wb(10 ** 9) == 32 * 4096


def test_argument_errors_without_gpu():
    lib = _lib()
    pair = (ctypes.c_double * 2)(0.0, 2.0)

    def call(**over):
        a = dict(x=FAKE, Wu=FAKE, Wz=FAKE, ne=10, M=9, nq=8, a_values=FAKE, da_values=FAKE, c_values=None,
                 rhs_values=FAKE, goal_values=FAKE, table_layout=0, a_ends=FAKE, kind_left=0, kind_right=1,
                 kappa=pair, g=pair, a_bnd=pair, jump_free=0, eta=FAKE, eta2=FAKE, q=None, out4=FAKE, work=FAKE,
                 stream=None)
        assert set(over) <= set(a)
        a.update(over)
        rc = lib.lssvr_estimate_goal(*a.values())
        return rc, lib.lssvr_last_error().decode()

    for over, code, sub in (
            ({"ne": 0}, -2, "ne"), ({"ne": (1 << 40) + 1}, -2, "too large"), ({"M": 0}, -3, "M = 0"),
            ({"M": 34}, -3, "M = 34"), ({"nq": 0}, -7, "nq"), ({"nq": 33}, -7, "nq"),
            ({"x": None}, -1, "non-NULL"), ({"Wu": None}, -1, "non-NULL"), ({"Wz": None}, -1, "non-NULL"),
            ({"eta": None}, -1, "non-NULL"), ({"eta2": None}, -1, "non-NULL"), ({"out4": None}, -1, "non-NULL"),
            ({"work": None}, -1, "non-NULL"), ({"a_values": None}, -1, "non-NULL"),
            ({"da_values": None}, -1, "non-NULL"), ({"rhs_values": None}, -1, "non-NULL"),
            ({"goal_values": None}, -1, "goal_values"), ({"table_layout": 2}, -2, "unknown table_layout"),
            ({"a_ends": None}, -1, "a_ends"), ({"kind_left": 2}, -2, "end kinds"),
            ({"kind_right": -1}, -2, "end kinds"),
            ({"kappa": None}, -1, "kappa_host"), ({"kappa": (ctypes.c_double * 2)(0.0, -1.0)}, -2, "kappa[1]"),
            ({"g": None}, -1, "g_host"), ({"a_bnd": None}, -1, "a_bnd_host"), ({"jump_free": 2}, -2, "jump_free")):
        rc, msg = call(**over)
        assert rc == code and sub in msg, (over, rc, msg)


# ---------------------------------------------------------------------------
# facade
# ---------------------------------------------------------------------------
def _j(x):
    return np.exp(-np.asarray(x, dtype=np.float64) ** 2)


def test_facade_goal_value_errors_without_gpu():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    kw = dict(lssvr_M=5, lssvr_gamma=1e10, n_colloc=16, rhs=_j)
    s = pkg.FEMLSSVRPrimalSolver(9, convection=lambda x: 0.1 + 0.0 * x, **kw)
    for call in (lambda: s.solve_goal(_j), lambda: s.solve_adaptive(goal=_j)):
        with pytest.raises(ValueError, match="convection"):
            call()
    s = pkg.FEMLSSVRPrimalSolver(9, **kw)
    with pytest.raises(ValueError, match="mode='h'"):
        s.solve_adaptive(goal=_j, mode="hp")
    for bad in (1.0, "mean", (1, 2)):
        with pytest.raises(ValueError, match="callable"):
            s.solve_goal(bad)
        with pytest.raises(ValueError, match="callable"):
            s.solve_adaptive(goal=bad)
    with pytest.raises(ValueError, match="nq"):
        s.solve_goal(_j, nq=33)
    assert s._goal_nq(None) == 16 and s._goal_nq(8) == 8 and s._nq(None) == 8      # the goal path's own default
    s.lssvr_M = 20
    assert s._goal_nq(None) == 32
    s.lssvr_M = 5
    s.element_degrees = np.full(8, 5)
    for call in (lambda: s.solve_goal(_j), lambda: s.solve_adaptive(goal=_j)):
        with pytest.raises(ValueError, match="element_degrees"):
            call()
    for solver in (ops.SOLVER_DUAL, ops.SOLVER_SHARED, ops.SOLVER_PRIMAL_WAVE):
        s = pkg.FEMLSSVRPrimalSolver(9, solver=solver, **kw)
        with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
            s.solve_goal(_j)
        with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
            s.solve_adaptive(goal=_j)
    s = pkg.FEMLSSVRPrimalSolver(9, boundary=(None, ("robin", 1.0, 0.0)), **kw)
    s.fem_solver = "flux"                                   # (the constructor refuses the pair; attributes are public)
    with pytest.raises(ValueError, match="bands"):
        s.solve_goal(_j)
    with pytest.raises(ValueError, match="bands"):
        s.solve_adaptive(goal=_j)
    assert s.dual is None and s.adapt_history == []
