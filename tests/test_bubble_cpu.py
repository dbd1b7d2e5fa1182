"""CPU: the bubble-condensed P1 assembly without a device -- the host entry
lssvr_p1_assemble_bubble_host against the numpy prototype, the structure of the condensed matrices, and every refusal
of the C ABI and of the facade's ``fem_order``, each before any device call."""
import ctypes
import math
import types

import numpy as np
import pytest

from bubble_rules import LD, QUANTITIES, host_assemble, mesh, proto, reading, rounding_bar, tables

ORDER_NQUAD = [(2, 3), (2, 5), (3, 4), (3, 5), (4, 5)]      # order in 2 .. 4, nquad in {order+1, 5}


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("order,nquad", ORDER_NQUAD)
@pytest.mark.parametrize("ne", [1, 2, 7, 257])
def test_host_entry_matches_the_prototype(ne, order, nquad, R):
    """Bands, loads, kloc4 and floc of the host entry against the np.longdouble run of the prototype, each within
    the rounding bar (10x the float64 prototype's own reading, bubble_rules)."""
    x = mesh(ne, nquad)
    fq, aq, cq, bq = tables(x, nquad, R)
    got = host_assemble(x, order, nquad, fq, aq, cq, bq)
    p64 = proto.assemble(x, order, nquad, fq, aq, cq, bq)
    pld = proto.assemble(x, order, nquad, fq, aq, cq, bq, dtype=LD)
    for k in QUANTITIES:
        err, bar = reading(got[k], pld[k]), rounding_bar(p64[k], pld[k])
        print(f"ne={ne} order={order} nquad={nquad} R={R} {k}: {err:.3e} (bar {bar:.1e})")
        assert err <= bar, k


@pytest.mark.parametrize("order,nquad", ORDER_NQUAD)
def test_absent_tables_are_a_one_and_exact_zeros(order, nquad):
    """a_quad = NULL is the table of ones, b_quad / c_quad = NULL those of zeros, to the rounding bar."""
    x = mesh(7, nquad)
    fq, aq, cq, bq = tables(x, nquad, 2, with_b=False, with_c=False, const_a=1.0)
    got = host_assemble(x, order, nquad, fq)
    zero = np.zeros_like(aq)
    p64 = proto.assemble(x, order, nquad, fq, aq, zero, zero)
    pld = proto.assemble(x, order, nquad, fq, aq, zero, zero, dtype=LD)
    for k in QUANTITIES:
        assert reading(got[k], pld[k]) <= rounding_bar(p64[k], pld[k]), k


@pytest.mark.parametrize("order,nquad", ORDER_NQUAD)
def test_constant_a_decouples_the_bubbles(order, nquad):
    """Constant a, b = c = 0: N_k' (k >= 2) is orthogonal to the constants N_0', N_1', so the condensed matrix is
    the P1 one, kloc4 = (a / h) [[1, -1], [-1, 1]], and floc the plain P1 load less the bubbles' share, which for
    these bubbles is zero too (K_vb = 0) -- both to the rounding bar, for every order."""
    a0 = 1.7
    x = mesh(7, nquad)
    fq, aq, _, _ = tables(x, nquad, 2, with_b=False, with_c=False, const_a=a0)
    got = host_assemble(x, order, nquad, fq, aq)
    p64 = proto.assemble(x, order, nquad, fq, aq)
    h = np.diff(x.astype(LD))
    k = LD(a0) / h
    want_k = np.stack([k, -k, -k, k], axis=1)
    t, w = (v.astype(LD) for v in proto.rule(nquad))
    want_f = np.stack([h * ((w * fq.astype(LD)) @ (1 - t)), h * ((w * fq.astype(LD)) @ t)], axis=-1)
    for name, want in (("kloc4", want_k), ("floc", want_f)):
        err, bar = reading(got[name], want), rounding_bar(p64[name], want)
        print(f"order={order} nquad={nquad} {name}: {err:.3e} (bar {bar:.1e})")
        assert err <= bar, name


@pytest.mark.parametrize("order,nquad", ORDER_NQUAD)
@pytest.mark.parametrize("ne", [2, 7, 257])
def test_bands_are_symmetric_without_convection(ne, order, nquad):
    """b = 0: sub and sup agree within the rounding bar of the two bands (not to the bit: S01 and S10 come from two
    eliminations)."""
    x = mesh(ne, nquad)
    fq, aq, cq, _ = tables(x, nquad, 1, with_b=False)
    got = host_assemble(x, order, nquad, fq, aq, cq)
    p64 = proto.assemble(x, order, nquad, fq, aq, cq)
    pld = proto.assemble(x, order, nquad, fq, aq, cq, dtype=LD)
    scale = float(np.max(np.abs(pld["sub"])))
    bar = max(rounding_bar(p64["sub"], pld["sub"], scale), rounding_bar(p64["sup"], pld["sup"], scale))
    err = float(np.max(np.abs(got["sub"] - got["sup"]))) / scale
    print(f"ne={ne} order={order} nquad={nquad} |sub - sup|: {err:.3e} (bar {bar:.1e})")
    assert err <= bar


def test_zero_pivot_leaves_a_non_finite_band_entry():
    """There is no info word: a = 0 and c = 0 make the bubble block zero, and its elimination 0 / 0."""
    x = mesh(3)
    fq, aq, _, _ = tables(x, 4, 1, with_b=False, with_c=False, const_a=0.0)
    got = host_assemble(x, 3, 4, fq, aq)
    assert not np.all(np.isfinite(got["diag"])) and not np.all(np.isfinite(got["sub"]))


NULL, SIZE, DEGREE, QUAD = -1, -2, -3, -7


def _abi_call(lib, host, **change):
    ne, R = 4, 2
    fake = ctypes.c_void_p(4096)
    a = dict(x=fake, ne=ne, order=3, nquad=4, R=R, rhs_quad=fake, a_quad=None, c_quad=None, b_quad=None, diag=fake,
             sub=fake, sup=fake, load=fake, kloc4=None, floc=None, work=fake, work_bytes=(4 + 2 * R) * ne * 8)
    a.update(change)
    if host:
        cast = lambda v: ctypes.cast(v, ctypes.POINTER(ctypes.c_double)) if v is not None else None   # noqa: E731
        for k in ("x", "rhs_quad", "a_quad", "c_quad", "b_quad", "diag", "sub", "sup", "load", "kloc4", "floc"):
            a[k] = cast(a[k])
        return lib.lssvr_p1_assemble_bubble_host(*a.values())
    return lib.lssvr_p1_assemble_bubble(*a.values(), None)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_abi_refusals(host):
    """Every refusal of the entry by its error code, before any HIP call (the pointers are fakes)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    for change, code, word in (
            (dict(order=1), DEGREE, b"order"), (dict(order=5), DEGREE, b"order"), (dict(order=0), DEGREE, b"order"),
            (dict(nquad=3), QUAD, b"nquad"), (dict(nquad=6), QUAD, b"nquad"), (dict(order=4, nquad=4), QUAD, b"nquad"),
            (dict(R=0), SIZE, b"R = 0"), (dict(R=9), SIZE, b"R = 9"),
            (dict(ne=0), SIZE, b"ne"), (dict(ne=-3), SIZE, b"ne"),
            (dict(x=None), NULL, b"non-NULL"), (dict(rhs_quad=None), NULL, b"non-NULL"),
            (dict(diag=None), NULL, b"non-NULL"), (dict(sub=None), NULL, b"non-NULL"),
            (dict(sup=None), NULL, b"non-NULL"), (dict(load=None), NULL, b"non-NULL"),
            (dict(work=None), NULL, b"work"), (dict(work_bytes=8), SIZE, b"lssvr_p1_bubble_work_bytes")):
        rc = _abi_call(lib, host, **change)
        assert rc == code and word in lib.lssvr_last_error(), (change, rc, lib.lssvr_last_error())
    assert lib.lssvr_p1_bubble_work_bytes(1000, 3) == 10 * 1000 * 8


def _f(x):
    return np.sin(np.asarray(x, dtype=np.float64))


def _solver(**kw):
    import hybrid_fem_lssvr_amd as pkg
    kw = {**dict(rhs=_f, nquad=4, fem_order=3), **kw}
    return pkg.FEMLSSVRPrimalSolver(6, lssvr_M=9, lssvr_gamma=1e4, n_colloc=16, **kw)


@pytest.mark.parametrize("bad", [0, 5, -1, 2.0, "2", None, True])
def test_fem_order_must_be_an_integer_in_1_to_4(bad):
    with pytest.raises(ValueError, match="fem_order must be an integer in 1 .. 4"):
        _solver(fem_order=bad)


def test_construction_refusals():
    for order, nquad in ((2, 2), (3, 3), (4, 4), (4, 2)):
        with pytest.raises(ValueError, match="needs nquad in fem_order\\+1"):
            _solver(fem_order=order, nquad=nquad)
    with pytest.raises(ValueError, match="fem_order > 1 needs fem_solver='bands' or 'pivot'"):
        _solver(fem_solver="flux")
    with pytest.raises(ValueError, match="nonlinear has no fem_order > 1"):
        _solver(nonlinear=("poly", [_f, _f]))
    for order in (1, 2, 3, 4):
        assert _solver(fem_order=order, nquad=5).fem_order == order
    assert _solver(fem_order=1, nquad=2, fem_solver="flux").fem_order == 1


@pytest.fixture
def no_device(monkeypatch):
    """Every public ``ops`` function and every upload fails the test: what is refused is refused before them."""
    from hybrid_fem_lssvr_amd import ops, solver

    def forbidden(name):
        def fn(*a, **k):
            raise AssertionError(f"{name} was reached: the refusal must come before any device call")
        return fn
    for nm, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not nm.startswith("_") and fn.__module__ == ops.__name__:
            monkeypatch.setattr(ops, nm, forbidden(nm))
    monkeypatch.setattr(solver, "_to_dev", forbidden("_to_dev"))


def test_sin_rhs_is_refused_before_any_device_call(no_device):
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd.solver import SinRHS
    s = pkg.FEMLSSVRPrimalSolver(6, nquad=4, fem_order=3)              # the default right-hand side is a SinRHS
    for call in (s.solve_fem, s.solve, lambda: s.solve_many([_f, SinRHS(1.0, math.pi)])):
        with pytest.raises(ValueError, match="tabulated loads only"):
            call()
    with pytest.raises(ValueError, match="at most 8 load cases"):
        _solver().solve_many([_f] * 9)


def test_methods_that_assemble_for_themselves_refuse(no_device):
    """nonlinear=, solve_eigen, the three time loops, every *_sensitivity method, solve_goal and the adaptive modes
    built on them: ValueError before any device call."""
    s = _solver()
    one = lambda x: np.ones_like(np.asarray(x, dtype=np.float64))      # noqa: E731
    calls = dict(
        solve_eigen=lambda: s.solve_eigen(2),
        solve_transient=lambda: s.solve_transient(_f, 0.1, nsteps=2),
        solve_transient_adaptive=lambda: s.solve_transient_adaptive(_f, 0.1, rtol=1e-3, atol=1e-6, dt0=0.01),
        solve_wave=lambda: s.solve_wave(_f, _f, 0.1, nsteps=2),
        solve_transient_sensitivity=lambda: s.solve_transient_sensitivity(_f, 0.1, nsteps=2, goal=one),
        solve_wave_sensitivity=lambda: s.solve_wave_sensitivity(_f, _f, 0.1, nsteps=2, goal=one),
        solve_sensitivity=lambda: s.solve_sensitivity(one),
        solve_sensitivity_enhanced=lambda: s.solve_sensitivity(one, of="enhanced"),
        solve_semilinear_sensitivity=lambda: s.solve_semilinear_sensitivity(one),
        solve_goal=lambda: s.solve_goal(one),
        adaptive_goal=lambda: s.solve_adaptive(goal=one),
        adaptive_hp=lambda: s.solve_adaptive(mode="hp"))
    for name, call in calls.items():
        with pytest.raises(ValueError, match="has no fem_order > 1"):
            call()
    # the attribute is public: a solver switched to Newton after construction is refused where it solves
    s.nonlinear = ("poly", [_f, _f])
    with pytest.raises(ValueError, match="has no fem_order > 1"):
        s.solve_fem()
