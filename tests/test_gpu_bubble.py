"""GPU: the bubble-condensed P1 solve -- lssvr_p1_assemble_bubble bit-equal to its host
mirror, the nodal convergence orders h^(2 fem_order) through the facade, every boundary family, solve_many, the
dominance guard, the enhanced solution above the P1 floor, and ``fem_order=1`` as the calls it always made."""
import functools
import types

import numpy as np
import pytest

from bubble_rules import EPS, LD, QUANTITIES, host_assemble, mesh, proto, reading, rounding_bar, tables

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


@pytest.mark.parametrize("R", [1, 8])
@pytest.mark.parametrize("order", [2, 3, 4])
@pytest.mark.parametrize("ne", [1, 2, 7, 255, 256, 257, 5000])
def test_device_is_bit_equal_to_the_host_entry(dev, ne, order, R):
    """Every output of the device entry against lssvr_p1_assemble_bubble_host, bit for bit, around the workgroup
    edges (256 threads); R = 1 at nquad = order + 1, R = 8 at nquad = 5, so every instantiation but (2, 4) runs --
    that one at ne = 257."""
    from hybrid_fem_lssvr_amd import ops
    for nquad in sorted({order + 1 if R == 1 else 5} | ({4} if (ne, order) == (257, 2) else set())):
        x = mesh(ne, nquad)
        fq, aq, cq, bq = tables(x, nquad, R)
        want = host_assemble(x, order, nquad, fq, aq, cq, bq)
        got = ops.p1_assemble_bubble(_t(x, dev), order, nquad, _t(fq if R > 1 else fq[0], dev), a_quad=_t(aq, dev),
                                     c_quad=_t(cq, dev), b_quad=_t(bq, dev), want_local=True)
        assert "off" not in got and sorted(got) == sorted(QUANTITIES)
        assert tuple(got["load"].shape) == ((R, ne + 1) if R > 1 else (ne + 1,))
        for k in QUANTITIES:
            g = got[k].cpu().numpy().reshape(want[k].shape)
            assert np.array_equal(g, want[k]), (k, nquad, float(np.max(np.abs(g - want[k]))))
        # no tables: a = 1, b = c = 0
        want = host_assemble(x, order, nquad, fq)
        got = ops.p1_assemble_bubble(_t(x, dev), order, nquad, _t(fq, dev))
        for k in ("diag", "sub", "sup", "load"):
            assert np.array_equal(got[k].cpu().numpy(), want[k]), (k, nquad)


def _record_solver(ne, order, **kw):
    import hybrid_fem_lssvr_amd as pkg
    kw = {**dict(lssvr_M=9, lssvr_gamma=1e4, n_colloc=16), **kw}
    return pkg.FEMLSSVRPrimalSolver(ne + 1, global_domain=(0.0, 1.0), mesh=proto.graded_mesh(ne), rhs=proto.f_fn,
                                    coef=(proto.a_fn, proto.da_fn), convection=proto.b_fn, reaction=proto.c_fn,
                                    boundary=(("dirichlet", float(proto.u_fn(0.0))), ("dirichlet", float(proto.u_fn(1.0)))),
                                    nquad=order + 1, fem_order=order, **kw)


# fem_order: (the two meshes, the range of the observed order) -- where the prototype's error is still above 1e-10
ORDERS = {1: ((16, 32), (1.8, 2.2)), 2: ((8, 16), (3.7, 4.3)), 3: ((8, 16), (5.7, 6.3)), 4: ((4, 8), (7.7, 8.3))}


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_nodal_convergence_through_the_facade(order, note):
    """The record's problem (graded mesh, a, b, c variable, nquad = fem_order + 1): the max nodal error falls like
    h^(2 fem_order), and each device error is within 2x the prototype's on the same case."""
    (n0, n1), (lo, hi) = ORDERS[order]
    errs = []
    for ne in (n0, n1):
        s = _record_solver(ne, order)
        u, _ = s.solve_fem()
        err = float(np.max(np.abs(u - proto.u_fn(proto.graded_mesh(ne)))))
        perr = proto.nodal_error(ne, order)
        print(f"fem_order={order} ne={ne}: device {err:.3e}, prototype {perr:.3e}")
        note(f"fem_order={order} ne={ne} nodal error", err, 2.0 * perr)
        assert err <= 2.0 * perr
        errs.append(err)
    rate = float(np.log2(errs[0] / errs[1]))
    print(f"fem_order={order}: observed order {rate:.2f} from ne = {n0} -> {n1}")
    assert lo <= rate <= hi


def _a(x):
    return 1.0 + 0.3 * np.sin(np.pi * x)


def _da(x):
    return 0.3 * np.pi * np.cos(np.pi * x)


def _b(x):
    return 0.8 * np.sin(np.pi * x)          # (zero at both ends: a Neumann end keeps its coercivity)


def _c(x):
    return 1.0 + 0.5 * np.cos(np.pi * x)


def _f(x):
    return np.exp(x) * np.sin(3.0 * x)


FAMILIES = {
    "dirichlet": dict(boundary=(("dirichlet", 0.3), ("dirichlet", -0.2))),
    "robin-dirichlet": dict(boundary=(("robin", 2.0, 0.5), ("dirichlet", 0.1))),
    "neumann-neumann": dict(boundary=(("neumann", 0.4), ("neumann", -0.3))),
    "periodic": dict(boundary="periodic"),
    "pivot": dict(boundary=(("dirichlet", 0.3), ("dirichlet", -0.2)), fem_solver="pivot"),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_boundary_family(family, note):
    """fem_order = 3 on 33 non-uniform elements with periodic coefficients: the device's bands within 32 eps of each
    entry's scale of the prototype's assembly, and the nodal values against the prototype's dense np.longdouble solve
    on the device's own bands, at the rounding bar."""
    import hybrid_fem_lssvr_amd as pkg
    ne, order, nquad = 33, 3, 4
    x = mesh(ne)
    kw = FAMILIES[family]
    s = pkg.FEMLSSVRPrimalSolver(ne + 1, lssvr_M=9, lssvr_gamma=1e4, n_colloc=16, global_domain=(-1.0, 1.0), mesh=x,
                                 rhs=_f, coef=(_a, _da), convection=_b, reaction=_c, nquad=nquad, fem_order=order, **kw)
    u, _ = s.solve_fem()
    bands = {k: s.bands[k].cpu().numpy() for k in ("diag", "sub", "sup", "load")}
    xq = proto.quad_points(x, nquad)
    want = proto.assemble(x, order, nquad, _f(xq), _a(xq), _c(xq), _b(xq))
    for k in bands:
        err = reading(bands[k], want[k].reshape(bands[k].shape))
        print(f"{family} {k}: {err:.3e} of the entry's scale (bar {32 * EPS:.1e})")
        assert err <= 32 * EPS, k
    periodic = family == "periodic"
    if periodic:
        free, kappa, ends = (False, False), (0.0, 0.0), (0.0, 0.0)
    else:
        spec = kw["boundary"]
        free = tuple(sp[0] != "dirichlet" for sp in spec)
        kappa = tuple(sp[1] if sp[0] == "robin" else 0.0 for sp in spec)
        ends = tuple(sp[-1] for sp in spec)
    args = (bands["diag"], bands["sub"], bands["sup"], bands["load"], ends, free, kappa, periodic)
    u64, uld = proto.solve_bands(*args), proto.solve_bands(*args, dtype=LD)
    err, bar = reading(u, uld), rounding_bar(u64, uld)
    print(f"{family} nodal values: {err:.3e} (bar {bar:.1e})")
    note(f"bubble {family} nodal vs longdouble dense solve", err, bar)
    assert err <= bar


def test_solve_many_rows_are_the_single_solves(dev):
    """Three right-hand sides with different end values in ONE assembly and one solve: each row bit-equal to the
    single solve of that case."""
    import hybrid_fem_lssvr_amd as pkg
    x = mesh(33)
    s = pkg.FEMLSSVRPrimalSolver(34, lssvr_M=9, lssvr_gamma=1e4, n_colloc=16, global_domain=(-1.0, 1.0), mesh=x,
                                 rhs=_f, coef=(_a, _da), convection=_b, reaction=_c, nquad=4, fem_order=3)
    rhs_list = [_f, lambda t: np.cos(2.0 * t), lambda t: 1.0 + t * t]
    bc = np.array([[0.3, -0.2], [0.0, 1.0], [-0.5, 0.25]])
    _, U = s._fem_many(rhs_list, bc)
    U = U.cpu().numpy()
    for j, f in enumerate(rhs_list):
        one = s._fem(f, float(bc[j, 0]), float(bc[j, 1]))[2].cpu().numpy()
        assert np.array_equal(U[j], one), j
    sols = s.solve_many(rhs_list, bc)
    assert len(sols) == 3 and all(int(e.n_fallback) == 0 for e in sols)


def test_dominance_guard():
    """a = 0.002 and b = 30 - 25 x on the two elements [-1, 0.1, 1]: the interior row of the condensed bands is not
    dominant (the prototype says so first).  ``fem_solver="bands"`` refuses before the solve; "pivot" solves, and
    its value is the prototype's: one unknown, u_1 = load_1 / diag_1, each within 32 eps of the prototype's entry,
    hence 100 eps with the division and the solve's own rounding."""
    import hybrid_fem_lssvr_amd as pkg
    x = np.array([-1.0, 0.1, 1.0])
    a = lambda t: 0.002 + 0.0 * np.asarray(t)        # noqa: E731
    b = lambda t: 30.0 - 25.0 * np.asarray(t)        # noqa: E731
    one = lambda t: 1.0 + 0.0 * np.asarray(t)        # noqa: E731
    xq = proto.quad_points(x, 4)
    want = proto.assemble(x, 3, 4, one(xq), a(xq), None, b(xq))
    row, margin = proto.dominance(want["diag"], want["sub"], want["sup"])
    assert row == 1 and margin < -1.0
    kw = dict(lssvr_M=9, lssvr_gamma=1e4, n_colloc=16, global_domain=(-1.0, 1.0), mesh=x, rhs=one,
              coef=(a, lambda t: 0.0 * np.asarray(t)), convection=b, nquad=4, fem_order=3,
              boundary=(("dirichlet", 0.0), ("dirichlet", 0.0)))
    with pytest.raises(ValueError, match=r"row 1 .*\[-1, 1\].* not diagonally dominant.*fem_solver='pivot'"):
        pkg.FEMLSSVRPrimalSolver(3, **kw).solve_fem()
    u, _ = pkg.FEMLSSVRPrimalSolver(3, fem_solver="pivot", **kw).solve_fem()
    u_ref = proto.solve_bands(want["diag"], want["sub"], want["sup"], want["load"][0])
    assert np.max(np.abs(u - u_ref)) <= 100 * EPS * np.max(np.abs(u_ref))


def test_the_floor_is_lifted(note):
    """The record's problem on 16 elements, M = 9, 16 points, gamma = 1e4: the max error of the ENHANCED solution over
    2001 points with fem_order = 3 is below that with fem_order = 1, and within 2x of the prototype pipeline's own
    (prototype nodal values into the oracle's enhancement)."""
    from oracle import lssvr_oracle as orc
    ne, xs = 16, np.linspace(0.0, 1.0, 2001)
    exact = proto.u_fn(xs)
    errs = {}
    for order in (1, 3):
        s = _record_solver(ne, order)
        s.solve()
        errs[order] = float(np.max(np.abs(s.evaluate_solution(xs) - exact)))
    x, U = proto.solve_problem(ne, 3)
    W, _ = orc.enhance_all(x, U, 9, 1e4, 16, rhs=proto.f_fn, global_domain=(0.0, 1.0), coef_a=proto.a_fn,
                           coef_da=lambda t: proto.da_fn(t) - proto.b_fn(t), coef_c=proto.c_fn,
                           bc_left=float(proto.u_fn(0.0)), bc_right=float(proto.u_fn(1.0)))
    perr = float(np.max(np.abs(orc.evaluate_solution(x, W, xs)[0] - exact)))
    print(f"enhanced max error, ne=16: fem_order=1 {errs[1]:.3e}, fem_order=3 {errs[3]:.3e}, prototype pipeline "
          f"{perr:.3e}")
    note("enhanced max error fem_order=1", errs[1])
    note("enhanced max error fem_order=3", errs[3], 2.0 * perr)
    assert errs[3] < errs[1]
    assert errs[3] <= 2.0 * perr


def test_fem_order_1_runs_the_calls_it_always_made(monkeypatch, dev):
    """``fem_order=1`` (given or not) reaches exactly the ``ops`` functions of the solve before ``fem_order`` existed,
    and ``bands`` holds what ``ops.p1_assemble`` gives for the case, bit for bit."""
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    x = mesh(33)
    kw = dict(lssvr_M=9, lssvr_gamma=1e4, n_colloc=16, global_domain=(-1.0, 1.0), mesh=x, rhs=_f, coef=(_a, _da),
              convection=_b, reaction=_c, nquad=3)
    xd = _t(x, dev)
    xq = ops.quad_points(xd, 3)
    xqh = xq.cpu().numpy()
    want = ops.p1_assemble(xd, 3, rhs_quad=_t(_f(xqh), dev), a_quad=_t(_a(xqh), dev), c_quad=_t(_c(xqh), dev),
                           b_quad=_t(_b(xqh), dev), want_local=True)
    want = {k: v.cpu().numpy() for k, v in want.items()}
    calls = []

    def logged(label, fn):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            calls.append(label)
            return fn(*a, **k)
        return wrapper
    for nm, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not nm.startswith("_") and fn.__module__ == ops.__name__:
            monkeypatch.setattr(ops, nm, logged(nm, fn))
    expected = ["quad_points", "p1_assemble", "tridiag_ns_dirichlet_solve", "colloc_points", "enhance_varcoef"]
    for extra in ({}, dict(fem_order=1)):
        del calls[:]
        s = pkg.FEMLSSVRPrimalSolver(34, **kw, **extra)
        s.solve()
        assert calls == expected, calls
        assert sorted(s.bands) == sorted(want)
        for k in want:
            assert np.array_equal(s.bands[k].cpu().numpy(), want[k]), k
    del calls[:]
    s = pkg.FEMLSSVRPrimalSolver(34, **{**kw, "nquad": 4}, fem_order=3)
    s.solve()
    assert calls == ["quad_points", "p1_assemble_bubble", "band_dominance", "tridiag_ns_dirichlet_solve",
                     "colloc_points", "enhance_varcoef"], calls
