"""GPU: the P1 half of several load cases -- ``ops.p1_load_multi`` and the two multi-RHS tridiagonal solves
(include/lssvr_hip.h: lssvr_p1_load_multi, lssvr_tridiag_dirichlet_solve_multi, lssvr_tridiag_ns_dirichlet_solve_multi)
against nc calls of the single entries, bit for bit, and against host references of their own; then
``FEMLSSVRPrimalSolver.solve_many``, which runs on them, against the per-case path it replaced."""
import functools

import numpy as np
import pytest

from oracle import lssvr_oracle as orc
import convection_rules as cr

pytestmark = pytest.mark.gpu

# m = ne - 1 unknowns, chunks of 8, base level of 512: empty and tiny base (1, 2, 3); full base (513); one level whose
# last chunk holds one unknown (514); last unknown a separator (521); reduced system exactly fills the base (4098);
# two (4105) and three (33000) chunked levels
SIZES = [1, 2, 3, 513, 514, 521, 4098, 4105, 33000]
MESHES = ["uniform", "graded"]
OPERATORS = ["sym", "ns"]

# The bars of tests/test_gpu_conv.py::test_tridiag_ns_dirichlet_solve, copied as formulas: the residual within
# 1e-13 max|diag| max|u| max(1, log2 ne); the forward error against the long-double Thomas solve within
# max(10 x LAPACK's own distance from it, _forward_bar(ne)) max|u|, a size between two listed ones taking the bar of
# the next listed size.
TRIDIAG_FORWARD_BAR = {1: 0.0, 2: 1e-15, 3: 1e-15, 24: 1e-14, 511: 2.5e-12, 512: 2.5e-12, 513: 2.5e-12,
                       514: 2.5e-12, 1025: 4e-12, 16385: 2e-9, 100000: 7e-8, 1234567: 2e-6}


def _forward_bar(ne):
    return TRIDIAG_FORWARD_BAR[min(k for k in TRIDIAG_FORWARD_BAR if k >= ne)]


def _rc():
    from hybrid_fem_lssvr_amd import ops
    return ops.TRIDIAG_MULTI_CASES


def _case_counts():
    rc = _rc()
    return [1, 2, rc, rc + 1, 2 * rc + 1]


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _nodes(ne, mesh):
    t = np.linspace(0.0, 1.0, ne + 1)
    return -1.0 + 2.0 * (t if mesh == "uniform" else 0.3 * t + 0.7 * t * t)


def _a(x):
    return 1.0 + 0.25 * np.asarray(x, dtype=np.float64) ** 2


def _c(x):
    return 2.0 + np.cos(2.0 * np.pi * np.asarray(x, dtype=np.float64))


def _bc(ncases):
    return np.array([[0.25 + 0.1 * j, -0.5 - 0.05 * j] for j in range(ncases)])


def _thomas_ld_many(diag, sub, sup, loads, bc):
    """cr.thomas_ns_ld for every row of ``loads`` at once: Thomas elimination without pivoting in long double, the
    matrix eliminated once.  Returns long double [ncases, ne+1]."""
    ld = np.longdouble
    ncases, n = loads.shape
    u = np.zeros((ncases, n), dtype=ld)
    u[:, 0], u[:, -1] = bc[:, 0].astype(ld), bc[:, 1].astype(ld)
    m = n - 2
    if m <= 0:
        return u
    d = np.asarray(diag[1:-1], dtype=ld).copy()
    lo = np.asarray(sub[1:-1], dtype=ld)
    up = np.asarray(sup[1:-1], dtype=ld)
    r = np.asarray(loads[:, 1:-1], dtype=ld).T.copy()               # [m, ncases]
    r[0] -= ld(sub[0]) * u[:, 0]
    r[-1] -= ld(sup[-1]) * u[:, -1]
    for i in range(1, m):
        w = lo[i - 1] / d[i - 1]
        d[i] -= w * up[i - 1]
        r[i] -= w * r[i - 1]
    x = np.zeros((m, ncases), dtype=ld)
    x[-1] = r[-1] / d[-1]
    for i in range(m - 2, -1, -1):
        x[i] = (r[i] - up[i] * x[i + 1]) / d[i]
    u[:, 1:-1] = x.T
    return u


def _lapack_many(diag, sub, sup, loads, bc):
    """cr.banded_ns for every row of ``loads``: LAPACK's banded LU with partial pivoting."""
    from scipy.linalg import solve_banded
    ncases, n = loads.shape
    u = np.zeros((ncases, n))
    u[:, 0], u[:, -1] = bc[:, 0], bc[:, 1]
    if n <= 2:
        return u
    ab = np.zeros((3, n - 2))
    ab[1] = diag[1:-1]
    ab[0, 1:] = sup[1:-1]
    ab[2, :-1] = sub[1:-1]
    r = np.array(loads[:, 1:-1].T)
    r[0] -= sub[0] * bc[:, 0]
    r[-1] -= sup[-1] * bc[:, 1]
    u[:, 1:-1] = solve_banded((1, 1), ab, r).T
    return u


@functools.lru_cache(maxsize=None)
def _problem(ne, mesh, operator):
    """(diag, sub, sup, loads[2 RC + 1, ne+1], bc, u_ld, u_lapack), computed once and shared: do not write to them.
    "sym": the bands of -(a u')' + c u with a > 0, c >= 0 (sub is sup is off); "ns": those of -u'' + b u' + u with
    the largest cell Peclet number at 0.5."""
    nodes = _nodes(ne, mesh)
    ncases = 2 * _rc() + 1
    if operator == "sym":
        diag, off, load0, _ = orc.p1_bands(nodes, orc.poisson_rhs, _a, 2, _c)
        sub = sup = off
    else:
        unit = cr.cell_peclet(nodes, None, cr.SHAPES["pos"]).max()
        b = lambda x: (0.5 / unit) * cr.SHAPES["pos"](np.asarray(x, dtype=np.float64))     # noqa: E731
        diag, sub, sup, load0, _ = cr.conv_bands(nodes, orc.poisson_rhs, None, b, lambda x: 1.0 + 0.0 * x)
    h = np.diff(nodes)
    hbar = np.concatenate([[h[0]], 0.5 * (h[:-1] + h[1:]), [h[-1]]])
    loads = np.stack([(1.0 + 0.25 * j) * load0 + 0.5 * j * hbar * np.cos((j + 1) * nodes) for j in range(ncases)])
    bc = _bc(ncases)
    return diag, sub, sup, loads, bc, _thomas_ld_many(diag, sub, sup, loads, bc), _lapack_many(diag, sub, sup, loads, bc)


def _entries(operator):
    from hybrid_fem_lssvr_amd import ops
    if operator == "sym":
        return (lambda d, lo, up, *a, **k: ops.tridiag_dirichlet_solve(d, lo, *a, **k),
                lambda d, lo, up, *a, **k: ops.tridiag_dirichlet_solve_multi(d, lo, *a, **k))
    return ops.tridiag_ns_dirichlet_solve, ops.tridiag_ns_dirichlet_solve_multi


# ---------------------------------------------------------------------------
# 1. the loads
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nquad", [1, 2, 5])
@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("ne", [1, 2, 300])
def test_p1_load_multi_is_the_assembled_load(dev, ne, mesh, nquad):
    """Every load[j] has the bits of the load that ops.p1_assemble writes for rhs_quad[j]: without coefficient
    tables, with a_quad and c_quad (lssvr_p1_assemble_react), with b_quad too (lssvr_p1_assemble_conv); for every
    case count of the solves.  300 elements are more than one workgroup of nodes."""
    from hybrid_fem_lssvr_amd import ops
    x = _t(_nodes(ne, mesh), dev)
    xq = ops.quad_points(x, nquad)
    ncases = 2 * _rc() + 1
    fq = _t(np.stack([(1.0 + 0.25 * j) * orc.poisson_rhs(xq.cpu().numpy()) + 0.5 * j for j in range(ncases)]), dev)
    variants = [{}, dict(a_quad=_t(_a(xq.cpu().numpy()), dev), c_quad=_t(_c(xq.cpu().numpy()), dev))]
    variants.append(dict(variants[1], b_quad=_t(0.5 + 0.0 * xq.cpu().numpy(), dev)))
    for nc in _case_counts():
        got = ops.p1_load_multi(x, fq[:nc], nquad).cpu().numpy()
        assert got.shape == (nc, ne + 1)
        for kw in variants:
            for j in range(nc):
                want = ops.p1_assemble(x, nquad, rhs_quad=fq[j], **kw)["load"].cpu().numpy()
                assert np.array_equal(got[j], want), (nc, j, sorted(kw))


# ---------------------------------------------------------------------------
# 2. the solves
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("ne", SIZES)
def test_tridiag_multi_is_the_single_entry_case_by_case(dev, ne, mesh, operator):
    """Row j of the multi solve has the bits of the single entry on case j, for nc in {1, 2, RC, RC+1, 2 RC+1};
    u[j][0] and u[j][ne] are bc[j] exactly; bc=None gives zeros there and the single entry's bits with (0, 0); a
    second call repeats the first bit for bit."""
    diag, sub, sup, loads, bc, _, _ = _problem(ne, mesh, operator)
    single, multi = _entries(operator)
    d, lo, up, L = _t(diag, dev), _t(sub, dev), _t(sup, dev), _t(loads, dev)
    ref = np.stack([single(d, lo, up, L[j], bc[j, 0], bc[j, 1]).cpu().numpy() for j in range(len(loads))])
    for nc in _case_counts():
        u = multi(d, lo, up, L[:nc], _t(bc[:nc], dev)).cpu().numpy()
        assert u.shape == (nc, ne + 1)
        assert np.array_equal(u[:, 0], bc[:nc, 0]) and np.array_equal(u[:, -1], bc[:nc, 1])
        for j in range(nc):
            assert np.array_equal(u[j], ref[j]), (nc, j, float(np.max(np.abs(u[j] - ref[j]))))
        again = multi(d, lo, up, L[:nc], bc[:nc]).cpu().numpy()            # (a host bc is copied to the device)
        assert np.array_equal(again, u), nc
    nc = _rc() + 1
    u = multi(d, lo, up, L[:nc]).cpu().numpy()
    assert not u[:, 0].any() and not u[:, -1].any()
    for j in (0, nc - 1):
        assert np.array_equal(u[j], single(d, lo, up, L[j], 0.0, 0.0).cpu().numpy()), j


@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("mesh", MESHES)
@pytest.mark.parametrize("ne", SIZES)
def test_tridiag_multi_against_host_references(dev, note, ne, mesh, operator):
    """Independent of the single entry: every case of a 2 RC + 1 case call meets the residual bar and the forward
    bar that tests/test_gpu_conv.py::test_tridiag_ns_dirichlet_solve puts on the single entry (copied above)."""
    diag, sub, sup, loads, bc, u_ld, u_la = _problem(ne, mesh, operator)
    _, multi = _entries(operator)
    u = multi(_t(diag, dev), _t(sub, dev), _t(sup, dev), _t(loads, dev), _t(bc, dev)).cpu().numpy()
    worst_res = worst_fwd = 0.0
    for j in range(len(loads)):
        scale = float(np.max(np.abs(u_ld[j])))
        if ne > 1:
            r = diag[1:-1] * u[j, 1:-1] + sub[:-1] * u[j, :-2] + sup[1:] * u[j, 2:] - loads[j, 1:-1]
            res, res_bar = np.max(np.abs(r)), 1e-13 * np.max(np.abs(diag)) * scale * max(1.0, np.log2(ne))
            worst_res = max(worst_res, res / res_bar)
            print(f"ne={ne} {mesh} {operator} case {j}: residual {res:.2e} (bar {res_bar:.2e})")
            assert res <= res_bar, j
        lapack = float(np.max(np.abs(u_la[j].astype(np.longdouble) - u_ld[j])))
        fwd = float(np.max(np.abs(u[j].astype(np.longdouble) - u_ld[j])))
        bar = max(10.0 * lapack, _forward_bar(ne)) * scale
        if bar > 0:
            worst_fwd = max(worst_fwd, fwd / bar)
        print(f"ne={ne} {mesh} {operator} case {j}: forward {fwd:.2e}, LAPACK {lapack:.2e}, bar {bar:.2e}")
        assert fwd <= bar, j
    note(f"tridiag multi ne={ne} {mesh} {operator}: largest residual / bar over the cases", worst_res, 1.0)
    note(f"tridiag multi ne={ne} {mesh} {operator}: largest forward error / bar over the cases", worst_fwd, 1.0)


# ---------------------------------------------------------------------------
# 3. output discipline and validation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("operator", OPERATORS)
@pytest.mark.parametrize("ne", [3, 4105])
def test_tridiag_multi_writes_its_cases_only(dev, ne, operator):
    """out holds two cases more than the call has and is filled with a sentinel, work is the caller's: the first nc
    rows are the solution, the rest keep the sentinel; a pass with idle slots (nc = RC + 2: a pass of two) and a pass
    of one (RC + 1) store nothing outside their cases."""
    import torch
    from hybrid_fem_lssvr_amd import _capi
    diag, sub, sup, loads, bc, _, _ = _problem(ne, "graded", operator)
    _, multi = _entries(operator)
    d, lo, up, L = _t(diag, dev), _t(sub, dev), _t(sup, dev), _t(loads, dev)
    lib = _capi.load()
    for nc in (2, _rc() + 1, _rc() + 2):
        want = multi(d, lo, up, L[:nc], bc[:nc]).cpu().numpy()
        out = torch.full((nc + 2, ne + 1), -7.25, dtype=torch.float64, device=dev)
        nbytes = lib.lssvr_tridiag_multi_work_bytes(ne, nc)
        work = torch.full((nbytes // 8 + 64,), -7.25, dtype=torch.float64, device=dev)
        got = multi(d, lo, up, L[:nc], bc[:nc], out=out, work=work)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (nc, ne + 1)
        assert np.array_equal(out[:nc].cpu().numpy(), want)
        assert bool((out[nc:] == -7.25).all().item())
        assert bool((work[(nbytes + 7) // 8:] == -7.25).all().item())       # nothing past the stated size


def test_p1_load_multi_writes_its_cases_only(dev):
    import torch
    from hybrid_fem_lssvr_amd import ops
    x = _t(_nodes(300, "graded"), dev)
    fq = _t(np.stack([(1.0 + j) * orc.poisson_rhs(ops.quad_points(x, 2).cpu().numpy()) for j in range(3)]), dev)
    out = torch.full((5, 301), -7.25, dtype=torch.float64, device=dev)
    got = ops.p1_load_multi(x, fq, 2, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (3, 301)
    assert np.array_equal(out[:3].cpu().numpy(), ops.p1_load_multi(x, fq, 2).cpu().numpy())
    assert bool((out[3:] == -7.25).all().item())


def test_multi_entries_reject_wrong_arguments(dev):
    """Shapes and the workspace are checked on the host, before any launch."""
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    z = lambda *n: torch.zeros(*n, dtype=torch.float64, device=dev)                # noqa: E731
    for sizes in ((6, 5, (2, 5)), (5, 5, (2, 6)), (6, 4, (2, 6)), (6, 5, (12,))):
        with pytest.raises(ValueError, match="band lengths"):
            ops.tridiag_dirichlet_solve_multi(*(z(n) for n in sizes))
    for sizes in ((6, 5, 4, (2, 6)), (6, 5, 5, (2, 5)), (6, 5, 5, (12,))):
        with pytest.raises(ValueError, match="band lengths"):
            ops.tridiag_ns_dirichlet_solve_multi(*(z(n) for n in sizes))
    with pytest.raises(ValueError, match="out must be"):
        ops.tridiag_dirichlet_solve_multi(z(6), z(5), z(3, 6), out=z(2, 6))
    with pytest.raises(ValueError, match="out must be"):
        ops.tridiag_ns_dirichlet_solve_multi(z(6), z(5), z(5), z(3, 6), out=z(3, 5))
    with pytest.raises(ValueError, match=r"bc must be \[nc, 2\]"):
        ops.tridiag_dirichlet_solve_multi(z(6), z(5), z(3, 6), z(2, 2))
    with pytest.raises(ValueError, match="work holds"):
        ops.tridiag_dirichlet_solve_multi(z(6), z(5), z(3, 6), work=z(4))
    with pytest.raises(ValueError, match="work holds"):
        ops.tridiag_ns_dirichlet_solve_multi(z(6), z(5), z(5), z(3, 6), work=z(4))
    with pytest.raises(ValueError, match="rhs_quad must be"):
        ops.p1_load_multi(z(6), z(3, 5, 3), 2)
    with pytest.raises(ValueError, match="rhs_quad must be"):
        ops.p1_load_multi(z(6), z(5, 2), 2)
    with pytest.raises(ValueError, match="out must be"):
        ops.p1_load_multi(z(6), z(3, 5, 2), 2, out=z(2, 6))
    # the ABI's own check of the workspace, with valid device pointers and no launch
    lib = _capi.load()
    d, o, L, u, w = z(6), z(5), z(3, 6), z(3, 6), z(4)
    rc = lib.lssvr_tridiag_dirichlet_solve_multi(d.data_ptr(), o.data_ptr(), L.data_ptr(), 5, 3, None, u.data_ptr(),
                                                 w.data_ptr(), 32, torch.cuda.current_stream().cuda_stream)
    assert rc == -2 and b"work holds" in lib.lssvr_last_error()


# ---------------------------------------------------------------------------
# 4. facade
# ---------------------------------------------------------------------------
def _per_case_path(s, fs, bc):
    """What solve_many computed before the multi entries: the assembly and the single solve case by case, as
    FEMLSSVRPrimalSolver._fem makes them, from public ops calls; then the same ops.enhance_multi call."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    from hybrid_fem_lssvr_amd.solver import SinRHS, _Equation, _tabulate, _to_dev, _zero
    dev = torch.device(s.device)
    x = _to_dev(np.linspace(s.global_domain[0], s.global_domain[1], s.num_fem_nodes), dev)
    xq = ops.quad_points(x, s.nquad)
    kw = {}
    if s.coef is not None:
        kw["a_quad"] = _tabulate(s.coef[0], xq)
    if s.reaction is not None:
        kw["c_quad"] = _tabulate(s.reaction, xq)
    if s.convection is not None:
        kw["b_quad"] = _tabulate(s.convection, xq)
    us = []
    for f, (u0, u1) in zip(fs, bc):
        if isinstance(f, SinRHS):
            bands = ops.p1_assemble(x, s.nquad, rhs=(f.amp, f.omega), want_local=True, **kw)
        else:
            bands = ops.p1_assemble(x, s.nquad, rhs_quad=_to_dev(f(xq.cpu().numpy()), dev), want_local=True, **kw)
        if s.convection is not None:
            us.append(ops.tridiag_ns_dirichlet_solve(bands["diag"], bands["sub"], bands["sup"], bands["load"],
                                                     float(u0), float(u1)))
        else:
            us.append(ops.tridiag_dirichlet_solve(bands["diag"], bands["off"], bands["load"], float(u0), float(u1)))
    M, n = int(s.lssvr_M), int(s.n_colloc)
    pm = M <= 16
    pts = ops.colloc_points(x, n)
    ta, tda, _, tc = _Equation(_zero, s.coef, s.reaction, s.convection).tables(pts, pm)
    tf = torch.stack([_tabulate(f, pts, pm) for f in fs])
    gd = (float(s.global_domain[0]), float(s.global_domain[1]))
    W, _ = ops.enhance_multi(x, torch.stack(us), M, float(s.lssvr_gamma), n, ta, tda, tf, c_values=tc,
                             bc=_to_dev(bc, dev), point_major=pm, global_domain=gd)
    return torch.stack(us), W


@pytest.mark.parametrize("variant", ["poisson", "coef+reaction", "convection", "poisson+sin"])
def test_facade_solve_many_keeps_its_bits(dev, variant):
    """solve_many(fs)[j].W and the nodal values behind it equal, bit for bit, what the per-case P1 path followed by
    the same ops.enhance_multi call gives: Poisson, coef + reaction, convection, and a list that mixes a SinRHS with
    callables.  2 RC + 1 cases: two full passes and a pass of one."""
    import hybrid_fem_lssvr_amd as pkg
    a, da, c, f = orc.react_functions(4.0)
    kw = dict(lssvr_M=9, lssvr_gamma=1e4, n_colloc=16, nquad=3)
    if variant == "coef+reaction":
        kw.update(coef=(a, da), reaction=c)
    elif variant == "convection":
        kw.update(coef=(cr.man_a, cr.man_da), reaction=cr.man_c, convection=cr.man_b)
        f = cr.man_f
    ncases = 2 * _rc() + 1 if variant != "poisson+sin" else 3
    fs = [(lambda x, j=j: (1.0 + 0.25 * j) * f(x) + 0.5 * j) for j in range(ncases)]
    if variant == "poisson+sin":
        fs[1] = pkg.solver.SinRHS(float(np.pi ** 2), float(np.pi))
    s = pkg.FEMLSSVRPrimalSolver(61, **kw)
    bc = _bc(ncases)
    sols = s.solve_many(fs, bc=bc)
    U_ref, W_ref = _per_case_path(s, fs, bc)
    _, U = s._fem_many(fs, bc)
    assert np.array_equal(U.cpu().numpy(), U_ref.cpu().numpy())
    for j, sol in enumerate(sols):
        assert np.array_equal(sol.W.cpu().numpy(), W_ref[j].cpu().numpy()), j
        assert sol.n_fallback == 0
