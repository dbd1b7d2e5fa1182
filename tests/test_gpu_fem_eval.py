"""GPU parity tests of the rows either side of the enhancement kernel: element-local
P1 assembly (Dual.py:117-128), Dirichlet + tridiagonal solve (Dual.py:129-130),
evaluate_solution (Dual.py:176-203), the variable-coefficient rows (BASELINE config 5)
and the Python facade that mirrors the reference's call surface."""
import functools

import numpy as np
import pytest

import convection_rules as cr
from oracle import lssvr_oracle as orc
from oracle import closed_form_mp as cf

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


@pytest.mark.parametrize("nquad", [1, 2, 3, 4, 5])
def test_p1_assemble_vs_oracle(dev, nquad):
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(7 + nquad)
    ne = 4097
    nodes = np.cumsum(np.concatenate([[-2.0], rng.uniform(1e-3, 2e-3, ne)]))
    out = ops.p1_assemble(_t(nodes, dev), nquad, want_local=True)
    kd, fl, fr = orc.p1_assemble_local(nodes, nquad=nquad)
    diag, off, load = orc.p1_scatter(kd, fl, fr)
    h = {k: v.cpu().numpy() for k, v in out.items()}
    assert np.allclose(h["kloc"], kd, rtol=1e-15, atol=0)
    assert np.allclose(h["floc"][:, 0], fl, rtol=1e-13, atol=1e-18)
    assert np.allclose(h["floc"][:, 1], fr, rtol=1e-13, atol=1e-18)
    assert np.allclose(h["diag"], diag, rtol=1e-15, atol=0)
    assert np.array_equal(h["off"], -h["kloc"])
    assert np.allclose(h["load"], load, rtol=1e-13, atol=1e-18)
    # tabulated right-hand side (arbitrary callable on the host) == in-kernel sin
    xq = ops.quad_points(_t(nodes, dev), nquad)
    assert np.allclose(xq.cpu().numpy(), orc.quad_points(nodes, nquad), rtol=1e-15, atol=0)
    out2 = ops.p1_assemble(_t(nodes, dev), nquad, rhs_quad=_t(orc.poisson_rhs(xq.cpu().numpy()), dev))
    assert np.allclose(out2["load"].cpu().numpy(), h["load"], rtol=1e-13, atol=1e-18)


@pytest.mark.parametrize("ne", [1, 2, 3, 24, 511, 512, 513, 514, 1025, 16385, 100000, 1234567])
def test_tridiag_dirichlet_solve(dev, ne):
    from hybrid_fem_lssvr_amd import ops
    nodes = np.linspace(-1, 1, ne + 1)
    kd, fl, fr = orc.p1_assemble_local(nodes)
    diag, off, load = orc.p1_scatter(kd, fl, fr)
    u = ops.tridiag_dirichlet_solve(_t(diag, dev), _t(off, dev), _t(load, dev), 0.25, -0.5).cpu().numpy()
    ref = orc.banded_dirichlet(diag, off, load, 0.25, -0.5)
    assert u[0] == 0.25 and u[-1] == -0.5
    scale = np.max(np.abs(ref))
    # Backward stability first: the residual is at rounding level of |A| |u| (normwise; a
    # row-wise bound is meaningless where u crosses zero).
    if ne > 1:
        r = diag[1:-1] * u[1:-1] + off[:-1] * u[:-2] + off[1:] * u[2:] - load[1:-1]
        assert np.max(np.abs(r)) <= 1e-13 * np.max(np.abs(diag)) * scale * max(1.0, np.log2(ne))
    # Forward agreement: the P1 Laplacian has cond ~ ne^2, so two backward-stable float64
    # solvers (LAPACK banded LU here; recursive substructuring on the device) differ by up to
    # ~cond*eps; LAPACK itself is 3e-13 (ne=1025) / 9e-11 (ne=1e5) from a long-double Thomas.
    # Pinned at ~5x what the device solver measured on an MI355X (scripts/measure_bars.py, round 2):
    # max|u - ref| = 1.6e-15 (24), 4.4e-13 (511), 6.6e-14 (512), 3.9e-13 (513), 3.0e-13 (514),
    # 6.5e-13 (1025), 3.8e-10 (16385), 1.4e-8 (1e5), 3.5e-7 (1234567).
    assert np.max(np.abs(u - ref)) <= TRIDIAG_FORWARD_BAR[ne] * scale


TRIDIAG_FORWARD_BAR = {1: 0.0, 2: 1e-15, 3: 1e-15, 24: 1e-14, 511: 2.5e-12, 512: 2.5e-12, 513: 2.5e-12,
                       514: 2.5e-12, 1025: 4e-12, 16385: 2e-9, 100000: 7e-8, 1234567: 2e-6}


@functools.lru_cache(maxsize=None)
def _buffer_case(ne, operator):
    """(single entry, its sizer's name, the bands in the entry's order), computed once and shared: do not write to
    the arrays.  "sym": the P1 Laplacian; "ns": -u'' + b u' + u with the cell Peclet number at 0.5."""
    from hybrid_fem_lssvr_amd import ops
    nodes = np.linspace(-1, 1, ne + 1)
    if operator == "sym":
        diag, off, load, _ = orc.p1_bands(nodes)
        return ops.tridiag_dirichlet_solve, "lssvr_tridiag_work_bytes", (diag, off, load)
    b = lambda x: 0.5 * ne + 0.0 * np.asarray(x, dtype=np.float64)          # noqa: E731  (|b| h / 2, h = 2 / ne)
    diag, sub, sup, load, _ = cr.conv_bands(nodes, orc.poisson_rhs, None, b, lambda x: 1.0 + 0.0 * x)
    return ops.tridiag_ns_dirichlet_solve, "lssvr_tridiag_ns_work_bytes", (diag, sub, sup, load)


# 514: one chunked level, a last chunk of one row; 4105: two chunked levels
@pytest.mark.parametrize("operator", ["sym", "ns"])
@pytest.mark.parametrize("ne", [514, 4105])
def test_tridiag_caller_buffers(dev, ne, operator):
    """Caller-supplied ``out`` and ``work``: ``work`` of exactly lssvr_tridiag_work_bytes(ne) /
    lssvr_tridiag_ns_work_bytes(ne) is enough -- 64 guard doubles behind it keep their sentinel -- and the result is
    bit-equal to the call that allocates both; an ``out`` of ne doubles is refused."""
    import torch
    from hybrid_fem_lssvr_amd import _capi
    solve, sizer, bands = _buffer_case(ne, operator)
    bands = [_t(b, dev) for b in bands]
    u_ref = solve(*bands, 0.25, -0.5)
    nbytes = getattr(_capi.load(), sizer)(ne)
    assert nbytes % 8 == 0
    sentinel = -7.25
    buf = torch.full((nbytes // 8 + 64,), sentinel, dtype=torch.float64, device=dev)
    out = torch.full((ne + 1,), sentinel, dtype=torch.float64, device=dev)
    u = solve(*bands, 0.25, -0.5, out=out, work=buf[:nbytes // 8])
    assert u is out
    assert torch.equal(buf[nbytes // 8:], torch.full((64,), sentinel, dtype=torch.float64, device=dev))
    assert torch.equal(out, u_ref)
    with pytest.raises(ValueError, match="out must hold"):
        solve(*bands, 0.25, -0.5, out=out[:ne])


@pytest.mark.parametrize("operator", ["sym", "ns"])
def test_tridiag_single_entry_in_a_graph(dev, operator):
    """A single-RHS call with ``out`` and ``work`` given is captured in a hipGraph (as ops.StepGraph captures: after
    a warm-up call, capture_error_mode="thread_local") and replayed once: the end values travel by value, so the
    entry does nothing a capture forbids (no allocation, copy or synchronisation), and the replay has the bits of
    the eager call with u[0], u[ne] exact.  ne = 4105: two chunked levels."""
    import torch
    from hybrid_fem_lssvr_amd import _capi
    ne = 4105
    solve, sizer, bands = _buffer_case(ne, operator)
    bands = [_t(b, dev) for b in bands]
    u_ref = solve(*bands, 0.25, -0.5)
    work = torch.empty(getattr(_capi.load(), sizer)(ne) // 8, dtype=torch.float64, device=dev)
    out = torch.empty(ne + 1, dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        solve(*bands, 0.25, -0.5, out=out, work=work)             # warm-up outside the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        solve(*bands, 0.25, -0.5, out=out, work=work)
    out.fill_(-7.25)
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(out, u_ref)
    assert out[0].item() == 0.25 and out[-1].item() == -0.5


@pytest.mark.parametrize("ne", [1, 2, 3, 24, 2047, 2048, 2049, 100000, 1234567, 10000000])
def test_p1_flux_solve(dev, ne):
    """Prefix-scan solve of the P1 system: residual at rounding level, and -- unlike any
    elimination -- a forward error that does not grow like cond(A) ~ ne^2 (checked against a
    long-double Thomas solve where that is affordable)."""
    from hybrid_fem_lssvr_amd import ops
    nodes = np.linspace(-1, 1, ne + 1)
    kd, fl, fr = orc.p1_assemble_local(nodes)
    diag, off, load = orc.p1_scatter(kd, fl, fr)
    u = ops.p1_flux_solve(_t(kd, dev), _t(load, dev), 0.25, -0.5).cpu().numpy()
    assert u[0] == 0.25 and u[-1] == -0.5
    # exact-structure reference: the same three sums in long double
    ld = np.longdouble
    k = kd.astype(ld)
    l = load.astype(ld).copy()
    l[0] = 0
    S = np.cumsum(l[:ne])
    R = np.cumsum(1 / k)
    T = np.cumsum(S / k)
    q0 = (ld(-0.5) - ld(0.25) + T[-1]) / R[-1]
    uref = np.concatenate([[ld(0.25)], ld(0.25) + q0 * R - T])
    assert float(np.max(np.abs(u[:-1] - uref[:-1]))) <= 4e-15 * max(1.0, np.log2(ne + 1))
    # Against LAPACK on the ASSEMBLED float64 bands the two differ by much more than either
    # solver's error: rounding diag = k_{i-1} + k_i (1e-16 relative) breaks the zero row sums of
    # D^T K D, i.e. adds a spurious reaction term, which moves the solution by ~ne^2 * eps
    # (2.5e-8 at ne = 1e5, measured in long double).
    ref = orc.banded_dirichlet(diag, off, load, 0.25, -0.5)
    assert np.max(np.abs(u - ref)) <= 5e-16 * max(ne, 10) ** 2 + 1e-13


def test_fem_nodal_error_matches_survey(dev):
    """Manufactured solution: P1 with the 2-point Gauss load has max nodal error 3.274e-6 on 24
    elements -- the pin for the scikit-fem part that cannot run here."""
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(25, lssvr_M=8, lssvr_gamma=1e4)
    u_flux, _ = pkg.FEMLSSVRPrimalSolver(25, lssvr_M=8, lssvr_gamma=1e4, fem_solver="flux").solve_fem()
    u_fem, basis = s.solve_fem()
    assert np.max(np.abs(u_fem - u_flux)) < 1e-14
    assert basis.N == 25 and basis.mesh.t.shape == (2, 24) and basis.mesh.p.shape == (1, 25)
    assert np.array_equal(basis.get_dofs(), [0, 24])
    err = np.max(np.abs(u_fem - np.sin(np.pi * s.fem_nodes)))
    assert abs(err - 3.274e-6) < 2e-9
    assert np.max(np.abs(u_fem - orc.fem_p1_solve(np.linspace(-1, 1, 25)))) < 1e-14


def test_eval_golden_indices_and_values(dev, golden):
    from hybrid_fem_lssvr_amd import ops
    g = golden("G7_eval_default")
    u, elem = ops.evaluate(_t(g["nodes"], dev), _t(g["W"], dev), _t(g["xq"], dev))
    u, elem = u.cpu().numpy(), elem.cpu().numpy()
    assert np.array_equal(elem, g["elem"])                 # indices: bit-exact
    assert np.array_equal(u, g["u_ref"])                   # numpy's legval order: bit-exact
    # NaN query: no branch of Dual.py:182-201 fires
    u2, e2 = ops.evaluate(_t(g["nodes"], dev), _t(g["W"], dev), _t(np.array([np.nan, 0.1]), dev))
    assert e2.cpu().numpy()[0] == -1 and u2.cpu().numpy()[0] == 0.0


@pytest.mark.parametrize("M", [1, 2, 3, 9, 33])
def test_eval_nonuniform_mesh(dev, M):
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(M)
    ne = 5000
    nodes = np.cumsum(np.concatenate([[3.0], rng.uniform(1e-4, 1.0, ne)]))
    W = rng.standard_normal((ne, M))
    xq = np.concatenate([rng.uniform(nodes[0] - 1, nodes[-1] + 1, 20000), nodes,
                         np.nextafter(nodes, np.inf), np.nextafter(nodes, -np.inf)])
    u, elem = ops.evaluate(_t(nodes, dev), _t(W, dev), _t(xq, dev))
    uo, eo = orc.evaluate_solution_vec(nodes, W, xq)
    assert np.array_equal(elem.cpu().numpy(), eo)
    assert np.array_equal(u.cpu().numpy(), uo)
    # the O(P*ne) scan of the reference on a subsample
    sub = slice(0, 300)
    assert np.array_equal(eo[sub], orc.locate_elements_scan(nodes, xq[sub]))


def test_eval_full_size(dev):
    """1e6 elements, 2e6 query points: indices exact against searchsorted, values against
    the vectorised numpy restatement."""
    from hybrid_fem_lssvr_amd import ops
    ne, M = 1000000, 9
    nodes = np.linspace(-1, 1, ne + 1)
    rng = np.random.default_rng(3)
    W = rng.standard_normal((ne, M))
    xq = np.concatenate([np.linspace(-1.001, 1.001, 1000001), nodes[::2][:999999]])
    u, elem = ops.evaluate(_t(nodes, dev), _t(W, dev), _t(xq, dev))
    uo, eo = orc.evaluate_solution_vec(nodes, W, xq)
    assert np.array_equal(elem.cpu().numpy(), eo)
    assert np.array_equal(u.cpu().numpy(), uo)


def test_varcoef_config5(dev):
    """-(a u')' = f with a smooth random a(x): no reference
    oracle exists (Dual.py:44 hard-codes -u''), so the pin is the extended-precision
    minimiser of the same QP and the manufactured solution."""
    from hybrid_fem_lssvr_amd import ops
    c, phi = orc.varcoef_params()
    a, da, f = orc.varcoef_functions(c, phi)
    for ne, M, n in ((2000, 9, 16), (300, 20, 32), (100, 26, 40)):      # lane, lane (AGPR), wave
        nodes = np.linspace(-1, 1, ne + 1)
        values = orc.fem_p1_solve(nodes, rhs=f, coef_a=a)
        x = _t(nodes, dev)
        xc = ops.colloc_points(x, n).cpu().numpy()
        W, st = ops.enhance_varcoef(x, _t(values, dev), M, 1e4, n, _t(a(xc), dev), _t(da(xc), dev),
                                    _t(f(xc), dev), global_domain=(-1.0, 1.0))
        W, st = W.cpu().numpy(), st.cpu().numpy()
        assert np.all(st == 0)
        Wo = orc.enhance_all_vec(nodes, values, M, 1e4, n, rhs=f, coef_a=a, coef_da=da)
        assert orc.rel_l2_coef(W, Wo).max() <= 1e-11
        if cf.HAVE_MP:
            sel = [0, ne // 3, ne - 1]
            tr = cf.truth_all(nodes, values, M, 1e4, n, f, (-1.0, 1.0), sel, coef_a=a, coef_da=da)
            assert orc.rel_l2_coef(W[sel], tr).max() <= 1e-13
        xq = np.linspace(-1, 1, 4001)
        uq, _ = orc.evaluate_solution_vec(nodes, W, xq)
        uo, _ = orc.evaluate_solution_vec(nodes, Wo, xq)
        p1 = np.interp(xq, nodes, values)
        ex = np.sin(np.pi * xq)
        # manufactured solution: same L2 error as the CPU restatement, and below plain P1
        assert abs(np.linalg.norm(uq - ex) - np.linalg.norm(uo - ex)) <= 1e-10 * np.linalg.norm(ex)
        # measured (scripts/measure_bars.py): the enhancement's error is 1/1.90 .. 1/1.91 of P1's
        # at all three sizes (the nodal error of the P1 solve dominates both)
        assert np.linalg.norm(uq - ex) < np.linalg.norm(p1 - ex) / 1.7


# Variable-coefficient rows where the collocation matrix is (near) square: n in [M-2, M+12].  The Poisson kernels
# refine there (corrected semi-normal equations on polynomial rows); weighted rows have no such form, and float64
# itself loses the digits: a float64 KKT solve and the float64 BC-eliminated solve of the SAME element read
# 5.7e-6 / 3.3e-6 at (33, 31), 2e-10 at (33, 33), 5e-12 at (26, 24) against the 60-digit minimiser (h = 1/12; CPU study
# of round 4).  What the kernels owe there is the float64 problem's own accuracy: the bar is 10 x the worse of the two
# float64 oracles (floor 1e-13), per case, measured next to it.
VC_NEAR_SQUARE = [(12, 10), (16, 14), (20, 18), (20, 20), (22, 20), (22, 22),            # lane kernel (direct Gram)
                  (26, 24), (26, 26), (33, 31), (33, 33), (33, 36), (33, 40), (33, 45)]   # f64-MFMA kernel


@pytest.mark.parametrize("h", [1.0 / 12, 0.5])
@pytest.mark.parametrize("M,n", VC_NEAR_SQUARE)
def test_varcoef_near_square_holds_float64_accuracy(dev, note, M, n, h):
    from hybrid_fem_lssvr_amd import ops
    if not cf.HAVE_MP:
        pytest.skip("mpmath not importable")
    c, phi = orc.varcoef_params()
    a, da, f = orc.varcoef_functions(c, phi)
    ne = 130                                                   # three waves of the lane kernel, 65 pairs of the other
    nodes = -1.0 + h * np.arange(ne + 1)
    values = np.sin(np.pi * nodes)
    x = _t(nodes, dev)
    xc = ops.colloc_points(x, n).cpu().numpy()
    W, st = ops.enhance_varcoef(x, _t(values, dev), M, 1e4, n, _t(a(xc), dev), _t(da(xc), dev), _t(f(xc), dev),
                                global_domain=(nodes[0], nodes[-1]))
    W, st = W.cpu().numpy(), st.cpu().numpy()
    assert np.all(st == 0)
    sel = [1, 64, 127]
    tr = cf.truth_all(nodes, values, M, 1e4, n, f, (nodes[0], nodes[-1]), sel, coef_a=a, coef_da=da)
    f64 = 0.0
    for k, i in enumerate(sel):
        gl, gr = orc.boundary_values(i, ne, nodes[i], nodes[i + 1], values[i], values[i + 1], (nodes[0], nodes[-1]))
        s = orc.element_system(nodes[i], nodes[i + 1], gl, gr, M, 1e4, n, f, a, da)
        for solve in (orc.solve_primal_kkt, orc.solve_bc_eliminated):
            f64 = max(f64, float(orc.rel_l2_coef(solve(s), tr[k])))
    err = float(orc.rel_l2_coef(W[sel], tr).max())
    bar = max(10.0 * f64, 1e-13)
    note("varcoef near-square M=%d n=%d h=%.3g vs 60-digit minimiser (float64 oracles: %.1e)" % (M, n, h, f64), err, bar)
    assert err <= bar


def test_facade_reference_demo(dev, golden):
    """The reference's __main__ (Dual.py:206-217): 25 nodes, M=8, gamma=1e4, 201 points."""
    import hybrid_fem_lssvr_amd as pkg
    g = golden("G2_default_ne24_M8_n12")
    solver = pkg.FEMLSSVRPrimalSolver(25, lssvr_M=8, lssvr_gamma=1e4, global_domain=(-1, 1))
    solver.solve()
    assert len(solver.lssvr_functions) == 24
    f0 = solver.lssvr_functions[0]
    assert tuple(f0.domain) == (solver.fem_nodes[0], solver.fem_nodes[1]) and len(f0.coef) == 8
    W = np.array([f.coef for f in solver.lssvr_functions])
    assert orc.rel_l2_coef(W, g["coef_truth"]).max() <= 1e-12     # nodal values differ by ~3e-16
    assert orc.rel_l2_coef(W, g["coef_ref"]).max() <= 1e-10
    test_points = np.linspace(-1, 1, 201)
    computed = solver.evaluate_solution(test_points)
    exact = pkg.true_solution(test_points)
    rel = np.linalg.norm(computed - exact) / np.linalg.norm(exact)
    assert abs(rel - 3.255e-6) < 5e-9
    # user-assigned nodal values are authoritative (Dual.py:139 reads only the attributes)
    solver.fem_values = g["values_sel"][:, 0].tolist() + [g["values_sel"][-1, 1]]
    solver.solve_lssvr_subproblems()
    W = np.array([f.coef for f in solver.lssvr_functions])
    assert orc.rel_l2_coef(W, g["coef_truth"]).max() <= 1e-13


def test_lssvr_primal_function(dev, golden):
    """Single-element entry with the reference's signature and boundary-flag semantics
    (Dual.py:20-22, 65-75)."""
    import hybrid_fem_lssvr_amd as pkg
    g = golden("G1_c1_ne8_M5_n5")
    for k in (0, 3, 7):
        a, b = g["nodes_sel"][k]
        ul, ur = g["values_sel"][k]
        fn = pkg.lssvr_primal(pkg.poisson_rhs, [a, b], ul, ur, 5, 1e4, is_left_boundary=(k == 0),
                              is_right_boundary=(k == 7), global_domain_range=(-1, 1), n_colloc=5)
        assert orc.rel_l2_coef(fn.coef, g["coef_truth"][k]) <= 1e-13
        assert orc.rel_l2_coef(fn.coef, g["coef_ref"][k]) <= 3e-10
        assert tuple(fn.domain) == (a, b)
    # a flag without the matching end point keeps the nodal value (Dual.py:65: `and xmin == global_xmin`)
    fn = pkg.lssvr_primal(pkg.poisson_rhs, [-0.5, 0.0], 0.7, 0.1, 6, 1e4, is_left_boundary=True,
                          global_domain_range=(-1, 1))
    assert abs(fn(-0.5) - 0.7) < 1e-13
    # an arbitrary Python callable as rhs_func goes through host tabulation
    fn2 = pkg.lssvr_primal(lambda x: np.pi ** 2 * np.sin(np.pi * x), [-0.5, 0.0], 0.7, 0.1, 6, 1e4,
                           is_left_boundary=True, global_domain_range=(-1, 1))
    assert orc.rel_l2_coef(fn2.coef, fn.coef) <= 1e-14


def test_capi_argument_errors(dev):
    """<0 return + message for bad arguments, no launch."""
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    x = torch.linspace(0, 1, 11, dtype=torch.float64, device=dev)
    with pytest.raises(_capi.LssvrHipError, match="M = 40"):
        ops.enhance(x, x, 40, 1e4, 12, global_domain=(0.0, 1.0))
    with pytest.raises(_capi.LssvrHipError, match="n_colloc"):
        ops.enhance(x, x, 5, 1e4, 1, global_domain=(0.0, 1.0))
    with pytest.raises(_capi.LssvrHipError, match="gamma"):
        ops.enhance(x, x, 5, -1.0, 12, global_domain=(0.0, 1.0))
    with pytest.raises(RuntimeError, match="device memory"):
        ops.enhance(x.cpu(), x.cpu(), 5, 1e4, 12, global_domain=(0.0, 1.0))
    with pytest.raises(_capi.LssvrHipError, match="nquad"):
        ops.p1_assemble(x, 9)


def test_fused_step_equals_separate_launches(dev):
    """lssvr_step (assembly + enhancement in one grid) == the two stand-alone kernels, bit for
    bit, including the shard offsets; the profiled entry returns the same W and a duration."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    ne, M, n = 5003, 9, 16
    nodes = np.linspace(-3.0, 2.0, ne + 1)
    x, u = _t(nodes, dev), _t(np.sin(np.pi * nodes), dev)
    for off, neg in ((0, ne), (7, ne + 20)):
        plan = ops.StepPlan(x, u, M, 1e4, n, elem_offset=off, ne_global=neg, global_domain=(-3.0, 2.0))
        W, st = plan.launch()
        torch.cuda.synchronize()
        W2, st2 = ops.enhance(x, u, M, 1e4, n, elem_offset=off, ne_global=neg, global_domain=(-3.0, 2.0))
        b2 = ops.p1_assemble(x, 2)
        assert torch.equal(W, W2) and torch.equal(st, st2)
        for k in ("diag", "off", "load"):
            assert torch.equal(plan.bands[k], b2[k]), k
    W3 = torch.empty_like(W2)
    dt = ops.enhance_profiled(x, u, M, 1e4, n, elem_offset=7, ne_global=ne + 20,
                              global_domain=(-3.0, 2.0), out=W3)
    assert torch.equal(W3, W2) and 1e-7 < dt < 1e-2
    # lssvr_enhance_ws_sequence: k stamped launches back to back, one synchronisation; same result
    W3.zero_()
    dts = ops.enhance_profiled(x, u, M, 1e4, n, elem_offset=7, ne_global=ne + 20,
                               global_domain=(-3.0, 2.0), out=W3, repeats=5)
    assert len(dts) == 5 and all(1e-7 < t < 1e-2 for t in dts) and torch.equal(W3, W2)
    from hybrid_fem_lssvr_amd import _capi
    with pytest.raises(_capi.LssvrHipError):
        ops.enhance_profiled(x, u, M, 1e4, n, global_domain=(-3.0, 2.0), out=W3, repeats=0)


def test_varcoef_config5_full_size(dev, note):
    """BASELINE config 5 at its full size (1e6 elements, degree 8, 16 points, random smooth a(x)):
    boundary rows on every element, a sample against the batched oracle and the 60-digit
    minimiser -- the whole polynomial and the enhancement relative to its own norm
    (oracle.rel_l2_bubble; the bubble is 1.3e-12 of the polynomial here, below the 1e-11 bar of
    the whole-polynomial check) -- and every element's leading bubble coefficient against its
    asymptotic value.  No reference counterpart exists for this
    configuration (Dual.py:44)."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    c, phi = orc.varcoef_params()
    a, da, f = orc.varcoef_functions(c, phi)
    ne, M, n = 1000000, 9, 16
    nodes = np.linspace(-1, 1, ne + 1)
    values = np.sin(np.pi * nodes)
    values[0] = values[-1] = 0.0
    x = _t(nodes, dev)
    xc = ops.colloc_points(x, n).cpu().numpy()
    W, st = ops.enhance_varcoef(x, _t(values, dev), M, 1e4, n, _t(a(xc), dev), _t(da(xc), dev),
                                _t(f(xc), dev), global_domain=(-1.0, 1.0))
    assert int(st.sum().item()) == 0
    W = W.cpu().numpy()
    sgn = (-1.0) ** np.arange(M)
    assert np.max(np.abs(W @ sgn - values[:-1])) < 1e-12
    assert np.max(np.abs(W.sum(1) - values[1:])) < 1e-12
    # The bubble's own conditioning: the right-hand side of the eliminated system is
    # phi_k = -(f_k / scl^2 + (a'_k / scl) d_1), d_1 = (g_r - g_l) / 2 -- the a' u' part of f cancels
    # against the slope of the linear part and leaves a u''.  Where u'' -> 0 (the elements next to
    # x = -1, 0, 1 for u = sin(pi x)) the two terms are 1.5e4 times larger than their sum, so one ulp
    # in the tabulated f moves the EXACT minimiser's bubble by 1.7e-12 of itself (measured with the
    # 60-digit solve: oracle probe in DESIGN.md section 6).  kappa_e = max_k (|f~| + |b d_1|) / max_k |phi|
    # is that amplification; the bubble is held to 2e-15 kappa_e (minimiser) / 2e-14 kappa_e (oracle) --
    # ~10x what was measured -- i.e. to the plain bar wherever the bubble is not a difference of larger numbers.
    def kappa(s0, s1):
        el = np.arange(s0, s1)
        aa, bb = nodes[el], nodes[el + 1]
        hh = bb - aa
        xk = aa[:, None] + (hh / (n - 1))[:, None] * np.arange(n)[None, :]
        scl = 2.0 / hh
        gl, gr = values[el].copy(), values[el + 1].copy()
        ft = f(xk) / (scl * scl)[:, None]
        bd = (da(xk) / scl[:, None]) * (0.5 * (gr - gl))[:, None]
        return (np.abs(ft) + np.abs(bd)).max(1) / np.abs(ft + bd).max(1)

    worst = 0.0
    for s0 in (0, 600000, ne - 5000):
        Wo = orc.enhance_all_vec(nodes[s0:s0 + 5001], values[s0:s0 + 5001], M, 1e4, n, rhs=f,
                                 coef_a=a, coef_da=da, global_domain=(-1.0, 1.0))
        assert orc.rel_l2_coef(W[s0:s0 + 5000], Wo).max() <= 1e-11
        worst = max(worst, (orc.rel_l2_bubble(W[s0:s0 + 5000], Wo) / kappa(s0, s0 + 5000)).max())
    note("config 5 bubble / kappa vs batched oracle, 1.5e4 elements", worst, 2e-14)
    assert worst <= 2e-14, worst                # measured 1.3e-15
    # every element: the rows enforce -a u'' - a' u' = f, i.e. u'' = -(f + a' u') / a with u' the
    # slope of the nodal values to leading order -- for the manufactured u = sin(pi x) that is
    # u'' = -pi^2 sin(pi x) whatever a is: bubble = -(u''/2)(x-a)(b-x), w_2 = -(2/3)(pi^2 h^2 / 8) sin(pi x_mid)
    xm = 0.5 * (nodes[:-1] + nodes[1:])
    lead = -(2.0 / 3.0) * (np.pi ** 2 / 8.0) * (2.0 / ne) ** 2 * np.sin(np.pi * xm)
    big = np.abs(np.sin(np.pi * xm)) > 1e-3
    dev_lead = np.max(np.abs(W[big, 2] / lead[big] - 1.0))
    note("config 5 max |w_2 / asymptote - 1| over all elements", dev_lead)
    assert dev_lead < 1e-4
    if cf.HAVE_MP:
        sel = [0, 333333, ne - 1]
        tr = cf.truth_all(nodes, values, M, 1e4, n, f, (-1.0, 1.0), sel, coef_a=a, coef_da=da)
        assert orc.rel_l2_coef(W[sel], tr).max() <= 1e-13
        bt = (orc.rel_l2_bubble(W[sel], tr) / np.array([kappa(i, i + 1)[0] for i in sel])).max()
        note("config 5 bubble / kappa vs 60-digit minimiser", bt, 2e-15)
        assert bt <= 2e-15, bt                  # measured 1.5e-16
        # ... and where the bubble is well conditioned (kappa < 10) the plain 1e-13 holds
        mid = [250000, 333333, 600000]
        trm = cf.truth_all(nodes, values, M, 1e4, n, f, (-1.0, 1.0), mid, coef_a=a, coef_da=da)
        assert max(kappa(i, i + 1)[0] for i in mid) < 10.0
        bm = orc.rel_l2_bubble(W[mid], trm).max()
        note("config 5 bubble vs 60-digit minimiser, well-conditioned elements", bm, 5e-15)
        assert bm <= 5e-15, bm                  # measured 6.4e-16


def test_step_is_hip_graph_capturable(dev):
    """include/lssvr_hip.h promises every call is asynchronous on the caller's stream and safe
    to capture: record the fused step + evaluation into a hipGraph, replay it on new nodal
    values, compare with eager launches."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    ne, M, n = 4096, 9, 16
    nodes = np.linspace(-1, 1, ne + 1)
    x = _t(nodes, dev)
    u = _t(np.sin(np.pi * nodes), dev)
    xq = _t(np.linspace(-1, 1, 1001), dev)
    plan = ops.StepPlan(x, u, M, 1e4, n, global_domain=(-1.0, 1.0))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        plan.launch()                      # warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.launch()
        uq_g, _ = ops.evaluate(x, plan.W, xq, want_elem=False)
    u.copy_(_t(np.cos(nodes), dev))        # new input, same buffers
    g.replay()
    torch.cuda.synchronize()
    W_g, uq_graph = plan.W.clone(), uq_g.clone()
    W_e, _ = ops.enhance(x, u, M, 1e4, n, global_domain=(-1.0, 1.0))
    uq_e, _ = ops.evaluate(x, W_e, xq, want_elem=False)
    assert torch.equal(W_g, W_e) and torch.equal(uq_graph, uq_e)


def test_step_graph_replays_equal_eager_steps(dev):
    """ops.StepGraph: K launches of a bound plan captured once; a replay after new nodal values were
    written in place gives what an eager launch gives."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    ne, M, n = 5000, 9, 16
    nodes = np.linspace(-2, 2, ne + 1)
    x = _t(nodes, dev)
    u = _t(np.sin(np.pi * nodes), dev)
    plan = ops.StepPlan(x, u, M, 1e4, n, global_domain=(-2.0, 2.0))
    g = ops.StepGraph(plan, steps=3)
    u.copy_(_t(np.cos(0.5 * nodes), dev))
    W, st = g.replay()
    torch.cuda.synchronize()
    W_g = W.clone()
    assert int(st.sum()) == 0
    W_e, _ = ops.enhance(x, u, M, 1e4, n, global_domain=(-2.0, 2.0))
    assert torch.equal(W_g, W_e)
    bands = {k: v.clone() for k, v in plan.bands.items()}
    plan.launch()
    torch.cuda.synchronize()
    assert all(torch.equal(bands[k], plan.bands[k]) for k in bands)


def test_c_abi_demo_program(dev):
    """examples/c_abi_demo.cpp drives the whole solve-then-enhance path through the C ABI alone
    (hipMalloc'd buffers, no Python, no torch) and checks the reference demo's error figures."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "examples", "c_abi_demo")
    if not os.path.exists(exe):
        pytest.fail("examples/c_abi_demo missing: run __graft_entry__.build()")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "OK" in r.stdout


def test_eval_error_norms_on_device(dev):
    """lssvr_eval_error: L2 / max error against sin(pi x) reduced on the device == the host
    computation of Dual.py:216-217 on the same points (reference demo: rel-L2 3.255e-06)."""
    import torch
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    s = pkg.FEMLSSVRPrimalSolver(25, lssvr_M=8, lssvr_gamma=1e4)
    s.solve()
    xq_h = np.concatenate([np.linspace(-1, 1, 201), [np.nan]])
    xq = _t(xq_h, dev)
    out = ops.eval_error(s.enhanced.nodes, s.enhanced.W, xq).cpu().numpy()
    u = s.evaluate_solution(xq_h[:-1])
    ex = np.sin(np.pi * xq_h[:-1])
    # (u - ex) ~ 3e-6 while ex itself carries ~1e-16 of sin rounding: 1e-10 relative on the sum
    assert abs(out[0] - np.sum((u - ex) ** 2)) <= 1e-9 * np.sum((u - ex) ** 2)
    assert abs(out[1] - np.sum(ex ** 2)) <= 1e-13 * np.sum(ex ** 2)
    assert abs(out[2] - np.max(np.abs(u - ex))) <= 1e-15 + 1e-9 * out[2]
    assert abs(np.sqrt(out[0] / out[1]) - 3.255e-6) < 5e-9
    # accumulation across calls (shards): second call adds to the same buffer
    acc = torch.zeros(3, dtype=torch.float64, device=dev)
    ops.eval_error(s.enhanced.nodes, s.enhanced.W, xq[:100].contiguous(), out=acc)
    ops.eval_error(s.enhanced.nodes, s.enhanced.W, xq[100:].contiguous(), out=acc)
    assert np.allclose(acc.cpu().numpy(), out, rtol=1e-12, atol=0)


@pytest.mark.parametrize("M,n", [(9, 16), (22, 44), (33, 64)])
def test_facade_callable_rhs_is_tabulated_in_the_kernels_layout(dev, M, n):
    """An arbitrary ``rhs_func`` (Dual.py:20, 157) reaches the kernels as a table at np.linspace's points:
    point-major for the lane kernels (M <= 22), element-major above -- same values, so the result equals the
    named in-kernel f to rounding and (M <= 22) the element-major call bit for bit."""
    import torch
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    ne = 333
    nodes = np.linspace(-1, 1, ne + 1)
    values = orc.fem_p1_solve(nodes)
    named = pkg.enhance_elements(nodes, values, M, 1e4, n_colloc=n)
    tabd = pkg.enhance_elements(nodes, values, M, 1e4, n_colloc=n, rhs=lambda x: np.pi ** 2 * np.sin(np.pi * x))
    assert named.n_fallback == 0 and tabd.n_fallback == 0
    assert orc.rel_l2_coef(tabd.W.cpu().numpy(), named.W.cpu().numpy()).max() <= 1e-13
    x, u = _t(nodes, dev), _t(values, dev)
    f_em = _t(orc.poisson_rhs(ops.colloc_points(x, n).cpu().numpy()), dev)
    W_em, _ = ops.enhance(x, u, M, 1e4, n, global_domain=(-1.0, 1.0), rhs_values=f_em)
    torch.cuda.synchronize()
    assert torch.equal(W_em, tabd.W)


@pytest.mark.parametrize("M,n", [(9, 16), (22, 16), (33, 64)])
def test_facade_callable_rhs_sees_points_on_the_last_axis(dev, M, n):
    """the reference hands ``rhs_func`` the 1-D array of ONE element's n points (Dual.py:40-44), so a
    callable may return a per-point vector of shape (n,) or otherwise rely on the last axis being the points.
    The facade evaluates it on the element-major ``x[e, k]`` at every degree (and transposes the TABLE for the
    lane kernels): a constant-in-e, varying-in-k right-hand side broadcasts the same below and above M = 22 --
    also on a mesh with ne == n, where a transposed evaluation would go unnoticed by the shape check."""
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    profile = np.cos(np.arange(n) * 0.37) + 2.0                       # f_k: depends on the POINT index only

    def per_point(x):
        assert x.shape[-1] == n                                       # points along the last axis, always
        return profile                                                # shape (n,): broadcasts over elements

    for ne in (n, 40):
        nodes = np.linspace(-1, 1, ne + 1)
        values = orc.fem_p1_solve(nodes)
        got = pkg.enhance_elements(nodes, values, M, 1e4, n_colloc=n, rhs=per_point)
        x, u = _t(nodes, dev), _t(values, dev)
        table = _t(np.broadcast_to(profile, (ne, n)).copy(), dev)     # element-major [ne, n]
        want, st = ops.enhance(x, u, M, 1e4, n, global_domain=(-1.0, 1.0), rhs_values=table)
        assert got.n_fallback == 0 and int(st.sum()) == 0
        assert orc.rel_l2_coef(got.W.cpu().numpy(), want.cpu().numpy()).max() <= 1e-14
