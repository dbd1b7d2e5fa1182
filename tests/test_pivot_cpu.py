"""CPU: the pivoting tridiagonal solve as far as it goes without a GPU -- the reference of
tests/pivot_rules.py, the facts that make the resonant Helmholtz case a fair one, the facade's host logic and the
C ABI."""
import os
import re

import numpy as np
import pytest

import convection_rules as cr
import pivot_rules as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssvr_hip.h")
NAMES = ("lssvr_tridiag_pivot_work_bytes", "lssvr_tridiag_pivot_solve_multi", "lssvr_tridiag_pivot_solve_host")


@pytest.mark.parametrize("ne", [65, 4097])
def test_reference_pinned_to_long_double_thomas(ne):
    """refined_ld against thomas_ns_ld on the dominant control (Peclet 0.5, c = 1), where the unpivoted long-double
    elimination is safe.  Allowed distance: rounding level of long double x condition number x max|u|, with
    2^-64 for the rounding level, ||A||_inf ||A^-1 1||_inf for the condition number (the matrix is an M-matrix:
    A^-1 >= 0, so ||A^-1||_inf = ||A^-1 1||_inf) and a factor 16 for the two solutions' independent errors.
    Observed: 6.0e-18 at 65 elements (bar 1.0e-16), 3.7e-17 at 4097 (bar 7.1e-15)."""
    from scipy.linalg import solve_banded
    bands, u_ld, _ = cr.peclet_case(ne, 0.5, "pos")
    u_ref, _ = pr.refined_ld(bands)
    _, ab, _ = pr.system(bands, pr.ENDS_D)
    norm = np.max(np.abs(ab[1]) + np.abs(np.r_[ab[0, 1:], 0.0]) + np.abs(np.r_[0.0, ab[2, :-1]]))
    cond = norm * np.max(np.abs(solve_banded((1, 1), ab, np.ones(ab.shape[1]))))
    bar = 16.0 * 2.0 ** -64 * cond * float(np.max(np.abs(u_ld)))
    dist = float(np.max(np.abs(u_ref - u_ld)))
    print(f"ne={ne}: |refined_ld - thomas_ld| = {dist:.2e}, cond = {cond:.3g}, bar {bar:.2e}")
    assert dist <= bar


@pytest.mark.parametrize("ne", [11, 19, 67, 515])
def test_resonant_case_is_fair(ne):
    """k h = 0.3952 (L = 8, j = 1): the 7 x 7 interior block of a length-8 chunk of the unpivoted solver is singular to
    working precision, the global matrix is harmless, and LAPACK's pivoting LU solves it to rounding level."""
    bands = pr.helmholtz(ne, 8)
    A = pr.dense(bands)
    u_ref, u_la = pr.refined_ld(bands)
    assert abs(np.sqrt(pr.helmholtz_k2(ne, 8)) * 2.0 / ne - 0.3952) < 1e-4
    assert np.linalg.cond(A[:7, :7]) >= 1e15
    assert np.linalg.cond(A) <= 1e4
    assert float(np.max(np.abs(u_la - u_ref))) <= 1e-13


def test_zero_diagonal_parity():
    """The hand-made zero-diagonal system is well conditioned for an even number of unknowns and exactly singular for an
    odd one."""
    for m, cond in ((2, 1.0), (8, 5.4), (14, 9.4), (64, 41.0), (512, 327.0)):
        assert abs(np.linalg.cond(pr.dense(pr.zero_diagonal(m))) / cond - 1.0) < 0.02
    for m in (7, pr.B + 1):
        assert np.linalg.matrix_rank(pr.dense(pr.zero_diagonal(m))) == m - 1


def _solver(**kw):
    import hybrid_fem_lssvr_amd as pkg
    return pkg.FEMLSSVRPrimalSolver(12, lssvr_M=9, n_colloc=16, **kw)


def test_facade_host_logic():
    """``"bands"`` keeps its refusals, ``"pivot"`` is constructed with the same problems; periodic ends and an unknown
    name are refused at construction."""
    import hybrid_fem_lssvr_amd as pkg
    neg = lambda x: -3.0 + 0.0 * x                                               # noqa: E731
    fast = lambda x: 5.0 * 11 + 0.0 * x                                          # noqa: E731  (h = 2/11: Peclet 5)
    assert _solver(fem_solver="pivot", reaction=neg, convection=fast).fem_solver == "pivot"
    assert _solver(fem_solver="pivot", reaction=neg, boundary=(("robin", 0.5, 1.0), None), element_lists=True)
    with pytest.raises(ValueError, match="boundary='periodic' needs fem_solver='bands'"):
        _solver(fem_solver="pivot", reaction=lambda x: 1.0 + 0.0 * x, boundary="periodic")
    with pytest.raises(ValueError, match="'bands', 'flux' or 'pivot'"):
        _solver(fem_solver="thomas")
    # two Neumann ends: still refused before anything is launched, with the word for this solver
    s = _solver(fem_solver="pivot", boundary=(("neumann", 0.0), ("neumann", 0.0)))
    with pytest.raises(ValueError, match="singular problem: .* nonzero at a quadrature point"):
        s._check_boundary(s._default_mesh())
    s = _solver(boundary=(("neumann", 0.0), ("neumann", 0.0)))
    with pytest.raises(ValueError, match="singular problem: .* positive at a quadrature point"):
        s._check_boundary(s._default_mesh())
    s = _solver(fem_solver="pivot", reaction=neg, boundary=(("neumann", 0.0), ("neumann", 0.0)))
    s._check_boundary(s._default_mesh())
    # the inflow end check belongs to the unpivoted solve alone
    weak = dict(convection=lambda x: 1.0 + 0.0 * x, boundary=(("neumann", 0.0), None))
    with pytest.raises(ValueError, match="kappa \\+ b n / 2"):
        s = _solver(**weak)
        s._check_boundary(s._default_mesh())
    s = _solver(fem_solver="pivot", **weak)
    s._check_boundary(s._default_mesh())
    assert pkg.FEMLSSVRPrimalSolver(5).fem_solver == "bands"


def _host_solve(bands, ends, loads=None):
    """lssvr_tridiag_pivot_solve_host: the kernels' own partition routines, level by level, on host arrays."""
    import ctypes
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    diag, sub, sup, load = (np.ascontiguousarray(b, dtype=np.float64) for b in bands)
    kinds, kappa, values = ends
    load = load if loads is None else np.ascontiguousarray(loads, dtype=np.float64)
    nc = 1 if load.ndim == 1 else load.shape[0]
    ev = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float64), (nc, 2)))
    u = np.full((nc, len(diag)), np.nan)
    info = np.full(1, -1, dtype=np.int32)
    rc = lib.lssvr_tridiag_pivot_solve_host(diag.ctypes.data, sub.ctypes.data, sup.ctypes.data, load.ctypes.data,
                                            kinds[0], kinds[1], ev.ctypes.data, (ctypes.c_double * 2)(*kappa),
                                            len(sub), nc, u.ctypes.data, info.ctypes.data)
    assert rc == 0
    return (u[0] if load.ndim == 1 else u), int(info[0])


def _host_check(tag, bands, ends):
    u_ref, u_la = pr.refined_ld(bands, ends)
    fwd_bar, res_bar, lapack, la_res = pr.bars(bands, ends, u_ref, u_la)
    u, info = _host_solve(bands, ends)
    fwd = float(np.max(np.abs(u.astype(np.longdouble) - u_ref)))
    res = pr.residual(bands, ends, u)
    print(f"{tag}: forward {fwd:.2e} (LAPACK {lapack:.2e}, bar {fwd_bar:.2e}), residual {res:.2e} (LAPACK {la_res:.2e}, "
          f"bar {res_bar:.2e}), info {info}")
    assert info == 0 and np.all(np.isfinite(u))
    assert fwd <= fwd_bar, (tag, fwd, fwd_bar)
    assert res <= res_bar, (tag, res, res_bar)


# wavenumbers resonant for runs of L elements (j-th eigenvalue): a run of L elements has L - 1 interior nodes, so some
# partition's inner block, at the first level or at a reduced one, is singular or close to it for many of these
RESONANT = [(3, 1), (4, 1), (5, 1), (6, 1), (6, 2), (7, 1), (8, 1), (9, 3), (11, 1), (11, 2), (11, 3), (13, 2)]


@pytest.mark.parametrize("L,j", RESONANT)
def test_host_routines_on_resonant_sweep(L, j):
    """The kernels' partition routines on the host, every level, against refined_ld with the bars of the GPU test, over
    a sweep of resonant wavenumbers and sizes from one level to five, with Dirichlet ends and with one free end of
    negative kappa."""
    for ne in (9, 19, 67, 131, 515, 1031, 4099, 20011, 50003, 100003):
        if ne % L == 0:
            ne += 1
        k2 = pr.resonant_k2(2.0 / ne, L, j)
        nodes = np.linspace(-1.0, 1.0, ne + 1)
        bands = pr.conv_bands(nodes, pr.orc.poisson_rhs, None, None,
                              lambda x: -k2 + 0.0 * np.asarray(x, dtype=np.float64))[:4]
        _host_check(f"L={L} j={j} ne={ne}", bands, pr.ENDS_D)
        if ne <= 4099 or ne == 100003:
            _host_check(f"L={L} j={j} ne={ne} free right end", bands,
                        ((pr.DIRICHLET, pr.ROBIN), (0.0, -0.5), (0.25, 0.3)))


@pytest.mark.parametrize("name", [p[0] for p in pr.PROBLEMS])
def test_host_routines_on_the_problems(name):
    """Problems 1 to 6 at every size of the GPU test, through the host entry."""
    for m in pr.sizes(name):
        bands, ends, _, _ = pr.case(name, m)
        _host_check(f"{name} m={m}", bands, ends)


def test_host_routines_singular_and_several_cases():
    """info > 0 for the exactly singular zero-diagonal systems, 0 for the even ones; nine cases in two passes have the
    bits of nine one-case calls."""
    for m in (7, pr.B + 1, 1001):
        u, info = _host_solve(pr.zero_diagonal(m), pr.ENDS_D)
        assert info > 0 and np.all(np.isfinite(u))
        assert _host_solve(pr.zero_diagonal(m + 1), pr.ENDS_D)[1] == 0
    bands = pr.turning(5003)
    rng = np.random.default_rng(5)
    loads = np.stack([bands[3] * (1.0 + 0.1 * q) + 0.01 * rng.standard_normal(5004) for q in range(9)])
    ends = ((pr.ROBIN, pr.DIRICHLET), (-0.5, 0.0), (0.3, -0.5))
    U, info = _host_solve(bands, ends, loads)
    assert info == 0
    for q in range(9):
        assert np.array_equal(U[q], _host_solve((bands[0], bands[1], bands[2], loads[q]), ends)[0]), q


def test_abi():
    """The symbols are exported, declared and bound, the ABI is still 7, and the workspace size is host arithmetic
    that grows with ne and with nc up to the eight cases of a pass."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for nm in NAMES:
        assert hasattr(lib, nm) and nm in _capi.SIGNATURES and re.search(r"\b%s\s*\(" % nm, hdr), nm
    assert lib.lssvr_version() == 7 and _capi.ABI_VERSION == 7
    wb = lib.lssvr_tridiag_pivot_work_bytes
    sizes = [1, 2, 7, 8, 9, 127, 128, 129, 513, 1000, 4097, 100003, 10 ** 6, 10 ** 7]
    for nc in (1, 3, 8, 9):
        w = [wb(ne, nc) for ne in sizes]
        assert all(a <= b for a, b in zip(w, w[1:])) and w[0] > 0, (nc, w)
    for ne in sizes:
        w = [wb(ne, nc) for nc in (1, 2, 3, 8, 9, 20)]
        assert all(a <= b for a, b in zip(w, w[1:])) and w[3] == w[4] == w[5], (ne, w)
    assert wb(10 ** 6, 1) > 8 * 5 * 10 ** 6 // 4                              # LO, D, UP, R, X of the first level


def test_argument_errors_without_gpu():
    import ctypes
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    f = [0x10000 * (i + 1) for i in range(8)]
    kap = (ctypes.c_double * 2)(-0.5, 0.0)

    def call(diag=f[0], sub=f[1], sup=f[2], load=f[3], kl=1, kr=0, ne=10, nc=1, u=f[4], work=f[5], wb=1 << 20,
             kappa=kap):
        return lib.lssvr_tridiag_pivot_solve_multi(diag, sub, sup, load, kl, kr, None, kappa, ne, nc, u, None, work, wb,
                                                   None)
    assert call(ne=0) == -2 and call(nc=0) == -2
    assert call(sup=None) == -1 and call(u=None) == -1 and call(kappa=None) == -1
    assert call(kl=2) == -2
    assert call(kappa=(ctypes.c_double * 2)(float("inf"), 0.0)) == -2 and b"finite" in lib.lssvr_last_error()
    assert call(wb=8) == -2 and b"lssvr_tridiag_pivot_work_bytes" in lib.lssvr_last_error()
    # each NULL, the words of each message, and the order of the checks: ne, nc, NULL, end kinds, work_bytes
    for nm in ("diag", "sub", "sup", "load", "u", "work"):
        assert call(**{nm: None}) == -1, nm
        assert b"diag, sub, sup, load, u, work must be non-NULL" in lib.lssvr_last_error()
    assert call(ne=0, nc=0) == -2 and b"ne = 0 < 1" in lib.lssvr_last_error()
    assert call(nc=0, diag=None) == -2 and b"nc = 0 < 1" in lib.lssvr_last_error()
    assert call(diag=None, kl=2) == -1 and call(kl=2, wb=8) == -2 and b"end kinds" in lib.lssvr_last_error()
    assert call(kr=1, kappa=(ctypes.c_double * 2)(-0.5, float("nan"))) == -2 and b"kappa[1]" in lib.lssvr_last_error()
    need = lib.lssvr_tridiag_pivot_work_bytes(10, 1)
    assert call(wb=need - 1) == -2 and b"work holds %d bytes, lssvr_tridiag_pivot_work_bytes(10, 1) = %d" % (
        need - 1, need) in lib.lssvr_last_error()

    # the host entry: the same checks but for work, which it does not take
    def host(diag=f[0], sub=f[1], sup=f[2], load=f[3], kl=1, kr=0, ne=10, nc=1, u=f[4], kappa=kap):
        return lib.lssvr_tridiag_pivot_solve_host(diag, sub, sup, load, kl, kr, None, kappa, ne, nc, u, None)
    assert host(ne=0) == -2 and b"ne = 0 < 1" in lib.lssvr_last_error()
    assert host(nc=0, u=None) == -2 and b"nc = 0 < 1" in lib.lssvr_last_error()
    for nm in ("diag", "sub", "sup", "load", "u"):
        assert host(**{nm: None}) == -1, nm
        assert b"diag, sub, sup, load, u must be non-NULL" in lib.lssvr_last_error()
    assert host(u=None, kl=2) == -1 and host(kl=2) == -2 and b"end kinds" in lib.lssvr_last_error()
    assert host(kappa=None) == -1
    assert host(kappa=(ctypes.c_double * 2)(float("inf"), 0.0)) == -2 and b"finite" in lib.lssvr_last_error()
