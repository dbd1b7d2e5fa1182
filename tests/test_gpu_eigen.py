"""GPU: the eigenproblem kernels one by one against numpy, the device Ritz step and Sturm count against their host
mirrors, and FEMLSSVRPrimalSolver.solve_eigen end to end on the problems of tests/eigen_rules.py."""
import math

import numpy as np
import pytest

import eigen_rules as er

pytestmark = pytest.mark.gpu
proto = er.proto
EPS = er.EPS
# nodes of the kernel tests: one node pair, odd sizes, one workgroup -1 / +0 / +1, two workgroups + 1, and past the
# grid cap (every workgroup then walks more than one chunk)
KERNEL_NODES = [2, 3, 7, er.BLK - 1, er.BLK, er.BLK + 1, 2 * er.BLK + 1, er.BLK * er.MAXBLK + 77]
ENDS = [((0, 0), (0.0, 0.0)), ((1, 0), (1.5, 0.0)), ((1, 1), (0.0, 2.0))]


def _t(a, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device=dev) if dtype is None else \
        torch.as_tensor(np.ascontiguousarray(a), device=dev, dtype=dtype)


def _rand_bands(n, rng):
    kd, md = rng.uniform(1.0, 3.0, n), rng.uniform(0.5, 1.0, n)
    ko, mo = rng.uniform(-1.5, -0.5, n - 1), rng.uniform(0.1, 0.25, n - 1)
    return kd, ko, md, mo


def _apply_ref(bands, kinds, kappa, Z):
    """(MZ, KZ, A, B, sum|terms| of A, of B) with rows outside the unknowns zero and not read."""
    al, be, mu, nu = proto.reduced(bands, kinds, kappa)
    sh, hi = proto.unknowns(len(bands[1]), kinds)
    Zu = np.ascontiguousarray(Z[:, sh:hi])
    KZ, MZ = np.zeros_like(Z), np.zeros_like(Z)
    KZ[:, sh:hi], MZ[:, sh:hi] = proto.tri_apply(al, be, Zu), proto.tri_apply(mu, nu, Zu)
    aK = proto.tri_apply(np.abs(al), np.abs(be), np.abs(Zu))
    aM = proto.tri_apply(np.abs(mu), np.abs(nu), np.abs(Zu))
    return MZ, KZ, Zu @ KZ[:, sh:hi].T, Zu @ MZ[:, sh:hi].T, np.abs(Zu) @ aK.T, np.abs(Zu) @ aM.T, aK, aM, sh, hi


@pytest.mark.parametrize("n", KERNEL_NODES)
def test_apply_kernel(dev, n):
    """MZ, KZ to a few ulp of their three terms, the Gram entries within 4 (ne+1) 2^-53 sum|terms|; two runs bit-identical;
    row j of the nb-case call equals the nb = 1 call."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(n)
    bands = _rand_bands(n, rng)
    tb = [_t(b, dev) for b in bands]
    for nb, (kinds, kappa) in zip((1, 4, 8) if n > 2 else (1, 2, 8), ENDS):
        Z = rng.standard_normal((nb, n))
        MZ, KZ, gram = ops.eig_apply(*tb, _t(Z, dev), kinds, kappa)
        MZ2, KZ2, gram2 = ops.eig_apply(*tb, _t(Z, dev), kinds, kappa)
        assert torch.equal(MZ, MZ2) and torch.equal(KZ, KZ2) and torch.equal(gram, gram2)
        rMZ, rKZ, A, B, sA, sB, aK, aM, sh, hi = _apply_ref(bands, kinds, kappa, Z)
        gMZ, gKZ, g = MZ.cpu().numpy(), KZ.cpu().numpy(), gram.cpu().numpy()
        assert np.all(gKZ[:, :sh] == 0) and np.all(gKZ[:, hi:] == 0) and np.all(gMZ[:, :sh] == 0) and \
            np.all(gMZ[:, hi:] == 0)
        assert np.all(np.abs(gKZ - rKZ)[:, sh:hi] <= 4 * EPS * aK) and np.all(np.abs(gMZ - rMZ)[:, sh:hi] <= 4 * EPS * aM)
        assert np.all(np.abs(g[0] - A) <= 4 * n * EPS * sA), np.max(np.abs(g[0] - A) / sA)
        assert np.all(np.abs(g[1] - B) <= 4 * n * EPS * sB)
        assert np.array_equal(g[0], g[0].T) and np.array_equal(g[1], g[1].T)
        j = nb - 1
        MZ1, KZ1, _ = ops.eig_apply(*tb, _t(Z[j:j + 1], dev), kinds, kappa)
        assert torch.equal(MZ1[0], MZ[j]) and torch.equal(KZ1[0], KZ[j])


@pytest.mark.parametrize("n", KERNEL_NODES)
def test_rotate_kernel(dev, n):
    """X, Y to a few ulp of their nb terms, res2 and |X_j|^2 within 4 (ne+1) 2^-53 sum|terms|; signs; reproducible; row
    j of X for a one-column Q equals the nb = 1 call."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(1000 + n)
    for nb, (kinds, _) in zip((1, 5, 8), ENDS):
        sh, hi = proto.unknowns(n - 1, kinds)
        Z, MZ, KZ = (rng.standard_normal((nb, n)) for _ in range(3))
        Q, theta = rng.standard_normal((nb, nb)), rng.standard_normal(nb)
        args = [_t(a, dev) for a in (Z, MZ, KZ, Q, theta)]
        X, Y, res2 = ops.eig_rotate(*args, kinds)
        X2, Y2, res22 = ops.eig_rotate(*args, kinds)
        assert torch.equal(X, X2) and torch.equal(Y, Y2) and torch.equal(res2, res22)
        mask = np.zeros(n)
        mask[sh:hi] = 1.0
        sign = np.where((Q.T @ Z[:, sh]) < 0, -1.0, 1.0) if hi > sh else np.ones(nb)
        Qs = Q * sign[None, :]
        rX, rY, rR = (Qs.T @ (V * mask) for V in (Z, MZ, KZ))
        aX, aY, aR = (np.abs(Qs).T @ np.abs(V * mask) for V in (Z, MZ, KZ))
        gX, gY, g2 = X.cpu().numpy(), Y.cpu().numpy(), res2.cpu().numpy()
        assert np.all(np.abs(gX - rX) <= 2 * nb * EPS * aX) and np.all(np.abs(gY - rY) <= 2 * nb * EPS * aY)
        assert np.all((gX * (1 - mask)) == 0) and np.all((gY * (1 - mask)) == 0)
        if hi > sh:
            assert np.all(gX[:, sh] >= 0)
        r = rR - theta[:, None] * rY
        ar = aR + np.abs(theta)[:, None] * aY
        # the squares of residual entries that carry their own rounding 2 nb eps ar: (r + d)^2 - r^2 <= 2 |r| d + d^2
        slack = np.sum(2 * np.abs(r) * (4 * nb * EPS * ar) + (4 * nb * EPS * ar) ** 2, axis=1)
        assert np.all(np.abs(g2[0] - np.sum(r * r, axis=1)) <= 4 * n * EPS * np.sum(r * r, axis=1) + slack)
        assert np.all(np.abs(g2[1] - np.sum(rX * rX, axis=1)) <= 4 * n * EPS * np.sum(rX * rX, axis=1)
                      + np.sum(2 * np.abs(rX) * (2 * nb * EPS * aX), axis=1) + 1e-300)
    # nb = 1: the column of a wider call with a Q that passes it through
    Z = rng.standard_normal((3, n))
    Qp = np.eye(3)
    th = np.zeros(3)
    Xw, _, _ = ops.eig_rotate(_t(Z, dev), _t(Z, dev), _t(Z, dev), _t(Qp, dev), _t(th, dev), (0, 0))
    X1, _, _ = ops.eig_rotate(*(_t(Z[1:2], dev),) * 3, _t(np.eye(1), dev), _t(th[:1], dev), (0, 0))
    assert torch.equal(Xw[1], X1[0])


def _ritz_dev(dev, A, B, sigma):
    from hybrid_fem_lssvr_amd import ops
    theta, Q, info = ops.eig_ritz(_t(np.stack([A, B]), dev), sigma)
    return theta.cpu().numpy(), Q.cpu().numpy(), int(info.item())


@pytest.mark.parametrize("nb", range(1, 9))
def test_ritz_device_equals_host(dev, nb):
    """The device Ritz step is bit-equal to lssvr_eig_ritz_host on the same A, B: random SPD B, a repeated eigenvalue."""
    for seed, sigma, rep in ((nb, 0.0, False), (100 + nb, 4.0, False), (200 + nb, 1.0, True)):
        A, B, d = er.random_pencil(nb, seed, repeated=rep)
        th_d, Q_d, info_d = _ritz_dev(dev, A, B, sigma)
        th_h, Q_h, info_h = er.ritz_host(A, B, sigma)
        assert info_d == info_h == 0
        assert np.array_equal(th_d, th_h) and np.array_equal(Q_d, Q_h)
        er.check_ritz(A, B, sigma, th_d, Q_d, info_d, d)


def test_ritz_device_dependent_column(dev):
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((5, 40))
    Z[2] = Z[0]
    D = np.linspace(1.0, 3.0, 40)
    A, B = (Z * D[None, :]) @ Z.T, Z @ Z.T
    th_d, Q_d, info_d = _ritz_dev(dev, A, B, 0.0)
    th_h, Q_h, info_h = er.ritz_host(A, B, 0.0)
    assert info_d == info_h == 1 and np.all(np.isfinite(th_d)) and np.all(np.isfinite(Q_d))
    assert np.array_equal(th_d, th_h) and np.array_equal(Q_d, Q_h) and np.all(Q_d[:, -1] == 0.0)


@pytest.mark.parametrize("name,m", er.cases(600))
def test_count_device(dev, name, m):
    """lssvr_eig_count equals lssvr_eig_count_host, and both equal #{lambda_ref < s}."""
    from hybrid_fem_lssvr_amd import ops
    p = er.case(name, m)
    shifts, lo, hi = er.count_shifts(er.ref_values(p))
    pivmin = er.count_pivmin(p.bands, shifts)
    got = ops.eig_count(*(_t(b, dev) for b in p.bands), _t(shifts, dev), pivmin, p.kinds, p.kappa).cpu().numpy()
    host = er.count_host(p.bands, p.kinds, p.kappa, shifts, pivmin)
    assert np.array_equal(got, host)
    assert np.all((got >= lo) & (got <= hi))


@pytest.mark.parametrize("M,ne,pm", [(2, 5, False), (2, 1, True), (9, 67, True), (16, 129, False), ("mixed", 70, True)])
def test_rayleigh_kernel(dev, M, ne, pm):
    """The three sums against numpy Gauss quadrature of the same rows, relative to out[2], within 4 ne nq 2^-53."""
    from hybrid_fem_lssvr_amd import ops
    rng = np.random.default_rng(ne)
    nodes = np.sort(np.concatenate([[-1.0, 1.0], rng.uniform(-1, 1, ne - 1)]))
    if M == "mixed":
        M = 12
        W = rng.standard_normal((ne, M))
        deg = rng.integers(2, M + 1, ne)
        W[np.arange(M)[None, :] >= deg[:, None]] = 0.0
    else:
        W = rng.standard_normal((ne, M))
    nq = max(M, 8)

    def a(x):
        return 1.0 + 0.25 * x * x

    def c(x):
        return 3.0 * np.sin(2.0 * x)            # (either sign: out[2] is then larger than |out[0]|)

    kinds, kappa = (1, 1), (0.7, 2.0)
    x = _t(nodes, dev)
    pts = ops.estimate_points(x, nq).cpu().numpy()
    tabs = [_t(f(pts).T if pm else f(pts), dev) for f in (a, c, er.graded_rho)]
    out = ops.eig_rayleigh(x, _t(W, dev), nq, *tabs, point_major=pm, end_kinds=kinds, kappa=kappa)
    out2 = ops.eig_rayleigh(x, _t(W, dev), nq, *tabs, point_major=pm, end_kinds=kinds, kappa=kappa)
    import torch
    assert torch.equal(out, out2)
    got = out.cpu().numpy()
    num, den, mag = proto.rayleigh(nodes, W, nq, a, c, er.graded_rho, kinds, kappa)
    bar = 4 * ne * nq * EPS
    assert abs(got[0] - num) <= bar * mag and abs(got[2] - mag) <= bar * mag and abs(got[1] - den) <= bar * den
    assert got[2] >= abs(got[0])


def _solve(p, k, **kw):
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(mesh=p.nodes, lssvr_M=9, lssvr_gamma=1e4, n_colloc=16,
                                 global_domain=(float(p.nodes[0]), float(p.nodes[-1])),
                                 coef=None if p.a is None else (p.a, p.da), reaction=p.c, boundary=p.boundary())
    return s.solve_eigen(k=k, sigma=p.sigma, weight=p.rho, **kw)


@pytest.mark.parametrize("name,m", er.cases(600))
def test_solve_eigen(dev, name, m, note, monkeypatch):
    """The facade on problems 1-5: every check of eigen_rules.check_solution; the solver that problem 3 and 4 must
    take; one k per case also enhanced, the Rayleigh quotient finite and the modes evaluable."""
    from hybrid_fem_lssvr_amd import ops
    calls = {"pivot": 0, "bc": 0}
    piv, bc = ops.tridiag_pivot_solve_multi, ops.tridiag_bc_solve_multi
    monkeypatch.setattr(ops, "tridiag_pivot_solve_multi",
                        lambda *a, **kw: (calls.__setitem__("pivot", calls["pivot"] + 1), piv(*a, **kw))[1])
    monkeypatch.setattr(ops, "tridiag_bc_solve_multi",
                        lambda *a, **kw: (calls.__setitem__("bc", calls["bc"] + 1), bc(*a, **kw))[1])
    p = er.case(name, m)
    ks = er.ks_of(p)
    for k in ks:
        r = _solve(p, k, enhance=(k == ks[-1]))
        assert r.converged and r.iterations <= 200
        er.check_solution(p, k, r.values_fem, r.nodal, r.residuals, r.index, note)
        if k == ks[-1]:
            assert r.values is not None and np.all(np.isfinite(r.values)) and len(r.modes) == k
            mid = r.evaluate(0, 0.5 * (p.nodes[:-1] + p.nodes[1:]))
            assert np.all(np.isfinite(mid))
    if name == "neumann":
        assert calls["pivot"] == 0 and calls["bc"] > 0
    if name == "interior":
        assert calls["bc"] == 0 and calls["pivot"] > 0
        # (the P1 eigenvalues overshoot by about (j pi / ne)^2 / 12: below some 33 elements mode 5 moves out past
        # mode 1 and the four nearest are the modes 1 .. 4, which check_solution has verified against the closed form)
        if p.ne >= 33:
            assert sorted(r.index) == [2, 3, 4, 5] and set(r.index[:2]) == {3, 4} and list(r.index[2:]) == [2, 5]


def test_solve_eigen_large(dev, note):
    """100001 unknowns, problem 1, k = 4, sigma = 0: the closed form, no scipy; the floor alone is the bar."""
    p = er.poisson(er.BIG)
    r = _solve(p, 4, enhance=False)
    assert r.converged and r.iterations <= 200
    exact = np.array([er.poisson_exact(p.ne, j) for j in range(1, 5)])
    bar = er.eig_bar(p, with_lapack=False)
    note("iterations", r.iterations)
    note("eigenvalue error", np.max(np.abs(r.values_fem - exact)), bar)
    assert np.all(np.abs(r.values_fem - exact) <= bar)
    assert list(r.index) == [0, 1, 2, 3]
    kmax = p.scales[0]
    xn = np.sqrt(np.sum(r.nodal ** 2, axis=1))
    assert np.all(r.residuals <= 1e-12 * kmax * xn)
    for j in range(4):
        assert abs(r.residuals[j] - er.residual_ld(p, r.values_fem[j], r.nodal[j])) <= \
            64 * EPS * 6 * er.block_ratio(p, 4) * kmax * xn[j]


@pytest.mark.parametrize("ne", [8, 16, 32])
def test_enhanced_eigenvalue(dev, ne, note):
    """-u'' = lambda u, Dirichlet, M = 9, modes j = 1, 2: the enhanced value is strictly closer to (j pi / 2)^2 than the
    P1 value, and agrees with the CPU value -- the oracle's reaction-row enhancement of the same nodal values, then
    numpy Gauss quadrature -- at the parity bar of the reaction tests (1e-11 on the coefficients; the quotient weights
    coefficient k with P_k' up to k (k + 1) / 2 <= 36, so 36 x that on the value).  Improvement factors measured with
    the prototype on the CPU: 6.0e3 / 3.6e2 at ne = 8, 9.7e4 / 6.0e3 at 16, 1.5e6 / 9.7e4 at 32."""
    from oracle import lssvr_oracle as orc
    p = er.poisson(ne - 1)
    r = _solve(p, 2)
    order = np.argsort(r.values_fem)
    for j, col in zip((1, 2), order):
        exact = (j * math.pi / 2.0) ** 2
        e_fem, e_enh = abs(r.values_fem[col] - exact), abs(r.values[col] - exact)
        note(f"mode {j} improvement factor", e_fem / e_enh)
        assert e_enh < e_fem
        val, W = proto.enhanced_value(p.nodes, r.nodal[col], r.values_fem[col], 9, 1e4, 16)
        Wg = r.modes[col].W.cpu().numpy()
        note(f"mode {j} coefficient parity", orc.rel_l2_coef(Wg, W).max(), 1e-11)
        note(f"mode {j} value parity", abs(r.values[col] - val) / val, 36e-11)
        assert orc.rel_l2_coef(Wg, W).max() <= 1e-11
        assert abs(r.values[col] - val) <= 36e-11 * val
