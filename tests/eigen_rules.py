"""Problems, references and bars of the eigenproblem entries (include/lssvr_hip.h: lssvr_eig_*)
and of FEMLSSVRPrimalSolver.solve_eigen.  A plain module shared by tests/test_eigen_cpu.py and tests/test_gpu_eigen.py:
the bands come from tests/convection_rules.py (b = None), the numpy statement of the algorithm from
scripts/proto/eigen_proto.py, the reference from scipy.linalg.eigh on the dense pencil -- or, for the uniform Poisson
problem, from the closed form of the discrete eigenvalues."""
import functools
import importlib.util
import math
import os
import re

import numpy as np

import convection_rules as cr
import pivot_rules as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "hybrid_fem_lssvr_amd", "csrc", "eigen.hip")).read()
BLK = int(re.search(r"constexpr int kEigBlock = (\d+);", _SRC).group(1))           # nodes per workgroup
MAXBLK = int(re.search(r"constexpr int kEigMaxBlocks = (\d+);", _SRC).group(1))    # grid cap of the reductions
SWEEPS = int(re.search(r"constexpr int kRitzSweeps = (\d+);", _SRC).group(1))

_spec = importlib.util.spec_from_file_location("eigen_proto", os.path.join(ROOT, "scripts", "proto", "eigen_proto.py"))
proto = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(proto)

DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN
EPS = 2.0 ** -53
DD = (DIRICHLET, DIRICHLET)


def block_width(k, m):
    return min(8, k + 2, m)


# numbers of unknowns: 1, 2, around the block widths of k = 4 and k = 6 (nb - 1, nb, nb + 1), around the coarsest level
# of the pivoting solve, one workgroup of nodes -1 / +0 / +1 (BLK - 2 unknowns between two Dirichlet ends are BLK
# nodes), two workgroups + 1
SIZES = sorted({1, 2, 5, 6, 7, 8, 9, pr.B - 1, pr.B, pr.B + 1, BLK - 3, BLK - 2, BLK - 1, BLK, BLK + 1, 2 * BLK - 1,
                2 * BLK + 1})
KS = (1, 2, 4, 6)
BIG = 100001            # unknowns of the one large run: problem 1, k = 4, sigma = 0


def ks_for(m):
    return sorted({min(k, m) for k in KS})


def _zero(x):
    return np.zeros_like(np.asarray(x, dtype=np.float64))


def _one(x):
    return np.ones_like(np.asarray(x, dtype=np.float64))


# --------------------------------------------------------------------------
# the problems: name -> Problem(nodes, a, da, c, rho, kinds, kappa, sigma); every case is computed once and shared
# --------------------------------------------------------------------------
class Problem:
    def __init__(self, name, nodes, a=None, da=None, c=None, rho=None, kinds=DD, kappa=(0.0, 0.0), sigma=0.0,
                 ks=None):
        self.name, self.nodes, self.a, self.da, self.c, self.rho = name, nodes, a, da, c, rho
        self.kinds, self.kappa, self.sigma, self.ks = kinds, kappa, sigma, ks
        self.ne = len(nodes) - 1
        sh, hi = proto.unknowns(self.ne, kinds)
        self.sh, self.hi, self.m = sh, hi, hi - sh

    @functools.cached_property
    def bands(self):
        """(kdiag, koff, mdiag, moff) from convection_rules.conv_bands with b = None."""
        kd, ko = cr.conv_bands(self.nodes, _zero, self.a, None, _zero if self.c is None else self.c)[:2]
        md, mo = cr.conv_bands(self.nodes, _zero, _zero, None, _one if self.rho is None else self.rho)[:2]
        return kd, ko, md, mo

    @functools.cached_property
    def reduced(self):
        return proto.reduced(self.bands, self.kinds, self.kappa)

    @functools.cached_property
    def scales(self):
        """(max |K band|, min M diagonal, Gershgorin floor of M's smallest eigenvalue) over the unknowns."""
        al, be, mu, nu = self.reduced
        row = mu.copy()
        row[1:] -= np.abs(nu)
        row[:-1] -= np.abs(nu)
        return max(float(np.abs(al).max()), float(np.abs(be).max()) if be.size else 0.0), float(mu.min()), float(row.min())

    @functools.cached_property
    def reference(self):
        """(lambda[m] ascending, V[m, m] M-orthonormal columns) by scipy.linalg.eigh on the dense pencil."""
        from scipy.linalg import eigh
        Kd, Md = proto.dense(self.bands, self.kinds, self.kappa)
        return eigh(Kd, Md)

    def boundary(self):
        """The facade's ``boundary`` argument."""
        if self.kinds == DD:
            return None
        return tuple(None if kd == DIRICHLET else ("robin", kp, 0.0) for kd, kp in zip(self.kinds, self.kappa))

    def nearest(self, k, lam=None):
        """Indices (into the ascending spectrum) of the k eigenvalues nearest sigma, nearest first."""
        lam = self.reference[0] if lam is None else lam
        return np.argsort(np.abs(lam - self.sigma), kind="stable")[:k]


def poisson_exact(ne, j):
    """The j-th discrete Dirichlet eigenvalue of -u'' on ne uniform P1 elements of (-1, 1) (pivot_rules.resonant_k2),
    j = 1 .. ne - 1; the vector is sin(j pi i / ne); the continuous value is (j pi / 2)^2."""
    return pr.resonant_k2(2.0 / ne, ne, j)


def poisson_spectrum(ne):
    return np.array([poisson_exact(ne, j) for j in range(1, ne)])


@functools.lru_cache(maxsize=None)
def poisson(m):
    """1. uniform Poisson, Dirichlet: m unknowns on m + 1 elements of (-1, 1)."""
    return Problem("poisson", np.linspace(-1.0, 1.0, m + 2))


def graded_nodes(ne):
    t = np.linspace(0.0, 1.0, ne + 1)
    return -1.0 + 2.0 * t ** 1.5


def graded_c(x):
    return 1.0 + np.asarray(x, dtype=np.float64) ** 2


def graded_rho(x):
    return 1.0 + 0.5 * np.asarray(x, dtype=np.float64) ** 2


@functools.lru_cache(maxsize=None)
def graded(m, robin=False):
    """2. graded mesh, a = 1 + x^2 / 4, c = 1 + x^2 >= 0, rho = 1 + x^2 / 2; Dirichlet ends, or Robin ends with
    kappa = 2 (one Robin and one Dirichlet end where m = 1)."""
    if not robin:
        return Problem("graded", graded_nodes(m + 1), cr.man_a, cr.man_da, graded_c, graded_rho)
    if m == 1:
        return Problem("graded-robin", graded_nodes(1), cr.man_a, cr.man_da, graded_c, graded_rho, (ROBIN, DIRICHLET),
                       (2.0, 0.0))
    return Problem("graded-robin", graded_nodes(m - 1), cr.man_a, cr.man_da, graded_c, graded_rho, (ROBIN, ROBIN),
                   (2.0, 2.0))


@functools.lru_cache(maxsize=None)
def neumann(m):
    """3. -u'' = lambda u with two Neumann ends: lambda_0 = 0, K is singular; sigma = -1 keeps K - sigma M positive
    definite, so the facade must take the solve that does not pivot.  m >= 2 unknowns on m - 1 elements."""
    return Problem("neumann", np.linspace(-1.0, 1.0, m), kinds=(ROBIN, ROBIN), sigma=-1.0)


def interior_ne(m):
    """Elements for problem 4: m + 1, moved up while a multiple of pivot_rules.P or P - 1 (no partition of the pivoting
    solve is then resonant at a shift between two eigenvalues of the whole interval)."""
    ne = m + 1
    while ne % pr.P == 0 or ne % (pr.P - 1) == 0:
        ne += 1
    return ne


@functools.lru_cache(maxsize=None)
def interior(m):
    """4. problem 1 with sigma midway between lambda_3 and lambda_4 and k = 4, the modes counted from 0 as the Sturm
    count and ``index`` count them (lambda_0 the lowest; lambda_i is poisson_exact(ne, i + 1), the closed form counts
    from 1).  The eigenvalues grow like (i + 1)^2: the distances from sigma are 4.5, 4.5, 11.5, 15.5, 16.5, ... times
    (pi / 2)^2 for the modes 3, 4, 2, 5, 1, so k = 4 returns the modes 2, 3, 4, 5.  The shifted matrix is indefinite:
    the pivoting solve.  At least 6 unknowns."""
    ne = interior_ne(max(m, 6))
    sigma = 0.5 * (poisson_exact(ne, 4) + poisson_exact(ne, 5))
    return Problem("interior", np.linspace(-1.0, 1.0, ne + 1), sigma=sigma, ks=(4,))


def well_c(x):
    x = np.asarray(x, dtype=np.float64)
    return 400.0 * (x * x - 0.25) ** 2


@functools.lru_cache(maxsize=None)
def double_well(m):
    """5. -u'' + 400 (x^2 - 1/4)^2 u = lambda u, Dirichlet: a symmetric double well, the two lowest eigenvalues close.
    scipy.linalg.eigh on the P1 pencil gives lambda_1, lambda_2, lambda_3 = 15.4271, 19.9038, 42.6189 at 255 unknowns
    (gap 4.477, 29 % of lambda_1, a fifth of the distance to lambda_3) and 15.4694, 19.9901, 42.8815 at 31: a pair, close
    next to the rest of the spectrum but well separated at REL_GAP."""
    return Problem("double-well", np.linspace(-1.0, 1.0, m + 2), c=well_c, ks=(2,))


PROBLEMS = {"poisson": (poisson, 1), "graded": (graded, 1), "graded-robin": (lambda m: graded(m, True), 1),
            "neumann": (neumann, 2), "interior": (interior, 6), "double-well": (double_well, 6)}


def case(name, m):
    make, _ = PROBLEMS[name]
    return make(m)


def cases(max_m=None):
    """[(name, m)] of every problem at every size it runs at (its own least size upwards)."""
    out = []
    for name, (_, least) in PROBLEMS.items():
        out += [(name, m) for m in SIZES if m >= least and (max_m is None or m <= max_m)]
    return out


def ks_of(p):
    return ks_for(p.m) if p.ks is None else tuple(k for k in p.ks if k <= p.m)


def ref_values(p):
    """The reference eigenvalues, ascending: the closed form for the uniform Poisson problems, else scipy."""
    if p.name in ("poisson", "interior"):
        return poisson_spectrum(p.ne)
    return p.reference[0]


# --------------------------------------------------------------------------
# bars
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lapack_distance(m):
    """max_j |scipy.linalg.eigh - closed form| over the spectrum of problem 1 with m unknowns."""
    p = poisson(m)
    return float(np.max(np.abs(p.reference[0] - poisson_spectrum(p.ne))))


# The floor of the eigenvalue bar is FLOOR_MULT 2^-53 max|K band| / min(M diag), the rounding scale of a Rayleigh
# quotient whose numerator is a sum of terms of size max|K| x_i^2 and whose denominator is at least min(M diag) |x|^2 / 3.
# Measured on the CPU (scripts/proto/eigen_proto.py against the closed form, problem 1, k = 4, sigma = 0), in units of
# 2^-53 max|K| / min(M diag):   m = 5: 9.5 (all five eigenvalues, the largest is 4 units itself)   31: 0.27   255: 0.25
# 513: 0.17   100001: 0.28 (the device run at 100001 gives the same 0.28);
# LAPACK's own distance in the same unit:   m = 5: 14   31: 27   255: 16   513: 138  (the dense solve is not run at
# 100001, where the floor alone is the bar: 1.3e-5 against eigenvalues 2.47 .. 39.5).  The device sums run in another
# order (64 lanes, 4 waves, up to 1024 blocks) with the same error model; 16 covers the small systems, whose blocks
# reach the top of the spectrum, and leaves a factor 50 over what the prototype shows elsewhere.
FLOOR_MULT = 16.0


def eig_bar(p, with_lapack=True):
    """|theta_j - lambda_ref| <= max(10 x LAPACK's distance from the closed form on problem 1 at this size, floor)."""
    kmax, mdmin, _ = p.scales
    floor = FLOOR_MULT * EPS * kmax / mdmin
    return max(10.0 * lapack_distance(p.m), floor) if with_lapack else floor


REL_GAP = 1e-3          # an eigenvalue closer than this (relative) to a neighbour is compared as part of a subspace


def residual_ld(p, theta, x):
    """|K x - theta M x|_2 over the unknowns in long double, x [ne+1]."""
    ld = np.longdouble
    al, be, mu, nu = (t.astype(ld) for t in p.reduced)
    v = np.asarray(x, dtype=ld)[p.sh:p.hi]
    d, o = al - ld(theta) * mu, be - ld(theta) * nu
    r = d * v
    r[:-1] += o * v[1:]
    r[1:] += o * v[:-1]
    return float(np.sqrt(np.sum(r * r)))


def m_inner(p, X, Y):
    """X M Y^T for rows over the full node range."""
    _, _, mu, nu = p.reduced
    return X[:, p.sh:p.hi] @ proto.tri_apply(mu, nu, np.ascontiguousarray(Y[:, p.sh:p.hi])).T


def block_ratio(p, k):
    """max / min of |lambda - sigma| over the block of nb = min(8, k + 2, m) eigenvalues nearest sigma: the spread of
    the scales of the iteration vectors, whose square is the condition number of B = Z^T M Z."""
    lam = ref_values(p)
    d = np.sort(np.abs(lam - p.sigma))[:block_width(k, p.m)]
    return float(d[-1] / d[0])


def check_solution(p, k, theta, X, residuals, index, note=None):
    """Every property a converged solve must have, against the reference of ``p``; theta[k], X[k, ne+1]."""
    lam = ref_values(p)
    want = p.nearest(k, lam)
    kmax, _, mmin = p.scales
    nb = block_width(k, p.m)
    ratio = block_ratio(p, k)
    # the eigenvalues, in the order of their distance from sigma, and their positions in the spectrum
    bar = eig_bar(p)
    # (two values at the same distance from sigma, as in problem 4, may come in either order: every theta is paired
    # with the reference value nearest to it, the set must be the wanted one and the distances must not decrease)
    match = np.array([int(np.argmin(np.abs(lam - t))) for t in theta])
    err = np.abs(theta - lam[match])
    if note:
        note("eigenvalue error / bar", float(np.max(err / bar)), 1.0)
    assert np.all(err <= bar), (p.name, p.m, k, theta, lam[match], bar)
    assert sorted(match) == sorted(want), (p.name, p.m, k, match, want)
    dist = np.abs(lam[match] - p.sigma)
    assert np.all(dist[1:] >= dist[:-1] - 2.0 * bar), (p.name, p.m, k, dist)
    assert index is not None and list(index) == list(match), (p.name, p.m, k, index, match)
    want = match
    # rows outside the unknowns are exactly 0, the first unknown is positive
    assert np.all(X[:, :p.sh] == 0.0) and np.all(X[:, p.hi:] == 0.0)
    assert np.all(X[:, p.sh] > 0.0)
    # M-orthonormal: Q^T B Q = I holds to the rounding of an nb-term Gram matrix of condition ratio^2
    G = m_inner(p, X, X)
    orth = float(np.max(np.abs(G - np.eye(k))))
    orth_bar = 256.0 * EPS * nb * ratio ** 2
    if note:
        note("orthonormality", orth, orth_bar)
    assert orth <= orth_bar, (p.name, p.m, k, orth, orth_bar)
    # the returned residuals against long double: the device forms K Z Q - theta M Z Q from nb columns of scale <= ratio
    xn = np.sqrt(np.sum(X * X, axis=1))
    for j in range(k):
        r_ld = residual_ld(p, theta[j], X[j])
        res_bar = 64.0 * EPS * nb * ratio * kmax * xn[j]
        assert abs(residuals[j] - r_ld) <= res_bar, (p.name, p.m, k, j, residuals[j], r_ld, res_bar)
    # vectors: Davis-Kahan, sin(angle) <= |r|_{M^-1} / gap <= |r|_2 / (sqrt(mmin) gap), for ours and for the reference's
    if p.name in ("poisson", "interior"):
        i = np.arange(p.ne + 1)
        V = np.array([np.sin((j + 1) * math.pi * i / p.ne) for j in range(p.m)])
        V /= np.sqrt(np.diag(m_inner(p, V, V)))[:, None]
    else:
        V = np.zeros((p.m, p.ne + 1))
        V[:, p.sh:p.hi] = p.reference[1].T
    done = set()
    for j in range(k):
        if j in done:
            continue
        # the cluster of wanted eigenvalues around lam[want[j]] that are relatively close to each other
        group = [i for i in range(k) if abs(lam[want[i]] - lam[want[j]]) <= REL_GAP * max(abs(lam[want[j]]), 1.0)]
        done.update(group)
        idx = want[group]
        rest = np.delete(lam, idx)
        gap = float(np.min(np.abs(rest[:, None] - lam[idx][None, :]))) if rest.size else np.inf
        r_all = sum(residual_ld(p, theta[i], X[i]) + residual_ld(p, lam[want[i]], V[want[i]]) for i in group)
        sin_bar = 2.0 * r_all / (math.sqrt(mmin) * gap) + 64.0 * EPS * nb * ratio ** 2
        C = m_inner(p, V[idx], X[group])                    # cosines between the two bases
        dev = float(np.max(np.abs(C @ C.T - np.eye(len(group)))))
        assert dev <= 2.0 * sin_bar ** 2 + 256.0 * EPS * nb * ratio ** 2, (p.name, p.m, k, group, dev, sin_bar)
        if len(group) == 1:
            s = 1.0 if C[0, 0] > 0 else -1.0
            d = X[group[0]] - s * V[idx[0]]
            dist = math.sqrt(abs(float(m_inner(p, d[None], d[None])[0, 0])))
            assert dist <= math.sqrt(2.0) * sin_bar + 256.0 * EPS * nb * ratio ** 2, (p.name, p.m, k, j, dist, sin_bar)


# --------------------------------------------------------------------------
# the library's host entries through ctypes (no device is touched)
# --------------------------------------------------------------------------
def _hd(a):
    import ctypes
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def ritz_host(A, B, sigma):
    """lssvr_eig_ritz_host -> (theta[nb], Q[nb, nb], info)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    nb = A.shape[0]
    theta, Q, info = np.full(nb, np.nan), np.full((nb, nb), np.nan), np.full(1, -1, dtype=np.int32)
    _capi.check(lib.lssvr_eig_ritz_host(_hd(A), _hd(B), nb, float(sigma), _hd(theta), _hd(Q), info.ctypes.data),
                "lssvr_eig_ritz_host")
    return theta, Q, int(info[0])


def count_host(bands, kinds, kappa, shifts, pivmin=None):
    """lssvr_eig_count_host -> int32[ns]."""
    import ctypes
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    kd, ko, md, mo = (np.ascontiguousarray(t, dtype=np.float64) for t in bands)
    shifts = np.ascontiguousarray(shifts, dtype=np.float64)
    if pivmin is None:
        pivmin = count_pivmin(bands, shifts)
    out = np.full(len(shifts), -1, dtype=np.int32)
    kap = (ctypes.c_double * 2)(*map(float, kappa))
    _capi.check(lib.lssvr_eig_count_host(_hd(kd), _hd(ko), _hd(md), _hd(mo), int(kinds[0]), int(kinds[1]), kap, len(ko),
                                         _hd(shifts), len(shifts), float(pivmin), out.ctypes.data),
                "lssvr_eig_count_host")
    return out


def count_pivmin(bands, shifts):
    """dstebz's pivmin for the shifted matrices: the smallest normal number times max(1, max beta^2)."""
    _, ko, _, mo = bands
    big = float(np.max(np.abs(ko))) + float(np.max(np.abs(shifts))) * float(np.max(np.abs(mo)))
    return np.finfo(np.float64).tiny * max(1.0, big * big)


def pivot_solve_host(al, be, mu, nu, sigma, Y):
    """proto.shifted_solve through lssvr_tridiag_pivot_solve_host: the m unknowns between two Dirichlet ends of value 0
    (a Robin end's kappa is already on alpha's end entry)."""
    import ctypes
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    m, nb = len(al), Y.shape[0]
    ne = m + 1
    diag = np.ones(ne + 1)
    diag[1:-1] = al - sigma * mu
    off = np.zeros(ne)
    off[1:-1] = be - sigma * nu
    load = np.zeros((nb, ne + 1))
    load[:, 1:-1] = Y
    u = np.full((nb, ne + 1), np.nan)
    info = np.full(1, -1, dtype=np.int32)
    kap = (ctypes.c_double * 2)(0.0, 0.0)
    _capi.check(lib.lssvr_tridiag_pivot_solve_host(diag.ctypes.data, off.ctypes.data, off.ctypes.data, load.ctypes.data,
                                                   0, 0, None, kap, ne, nb, u.ctypes.data, info.ctypes.data),
                "lssvr_tridiag_pivot_solve_host")
    assert info[0] == 0, info
    return np.ascontiguousarray(u[:, 1:-1])


def sturm_host(al, be, mu, nu, s):
    """proto.sturm_count through lssvr_eig_count_host (the reduced system as Dirichlet-Dirichlet bands)."""
    m = len(al)
    kd, md = np.zeros(m + 2), np.ones(m + 2)
    kd[1:-1], md[1:-1] = al, mu
    ko, mo = np.zeros(m + 1), np.zeros(m + 1)
    ko[1:-1], mo[1:-1] = be, nu
    return int(count_host((kd, ko, md, mo), DD, (0.0, 0.0), [s])[0])


def count_shifts(lam):
    """The shifts of the count tests and what each must return: between every pair of neighbouring reference
    eigenvalues, below the first and above the last -> the exact count; on an eigenvalue -> either neighbour."""
    lam = np.asarray(lam, dtype=np.float64)
    mid = 0.5 * (lam[1:] + lam[:-1])
    span = max(1.0, float(lam[-1] - lam[0]))
    shifts = np.concatenate([[lam[0] - 0.1 * span], mid, [lam[-1] + 0.1 * span], lam])
    lo = np.concatenate([[0], np.arange(1, len(lam)), [len(lam)], np.arange(len(lam))])
    hi = np.concatenate([[0], np.arange(1, len(lam)), [len(lam)], np.arange(len(lam)) + 1])
    return shifts, lo, hi


def random_pencil(nb, seed, repeated=False):
    """(A, B): B = G^T G + I/4 with G random nb x nb (symmetric positive definite), A = B^(1/2)-congruent to a diagonal
    of known values: A = L D L^T with B = L L^T, so the eigenvalues of (A, B) are D.  ``repeated``: two equal values."""
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((nb, nb))
    B = G.T @ G + 0.25 * np.eye(nb)
    d = np.sort(rng.uniform(-3.0, 10.0, nb))
    if repeated and nb > 1:
        d[1] = d[0]
    L = np.linalg.cholesky(B)
    U = np.linalg.qr(rng.standard_normal((nb, nb)))[0]
    A = L @ (U * d[None, :]) @ U.T @ L.T
    return 0.5 * (A + A.T), 0.5 * (B + B.T), d


def check_ritz(A, B, sigma, theta, Q, info, d=None):
    """Q^T A Q = diag theta, Q^T B Q = I, theta ordered by |theta - sigma| and equal to the known values."""
    nb = A.shape[0]
    assert info == 0 and np.all(np.isfinite(theta)) and np.all(np.isfinite(Q))
    cond = np.linalg.cond(B)
    scale = float(np.max(np.abs(A))) * float(np.max(np.abs(Q))) ** 2
    bar = 64.0 * EPS * nb * nb * cond
    assert np.max(np.abs(Q.T @ B @ Q - np.eye(nb))) <= bar, (nb, np.max(np.abs(Q.T @ B @ Q - np.eye(nb))), bar)
    assert np.max(np.abs(Q.T @ A @ Q - np.diag(theta))) <= bar * max(scale, 1.0)
    key = np.abs(theta - sigma)
    assert np.all(key[1:] >= key[:-1])
    if d is not None:
        assert np.max(np.abs(np.sort(theta) - np.sort(d))) <= bar * max(float(np.max(np.abs(d))), 1.0)
