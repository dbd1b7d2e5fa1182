"""Problems and reference of the pivoting tridiagonal solve (include/lssvr_hip.h: lssvr_tridiag_pivot_solve_multi,
DESIGN.md section 24): P1 systems that are well posed but not diagonally dominant, and a long-double-refined LAPACK
solution to compare with.  A plain module shared by tests/test_pivot_cpu.py and tests/test_gpu_pivot.py; the bands come
from tests/convection_rules.py."""
import functools
import math
import os
import re

import numpy as np

import convection_rules as cr
from convection_rules import conv_bands                     # noqa: F401  (imported, not copied)
from oracle import lssvr_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "hybrid_fem_lssvr_amd", "csrc", "tridiag_pivot.hip")).read()
P = int(re.search(r"constexpr int kP = (\d+);", _SRC).group(1))                # rows per partition
B = int(re.search(r"constexpr int kPivBase = (\d+);", _SRC).group(1))          # unknowns of the coarsest level

DIRICHLET, ROBIN = 0, 1
ENDS_D = ((DIRICHLET, DIRICHLET), (0.0, 0.0), (0.25, -0.5))                     # (kinds, kappa, end values)

# numbers of unknowns m: around a partition, two partitions, the coarsest level, one and two levels above it, and one
# size near 1e5 (six levels at P = 8, B = 32)
SIZES = [1, 2, 3, P - 1, P, P + 1, 2 * P - 1, 2 * P + 1, B - 1, B, B + 1, B * P // 2 - 1, B * P // 2 + 1, 100002]


def resonant_k2(h, L, j=1):
    """k^2 = (6 / h^2) (1 - cos t) / (2 + cos t), t = j pi / L: the j-th discrete Dirichlet eigenvalue of
    -u'' on a run of L uniform P1 elements of length h.  With c = -k^2 the interior block of such a run is singular."""
    t = j * math.pi / L
    return (6.0 / (h * h)) * (1.0 - math.cos(t)) / (2.0 + math.cos(t))


# --------------------------------------------------------------------------
# the system of a call, and its reference solution
# --------------------------------------------------------------------------
def system(bands, ends):
    """(sh, ab[3, m], rhs[m]) of the unknowns of a call: nodes sh .. sh+m-1, LAPACK banded storage."""
    diag, sub, sup, load = (np.asarray(t, dtype=np.float64) for t in bands)
    kinds, kappa, values = ends
    ne = len(sub)
    f0, f1 = kinds[0] == ROBIN, kinds[1] == ROBIN
    sh, hi = (0 if f0 else 1), (ne + 1 if f1 else ne)
    m = hi - sh
    ab = np.zeros((3, max(m, 0)))
    if m <= 0:
        return sh, ab, np.zeros(0)
    ab[1] = diag[sh:hi]
    ab[0, 1:] = sup[sh:hi - 1]
    ab[2, :-1] = sub[sh:hi - 1]
    r = load[sh:hi].copy()
    if f0:
        ab[1, 0] += kappa[0]
        r[0] += values[0]
    else:
        r[0] -= sub[0] * values[0]
    if f1:
        ab[1, -1] += kappa[1]
        r[-1] += values[1]
    else:
        r[-1] -= sup[ne - 1] * values[1]
    return sh, ab, r


def _residual_ld(ab, r, x):
    ld = np.longdouble
    x = np.asarray(x, dtype=ld)
    res = np.asarray(r, dtype=ld) - ab[1].astype(ld) * x
    res[:-1] -= ab[0, 1:].astype(ld) * x[1:]
    res[1:] -= ab[2, :-1].astype(ld) * x[:-1]
    return res


def _full(bands, ends, sh, x, dtype):
    ne = len(bands[1])
    u = np.zeros(ne + 1, dtype=dtype)
    u[0], u[-1] = ends[2]                                   # (a free end is overwritten by its unknown)
    u[sh:sh + len(x)] = x
    return u


def refined_ld(bands, ends=ENDS_D):
    """(u_ref long double [ne+1], u_lapack float64 [ne+1]): LAPACK's pivoting banded LU, then iterative refinement with
    the residual in long double and the correction again through solve_banded, until the correction stops shrinking
    (at most 5 steps).  Valid while cond * 2^-53 << 1."""
    from scipy.linalg import solve_banded
    sh, ab, r = system(bands, ends)
    if ab.shape[1] == 0:
        z = np.zeros(0)
        return _full(bands, ends, sh, z, np.longdouble), _full(bands, ends, sh, z, np.float64)
    x0 = solve_banded((1, 1), ab, r)
    x = x0.astype(np.longdouble)
    last = np.inf
    for _ in range(5):
        dx = solve_banded((1, 1), ab, _residual_ld(ab, r, x).astype(np.float64))
        size = float(np.max(np.abs(dx)))
        if not size < last:
            break
        x = x + dx.astype(np.longdouble)
        last = size
    return _full(bands, ends, sh, x, np.longdouble), _full(bands, ends, sh, x0, np.float64)


def residual(bands, ends, u):
    """max |r| over the rows of the unknowns, in long double."""
    sh, ab, r = system(bands, ends)
    if ab.shape[1] == 0:
        return 0.0
    return float(np.max(np.abs(_residual_ld(ab, r, np.asarray(u)[sh:sh + ab.shape[1]]))))


def dense(bands, ends=ENDS_D):
    sh, ab, _ = system(bands, ends)
    return np.diag(ab[1]) + np.diag(ab[0, 1:], 1) + np.diag(ab[2, :-1], -1)


# --------------------------------------------------------------------------
# the problems; every case is computed once and shared: do not write to the arrays
# --------------------------------------------------------------------------
def helmholtz_ne(m, L):
    """Elements for m unknowns between two Dirichlet ends, moved up by one where that is a multiple of L (there the
    global matrix is singular)."""
    ne = m + 1
    return ne + 1 if ne % L == 0 else ne


def helmholtz_k2(ne, L):
    return resonant_k2(2.0 / ne, L, 1)


@functools.lru_cache(maxsize=None)
def helmholtz(ne, L):
    """1. -u'' - k^2 u = pi^2 sin(pi x) on a uniform mesh of (-1, 1), k^2 resonant for runs of L elements."""
    k2 = helmholtz_k2(ne, L)
    nodes = np.linspace(-1.0, 1.0, ne + 1)
    return conv_bands(nodes, orc.poisson_rhs, None, None, lambda x: -k2 + 0.0 * np.asarray(x, dtype=np.float64))[:4]


@functools.lru_cache(maxsize=None)
def zero_diagonal(m):
    """2. diag = 0, sub = sup = 1, m unknowns between two Dirichlet ends: non-singular for even m, exactly singular for
    odd m."""
    ne = m + 1
    rng = np.random.default_rng(77 + m)
    return np.zeros(ne + 1), np.ones(ne), np.ones(ne), rng.standard_normal(ne + 1)


KAPPA_TURN = 12.0


def turning_c(x):
    return -(KAPPA_TURN ** 2) * np.asarray(x, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def turning(ne):
    """3. -u'' - kappa^2 x u = pi^2 sin(pi x), kappa = 12: c changes sign at x = 0."""
    return conv_bands(np.linspace(-1.0, 1.0, ne + 1), orc.poisson_rhs, None, None, turning_c)[:4]


def peclet(ne, pe, shape):
    """4. / 5. the bands of convection_rules.peclet_case."""
    return cr.peclet_case(ne, pe, shape)[0]


PROBLEMS = [("helm8", lambda m: helmholtz(helmholtz_ne(m, 8), 8), ENDS_D),
            ("helmP-1", lambda m: helmholtz(helmholtz_ne(m, P - 1), P - 1), ENDS_D),
            ("zero-diag", lambda m: zero_diagonal(m + m % 2), ENDS_D),
            ("turning", lambda m: turning(m + 1), ENDS_D),
            ("pe5-pos", lambda m: peclet(m + 1, 5.0, "pos"), ENDS_D),
            ("pe5-neg", lambda m: peclet(m + 1, 5.0, "neg"), ENDS_D),
            ("pe5-change", lambda m: peclet(m + 1, 5.0, "change"), ENDS_D),
            ("pe0.5-pos", lambda m: peclet(m + 1, 0.5, "pos"), ENDS_D),
            # 6. one Robin end with kappa = -0.5 (m unknowns: ne = m), one inflow Neumann end (b > 0: inflow on the left)
            ("turning-robin", lambda m: turning(m), ((ROBIN, DIRICHLET), (-0.5, 0.0), (0.3, -0.5))),
            ("pe5-pos-neumann", lambda m: peclet(m, 5.0, "pos"), ((ROBIN, DIRICHLET), (0.0, 0.0), (0.3, -0.5)))]
if P != 8:      # (L = P: the partition itself; the same case as helm8 when P = 8)
    PROBLEMS.insert(2, ("helmP", lambda m: helmholtz(helmholtz_ne(m, P), P), ENDS_D))


def sizes(name):
    """The sizes a problem runs at: all of them, for every problem.  (The inflow Neumann end at Peclet 5 is the worst
    conditioned: LAPACK is 1e-5 of max|u| from the refined solution at 100002 unknowns, so cond * 2^-53 is still well
    below 1 and the refinement converges.)"""
    return SIZES


@functools.lru_cache(maxsize=None)
def case(name, m):
    """(bands, ends, u_ref, u_lapack) of problem ``name`` with m unknowns."""
    _, make, ends = next(p for p in PROBLEMS if p[0] == name)
    bands = make(m)
    u_ref, u_la = refined_ld(bands, ends)
    return bands, ends, u_ref, u_la


# The bars of test_tridiag_dirichlet_solve (tests/test_gpu_fem_eval.py), copied as numbers as tests/test_gpu_conv.py
# does; a size between two listed ones takes the bar of the next listed size.
TRIDIAG_FORWARD_BAR = {1: 0.0, 2: 1e-15, 3: 1e-15, 24: 1e-14, 511: 2.5e-12, 512: 2.5e-12, 513: 2.5e-12,
                       514: 2.5e-12, 1025: 4e-12, 16385: 2e-9, 100000: 7e-8, 1234567: 2e-6}


def forward_bar(ne):
    return TRIDIAG_FORWARD_BAR[min(k for k in TRIDIAG_FORWARD_BAR if k >= ne)]


def bars(bands, ends, u_ref, u_la):
    """(forward bar, residual bar, LAPACK's forward error, LAPACK's residual) of a case: the bars test_gpu_conv.py
    holds the unpivoted solver to.  forward: max(10 x LAPACK's distance from u_ref, forward_bar(ne)) max|u_ref|;
    residual: max(10 x LAPACK's residual, 1e-13 max|band| max|u| max(1, log2 ne))."""
    ne = len(bands[1])
    scale = float(np.max(np.abs(u_ref)))
    lapack = float(np.max(np.abs(u_la.astype(np.longdouble) - u_ref)))
    la_res = residual(bands, ends, u_la)
    amax = max(float(np.max(np.abs(b))) for b in bands[:3])
    fwd = max(10.0 * lapack, forward_bar(ne)) * scale
    res = max(10.0 * la_res, 1e-13 * amax * scale * max(1.0, math.log2(ne)))
    return fwd, res, lapack, la_res
