"""numpy restatement of the flux prefix-scan Dirichlet solve (csrc/flux_solve.hip: lssvr_p1_flux_solve,
lssvr_p1_flux_aggregate, lssvr_p1_flux_finish), its error scale, and the problems the tests share.  A plain module, no
GPU and no torch: tests/test_flux_cpu.py pins it to an elimination of the assembled system, tests/test_gpu_flux.py
compares the kernels with it.

With k_e = abar_e / h_e, l_0 = 0 and l_e = load_e (the header comment of flux_solve.hip):
    S_e = sum_{j<=e} l_j,   R_m = sum_{e<m} 1/k_e,   T_m = sum_{e<m} S_e/k_e,
    q_0 = (u1 - u0 + T_ne) / R_ne,      u_m = u0 + q_0 R_m - T_m.
The three sums are one scan of (a1,r1,g1) o (a2,r2,g2) = (a1+a2, r1+r2, g1+g2 + r2*a1) over the elements
(l_e, 1/k_e, l_e/k_e); the value after element e is (S_e, R_{e+1}, T_{e+1}).

THE ERROR SCALE.  A float64 evaluation of the three sums in any association is measured against
    scale_m = |u0| + |q_0| R_m + sum_{e<m} |S_e|/k_e + (R_m/R_ne) (sum_{e<ne} |S_e|/k_e + |q_0| R_ne),
the last term being the error of q_0 carried into node m.  Every bar of the flux tests is BAR_C * EPS * scale_m.

THE REFERENCE'S OWN ERROR.  The sums are taken in long double (64-bit mantissa) as recursive blocked sums: the running
sum inside blocks of 64, the running sum of the block totals, recursively.  A term then passes through at most
levels * 64 additions, levels = ceil(log_64 n) <= 4 below 1.6e7 terms, so the worst case is levels * 64 * 2^-64 <=
2^-56 = EPS / 16 of the sum of the absolute values -- every size.  A sequential long-double cumsum is NOT enough: its
worst case grows like n * 2^-64, and adding the same 1/k_e a million times rounds the same way a million times.  On the
uniform mesh with a standard-normal load it is 0.003 EPS * scale from the blocked sums at 262145 elements and 18.5 at
1000003, where a float64 tree scan is within 0.54 of the blocked sums (tests/test_flux_cpu.py keeps both figures)."""
import functools
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
if not np.finfo(LD).eps < 2e-19:
    raise RuntimeError("flux_rules needs a long double with a 64-bit mantissa (eps %.3g found): the reference would be "
                       "no more accurate than the float64 scan it judges" % float(np.finfo(LD).eps))

U0, U1 = 0.25, -0.5
BLOCK = 64

# The GPU matrix: the per-thread item boundary (4 elements a thread), one tile (1024) exactly and +-1, two tiles + 1,
# 256 tiles exactly and +-1 (the first carry iteration of the aggregate scan, 1-element tail), 257 tiles + 2 (1026-element
# tail).
SIZES = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2049, 262143, 262144, 262145, 263170)
NAMES = ("uniform", "graded", "graded_rev", "layered", "zero_load")

# BAR_C = 4 x the largest err / (EPS * scale) that `emulated_scan` (a float64 Hillis-Steele scan of the operator over
# the whole array, judged by the blocked long-double reference) shows over NAMES x SIZES, rounded up to an integer:
# the largest is 1.83 (layered, ne = 1023; the next are 1.18 at graded_rev, ne = 262143, and 1.15 at layered,
# ne = 262143; the uniform problem stays below 0.69), 4 x 1.83 = 7.3 -> 8.  The factor 4 is for the kernel's different
# association (4 sequential items a thread, three scan levels).  tests/test_flux_cpu.py recomputes the maximum and
# holds the constant to this sentence.
BAR_C = 8


# --------------------------------------------------------------------------
# sums
# --------------------------------------------------------------------------
def blocked_cumsum(x):
    """Inclusive running sum of a long-double vector by recursive blocks of BLOCK (see the module docstring)."""
    x = np.asarray(x, dtype=LD)
    n = len(x)
    if n <= BLOCK:
        return np.cumsum(x, dtype=LD)
    nb = -(-n // BLOCK)
    pad = np.zeros(nb * BLOCK, dtype=LD)
    pad[:n] = x
    inner = np.cumsum(pad.reshape(nb, BLOCK), axis=1, dtype=LD)
    before = np.zeros(nb, dtype=LD)
    before[1:] = blocked_cumsum(inner[:, -1])[:-1]
    return (inner + before[:, None]).reshape(-1)[:n]


def _terms(kloc, load, first_global):
    k = np.asarray(kloc, dtype=LD)
    l = np.array(np.asarray(load)[:len(k)], dtype=LD)
    if first_global:
        l[0] = 0
    return k, l


def combine(x, y):
    """(a1,r1,g1) o (a2,r2,g2), x first: the operator of flux_solve.hip in whatever type the operands have."""
    return (x[0] + y[0], x[1] + y[1], (x[2] + y[2]) + y[1] * x[0])


def shard_aggregate(kloc, load, first_global):
    """(a, r, g) of a shard in long double: (S, R, T) over its own elements, l_0 = 0 when ``first_global``, else
    load[0] counts.  load[len(kloc)] is not read."""
    k, l = _terms(kloc, load, first_global)
    S = blocked_cumsum(l)
    return S[-1], blocked_cumsum(1 / k)[-1], blocked_cumsum(S / k)[-1]


def shard_aggregate_abs(kloc, load, first_global):
    """The sum of the absolute values of the terms of each component of :func:`shard_aggregate`: (sum |l_e|,
    sum 1/k_e, sum |S_e|/k_e) -- what a rounding error of a float64 evaluation is measured against."""
    k, l = _terms(kloc, load, first_global)
    S = blocked_cumsum(l)
    return blocked_cumsum(np.abs(l))[-1], blocked_cumsum(1 / k)[-1], blocked_cumsum(np.abs(S) / k)[-1]


def reference(kloc, load, u0, u1):
    """(u[ne+1], scale[ne+1]) in long double; load[0] and load[ne] are not read.  u[0] = u0, and u[ne] is the formula's
    value (u1 up to the reference's own rounding)."""
    k, l = _terms(kloc, load, True)
    u0, u1 = LD(u0), LD(u1)
    S = blocked_cumsum(l)
    R = blocked_cumsum(1 / k)
    T = blocked_cumsum(S / k)
    Tabs = blocked_cumsum(np.abs(S) / k)
    q0 = ((u1 - u0) + T[-1]) / R[-1]
    u = np.concatenate([[u0], (u0 + q0 * R) - T])
    scale = np.concatenate([[abs(u0)], abs(u0) + abs(q0) * R + Tabs + (R / R[-1]) * (Tabs[-1] + abs(q0) * R[-1])])
    return u, scale


def zero_load_formula(kloc, u0, u1):
    """u_m = u0 + (u1 - u0) R_m / R_ne in long double: the solution with no load."""
    R = blocked_cumsum(1 / np.asarray(kloc, dtype=LD))
    return np.concatenate([[LD(u0)], LD(u0) + (LD(u1) - LD(u0)) * (R / R[-1])])


def emulated_scan(kloc, load, u0, u1):
    """float64 u[ne+1] by a Hillis-Steele scan of the operator over the whole array: a balanced association, not the
    kernel's exact order.  Sets BAR_C.  The ends are u0 and u1 as the kernel writes them."""
    k = np.asarray(kloc, dtype=np.float64)
    ne = len(k)
    l = np.array(np.asarray(load, dtype=np.float64)[:ne])
    l[0] = 0.0
    a, r, g = l, 1.0 / k, l * (1.0 / k)
    off = 1
    while off < ne:
        a2, r2, g2 = a.copy(), r.copy(), g.copy()
        a2[off:], r2[off:], g2[off:] = combine((a[:-off], r[:-off], g[:-off]), (a[off:], r[off:], g[off:]))
        a, r, g = a2, r2, g2
        off *= 2
    q0 = ((u1 - u0) + g[-1]) / r[-1]
    u = np.concatenate([[u0], (u0 + q0 * r) - g])
    u[-1] = u1
    return u


def ratio(u, u_ref, scale):
    """max_m |u_m - u_ref_m| / (EPS * scale_m), the figure every bar is a multiple of (0 where scale is 0)."""
    err = np.abs(np.asarray(u).astype(LD) - u_ref)
    if np.isnan(err).any():
        return math.inf
    ok = scale > 0
    return float(max(np.max(err[ok] / (EPS * scale[ok]), initial=0.0), math.inf if np.any(err[~ok] > 0) else 0.0))


# --------------------------------------------------------------------------
# problems
# --------------------------------------------------------------------------
def _mesh(ne, name):
    """(h[ne], abar[ne]) of a mesh of length 2."""
    rng = np.random.default_rng([NAMES.index(name if name != "zero_load" else "layered"), ne])
    if name == "uniform":
        return np.full(ne, 2.0 / ne), np.ones(ne)
    if name in ("graded", "graded_rev"):
        h = np.geomspace(1.0, 1e-6, ne)
        h *= 2.0 / h.sum()
        return (h[::-1].copy() if name == "graded_rev" else h), np.ones(ne)
    h = rng.uniform(0.2, 1.0, ne)
    h *= 2.0 / h.sum()
    return h, 10.0 ** rng.uniform(-3.0, 3.0, ne)


def problems(ne, name, boost=(), poison=True):
    """(kloc[ne], load[ne+1]) in float64, built from h and abar directly.
      uniform     the uniform mesh of (-1, 1), a = 1, the 2-point Gauss load of f = pi^2 sin(pi x)
      graded      h = geomspace(1, 1e-6, ne) scaled to length 2, a = 1: a boundary layer as refinement leaves it
      graded_rev  the same mesh reversed
      layered     h ~ U(0.2, 1) scaled to length 2, abar = 10**U(-3, 3) per element
      zero_load   the layered k with load = 0
    The loads that are not the Poisson one or zero are standard normal x nodal h (fixed seeds, changing sign).
    ``boost``: nodes whose load is multiplied by 1e3 (the first nodes of later shards).  ``poison``: load[0] and
    load[ne] are NaN -- the solve must not use the first and never reads the last."""
    h, abar = _mesh(ne, name)
    kloc = abar / h
    if name == "uniform":
        from oracle import lssvr_oracle as orc
        nodes = np.linspace(-1.0, 1.0, ne + 1)
        kloc, fl, fr = orc.p1_assemble_local(nodes)
        load = orc.p1_scatter(kloc, fl, fr)[2]
    elif name == "zero_load":
        load = np.zeros(ne + 1)
    else:
        rng = np.random.default_rng([100 + NAMES.index(name), ne])
        hn = np.concatenate([[h[0]], 0.5 * (h[:-1] + h[1:]), [h[-1]]])
        load = rng.standard_normal(ne + 1) * hn
    for i in boost:
        load[i] *= 1e3
    if poison:
        load[0] = load[ne] = np.nan
    return kloc, load


@functools.lru_cache(maxsize=None)
def case(ne, name, boost=()):
    """(kloc, load, u_ref, scale) of ``problems(ne, name, boost)`` with the ends (U0, U1): computed once and shared,
    read-only."""
    kloc, load = problems(ne, name, boost)
    u, scale = reference(kloc, load, U0, U1)
    for t in (kloc, load, u, scale):
        t.setflags(write=False)
    return kloc, load, u, scale


# --------------------------------------------------------------------------
# shards
# --------------------------------------------------------------------------
SHARD_SIZES = (9, 2049, 263170)
SHARD_NAMES = ("graded", "layered")
CUT_KINDS = ("thirds", "first_one", "last_one", "tile_edge", "in_thread", "random7")


def cuts(ne, kind):
    """Interior cut nodes of a cut list, ascending, or None where the mesh is too short for it (the tile-edge lists need
    more than 1027 elements)."""
    if kind == "thirds":
        c = [ne // 3, 2 * ne // 3]
    elif kind == "first_one":
        c = [1]
    elif kind == "last_one":
        c = [ne - 1]
    elif kind == "tile_edge":
        c = [1024]
    elif kind == "in_thread":
        c = [1022, 1027]
    else:
        c = sorted(int(i) for i in np.random.default_rng([7, ne]).choice(np.arange(1, ne), 7, replace=False))
    return tuple(c) if c[-1] < ne else None


def shard_matrix():
    return [(ne, name, kind) for ne in SHARD_SIZES for name in SHARD_NAMES for kind in CUT_KINDS
            if cuts(ne, kind) is not None]


def shard_boost(ne):
    """Every node at which some cut list of this size starts a shard: their loads are x 1e3 in the shard problems, so
    that a dropped load[0] of a later shard stands far above the bar, and one reference serves all cut lists."""
    return tuple(sorted({c for kind in CUT_KINDS for c in (cuts(ne, kind) or ())}))
