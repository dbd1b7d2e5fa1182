"""CPU: the rules of tests/flux_rules.py -- the long-double reference of the flux prefix-scan solve, its shard
aggregates and the constant of the bar -- pinned without a GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import flux_rules as fr

LD = np.longdouble
U_LD = 2.0 ** -64                    # unit roundoff of the long double
SMALL = (1, 2, 3, 37, 300)


def _bands_ld(kloc):
    """(diag[ne+1], off[ne]) of D^T K D assembled in long double from the float64 kloc."""
    k = np.asarray(kloc, dtype=LD)
    diag = np.zeros(len(k) + 1, dtype=LD)
    diag[:-1] += k
    diag[1:] += k
    return diag, -k


def _thomas(diag, off, load, u0, u1, zero, div=lambda a, b: a / b):
    """Dirichlet ends eliminated into their neighbours, Thomas elimination without pivoting, in the type of the
    arguments."""
    n = len(diag)
    u = [zero] * n
    u[0], u[-1] = u0, u1
    m = n - 2
    if m <= 0:
        return u
    d = [diag[i] for i in range(1, n - 1)]
    r = [load[i] for i in range(1, n - 1)]
    r[0] = r[0] - off[0] * u0
    r[-1] = r[-1] - off[-1] * u1
    for i in range(1, m):
        w = div(off[i], d[i - 1])
        d[i] = d[i] - w * off[i]
        r[i] = r[i] - w * r[i - 1]
    x = [zero] * m
    x[-1] = div(r[-1], d[-1])
    for i in range(m - 2, -1, -1):
        x[i] = div(r[i] - off[i + 1] * x[i + 1], d[i])
    u[1:-1] = x
    return u


def _thomas_bound(kloc, u):
    """Forward error bound of the long-double Thomas solve, node by node.  The interior matrix A is a symmetric
    M-matrix, for which the computed solution solves (A + dA) x = b exactly with |dA| <= (4u + O(u^2)) |A|
    (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 9.12 with |L||U| = |LU|); rounding
    diag = k_{i-1} + k_i to the 64-bit mantissa and the two end terms of the right-hand side are perturbations of the
    same kind, u each.  Hence |dx| <= 6u |A^-1| |A| |x| to first order; taken at 8u.  A^-1 is the Green's function
    G_ij = R_min(i,j) (R_ne - R_max(i,j)) / R_ne, R_m = sum_{e<m} 1/k_e."""
    k = np.asarray(kloc, dtype=np.float64)
    ne = len(k)
    R = np.concatenate([[0.0], np.cumsum(1.0 / k)])
    i = np.arange(1, ne)
    G = np.minimum.outer(R[i], R[i]) * (R[-1] - np.maximum.outer(R[i], R[i])) / R[-1]
    ua = np.abs(np.asarray(u, dtype=np.float64))
    Ax = (k[:-1] + k[1:]) * ua[1:-1] + k[:-1] * ua[:-2] + k[1:] * ua[2:]       # |A| |x| with the end values
    out = np.zeros(ne + 1)
    out[1:-1] = 8 * U_LD * (G @ Ax)
    return out


@pytest.mark.parametrize("name", fr.NAMES)
@pytest.mark.parametrize("ne", SMALL)
def test_reference_matches_long_double_thomas(ne, name):
    """The three sums against an elimination of the assembled bands D^T K D in long double: another algorithm on the
    same data.  The bar is the elimination's own forward bound plus the reference's EPS/16 * scale."""
    kloc, load, u_ref, scale = fr.case(ne, name)
    diag, off = _bands_ld(kloc)
    l = np.asarray(load, dtype=LD)
    u = np.array(_thomas(diag, off, l, LD(fr.U0), LD(fr.U1), LD(0)), dtype=LD)
    bound = _thomas_bound(kloc, u_ref) + (fr.EPS / 16) * scale.astype(np.float64)
    err = np.abs(u - u_ref).astype(np.float64)
    assert not np.isnan(err).any()
    assert np.all(err <= bound), (float(np.max(err - bound)), int(np.argmax(err - bound)))


def _frac(v):
    return Fraction(*v.as_integer_ratio())


@pytest.mark.parametrize("name", fr.NAMES)
@pytest.mark.parametrize("ne", SMALL)
def test_reference_within_its_stated_accuracy_of_the_exact_solution(ne, name):
    """The same elimination in exact rational arithmetic (every float64 is a rational): the reference is within
    EPS/16 * scale of the exact solution of D^T K D u = load, the accuracy flux_rules claims for it -- and the last
    node, which the reference leaves to the formula, comes out as u1 to that accuracy."""
    kloc, load, u_ref, scale = fr.case(ne, name)
    k = [_frac(np.float64(v)) for v in kloc]
    diag = [Fraction(0)] * (ne + 1)
    for e in range(ne):
        diag[e] += k[e]
        diag[e + 1] += k[e]
    l = [Fraction(0)] + [_frac(np.float64(v)) for v in load[1:-1]] + [Fraction(0)]
    u = _thomas(diag, [-v for v in k], l, Fraction(fr.U0), Fraction(fr.U1), Fraction(0))
    for m in range(ne + 1):
        assert abs(_frac(u_ref[m]) - u[m]) <= Fraction(fr.EPS / 16) * _frac(scale[m]), m


@pytest.mark.parametrize("name", fr.NAMES)
def test_zero_load_formula_and_blocked_sums(name):
    """The blocked running sum against math.fsum (exact, correctly rounded) at the block edges, and the closed
    formula of the zero-load problem against the reference."""
    kloc, load, u_ref, scale = fr.case(2049, name)
    x = 1.0 / kloc
    c = fr.blocked_cumsum(x)
    for m in (1, 63, 64, 65, 128, 1000, 2048, 2049):
        exact = math.fsum(x[:m])
        assert abs(float(c[m - 1] - LD(exact))) <= (2.0 ** -53 + 2.0 ** -56) * exact      # fsum's rounding to float64 + ours
    if name == "zero_load":
        f = fr.zero_load_formula(kloc, fr.U0, fr.U1)
        assert fr.ratio(f, u_ref, scale) <= 1.0 / 8


@pytest.mark.parametrize("name", fr.NAMES)
@pytest.mark.parametrize("ne", (2, 37, 300, 2049))
def test_shard_aggregates_combine_to_the_whole(ne, name):
    """Cut at random nodes, one aggregate per piece, combined in order: the whole mesh's aggregate to long-double
    rounding.  The bar: 2^-56 (the blocked sums' worst case, twice: pieces and whole; the few combines add 2^-64
    each) of the sum of the absolute values of the terms l_j / k_e of each component."""
    kloc, load = fr.problems(ne, name, poison=False)
    rng = np.random.default_rng([11, ne])
    k, l = kloc.astype(LD), load[:ne].astype(LD).copy()
    l[0] = 0
    absum = (np.sum(np.abs(l)), np.sum(1 / k), np.sum(fr.blocked_cumsum(np.abs(l)) / k))
    whole = fr.shard_aggregate(kloc, load, True)
    for ncut in (1, 3, 7):
        if ncut >= ne:
            continue
        c = [0] + sorted(int(i) for i in rng.choice(np.arange(1, ne), ncut, replace=False)) + [ne]
        acc = None
        for s0, s1 in zip(c[:-1], c[1:]):
            piece = fr.shard_aggregate(kloc[s0:s1], load[s0:s1 + 1], s0 == 0)
            acc = piece if acc is None else fr.combine(acc, piece)
        for got, want, sc in zip(acc, whole, absum):
            assert abs(got - want) <= 2.0 ** -55 * sc
    # dropping a later shard's load[0] is not within that bar: the check can fail
    if ne > 2 and name != "zero_load":
        s0 = ne // 3
        wrong = fr.combine(fr.shard_aggregate(kloc[:s0], load[:s0 + 1], True),
                           fr.shard_aggregate(kloc[s0:], load[s0:], True))
        assert abs(wrong[0] - whole[0]) > 2.0 ** -55 * absum[0]


def test_whole_aggregate_is_the_reference_sums():
    """shard_aggregate of the whole mesh gives the q_0 of the reference: u_1 = u0 + q_0 / k_0."""
    kloc, load, u_ref, scale = fr.case(300, "layered")
    a, r, g = fr.shard_aggregate(kloc, load, True)
    q0 = ((LD(fr.U1) - LD(fr.U0)) + g) / r
    assert abs((LD(fr.U0) + q0 / LD(kloc[0])) - u_ref[1]) <= (fr.EPS / 16) * scale[1]


def test_bar_constant_is_four_times_the_emulated_scan():
    """BAR_C = ceil(4 x the largest err / (EPS * scale) of the float64 Hillis-Steele scan over the GPU matrix), and
    hence every case of the matrix is reachable by a correct float64 scan with a factor 4 to spare."""
    worst = 0.0
    for name in fr.NAMES:
        for ne in fr.SIZES:
            kloc, load, u_ref, scale = fr.case(ne, name)
            u = fr.emulated_scan(kloc, load, fr.U0, fr.U1)
            assert u[0] == fr.U0 and u[-1] == fr.U1 and not np.isnan(u).any()
            r = fr.ratio(u, u_ref, scale)
            assert r <= fr.BAR_C, (name, ne, r)
            worst = max(worst, r)
    assert fr.BAR_C == math.ceil(4 * worst), worst


def test_plain_long_double_cumsum_is_not_a_reference():
    """Why the sums are blocked: on the uniform mesh with a standard-normal load at 1e6 elements a sequential
    long-double cumsum is more than one bar away from the blocked reference (18.5 EPS * scale), which the float64 scan
    agrees with to a quarter of the bar (0.54)."""
    ne = 1000003
    h = np.full(ne, 2.0 / ne)
    kloc = 1.0 / h
    load = np.random.default_rng(0).standard_normal(ne + 1) * h[0]
    u_ref, scale = fr.reference(kloc, load, fr.U0, fr.U1)
    k, l = kloc.astype(LD), load[:ne].astype(LD).copy()
    l[0] = 0
    S, R = np.cumsum(l), np.cumsum(1 / k)
    T = np.cumsum(S / k)
    q0 = ((LD(fr.U1) - LD(fr.U0)) + T[-1]) / R[-1]
    u_seq = np.concatenate([[LD(fr.U0)], (LD(fr.U0) + q0 * R) - T])
    assert fr.ratio(u_seq[:-1], u_ref[:-1], scale[:-1]) > fr.BAR_C
    assert fr.ratio(fr.emulated_scan(kloc, load, fr.U0, fr.U1), u_ref, scale) <= fr.BAR_C / 4


def test_shard_cut_lists():
    """The cut lists of the GPU shard test are what its docstring says, and the boosted nodes are the shard starts."""
    assert fr.cuts(9, "tile_edge") is None and fr.cuts(9, "in_thread") is None
    assert fr.cuts(2049, "tile_edge") == (1024,) and fr.cuts(2049, "in_thread") == (1022, 1027)
    assert fr.cuts(263170, "thirds") == (87723, 175446) and fr.cuts(9, "last_one") == (8,)
    for ne in fr.SHARD_SIZES:
        c = fr.cuts(ne, "random7")
        assert len(set(c)) == 7 and 0 < c[0] and c[-1] < ne
        assert set(c) <= set(fr.shard_boost(ne))
    assert len(fr.shard_matrix()) == 2 * (4 + 6 + 6)
