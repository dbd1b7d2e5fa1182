"""CPU: the rules of the dual Gram solver's size sweep (tests/dual_rules.py) and its fixture
(tests/golden/G9_dual_grid.npz) agree with each other and meet the conditions the GPU tests lean on.  No GPU, no
mpmath: the 60-digit truths are read from the fixture.

The argument path of the entries WITHOUT a dual route (react, multi, subset, step, step_varcoef: n_colloc < M - 2 is
LSSVR_ERR_SOLVER with the entry's own message) is already held without a device by the single-fault tables of
tests/test_capi_cpu.py (_STEP, _STEP_VC, _SUBSET), tests/test_react_cpu.py and tests/test_multi_cpu.py."""
import numpy as np
import pytest

import dual_rules as dr
from oracle import lssvr_oracle as orc


def test_grid_holds_every_class_and_both_sides_of_every_edge():
    assert len(dr.GRID) == 11 * 15 == len(set(dr.GRID))
    cls = {c: [p for p in dr.GRID if dr.kernel_class(*p) == c] for c in dr.CLASSES}
    assert all(cls[c] for c in dr.CLASSES) and sum(map(len, cls.values())) == len(dr.GRID)
    grid = set(dr.GRID)
    # the dispatch itself, restated independently of kernel_class: lanes per element that hold max(n, M)
    for M, n in dr.GRID:
        lanes = next(l for l in (16, 32, 64) if max(M, n) <= l)
        assert dr.kernel_class(M, n) == {16: "g16", 32: "g32", 64: "w64"}[lanes]
    # n and M at edge - 1, edge, edge + 1 of both lane classes, with the other size well inside the class
    for edge, lo, hi in ((16, "g16", "g32"), (32, "g32", "w64")):
        for small in (2, 3):
            for v, want in ((edge - 1, lo), (edge, lo), (edge + 1, hi)):
                assert (small, v) in grid and dr.kernel_class(small, v) == want          # n crosses the edge
                assert (v, small) in grid and dr.kernel_class(v, small) == want          # M crosses the edge
        assert (edge, edge) in grid and (edge + 1, edge + 1) in grid                     # M == n == LPE, and one past
    # the upper limits of the 64-row kernel, and M = 33 with at most 32 points (need = 33: half its rows idle)
    assert {(33, 64), (33, 63), (2, 64), (2, 63), (33, 62)} <= grid
    assert [n for M, n in dr.GRID if M == 33 and n <= 32] == [n for n in dr.NS if n <= 32]
    assert all(dr.kernel_class(33, n) == "w64" for n in dr.NS)
    # the small end: two and three points under the largest degrees, two to four coefficients under few points
    assert {(33, 2), (33, 3), (32, 2), (18, 3), (2, 2), (3, 2), (4, 3), (2, 3)} <= grid
    for bad in ((1, 5), (34, 5), (5, 1), (5, 65)):
        with pytest.raises(ValueError):
            dr.kernel_class(*bad)
    # the corner lists: every class in each, every shard corner a corner
    assert {dr.kernel_class(*p) for p in dr.CORNERS} == set(dr.CLASSES)
    assert [dr.kernel_class(*p) for p in dr.SHARD_CORNERS] == list(dr.CLASSES) and set(dr.SHARD_CORNERS) <= set(dr.CORNERS)
    # the variable-coefficient instantiation is reached only with n < M - 2: one such corner per class
    assert {dr.kernel_class(M, n) for M, n in dr.CORNERS if n < M - 2} == set(dr.CLASSES)


def test_mesh_is_the_stated_one():
    nodes, values, gd = dr.mesh()
    h = np.diff(nodes)
    assert len(nodes) == 10 and nodes[0] == -0.9 and gd == (nodes[0], nodes[-1])
    assert h.min() >= 0.05 and h.max() <= 0.4 and h.max() / h.min() > 2          # non-uniform
    assert 0 < np.abs(values - np.sin(np.pi * nodes)).max() < 5e-2               # the noise is there
    assert values[0] != 0.0 and values[-1] != 0.0                                # the Dirichlet replacement shows
    assert dr.mesh() is dr.mesh() and not nodes.flags.writeable
    lo, hi = dr.wide_domain()
    assert lo < nodes[0] and hi > nodes[-1]
    # systems(): the end elements take the Dirichlet zero on the mesh itself and the nodal value as a window
    s0, _, s8 = dr.systems(5, 16)
    assert s0.g[0] == 0.0 and s8.g[1] == 0.0 and s0.g[1] == values[1]
    s0, _, s8 = dr.systems(5, 16, interior=True)
    assert s0.g[0] == values[0] and s8.g[1] == values[-1]


# every class, both sides of n = M - 2, the extremes of both sizes: 20 pairs
SAMPLE = ((2, 2), (2, 64), (3, 3), (3, 64), (4, 33), (5, 16), (15, 2), (15, 63), (16, 16), (16, 64), (17, 14), (17, 17),
          (18, 15), (31, 30), (32, 17), (32, 32), (33, 2), (33, 31), (33, 33), (33, 64))


@pytest.mark.parametrize("M,n", SAMPLE)
def test_fixture_and_rules_agree(M, n):
    """dual_float64 recomputed here reproduces the stored proto_err up to a factor 2 (it is a rounding-level
    quantity: another BLAS may order its sums differently), against the stored 60-digit truth.  Below 4 u (two bits:
    the rounding of the truth to float64 and of one more operation) the factor is noise, and only that ceiling is asked."""
    assert (M, n) in dr.GRID
    truth, case = dr.fixture().grid(M, n)
    assert truth.shape == (3, M) and np.all(np.isfinite(truth))
    e = dr.proto_err(dr.systems(M, n), truth)
    small = 4 * 2.0 ** -52
    assert (e <= small and case.proto_err <= small) or (0.5 * case.proto_err <= e <= 2 * case.proto_err), \
        (e, case.proto_err)


@pytest.mark.parametrize("M,n", [(16, 3), (32, 17), (33, 12)])
def test_fixture_corner_blocks_agree(M, n):
    """The same for the variable-coefficient truths and the interior-window truths, and the two differ from the
    Poisson ones where they must: another operator, another boundary value."""
    fx = dr.fixture()
    small = 4 * 2.0 ** -52
    tp, _ = fx.corner(M, n)
    tv, cv = fx.corner(M, n, vc=True)
    e = dr.proto_err(dr.systems(M, n, vc=True), tv)
    assert (e <= small and cv.proto_err <= small) or 0.5 * cv.proto_err <= e <= 2 * cv.proto_err
    assert orc.rel_l2_coef(tv, tp).min() > 1e-6          # (far above every bar: a launch of the wrong body shows)
    if (M, n) in dr.GRID:
        assert np.array_equal(tp, fx.grid(M, n)[0])
    if (M, n) in dr.SHARD_CORNERS:
        tw, cw = fx.window(M, n)
        e = dr.proto_err(dr.systems(M, n, interior=True), tw)
        assert (e <= small and cw.proto_err <= small) or 0.5 * cw.proto_err <= e <= 2 * cw.proto_err
        assert np.array_equal(tw[1], tp[1])                                  # element 4 is interior either way
        assert orc.rel_l2_coef(tw[[0, 2]], tp[[0, 2]]).min() > 1e-6          # the ends are not


def test_truth_satisfies_the_boundary_rows():
    """Independent of any solver: B w = g for the stored truths (the Dirichlet zero at the mesh ends)."""
    nodes, values, _ = dr.mesh()
    fx = dr.fixture()
    for M, n in dr.GRID:
        tr, _ = fx.grid(M, n)
        sgn = (-1.0) ** np.arange(M)
        gl = np.array([0.0, values[4], values[8]])
        gr = np.array([values[1], values[5], 0.0])
        assert np.abs(tr @ sgn - gl).max() < 1e-13 and np.abs(tr.sum(1) - gr).max() < 1e-13, (M, n)


def test_caps_hold_for_the_fixture():
    """At most 15 % of GRID outside the envelope, none of them on the production route n <= M - 2; every bar is
    the floor or ten times the restatement's own error, and no bar of a checked case is looser than 1e-7."""
    cases = dr.fixture().cases()
    assert len(cases) == len(dr.GRID) and all(np.isfinite(c.proto_err) and c.proto_err >= 0 for c in cases)
    outside = [c for c in cases if not dr.in_envelope(c)]
    assert len(outside) <= dr.CAP * len(cases), [(c.M, c.n, c.proto_err) for c in outside]
    assert not [c for c in outside if c.n <= c.M - 2]
    for c in cases:
        assert dr.bar(c) == max(1e-12 if c.M <= 22 else 5e-11, 10 * c.proto_err)
        assert not dr.in_envelope(c) or dr.bar(c) <= 10 * dr.ENVELOPE
    fx = dr.fixture()
    for M, n in dr.CORNERS:
        assert dr.in_envelope(fx.corner(M, n)[1])
        assert n >= M - 2 or dr.in_envelope(fx.corner(M, n, vc=True)[1])
    for M, n in dr.SHARD_CORNERS:
        assert dr.in_envelope(fx.window(M, n)[1])


def test_restatement_variants_share_one_function():
    """scripts/proto/dual_projected.py's first prototype (w recomputed from lam) and the kernels' arrangement
    (carried w, safeguard, re-projection) are options of one function; on a benign case both reach the truth, and
    the carried form holds the boundary rows to the last bit or two."""
    truth, _ = dr.fixture().grid(17, 14)
    for s, t in zip(dr.systems(17, 14), truth):
        plain = orc.solve_dual_projected(s, refine=3)
        carried = dr.dual_float64(s)
        assert orc.rel_l2_coef(plain[None], t[None])[0] < 1e-13
        assert orc.rel_l2_coef(carried[None], t[None])[0] < 1e-13
        assert np.abs(s.B @ carried - s.g).max() <= 4e-16 * np.abs(s.B).sum(1).max() * np.abs(carried).max()
