"""CPU: the oracle pinned against the golden vectors generated from the reference
(tests/golden/*.npz, made by oracle/gen_golden.py in the build container).

The reference ships no tests or fixtures of its own; these vectors
hold, per element, the reference's SLSQP output and the 60-digit minimiser of the same QP."""
import numpy as np
import pytest

from oracle import lssvr_oracle as orc
from oracle import closed_form_mp as cf

CASES = [
    ("G1_c1_ne8_M5_n5", 3e-10),
    ("G2_default_ne24_M8_n12", 1e-10),
    ("G3_ne24_M9_n16", 1e-10),
    ("G4_ne4096_M9_n16", 1e-10),
    ("G5_ne24_M33_n64", 1e-10),
    ("G6a_wide_ne100008_M9_n16", 1e-10),
    ("G6b_wide_ne10000008_M9_n16", 2e-10),
    ("G8_classdefaults_ne4_M12_n12", 3e-10),
]


def _systems(g):
    lo, hi, ne = float(g["lo"]), float(g["hi"]), int(g["ne"])
    M, n, gamma = int(g["M"]), int(g["n"]), float(g["gamma"])
    for k, e in enumerate(g["elements"]):
        a, b = g["nodes_sel"][k]
        ul, ur = g["values_sel"][k]
        gl, gr = orc.boundary_values(int(e), ne, a, b, ul, ur, (lo, hi))
        yield k, orc.element_system(a, b, gl, gr, M, gamma, n)


@pytest.mark.parametrize("name,tol_ref", CASES)
def test_closed_forms_vs_golden(golden, name, tol_ref):
    g = golden(name)
    nodes = np.linspace(float(g["lo"]), float(g["hi"]), int(g["ne"]) + 1)
    assert np.array_equal(nodes[g["elements"]], g["nodes_sel"][:, 0])        # node indices exact
    assert np.array_equal(nodes[g["elements"] + 1], g["nodes_sel"][:, 1])
    for k, s in _systems(g):
        w_bce = orc.solve_bc_eliminated(s)        # the algorithm of the HIP kernels
        w_kkt = orc.solve_primal_kkt(s)
        assert orc.rel_l2_coef(w_bce, g["coef_truth"][k]) <= 1e-13
        assert orc.rel_l2_coef(w_kkt, g["coef_truth"][k]) <= 1e-13
        assert orc.rel_l2_coef(w_bce, g["coef_ref"][k]) <= tol_ref
    # the reference itself sits this far from the exact minimiser
    assert orc.rel_l2_coef(g["coef_ref"], g["coef_truth"]).max() <= tol_ref


@pytest.mark.skipif(not cf.HAVE_MP, reason="mpmath missing")
@pytest.mark.parametrize("name", ["G1_c1_ne8_M5_n5", "G3_ne24_M9_n16", "G6b_wide_ne10000008_M9_n16"])
def test_truth_regenerates(golden, name):
    g = golden(name)
    for k, s in list(_systems(g))[:3]:
        assert orc.rel_l2_coef(cf.solve_truth(s), g["coef_truth"][k]) <= 1e-15


def test_dual_gram_form_accuracy(golden):
    """north_star's (n+2) Gram form: fine at h = 1/12, visibly worse on config 1
     -- which is why it is not the default solver."""
    g = golden("G3_ne24_M9_n16")
    errs = [orc.rel_l2_coef(orc.solve_dual_gram(s), g["coef_truth"][k]) for k, s in _systems(g)]
    assert max(errs) <= 1e-12
    g1 = golden("G1_c1_ne8_M5_n5")
    errs1 = [orc.rel_l2_coef(orc.solve_dual_gram(s), g1["coef_truth"][k]) for k, s in _systems(g1)]
    assert max(errs1) <= 1e-8


def test_slsqp_restatement_reproduces_reference(golden):
    """The CPU baseline (per-element SLSQP loop) against the reference's own output."""
    g = golden("G3_ne24_M9_n16")
    nodes = np.linspace(-1, 1, 25)
    vals = np.concatenate([g["values_sel"][:, 0], g["values_sel"][-1:, 1]])
    C, ok = orc.slsqp_loop(nodes, vals, 9, 1e4, 16, elements=[0, 11, 23])
    assert ok.all()
    assert orc.rel_l2_coef(C, g["coef_ref"][[0, 11, 23]]).max() <= 1e-10
    assert orc.rel_l2_coef(C, g["coef_truth"][[0, 11, 23]]).max() <= 1e-10


def test_numpy_arithmetic_restatements():
    rng = np.random.default_rng(0)
    for _ in range(50):
        a = rng.uniform(-1e6, 1e6)
        b = a + rng.uniform(1e-7, 10)
        n = int(rng.integers(2, 70))
        assert np.array_equal(orc.np_linspace(a, b, n), np.linspace(a, b, n))
    from numpy.polynomial import polyutils as pu
    from numpy.polynomial.legendre import Legendre, legval
    off, scl = orc.mapparms(0.3, 0.7)
    assert (off, scl) == tuple(pu.mapparms([0.3, 0.7], [-1, 1]))
    c = rng.standard_normal(9)
    t = rng.uniform(-1, 1, 33)
    assert np.array_equal(orc.clenshaw(t, c), legval(t, c))
    # PDE rows through legder + legval == -scl^2 L'' to rounding, both recurrences
    A = orc.legendre_rows_reference(0.3, 0.7, 9, np.linspace(0.3, 0.7, 16))
    s = orc.element_system(0.3, 0.7, 0.0, 0.0, 9, 1e4, 16)
    assert np.max(np.abs(A - s.scl ** 2 * s.Ahat)) <= 1e-13 * np.max(np.abs(A))
    assert np.max(np.abs(orc.gegenbauer_d2(s.t, 9) + s.Ahat)) <= 1e-13 * np.max(np.abs(s.Ahat))
    L, D1, D2 = orc.legendre_tables(s.t, 9)
    assert np.max(np.abs(orc.gegenbauer_d1(s.t, 9) - D1)) <= 1e-13 * np.max(np.abs(D1))
    u = Legendre(c, [0.3, 0.7])
    assert np.allclose(-u.deriv(2)(s.x), s.scl ** 2 * (s.Ahat @ c), rtol=1e-12)


def test_evaluate_solution_vs_reference(golden):
    g = golden("G7_eval_default")
    u, elem = orc.evaluate_solution(g["nodes"], g["W"], g["xq"])
    assert np.array_equal(elem, g["elem"])
    assert np.array_equal(u, g["u_ref"])
    uv, ev = orc.evaluate_solution_vec(g["nodes"], g["W"], g["xq"])
    assert np.array_equal(ev, g["elem"]) and np.array_equal(uv, g["u_ref"])
    assert np.array_equal(orc.locate_elements_scan(g["nodes"], g["xq"]), g["elem"])


def test_p1_fem_analytic_pins():
    """scikit-fem is absent: the P1 step is pinned by the analytic tridiagonal system and by
    the manufactured solution."""
    nodes = np.linspace(-1, 1, 25)
    kd, fl, fr = orc.p1_assemble_local(nodes)
    assert np.allclose(kd, 12.0)
    diag, off, load = orc.p1_scatter(kd, fl, fr)
    assert np.allclose(diag[1:-1], 24.0) and np.allclose(off, -12.0)
    u = orc.thomas_dirichlet(diag, off, load)
    assert abs(np.max(np.abs(u - np.sin(np.pi * nodes))) - 3.274e-6) < 2e-9
    assert np.max(np.abs(orc.banded_dirichlet(diag, off, load) - u)) < 1e-14
    n8 = np.linspace(-1, 1, 9)
    u8 = orc.fem_p1_solve(n8)
    assert abs(np.max(np.abs(u8 - np.sin(np.pi * n8))) - 2.731e-4) < 2e-7
    # hybrid accuracy of SURVEY.md Appendix B.1 (reference demo configuration)
    W, st = orc.enhance_all(nodes, u, 8, 1e4, 12)
    xq = np.linspace(-1, 1, 201)
    uq, _ = orc.evaluate_solution(nodes, W, xq)
    ex = orc.true_solution(xq)
    assert abs(np.linalg.norm(uq - ex) / np.linalg.norm(ex) - 3.255e-6) < 5e-9
    assert np.all(st == 0)


def test_batched_oracle_equals_loop():
    rng = np.random.default_rng(5)
    nodes = np.cumsum(np.concatenate([[0.0], rng.uniform(0.01, 0.2, 40)]))
    vals = rng.standard_normal(41)
    for M, n in ((5, 5), (9, 16), (12, 12)):
        Wl, _ = orc.enhance_all(nodes, vals, M, 1e4, n, solver="primal")
        Wv = orc.enhance_all_vec(nodes, vals, M, 1e4, n)
        assert orc.rel_l2_coef(Wv, Wl).max() <= 1e-13


# --------------------------------------------------------------------------------------------
# recipe <-> data: the committed fixtures regenerate, and the reference's loop reproduces them
# --------------------------------------------------------------------------------------------
ALL_FIXTURES = [c[0] for c in CASES]


@pytest.mark.parametrize("name", [c for c in ALL_FIXTURES if "10000008" not in c] + ["G7_eval_default"])
def test_golden_inputs_regenerate_bit_for_bit(golden, name):
    """oracle/gen_golden.py takes nodal values from the FROZEN stand-in ``fem_p1_solve_golden_v1``:
    what it would write today equals the stored inputs bit for bit (the living ``fem_p1_solve`` is
    3e-11 away at 1e5 elements).  G6b's 1e7-node Thomas loop (30 s) is left to ``gen_golden.py --verify``."""
    g = golden(name)
    if "elements" not in g:
        assert np.array_equal(orc.fem_p1_solve_golden_v1(g["nodes"]), g["values"])
        return
    nodes = np.linspace(float(g["lo"]), float(g["hi"]), int(g["ne"]) + 1)
    v = orc.fem_p1_solve_golden_v1(nodes)
    e = g["elements"]
    assert np.array_equal(nodes[e], g["nodes_sel"][:, 0]) and np.array_equal(nodes[e + 1], g["nodes_sel"][:, 1])
    assert np.array_equal(v[e], g["values_sel"][:, 0]) and np.array_equal(v[e + 1], g["values_sel"][:, 1])


def _rerun_on_stored_inputs(g, limit=None):
    """``lssvr_primal`` (Dual.py:20-98) as ``orc.slsqp_element`` restates it step for step, on a fixture's
    STORED inputs, numpy's global RNG seeded per element exactly as ``oracle/gen_golden.py`` seeded it
    (``1234 + i``): the start vector, the constraint rows and the SLSQP call are the reference's own."""
    lo, hi, ne = float(g["lo"]), float(g["hi"]), int(g["ne"])
    M, n, gamma = int(g["M"]), int(g["n"]), float(g["gamma"])
    out = []
    for k, i in enumerate(g["elements"][:limit]):
        np.random.seed(1234 + int(i) % 100000)
        c, _ = orc.slsqp_element(orc.poisson_rhs, g["nodes_sel"][k, 0], g["nodes_sel"][k, 1],
                                 g["values_sel"][k, 0], g["values_sel"][k, 1], M, gamma, n,
                                 left=(int(i) == 0), right=(int(i) == ne - 1), global_domain=(lo, hi))
        out.append(c)
    return np.array(out)


@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_reference_rerun_on_stored_inputs_is_bit_equal(golden, name):
    """The reference's element solve, restated in the oracle and run on the inputs each fixture stores with
    the seeds the generator used, returns ``coef_ref`` -- the reference's own output -- bit for bit: the
    restatement IS the reference on these inputs, and the committed recipe reproduces the committed data.
    (Degree 32 costs 7 s per element: one of G5's three elements here.  ``oracle/gen_golden.py --verify``
    reruns the reference itself on every element where its source is at hand.)"""
    g = golden(name)
    limit = 1 if int(g["M"]) > 20 else None
    got = _rerun_on_stored_inputs(g, limit=limit)
    assert len(got) >= 1 and np.array_equal(got, g["coef_ref"][:len(got)])


def test_reference_rerun_eval_case_is_bit_equal(golden):
    """G7: the reference's loop over all 24 elements (``solve_lssvr_subproblems``, Dual.py:139-169: one
    global seed, 777, for the whole loop) through the restatement, then ``evaluate_solution``: the stored
    coefficients and the stored u(x) -- NaN at the NaN probe included -- bit for bit."""
    g = golden("G7_eval_default")
    nodes, values = g["nodes"], g["values"]
    ne = len(nodes) - 1
    np.random.seed(777)
    W = np.array([orc.slsqp_element(orc.poisson_rhs, nodes[i], nodes[i + 1], values[i], values[i + 1],
                                    int(g["M"]), float(g["gamma"]), int(g["n"]), left=(i == 0),
                                    right=(i == ne - 1), global_domain=(float(nodes[0]), float(nodes[-1])))[0]
                  for i in range(ne)])
    u, _ = orc.evaluate_solution(nodes, W, g["xq"])
    assert np.array_equal(W, g["W"]) and np.array_equal(u, g["u_ref"], equal_nan=True)


def test_bubble_metric_sees_a_missing_enhancement():
    """``rel_l2_coef`` is dominated by the linear part on fine meshes (1.2 h^2: a result with NO
    enhancement reads 1.5e-10 on 1e5 elements of [-1,1] and 1.5e-14 on 1e7 -- below every parity bar);
    ``rel_l2_bubble`` reads 1 for it at every mesh size.  The full-size GPU tests assert the latter."""
    for ne, expect in ((100000, 1.5e-10), (10000000, 1.5e-14)):
        nodes = np.linspace(-1, 1, ne + 1)[ne // 3: ne // 3 + 41]
        values = np.sin(np.pi * nodes)
        W = orc.enhance_all_vec(nodes, values, 9, 1e4, 16, global_domain=(-1.0, 1.0))
        Wz = W.copy()
        Wz[:, 2:] = 0.0
        whole = orc.rel_l2_coef(Wz, W).max()
        assert 0.5 * expect < whole < 2.0 * expect, whole          # invisible at the 1e-12 / 1e-13 bars
        assert np.all(orc.rel_l2_bubble(Wz, W) == 1.0)             # unmistakable
        assert orc.rel_l2_bubble(W, W).max() == 0.0
        pert = W.copy()
        pert[:, 2] *= 1.0 + 1e-9          # w_2 carries the bubble on a fine mesh (w_4 is 1e-11 of it)
        assert 5e-10 < orc.rel_l2_bubble(pert, W).min() <= orc.rel_l2_bubble(pert, W).max() < 1.1e-9
    # no bubble in the reference row: 0 when none is returned, inf otherwise
    lin = np.array([[0.3, 0.1, 0.0, 0.0]])
    assert orc.rel_l2_bubble(lin, lin)[0] == 0.0
    assert np.isinf(orc.rel_l2_bubble(lin + [[0, 0, 1e-3, 0]], lin)[0])
