"""CPU: the host side of hp-adaptive refinement -- the four C entries are exported and bound, their argument
errors come back before any HIP call, the numpy restatement of the kernels' rules (tests/hp_rules.py) agrees with
cases worked out by hand, and the facade validates before it touches a GPU."""
import ctypes
import math

import numpy as np
import pytest

import hp_rules

FAKE = ctypes.c_void_p(4096)       # never dereferenced: every call below fails validation first
NAMES = ("lssvr_smoothness", "lssvr_refine_hp", "lssvr_group_work_bytes", "lssvr_group_by_degree")


def _lib():
    from hybrid_fem_lssvr_amd import _capi
    return _capi.load()


def test_symbols_exported_and_bound():
    from hybrid_fem_lssvr_amd import _capi
    lib = _lib()
    for nm in NAMES:
        assert nm in _capi.SIGNATURES
        fn = getattr(lib, nm)
        assert fn.argtypes == _capi.SIGNATURES[nm][1] and fn.restype is _capi.SIGNATURES[nm][0]
    assert lib.lssvr_version() == 7


def test_smoothness_argument_errors():
    lib = _lib()

    def call(W=FAKE, ldw=9, deg=FAKE, ne=8, sigma=FAKE):
        return lib.lssvr_smoothness(W, ldw, deg, ne, sigma, None)

    for ldw in (1, 34, 0, -3):
        assert call(ldw=ldw) == -3 and b"ldw" in lib.lssvr_last_error()
    assert call(ne=0) == -2
    for kw in (dict(W=None), dict(deg=None), dict(sigma=None)):
        assert call(**kw) == -1, kw


def test_refine_hp_argument_errors():
    lib = _lib()

    def call(ne=8, theta=0.5, h_min=0.0, dM=2, M_max=21, x=FAKE, eta2=FAKE, mx=FAKE, sigma=FAKE, deg=FAKE, work=FAKE,
             x_new=FAKE, deg_new=FAKE, ne_new=FAKE, counts=FAKE):
        return lib.lssvr_refine_hp(x, ne, eta2, mx, theta, h_min, sigma, deg, 1.0, dM, M_max, work, x_new, deg_new,
                                   None, ne_new, counts, None)

    for dM in (0, -1):
        assert call(dM=dM) == -3 and b"dM" in lib.lssvr_last_error()
    for mm in (34, 1, 0, -5):
        assert call(M_max=mm) == -3 and b"M_max" in lib.lssvr_last_error()
    for th in (-0.1, 1.5, float("nan")):
        assert call(theta=th) == -2 and b"theta" in lib.lssvr_last_error()
    for hm in (-1.0, float("nan"), float("inf")):
        assert call(h_min=hm) == -2 and b"h_min" in lib.lssvr_last_error()
    assert call(ne=0) == -2
    for kw in (dict(x=None), dict(eta2=None), dict(mx=None), dict(sigma=None), dict(deg=None), dict(work=None),
               dict(x_new=None), dict(deg_new=None), dict(ne_new=None), dict(counts=None)):
        assert call(**kw) == -1, kw


def test_group_by_degree_argument_errors_and_work_bytes():
    lib = _lib()
    assert lib.lssvr_group_by_degree(FAKE, 0, FAKE, FAKE, FAKE, None) == -2
    for i in range(4):
        args = [FAKE, 8, FAKE, FAKE, FAKE]
        args[i if i == 0 else i + 1] = None
        assert lib.lssvr_group_by_degree(*args, None) == -1, i
    prev = 0
    for ne in (1, 255, 256, 257, 10 ** 6, 10 ** 9):
        b = lib.lssvr_group_work_bytes(ne)
        # 32 int64 counters per workgroup of 256 elements, at most 1024 workgroups
        assert b == 8 * 32 * min(1024, (ne + 255) // 256) and b >= prev
        prev = b


# ---------------------------------------------------------------------------
# hp_rules against hand-computed cases
# ---------------------------------------------------------------------------
def test_rule_envelope_over_parity_zeros():
    """An odd solution: the even coefficients vanish.  |w| = e^-1, 0, e^-3, 0, e^-5 at p = 1 .. 5 has the envelope
    e^-1, e^-3, e^-3, e^-5, e^-5: ln env = -1, -3, -3, -5, -5 against p = 1 .. 5, pbar = 3, ybar = -17/5,
    sum (p - pbar)(y - ybar) = (-2)(2.4) + (-1)(0.4) + 0 + (1)(-1.6) + (2)(-1.6) = -10, sum (p - pbar)^2 = 10:
    sigma = 1 -- the decay rate of the non-zero coefficients, which a fit through ln 0 would not give."""
    w = np.array([[0.0, math.exp(-1), 0.0, -math.exp(-3), 0.0, math.exp(-5), 7.0, 7.0]])
    assert hp_rules.smoothness(w, [6])[0] == pytest.approx(1.0, abs=1e-14)
    # p = 0 enters mx only: a large mean value changes nothing while every envelope point stays above 2^-52 mx
    w[0, 0] = 1e6
    assert hp_rules.smoothness(w, [6])[0] == pytest.approx(1.0, abs=1e-14)
    # ... and takes points away when it does not: mx = 2^51 e^-1 keeps p = 1 (env = e^-1) only -> +inf
    w[0, 0] = 2.0 ** 51 * math.exp(-1)
    assert hp_rules.smoothness(w, [6])[0] == np.inf
    # an exact geometric decay: slope of -0.7 p
    g = np.exp(-0.7 * np.arange(12))[None]
    assert hp_rules.smoothness(g, [12])[0] == pytest.approx(0.7, abs=1e-14)
    # a growing tail is flat in the envelope: sigma = 0
    assert hp_rules.smoothness(np.array([[1.0, 1.0, 2.0, 3.0]]), [4])[0] == 0.0


def test_rule_inf_and_nan_cases():
    inf, nan = np.inf, np.nan
    W = np.array([[0.0, 0.0, 0.0, 0.0, 0.0],       # mx == 0
                  [1.0, 0.5, 0.25, 0.1, 0.1],      # M = 2 < 3
                  [1.0, 0.0, 0.0, 0.0, 0.0],       # no envelope point is kept
                  [1.0, 0.0, 0.0, 0.5, 0.0],       # env = .5 .5 .5 0: three kept, slope 0
                  [1.0, nan, 0.5, 0.2, 0.1],
                  [1.0, 0.5, inf, 0.2, 0.1],
                  [1.0, 0.5, 0.25, 0.1, nan],      # the NaN is beyond M = 4: not part of the series
                  [nan, 0.5, 0.25, 0.1, 0.1],      # M = 2 with a NaN: NaN wins over M < 3
                  [1.0, 0.5, 0.25, 0.1, 0.1],      # degree the row cannot hold
                  [1.0, 0.5, 0.25, 0.1, 0.1]])
    deg = [5, 2, 5, 5, 5, 5, 4, 2, 6, 1]
    s = hp_rules.smoothness(W, deg)
    assert s[0] == inf and s[1] == inf and s[2] == inf
    assert s[3] == 0.0
    assert np.isnan(s[4]) and np.isnan(s[5]) and np.isnan(s[7]) and np.isnan(s[8]) and np.isnan(s[9])
    # row 6: ln(.5, .25, .1) against p = 1, 2, 3: slope (ln .1 - ln .5) / 2
    assert s[6] == pytest.approx(0.5 * math.log(5.0), abs=1e-14)


def test_rule_marking_tie_and_precedence():
    """theta = 0.5, max = 4: the threshold is 1.0 and a tie is marked.  Of the marked elements the smooth ones that
    have room are raised, the others bisected unless h_min forbids it; nothing else changes."""
    x = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 4.25, 5.0, 6.0, 7.0])
    eta2 = np.array([1.0, np.nextafter(1.0, 0.0), 4.0, 2.0, 3.0, np.nan, 2.0, 0.5])
    sig = np.array([2.0, 9.0, 0.5, 2.0, 0.2, 3.0, np.nan, 9.0])
    deg = np.array([5, 5, 5, 20, 7, 9, 6, 5], dtype=np.int32)
    assert list(hp_rules.marked(eta2, 4.0, 0.5)) == [True, False, True, True, True, True, True, False]
    up, split = hp_rules.actions(x, eta2, 4.0, 0.5, 0.2, sig, deg, 1.0, 2, 21)
    #            tie->raised  below  rough  no room(20+2>21)  rough but short  NaN eta2, smooth  NaN sigma  unmarked
    assert list(up) == [True, False, False, False, False, True, False, False]
    assert list(split) == [False, False, True, True, False, False, True, False]
    xn, dn, par, (ns, nr) = hp_rules.refine_hp(x, eta2, 4.0, 0.5, 0.2, sig, deg, 1.0, 2, 21)
    assert (ns, nr) == (3, 2)
    assert list(xn) == [0.0, 1.0, 2.0, 2.5, 3.0, 3.5, 4.0, 4.25, 5.0, 5.5, 6.0, 7.0]
    assert list(dn) == [7, 5, 5, 5, 20, 20, 7, 11, 6, 6, 5] and dn.dtype == np.int32
    assert list(par) == [0, 1, 2, 2, 3, 3, 4, 5, 6, 6, 7]
    # deg + dM == M_max is still room
    up, _ = hp_rules.actions(x, eta2, 4.0, 0.5, 0.2, sig, deg, 1.0, 1, 21)
    assert up[3]
    # max == 0 marks the non-finite only; sigma == sigma_min is smooth
    up, split = hp_rules.actions(x, np.where(np.isnan(eta2), np.nan, 0.0), 0.0, 0.5, 0.0, np.full(8, 1.0), deg, 1.0, 2, 21)
    assert list(up | split) == [False] * 5 + [True] + [False] * 2 and up[5]


def test_rule_group_by_degree():
    deg = [5, 33, 2, 5, 40, 2, 1, 5, 33]
    ids, off = hp_rules.group_by_degree(deg)
    assert list(ids) == [2, 5, 0, 3, 7, 1, 8]
    assert off.shape == (35,) and list(off[:7]) == [0, 0, 0, 2, 2, 2, 5] and off[33] == 5 and off[34] == 7
    assert list(ids[off[5]:off[6]]) == [0, 3, 7] and list(ids[off[33]:off[34]]) == [1, 8]


# ---------------------------------------------------------------------------
# facade
# ---------------------------------------------------------------------------
def test_facade_hp_validates_before_any_gpu_use():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    one = lambda x: 1.0 + 0.0 * np.asarray(x)       # noqa: E731
    zero = lambda x: 0.0 * np.asarray(x)            # noqa: E731
    with pytest.raises(ValueError, match="coef"):
        pkg.FEMLSSVRPrimalSolver(9, lssvr_M=5, coef=(one, zero)).solve_adaptive(mode="hp")
    with pytest.raises(ValueError, match="reaction"):
        pkg.FEMLSSVRPrimalSolver(9, lssvr_M=5, reaction=one).solve_adaptive(mode="hp")
    with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
        pkg.FEMLSSVRPrimalSolver(9, lssvr_M=5, solver=ops.SOLVER_DUAL).solve_adaptive(mode="hp")
    s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=5)
    assert s.element_degrees is None
    with pytest.raises(ValueError, match="mode"):
        s.solve_adaptive(mode="p")
    for mm in (4, 34, 7.5):
        with pytest.raises(ValueError, match="M_max"):
            s.solve_adaptive(mode="hp", M_max=mm)
    for dM in (0, -2, 1.5):
        with pytest.raises(ValueError, match="dM"):
            s.solve_adaptive(mode="hp", dM=dM)
    with pytest.raises(ValueError, match="sigma_min"):
        s.solve_adaptive(mode="hp", sigma_min=float("nan"))
    with pytest.raises(ValueError, match="max_dof"):
        s.solve_adaptive(mode="hp", max_dof=39)          # 8 elements of 5 coefficients
    with pytest.raises(ValueError, match="max_dof"):
        s.solve_adaptive(max_dof=600)                    # mode "h" is bounded by max_elements
    with pytest.raises(ValueError, match="theta"):
        s.solve_adaptive(mode="hp", theta=2.0)
    assert s.adapt_history == [] and s.element_degrees is None


def test_facade_checks_element_degrees():
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(5, lssvr_M=5)
    s.fem_nodes, s.fem_values = np.linspace(-1, 1, 5), np.zeros(5)
    for bad in ([5, 5, 5], [5, 5, 5, 1], [5, 5, 5, 34], [5.0, 5.0, 5.0, 5.0]):
        s.element_degrees = bad
        with pytest.raises(ValueError, match="element_degrees"):
            s._check_degrees(4)
    s.element_degrees = [2, 9, 33, 5]
    assert list(s._check_degrees(4)) == [2, 9, 33, 5]
    one = lambda x: 1.0 + 0.0 * np.asarray(x)       # noqa: E731
    r = pkg.FEMLSSVRPrimalSolver(5, lssvr_M=5, reaction=one)
    r.element_degrees = [5, 5, 5, 5]
    with pytest.raises(ValueError, match="reaction"):
        r._check_degrees(4)


def test_group_colloc_is_max_of_n_colloc_and_2M():
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(5, lssvr_M=5, n_colloc=16)
    for M in range(2, 34):
        n = s.group_colloc(M)
        assert n == max(16, 2 * M) == hp_rules.n_colloc(16, M)
        assert n >= 2 * (M - 2)                          # the parity-solve regime of the large-degree kernels
    assert pkg.FEMLSSVRPrimalSolver(5, lssvr_M=5, n_colloc=80).group_colloc(33) == 80
