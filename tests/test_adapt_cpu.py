"""CPU: the host side of the a posteriori indicator and h-refinement (ABI 6) -- the Gauss rule,
argument errors of the new C entries (reported before any HIP call) and the facade's validation."""
import ctypes

import numpy as np
import pytest

FAKE = ctypes.c_void_p(4096)       # never dereferenced: every call below fails validation first


def _lib():
    from hybrid_fem_lssvr_amd import _capi
    return _capi.load()


@pytest.mark.parametrize("nq", list(range(1, 33)))
def test_gauss_rule_matches_leggauss(nq):
    """Nodes within 1e-15 of numpy's leggauss; weights within 4e-15 of it -- leggauss itself is off
    by up to 1.6e-15 in its end weights (nq = 17), so the rule is also held to the 40-digit one (1 ulp)."""
    import mpmath as mp
    from hybrid_fem_lssvr_amd import ops
    xi, wt = ops.gauss_rule(nq)
    xr, wr = np.polynomial.legendre.leggauss(nq)
    assert np.all(np.diff(xi) > 0)
    assert np.array_equal(xi, -xi[::-1]) and np.array_equal(wt, wt[::-1])
    assert np.max(np.abs(xi - xr)) <= 1e-15
    assert np.max(np.abs(wt - wr)) <= 4e-15
    with mp.workdps(40):
        xs = [mp.findroot(lambda z: mp.legendre(nq, z), mp.mpf(v)) for v in xr]
        ws = [2 / ((1 - z ** 2) * mp.diff(lambda t: mp.legendre(nq, t), z) ** 2) for z in xs]
    xs = np.array([float(v) for v in xs])
    ws = np.array([float(v) for v in ws])
    assert np.all(np.abs(xi - xs) <= np.spacing(np.abs(xs)) + 1e-300)
    assert np.all(np.abs(wt - ws) <= np.spacing(ws))


def test_gauss_rule_argument_errors():
    lib = _lib()
    buf = (ctypes.c_double * 40)()
    for nq in (0, 33, -1):
        assert lib.lssvr_gauss_rule(nq, buf, buf) == -7
        assert b"nq" in lib.lssvr_last_error()
    assert lib.lssvr_gauss_rule(4, None, buf) == -1


def test_eval_deriv_argument_errors():
    lib = _lib()
    for order in (-1, 3):
        rc = lib.lssvr_eval_deriv(FAKE, FAKE, 4, 9, order, FAKE, 10, FAKE, None, None)
        assert rc == -3 and b"order" in lib.lssvr_last_error()
    assert lib.lssvr_eval_deriv(FAKE, FAKE, 0, 9, 1, FAKE, 10, FAKE, None, None) == -2
    assert lib.lssvr_eval_deriv(FAKE, FAKE, 4, 0, 1, FAKE, 10, FAKE, None, None) == -3
    assert lib.lssvr_eval_deriv(None, FAKE, 4, 9, 1, FAKE, 10, FAKE, None, None) == -1
    assert lib.lssvr_eval_deriv(FAKE, FAKE, 4, 9, 2, FAKE, 10, None, None, None) == -1


def test_estimate_argument_errors():
    from hybrid_fem_lssvr_amd import _capi
    lib = _lib()
    p = _capi.rhs_params(1.0, 1.0)

    def est(ne=8, M=9, nq=16, rhs_id=1, params=p, vals=None, x=FAKE, W=FAKE, eta2=FAKE, out3=FAKE, work=FAKE):
        return lib.lssvr_estimate(x, W, ne, M, nq, rhs_id, params, vals, eta2, None, out3, work, None)

    for nq in (0, 33):
        assert est(nq=nq) == -7 and b"nq" in lib.lssvr_last_error()
    assert est(M=34) == -3 and b"M = 34" in lib.lssvr_last_error()
    assert est(M=0) == -3
    assert est(ne=0) == -2
    for kw in (dict(x=None), dict(W=None), dict(eta2=None), dict(out3=None), dict(work=None)):
        assert est(**kw) == -1, kw
    assert est(rhs_id=7) == -4
    assert est(params=None) == -4                       # SIN without its parameters
    assert est(rhs_id=0) == -4 and est(rhs_id=2) == -4  # tables without values
    assert lib.lssvr_estimate_points(FAKE, 8, 0, FAKE, None) == -7
    assert lib.lssvr_estimate_points(FAKE, 8, 33, FAKE, None) == -7
    assert lib.lssvr_estimate_points(None, 8, 4, FAKE, None) == -1


def test_refine_argument_errors():
    lib = _lib()

    def ref(ne=8, theta=0.5, h_min=0.0, x=FAKE, eta2=FAKE, mx=FAKE, work=FAKE, x_new=FAKE, ne_new=FAKE):
        return lib.lssvr_refine(x, ne, eta2, mx, theta, h_min, work, x_new, None, ne_new, None)

    for th in (-0.1, 1.5, float("nan")):
        assert ref(theta=th) == -2 and b"theta" in lib.lssvr_last_error()
    for hm in (-1.0, float("nan"), float("inf")):
        assert ref(h_min=hm) == -2 and b"h_min" in lib.lssvr_last_error()
    assert ref(ne=0) == -2
    for kw in (dict(x=None), dict(eta2=None), dict(mx=None), dict(work=None), dict(x_new=None),
               dict(ne_new=None)):
        assert ref(**kw) == -1, kw


def test_adapt_work_bytes():
    lib = _lib()
    prev = 0
    for ne in (1, 2, 127, 128, 129, 1000, 10 ** 6, 2 * 10 ** 6, 10 ** 8):
        b = lib.lssvr_adapt_work_bytes(ne)
        assert b >= 8 * ((ne + 255) // 256) and b >= 24 and b % 8 == 0 and b >= prev
        prev = b


def test_facade_validates_before_any_gpu_use():
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9)
    for th in (-0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="theta"):
            s.solve_adaptive(theta=th)
    for me in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_elements"):
            s.solve_adaptive(max_elements=me)
    with pytest.raises(ValueError, match="max_elements"):
        s.solve_adaptive(max_elements=4)             # 8 initial elements
    with pytest.raises(ValueError, match="max_iter"):
        s.solve_adaptive(max_iter=0)
    with pytest.raises(ValueError, match="nq"):
        s.solve_adaptive(nq=40)
    with pytest.raises(RuntimeError, match="solve"):
        s.estimate()
    assert s.adapt_history == []
