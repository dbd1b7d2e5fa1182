"""CPU: the eigenproblem feature where there is no GPU -- the numpy prototype against scipy, the
whole iteration with the library's host entries in the loop, the host mirrors of the Ritz step and the Sturm count,
the argument errors of every new entry and the facade's refusals."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                # (the fault table's child process runs this file as a script)
    sys.path.insert(0, ROOT)

import eigen_rules as er                # noqa: E402

proto = er.proto


@pytest.mark.parametrize("name,m", er.cases(600))
def test_prototype_against_reference(name, m):
    """scripts/proto/eigen_proto.py on problems 1-5: eigenvalues within the bar of scipy.linalg.eigh (the closed form on
    the uniform Poisson problems), positions from the Sturm count, M-orthonormal vectors, residuals, vectors."""
    p = er.case(name, m)
    for k in er.ks_of(p):
        r = proto.solve(p.bands, p.kinds, p.kappa, k=k, sigma=p.sigma)
        assert r["converged"] and r["iterations"] <= 200
        er.check_solution(p, k, r["theta"], r["X"], r["residuals"], r["index"])


def test_interior_shift_returns_modes_2_to_5():
    p = er.interior(33)
    r = proto.solve(p.bands, k=4, sigma=p.sigma)
    assert sorted(r["index"]) == [2, 3, 4, 5] and set(r["index"][:2]) == {3, 4} and list(r["index"][2:]) == [2, 5]
    assert r["counts"] == (2, 6)


@pytest.mark.parametrize("name,m", [("poisson", 7), ("poisson", 33), ("poisson", er.BLK + 1), ("interior", 9),
                                    ("interior", 33), ("interior", er.BLK + 1), ("double-well", 33),
                                    ("double-well", er.BLK + 1)])
def test_iteration_through_the_host_entries(name, m):
    """The prototype's loop with lssvr_tridiag_pivot_solve_host as the solve, lssvr_eig_ritz_host as the Ritz step and
    lssvr_eig_count_host as the count: the same checks hold."""
    p = er.case(name, m)
    for k in er.ks_of(p):
        r = proto.solve(p.bands, p.kinds, p.kappa, k=k, sigma=p.sigma, solve_fn=er.pivot_solve_host,
                        ritz_fn=er.ritz_host, count_fn=er.sturm_host)
        assert r["converged"]
        er.check_solution(p, k, r["theta"], r["X"], r["residuals"], r["index"])


@pytest.mark.parametrize("nb", range(1, 9))
def test_ritz_host_random_pencils(nb):
    for seed, sigma, rep in ((nb, 0.0, False), (100 + nb, 4.0, False), (200 + nb, 1.0, True)):
        A, B, d = er.random_pencil(nb, seed, repeated=rep)
        theta, Q, info = er.ritz_host(A, B, sigma)
        er.check_ritz(A, B, sigma, theta, Q, info, d)


def test_ritz_host_dependent_column():
    """A rank-deficient B (column 2 = column 0 of the vectors behind it): info > 0, nothing non-finite, the dependent
    column is zero and ordered last, the others still diagonalise the pencil on their span."""
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((5, 40))
    Z[2] = Z[0]
    D = np.linspace(1.0, 3.0, 40)
    A, B = (Z * D[None, :]) @ Z.T, Z @ Z.T
    theta, Q, info = er.ritz_host(A, B, 0.0)
    assert info == 1
    assert np.all(np.isfinite(theta)) and np.all(np.isfinite(Q))
    assert np.all(Q[:, -1] == 0.0) and theta[-1] == 0.0
    Qg = Q[:, :-1]
    assert np.max(np.abs(Qg.T @ B @ Qg - np.eye(4))) <= 1e-12
    assert np.max(np.abs(Qg.T @ A @ Qg - np.diag(theta[:-1]))) <= 1e-12 * np.max(np.abs(A))
    # a zero vector in the block
    Z[2] = 0.0
    _, Q, info = er.ritz_host((Z * D[None, :]) @ Z.T, Z @ Z.T, 0.0)
    assert info == 1 and np.all(np.isfinite(Q)) and np.all(Q[:, -1] == 0.0)


@pytest.mark.parametrize("name,m", er.cases(600))
def test_count_host(name, m):
    """lssvr_eig_count_host = #{lambda_ref < s} between every pair of neighbouring reference eigenvalues, below the
    first and above the last; on a reference eigenvalue either neighbour count."""
    p = er.case(name, m)
    lam = er.ref_values(p)
    shifts, lo, hi = er.count_shifts(lam)
    got = er.count_host(p.bands, p.kinds, p.kappa, shifts)
    assert np.all((got >= lo) & (got <= hi)), (name, m, np.nonzero((got < lo) | (got > hi))[0][:5])
    al, be, mu, nu = p.reduced
    assert [proto.sturm_count(al, be, mu, nu, s) for s in shifts[:8]] == list(got[:8])


@pytest.mark.parametrize("ne", [8, 16, 32])
def test_enhanced_eigenvalue_is_closer_in_the_prototype(ne):
    """-u'' = lambda u, Dirichlet, M = 9: the Rayleigh quotient of the modes enhanced by the oracle's reaction rows is
    strictly closer to (j pi / 2)^2 than the P1 value, j = 1, 2 -- the condition the GPU test relies on.  Measured
    here: factors 6.0e3 / 3.6e2 at ne = 8, 9.7e4 / 6.0e3 at 16, 1.5e6 / 9.7e4 at 32."""
    for _, j, e_fem, e_enh in proto.improvement_table((ne,)):
        assert e_enh < e_fem, (ne, j, e_fem, e_enh)


# --- argument errors of the new entries: fake pointers, a child process that sees no GPU ------------------------------
_F = [0x10000 * (i + 1) for i in range(12)]
_BANDS = dict(kdiag=_F[0], koff=_F[1], mdiag=_F[2], moff=_F[3], kind_left=0, kind_right=1, kappa="K")
_ARGS = {
    "lssvr_eig_apply": dict(**_BANDS, ne=10, nb=4, Z=_F[4], MZ=_F[5], KZ=_F[6], gram=_F[7], work=_F[8],
                            work_bytes=1 << 30, stream=None),
    "lssvr_eig_ritz": dict(A=_F[0], B=_F[1], nb=4, sigma=0.0, theta=_F[2], Q=_F[3], info=None, stream=None),
    "lssvr_eig_ritz_host": dict(A="A", B="A", nb=4, sigma=0.0, theta="A", Q="A", info=None),
    "lssvr_eig_rotate": dict(Z=_F[0], MZ=_F[1], KZ=_F[2], Q=_F[3], theta=_F[4], kind_left=0, kind_right=0, ne=10, nb=4,
                             X=_F[5], Y=_F[6], res2=_F[7], work=_F[8], work_bytes=1 << 30, stream=None),
    "lssvr_eig_count": dict(**_BANDS, ne=10, shifts=_F[4], ns=3, pivmin=1e-300, counts=_F[5], stream=None),
    "lssvr_eig_count_host": dict(kdiag="A", koff="A", mdiag="A", moff="A", kind_left=0, kind_right=1, kappa="K", ne=10,
                                 shifts="A", ns=3, pivmin=1e-300, counts=_F[5]),
    "lssvr_eig_rayleigh": dict(x=_F[0], W=_F[1], ne=10, M=9, nq=9, a_values=_F[2], c_values=_F[3], rho_values=_F[4],
                               table_layout=0, kind_left=0, kind_right=1, kappa="K", out3=_F[5], work=_F[6],
                               stream=None),
}
_NB = [({"nb": 0}, -2, "nb = 0"), ({"nb": 9}, -2, "nb = 9")]
_KINDS = [({"kind_left": 2}, -2, "end kinds"), ({"kind_right": -1}, -2, "end kinds")]
_KAPPA = [({"kappa": None}, -1, "kappa_host"), ({"kappa": "KNAN"}, -2, "must be finite")]
_EIG_BANDS = [({"ne": -1}, -2, "ne"), ({"kdiag": None}, -1, "non-NULL"), ({"koff": None}, -1, "non-NULL"),
              ({"mdiag": None}, -1, "non-NULL"), ({"moff": None}, -1, "non-NULL")] + _KINDS + _KAPPA
_WORK = [({"work": None}, -1, "work must be non-NULL"), ({"work_bytes": 8}, -2, "lssvr_eig_work_bytes")]
_RITZ = _NB + [({"A": None}, -1, "non-NULL"), ({"B": None}, -1, "non-NULL"), ({"theta": None}, -1, "non-NULL"),
               ({"Q": None}, -1, "non-NULL"), ({"sigma": float("nan")}, -2, "sigma"),
               ({"sigma": float("inf")}, -2, "sigma")]
_COUNT = [({"ns": -1}, -2, "ns"), ({"shifts": None}, -1, "non-NULL"), ({"counts": None}, -1, "non-NULL"),
          ({"pivmin": 0.0}, -2, "pivmin"), ({"pivmin": float("nan")}, -2, "pivmin")]
FAULTS = {
    "lssvr_eig_apply": _EIG_BANDS + _NB + _WORK + [({"Z": None}, -1, "non-NULL"), ({"MZ": None}, -1, "non-NULL"),
                                                  ({"KZ": None}, -1, "non-NULL"), ({"gram": None}, -1, "non-NULL")],
    "lssvr_eig_ritz": _RITZ,
    "lssvr_eig_ritz_host": _RITZ,
    "lssvr_eig_rotate": [({"ne": -1}, -2, "ne")] + _NB + _KINDS + _WORK + [
        ({nm: None}, -1, "non-NULL") for nm in ("Z", "MZ", "KZ", "Q", "theta", "X", "Y", "res2")],
    "lssvr_eig_count": _EIG_BANDS + _COUNT,
    "lssvr_eig_count_host": _EIG_BANDS + _COUNT,
    "lssvr_eig_rayleigh": [({"ne": -1}, -2, "ne"), ({"M": 0}, -3, "M = 0"), ({"M": 34}, -3, "M = 34"),
                           ({"nq": 0}, -7, "nq"), ({"nq": 33}, -7, "nq"), ({"x": None}, -1, "non-NULL"),
                           ({"W": None}, -1, "non-NULL"), ({"out3": None}, -1, "non-NULL"),
                           ({"work": None}, -1, "non-NULL"), ({"a_values": None}, -1, "non-NULL"),
                           ({"c_values": None}, -1, "non-NULL"), ({"rho_values": None}, -1, "non-NULL"),
                           ({"table_layout": 2}, -2, "unknown table_layout")] + _KINDS + _KAPPA,
}
# ne == 0 (ns == 0 for the counts): success, nothing launched, no pointer read
_EMPTY = {"lssvr_eig_apply": {"ne": 0}, "lssvr_eig_rotate": {"ne": 0}, "lssvr_eig_count": {"ne": 0},
          "lssvr_eig_count_host": {"ne": 0}, "lssvr_eig_rayleigh": {"ne": 0}}


def _call(lib, name, over):
    args = dict(_ARGS[name], **over)
    assert list(args) == list(_ARGS[name]), (name, over)
    host = (ctypes.c_double * 64)(*([1.0] * 64))
    conv = {"K": (ctypes.c_double * 2)(0.0, 0.5), "KNAN": (ctypes.c_double * 2)(0.0, float("nan")), "A": host}
    vals = [conv[v] if isinstance(v, str) else v for v in args.values()]
    return getattr(lib, name)(*vals)


def _run_fault_table():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    out = []
    for name, faults in FAULTS.items():
        for over, _, _ in faults:
            rc = _call(lib, name, over)
            out.append((name, {k: repr(v) for k, v in over.items()}, rc, lib.lssvr_last_error().decode()))
    empty = [(name, _call(lib, name, over)) for name, over in _EMPTY.items()]
    sizes = [lib.lssvr_eig_work_bytes(1000, 8), lib.lssvr_eig_work_bytes(1000, 1), lib.lssvr_eig_work_bytes(0, 4)]
    return dict(faults=out, empty=empty, sizes=sizes)


def test_argument_errors_without_gpu():
    """Every new entry rejects each single broken rule with its own code and message, on the host: the table runs in a
    child process with no GPU visible, so a check that had moved behind a launch would fail there."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="4096", ROCR_VISIBLE_DEVICES="4096")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--faults"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    want = [(name, rc, sub) for name, faults in FAULTS.items() for _, rc, sub in faults]
    assert len(got["faults"]) == len(want) and len(want) > 80
    bad = [(n, o, rc, msg, w_rc, sub) for (n, o, rc, msg), (_, w_rc, sub) in zip(got["faults"], want)
           if rc != w_rc or sub not in msg]
    assert not bad, "\n".join(map(repr, bad))
    assert all(rc == 0 for _, rc in got["empty"]), got["empty"]
    big, small, none = got["sizes"]
    assert big >= 8 * 72 * math.ceil(1001 / er.BLK) and small >= 8 * 3 and big > small >= none >= 0


# --- the facade's refusals, each before any device call (there is no device here) ----------------------------------
def _solver(**kw):
    import hybrid_fem_lssvr_amd as pkg
    return pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, lssvr_gamma=1e4, n_colloc=16, **kw)


@pytest.mark.parametrize("kw,call,match", [
    (dict(convection=lambda x: 1.0 + 0.0 * x), {}, "convection"),
    (dict(boundary="periodic", reaction=lambda x: 1.0 + 0.0 * x), {}, "periodic"),
    (dict(fem_solver="flux"), {}, "flux"),
    (dict(boundary=(("dirichlet", 0.5), None)), {}, "homogeneous"),
    (dict(boundary=(("neumann", 1.0), None)), {}, "homogeneous"),
    (dict(boundary=(("robin", 2.0, -0.25), ("robin", 2.0, 0.0))), {}, "homogeneous"),
    ({}, dict(weight=lambda x: 0.0 * x), "weight must be positive"),
    ({}, dict(weight=lambda x: x), "weight must be positive"),
    ({}, dict(k=7), "k must be an integer in 1 .. 6"),
    ({}, dict(k=0), "k must be an integer in 1 .. 6"),
    (dict(mesh=np.linspace(-1, 1, 4)), dict(k=3), "number of unknowns"),
    ({}, dict(sigma=float("nan")), "sigma"),
])
def test_facade_refusals(kw, call, match):
    s = _solver(**kw)
    with pytest.raises(ValueError, match=match):
        s.solve_eigen(**call)


def test_facade_exports():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    assert pkg.EigenSolution is not None and callable(pkg.FEMLSSVRPrimalSolver.solve_eigen)
    for name in ("eig_apply", "eig_ritz", "eig_rotate", "eig_count", "eig_rayleigh"):
        assert callable(getattr(ops, name))
    import torch
    x = torch.linspace(0, 1, 5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.eig_apply(x, x[:4], x, x[:4], x.reshape(1, 5))


if __name__ == "__main__" and sys.argv[1:] == ["--faults"]:
    sys.path.insert(0, ROOT)
    print(json.dumps(_run_fault_table()))
