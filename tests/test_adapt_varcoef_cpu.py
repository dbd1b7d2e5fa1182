"""CPU: the host side of the variable-coefficient indicator (ABI 7) -- lssvr_estimate_varcoef is exported and
bound, rejects every single bad argument before any HIP call (in a child process that sees no GPU), and the
facade's ``coef`` keyword is validated in the constructor."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssvr_hip.h")

_F = [0x10000 * (i + 1) for i in range(12)]        # fake device pointers: never dereferenced
_VALID = dict(x=_F[0], W=_F[1], ne=10, M=9, nq=16, a_values=_F[2], da_values=_F[3], rhs_values=_F[4],
              table_layout=0, a_ends=_F[5], eta2=_F[6], jump=None, out3=_F[7], work=_F[8], stream=None)
# (overrides, rc, message substring): one broken rule each; no case may reach a launch
FAULTS = [({"x": None}, -1, "non-NULL"), ({"W": None}, -1, "non-NULL"), ({"eta2": None}, -1, "non-NULL"),
          ({"out3": None}, -1, "non-NULL"), ({"work": None}, -1, "non-NULL"),
          ({"a_values": None}, -1, "non-NULL"), ({"da_values": None}, -1, "non-NULL"),
          ({"rhs_values": None}, -1, "non-NULL"), ({"a_ends": None}, -1, "a_ends"),
          ({"ne": 0}, -2, "ne"), ({"ne": -1}, -2, "ne"), ({"ne": (1 << 40) + 1}, -2, "too large"),
          ({"M": 0}, -3, "M = 0"), ({"M": 34}, -3, "M = 34"), ({"M": -5}, -3, "M = -5"),
          ({"nq": 0}, -7, "nq"), ({"nq": 33}, -7, "nq"), ({"nq": -1}, -7, "nq"),
          ({"table_layout": 2}, -2, "unknown table_layout"), ({"table_layout": -1}, -2, "unknown table_layout"),
          ({"table_layout": 1, "a_ends": None}, -1, "a_ends")]


def _run_faults():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    out = []
    for over, _, _ in FAULTS:
        args = dict(_VALID, **over)
        assert list(args) == list(_VALID)
        rc = lib.lssvr_estimate_varcoef(*args.values())
        out.append((over, rc, lib.lssvr_last_error().decode()))
    return out


def test_estimate_varcoef_exported_and_bound():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    assert hasattr(lib, "lssvr_estimate_varcoef")
    restype, argtypes = _capi.SIGNATURES["lssvr_estimate_varcoef"]
    assert restype is ctypes.c_int and len(argtypes) == len(_VALID)
    assert lib.lssvr_version() == _capi.ABI_VERSION == 7
    assert "lssvr_estimate_varcoef(" in open(HEADER).read()


def test_estimate_varcoef_single_faults_without_gpu():
    """Every single bad argument returns its code and message on the host: the calls run in a child process
    with no GPU visible, so a check that sat behind a HIP call would fail there."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="4096", ROCR_VISIBLE_DEVICES="4096")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--faults"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == len(FAULTS)
    bad = [(over, rc, msg, w_rc, sub) for (over, rc, msg), (_, w_rc, sub) in zip(got, FAULTS)
           if rc != w_rc or sub not in msg]
    assert not bad, "\n".join(map(repr, bad))


def _one(x):
    return 1.0 + 0.0 * x


def _zero(x):
    return 0.0 * x


@pytest.mark.parametrize("coef", [_one, (_one,), (_one, _zero, _zero), (_one, 1.0), (1.0, _zero), "ab",
                                  {"a": _one, "da": _zero}])
def test_facade_rejects_malformed_coef(coef):
    import hybrid_fem_lssvr_amd as pkg
    with pytest.raises(ValueError, match="coef"):
        pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, coef=coef)


def test_facade_rejects_coef_with_other_solvers():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    with pytest.raises(ValueError, match="shared operator"):
        pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, coef=(_one, _zero), solver=ops.SOLVER_SHARED)
    for sid in (ops.SOLVER_DUAL, ops.SOLVER_PRIMAL_WAVE, ops.SOLVER_PRIMAL_MOMENT):
        with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
            pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, coef=(_one, _zero), solver=sid)


def test_facade_accepts_coef_pair():
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, coef=[_one, _zero])
    assert s.coef == (_one, _zero)
    assert pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9).coef is None


if __name__ == "__main__" and sys.argv[1:] == ["--faults"]:
    sys.path.insert(0, ROOT)
    print(json.dumps(_run_faults()))
