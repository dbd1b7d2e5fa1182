"""CPU: the host side of the multiple-load-case entry -- ``lssvr_enhance_multi`` is exported, declared and bound
(additive: the ABI stays 7), rejects every single bad argument before any HIP call (child process that sees no
GPU), and ``ops.enhance_multi`` refuses host tensors and mismatched shapes before it reaches the library."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssvr_hip.h")
NAME = "lssvr_enhance_multi"

_F = [0x10000 * (i + 1) for i in range(16)]        # fake device pointers: never dereferenced
_VALID = dict(x=_F[0], u=_F[1], ne=10, elem_offset=0, ne_global=10, gxmin=-1.0, gxmax=1.0, bc_values=_F[2], ncases=3,
              M=9, n_colloc=16, gamma=1e4, a_values=_F[3], da_values=_F[4], c_values=_F[5], rhs_values=_F[6],
              table_layout=1, W=_F[7], status=_F[8], fail_count=None, stream=None, kernel_ms_host=None)
# (overrides, rc, message substring): one broken rule each; no case may reach a launch
FAULTS = [({"x": None}, -1, "non-NULL"), ({"u": None}, -1, "non-NULL"), ({"W": None}, -1, "non-NULL"),
          ({"a_values": None}, -1, "non-NULL"), ({"da_values": None}, -1, "non-NULL"),
          ({"rhs_values": None}, -1, "non-NULL"),
          ({"ne": -1}, -2, "ne"), ({"ne": 11}, -2, "shard"), ({"ne_global": 9}, -2, "shard"),
          ({"elem_offset": -1}, -2, "shard"),
          ({"M": 1}, -3, "M = 1"), ({"M": 34}, -3, "M = 34"),
          ({"n_colloc": 1}, -2, "n_colloc"), ({"n_colloc": 4097}, -2, "n_colloc"),
          ({"gamma": 0.0}, -2, "gamma"), ({"gamma": float("nan")}, -2, "gamma"),
          ({"ncases": 0}, -2, "ncases"), ({"ncases": -3}, -2, "ncases"),
          ({"table_layout": 2}, -2, "unknown table_layout"), ({"table_layout": -1}, -2, "unknown table_layout"),
          ({"M": 9, "n_colloc": 6}, -5, "M-2"), ({"M": 22, "n_colloc": 19}, -5, "M-2"),
          ({"M": 33, "n_colloc": 30}, -5, "M-2"),
          # the same rules without the c table (variable-coefficient rows)
          ({"c_values": None, "ncases": 0}, -2, "ncases"), ({"c_values": None, "a_values": None}, -1, "non-NULL"),
          ({"c_values": None, "M": 16, "n_colloc": 13}, -5, "M-2")]
# valid calls that must return 0 without a device: nothing to do
NOOPS = [{"ne": 0, "ne_global": 0}, {"ne": 0, "ne_global": 0, "x": None, "u": None, "W": None, "rhs_values": None},
         {"ne": 0, "ne_global": 7, "elem_offset": 7, "c_values": None, "bc_values": None}]


def _run_faults():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    rows = []
    for over in [f[0] for f in FAULTS] + NOOPS:
        args = dict(_VALID, **over)
        assert list(args) == list(_VALID)
        rc = getattr(lib, NAME)(*args.values())
        rows.append((rc, lib.lssvr_last_error().decode()))
    return rows


def test_multi_entry_exported_declared_and_bound():
    from hybrid_fem_lssvr_amd import _capi, ops
    lib = _capi.load()
    src = open(HEADER).read()
    assert hasattr(lib, NAME)
    assert "int " + NAME + "(" in src
    restype, argtypes = _capi.SIGNATURES[NAME]
    assert restype is ctypes.c_int and len(argtypes) == len(_VALID)
    # ..., gxmax, bc_values (device pointer), ncases (int), M, ...
    assert argtypes[7] is ctypes.c_void_p and argtypes[8] is ctypes.c_int and argtypes[-1] == ctypes.POINTER(ctypes.c_float)
    assert lib.lssvr_version() == _capi.ABI_VERSION == 7          # additive: no ABI bump
    assert "#define LSSVR_ABI_VERSION 7" in src
    assert callable(ops.enhance_multi)


def test_facade_has_solve_many():
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9)
    assert callable(s.solve_many)
    with pytest.raises(ValueError, match="rhs_list"):
        s.solve_many([])
    with pytest.raises(ValueError, match="one .left, right. pair per case"):
        s.solve_many([lambda x: x, lambda x: x], bc=[(0.0, 1.0)])


def test_multi_single_faults_without_gpu():
    """Every single bad argument returns its code and message on the host, and ne == 0 is a successful no-op: the
    calls run in a child process with no GPU visible, so a check that sat behind a HIP call would fail there."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="4096", ROCR_VISIBLE_DEVICES="4096")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--faults"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == len(FAULTS) + len(NOOPS)
    bad = [(over, rc, msg, w_rc, sub) for (rc, msg), (over, w_rc, sub) in zip(got, FAULTS)
           if rc != w_rc or sub not in msg]
    assert not bad, "\n".join(map(repr, bad))
    assert [rc for rc, _ in got[len(FAULTS):]] == [0] * len(NOOPS)


def test_ops_enhance_multi_rejects_host_tensors():
    """Host tensors never reach the library: the device check comes first (there is no CPU path)."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    ne, n, nc = 6, 8, 2
    x = torch.linspace(-1, 1, ne + 1, dtype=torch.float64)
    U = torch.zeros((nc, ne + 1), dtype=torch.float64)
    t = torch.ones((ne, n), dtype=torch.float64)
    f = torch.ones((nc, ne, n), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.enhance_multi(x, U, 5, 1e4, n, t, t, f, global_domain=(-1.0, 1.0))
    with pytest.raises(TypeError, match="torch.Tensor"):
        ops.enhance_multi(x.numpy(), U, 5, 1e4, n, t, t, f, global_domain=(-1.0, 1.0))


@pytest.mark.parametrize("bad,match", [
    (dict(U=(2, 8)), "U must be"), (dict(U=(3, 7)), "rhs_values must be"), (dict(U=(7,)), "U must be"), (dict(a=(6, 7)), "a_values must be"),
    (dict(da=(8, 6)), "da_values must be"), (dict(c=(6, 9)), "c_values must be"),
    (dict(f=(3, 6, 8)), "rhs_values must be"), (dict(f=(6, 8)), "rhs_values must be"),
    (dict(f=(2, 8, 6)), "rhs_values must be"), (dict(pm=True), "point-major")])
def test_ops_enhance_multi_rejects_mismatched_shapes(bad, match):
    """Shapes are checked on the tensors' metadata before anything is handed to the library: ne = 6, n = 8, two
    cases, element-major unless ``pm``."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64)                         # noqa: E731
    x = torch.linspace(-1, 1, 7, dtype=torch.float64)
    with pytest.raises(ValueError, match=match):
        ops.enhance_multi(x, z(*bad.get("U", (2, 7))), 5, 1e4, 8, z(*bad.get("a", (6, 8))), z(*bad.get("da", (6, 8))),
                          z(*bad.get("f", (2, 6, 8))), c_values=z(*bad.get("c", (6, 8))),
                          point_major=bad.get("pm", False), global_domain=(-1.0, 1.0))


if __name__ == "__main__" and sys.argv[1:] == ["--faults"]:
    sys.path.insert(0, ROOT)
    print(json.dumps(_run_faults()))
