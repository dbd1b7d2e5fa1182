"""CPU: the step memo's sizing and validation (lssvr_step_plan_memo_bytes / lssvr_step_plan_memo_bind) are host
arithmetic on the plan -- they run without a GPU, on fake pointers that are never dereferenced."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = [0x10000 * (i + 1) for i in range(8)]


def _create(lib, ne=100, M=9, n=16):
    from hybrid_fem_lssvr_amd import _capi
    rhs = _capi.rhs_params(9.869604401089358, 3.141592653589793)
    h = ctypes.c_void_p()
    rc = lib.lssvr_step_plan_create(ctypes.byref(h), FAKE[0], FAKE[1], ne, 0, ne, -1.0, 1.0, 0.0, 0.0, M, n, 1e4,
                                    rhs, 2, FAKE[2], FAKE[3], FAKE[4], FAKE[5], FAKE[6], None)
    return rc, h


def _formula(M, ne):
    """3 (M-2) - 2 planes of ne rounded up to 64 doubles (none at M = 2: no loop), then the ne + 1 keys."""
    planes = max(3 * (M - 2) - 2, 0)
    return 8 * (planes * ((ne + 63) // 64 * 64) + ne + 1)


@pytest.mark.parametrize("M", [2, 3, 9, 22])
@pytest.mark.parametrize("ne", [1, 63, 64, 65])
def test_memo_bytes_formula(M, ne):
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    rc, h = _create(lib, ne=ne, M=M, n=max(16, 2 * M))
    assert rc == 0 and h.value
    try:
        assert lib.lssvr_step_plan_memo_bytes(h) == _formula(M, ne)
    finally:
        lib.lssvr_step_plan_destroy(h)


def test_memo_bytes_zero_without_a_fused_step():
    """M = 23 runs the MFMA kernels; n = M - 2 at M = 14 is the near-square regime with refinement steps (two
    launches): neither has a memo.  A NULL plan has none either."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    for M, n in ((23, 46), (14, 12)):
        rc, h = _create(lib, M=M, n=n)
        assert rc == 0 and h.value, (M, n)
        try:
            assert lib.lssvr_step_plan_memo_bytes(h) == 0, (M, n)
            assert lib.lssvr_step_plan_memo_bind(h, FAKE[7], 1 << 30, None) == -5, (M, n)    # LSSVR_ERR_SOLVER
            assert b"memo" in lib.lssvr_last_error()
        finally:
            lib.lssvr_step_plan_destroy(h)
    assert lib.lssvr_step_plan_memo_bytes(None) == 0


# The failing binds run in a child process that sees no GPU: a check moved behind the fill launch would fail there
# with a HIP error (LSSVR_ERR_LAUNCH = -6) instead of its own code.
_CHILD = r"""
import ctypes, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from hybrid_fem_lssvr_amd import _capi
import test_step_memo_cpu as t
lib = _capi.load()
rc, h = t._create(lib)
assert rc == 0 and h.value
nb = lib.lssvr_step_plan_memo_bytes(h)
assert nb == t._formula(9, 100)
memo = t.FAKE[7]
assert lib.lssvr_step_plan_memo_bind(None, memo, nb, None) == -1                       # NULL plan
assert lib.lssvr_step_plan_memo_bind(h, memo, nb - 8, None) == -2                      # short buffer
assert b"memo_bytes" in lib.lssvr_last_error()
assert lib.lssvr_step_plan_memo_bind(h, memo + 4, nb, None) == -2                      # misaligned pointer
assert b"aligned" in lib.lssvr_last_error()
assert lib.lssvr_step_plan_memo_bind(h, None, 0, None) == 0                            # unbind: no launch
assert lib.lssvr_step_plan_destroy(h) == 0
print("memo-bind-checks-ok")
"""


def test_memo_bind_rejects_before_any_hip_call():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    src = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    r = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "memo-bind-checks-ok" in r.stdout, r.stdout + r.stderr


def test_create_is_still_host_arithmetic():
    """lssvr_step_plan_create: no HIP call, no device memory -- a plan is created, sized and destroyed here, and a
    failed create still leaves a NULL handle."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    rc, h = _create(lib)
    assert rc == 0 and h.value and lib.lssvr_step_plan_memo_bytes(h) > 0
    assert lib.lssvr_step_plan_destroy(h) == 0
    rc, h = _create(lib, M=40)
    assert rc < 0 and not h.value
