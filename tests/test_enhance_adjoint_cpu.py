"""The adjoint of the element solve without a GPU: the numpy prototype against its own complex
step, the negative control, lssvr_enhance_adjoint_host against the numpy restatement bit for bit, every refusal of the
entry, the symbols, and the refusals of ops.enhance_adjoint and of the facade before any device call."""
import os
import re

import numpy as np
import pytest

import enhance_adjoint_rules as R
from enhance_adjoint_rules import proto

ROOT = R.ROOT
SYMBOLS = ("lssvr_enhance_adjoint_work_bytes", "lssvr_enhance_adjoint", "lssvr_enhance_adjoint_host")


@pytest.mark.parametrize("c", R.all_cases(), ids=lambda c: c.id)
def test_prototype_reading_stays_within_read(c):
    reading = c.reference[0]
    print(f"{c.id}: reading {reading:.2e}")
    assert reading <= R.READ_SLACK * R.READ[(c.M, c.n)]


@pytest.mark.parametrize("c", [R.case(7, M, n, True, True) for M, n in R.PAIRS + (R.SQUARE,)], ids=lambda c: c.id)
def test_negative_control_reads_far_above_the_bar(c):
    assert proto.negative_control(c) > 1.0e3 * c.bar


@pytest.mark.parametrize("c", R.all_cases(), ids=lambda c: c.id)
def test_host_mirror_equals_the_restatement(c):
    want = c.wants()
    _, got = R.adjoint_host(c, want)
    R.check_against(got, want, c.restatement)
    assert np.array_equal(got["pairs"], c.restatement["pairs"])


@pytest.mark.parametrize("want", (("f",), ("u",), ("bc", "a"), ("da", "c")), ids="-".join)
def test_host_mirror_skips_null_outputs(want):
    c = R.case(65, 9, 16, True, True)
    R.check_against(R.adjoint_host(c, want)[1], want, c.restatement)


def test_host_mirror_shards_and_fallback():
    c = R.case(65, 4, 8, True, True)
    _, got = R.adjoint_host(c, R.OUTPUTS, rows=(10, 40), elem_offset=10, ne_global=65)
    assert np.array_equal(got["pairs"], c.restatement["pairs"][10:40]) and np.all(got["bc"] == 0.0)
    c = R.case(7, 9, 16, True, True)
    st = np.zeros(7, dtype=np.int32)
    st[3] = 1
    f = c.f.copy()
    f[3] = np.nan
    _, got = R.adjoint_host(c, R.OUTPUTS, status=st, f=f)
    ref = proto.kernel_adjoint(c.x, c.M, c.n, c.gamma, f, c.W, c.Wbar, c.a, c.da, c.c, status=st)
    assert np.array_equal(got["pairs"], ref["pairs"])
    assert np.array_equal(got["pairs"][3], [0.5 * (c.Wbar[3, 0] - c.Wbar[3, 1]), 0.5 * (c.Wbar[3, 0] + c.Wbar[3, 1])])
    for k in R.TABLES:
        assert np.array_equal(got[k], ref[k]) and np.all(got[k][3] == 0.0) and np.all(np.isfinite(got[k]))


def _codes():
    from hybrid_fem_lssvr_amd import _capi
    text = open(os.path.join(ROOT, "include", "lssvr_hip.h")).read()
    return {k: int(re.search(rf"#define {k}\s+\((-?\d+)\)", text).group(1))
            for k in ("LSSVR_ERR_SIZE", "LSSVR_ERR_DEGREE", "LSSVR_ERR_NULL")}, _capi


REFUSALS = [
    ("LSSVR_ERR_SIZE", dict(ne=0)), ("LSSVR_ERR_SIZE", dict(n=6)), ("LSSVR_ERR_SIZE", dict(n=65)),
    ("LSSVR_ERR_SIZE", dict(elem_offset=1)), ("LSSVR_ERR_SIZE", dict(elem_offset=-1)),
    ("LSSVR_ERR_SIZE", dict(work_bytes=8)), ("LSSVR_ERR_DEGREE", dict(M=2)), ("LSSVR_ERR_DEGREE", dict(M=17)),
    ("LSSVR_ERR_NULL", dict(x=None)), ("LSSVR_ERR_NULL", dict(f=None)), ("LSSVR_ERR_NULL", dict(W=None)),
    ("LSSVR_ERR_NULL", dict(Wbar=None)), ("LSSVR_ERR_NULL", dict(work=None)),
    ("LSSVR_ERR_NULL", dict(gu=None, gbc=None, ga=None, gda=None, gc=None, gf=None)),
    ("LSSVR_ERR_NULL", dict(a=None, da=None)), ("LSSVR_ERR_NULL", dict(a=None, da=None, ga=None)),
    ("LSSVR_ERR_NULL", dict(c=None)), ("LSSVR_ERR_NULL", dict(a=None, ga=None, gda=None)),
]


@pytest.mark.parametrize("code,override", REFUSALS, ids=lambda v: v if isinstance(v, str) else "-".join(v))
def test_entry_refusals_write_nothing(code, override):
    codes, _ = _codes()
    c = R.case(7, 9, 16, True, True)
    rc, got = R.adjoint_host(c, R.OUTPUTS, check=False, override=override)
    assert rc == codes[code]
    for k in R.OUTPUTS + ("pairs",):
        assert np.all(got[k] == R.CANARY), k


def test_symbols_in_header_library_and_binding():
    from hybrid_fem_lssvr_amd import _capi
    text = open(os.path.join(ROOT, "include", "lssvr_hip.h")).read()
    lib = _capi.load()
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\(", text) and name in _capi.SIGNATURES and hasattr(lib, name)
        assert not name.startswith("lssvr_ts_")
    assert lib.lssvr_version() == 7
    assert lib.lssvr_enhance_adjoint_work_bytes(300) == 300 * 16


# ---- ops.enhance_adjoint and the facade on a fake library: nothing reaches the device --------------------------------------
class _FakeLib:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called: the check must come before any library call")


def test_ops_refusals(monkeypatch):
    import torch
    from hybrid_fem_lssvr_amd import _capi, ops
    monkeypatch.setattr(_capi, "load", lambda: _FakeLib())
    t = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.enhance_adjoint(t, t, t, 9, 1e4, 16, t)
    with pytest.raises(TypeError):
        ops.enhance_adjoint(np.zeros(8), t, t, 9, 1e4, 16, t)


class _FakeCuda:
    """A stand-in for a device tensor: passes ops._dev, holds a shape, has no memory."""

    def __init__(self, *shape):
        import torch
        self.shape, self.dtype, self.is_cuda, self.device = shape, torch.float64, True, "cuda:0"

    def dim(self):
        return len(self.shape)

    def numel(self):
        return int(np.prod(self.shape))

    def is_contiguous(self):
        return True


@pytest.mark.parametrize("kw,match", [
    (dict(M=2), "M must be"), (dict(M=17), "M must be"), (dict(n=6), "n_colloc"), (dict(n=65), "n_colloc"),
    (dict(want=()), "want"), (dict(want=("u", "u")), "want"), (dict(want=("z",)), "want"),
    (dict(want=("a",)), "a_values"), (dict(want=("c",)), "c_values"), (dict(da=True), "da_values needs"),
    (dict(W=(7, 8)), "W must hold"), (dict(f=(7, 15)), "rhs_values must hold")])
def test_ops_argument_checks(monkeypatch, kw, match):
    from hybrid_fem_lssvr_amd import _capi, ops
    monkeypatch.setattr(_capi, "load", lambda: _FakeLib())
    monkeypatch.setattr(ops.torch, "Tensor", _FakeCuda)
    M, n = kw.get("M", 9), kw.get("n", 16)
    x, W = _FakeCuda(8), _FakeCuda(*kw.get("W", (7, M)))
    f = _FakeCuda(*kw.get("f", (7, n)))
    with pytest.raises(ValueError, match=match):
        ops.enhance_adjoint(x, W, _FakeCuda(7, M), M, 1e4, n, f, want=kw.get("want", ("u", "f")),
                            da_values=_FakeCuda(7, n) if kw.get("da") else None, global_domain=(-1.0, 1.0))


def _solver(**kw):
    import hybrid_fem_lssvr_amd as pkg
    base = dict(mesh=proto.mesh(7), nquad=2, rhs=R.p1proto.rhs, lssvr_M=9, n_colloc=16, fem_solver="bands")
    base.update(kw)
    return pkg.FEMLSSVRPrimalSolver(**base)


@pytest.mark.parametrize("kw,call,match", [
    (dict(lssvr_M=2), {}, "lssvr_M"), (dict(lssvr_M=17, n_colloc=20), {}, "lssvr_M"), (dict(n_colloc=6), {}, "n_colloc"),
    (dict(boundary="periodic"), {}, "periodic"), ({}, dict(of="w"), "of must be"),
    ({}, dict(goal=None), "exactly one"), ({}, dict(goal=None, observe=([2.0], [0.0])), "lie in the mesh"),
    (dict(fem_solver="flux"), {}, "flux")])
def test_facade_refusals_before_any_device_call(monkeypatch, kw, call, match):
    from hybrid_fem_lssvr_amd import _capi
    monkeypatch.setattr(_capi, "load", lambda: _FakeLib())
    s = _solver(**kw)
    monkeypatch.setattr(s, "solve_fem", lambda: (_ for _ in ()).throw(AssertionError("solve_fem was reached")))
    args = dict(goal=R.p1proto.goal_density, of="enhanced")
    args.update(call)
    with pytest.raises(ValueError, match=match):
        s.solve_sensitivity(**args)


def test_of_p1_issues_todays_calls(monkeypatch):
    """The default path: the same checks and calls as before, in the same order, and nothing of the new path."""
    import hybrid_fem_lssvr_amd.solver as sm
    s = _solver()
    seen = []
    monkeypatch.setattr(s, "_check_sensitivity", lambda g, o: (seen.append("check"), (None, None))[1])
    monkeypatch.setattr(s, "solve_fem", lambda: (_ for _ in ()).throw(KeyboardInterrupt("reached solve_fem")))
    monkeypatch.setattr(s, "_solve_sensitivity_enhanced", lambda g, o: seen.append("enhanced"))
    for kw in ({}, dict(of="p1")):
        with pytest.raises(KeyboardInterrupt):
            s.solve_sensitivity(R.p1proto.goal_density, **kw)
    assert seen == ["check", "check"]
    assert sm.FEMLSSVRPrimalSolver.solve_sensitivity.__kwdefaults__["of"] == "p1"
