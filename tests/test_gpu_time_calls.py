"""GPU: the sequence of ``ops`` calls of the three time loops (DESIGN.md sections 26, 28, 29) -- solve_transient with
BDF1 and BDF2, solve_transient(nonlinear=...) and solve_wave without and with damping, each with and without the
enhanced snapshots -- held against literal lists, and the one device-to-host copy each makes once its loop runs.  The
lists pin what the host code between the launches does: a change of the loops that adds, drops or reorders a launch
fails here before it shows in a number."""
import functools
import math
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NODES = np.array([-1.0, -0.55, -0.2, 0.3, 0.62, 1.0])          # 5 elements, non-uniform
CPU = "Tensor.cpu"


def _zero(x):
    return np.zeros_like(np.asarray(x, dtype=np.float64))


def _one(x):
    return np.ones_like(np.asarray(x, dtype=np.float64))


def _solve(name, enhance):
    import hybrid_fem_lssvr_amd as pkg
    s = pkg.FEMLSSVRPrimalSolver(len(NODES), lssvr_M=9, lssvr_gamma=1e4, n_colloc=16, mesh=NODES,
                                 global_domain=(-1.0, 1.0), boundary=(("robin", 2.0, 0.0), ("dirichlet", 0.0)),
                                 coef=(lambda x: 1.0 + 0.5 * np.sin(2.0 * x), lambda x: np.cos(2.0 * x)),
                                 reaction=lambda x: 0.5 + 0.3 * np.cos(3.0 * x))
    kw = dict(nsteps=3, snapshots=[2, 3], enhance=enhance, weight=lambda x: 1.0 + 0.4 * x * x,
              forcing=[(lambda t: math.exp(-t), lambda x: np.sin(math.pi * x)), (1.0, lambda x: x * x)],
              end_data=(lambda t: 0.3 * math.cos(t), 0.0))
    u0 = lambda x: np.where(np.asarray(x) == 1.0, 0.0, np.cos(0.5 * math.pi * x))      # noqa: E731
    if name.startswith("wave"):
        return s.solve_wave(u0, _zero, 0.3, damping=(lambda x: 0.6 + 0.4 * np.sin(2.0 * x)) if name == "wave-damped"
                            else None, **kw)
    if name == "newton":
        kw.update(nonlinear=("poly", [_zero, _zero, _zero, _one]), newton_iters=2, newton_tol=1.0)
    return s.solve_transient(u0, 0.3, scheme="bdf1" if name == "bdf1" else "bdf2", **kw)


def record(monkeypatch, name, enhance):
    """The names of the public ``ops`` functions in the order the solve reaches them (calls that one of them makes to
    another included), with CPU where a tensor is copied to the host."""
    import torch
    from hybrid_fem_lssvr_amd import ops
    calls = []

    def logged(label, fn):
        @functools.wraps(fn)
        def wrapper(*a, **k):
            calls.append(label)
            return fn(*a, **k)
        return wrapper
    for nm, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and not nm.startswith("_") and fn.__module__ == ops.__name__:
            monkeypatch.setattr(ops, nm, logged(nm, fn))
    monkeypatch.setattr(torch.Tensor, "cpu", logged(CPU, torch.Tensor.cpu))
    sol = _solve(name, enhance)
    assert sol.nodal.shape == (2, len(NODES)) and len(sol.enhanced) == (2 if enhance else 0)
    return calls


# the launch that opens each loop (solve_wave: the one that writes the first step's right-hand side)
LOOP_OPENS = {"bdf1": "ts_rhs", "bdf2": "ts_rhs", "newton": "ts_rhs", "wave": "wave_advance",
              "wave-damped": "wave_advance"}
# after the loop has started: the ONE read-back of the snapshots, the bands and the monitor (the enhancement reads
# nothing back)
COPIES_IN_AND_AFTER_THE_LOOP = 1
EXPECTED = {
    ("bdf1", False): [
        "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "ts_rhs", "tridiag_bc_solve_multi", "ts_rhs",
        "tridiag_bc_solve_multi", "ts_rhs", "tridiag_bc_solve_multi"],
    ("bdf1", True): [
        "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "ts_rhs", "tridiag_bc_solve_multi", "ts_rhs",
        "tridiag_bc_solve_multi", "ts_source_table", "ts_rhs", "tridiag_bc_solve_multi", "ts_source_table",
        "enhance_multi"],
    ("bdf2", False): [
        "p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "ts_rhs",
        "tridiag_bc_solve_multi", "ts_rhs", "tridiag_bc_solve_multi", "ts_rhs", "tridiag_bc_solve_multi"],
    ("bdf2", True): [
        "p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "ts_rhs",
        "tridiag_bc_solve_multi", "ts_rhs", "tridiag_bc_solve_multi", "ts_source_table", "ts_rhs",
        "tridiag_bc_solve_multi", "ts_source_table", "enhance_multi"],
    ("newton", False): [
        "p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "ts_rhs", "ts_nl_assemble",
        "nl_kind", "tridiag_bc_solve_multi", "nl_residual", "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi",
        "nl_residual", "ts_rhs", "nl_step", "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi", "nl_residual",
        "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi", "nl_residual", "ts_rhs", "nl_step", "ts_nl_assemble",
        "nl_kind", "tridiag_bc_solve_multi", "nl_residual", "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi",
        "nl_residual"],
    ("newton", True): [
        "p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "ts_rhs", "ts_nl_assemble",
        "nl_kind", "tridiag_bc_solve_multi", "nl_residual", "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi",
        "nl_residual", "ts_rhs", "nl_step", "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi", "nl_residual",
        "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi", "nl_residual", "ts_source_table", "nl_linearize",
        "nl_kind", "ts_rhs", "nl_step", "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi", "nl_residual",
        "ts_nl_assemble", "nl_kind", "tridiag_bc_solve_multi", "nl_residual", "ts_source_table", "nl_linearize",
        "nl_kind", "enhance_varcoef", "enhance_varcoef"],
    ("wave", False): [
        "p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "eig_apply",
        "tridiag_bc_solve_multi", "wave_advance", "tridiag_bc_solve_multi", "wave_advance", "tridiag_bc_solve_multi",
        "wave_advance", "eig_apply", "tridiag_bc_solve_multi", "wave_advance", "eig_apply"],
    ("wave", True): [
        "p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "eig_apply",
        "tridiag_bc_solve_multi", "wave_advance", "tridiag_bc_solve_multi", "wave_advance", "tridiag_bc_solve_multi",
        "wave_advance", "eig_apply", "ts_source_table", "tridiag_bc_solve_multi", "wave_advance", "eig_apply",
        "ts_source_table", "enhance_multi"],
    ("wave-damped", False): [
        "p1_assemble", "p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "eig_apply",
        "eig_apply", "tridiag_bc_solve_multi", "wave_advance", "tridiag_bc_solve_multi", "wave_advance",
        "tridiag_bc_solve_multi", "wave_advance", "eig_apply", "tridiag_bc_solve_multi", "wave_advance", "eig_apply"],
    ("wave-damped", True): [
        "p1_assemble", "p1_assemble", "p1_assemble", "p1_assemble", "p1_load_multi", "tridiag_work", "eig_apply",
        "eig_apply", "tridiag_bc_solve_multi", "wave_advance", "tridiag_bc_solve_multi", "wave_advance",
        "tridiag_bc_solve_multi", "wave_advance", "eig_apply", "ts_source_table", "ts_source_table",
        "tridiag_bc_solve_multi", "wave_advance", "eig_apply", "ts_source_table", "ts_source_table", "enhance_multi"],
}


@pytest.mark.parametrize("enhance", [False, True])
@pytest.mark.parametrize("name", ["bdf1", "bdf2", "newton", "wave", "wave-damped"])
def test_call_sequence_and_one_copy(dev, monkeypatch, name, enhance):
    calls = record(monkeypatch, name, enhance)
    print(name, enhance, calls)
    assert [c for c in calls if c != CPU] == EXPECTED[name, enhance]
    assert calls[calls.index(LOOP_OPENS[name]):].count(CPU) == COPIES_IN_AND_AFTER_THE_LOOP
