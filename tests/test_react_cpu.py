"""CPU: the host side of the reaction term -(a u')' + c u = f -- the four new entries are exported, declared and
bound (additive: the ABI stays 7), each rejects every single bad argument before any HIP call (child process that
sees no GPU), the facade validates ``reaction``, and the float64 restatement the GPU tests compare against agrees
with its own 60-digit solve."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lssvr_hip.h")
NEW = ["lssvr_enhance_react", "lssvr_enhance_react_ws", "lssvr_p1_assemble_react", "lssvr_estimate_react"]

_F = [0x10000 * (i + 1) for i in range(16)]        # fake device pointers: never dereferenced
_ENH = dict(x=_F[0], u=_F[1], ne=10, elem_offset=0, ne_global=10, gxmin=-1.0, gxmax=1.0, bc_left=0.0, bc_right=0.0,
            M=9, n_colloc=16, gamma=1e4, a_values=_F[2], da_values=_F[3], c_values=_F[4], rhs_values=_F[5],
            W=_F[6], status=_F[7], fail_count=None, stream=None)
_ENH_WS = dict(x=_F[0], u=_F[1], ne=10, elem_offset=0, ne_global=10, gxmin=-1.0, gxmax=1.0, bc_left=0.0,
               bc_right=0.0, M=9, n_colloc=16, gamma=1e4, a_values=_F[2], da_values=_F[3], c_values=_F[4],
               rhs_values=_F[5], table_layout=1, W=_F[6], status=_F[7], fail_count=None, work=None, work_bytes=0,
               stream=None, kernel_ms_host=None)
_P1 = dict(x=_F[0], ne=10, nquad=2, rhs_id=0, rhs_params_host=None, rhs_quad=_F[1], a_quad=_F[2], c_quad=_F[3],
           diag=_F[4], off=_F[5], load=_F[6], kloc=None, floc=None, stream=None)
_EST = dict(x=_F[0], W=_F[1], ne=10, M=9, nq=16, a_values=_F[2], da_values=_F[3], c_values=_F[4], rhs_values=_F[5],
            table_layout=0, a_ends=_F[6], eta2=_F[7], jump=None, out3=_F[8], work=_F[9], stream=None)

# (overrides, rc, message substring): one broken rule each; no case may reach a launch
_ENH_FAULTS = [({"x": None}, -1, "non-NULL"), ({"u": None}, -1, "non-NULL"), ({"W": None}, -1, "non-NULL"),
               ({"a_values": None}, -1, "non-NULL"), ({"da_values": None}, -1, "non-NULL"),
               ({"rhs_values": None}, -1, "non-NULL"), ({"c_values": None}, -1, "c_values"),
               ({"ne": -1}, -2, "ne"), ({"ne_global": 9}, -2, "shard"), ({"elem_offset": -1}, -2, "shard"),
               ({"M": 1}, -3, "M = 1"), ({"M": 34}, -3, "M = 34"),
               ({"n_colloc": 1}, -2, "n_colloc"), ({"n_colloc": 4097}, -2, "n_colloc"),
               ({"gamma": 0.0}, -2, "gamma"),
               ({"M": 22, "n_colloc": 19}, -5, "M-2"), ({"M": 33, "n_colloc": 30}, -5, "M-2")]
FAULTS = {
    "lssvr_enhance_react": (_ENH, _ENH_FAULTS),
    "lssvr_enhance_react_ws": (_ENH_WS, _ENH_FAULTS + [
        ({"table_layout": 2}, -2, "unknown table_layout"), ({"table_layout": -1}, -2, "unknown table_layout"),
        ({"work_bytes": -1}, -1, "work"), ({"work_bytes": 64}, -1, "work")]),
    "lssvr_p1_assemble_react": (_P1, [
        ({"x": None}, -1, "non-NULL"), ({"diag": None}, -1, "non-NULL"), ({"off": None}, -1, "non-NULL"),
        ({"load": None}, -1, "non-NULL"), ({"rhs_quad": None}, -4, "rhs_quad"),
        ({"rhs_id": 1}, -4, "rhs_params"), ({"rhs_id": 7}, -4, "unknown rhs_id"),
        ({"ne": 0}, -2, "ne"), ({"ne": -3}, -2, "ne"), ({"nquad": 0}, -7, "nquad"), ({"nquad": 6}, -7, "nquad"),
        # without c_quad the call IS lssvr_p1_assemble: same checks
        ({"c_quad": None, "nquad": 6}, -7, "nquad"), ({"c_quad": None, "x": None}, -1, "non-NULL")]),
    "lssvr_estimate_react": (_EST, [
        ({"x": None}, -1, "non-NULL"), ({"W": None}, -1, "non-NULL"), ({"eta2": None}, -1, "non-NULL"),
        ({"out3": None}, -1, "non-NULL"), ({"work": None}, -1, "non-NULL"),
        ({"a_values": None}, -1, "non-NULL"), ({"da_values": None}, -1, "non-NULL"),
        ({"rhs_values": None}, -1, "non-NULL"), ({"c_values": None}, -1, "c_values"),
        ({"a_ends": None}, -1, "a_ends"),
        ({"ne": 0}, -2, "ne"), ({"ne": -1}, -2, "ne"), ({"ne": (1 << 40) + 1}, -2, "too large"),
        ({"M": 0}, -3, "M = 0"), ({"M": 34}, -3, "M = 34"),
        ({"nq": 0}, -7, "nq"), ({"nq": 33}, -7, "nq"),
        ({"table_layout": 2}, -2, "unknown table_layout"), ({"table_layout": -1}, -2, "unknown table_layout")]),
}


def _run_faults():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    out = {}
    for name, (valid, faults) in FAULTS.items():
        rows = []
        for over, _, _ in faults:
            args = dict(valid, **over)
            assert list(args) == list(valid)
            rc = getattr(lib, name)(*args.values())
            rows.append((rc, lib.lssvr_last_error().decode()))
        out[name] = rows
    return out


def test_error_codes_are_the_headers():
    src = open(HEADER).read()
    for name, val in (("LSSVR_ERR_NULL", -1), ("LSSVR_ERR_SIZE", -2), ("LSSVR_ERR_DEGREE", -3),
                      ("LSSVR_ERR_RHS", -4), ("LSSVR_ERR_SOLVER", -5), ("LSSVR_ERR_QUAD", -7)):
        assert any(line.split()[:3] == ["#define", name, "(%d)" % val] or line.split()[:3] == ["#define", name, str(val)]
                   for line in src.splitlines()), name


def test_react_entries_exported_declared_and_bound():
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    src = open(HEADER).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name + "(" in src, name
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(FAULTS[name][0]), name
    assert lib.lssvr_version() == _capi.ABI_VERSION == 7          # additive: no ABI bump
    assert "#define LSSVR_ABI_VERSION 7" in src


def test_react_single_faults_without_gpu():
    """Every single bad argument of every new entry returns its code and message on the host: the calls run in
    a child process with no GPU visible, so a check that sat behind a HIP call would fail there."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="4096", ROCR_VISIBLE_DEVICES="4096")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--faults"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    bad = []
    for name, (_, faults) in FAULTS.items():
        assert len(got[name]) == len(faults)
        bad += [(name, over, rc, msg, w_rc, sub) for (rc, msg), (over, w_rc, sub) in zip(got[name], faults)
                if rc != w_rc or sub not in msg]
    assert not bad, "\n".join(map(repr, bad))


def _one(x):
    return 1.0 + 0.0 * x


def _zero(x):
    return 0.0 * x


@pytest.mark.parametrize("reaction", [1.0, "c", (_one,), np.ones(3)])
def test_facade_rejects_reaction_that_is_not_callable(reaction):
    import hybrid_fem_lssvr_amd as pkg
    with pytest.raises(ValueError, match="reaction"):
        pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, reaction=reaction)


def test_facade_rejects_reaction_with_flux_solver():
    import hybrid_fem_lssvr_amd as pkg
    with pytest.raises(ValueError, match="flux"):
        pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, reaction=_one, fem_solver="flux")


def test_facade_rejects_reaction_with_other_solvers():
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import ops
    for sid in (ops.SOLVER_DUAL, ops.SOLVER_PRIMAL_WAVE, ops.SOLVER_PRIMAL_MOMENT, ops.SOLVER_SHARED):
        with pytest.raises(ValueError, match="SOLVER_PRIMAL"):
            pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, reaction=_one, solver=sid)


def test_facade_accepts_reaction_with_and_without_coef():
    import hybrid_fem_lssvr_amd as pkg
    assert pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, reaction=_one).coef is None
    s = pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9, coef=(_one, _zero), reaction=_one)
    assert s.reaction is _one and s.coef == (_one, _zero)
    assert pkg.FEMLSSVRPrimalSolver(9, lssvr_M=9).reaction is None


@pytest.mark.parametrize("k", [1.0, 1e4])
@pytest.mark.parametrize("ne,M,n", [(2000, 9, 16), (300, 20, 32), (100, 26, 40), (25, 9, 16)])
def test_restatement_agrees_with_its_60_digit_solve(ne, M, n, k):
    """Both float64 solves of the restated system against the 60-digit minimiser of the same QP on elements 0,
    ne/3, ne-1: measured 2e-14 or better on these inputs, so the GPU tests' bars (1e-11 / 1e-10 against the
    restatement, 1e-13 against the minimiser) are reachable.  The bar here is 1e-13, the one the kernels get."""
    from oracle import closed_form_mp as cf
    from oracle import lssvr_oracle as orc
    if not cf.HAVE_MP:
        pytest.skip("mpmath not importable")
    a, da, c, f = orc.react_functions(k)
    nodes = np.linspace(-1, 1, ne + 1)
    values = np.sin(np.pi * nodes)
    sel = [0, ne // 3, ne - 1]
    kw = dict(elements=sel, coef_a=a, coef_da=da, coef_c=c)
    tr = cf.truth_all(nodes, values, M, 1e4, n, f, **kw)
    for solver in ("bc_elim", "primal"):
        W, _ = orc.enhance_all(nodes, values, M, 1e4, n, rhs=f, solver=solver, **kw)
        err = orc.rel_l2_coef(W, tr).max()
        print(f"ne={ne} M={M} n={n} k={k:g} {solver}: {err:.2e}")
        assert err <= 1e-13


def test_p1_restatement_is_the_old_one_without_c():
    from oracle import lssvr_oracle as orc
    a, da, c, f = orc.react_functions(1.0)
    nodes = np.linspace(-1, 1, 38)
    d, o, ld, k = orc.p1_bands(nodes, f, a, 3, lambda x: 0.0 * x)
    d0, o0, l0 = orc.p1_scatter(*orc.p1_assemble_local(nodes, f, a, 3))
    assert np.array_equal(d, d0) and np.array_equal(o, o0) and np.array_equal(ld, l0)
    # manufactured u = sin(pi x): the P1 solve with the mass matrix converges at second order
    errs = []
    for ne in (40, 80):
        x = np.linspace(-1, 1, ne + 1)
        errs.append(np.max(np.abs(orc.fem_p1_solve(x, f, a, 3, c) - np.sin(np.pi * x))))
    assert errs[1] < errs[0] / 3.5


if __name__ == "__main__" and sys.argv[1:] == ["--faults"]:
    sys.path.insert(0, ROOT)
    print(json.dumps(_run_faults()))
