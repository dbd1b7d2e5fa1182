"""CPU: adjoint sensitivities of the Newmark loop where there is no GPU -- the library's host
mirrors against the numpy restatement bit for bit, the backward sweep and the sums against the complex step, chunk
independence, the negative control, the argument errors of the four entries and the facade's refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import wave_sensitivity_rules as wr

proto = wr.proto
D, R = wr.D, wr.R


@pytest.mark.parametrize("damped", [False, True], ids=["undamped", "damped"])
@pytest.mark.parametrize("mode", wr.MODES)
@pytest.mark.parametrize("ne", [1, 2, 5, 33])
def test_advance_host_mirror_is_the_numpy_restatement(ne, mode, damped):
    """Every output is bit-equal, with no ulp allowance: each value is a chain of single IEEE operations in a written
    order, which numpy reproduces; what a mode does not write keeps its canaries."""
    for seed in range(3):
        d = wr.advance_inputs(ne, seed)
        for nm in (0, 1):
            for with_p in (True, False):
                wr.check_advance(wr.advance_host(d, mode, damped, nm, with_p),
                                 wr.advance_numpy(d, mode, damped, nm, with_p))


@pytest.mark.parametrize("nR", [0, 2, 8])
@pytest.mark.parametrize("m", [1, 3, 8])
@pytest.mark.parametrize("ne", [1, 2, 7, 33])
def test_sensitivity_host_mirror_is_the_numpy_restatement(ne, m, nR):
    """Every output is bit-equal; every NULL-output combination leaves what was not asked for untouched (and the
    trajectory only it reads is not handed over); an accumulating call continues from what the outputs hold."""
    tabs = wr.TABLES if nR else wr.TABLES[:4]
    for n0 in (0, 3):          # a chunk that ends at level 0, and one further in
        d = wr.kernel_inputs(ne, m, nR, n0)
        for nq in (1, 2, 5):
            for kinds in ((D, D), (R, D), (D, R), (R, R)):
                wr.check_against(wr.sens_host(d, nq, tabs, kinds, ends=True)[1], tabs, wr.sens_numpy(d, nq, kinds), True)
            init = wr.initial(d, nq)
            ref0, ref1 = wr.sens_numpy(d, nq), wr.sens_numpy(d, nq, (R, D), init)
            for want in wr.wants(nR):
                if want:
                    wr.check_against(wr.sens_host(d, nq, want)[1], want, ref0, False)
                wr.check_against(wr.sens_host(d, nq, want, (R, D), ends=True, init=init)[1], want, ref1, True, init)


@pytest.mark.parametrize("c", wr.cpu_cases(), ids=lambda c: c.id)
def test_adjoint_against_complex_step(c):
    """The prototype's trajectories and adjoint states through the library's host mirror in chunks of 8, against the
    complex-step derivative of every table entry, initial value and end datum: within 10x the prototype's own
    reading."""
    dev_by_group, adj, cs = c.reference
    lam, B, ub, vb = proto.backward(c.p, adj["P"])
    got = wr.host_sweep(c.p, adj["U"], adj["V"], adj["A"], lam, B, ub, vb, 8)
    dev = c.deviation(got)
    print(f"{c.id}: host mirror {dev:.2e}, prototype {c.read:.2e}, bar {c.bar:.2e}; "
          + " ".join(f"{k} {v:.1e}" for k, v in dev_by_group.items()))
    assert dev <= c.bar
    assert c.read <= wr.READ_SLACK * wr.READ[c.ne]          # the prototype itself stays where it was measured
    assert ("d" in got) == c.damped
    for s, end in ((0, 0), (1, -1)):
        if c.kinds[s] == D:
            assert np.all(lam[:, end] == 0.0) and got["u0"][end] == 0.0 and got["kappa"][s] == 0.0
        else:
            assert got["accel0"][s] == 0.0


@pytest.mark.parametrize("c", [wr.case(33, 2, (D, R), 17, True, 1, "random"), wr.case(7, 5, (R, R), 9, False, 0, "observe")],
                         ids=lambda c: c.id)
def test_chunking_does_not_change_a_bit(c):
    """A sweep in chunks of 8, 3 and 1 gives the same tables and end gradients bit for bit: every sum continues from
    the stored value, so the order of the additions does not depend on the cut.  And the numpy sums are those bits."""
    _, adj, _ = c.reference
    lam, B, ub, vb = proto.backward(c.p, adj["P"])
    args = (c.p, adj["U"], adj["V"], adj["A"], lam, B, ub, vb)
    ref = wr.host_sweep(*args, 8)
    groups = [k for k in proto.GROUPS if k in ref]
    for size in (3, 1):
        got = wr.host_sweep(*args, size)
        for k in groups:
            assert np.array_equal(got[k], ref[k]), (size, k)
    num = proto.sweep_gradients(*args, None, 8)
    for k in groups:
        assert np.array_equal(num[k], ref[k]), k


NEGATIVE_CONTROL_FACTOR = 1e12          # the prototype reads 3.4e+00 against a bar of 3.8e-14: 8.9e13


def test_negative_control_abar_without_the_velocity_bar():
    """abar* = abar in the place of abar + c_va vbar: on the damped N = 3 case with gamma = 0.6 the gradients are far
    off."""
    c = wr.case(*wr.CONTROL)
    adj = c.reference[1]
    lam, B, ub, vb = proto.backward(c.p, adj["P"], wrong=True)
    got = wr.host_sweep(c.p, adj["U"], adj["V"], adj["A"], lam, B, ub, vb, 8)
    dev = c.deviation(got)
    print(f"without c_va vbar the sweep reads {dev:.2e}, the bar is {c.bar:.2e}: factor {dev / c.bar:.2e}")
    assert dev > NEGATIVE_CONTROL_FACTOR * c.bar


CHILD = r'''
import ctypes, sys
sys.path.insert(0, sys.argv[1])
import wave_sensitivity_rules as wr
import numpy as np
from hybrid_fem_lssvr_amd import _capi
lib = _capi.load()
hp, D, R = wr._hp, wr.D, wr.R
a = wr.advance_inputs(4)
ka = {k: wr._c(a[k]) for k in ("lam", "Vbar", "Abar", "P", "mdiag", "moff", "ddiag", "doff")}
oa = {k: np.zeros(5) for k in "vaub"}

def adv(**change):
    v = dict(lam=hp(ka["lam"]), Vbar=hp(ka["Vbar"]), Abar=hp(ka["Abar"]), P=hp(ka["P"]), mdiag=hp(ka["mdiag"]),
             moff=hp(ka["moff"]), ddiag=hp(ka["ddiag"]), doff=hp(ka["doff"]), ne=4, dt=0.1, beta=0.25, gamma=0.5,
             v=hp(oa["v"]), a=hp(oa["a"]), u=hp(oa["u"]), b=hp(oa["b"]))
    assert set(change) <= set(v)
    v.update(change)
    return list(v.values())

nan, inf = float("nan"), float("inf")
ADV = ((dict(ne=0), -2, b"ne = 0"), (dict(dt=0.0), -2, b"must be finite and > 0"), (dict(dt=nan), -2, b"finite"),
       (dict(beta=-1.0), -2, b"finite and > 0"), (dict(beta=inf), -2, b"finite"), (dict(gamma=0.0), -2, b"finite and > 0"),
       (dict(gamma=nan), -2, b"finite"), (dict(Vbar=None), -1, b"Vbar, Abar"), (dict(Abar=None), -1, b"Vbar, Abar"),
       (dict(lam=None, b=None, v=None, a=None, u=None), -1, b"B_out must be non-NULL without lam"),
       (dict(lam=None), -2, b"must be NULL without lam"), (dict(mdiag=None), -1, b"mdiag, moff"),
       (dict(moff=None), -1, b"mdiag, moff"), (dict(ddiag=None), -1, b"ddiag and doff go together"),
       (dict(doff=None), -1, b"ddiag and doff go together"), (dict(v=None), -1, b"V_out, A_out"),
       (dict(a=None), -1, b"V_out, A_out"), (dict(v=hp(ka["Vbar"])), -2, b"none of them an input"),
       (dict(b=hp(ka["lam"])), -2, b"none of them an input"), (dict(u=hp(oa["b"])), -2, b"must be distinct"),
       (dict(a=hp(ka["mdiag"])), -2, b"none of them an input"))
s = wr.kernel_inputs(4, 3, 2, 1)
ks = {k: wr._c(s[k]) for k in ("x", "Utraj", "Vtraj", "Atraj", "Z", "Brows", "phi", "band_ends")}
o = wr.blank(s, 2)

def sens(**change):
    v = dict(x=hp(ks["x"]), ne=4, nq=2, U=hp(ks["Utraj"]), V=hp(ks["Vtraj"]), A=hp(ks["Atraj"]), Z=hp(ks["Z"]), n0=1,
             m=3, phi=hp(ks["phi"]), R=2, ga=hp(o["a"]), gc=hp(o["c"]), grho=hp(o["rho"]), gd=hp(o["d"]), gf=hp(o["f"]),
             acc=0, B=hp(ks["Brows"]), be=hp(ks["band_ends"]), k0=D, k1=R, g=hp(o["g"]), kap=hp(o["kappa"]))
    assert set(change) <= set(v)
    v.update(change)
    return list(v.values())

none5 = dict(ga=None, gc=None, grho=None, gd=None, gf=None)
SENS = ((dict(ne=0), -2, b"ne = 0"), (dict(m=0), -2, b"m = 0"), (dict(m=9), -2, b"m = 9"), (dict(n0=-1), -2, b"n0 = -1"),
        (dict(R=-1), -2, b"R = -1"), (dict(R=9), -2, b"R = 9"), (dict(R=0), -2, b"R = 0 is allowed only with gf NULL"),
        (dict(k1=2), -2, b"end kinds"), (dict(nq=0), -7, b"nquad = 0"), (dict(nq=6), -7, b"nquad = 6"),
        (dict(x=None), -1, b"x, Utraj, Z"), (dict(U=None), -1, b"x, Utraj, Z"), (dict(Z=None), -1, b"x, Utraj, Z"),
        (dict(none5, g=None, kap=None), -1, b"one of ga, gc, grho, gd, gf, out_g"),
        (dict(phi=None), -1, b"phi must be non-NULL with gf"), (dict(V=None), -1, b"Vtraj must be non-NULL with gd"),
        (dict(A=None), -1, b"Atraj must be non-NULL with grho"), (dict(kap=None), -1, b"out_g and out_kappa"),
        (dict(g=None), -1, b"out_g and out_kappa"), (dict(B=None), -1, b"Brows and band_ends"),
        (dict(be=None), -1, b"Brows and band_ends"), (dict(ga=hp(ks["Z"])), -2, b"none of them an input"),
        (dict(gc=hp(o["a"])), -2, b"must be distinct"), (dict(g=hp(ks["Brows"])), -2, b"none of them an input"))

def dev(args):
    return [v if v is None or isinstance(v, (int, float)) else ctypes.cast(v, ctypes.c_void_p).value for v in args]

for host, device, args, table in ((lib.lssvr_newmark_adjoint_advance_host, lib.lssvr_newmark_adjoint_advance, adv, ADV),
                                  (lib.lssvr_newmark_sensitivity_host, lib.lssvr_newmark_sensitivity, sens, SENS)):
    assert host(*args()) == 0
    for change, code, word in table:
        rc = host(*args(**change))
        assert rc == code and word in lib.lssvr_last_error(), ("host", change, rc, lib.lssvr_last_error())
        # the device entry: the same checks, before any launch (the pointers are host addresses: nothing may launch)
        rc = device(*dev(args(**change)), None)
        assert rc == code and word in lib.lssvr_last_error(), ("device", change, rc, lib.lssvr_last_error())
# what is allowed: the first call; no damping; the ends alone; R = 0 and no phi without gf; no trajectories without
# their tables; without out_g neither Brows, band_ends nor the kinds are read
assert lib.lssvr_newmark_adjoint_advance_host(*adv(lam=None, v=None, a=None, u=None, mdiag=None, moff=None)) == 0
assert lib.lssvr_newmark_adjoint_advance_host(*adv(ddiag=None, doff=None, P=None, u=None)) == 0
assert lib.lssvr_newmark_sensitivity_host(*sens(**none5)) == 0
assert lib.lssvr_newmark_sensitivity_host(*sens(gf=None, R=0, phi=None, gd=None, V=None, grho=None, A=None)) == 0
assert lib.lssvr_newmark_sensitivity_host(*sens(g=None, kap=None, B=None, be=None, k0=7, k1=7)) == 0
print("ROWS", len(ADV) + len(SENS))
'''


def test_argument_errors_in_a_child_that_sees_no_gpu():
    """Each broken argument of the four entries is refused with its code and a word of lssvr_last_error(), one
    mistake per row, in a child process without a visible GPU: nothing can have been launched."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", CHILD, here], env=env, capture_output=True, text=True, cwd=wr.ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ROWS 45" in r.stdout


def test_ops_wrappers_check_on_the_host():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros(5, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.newmark_sensitivity(t, t.view(1, 5), t.view(1, 5), 0)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.newmark_adjoint_advance(None, t, t, None, None, None, None, 0.1, 0.25, 0.5)


def _one(x):
    return 1.0 + 0.0 * x


_OBS = dict(goal=None, observe=([0, 2], [0.0], [[1.0], [0.5]]))
REFUSALS = [
    ("convection", dict(convection=_one, fem_solver="pivot"), {}, "has no convection term"),
    ("periodic", dict(boundary="periodic", reaction=_one), {}, "has no boundary='periodic'"),
    ("pivot", dict(fem_solver="pivot"), {}, "needs fem_solver='bands'"),
    ("nonlinear", dict(nonlinear=("poly", [_one])), {}, "solve_wave_sensitivity has no semilinear form"),
    ("beta", {}, dict(beta=0.1), "unconditionally stable"),
    ("v0", {}, dict(_v0=3.0), "v0 must be a callable"),
    ("damping", {}, dict(damping=2.0), "damping must be a callable"),
    ("accel0", {}, dict(end_data=(_one, 0.0)), "end_accel0"),
    ("neither", {}, dict(goal=None), "solve_wave_sensitivity needs exactly one of goal"),
    ("both", {}, dict(observe=_OBS["observe"]), "exactly one of goal"),
    ("goal not callable", {}, dict(goal=3.0), "goal must be a callable j(x)"),
    ("goal step below", {}, dict(goal_steps=[-1]), "goal_steps must be step indices in 0 .. nsteps = 4"),
    ("goal step beyond", {}, dict(goal_steps=[2, 5]), "goal_steps must be step indices"),
    ("goal step twice", {}, dict(goal_steps=[2, 2]), "goal_steps must not name a step twice"),
    ("non-finite goal", {}, dict(goal=lambda x: np.full_like(x, np.nan)), "goal is not finite at a quadrature point"),
    ("goal_steps with observe", {}, dict(_OBS, goal_steps=[1]), "goal_steps and goal_weights belong to goal="),
    ("observe not a triple", {}, dict(goal=None, observe=([0.0], [1.0])), "observe must be a triple"),
    ("observe step", {}, dict(goal=None, observe=([5], [0.0], [[1.0]])), "observe steps must be step indices"),
    ("observe step twice", {}, dict(goal=None, observe=([1, 1], [0.0], [[1.0], [1.0]])), "must not name a step twice"),
    ("observe shape", {}, dict(goal=None, observe=([1, 2], [0.0], [[1.0]])), "d_obs must be [len(steps), nobs] = [2, 1]"),
    ("observe non-finite", {}, dict(goal=None, observe=([2], [0.0], [[np.nan]])), "observe d_obs is not finite"),
    ("observe outside", {}, dict(goal=None, observe=([2], [1.5], [[0.0]])), "every x_obs must lie in the mesh"),
    ("too large", {}, dict(max_state_bytes=2 * 5 * 9 * 8 - 1), "checkpointing"),
    ("too large, damped", {}, dict(damping=_one, max_state_bytes=3 * 5 * 9 * 8 - 1), "3 (nsteps+1)(ne+1) 8"),
    ("nsteps", {}, dict(nsteps=0), "nsteps must be an integer >= 1"),
]


def test_facade_refusals(monkeypatch):
    """Every refusal is a ValueError with its reason, raised before the library is loaded or a device looked up."""
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import _capi, solver

    def forbidden(*a, **k):
        raise AssertionError("a device call was reached before the refusal")
    monkeypatch.setattr(_capi, "load", forbidden)
    monkeypatch.setattr(solver, "_device", forbidden)
    for name, ctor, kw, match in REFUSALS:
        kw = {"goal": _one, "nsteps": 4, **kw}
        v0 = kw.pop("_v0", _one)
        s = pkg.FEMLSSVRPrimalSolver(9, **ctor)
        with pytest.raises(ValueError, match=re.escape(match)):
            s.solve_wave_sensitivity(_one, v0, 0.1, **kw)
            raise AssertionError(f"{name}: not refused")
    # what is not refused reaches the device: the same size as the "too large" cases, to the byte; step 0 counts
    for kw in (dict(goal=_one, max_state_bytes=2 * 5 * 9 * 8), dict(goal=_one, damping=_one, max_state_bytes=3 * 5 * 9 * 8),
               dict(_OBS), dict(goal=_one, goal_steps=[0, 4])):
        with pytest.raises(AssertionError, match="device call"):
            pkg.FEMLSSVRPrimalSolver(9).solve_wave_sensitivity(_one, _one, 0.1, nsteps=4, **kw)


def test_demo_record_of_the_prototype():
    """The inverse problem of the prototype: the misfit falls monotonically, to the recorded value."""
    hist = proto.demo()
    assert all(b < a for a, b in zip(hist, hist[1:]))
    assert abs(hist[-1] - wr.DEMO_FINAL) <= 1e-6 * wr.DEMO_FINAL
