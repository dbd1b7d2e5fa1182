"""CPU: wave problems where there is no GPU -- the host mirror of lssvr_wave_advance against a
plain numpy restatement bit for bit, its argument errors, the numpy prototype with the host mirror in its loop against
the discrete mode, the energy bounds, the fixed point and the temporal order, and the facade's refusals."""
import math

import numpy as np
import pytest

import wave_rules as wr

proto = wr.proto


@pytest.mark.parametrize("beta,gamma", wr.NEWMARK)
@pytest.mark.parametrize("damped", [False, True])
@pytest.mark.parametrize("R", [1, 2, 8])
@pytest.mark.parametrize("nc", [1, 3, 8])
@pytest.mark.parametrize("ne", [1, 2, 5, 33])
def test_advance_host_is_the_numpy_restatement(ne, nc, R, damped, beta, gamma):
    """All three modes bit for bit, what a mode does not write is left alone, and the fused call equals the split
    pair (state only, then the first-step mode on the new state)."""
    d = wr.kernel_inputs(ne, nc, R)
    got = {}
    for label, kw in wr.modes_of(d, damped):
        got[label] = wr.advance_host(dt=wr.KERNEL_DT, beta=beta, gamma=gamma, **kw)[1:]
        want = wr.advance_numpy(dt=wr.KERNEL_DT, beta=beta, gamma=gamma, **kw)
        for g, w, nm in zip(got[label], want, ("V_out", "Acc_out", "rhs_out")):
            if g is None:
                assert label == "state" and nm == "rhs_out"
            else:
                assert np.array_equal(g, w, equal_nan=True), (label, nm)
    assert np.all(np.isnan(got["first"][0])) and np.all(np.isnan(got["first"][1]))
    v, acc, _ = got["state"]
    dd, do = (d["dd"], d["do"]) if damped else (None, None)
    split = wr.advance_host(None, d["U_new"], v, acc, d["md"], d["mo"], dd, do, d["loads"], d["phi"], wr.KERNEL_DT,
                            beta, gamma)[3]
    assert np.array_equal(split, got["fused"][2])
    assert np.array_equal(v, got["fused"][0]) and np.array_equal(acc, got["fused"][1])


def test_argument_errors():
    """Aliasing, both modes NULL and the range errors return the error code and write nothing (the device entry
    validates before it launches, so it can be called here with host addresses standing in)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    d = wr.kernel_inputs(4, 2, 2)
    ok = dict(U_new=d["U_new"], U=d["U"], V=d["V"], Acc=d["Acc"], md=d["md"], mo=d["mo"], dd=d["dd"], do=d["do"],
              loads=d["loads"], phi=d["phi"], dt=0.1, beta=0.25, gamma=0.5)
    assert wr.advance_host(**ok, check=False)[0] == 0
    keep = {k: np.array(v) for k, v in d.items()}

    def outs():
        return tuple(np.full((2, 5), 7.0) for _ in range(3))

    def refused(code, o=None, **change):
        o = outs() if o is None else o
        rc = wr.advance_host(**{**ok, **change}, check=False, outs=o)[0]
        assert rc == code, (change, rc)
        for t in o:
            if t is not None and all(t is not v for v in d.values()):
                assert np.all(t == 7.0), change
        for k, v in d.items():
            assert np.array_equal(v, keep[k]), (change, k)

    for bad in (dict(dt=0.0), dict(dt=-0.1), dict(dt=math.inf), dict(dt=math.nan), dict(beta=0.0), dict(beta=math.nan),
                dict(gamma=0.0), dict(gamma=-0.5), dict(gamma=math.inf), dict(nc=0), dict(nc=9), dict(R=0), dict(R=9)):
        refused(-2, **bad)
    a, b, c = outs()
    refused(-2, o=(d["V"], b, c))                  # V_out is V
    refused(-2, o=(d["Acc"], b, c))                # V_out is Acc
    refused(-2, o=(a, d["V"], c))                  # Acc_out is V
    refused(-2, o=(a, d["Acc"], c))                # Acc_out is Acc
    refused(-2, o=(a, a, c))                       # the two outputs are one
    refused(-2, o=(a, b, d["U"]))                  # rhs_out is an input
    refused(-2, o=(a, b, a))                       # rhs_out is V_out
    refused(-2, o=(a, b, None), U_new=None)        # both modes NULL
    assert b"NULL" in lib.lssvr_last_error()
    refused(-1, o=(None, b, c))                    # V_out missing with U_new
    refused(-1, V=None)
    refused(-1, md=None)
    refused(-1, do=None)                           # ddiag without doff
    addr = [d[k].ctypes.data for k in ("U_new", "U", "V", "Acc", "md", "mo", "dd", "do", "loads", "phi")]
    o = outs()
    tail = [t.ctypes.data for t in o]
    assert lib.lssvr_wave_advance(*addr, 4, 0, 2, 0.1, 0.25, 0.5, *tail, None) == -2           # nc < 1, no launch
    assert lib.lssvr_wave_advance(*addr, 4, 2, 2, 0.1, 0.25, 0.5, addr[2], tail[1], tail[2], None) == -2     # aliasing
    assert lib.lssvr_wave_advance(None, *addr[1:], 4, 2, 2, 0.1, 0.25, 0.5, tail[0], tail[1], None, None) == -2
    assert lib.lssvr_wave_advance(*addr, 0, 2, 2, 0.1, 0.25, 0.5, *tail, None) == -2           # ne < 1
    assert all(np.all(t == 7.0) for t in o)


def test_ops_wrapper_rejects_host_tensors_and_aliasing():
    import torch
    from hybrid_fem_lssvr_amd import ops
    t = torch.zeros((1, 5), dtype=torch.float64)
    with pytest.raises(RuntimeError, match="device memory"):
        ops.wave_advance(t, t, t, t, t[0], t[0, :4], None, None, t, torch.zeros((1, 1), dtype=torch.float64), 0.1,
                         0.25, 0.5)
    with pytest.raises(ValueError, match="nothing to compute"):
        ops.wave_advance(None, t, t, t, None, None, None, None, None, None, 0.1, 0.25, 0.5, rhs=False)


@pytest.mark.parametrize("ne", wr.MODE_NE)
def test_discrete_mode(ne):
    """u^n = cos(n theta) u0, theta = 2 atan(omega_h dt / 2): the prototype with the host mirror in its loop, within
    10x the prototype's own reading."""
    case = wr.mode(ne)
    r = case.run(adv_fn=wr.advance_host_fn)
    err, bar = wr.mode_error(case, ne, r["nodal"]), wr.mode_bar(ne)
    print(f"mode ne={ne}: host mirror {err:.2e}, prototype {bar / wr.MARGIN:.2e}, bar {bar:.2e}")
    assert err <= bar
    # the prototype itself stays at rounding level: acc' = (u' - ut) / (beta dt^2) cancels to eps / (beta dt^2 omega^2)
    # ~ 3e-12 relative, which reaches u through dt v over the 40 steps as ~ 1e-13
    assert bar <= wr.MARGIN * 1e-12
    # the mode does move: cos(40 theta) is well away from 1
    assert np.max(np.abs(r["nodal"][-1] - case.u0(case.nodes))) > 1e-2 * case.scale


def test_energy_bounds():
    """d = 0, f = 0: the average-acceleration rule conserves E (float64 and longdouble prototypes, host mirror in the
    loop); d > 0: E does not increase; gamma = 0.6: E decays without damping."""
    case = wr.energy_case()
    read64, readl = (wr.energy_drift(case.run(t)["energy"]) for t in (np.float64, np.longdouble))
    bar = wr.energy_bar()
    drift = wr.energy_drift(case.run(adv_fn=wr.advance_host_fn)["energy"])
    print(f"energy drift: host mirror {drift:.2e}, prototype {read64:.2e}, longdouble {readl:.2e}, bar {bar:.2e}")
    assert drift <= bar and readl <= read64 + wr.FLOOR and read64 <= 1e-11
    e = case.run(adv_fn=wr.advance_host_fn)
    assert np.max(np.abs(e["nodal"][-1] - case.u0(case.nodes))) > 0.1          # no frozen vector
    damped = wr.energy_case(d=wr.damping).run(adv_fn=wr.advance_host_fn)["energy"]
    assert wr.energy_rise(damped) <= bar and damped[-1] < 0.9 * damped[0]
    lossy = wr.energy_case(beta=0.3025, gamma=0.6).run(adv_fn=wr.advance_host_fn)["energy"]
    assert wr.energy_rise(lossy) <= bar and lossy[-1] < lossy[0] * (1.0 - 1e-3)


@pytest.mark.parametrize("damped", [False, True])
def test_stationary_solution_is_a_fixed_point(damped):
    case, ustat = wr.stationary(wr.damping if damped else None)
    r = case.run(adv_fn=wr.advance_host_fn)
    err, bar = wr.stationary_error(ustat, r["nodal"]), wr.stationary_bar(damped)
    print(f"fixed point damped={damped}: host mirror {err:.2e}, prototype {bar / wr.MARGIN:.2e}")
    assert err <= bar and bar <= wr.MARGIN * 1e-13


def test_temporal_order():
    """The standing wave on 2048 elements at 8 / 16 / 32 steps: second order, the bar the prototype's order - 0.1."""
    errs, orders = proto.temporal_orders(adv_fn=wr.advance_host_fn)
    bar = wr.order_bar()
    print(f"errors {errs}, orders {orders}, bar {bar:.3f}")
    assert all(o >= bar for o in orders) and 1.8 <= bar <= 2.1


def test_first_acceleration_and_moving_end():
    """The general case: acc0 holds g''(0) at the moving Dirichlet end, and the float64 loop with the host mirror in it
    stays within rounding of the longdouble loop in u, v and acc (each with its own bar)."""
    case, ref, p64 = wr.references("general-33")
    assert float(p64["accel0"][-1]) == case.end_accel0[1]
    got = wr.loop_reading("general-33", case.run(adv_fn=wr.advance_host_fn))
    for k, (err, bar, read) in got.items():
        print(f"{k}: host mirror {err:.2e}, prototype {read:.2e}, bar {bar:.2e}")
        assert err <= bar and read <= 1e-9          # acc carries eps / (beta dt^2) = 1e-11 per step


def test_facade_refusals(monkeypatch):
    wr.tr.check_refusals(monkeypatch, wr.call_wave, wr.refusals(), wr.passing())


def test_accuracy_record_of_the_prototype():
    """The standing wave on 8, 16, 32 elements: the enhanced snapshot is closer to u than the P1 interpolant."""
    for ne, e_p1, e_enh in proto.accuracy_record():
        print(f"ne={ne}: interpolant {e_p1:.4e}, enhanced {e_enh:.4e}")
        if ne in wr.ACCURACY:
            want = wr.ACCURACY[ne]
            assert abs(e_p1 - want[0]) <= 5e-4 * want[0] and abs(e_enh - want[1]) <= 5e-4 * want[1]
        assert e_enh < e_p1
