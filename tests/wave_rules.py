"""Shared cases and bars of the wave tests: tests/test_wave_cpu.py runs them through the numpy
prototype and the library's host mirror, tests/test_gpu_wave.py through the device.

The bars follow section 26's rule.  Every "within rounding" bar is 10x what the float64 prototype
(scripts/proto/wave_proto.py, LAPACK's banded LU) itself reads on the SAME case against a better reference -- the
closed form of the discrete mode, or the same loop in np.longdouble --, with a floor of 4 eps.  The reading is taken
when the test runs (cached), never from the code under test; the figures read when the cases were written are recorded
beside them."""
import functools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import wave_proto as proto              # noqa: E402
import transient_rules as tr            # noqa: E402
from oracle import lssvr_oracle as orc  # noqa: E402,F401

EPS = 2.0 ** -52
FLOOR = 4.0 * EPS
MARGIN = 10.0
DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN
NEWMARK = ((0.25, 0.5), (0.3025, 0.6))          # average acceleration, and a damped pair with beta = (gamma + 1/2)^2 / 4


_zero, _hp, _h = tr._zero, tr._hp, tr._h


class Case:
    """One wave problem: what proto.solve takes, and the facade's constructor and call arguments."""

    def __init__(self, name, nodes, u0, v0, t_end, nsteps, a=None, da=None, c=None, rho=None, d=None, forcing=None,
                 kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), end_data=(0.0, 0.0), end_accel0=(0.0, 0.0),
                 snapshots=None, beta=0.25, gamma=0.5):
        self.name, self.nodes, self.u0, self.v0, self.t_end, self.nsteps = name, nodes, u0, v0, t_end, nsteps
        self.a, self.da, self.c, self.rho, self.d, self.forcing = a, da, c, rho, d, forcing
        self.kinds, self.kappa, self.end_data, self.end_accel0 = kinds, kappa, end_data, end_accel0
        self.snapshots = [nsteps] if snapshots is None else list(snapshots)
        self.beta, self.gamma = beta, gamma
        self.scale = float(np.max(np.abs(u0(nodes))))

    @property
    def dt(self):
        return self.t_end / self.nsteps

    def run(self, dtype=np.float64, **kw):
        return proto.solve(self.nodes, self.u0, self.v0, self.t_end, self.nsteps, a=self.a, c=self.c, rho=self.rho,
                           d=self.d, forcing=self.forcing, kinds=self.kinds, kappa=self.kappa, end_data=self.end_data,
                           end_accel0=self.end_accel0, snapshots=self.snapshots, beta=self.beta, gamma=self.gamma,
                           dtype=dtype, **kw)

    def facade(self, M=9, n_colloc=16, gamma_reg=1e4):
        """(constructor kwargs, solve_wave kwargs) of the same problem."""
        bnd = tuple(("dirichlet", 0.0) if k == DIRICHLET else ("robin", kp, 0.0)
                    for k, kp in zip(self.kinds, self.kappa))
        ctor = dict(num_fem_nodes=len(self.nodes), lssvr_M=M, lssvr_gamma=gamma_reg, n_colloc=n_colloc,
                    mesh=self.nodes, global_domain=(float(self.nodes[0]), float(self.nodes[-1])), boundary=bnd,
                    coef=None if self.a is None else (self.a, self.da), reaction=self.c)
        call = dict(nsteps=self.nsteps, weight=self.rho, damping=self.d, end_data=self.end_data,
                    end_accel0=self.end_accel0, forcing=[(0.0, _zero)] if not self.forcing else self.forcing,
                    snapshots=self.snapshots, beta=self.beta, gamma=self.gamma)
        return ctor, call


def _mesh33(seed=29):
    w = np.random.default_rng(seed).uniform(0.5, 1.5, 32)
    nodes = -1.0 + 2.0 * np.concatenate([[0.0], np.cumsum(w)]) / np.sum(w)
    nodes[-1] = 1.0
    return nodes


# ---- the discrete mode: a = rho = 1, zero Dirichlet ends, u0 the first eigenvector of (K, M) on a uniform mesh, v0 = 0 ---
MODE_NE = (2, 5, 32, 33)
MODE_DT, MODE_STEPS = 0.01, 40
# max_n |u^n - cos(n theta) u0|_inf / |u0|_inf.  ne: the float64 prototype when the cases were written
MODE_READ = {2: 1.0e-13, 5: 3.0e-13, 32: 1.7e-13, 33: 4.0e-13}


def mode(ne):
    nodes = np.linspace(-1.0, 1.0, ne + 1)

    def u0(x):
        v = np.sin(math.pi * (np.asarray(x, dtype=np.float64) + 1.0) / 2.0)
        return np.where(np.abs(np.asarray(x)) == 1.0, 0.0, v)
    return Case(f"mode-{ne}", nodes, u0, _zero, MODE_DT * MODE_STEPS, MODE_STEPS,
                snapshots=list(range(1, MODE_STEPS + 1)))


def mode_error(case, ne, nodal):
    """max_n |u^n - cos(n theta) u0|_inf / |u0|_inf with theta = 2 atan(omega_h dt / 2),
    omega_h^2 = (6 / h^2)(1 - cos s)/(2 + cos s), s = pi / ne."""
    h, s = 2.0 / ne, math.pi / ne
    om = math.sqrt((6.0 / h ** 2) * (1.0 - math.cos(s)) / (2.0 + math.cos(s)))
    th = 2.0 * math.atan(0.5 * om * MODE_DT)
    cosn = np.cos(th * np.arange(1, MODE_STEPS + 1))
    return float(np.max(np.abs(np.asarray(nodal) - cosn[:, None] * case.u0(case.nodes)[None, :]))) / case.scale


@functools.lru_cache(maxsize=None)
def mode_bar(ne):
    case = mode(ne)
    return max(MARGIN * mode_error(case, ne, case.run()["nodal"]), FLOOR)


# ---- energy: d = 0, f = 0, variable a, c, rho, non-uniform 33-node mesh, Robin left, Dirichlet-0 right, 64 steps ------
def energy_case(d=None, beta=0.25, gamma=0.5):
    return Case("energy-33" + ("" if d is None else "-damped") + ("" if gamma == 0.5 else f"-gamma{gamma}"), _mesh33(),
                lambda x: np.where(np.asarray(x) == 1.0, 0.0, np.cos(0.5 * math.pi * np.asarray(x, dtype=np.float64))
                                   * (1.0 + 0.3 * np.asarray(x, dtype=np.float64))),
                lambda x: np.where(np.asarray(x) == 1.0, 0.0, 0.5 * np.sin(math.pi * (1.0 - np.asarray(x)))),
                1.28, 64, a=lambda x: 1.0 + 0.5 * np.sin(2.0 * x), da=lambda x: np.cos(2.0 * x),
                c=lambda x: 0.5 + 0.3 * np.cos(3.0 * x), rho=lambda x: 1.0 + 0.4 * x * x, d=d,
                kinds=(ROBIN, DIRICHLET), kappa=(2.0, 0.0), snapshots=list(range(1, 65)), beta=beta, gamma=gamma)


def damping(x):
    return 0.6 + 0.4 * np.sin(2.0 * np.asarray(x, dtype=np.float64))


def energy_drift(energy):
    """max_n |E^n - E^0| / E^0."""
    e = np.asarray(energy, dtype=np.float64)
    return float(np.max(np.abs(e[1:] - e[0])) / e[0])


def energy_rise(energy):
    """max_n (E^{n+1} - E^n)^+ / E^0: 0 for a non-increasing sequence."""
    e = np.asarray(energy, dtype=np.float64)
    return float(max(0.0, np.max(np.diff(e))) / e[0])


@functools.lru_cache(maxsize=None)
def energy_bar():
    """10x the float64 prototype's own drift on the undamped case (its longdouble loop drifts by rounding of that type
    only: the rule conserves E exactly)."""
    return max(MARGIN * energy_drift(energy_case().run()["energy"]), FLOOR)


# max_n |E^n - E^0| / E^0 of the undamped case: (float64 prototype, np.longdouble prototype)
ENERGY_READ = (1.5e-13, 2.3e-14)


# ---- a general problem: the 33-node mesh, variable a, c, rho, d, Robin left, moving Dirichlet right, R = 2 ---------------
def general(nsteps=64, snapshots=(32, 64), d=damping):
    return Case("general-33" + ("" if d is not None else "-undamped"), _mesh33(26), lambda x: np.cos(x),
                lambda x: 0.6 * np.asarray(x, dtype=np.float64) ** 2,
                0.64, nsteps, a=lambda x: 1.0 + 0.5 * np.sin(2.0 * x), da=lambda x: np.cos(2.0 * x),
                c=lambda x: 0.5 + 0.3 * np.cos(3.0 * x), rho=lambda x: 1.0 + 0.4 * x * x, d=d,
                forcing=[(lambda t: math.exp(-t), lambda x: np.sin(math.pi * x)),
                         (lambda t: math.cos(2.0 * t), lambda x: x * x)],
                kinds=(ROBIN, DIRICHLET), kappa=(2.0, 0.0),
                # right end: g = cos(1) + 0.2 sin(3 t) + t^2 / 2: g(0) = u0(1), g'(0) = 0.6 = v0(1), g''(0) = 1
                end_data=(lambda t: 0.3 * math.cos(t),
                          lambda t: math.cos(1.0) + 0.2 * math.sin(3.0 * t) + 0.5 * t * t),
                end_accel0=(0.0, 1.0), snapshots=list(snapshots))


CASES = {"general-33": general, "general-33-undamped": lambda: general(d=None)}
# max over the snapshots against the np.longdouble loop on the device's bands, scaled by |u0|_inf, |v|_inf, |acc|_inf of
# the reference.  name: (u, v, acc) of the float64 prototype when the cases were written
LOOP_READ = {"general-33": (3.7e-13, 2.4e-12, 4.1e-11)}

# What the device assembled is shared only after it has been held, array by array, against the oracle's assembly
# (section 26's bar and reasoning: 32 eps of the entry's scale).
BANDS_BAR = 32.0 * EPS


def bands_error(case, bands):
    """max over (mass, damp, stiff, step, loads) of |device - oracle| / scale."""
    want = proto.assemble(case.nodes, case.dt, case.beta, case.gamma, case.a, case.c, case.rho, case.d,
                          [f for _, f in case.forcing] if case.forcing else [_zero])

    def matrix(got, ref):
        (gd, go), (wd, wo) = got, ref
        assert gd.shape == wd.shape and go.shape == wo.shape
        sc = np.abs(wd)
        return max(float(np.max(np.abs(gd - wd) / sc)), float(np.max(np.abs(go - wo) / np.maximum(sc[:-1], sc[1:]))))

    worst = 0.0
    for k in ("mass", "stiff", "step"):
        worst = max(worst, matrix(bands[k], want[k]))
    assert (bands["damp"] is None) == (want["damp"] is None)
    if want["damp"] is not None:
        worst = max(worst, matrix(bands["damp"], want["damp"]))
    assert bands["loads"].shape == want["loads"].shape
    for got_r, want_r in zip(bands["loads"], want["loads"]):
        sc = float(np.max(np.abs(want_r)))
        worst = max(worst, float(np.max(np.abs(got_r - want_r))) / sc if sc > 0.0 else float(np.max(np.abs(got_r))))
    return worst


def references(name, bands=None):
    """(case, np.longdouble loop, float64 loop), computed once per (name, bands)."""
    return tr.references(CASES, name, bands)


def loop_reading(name, got, bands=None):
    """{field: (error of ``got[field]``, bar, the float64 prototype's own error)} for nodal, velocity and accel: max
    |. - the np.longdouble prototype|_inf over the snapshots, scaled by the reference's own max; bar 10x the
    prototype's.  accel carries 1 / dt^2, so it is read and barred on its own."""
    case, ref, p64 = references(name, bands)
    out = {}
    for k in ("nodal", "velocity", "accel"):
        sc = float(np.max(np.abs(ref[k])))
        err, read = (float(np.max(np.abs(np.asarray(v[k], dtype=np.longdouble) - ref[k]))) / sc for v in (got, p64))
        out[k] = (err, max(MARGIN * read, FLOOR), read)
    return out


# ---- the stationary solution: v0 = 0, f steady, u0 the P1 solution ----------------------------------------------------------
def stationary(d=None):
    g = general()
    f = lambda x: np.sin(math.pi * x) + x * x      # noqa: E731
    gl, gr = 0.3, -0.2
    kd, ko, load, _ = orc.p1_bands(g.nodes, f, g.a, 2, g.c)
    ustat = proto.bc_solve(kd, ko, load, g.kinds, g.kappa, (gl, gr))
    case = Case("stationary" + ("" if d is None else "-damped"), g.nodes, lambda x: ustat, _zero, 0.05, 5, a=g.a,
                da=g.da, c=g.c, rho=g.rho, d=d, forcing=[(1.0, f)], kinds=g.kinds, kappa=g.kappa, end_data=(gl, gr),
                snapshots=[1, 2, 3, 4, 5])
    return case, ustat


def stationary_error(ustat, nodal):
    return float(np.max(np.abs(np.asarray(nodal) - ustat[None, :]))) / float(np.max(np.abs(ustat)))


@functools.lru_cache(maxsize=None)
def stationary_bar(damped):
    case, ustat = stationary(damping if damped else None)
    return max(MARGIN * stationary_error(ustat, case.run()["nodal"]), FLOOR)


# ---- temporal order: the standing wave on 2048 elements, 8 / 16 / 32 steps to t = 0.8 -------------------------------------
# the prototype's orders when the cases were written
ORDER_READ = (1.996, 2.000)


@functools.lru_cache(maxsize=None)
def order_bar():
    """The prototype's measured order minus 0.1 (the gap between the finite-step order and its limit)."""
    return min(proto.temporal_orders()[1]) - 0.1


# ---- the enhanced snapshots -------------------------------------------------------------------------------------------------
ENH_FAMILY_BAR = 1e-11          # the reaction-row tests' bar against the float64 restatement, M <= 22
ENH_CASES = ((9, 16), (20, 24))


def enhanced_rows(name, M, n_colloc, gamma_reg=1e4, dtype=np.float64, bands=None):
    """W [ns, ne, M] of the case's snapshots: the oracle's rows on the prototype's u, v, acc computed in ``dtype``."""
    case, ref, p64 = references(name, bands)
    r = p64 if dtype == np.float64 else ref
    fl = [f for _, f in case.forcing] if case.forcing else [_zero]
    return np.stack([proto.enhance_snapshot(case.nodes, r["nodal"][k], r["velocity"][k], r["accel"][k],
                                            r["phi"][k] if case.forcing else [0.0], fl, M, gamma_reg, n_colloc,
                                            a=case.a, da=case.da, c=case.c, rho=case.rho, d=case.d, kinds=case.kinds,
                                            g=r["g"][k])
                     for k in range(len(case.snapshots))])


def enhanced_reference(name, M, n_colloc, bands=None):
    """(W of the np.longdouble loop's data, the family's bar 1e-11, the noise the float64 loop's own rounding -- amplified
    by 1 / dt^2 in acc -- puts into W; recorded, it does not widen the bar)."""
    Wl = enhanced_rows(name, M, n_colloc, dtype=np.longdouble, bands=bands)
    W64 = enhanced_rows(name, M, n_colloc, bands=bands)
    noise = max(float(orc.rel_l2_coef(W64[k], Wl[k]).max()) for k in range(len(Wl)))
    return Wl, ENH_FAMILY_BAR, noise


# ---- the accuracy record: the standing wave, 64 steps to t = 0.8, M = 9, 16 points, gamma = 1e4 ------------------------
# ne: (max |I_h u_h - u|, max |enhanced - u|) over 2001 points, by the prototype
ACCURACY = {8: (1.3202e-2, 7.6642e-3), 16: (3.3456e-3, 1.8828e-3), 32: (8.1231e-4, 4.4161e-4)}


# ---- the host mirror --------------------------------------------------------------------------------------------------------
def advance_host(U_new, U, V, Acc, md, mo, dd, do, loads, phi, dt, beta, gamma, rhs=True, check=True, outs=None,
                 nc=None, R=None):
    """lssvr_wave_advance_host -> (rc, V_out, Acc_out, rhs_out), arrays [nc, ne+1]; what the mode does not write stays
    NaN.  ``outs``: (V_out, Acc_out, rhs_out) to pass instead (aliasing tests); ``nc`` / ``R``: overrides."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    U_new, U, V, Acc, md, mo, dd, do, loads, phi = (_h(t) for t in (U_new, U, V, Acc, md, mo, dd, do, loads, phi))
    if outs is None:
        outs = (np.full(U.shape, np.nan), np.full(U.shape, np.nan), np.full(U.shape, np.nan) if rhs else None)
    rc = lib.lssvr_wave_advance_host(_hp(U_new), _hp(U), _hp(V), _hp(Acc), _hp(md), _hp(mo), _hp(dd), _hp(do),
                                     _hp(loads), _hp(phi), U.shape[1] - 1, U.shape[0] if nc is None else nc,
                                     (1 if loads is None else loads.shape[0]) if R is None else R, dt, beta, gamma,
                                     _hp(outs[0]), _hp(outs[1]), _hp(outs[2]))
    if check:
        _capi.check(rc, "lssvr_wave_advance_host")
    return (rc, *outs)


def advance_host_fn(U_new, U, V, Acc, md, mo, dd, do, L, phi, dt, beta, gamma, rhs=True):
    """proto.advance through the host mirror: the ``adv_fn`` of proto.solve (one case)."""
    row = lambda t: None if t is None else np.asarray(t, dtype=np.float64)[None, :]      # noqa: E731
    _, v, acc, out = advance_host(row(U_new), row(U), row(V), row(Acc), md, mo, dd, do, L if rhs else None,
                                  row(phi) if rhs else None, dt, beta, gamma, rhs=rhs)
    if U_new is None:
        return None, None, out[0]
    return v[0], acc[0], (out[0] if rhs else None)


def advance_numpy(U_new, U, V, Acc, md, mo, dd, do, loads, phi, dt, beta, gamma, rhs=True):
    """The plain numpy restatement, case by case -> (V_out, Acc_out, rhs_out) [nc, ne+1]; NaN where nothing is written."""
    outs = [np.full(U.shape, np.nan) for _ in range(3)]
    for j in range(U.shape[0]):
        r = proto.advance(None if U_new is None else U_new[j], U[j], V[j], Acc[j], md, mo, dd, do, loads,
                          None if phi is None else phi[j], dt, beta, gamma, rhs=rhs)
        for o, t in zip(outs, r):
            if t is not None:
                o[j] = t
    return outs


def kernel_inputs(ne, nc, R, seed=0):
    """Seeded inputs of the kernel: bands of a random positive mesh, weight and damping, nc states, R loads."""
    rng = np.random.default_rng(2900 * seed + ne % 9973 + 17 * nc + 31 * R)
    h = rng.uniform(0.5, 1.5, ne)

    def mass(w):
        md = np.zeros(ne + 1)
        md[:-1] += w * h / 3.0
        md[1:] += w * h / 3.0
        return md, w * h / 6.0
    md, mo = mass(rng.uniform(0.5, 2.0, ne))
    dd, do = mass(rng.uniform(0.0, 1.0, ne))
    shape = (nc, ne + 1)
    return dict(md=md, mo=mo, dd=dd, do=do, U_new=rng.standard_normal(shape), U=rng.standard_normal(shape),
                V=rng.standard_normal(shape), Acc=rng.standard_normal(shape), loads=rng.standard_normal((R, ne + 1)),
                phi=rng.standard_normal((nc, R)))


KERNEL_DT = 0.037


def modes_of(d, damped):
    """The calls of one input set: (label, kwargs of advance_*) for the fused, first-step and state-only modes."""
    dd, do = (d["dd"], d["do"]) if damped else (None, None)
    base = dict(U=d["U"], V=d["V"], Acc=d["Acc"], md=d["md"], mo=d["mo"], dd=dd, do=do, loads=d["loads"], phi=d["phi"])
    return [("fused", dict(base, U_new=d["U_new"], rhs=True)), ("first", dict(base, U_new=None, rhs=True)),
            ("state", dict(base, U_new=d["U_new"], rhs=False))]


# ---- what solve_wave refuses: (name, constructor kwargs, call kwargs, a fragment of the message) -------------------------
def refusals():
    z = lambda x: 0.0 * x      # noqa: E731
    me = "solve_wave "
    stable = "the Newmark rule is unconditionally stable for gamma >= 1/2 and beta >= (gamma + 1/2)^2 / 4 only"
    return [
        ("convection", dict(convection=z), {}, me + tr.STRUCTURAL[0]),
        ("periodic", dict(boundary="periodic", reaction=lambda x: 1.0 + 0.0 * x), {}, me + tr.STRUCTURAL[1]),
        ("fem_solver flux", dict(fem_solver="flux"), {}, me + tr.STRUCTURAL[2]),
        ("fem_solver pivot", dict(fem_solver="pivot"), {}, me + tr.STRUCTURAL[2]),
        ("element_degrees", dict(_degrees=True), {}, me + tr.STRUCTURAL[3]),
        ("solver", dict(solver=1), {}, me + tr.STRUCTURAL[4]),
        ("nonlinear", dict(nonlinear=("poly", [z, z])), {}, "solve_wave has no semilinear form"),
        ("rho <= 0", {}, dict(weight=lambda x: x), tr.RHO_MSG),
        ("shifted reaction < 0", dict(reaction=lambda x: -1e4 + 0.0 * x), {},
         "c + rho / (beta dt^2) + gamma d / (beta dt) < 0 at a quadrature point (dt = 0.1)"),
        ("gamma < 1/2", {}, dict(gamma=0.4), "beta = 0.25, gamma = 0.4: " + stable),
        ("beta < (gamma + 1/2)^2 / 4", {}, dict(beta=0.25, gamma=0.6), "beta = 0.25, gamma = 0.6: " + stable),
        ("beta not finite", {}, dict(beta=math.nan), "beta and gamma must be finite, got nan, 0.5"),
        ("callable Dirichlet data without end_accel0", {}, dict(end_data=(lambda t: math.sin(t), 0.0)),
         "end_accel0 = (g_left''(0), g_right''(0)) is needed when a Dirichlet end has callable end_data"),
        ("end_accel0 of the wrong shape", {}, dict(end_accel0=(0.0, 0.0, 0.0)),
         "end_accel0 must be a pair (g_left''(0), g_right''(0))"),
        ("end_accel0 not finite", {}, dict(end_accel0=(math.inf, 0.0)),
         "end_accel0 is not finite where it is tabulated"),
        ("damping not callable", {}, dict(damping=1.0), "damping must be a callable d(x) or None"),
        ("non-finite damping", {}, dict(damping=lambda x: np.full_like(x, np.nan)),
         "damping is not finite at a quadrature point"),
        ("v0 not callable", {}, dict(_v0=0.0), "v0 must be a callable v0(x)"),
        ("non-finite v0", {}, dict(_v0=lambda x: np.full_like(x, np.inf)), "v0 is not finite where it is tabulated"),
        ("non-finite u0", {}, dict(_u0=lambda x: np.full_like(x, np.inf)), "u0 is not finite where it is tabulated"),
        ("R > 8", {}, dict(forcing=[(1.0, z)] * 9), "forcing must hold 1 .. 8 terms (R <= 8), got 9"),
        ("snapshot 0", {}, dict(snapshots=[0]), "snapshots must be step indices in 1 .. nsteps = 4, got [0]"),
        ("snapshot past the end", {}, dict(snapshots=[2, 5]),
         "snapshots must be step indices in 1 .. nsteps = 4, got [2, 5]"),
        ("nsteps 0", {}, dict(nsteps=0), "nsteps must be an integer >= 1, got 0"),
        ("non-finite forcing", {}, dict(forcing=[(1.0, lambda x: np.full_like(x, np.nan))]),
         "forcing[0] f_x is not finite at a quadrature point"),
        ("forcing of the wrong shape", {}, dict(forcing=[(1.0, lambda x: np.ones(3))]),
         "forcing[0] f_x must return one value per point ([8, 2] at the quadrature points)"),
        ("non-finite phi", {}, dict(forcing=[(lambda t: math.inf, z)]),
         "forcing phi is not finite where it is tabulated"),
        # (a Dirichlet end starts at g(0), so the value is met in u0's table first)
        ("non-finite end data", {}, dict(end_data=(lambda t: math.nan, 0.0), end_accel0=(0.0, 0.0)),
         "u0 is not finite where it is tabulated"),
        ("non-finite weight at a node", {}, dict(weight=lambda x: np.where(x == 1.0, np.nan, 1.0)),
         "weight is not finite at a collocation point"),
    ]


def passing():
    """(constructor kwargs, call kwargs) that the check lets through: c mildly negative, c + rho / (beta dt^2) >= 0 (the
    refusal comes from the missing device), and callable data at a ROBIN end, which needs no end_accel0."""
    return [(dict(reaction=lambda x: -5.0 + 0.0 * x), dict(nsteps=4)),
            (dict(boundary=(("robin", 1.0, 0.0), ("robin", 1.0, 0.0))),
             dict(nsteps=4, end_data=(lambda t: math.sin(t), 0.0)))]


def call_wave(s, u0, v0, **kw):
    return s.solve_wave(u0, v0, 0.4, **kw)
