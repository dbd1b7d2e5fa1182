"""Shared cases and bars of the transient tests: tests/test_transient_cpu.py runs them through
the numpy prototype and the library's host mirrors, tests/test_gpu_transient.py through the device.

The bars.  Every "within rounding" bar is 10x what the float64 prototype (scripts/proto/transient_proto.py, LAPACK's
banded LU) itself reads on the SAME case against a better reference -- the closed form, or the same loop in
np.longdouble --, which allows for a different elimination order and nothing more.  The reading is taken when the test
runs (cached), never from the code under test, with a floor of 4 eps (a result of size 1 rounded a few times); the
figures read when the cases were written are recorded beside them, with the device's own figures next to them."""
import ctypes
import functools
import hashlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import transient_proto as proto         # noqa: E402
from oracle import lssvr_oracle as orc  # noqa: E402,F401

EPS = 2.0 ** -52
FLOOR = 4.0 * EPS
MARGIN = 10.0
DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN


def _zero(x):
    return np.zeros_like(np.asarray(x, dtype=np.float64))


class Case:
    """One transient problem: what proto.solve takes (``kw``), and the facade's constructor and call arguments."""

    def __init__(self, name, nodes, u0, t_end, nsteps, scheme="bdf2", a=None, da=None, c=None, rho=None, forcing=None,
                 kinds=(DIRICHLET, DIRICHLET), kappa=(0.0, 0.0), end_data=(0.0, 0.0), snapshots=None):
        self.name, self.nodes, self.u0, self.t_end, self.nsteps, self.scheme = name, nodes, u0, t_end, nsteps, scheme
        self.a, self.da, self.c, self.rho, self.forcing = a, da, c, rho, forcing
        self.kinds, self.kappa, self.end_data = kinds, kappa, end_data
        self.snapshots = [nsteps] if snapshots is None else snapshots
        self.scale = float(np.max(np.abs(u0(nodes))))

    def run(self, dtype=np.float64, **kw):
        """proto.solve of the case (``bands``: the assembled arrays to run on instead of the oracle's)."""
        return proto.solve(self.nodes, self.u0, self.t_end, self.nsteps, self.scheme, a=self.a, c=self.c, rho=self.rho,
                           forcing=self.forcing, kinds=self.kinds, kappa=self.kappa, end_data=self.end_data,
                           snapshots=self.snapshots, dtype=dtype, **kw)

    def facade(self, M=9, n_colloc=16, gamma=1e4):
        """(constructor kwargs, solve_transient kwargs) of the same problem."""
        bnd = tuple(("dirichlet", 0.0) if k == DIRICHLET else ("robin", kp, 0.0)
                    for k, kp in zip(self.kinds, self.kappa))
        ctor = dict(num_fem_nodes=len(self.nodes), lssvr_M=M, lssvr_gamma=gamma, n_colloc=n_colloc, mesh=self.nodes,
                    global_domain=(float(self.nodes[0]), float(self.nodes[-1])), boundary=bnd,
                    coef=None if self.a is None else (self.a, self.da), reaction=self.c)
        call = dict(nsteps=self.nsteps, scheme=self.scheme, weight=self.rho, end_data=self.end_data,
                    forcing=[(0.0, _zero)] if not self.forcing else self.forcing, snapshots=self.snapshots)
        return ctor, call


# ---- mode decay: a = rho = 1, c = f = 0, zero Dirichlet ends, u0 = sin(k pi (x + 1) / 2) on a uniform mesh ---------------
DECAY_NE = (2, 5, 32, 33)
DECAY_DT, DECAY_STEPS, DECAY_K = 0.01, 40, 1
# max_n |u^n - s_n u0|_inf / |u0|_inf.  (scheme, ne): (prototype, host mirrors in the loop, device loop)
DECAY_READ = {("bdf1", 2): (7.8e-16, 7.8e-16, 7.8e-16), ("bdf1", 5): (3.5e-16, 3.5e-16, 1.3e-15),
              ("bdf1", 32): (1.2e-14, 1.2e-14, 2.1e-15), ("bdf1", 33): (5.9e-15, 5.9e-15, 4.6e-15),
              ("bdf2", 2): (2.3e-15, 2.3e-15, 2.3e-15), ("bdf2", 5): (1.2e-15, 1.2e-15, 1.6e-15),
              ("bdf2", 32): (2.4e-15, 2.4e-15, 1.7e-15), ("bdf2", 33): (6.0e-15, 6.0e-15, 7.6e-15)}


def decay(ne, scheme, k=DECAY_K):
    nodes = np.linspace(-1.0, 1.0, ne + 1)

    def u0(x):
        v = np.sin(k * math.pi * (np.asarray(x, dtype=np.float64) + 1.0) / 2.0)
        return np.where(np.abs(np.asarray(x)) == 1.0, 0.0, v)          # the ends hold the Dirichlet value exactly
    return Case(f"decay-{scheme}-{ne}", nodes, u0, DECAY_DT * DECAY_STEPS, DECAY_STEPS, scheme,
                snapshots=list(range(1, DECAY_STEPS + 1)))


def decay_factors(ne, scheme, k=DECAY_K):
    """s_1 .. s_nsteps of the discrete mode: z = dt (6 / h^2) (1 - cos th) / (2 + cos th), th = k pi / ne."""
    h, th = 2.0 / ne, k * math.pi / ne
    z = DECAY_DT * (6.0 / h ** 2) * (1.0 - math.cos(th)) / (2.0 + math.cos(th))
    s = [1.0, 1.0 / (1.0 + z)]
    for _ in range(2, DECAY_STEPS + 1):
        s.append(s[-1] / (1.0 + z) if scheme == "bdf1" else (2.0 * s[-1] - 0.5 * s[-2]) / (1.5 + z))
    return np.array(s[1:])


def decay_error(case, ne, nodal):
    """max_n |u^n - s_n u0|_inf / |u0|_inf."""
    s = decay_factors(ne, case.scheme)
    return float(np.max(np.abs(np.asarray(nodal) - s[:, None] * case.u0(case.nodes)[None, :]))) / case.scale


@functools.lru_cache(maxsize=None)
def decay_bar(ne, scheme):
    case = decay(ne, scheme)
    return max(MARGIN * decay_error(case, ne, case.run()["nodal"]), FLOOR)


# ---- a general problem: non-uniform 33-node mesh, variable a, c, rho, Robin left, moving Dirichlet right, R = 2 ----------
def general(nsteps=64, snapshots=(32, 64)):
    w = np.random.default_rng(26).uniform(0.5, 1.5, 32)
    nodes = -1.0 + 2.0 * np.concatenate([[0.0], np.cumsum(w)]) / np.sum(w)
    nodes[-1] = 1.0
    return Case("general-33", nodes, lambda x: np.cos(x), 0.64, nsteps, "bdf2",
                a=lambda x: 1.0 + 0.5 * np.sin(2.0 * x), da=lambda x: np.cos(2.0 * x),
                c=lambda x: 0.5 + 0.3 * np.cos(3.0 * x), rho=lambda x: 1.0 + 0.4 * x * x,
                forcing=[(lambda t: math.exp(-t), lambda x: np.sin(math.pi * x)),
                         (lambda t: math.cos(2.0 * t), lambda x: x * x)],
                kinds=(ROBIN, DIRICHLET), kappa=(2.0, 0.0),
                end_data=(lambda t: 0.3 * math.cos(t), lambda t: math.cos(1.0) + 0.2 * math.sin(3.0 * t)),
                snapshots=list(snapshots))


# ---- conservation: two Neumann ends, c = f = g = 0, non-uniform mesh, variable rho --------------------------------------
def neumann(nsteps=50):
    w = np.random.default_rng(7).uniform(0.5, 1.5, 24)
    nodes = -1.0 + 2.0 * np.concatenate([[0.0], np.cumsum(w)]) / np.sum(w)
    nodes[-1] = 1.0
    return Case("neumann-25", nodes, lambda x: np.exp(-4.0 * (x - 0.2) ** 2), 0.5, nsteps, "bdf2",
                rho=lambda x: 1.0 + 0.5 * np.sin(3.0 * x), kinds=(ROBIN, ROBIN),
                snapshots=list(range(1, nsteps + 1)))


def total_mass(case, nodal):
    """sum_i (M u)_i of every row of ``nodal``, by math.fsum (exactly rounded: the check adds no noise of its own)."""
    md, mo = proto.mass_bands(case.nodes, case.rho)
    return np.array([math.fsum(proto.tri_apply(md, mo, np.asarray(u, dtype=np.float64)).tolist()) for u in nodal])


def mass_drift(case, nodal):
    """max_n |mass(u^n) - mass(u^0)| / mass(|u^0|)."""
    u_init = case.u0(case.nodes)
    m0 = total_mass(case, [u_init])[0]
    return float(np.max(np.abs(total_mass(case, nodal) - m0))) / total_mass(case, [np.abs(u_init)])[0]


# ---- the bars of the loop tests -----------------------------------------------------------------------------------------------
# Both prototype loops (float64 and np.longdouble) run on the float64 mass bands, step matrices and loads that the code
# under test assembled (``bands``; None: the oracle's), so that the comparison sees the time loop alone.  The oracle's
# assembly rounds the same bands differently in the last bit; that fixed perturbation enters every step again, and the
# low modes are barely damped (0.976 per step on the decay case), so it grows linearly with the step count: against
# the oracle's bands the device read 1.40e-14 on decay-bdf2-33, where the float64 prototype on its own bands reads
# 1.25e-15.
# max over the snapshots of |u - u_longdouble|_inf / |u0|_inf on the device's bands.  name: (prototype float64, device,
# device against the loop on the oracle's bands -- recorded, no bar)
LOOP_READ = {"general-33": (1.3e-15, 2.4e-15, 6.4e-15), "neumann-25": (1.4e-15, 1.8e-15, 4.0e-15),
             "decay-bdf2-33": (1.5e-15, 3.0e-15, 1.4e-14)}
# max_n |mass drift|.  (prototype float64, host mirrors, device)
MASS_READ = (2.6e-15, 2.6e-15, 2.8e-15)


# What the device assembled is shared only after it has been checked, array by array, against the oracle's assembly
# of the same problem (proto.mass_bands, proto.step_bands, proto.loads): a facade that dropped a, took a wrong
# c + alpha rho / dt or ordered the loads differently from phi fails here.  The bar is 32 eps of the entry's scale.
# Each entry is a sum of at most six terms (two elements; stiffness, mass), each term at most eight rounded operations
# deep (weight products, the two-point quadrature sum, h, the scatter), so either assembly is within 12 eps of the sum
# of its terms' sizes, and the two within 24; 32 is the next power of two.  The scale of a matrix entry is the larger
# neighbouring diagonal entry (every term of off[i] also sits in diag[i] and diag[i+1]; a relative bar on off itself
# would fail where stiffness and mass cancel), that of a load entry max |load| of its row (f changes sign).
BANDS_BAR = 32.0 * EPS
# max scaled difference, device against oracle, over all arrays.  name: device
BANDS_READ = {"general-33": 2.2e-16, "neumann-25": 2.2e-16, "decay-bdf2-33": 1.9e-16, "decay-bdf1-5": 5.6e-17}


def bands_error(case, bands):
    """max over (mass, every step matrix, loads) of |device - oracle| / scale, and the set of alphas."""
    dt = case.t_end / case.nsteps
    worst = 0.0

    def matrix(got, want):
        (gd, go), (wd, wo) = got, want
        assert gd.shape == wd.shape and go.shape == wo.shape
        sc = np.abs(wd)
        return max(float(np.max(np.abs(gd - wd) / sc)), float(np.max(np.abs(go - wo) / np.maximum(sc[:-1], sc[1:]))))

    worst = max(worst, matrix(bands["mass"], proto.mass_bands(case.nodes, case.rho)))
    alphas = {proto.SCHEMES["bdf1"][0], proto.SCHEMES[case.scheme][0]}
    assert set(bands["step"]) == alphas
    for al in alphas:
        worst = max(worst, matrix(bands["step"][al], proto.step_bands(case.nodes, al, dt, case.a, case.c, case.rho)))
    want = proto.loads(case.nodes, [f for _, f in case.forcing] if case.forcing else [_zero])
    assert bands["loads"].shape == want.shape
    for got_r, want_r in zip(bands["loads"], want):
        sc = float(np.max(np.abs(want_r)))
        worst = max(worst, float(np.max(np.abs(got_r - want_r))) / sc if sc > 0.0 else float(np.max(np.abs(got_r))))
    return worst


_REFERENCES = {}


def _band_bytes(v):
    """The bytes of every array in ``v`` (arrays, tuples and dicts of them, None), dict entries in key order."""
    if isinstance(v, dict):
        v = [v[k] for k in sorted(v)]
    if isinstance(v, (tuple, list)):
        return b"".join(_band_bytes(t) for t in v)
    return b"" if v is None else np.ascontiguousarray(v).tobytes()


def references(cases, name, bands=None):
    """(case, np.longdouble loop, float64 loop) of ``cases[name]``, computed once per (cases, name, bands): the one
    cache of the transient, semilinear transient and wave rules."""
    key = (id(cases), name, None if bands is None else hashlib.sha1(_band_bytes(bands)).hexdigest())
    if key not in _REFERENCES:
        case = cases[name]()
        _REFERENCES[key] = (case, case.run(np.longdouble, bands=bands), case.run(bands=bands))
    return _REFERENCES[key]


def _references(name, bands=None):
    return references(CASES, name, bands)


def loop_reading(name, nodal, bands=None):
    """(error of ``nodal``, bar, the float64 prototype's own error): max |. - the np.longdouble prototype|_inf /
    |u0|_inf over the case's snapshots; the bar is 10x the prototype's."""
    case, ref, p64 = _references(name, bands)
    err, read = (float(np.max(np.abs(np.asarray(v, dtype=np.longdouble) - ref["nodal"]))) / case.scale
                 for v in (nodal, p64["nodal"]))
    return err, max(MARGIN * read, FLOOR), read


def mass_bar():
    case = CASES["neumann-25"]()
    return max(MARGIN * mass_drift(case, case.run()["nodal"]), FLOOR)


CASES = {"general-33": general, "neumann-25": neumann, "decay-bdf2-33": lambda: decay(33, "bdf2")}


# ---- the host mirrors ---------------------------------------------------------------------------------------------------------
def _hp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _h(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def rhs_host(md, mo, U0, U1, loads, phi, beta0, beta1, inv_dt, check=True):
    """lssvr_ts_rhs_host -> (rc, out [nc, ne+1]); U0 [nc, ne+1], loads [R, ne+1], phi [nc, R]."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    md, mo, U0, loads, phi = (_h(t) for t in (md, mo, U0, loads, phi))
    U1 = None if U1 is None else _h(U1)
    out = np.full(U0.shape, np.nan)
    rc = lib.lssvr_ts_rhs_host(_hp(md), _hp(mo), _hp(U0), None if U1 is None else _hp(U1), _hp(loads), _hp(phi),
                               len(mo), U0.shape[0], loads.shape[0], beta0, beta1, inv_dt, _hp(out))
    if check:
        _capi.check(rc, "lssvr_ts_rhs_host")
    return rc, out


def step_rhs_host(md, mo, u0, u1, beta0, beta1, inv_dt, L, phi):
    """proto.step_rhs through the host mirror: the ``rhs_fn`` of proto.solve."""
    return rhs_host(md, mo, u0[None, :], None if u1 is None else u1[None, :], L, np.asarray(phi)[None, :], beta0,
                    beta1, inv_dt)[1][0]


def source_host(U2, U0, U1, ftab, rho_tab, phi, alpha, beta0, beta1, inv_dt, pm, check=True):
    """lssvr_ts_source_table_host -> (rc, out); ftab [R, ne, n] / [R, n, ne] with ``pm``."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    U2, U0, ftab, rho_tab, phi = (_h(t) for t in (U2, U0, ftab, rho_tab, phi))
    U1 = None if U1 is None else _h(U1)
    ne = len(U2) - 1
    n = rho_tab.shape[0] if pm else rho_tab.shape[1]
    out = np.full(rho_tab.shape, np.nan)
    rc = lib.lssvr_ts_source_table_host(_hp(U2), _hp(U0), None if U1 is None else _hp(U1), _hp(ftab), _hp(rho_tab),
                                        _hp(phi), ne, n, ftab.shape[0], int(pm), alpha, beta0, beta1, inv_dt, _hp(out))
    if check:
        _capi.check(rc, "lssvr_ts_source_table_host")
    return rc, out


# ---- the plain numpy restatement of the two kernels (every sum in the documented order) -------------------------------------
def rhs_numpy(md, mo, U0, U1, loads, phi, beta0, beta1, inv_dt):
    out = np.empty_like(U0)
    for j in range(U0.shape[0]):
        out[j] = proto.step_rhs(md, mo, U0[j], None if U1 is None else U1[j], beta0, beta1, inv_dt, loads, phi[j])
    return out


def source_numpy(U2, U0, U1, ftab, rho_tab, phi, alpha, beta0, beta1, inv_dt, pm):
    """Element-major arithmetic on [ne, n] views; the result in the layout of the inputs."""
    F = np.transpose(ftab, (0, 2, 1)) if pm else ftab
    rho = rho_tab.T if pm else rho_tab
    n = rho.shape[1]
    d = alpha * U2 - beta0 * U0
    w = inv_dt * (d if beta1 == 0.0 else d - beta1 * U1)
    f = phi[0] * F[0]
    for r in range(1, F.shape[0]):
        f = f + phi[r] * F[r]
    t = np.arange(n, dtype=np.float64) / float(n - 1)
    out = f - rho * (w[:-1, None] + (w[1:] - w[:-1])[:, None] * t[None, :])
    return np.ascontiguousarray(out.T) if pm else out


def kernel_inputs(ne, nc, R, n, seed=0):
    """Seeded inputs of both kernels: bands of a random positive mesh and weight, nc vector pairs, R loads and tables."""
    rng = np.random.default_rng(1000 * seed + ne % 9973 + 17 * nc + 31 * R + n)
    nodes = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 1.5, ne))])
    h = np.diff(nodes)
    rho = rng.uniform(0.5, 2.0, ne)
    md = np.zeros(ne + 1)
    md[:-1] += rho * h / 3.0
    md[1:] += rho * h / 3.0
    mo = rho * h / 6.0
    return dict(md=md, mo=mo, U0=rng.standard_normal((nc, ne + 1)), U1=rng.standard_normal((nc, ne + 1)),
                U2=rng.standard_normal(ne + 1), loads=rng.standard_normal((R, ne + 1)),
                phi=rng.standard_normal((nc, R)), ftab=rng.standard_normal((R, ne, n)),
                rho_tab=rng.uniform(0.5, 2.0, (ne, n)))


# ---- the enhanced snapshots ---------------------------------------------------------------------------------------------------
ENH_FAMILY_BAR = 1e-11          # the reaction-row tests' bar against the float64 restatement, M <= 22
# max rel-L2 of W.  (M, n_colloc): (the prototype's own float64 noise, device against the prototype)
ENH_READ = {(9, 16): (2.4e-15, 5.5e-15), (20, 24): (8.2e-15, 7.1e-15)}


def enhanced_rows(name, M, n_colloc, gamma=1e4, dtype=np.float64, bands=None):
    """W [ns, ne, M] of the case's snapshots: the oracle's rows on the prototype's u and w computed in ``dtype``."""
    case, ref, p64 = _references(name, bands)
    r = p64 if dtype == np.float64 else ref
    fl = [f for _, f in case.forcing] if case.forcing else [_zero]
    return np.stack([proto.enhance_snapshot(case.nodes, np.asarray(r["nodal"][k], dtype=np.float64),
                                            np.asarray(r["diffs"][k], dtype=np.float64),
                                            r["phi"][k] if case.forcing else [0.0], fl, M, gamma, n_colloc, a=case.a,
                                            da=case.da, c=case.c, rho=case.rho, kinds=case.kinds, g=r["g"][k])
                     for k in range(len(case.snapshots))])


def enhanced_reference(name, M, n_colloc, bands=None):
    """(W of the np.longdouble loop's data, bar, noise): the bar is the larger of the family's and 10x the noise that the
    float64 loop's own rounding -- amplified by 1 / dt in w -- puts into W."""
    Wl = enhanced_rows(name, M, n_colloc, dtype=np.longdouble, bands=bands)
    W64 = enhanced_rows(name, M, n_colloc, bands=bands)
    noise = max(float(orc.rel_l2_coef(W64[k], Wl[k]).max()) for k in range(len(Wl)))
    return Wl, max(ENH_FAMILY_BAR, MARGIN * noise), noise


# ---- the accuracy record: u = exp(-t) cos(pi x / 2), 64 BDF2 steps to t = 1, M = 9, 16 points, gamma = 1e4 ----------
# ne: (max |I_h u_h - u|, max |enhanced - u|) over 2001 points, by the prototype; the device agrees to 3 digits
ACCURACY = {8: (9.298e-3, 2.457e-3), 16: (2.375e-3, 6.184e-4), 32: (5.970e-4, 1.548e-4)}
ACCURACY_STEPS, ACCURACY_T, ACCURACY_POINTS = 64, 1.0, 2001


# ---- what solve_transient refuses: (name, constructor kwargs, call kwargs, a fragment of the message) ----------------------
STRUCTURAL = ("has no convection term", "has no boundary='periodic'", "needs fem_solver='bands'",
              "has no element_degrees", "needs solver=ops.SOLVER_PRIMAL")
RHO_MSG = "weight must be positive at every quadrature point (rho > 0)"


def refusals():
    u0 = lambda x: 0.0 * x      # noqa: E731
    base = dict(nsteps=4)
    me = "solve_transient "
    return [
        ("convection", dict(convection=lambda x: 0.0 * x), base, me + STRUCTURAL[0]),
        ("periodic", dict(boundary="periodic", reaction=lambda x: 1.0 + 0.0 * x), base, me + STRUCTURAL[1]),
        ("fem_solver flux", dict(fem_solver="flux"), base, me + STRUCTURAL[2]),
        ("fem_solver pivot", dict(fem_solver="pivot"), base, me + STRUCTURAL[2]),
        ("element_degrees", dict(_degrees=True), base, me + STRUCTURAL[3]),
        ("solver", dict(solver=1), base, me + STRUCTURAL[4]),
        ("rho <= 0", {}, dict(nsteps=4, weight=lambda x: x), RHO_MSG),
        ("c + rho/dt < 0", dict(reaction=lambda x: -100.0 + 0.0 * x), dict(nsteps=4),
         "c + rho / dt < 0 at a quadrature point (dt = 0.1)"),
        ("R > 8", {}, dict(nsteps=4, forcing=[(1.0, u0)] * 9), "forcing must hold 1 .. 8 terms (R <= 8), got 9"),
        ("snapshot 0", {}, dict(nsteps=4, snapshots=[0]), "snapshots must be step indices in 1 .. nsteps = 4, got [0]"),
        ("snapshot past the end", {}, dict(nsteps=4, snapshots=[2, 5]),
         "snapshots must be step indices in 1 .. nsteps = 4, got [2, 5]"),
        ("non-finite forcing", {}, dict(nsteps=4, forcing=[(1.0, lambda x: np.full_like(x, np.nan))]),
         "forcing[0] f_x is not finite at a quadrature point"),
        ("non-finite forcing at a node (a collocation point, no quadrature point)", {},
         dict(nsteps=4, forcing=[(1.0, lambda x: np.where(x == -1.0, np.inf, 1.0))]),
         "forcing[0] f_x is not finite at a collocation point"),
        ("non-finite weight at a node", {}, dict(nsteps=4, weight=lambda x: np.where(x == 1.0, np.nan, 1.0)),
         "weight is not finite at a collocation point"),
        ("forcing of the wrong shape", {}, dict(nsteps=4, forcing=[(1.0, lambda x: np.ones(3))]),
         "forcing[0] f_x must return one value per point ([8, 2] at the quadrature points)"),
        ("non-finite phi", {}, dict(nsteps=4, forcing=[(lambda t: math.inf, u0)]),
         "forcing phi is not finite where it is tabulated"),
        # (a Dirichlet end starts at g(0), so the value is met in u0's table first)
        ("non-finite end data", {}, dict(nsteps=4, end_data=(lambda t: math.nan, 0.0)),
         "u0 is not finite where it is tabulated"),
        ("non-finite u0", {}, dict(nsteps=4, _u0=lambda x: np.full_like(x, np.inf)),
         "u0 is not finite where it is tabulated"),
        ("scheme", {}, dict(nsteps=4, scheme="bdf3"), "scheme must be 'bdf1' or 'bdf2', got 'bdf3'"),
    ]


def passing():
    """(constructor kwargs, call kwargs) that the check lets through.  c mildly negative is allowed: c + rho / dt >= 0
    (the refusal comes later, from the missing device)."""
    return [(dict(reaction=lambda x: -5.0 + 0.0 * x), dict(nsteps=4))]


def call_transient(s, u0, v0, **kw):
    return s.solve_transient(u0, 0.4, **kw)


def check_refusals(monkeypatch, call, refusals, passing):
    """Every row of ``refusals`` is a ValueError with the row's fragment in its message, raised on the host: the library
    loader and the device lookup are replaced by functions that fail the test, so no entry is bound and no kernel can
    be launched.  Every row of ``passing`` gets as far as the device.  ``call(solver, u0, v0, **call kwargs)`` runs the
    method under test; ``_degrees`` / ``_u0`` / ``_v0`` in a row's kwargs set element_degrees and replace the zero
    start, and lssvr_M = 9, n_colloc = 16, nsteps = 4 where a refusal row does not say."""
    import re
    import pytest
    import hybrid_fem_lssvr_amd as pkg
    from hybrid_fem_lssvr_amd import _capi, solver

    def forbidden(*a, **k):
        raise AssertionError("a device call was reached before the refusal")
    monkeypatch.setattr(_capi, "load", forbidden)
    monkeypatch.setattr(solver, "_device", forbidden)
    z = lambda x: 0.0 * x      # noqa: E731
    for name, ctor, kw, match in refusals:
        ctor, kw = dict(ctor), dict(kw)
        degrees = ctor.pop("_degrees", False)
        u0, v0 = kw.pop("_u0", z), kw.pop("_v0", z)
        ctor.setdefault("lssvr_M", 9)
        ctor.setdefault("n_colloc", 16)
        kw.setdefault("nsteps", 4)
        s = pkg.FEMLSSVRPrimalSolver(9, **ctor)
        if degrees:
            s.element_degrees = np.full(8, 9)
        with pytest.raises(ValueError, match=re.escape(match)):
            call(s, u0, v0, **kw)
            raise AssertionError(f"{name}: not refused")
    for ctor, kw in passing:
        with pytest.raises(AssertionError, match="device call"):
            call(pkg.FEMLSSVRPrimalSolver(9, **ctor), z, z, **kw)
