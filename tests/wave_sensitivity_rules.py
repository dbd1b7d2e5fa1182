"""Shared cases, restatement and bars of the wave sensitivity tests:
tests/test_wave_sensitivity_cpu.py runs them through the numpy prototype and the library's host mirrors,
tests/test_gpu_wave_sensitivity.py through the device.

The restatement is scripts/proto/wave_sensitivity_proto.py: the dense Newmark loop, the complex-step derivative of every
datum (the yardstick: no subtraction, so it carries the rounding of one loop and nothing else), the backward sweep in
the order of csrc/lssvr_newmark_adj.hpp and the sums over time in that of csrc/lssvr_chunk_sens.hpp.  The bar of a
case is 10x what the float64 prototype itself reads on the SAME case -- the deviation of its adjoint gradients from the
complex step, the largest over the groups (a, c, rho, d, f tables, u0, v0, g, kappa, accel0), each relative to the
largest entry of its group.  The reading is taken when the test runs (cached), never from the code under test; READ
records what it was when the cases were written."""
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import wave_sensitivity_proto as proto         # noqa: E402

sp = proto.sp
MARGIN = 10.0
DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN
D, R = DIRICHLET, ROBIN
END_COMBOS = sp.END_COMBOS
TABLES = proto.TABLES
NEWMARK = proto.NEWMARK
# the largest reading of the prototype over the cases of each mesh, when they were written; the prototype must stay
# within 4x of it (another LAPACK build may round otherwise, a broken restatement reads 1e-3 and more)
READ = {1: 2.0e-14, 2: 6.0e-15, 7: 4.3e-13, 33: 1.2e-12}
READ_SLACK = 4.0


class Case:
    """One loop: ``ne`` non-uniform elements, ``nq`` points, the end kinds, ``N`` steps, damped or not, the index of
    the (beta, gamma) pair and the functional ("random": any nodal p_n, some levels zero, p_0 != 0; "goal": the
    terminal int (1 + x^2) u; "observe": the misfit at 9 points and three steps, the start among them)."""

    def __init__(self, ne, nq, kinds, N, damped, nm, functional="random"):
        self.ne, self.nq, self.kinds, self.N, self.damped, self.nm, self.kind = (ne, nq, tuple(kinds), N, bool(damped),
                                                                                 nm, functional)
        self.p = proto.problem(ne, nq, kinds, N, damped, NEWMARK[nm])
        self.J = proto.functional(self.p, functional)

    @property
    def id(self):
        return (f"ne{self.ne}-q{self.nq}-{''.join('DR'[k] for k in self.kinds)}-N{self.N}-{'d' if self.damped else 'u'}"
                f"-nm{self.nm}-{self.kind}")

    @functools.cached_property
    def reference(self):
        """(per-group readings, adjoint dict, complex-step dict) of the prototype."""
        return proto.reading((self.p, self.J))

    @property
    def read(self):
        return max(self.reference[0].values())

    @property
    def bar(self):
        return MARGIN * self.read

    def deviation(self, grads):
        """The largest group deviation of ``grads`` from the complex step."""
        return max(proto.deviations(grads, self.reference[2]).values())


@functools.lru_cache(maxsize=None)
def case(*key):
    return Case(*key)


CONTROL = (7, 2, (D, R), 3, True, 1, "random")


def cpu_cases():
    """7 elements: the four end combinations with N = 3, 8, 9, 17 (remainder chunks of 3, 0, 1, 1); 33 elements: with
    N = 9, 17; one and two elements with N = 3.  nquad 1, 2, 5, damping, the two (beta, gamma) pairs and the three
    functionals rotate so that every pairing with an end combination occurs."""
    out = []
    for ne, Ns in ((7, (3, 8, 9, 17)), (33, (9, 17))):
        for ki, kinds in enumerate(END_COMBOS):
            for j, N in enumerate(Ns):
                r = ki + j + (ne == 33)
                nq = (1, 2, 5)[r % 3]
                if nq == 1 and kinds == (R, R):          # one point makes M_rho singular when no end is held: no acc^0
                    nq = 3
                out.append(case(ne, nq, kinds, N, (r // 2) % 2 == 0, (ki + j // 2 + (ne == 33)) % 2,
                                ("random", "goal", "observe")[(ki + 2 * j) % 3]))
    for ki, kinds in enumerate(END_COMBOS):
        out.append(case(1, 1 + ki, kinds, 3, ki % 2 == 0, ki // 2, ("random", "goal", "observe")[ki % 3]))
        out.append(case(2, 2 + ki % 2, kinds, 3, ki % 2 == 1, 1 - ki // 2, ("observe", "random", "goal")[ki % 3]))
    out.append(case(*CONTROL))
    return list(dict.fromkeys(out))


def facade_cases():
    """33 elements, nquad 2: the four end combinations x (goal, observe) x damped or not; N = 9 and 17 and the two
    (beta, gamma) pairs alternate."""
    out = []
    for ki, kinds in enumerate(END_COMBOS):
        for fi, fn in enumerate(("goal", "observe")):
            for di in range(2):
                out.append(case(33, 2, kinds, (9, 17)[(ki + fi + di) % 2], bool(di), (ki + fi) % 2, fn))
    return out


def facade_solver(c, **kw):
    """The facade configured for the case ``c``."""
    import hybrid_fem_lssvr_amd as pkg
    ends = [("robin", float(c.p.kappa[s]), 0.0) if c.kinds[s] == ROBIN else ("dirichlet", 0.0) for s in range(2)]
    return pkg.FEMLSSVRPrimalSolver(mesh=c.p.x, nquad=c.nq, coef=(sp.coef_a, sp.coef_da), reaction=sp.reaction,
                                    boundary=tuple(ends), lssvr_M=9, n_colloc=16, **kw)


def facade_args(c):
    """The keywords of solve_wave / solve_wave_sensitivity for the loop of ``c`` (without the functional)."""
    return dict(nsteps=c.N, weight=proto.weight, damping=proto.damping if c.damped else None,
                forcing=[(f, fx) for f, fx in proto.FORCING], end_data=(proto.g_left, proto.g_right),
                end_accel0=proto.ACCEL0, beta=c.p.beta, gamma=c.p.gamma)


def facade_functional(c):
    if c.kind == "goal":
        return dict(goal=sp.goal_density)
    steps, xo, d = proto.observations(c.N)
    return dict(observe=(steps, xo, d))


def facade_gradients(s):
    """The gradient dict (the groups of proto.deviations) of a WaveSensitivity ``s``."""
    return dict(a=s.d_coef, c=s.d_reaction, rho=s.d_weight, d=s.d_damping, f=s.d_forcing, u0=s.d_u0, v0=s.d_v0,
                g=s.d_end_values, kappa=s.d_kappa, accel0=s.d_end_accel0)


# ---- the kernels' inputs and the host mirrors ----------------------------------------------------------------------------
CANARY = -7.25e77


def _hp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _c(t):
    return None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.float64))


MODES = ("first", "middle", "last")


def advance_inputs(ne, seed=0):
    """Random inputs of size 1 for one adjoint advance: lam, Vbar, Abar, P [ne+1], the bands, dt."""
    rng = np.random.default_rng(77 * ne + seed)
    n1 = ne + 1
    d = {k: rng.standard_normal(n1) for k in ("lam", "Vbar", "Abar", "P", "mdiag", "ddiag")}
    d.update(moff=rng.standard_normal(ne), doff=rng.standard_normal(ne), dt=0.05 + 0.1 * rng.random(), ne=ne)
    return d


def advance_keys(mode):
    return {"first": ("b",), "middle": ("v", "a", "b"), "last": ("v", "a", "u")}[mode]


def advance_numpy(d, mode, damped, nm, with_p=True):
    """{key: vector} of the numpy restatement for the mode."""
    beta, gamma = NEWMARK[nm]
    P = d["P"] if with_p else None
    if mode == "first":
        return dict(b=proto.adjoint_seed(P, d["Vbar"], d["Abar"], d["dt"], beta, gamma))
    dd, do = (d["ddiag"], d["doff"]) if damped else (None, None)
    u, v, a, b = proto.adjoint_advance(d["lam"], d["Vbar"], d["Abar"], d["mdiag"], d["moff"], dd, do, P, d["dt"], beta,
                                       gamma)
    full = dict(u=u, v=v, a=a, b=b)
    return {k: full[k] for k in advance_keys(mode)}


def advance_host(d, mode, damped, nm, with_p=True):
    """lssvr_newmark_adjoint_advance_host -> {key: vector} for every key, canaries where the mode does not write."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    beta, gamma = NEWMARK[nm]
    out = {k: np.full(d["ne"] + 1, CANARY) for k in ("v", "a", "u", "b")}
    keys = advance_keys(mode)
    first = mode == "first"
    keep = {k: _c(d[k]) for k in ("lam", "Vbar", "Abar", "P", "mdiag", "moff", "ddiag", "doff")}
    g = lambda k, on=True: _hp(keep[k]) if on else None          # noqa: E731
    rc = lib.lssvr_newmark_adjoint_advance_host(g("lam", not first), g("Vbar"), g("Abar"), g("P", with_p),
                                                g("mdiag", not first), g("moff", not first),
                                                g("ddiag", damped and not first), g("doff", damped and not first),
                                                d["ne"], d["dt"], beta, gamma,
                                                *(_hp(out[k]) if k in keys else None for k in ("v", "a", "u", "b")))
    _capi.check(rc, "lssvr_newmark_adjoint_advance_host")
    return out


def check_advance(got, ref):
    for k in ("v", "a", "u", "b"):
        if k in ref:
            assert np.array_equal(got[k], ref[k]), k
        else:
            assert np.all(got[k] == CANARY), f"{k} was written though the mode does not write it"


def kernel_inputs(ne, m, nR, n0=0, seed=0):
    """Random inputs of size 1 for one chunk: x [ne+1] non-uniform, Utraj, Vtraj, Atraj [N+1, ne+1] with N = n0+m (one
    row past the chunk), Z and Brows [m, ne+1], phi [N+1, max(R, 1)], band_ends [2]."""
    rng = np.random.default_rng(1000 * ne + 10 * m + nR + seed)
    N = n0 + m
    x = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(ne))]) / ne - 0.3
    tr = lambda: rng.standard_normal((N + 1, ne + 1))          # noqa: E731
    return dict(x=x, Utraj=tr(), Vtraj=tr(), Atraj=tr(), Z=rng.standard_normal((m, ne + 1)),
                Brows=rng.standard_normal((m, ne + 1)), phi=rng.standard_normal((N + 1, max(nR, 1))),
                band_ends=rng.standard_normal(2), n0=n0, R=nR, m=m, ne=ne)


def initial(d, nq, seed=1):
    """Random contents for the outputs of an accumulating call: the tables and kappa."""
    rng = np.random.default_rng(seed + d["ne"])
    out = {k: rng.standard_normal((d["ne"], nq)) for k in TABLES[:4]}
    out["f"] = rng.standard_normal((d["R"], d["ne"], nq))
    out["kappa"] = rng.standard_normal(2)
    return out


def blank(d, nq, init=None):
    """The output dict of a call, N+1 rows of g: canaries, or copies of ``init`` (an accumulating call)."""
    N = d["Utraj"].shape[0] - 1
    out = {k: np.full((d["ne"], nq), CANARY) for k in TABLES[:4]}
    out["f"] = np.full((max(d["R"], 1), d["ne"], nq), CANARY)[:d["R"]]
    out["g"], out["kappa"] = np.full((N + 1, 2), CANARY), np.full(2, CANARY)
    if init is not None:
        for k, v in init.items():
            out[k] = np.array(v, dtype=np.float64)
    return out


def sens_host(d, nq, want=TABLES, kinds=(D, D), ends=False, init=None, check=True):
    """lssvr_newmark_sensitivity_host on the inputs ``d`` -> (rc, dict): every table of TABLES, canary-filled where it
    is not in ``want`` (and then not handed over, nor the trajectory only it reads), and "g", "kappa" likewise with
    ``ends``.  ``init``: the sums continue from it (accumulate = 1)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    out = blank(d, nq, init)
    x, U, V, A, Z, B, phi, be = (_c(d[k]) for k in ("x", "Utraj", "Vtraj", "Atraj", "Z", "Brows", "phi", "band_ends"))
    rc = lib.lssvr_newmark_sensitivity_host(_hp(x), d["ne"], int(nq), _hp(U), _hp(V) if "d" in want else None,
                                            _hp(A) if "rho" in want else None, _hp(Z), d["n0"], d["m"],
                                            _hp(phi) if "f" in want else None, d["R"],
                                            *(_hp(out[k]) if k in want else None for k in TABLES),
                                            int(init is not None), _hp(B) if ends else None, _hp(be) if ends else None,
                                            int(kinds[0]), int(kinds[1]), _hp(out["g"]) if ends else None,
                                            _hp(out["kappa"]) if ends else None)
    if check:
        _capi.check(rc, "lssvr_newmark_sensitivity_host")
    return rc, out


def sens_numpy(d, nq, kinds=(D, D), init=None):
    """The same dict from the numpy restatement, in the order of csrc/lssvr_chunk_sens.hpp."""
    names = TABLES if d["R"] else TABLES[:4]
    out = proto.chunk_tables(d["x"], nq, d["Utraj"], d["Vtraj"], d["Atraj"], d["Z"], d["n0"], d["phi"], d["R"], names,
                             init)
    out["g"] = np.full((d["Utraj"].shape[0], 2), CANARY)
    out["kappa"] = proto.chunk_ends(d["Utraj"], d["Z"], d["Brows"], d["n0"], d["band_ends"], kinds, out["g"],
                                    None if init is None else init["kappa"])
    return out


def wants(nR):
    """Every subset of the five tables ("f" only with R > 0); the empty one goes with the end gradients alone."""
    names = TABLES if nR else TABLES[:4]
    return [tuple(k for i, k in enumerate(names) if bits >> i & 1) for bits in range(1 << len(names))]


def check_against(got, want_tables, ref, ends, init=None):
    """``got`` equals ``ref`` bit for bit in every table of ``want_tables`` (and in g, kappa with ``ends``) and holds
    what it was prefilled with -- canaries, or ``init`` -- everywhere else."""
    for k in TABLES:
        if k in want_tables:
            assert np.array_equal(got[k], ref[k]), k
        else:
            assert np.array_equal(got[k], np.full(got[k].shape, CANARY) if init is None else init[k]), \
                f"{k} was written though it was not asked for"
    if ends:
        assert np.array_equal(got["g"], ref["g"]) and np.array_equal(got["kappa"], ref["kappa"])
    else:
        assert np.all(got["g"] == CANARY)
        assert np.array_equal(got["kappa"], np.full(2, CANARY) if init is None else init["kappa"])


def host_sweep(p, U, V, A, lam, B, ub, vb, size):
    """proto.sweep_gradients through the library's host mirror, in chunks of ``size`` levels."""
    def tables(x, nq, Utraj, Vtraj, Atraj, Z, n0, phi, nR, want, init):
        d = dict(x=x, Utraj=Utraj, Vtraj=Vtraj, Atraj=Atraj, Z=Z, Brows=Z, phi=phi, band_ends=np.zeros(2), n0=n0, R=nR,
                 m=len(Z), ne=len(x) - 1)
        full = None
        if init is not None:
            full = {k: init.get(k, np.zeros((d["ne"], nq))) for k in TABLES[:4]}
            full.update(f=init["f"], kappa=np.zeros(2))
        got = sens_host(d, nq, want, init=full)[1]
        return {k: got[k] for k in want}

    def ends(Utraj, Z, Brows, n0, be, kinds, out_g, kap):
        from hybrid_fem_lssvr_amd import _capi
        lib = _capi.load()
        kout = np.full(2, CANARY) if kap is None else np.array(kap)          # (the tables all NULL: the ends alone)
        rc = lib.lssvr_newmark_sensitivity_host(_hp(_c(p.x)), len(p.x) - 1, p.nq, _hp(_c(Utraj)), None, None,
                                                _hp(_c(Z)), n0, len(Z), None, 0, None, None, None, None, None,
                                                int(kap is not None), _hp(_c(Brows)), _hp(_c(be)), int(kinds[0]),
                                                int(kinds[1]), _hp(out_g), _hp(kout))
        _capi.check(rc, "lssvr_newmark_sensitivity_host")
        return kout
    return proto.sweep_gradients(p, U, V, A, lam, B, ub, vb, None, size, tables, ends)


# ---- the inverse problem of the prototype --------------------------------------------------------------------------------
DEMO_FINAL = 3.370865e-03          # the misfit after 20 steps, as the prototype prints it
DEMO_WITHIN = 1.5                  # the device ends within this factor of the prototype
