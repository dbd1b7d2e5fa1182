"""Shared cases, restatement and bars of the transient sensitivity tests:
tests/test_transient_sensitivity_cpu.py runs them through the numpy prototype and the library's host mirror,
tests/test_gpu_transient_sensitivity.py through the device.

The restatement is scripts/proto/transient_sensitivity_proto.py: the dense BDF loop, the complex-step derivative of every
datum (the yardstick: no subtraction, so it carries the rounding of one loop and nothing else), the backward loop and
the sums over time in the order of csrc/lssvr_chunk_sens.hpp.  The bar of a case is 10x what the float64 prototype itself
reads on the SAME case -- the deviation of its adjoint gradients from the complex step, the largest over the groups
(a, c, rho, f tables, u0, g, kappa), each relative to the largest entry of its group.  The reading is taken when the test
runs (cached), never from the code under test; READ records what it was when the cases were written."""
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import transient_sensitivity_proto as proto         # noqa: E402

sp = proto.sp
MARGIN = 10.0
DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN
D, R = DIRICHLET, ROBIN
END_COMBOS = sp.END_COMBOS
TABLES = ("a", "c", "rho", "f")
# the largest reading of the prototype over the cases of each mesh, when they were written; the prototype must stay
# within 4x of it (another LAPACK build may round otherwise, a broken restatement reads 1e-3 and more)
READ = {7: 1.4e-14, 33: 2.3e-13}
READ_SLACK = 4.0


class Case:
    """One loop: ``ne`` non-uniform elements, ``nq`` points, the end kinds, the scheme, ``N`` steps and the functional
    ("random": any nodal p_n, some steps zero; "goal": the terminal int (1 + x^2) u; "observe": the misfit at 9 points
    and two steps)."""

    def __init__(self, ne, nq, kinds, scheme, N, functional="random"):
        self.ne, self.nq, self.kinds, self.scheme, self.N, self.kind = ne, nq, tuple(kinds), scheme, N, functional
        self.p = proto.problem(ne, nq, kinds, scheme, N)
        self.J = proto.functional(self.p, functional)

    @property
    def id(self):
        return f"ne{self.ne}-q{self.nq}-{''.join('DR'[k] for k in self.kinds)}-{self.scheme}-N{self.N}-{self.kind}"

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


def cpu_cases():
    """7 elements: the four end combinations with N = 3, 8, 9, 17; 33 elements: with N = 9, 17.  nquad 1, 2, 5, the two
    schemes and the three functionals rotate so that every pairing with an end combination occurs."""
    out = []
    for ne, Ns in ((7, (3, 8, 9, 17)), (33, (9, 17))):
        for ki, kinds in enumerate(END_COMBOS):
            for j, N in enumerate(Ns):
                r = ki + j + (ne == 33)
                out.append(case(ne, (1, 2, 5)[r % 3], kinds, ("bdf2", "bdf1")[(r // 2) % 2], N,
                                ("random", "goal", "observe")[(ki + 2 * j) % 3]))
    out.append(case(7, 2, (D, R), "bdf2", 3, "random"))          # the case of the negative control
    return list(dict.fromkeys(out))


def facade_cases():
    """33 elements, nquad 2: the four end combinations x (goal, observe) x (bdf1, bdf2); N = 9 and 17 alternate."""
    out = []
    for ki, kinds in enumerate(END_COMBOS):
        for fi, fn in enumerate(("goal", "observe")):
            for si, scheme in enumerate(("bdf1", "bdf2")):
                out.append(case(33, 2, kinds, scheme, (9, 17)[(ki + fi + si) % 2], fn))
    return out


def facade_solver(c, **kw):
    """The facade configured for the case ``c``."""
    import hybrid_fem_lssvr_amd as pkg
    ends = [("robin", float(c.p.kappa[s]), 0.0) if c.kinds[s] == ROBIN else ("dirichlet", 0.0) for s in range(2)]
    return pkg.FEMLSSVRPrimalSolver(mesh=c.p.x, nquad=c.nq, coef=(sp.coef_a, sp.coef_da), reaction=sp.reaction,
                                    boundary=tuple(ends), lssvr_M=9, n_colloc=16, **kw)


def facade_args(c):
    """The keywords of solve_transient / solve_transient_sensitivity for the loop of ``c`` (without the functional)."""
    return dict(nsteps=c.N, scheme=c.scheme, weight=proto.weight, forcing=[(f, fx) for f, fx in proto.FORCING],
                end_data=(proto.g_left, proto.g_right))


def facade_functional(c):
    if c.kind == "goal":
        return dict(goal=sp.goal_density)
    steps, xo, d = proto.observations(c.N)
    return dict(observe=(steps, xo, d))


def facade_gradients(s):
    """The gradient dict (the groups of proto.deviations) of a TransientSensitivity ``s``."""
    return dict(a=s.d_coef, c=s.d_reaction, rho=s.d_weight, f=s.d_forcing, u0=s.d_u0, g=s.d_end_values,
                kappa=s.d_kappa)


# ---- the kernel's inputs and the host mirror ---------------------------------------------------------------------------------
def kernel_inputs(ne, m, nR, n0=None, seed=0):
    """Random inputs of size 1 for one chunk: x [ne+1] non-uniform, Utraj [N+1, ne+1] with N = n0+m (one row past the
    chunk), Z and Brows [m, ne+1], phi [N, max(R, 1)], band_ends [2, 2], coef [m, 3] (BDF2 rows and BDF1 rows mixed, the
    row of step 1 BDF1), band_rows, inv_dt.  ``n0`` defaults to 1: the chunk then ends at step 1, where row n-2 does not
    exist."""
    rng = np.random.default_rng(1000 * ne + 10 * m + nR + seed)
    n0 = 1 if n0 is None else n0
    N = n0 + m
    x = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(ne))]) / ne - 0.3
    steps = [n0 + m - 1 - i for i in range(m)]
    coef = np.array([proto.BDF["bdf1"] if n == 1 or rng.random() < 0.25 else proto.BDF["bdf2"] for n in steps])
    return dict(x=x, Utraj=rng.standard_normal((N + 1, ne + 1)), Z=rng.standard_normal((m, ne + 1)),
                Brows=rng.standard_normal((m, ne + 1)), phi=rng.standard_normal((N, max(nR, 1))),
                band_ends=rng.standard_normal((2, 2)), coef=coef, band_rows=[int(n != 1) for n in steps], n0=n0,
                inv_dt=7.0 + rng.random(), R=nR, m=m, ne=ne)


def initial(d, nq, seed=1):
    """Random contents for the outputs of an accumulating call: the tables and kappa."""
    rng = np.random.default_rng(seed + d["ne"])
    out = {k: rng.standard_normal((d["ne"], nq)) for k in ("a", "c", "rho")}
    out["f"] = rng.standard_normal((d["R"], d["ne"], nq))
    out["kappa"] = rng.standard_normal(2)
    return out


CANARY = -7.25e77


def _hp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _c(t):
    return None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.float64))


def band_mask(rows):
    return sum(int(r) << i for i, r in enumerate(rows))


def blank(d, nq, init=None):
    """The output dict of a call, N+1 rows of g: canaries, or copies of ``init`` (an accumulating call)."""
    N = d["Utraj"].shape[0] - 1
    out = {k: np.full((d["ne"], nq), CANARY) for k in ("a", "c", "rho")}
    out["f"] = np.full((max(d["R"], 1), d["ne"], nq), CANARY)[:d["R"]]
    out["g"], out["kappa"] = np.full((N + 1, 2), CANARY), np.full(2, CANARY)
    if init is not None:
        for k, v in init.items():
            out[k] = np.array(v, dtype=np.float64)
    return out


def ts_sens_host(d, nq, want=TABLES, kinds=(D, D), ends=False, init=None, check=True):
    """lssvr_transient_sensitivity_host on the inputs ``d`` -> (rc, dict): every table of TABLES, canary-filled where it is not
    in ``want`` (and then not handed over), and "g" [N+1, 2], "kappa" [2] likewise with ``ends``.  ``init``: the sums
    continue from it (accumulate = 1)."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    out = blank(d, nq, init)
    x, U, Z, B, phi, be, coef = (_c(d[k]) for k in ("x", "Utraj", "Z", "Brows", "phi", "band_ends", "coef"))
    rc = lib.lssvr_transient_sensitivity_host(_hp(x), d["ne"], int(nq), _hp(U), _hp(Z), d["n0"], d["m"], d["inv_dt"], _hp(coef),
                                       _hp(phi), d["R"], *(_hp(out[k]) if k in want else None for k in TABLES),
                                       int(init is not None), _hp(B), _hp(be), band_mask(d["band_rows"]),
                                       int(kinds[0]), int(kinds[1]), _hp(out["g"]) if ends else None,
                                       _hp(out["kappa"]) if ends else None)
    if check:
        _capi.check(rc, "lssvr_transient_sensitivity_host")
    return rc, out


def ts_sens_numpy(d, nq, kinds=(D, D), init=None):
    """The same dict from the numpy restatement, in the order of csrc/lssvr_chunk_sens.hpp."""
    out = proto.chunk_tables(d["x"], nq, d["Utraj"], d["Z"], d["n0"], d["inv_dt"], d["coef"], d["phi"], d["R"], init)
    out["g"] = np.full((d["Utraj"].shape[0], 2), CANARY)
    out["kappa"] = proto.chunk_ends(d["Utraj"], d["Z"], d["Brows"], d["n0"], d["band_ends"], d["band_rows"], kinds,
                                    out["g"], None if init is None else init["kappa"])
    return out


def wants(nR):
    """Every subset of the four tables ("f" only with R > 0); the empty one goes with the end gradients alone."""
    names = TABLES if nR else TABLES[:3]
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


def host_sweep(p, U, lam, B, size):
    """proto.sweep_gradients through the library's host mirror, in chunks of ``size`` steps."""
    def tables(x, nq, Utraj, Z, n0, inv_dt, coef, phi, nR, init):
        d = dict(x=x, Utraj=Utraj, Z=Z, Brows=Z, phi=phi, band_ends=np.zeros((2, 2)), coef=coef,
                 band_rows=[0] * len(Z), n0=n0, inv_dt=inv_dt, R=nR, m=len(Z), ne=len(x) - 1)
        got = ts_sens_host(d, nq, init=None if init is None else dict(init, kappa=np.zeros(2)))[1]
        return {k: got[k] for k in TABLES}

    def ends(Utraj, Z, Brows, n0, be, rows, kinds, out_g, kap):
        from hybrid_fem_lssvr_amd import _capi
        lib = _capi.load()
        kout = np.full(2, CANARY) if kap is None else np.array(kap)          # (the tables all NULL: the ends alone)
        rc = lib.lssvr_transient_sensitivity_host(_hp(_c(p.x)), len(p.x) - 1, p.nq, _hp(_c(Utraj)), _hp(_c(Z)), n0, len(Z),
                                           1.0, _hp(np.zeros((len(Z), 3))), None, 0, None, None, None, None,
                                           int(kap is not None), _hp(_c(Brows)), _hp(_c(be)), band_mask(rows),
                                           int(kinds[0]), int(kinds[1]), _hp(out_g), _hp(kout))
        _capi.check(rc, "lssvr_transient_sensitivity_host")
        return kout
    return proto.sweep_gradients(p, U, lam, B, size, tables, ends)


# ---- the inverse problem of the prototype --------------------------------------------------------------------------------
DEMO_FINAL = 6.875278e-03          # the misfit after 20 steps, as the prototype prints it
DEMO_WITHIN = 1.5                  # the device ends within this factor of the prototype
