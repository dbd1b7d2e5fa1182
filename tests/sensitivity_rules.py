"""Shared cases, restatement and bars of the sensitivity tests: tests/test_sensitivity_cpu.py runs
them through the numpy prototype and the library's host mirror, tests/test_gpu_sensitivity.py through the device.

The restatement is scripts/proto/sensitivity_proto.py: the dense assembly and solve, the complex-step derivative (the
yardstick: no subtraction, so it carries the rounding of one solve and nothing else) and the adjoint formulas in the
order of csrc/lssvr_sens.hpp.  The bar of a case is 10x what the float64 prototype itself reads on the SAME case -- the
deviation of its adjoint gradients from the complex step, the largest over the groups (a, b, c, f tables, end data),
each relative to the largest entry of its group.  The reading is taken when the test runs (cached), never from the code
under test; READ records what it was when the cases were written."""
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import sensitivity_proto as proto         # noqa: E402

MARGIN = 10.0
DIRICHLET, ROBIN = proto.DIRICHLET, proto.ROBIN
D, R = DIRICHLET, ROBIN
TABLES = ("a", "b", "c", "f")
# the largest reading of the prototype over the cases of each mesh, when they were written; the prototype must stay
# within 4x of it (another LAPACK build may round otherwise, a broken restatement reads 1e-3 and more)
READ = {7: 1.0e-14, 33: 2.6e-13}
READ_SLACK = 4.0


class Case:
    """One problem: ``ne`` non-uniform elements, ``nq`` points, with or without b and c (``react`` may be "helmholtz":
    c = -15, no b), the end kinds and the functional ("random": any nodal p; "goal": int (1 + x^2) u; "observe": the
    misfit at 9 points)."""

    def __init__(self, ne, nq, conv, react, kinds, functional="random"):
        self.ne, self.nq, self.conv, self.react, self.kinds, self.kind = ne, nq, conv, react, tuple(kinds), functional
        self.x = proto.mesh(ne)
        self.tabs = proto.case_tables(self.x, nq, conv, react)
        self.J = proto.functional(self.x, functional, nq)
        self.kappa, self.g = proto.KAPPA, proto.END_DATA

    @property
    def id(self):
        return (f"ne{self.ne}-q{self.nq}-{'b' if self.conv else ''}"
                f"{'h' if self.react == 'helmholtz' else 'c' if self.react else ''}-"
                f"{''.join('DR'[k] for k in self.kinds)}-{self.kind}")

    @functools.cached_property
    def reference(self):
        """(reading, adjoint dict, complex-step dict) of the prototype."""
        return proto.reading(self.x, self.tabs, self.kinds, self.J, self.kappa, self.g)

    @property
    def bar(self):
        return MARGIN * self.reference[0]

    def wrong_adjoint(self):
        """The gradients a forgotten transposition gives: z from the UNTRANSPOSED matrix."""
        u, K, bands = proto.primal(self.x, self.tabs, self.kinds, self.kappa, self.g)
        p = self.J.gradient(self.x, u)
        z = proto.bc_solve(K, p, self.kinds, self.kappa, (0.0, 0.0))
        ga, gb, gc, gf = (t[0] for t in proto.table_gradients(self.x, u, z, self.nq))
        return dict(a=ga, b=gb, c=gc, f=gf,
                    ends=proto.end_gradients(u, z, p, (bands[1][0], bands[2][-1]), self.kinds)[0])


@functools.lru_cache(maxsize=None)
def case(*key):
    return Case(*key)


def cpu_cases():
    """Test 2: 7 and 33 elements, the four end combinations, with and without b and c, nquad 1, 2, 5, and one
    Helmholtz case per mesh."""
    out = []
    for ne in (7, 33):
        for conv in (False, True):
            for nq in (1, 2, 5):
                out += [case(ne, nq, conv, conv, kinds) for kinds in proto.END_COMBOS]
        out.append(case(ne, 2, False, "helmholtz", (D, R)))
    return out


def facade_cases():
    """Test 6, 33 elements, nquad 2 -> (case, fem_solver): the four end combinations with goal and observe (b and c,
    "bands"), one pair without b and c, convection on "pivot", Helmholtz on "pivot"."""
    out = []
    for kinds in proto.END_COMBOS:
        out += [(case(33, 2, True, True, kinds, fn), "bands") for fn in ("goal", "observe")]
        out.append((case(33, 2, True, True, kinds, "goal"), "pivot"))
    out += [(case(33, 2, False, False, (D, R), fn), "bands") for fn in ("goal", "observe")]
    out += [(case(33, 2, False, "helmholtz", (D, R), fn), "pivot") for fn in ("goal", "observe")]
    return out


def facade_solver(c, fem_solver, **kw):
    """The facade configured for the case ``c``."""
    import hybrid_fem_lssvr_amd as pkg
    ends = []
    for s in range(2):
        ends.append(("robin", c.kappa[s], c.g[s]) if c.kinds[s] == ROBIN else ("dirichlet", c.g[s]))
    react = None if not c.react else proto.helmholtz if c.react == "helmholtz" else proto.reaction
    return pkg.FEMLSSVRPrimalSolver(mesh=c.x, nquad=c.nq, rhs=proto.rhs, coef=(proto.coef_a, proto.coef_da),
                                    convection=proto.convection(c.ne) if c.conv else None, reaction=react,
                                    boundary=tuple(ends), fem_solver=fem_solver, lssvr_M=9, n_colloc=16, **kw)


def facade_gradients(c, s):
    """The gradient dict (the groups of proto.deviation) of a Sensitivity ``s``."""
    return dict(a=s.d_coef, b=s.d_convection, c=s.d_reaction, f=s.d_rhs,
                ends=np.concatenate([s.d_end_values, s.d_kappa]))


# ---- the kernel's inputs and the host mirror ---------------------------------------------------------------------------------
def kernel_inputs(ne, nc, nu, seed=0):
    """x [ne+1] non-uniform, U [nu, ne+1], Z and P [nc, ne+1], band_ends [2]: random, of size 1."""
    rng = np.random.default_rng(1000 * ne + 10 * nc + nu + seed)
    x = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(ne))]) / ne - 0.3
    return dict(x=x, U=rng.standard_normal((nu, ne + 1)), Z=rng.standard_normal((nc, ne + 1)),
                P=rng.standard_normal((nc, ne + 1)), band_ends=rng.standard_normal(2))


CANARY = -7.25e77


def _hp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def sens_host(x, nq, U, Z, want=TABLES, P=None, band_ends=None, kinds=(D, D), ends=False, check=True):
    """lssvr_p1_sensitivity_host -> (rc, dict): every table of TABLES as [nc, ne, nq], canary-filled where it is not in
    ``want`` (and then not handed over), and "ends" [nc, 4] likewise with ``ends``."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    x, U, Z, P, band_ends = (None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.float64))
                             for t in (x, U, Z, P, band_ends))
    shape = (Z.shape[0], len(x) - 1, int(nq))
    out = {k: np.full(shape, CANARY) for k in TABLES}
    out["ends"] = np.full((Z.shape[0], 4), CANARY)
    rc = lib.lssvr_p1_sensitivity_host(_hp(x), len(x) - 1, int(nq), _hp(U), U.shape[0], _hp(Z), Z.shape[0],
                                       *(_hp(out[k]) if k in want else None for k in TABLES), _hp(P), _hp(band_ends),
                                       int(kinds[0]), int(kinds[1]), _hp(out["ends"]) if ends else None)
    if check:
        _capi.check(rc, "lssvr_p1_sensitivity_host")
    return rc, out


def sens_numpy(x, nq, U, Z, P=None, band_ends=None, kinds=(D, D)):
    """The same dict from the numpy restatement of the formulas, in the order of csrc/lssvr_sens.hpp."""
    out = dict(zip(TABLES, proto.table_gradients(x, U, Z, nq)))
    if band_ends is not None:
        out["ends"] = proto.end_gradients(U, Z, P, band_ends, kinds)
    return out


WANTS = (TABLES, ("a",), ("b",), ("c",), ("f",), ("a", "f"), ("b", "c"))


def check_against(got, want_tables, ref, ends):
    """``got`` (canary-prefilled) equals ``ref`` bit for bit in every table of ``want_tables`` (and in the ends with
    ``ends``) and holds its canaries everywhere else."""
    for k in TABLES:
        if k in want_tables:
            assert np.array_equal(got[k], ref[k]), k
        else:
            assert np.all(got[k] == CANARY), f"{k} was written though it was not asked for"
    if ends:
        assert np.array_equal(got["ends"], ref["ends"])
    else:
        assert np.all(got["ends"] == CANARY)


# ---- the inverse problem of the prototype --------------------------------------------------------------------------------
DEMO_FINAL = 4.825151e-05          # the misfit after 20 steps, as the prototype prints it
