"""Shared cases, restatement and bars of the enhancement-adjoint tests:
tests/test_enhance_adjoint_cpu.py runs them through the numpy prototype and the library's host mirror,
tests/test_gpu_enhance_adjoint.py through the device.

The restatement is scripts/proto/enhance_adjoint_proto.py: the forward element solve with complex data, the complex-step
derivative (the yardstick: no subtraction) and the adjoint formulas in the order of csrc/lssvr_enh_adj.hpp.  The bar of
a case is 10x what the float64 prototype itself reads on the SAME case -- the deviation of its adjoint from the complex
step, the largest over the groups (g, a, da, c, f), each relative to the largest entry of its group.  The reading is
taken when the test runs (cached), never from the code under test; READ records what it was when the cases were
written."""
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "scripts", "proto")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import enhance_adjoint_proto as proto         # noqa: E402
import sensitivity_proto as p1proto           # noqa: E402

MARGIN = 10.0
TABLES = proto.TABLES
OUTPUTS = ("u", "bc") + TABLES
MESHES = (1, 2, 7, 65, 300)
PAIRS = proto.PAIRS                 # well-conditioned
SQUARE = proto.SQUARE               # n = M - 2
VARIANTS = ((True, True), (False, True), (True, False), (False, False))        # (a and da, c)
# the largest reading of the prototype over the meshes and table variants of each pair, when the cases were written;
# the prototype must stay within 4x of it (another LAPACK build may round otherwise, a broken restatement reads 1e-3
# and more)
READ = {(3, 2): 1.1e-15, (4, 8): 1.5e-15, (9, 16): 1.5e-14, (16, 32): 2.5e-13, (9, 7): 5.1e-14}
READ_SLACK = 4.0
CANARY = -7.25e77
DOMAIN = (-1.0, 1.0)


class Case(proto.Case):
    @functools.cached_property
    def reference(self):
        """(reading, adjoint dict, complex-step dict) of the prototype."""
        return proto.reading(self)

    @property
    def bar(self):
        return MARGIN * self.reference[0]

    @functools.cached_property
    def restatement(self):
        """The numpy restatement of every output: pairs, u, bc and the tables."""
        out = self.adjoint()
        out["u"], out["bc"] = proto.gather(out["pairs"], True, True)
        return out

    def wants(self):
        return tuple(k for k in OUTPUTS if not ((k in ("a", "da") and not self.has_a) or (k == "c" and not self.has_c)))


@functools.lru_cache(maxsize=None)
def case(*key):
    return Case(*key)


def all_cases():
    """Every mesh with every pair (the square one included); the table variants on the 7- and 65-element meshes."""
    out = []
    for ne in MESHES:
        for M, n in PAIRS + (SQUARE,):
            for has_a, has_c in (VARIANTS if ne in (7, 65) else VARIANTS[:1]):
                out.append(case(ne, M, n, has_a, has_c))
    return out


def bar_cases():
    """The cases that carry the complex-step bar: one mesh per pair is enough for the yardstick (130 batched solves
    each), the small meshes and every table variant."""
    return [c for c in all_cases() if c.ne in (1, 2, 7)]


def _hp(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def adjoint_host(c, want, x=None, elem_offset=0, ne_global=None, status=None, f=None, rows=None, check=True,
                 override=None):
    """lssvr_enhance_adjoint_host on the case ``c`` (or the element range ``rows`` of it as a shard) -> (rc, dict):
    every output of OUTPUTS canary-filled where it is not in ``want`` (and then not handed over), and "pairs"."""
    from hybrid_fem_lssvr_amd import _capi
    lib = _capi.load()
    sl = slice(None) if rows is None else slice(*rows)
    x = c.x if rows is None else c.x[rows[0]:rows[1] + 1]
    ne = len(x) - 1
    cut = lambda t: None if t is None else np.ascontiguousarray(t[sl])        # noqa: E731
    tabs = dict(a=cut(c.a), da=cut(c.da), c=cut(c.c), f=cut(c.f if f is None else f), W=cut(c.W), Wbar=cut(c.Wbar))
    out = {k: np.full((ne, c.n), CANARY) for k in TABLES}
    out.update(u=np.full(ne + 1, CANARY), bc=np.full(2, CANARY), pairs=np.full((ne, 2), CANARY))
    st = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
    args = dict(x=_hp(x), ne=ne, elem_offset=elem_offset, ne_global=ne if ne_global is None else ne_global,
                gxmin=DOMAIN[0], gxmax=DOMAIN[1], M=c.M, n=c.n, gamma=c.gamma, a=_hp(tabs["a"]), da=_hp(tabs["da"]),
                c=_hp(tabs["c"]), f=_hp(tabs["f"]), W=_hp(tabs["W"]), status=None if st is None else st.ctypes.data,
                Wbar=_hp(tabs["Wbar"]), **{"g" + k: (_hp(out[k]) if k in want else None) for k in OUTPUTS},
                work=out["pairs"].ctypes.data, work_bytes=out["pairs"].nbytes)
    args.update(override or {})
    rc = lib.lssvr_enhance_adjoint_host(*args.values())
    if check:
        _capi.check(rc, "lssvr_enhance_adjoint_host")
    return rc, out


def check_against(got, want, ref):
    """``got`` (canary-prefilled) equals ``ref`` bit for bit in every output of ``want`` and holds its canaries
    everywhere else."""
    for k in OUTPUTS:
        if k in want:
            assert np.array_equal(np.asarray(got[k]).reshape(ref[k].shape), ref[k]), k
        else:
            assert np.all(np.asarray(got[k]) == CANARY), f"{k} was written though it was not asked for"


def deviation(got, c):
    """The deviation of the outputs ``got`` (pairs as "g") from the complex step of the case, over the groups ``got``
    holds."""
    cs = c.reference[2]
    return proto.deviation(got, {k: v for k, v in cs.items() if k in got})


# ---- the whole chain (the facade) ---------------------------------------------------------------------------------------
CHAIN_NE, CHAIN_M, CHAIN_N, CHAIN_GAMMA = 33, 9, 16, 1.0e4
CHAIN_KINDS = ((p1proto.DIRICHLET, p1proto.DIRICHLET), (p1proto.DIRICHLET, p1proto.ROBIN))


@functools.lru_cache(maxsize=None)
def chain(kinds, functional):
    """(Chain, per-set readings, adjoint dict, complex-step dict, value) of the prototype."""
    ch = proto.Chain(proto.mesh(CHAIN_NE), 2, CHAIN_M, CHAIN_N, CHAIN_GAMMA, kinds, functional)
    return (ch,) + proto.chain_reading(ch)


def facade_solver(ch, **kw):
    import hybrid_fem_lssvr_amd as pkg
    ends = []
    for s in range(2):
        ends.append(("robin", ch.kappa[s], ch.g[s]) if ch.kinds[s] == p1proto.ROBIN else ("dirichlet", ch.g[s]))
    return pkg.FEMLSSVRPrimalSolver(mesh=ch.x, nquad=ch.nq, rhs=p1proto.rhs, coef=(p1proto.coef_a, p1proto.coef_da),
                                    convection=p1proto.convection(len(ch.x) - 1), reaction=p1proto.reaction,
                                    boundary=tuple(ends), fem_solver="bands", lssvr_M=ch.M, lssvr_gamma=ch.gamma,
                                    n_colloc=ch.n, **kw)


def facade_gradients(s):
    """The groups of proto.Chain.adjoint of a Sensitivity ``s`` of the enhanced output."""
    return dict(a=s.d_coef, b=s.d_convection, c=s.d_reaction, f=s.d_rhs,
                ends=np.concatenate([s.d_end_values, s.d_kappa]), cf=s.d_rhs_colloc, ca=s.d_coef_colloc,
                cda=s.d_dcoef_colloc, cc=s.d_reaction_colloc)
