"""Rules of the dual Gram solver's size sweep (csrc/enhance_dual.hip), shared by tests/test_dual_cpu.py,
tests/test_gpu_dual_grid.py and the recipe of tests/golden/G9_dual_grid.npz (oracle/gen_golden.py).  A plain module,
no GPU and no torch.

THE DISPATCH.  ``need = max(n, M)`` picks the kernel: 16 lanes per element up to 16 (four elements a wave), 32 lanes up
to 32 (two a wave), the wave-per-element kernel above (M <= 33, n <= 64).  GRID puts n and M on both sides of every one
of those edges (15/16/17, 31/32/33, 63/64), at the small end (2, 3; M = 2 has no bubble coefficient at all, M = 3 one)
and at M = 33 with few points, where the 64-row kernel runs with most rows idle.

THE REFERENCE.  The 60-digit minimiser of the element's QP (oracle/closed_form_mp.py), stored in the fixture for the
elements SEL of ``mesh()``, so that the GPU machine needs no mpmath.  ``dual_float64`` is the float64 numpy restatement
of the arrangement the kernels implement (``oracle.lssvr_oracle.solve_dual_projected``: boundary block eliminated,
Jacobi equilibration, LAPACK's partially pivoted LU, three safeguarded refinement steps with the carried w,
re-projection); its relative L2 coefficient error against the truth is the fixture's ``proto_err``.

THE BAR.  ``bar = max(floor, 10 x proto_err)``: floor 1e-12 up to M = 22 and 5e-11 above (the bars
tests/test_gpu_enhance_dual.py pins on the golden fixtures); the factor 10 covers the kernels' own order of the
reductions and FMAs against numpy's -- no kernel result enters it.  The dual form's float64 accuracy degrades with the
rank deficit n - (M - 2) and with gamma scl^4 (M = 3 with 64 points: one bubble coefficient behind a rank-1 64 x 64
matrix); a case whose ``proto_err`` exceeds ENVELOPE is checked for status, finiteness and the boundary rows only.
At most CAP of GRID may be outside, and no case with n <= M - 2 (the route ``lssvr_enhance`` takes by itself)."""
import collections
import functools
import os

import numpy as np

from oracle import lssvr_oracle as orc

MS = (2, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33)
NS = (2, 3, 14, 15, 16, 17, 18, 30, 31, 32, 33, 34, 62, 63, 64)
GRID = tuple((M, n) for M in MS for n in NS)
CLASSES = ("g16", "g32", "w64")
# the class corners at which every instantiation (in-kernel sin, tabulated, variable coefficients) is launched
CORNERS = ((5, 16), (16, 3), (17, 32), (32, 17), (33, 12), (20, 64), (33, 64))
# one corner per class for the shard / lane-group launches (n = LPE in the lane classes, idle rows in the 64-row one)
SHARD_CORNERS = ((5, 16), (17, 32), (33, 12))

NE = 9
SEL = (0, 4, 8)
GAMMA = 1e4
ENVELOPE = 1e-8
CAP = 0.15
MARGIN = 10.0
MP = 33                       # row length of the fixture's coefficient arrays (zero beyond M)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G9_dual_grid.npz")

Case = collections.namedtuple("Case", "M n proto_err")


def kernel_class(M, n):
    """The kernel ``enhance_dual`` launches for (M, n): "g16" | "g32" | "w64"."""
    if not (2 <= M <= 33 and 2 <= n <= 64):
        raise ValueError("the dual solver takes 2 <= M <= 33, 2 <= n <= 64, got (%d, %d)" % (M, n))
    need = max(M, n)
    return "g16" if need <= 16 else "g32" if need <= 32 else "w64"


def floor(M):
    return 1e-12 if M <= 22 else 5e-11


def bar(case):
    """max(floor, 10 x proto_err) of a :class:`Case`; ``proto_err`` is the reference's own error, never the kernel's."""
    return max(floor(case.M), MARGIN * case.proto_err)


def in_envelope(case):
    return case.proto_err <= ENVELOPE


@functools.lru_cache(maxsize=None)
def mesh(ne=NE):
    """(nodes[ne+1], values[ne+1], global_domain) of the one seeded non-uniform mesh: element widths U(0.05, 0.4) from
    -0.9, nodal values sin(pi x) + 1e-2 standard normal noise (not zero at the ends: the Dirichlet replacement shows).
    ne = 9 is odd on purpose: the last wave of the 16-lane kernel has one live and three idle groups, that of the
    32-lane kernel one live and one idle.  Read-only."""
    rng = np.random.default_rng([20261019, ne])
    nodes = np.cumsum(np.concatenate([[-0.9], rng.uniform(0.05, 0.4, ne)]))
    values = np.sin(np.pi * nodes) + 1e-2 * rng.standard_normal(ne + 1)
    for t in (nodes, values):
        t.setflags(write=False)
    return nodes, values, (float(nodes[0]), float(nodes[-1]))


@functools.lru_cache(maxsize=None)
def varcoef():
    """(a, a', f) of the non-trivial coefficient the variable-coefficient launches use."""
    return orc.varcoef_functions(*orc.varcoef_params())


def wide_domain():
    """A global domain that contains ``mesh()`` strictly: no element end is a Dirichlet end."""
    nodes = mesh()[0]
    return (float(nodes[0]) - 1.0, float(nodes[-1]) + 1.0)


def systems(M, n, elements=SEL, vc=False, interior=False):
    """The element systems of ``elements`` of ``mesh()``: Poisson rows with f = pi^2 sin(pi x), or (``vc``) the rows
    of -(a u')' = f with :func:`varcoef`; ``interior``: the mesh as a window of a larger one (:func:`wide_domain`)."""
    nodes, values, gd = mesh()
    kw = {}
    rhs = orc.poisson_rhs
    if vc:
        a, da, rhs = varcoef()
        kw = dict(coef_a=a, coef_da=da)
    return list(orc.mesh_element_systems(nodes, values, M, GAMMA, n, rhs, wide_domain() if interior else gd,
                                         list(elements), **kw))


def dual_float64(system):
    """float64 restatement of the arrangement the kernels implement (see the module docstring)."""
    return orc.solve_dual_projected(system, refine=3, carried=True)


def proto_err(systems_, truth):
    """max over the elements of the relative L2 coefficient error of :func:`dual_float64` against ``truth``."""
    W = np.array([dual_float64(s) for s in systems_])
    return float(orc.rel_l2_coef(W, np.asarray(truth)[:, :W.shape[1]]).max())


class Fixture:
    """tests/golden/G9_dual_grid.npz: truths (60 digits) and ``proto_err`` of GRID, CORNERS (Poisson and variable
    coefficients) and SHARD_CORNERS as an interior window, all for the elements SEL of ``mesh()``."""

    def __init__(self, path=FIXTURE):
        g = dict(np.load(path, allow_pickle=False))
        self.g = g
        if (tuple(g["Ms"]), tuple(g["ns"]), tuple(g["sel"])) != (MS, NS, SEL) or \
                tuple(map(tuple, g["corners"])) != CORNERS or tuple(map(tuple, g["shard_corners"])) != SHARD_CORNERS:
            raise RuntimeError("G9_dual_grid.npz was written for another grid: rerun oracle/gen_golden.py --only G9")
        nodes, values, _ = mesh()
        if not (np.array_equal(g["nodes"], nodes) and np.array_equal(g["values"], values)):
            raise RuntimeError("G9_dual_grid.npz was written for another mesh: rerun oracle/gen_golden.py --only G9")

    def _get(self, truth, err, idx, M, n):
        return self.g[truth][idx][:, :M], Case(M, n, float(self.g[err][idx]))

    def grid(self, M, n):
        """(truth[3, M], Case) of a GRID pair."""
        return self._get("truth", "proto_err", (MS.index(M), NS.index(n)), M, n)

    def corner(self, M, n, vc=False):
        """(truth[3, M], Case) of a CORNERS pair: Poisson rows, or the rows of :func:`varcoef`."""
        return self._get("vc_truth" if vc else "corner_truth", "vc_proto_err" if vc else "corner_proto_err",
                         CORNERS.index((M, n)), M, n)

    def window(self, M, n):
        """(truth[3, M], Case) of a SHARD_CORNERS pair with every element interior."""
        return self._get("window_truth", "window_proto_err", SHARD_CORNERS.index((M, n)), M, n)

    def cases(self):
        return [self.grid(M, n)[1] for M, n in GRID]


@functools.lru_cache(maxsize=None)
def fixture():
    return Fixture()


def build_fixture(progress=None):
    """The arrays of the fixture (needs mpmath): ``oracle/gen_golden.py --only G9`` stores them."""
    from oracle import closed_form_mp as cf

    def block(pairs, **kw):
        tr = np.zeros((len(pairs), len(SEL), MP))
        er = np.zeros(len(pairs))
        for i, (M, n) in enumerate(pairs):
            ss = systems(M, n, **kw)
            tr[i, :, :M] = [cf.solve_truth(s) for s in ss]
            er[i] = proto_err(ss, tr[i])
            if progress:
                progress(M, n, kw, er[i])
        return tr, er

    nodes, values, _ = mesh()
    out = dict(Ms=np.array(MS), ns=np.array(NS), sel=np.array(SEL), corners=np.array(CORNERS),
               shard_corners=np.array(SHARD_CORNERS), nodes=np.array(nodes), values=np.array(values),
               gamma=np.float64(GAMMA))
    tr, er = block(GRID)
    out["truth"], out["proto_err"] = tr.reshape(len(MS), len(NS), len(SEL), MP), er.reshape(len(MS), len(NS))
    out["corner_truth"], out["corner_proto_err"] = block(CORNERS)
    out["vc_truth"], out["vc_proto_err"] = block(CORNERS, vc=True)
    out["window_truth"], out["window_proto_err"] = block(SHARD_CORNERS, interior=True)
    return out
