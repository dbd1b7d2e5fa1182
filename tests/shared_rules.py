"""numpy restatement of the shared-operator enhancement (csrc/enhance_shared.hip: lssvr_enhance_shared), the cases the
CPU and GPU tests share, and the bars.  A plain module, no GPU and no torch: tests/test_shared_cpu.py pins it to the
float64 oracle, tests/test_gpu_shared.py compares the kernel with it.

THE OPERATION.  On a uniform mesh the minimiser is linear in the data,
    w_e = sum_k P_k f(x_k) (h_e/2)^2 + P_l g_l + P_r g_r,
with P the (n+2) x M response table of ONE canonical element of length h0, laid out as ops.build_shared_operator lays it
out: unit f~ rows on the first n elements of an (n+2)-element auxiliary mesh of spacing h0 centred on 0, unit g_r on
element n, unit g_l on element n+1.  :func:`restate` does exactly this with the oracle's element solve; x_k, (h_e/2)^2
and (g_l, g_r) are each element's own, as in the kernel.

THE BARS.  Nothing here is read from the kernel.  For every case the restatement's OWN distance from the float64 oracle
(orc.enhance_all_vec on the same data) is read on the CPU, in rel_l2_coef and in rel_l2_bubble; the GPU bar is
max(MARGIN x that reading, FLOOR) with MARGIN = 10 (wave_rules.MARGIN: one different order of summation) and FLOOR =
1e-13 (the general path's bar).  The readings taken when the cases were written stand beside them; test_shared_cpu.py
recomputes them and holds them to those figures."""
import functools

import numpy as np

from oracle import closed_form_mp as cf
from oracle import lssvr_oracle as orc

MARGIN = 10.0
FLOOR = 1e-13
GAMMA = 1e4
NE0 = 130                     # two full waves of 64 and a tail of two
LO, HI = -1.0, 1.0
BC = (0.3, -0.7)              # shard test: differs from the nodal end values


# --------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------
def colloc(nodes, n):
    """x[e, k] = np.linspace(nodes[e], nodes[e+1], n)[k] (orc.np_linspace, vectorised as in orc.enhance_all_vec)."""
    nodes = np.asarray(nodes, dtype=np.float64)
    a, b = nodes[:-1], nodes[1:]
    step = (b - a) / (n - 1)
    x = np.arange(n, dtype=np.float64)[None, :] * step[:, None]
    x = x + a[:, None]
    x[:, -1] = b
    return x


def spacing(nodes):
    """The h0 the facade hands to ops.build_shared_operator: the mean element length."""
    return float((nodes[-1] - nodes[0]) / (len(nodes) - 1))


@functools.lru_cache(maxsize=None)
def _response_table(h0, M, gamma, n, truth):
    nel = n + 2
    nodes = (np.arange(nel + 1, dtype=np.float64) - 0.5 * nel) * h0
    scl = 2.0 / float(nodes[1] - nodes[0])
    solve = cf.solve_truth if truth else orc.solve_bc_eliminated
    P = np.zeros((nel, M))
    for k in range(n):
        f = np.zeros(n)
        f[k] = scl * scl                                   # f~ = f / scl^2 = e_k
        P[k] = solve(orc.element_system(nodes[k], nodes[k + 1], 0.0, 0.0, M, gamma, n, f_values=f))
    zero = np.zeros(n)
    P[n] = solve(orc.element_system(nodes[n + 1], nodes[n + 2], 1.0, 0.0, M, gamma, n, f_values=zero))   # g_l
    P[n + 1] = solve(orc.element_system(nodes[n], nodes[n + 1], 0.0, 1.0, M, gamma, n, f_values=zero))   # g_r
    P.setflags(write=False)
    return P


def response_table(h0, M, gamma, n, truth=False):
    """float64[n+2, M]: rows k < n the response to f~ = e_k, row n to g_l = 1, row n+1 to g_r = 1.  ``truth``: every
    element solve in 60 digits (cf.solve_truth), rounded once."""
    return _response_table(float(h0), int(M), float(gamma), int(n), bool(truth))


def end_values(nodes, values, global_domain, bc=(0.0, 0.0), elem_offset=0, ne_global=None):
    """(g_l[ne], g_r[ne]) by orc.boundary_values (Dual.py:65-75) for the shard (nodes, values)."""
    ne = len(nodes) - 1
    ng = elem_offset + ne if ne_global is None else ne_global
    g = np.array([orc.boundary_values(e + elem_offset, ng, nodes[e], nodes[e + 1], values[e], values[e + 1],
                                      global_domain, bc[0], bc[1]) for e in range(ne)], dtype=np.float64)
    return g[:, 0], g[:, 1]


def restate(nodes, values, M, gamma, n, f_table, global_domain, bc=(0.0, 0.0), elem_offset=0, ne_global=None,
            h0=None, truth=False):
    """W float64[ne, M] of lssvr_enhance_shared; ``f_table`` float64[ne, n] is f at :func:`colloc`."""
    nodes = np.asarray(nodes, dtype=np.float64)
    values = np.asarray(values, dtype=np.float64)
    P = response_table(spacing(nodes) if h0 is None else h0, M, gamma, n, truth)
    h = nodes[1:] - nodes[:-1]
    ft = np.asarray(f_table, dtype=np.float64) * (0.25 * (h * h))[:, None]
    gl, gr = end_values(nodes, values, global_domain, bc, elem_offset, ne_global)
    W = np.zeros((len(h), M))
    for k in range(n):                  # the kernel's order of summation (it fuses each step; numpy rounds twice)
        W += ft[:, k:k + 1] * P[k][None, :]
    W += gl[:, None] * P[n][None, :]
    W += gr[:, None] * P[n + 1][None, :]
    return W


def linear_rows(nodes, values, M, global_domain, bc=(0.0, 0.0), elem_offset=0, ne_global=None):
    """The fallback rows [0.5 (g_l + g_r), 0.5 (g_r - g_l), 0, ...] (Dual.py:164-169), the kernel's two operations."""
    gl, gr = end_values(np.asarray(nodes, dtype=np.float64), np.asarray(values, dtype=np.float64), global_domain, bc,
                        elem_offset, ne_global)
    W = np.zeros((len(gl), M))
    W[:, 0] = 0.5 * (gl + gr)
    W[:, 1] = 0.5 * (gr - gl)
    return W


def oracle(nodes, values, M, gamma, n, f_table, global_domain, bc=(0.0, 0.0)):
    """orc.enhance_all_vec on the same data (one chunk: the table stands in for rhs(x))."""
    f_table = np.asarray(f_table, dtype=np.float64)
    return orc.enhance_all_vec(nodes, values, M, gamma, n, rhs=lambda x: f_table, global_domain=global_domain,
                               bc_left=bc[0], bc_right=bc[1], chunk=len(nodes))


def reading(nodes, values, M, gamma, n, f_table, global_domain, bc=(0.0, 0.0), truth=False):
    """(rel_l2_coef, rel_l2_bubble) maxima of the restatement against the float64 oracle: what the bars are built
    from."""
    Wr = restate(nodes, values, M, gamma, n, f_table, global_domain, bc, truth=truth)
    Wo = oracle(nodes, values, M, gamma, n, f_table, global_domain, bc)
    return float(orc.rel_l2_coef(Wr, Wo).max()), float(orc.rel_l2_bubble(Wr, Wo).max())


def bar(read):
    return max(MARGIN * read, FLOOR)


# --------------------------------------------------------------------------
# data
# --------------------------------------------------------------------------
def mesh(ne=NE0, lo=LO, hi=HI):
    return np.linspace(lo, hi, ne + 1)


def nodal(nodes):
    """Smooth nodal values that vanish nowhere near the ends (so that bc substitution is visible) and have no
    symmetry a left/right slip could hide behind."""
    return np.sin(np.pi * nodes) + 0.25 * np.cos(3.0 * nodes) + 0.125 * nodes


def sine_table(nodes, n, amp=orc.PI_SQ, omega=orc.PI):
    """amp * np.sin(omega * x_k): numpy's argument rounding, numpy's sine."""
    return amp * np.sin(omega * colloc(nodes, n))


def distinct_table(ne, n, e0=0):
    """Entry (e, k) = 1 + e + k/64: distinct for every pair (k < 64), exact in float64: a row or column slip cannot
    cancel."""
    return 1.0 + (e0 + np.arange(ne, dtype=np.float64))[:, None] + np.arange(n, dtype=np.float64)[None, :] / 64.0


def sine_exact(nodes, n, amp, omega):
    """amp * sin(fl(omega * x_k)) with the sine in extended precision (mpmath at 40 digits where present, else
    np.longdouble) at the float64 argument numpy would form, rounded once; the product with amp is float64's."""
    arg = omega * colloc(nodes, n)
    if cf.HAVE_MP:
        import mpmath as mp
        with mp.workdps(40):
            s = np.array([float(mp.sin(mp.mpf(float(v)))) for v in arg.ravel()]).reshape(arg.shape)
    else:
        s = np.sin(arg.astype(np.longdouble)).astype(np.float64)
    return amp * s


# --------------------------------------------------------------------------
# case lists
# --------------------------------------------------------------------------
N_LIST = (5, 7, 12, 17, 23, 30, 36, 44, 52, 60)       # none a multiple of 8


def n_for(M):
    """The smallest n of N_LIST with n >= M + max(0, M - 12): n = M is allowed up to M = 12, twice the excess over 12
    beyond.  The solve needs n >= M - 2 only, but on this mesh (eps = 1/(gamma scl^4) = 3.5e-13) a near-square system
    above M = 18 is so ill-conditioned that two float64 solves of the SAME element disagree: the restatement reads
    1.8e-13 at (M, n) = (23, 23), 2.0e-11 at (24, 23), 1.9e-10 at (29, 30), 2.5e-8 at (30, 30), 9.6e-12 at (31, 36),
    9.8e-9 at (33, 36) against orc.enhance_all_vec -- beyond the existing 1e-11, a statement about the problem and not
    about any kernel; such (M, n) do not belong on the BASELINE meshes and are not cases here.  With this rule every
    degree reads 2.4e-14 .. 2.5e-14 (RECORDED)."""
    return next(n for n in N_LIST if n >= M + max(0, M - 12))


DEGREES = tuple((M, n_for(M)) for M in range(2, 34))
TAILS = (1, 2, 63, 64, 65, 255, 256, 257, 300)
TAIL_CFG = ((9, 16), (33, 40))
STAGING = tuple((n, min(9, n + 2)) for n in (2, 5, 7, 8, 9, 12, 17))      # (n, M <= n + 2)
FALLBACK_NE = (65, 130)
FALLBACK_M = (2, 3, 9, 33)
SHARD_NE, SHARD_CUTS = 300, (0, 63, 64, 65, 250, 300)
STORE_M, STORE_N, STORE_NE = 32, 52, 65536     # 65536 * 32 = 2^21 doubles exactly: the last write-through size
BUBBLE = ((4096, 9, 16, 1e4, -1.0, 1.0), (3000, 16, 24, 1e3, -125.0, 125.0))

# Largest readings of the restatement against orc.enhance_all_vec when the cases were written, (rel_l2_coef,
# rel_l2_bubble) per list; ne = NE0 on [-1, 1].  rel_l2_coef is 2.4e-14 .. 2.5e-14 on every case: it is the end element
# (|x|/h = 65 roundings of t_k = off + scl x_k that the canonical element does not share), not the degree.
# test_shared_cpu.py recomputes every reading, prints it, and allows RECORD_SLACK x these (another LAPACK build may round
# the oracle's LU differently), never more.
RECORDED = {"degrees": (2.5e-14, 4.1e-14),      # bubble: 4.0e-14 at M = 32, below 1.1e-14 up to M = 27
            "staging": (2.5e-14, 2.0e-15),
            "bubble": (2.0e-13, 2.3e-13)}       # BUBBLE: (4.3e-16, 1.1e-14) at ne = 4096, (2.0e-13, 2.2e-13) at ne = 3000
RECORD_SLACK = 4.0


@functools.lru_cache(maxsize=None)
def degree_case(M, n, kind="sine", ne=NE0):
    """(nodes, values, f_table, (coef, bubble) reading) of a default-mesh case; ``kind``: "sine" (Poisson f) or
    "distinct"."""
    nodes = mesh(ne)
    values = nodal(nodes)
    f = sine_table(nodes, n) if kind == "sine" else distinct_table(ne, n)
    for arr in (nodes, values, f):
        arr.setflags(write=False)
    return nodes, values, f, reading(nodes, values, M, GAMMA, n, f, (LO, HI))


# --------------------------------------------------------------------------
# trigonometry cases (item 4): the host arithmetic of the kernel's branch decisions
# --------------------------------------------------------------------------
class Trig:
    """One in-kernel-sine case: mesh, (amp, omega), (M, n) and the branch it is meant to reach."""

    def __init__(self, name, branch, ne, amp, omega, M, n):
        self.name, self.branch, self.ne, self.amp, self.omega, self.M, self.n = name, branch, ne, amp, omega, M, n
        self.nodes = mesh(ne)
        self.values = nodal(self.nodes)

    def __repr__(self):
        return self.name


RESTORE_LO, RESTORE_HI = 0.999999e-7, 1.000001e-7


def trig_predicates(nodes, n, omega):
    """What the kernel decides, recomputed in float64 exactly as it computes it (products and sums are single float64
    operations there; -ffp-contract=off): per element th0 = fl(omega a), dth = fl(omega fl(h/(n-1))), crit = |th0| +
    n |dth|; per point arg = fl(omega x_k) and delta = arg - th0 - k dth (the kernel's one fused operation is taken in
    long double and rounded: the predicates keep 1e-6 relative away from 1e-7, so the last bit does not move them); per
    wave of 64 elements the wave-uniform decisions -- ``restore`` / ``quiet`` [wave, k]: some lane of the wave restores
    the argument at point k (then the whole wave evaluates the sine afresh) / no lane does (first-order restore).  Dead lanes of the last wave repeat the last element and change no
    decision."""
    nodes = np.asarray(nodes, dtype=np.float64)
    a, b = nodes[:-1], nodes[1:]
    step = (b - a) / (n - 1)
    th0 = omega * a
    dth = omega * step
    crit = np.abs(th0) + float(n) * np.abs(dth)
    arg = omega * colloc(nodes, n)
    LD = np.longdouble
    k = np.arange(n, dtype=LD)[None, :]
    delta = ((arg - th0[:, None]).astype(LD) - k * dth.astype(LD)[:, None]).astype(np.float64)
    ne = len(a)
    waves = [slice(s, min(s + 64, ne)) for s in range(0, ne, 64)]
    return dict(th0=th0, dth=dth, crit=crit, arg=arg, delta=delta, waves=waves,
                step_table=[bool(not np.all(np.abs(dth[w]) < 0.5)) for w in waves],
                small=[bool(np.all(crit[w] < 64.0)) for w in waves],
                mixed=[bool(np.any(crit[w] < 64.0) and not np.all(crit[w] < 64.0)) for w in waves],
                large=[bool(not np.any(crit[w] < 64.0)) for w in waves],
                restore=np.array([np.any(np.abs(delta[w]) >= RESTORE_HI, axis=0) for w in waves]),
                quiet=np.array([np.all(np.abs(delta[w]) < RESTORE_LO, axis=0) for w in waves]))


# (a1) step angle through the table, rotation used as it is: a coarse mesh, omega h/(n-1) = 2 and |th0| + n|dth| <= 26
# (a2) step angle through the table on the per-point path: omega h/(n-1) = 2.56; a Taylor pair would be off by
#      2.56^15/15! = 1e-6 there
# (a3) a second (amp, omega) on the plain path: Taylor pair, rotation as it is
# (b)  omega = 200 on 322 elements: waves entirely below 64, entirely above, and straddling
# (c)  |omega x| up to 1e9: ulp(1e9) = 1.2e-7, so numpy's rounding of the argument moves it by more than 1e-7 at about
#      half of the (wave, point) pairs and by less at the others (both restores run)
# (d)  |omega x| up to 4e9: beyond 3e9 the in-kernel sine gives NaN -> linear fallback
TRIG = (
    Trig("a1_table_step_small_args", "a", 4, 1.5, 16.0, 6, 5),
    Trig("a2_table_step_per_point", "a", NE0, 1.5, 2500.0, 9, 16),
    Trig("a3_other_amp_omega", "a3", NE0, 2.5, 1.7, 9, 16),
    Trig("b_straddle_64", "b", 322, orc.PI_SQ, 200.0, 9, 16),
    Trig("c_restore_1e9", "c", NE0, 1.0, 1.0e9, 9, 16),
)
TRIG_D = Trig("d_beyond_3e9", "d", NE0, 1.0, 4.0e9, 9, 16)
D_OK, D_NAN = 2.9e9, 3.1e9


def trig_reaches(case):
    """The branch evidence of one case: a dict of named booleans, all of which must hold."""
    p = trig_predicates(case.nodes, case.n, case.omega)
    if case.name.startswith("a1"):
        return dict(step_table_everywhere=all(p["step_table"]), rotation_as_is=all(p["small"]))
    if case.name.startswith("a2"):
        return dict(step_table_everywhere=all(p["step_table"]), per_point=not any(p["small"]),
                    taylor_would_show=bool(np.min(np.abs(p["dth"])) > 2.0))
    if case.branch == "a3":
        return dict(taylor_pair=not any(p["step_table"]), rotation_as_is=all(p["small"]),
                    not_default=(case.amp, case.omega) != (orc.PI_SQ, orc.PI))
    if case.branch == "b":
        return dict(taylor_pair=not any(p["step_table"]), some_wave_small=any(p["small"]),
                    some_wave_straddles=any(p["mixed"]), some_wave_large=any(p["large"]),
                    tail_wave=len(case.nodes) % 64 != 1)
    if case.branch == "c":
        big = np.abs(p["arg"]).max()
        return dict(fresh_sine_somewhere=bool(p["restore"].any()), first_order_somewhere=bool(p["quiet"][:, 1:].any()),
                    order_1e9=bool(5e8 <= big < D_OK), per_point=not any(p["small"]),
                    uniform_to_the_ulp=bool(np.ptp(np.diff(case.nodes)) <= 2.0 ** -52))
    if case.branch == "d":
        ok, nan = d_split(case)
        return dict(some_ok=bool(ok.any()), some_nan=bool(nan.any()), some_between=bool((~ok & ~nan).any()))
    raise ValueError(case.name)


def d_split(case):
    """(ok[ne], nan[ne]): every |omega x_k| of the element below D_OK / above D_NAN."""
    arg = np.abs(case.omega * colloc(case.nodes, case.n))
    return np.all(arg < D_OK, axis=1), np.all(arg > D_NAN, axis=1)
