"""numpy prototype of the adjoint of the element solve: the map (g, a, da, c, f) -> W of
oracle/lssvr_oracle.py::element_system + solve_bc_eliminated restated for all elements at once with complex data allowed
(np.linalg.solve), the complex-step derivative Im J(theta + i 1e-30 delta) / 1e-30 of J = sum Wbar . W with respect to
every datum, and the adjoint formulas that csrc/lssvr_enh_adj.hpp evaluates, in its order of operations (direct Gram,
LDL^T without square roots, two triangular solves, a second sweep over the points), one rounding per operation: bit for
bit the library's values.  Then the fallback rule, the nodal gather with end replacement and, composed with
sensitivity_proto, the whole chain  tables -> P1 solve -> enhancement -> J.  No GPU, nothing but numpy.

Run as a script it prints what DESIGN.md section 33 records."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(os.path.dirname(_HERE)), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle.lssvr_oracle import legendre_tables, mapparms, np_linspace      # noqa: E402
import sensitivity_proto as p1                                                 # noqa: E402

CSTEP = 1e-30
TABLES = ("a", "da", "c", "f")
GROUPS = ("g",) + TABLES
ST_FALLBACK = 1


# ---- the forward restatement: real or complex data ------------------------------------------------------------------------
def colloc_points(x, n):
    """[ne, n]: np.linspace(x_e, x_{e+1}, n) of every element."""
    return np.stack([np_linspace(x[e], x[e + 1], n) for e in range(len(x) - 1)])


def element_operators(x, M, n):
    """The mesh-only parts: (scl [ne], L, D1, D2 [ne, n, M], B [ne, 2, M]) in the oracle's arithmetic."""
    ne = len(x) - 1
    off, scl = (np.array(v) for v in zip(*(mapparms(x[e], x[e + 1]) for e in range(ne))))
    t = off[:, None] + scl[:, None] * colloc_points(x, n)
    L, D1, D2 = (v.reshape(ne, n, M) for v in legendre_tables(t.ravel(), M))
    tab = np.stack([off + scl * x[:-1], off + scl * x[1:]], axis=1)
    B = legendre_tables(tab.ravel(), M)[0].reshape(ne, 2, M)
    return scl, L, D1, D2, B


def forward(x, g, M, n, gamma, f, a=None, da=None, c=None):
    """W [ne, M] of the end values g [ne, 2] and the tables [ne, n] (a None: a = 1, da = 0; c None: 0): the notation of
    element_system / solve_bc_eliminated, S v = r by np.linalg.solve."""
    scl, L, D1, D2, B = element_operators(x, M, n)
    s1, s2 = scl[:, None, None], (scl * scl)[:, None, None]
    A = -D2 if a is None else -(a[:, :, None] * D2) - (da[:, :, None] / s1) * D1
    if c is not None:
        A = A + (c[:, :, None] / s2) * L
    ftil = f / s2[:, :, 0]
    eps = 1.0 / (gamma * scl ** 4)
    B1i = np.linalg.inv(B[:, :, :2])
    d = np.einsum("eij,ej->ei", B1i, g)
    if M == 2:
        return d
    C = B1i @ B[:, :, 2:]
    Abar = A[:, :, 2:] - A[:, :, :2] @ C
    fbar = ftil - np.einsum("ekj,ej->ek", A[:, :, :2], d)
    At = np.swapaxes(Abar, 1, 2)
    S = At @ Abar + eps[:, None, None] * (np.eye(M - 2) + np.swapaxes(C, 1, 2) @ C)
    r = np.einsum("ejk,ek->ej", At, fbar) + eps[:, None] * np.einsum("eij,ei->ej", C, d)
    v = np.linalg.solve(S, r[:, :, None])[:, :, 0]
    return np.concatenate([d - np.einsum("eij,ej->ei", C, v), v], axis=1)


def complex_step(x, g, M, n, gamma, Wbar, f, a=None, da=None, c=None):
    """dict(g= [ne, 2], f=, a=, da=, c= [ne, n]) of J = sum Wbar . W: entry k of every element is perturbed in one
    batched solve (the elements do not couple)."""
    data = dict(g=g, f=f, a=a, da=da, c=c)
    out = {}
    for name, v in data.items():
        if v is None:
            continue
        grad = np.zeros(v.shape)
        for k in range(v.shape[1]):
            t = dict(data)
            t[name] = v.astype(complex)
            t[name][:, k] += 1j * CSTEP
            W = forward(x, t["g"], M, n, gamma, t["f"], t["a"], t["da"], t["c"])
            grad[:, k] = np.sum(Wbar * W, axis=1).imag / CSTEP
        out[name] = grad
    return out


# ---- the adjoint, in the order of csrc/lssvr_enh_adj.hpp ---------------------------------------------------------------------
def _legendre_p(t, M):
    L = [np.ones_like(t), t]
    for p in range(1, M - 1):
        al, be = float(2 * p + 1) / float(p + 1), float(p) / float(p + 1)
        L.append((al * t) * L[p] - be * L[p - 1])
    return L[:M]


def _legendre_d1(t, M):
    """D1[p] = L'_p, p < M: D1[0] = 0 (never read), r_m = L'_{m+1} by the Gegenbauer recurrence."""
    r = [np.ones_like(t), 3.0 * t]
    for m in range(2, M - 1):
        al, be = float(2 * m + 1) / float(m), float(m + 1) / float(m)
        r.append((al * t) * r[m - 1] - be * r[m - 2])
    return [None] + r[:M - 1]


def _legendre_d2(t, M):
    """D2[p] = L''_p, p < M: D2[0] = D2[1] = 0 (never read), q_m = L''_{m+2}."""
    q = [np.full_like(t, 3.0), 15.0 * t]
    for m in range(2, M - 2):
        al, be = float(2 * m + 3) / float(m), float(m + 3) / float(m)
        q.append((al * t) * q[m - 1] - be * q[m - 2])
    return [None, None] + q[:M - 2]


def _tri(i, j):
    return i * (i + 1) // 2 + j


def kernel_adjoint(x, M, n, gamma, f, W, Wbar, a=None, da=None, c=None, status=None, drop_qw=False):
    """dict(pairs= [ne, 2] = (gl, gr) of every element, a=, da=, c=, f= [ne, n]) of the stored W [ne, M] and
    Wbar = dJ/dW: every operation of enh_adj_element, all elements at once.  ``drop_qw``: the negative control, the
    - q (. w) terms of the table gradients left out."""
    x, f, W, Wbar = (np.asarray(v, dtype=np.float64) for v in (x, f, W, Wbar))
    ne, MR = len(x) - 1, M - 2
    one, zero = np.ones((ne, n)), np.zeros((ne, n))
    ta_, td_, tc_ = (one if a is None else a), (zero if da is None else da), (zero if c is None else c)
    with np.errstate(all="ignore"):
        xa, xb = x[:-1], x[1:]
        oldlen = xb - xa
        off = (-xb - xa) / oldlen
        scl = 2.0 / oldlen
        step = oldlen / float(n - 1)
        scl2 = scl * scl
        inv_scl2 = 1.0 / scl2
        eps = 1.0 / (gamma * (scl2 * scl2))
        hs = 0.5 * oldlen
        ta, tb = off + scl * xa, off + scl * xb
        La, Lb = _legendre_p(ta, M), _legendre_p(tb, M)
        idet = 1.0 / (tb - ta)
        C0 = [(tb * La[j + 2] - ta * Lb[j + 2]) * idet for j in range(MR)]
        C1 = [(Lb[j + 2] - La[j + 2]) * idet for j in range(MR)]

        def point(k):
            if k == n - 1:
                xk = xb
            else:
                xk = np.where(step == 0.0, (float(k) / float(n - 1)) * oldlen, float(k) * step) + xa
            t = off + scl * xk
            return t, ta_[:, k], td_[:, k] * hs, tc_[:, k] * inv_scl2

        # pass 1: S = sum_k Abar_k Abar_k^T (packed lower triangle), then the ridge
        S = [np.zeros(ne) for _ in range(MR * (MR + 1) // 2)]
        for k in range(n):
            t, ak, bk, cs = point(k)
            L, D1, D2 = _legendre_p(t, M), _legendre_d1(t, M), _legendre_d2(t, M)
            A0, A1 = cs, cs * t - bk
            Ab = [((cs * L[j + 2] - bk * D1[j + 2]) - ak * D2[j + 2]) - (A0 * C0[j] + A1 * C1[j]) for j in range(MR)]
            for i in range(MR):
                for j in range(i + 1):
                    S[_tri(i, j)] = S[_tri(i, j)] + Ab[i] * Ab[j]
        for i in range(MR):
            for j in range(i + 1):
                cc = C0[i] * C0[j] + C1[i] * C1[j]
                if i == j:
                    cc = cc + 1.0
                S[_tri(i, j)] = S[_tri(i, j)] + eps * cc
        # LDL^T in place: unit L below the diagonal, the diagonal holds 1 / d_j
        for j in range(MR):
            rinv = 1.0 / S[_tri(j, j)]
            S[_tri(j, j)] = rinv
            for cc_ in range(j + 1, MR):
                lcj = S[_tri(cc_, j)] * rinv
                for i in range(cc_, MR):
                    S[_tri(i, cc_)] = S[_tri(i, cc_)] - S[_tri(i, j)] * lcj
                S[_tri(cc_, j)] = lcj
        wb = [Wbar[:, i] for i in range(M)]
        w = [W[:, i] for i in range(M)]
        y = [wb[j + 2] - (C0[j] * wb[0] + C1[j] * wb[1]) for j in range(MR)]
        for i in range(MR):
            s = y[i]
            for j in range(i):
                s = s - S[_tri(i, j)] * y[j]
            y[i] = s
        for i in range(MR - 1, -1, -1):
            s = y[i] * S[_tri(i, i)]
            for j in range(i + 1, MR):
                s = s - S[_tri(j, i)] * y[j]
            y[i] = s
        yh0, yh1 = np.zeros(ne), np.zeros(ne)
        for j in range(MR):
            yh0 = yh0 - C0[j] * y[j]
            yh1 = yh1 - C1[j] * y[j]
        yh = [yh0, yh1] + y

        # pass 2: q_k, e_k from the six evaluations, the table rows and Ahat1^T q
        out = {k: np.zeros((ne, n)) for k in TABLES}
        t0, t1 = np.zeros(ne), np.zeros(ne)

        def dot(T, v, first):
            s = np.zeros(ne)
            for p in range(first, M):
                s = s + T[p] * v[p]
            return s

        for k in range(n):
            t, ak, bk, cs = point(k)
            L, D1, D2 = _legendre_p(t, M), _legendre_d1(t, M), _legendre_d2(t, M)
            Ly, D1y, D2y = dot(L, yh, 0), dot(D1, yh, 1), dot(D2, yh, 2)
            Lw, D1w, D2w = dot(L, w, 0), dot(D1, w, 1), dot(D2, w, 2)
            q = (cs * Ly - bk * D1y) - ak * D2y
            e = f[:, k] * inv_scl2 - ((cs * Lw - bk * D1w) - ak * D2w)
            t0 = t0 + cs * q
            t1 = t1 + (cs * t - bk) * q
            if drop_qw:
                D2w = D1w = Lw = np.zeros(ne)
            out["f"][:, k] = q * inv_scl2
            out["a"][:, k] = -(e * D2y - q * D2w)
            out["da"][:, k] = -((e * D1y - q * D1w) * hs)
            out["c"][:, k] = (e * Ly - q * Lw) * inv_scl2
        z0 = (wb[0] - eps * yh0) - t0
        z1 = (wb[1] - eps * yh1) - t1
        gl = (tb * z0 - z1) * idet
        gr = (z1 - ta * z0) * idet
        if status is not None:
            fb = np.asarray(status) == ST_FALLBACK
            gl = np.where(fb, 0.5 * (wb[0] - wb[1]), gl)
            gr = np.where(fb, 0.5 * (wb[0] + wb[1]), gr)
            for k in TABLES:
                out[k][fb] = 0.0
    out["pairs"] = np.stack([gl, gr], axis=1)
    return out


def replaced_ends(x, elem_offset=0, ne_global=None, global_domain=None):
    """(left, right): whether the forward call replaces the nodal value of the shard's first / last node by the Dirichlet
    value -- oracle/lssvr_oracle.py::boundary_values."""
    ne = len(x) - 1
    ne_global = ne if ne_global is None else ne_global
    gd = (x[0], x[-1]) if global_domain is None else global_domain
    return (elem_offset == 0 and x[0] == gd[0]), (elem_offset + ne == ne_global and x[-1] == gd[1])


def gather(pairs, left, right):
    """(gu [ne+1], gbc [2]): gu_i = gr(element i-1) + gl(element i), the left element's term first; a replaced end goes
    to gbc and leaves 0 in gu."""
    ne = len(pairs)
    gu = np.zeros(ne + 1)
    gu[0], gu[ne] = pairs[0, 0], pairs[ne - 1, 1]
    gu[1:ne] = pairs[:-1, 1] + pairs[1:, 0]
    gbc = np.zeros(2)
    if left:
        gbc[0], gu[0] = gu[0], 0.0
    if right:
        gbc[1], gu[ne] = gu[ne], 0.0
    return gu, gbc


def end_values(u, left, right, bc):
    """g [ne, 2] of the nodal values u with the replaced ends."""
    g = np.stack([u[:-1], u[1:]], axis=1).astype(np.result_type(u, np.asarray(bc)))
    if left:
        g[0, 0] = bc[0]
    if right:
        g[-1, 1] = bc[1]
    return g


def deviation(got, want):
    """The largest deviation over the groups of ``want``, each relative to its largest entry."""
    worst = 0.0
    for k, ref in want.items():
        scale = float(np.max(np.abs(ref)))
        err = float(np.max(np.abs(np.asarray(got[k]) - ref)))
        worst = max(worst, err / scale if scale > 0.0 else err)
    return worst


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def mesh(ne, seed=3):
    return p1.mesh(ne, seed)


def conv_b(x):
    return 0.4 + 0.2 * x


class Case:
    """``ne`` non-uniform elements on [-1, 1], degree M - 1, n points, with or without the a (and da = a' - b) and c
    tables: a = 1 + 0.3 sin 2x, c = 1.5 + cos 3x, random f, u and Wbar, gamma = 1e4; W is the forward restatement's."""

    def __init__(self, ne, M, n, has_a=True, has_c=True, gamma=1.0e4, x=None):
        self.ne, self.M, self.n, self.has_a, self.has_c, self.gamma = ne, M, n, has_a, has_c, gamma
        self.x = mesh(ne) if x is None else np.asarray(x, dtype=np.float64)
        xc = colloc_points(self.x, n)
        rng = np.random.default_rng(100000 * ne + 100 * M + n)
        self.f = rng.standard_normal((ne, n))
        self.u = rng.standard_normal(ne + 1)
        self.Wbar = rng.standard_normal((ne, M))
        self.bc = (0.3, -0.2)
        self.a = p1.coef_a(xc) if has_a else None
        self.da = p1.coef_da(xc) - conv_b(xc) if has_a else None
        self.c = p1.reaction(xc) if has_c else None
        self.g = end_values(self.u, True, True, self.bc)
        self.W = forward(self.x, self.g, M, n, gamma, self.f, self.a, self.da, self.c)

    @property
    def id(self):
        return f"ne{self.ne}-M{self.M}-n{self.n}-{'a' if self.has_a else ''}{'c' if self.has_c else ''}"

    def tables(self):
        return dict(f=self.f, a=self.a, da=self.da, c=self.c)

    def adjoint(self, **kw):
        return kernel_adjoint(self.x, self.M, self.n, self.gamma, self.f, self.W, self.Wbar, self.a, self.da, self.c, **kw)


def reading(case, **kw):
    """(the largest deviation of the adjoint from the complex step over the groups g, a, da, c, f, each relative to the
    largest entry of its group; the adjoint dict; the complex-step dict)."""
    adj = case.adjoint(**kw)
    adj["g"] = adj["pairs"]
    cs = complex_step(case.x, case.g, case.M, case.n, case.gamma, case.Wbar, case.f, case.a, case.da, case.c)
    return deviation(adj, cs), adj, cs


def negative_control(case):
    """The same comparison with the - q (. w) terms dropped: far above any bar."""
    return reading(case, drop_qw=True)[0]


# ---- the whole chain: tables -> P1 solve -> enhancement -> J(W) ---------------------------------------------------------------
def legendre_at(x, xo, M):
    """(e, P [len(xo), M]): the element of every point and L_p at its local coordinate."""
    e = np.clip(np.searchsorted(x, xo, side="right") - 1, 0, len(x) - 2)
    off, scl = (np.array(v) for v in zip(*(mapparms(x[i], x[i + 1]) for i in e)))
    return e, legendre_tables(off + scl * xo, M)[0]


class EnhancedGoal:
    """J(W) = int j u_enh dx by an nq-point Gauss rule per element (the facade: max(M, 8) points): linear, Wbar
    [ne, M] fixed."""

    def __init__(self, x, M, nq, density=p1.goal_density):
        xi, w = np.polynomial.legendre.leggauss(nq)
        h = np.diff(x)
        xq = 0.5 * (x[:-1] + x[1:])[:, None] + 0.5 * h[:, None] * xi[None, :]
        P = legendre_tables(np.tile(xi, len(h)), M)[0]
        jw = density(xq) * (0.5 * h[:, None] * w[None, :])
        self.Wbar = np.einsum("eq,eqm->em", jw, P.reshape(len(h), nq, M))

    def value(self, W):
        return np.sum(self.Wbar * W)

    def gradient(self, W):
        return self.Wbar


class EnhancedMisfit:
    """J(W) = 1/2 sum_i (u_enh(x_i) - d_i)^2."""

    def __init__(self, x, M, xo, d):
        self.e, self.P = legendre_at(x, np.asarray(xo, dtype=np.float64), M)
        self.d = np.asarray(d, dtype=np.float64)

    def residual(self, W):
        return np.sum(self.P * W[self.e], axis=1) - self.d

    def value(self, W):
        r = self.residual(W)
        return 0.5 * (r @ r)

    def gradient(self, W):
        out = np.zeros(W.shape)
        np.add.at(out, self.e, self.residual(W)[:, None] * self.P)
        return out


class Chain:
    """The facade's problem on the mesh x: quadrature tables ``qt`` (f, a, b, c at the Gauss points of the P1 assembly),
    collocation tables ``ct`` (f, a, da = a' - b, c at the collocation points), end kinds / kappa / end data of
    sensitivity_proto, and a functional J of W."""

    def __init__(self, x, nq, M, n, gamma, kinds, functional, conv=True, react=True, kappa=p1.KAPPA, g=p1.END_DATA):
        self.x, self.nq, self.M, self.n, self.gamma, self.kinds, self.kappa, self.g = x, nq, M, n, gamma, kinds, kappa, g
        self.conv, self.react = conv, react
        self.qt = p1.case_tables(x, nq, conv, react)
        xc = colloc_points(x, n)
        b = p1.convection(len(x) - 1)(xc) if conv else 0.0
        self.ct = dict(f=p1.rhs(xc), a=p1.coef_a(xc), da=p1.coef_da(xc) - b, c=p1.reaction(xc) if react else None)
        self.J = (EnhancedGoal(x, M, max(M, 8)) if functional == "goal" else
                  EnhancedMisfit(x, M, *p1.observations(x)))
        # the enhancement replaces a nodal value only at a Dirichlet end (the facade hands it the end value there)
        self.left, self.right = (k == p1.DIRICHLET for k in kinds)

    def W_of(self, qt, ct, kappa, g):
        u = p1.primal(self.x, qt, self.kinds, kappa, g)[0]
        return forward(self.x, end_values(u, self.left, self.right, g), self.M, self.n, self.gamma, ct["f"], ct["a"],
                       ct["da"], ct["c"]), u

    def adjoint(self):
        """dict(a, b, c, f [ne, nq]; ca, cda, cc, cf [ne, n]; ends [4]) by one enhancement adjoint and one P1 adjoint."""
        W, u = self.W_of(self.qt, self.ct, self.kappa, self.g)
        Wbar = self.J.gradient(W)
        adj = kernel_adjoint(self.x, self.M, self.n, self.gamma, self.ct["f"], W, Wbar, self.ct["a"], self.ct["da"],
                             self.ct["c"])
        gu, gbc = gather(adj["pairs"], self.left, self.right)
        _, K, bands = p1.primal(self.x, self.qt, self.kinds, self.kappa, self.g)
        z = p1.adjoint(K, gu, self.kinds, self.kappa)
        ga, gb, gc, gf = (t[0] for t in p1.table_gradients(self.x, u, z, self.nq))
        ends = p1.end_gradients(u, z, gu, (bands[1][0], bands[2][-1]), self.kinds)[0]
        ends[:2] += gbc
        out = dict(a=ga, b=gb, c=gc, f=gf, ends=ends, cf=adj["f"], ca=adj["a"], cda=adj["da"], cc=adj["c"])
        return {k: v for k, v in out.items() if self._has(k)}, self.J.value(W)

    def _has(self, k):
        return not ((k == "b" and not self.conv) or (k in ("c", "cc") and not self.react))

    def complex_step(self):
        out = {}
        full = p1._full(self.x, self.qt)
        for name in "abcf":
            if not self._has(name):
                continue
            grad = np.zeros(full[name].shape)
            for idx in np.ndindex(*grad.shape):
                t = {k: v.astype(complex) if k == name else v for k, v in full.items()}
                t[name][idx] += 1j * CSTEP
                grad[idx] = self.J.value(self.W_of(t, self.ct, self.kappa, self.g)[0]).imag / CSTEP
            out[name] = grad
        u = p1.primal(self.x, self.qt, self.kinds, self.kappa, self.g)[0]
        gend = end_values(u, self.left, self.right, self.g)
        cs = complex_step_J(self.x, gend, self.M, self.n, self.gamma, self.J, self.ct)
        out.update({"c" + k: v for k, v in cs.items() if k != "g"})
        ends = np.zeros(4)
        for s in range(2):
            gg = np.array(self.g, dtype=complex)
            gg[s] += 1j * CSTEP
            ends[s] = self.J.value(self.W_of(full, self.ct, self.kappa, gg)[0]).imag / CSTEP
            if self.kinds[s] == p1.ROBIN:
                kk = np.array(self.kappa, dtype=complex)
                kk[s] += 1j * CSTEP
                ends[2 + s] = self.J.value(self.W_of(full, self.ct, kk, self.g)[0]).imag / CSTEP
        out["ends"] = ends
        return out

    def reading(self):
        """(per-group deviations dict, adjoint dict, complex-step dict, value)."""
        adj, value = self.adjoint()
        cs = self.complex_step()
        dev = {k: deviation({k: adj[k]}, {k: cs[k]}) for k in cs}
        return dev, adj, cs, value


def complex_step_J(x, g, M, n, gamma, J, ct):
    """The complex step of a functional J(W) (not necessarily linear) with respect to the collocation tables."""
    data = dict(g=g, **ct)
    out = {}
    for name in TABLES:
        v = data[name]
        if v is None:
            continue
        grad = np.zeros(v.shape)
        for e in range(v.shape[0]):         # (a misfit couples the points of an element only: one element at a time)
            for k in range(v.shape[1]):
                t = dict(data)
                t[name] = v.astype(complex)
                t[name][e, k] += 1j * CSTEP
                sl = slice(e, e + 1)
                W = forward(x[e:e + 2], t["g"][sl], M, n, gamma, t["f"][sl],
                            None if t["a"] is None else t["a"][sl], None if t["da"] is None else t["da"][sl],
                            None if t["c"] is None else t["c"][sl])
                Wfull = np.array(J._W0, dtype=complex)
                Wfull[e] = W[0]
                grad[e, k] = J.value(Wfull).imag / CSTEP
        out[name] = grad
    return out


GROUP_SETS = dict(quadrature=("a", "b", "c", "f"), collocation=("ca", "cda", "cc", "cf"), ends=("ends",))


def chain_reading(chain):
    """(dict(quadrature=, collocation=, ends=) of the largest deviation in each set of groups, adjoint, complex step)."""
    W, _ = chain.W_of(chain.qt, chain.ct, chain.kappa, chain.g)
    chain.J._W0 = W
    dev, adj, cs, value = chain.reading()
    return {s: max(dev[k] for k in ks if k in dev) for s, ks in GROUP_SETS.items()}, adj, cs, value


PAIRS = ((3, 2), (4, 8), (9, 16), (16, 32))
SQUARE = (9, 7)
ISSUE_CASES = ((5, 8, 0.37), (9, 16, 0.11), (16, 14, 1.3))


def main():
    print("adjoint against the complex step, one uniform element of width h (all tables):")
    for M, n, h in ISSUE_CASES:
        c = Case(1, M, n, x=[-0.5 * h, 0.5 * h])
        print(f"  (M, n) = ({M}, {n}), h = {h}: reading {reading(c)[0]:.1e}   negative control {negative_control(c):.1e}")
    print("the cases of tests/enhance_adjoint_rules.py:")
    for ne in (1, 2, 7, 65, 300):
        for M, n in PAIRS + (SQUARE,):
            c = Case(ne, M, n)
            print(f"  {c.id}: reading {reading(c)[0]:.1e}   negative control {negative_control(c):.1e}")
    print("the whole chain on 33 elements (M = 9, n = 16, nquad = 2): quadrature / collocation / ends")
    for kinds in ((p1.DIRICHLET, p1.DIRICHLET), (p1.DIRICHLET, p1.ROBIN)):
        for fn in ("goal", "observe"):
            ch = Chain(mesh(33), 2, 9, 16, 1.0e4, kinds, fn)
            r = chain_reading(ch)[0]
            print(f"  {'DR'[kinds[0]]}{'DR'[kinds[1]]} {fn}: " + " / ".join(f"{r[s]:.1e}" for s in GROUP_SETS))


if __name__ == "__main__":
    main()
