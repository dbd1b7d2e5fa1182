"""numpy prototype of the bubble-condensed P1 assembly: the float64 / np.longdouble
restatement that the tests take their bars from.

    -(a u')' + b u' + c u = f,   element space  N_0 = 1 - t, N_1 = t, N_k = (P_k(s) - P_{k-2}(s)) / sqrt(2 (2k - 1)),
    s = 2t - 1, k = 2 .. p;  K_ij = sum_q w_q [a_q N_i' N_j' / h + b_q N_i N_j' + c_q h N_i N_j];  the bubble block is
    eliminated element by element and the condensed 2 x 2 matrices are assembled into (diag, sub, sup).

Every routine takes ``dtype``: np.float64 (the prototype) or np.longdouble (its own reference).  The inputs -- mesh,
tables, the points and weights of the rule -- are float64 numbers in both, so the two runs solve the same discrete
problem and differ by rounding alone.  The sums run in the order of csrc/p1_bubble.hip; nothing here is needed to be
bit-equal to it.  Run as a script it prints the convergence table of section 37.
"""
import numpy as np

# Gauss-Legendre on [0,1], the digits of csrc/lssvr_p1.hpp (quad_rule)
_RULES = {
    1: (["0.5"], ["1.0"]),
    2: (["0.21132486540518711775", "0.78867513459481288225"], ["0.5", "0.5"]),
    3: (["0.11270166537925831148", "0.5", "0.88729833462074168852"],
        ["0.27777777777777777778", "0.44444444444444444444", "0.27777777777777777778"]),
    4: (["0.069431844202973712388", "0.33000947820757186760", "0.66999052179242813240", "0.93056815579702628761"],
        ["0.17392742256872692869", "0.32607257743127307131", "0.32607257743127307131", "0.17392742256872692869"]),
    5: (["0.046910077030668003601", "0.23076534494715845448", "0.5", "0.76923465505284154552",
         "0.95308992296933199640"],
        ["0.11846344252809454376", "0.23931433524968323402", "0.28444444444444444444", "0.23931433524968323402",
         "0.11846344252809454376"]),
}


def rule(nquad):
    """(t_q, w_q) on [0,1] as float64 -- the numbers the library holds."""
    t, w = _RULES[int(nquad)]
    return np.array([float(v) for v in t]), np.array([float(v) for v in w])


def quad_points(x, nquad):
    """x_e + h_e t_q, [ne, nquad] (float64, as lssvr_quad_points)."""
    x = np.asarray(x, dtype=np.float64)
    return x[:-1, None] + np.diff(x)[:, None] * rule(nquad)[0][None, :]


def shapes(p, t, dtype=np.float64):
    """(N [p+1, nq], D = dN/dt [p+1, nq]) at the points t; d/ds (P_k - P_{k-2}) = (2k - 1) P_{k-1}."""
    t = np.asarray(t, dtype=dtype)
    s = 2 * t - 1
    P = [np.ones_like(s), s]
    for m in range(2, p + 1):
        P.append(((2 * m - 1) * s * P[m - 1] - (m - 1) * P[m - 2]) / m)
    N, D = [1 - t, t], [-np.ones_like(t), np.ones_like(t)]
    for m in range(2, p + 1):
        sc = np.sqrt(dtype(2 * (2 * m - 1)))
        N.append((P[m] - P[m - 2]) / sc)
        D.append(sc * P[m - 1])
    return np.array(N, dtype=dtype), np.array(D, dtype=dtype)


def condense(p, nquad, h, fq, aq=None, cq=None, bq=None, dtype=np.float64):
    """The condensed element quantities of every element at once: (S [ne, 4] = S00, S01, S10, S11, g [R, ne, 2]).
    h [ne]; fq [R, ne, nquad]; aq, cq, bq [ne, nquad] or None (a = 1, c = 0, b = 0).  p = 1: no bubbles, S = K."""
    t, w = rule(nquad)
    N, D = shapes(p, t, dtype)
    w = w.astype(dtype)
    h = np.asarray(h, dtype=dtype)
    fq = np.asarray(fq, dtype=dtype)
    ne, n, nb = h.size, p + 1, p - 1
    wa = np.broadcast_to(w, (ne, nquad)) if aq is None else w * np.asarray(aq, dtype=dtype)
    wb = None if bq is None else w * np.asarray(bq, dtype=dtype)
    wc = None if cq is None else w * np.asarray(cq, dtype=dtype)
    K = np.zeros((n, n, ne), dtype=dtype)
    for i in range(n):
        for j in range(i, n):
            A = np.zeros(ne, dtype=dtype)
            C = np.zeros(ne, dtype=dtype)
            for q in range(nquad):
                A = A + (wa[:, q] * D[i, q]) * D[j, q]
                if wc is not None:
                    C = C + (wc[:, q] * N[i, q]) * N[j, q]
            K[i, j] = A / h + h * C
            K[j, i] = K[i, j]
    if wb is not None:
        for i in range(n):
            for j in range(n):
                B = np.zeros(ne, dtype=dtype)
                for q in range(nquad):
                    B = B + (wb[:, q] * N[i, q]) * D[j, q]
                K[i, j] = K[i, j] + B
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(nb):                      # K_bb = L U, no pivoting
            for i in range(k + 1, nb):
                l = K[2 + i, 2 + k] / K[2 + k, 2 + k]
                K[2 + i, 2 + k] = l
                for j in range(k + 1, nb):
                    K[2 + i, 2 + j] = K[2 + i, 2 + j] - l * K[2 + k, 2 + j]
        Z = np.zeros((2, max(nb, 1), ne), dtype=dtype)
        for v in range(2):                       # Z K_bb = K_vb
            for j in range(nb):
                s = K[v, 2 + j].copy()
                for k in range(j):
                    s = s - Z[v, k] * K[2 + k, 2 + j]
                Z[v, j] = s / K[2 + j, 2 + j]
            for j in range(nb - 2, -1, -1):
                s = Z[v, j].copy()
                for k in range(j + 1, nb):
                    s = s - Z[v, k] * K[2 + k, 2 + j]
                Z[v, j] = s
        S = np.zeros((ne, 4), dtype=dtype)
        for v in range(2):
            for c2 in range(2):
                s = K[v, c2].copy()
                for j in range(nb):
                    s = s - Z[v, j] * K[2 + j, c2]
                S[:, 2 * v + c2] = s
        R = fq.shape[0]
        g = np.zeros((R, ne, 2), dtype=dtype)
        for r in range(R):
            fw = w * fq[r]
            gi = []
            for i in range(n):
                s = np.zeros(ne, dtype=dtype)
                for q in range(nquad):
                    s = s + N[i, q] * fw[:, q]
                gi.append(h * s)
            for v in range(2):
                s = gi[v].copy()
                for j in range(nb):
                    s = s - Z[v, j] * gi[2 + j]
                g[r, :, v] = s
    return S, g


def assemble(x, p, nquad, fq, aq=None, cq=None, bq=None, dtype=np.float64):
    """dict(diag [ne+1], sub [ne], sup [ne], load [R, ne+1], kloc4 [ne, 4], floc [R, ne, 2]) in ``dtype``; fq
    [R, ne, nquad] or [ne, nquad] (then R = 1 and load, floc keep the leading axis)."""
    x = np.asarray(x, dtype=np.float64)
    fq = np.asarray(fq, dtype=np.float64)
    if fq.ndim == 2:
        fq = fq[None]
    h = np.diff(x.astype(dtype))
    S, g = condense(p, nquad, h, fq, aq, cq, bq, dtype)
    ne = h.size
    diag = np.zeros(ne + 1, dtype=dtype)
    diag[1:] = S[:, 3]
    diag[1:-1] = S[:-1, 3] + S[1:, 0]
    diag[0] = S[0, 0]
    load = np.zeros((fq.shape[0], ne + 1), dtype=dtype)
    load[:, 1:] = g[:, :, 1]
    load[:, 1:-1] = g[:, :-1, 1] + g[:, 1:, 0]
    load[:, 0] = g[:, 0, 0]
    return dict(diag=diag, sub=S[:, 2].copy(), sup=S[:, 1].copy(), load=load, kloc4=S, floc=g)


def matrix(diag, sub, sup, load, ends=(0.0, 0.0), free=(False, False), kappa=(0.0, 0.0), periodic=False,
           dtype=np.float64):
    """(A, rhs) of the nodal system the tridiagonal solves stand for: Dirichlet ends are identity rows with the value
    ``ends[i]``; a ``free`` end keeps its row, kappa on the diagonal and g = ends[i] on the right; ``periodic``: node
    ne is node 0 (n = ne unknowns, rows 0 and ne added)."""
    d, lo, up, b = (np.asarray(v, dtype=dtype) for v in (diag, sub, sup, load))
    ne = lo.size
    A = np.zeros((ne + 1, ne + 1), dtype=dtype)
    A[np.arange(ne + 1), np.arange(ne + 1)] = d
    A[np.arange(1, ne + 1), np.arange(ne)] = lo
    A[np.arange(ne), np.arange(1, ne + 1)] = up
    b = b.copy()
    if periodic:
        A[0] += A[ne]
        A[:, 0] += A[:, ne]
        b[0] += b[ne]
        return A[:ne, :ne].copy(), b[:ne].copy()
    for i, f, k, g in ((0, free[0], kappa[0], ends[0]), (ne, free[1], kappa[1], ends[1])):
        if f:
            A[i, i] += dtype(k)
            b[i] += dtype(g)
        else:
            A[i] = 0
            A[i, i] = 1
            b[i] = dtype(g)
    return A, b


def dense_solve(A, b, dtype=np.float64):
    """Gaussian elimination with partial pivoting in ``dtype`` (LAPACK has no np.longdouble)."""
    if dtype == np.float64:
        return np.linalg.solve(A, b)
    A, b = A.astype(dtype).copy(), b.astype(dtype).copy()
    n = b.size
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        l = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= l[:, None] * A[k, k:][None, :]
        b[k + 1:] -= l * b[k]
    u = np.zeros(n, dtype=dtype)
    for k in range(n - 1, -1, -1):
        u[k] = (b[k] - A[k, k + 1:] @ u[k + 1:]) / A[k, k]
    return u


def solve_bands(diag, sub, sup, load, ends=(0.0, 0.0), free=(False, False), kappa=(0.0, 0.0), periodic=False,
                dtype=np.float64):
    """Nodal values [ne+1] of one load on the given bands (periodic: u[ne] = u[0])."""
    A, b = matrix(diag, sub, sup, load, ends, free, kappa, periodic, dtype)
    u = dense_solve(A, b, dtype)
    return np.append(u, u[0]) if periodic else u


def dominance(diag, sub, sup, free=(False, False), kappa=(0.0, 0.0), periodic=False):
    """(worst row, its margin diag - |sub[i-1]| - |sup[i]|) over the rows of the system (Dirichlet end rows are not
    rows of it): the hypothesis of the unpivoted solve holds when the margin is >= 0."""
    d = np.array(diag, dtype=np.float64)
    ne = d.size - 1
    d[1:] -= np.abs(sub)
    d[:-1] -= np.abs(sup)
    if periodic:
        d[0] = d[ne] = d[0] + d[ne]
    else:
        for i, f, k in ((0, free[0], kappa[0]), (ne, free[1], kappa[1])):
            d[i] = d[i] + k if f else np.inf
    d = np.where(np.isfinite(d) | (d == np.inf), d, -np.inf)
    row = int(np.argmin(d))
    return row, float(d[row])


# ---- the problem of the accuracy record ---------------------------------------------------------------------------
def a_fn(x):
    return 1 + 0.5 * x


def da_fn(x):
    return 0.5 + 0 * x


def b_fn(x):
    return 3 + x


def c_fn(x):
    return 2 + np.cos(x)


def u_fn(x):
    return np.sin(3 * x) + x * x


def f_fn(x):
    du, ddu = 3 * np.cos(3 * x) + 2 * x, -9 * np.sin(3 * x) + 2
    return -(da_fn(x) * du + a_fn(x) * ddu) + b_fn(x) * du + c_fn(x) * u_fn(x)


def graded_mesh(ne):
    return np.linspace(0.0, 1.0, ne + 1) ** 1.3


def solve_problem(ne, p, nquad=None, dtype=np.float64):
    """(x, U) of the record's problem on graded_mesh(ne) with Dirichlet ends u(0), u(1)."""
    nquad = p + 1 if nquad is None else nquad
    x = graded_mesh(ne)
    xq = quad_points(x, nquad)
    s = assemble(x, p, nquad, f_fn(xq), a_fn(xq), c_fn(xq), b_fn(xq), dtype)
    return x, solve_bands(s["diag"], s["sub"], s["sup"], s["load"][0], (u_fn(0.0), u_fn(1.0)), dtype=dtype)


def nodal_error(ne, p, nquad=None):
    x, U = solve_problem(ne, p, nquad)
    return float(np.max(np.abs(U - u_fn(x))))


if __name__ == "__main__":
    for p in (1, 2, 3, 4):
        errs = [nodal_error(ne, p) for ne in (4, 8, 16, 32)]
        print(p, " ".join(f"{e:.2e}" for e in errs), " ".join(f"{np.log2(errs[i] / errs[i + 1]):.2f}" for i in range(3)))
