"""numpy restatement of the rules of the three hp kernels (include/lssvr_hip.h: lssvr_smoothness, lssvr_refine_hp,
lssvr_group_by_degree), statement by statement from their contracts.  A plain module: the CPU tests pin it to
hand-computed cases, the GPU tests compare the kernels with it, scripts/proto/hp_adapt.py runs its loop on it."""
import numpy as np


def smoothness(W, deg):
    """sigma[e]: minus the least-squares slope of ln env_p against p over the kept points of row e."""
    W = np.asarray(W, dtype=np.float64)
    out = np.empty(W.shape[0])
    for e, M in enumerate(np.asarray(deg)):
        M = int(M)
        if not 2 <= M <= W.shape[1]:
            out[e] = np.nan
            continue
        c = np.abs(W[e, :M])
        if not np.all(np.isfinite(c)):
            out[e] = np.nan
            continue
        mx = c.max()
        if mx == 0.0 or M < 3:
            out[e] = np.inf
            continue
        env = np.maximum.accumulate(c[:0:-1])[::-1]            # env[p-1] = max_{p <= q < M} c_q, p = 1 .. M-1
        p = np.arange(1, M, dtype=np.float64)
        keep = (env >= mx * 2.0 ** -52) & (env > 0.0)
        if keep.sum() < 2:
            out[e] = np.inf
            continue
        p, y = p[keep], np.log(env[keep])
        dp = p - p.mean()
        out[e] = -np.sum(dp * (y - y.mean())) / np.sum(dp * dp)
    return out


def marked(eta2, mx, theta):
    """lssvr_refine's predicate without the length condition."""
    eta2 = np.asarray(eta2, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(eta2) | ((mx > 0) & (eta2 >= (theta * theta) * mx))


def actions(x, eta2, mx, theta, h_min, sigma, deg, sigma_min, dM, M_max):
    """(raise[ne], split[ne]) of lssvr_refine_hp: a marked element is raised iff sigma >= sigma_min and deg + dM <=
    M_max (NaN compares false), otherwise bisected iff it is at least 2 h_min long, otherwise left."""
    x = np.asarray(x, dtype=np.float64)
    deg = np.asarray(deg, dtype=np.int64)
    m = marked(eta2, mx, theta)
    with np.errstate(invalid="ignore"):
        smooth = np.asarray(sigma, dtype=np.float64) >= sigma_min
    up = m & smooth & (deg + dM <= M_max)
    split = m & ~up & ((x[1:] - x[:-1]) >= 2.0 * h_min)
    return up, split


def refine_hp(x, eta2, mx, theta, h_min, sigma, deg, sigma_min, dM, M_max):
    """(x_new[ne_new+1], deg_new[ne_new] int32, parent[ne_new] int64, (bisected, raised))."""
    x = np.asarray(x, dtype=np.float64)
    deg = np.asarray(deg, dtype=np.int32)
    up, split = actions(x, eta2, mx, theta, h_min, sigma, deg, sigma_min, dM, M_max)
    ne = deg.size
    counts = 1 + split.astype(np.int64)
    pos = np.concatenate([[0], np.cumsum(counts)[:-1]])
    x_new = np.empty(ne + int(split.sum()) + 1)
    x_new[pos] = x[:-1]
    x_new[pos[split] + 1] = 0.5 * (x[:-1][split] + x[1:][split])
    x_new[-1] = x[-1]
    parent = np.repeat(np.arange(ne, dtype=np.int64), counts)
    deg_new = np.repeat(np.where(up, deg + np.int32(dM), deg).astype(np.int32), counts)
    return x_new, deg_new, parent, (int(split.sum()), int(up.sum()))


def group_by_degree(deg):
    """(ids[number of valid degrees] int64, offsets[35] int64): a stable sort of the elements with 2 <= deg <= 33
    by degree; the elements of degree M are ids[offsets[M]:offsets[M+1]]."""
    deg = np.asarray(deg, dtype=np.int64)
    valid = np.nonzero((deg >= 2) & (deg <= 33))[0]
    ids = valid[np.argsort(deg[valid], kind="stable")].astype(np.int64)
    offsets = np.searchsorted(deg[ids], np.arange(35), side="left").astype(np.int64)
    return ids, offsets


def n_colloc(n_base, M):
    """Collocation points of a degree-M group of the facade: max(n_colloc, 2 M)."""
    return max(int(n_base), 2 * int(M))
