"""Test infrastructure: float64 numpy restatements of the point-cloud preparation passes (cn_knn_query in
csrc/cn_mesh_eval.hip, csrc/cn_cloud.hip) -- brute-force k nearest neighbours under the (distance, index) order,
the voxel means from fp32-computed keys and sequential float64 sums, PCA normals through numpy.linalg.eigh, and
the statistical outlier rule -- and the clouds the tests share."""
import numpy as np

KEY_NONE = (1 << 63) - 1


def brute_knn(queries, targets, ranks, exclude_self=False):
    """(dist [Q, ranks], index [Q, ranks]) in float64 from the fp32 coordinates: the first `ranks` targets of every
    query under the total order (distance, index) -- a stable sort of the distances, so equal distances keep
    ascending index.  Ranks past the number of targets are (inf, -1).  exclude_self drops target i for query i."""
    q = np.asarray(queries, dtype=np.float64)
    t = np.asarray(targets, dtype=np.float64)
    d2 = ((q[:, None, :] - t[None, :, :]) ** 2)
    d2 = (d2[:, :, 0] + d2[:, :, 1]) + d2[:, :, 2]
    if exclude_self:
        assert len(q) == len(t)
        d2[np.arange(len(q)), np.arange(len(q))] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")[:, :ranks]
    d = np.sqrt(np.take_along_axis(d2, order, axis=1))
    dist = np.full((len(q), ranks), np.inf)
    index = np.full((len(q), ranks), -1, dtype=np.int64)
    n = order.shape[1]
    dist[:, :n] = d
    index[:, :n] = np.where(np.isfinite(d), order, -1)
    return dist, index


def voxel_keys_ref(points, origin, voxel):
    """cn_voxel_keys with its fp32 arithmetic: int64 keys, KEY_NONE for a point that is not finite or outside the
    21-bit range on some axis."""
    p = np.asarray(points, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        f = (p - np.asarray(origin, dtype=np.float32)) / np.float32(voxel)
        ok = np.all((f >= 0) & (f < np.float32(2097152.0)), axis=1)
    i = np.where(ok[:, None], np.floor(np.where(ok[:, None], f, 0)), 0).astype(np.int64)
    return np.where(ok, (i[:, 0] << 42) | (i[:, 1] << 21) | i[:, 2], KEY_NONE)


def voxel_ref(points, origin, voxel, normals=None, colors=None):
    """The voxel means: a dict with keys (ascending), counts, points / colors (float64 sums taken sequentially in
    ascending original index, divided by the count), normals (the float64 sum over its length, zero for a zero
    sum) and n_dropped."""
    keys = voxel_keys_ref(points, origin, voxel)
    ok = keys != KEY_NONE
    uniq, inv = np.unique(keys[ok], return_inverse=True)
    counts = np.bincount(inv, minlength=len(uniq))

    def sums(x):
        s = np.zeros((len(uniq), 3))
        np.add.at(s, inv, np.asarray(x, dtype=np.float32).astype(np.float64)[ok])  # unbuffered: in index order
        return s
    out = {"keys": uniq, "counts": counts, "points": sums(points) / counts[:, None], "normals": None, "colors": None,
           "n_dropped": int((~ok).sum())}
    if colors is not None:
        out["colors"] = sums(colors) / counts[:, None]
    if normals is not None:
        s = sums(normals)
        length = np.sqrt((s[:, 0] ** 2 + s[:, 1] ** 2) + s[:, 2] ** 2)
        out["normals"] = np.where(length[:, None] > 0, s / np.where(length > 0, length, 1.0)[:, None], 0.0)
    return out


def normals_ref(points, index):
    """PCA normals from neighbour rows index [N, k] (entries outside [0, N) skipped): (normals [N, 3] float64, the
    eigenvector of the smallest eigenvalue of the neighbours' covariance by eigh, sign as eigh leaves it; eig
    [N, 3] ascending; valid [N] bool, False -- and a zero normal -- for fewer than 3 neighbours, non-finite input or
    l1 <= 1e-12 l2)."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    N = len(p)
    normals, eig, valid = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N, dtype=bool)
    for i, row in enumerate(np.asarray(index)):
        nb = p[row[(row >= 0) & (row < N)]]
        if len(nb) < 3 or not np.all(np.isfinite(nb)) or not np.all(np.isfinite(p[i])):
            continue
        d = nb - nb.mean(0)
        w, v = np.linalg.eigh(d.T @ d / len(nb))
        eig[i] = w
        if w[1] > 1e-12 * w[2]:
            normals[i], valid[i] = v[:, 0], True
    return normals, eig, valid


def angle(a, b):
    """The sign-free angle between unit vectors, by atan2 of |a x b| and |a . b| (accurate near zero)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs(np.sum(a * b, axis=-1)))


def knn_means_ref(dist, index):
    """Per row the float64 mean of the distances whose index is not -1, in row order (inf for a row without one)."""
    d, ok = np.asarray(dist, dtype=np.float64), np.asarray(index) >= 0
    out = np.full(len(d), np.inf)
    for i in range(len(d)):
        if ok[i].any():
            s = 0.0
            for x in d[i][ok[i]]:
                s += x
            out[i] = s / ok[i].sum()
    return out


def outlier_ref(means, std_ratio):
    """(mu, sigma, cut, keep) of the statistical outlier rule over the finite means: keep where mean <= mu +
    std_ratio sigma, sigma the population standard deviation."""
    m = np.asarray(means, dtype=np.float64)
    f = m[np.isfinite(m)]
    mu = f.mean()
    sigma = np.sqrt(np.mean((f - mu) ** 2))
    cut = mu + std_ratio * sigma
    return mu, sigma, cut, m <= cut


def ellipsoid(n, seed, radii=(0.5, 0.4, 0.3)):
    """(points fp32 [n, 3] on the ellipsoid with those semi-axes, its analytic unit normals at them float64)."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = np.asarray(radii)
    p = (u * r).astype(np.float32)
    g = p.astype(np.float64) / r ** 2
    return p, g / np.linalg.norm(g, axis=1, keepdims=True)
