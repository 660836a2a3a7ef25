"""Float64 numpy restatement of the ICP registration (copenerf.metrics.icp_register and the kernels under it):
brute-force nearest neighbours in row chunks, the 32 sums of cn_icp_accumulate with their slot layout, the two
closed-form solvers and the loop with its stopping rule.  The yardstick of tests/test_gpu_icp*.py and
tests/test_icp_host.py; numpy only."""
import math

import numpy as np

SUMS = 32


def rotation(axis, degrees):
    """Rodrigues' rotation about `axis` by `degrees`."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(degrees)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def similarity(R, t, s=1.0):
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * np.asarray(R, dtype=np.float64), t
    return M


def apply(T, p):
    return np.asarray(p, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]


def transform_terms(T32, p):
    """For the fp32 matrix T32 [3, 4] and fp32 points p [n, 3]: (the exact float64 value of t + a x + b y + c z,
    max(|t|, |a x|, |b y|, |c z|)) per component -- what cn_cloud_transform's three fmafs are measured against."""
    M, p = np.asarray(T32, dtype=np.float64), np.asarray(p, dtype=np.float64)
    terms = np.concatenate([M[None, :, :3] * p[:, None, :], np.broadcast_to(M[None, :, 3:], (len(p), 3, 1))], axis=2)
    return terms.sum(2), np.abs(terms).max(2)


def nearest(queries, targets, max_dist=np.inf, chunk=1024):
    """(index int64 [Q], dist float64 [Q]): the nearest target of every query by brute force in float64, -1 where
    none is nearer than max_dist.  Every query is compared with every target through |q|^2 + |t|^2 - 2 q . t (one
    matrix product per chunk of rows, about the centroid of the targets); that form loses 1e-16 |x|^2 to
    cancellation, which can only exchange two targets whose squared distances agree that closely, and the distance
    returned is computed directly from the chosen pair."""
    q, t = np.asarray(queries, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    index, dist = np.full(len(q), -1, dtype=np.int64), np.full(len(q), np.inf)
    if len(t) == 0:
        return index, dist
    mid = t.mean(0)
    tc = t - mid
    t2 = (tc * tc).sum(1)
    for i in range(0, len(q), chunk):
        qc = q[i:i + chunk] - mid
        j = ((qc * qc).sum(1)[:, None] + t2[None] - 2.0 * (qc @ tc.T)).argmin(1)
        d = np.sqrt(((q[i:i + chunk] - t[j]) ** 2).sum(1))
        index[i:i + chunk] = np.where(d < max_dist, j, -1)
        dist[i:i + chunk] = d
    return index, dist


def unit_normals32(n):
    """(unit normals fp32 [N, 3], usable [N]) exactly as the kernels normalise: fp32, |v| = sqrt((x x + y y) + z z)."""
    n = np.asarray(n, dtype=np.float32)
    with np.errstate(all="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = (length > 0) & (length < np.inf)
        u = n / np.where(ok, length, np.float32(1))[:, None]
    return u, ok


def sums(moved, targets, index, pivot, mode, normals=None):
    """(sums [32], the sums of the terms' absolute values [32]) in cn_icp_accumulate's layout, from the transformed
    source `moved` [Q, 3], targets [N, 3], index [Q] (negative or >= N: no pair) and, mode 1, raw target normals."""
    out, mag = np.zeros(SUMS), np.zeros(SUMS)
    index = np.asarray(index, dtype=np.int64)
    N = len(targets)
    use = (index >= 0) & (index < N)
    left = 0
    if mode == 1:
        u, ok = unit_normals32(normals)
        bad = use & ~ok[np.clip(index, 0, max(N - 1, 0))] if N else use
        left = int(bad.sum())
        use = use & ~bad
    if not use.any():
        out[30] = left if mode == 1 else 0
        mag[30] = out[30]
        return out, mag
    c = np.asarray(pivot, dtype=np.float64)
    P, Qt = np.asarray(moved, dtype=np.float64)[use], np.asarray(targets, dtype=np.float64)[index[use]]
    e, p, q = P - Qt, P - c, Qt - c
    cols = [np.ones(len(P)), (e * e).sum(1)]
    if mode == 0:
        cols += [p[:, 0], p[:, 1], p[:, 2], q[:, 0], q[:, 1], q[:, 2]]
        cols += [q[:, a] * p[:, b] for a in range(3) for b in range(3)]
        cols += [(p * p).sum(1)]
    else:
        n = u[index[use]].astype(np.float64)
        J = np.concatenate([np.cross(p, n), n], axis=1)
        r = (e * n).sum(1)
        cols += [r * r]
        cols += [J[:, a] * J[:, b] for a in range(6) for b in range(a, 6)]
        cols += [J[:, a] * r for a in range(6)]
    for k, col in enumerate(cols):
        out[k], mag[k] = math.fsum(col), math.fsum(np.abs(col))
    if mode == 1:
        out[30] = mag[30] = left
    return out, mag


def solve_point(s, with_scale=False, pivot=(0.0, 0.0, 0.0)):
    c = np.asarray(pivot, dtype=np.float64)
    n = s[0]
    mp, mq = s[2:5] / n, s[5:8] / n
    C = s[8:17].reshape(3, 3) / n - np.outer(mq, mp)
    var = s[17] / n - mp @ mp
    U, D, Vt = np.linalg.svd(C)
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ S @ Vt
    scale = (D * np.diag(S)).sum() / var if with_scale else 1.0
    return similarity(R, (mq + c) - scale * (R @ (mp + c)), scale)


def solve_plane(s, pivot=(0.0, 0.0, 0.0)):
    c = np.asarray(pivot, dtype=np.float64)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[3:24]
    A = A + np.triu(A, 1).T
    x = -np.linalg.solve(A, s[24:30])
    th = np.linalg.norm(x[:3])
    R = rotation(x[:3], math.degrees(th)) if th > 0 else np.eye(3)
    return similarity(R, c - R @ c + x[3:])


def register(source, target, max_corr_dist, init=None, mode="point", with_scale=False, target_normals=None,
             max_iters=50, tol=1e-6, fp32_transform=False):
    """The loop of metrics.icp_register in float64: dict(transform, fitness, inlier_rmse, iterations, converged,
    history).  fp32_transform rounds the matrix applied to the points to fp32, as the device's is."""
    src, tgt = np.asarray(source, dtype=np.float64), np.asarray(target, dtype=np.float64)
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    pivot = 0.5 * (tgt.min(0) + tgt.max(0))
    m = {"point": 0, "plane": 1}[mode]
    history, converged, iterations = [], False, 0
    while True:
        moved = apply(T.astype(np.float32).astype(np.float64) if fp32_transform else T, src)
        index, _ = nearest(moved, tgt, max_corr_dist)
        s, _ = sums(moved, tgt, index, pivot, m, target_normals)
        fitness, rmse = s[0] / len(src), math.sqrt(s[1] / s[0]) if s[0] else float("nan")
        history.append((fitness, rmse))
        if len(history) > 1 and abs(fitness - history[-2][0]) < tol and abs(rmse - history[-2][1]) < tol:
            converged = True
        if converged or iterations == max_iters:
            break
        T = (solve_point(s, with_scale, pivot) if m == 0 else solve_plane(s, pivot)) @ T
        iterations += 1
    return dict(transform=T, fitness=fitness, inlier_rmse=rmse, iterations=iterations, converged=converged,
                history=history)


def bumpy_field(x, axes=(0.9, 0.6, 0.4)):
    """F of bumpy_ellipsoid at points x [..., 3]: negative inside the surface."""
    x = np.asarray(x, dtype=np.float64)
    a = np.asarray(axes, dtype=np.float64)
    return (((x / a) ** 2).sum(-1) - 1.0
            - 0.08 * np.sin(3 * x[..., 0] + 0.5) * np.sin(2 * x[..., 1] - 0.3) * np.cos(2.5 * x[..., 2] + 0.2))


def bumpy_ellipsoid(n, seed, axes=(0.9, 0.6, 0.4)):
    """(points [n, 3], outward unit normals [n, 3]) in float64 on the asymmetric surface
    F(x) = (x / a)^2 + (y / b)^2 + (z / c)^2 - 1 - 0.08 sin(3 x + 0.5) sin(2 y - 0.3) cos(2.5 z + 0.2) = 0,
    each point found along a random ray from the origin by bisection (F < 0 at the origin, > 0 at radius 1.2, and
    rising along every ray there: the bump's slope is below the quadric's), the normal its gradient."""
    a = np.asarray(axes, dtype=np.float64)
    d = np.random.default_rng(seed).standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)

    def F(x):
        return bumpy_field(x, axes)

    lo, hi = np.zeros(n), np.full(n, 1.2)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        inside = F(d * mid[:, None]) < 0
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    x = d * (0.5 * (lo + hi))[:, None]
    sx, cx = np.sin(3 * x[:, 0] + 0.5), np.cos(3 * x[:, 0] + 0.5)
    sy, cy = np.sin(2 * x[:, 1] - 0.3), np.cos(2 * x[:, 1] - 0.3)
    sz, cz = np.sin(2.5 * x[:, 2] + 0.2), np.cos(2.5 * x[:, 2] + 0.2)
    g = 2 * x / a ** 2 - 0.08 * np.stack([3 * cx * sy * cz, 2 * sx * cy * cz, -2.5 * sx * sy * sz], axis=1)
    return x, g / np.linalg.norm(g, axis=1, keepdims=True)
