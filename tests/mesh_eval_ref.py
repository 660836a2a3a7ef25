"""Test infrastructure: float64 numpy restatements of the mesh geometry metrics' device passes
(csrc/cn_mesh_eval.hip) -- chunked brute-force nearest neighbour, the area-weighted surface sampler from
philox_ref's uniforms, the cloud statistics and the metric dictionary -- and the meshes the tests share."""
import numpy as np

from philox_ref import uniform

EPS32 = 2.0 ** -24


def dist_bar(d64):
    """The distance bound of cn_nn_query against float64: three fp32 subtractions, three squares, two adds and a
    square root, each within 2^-24 relative: 8 x 2^-24 relative (and a floor for exact zeros)."""
    return 8.0 * EPS32 * d64 + 1e-30


def brute_nn(queries, targets, chunk=32):
    """(dist [Q], index [Q], second [Q]) in float64 from the fp32 coordinates: the distance to and the index of
    the nearest target (the first index among equal distances), and the smallest distance that is strictly
    larger than the nearest one (inf when there is none) -- the gap a test asserts before it compares indices.
    All pairs, a few query rows at a time in buffers that stay in the cache."""
    q = np.asarray(queries, dtype=np.float64)
    t = np.ascontiguousarray(np.asarray(targets, dtype=np.float64).T)
    dist, index, second = np.empty(len(q)), np.empty(len(q), dtype=np.int64), np.empty(len(q))
    d2, buf = np.empty((chunk, t.shape[1])), np.empty((chunk, t.shape[1]))
    for s in range(0, len(q), chunk):
        c = q[s:s + chunk]
        n = len(c)
        a, b = d2[:n], buf[:n]
        np.subtract(c[:, 0:1], t[0], out=a)
        np.multiply(a, a, out=a)
        for ax in (1, 2):
            np.subtract(c[:, ax:ax + 1], t[ax], out=b)
            np.multiply(b, b, out=b)
            np.add(a, b, out=a)
        i = a.argmin(1)
        best = a[np.arange(n), i]
        a[a <= best[:, None]] = np.inf
        dist[s:s + n], index[s:s + n], second[s:s + n] = np.sqrt(best), i, np.sqrt(a.min(1))
    return dist, index, second


def tri_areas(vertices, triangles):
    """Triangle areas in float64 from the fp32 vertices, in the kernel's order of operations."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    a, b, c = (v[np.asarray(triangles)[:, k]] for k in range(3))
    u, w = b - a, c - a
    cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def sample_ref(vertices, triangles, S, seed, offset=0):
    """The sampler in float64: a dict with the uniforms u [S, 3] (elements 4 i .. 4 i + 2 of cn_uniform_philox's
    stream), areas, cdf, area, tri [S] (the first t with cdf[t] > u0 area), margin [S] (how far u0 area is from
    the nearest cdf entry, relative to the area) and points [S, 3] (the barycentric expression in float64)."""
    u = uniform(4 * S, seed, offset).reshape(S, 4)[:, :3]
    areas = tri_areas(vertices, triangles)
    cdf = np.cumsum(areas)
    area = cdf[-1]
    x = u[:, 0].astype(np.float64) * area
    tri = np.searchsorted(cdf, x, side="right")
    edges = np.concatenate([[0.0], cdf])
    margin = np.minimum(x - edges[tri], edges[tri + 1] - x) / area  # (cdf[tri - 1] <= x < cdf[tri])
    return {"u": u, "areas": areas, "cdf": cdf, "area": area, "tri": tri, "margin": margin,
            "points": bary_points(vertices, triangles, tri, u)}


def bary_points(vertices, triangles, tri, u):
    """(1 - sqrt(u1)) a + sqrt(u1) (1 - u2) b + sqrt(u1) u2 c in float64 for the given triangles."""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles)[np.asarray(tri)]
    r = np.sqrt(u[:, 1].astype(np.float64))[:, None]
    u2 = u[:, 2].astype(np.float64)[:, None]
    return (1 - r) * v[t[:, 0]] + r * (1 - u2) * v[t[:, 1]] + r * u2 * v[t[:, 2]]


def cloud_stats_ref(dist, threshold, max_dist, points=None, crop_min=None, crop_max=None):
    """cn_cloud_stats in float64: [inside the crop, of those with dist < max_dist, the sum of their distances,
    of those with dist < threshold]; the comparisons are on the fp32 values, as on the device."""
    d = np.asarray(dist, dtype=np.float32)
    inside = np.ones(len(d), dtype=bool)
    if crop_min is not None:
        p = np.asarray(points, dtype=np.float32)
        inside = np.all((p >= np.asarray(crop_min, np.float32)) & (p <= np.asarray(crop_max, np.float32)), axis=1)
    near = inside & (d < np.float32(max_dist))
    return [float(inside.sum()), float(near.sum()), float(d[near].astype(np.float64).sum()),
            float((near & (d < np.float32(threshold))).sum())]


def geometry_ref(samples, gt, threshold, max_dist=np.inf, crop_min=None, crop_max=None, area=None, dists=None):
    """The metric dictionary from float64 brute-force distances between the two clouds (dists: those distances,
    samples to gt and gt to samples, where the caller has them already)."""
    def side(a, b, d):
        d = brute_nn(a, b)[0] if d is None else d
        d = np.where(d < max_dist, d, max_dist).astype(np.float32)
        return cloud_stats_ref(d, threshold, max_dist, a, crop_min, crop_max)
    dists = dists or (None, None)
    (n_p, near_p, sum_p, hit_p), (n_g, near_g, sum_g, hit_g) = side(samples, gt, dists[0]), side(gt, samples, dists[1])
    acc, comp = sum_p / near_p, sum_g / near_g
    P, R = hit_p / n_p, hit_g / n_g
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "precision": P, "recall": R,
            "fscore": 2 * P * R / (P + R) if P + R > 0 else 0.0, "n_pred": int(n_p), "n_gt": int(n_g),
            "n_pred_far": int(n_p - near_p), "n_gt_far": int(n_g - near_g), "area": area}


def icosphere(level=2, radius=1.0):
    """(vertices float32 [V, 3], triangles int32 [T, 3]) of an icosahedron subdivided `level` times."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(np.float32), np.array(f, dtype=np.int32)
