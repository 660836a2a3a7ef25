"""Test infrastructure: restatements of the mesh shading pass (csrc/cn_mesh_shade.hip) and of the two normal metric
kernels (cn_cloud_normal_stats in csrc/cn_mesh_eval.hip, cn_normal_errors in csrc/cn_metrics.hip).

shade_ref, normal_stats_ref and normal_errors_ref are the yardsticks: float64 numpy from the fp32 inputs.  They are
given what the pass under test is given -- the rasteriser's tri image, the nearest neighbours' index / dist -- so no
comparison depends on a coverage or tie decision.

shade_f32, normal_stats_f32 and normal_errors_f32 are NOT the yardstick and not the code under test: they restate the
kernels' fp32 operation order in numpy float32 so that the bounds of the GPU tests can be measured on the CPU against
the float64 versions (tests/test_mesh_shade_host.py does, and pins the figures below).  The GPU bar is four times
each figure: the margin for the device's division, square root and atan2f differing from numpy's in the last place,
the factor F32_WORST / EPS_DEPTH of mesh_raster_ref.py use."""
import numpy as np

from mesh_raster_ref import box_mesh, look_at, make_view, merge, scene_group, scene_thread  # noqa: F401

ANGLE_THRESHOLDS = (11.25, 22.5, 30.0)
ANGLE_CLEAR = 1e-3      # degrees: no test angle lies this close to a threshold (normal_errors_ref asserts it)
IMAGE_NEAR = 1e-4       # a picture value this close to an integer may land on either side: compared within one level
IMAGE_NEAR_SHARE = 0.01  # at most this share of a scene's covered pixels may be of that kind (asserted on the CPU)

# The worst figures of the fp32 restatements against float64 on the GPU tests' scenes (scene_thread and scene_group,
# every covered pixel, attributes = the vertex positions; the metric kernels on metric_cases()), measured by
# tests/test_mesh_shade_host.py, which pins them.  The GPU bounds are MARGIN times each.
MARGIN = 4.0
ATTR_F32_WORST = 1.71e-6        # absolute, attributes of |value| <= 2 (measured 1.702e-6: scene_group)
NORMAL_F32_WORST_DEG = 7.6e-6   # the angle between the two unit normals, degrees (measured 7.55e-6, camera frame)
STATS_F32_WORST = 2.5e-10       # relative, cn_cloud_normal_stats' sum of |cos| (measured 2.48e-10 over 2120 pairs)
ERRORS_F32_WORST = 5.1e-8       # relative, cn_normal_errors' sum of angles (2.36e-8) and of squares (5.02e-8)
ANGLE_F32_WORST_DEG = 9.3e-6    # absolute, cn_normal_errors' per-pixel angle, degrees (measured 9.21e-6, angles <= 40)
EPS_ATTR = MARGIN * ATTR_F32_WORST
EPS_NORMAL_DEG = MARGIN * NORMAL_F32_WORST_DEG
EPS_STATS = MARGIN * STATS_F32_WORST
EPS_ERRORS = MARGIN * ERRORS_F32_WORST
EPS_ANGLE_DEG = MARGIN * ANGLE_F32_WORST_DEG


def to_u8(v):
    """cn_visuals.hip's conversion: NaN and negatives 0, truncation, saturation at 255."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.floor(np.minimum(np.where(np.isnan(v), 0.0, v), 255.0)), 0.0).astype(np.uint8)


def camera_centre(P):
    """The camera centre of a projection P [3, 4]: its null vector, in float64."""
    _, _, vt = np.linalg.svd(np.asarray(P, dtype=np.float32).astype(np.float64))
    return vt[-1, :3] / vt[-1, 3]


def _unit(f, v):
    """v / sqrt((x x + y y) + z z) in dtype f: (unit, usable)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).astype(f)
        ok = (length > 0) & np.isfinite(length)
        return np.where(ok[..., None], v / np.where(ok, length, f(1))[..., None], f(0)).astype(f), ok


def _shade(f, vertices, triangles, P, tri, attr, vnormals, rot, light, ambient, grey, albedo_from_attr, fill):
    P = np.asarray(P, dtype=np.float32).astype(f)
    X = np.asarray(vertices, dtype=np.float32).astype(f)
    triangles = np.asarray(triangles).reshape(-1, 3)
    tri = np.asarray(tri)
    h, w = tri.shape
    T, V = len(triangles), len(X)
    ok = (tri >= 0) & (tri < T)
    ids = triangles[np.where(ok, tri, 0)] if T else np.zeros((h, w, 3), dtype=np.int64)
    ok &= ((ids >= 0) & (ids < V)).all(-1)
    ys, xs = np.nonzero(ok)
    ids = ids[ys, xs].astype(np.int64)
    n_px = len(ys)
    ar = np.arange(n_px)
    Xc = X[ids] if n_px else np.zeros((0, 3, 3), dtype=f)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b, c = (((P[r, 0] * Xc[..., 0] + P[r, 1] * Xc[..., 1]) + P[r, 2] * Xc[..., 2]) + P[r, 3] for r in range(3))
        sx, sy, iw = a / c, b / c, f(1.0) / c
        px, py = xs.astype(f), ys.astype(f)
        g, area = [], None
        for k in range(3):
            i, j = (k + 1) % 3, (k + 2) % 3
            fwd = ids[:, i] < ids[:, j]
            lo, hi = np.where(fwd, i, j), np.where(fwd, j, i)
            sg = np.where(fwd, 1.0, -1.0).astype(f)
            lx, ly = sx[ar, lo], sy[ar, lo]
            dx, dy = sx[ar, hi] - lx, sy[ar, hi] - ly
            g.append((sg * (dx * (py - ly) - dy * (px - lx))) * iw[:, k])
            if k == 2:
                area = sg * (dx * (sy[:, 2] - ly) - dy * (sx[:, 2] - lx))
        den = (g[0] + g[1]) + g[2]
        lam = [gk / den for gk in g]
        assert all(x.dtype == f for x in lam)
        out = {"mask": ok, "lam": np.stack(lam, 1)}

        def interp(A):
            A = np.asarray(A, dtype=np.float32).astype(f)
            return (lam[0][:, None] * A[ids[:, 0]] + lam[1][:, None] * A[ids[:, 1]]) + lam[2][:, None] * A[ids[:, 2]]

        if attr is not None:
            full = np.full((h, w, np.asarray(attr).shape[1]), fill, dtype=f)
            full[ys, xs] = interp(attr)
            out["attr"] = full
        u, v = Xc[:, 1] - Xc[:, 0], Xc[:, 2] - Xc[:, 0]
        n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                      u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
        det = (P[0, 0] * (P[1, 1] * P[2, 2] - P[1, 2] * P[2, 1]) - P[0, 1] * (P[1, 0] * P[2, 2] - P[1, 2] * P[2, 0])) + \
            P[0, 2] * (P[1, 0] * P[2, 1] - P[1, 1] * P[2, 0])
        turn = np.where(area * det < 0, 1.0, -1.0).astype(f)
        n, _ = _unit(f, turn[:, None] * n)
        out["facing"] = turn
        if vnormals is not None:
            m = interp(vnormals)
            good = _unit(f, m)[1]
            mlen = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
            dot = (m[:, 0] * n[:, 0] + m[:, 1] * n[:, 1]) + m[:, 2] * n[:, 2]
            side = np.where(dot < 0, -1.0, 1.0).astype(f)
            sm = (side[:, None] * m) / np.where(good, mlen, f(1))[:, None]
            n = np.where(good[:, None], sm, n).astype(f)
        if rot is not None:
            R = np.asarray(rot, dtype=np.float32).astype(f)
            n = np.stack([(R[r, 0] * n[:, 0] + R[r, 1] * n[:, 1]) + R[r, 2] * n[:, 2] for r in range(3)], 1)
        full = np.zeros((h, w, 3), dtype=f)
        full[ys, xs] = n
        out["normal"] = full
        out["normal_pre"] = n * f(128.0) + f(128.0)  # [covered, 3], in the order of np.nonzero(mask)
        L = np.asarray(light, dtype=np.float32).astype(f)
        lamb = np.maximum(f(0.0), (n[:, 0] * L[0] + n[:, 1] * L[1]) + n[:, 2] * L[2])
        s = f(np.float32(ambient)) + (f(1.0) - f(np.float32(ambient))) * lamb
        alb = interp(np.asarray(attr)[:, :3]) if albedo_from_attr else np.full((n_px, 3), f(np.float32(grey)), dtype=f)
        out["shaded_pre"] = (alb * s[:, None]) * f(255.0)
    return out


def shade_ref(vertices, triangles, P, tri, attr=None, vnormals=None, rot=None, light=(0.0, 0.0, 1.0), ambient=0.3,
              grey=0.8, albedo_from_attr=False, fill=0.0):
    """One view in float64 from the fp32 inputs, given the tri image [h, w]: a dict with mask [h, w] (not background),
    lam [covered, 3], attr [h, w, C] (with attr), normal [h, w, 3], facing [covered] (+1: the normal as wound faces the
    camera) and the pictures' values before the conversion, normal_pre / shaded_pre [covered, 3] in np.nonzero(mask)'s
    order."""
    return _shade(np.float64, vertices, triangles, P, tri, attr, vnormals, rot, light, ambient, grey, albedo_from_attr, fill)


def shade_f32(vertices, triangles, P, tri, attr=None, vnormals=None, rot=None, light=(0.0, 0.0, 1.0), ambient=0.3,
              grey=0.8, albedo_from_attr=False, fill=0.0):
    """The kernel's operation order in numpy float32: what shade_ref returns, in float32."""
    return _shade(np.float32, vertices, triangles, P, tri, attr, vnormals, rot, light, ambient, grey, albedo_from_attr, fill)


def angle_deg(a, b):
    """The angle in degrees between unit vectors [..., 3], float64, by atan2."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))


def compare_pictures(got, pre, share_cap=None):
    """The picture criterion: got uint8 [covered, 3] equals to_u8(pre) exactly where pre (the reference's value before
    the conversion) is farther than IMAGE_NEAR from an integer, and within one level elsewhere.  Returns the share of
    pixels with a channel of the second kind, asserted against share_cap when given."""
    pre = np.asarray(pre, dtype=np.float64)
    near = np.abs(pre - np.round(pre)) <= IMAGE_NEAR
    want = to_u8(pre).astype(np.int64)
    got = np.asarray(got).astype(np.int64)
    assert np.array_equal(got[~near], want[~near])
    assert np.all(np.abs(got[near] - want[near]) <= 1)
    share = float(near.any(-1).mean()) if len(pre) else 0.0
    if share_cap is not None:
        assert share <= share_cap, share
    return share


# ---- the metric kernels --------------------------------------------------------------------------------------------

def _normal_stats(f, qn, tn, index, dist, max_dist, points, crop_min, crop_max):
    qn, tn = np.asarray(qn, dtype=np.float32), np.asarray(tn, dtype=np.float32)
    index, dist = np.asarray(index), np.asarray(dist, dtype=np.float32)
    Q, N = len(qn), len(tn)
    inside = np.ones(Q, dtype=bool)
    if points is not None:
        p = np.asarray(points, dtype=np.float32)
        inside = ((p >= np.asarray(crop_min, dtype=np.float32)) & (p <= np.asarray(crop_max, dtype=np.float32))).all(1)
    with np.errstate(invalid="ignore"):
        pair = inside & (index >= 0) & (index < N) & (dist < np.float32(max_dist))
    q, qok = _unit(f, qn[pair].astype(f))
    t, tok = _unit(f, tn[index[pair]].astype(f) if N else np.zeros((0, 3), dtype=f))
    ok = qok & tok
    cos = np.abs((q[:, 0] * t[:, 0] + q[:, 1] * t[:, 1]) + q[:, 2] * t[:, 2])[ok]
    return np.array([ok.sum(), cos.astype(np.float64).sum(), (~ok).sum()], dtype=np.float64)


def normal_stats_ref(qn, tn, index, dist, max_dist=np.inf, points=None, crop_min=None, crop_max=None):
    """cn_cloud_normal_stats in float64 from the fp32 inputs: (pairs counted, sum |q . t[index]|, pairs left out)."""
    return _normal_stats(np.float64, qn, tn, index, dist, max_dist, points, crop_min, crop_max)


def normal_stats_f32(qn, tn, index, dist, max_dist=np.inf, points=None, crop_min=None, crop_max=None):
    """The kernel's fp32 normalisation and dot product, summed in double."""
    return _normal_stats(np.float32, qn, tn, index, dist, max_dist, points, crop_min, crop_max)


def _normal_errors(f, pred, gt, mask, check):
    pred, gt = np.asarray(pred, dtype=np.float32).reshape(-1, 3), np.asarray(gt, dtype=np.float32).reshape(-1, 3)
    valid = np.ones(len(pred), dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    p, pok = _unit(f, pred.astype(f))
    g, gok = _unit(f, gt.astype(f))
    valid = valid & pok & gok
    cx = p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1]
    cy = p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2]
    cz = p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0]
    cr = np.sqrt((cx * cx + cy * cy) + cz * cz)
    dt = (p[:, 0] * g[:, 0] + p[:, 1] * g[:, 1]) + p[:, 2] * g[:, 2]
    rad = np.arctan2(cr, dt)
    assert rad.dtype == f
    ang = (rad.astype(np.float64) * 57.29577951308232).astype(f)
    ang = np.where(valid, ang, np.nan).astype(f)
    a = ang[valid].astype(np.float64)
    if check:
        for th in ANGLE_THRESHOLDS:
            assert not np.any(np.abs(a - th) <= ANGLE_CLEAR), th
    sums = np.array([valid.sum(), a.sum(), (a * a).sum()] + [(a < th).sum() for th in ANGLE_THRESHOLDS], dtype=np.float64)
    return ang, sums


def normal_errors_ref(pred, gt, mask=None, check=True):
    """cn_normal_errors in float64 from the fp32 inputs: (angle [n] in degrees, NaN where invalid; the six sums).
    check: assert that no valid angle lies within ANGLE_CLEAR of a threshold, so that the counts are decided."""
    return _normal_errors(np.float64, pred, gt, mask, check)


def normal_errors_f32(pred, gt, mask=None):
    """The kernel's fp32 operation order (normalise, cross, dot, atan2, degrees), the sums in double."""
    return _normal_errors(np.float32, pred, gt, mask, False)


# ---- scenes and cases ----------------------------------------------------------------------------------------------

def projections(views, h, w):
    """fp32 [N, 3, 4] of mesh_raster_ref-style views, by copenerf.mesh.camera_projection."""
    from copenerf.mesh import camera_projection
    return np.stack([camera_projection(v["camera_mat"], v["world_mat"], v.get("scale_mat"), (h, w)) for v in views])


def rotation(axis, degrees):
    """Rodrigues' rotation matrix, float64."""
    axis = np.asarray(axis, dtype=np.float64)
    k = axis / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.radians(degrees)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def random_normals(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= rng.uniform(0.2, 3.0, size=(n, 1)) / np.linalg.norm(v, axis=1, keepdims=True)  # (any length)
    return v.astype(np.float32)


def metric_cases():
    """The inputs the metric kernels' bounds are measured on: (qn, tn, index, dist) for the statistics, 3000 pairs
    of normals of arbitrary length, and (pred, gt) for the errors, a 64 x 48 map against itself rotated by a few
    degrees around per-pixel axes."""
    rng = np.random.default_rng(7)
    Q, N = 3000, 1700
    qn, tn = random_normals(Q, 1), random_normals(N, 2)
    index = rng.integers(0, N, size=Q).astype(np.int32)
    dist = rng.uniform(0.0, 1.0, size=Q).astype(np.float32)
    n = 64 * 48
    pred = random_normals(n, 3)
    axes = np.cross(pred.astype(np.float64), rng.normal(size=(n, 3)))
    ang = rng.uniform(0.5, 40.0, size=n)
    for th in ANGLE_THRESHOLDS:
        ang = np.where(np.abs(ang - th) < 0.05, ang + 0.1, ang)
    gt = np.stack([rotation(ax, a) @ p for ax, a, p in zip(axes, ang, pred.astype(np.float64))])
    gt *= rng.uniform(0.5, 2.0, size=(n, 1))
    return (qn, tn, index, dist), (pred, gt.astype(np.float32))
