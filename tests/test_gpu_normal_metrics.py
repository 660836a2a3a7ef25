"""cn_cloud_normal_stats, cn_normal_errors, metrics.normal_metrics and metrics.mesh_geometry_metrics(gt_normals=...)
against the float64 restatements of tests/mesh_shade_ref.py, which are given the kernel's own index / dist.

Bounds.  Counts are exact.  On mesh_shade_ref.metric_cases() the sums are held to EPS_STATS / EPS_ERRORS, four times
the fp32 restatement's relative error against float64 measured on the CPU and pinned (tests/test_mesh_shade_host.py).
Those figures are sums over thousands of terms whose roundings average out; a sum over a handful of terms does not, so
the size sweeps use per-term bounds from the number format instead: a unit vector's components carry at most 1.5
roundings of 2^-24 each and the three products and two sums of a dot product another 2.5, so |cos| of two unit
vectors is within COS_TERM = 4e-7, and a sum of n of them within n times that; a per-pixel angle is within
EPS_ANGLE_DEG (four times the restatement's worst, pinned), a sum of n angles within n times that and a sum of
squares within 2 x 180 times that."""
import numpy as np
import pytest
import torch

import mesh_shade_ref as R
from mesh_eval_ref import brute_nn, icosphere

pytestmark = pytest.mark.gpu
DEV = "cuda"
COS_TERM = 4e-7


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stats_case(Q, N=97, seed=0):
    rng = np.random.default_rng(1000 + Q + seed)
    qn, tn = R.random_normals(Q, 2 * Q + 1), R.random_normals(N, 2 * Q + 2)
    index = rng.integers(-1, N, size=Q).astype(np.int32)  # -1 among them: no neighbour
    dist = rng.uniform(0.0, 1.0, size=Q).astype(np.float32)
    pts = rng.uniform(-1.0, 1.0, size=(Q, 3)).astype(np.float32)
    if Q >= 63:  # zero and NaN normals on both sides, an infinite one, an index past the targets
        qn[5], qn[17], qn[40, 1] = 0.0, np.nan, np.inf
        tn[3], tn[11, 2] = 0.0, np.nan
        index[7], index[23], index[29] = 3, 11, N
        dist[7], pts[7] = 0.1, 0.0  # (a pair for certain, left out for its target's zero normal)
    return qn, tn, index, dist, pts


@pytest.mark.parametrize("Q", [0, 1, 63, 64, 65, 1025, 256 * 1024 + 1])  # one block's tail; two blocks; a second round of partials
@pytest.mark.parametrize("crop", [False, True])
def test_cloud_normal_stats_against_float64(Q, crop):
    from copenerf import ops
    qn, tn, index, dist, pts = _stats_case(Q)
    max_dist = 0.6
    box = ((-0.8, -1.0, -0.5), (0.9, 0.7, 1.0)) if crop else (None, None)
    want = R.normal_stats_ref(qn, tn, index, dist, max_dist, pts if crop else None, *box)
    args = (_t(qn), _t(tn), _t(index), _t(dist), max_dist, _t(pts) if crop else None, *box)
    out = ops.cloud_normal_stats(*args)
    assert torch.equal(out, ops.cloud_normal_stats(*args))  # bitwise
    got = out.tolist()
    print(Q, crop, got, list(want))
    assert got[0] == want[0] and got[2] == want[2]
    assert abs(got[1] - want[1]) <= COS_TERM * max(want[0], 1)
    if Q >= 63:
        assert 0 < got[0] < Q and got[2] >= 1
    if Q >= 1025:  # every exclusion took something away
        inf = ops.cloud_normal_stats(_t(qn), _t(tn), _t(index), _t(dist)).tolist()
        everything = R.normal_stats_ref(qn, tn, index, dist)
        assert inf[0] == everything[0] > got[0] and inf[2] == everything[2] >= got[2]


def test_cloud_normal_stats_rules_and_pinned_bound():
    from copenerf import ops
    # antiparallel normals count as 1; lengths do not matter; the exclusions one by one
    qn = np.array([[0, 0, 2], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1], [3, 0, 0]], dtype=np.float32)
    tn = np.array([[0, 0, -3], [np.nan, 0, 0], [0, 0.5, 0]], dtype=np.float32)
    index = np.array([0, -1, 0, 0, 1, 0, 2], dtype=np.int32)
    dist = np.array([0.1, 0.1, 0.9, 0.1, 0.1, 0.1, 0.2], dtype=np.float32)
    pts = np.zeros((7, 3), dtype=np.float32)
    pts[5] = 5
    got = ops.cloud_normal_stats(_t(qn), _t(tn), _t(index), _t(dist), 0.5, _t(pts), (-1, -1, -1), (1, 1, 1)).tolist()
    assert got == [2.0, 1.0, 2.0] == list(R.normal_stats_ref(qn, tn, index, dist, 0.5, pts, (-1, -1, -1), (1, 1, 1)))
    (qn, tn, index, dist), _ = R.metric_cases()
    want = R.normal_stats_ref(qn, tn, index, dist, 0.7)
    got = ops.cloud_normal_stats(_t(qn), _t(tn), _t(index), _t(dist), 0.7).tolist()
    rel = abs(got[1] - want[1]) / want[1]
    print("sum of |cos| relative error %.3e (bound %.3e)" % (rel, R.EPS_STATS))
    assert got[0] == want[0] == 2120 and got[2] == 0 and rel <= R.EPS_STATS


def _errors(pred, gt, mask=None):
    from copenerf import ops
    angle, sums = ops.normal_errors(_t(pred), _t(gt), _t(mask))
    a2, s2 = ops.normal_errors(_t(pred), _t(gt), _t(mask))
    assert torch.equal(sums, s2) and np.array_equal(angle.cpu().numpy().view(np.uint32), a2.cpu().numpy().view(np.uint32))
    return angle.cpu().numpy(), np.array(sums.tolist())


def _check_errors(pred, gt, mask=None):
    got_a, got_s = _errors(pred, gt, mask)
    want_a, want_s = R.normal_errors_ref(pred, gt, mask)
    valid = ~np.isnan(want_a)
    assert np.array_equal(np.isnan(got_a), ~valid)
    assert np.array_equal(got_s[[0, 3, 4, 5]], want_s[[0, 3, 4, 5]])
    n = max(want_s[0], 1)
    if valid.any():
        assert np.abs(got_a[valid] - want_a[valid]).max() <= R.EPS_ANGLE_DEG
    assert abs(got_s[1] - want_s[1]) <= n * R.EPS_ANGLE_DEG
    assert abs(got_s[2] - want_s[2]) <= n * 360.0 * R.EPS_ANGLE_DEG
    return got_a, got_s, want_s


@pytest.mark.parametrize("n", [1, 255, 256, 257, 64 * 48])
def test_normal_errors_sizes_rotations_and_masks(n):
    """Identical maps give 0 exactly, antiparallel ones 180; maps rotated by known angles give exact counts; mean and
    rmse against float64; mask, zero and NaN normals are invalid."""
    p = R.random_normals(n, n)
    a, s = _errors(p, p)
    assert np.all(a == 0) and list(s) == [n, 0, 0, n, n, n]
    a, s = _errors(p, -p)
    assert np.all(a == 180) and list(s) == [n, 180.0 * n, 32400.0 * n, 0, 0, 0]
    axis = np.array([0.3, -0.7, 0.64])
    axis /= np.linalg.norm(axis)
    q = np.cross(p.astype(np.float64), axis)  # perpendicular to the axis: turned by exactly the rotation's angle
    for deg in (5, 11, 12, 22, 23, 29, 31, 90):
        g = (q @ R.rotation(axis, deg).T).astype(np.float32)
        a, s, want = _check_errors(q.astype(np.float32), g)
        assert list(s[3:]) == [n * (deg < t) for t in R.ANGLE_THRESHOLDS] and np.abs(a - deg).max() < 1e-4
        mean, rmse = s[1] / s[0], np.sqrt(s[2] / s[0])
        assert abs(mean - want[1] / n) <= R.EPS_ANGLE_DEG and abs(rmse - np.sqrt(want[2] / n)) <= 2 * R.EPS_ANGLE_DEG
    # a mask and unusable normals
    rng = np.random.default_rng(n)
    p, g = q.astype(np.float32), (q @ R.rotation(axis, 17.0).T).astype(np.float32)
    mask = (rng.random(n) < 0.7).astype(np.uint8)
    if n >= 255:
        p, g = p.copy(), g.copy()
        p[3], g[9], p[20, 0], g[31, 2] = 0.0, 0.0, np.nan, np.inf
        mask[[3, 9, 20, 31, 40]] = 1, 1, 1, 1, 0
    a, s, want = _check_errors(p, g, mask)
    assert s[0] == want[0] == (mask != 0).sum() - (4 if n >= 255 else 0)
    assert list(s[3:]) == [0, s[0], s[0]]
    a, s = _errors(p, g, np.zeros(n, dtype=np.uint8))
    assert np.all(np.isnan(a)) and list(s) == [0] * 6


def test_normal_errors_pinned_bound_and_normal_metrics():
    from copenerf import metrics
    _, (pred, gt) = R.metric_cases()
    a, s, want = _check_errors(pred, gt)
    rel = max(abs(s[1] - want[1]) / want[1], abs(s[2] - want[2]) / want[2])
    print("sums' relative error %.3e (bound %.3e)" % (rel, R.EPS_ERRORS))
    assert rel <= R.EPS_ERRORS
    h, w = 48, 64
    rng = np.random.default_rng(3)
    mask = rng.random((h, w)) < 0.8
    tp, tg, tm = _t(pred.reshape(h, w, 3)), _t(gt.reshape(h, w, 3)), _t(mask)
    res = metrics.normal_metrics(tp, tg, tm)
    ang, sums = R.normal_errors_ref(pred, gt, mask)
    v = ang[~np.isnan(ang)]
    assert list(res) == list(metrics.NORMAL_KEYS) == ["mean", "median", "rmse", "a11.25", "a22.5", "a30"]
    assert abs(res["mean"] - v.mean()) <= R.EPS_ANGLE_DEG and abs(res["rmse"] - np.sqrt((v * v).mean())) <= 2 * R.EPS_ANGLE_DEG
    assert abs(res["median"] - np.median(v)) <= R.EPS_ANGLE_DEG
    assert [res["a11.25"], res["a22.5"], res["a30"]] == [float(x) / len(v) for x in sums[3:]]
    # the median by np.median's rule on the kernel's own buffer, odd and even counts
    for keep in (len(v) - 1, len(v) - 2):
        m2 = mask.reshape(-1).copy()
        m2[np.flatnonzero(m2)[keep:]] = False
        got_a, _ = _errors(pred, gt, m2.astype(np.uint8))
        r2 = metrics.normal_metrics(tp, tg, _t(m2.reshape(h, w)))
        assert m2.sum() == keep and r2["median"] == float(np.median(got_a[~np.isnan(got_a)].astype(np.float64)))
    # a stack: the mean over the images that have a valid pixel; none: None
    empty = torch.zeros(h, w, dtype=torch.bool, device=DEV)
    stack = metrics.normal_metrics(torch.stack([tp, tp, tg]), torch.stack([tg, tp, tg]), torch.stack([tm, empty, tm]))
    assert stack["mean"] == 0.5 * res["mean"] and stack["a11.25"] == 0.5 * (res["a11.25"] + 1.0)
    assert metrics.normal_metrics(torch.stack([tp, tp]), torch.stack([tg, tg]), torch.stack([empty, empty])) is None
    zero = torch.zeros_like(tp)
    assert metrics.normal_metrics(tp, zero) is None and metrics.normal_metrics(tp, tg)["mean"] > 0


# ---- mesh_geometry_metrics(gt_normals=...) ---------------------------------------------------------------------------

def _fibonacci(n, radius):
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    phi = np.pi * (1 + 5 ** 0.5) * k
    r = np.sqrt(1 - z * z)
    unit = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    return (radius * unit).astype(np.float32), unit.astype(np.float32)


def _cube_cloud(half=0.6, n=20):
    """Points on the six faces of a cube, away from its edges, with the faces' normals."""
    g = (np.arange(n) + 0.5) / n * 2 * half * 0.9 - half * 0.9
    a, b = (x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij"))
    pts, nrm = [], []
    for axis in range(3):
        for side in (-1.0, 1.0):
            p = np.zeros((len(a), 3))
            p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = side * half, a, b
            e = np.zeros(3)
            e[axis] = side
            pts.append(p)
            nrm.append(np.tile(e, (len(a), 1)))
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32)


def _restate(v, f, gt, gtn, S, seed, max_dist, transform=None):
    """The normal entries in float64 from the device's own samples and nearest neighbours (both deterministic, so
    these are the ones mesh_geometry_metrics used), and the share of pairs whose neighbour a float64 brute force
    search disagrees on (near-ties only)."""
    from copenerf import metrics, ops
    tv = _t(v)
    if transform is not None:
        M = torch.as_tensor(transform, dtype=torch.float32).to(DEV)
        tv = (tv @ M[:3, :3].T + M[:3, 3]).contiguous()
    handle, _ = ops.mesh_area(tv, _t(f))
    samples, tri = ops.mesh_sample(handle, S, torch.tensor([seed, 0], dtype=torch.uint64, device=DEV), want_tri=True)
    c = tv.cpu().numpy().astype(np.float64)[f[tri.cpu().numpy()]]
    sn = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    sn /= np.linalg.norm(sn, axis=1, keepdims=True)
    out, disagree = [], 0.0
    for q, t, qn, tn in ((samples, _t(gt), sn, gtn), (_t(gt), samples, gtn, sn)):
        dist, index = metrics.nearest_distances(q, t, max_dist)
        index, dist = index.cpu().numpy(), dist.cpu().numpy()
        d64, i64, second = brute_nn(q.cpu().numpy(), t.cpu().numpy())
        found = index >= 0
        clear = found & (second - d64 > 1e-5)
        assert np.array_equal(index[clear], i64[clear])
        assert np.array_equal(found, d64 < max_dist) or np.abs(d64[found != (d64 < max_dist)] - max_dist).max() < 1e-5
        disagree = max(disagree, float((index[found] != i64[found]).mean()))
        qn64, tn64 = np.asarray(qn, dtype=np.float64), np.asarray(tn, dtype=np.float64)
        cos = np.abs((qn64[found] / np.linalg.norm(qn64[found], axis=1, keepdims=True) *
                      (tn64[index[found]] / np.linalg.norm(tn64[index[found]], axis=1, keepdims=True))).sum(1))
        out.append((int(found.sum()), float(cos.mean())))
    return out, disagree


@pytest.mark.parametrize("case", ["concentric", "cube"])
def test_mesh_geometry_metrics_with_normals(case):
    from copenerf import metrics
    S, seed = 4000, 5
    if case == "concentric":
        v, f = icosphere(3, 1.0)
        gt, gtn = _fibonacci(3000, 1.05)
        gtn = (gtn * np.linspace(0.5, 2.0, len(gtn))[:, None]).astype(np.float32)  # any length
        max_dist = float("inf")
    else:
        v, f = icosphere(3, 0.5)
        gt, gtn = _cube_cloud()
        max_dist = 0.3  # the cube's corner regions are farther from the sphere than this
    kw = dict(threshold=0.1, max_dist=max_dist, n_samples=S, seed=seed)
    plain = metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt), **kw)
    res = metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt), gt_normals=_t(gtn), **kw)
    assert tuple(plain) == metrics.GEOMETRY_KEYS and tuple(res) == metrics.GEOMETRY_KEYS + metrics.NORMAL_GEOMETRY_KEYS
    assert all(res[k] == plain[k] for k in plain)  # without gt_normals: exactly today's keys and values
    (want_p, want_g), disagree = _restate(v, f, gt, gtn, S, seed, max_dist)
    print(case, {k: res[k] for k in metrics.NORMAL_GEOMETRY_KEYS}, "restated", want_p, want_g, "near-ties", disagree)
    assert res["n_pred_normal"] == want_p[0] == res["n_pred"] - res["n_pred_far"]
    assert res["n_gt_normal"] == want_g[0] == res["n_gt"] - res["n_gt_far"]
    # (the device's face normals are fp32 cross products: COS_TERM covers their rounding as it covers the kernel's)
    assert abs(res["normal_accuracy"] - want_p[1]) <= 2 * COS_TERM
    assert abs(res["normal_completeness"] - want_g[1]) <= 2 * COS_TERM
    assert res["normal_consistency"] == 0.5 * (res["normal_accuracy"] + res["normal_completeness"])
    assert disagree < 0.01
    if case == "concentric":
        # analytic: a face normal of the icosphere is within `face` of the direction of any point of the face, a
        # sample and its nearest ground-truth point (and the reverse) within `gap` of one another as directions
        c = v[f].astype(np.float64)
        fn = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        fn /= np.linalg.norm(fn, axis=1, keepdims=True)
        face = np.degrees(np.arccos(np.clip((fn[:, None, :] * c).sum(-1), -1, 1).min()))
        gap = np.degrees(2.0 * np.sqrt(4 * np.pi / min(S, len(gt))))  # twice the clouds' mean spacing
        floor = np.cos(np.radians(face + gap))
        assert floor > 0.95
        for k in ("normal_accuracy", "normal_completeness", "normal_consistency"):
            assert floor <= res[k] <= 1.0, (k, res[k], floor)
        assert res["n_pred_normal"] == S and res["n_gt_normal"] == len(gt)
    else:
        assert 0 < res["n_gt_normal"] < len(gt) and 0 < res["n_pred_normal"] < S
        assert 0.5 < res["normal_consistency"] < 0.99  # a sphere is no cube
    # a transform turns the mesh's normals with it
    Rm = R.rotation((0.4, -0.2, 0.9), 71.0)
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = 1.3 * Rm, (0.2, -0.4, 0.1)
    gt2 = (gt.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    gtn2 = (gtn.astype(np.float64) @ Rm.T).astype(np.float32)
    kw2 = dict(kw, threshold=0.13, max_dist=max_dist * 1.3)
    moved = metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt2), gt_normals=_t(gtn2), transform=M, **kw2)
    (mp, mg), _ = _restate(v, f, gt2, gtn2, S, seed, max_dist * 1.3, transform=M)
    assert (moved["n_pred_normal"], moved["n_gt_normal"]) == (mp[0], mg[0])
    assert abs(moved["normal_accuracy"] - mp[1]) <= 2 * COS_TERM and abs(moved["normal_completeness"] - mg[1]) <= 2 * COS_TERM
    assert abs(moved["normal_consistency"] - res["normal_consistency"]) < 0.01


def test_cull_gt_filters_the_normals_with_the_points():
    from copenerf import mesh, metrics, ops
    from mesh_raster_ref import side_views
    v, f = icosphere(3, 0.5)
    gt, gtn = _fibonacci(3000, 1.2)  # wider than the views: some points fall outside both frustums
    h, w = 48, 64
    views = side_views(h, w)[:2]
    kw = dict(threshold=0.8, n_samples=3000, seed=2, cull_views=views, cull_resolution=(h, w))
    got = metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt), gt_normals=_t(gtn), cull_gt=True, **kw)
    seen = (ops.mesh_visibility(_t(gt), mesh.view_projections(views, (h, w), None, DEV), h, w) > 0).cpu().numpy()
    assert 0 < seen.sum() < len(gt)
    by_hand = metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt[seen]), gt_normals=_t(gtn[seen]), **kw)
    assert got == by_hand
    shifted = metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt[seen]), gt_normals=_t(np.roll(gtn, 500, axis=0)[seen]), **kw)
    assert shifted["normal_consistency"] < got["normal_consistency"] - 0.05 and shifted["chamfer"] == got["chamfer"]
    with pytest.raises(ValueError, match="normals for"):
        metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt), gt_normals=_t(gtn[:-1]), **kw)
