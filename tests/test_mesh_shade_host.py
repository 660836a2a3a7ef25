"""The host side of mesh shading and the normal metrics, no device needed: the float64 yardsticks of
tests/mesh_shade_ref.py check themselves (the reprojection identity of the perspective-correct weights, the facing
rule against the null-vector camera centre), the fp32 restatements' errors on the GPU tests' scenes are what the GPU
tests' bounds assume, and tools/render_mesh.py / tools/evaluate_mesh.py parse the new arguments and refuse a PLY
without the normals or colours a flag needs.

Measured here on the CPU (mesh_shade_ref pins these; the GPU bounds are four times each):
  attributes (= vertex positions, |value| <= 2), all 20,697 covered pixels of scene_thread and scene_group:
      worst absolute difference of shade_f32 against shade_ref 1.702e-6 (scene_group); pinned 1.71e-6
  normals, as an angle: 5.24e-6 degrees in the world frame, 7.55e-6 in the camera frame; pinned 7.6e-6
  cn_cloud_normal_stats' sum of |cos| over 2120 counted pairs: relative 2.48e-10; pinned 2.5e-10
  cn_normal_errors' sum of angles 2.36e-8 and of squares 5.02e-8 relative, pinned 5.1e-8; per-pixel angle 9.21e-6
      degrees absolute (angles up to 40 degrees), pinned 9.3e-6
  pictures: in the camera frame at most 0.06 % of a view's covered pixels hold a value within 1e-4 of an integer
      (cap 1 %); in the world frame the icosphere's symmetric faces put 8 % of them exactly on 128, which is why the
      GPU picture test renders in the camera frame."""
import os
import sys

import numpy as np
import pytest

import mesh_shade_ref as R
from mesh_raster_ref import raster_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scenes():
    for name, sc in (("scene_thread", R.scene_thread()), ("scene_group", R.scene_group())):
        v, f, views, h, w = sc[:5]
        P = R.projections(views, h, w)
        tris = [raster_f32(v, f, P[i], h, w, 1e-4)[1] for i in range(len(P))]
        yield name, v, f, views, P, tris


@pytest.fixture(scope="module")
def scenes():
    return list(_scenes())


def test_reprojection_identity_and_facing_rule(scenes):
    """With attr = the vertex positions, proj . [attr, 1] gives back the pixel: the identity the weights must satisfy.
    The normal as wound faces the camera iff (signed screen area) x det(proj[:, :3]) < 0: checked against the
    null-vector camera centre at every covered pixel, and the oriented normal points at the camera."""
    covered = 0
    for name, v, f, views, P, tris in scenes:
        for i, tri in enumerate(tris):
            a = R.shade_ref(v, f, P[i], tri, attr=v)
            m = a["mask"]
            ys, xs = np.nonzero(m)
            covered += len(ys)
            X = np.concatenate([a["attr"][m], np.ones((len(ys), 1))], 1) @ P[i].astype(np.float64).T
            assert np.abs(X[:, 0] / X[:, 2] - xs).max() < 1e-12 and np.abs(X[:, 1] / X[:, 2] - ys).max() < 1e-12
            assert np.abs(a["lam"].sum(1) - 1).max() < 1e-14
            C = R.camera_centre(P[i])
            corners = v[f[tri[ys, xs]]].astype(np.float64)
            wound = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
            assert np.array_equal(((C - corners[:, 0]) * wound).sum(1) > 0, a["facing"] > 0), (name, i)
            assert np.all(((C - corners[:, 0]) * a["normal"][m]).sum(1) > 0)
            assert np.abs(np.linalg.norm(a["normal"][m], axis=1) - 1).max() < 1e-14
    assert covered == 20697


def test_fp32_restatement_errors_are_the_pinned_figures(scenes):
    """What the GPU shade tests' bounds are made of (the module docstring has the figures)."""
    worst_attr = worst_world = worst_cam = 0.0
    for name, v, f, views, P, tris in scenes:
        col = (np.abs(v) / np.abs(v).max()).astype(np.float32)
        for i, tri in enumerate(tris):
            a, b = R.shade_ref(v, f, P[i], tri, attr=v), R.shade_f32(v, f, P[i], tri, attr=v)
            m = a["mask"]
            assert np.array_equal(m, b["mask"]) and b["attr"].dtype == np.float32 and b["normal"].dtype == np.float32
            worst_attr = max(worst_attr, float(np.abs(a["attr"][m] - b["attr"][m]).max()))
            worst_world = max(worst_world, float(R.angle_deg(a["normal"][m], b["normal"][m]).max()))
            kw = dict(attr=col, rot=views[i]["world_mat"][:3, :3].astype(np.float32), albedo_from_attr=True)
            a, b = R.shade_ref(v, f, P[i], tri, **kw), R.shade_f32(v, f, P[i], tri, **kw)
            worst_cam = max(worst_cam, float(R.angle_deg(a["normal"][m], b["normal"][m]).max()))
            for key in ("normal_pre", "shaded_pre"):  # the picture criterion, the restatement standing in for the device
                R.compare_pictures(R.to_u8(b[key]), a[key], share_cap=R.IMAGE_NEAR_SHARE)
    print("attr %.3e  normal world %.3e deg  camera %.3e deg" % (worst_attr, worst_world, worst_cam))
    assert 0.5 * R.ATTR_F32_WORST < worst_attr <= R.ATTR_F32_WORST
    assert 0.5 * R.NORMAL_F32_WORST_DEG < max(worst_world, worst_cam) <= R.NORMAL_F32_WORST_DEG
    assert R.EPS_ATTR == 4 * R.ATTR_F32_WORST and R.EPS_NORMAL_DEG == 4 * R.NORMAL_F32_WORST_DEG


def test_metric_restatement_errors_are_the_pinned_figures():
    (qn, tn, index, dist), (pred, gt) = R.metric_cases()
    a, b = R.normal_stats_ref(qn, tn, index, dist, 0.7), R.normal_stats_f32(qn, tn, index, dist, 0.7)
    assert a[0] == b[0] == 2120 and a[2] == b[2] == 0
    rel = abs(a[1] - b[1]) / a[1]
    ang_a, sa = R.normal_errors_ref(pred, gt)
    ang_b, sb = R.normal_errors_f32(pred, gt)
    assert np.array_equal(sa[[0, 3, 4, 5]], sb[[0, 3, 4, 5]]) and sa[0] == 64 * 48
    rel_e = max(abs(sa[1] - sb[1]) / sa[1], abs(sa[2] - sb[2]) / sa[2])
    worst = float(np.abs(ang_a - ang_b).max())
    print("stats %.3e  errors %.3e  angle %.3e deg" % (rel, rel_e, worst))
    assert 0.5 * R.STATS_F32_WORST < rel <= R.STATS_F32_WORST
    assert 0.5 * R.ERRORS_F32_WORST < rel_e <= R.ERRORS_F32_WORST
    assert 0.5 * R.ANGLE_F32_WORST_DEG < worst <= R.ANGLE_F32_WORST_DEG
    assert R.EPS_STATS == 4 * R.STATS_F32_WORST and R.EPS_ERRORS == 4 * R.ERRORS_F32_WORST


def test_yardsticks_on_known_answers():
    # the angle yardstick: rotations by known angles, identical and antiparallel maps, a threshold too close
    p = R.random_normals(50, 5)
    for deg in (5, 11, 12, 22, 23, 29, 31, 90):
        axis = np.cross(p[0], p[1]) / np.linalg.norm(np.cross(p[0], p[1]))
        q = (p - np.outer(p @ axis, axis)).astype(np.float32)  # perpendicular to the axis: rotated by exactly deg
        g = (q.astype(np.float64) @ R.rotation(axis, deg).T).astype(np.float32)
        ang, sums = R.normal_errors_ref(q, g)
        assert np.abs(ang - deg).max() < 1e-4
        assert list(sums[3:]) == [50 * (deg < t) for t in R.ANGLE_THRESHOLDS]
    assert R.normal_errors_ref(p, p)[1][1] == 0 and np.all(R.normal_errors_ref(p, -p)[0] == 180)
    q = np.array([[1.0, 0, 0]], dtype=np.float32)
    g = np.array([[np.cos(np.radians(22.5)), np.sin(np.radians(22.5)), 0]], dtype=np.float32)
    with pytest.raises(AssertionError):
        R.normal_errors_ref(q, g)
    # the statistics yardstick: the exclusions one by one
    qn = np.array([[0, 0, 2], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1]], dtype=np.float32)
    tn = np.array([[0, 0, -3], [np.nan, 0, 0]], dtype=np.float32)
    index = np.array([0, -1, 0, 0, 1, 0], dtype=np.int32)
    dist = np.array([0.1, 0.1, 0.9, 0.1, 0.1, 0.1], dtype=np.float32)
    pts = np.zeros((6, 3), dtype=np.float32)
    pts[5] = 5
    got = R.normal_stats_ref(qn, tn, index, dist, 0.5, pts, (-1, -1, -1), (1, 1, 1))
    assert list(got) == [1, 1, 2]  # antiparallel counts as 1; the zero and the NaN normal are left out
    assert R.to_u8([-1, np.nan, 0.99, 1.0, 254.999, 255, 300]).tolist() == [0, 0, 0, 1, 254, 255, 255]


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    return __import__(name)


def test_tools_parse_the_new_arguments(capsys):
    rm, em = _tool("render_mesh"), _tool("evaluate_mesh")
    a = rm.parse_args(["m.ply", "--K", "K.npy", "--world-mats", "W.npy", "--resolution", "48", "64", "--out", "d"])
    assert (a.frame, a.smooth, a.colors, a.transform, a.scale_mat, a.resolution) == ("camera", False, False, None, None, [48, 64])
    a = rm.parse_args(["m.ply", "--K", "K.npy", "--world-mats", "W.npy", "--scale-mat", "S.npy", "--resolution", "4", "6",
                       "--out", "d", "--frame", "world", "--smooth", "--colors", "--transform", "T.npy"])
    assert (a.frame, a.smooth, a.colors, a.transform, a.scale_mat) == ("world", True, True, "T.npy", "S.npy")
    with pytest.raises(SystemExit):
        rm.parse_args(["m.ply", "--K", "K.npy", "--world-mats", "W.npy", "--resolution", "4", "6", "--out", "d", "--frame", "x"])
    capsys.readouterr()
    base = ["mesh.ply", "gt.ply", "--threshold", "0.1", "--samples", "10"]
    a = em.parse_args(base)
    assert (a.normals, a.gt_mesh_samples, a.normal_maps_out) == (False, None, None)
    a = em.parse_args(base + ["--normals", "--gt-mesh-samples", "500", "--cull-views", "K.npy", "W.npy", "--cull-resolution",
                              "4", "6", "--normal-maps-out", "n"])
    assert (a.normals, a.gt_mesh_samples, a.normal_maps_out) == (True, 500, "n")
    for extra, msg in ((["--normal-maps-out", "n"], "needs --cull-views"), (["--gt-mesh-samples", "0"], "positive")):
        with pytest.raises(SystemExit) as e:
            em.parse_args(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err


def test_tools_refuse_a_ply_without_what_a_flag_needs(tmp_path):
    from copenerf.mesh import write_ply
    rm, em = _tool("render_mesh"), _tool("evaluate_mesh")
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    n = np.tile(np.array([[0, 0, 1]], dtype=np.float32), (3, 1))
    c = np.full((3, 3), 200, dtype=np.uint8)
    bare, full, cloud = (str(tmp_path / x) for x in ("bare.ply", "full.ply", "cloud.ply"))
    write_ply(bare, v, f)
    write_ply(full, v, f, normals=n, colors=c)
    write_ply(cloud, v, np.zeros((0, 3), dtype=np.int32), normals=n)
    assert [x is None for x in rm.load_mesh(bare)[2:]] == [True, True]
    got = rm.load_mesh(full, smooth=True, colors=True)
    assert np.array_equal(got[2], n) and np.array_equal(got[3], c)
    assert [x is None for x in rm.load_mesh(full)[2:]] == [True, True]  # not asked for: not used
    for kw, msg in ((dict(smooth=True), "--smooth needs vertex normals"), (dict(colors=True), "--colors needs vertex colours")):
        with pytest.raises(SystemExit, match=msg):
            rm.load_mesh(bare, **kw)
    with pytest.raises(SystemExit, match="--normals needs vertex normals"):
        em.load_ground_truth(bare, normals=True)
    pts, tri, nrm = em.load_ground_truth(cloud, normals=True)
    assert tri is None and np.array_equal(nrm, n)
    assert em.load_ground_truth(cloud)[2] is None
    with pytest.raises(SystemExit, match="--gt-mesh-samples needs a mesh"):
        em.load_ground_truth(cloud, normals=True, mesh_samples=10)
    pts, tri, nrm = em.load_ground_truth(bare, normals=True, mesh_samples=10)  # the faces' own normals: none needed
    assert np.array_equal(tri, f) and nrm is None


def test_geometry_from_stats_is_unchanged_and_the_normal_entries_follow():
    from copenerf import metrics
    r = metrics.geometry_from_stats([10, 8, 4.0, 0], [20, 20, 5.0, 0], 3.5)
    assert tuple(r) == metrics.GEOMETRY_KEYS and not set(r) & set(metrics.NORMAL_GEOMETRY_KEYS)
    assert r["accuracy"] == 0.5 and r["completeness"] == 0.25 and r["n_pred_far"] == 2
    n = metrics.normal_geometry_from_stats([8, 6.0, 0], [20, 10.0, 1])
    assert tuple(n) == metrics.NORMAL_GEOMETRY_KEYS
    assert n == {"normal_accuracy": 0.75, "normal_completeness": 0.5, "normal_consistency": 0.625, "n_pred_normal": 8,
                 "n_gt_normal": 20}
    e = metrics.normal_geometry_from_stats([0, 0.0, 3], [0, 0.0, 0])
    assert np.isnan(e["normal_accuracy"]) and np.isnan(e["normal_consistency"]) and e["n_pred_normal"] == 0
    r.update(n)
    assert list(r)[:len(metrics.GEOMETRY_KEYS)] == list(metrics.GEOMETRY_KEYS)  # the normal keys come after the others
