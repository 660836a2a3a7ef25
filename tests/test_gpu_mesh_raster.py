"""cn_mesh_raster, cn_mesh_visibility, cn_mesh_select_mask and what is built on them (mesh.render_mesh_depth,
mesh.cull_mesh, metrics.mesh_geometry_metrics' cull_* keywords, tools/evaluate_mesh.py's --cull-views) against the
float64 restatement tests/mesh_raster_ref.py.

At decided pixels (edge margin above 1e-3 pixels) coverage and triangle ids equal the reference's exactly; the depth
is within EPS_DEPTH = 4.16e-6 relative: four times the 1.04e-6 (17.4 x 2^-24) that the kernel's fp32 operation order,
restated in numpy float32, shows against the float64 reference on these very scenes (measured on the CPU by
tests/test_mesh_raster_host.py, which pins it).  At most 3 % of a view's covered pixels may be undecided (the
reference alone leaves out 1.7 % on scene_thread, 0.7 % on scene_group).  Visibility counts are exact at decided
points, culls exact where every vertex is stable (asserted).  Determinism is bitwise."""
import os
import sys

import numpy as np
import pytest
import torch

import mesh_raster_ref as R
from mesh_eval_ref import brute_nn, geometry_ref, icosphere

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 1e-4


def _proj(views, h, w, transform=None):
    from copenerf.mesh import camera_projection
    return np.stack([camera_projection(v["camera_mat"], v["world_mat"], v.get("scale_mat"), (h, w), transform)
                     for v in views])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _raster(v, f, P, h, w, **kw):
    from copenerf import ops
    depth, tri = ops.mesh_raster(_t(v), _t(f), _t(P), h, w, near=NEAR, **kw)
    return depth.cpu().numpy(), tri.cpu().numpy()


def _check_views(v, f, P, h, w, got, cap=0.03):
    worst = 0.0
    for i in range(len(P)):
        ref = R.raster_ref(v, f, P[i], h, w, NEAR)
        err, left = R.compare_view(got[0][i], got[1][i], ref, cap=cap)
        print("view %d: worst relative depth error %.3e, undecided share %.4f" % (i, err, left))
        worst = max(worst, err)
    return worst


# a pinhole looking down +z: pixel = 10 (x, y) / z + centre
def _pinhole(h, w, f=10.0):
    return np.array([[[f, 0, 0.5 * (w - 1), 0], [0, f, 0.5 * (h - 1), 0], [0, 0, 1, 0]]], dtype=np.float32)


def test_edge_shapes():
    P = _pinhole(8, 8)
    v = np.array([[-0.3, -0.25, 1.0], [0.32, -0.2, 1.0], [0.05, 0.33, 1.0]], dtype=np.float32)
    for vv, ff in ((v, np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))):
        depth, tri = _raster(vv, ff, P, 8, 8)  # T = 0 (and V = 0): all background
        assert depth.shape == (1, 8, 8) and np.all(np.isinf(depth)) and np.all(depth > 0) and np.all(tri == -1)
    one = np.array([[0, 1, 2]], dtype=np.int32)
    stats = {}
    depth, tri = _raster(v, one, P, 8, 8, stats=stats)
    ref = R.raster_ref(v, one, P[0], 8, 8, NEAR)
    assert (ref[2] > R.DELTA).all() and (ref[1] >= 0).sum() >= 10
    assert np.array_equal(tri[0], ref[1])
    assert np.all(depth[0][ref[1] >= 0] == 1.0) and np.all(np.isinf(depth[0][ref[1] < 0]))  # a plane at c = 1: exact
    assert stats == {"thread_pairs": 1, "group_pairs": 0}
    assert np.array_equal(_raster(v, one[:, ::-1].copy(), P, 8, 8)[1], tri)  # two-sided: the other winding covers the same
    # sizes that are multiples of nothing, more than one block of triangles; an out-of-range index (either side) and
    # a degenerate triangle are skipped: the images are those of the list without them
    sv, sf = icosphere(2, 0.5)
    extra = np.array([[0, 1, len(sv)], [-1, 2, 3], [5, 5, 7], [2 ** 31 - 1, 0, 1]], dtype=np.int32)
    for (h, w), views in (((64, 96), R.three_views(64, 96)), ((23, 37), R.three_views(23, 37)[:2])):
        Pv = _proj(views, h, w)
        got = _raster(sv, sf, Pv, h, w)
        _check_views(sv, sf, Pv, h, w, got, cap=1.0)  # (these sizes are about shapes: no cap on the undecided share)
        assert (got[1] >= 0).any() and (got[1] < 0).any()
        mixed = np.concatenate([extra[:2], sf, extra[2:]])
        d2, t2 = _raster(sv, mixed, Pv, h, w)
        assert np.array_equal(d2, got[0]) and np.array_equal(np.where(t2 >= 0, t2 - 2, -1), got[1])


def test_thread_path_icosphere():
    v, f, views, h, w = R.scene_thread()
    P = _proj(views, h, w)
    stats = {}
    got = _raster(v, f, P, h, w, stats=stats)  # N = 3 in one call
    worst = _check_views(v, f, P, h, w, got)
    assert worst <= R.EPS_DEPTH
    assert stats["group_pairs"] == 0 and 0 < stats["thread_pairs"] <= 3 * len(f)


def test_workgroup_path_quads_sphere_and_straddler():
    v, f, views, h, w, straddler = R.scene_group()
    P = _proj(views, h, w)
    stats = {}
    got = _raster(v, f, P, h, w, stats=stats)
    worst = _check_views(v, f, P, h, w, got)
    assert worst <= R.EPS_DEPTH
    assert stats["group_pairs"] == 12 and stats["thread_pairs"] > 100  # the four large triangles in three views; the sphere
    assert not np.any(got[1] == straddler)  # a corner behind the camera: skipped whole, no trace
    assert np.mean(got[1] < 4) > 0.5 and np.mean(got[1] >= 4) > 0.1
    # a budget no box exceeds / every box exceeds: one path alone gives the same images, bit for bit
    for budget, key in ((h * w, "group_pairs"), (1, None)):
        s2 = {}
        again = _raster(v, f, P, h, w, pixel_budget=budget, stats=s2)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])
        assert s2["group_pairs"] == 0 if key else s2["group_pairs"] > 100


def _grid_mesh(n=40, half=3.0, jitter=0.3, seed=3):
    """A jittered n x n planar grid of quads (two triangles each, the diagonal alternating), tilted against the
    camera of _grid_view, reaching past the image on every side."""
    rng = np.random.default_rng(seed)
    g = np.linspace(-half, half, n + 1)
    y, z = np.meshgrid(g, g, indexing="ij")
    step = 2 * half / n
    y = y + rng.uniform(-jitter, jitter, y.shape) * step
    z = z + rng.uniform(-jitter, jitter, z.shape) * step
    v = np.stack([0.3 * y + 0.2 * z, y, z], -1).reshape(-1, 3).astype(np.float32)
    tris = []
    for i in range(n):
        for j in range(n):
            q = i * (n + 1) + j
            a, b, c, d = q, q + 1, q + n + 2, q + n + 1
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 else [(a, b, d), (b, c, d)]
    return v, np.array(tris, dtype=np.int32)


def test_no_cracks_on_a_jittered_grid():
    v, f = _grid_mesh()
    h, w = 64, 96
    P = _proj([R.make_view((2.0, 0.1, -0.05), (0.0, 0.0, 0.0), 0.9 * h, h, w)], h, w)
    sx, sy, c = R.project64(P[0], v)
    assert c.min() > 0.3 and sx.min() < -5 and sx.max() > w + 5 and sy.min() < -5 and sy.max() > h + 5
    stats = {}
    depth, tri = _raster(v, f, P, h, w, stats=stats)
    assert np.all(tri >= 0) and np.all(np.isfinite(depth))  # every pixel, no exclusion: the canonical edge order
    assert stats["thread_pairs"] > 0 and stats["group_pairs"] > 0  # the near triangles are large: both paths meet
    _check_views(v, f, P, h, w, (depth, tri), cap=1.0)
    # in random vertex order (other triangles run each shared edge from the larger index) it stays closed
    perm = np.random.default_rng(1).permutation(len(v))
    inv = np.argsort(perm)
    assert np.all(_raster(v[perm], inv[f].astype(np.int32), P, h, w)[1] >= 0)


def test_determinism_batches_and_ties():
    v, f, views, h, w, _ = R.scene_group()
    P = _proj(views, h, w)
    a = _raster(v, f, P, h, w)
    b = _raster(v, f, P, h, w)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])  # bitwise (inf == inf)
    singles = [_raster(v, f, P[i:i + 1], h, w) for i in range(3)]
    assert np.array_equal(np.concatenate([s[0] for s in singles]), a[0])
    assert np.array_equal(np.concatenate([s[1] for s in singles]), a[1])
    for batch in (1, 2):  # a batch that divides N and one that leaves a remainder
        c = _raster(v, f, P, h, w, view_batch=batch)
        assert np.array_equal(c[0], a[0]) and np.array_equal(c[1], a[1])
    twice = _raster(v, np.concatenate([f, f]), P, h, w)  # every fragment ties with its copy: the smaller id wins
    assert twice[1].max() < len(f) and np.array_equal(twice[1], a[1]) and np.array_equal(twice[0], a[0])


_CULL = {}


def _cull_scene():
    """scene_cull, the device's depth maps of it, and the reference's visibility for them (computed once)."""
    if not _CULL:
        from copenerf import ops
        v, f, views, h, w = R.scene_cull()
        P = _proj(views, h, w)
        tv, tf, tP = _t(v), _t(f), _t(P)
        depth, _ = ops.mesh_raster(tv, tf, tP, h, w, near=NEAR)
        _CULL.update(v=v, f=f, views=views, h=h, w=w, P=P, tv=tv, tf=tf, tP=tP, depth=depth,
                     ref=R.visibility_ref(v, P, h, w, depth.cpu().numpy(), tol_abs=R.CULL_TOL_ABS, near=NEAR))
    return _CULL


def _cull_ref(f, keep):
    """(kept vertex ids, kept triangle ids, the kept triangles renumbered) for a per-vertex keep mask."""
    tk = np.all(keep[f], axis=1)
    return np.nonzero(keep)[0], np.nonzero(tk)[0], (np.cumsum(keep) - 1)[f[tk]]


def test_visibility_counts():
    from copenerf import ops
    s = _cull_scene()
    h, w = s["h"], s["w"]
    count, decided, _ = s["ref"]
    got = ops.mesh_visibility(s["tv"], s["tP"], h, w, depth=s["depth"], tol_abs=R.CULL_TOL_ABS, near=NEAR).cpu().numpy()
    print("undecided share %.4f" % (1 - decided.mean()))
    assert 1 - decided.mean() <= 0.03 and np.array_equal(got[decided], count[decided])
    assert got.min() == 0 and got.max() == 3 and np.abs(got - count).max() <= 1
    # the frustum test alone, on the vertices and on a cloud of 20000 points that reaches behind the cameras
    pts = np.random.default_rng(2).uniform(-3.0, 3.0, (20000, 3)).astype(np.float32)
    for p, tp in ((s["v"], s["tv"]), (pts, _t(pts))):
        count, decided, _ = R.visibility_ref(p, s["P"], h, w, near=NEAR)
        got = ops.mesh_visibility(tp, s["tP"], h, w, near=NEAR).cpu().numpy()
        assert 1 - decided.mean() <= 0.03 and np.array_equal(got[decided], count[decided])
        assert got.min() == 0 and got.max() == 3
    # a tolerance moves the bound: with none, fewer vertices pass than with CULL_TOL_ABS; a relative one likewise
    none = ops.mesh_visibility(s["tv"], s["tP"], h, w, depth=s["depth"], near=NEAR).cpu().numpy()
    rel = ops.mesh_visibility(s["tv"], s["tP"], h, w, depth=s["depth"], tol_rel=0.03, near=NEAR).cpu().numpy()
    want, dec, _ = R.visibility_ref(s["v"], s["P"], h, w, s["depth"].cpu().numpy(), tol_rel=0.03, near=NEAR)
    assert np.array_equal(rel[dec], want[dec]) and none.sum() < rel.sum()
    assert ops.mesh_visibility(s["tv"][:0], s["tP"], h, w).shape == (0,)
    assert torch.equal(ops.mesh_visibility(s["tv"], s["tP"][:0], h, w), torch.zeros(len(s["v"]), dtype=torch.int32, device=DEV))


def test_cull_mesh_against_reference():
    from copenerf import mesh, ops
    s = _cull_scene()
    count, _, stable = s["ref"]
    assert stable.all()  # CULL_TOL_ABS and the cameras leave no vertex's outcome to rounding
    for m in (1, 2):
        keep = count >= m
        kv, kt, tris = _cull_ref(s["f"], keep)
        assert 0 < len(kt) < len(s["f"])
        cv, cf, kept = mesh.cull_mesh(s["tv"], s["tf"], s["views"], (s["h"], s["w"]), min_views=m, tol_abs=R.CULL_TOL_ABS,
                                      tol_rel=0.0, near=NEAR)
        assert kept.dtype == torch.int32 and cf.dtype == torch.int32
        assert np.array_equal(kept.cpu().numpy(), kv) and np.array_equal(cf.cpu().numpy(), tris)
        assert np.array_equal(cv.cpu().numpy(), s["v"][kv])
    # ops.mesh_cull with masks of either type, none kept and all kept
    keep = torch.from_numpy(count >= 1).to(DEV)
    a, b = ops.mesh_cull(s["tv"], s["tf"], keep), ops.mesh_cull(s["tv"], s["tf"], keep.to(torch.uint8) * 7)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ev, ef, ek = ops.mesh_cull(s["tv"], s["tf"], torch.zeros_like(keep))
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ek.shape == (0,)
    fv, ff, fk = ops.mesh_cull(s["tv"], s["tf"], torch.ones_like(keep))
    assert torch.equal(fv, s["tv"]) and torch.equal(ff, s["tf"]) and torch.equal(fk.long(), torch.arange(len(s["v"]), device=DEV))
    # a view that sees nothing of the mesh: an empty mesh, no error
    sv, sf = icosphere(2, 0.5)
    away = [R.make_view((1.8, 0.3, 0.4), (4.0, 0.3, 0.4), 0.9 * 64, 64, 96)]
    ev, ef, ek = mesh.cull_mesh(_t(sv), _t(sf), away, (64, 96))
    assert ev.shape == (0, 3) and ef.shape == (0, 3) and ek.shape == (0,)
    out = mesh.render_mesh_depth(_t(sv), _t(sf), away, (64, 96))
    assert torch.isinf(out["depth"]).all() and (out["tri"] == -1).all()


def _gt_cloud(n=3000, radius=0.52):
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    phi = np.pi * (1 + 5 ** 0.5) * k
    r = np.sqrt(1 - z * z)
    return (radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)).astype(np.float32)


KEYS = ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore", "n_pred", "n_gt", "n_pred_far",
        "n_gt_far", "area")
S, SEED, TAU = 8000, 11, 0.05


def _e2e():
    """The icosphere and a smaller duplicate on its far side, hidden from the three side cameras: only the hemisphere
    they do not see would expose it."""
    sv, sf = icosphere(3, 0.5)
    v, f = R.merge((sv, sf), (0.6 * sv + np.float32([-1.2, 0.0, 0.0]), sf))
    _, _, views, h, w = R.scene_cull()
    return v, f, views, h, w


def _compare(got, want):
    assert tuple(got) == KEYS
    for k in ("n_pred", "n_gt", "n_pred_far", "n_gt_far"):
        assert got[k] == want[k], k
    for k in ("accuracy", "completeness", "chamfer"):
        assert got[k] == pytest.approx(want[k], rel=1e-6), k
    for k in ("precision", "recall", "fscore"):
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), k


def test_geometry_metrics_with_view_culling():
    from copenerf import metrics, ops
    v, f, views, h, w = _e2e()
    gt = _gt_cloud()
    tv, tf, tgt = _t(v), _t(f), _t(gt)
    P = _proj(views, h, w)
    kw = dict(threshold=TAU, n_samples=S, seed=SEED)
    # without the new keywords: bitwise what the unchanged passes give when composed as before
    handle, area = ops.mesh_area(tv, tf)
    samples, _ = ops.mesh_sample(handle, S, torch.tensor([SEED, 0], dtype=torch.uint64, device=DEV))
    sides = torch.stack([metrics._cloud_side(samples, tgt, TAU, float("inf"), None, None),
                         metrics._cloud_side(tgt, samples, TAU, float("inf"), None, None)]).tolist()
    plain = metrics.mesh_geometry_metrics(tv, tf, tgt, **kw)
    assert plain == metrics.geometry_from_stats(sides[0], sides[1], float(area.item()))
    assert plain == metrics.mesh_geometry_metrics(tv, tf, tgt, cull_views=None, cull_resolution=None, cull_gt=False, **kw)
    # culled: the reference's cull of the same mesh (from the device's depth maps), sampled by the device sampler,
    # measured in float64
    depth, _ = ops.mesh_raster(tv, tf, _t(P), h, w, near=ops.MESH_NEAR)
    count, _, stable = R.visibility_ref(v, P, h, w, depth.cpu().numpy(), tol_abs=R.CULL_TOL_ABS, near=ops.MESH_NEAR)
    assert stable.all()
    kv, kt, tris = _cull_ref(f, count >= 1)
    assert len(kt) < 0.6 * len(f) and not np.any(kv >= len(v) // 2)  # the far hemisphere and the whole duplicate go
    cull = dict(cull_views=views, cull_resolution=(h, w), cull_tol_abs=R.CULL_TOL_ABS, cull_tol_rel=0.0)
    got = metrics.mesh_geometry_metrics(tv, tf, tgt, **kw, **cull)
    handle, area = ops.mesh_area(_t(v[kv]), _t(tris.astype(np.int32)))
    samples = ops.mesh_sample(handle, S, torch.tensor([SEED, 0], dtype=torch.uint64, device=DEV))[0].cpu().numpy()
    dists = (brute_nn(samples, gt)[0], brute_nn(gt, samples)[0])
    for d in dists:  # no float64 distance within the fp32 bound of the threshold: the counts are decided
        assert np.all(np.abs(d - TAU) > 1e-6 * d)
    want = geometry_ref(samples, gt, TAU, area=area.item(), dists=dists)
    print(got)
    _compare(got, want)
    assert got["area"] == area.item() and got["n_pred"] == S and got["area"] < 0.5 * plain["area"]
    assert got["accuracy"] < 0.5 * plain["accuracy"]  # the hidden duplicate no longer counts against accuracy
    # cull_gt: the ground-truth points outside every frustum go too (here none is: the sphere is in all three)
    cnt, dec, _ = R.visibility_ref(gt, P, h, w, near=ops.MESH_NEAR)
    both = metrics.mesh_geometry_metrics(tv, tf, tgt, cull_gt=True, **kw, **cull)
    assert int(((cnt > 0) & dec).sum()) <= both["n_gt"] <= int(((cnt > 0) | ~dec).sum())
    far = np.concatenate([gt, gt + np.float32([0.0, 6.0, 0.0])])  # a copy outside every frustum
    assert metrics.mesh_geometry_metrics(tv, tf, _t(far), cull_gt=True, **kw, **cull) == both
    with pytest.raises(ValueError, match="together"):
        metrics.mesh_geometry_metrics(tv, tf, tgt, cull_views=views, **kw)
    with pytest.raises(ValueError, match="cull_gt"):
        metrics.mesh_geometry_metrics(tv, tf, tgt, cull_gt=True, **kw)


def test_evaluate_mesh_tool_with_view_culling(tmp_path):
    from copenerf import mesh, metrics
    from copenerf.pose_refine import load_depth_dir
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_mesh
    v, f, views, h, w = _e2e()
    gt = _gt_cloud()
    tv, tf = _t(v), _t(f)
    paths = {k: str(tmp_path / k) for k in ("mesh.ply", "gt.ply", "K.npy", "W.npy", "culled.ply", "depths", "results.txt")}
    mesh.write_ply(paths["mesh.ply"], v, f)
    mesh.write_ply(paths["gt.ply"], gt, np.zeros((0, 3), dtype=np.int32))
    np.save(paths["K.npy"], views[0]["camera_mat"])  # one camera matrix for all views
    np.save(paths["W.npy"], np.stack([x["world_mat"] for x in views]))
    res = evaluate_mesh.main([paths["mesh.ply"], paths["gt.ply"], "--threshold", str(TAU), "--samples", str(S), "--seed", str(SEED),
                              "--cull-views", paths["K.npy"], paths["W.npy"], "--cull-resolution", str(h), str(w),
                              "--cull-tol-abs", str(R.CULL_TOL_ABS), "--cull-tol-rel", "0", "--cull-min-views", "2",
                              "--depths-out", paths["depths"], "--culled-out", paths["culled.ply"], "--out", paths["results.txt"]])
    want = metrics.mesh_geometry_metrics(tv, tf, _t(gt), threshold=TAU, n_samples=S, seed=SEED, cull_views=views,
                                         cull_resolution=(h, w), cull_min_views=2, cull_tol_abs=R.CULL_TOL_ABS, cull_tol_rel=0.0)
    assert res == want
    assert [line.split(": ")[0] for line in open(paths["results.txt"]).read().splitlines()] == list(KEYS)
    cv, cf, _ = mesh.cull_mesh(tv, tf, views, (h, w), min_views=2, tol_abs=R.CULL_TOL_ABS, tol_rel=0.0)
    pv, pf, _, _ = mesh.read_ply(paths["culled.ply"])
    assert np.array_equal(pv, cv.cpu().numpy()) and np.array_equal(pf, cf.cpu().numpy()) and 0 < len(pf) < len(f)
    depth = mesh.render_mesh_depth(tv, tf, views, (h, w))["depth"].cpu().numpy()
    files = load_depth_dir(paths["depths"])
    assert sorted(os.listdir(paths["depths"])) == ["depth_%06d.npz" % i for i in range(3)]
    assert files.dtype == np.float32 and np.array_equal(files, np.where(np.isinf(depth), np.float32(0), depth))
    assert (files == 0).any() and (files > 1).any()
