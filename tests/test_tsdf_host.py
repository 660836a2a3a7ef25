"""The references of the TSDF fusion tests against each other, on the CPU: fuse_f32 (the kernel's fp32 operation
order in numpy) against fuse_ref (float64) on every scene the GPU tests use pins F32_WORST -- the GPU bar is four times
it -- and every scene's undecided share; the same for the colour sums and the sampler; the float64 pipeline pins the
end-to-end test's distance bar; isosurface_observed_ref without NaN is mesh_ref.isosurface; and the argument
validation of fusion.TSDFVolume and tools/fuse_depths.py, which needs no device."""
import os
import sys

import numpy as np
import pytest

import mesh_clean_ref as CR
import mesh_ref as MR
import tsdf_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX1 = ((-1.0,) * 3, (1.0,) * 3)


def _scenes():
    for dims, hw in T.SPHERE_CASES:
        yield f"sphere {dims} at {hw}", T.scene_sphere(dims, hw)[:6], {}
    w = T.scene_wall()
    yield "wall", w[:6], {}
    yield "wall with depth_max", w[:6], {"depth_max": w[8]}


def test_fp32_restatement_against_float64_pins_the_gpu_bar():
    worst_all, worst_c = 0.0, 0.0
    for label, args, kw in _scenes():
        col = T.pixel_colors(args[4].shape[0], *args[4].shape[1:])
        ref = T.fuse_ref(*args, color=col, **kw)
        got = T.fuse_f32(*args, color=col, **kw)
        decided, observed = ~ref[3], ref[1] > 0
        share = float((ref[3] & observed).sum()) / int(observed.sum())
        worst = float(np.abs(got[0].astype(np.float64)[decided] - ref[0][decided]).max())
        wc = float(np.abs(got[2].astype(np.float64)[decided] - ref[2][decided]).max())
        print(label, "observed", int(observed.sum()), "undecided share", share, "worst |tsum32 - tsum64|", worst, "csum", wc)
        assert np.array_equal(got[1].astype(np.float64)[decided], ref[1][decided]), label
        assert 0.005 <= share <= 0.03, (label, share)  # measured: 2.4 %, 2.4 %, 2.6 %, 1.2 %, 1.3 %; the GPU cap is 5 %
        assert int(observed.sum()) > 1000  # (the scene is not empty)
        worst_all, worst_c = max(worst_all, worst), max(worst_c, wc)
    # the pins: the measurement lies under the pinned figure and within a fifth of it
    assert 0.8 * T.F32_WORST <= worst_all <= T.F32_WORST, worst_all
    assert 0.8 * T.F32_WORST_CSUM <= worst_c <= T.F32_WORST_CSUM, worst_c
    assert T.EPS_TSUM == 4.0 * T.F32_WORST and T.EPS_CSUM == 4.0 * T.F32_WORST_CSUM


def test_reference_rules_on_the_wall_scene():
    """Free space counts +1, depth_max removes exactly the wall's observations, and pixels that saw nothing (0, +inf,
    NaN) are ignored."""
    dims, lo, hi, P, depth, trunc, ds, dw, dmax = T.scene_wall()
    t, w, _, _ = T.fuse_ref(dims, lo, hi, P, depth, trunc)
    assert w.max() == 3 and (w == 0).any()
    free = t == w  # every observation saturated: in front of everything every observing camera saw
    assert free[w > 0].mean() > 0.3 and (t <= w).all() and (t[w > 0] >= -w[w > 0]).all()
    # the same scene without the wall's pixels is the scene with depth_max
    t2, w2, _, _ = T.fuse_ref(dims, lo, hi, P, depth, trunc, depth_max=dmax)
    t3, w3, _, _ = T.fuse_ref(dims, lo, hi, P, ds, trunc)
    assert np.array_equal(t2, t3) and np.array_equal(w2, w3) and w2.sum() < w.sum()
    for empty in (0.0, np.inf, np.nan):
        d = np.where(np.isfinite(ds), ds, np.float32(empty)).astype(np.float32)
        t4, w4, _, _ = T.fuse_ref(dims, lo, hi, P, d, trunc)
        assert np.array_equal(t4, t3) and np.array_equal(w4, w3), empty


def test_observed_mesher_reference_without_nan_is_the_plain_reference():
    for make in (MR.sphere_soft, MR.two_spheres, MR.torus):
        u = make()
        a, b = MR.isosurface(u, 0.0, *BOX1), T.isosurface_observed_ref(u, 0.0, *BOX1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), make.__name__


@pytest.mark.parametrize("how", ["half", "slab", "random"])
def test_observed_mesher_reference_properties(how):
    for make in (MR.sphere_soft, MR.two_spheres, MR.torus):
        u = T.punch(make(), how)
        v, t = T.isosurface_observed_ref(u, 0.0, *BOX1)
        pv, pt = MR.isosurface(make(), 0.0, *BOX1)
        assert 0 < len(t) < len(pt) and len(v) < len(pv), (make.__name__, how)
        assert np.isfinite(v).all()
        # every vertex is one of the full mesh's (the same edge, the same position), every triangle too
        full = {tuple(r) for r in np.round(pv, 12)}
        assert all(tuple(r) in full for r in np.round(v, 12))
        tri_pos = {tuple(np.round(pv[r], 12).reshape(-1)) for r in pt}
        assert all(tuple(np.round(v[r], 12).reshape(-1)) in tri_pos for r in t)
        if how == "random":
            assert len(v) > len(np.unique(t))  # edges whose every cell was skipped keep their vertex, unreferenced


def test_sampler_restatement_pins_its_bar():
    attr, mask, lo, hi = T.sample_volume()
    pts = T.sample_points(lo, hi, attr.shape[:3])
    worst = 0.0
    for m in (None, mask):
        ref, ws = T.volume_sample_ref(attr, pts, lo, hi, m, fill=-5.0)
        got = T.volume_sample_f32(attr, pts, lo, hi, m, fill=-5.0)
        ok = ws >= T.SAMPLE_MIN_WEIGHT
        assert 1.0 - ok.mean() < T.SAMPLE_LEFT_OUT_CAP
        worst = max(worst, float(np.abs(got.astype(np.float64)[ok] - ref[ok]).max()))
        if m is None:
            np.testing.assert_allclose(ws, 1.0, atol=1e-12)
    print("sampler worst |f32 - f64|", worst)
    assert 0.8 * T.F32_WORST_SAMPLE <= worst <= T.F32_WORST_SAMPLE, worst
    # trilinear interpolation reproduces a linear field, inside and (clamped) on the faces
    x, y, z = np.meshgrid(*T.voxel_axes(attr.shape[:3], lo, hi, np.float64), indexing="ij")
    lin = (0.3 * x - 0.2 * y + 0.5 * z + 0.1).astype(np.float32)
    inside = pts[:700]
    got, _ = T.volume_sample_ref(lin, inside, lo, hi)
    want = 0.3 * inside[:, 0].astype(np.float64) - 0.2 * inside[:, 1] + 0.5 * inside[:, 2] + 0.1
    np.testing.assert_allclose(got[:, 0], want, atol=2e-7)
    un = T.unobserved_points(lo, hi, attr.shape[:3])
    ref, ws = T.volume_sample_ref(attr, un, lo, hi, mask, fill=-5.0)
    assert (ws == 0).all() and (ref == -5.0).all()


def test_float64_pipeline_pins_the_end_to_end_bar():
    dims, lo, hi, P, depth, trunc, _ = T.scene_sphere(*T.SPHERE_CASES[0])
    t, w, _, _ = T.fuse_ref(dims, lo, hi, P, depth, trunc)
    u = np.where(w >= 1, t / np.maximum(w, 1), np.nan).astype(np.float32)
    v, tri = T.isosurface_observed_ref(u, 0.0, lo, hi)
    kept, tri2, _, _ = CR.clean(tri, len(v), False, 1)
    v2 = v[kept]
    assert len(tri2) == len(tri) > 5000 and len(v2) < len(v)
    assert np.array_equal(np.unique(tri2), np.arange(len(v2)))
    worst = float(np.abs(np.linalg.norm(v2, axis=1) - 0.5).max())
    print("float64 pipeline: V", len(v2), "T", len(tri2), "worst distance from the sphere", worst, "bar", T.PIPELINE_BAR)
    assert 0.9 * T.PIPELINE_WORST <= worst <= T.PIPELINE_WORST, worst
    assert T.PIPELINE_BAR == 1.5 * T.PIPELINE_WORST
    assert MR.signed_volume(v2, tri2) > 0  # normals point out of the surface


def test_tsdf_volume_argument_validation():
    from copenerf import fusion
    ok = dict(bound_min=(-1, -1, -1), bound_max=(1, 1, 1), dims=8, trunc=0.1, device="cuda")
    for bad, exc in ((dict(bound_max=(1, -1, 1)), ValueError), (dict(bound_min=(0, 0)), ValueError),
                     (dict(dims=(8, 1, 8)), ValueError), (dict(dims=(8, 8)), ValueError), (dict(dims=(2048,) * 3), ValueError),
                     (dict(trunc=0.0), ValueError), (dict(trunc=float("inf")), ValueError),
                     (dict(device="cpu"), RuntimeError)):  # no CPU fallback
        with pytest.raises(exc):
            fusion.TSDFVolume(**{**ok, **bad})


def test_ops_refuse_cpu_tensors():
    import torch
    from copenerf import ops
    z = torch.zeros(4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsdf_integrate(z, z.clone(), (-1,) * 3, (1,) * 3, torch.zeros(1, 3, 4), torch.zeros(1, 2, 2), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tsdf_finalize(z, z.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.volume_sample(z, torch.zeros(3, 3), (-1,) * 3, (1,) * 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.isosurface(z, 0.0, (-1,) * 3, (1,) * 3, observed=True)


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuse_depths
    return fuse_depths


def test_tool_argument_validation(capsys):
    tool = _tool()
    base = ["out.ply", "--depths", "d", "--K", "k.npy", "--world-mats", "w.npy", "--bound-min", "-1", "-1", "-1",
            "--bound-max", "1", "1", "1"]
    a = tool.parse_args(base + ["--dims", "8", "9", "10"])
    assert a.dims == [8, 9, 10] and a.trunc is None and a.min_weight == 1 and a.views_per_call == 8
    a = tool.parse_args(base + ["--voxel-size", "0.25"])
    assert a.dims == [9, 9, 9]
    for bad in (["--dims", "8", "1", "8"], ["--dims", "8", "8", "8", "--voxel-size", "0.1"], [], ["--voxel-size", "0"],
                ["--dims", "8", "8", "8", "--trunc", "-1"], ["--dims", "8", "8", "8", "--min-weight", "0"],
                ["--dims", "8", "8", "8", "--depth-max", "0"], ["--dims", "2048", "2048", "2048"],
                ["--dims", "8", "8", "8", "--views-per-call", "0"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
    with pytest.raises(SystemExit):
        tool.parse_args(["out.ply", "--depths", "d", "--K", "k.npy", "--world-mats", "w.npy", "--bound-min", "1", "-1", "-1",
                         "--bound-max", "1", "1", "1", "--dims", "8", "8", "8"])
    capsys.readouterr()


def test_tool_loads_depth_trees_and_views(tmp_path):
    tool = _tool()
    d = np.arange(3 * 4 * 5, dtype=np.float32).reshape(3, 4, 5)
    tree = tmp_path / "depths"
    tree.mkdir()
    for i, m in enumerate(d):
        np.savez(tree / ("depth_%06d.npz" % i), pred=m)
    np.save(tmp_path / "depths.npy", d)
    assert np.array_equal(tool.load_depths(str(tree)), d) and np.array_equal(tool.load_depths(str(tmp_path / "depths.npy")), d)
    np.save(tmp_path / "flat.npy", d[0])
    with pytest.raises(SystemExit, match="depth maps"):
        tool.load_depths(str(tmp_path / "flat.npy"))
    K, W = np.diag([1.0, -1.0, -1.0, 1.0]), np.stack([np.eye(4)] * 3)
    np.save(tmp_path / "K.npy", K)
    np.save(tmp_path / "W.npy", W)
    views = tool.load_views(str(tmp_path / "K.npy"), str(tmp_path / "W.npy"), None, 3)
    assert len(views) == 3 and np.array_equal(views[2]["camera_mat"], K) and "scale_mat" not in views[0]
    with pytest.raises(SystemExit, match="world-to-camera"):
        tool.load_views(str(tmp_path / "K.npy"), str(tmp_path / "W.npy"), None, 4)
    np.save(tmp_path / "S.npy", np.stack([np.eye(4)] * 2))
    with pytest.raises(SystemExit, match="S.npy"):
        tool.load_views(str(tmp_path / "K.npy"), str(tmp_path / "W.npy"), str(tmp_path / "S.npy"), 3)
