"""TSDF fusion on the device: cn_tsdf_integrate / cn_tsdf_finalize / cn_volume_sample against the float64
restatements of tests/tsdf_ref.py, fusion.TSDFVolume end to end, and tools/fuse_depths.py.

Bars (tests/tsdf_ref.py, measured and pinned by tests/test_tsdf_host.py).  At decided voxels wsum is exact and
|tsum - ref| <= EPS_TSUM = 4 x the fp32 restatement's worst error; at most 5 % of the voxels any view observes may be
undecided (a pixel coordinate within 1e-3 px of a rounding boundary, c within 1e-5 of near, s within 1e-5 of -trunc).
csum and the sampler: 4 x their restatements' errors.  Splits, repeats and finalize: bitwise."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import mesh_clean_ref as CR
import tsdf_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _integrate(dims, lo, hi, P, depth, trunc, color=None, split=None, **kw):
    """(tsum, wsum, csum) device tensors from zero volumes; split: the sizes of the calls the views go in by."""
    from copenerf import ops
    tsum, wsum = torch.zeros(dims, device=DEV), torch.zeros(dims, device=DEV)
    csum = torch.zeros(tuple(dims) + (3,), device=DEV) if color is not None else None
    Pd, dd, cd = _dev(P), _dev(depth), _dev(color)
    v0 = 0
    for n in split or (len(P),):
        sl = slice(v0, v0 + n)
        ops.tsdf_integrate(tsum, wsum, lo, hi, Pd[sl].contiguous(), dd[sl].contiguous(), trunc, csum=csum,
                           color=None if cd is None else cd[sl].contiguous(), **kw)
        v0 += n
    assert v0 == len(P)
    return tsum, wsum, csum


@functools.lru_cache(maxsize=None)
def _sphere(i):
    """Scene i of SPHERE_CASES with its colours and its float64 reference, computed once and left unchanged."""
    scene = T.scene_sphere(*T.SPHERE_CASES[i])
    col = T.pixel_colors(6, *T.SPHERE_CASES[i][1])
    return scene, col, T.fuse_ref(*scene[:6], color=col)


@functools.lru_cache(maxsize=None)
def _wall():
    return T.scene_wall()


@pytest.mark.parametrize("case", range(len(T.SPHERE_CASES)))
def test_sphere_six_views_against_float64(case):
    scene, col, ref = _sphere(case)
    tsum, wsum, csum = _integrate(*scene[:6], color=col)
    T.compare_fusion(tsum.cpu().numpy(), wsum.cpu().numpy(), ref)
    decided = ~ref[3]
    worst_c = float(np.abs(csum.cpu().numpy().astype(np.float64)[decided] - ref[2][decided]).max())
    print("worst |csum - ref|", worst_c, "bar", T.EPS_CSUM)
    assert worst_c <= T.EPS_CSUM, worst_c
    # without colours: the same tsum and wsum, bitwise (the other kernel instance)
    t2, w2, _ = _integrate(*scene[:6])
    assert torch.equal(t2, tsum) and torch.equal(w2, wsum)
    # the brick rejection changes nothing
    t3, w3, c3 = _integrate(*scene[:6], color=col, brick_reject=False)
    assert torch.equal(t3, tsum) and torch.equal(w3, wsum) and torch.equal(c3, csum)


def test_splits_and_repeats_are_bitwise_and_no_views_is_a_no_op():
    from copenerf import ops
    scene, col, _ = _sphere(1)  # the odd-sized grid: the last wavefront is ragged
    one = _integrate(*scene[:6], color=col)
    assert float(one[1].max()) >= 3
    for split in ((3, 3), (1,) * 6, (6,), (2, 4)):
        got = _integrate(*scene[:6], color=col, split=split)
        for a, b in zip(one, got):
            assert torch.equal(a, b), split
    before = [t.clone() for t in one]
    dims, lo, hi, P, depth, trunc = scene[:6]
    ops.tsdf_integrate(one[0], one[1], lo, hi, torch.zeros(0, 3, 4, device=DEV), torch.zeros(0, *depth.shape[1:], device=DEV),
                       trunc, csum=one[2], color=torch.zeros(0, *depth.shape[1:], 3, device=DEV))
    for a, b in zip(one, before):
        assert torch.equal(a, b)


def test_sphere_in_front_of_a_wall():
    dims, lo, hi, P, depth, trunc, ds, dw, dmax = _wall()
    ref = T.fuse_ref(dims, lo, hi, P, depth, trunc)
    tsum, wsum, _ = _integrate(dims, lo, hi, P, depth, trunc)
    T.compare_fusion(tsum.cpu().numpy(), wsum.cpu().numpy(), ref)
    # free space: every observation saturated at +1, bitwise
    t, w = tsum.cpu().numpy(), wsum.cpu().numpy()
    free = (ref[0] == ref[1]) & (ref[1] > 0) & ~ref[3]
    assert free.sum() > 1000 and np.array_equal(t[free], w[free])
    # depth_max between sphere and wall removes the wall's observations exactly: the scene without the wall
    cut = _integrate(dims, lo, hi, P, depth, trunc, depth_max=dmax)
    only = _integrate(dims, lo, hi, P, ds, trunc)
    assert torch.equal(cut[0], only[0]) and torch.equal(cut[1], only[1])
    assert float(only[1].sum()) < float(wsum.sum())
    T.compare_fusion(cut[0].cpu().numpy(), cut[1].cpu().numpy(), T.fuse_ref(dims, lo, hi, P, depth, trunc, depth_max=dmax))
    # pixels set to 0, +inf and NaN are ignored (ds holds +inf off the sphere)
    for empty in (0.0, float("nan")):
        d = np.where(np.isfinite(ds), ds, np.float32(empty)).astype(np.float32)
        got = _integrate(dims, lo, hi, P, d, trunc)
        assert torch.equal(got[0], only[0]) and torch.equal(got[1], only[1]), empty
    # a view with the whole grid behind it changes nothing: the first camera turned round at its place
    flip = np.array(P[:1])
    flip[0, 2] *= -1.0
    P4, d4 = np.concatenate([P, flip]), np.concatenate([depth, np.ones_like(depth[:1])])
    got = _integrate(dims, lo, hi, P4, d4, trunc)
    assert torch.equal(got[0], tsum) and torch.equal(got[1], wsum)
    got = _integrate(dims, lo, hi, P4, d4, trunc, brick_reject=False)
    assert torch.equal(got[0], tsum) and torch.equal(got[1], wsum)


@pytest.mark.parametrize("min_weight", [1, 3])
def test_finalize_is_bitwise_the_division(min_weight):
    from copenerf import ops
    scene, col, _ = _sphere(1)
    tsum, wsum, csum = _integrate(*scene[:6], color=col)
    u, rgb = ops.tsdf_finalize(tsum, wsum, csum, min_weight)
    seen = wsum >= min_weight
    assert 0 < int(seen.sum()) < seen.numel()
    assert torch.equal(u[seen], (tsum / wsum)[seen]) and bool(torch.isnan(u[~seen]).all())
    assert torch.equal(rgb[seen], (csum / wsum[..., None])[seen]) and bool((rgb[~seen] == 0).all())
    u2 = ops.tsdf_finalize(tsum, wsum, None, min_weight)
    assert torch.equal(torch.nan_to_num(u2, nan=7.0), torch.nan_to_num(u, nan=7.0))


def test_volume_sample_against_float64():
    from copenerf import ops
    attr, mask, lo, hi = T.sample_volume()
    pts = T.sample_points(lo, hi, attr.shape[:3])
    ad, md, pd = _dev(attr), _dev(mask), _dev(pts)
    for m, mdev in ((None, None), (mask, md)):
        ref, ws = T.volume_sample_ref(attr, pts, lo, hi, m, fill=-5.0)
        got = ops.volume_sample(ad, pd, lo, hi, mask=mdev, fill=-5.0).cpu().numpy()
        ok = ws >= T.SAMPLE_MIN_WEIGHT
        left_out = 1.0 - float(ok.mean())
        err = float(np.abs(got.astype(np.float64)[ok] - ref[ok]).max())
        print("volume_sample", "masked" if m is not None else "plain", "worst error", err, "bar", T.EPS_SAMPLE, "left out", left_out)
        assert left_out < T.SAMPLE_LEFT_OUT_CAP
        assert err <= T.EPS_SAMPLE, err
    # one channel, given as [nx, ny, nz], and four
    for a in (attr[..., 0].copy(), np.concatenate([attr, attr[..., :1]], -1)):
        ref, _ = T.volume_sample_ref(a, pts, lo, hi)
        got = ops.volume_sample(_dev(a), pd, lo, hi).cpu().numpy()
        assert got.shape == ref.shape and float(np.abs(got - ref).max()) <= T.EPS_SAMPLE
    # a point with no observed corner gets `fill`
    un = _dev(T.unobserved_points(lo, hi, attr.shape[:3]))
    got = ops.volume_sample(ad, un, lo, hi, mask=md, fill=-5.0)
    assert got.shape == (un.shape[0], 3) and bool((got == -5.0).all())
    assert ops.volume_sample(ad, pd[:0], lo, hi).shape == (0, 3)


@functools.lru_cache(maxsize=None)
def _fused():
    """TSDFVolume on the first sphere scene with colours: (volume, scene, colours)."""
    from copenerf import fusion
    scene, col, _ = _sphere(0)
    dims, lo, hi, P, depth, trunc, views = scene
    vol = fusion.TSDFVolume(lo, hi, dims, trunc, DEV, with_colors=True)
    vol.integrate(depth, views, colors=_dev(col), views_per_call=4)  # numpy depths, device colours, two calls
    return vol, scene, col


def test_tsdf_volume_end_to_end():
    from copenerf import ops
    vol, scene, col = _fused()
    dims, lo, hi, P, depth, trunc, views = scene
    # the volume is the kernel's (view_projections gives the restated projections)
    tsum, wsum, csum = _integrate(dims, lo, hi, P, depth, trunc, color=col)
    assert torch.equal(vol.tsum, tsum) and torch.equal(vol.wsum, wsum) and torch.equal(vol.csum, csum)
    stats = {}
    v, t, c = vol.extract_mesh(with_colors=True, stats=stats)
    assert v.dtype == np.float32 and t.dtype == np.int32 and c.dtype == np.uint8 and c.shape == v.shape
    assert len(t) > 5000 and t.min() == 0 and t.max() == len(v) - 1
    assert np.array_equal(np.unique(t), np.arange(len(v)))  # every vertex is referenced
    assert stats["vertices_emitted"] > len(v)                # ... and some that were not have gone
    # the mesh is the reference mesher's on the GPU's own volume, then the reference clean
    u, rgb = vol.volume()
    rv, rt = T.isosurface_observed_ref(u.cpu().numpy(), 0.0, lo, hi)
    kept, rt2, _, _ = CR.clean(rt, len(rv), False, 1)
    assert np.array_equal(t, rt2) and v.shape == (len(kept), 3)
    err = float(np.abs(v.astype(np.float64) - rv[kept]).max())
    assert err <= 2e-6 * 0.8, err  # test_gpu_mesh.py's bar: 2e-6 x the largest |bound|
    worst = float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 0.5).max())
    print("end to end: V", len(v), "T", len(t), "worst distance from the sphere", worst, "reference pipeline",
          T.PIPELINE_WORST, "bar", T.PIPELINE_BAR)
    assert worst <= T.PIPELINE_BAR, worst
    # colours: the sampler on the fused colour volume, packed
    want = ops.rgb8_pack(ops.volume_sample(rgb, _dev(v), lo, hi, mask=u)).cpu().numpy()
    assert np.array_equal(c, want) and c.max() > 100
    # keep_largest / min_triangles go through, and without colours the geometry is the same
    v1, t1 = vol.extract_mesh(keep_largest=True)
    assert len(t1) <= len(t) and np.array_equal(np.unique(t1), np.arange(len(v1)))
    v2, t2 = vol.extract_mesh(min_weight=2)
    assert 0 < len(t2) < len(t)
    with pytest.raises(ValueError, match="with_colors"):
        vol.integrate(depth, views)


def test_tool_writes_the_library_calls_mesh(tmp_path, capsys):
    from copenerf import mesh, metrics
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuse_depths
    scene, col, _ = _sphere(0)
    dims, lo, hi, P, depth, trunc, views = scene
    tree = tmp_path / "depths"
    tree.mkdir()
    for i, d in enumerate(depth):
        np.savez(tree / ("depth_%06d.npz" % i), pred=np.where(np.isfinite(d), d, 0.0).astype(np.float32))
    np.save(tmp_path / "K.npy", np.stack([v["camera_mat"] for v in views]))
    np.save(tmp_path / "W.npy", np.stack([v["world_mat"] for v in views]))
    np.save(tmp_path / "imgs.npy", col)
    out = str(tmp_path / "fused.ply")
    got = fuse_depths.main([out, "--depths", str(tree), "--K", str(tmp_path / "K.npy"), "--world-mats", str(tmp_path / "W.npy"),
                            "--images", str(tmp_path / "imgs.npy"), "--bound-min", *map(str, lo), "--bound-max", *map(str, hi),
                            "--dims", *map(str, dims), "--trunc", str(trunc), "--views-per-call", "4"])
    assert "vertices" in capsys.readouterr().out
    want = mesh.fuse_depths(depth, views, lo, hi, dims, trunc, colors=col)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    v, t, _, c = mesh.read_ply(out)
    assert np.array_equal(v, want[0]) and np.array_equal(t, want[1]) and np.array_equal(c, want[2])
    # the default truncation is four voxels
    v4, t4 = mesh.fuse_depths(depth, views, lo, hi, dims)
    assert len(t4) > 0
    # the geometry metrics take the PLY's arrays as they are
    vd, td = _dev(v), _dev(t)
    from mesh_eval_ref import icosphere
    gt = _dev(icosphere(4, 0.5)[0].astype(np.float32))
    res = metrics.mesh_geometry_metrics(vd, td, gt, threshold=0.1, n_samples=20000, seed=0)
    print(res)
    # every vertex lies within PIPELINE_BAR = 0.043 of the sphere and the ground-truth points are 0.04 apart, so every
    # sample has one within 0.1; the six cameras leave part of the far side unseen, so the recall only has to show
    # that most of the sphere is there
    assert res["precision"] > 0.99 and res["recall"] > 0.5 and res["n_pred"] == 20000
