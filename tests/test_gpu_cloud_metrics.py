"""The ground-truth preparation arguments of metrics.mesh_geometry_metrics (gt_outliers, gt_voxel,
gt_estimate_normals, icp's voxel) and of tools/evaluate_mesh.py on the device: test_gpu_icp_metrics.py's
marching-tetrahedra sphere (radius 0.4) against samples of the same sphere displaced by a known translation, the
ground truth coming WITHOUT normals."""
import os
import sys

import numpy as np
import pytest
import torch

import icp_ref
import mesh_ref as MR

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
S, SEED, N_GT, N_REG = 8000, 3, 4000, 2000
TAU, REACH = 0.04, 0.15
MOTION = icp_ref.similarity(np.eye(3), (0.04, -0.03, 0.05))
ICP = dict(max_corr_dist=REACH, n_samples=N_REG, tol=1e-9, max_iters=200, mode="plane")
_SHARED = {}


def _shared():
    if not _SHARED:
        from copenerf import ops
        v, f = ops.isosurface(torch.from_numpy(MR.sphere_soft()).to(DEV), 0.0, *BOX)
        v, f = v.contiguous(), f.contiguous()
        handle, area = ops.mesh_area(v, f)  # (kept: the sampler reads the area on the device)
        own = ops.mesh_sample(handle, N_GT, torch.tensor([SEED + 1, 0], dtype=torch.uint64, device=DEV))[0].cpu().numpy()
        gt = icp_ref.apply(MOTION, own).astype(np.float32)
        tgt = torch.from_numpy(gt).to(DEV)
        # the analytic normals of the displaced sphere at the ground-truth points
        analytic = torch.nn.functional.normalize(tgt - torch.tensor(MOTION[:3, 3], dtype=torch.float32, device=DEV), dim=1)
        reg = ops.mesh_sample(handle, N_REG, torch.tensor([SEED, 4 * S], dtype=torch.uint64, device=DEV))[0].cpu().numpy()
        _SHARED.update(v=v, f=f, gt=gt, tgt=tgt, analytic=analytic.contiguous(), reg=reg)
    return _SHARED


def test_defaults_are_the_call_without_the_keywords_bitwise():
    from copenerf import metrics
    s = _shared()
    off = dict(gt_voxel=None, gt_outliers=None, gt_estimate_normals=None)
    for extra in (dict(), dict(gt_normals=s["analytic"]), dict(max_dist=0.05, crop_min=(-1, -1, 0), crop_max=(1, 1, 1)),
                  dict(icp=dict(max_corr_dist=REACH, n_samples=N_REG))):
        kw = dict(threshold=TAU, n_samples=S, seed=SEED, **extra)
        a = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], **kw)
        b = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], **off, **kw)
        assert list(a.items()) == list(b.items())


def test_estimated_normals_stand_in_for_the_analytic_ones():
    from copenerf import metrics
    s = _shared()
    kw = dict(threshold=TAU, n_samples=S, seed=SEED, transform=MOTION)
    want = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], gt_normals=s["analytic"], **kw)
    got = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], gt_estimate_normals=16, **kw)
    print(f"normal_consistency {got['normal_consistency']:.5f} with estimated normals, {want['normal_consistency']:.5f} "
          f"with the analytic ones; pairs {got['n_gt_normal']} / {want['n_gt_normal']}")
    assert tuple(got) == tuple(want)
    assert abs(got["normal_consistency"] - want["normal_consistency"]) <= 0.01
    assert got["n_gt_normal"] == want["n_gt_normal"] == N_GT  # no point was left without a normal
    assert all(got[k] == want[k] for k in metrics.GEOMETRY_KEYS)  # the distances do not see the normals
    with pytest.raises(ValueError, match="gt_estimate_normals with gt_normals"):
        metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], gt_normals=s["analytic"], gt_estimate_normals=16, **kw)


def test_plane_icp_runs_on_estimated_normals():
    from copenerf import metrics
    s = _shared()
    kw = dict(threshold=TAU, n_samples=S, seed=SEED)
    with pytest.raises(ValueError, match="gt_normals"):
        metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], icp=ICP, **kw)
    plain = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], **kw)
    got = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], icp=ICP, gt_estimate_normals=16, **kw)
    # the float64 restatement on the same registration samples and the same (device-estimated, fp32) normals
    normals = metrics.estimate_normals(s["tgt"], 16).cpu().numpy()
    ref = icp_ref.register(s["reg"], s["gt"], REACH, mode="plane", target_normals=normals, tol=ICP["tol"],
                           max_iters=ICP["max_iters"])
    err = np.abs(np.asarray(got["transform"]) - MOTION).max()
    ref_err = np.abs(ref["transform"] - MOTION).max()
    print(f"plane ICP on estimated normals: fscore {plain['fscore']:.4f} -> {got['fscore']:.4f}, max |T - motion| = "
          f"{err:.3e} (reference {ref_err:.3e}), iterations {got['icp_iterations']} (reference {ref['iterations']})")
    assert err <= ref_err + 2e-6
    assert got["icp_converged"] and got["fscore"] > plain["fscore"] and got["fscore"] > 0.99
    assert "normal_consistency" in got  # the estimated normals also turn the normal metrics on


def test_gt_voxel_and_outliers_leave_chamfer_within_the_voxel_size():
    from copenerf import metrics
    s = _shared()
    kw = dict(threshold=TAU, n_samples=S, seed=SEED, transform=MOTION)
    plain = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], **kw)
    for voxel in (0.01, 0.05):
        got = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], gt_voxel=voxel, **kw)
        print(f"gt_voxel {voxel}: n_gt {plain['n_gt']} -> {got['n_gt']}, chamfer {plain['chamfer']:.5f} -> {got['chamfer']:.5f}")
        assert abs(got["chamfer"] - plain["chamfer"]) <= voxel and got["n_gt"] < plain["n_gt"]
        assert got["n_gt"] == metrics.voxel_down_sample(s["tgt"], voxel)["points"].shape[0]
    # planted far points are removed before anything else: the ground truth is the clean one again
    far = torch.tensor([[3.0, 3.0, 3.0], [3.1, 3.0, 2.9], [-3.0, 2.0, 3.0]], device=DEV)
    dirty = torch.cat([s["tgt"], far]).contiguous()
    bad = metrics.mesh_geometry_metrics(s["v"], s["f"], dirty, **kw)
    fixed = metrics.mesh_geometry_metrics(s["v"], s["f"], dirty, gt_outliers=(8, 3.0), **kw)
    kept, mask = metrics.remove_statistical_outliers(dirty, 8, 3.0)
    assert not mask[N_GT:].any() and fixed["n_gt"] == kept.shape[0] < bad["n_gt"]
    assert fixed["completeness"] < bad["completeness"] and abs(fixed["completeness"] - plain["completeness"]) < 1e-3
    # icp's voxel: the registration runs on the down-sampled clouds and still undoes the motion
    kw = dict(threshold=TAU, n_samples=S, seed=SEED)
    reg = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], icp=dict(max_corr_dist=REACH, n_samples=N_REG, voxel=0.03), **kw)
    # (a sphere about the origin shows the translation alone: its centre goes to the transform's last column)
    assert reg["icp_converged"] and np.abs(np.asarray(reg["transform"])[:3, 3] - MOTION[:3, 3]).max() < 5e-3
    assert reg["n_gt"] == N_GT and reg["fscore"] > 0.99  # the evaluation still sees the whole ground truth
    with pytest.raises(ValueError, match="icp voxel"):
        metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], icp=dict(max_corr_dist=REACH, n_samples=N_REG, voxel=0.0), **kw)
    with pytest.raises(ValueError, match="gt_voxel"):
        metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], gt_voxel=-1.0, **kw)


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_mesh
    return evaluate_mesh


def test_evaluate_mesh_tool_estimates_missing_normals(tmp_path, capsys):
    from copenerf import metrics
    from copenerf.mesh import write_ply
    s = _shared()
    mesh, cloud, out = str(tmp_path / "mesh.ply"), str(tmp_path / "gt.ply"), str(tmp_path / "results.txt")
    write_ply(mesh, s["v"].cpu().numpy(), s["f"].cpu().numpy())
    write_ply(cloud, s["gt"], np.zeros((0, 3), dtype=np.int32))  # a ground truth without normals
    base = [mesh, cloud, "--threshold", str(TAU), "--samples", str(S), "--seed", str(SEED)]
    with pytest.raises(SystemExit, match="--normals needs vertex normals"):
        _tool().main(base + ["--normals"])
    with pytest.raises(SystemExit, match="--normals needs vertex normals"):
        _tool().main(base + ["--icp", str(REACH), "--icp-mode", "plane"])
    capsys.readouterr()
    res = _tool().main(base + ["--normals", "--gt-estimate-normals", "16", "--gt-voxel", "0.01", "--out", out])
    want = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], threshold=TAU, n_samples=S, seed=SEED, gt_voxel=0.01,
                                         gt_estimate_normals=16)
    assert res == want and all(k in res for k in metrics.NORMAL_GEOMETRY_KEYS)
    lines = open(out).read().splitlines()
    assert [line.split(": ")[0] for line in lines] == list(res) and capsys.readouterr().out.splitlines() == lines
    assert any(line.startswith("normal_consistency: ") for line in lines)


def test_prepare_cloud_tool(tmp_path, capsys):
    from copenerf.mesh import read_ply, write_ply
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prepare_cloud
    s = _shared()
    src, dst = str(tmp_path / "raw.ply"), str(tmp_path / "clean.ply")
    raw = np.concatenate([s["gt"], np.array([[3.0, 3.0, 3.0], [3.1, 3.0, 2.9]], dtype=np.float32)])
    write_ply(src, raw, np.zeros((0, 3), dtype=np.int32))
    n = prepare_cloud.main([src, dst, "--outliers", "8", "3.0", "--voxel", "0.01", "--estimate-normals", "16",
                            "--orient-to", *[str(x) for x in MOTION[:3, 3]]])
    p, f, nrm, c = read_ply(dst)
    assert len(p) == n < N_GT and (f is None or len(f) == 0) and c is None and nrm is not None
    assert np.abs(p).max() < 1.0  # the planted points are gone
    inward = -(p - MOTION[:3, 3]) / np.linalg.norm(p - MOTION[:3, 3], axis=1, keepdims=True)
    assert np.all(np.sum(nrm * inward, axis=1) > 0.9)  # unit normals, flipped towards the centre
