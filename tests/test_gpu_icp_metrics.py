"""metrics.mesh_geometry_metrics(icp=...) and tools/evaluate_mesh.py --icp on the device: a marching-tetrahedra sphere
(tests/mesh_ref.py's soft sphere of radius 0.4 through ops.isosurface) scored against samples of the same sphere
displaced by a known rigid motion -- a translation, the part of a rigid motion a sphere can show.  4000 samples on an
area of 2.0 lie about 0.022 apart; the score is taken at 0.04, about twice that, and the motion is 0.07 long."""
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
# a tolerance far below the default's: the loop runs on until its steps are of the order of 1e-9, so that the device
# and the float64 reference end at the same optimum and not one stopping step apart
ICP = dict(max_corr_dist=REACH, n_samples=N_REG, tol=1e-9, max_iters=200)
ICP_KEYS = ("icp_fitness", "icp_rmse", "icp_iterations", "icp_converged", "transform")
_SHARED = {}


def _registration_samples(vertices, triangles, transform=None):
    """The registration samples mesh_geometry_metrics(icp=...) draws for (S, SEED, N_REG): the mesh taken through
    `transform` in fp32 on the device, sampled by area at Philox offset 4 S (the evaluation's samples are at 0)."""
    from copenerf import ops
    if transform is not None:
        B = torch.as_tensor(transform, dtype=torch.float32).to(DEV)
        vertices = (vertices @ B[:3, :3].T + B[:3, 3]).contiguous()
    handle, area = ops.mesh_area(vertices, triangles)  # (kept: the sampler reads the area on the device)
    return ops.mesh_sample(handle, N_REG, torch.tensor([SEED, 4 * S], dtype=torch.uint64, device=DEV))[0].cpu().numpy()


def _shared():
    if not _SHARED:
        from copenerf import ops
        v, f = ops.isosurface(torch.from_numpy(MR.sphere_soft()).to(DEV), 0.0, *BOX)
        v, f = v.contiguous(), f.contiguous()
        handle, area = ops.mesh_area(v, f)  # (kept: the sampler reads the area on the device)
        own = ops.mesh_sample(handle, N_GT, torch.tensor([SEED + 1, 0], dtype=torch.uint64, device=DEV))[0].cpu().numpy()
        gt = icp_ref.apply(MOTION, own).astype(np.float32)
        reg = _registration_samples(v, f)
        ref = icp_ref.register(reg, gt, REACH, tol=ICP["tol"], max_iters=ICP["max_iters"])
        _SHARED.update(v=v, f=f, gt=gt, tgt=torch.from_numpy(gt).to(DEV), ref=ref)
    return _SHARED


def test_icp_raises_the_score_and_undoes_the_motion():
    from copenerf import metrics
    s = _shared()
    plain = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], threshold=TAU, n_samples=S, seed=SEED)
    got = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], threshold=TAU, n_samples=S, seed=SEED, icp=ICP)
    T, ref = np.asarray(got["transform"]), s["ref"]
    err, ref_err = np.abs(T - MOTION).max(), np.abs(ref["transform"] - MOTION).max()
    print(f"fscore {plain['fscore']:.4f} -> {got['fscore']:.4f}, chamfer {plain['chamfer']:.5f} -> {got['chamfer']:.5f}; "
          f"max |T - motion| = {err:.3e} (reference {ref_err:.3e}), iterations {got['icp_iterations']} (reference "
          f"{ref['iterations']}), rmse {got['icp_rmse']:.6e} (reference {ref['inlier_rmse']:.6e})")
    assert tuple(got) == tuple(plain) + ICP_KEYS
    assert got["fscore"] > plain["fscore"] and got["chamfer"] < plain["chamfer"]
    assert plain["fscore"] < 0.9 and got["fscore"] > 0.99
    assert err <= ref_err + 2e-6
    assert got["icp_converged"] is True and got["icp_fitness"] == 1.0 and got["icp_iterations"] >= 1
    assert got["icp_rmse"] == pytest.approx(ref["inlier_rmse"], rel=1e-3)
    # an initial transform is composed with: the mesh pulled back through a similarity, and that similarity given
    back = icp_ref.similarity(icp_ref.rotation((0.1, 0.7, -0.2), 25.0), (0.2, -0.1, 0.3), 1.5)
    inv = np.linalg.inv(back)
    pulled = torch.from_numpy(icp_ref.apply(inv, s["v"].cpu().numpy()).astype(np.float32)).to(DEV)
    via = metrics.mesh_geometry_metrics(pulled, s["f"], s["tgt"], threshold=TAU, n_samples=S, seed=SEED, transform=back, icp=ICP)
    # the float64 reference on this call's own registration samples: the pulled mesh taken through `back` as
    # mesh_geometry_metrics does it (fp32 on the device), sampled at offset 4 S.  A composition in the wrong order, or
    # onto the wrong side, would leave T back^-1 off the motion by the size of `back` itself.
    reg = _registration_samples(pulled, s["f"], back)
    ref_via = icp_ref.register(reg, s["gt"], REACH, tol=ICP["tol"], max_iters=ICP["max_iters"])
    via_err = np.abs(np.asarray(via["transform"]) @ inv - MOTION).max()
    ref_via_err = np.abs(ref_via["transform"] - MOTION).max()
    print(f"with an initial transform: max |T back^-1 - motion| = {via_err:.3e} (reference {ref_via_err:.3e}), "
          f"fscore {via['fscore']:.4f}")
    assert via_err <= ref_via_err + 2e-6
    assert via["fscore"] > 0.99 and via["fscore"] > plain["fscore"] and via["icp_converged"]


def test_icp_undoes_a_rotation_on_an_asymmetric_surface():
    """The same on a marching-tetrahedra mesh of tests/icp_ref.py's bumpy ellipsoid, where a rotation shows: the ground
    truth is the mesh's own samples taken through 5 degrees about a skew axis and a translation, the mesh comes pulled
    back through a similarity that is given as `transform`, and the composed transform is held to the float64
    reference's error on the same registration samples."""
    from copenerf import metrics, ops
    lo, hi, n = (-1.2, -1.2, -1.2), (1.2, 1.2, 1.2), 49
    u = icp_ref.bumpy_field(np.stack(MR.grid((n,) * 3, lo, hi), axis=-1)).astype(np.float32)
    v, f = ops.isosurface(torch.from_numpy(u).to(DEV), 0.0, lo, hi)
    v, f = v.contiguous(), f.contiguous()
    handle, area = ops.mesh_area(v, f)
    own = ops.mesh_sample(handle, N_GT, torch.tensor([SEED + 1, 0], dtype=torch.uint64, device=DEV))[0].cpu().numpy()
    motion = icp_ref.similarity(icp_ref.rotation((0.3, -0.5, 0.8), 5.0), (0.04, -0.03, 0.05))
    gt = icp_ref.apply(motion, own).astype(np.float32)
    back = icp_ref.similarity(icp_ref.rotation((0.1, 0.7, -0.2), 25.0), (0.2, -0.1, 0.3), 1.5)
    inv = np.linalg.inv(back)
    pulled = torch.from_numpy(icp_ref.apply(inv, v.cpu().numpy()).astype(np.float32)).to(DEV)
    reg = _registration_samples(pulled, f, back)
    ref = icp_ref.register(reg, gt, REACH, tol=ICP["tol"], max_iters=ICP["max_iters"])
    kw = dict(threshold=TAU, n_samples=S, seed=SEED, transform=back)
    plain = metrics.mesh_geometry_metrics(pulled, f, torch.from_numpy(gt).to(DEV), **kw)
    got = metrics.mesh_geometry_metrics(pulled, f, torch.from_numpy(gt).to(DEV), icp=ICP, **kw)
    err = np.abs(np.asarray(got["transform"]) @ inv - motion).max()
    ref_err = np.abs(ref["transform"] - motion).max()
    print(f"ellipsoid: fscore {plain['fscore']:.4f} -> {got['fscore']:.4f}, max |T back^-1 - motion| = {err:.3e} "
          f"(reference {ref_err:.3e}), iterations {got['icp_iterations']} (reference {ref['iterations']})")
    size = np.abs(motion - np.eye(4)).max()
    assert err <= ref_err + 2e-6
    assert ref_err < 0.5 * size  # the reference undoes most of the motion, so the line above cannot pass on a motion left in
    assert got["icp_converged"] and got["fscore"] > plain["fscore"] and got["chamfer"] < plain["chamfer"]


def test_icp_none_is_the_call_without_the_keyword_bitwise():
    from copenerf import metrics
    s = _shared()
    normals = torch.nn.functional.normalize(s["tgt"] - torch.tensor(MOTION[:3, 3], dtype=torch.float32, device=DEV), dim=1).contiguous()
    for extra in (dict(), dict(gt_normals=normals), dict(max_dist=0.05, crop_min=(-1, -1, 0), crop_max=(1, 1, 1))):
        kw = dict(threshold=TAU, n_samples=S, seed=SEED, **extra)
        a = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], **kw)
        b = metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], icp=None, **kw)
        assert list(a.items()) == list(b.items()) and not set(a) & set(ICP_KEYS)


def test_icp_argument_errors():
    from copenerf import metrics
    s = _shared()
    kw = dict(threshold=TAU, n_samples=S, seed=SEED)
    with pytest.raises(ValueError, match="gt_normals"):
        metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], icp=dict(ICP, mode="plane"), **kw)
    with pytest.raises(ValueError, match="stages or a single max_corr_dist"):
        metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], icp=dict(n_samples=100), **kw)
    with pytest.raises(ValueError, match="n_samples"):
        metrics.mesh_geometry_metrics(s["v"], s["f"], s["tgt"], icp=dict(max_corr_dist=0.1), **kw)


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_mesh
    return evaluate_mesh


def test_evaluate_mesh_tool_with_icp(tmp_path, capsys):
    from copenerf import metrics
    from copenerf.mesh import write_ply
    s = _shared()
    mesh, cloud = str(tmp_path / "mesh.ply"), str(tmp_path / "gt.ply")
    out, t_out = str(tmp_path / "results.txt"), str(tmp_path / "T.npy")
    write_ply(mesh, s["v"].cpu().numpy(), s["f"].cpu().numpy())
    write_ply(cloud, s["gt"], np.zeros((0, 3), dtype=np.int32))
    base = [mesh, cloud, "--threshold", str(TAU), "--samples", str(S), "--seed", str(SEED)]
    plain = _tool().main(base)
    capsys.readouterr()
    res = _tool().main(base + ["--icp", str(REACH), "0.05", "--icp-stride", "2", "1", "--icp-samples", str(N_REG),
                               "--transform-out", t_out, "--out", out])
    want = metrics.mesh_geometry_metrics(
        s["v"], s["f"], s["tgt"], threshold=TAU, n_samples=S, seed=SEED,
        icp=dict(stages=[dict(max_corr_dist=REACH, stride=2), dict(max_corr_dist=0.05, stride=1)], n_samples=N_REG,
                 mode="point", with_scale=False, max_iters=50, tol=1e-6))
    assert res == want and tuple(res) == tuple(plain) + ICP_KEYS
    assert res["fscore"] > plain["fscore"] and res["icp_converged"]
    lines = open(out).read().splitlines()
    assert [line.split(": ")[0] for line in lines] == list(res) and capsys.readouterr().out.splitlines() == lines
    saved = np.load(t_out)
    assert saved.dtype == np.float64 and np.array_equal(saved, np.asarray(res["transform"]))
