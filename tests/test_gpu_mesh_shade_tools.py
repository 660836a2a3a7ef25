"""tools/render_mesh.py and the new flags of tools/evaluate_mesh.py end to end on the device: the files written are
the library's own outputs, the normal entries follow the existing ones in results.txt, and without the new flags the
results file is what it was."""
import os
import sys

import numpy as np
import pytest
import torch

from mesh_eval_ref import icosphere
from mesh_raster_ref import three_views

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    return __import__(name)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _scene(tmp_path, h=24, w=32):
    from copenerf.mesh import write_ply
    v, f = icosphere(2, 0.5)
    vn = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    col = np.clip(np.abs(v) * 500, 0, 255).astype(np.uint8)
    views = three_views(h, w)[:2]
    paths = {k: str(tmp_path / k) for k in ("full.ply", "bare.ply", "K.npy", "W.npy")}
    write_ply(paths["full.ply"], v, f, normals=vn, colors=col)
    write_ply(paths["bare.ply"], v, f)
    np.save(paths["K.npy"], views[0]["camera_mat"])
    np.save(paths["W.npy"], np.stack([x["world_mat"] for x in views]))
    return v, f, vn, col, views, paths


def test_render_mesh_tool_writes_depth_normal_and_shaded_files(tmp_path, capsys):
    from PIL import Image
    from copenerf import mesh
    h, w = 24, 32
    v, f, vn, col, views, p = _scene(tmp_path, h, w)
    rm = _tool("render_mesh")
    base = ["--K", p["K.npy"], "--world-mats", p["W.npy"], "--resolution", str(h), str(w)]
    out = str(tmp_path / "plain")
    rm.main([p["bare.ply"], *base, "--out", out])
    assert "wrote 6 files" in capsys.readouterr().out
    want = mesh.render_mesh(_t(v), _t(f), views, (h, w))
    assert sorted(os.listdir(out)) == sorted(["depth_%06d.npz" % i for i in range(2)] + ["%06d_normal.png" % i for i in range(2)] +
                                             ["%06d_shaded.png" % i for i in range(2)])
    for i in range(2):
        depth = np.load(os.path.join(out, "depth_%06d.npz" % i))["pred"]
        d = want["depth"][i].cpu().numpy()
        assert depth.dtype == np.float32 and np.array_equal(depth, np.where(np.isinf(d), 0, d)) and (depth > 0).any()
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "%06d_normal.png" % i))), want["normal_image"][i].cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "%06d_shaded.png" % i))), want["shaded"][i].cpu().numpy())
    out2 = str(tmp_path / "rich")
    rm.main([p["full.ply"], *base, "--out", out2, "--smooth", "--colors", "--frame", "world"])
    want2 = mesh.render_mesh(_t(v), _t(f), views, (h, w), normals=_t(vn), colors=_t(col), frame="world")
    for key, name in (("normal_image", "%06d_normal.png"), ("shaded", "%06d_shaded.png")):
        got = np.asarray(Image.open(os.path.join(out2, name % 1)))
        assert np.array_equal(got, want2[key][1].cpu().numpy()) and not np.array_equal(got, want[key][1].cpu().numpy())
    with pytest.raises(SystemExit, match="--smooth needs vertex normals"):
        rm.main([p["bare.ply"], *base, "--out", out, "--smooth"])


def test_evaluate_mesh_tool_normals(tmp_path, capsys):
    from PIL import Image
    from copenerf import mesh, metrics
    from copenerf.mesh import write_ply
    h, w = 24, 32
    v, f, vn, col, views, p = _scene(tmp_path, h, w)
    em = _tool("evaluate_mesh")
    gt, gtn = (1.04 * vn).astype(np.float32), vn
    cloud, cloud_n = str(tmp_path / "gt.ply"), str(tmp_path / "gt_normals.ply")
    write_ply(cloud, gt, np.zeros((0, 3), dtype=np.int32))
    write_ply(cloud_n, gt, np.zeros((0, 3), dtype=np.int32), normals=gtn)
    base = ["--threshold", "0.1", "--samples", "2000", "--seed", "3"]
    out0, out1 = str(tmp_path / "r0.txt"), str(tmp_path / "r1.txt")
    plain = em.main([p["bare.ply"], cloud, *base, "--out", out0])
    assert plain == metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt), threshold=0.1, n_samples=2000, seed=3)
    assert [ln.split(": ")[0] for ln in open(out0).read().splitlines()] == list(metrics.GEOMETRY_KEYS)
    assert open(out0).read() == "".join(f"{k}: {x}\n" for k, x in plain.items())  # without the new flags: as before
    same = em.main([p["bare.ply"], cloud_n, *base, "--out", out1])  # normals in the file, not asked for: not used
    assert same == plain and open(out1).read() == open(out0).read()
    capsys.readouterr()
    res = em.main([p["bare.ply"], cloud_n, *base, "--normals", "--out", out1])
    assert res == metrics.mesh_geometry_metrics(_t(v), _t(f), _t(gt), gt_normals=_t(gtn), threshold=0.1, n_samples=2000, seed=3)
    lines = open(out1).read().splitlines()
    assert lines[:len(metrics.GEOMETRY_KEYS)] == open(out0).read().splitlines()
    assert [ln.split(": ")[0] for ln in lines[len(metrics.GEOMETRY_KEYS):]] == list(metrics.NORMAL_GEOMETRY_KEYS)
    assert capsys.readouterr().out.splitlines() == lines and res["normal_consistency"] > 0.97
    with pytest.raises(SystemExit, match="--normals needs vertex normals"):
        em.main([p["bare.ply"], cloud, *base, "--normals"])
    # the ground truth as a mesh, sampled by area with its face normals
    sampled = em.main([p["bare.ply"], p["bare.ply"], *base, "--normals", "--gt-mesh-samples", "3000"])
    pts, nrm = em.sample_ground_truth(v, f, 3000, 4, torch.device(DEV))
    assert sampled == metrics.mesh_geometry_metrics(_t(v), _t(f), pts, gt_normals=nrm, threshold=0.1, n_samples=2000, seed=3)
    assert sampled["n_gt"] == 3000 and sampled["normal_consistency"] > 0.97 and sampled["chamfer"] < 0.02
    no_normals = em.main([p["bare.ply"], p["bare.ply"], *base, "--gt-mesh-samples", "3000"])
    assert tuple(no_normals) == metrics.GEOMETRY_KEYS and all(no_normals[k] == sampled[k] for k in no_normals)
    # --normal-maps-out beside --depths-out
    nd, dd = str(tmp_path / "normals"), str(tmp_path / "depths")
    em.main([p["bare.ply"], cloud, *base, "--cull-views", p["K.npy"], p["W.npy"], "--cull-resolution", str(h), str(w),
             "--normal-maps-out", nd, "--depths-out", dd])
    want = mesh.render_mesh(_t(v), _t(f), views, (h, w))["normal_image"].cpu().numpy()
    assert sorted(os.listdir(nd)) == ["%06d_normal.png" % i for i in range(2)] and len(os.listdir(dd)) == 2
    for i in range(2):
        assert np.array_equal(np.asarray(Image.open(os.path.join(nd, "%06d_normal.png" % i))), want[i])
