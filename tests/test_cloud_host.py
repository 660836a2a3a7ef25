"""The host side of the point-cloud preparation (no device needed): the new flags of tools/evaluate_mesh.py and
tools/prepare_cloud.py parse and are refused in the combinations that make no sense, prepare_cloud's writer
round-trips a cloud PLY with normals, and the argument rules of the metrics entries and of the outlier cut."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = ["m.ply", "gt.ply", "--threshold", "0.01", "--samples", "1000"]


def test_evaluate_mesh_new_flags_parse():
    tool = _tool("evaluate_mesh")
    a = tool.parse_args(BASE)
    assert a.gt_outliers is None and a.gt_voxel is None and a.gt_estimate_normals is None and a.icp_voxel is None
    a = tool.parse_args(BASE + ["--normals", "--gt-outliers", "20", "2.0", "--gt-voxel", "0.005", "--gt-estimate-normals", "16"])
    assert a.gt_outliers == (20, 2.0) and a.gt_voxel == 0.005 and a.gt_estimate_normals == 16
    a = tool.parse_args(BASE + ["--icp", "0.1", "0.02", "--icp-mode", "plane", "--gt-estimate-normals", "12", "--icp-voxel", "0.01"])
    icp = tool.icp_kwargs(a)
    assert icp["voxel"] == 0.01 and icp["mode"] == "plane" and len(icp["stages"]) == 2
    assert "voxel" not in tool.icp_kwargs(tool.parse_args(BASE + ["--icp", "0.1"]))


@pytest.mark.parametrize("extra", [
    ["--gt-estimate-normals", "16"],                                   # nothing asks for normals
    ["--normals", "--gt-estimate-normals", "2"],                       # fewer than 3 neighbours span no plane
    ["--normals", "--gt-estimate-normals", "33"],
    ["--normals", "--gt-estimate-normals", "16", "--gt-mesh-samples", "1000"],
    ["--gt-outliers", "20", "2.0", "--gt-mesh-samples", "1000"],
    ["--gt-outliers", "0", "2.0"], ["--gt-outliers", "33", "2.0"], ["--gt-outliers", "20", "-1"],
    ["--gt-outliers", "x", "2.0"], ["--gt-outliers", "20"],
    ["--gt-voxel", "0"], ["--gt-voxel", "-0.1"], ["--gt-voxel", "inf"], ["--gt-voxel", "nan"],
    ["--icp-voxel", "0.01"],                                            # without --icp
    ["--icp", "0.1", "--icp-voxel", "0"],
])
def test_evaluate_mesh_refuses_senseless_combinations(extra):
    tool = _tool("evaluate_mesh")
    with pytest.raises(SystemExit):
        tool.parse_args(BASE + extra)


def test_prepare_cloud_flags():
    tool = _tool("prepare_cloud")
    a = tool.parse_args(["in.ply", "out.ply", "--voxel", "0.01", "--outliers", "20", "2", "--estimate-normals", "16",
                         "--orient-to", "0", "0", "5"])
    assert a.voxel == 0.01 and a.outliers == (20, 2.0) and a.estimate_normals == 16 and a.orient_to == [0.0, 0.0, 5.0]
    for bad in (["in.ply", "out.ply"], ["in.ply", "out.ply", "--orient-to", "0", "0", "1"],
                ["in.ply", "out.ply", "--voxel", "0"], ["in.ply", "out.ply", "--voxel", "nan"],
                ["in.ply", "out.ply", "--estimate-normals", "2"], ["in.ply", "out.ply", "--estimate-normals", "40"],
                ["in.ply", "out.ply", "--outliers", "40", "2"], ["in.ply", "out.ply", "--outliers", "20", "0"],
                ["in.ply", "--voxel", "0.1"]):
        with pytest.raises(SystemExit):
            tool.parse_args(bad)


def test_prepare_cloud_writer_round_trips_a_cloud_with_normals(tmp_path):
    from copenerf.mesh import read_ply
    tool = _tool("prepare_cloud")
    rng = np.random.default_rng(1)
    p = rng.standard_normal((37, 3)).astype(np.float32)
    n = rng.standard_normal((37, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    c = rng.integers(0, 256, (37, 3), dtype=np.uint8)
    for name, normals, colors in (("n", n, None), ("nc", n, c), ("plain", None, None)):
        path = tmp_path / f"{name}.ply"
        tool.write_cloud(path, p, normals, colors)
        rp, rf, rn, rc = read_ply(path)
        assert np.array_equal(rp, p) and (rf is None or len(rf) == 0)
        assert (rn is None) == (normals is None) and (rn is None or np.array_equal(rn, n))
        assert (rc is None) == (colors is None) and (rc is None or np.array_equal(rc, c))
    assert b"property float nx" in (tmp_path / "n.ply").read_bytes()[:400]


def test_metrics_entries_refuse_bad_arguments_before_the_device():
    from copenerf import metrics
    cpu = torch.zeros(10, 3)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        metrics.knn(cpu, cpu, 4)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        metrics.voxel_down_sample(cpu, 0.1)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        metrics.estimate_normals(cpu)
    with pytest.raises(RuntimeError, match="CUDA/HIP"):
        metrics.remove_statistical_outliers(cpu)


def test_outlier_cut():
    from copenerf import metrics
    m = np.array([1.0, 2.0, 3.0, 6.0])
    mu, sigma, cut = metrics.outlier_cut([len(m), m.sum(), (m * m).sum()], 1.5)
    assert math.isclose(mu, 3.0) and math.isclose(sigma, m.std()) and math.isclose(cut, 3.0 + 1.5 * m.std())
    assert metrics.outlier_cut([0.0, 0.0, 0.0], 2.0) == (0.0, 0.0, 0.0)
