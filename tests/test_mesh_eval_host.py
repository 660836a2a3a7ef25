"""The host side of the mesh geometry metrics (no device needed): mesh.read_ply against mesh.write_ply and
against hand-written ASCII / double / extra-property files, its refusals, the grid cell-size choice and the
argument rules of metrics.mesh_geometry_metrics."""
import math
import struct

import numpy as np
import pytest
import torch

from mesh_eval_ref import icosphere


def test_read_ply_round_trips_write_ply(tmp_path):
    from copenerf.mesh import read_ply, write_ply
    v, f = icosphere(1)
    rng = np.random.default_rng(0)
    n = rng.standard_normal(v.shape).astype(np.float32)
    c = rng.integers(0, 256, v.shape, dtype=np.uint8)
    for name, normals, colors in (("plain", None, None), ("n", n, None), ("c", None, c), ("nc", n, c)):
        path = tmp_path / f"{name}.ply"
        write_ply(path, v, f, normals=normals, colors=colors)
        rv, rf, rn, rc = read_ply(path)
        assert rv.dtype == np.float32 and rf.dtype == np.int32
        assert np.array_equal(rv, v) and np.array_equal(rf, f)
        assert (rn is None) == (normals is None) and (rn is None or np.array_equal(rn, n))
        assert (rc is None) == (colors is None) and (rc is None or (rc.dtype == np.uint8 and np.array_equal(rc, c)))


def test_read_ply_ascii_double_and_extra_properties(tmp_path):
    from copenerf.mesh import read_ply
    path = tmp_path / "a.ply"
    path.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty double x\n"
                    "property double y\nproperty double z\nproperty float quality\nproperty uchar red\n"
                    "property uchar green\nproperty uchar blue\nelement face 2\n"
                    "property list uchar uint vertex_indices\nproperty int flags\nend_header\n"
                    "0 0 0 0.5 255 0 0\n1 0 0 0.25 0 255 0\n0 1 0 0.125 0 0 255\n0 0 1.5 1 7 8 9\n"
                    "3 0 1 2 11\n3 0 2 3 12\n")
    v, f, n, c = read_ply(path)
    assert v.dtype == np.float32 and np.array_equal(v, [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]])
    assert np.array_equal(f, [[0, 1, 2], [0, 2, 3]]) and n is None
    assert np.array_equal(c, [[255, 0, 0], [0, 255, 0], [0, 0, 255], [7, 8, 9]])


def test_read_ply_binary_double_extra_elements_and_a_cloud(tmp_path):
    from copenerf.mesh import read_ply
    path = tmp_path / "b.ply"
    header = ("ply\nformat binary_little_endian 1.0\nelement camera 1\nproperty float fov\nelement vertex 3\n"
              "property double x\nproperty double y\nproperty double z\nproperty ushort label\nelement face 1\n"
              "property list int int vertex_index\nend_header\n")
    body = struct.pack("<f", 60.0)
    for i, p in enumerate(((0.1, 0.2, 0.3), (1, 2, 3), (-4, 5, 6e3))):
        body += struct.pack("<dddH", *p, i)
    body += struct.pack("<iiii", 3, 2, 1, 0)
    path.write_bytes(header.encode() + body)
    v, f, n, c = read_ply(path)
    assert np.array_equal(v, np.array([[0.1, 0.2, 0.3], [1, 2, 3], [-4, 5, 6e3]], dtype=np.float32))
    assert np.array_equal(f, [[2, 1, 0]]) and n is None and c is None
    cloud = tmp_path / "cloud.ply"
    cloud.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty float x\nproperty float y\n"
                      b"property float z\nend_header\n" + struct.pack("<6f", 1, 2, 3, 4, 5, 6))
    v, f, n, c = read_ply(cloud)
    assert np.array_equal(v, [[1, 2, 3], [4, 5, 6]]) and f is None


def test_read_ply_refuses_big_endian_quads_and_truncation(tmp_path):
    from copenerf.mesh import read_ply
    be = tmp_path / "be.ply"
    be.write_bytes(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\n"
                   b"property float z\nend_header\n")
    with pytest.raises(ValueError, match=r"be\.ply is big-endian"):
        read_ply(be)
    head = "ply\nformat {} 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n" \
           "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
    qa = tmp_path / "quad_ascii.ply"
    qa.write_text(head.format("ascii") + "0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError, match=r"quad_ascii\.ply has a face that is not a triangle"):
        read_ply(qa)
    qb = tmp_path / "quad_bin.ply"
    qb.write_bytes(head.format("binary_little_endian").encode() +
                   struct.pack("<12f", 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0) + struct.pack("<B4i", 4, 0, 1, 2, 3))
    with pytest.raises(ValueError, match=r"quad_bin\.ply has a face that is not a triangle"):
        read_ply(qb)
    short = tmp_path / "short.ply"
    short.write_bytes(head.format("binary_little_endian").encode() + struct.pack("<5f", 0, 0, 0, 1, 0))
    with pytest.raises(ValueError, match=r"short\.ply ends early"):
        read_ply(short)
    nope = tmp_path / "nope.ply"
    nope.write_bytes(b"solid\n")
    with pytest.raises(ValueError, match="not a PLY"):
        read_ply(nope)


@pytest.mark.parametrize("lo,hi,n", [((0, 0, 0), (1, 1, 1), 8000), ((-3, 2, 0), (5, 2.5, 40), 1_000_000),
                                     ((0, 0, 0), (1, 1, 0), 800), ((0, 0, 0), (0, 0, 0), 5),
                                     ((0, 0, 0), (1000, 1000, 1000), 2 ** 31 - 1), ((0, 0, 0), (1e-3, 1e6, 1), 10 ** 9)])
def test_cell_size_choice_respects_the_cap(lo, hi, n):
    from copenerf.metrics import nn_cell_size
    from copenerf.ops import NN_MAX_CELLS
    cell, dims = nn_cell_size(lo, hi, n)
    cells = dims[0] * dims[1] * dims[2]
    assert cell > 0 and min(dims) >= 1 and cells <= NN_MAX_CELLS
    for l, h, d in zip(lo, hi, dims):
        assert (h - l) / cell < d  # the box's far corner falls inside the last cell
    live = [h - l for l, h in zip(lo, hi) if h > l]
    if live and n / 8 <= NN_MAX_CELLS / 64:
        # away from the cap: about 8 targets per cell over the box
        assert math.prod(live) / cell ** len(live) == pytest.approx(n / 8, rel=1e-9)


def test_cell_size_choice_enlarges_at_the_cap():
    from copenerf.metrics import nn_cell_size
    cell, dims = nn_cell_size((0, 0, 0), (1, 1, 1), 2 ** 31 - 1)
    assert cell > (8 / (2 ** 31 - 1)) ** (1 / 3) and dims[0] * dims[1] * dims[2] <= 2 ** 26
    small, d2 = nn_cell_size((0, 0, 0), (1, 1, 1), 1000, max_cells=27)
    assert d2[0] * d2[1] * d2[2] <= 27 and small > 0.2


def test_mesh_geometry_metrics_argument_rules():
    from copenerf.metrics import mesh_geometry_metrics, nearest_distances
    v, f = icosphere(0)
    v, f, gt = torch.from_numpy(v), torch.from_numpy(f), torch.zeros(10, 3)
    with pytest.raises(ValueError, match="exactly one of n_samples and density"):
        mesh_geometry_metrics(v, f, gt, threshold=0.1)
    with pytest.raises(ValueError, match="exactly one of n_samples and density"):
        mesh_geometry_metrics(v, f, gt, threshold=0.1, n_samples=10, density=3.0)
    with pytest.raises(ValueError, match="crop_min and crop_max together"):
        mesh_geometry_metrics(v, f, gt, threshold=0.1, n_samples=10, crop_min=(0, 0, 0))
    with pytest.raises(ValueError, match="threshold"):
        mesh_geometry_metrics(v, f, gt, threshold=0.0, n_samples=10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh_geometry_metrics(v, f, gt, threshold=0.1, n_samples=10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nearest_distances(gt, gt)


def test_ops_refuse_cpu_tensors():
    from copenerf import ops
    v, f = icosphere(0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_area(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nn_grid(torch.zeros(4, 3), (0, 0, 0), 1.0, (1, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cloud_stats(torch.zeros(4), 0.1)


def test_geometry_from_stats_edge_cases():
    from copenerf.metrics import GEOMETRY_KEYS, geometry_from_stats
    r = geometry_from_stats([10, 8, 4.0, 0], [20, 20, 5.0, 0], 3.5)
    assert tuple(r) == GEOMETRY_KEYS
    assert r["precision"] == 0 and r["recall"] == 0 and r["fscore"] == 0.0  # P + R = 0
    assert r["accuracy"] == 0.5 and r["completeness"] == 0.25 and r["chamfer"] == 0.375
    assert (r["n_pred"], r["n_gt"], r["n_pred_far"], r["n_gt_far"], r["area"]) == (10, 20, 2, 0, 3.5)
    r = geometry_from_stats([10, 10, 1.0, 5], [10, 10, 1.0, 10], 1.0)
    assert r["precision"] == 0.5 and r["recall"] == 1.0 and r["fscore"] == pytest.approx(2 / 3)
