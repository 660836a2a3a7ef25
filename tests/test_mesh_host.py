"""Mesh extraction without a device: the host reference of the mesher (tests/mesh_ref.py) on analytic volumes,
the ABI v16 entry points' host-side checks and workspace formulas, the PLY writer, and the no-CPU-fallback
error of NeuSRenderer.extract_geometry."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mesh_ref as R
from helpers import REN_CFG, build_modules
from test_abi import _fake_net

BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def _mesh(u):
    v, t = R.isosurface(u, 0.0, *BOX)
    assert t.min() >= 0 and t.max() < len(v)
    assert len(np.unique(t)) == len(v)  # every vertex is referenced by some triangle
    return v, t


@pytest.mark.parametrize("make, radius", [(R.sphere_tie, 0.5), (R.sphere_soft, 0.4)])
def test_reference_spheres_are_closed_oriented_and_have_the_analytic_volume(make, radius):
    u = make()
    if make is R.sphere_tie:
        assert int((u == 0).sum()) == 6  # six grid points tie the threshold exactly
    v, t = _mesh(u)
    assert R.is_closed_oriented(t, len(v))
    assert R.euler_characteristic(t, len(v)) == 2
    ratio = R.signed_volume(v, t) / (4.0 / 3.0 * math.pi * radius ** 3)
    print(make.__name__, "V", len(v), "T", len(t), "volume ratio", ratio)
    assert ratio > 0 and abs(ratio - 1.0) <= 0.03, ratio  # positive: normals point out of the surface


@pytest.mark.parametrize("make, chi", [(R.two_spheres, 4), (R.torus, 0)])
def test_reference_topology(make, chi):
    v, t = _mesh(make())
    assert R.is_closed_oriented(t, len(v))
    assert R.euler_characteristic(t, len(v)) == chi
    assert R.signed_volume(v, t) > 0


def test_reference_open_mesh_where_the_box_cuts_the_surface():
    v, t = _mesh(R.sphere_cut())
    assert len(t) > 0
    assert not R.is_closed_oriented(t, len(v))
    # still consistently oriented: no directed edge twice
    e = R.directed_edges(t)
    assert len(np.unique(e[:, 0] * len(v) + e[:, 1])) == len(e)


def test_reference_orientation_rule_decides_every_case():
    """All 6 x 14 mixed masks: one triangle for a 1 : 3 split, two for 2 : 2; the midpoint rule's dot product is
    never zero (asserted inside)."""
    for k in range(6):
        for m in range(16):
            n = bin(m).count("1")
            assert len(R._triangles_of(k, m)) == {0: 0, 4: 0, 1: 1, 3: 1, 2: 2}[n]


def _rup(n, a=256):
    return (n + a - 1) // a * a


def test_mesh_abi_checks_and_workspace_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    assert lib.cn_abi_version() >= 16
    # null descriptors
    assert lib.cn_mesh_count(None, 4096, 1 << 20, None) == -1
    assert b"null descriptor" in lib.cn_last_error()
    assert lib.cn_mesh_emit(None, 4096, 1 << 20, None) == -1
    assert lib.cn_sdf_grid(None, 4096, 1 << 20, None) == -1
    assert b"null descriptor" in lib.cn_last_error()
    assert lib.cn_sdf_grid_workspace_bytes(None) == 0
    lo, hi = (_lib.c_f32 * 3)(-1, -1, -1), (_lib.c_f32 * 3)(1, 1, 1)
    assert lib.cn_grid_points(4, 4, 4, None, hi, 4096, 0, 64, 4096, None) == -1
    assert lib.cn_grid_points(4, 4, 4, lo, hi, None, 0, 64, 4096, None) == -1
    assert lib.cn_grid_points(4, 4, 4, lo, hi, 4096, 60, 5, 4096, None) == -2  # rows past the grid
    assert b"rows" in lib.cn_last_error()
    assert lib.cn_grid_points(4, 4, 4, lo, hi, 4096, 0, 64, 4100, None) == -3  # pts alignment
    # the mesher's workspace: N + 4 N + C + 4 C + the two scans' tile totals, every piece rounded up to 256
    for dims in ((2, 2, 2), (5, 7, 11), (41, 40, 43), (512, 512, 512)):
        N = dims[0] * dims[1] * dims[2]
        C = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
        want = (_rup(N) + _rup(4 * N) + _rup(C) + _rup(4 * C) + _rup(4 * -(-N // 1024)) + _rup(4 * -(-C // 1024)))
        assert lib.cn_mesh_workspace_bytes(*dims) == want, dims
    # dims of 1 and 700^3 (7 x vertices >= 2^31) are shape errors
    assert lib.cn_mesh_workspace_bytes(1, 8, 8) == 0
    assert lib.cn_mesh_workspace_bytes(700, 700, 700) == 0
    d = _lib.MeshDesc()
    d.u, d.counts = 4096, 4096
    for dims, msg in (((8, 1, 8), b"each at least 2"), ((700, 700, 700), b"too large")):
        d.nx, d.ny, d.nz = dims
        for fn in (lib.cn_mesh_count, lib.cn_mesh_emit):
            assert fn(ctypes.byref(d), 4096, 1 << 40, None) == -2
            assert msg in lib.cn_last_error(), lib.cn_last_error()
    # 12 x cells >= 2^31 alone is refused too; just below both bounds is accepted
    assert 7 * 600 ** 3 < 2 ** 31 <= 12 * 599 ** 3
    assert lib.cn_mesh_workspace_bytes(600, 600, 600) == 0
    assert 12 * 559 ** 3 < 2 ** 31 and lib.cn_mesh_workspace_bytes(560, 560, 560) > 0
    d.nx, d.ny, d.nz = 5, 7, 11
    need = lib.cn_mesh_workspace_bytes(5, 7, 11)
    assert lib.cn_mesh_count(ctypes.byref(d), 4096, need - 1, None) == -2
    assert b"workspace" in lib.cn_last_error()
    assert lib.cn_mesh_count(ctypes.byref(d), 4096 + 16, need, None) == -3
    d.u = None
    assert lib.cn_mesh_count(ctypes.byref(d), 4096, need, None) == -1
    d.u, d.max_vertices = 4096, 10  # emit: a capacity without a buffer
    assert lib.cn_mesh_emit(ctypes.byref(d), 4096, need, None) == -1
    assert b"null vertices" in lib.cn_last_error()
    d.max_vertices = -1
    assert lib.cn_mesh_emit(ctypes.byref(d), 4096, need, None) == -2


def test_sdf_grid_abi_checks_and_workspace_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    n = _fake_net(mode=2)  # bf16x6: the fused query
    d = _lib.SdfGridDesc()
    d.net, d.nx, d.ny, d.nz = ctypes.pointer(n), 21, 21, 21
    d.time_step, d.u = 4096, 4096
    total = 21 ** 3
    q = lib.cn_sdf_query_workspace_bytes
    # chunk = min(chunk_rows or 2^20, rows): one chunk's points (16 bytes a row, rounded up to 256) + its query
    assert lib.cn_sdf_grid_workspace_bytes(ctypes.byref(d)) == _rup(total * 16) + q(ctypes.byref(n), total)
    d.chunk_rows = 4096
    want = _rup(4096 * 16) + q(ctypes.byref(n), 4096)
    assert lib.cn_sdf_grid_workspace_bytes(ctypes.byref(d)) == want
    assert q(ctypes.byref(n), 4096) == 2 * 4096 * 64 * 4  # (the fused bf16x6 query: two fp32 [M][64] inputs)
    assert lib.cn_sdf_grid(ctypes.byref(d), 4096, want - 1, None) == -2
    assert b"workspace" in lib.cn_last_error()
    d.nx = d.ny = d.nz = 256
    d.chunk_rows = 0
    assert lib.cn_sdf_grid_workspace_bytes(ctypes.byref(d)) == _rup((1 << 20) * 16) + q(ctypes.byref(n), 1 << 20)
    # a chunk at the fused query's row bound (M x 64 x 4 bytes < 2^31) is refused up front
    d.chunk_rows = 1 << 23
    assert lib.cn_sdf_grid_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.cn_sdf_grid(ctypes.byref(d), 4096, 1 << 40, None) == -2
    assert b"chunk_rows" in lib.cn_last_error()
    d.chunk_rows = (1 << 23) - 1
    assert lib.cn_sdf_grid_workspace_bytes(ctypes.byref(d)) > 0
    d.chunk_rows = -1
    assert lib.cn_sdf_grid(ctypes.byref(d), 4096, 1 << 40, None) == -2
    d.chunk_rows, d.nx = 0, 0
    assert lib.cn_sdf_grid(ctypes.byref(d), 4096, 1 << 40, None) == -2
    d.nx, d.net = 256, None
    assert lib.cn_sdf_grid(ctypes.byref(d), 4096, 1 << 40, None) == -1


def _read_ply(path):
    with open(path, "rb") as f:
        raw = f.read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = next(int(l.split()[2]) for l in lines if l.startswith("element vertex"))
    nf = next(int(l.split()[2]) for l in lines if l.startswith("element face"))
    props = [l.split()[2] for l in lines if l.startswith("property float")]
    assert "property list uchar int vertex_indices" in lines
    vert = np.frombuffer(body, dtype="<f4", count=nv * len(props)).reshape(nv, len(props))
    faces = np.frombuffer(body, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=nf, offset=vert.nbytes)
    assert vert.nbytes + faces.nbytes == len(body)
    assert (faces["n"] == 3).all()
    return props, vert, faces["i"]


def test_write_ply_round_trip(tmp_path):
    from copenerf import write_ply
    import model
    assert model.write_ply is write_ply
    rng = np.random.default_rng(0)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    n = rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    p = str(tmp_path / "a.ply")
    write_ply(p, v, f)
    props, vert, faces = _read_ply(p)
    assert props == ["x", "y", "z"]
    assert np.array_equal(vert, v) and np.array_equal(faces, f)
    write_ply(p, v, f, normals=n)
    props, vert, faces = _read_ply(p)
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(vert[:, :3], v) and np.array_equal(vert[:, 3:], n) and np.array_equal(faces, f)
    write_ply(p, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    props, vert, faces = _read_ply(p)
    assert vert.shape == (0, 3) and faces.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(p, v, f + 7)


def test_extract_geometry_refuses_cpu_modules():
    from copenerf import NeuSRenderer
    sdf, col, dev = build_modules(0, dh_sdf=64, dh_col=64)
    r = NeuSRenderer(None, sdf, dev, col, None, **REN_CFG)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.extract_geometry(torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0]), 8, 0.0)
    from copenerf import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.isosurface(torch.zeros(4, 4, 4), 0.0, (-1, -1, -1), (1, 1, 1))
