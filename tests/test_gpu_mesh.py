"""Mesh extraction on the device (ABI v16): cn_grid_points, cn_sdf_grid, the marching-tetrahedra mesher
(cn_mesh_count / cn_mesh_emit) against the numpy reference tests/mesh_ref.py, and NeuSRenderer.extract_geometry
end to end.

Bars.  Triangles and counts: exact.  Vertices: 2e-6 x the largest |bound| (five or six fp32 roundings of 6e-8 on
quantities no larger than the bounds) against the reference's float64 positions.  Grid points: 2^-22 x the
largest |bound| against float64 linspace (two fp32 roundings).  SDF volume against oracle.neus_oracle: 1e-4 in
fp32 and bf16x6 (test_gpu_render.py's bar for the SDF); in bf16 a relative L2 error of 5e-2, the bar
test_gpu_bf16.py::test_sdf_field_bf16_mode_narrow_width applies to the SDF output."""
import os

import numpy as np
import pytest
import torch

import mesh_ref as R
from helpers import GOLDEN, REN_CFG, build_modules
from oracle import neus_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
VTX_REL = 2e-6


def _max_bound(lo, hi):
    return float(max(np.abs(np.asarray(lo)).max(), np.abs(np.asarray(hi)).max()))


# -- 1. grid points ------------------------------------------------------------------------------------
def test_grid_points_match_linspace_and_subranges_are_bitwise():
    from copenerf import ops
    dims, lo, hi, t = (5, 7, 11), (-0.7, -1.0, 0.1), (0.9, 0.4, 1.3), 0.3
    tt = ops.device_scalar(t, torch.device(DEV))
    pts = ops.grid_points(dims, lo, hi, tt)
    assert pts.shape == (5 * 7 * 11, 4)
    lo32, hi32 = np.float32(lo).astype(np.float64), np.float32(hi).astype(np.float64)
    ax = [np.linspace(l, h, n) for l, h, n in zip(lo32, hi32, dims)]
    ref = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)  # C order, z fastest
    got = pts.cpu().numpy()
    err = np.abs(got[:, :3].astype(np.float64) - ref).max()
    print("grid_points max error", err)
    assert err <= 2.0 ** -22 * _max_bound(lo, hi), err
    assert (got[:, 3] == np.float32(t)).all()
    for m0, M in ((0, 1), (37, 200), (384, 1), (100, 285)):
        sub = ops.grid_points(dims, lo, hi, tt, m0=m0, M=M)
        assert torch.equal(sub, pts[m0:m0 + M]), (m0, M)
    with pytest.raises(RuntimeError, match="rows"):
        ops.grid_points(dims, lo, hi, tt, m0=380, M=6)


# -- 2. the SDF volume ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dh, mode", [(256, "fp32"), (256, "bf16x6"), (256, "bf16"), (64, "fp32"),
                                      (64, "bf16x6"), (64, "bf16")])  # width 64: the layer path
def test_sdf_grid_is_the_composition_and_matches_the_oracle(dh, mode):
    from copenerf import ops
    sdfn = build_modules(7, dh_sdf=dh, device=DEV)[0]
    sdfn.mfma_dtype = mode
    lay = sdfn.layout()
    n, lo, hi = 21, BOX[0], BOX[1]
    t = ops.device_scalar(0.3, torch.device(DEV))
    with torch.no_grad():
        pk = sdfn.params_and_pack()[2]
        net, keep = ops.sdf_net(lay, pk)
        u3 = ops.sdf_grid(net, (n, n, n), lo, hi, t, chunk_rows=4096)  # three chunks, the last ragged
        u1 = ops.sdf_grid(net, (n, n, n), lo, hi, t, chunk_rows=n ** 3)
        u0 = ops.sdf_grid(net, (n, n, n), lo, hi, t)
        pts = ops.grid_points((n, n, n), lo, hi, t)
        uq = ops.sdf_query(net, pts, torch.empty(n ** 3, device=DEV))
        del keep
    assert torch.equal(u3, u1) and torch.equal(u0, u1)
    assert torch.equal(u1.reshape(-1), uq)
    ax = torch.linspace(-1.0, 1.0, n)
    x = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    x = torch.cat([x, torch.full((n ** 3, 1), 0.3)], 1)
    W, b = O.params_from_module(sdfn)
    P = O.SDFParams(W, b, skip=sdfn.skip_in[0], multires=sdfn.multires, scale=sdfn.scale)
    with torch.no_grad():
        ref = O.sdf_mlp(P, x)[:, 0]
    got = u1.reshape(-1).cpu()
    err = (got - ref).abs().max().item()
    rel = ((got - ref).norm() / ref.norm()).item()
    print(dh, mode, "sdf_grid vs oracle: max", err, "relative L2", rel)
    if mode == "bf16":
        assert rel <= 5e-2, rel  # test_gpu_bf16.py::test_sdf_field_bf16_mode_narrow_width's bar for the SDF
    else:
        assert err <= 1e-4, err  # test_gpu_render.py's bar for the SDF


# -- 3. the mesher against the host reference ----------------------------------------------------------
def _check_against_ref(u, thr, lo, hi, label):
    from copenerf import ops
    ud = torch.from_numpy(np.ascontiguousarray(u)).to(DEV)
    v, t = ops.isosurface(ud, thr, lo, hi)
    rv, rt = R.isosurface(u, thr, lo, hi)
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda and t.is_cuda
    assert v.shape == (len(rv), 3) and t.shape == (len(rt), 3), (label, v.shape, t.shape, rv.shape, rt.shape)
    assert np.array_equal(t.cpu().numpy(), rt), label
    err = float(np.abs(v.cpu().numpy().astype(np.float64) - rv).max()) if len(rv) else 0.0
    print(label, "V", len(rv), "T", len(rt), "vertex max error", err, "/ bound", err / _max_bound(lo, hi))
    assert err <= VTX_REL * _max_bound(lo, hi), (label, err)
    return v, t


def test_mesher_all_256_sign_patterns_of_one_cell():
    """Case A: every corner sign pattern of a single 2 x 2 x 2 cell, so every row of every tetrahedron's table;
    values +-(0.1 .. 0.8), distinct per corner."""
    mag = np.arange(1, 9, dtype=np.float32) / 10.0
    for pattern in range(256):
        sign = np.array([-1.0 if pattern >> i & 1 else 1.0 for i in range(8)], dtype=np.float32)
        u = (sign * mag).reshape(2, 2, 2)
        _check_against_ref(u, 0.0, (-0.5, 0.2, -1.0), (0.75, 1.1, 0.3), f"pattern {pattern}")


def test_mesher_smooth_random_field_odd_dims():
    """Case B: (5, 7, 11), a smooth random field, asymmetric bounds, a non-zero threshold."""
    rng = np.random.default_rng(3)
    x, y, z = R.grid((5, 7, 11), (0, 0, 0), (1, 1, 1))
    u = np.zeros_like(x)
    for _ in range(6):
        f = rng.uniform(0.5, 2.5, 3)
        ph = rng.uniform(0, 6.28, 3)
        u += rng.uniform(0.3, 1.0) * np.sin(6.28 * f[0] * x + ph[0]) * np.sin(6.28 * f[1] * y + ph[1]) * \
            np.sin(6.28 * f[2] * z + ph[2])
    u = u.astype(np.float32)
    _, t = _check_against_ref(u, 0.0, (-0.7, -1.0, 0.1), (0.9, 0.4, 1.3), "random")
    assert len(t) > 100
    _check_against_ref(u, 0.125, (-0.7, -1.0, 0.1), (0.9, 0.4, 1.3), "random thr 0.125")


@pytest.mark.parametrize("make", [R.sphere_tie, R.torus, R.two_spheres])
def test_mesher_analytic_volumes(make):
    """Case C: the tie sphere (six grid values equal the threshold), the torus, the two spheres."""
    _check_against_ref(make(), 0.0, *BOX, make.__name__)


def test_mesher_empty_volumes():
    """Case D: all positive / all negative: V = T = 0 with (0, 3) outputs."""
    from copenerf import ops
    for val in (0.5, -0.5):
        v, t = ops.isosurface(torch.full((6, 5, 4), val, device=DEV), 0.0, *BOX)
        assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32


def _sphere(dims, r):
    x, y, z = R.grid(dims, *BOX)
    return (np.sqrt(x * x + y * y + z * z) - r).astype(np.float32)


def test_mesher_many_scan_tiles():
    """Case E: (41, 40, 43), 70,520 grid vertices: 69 scan tiles of 1024 vertices, 64 of cells."""
    _check_against_ref(_sphere((41, 40, 43), 0.7), 0.0, *BOX, "sphere 41x40x43")


def test_mesher_scan_of_tile_totals_loops():
    """The scan's second level (one block over the tile totals) holds 1024 totals per round, which case E does
    not cross: (104, 103, 102) has 1,092,624 vertices and 1,061,106 cells, more than 1024 tiles of 1024 each,
    the smallest cubic-ish grid at which both scans take a second round."""
    dims = (104, 103, 102)
    assert (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1) > 1024 * 1024
    _check_against_ref(_sphere(dims, 0.9), 0.0, *BOX, "sphere 104x103x102")


def test_mesh_emit_writes_nothing_into_buffers_smaller_than_the_counts():
    from copenerf import ops
    u = torch.from_numpy(R.torus()).to(DEV)
    d, ws, counts = ops.mesh_count(u, 0.0, *BOX)
    V, T = counts.tolist()
    assert V > 0 and T > 0
    with pytest.raises(RuntimeError, match="buffers"):
        ops.mesh_emit(d, ws, torch.empty(V - 1, 3, device=DEV), torch.empty(T, 3, dtype=torch.int32, device=DEV), (V, T))
    v = torch.full((V - 1, 3), float("nan"), device=DEV)
    t = torch.full((T, 3), -7, dtype=torch.int32, device=DEV)
    ops.mesh_emit(d, ws, v, t)  # the kernel's own check against the device counts
    assert bool(torch.isnan(v).all()) and bool((t == -7).all())
    v = torch.empty(V, 3, device=DEV)
    ops.mesh_emit(d, ws, v, t, (V, T))
    v2, t2 = ops.isosurface(u, 0.0, *BOX)
    assert torch.equal(v, v2) and torch.equal(t, t2)


# -- 4. end to end -------------------------------------------------------------------------------------
def _renderer(mods, mode):
    from copenerf import NeuSRenderer
    sdf, col, dev = mods
    return NeuSRenderer(None, sdf, dev, col, None, **REN_CFG).to(DEV).set_mfma_dtype(mode)


def _matches_ref(r, res, n, t):
    u = r.sdf_volume(BOX[0], BOX[1], n, t).cpu().numpy()
    rv, rt = R.isosurface(u, 0.0, *BOX)
    assert res[0].dtype == np.float32 and res[1].dtype == np.int32
    assert res[0].shape == (len(rv), 3) and np.array_equal(res[1], rt)
    err = float(np.abs(res[0].astype(np.float64) - rv).max()) if len(rv) else 0.0
    print("extract_geometry V", len(rv), "T", len(rt), "vertex max error", err)
    assert err <= VTX_REL * 1.0, err
    return rv, rt


def test_extract_geometry_geometric_init_sphere_with_normals():
    r = _renderer(build_modules(7, device=DEV), "bf16x6")
    lo, hi = torch.tensor(BOX[0]), torch.tensor(BOX[1])
    v, tri, nrm = r.extract_geometry(lo, hi, 33, 0.0, time_step=0.3, with_normals=True)
    v2, tri2 = r.extract_geometry(lo, hi, 33, time_step=0.3)
    assert np.array_equal(v, v2) and np.array_equal(tri, tri2)
    _matches_ref(r, (v, tri), 33, 0.3)
    assert len(tri) > 0
    assert R.is_closed_oriented(tri, len(v))
    assert R.euler_characteristic(tri, len(v)) == 2
    assert R.signed_volume(v, tri) > 0
    # the normals: normalised SDFNetwork.gradient at (vertex, t)
    x = torch.cat([torch.from_numpy(v).to(DEV), torch.full((len(v), 1), 0.3, device=DEV)], 1)
    g = r.sdf_network.gradient(x)[:, 0, :3].detach()
    want = torch.nn.functional.normalize(g, dim=-1).cpu().numpy()
    assert nrm.dtype == np.float32 and np.array_equal(nrm, want)
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
    # and they agree with the triangles' orientation at every vertex
    a, b, c = (v[tri[:, i]].astype(np.float64) for i in range(3))
    fn = np.cross(b - a, c - a)  # area-weighted
    acc = np.zeros((len(v), 3))
    for i in range(3):
        np.add.at(acc, tri[:, i], fn)
    dots = np.einsum("ij,ij->i", acc, nrm.astype(np.float64))
    assert (dots > 0).all(), int((dots <= 0).sum())


def _checkpoint_renderer():
    import sys
    root = os.path.dirname(GOLDEN.rstrip(os.sep))
    sys.path.insert(0, os.path.join(os.path.dirname(root), "tools"))
    import extract_mesh
    return extract_mesh, os.path.join(GOLDEN, "ref_checkpoint.pt")


def test_extract_geometry_reference_checkpoint_layer_path_and_tool(tmp_path):
    """The width-64 reference checkpoint (the layer path: the fused query covers width 256 only) matches the host
    reference, whatever surface it holds; tools/extract_mesh.py writes a PLY that reads back to the same arrays."""
    from test_mesh_host import _read_ply
    extract_mesh, path = _checkpoint_renderer()
    r = extract_mesh.build_renderer(path).to(DEV).set_mfma_dtype("fp32")
    assert r.sdf_network.layout().HL == 128
    res = r.extract_geometry(torch.tensor(BOX[0]), torch.tensor(BOX[1]), 25, 0.0, time_step=0.5)
    _matches_ref(r, res, 25, 0.5)
    out = str(tmp_path / "mesh.ply")
    got = extract_mesh.main([path, out, "--resolution", "25", "--time", "0.5", "--mode", "fp32", "--normals"])
    assert np.array_equal(got[0], res[0]) and np.array_equal(got[1], res[1])
    props, vert, faces = _read_ply(out)
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(vert[:, :3], got[0]) and np.array_equal(vert[:, 3:], got[2]) and np.array_equal(faces, got[1])
