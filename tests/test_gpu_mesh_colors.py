"""Vertex colours on the device: cn_vertex_dirs, cn_rgb8_pack and cn_point_colors against copenerf's own
composition (bitwise), a float64 restatement of the directions, oracle.neus_oracle's networks, and
tools/extract_mesh.py end to end.

Bars.  cn_point_colors against the composition SDFNetwork.field / ops.vertex_dirs / RenderingNetwork.color: the
same launches with the same descriptors, so bitwise, for every chunk_rows.  cn_vertex_dirs against float64:
2^-22 per component (components are at most 1; the squares, the two sums, the square root and the quotient round
seven times, which bounds the relative error of a component by 3.5 x 2^-24).  rgb8: bitwise the torch formula.
Colours against the oracle in fp32 and bf16x6: max |d rgb| <= max(1e-4, 4 e32), e32 the fp32 oracle's own error
against the float64 oracle at the same vertices (1e-4: the project's bar for colour outputs; 4: the device's other
summation order); in bf16 a relative L2 error of 5e-2 (test_gpu_mesh.py's and test_gpu_bf16.py's bar for that
mode's outputs).  The 8-bit colours: within one level of the oracle's."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import GOLDEN, REN_CFG, build_modules
from oracle import neus_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["fp32", "bf16x6", "bf16"]
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
M_ROWS = 1537


def _renderer(mods, mode):
    from copenerf import NeuSRenderer
    sdf, col, dev = mods
    return NeuSRenderer(None, sdf, dev, col, None, **REN_CFG).to(DEV).set_mfma_dtype(mode)


def _points(M, seed=3):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return ((torch.rand(M, 3, device=DEV, generator=gen) - 0.5) * 1.6).contiguous()


def _packs(r):
    sdf_packed = r.sdf_network.params_and_pack()
    fold = r._can_fold()
    col_packed = r.color_network.params_and_pack(
        fold_feature=(sdf_packed[0][-1], sdf_packed[1][-1]) if fold else None)
    return sdf_packed, col_packed, fold


def _composition(r, x, t, fixed=None):
    """The module composition of vertex colours in one piece: (rgb [M, 3], ∇ₓSDF [M, 4])."""
    from copenerf import ops
    sdf_packed, col_packed, fold = _packs(r)
    M = x.shape[0]
    pts_time = torch.cat([x, t.expand(M, 1)], dim=1)
    _, feat, G = r.sdf_network.field(pts_time, want_feat="hidden" if fold else True, want_grad=True, packed=sdf_packed)
    dirs = ops.vertex_dirs(G) if fixed is None else fixed.expand(M, 3).contiguous()
    return r.color_network.color(pts_time, G, dirs, 1, feat, packed=col_packed), G


def _c_colors(r, x, t, **kw):
    from copenerf import ops
    sdf_packed, col_packed, _ = _packs(r)
    sn, k1 = ops.sdf_net(r.sdf_network.layout(), sdf_packed[2])
    cn, k2 = ops.color_net(r.color_network.layout(), col_packed[2])
    out = ops.point_colors(sn, cn, x, t, **kw)
    torch.cuda.synchronize()
    del k1, k2
    return out


def _unit64(v):
    """(float)(v / |v|) with the quotient in float64: cn_point_colors' fixed direction, restated."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    return (v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])).astype(np.float32)


def _rgb8_formula(rgb):
    return (rgb.clamp(0, 1) * 255 + 0.5).floor().to(torch.uint8)


# -- 1. the composition, bitwise -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_point_colors_is_the_composition_for_every_chunk(mode):
    from copenerf import ops
    r = _renderer(build_modules(7, device=DEV), mode)
    assert r._can_fold()
    x = _points(M_ROWS)
    t = ops.device_scalar(0.3, torch.device(DEV))
    with torch.no_grad():
        want, G = _composition(r, x, t)
        fixed_dir = (0.3, -0.5, 0.8)
        want_fixed, _ = _composition(r, x, t, fixed=torch.from_numpy(_unit64(fixed_dir)).to(DEV).view(1, 3))
        for chunk in (0, 512, M_ROWS, 4096):  # 2^18 (one chunk), a ragged last chunk, an exact fit, one chunk
            rgb, rgb8, grad = _c_colors(r, x, t, chunk_rows=chunk, want_rgb8=True, want_grad=True)
            assert rgb.shape == (M_ROWS, 3) and rgb.dtype == torch.float32 and grad.shape == (M_ROWS, 4)
            assert torch.equal(rgb, want), (mode, chunk, (rgb - want).abs().max().item())
            assert torch.equal(grad, G), (mode, chunk, (grad - G).abs().max().item())
            assert rgb8.dtype == torch.uint8 and torch.equal(rgb8, _rgb8_formula(rgb)), (mode, chunk)
            assert torch.equal(_c_colors(r, x, t, chunk_rows=chunk), want)  # without the optional outputs
            assert torch.equal(r.vertex_colors(x, 0.3, chunk_rows=chunk), want)
            # one fixed view direction on every row
            got = _c_colors(r, x, t, chunk_rows=chunk, view_dir=fixed_dir)
            assert torch.equal(got, want_fixed), (mode, chunk, (got - want_fixed).abs().max().item())
        assert not torch.equal(want_fixed, want)
        assert (want_fixed - want).abs().max().item() > 1e-3  # the direction reaches the colour
        assert torch.equal(r.vertex_colors(x, 0.3, view_dir=fixed_dir), want_fixed)
        assert torch.equal(r.vertex_colors(x, 0.3, view_dir=[3.0, -5.0, 8.0]),
                           _composition(r, x, t, fixed=torch.from_numpy(_unit64((3.0, -5.0, 8.0))).to(DEV).view(1, 3))[0])
        # M = 0
        e = _c_colors(r, x[:0], t, want_rgb8=True, want_grad=True)
        assert e[0].shape == (0, 3) and e[1].shape == (0, 3) and e[2].shape == (0, 4)
        assert r.vertex_colors(x[:0], 0.3).shape == (0, 3)
    with pytest.raises(RuntimeError, match="view_dir"):
        _c_colors(r, x, t, view_dir=(0.0, 0.0, 0.0))
    with pytest.raises(RuntimeError):
        ops.point_colors(None, None, x[:, :2], t)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_point_colors_refuses_networks_that_do_not_fold_and_vertex_colors_composes(mode):
    """SDF width 64 with a 256-wide feature: the feature head cannot fold (the configuration
    test_gpu_render_fwd.py skips).  cn_point_colors returns CN_ERR_UNSUPPORTED; NeuSRenderer.vertex_colors takes the
    module composition, in chunks."""
    from copenerf import ops
    r = _renderer(build_modules(7, dh_sdf=64, dh_col=64, device=DEV), mode)
    assert not r._can_fold()
    x = _points(M_ROWS)
    t = ops.device_scalar(0.3, torch.device(DEV))
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"cn_point_colors failed \(-5\).*folded feature head"):
            _c_colors(r, x, t)
        want, _ = _composition(r, x, t)
        for chunk in (0, 512, M_ROWS):
            assert torch.equal(r.vertex_colors(x, 0.3, chunk_rows=chunk), want), (mode, chunk)
        fixed_dir = (0.0, 0.0, -2.0)
        want_fixed, _ = _composition(r, x, t, fixed=torch.from_numpy(_unit64(fixed_dir)).to(DEV).view(1, 3))
        assert torch.equal(r.vertex_colors(x, 0.3, view_dir=fixed_dir, chunk_rows=512), want_fixed)
        assert not torch.equal(want_fixed, want)


# -- 2. cn_vertex_dirs -----------------------------------------------------------------------------------
def test_vertex_dirs_against_float64_zero_rows_and_both_signs():
    from copenerf import ops
    gen = torch.Generator(device=DEV).manual_seed(11)
    M = 70001  # many workgroups, the last one ragged
    big = torch.randn(M, 8, device=DEV, generator=gen)
    big[:, :3] *= torch.exp(torch.randn(M, 1, device=DEV, generator=gen) * 3.0)  # lengths over many octaves
    big[5, :3] = 0.0
    big[M - 1, :3] = 0.0
    big[7, :3] = torch.tensor([1e-20, 0.0, 0.0])  # below the floor of 1e-12 (its square underflows to 0)
    big[9, :3] = torch.tensor([0.0, -3.0, 0.0])
    for G in (big[:, :4].contiguous(), big[:, :4], big[:, :3]):  # ld 4, ld 8 (a column view), three columns
        g64 = G[:, :3].cpu().numpy().astype(np.float64)
        n32 = np.sqrt((g64 ** 2).sum(axis=1, keepdims=True))
        for sign in (-1.0, 1.0):
            got = ops.vertex_dirs(G, sign)
            assert got.shape == (M, 3) and got.is_contiguous()
            want = sign * g64 / np.maximum(n32, 1e-12)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            normal = n32[:, 0] > 1e-12
            print("vertex_dirs sign", sign, "ld", G.stride(0), "max error", err[normal].max())
            assert err[normal].max() <= 2.0 ** -22, err[normal].max()
            assert not bool(torch.isnan(got).any())
            z = got[[5, M - 1]]
            assert bool((z == 0).all())  # exact zeros (of either sign), no NaN
            assert got[7, 0].item() == pytest.approx(sign * 1e-8, rel=1e-6)  # divided by the floor, not by its length
            assert torch.equal(got[9], torch.tensor([0.0, -3.0, 0.0], device=DEV) * sign / 3.0)
        assert torch.equal(ops.vertex_dirs(G, 1.0), -ops.vertex_dirs(G, -1.0))
        assert torch.equal(ops.vertex_dirs(G), ops.vertex_dirs(G, -1.0))  # the default: inward
    assert ops.vertex_dirs(big[:0, :4]).shape == (0, 3)
    out = torch.empty(M, 3, device=DEV)
    assert ops.vertex_dirs(big[:, :4], out=out) is out
    with pytest.raises(RuntimeError):
        ops.vertex_dirs(big[:, :2])
    with pytest.raises(RuntimeError):
        ops.vertex_dirs(big[:, :4], out=torch.empty(M, 4, device=DEV))


# -- 3. rgb8 ---------------------------------------------------------------------------------------------
def test_rgb8_pack_is_the_torch_formula_with_nan_and_out_of_range_rows():
    from copenerf import ops
    gen = torch.Generator(device=DEV).manual_seed(4)
    rgb = torch.rand(3001, 3, device=DEV, generator=gen) * 1.5 - 0.25  # below 0 and above 1 among them
    levels = torch.arange(0, 256, device=DEV, dtype=torch.float32)
    edge = torch.cat([(levels + 0.5) / 255.0, levels / 255.0, (levels + 0.5) / 255.0 - 1e-7])  # rounding boundaries
    rgb[:256] = edge.view(3, 256).t()
    rgb[300] = torch.tensor([-1.0, 0.0, -0.0])
    rgb[301] = torch.tensor([1.0, 1.0 + 1e-6, 7.5])
    rgb[302] = torch.tensor([float("inf"), float("-inf"), 0.5])
    rgb[303] = float("nan")
    rgb[304, 1] = float("nan")
    rgb[3000, 2] = float("nan")
    got = ops.rgb8_pack(rgb)
    assert got.dtype == torch.uint8 and got.shape == rgb.shape
    want = _rgb8_formula(torch.nan_to_num(rgb, nan=0.0, posinf=float("inf"), neginf=float("-inf")))  # NaN -> 0
    assert torch.equal(got, want)
    assert bool((got[torch.isnan(rgb)] == 0).all()) and int(torch.isnan(rgb).sum()) == 5
    assert got[300].tolist() == [0, 0, 0] and got[301].tolist() == [255, 255, 255] and got[302].tolist() == [255, 0, 128]
    flat = ops.rgb8_pack(rgb.reshape(-1))  # any contiguous shape
    assert torch.equal(flat.view(-1, 3), got)
    with pytest.raises(RuntimeError):
        ops.rgb8_pack(rgb[:, :2])
    with pytest.raises(RuntimeError):
        ops.rgb8_pack(rgb.double())


# -- 4. the oracle ---------------------------------------------------------------------------------------
def _oracle_colors(r, x, dtype):
    sdfn, col = r.sdf_network, r.color_network
    W, b = O.params_from_module(sdfn)
    Wc, bc = O.params_from_module(col)
    cast = lambda ts: [t.to(dtype) for t in ts]  # noqa: E731
    P = O.SDFParams(cast(W), cast(b), skip=sdfn.skip_in[0], multires=sdfn.multires, scale=sdfn.scale)
    Pc = O.ColorParams(cast(Wc), cast(bc), multires_view=col.multires_view)
    x = x.to(dtype)
    with torch.no_grad():
        feat = O.sdf_mlp(P, x)[:, 1:]
    g = O.sdf_gradient(P, x).detach()
    with torch.no_grad():
        dirs = -torch.nn.functional.normalize(g[:, :3], dim=-1)
        return O.color_mlp(Pc, x, g, dirs, feat)


@pytest.mark.parametrize("mode", MODES)
def test_vertex_colors_match_the_oracle_on_the_geometric_init_sphere(mode):
    """Measured on an MI355X (1,718 vertices at resolution 33, t = 0.3; 1,720 in bf16), against the float64 oracle:
    e32 = 5.7e-8; fp32 max |d rgb| 5.7e-8, bf16x6 5.9e-8 (bar 1e-4); bf16 max 3.8e-5, relative L2 1.7e-5 (bar 5e-2);
    the 8-bit colours equal the oracle's in fp32 and bf16x6 and differ by at most one level in bf16."""
    from copenerf import ops
    r = _renderer(build_modules(7, device=DEV), mode)
    lo, hi = torch.tensor(BOX[0]), torch.tensor(BOX[1])
    v, tri, c8 = r.extract_geometry(lo, hi, 33, 0.0, time_step=0.3, with_colors=True)
    assert len(v) > 1000 and c8.dtype == np.uint8 and c8.shape == v.shape
    x = torch.cat([torch.from_numpy(v), torch.full((len(v), 1), 0.3)], dim=1)
    ref32 = _oracle_colors(r, x, torch.float32).double()
    ref64 = _oracle_colors(r, x, torch.float64)
    e32 = (ref32 - ref64).abs().max().item()
    with torch.no_grad():
        rgb = r.vertex_colors(torch.from_numpy(v).to(DEV), 0.3)
    got = rgb.cpu().double()
    err = (got - ref64).abs().max().item()
    rel = ((got - ref64).norm() / ref64.norm()).item()
    want8 = (ref64.clamp(0, 1) * 255 + 0.5).floor().to(torch.int64)
    d8 = (torch.from_numpy(c8).to(torch.int64) - want8).abs().max().item()
    print(mode, "V", len(v), "vertex colours vs float64 oracle: max", err, "relative L2", rel, "| e32", e32,
          "| vs fp32 oracle: max", (got - ref32).abs().max().item(), "| 8-bit levels", d8)
    assert torch.equal(torch.from_numpy(c8).to(DEV), ops.rgb8_pack(rgb))
    if mode == "bf16":
        assert rel <= 5e-2, rel
    else:
        assert err <= max(1e-4, 4 * e32), (err, e32)
    assert d8 <= 1, d8


# -- 5. end to end ---------------------------------------------------------------------------------------
def _extract_mesh():
    root = os.path.dirname(GOLDEN.rstrip(os.sep))
    sys.path.insert(0, os.path.join(os.path.dirname(root), "tools"))
    import extract_mesh
    return extract_mesh, os.path.join(GOLDEN, "ref_checkpoint.pt")


def test_extract_geometry_cleans_first_and_appends_colors_after_normals():
    from copenerf import ops
    r = _renderer(build_modules(7, device=DEV), "bf16x6")
    lo, hi = torch.tensor(BOX[0]), torch.tensor(BOX[1])
    plain = r.extract_geometry(lo, hi, 33, 0.0, time_step=0.3, with_normals=True)
    stats = {}
    v, tri, nrm, c8 = r.extract_geometry(lo, hi, 33, 0.0, time_step=0.3, with_normals=True, with_colors=True,
                                         keep_largest=True, stats=stats)
    # the sphere is one component: cleaning keeps all of it, bit for bit
    assert stats["components"] == stats["components_kept"] == 1
    assert np.array_equal(v, plain[0]) and np.array_equal(tri, plain[1]) and np.array_equal(nrm, plain[2])
    with torch.no_grad():
        rgb = r.vertex_colors(torch.from_numpy(v).to(DEV), 0.3)
    assert c8.dtype == np.uint8 and np.array_equal(c8, ops.rgb8_pack(rgb).cpu().numpy())
    assert len(np.unique(c8)) > 1
    # a threshold no component reaches: empty arrays of the right types, normals and colours included
    e = r.extract_geometry(lo, hi, 33, 0.0, time_step=0.3, with_normals=True, with_colors=True,
                           min_triangles=len(tri) + 1)
    assert [a.shape for a in e] == [(0, 3)] * 4
    assert [a.dtype for a in e] == [np.float32, np.int32, np.float32, np.uint8]
    # a fixed view direction reaches the colours
    c8f = r.extract_geometry(lo, hi, 33, 0.0, time_step=0.3, with_colors=True, view_dir=(0.0, 0.0, 1.0))[2]
    assert c8f.shape == c8.shape and not np.array_equal(c8f, c8)


def test_extract_mesh_tool_writes_a_coloured_clean_ply(tmp_path, capsys):
    """tools/extract_mesh.py on the width-64 reference checkpoint (no fold: the module composition) at resolution
    25: with --colors --normals --keep-largest the PLY reads back to the returned arrays, the kept mesh is one
    component of the plain one; without the new flags the output is extract_geometry's, as test_gpu_mesh.py pins."""
    import mesh_clean_ref as C
    from test_mesh_color_host import _cols, _read_ply_any
    from test_mesh_host import _read_ply
    extract_mesh, path = _extract_mesh()
    base = [path, None, "--resolution", "25", "--time", "0.5", "--mode", "fp32"]
    out = str(tmp_path / "plain.ply")
    base[1] = out
    plain = extract_mesh.main(base + ["--normals"])
    assert "components" not in capsys.readouterr().out
    r = extract_mesh.build_renderer(path).to(DEV).set_mfma_dtype("fp32")
    assert not r._can_fold()
    res = r.extract_geometry(torch.tensor(BOX[0]), torch.tensor(BOX[1]), 25, 0.0, time_step=0.5, with_normals=True)
    assert len(plain) == 3 and all(np.array_equal(a, b) for a, b in zip(plain, res))
    props, vert, faces = _read_ply(out)
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(vert[:, :3], plain[0]) and np.array_equal(vert[:, 3:], plain[2]) and np.array_equal(faces, plain[1])
    out2 = str(tmp_path / "clean.ply")
    base[1] = out2
    v, tri, nrm, c8 = extract_mesh.main(base + ["--colors", "--normals", "--keep-largest"])
    line = capsys.readouterr().out
    kept_ref, tri_ref, lab, cnt = C.clean(plain[1], len(plain[0]), keep_largest=True)
    n_kept = len(np.unique(lab[kept_ref]))
    print("checkpoint mesh:", len(plain[0]), "vertices,", len(np.unique(lab)), "components,", n_kept, "kept")
    assert f"{len(np.unique(lab))} components found, {n_kept} kept" in line and f"{len(v)} vertices" in line
    assert np.array_equal(v, plain[0][kept_ref]) and np.array_equal(tri, tri_ref) and np.array_equal(nrm, plain[2][kept_ref])
    assert c8.dtype == np.uint8 and c8.shape == v.shape
    with torch.no_grad():
        rgb = r.vertex_colors(torch.from_numpy(v).to(DEV), 0.5)
    from copenerf import ops
    assert np.array_equal(c8, ops.rgb8_pack(rgb).cpu().numpy())
    props, vert, faces = _read_ply_any(out2)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(_cols(vert, ["x", "y", "z"]), v) and np.array_equal(_cols(vert, ["nx", "ny", "nz"]), nrm)
    assert np.array_equal(_cols(vert, ["red", "green", "blue"]), c8) and np.array_equal(faces, tri)
