"""Coloured, floater-free mesh export without a device: the new entry points are exported and bound in the
header's field order, refuse bad arguments on the host and size their workspaces by the header's formulas; the PLY
writer's colour properties; and the host reference of floater removal (tests/mesh_clean_ref.py) against scipy's
connected components and the mesh properties of tests/mesh_ref.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import mesh_clean_ref as C
import mesh_ref as R
from test_abi import _fake_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "copenerf.h")
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
NEW = ["cn_vertex_dirs", "cn_rgb8_pack", "cn_point_colors_workspace_bytes", "cn_point_colors", "cn_mesh_label_init",
       "cn_mesh_label_rounds", "cn_mesh_component_sizes", "cn_mesh_clean_workspace_bytes", "cn_mesh_select",
       "cn_mesh_compact"]


def _rup(n, a=256):
    return (n + a - 1) // a * a


# -- 1. the ABI ----------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    from copenerf import _lib
    lib = _lib.load()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, src), name


def test_descriptor_layouts_match_header_order():
    from copenerf import _lib
    src = open(HEADER).read()
    for cname, py in (("cn_point_colors_desc", _lib.PointColorsDesc), ("cn_mesh_clean_desc", _lib.MeshCleanDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            decl = re.sub(r"^(const\s+)?\w+\s*\**", "", decl)
            names += [n.strip(" *") for n in decl.split(",")]
        assert names == [f[0] for f in py._fields_], (cname, names)
        assert ctypes.sizeof(py) % 8 == 0
    # the C layout: 8-byte pointers and int64 on natural alignment
    assert _lib.PointColorsDesc.chunk_rows.offset == 48 and _lib.PointColorsDesc.rgb.offset == 56
    assert ctypes.sizeof(_lib.PointColorsDesc) == 80
    assert _lib.MeshCleanDesc.triangles.offset == 8 and _lib.MeshCleanDesc.counts.offset == 40
    assert ctypes.sizeof(_lib.MeshCleanDesc) == 80


def test_mesh_clean_entry_points_check_on_the_host():
    from copenerf import _lib
    lib = _lib.load()
    assert lib.cn_mesh_label_init(None, None) == -1
    assert b"null descriptor" in lib.cn_last_error()
    assert lib.cn_mesh_label_rounds(None, 4, 4096, None) == -1
    assert lib.cn_mesh_component_sizes(None, None) == -1
    assert lib.cn_mesh_select(None, 4096, 1 << 20, None) == -1
    assert lib.cn_mesh_compact(None, 4096, 1 << 20, None) == -1
    assert b"null descriptor" in lib.cn_last_error()
    d = _lib.MeshCleanDesc()
    d.V, d.T = 10, 4
    need = lib.cn_mesh_clean_workspace_bytes(10, 4)
    calls = (lambda: lib.cn_mesh_label_init(ctypes.byref(d), None),
             lambda: lib.cn_mesh_label_rounds(ctypes.byref(d), 4, 4096, None),
             lambda: lib.cn_mesh_component_sizes(ctypes.byref(d), None),
             lambda: lib.cn_mesh_select(ctypes.byref(d), 4096, need, None),
             lambda: lib.cn_mesh_compact(ctypes.byref(d), 4096, need, None))
    for call in calls:  # null triangles, then null label
        d.triangles, d.label = None, 4096
        assert call() == -1
        assert b"null triangles" in lib.cn_last_error()
        d.triangles, d.label = 4096, None
        assert call() == -1
        assert b"null label" in lib.cn_last_error()
    d.triangles = d.label = d.tri_count = d.counts = 4096
    for V, T in ((-1, 4), (10, -1)):
        d.V, d.T = V, T
        for call in calls:
            assert call() == -2
            assert b"V %d, T %d" % (V, T) in lib.cn_last_error()
    d.V, d.T = 10, 4
    assert lib.cn_mesh_label_rounds(ctypes.byref(d), 0, 4096, None) == -2  # at least one round
    assert lib.cn_mesh_label_rounds(ctypes.byref(d), 4, None, None) == -1
    assert b"null changed" in lib.cn_last_error()
    d.tri_count = None
    assert lib.cn_mesh_component_sizes(ctypes.byref(d), None) == -1
    assert lib.cn_mesh_select(ctypes.byref(d), 4096, need, None) == -1
    assert b"null tri_count" in lib.cn_last_error()
    d.tri_count, d.counts = 4096, None
    assert lib.cn_mesh_select(ctypes.byref(d), 4096, need, None) == -1
    assert b"null counts" in lib.cn_last_error()
    d.counts = 4096
    assert lib.cn_mesh_select(ctypes.byref(d), 4096, need - 1, None) == -2
    assert b"workspace" in lib.cn_last_error()
    assert lib.cn_mesh_select(ctypes.byref(d), 4096 + 16, need, None) == -3
    assert lib.cn_mesh_select(ctypes.byref(d), None, need, None) == -2
    d.min_triangles = -1
    assert lib.cn_mesh_select(ctypes.byref(d), 4096, need, None) == -2
    assert b"min_triangles" in lib.cn_last_error()
    d.min_triangles, d.max_vertices = 0, 3  # compact: a capacity without a buffer
    assert lib.cn_mesh_compact(ctypes.byref(d), 4096, need, None) == -1
    assert b"null kept_vertices" in lib.cn_last_error()
    d.max_vertices = -1
    assert lib.cn_mesh_compact(ctypes.byref(d), 4096, need, None) == -2


def test_mesh_clean_workspace_formula():
    from copenerf import _lib
    lib = _lib.load()
    for V, T in ((0, 0), (1, 0), (19, 13), (1024, 1025), (4099, 4097), (3 * 10 ** 6, 6 * 10 ** 6)):
        want = (_rup(V) + _rup(T) + _rup(4 * V) + _rup(4 * T) + _rup(4 * max(1, -(-V // 1024))) +
                _rup(4 * max(1, -(-T // 1024))) + _rup(8))
        assert lib.cn_mesh_clean_workspace_bytes(V, T) == want, (V, T)
    assert lib.cn_mesh_clean_workspace_bytes(-1, 5) == 0
    assert lib.cn_mesh_clean_workspace_bytes(5, -1) == 0


def _fake_nets(mode=1):
    """The two networks of test_abi.py's cn_render_fwd checks: the full-width configuration, folded."""
    from copenerf import _lib
    n = _fake_net(mode=mode)
    for l in range(8):
        n.Wt[l], n.wt_rows[l], n.wt_cols[l] = 4096, 256, 256
    n.head_wp = 4096
    c = _lib.ColorNet()
    c.n_lin, c.d_feature, c.multires_view, c.mfma_dtype = 5, 256, 4, mode
    dims = [4 + 27 + 4 + 256, 256, 256, 256, 256]
    for l in range(5):
        c.in_dim[l], c.out_dim[l] = dims[l], (3 if l == 4 else 256)
    for l in range(4):
        c.W[l], c.w_rows[l], c.w_cols[l], c.bias[l] = 4096, 256, (256 + 64 if l == 0 else 256), 4096
    c.head_w = c.head_b = 4096
    return n, c


def test_point_colors_checks_and_plans_on_the_host():
    from copenerf import _lib
    lib = _lib.load()
    assert lib.cn_point_colors(None, 4096, 1 << 20, None) == -1
    assert b"null descriptor" in lib.cn_last_error()
    assert lib.cn_point_colors_workspace_bytes(None) == 0
    assert lib.cn_vertex_dirs(5, None, 4, -1.0, 4096, None) == -1
    assert lib.cn_vertex_dirs(5, 4096, 4, -1.0, None, None) == -1
    assert lib.cn_vertex_dirs(5, 4096, 2, -1.0, 4096, None) == -2  # fewer than three columns
    assert lib.cn_vertex_dirs(-1, 4096, 4, -1.0, 4096, None) == -2
    assert lib.cn_vertex_dirs(0, None, 4, -1.0, None, None) == 0
    assert lib.cn_rgb8_pack(3, None, 4096, None) == -1
    assert lib.cn_rgb8_pack(3, 4096, None, None) == -1
    assert lib.cn_rgb8_pack(-3, 4096, 4096, None) == -2
    assert lib.cn_rgb8_pack(0, None, None, None) == 0
    n, c = _fake_nets()
    d = _lib.PointColorsDesc()
    d.M, d.x, d.time_step, d.rgb = 1537, 4096, 4096, 4096
    assert lib.cn_point_colors(ctypes.byref(d), 4096, 1 << 40, None) == -1  # null networks
    assert lib.cn_point_colors_workspace_bytes(ctypes.byref(d)) == 0
    d.sdf_net, d.color_net = ctypes.pointer(n), ctypes.pointer(c)
    ws = lib.cn_point_colors_workspace_bytes(ctypes.byref(d))
    # at least the chunk's own rows (pts, sdf, ∇ₓSDF, dirs) and the eight kept bf16 activations
    assert ws >= _rup(1537 * 16) * 2 + _rup(1537 * 4) + _rup(1537 * 12) + 7 * 1537 * 256 * 2
    d.chunk_rows = 512  # the plan is one chunk's
    ws512 = lib.cn_point_colors_workspace_bytes(ctypes.byref(d))
    assert 0 < ws512 < ws
    d.chunk_rows = 4096  # more than M: M rows
    assert lib.cn_point_colors_workspace_bytes(ctypes.byref(d)) == ws
    d.chunk_rows = 0
    assert lib.cn_point_colors(ctypes.byref(d), 4096, ws - 1, None) == -2
    assert b"workspace" in lib.cn_last_error()
    assert lib.cn_point_colors(ctypes.byref(d), 4096 + 16, ws, None) == -3
    d.grad = 4096 + 4
    assert lib.cn_point_colors(ctypes.byref(d), 4096, ws, None) == -3  # grad rows are 16-byte vectors
    d.grad, d.rgb = None, None
    assert lib.cn_point_colors(ctypes.byref(d), 4096, ws, None) == -1
    d.rgb, d.M = 4096, -1
    assert lib.cn_point_colors(ctypes.byref(d), 4096, ws, None) == -2
    assert lib.cn_point_colors_workspace_bytes(ctypes.byref(d)) == 0
    d.M, d.chunk_rows = 1537, -1
    assert lib.cn_point_colors(ctypes.byref(d), 4096, ws, None) == -2
    # M = 0 writes nothing and needs nothing
    d.M, d.chunk_rows, d.x, d.rgb = 0, 0, None, None
    assert lib.cn_point_colors_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.cn_point_colors(ctypes.byref(d), None, 0, None) == 0
    # a chunk whose widest row (256 floats) reaches 2^31 bytes is refused before anything launches
    d.M, d.x, d.rgb, d.chunk_rows = 1 << 23, 4096, 4096, 1 << 21
    assert lib.cn_point_colors(ctypes.byref(d), 4096, 1 << 50, None) == -2
    assert b"2^31" in lib.cn_last_error()
    assert lib.cn_point_colors_workspace_bytes(ctypes.byref(d)) == 0
    d.chunk_rows = (1 << 21) - 1
    assert lib.cn_point_colors_workspace_bytes(ctypes.byref(d)) > 0
    d.chunk_rows = 0  # the default chunk, 2^18 rows, is below the bound
    assert lib.cn_point_colors_workspace_bytes(ctypes.byref(d)) > 0
    # a fixed direction that has none
    d.M = 1537
    zero = (_lib.c_f32 * 3)(0.0, 0.0, 0.0)
    d.view_dir = ctypes.cast(zero, ctypes.POINTER(_lib.c_f32))
    assert lib.cn_point_colors(ctypes.byref(d), 4096, ws, None) == -1
    assert b"view_dir" in lib.cn_last_error()
    d.view_dir = None
    # the networks: equal GEMM modes, the folded feature head
    c.mfma_dtype = 2
    assert lib.cn_point_colors(ctypes.byref(d), 4096, ws, None) == -1
    assert b"cn_point_colors: the networks' GEMM modes differ" in lib.cn_last_error()
    c.mfma_dtype, c.d_feature = 1, 128  # no fold: the colour network's feature is not the SDF's hidden layer
    c.in_dim[0] = 4 + 27 + 4 + 128
    c.w_cols[0] = 128 + 64
    assert lib.cn_point_colors(ctypes.byref(d), 4096, ws, None) == -5
    assert b"folded feature head" in lib.cn_last_error()
    assert lib.cn_point_colors_workspace_bytes(ctypes.byref(d)) == 0


# -- 2. the PLY writer ---------------------------------------------------------------------------------
def _read_ply_any(path):
    """(property names, vertex records as a structured array, faces [T, 3]) of a binary little-endian PLY with
    float and uchar vertex properties."""
    with open(path, "rb") as f:
        raw = f.read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = next(int(l.split()[2]) for l in lines if l.startswith("element vertex"))
    nf = next(int(l.split()[2]) for l in lines if l.startswith("element face"))
    first_face = lines.index(next(l for l in lines if l.startswith("element face")))
    fields = []
    for l in lines[:first_face]:
        if l.startswith("property "):
            _, typ, name = l.split()
            fields.append((name, {"float": "<f4", "uchar": "u1"}[typ]))
    assert lines[first_face + 1] == "property list uchar int vertex_indices"
    vdt = np.dtype(fields)
    vert = np.frombuffer(body, dtype=vdt, count=nv)
    faces = np.frombuffer(body, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=nf, offset=vert.nbytes)
    assert vert.nbytes + faces.nbytes == len(body)
    assert (faces["n"] == 3).all()
    return [n for n, _ in fields], vert, faces["i"]


def _cols(vert, names):
    return np.stack([vert[n] for n in names], axis=1)


def test_write_ply_colors_round_trip(tmp_path):
    from copenerf import write_ply
    rng = np.random.default_rng(1)
    v = rng.standard_normal((9, 3)).astype(np.float32)
    n = rng.standard_normal((9, 3)).astype(np.float32)
    c = rng.integers(0, 256, size=(9, 3)).astype(np.uint8)
    c[0], c[1] = 0, 255
    f = rng.integers(0, 9, size=(6, 3)).astype(np.int32)
    p = str(tmp_path / "c.ply")
    write_ply(p, v, f, normals=n, colors=c)
    props, vert, faces = _read_ply_any(p)
    assert props == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(_cols(vert, ["x", "y", "z"]), v) and np.array_equal(_cols(vert, ["nx", "ny", "nz"]), n)
    assert np.array_equal(_cols(vert, ["red", "green", "blue"]), c) and np.array_equal(faces, f)
    write_ply(p, v, f, colors=c)
    props, vert, faces = _read_ply_any(p)
    assert props == ["x", "y", "z", "red", "green", "blue"]
    assert np.array_equal(_cols(vert, ["x", "y", "z"]), v) and np.array_equal(_cols(vert, ["red", "green", "blue"]), c)
    assert np.array_equal(faces, f)
    e3 = np.zeros((0, 3), np.float32)
    write_ply(p, e3, np.zeros((0, 3), np.int32), normals=e3, colors=np.zeros((0, 3), np.uint8))
    props, vert, faces = _read_ply_any(p)
    assert len(props) == 9 and len(vert) == 0 and faces.shape == (0, 3)
    for bad in (c.astype(np.float32) / 255.0, c.astype(np.int32), c[:8], c[:, :2], np.concatenate([c, c[:, :1]], 1)):
        with pytest.raises(ValueError, match="colors"):
            write_ply(p, v, f, colors=bad)


def test_write_ply_without_colors_writes_the_same_bytes_as_before(tmp_path):
    """colors=None: byte for byte the file of the writer before colours existed, restated here."""
    from copenerf import write_ply
    rng = np.random.default_rng(2)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    n = rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, size=(5, 3)).astype(np.int32)
    faces = np.empty(5, dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"], faces["i"] = 3, f
    for normals in (None, n):
        props = ["property float x", "property float y", "property float z"]
        cols = [v]
        if normals is not None:
            props += ["property float nx", "property float ny", "property float nz"]
            cols.append(normals)
        header = "\n".join(["ply", "format binary_little_endian 1.0", "comment copenerf extract_geometry",
                            "element vertex 7", *props, "element face 5",
                            "property list uchar int vertex_indices", "end_header"]) + "\n"
        want = header.encode("ascii") + np.concatenate(cols, axis=1).astype("<f4").tobytes() + faces.tobytes()
        p = str(tmp_path / "b.ply")
        write_ply(p, v, f, normals=normals)
        assert open(p, "rb").read() == want
        write_ply(p, v, f, normals=normals, colors=None)
        assert open(p, "rb").read() == want


# -- 3. the host reference of floater removal ------------------------------------------------------------
def _cases():
    cases = {}
    for make in (R.two_spheres, R.torus):
        v, t = R.isosurface(make(), 0.0, *BOX)
        cases[make.__name__] = (t, len(v), v)
    t, V = C.fans()
    cases["fans"] = (t, V, None)
    cases["strip"] = (C.strip(4099), 4099, None)
    cases["strip permuted"] = (C.strip(4099, seed=5), 4099, None)
    t, V = C.disjoint_strips(7, 33)
    cases["strips"] = (t, V, None)
    return cases


def test_reference_labels_are_component_minima_and_match_scipy():
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        coo_matrix = None
    want_components = {"two_spheres": 2, "torus": 1, "fans": 3, "strip": 1, "strip permuted": 1, "strips": 7}
    for name, (t, V, _) in _cases().items():
        lab = C.labels(t, V)
        assert lab.dtype == np.int32 and lab.shape == (V,)
        roots = np.unique(lab)
        assert len(roots) == want_components[name], name
        # a label is the smallest id that carries it, and a triangle's corners share one
        assert np.array_equal(lab[roots], roots) and (lab <= np.arange(V)).all()
        for r in roots:
            assert np.flatnonzero(lab == r).min() == r
        assert (lab[t[:, 0]] == lab[t[:, 1]]).all() and (lab[t[:, 1]] == lab[t[:, 2]]).all()
        cnt = C.component_sizes(t, lab)
        assert cnt.sum() == len(t) and (cnt[np.setdiff1d(np.arange(V), roots)] == 0).all()
        if coo_matrix is not None:
            t64 = t.astype(np.int64)
            a = np.concatenate([t64[:, 0], t64[:, 1], t64[:, 2]])
            b = np.concatenate([t64[:, 1], t64[:, 2], t64[:, 0]])
            k, sl = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(V, V)), directed=False)
            assert k == len(roots) and C.same_partition(lab, sl), name


def test_reference_kept_meshes():
    cases = _cases()
    t, V, v = cases["two_spheres"]
    kept, tri, lab, cnt = C.clean(t, V, keep_largest=True)
    # the larger sphere (radius 0.30 at +0.45) has the larger ids: x is the slowest axis of the vertex order
    assert cnt.max() == len(tri) and 0 < len(tri) < len(t)
    assert tri.min() == 0 and tri.max() == len(kept) - 1 and (np.diff(kept) > 0).all()
    assert np.array_equal(kept[tri], t[np.isin(t[:, 0], kept)])  # renumbering undone: the kept triangles, in order
    assert R.is_closed_oriented(tri, len(kept))
    assert R.euler_characteristic(tri, len(kept)) == 2
    assert R.signed_volume(v[kept], tri) > 0
    assert (v[kept] > 0).all()  # the sphere around (+0.45, +0.45, +0.45)
    other, tri_o, _, _ = C.clean(t, V, min_triangles=len(tri))  # the threshold at the largest size keeps it alone
    assert np.array_equal(other, kept) and np.array_equal(tri_o, tri)
    both, tri_b, _, _ = C.clean(t, V, min_triangles=1)
    assert np.array_equal(both, np.arange(V)) and np.array_equal(tri_b, t)
    t, V, v = cases["torus"]
    kept, tri, _, _ = C.clean(t, V, keep_largest=True)
    assert np.array_equal(kept, np.arange(V)) and np.array_equal(tri, t)
    assert R.is_closed_oriented(tri, len(kept)) and R.euler_characteristic(tri, len(kept)) == 0
    # the fans (5, 5, 3 triangles; roots 0, 7, 14): the tie goes to the smaller root
    t, V, _ = cases["fans"]
    kept, tri, lab, cnt = C.clean(t, V, keep_largest=True)
    assert np.array_equal(np.flatnonzero(cnt), [0, 7, 14]) and list(cnt[[0, 7, 14]]) == [5, 5, 3]
    assert np.array_equal(kept, np.arange(7)) and np.array_equal(tri, t[:5])
    kept, tri, _, _ = C.clean(t, V, min_triangles=4)
    assert np.array_equal(kept, np.arange(14)) and np.array_equal(tri, t[:10])
    kept, tri, _, _ = C.clean(t, V, min_triangles=6)
    assert kept.shape == (0,) and tri.shape == (0, 3)
    kept, tri, _, _ = C.clean(t, V, keep_largest=True, min_triangles=6)
    assert kept.shape == (0,) and tri.shape == (0, 3)
    kept, tri, _, _ = C.clean(t[5:], V, keep_largest=True)  # without the first fan: its 7 vertices are isolated
    assert np.array_equal(kept, np.arange(7, 14)) and np.array_equal(tri, t[5:10] - 7)
    kept, tri, lab, cnt = C.clean(np.zeros((0, 3), np.int32), 0, keep_largest=True)
    assert kept.shape == (0,) and tri.shape == (0, 3) and lab.shape == (0,) and cnt.shape == (0,)


def test_ops_refuse_cpu_tensors():
    import torch
    from copenerf import ops
    t, V = C.fans()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_clean(torch.zeros(V, 3), torch.from_numpy(t), keep_largest=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_components(torch.from_numpy(t), V)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vertex_dirs(torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rgb8_pack(torch.zeros(4, 3))
