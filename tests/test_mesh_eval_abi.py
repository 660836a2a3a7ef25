"""The mesh geometry metric entries (cn_mesh_area / cn_mesh_sample, cn_nn_grid_build / cn_nn_query,
cn_cloud_stats) refuse bad arguments with the right status and a message before anything launches, size their
workspaces as include/copenerf.h documents, and their descriptors are laid out as the bindings say (no device
needed: every call here fails its checks, or has nothing to do, before a launch)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "copenerf.h")
ARG, SHAPE, ALIGN = -1, -2, -3
P = 4096  # a placeholder pointer: aligned, never dereferenced


def rup(n, m=256):
    return (n + m - 1) // m * m


def _load():
    from copenerf import _lib
    return _lib, _lib.load()


def _err(lib):
    return lib.cn_last_error() or b""


def _sample_desc(_lib, V=10, T=5):
    d = _lib.MeshSampleDesc()
    d.V, d.T, d.vertices, d.triangles, d.area = V, T, P, P, P
    return d


def test_mesh_sample_checks():
    _lib, lib = _load()
    assert lib.cn_mesh_area(None, P, 1 << 20, None) == ARG and b"null descriptor" in _err(lib)
    assert lib.cn_mesh_sample(None, P, 1 << 20, None) == ARG
    d = _sample_desc(_lib)
    d.area = None
    assert lib.cn_mesh_area(ctypes.byref(d), P, 1 << 20, None) == ARG and b"area" in _err(lib)
    d = _sample_desc(_lib, T=-1)
    assert lib.cn_mesh_area(ctypes.byref(d), P, 1 << 20, None) == SHAPE and b"T -1" in _err(lib)
    d = _sample_desc(_lib, T=1 << 31)
    assert lib.cn_mesh_area(ctypes.byref(d), P, 1 << 40, None) == SHAPE and b"2^31" in _err(lib)
    d = _sample_desc(_lib, V=1 << 31)
    assert lib.cn_mesh_area(ctypes.byref(d), P, 1 << 40, None) == SHAPE
    d = _sample_desc(_lib)
    need = lib.cn_mesh_sample_workspace_bytes(5)
    assert lib.cn_mesh_area(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_mesh_area(ctypes.byref(d), None, need, None) == SHAPE
    assert lib.cn_mesh_area(ctypes.byref(d), P + 16, need, None) == ALIGN and b"256-byte" in _err(lib)
    d.area = P + 4
    assert lib.cn_mesh_area(ctypes.byref(d), P, need, None) == ALIGN
    d = _sample_desc(_lib)
    d.S = 7  # no philox / points
    assert lib.cn_mesh_sample(ctypes.byref(d), P, need, None) == ARG and b"philox" in _err(lib)
    d.philox, d.points, d.S = P, P, -1
    assert lib.cn_mesh_sample(ctypes.byref(d), P, need, None) == SHAPE and b"S -1" in _err(lib)
    d.S = 1 << 31
    assert lib.cn_mesh_sample(ctypes.byref(d), P, need, None) == SHAPE and b"2^31" in _err(lib)
    d.S = 7
    assert lib.cn_mesh_sample(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    d = _sample_desc(_lib, T=0)
    d.S, d.philox, d.points = 7, P, P
    assert lib.cn_mesh_sample(ctypes.byref(d), P, 1 << 20, None) == SHAPE and b"without triangles" in _err(lib)


def _grid_desc(_lib, N=100, dims=(4, 5, 6), cell=0.5):
    g = _lib.NnGridDesc()
    g.N, g.points, g.cell, g.cell_start, g.sorted = N, P, cell, P, P
    g.dims = (_lib.c_i32 * 3)(*dims)
    return g


def test_nn_grid_checks():
    _lib, lib = _load()
    big = 1 << 40
    assert lib.cn_nn_grid_build(None, P, big, None) == ARG and b"null grid" in _err(lib)
    for N in (-1, 1 << 31):
        assert lib.cn_nn_grid_build(ctypes.byref(_grid_desc(_lib, N=N)), P, big, None) == SHAPE
        assert b"2^31" in _err(lib)
    assert lib.cn_nn_grid_build(ctypes.byref(_grid_desc(_lib, dims=(4, 0, 6))), P, big, None) == SHAPE
    # 2^26 cells are the most: 2^26 + 2^17 and a product that overflows 32 bits are refused
    for dims in ((513, 512, 256), (1 << 20, 1 << 20, 1 << 20), ((1 << 26) + 1, 1, 1)):
        assert lib.cn_nn_grid_build(ctypes.byref(_grid_desc(_lib, dims=dims)), P, big, None) == SHAPE
        assert b"2^26 cells" in _err(lib)
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.cn_nn_grid_build(ctypes.byref(_grid_desc(_lib, cell=cell)), P, big, None) == SHAPE
        assert b"cell size" in _err(lib)
    g = _grid_desc(_lib)
    g.origin[1] = float("nan")
    assert lib.cn_nn_grid_build(ctypes.byref(g), P, big, None) == SHAPE and b"origin[1]" in _err(lib)
    g = _grid_desc(_lib)
    g.cell_start = None
    assert lib.cn_nn_grid_build(ctypes.byref(g), P, big, None) == ARG and b"cell_start" in _err(lib)
    g = _grid_desc(_lib)
    g.sorted = P + 8
    assert lib.cn_nn_grid_build(ctypes.byref(g), P, big, None) == ALIGN and b"16-byte" in _err(lib)
    g = _grid_desc(_lib)
    g.points = None
    assert lib.cn_nn_grid_build(ctypes.byref(g), P, big, None) == ARG and b"null points" in _err(lib)
    g = _grid_desc(_lib)
    need = lib.cn_nn_grid_workspace_bytes(100, 120)
    assert lib.cn_nn_grid_build(ctypes.byref(g), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_nn_grid_build(ctypes.byref(g), P + 64, need, None) == ALIGN


def test_nn_query_checks():
    _lib, lib = _load()
    assert lib.cn_nn_query(None, None) == ARG and b"null descriptor" in _err(lib)
    q = _lib.NnQueryDesc()
    assert lib.cn_nn_query(ctypes.byref(q), None) == ARG and b"null grid" in _err(lib)
    g = _grid_desc(_lib)
    q.grid = ctypes.pointer(g)
    q.Q, q.queries, q.dist, q.max_dist = 10, P, P, float("inf")
    bad = _grid_desc(_lib, dims=(1 << 10, 1 << 10, 1 << 10))
    q.grid = ctypes.pointer(bad)
    assert lib.cn_nn_query(ctypes.byref(q), None) == SHAPE and b"2^26 cells" in _err(lib)
    q.grid = ctypes.pointer(g)
    for Q in (-1, 1 << 31):
        q.Q = Q
        assert lib.cn_nn_query(ctypes.byref(q), None) == SHAPE and b"Q " in _err(lib)
    q.Q, q.query_records = 10, 2
    assert lib.cn_nn_query(ctypes.byref(q), None) == ARG and b"query_records" in _err(lib)
    q.query_records = 0
    for md in (-1.0, float("nan")):
        q.max_dist = md
        assert lib.cn_nn_query(ctypes.byref(q), None) == SHAPE and b"max_dist" in _err(lib)
    q.max_dist, q.dist = 1.0, None
    assert lib.cn_nn_query(ctypes.byref(q), None) == ARG and b"null queries / dist" in _err(lib)
    q.dist, q.query_records, q.queries = P, 1, P + 4  # records are 16-byte aligned
    assert lib.cn_nn_query(ctypes.byref(q), None) == ALIGN
    q.Q, q.queries, q.dist = 0, None, None  # nothing to do: no launch
    assert lib.cn_nn_query(ctypes.byref(q), None) == 0


def test_cloud_stats_checks():
    _lib, lib = _load()
    assert lib.cn_cloud_stats(None, P, 1 << 20, None) == ARG and b"null descriptor" in _err(lib)
    d = _lib.CloudStatsDesc()
    d.Q, d.dist, d.out = 1000, P, P
    for Q in (-1, 1 << 31):
        d.Q = Q
        assert lib.cn_cloud_stats(ctypes.byref(d), P, 1 << 20, None) == SHAPE and b"2^31" in _err(lib)
    d.Q, d.out = 1000, None
    assert lib.cn_cloud_stats(ctypes.byref(d), P, 1 << 20, None) == ARG and b"out" in _err(lib)
    d.out = P + 4
    assert lib.cn_cloud_stats(ctypes.byref(d), P, 1 << 20, None) == ALIGN
    d.out = P
    need = lib.cn_cloud_stats_workspace_bytes(1000)
    assert lib.cn_cloud_stats(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_cloud_stats(ctypes.byref(d), P + 8, need, None) == ALIGN


def test_workspace_formulas_match_the_header():
    _, lib = _load()
    for T in (0, 1, 1024, 1025, 3_000_000):
        assert lib.cn_mesh_sample_workspace_bytes(T) == rup(8 * T) + rup(8 * max(1, -(-T // 1024)))
    assert lib.cn_mesh_sample_workspace_bytes(-1) == 0 and lib.cn_mesh_sample_workspace_bytes(1 << 31) == 0
    for N, cells in ((0, 1), (777, 105), (1_000_000, 125_000), (5, 1 << 26)):
        assert lib.cn_nn_grid_workspace_bytes(N, cells) == rup(4 * N) + rup(4 * cells) + rup(4 * -(-cells // 1024))
    assert lib.cn_nn_grid_workspace_bytes(1 << 31, 8) == 0 and lib.cn_nn_grid_workspace_bytes(8, (1 << 26) + 1) == 0
    assert lib.cn_nn_grid_workspace_bytes(8, 0) == 0
    for Q in (0, 1, 1024, 1025, 5_000_000):
        blocks = min(1024, max(1, -(-Q // 1024)))
        assert lib.cn_cloud_stats_workspace_bytes(Q) == rup(32 * blocks)
    assert lib.cn_cloud_stats_workspace_bytes(1 << 31) == 0


def test_struct_layouts_match_header_order():
    from copenerf import _lib
    src = open(HEADER).read()
    for cname, py in (("cn_mesh_sample_desc", _lib.MeshSampleDesc), ("cn_nn_grid_desc", _lib.NnGridDesc),
                      ("cn_nn_query_desc", _lib.NnQueryDesc), ("cn_cloud_stats_desc", _lib.CloudStatsDesc)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            decl = re.sub(r"^(const\s+)?\w+\s*\**", "", decl)
            names += [re.sub(r"\[[\w\s+-]+\]", "", n.strip(" *")) for n in decl.split(",")]
        assert names == [f[0] for f in py._fields_], (cname, names)
        assert ctypes.sizeof(py) % 8 == 0
    # the offsets a C compiler gives (natural alignment): the grid's pointers follow 7 four-byte fields
    assert _lib.NnGridDesc.cell_start.offset == 48 and ctypes.sizeof(_lib.NnGridDesc) == 64
    assert _lib.MeshSampleDesc.S.offset == 40 and ctypes.sizeof(_lib.MeshSampleDesc) == 72
    assert _lib.NnQueryDesc.max_dist.offset == 28 and ctypes.sizeof(_lib.NnQueryDesc) == 48
    assert _lib.CloudStatsDesc.out.offset == 56 and ctypes.sizeof(_lib.CloudStatsDesc) == 64
