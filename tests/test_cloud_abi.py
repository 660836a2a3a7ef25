"""The point-cloud preparation entries (cn_knn_query, cn_voxel_keys, cn_voxel_reduce, cn_cloud_normals,
cn_knn_mean_stats) are exported, leave the ABI at 22, refuse bad arguments with the right status and a message
before anything launches, size their workspaces as include/copenerf.h documents, and their descriptors are laid out
as the bindings say (no device needed: every call here fails its checks, or has nothing to do, before a launch)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "copenerf.h")
ARG, SHAPE, ALIGN = -1, -2, -3
P = 4096  # a placeholder pointer: aligned, never dereferenced
INF = float("inf")


def rup(n, m=256):
    return (n + m - 1) // m * m


def _load():
    from copenerf import _lib
    return _lib, _lib.load()


def _err(lib):
    return lib.cn_last_error() or b""


def test_exports_and_abi_version():
    _, lib = _load()
    for name in ("cn_knn_query", "cn_voxel_keys", "cn_voxel_reduce_workspace_bytes", "cn_voxel_reduce",
                 "cn_cloud_normals", "cn_knn_mean_stats_workspace_bytes", "cn_knn_mean_stats"):
        assert hasattr(lib, name), name
    assert lib.cn_abi_version() == 22
    assert re.search(r"#define CN_ABI_VERSION 22\b", open(HEADER).read())


def _grid_desc(_lib, N=100, dims=(4, 5, 6), cell=0.5):
    g = _lib.NnGridDesc()
    g.N, g.points, g.cell, g.cell_start, g.sorted = N, P, cell, P, P
    g.dims = (_lib.c_i32 * 3)(*dims)
    return g


def _knn_desc(_lib, g, Q=10, k=8):
    q = _lib.KnnQueryDesc()
    q.grid = ctypes.pointer(g)
    q.Q, q.queries, q.dist, q.index, q.max_dist, q.k = Q, P, P, P, INF, k
    return q


def test_knn_query_checks():
    _lib, lib = _load()
    assert lib.cn_knn_query(None, None) == ARG and b"null descriptor" in _err(lib)
    q = _lib.KnnQueryDesc()
    q.k = 4
    assert lib.cn_knn_query(ctypes.byref(q), None) == ARG and b"null grid" in _err(lib)
    g = _grid_desc(_lib)
    bad = _grid_desc(_lib, dims=(1 << 10, 1 << 10, 1 << 10))
    q = _knn_desc(_lib, bad)
    assert lib.cn_knn_query(ctypes.byref(q), None) == SHAPE and b"2^26 cells" in _err(lib)
    for Q in (-1, 1 << 31):
        q = _knn_desc(_lib, g, Q=Q)
        assert lib.cn_knn_query(ctypes.byref(q), None) == SHAPE and b"Q " in _err(lib)
    for k in (0, -1, 33, 1 << 20):
        q = _knn_desc(_lib, g, k=k)
        assert lib.cn_knn_query(ctypes.byref(q), None) == SHAPE and b"k %d" % k in _err(lib)
    for k in (1, 32):  # the ends of the range pass the k check (and stop at the next one)
        q = _knn_desc(_lib, g, k=k)
        q.query_records = 2
        assert lib.cn_knn_query(ctypes.byref(q), None) == ARG and b"query_records" in _err(lib)
    q = _knn_desc(_lib, g)
    q.exclude_self = 2
    assert lib.cn_knn_query(ctypes.byref(q), None) == ARG and b"exclude_self" in _err(lib)
    q.exclude_self = 1  # Q = 10 queries of N = 100 targets
    assert lib.cn_knn_query(ctypes.byref(q), None) == SHAPE and b"exclude_self with Q 10" in _err(lib)
    for md in (-1.0, float("nan")):
        q = _knn_desc(_lib, g)
        q.max_dist = md
        assert lib.cn_knn_query(ctypes.byref(q), None) == SHAPE and b"max_dist" in _err(lib)
    for field in ("queries", "dist", "index"):
        q = _knn_desc(_lib, g)
        setattr(q, field, None)
        assert lib.cn_knn_query(ctypes.byref(q), None) == ARG and b"null queries / dist / index" in _err(lib)
    for field in ("dist", "index", "count"):
        q = _knn_desc(_lib, g)
        setattr(q, field, P + 2)
        assert lib.cn_knn_query(ctypes.byref(q), None) == ALIGN
    q = _knn_desc(_lib, g)
    q.query_records, q.queries = 1, P + 4  # records are 16-byte aligned
    assert lib.cn_knn_query(ctypes.byref(q), None) == ALIGN and b"16-byte" in _err(lib)
    q = _knn_desc(_lib, g, Q=0)
    q.queries, q.dist, q.index = None, None, None  # nothing to do: no launch
    assert lib.cn_knn_query(ctypes.byref(q), None) == 0


def _keys_desc(_lib, N=100, voxel=0.1):
    d = _lib.VoxelKeysDesc()
    d.N, d.points, d.voxel, d.keys, d.valid = N, P, voxel, P, P
    return d


def test_voxel_keys_checks():
    _lib, lib = _load()
    assert lib.cn_voxel_keys(None, None) == ARG and b"null descriptor" in _err(lib)
    for N in (-1, 1 << 31):
        assert lib.cn_voxel_keys(ctypes.byref(_keys_desc(_lib, N=N)), None) == SHAPE and b"2^31" in _err(lib)
    for voxel in (0.0, -0.5, INF, float("nan")):
        assert lib.cn_voxel_keys(ctypes.byref(_keys_desc(_lib, voxel=voxel)), None) == SHAPE
        assert b"voxel size" in _err(lib)
    d = _keys_desc(_lib)
    d.origin[2] = INF
    assert lib.cn_voxel_keys(ctypes.byref(d), None) == SHAPE and b"origin[2]" in _err(lib)
    for field in ("points", "keys"):
        d = _keys_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_voxel_keys(ctypes.byref(d), None) == ARG and b"null points / keys" in _err(lib)
    d = _keys_desc(_lib)
    d.keys = P + 4
    assert lib.cn_voxel_keys(ctypes.byref(d), None) == ALIGN and b"8-byte" in _err(lib)
    d = _keys_desc(_lib)
    d.valid = P + 1
    assert lib.cn_voxel_keys(ctypes.byref(d), None) == ALIGN
    d = _keys_desc(_lib, N=0)
    d.points = d.keys = d.valid = None
    assert lib.cn_voxel_keys(ctypes.byref(d), None) == 0


def _reduce_desc(_lib, N=100):
    d = _lib.VoxelReduceDesc()
    d.N = N
    d.keys = d.order = d.points = d.out_points = d.out_keys = d.out_counts = d.totals = P
    return d


def test_voxel_reduce_checks():
    _lib, lib = _load()
    big = 1 << 40
    assert lib.cn_voxel_reduce(None, P, big, None) == ARG and b"null descriptor" in _err(lib)
    for N in (-1, 1 << 31):
        assert lib.cn_voxel_reduce(ctypes.byref(_reduce_desc(_lib, N=N)), P, big, None) == SHAPE and b"2^31" in _err(lib)
    d = _reduce_desc(_lib)
    d.totals = None
    assert lib.cn_voxel_reduce(ctypes.byref(d), P, big, None) == ARG and b"totals" in _err(lib)
    for field in ("keys", "order", "points", "out_points", "out_counts"):
        d = _reduce_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_voxel_reduce(ctypes.byref(d), P, big, None) == ARG and b"null keys / order" in _err(lib)
    for a, b in (("normals", "out_normals"), ("colors", "out_colors")):
        for field in (a, b):
            d = _reduce_desc(_lib)
            setattr(d, field, P)  # one of the pair without the other
            assert lib.cn_voxel_reduce(ctypes.byref(d), P, big, None) == ARG and b"go together" in _err(lib)
    for field in ("keys", "order", "out_keys"):
        d = _reduce_desc(_lib)
        setattr(d, field, P + 4)
        assert lib.cn_voxel_reduce(ctypes.byref(d), P, big, None) == ALIGN and b"8-byte" in _err(lib)
    d = _reduce_desc(_lib)
    d.out_points = P + 2
    assert lib.cn_voxel_reduce(ctypes.byref(d), P, big, None) == ALIGN
    d = _reduce_desc(_lib)
    need = lib.cn_voxel_reduce_workspace_bytes(100)
    assert lib.cn_voxel_reduce(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_voxel_reduce(ctypes.byref(d), None, need, None) == SHAPE
    assert lib.cn_voxel_reduce(ctypes.byref(d), P + 64, need, None) == ALIGN and b"256-byte" in _err(lib)


def _normals_desc(_lib, N=100, k=16):
    d = _lib.CloudNormalsDesc()
    d.N, d.points, d.index, d.k, d.normals = N, P, P, k, P
    return d


def test_cloud_normals_checks():
    _lib, lib = _load()
    assert lib.cn_cloud_normals(None, None) == ARG and b"null descriptor" in _err(lib)
    for N in (-1, 1 << 31):
        assert lib.cn_cloud_normals(ctypes.byref(_normals_desc(_lib, N=N)), None) == SHAPE and b"2^31" in _err(lib)
    for k in (0, 33, -4):
        assert lib.cn_cloud_normals(ctypes.byref(_normals_desc(_lib, k=k)), None) == SHAPE and b"k %d" % k in _err(lib)
    d = _normals_desc(_lib)
    d.orient = 3
    assert lib.cn_cloud_normals(ctypes.byref(d), None) == ARG and b"orient 3" in _err(lib)
    d.orient = 1
    d.orient_to[1] = float("nan")
    assert lib.cn_cloud_normals(ctypes.byref(d), None) == SHAPE and b"orient_to[1]" in _err(lib)
    for field in ("points", "index", "normals"):
        d = _normals_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_cloud_normals(ctypes.byref(d), None) == ARG and b"null points / index / normals" in _err(lib)
    for field in ("points", "index", "normals", "variation"):
        d = _normals_desc(_lib)
        setattr(d, field, P + 2)
        assert lib.cn_cloud_normals(ctypes.byref(d), None) == ALIGN
    d = _normals_desc(_lib, N=0)
    d.points = d.index = d.normals = None
    assert lib.cn_cloud_normals(ctypes.byref(d), None) == 0


def _mean_desc(_lib, N=1000, k=20):
    d = _lib.KnnMeanStatsDesc()
    d.N, d.k, d.dist, d.index, d.mean, d.out = N, k, P, P, P, P
    return d


def test_knn_mean_stats_checks():
    _lib, lib = _load()
    big = 1 << 20
    assert lib.cn_knn_mean_stats(None, P, big, None) == ARG and b"null descriptor" in _err(lib)
    for N in (-1, 1 << 31):
        assert lib.cn_knn_mean_stats(ctypes.byref(_mean_desc(_lib, N=N)), P, big, None) == SHAPE and b"2^31" in _err(lib)
    for k in (0, 33):
        assert lib.cn_knn_mean_stats(ctypes.byref(_mean_desc(_lib, k=k)), P, big, None) == SHAPE and b"k %d" % k in _err(lib)
    d = _mean_desc(_lib)
    d.out = None
    assert lib.cn_knn_mean_stats(ctypes.byref(d), P, big, None) == ARG and b"null out" in _err(lib)
    for field in ("dist", "index", "mean"):
        d = _mean_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_knn_mean_stats(ctypes.byref(d), P, big, None) == ARG and b"null dist / index / mean" in _err(lib)
    d = _mean_desc(_lib)
    d.out = P + 4
    assert lib.cn_knn_mean_stats(ctypes.byref(d), P, big, None) == ALIGN and b"8-byte" in _err(lib)
    d = _mean_desc(_lib)
    need = lib.cn_knn_mean_stats_workspace_bytes(1000)
    assert lib.cn_knn_mean_stats(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_knn_mean_stats(ctypes.byref(d), None, need, None) == SHAPE
    assert lib.cn_knn_mean_stats(ctypes.byref(d), P + 8, need, None) == ALIGN and b"256-byte" in _err(lib)


def test_workspace_formulas_match_the_header():
    _, lib = _load()
    for N in (0, 1, 1024, 1025, 3_000_000):
        assert lib.cn_voxel_reduce_workspace_bytes(N) == rup(4 * N) + rup(4 * max(1, -(-N // 1024)))
        blocks = min(1024, max(1, -(-N // 1024)))
        assert lib.cn_knn_mean_stats_workspace_bytes(N) == rup(24 * blocks)
    for fn in (lib.cn_voxel_reduce_workspace_bytes, lib.cn_knn_mean_stats_workspace_bytes):
        assert fn(-1) == 0 and fn(1 << 31) == 0


def test_struct_layouts_match_header_order():
    from copenerf import _lib
    src = open(HEADER).read()
    for cname, py in (("cn_knn_query_desc", _lib.KnnQueryDesc), ("cn_voxel_keys_desc", _lib.VoxelKeysDesc),
                      ("cn_voxel_reduce_desc", _lib.VoxelReduceDesc), ("cn_cloud_normals_desc", _lib.CloudNormalsDesc),
                      ("cn_knn_mean_stats_desc", _lib.KnnMeanStatsDesc)):
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
    # the offsets a C compiler gives (natural alignment)
    assert _lib.KnnQueryDesc.k.offset == 32 and _lib.KnnQueryDesc.dist.offset == 40 and ctypes.sizeof(_lib.KnnQueryDesc) == 64
    assert _lib.VoxelKeysDesc.voxel.offset == 28 and _lib.VoxelKeysDesc.keys.offset == 32 and ctypes.sizeof(_lib.VoxelKeysDesc) == 48
    assert _lib.VoxelReduceDesc.totals.offset == 88 and ctypes.sizeof(_lib.VoxelReduceDesc) == 96
    assert _lib.CloudNormalsDesc.orient_to.offset == 32 and _lib.CloudNormalsDesc.normals.offset == 48
    assert ctypes.sizeof(_lib.CloudNormalsDesc) == 64
    assert _lib.KnnMeanStatsDesc.dist.offset == 16 and ctypes.sizeof(_lib.KnnMeanStatsDesc) == 48
    from copenerf import ops
    assert ops.VOXEL_KEY_NONE == (1 << 63) - 1 and "#define CN_VOXEL_KEY_NONE INT64_MAX" in src
