"""cn_mesh_shade, cn_cloud_normal_stats (with its workspace query) and cn_normal_errors are exported, additive to ABI
v22, refuse bad arguments with the right status and a message before anything launches, and their descriptors are
laid out as the bindings say (no device needed: every call here fails its checks, or has nothing to do, before a
launch)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "copenerf.h")
ARG, SHAPE, ALIGN = -1, -2, -3
P = 4096  # a placeholder pointer: aligned, never dereferenced
NEW = ("cn_mesh_shade", "cn_cloud_normal_stats_workspace_bytes", "cn_cloud_normal_stats", "cn_normal_errors_workspace_bytes",
       "cn_normal_errors")


def rup(n, m=256):
    return (n + m - 1) // m * m


def _load():
    from copenerf import _lib
    return _lib, _lib.load()


def _err(lib):
    return lib.cn_last_error() or b""


def test_symbols_exported_and_abi_version_unchanged():
    _lib, lib = _load()
    assert lib.cn_abi_version() == 22 and _lib.ABI_VERSION == 22
    src = open(HEADER).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
        assert re.search(r"\b%s\(" % name, src), name


def _shade_desc(_lib, V=10, T=5, N=2, h=8, w=9, C=3):
    d = _lib.MeshShadeDesc()
    d.V, d.T, d.N, d.h, d.w, d.C, d.ambient, d.grey = V, T, N, h, w, C, 0.3, 0.8
    d.light = (ctypes.c_float * 3)(0, 0, 1)
    d.vertices = d.triangles = d.proj = d.tri = d.attr = d.attr_out = d.normal_out = P
    return d


def test_mesh_shade_checks():
    _lib, lib = _load()
    assert lib.cn_mesh_shade(None, None) == ARG and b"null descriptor" in _err(lib)
    for kw in (dict(V=-1), dict(T=1 << 31), dict(V=1 << 31), dict(N=-1), dict(h=0), dict(w=-2), dict(h=1 << 16, w=1 << 15)):
        assert lib.cn_mesh_shade(ctypes.byref(_shade_desc(_lib, **kw)), None) == SHAPE, kw
    assert b"h w below 2^31" in _err(lib)
    for C in (0, -1, 17):
        assert lib.cn_mesh_shade(ctypes.byref(_shade_desc(_lib, C=C)), None) == SHAPE and b"1 .. 16" in _err(lib), C
    d = _shade_desc(_lib, C=2)
    d.albedo_from_attr, d.shaded_img = 1, P
    assert lib.cn_mesh_shade(ctypes.byref(d), None) == SHAPE and b"at least 3" in _err(lib)
    for amb in (-0.1, 1.5, float("nan")):
        d = _shade_desc(_lib)
        d.ambient = amb
        assert lib.cn_mesh_shade(ctypes.byref(d), None) == SHAPE and b"ambient" in _err(lib)
    d = _shade_desc(_lib)
    d.light = (ctypes.c_float * 3)(0, float("inf"), 1)
    assert lib.cn_mesh_shade(ctypes.byref(d), None) == SHAPE and b"light" in _err(lib)
    for field in ("proj", "tri", "vertices", "triangles", "attr"):
        d = _shade_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_mesh_shade(ctypes.byref(d), None) == ARG and b"null" in _err(lib), field
    d = _shade_desc(_lib)
    d.attr_out = d.normal_out = None
    assert lib.cn_mesh_shade(ctypes.byref(d), None) == ARG and b"outputs" in _err(lib)
    for field in ("vertices", "tri", "attr", "vnormals", "rot", "attr_out", "normal_out"):
        d = _shade_desc(_lib)
        setattr(d, field, P + 2)
        assert lib.cn_mesh_shade(ctypes.byref(d), None) == ALIGN, field
    # no views: nothing to do, no launch, no buffers needed
    d = _lib.MeshShadeDesc()
    d.h, d.w = 4, 4
    assert lib.cn_mesh_shade(ctypes.byref(d), None) == 0


def _stats_desc(_lib, Q=10, N=7):
    d = _lib.CloudNormalStatsDesc()
    d.Q, d.N, d.max_dist = Q, N, 1.0
    d.query_normals = d.target_normals = d.index = d.dist = d.out = P
    return d


def test_cloud_normal_stats_checks_and_workspace():
    _lib, lib = _load()
    big = 1 << 30
    assert lib.cn_cloud_normal_stats(None, P, big, None) == ARG and b"null descriptor" in _err(lib)
    for kw in (dict(Q=-1), dict(Q=1 << 31), dict(N=-1), dict(N=1 << 31)):
        assert lib.cn_cloud_normal_stats(ctypes.byref(_stats_desc(_lib, **kw)), P, big, None) == SHAPE, kw
    d = _stats_desc(_lib)
    d.max_dist = float("nan")
    assert lib.cn_cloud_normal_stats(ctypes.byref(d), P, big, None) == SHAPE and b"max_dist" in _err(lib)
    for field in ("query_normals", "target_normals", "index", "dist", "out"):
        d = _stats_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_cloud_normal_stats(ctypes.byref(d), P, big, None) == ARG and b"null" in _err(lib), field
    for field, off in (("query_normals", 2), ("index", 1), ("points", 2), ("out", 4)):
        d = _stats_desc(_lib)
        setattr(d, field, P + off)
        assert lib.cn_cloud_normal_stats(ctypes.byref(d), P, big, None) == ALIGN, field
    d = _stats_desc(_lib)
    need = lib.cn_cloud_normal_stats_workspace_bytes(10)
    assert lib.cn_cloud_normal_stats(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_cloud_normal_stats(ctypes.byref(d), None, need, None) == SHAPE
    assert lib.cn_cloud_normal_stats(ctypes.byref(d), P + 16, need, None) == ALIGN and b"256-byte" in _err(lib)
    for Q in (0, 1, 1024, 1025, 1 << 20, (1 << 20) + 1, (1 << 31) - 1):
        blocks = min(1024, max(1, -(-Q // 1024)))
        assert lib.cn_cloud_normal_stats_workspace_bytes(Q) == rup(24 * blocks), Q
    assert lib.cn_cloud_normal_stats_workspace_bytes(-1) == 0 and lib.cn_cloud_normal_stats_workspace_bytes(1 << 31) == 0


def test_normal_errors_checks_and_workspace():
    _, lib = _load()
    big = 1 << 30
    for n in (-1, 1 << 31):
        assert lib.cn_normal_errors(n, P, P, None, P, P, P, big, None) == SHAPE and b"[0, 2^31)" in _err(lib)
    for args in ((None, P, None, P, P), (P, None, None, P, P), (P, P, None, None, P), (P, P, None, P, None)):
        assert lib.cn_normal_errors(10, *args, P, big, None) == ARG and b"null" in _err(lib), args
    assert lib.cn_normal_errors(10, P + 2, P, None, P, P, P, big, None) == ALIGN
    assert lib.cn_normal_errors(10, P, P, None, P, P + 4, P, big, None) == ALIGN and b"out 8-byte" in _err(lib)
    need = lib.cn_normal_errors_workspace_bytes(10)
    assert lib.cn_normal_errors(10, P, P, None, P, P, P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_normal_errors(10, P, P, None, P, P, None, need, None) == SHAPE
    assert lib.cn_normal_errors(10, P, P, None, P, P, P + 8, need, None) == ALIGN and b"256-byte" in _err(lib)
    for n in (0, 1, 2048, 2049, 1 << 21, (1 << 21) + 1):
        blocks = min(1024, max(1, -(-n // 2048)))
        assert lib.cn_normal_errors_workspace_bytes(n) == rup(48 * blocks), n
    assert lib.cn_normal_errors_workspace_bytes(-1) == 0 and lib.cn_normal_errors_workspace_bytes(1 << 31) == 0


def test_struct_layouts_match_header_order():
    from copenerf import _lib
    src = open(HEADER).read()
    for cname, py in (("cn_mesh_shade_desc", _lib.MeshShadeDesc), ("cn_cloud_normal_stats_desc", _lib.CloudNormalStatsDesc)):
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
    S, C = _lib.MeshShadeDesc, _lib.CloudNormalStatsDesc
    assert (S.N.offset, S.C.offset, S.proj.offset, S.rot.offset, S.fill.offset, S.light.offset, S.grey.offset,
            S.albedo_from_attr.offset, S.background.offset, S.attr_out.offset, S.shaded_img.offset, ctypes.sizeof(S)) == \
        (32, 44, 48, 80, 88, 96, 108, 112, 116, 120, 144, 152)
    assert (C.query_normals.offset, C.points.offset, C.crop_min.offset, C.crop_max.offset, C.max_dist.offset, C.out.offset,
            ctypes.sizeof(C)) == (16, 48, 56, 68, 80, 88, 96)
