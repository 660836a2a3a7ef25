"""cn_mesh_raster, cn_mesh_visibility and cn_mesh_select_mask are exported, additive to ABI v22, refuse bad
arguments with the right status and a message before anything launches, size their workspace as include/copenerf.h
documents, and their descriptors are laid out as the bindings say (no device needed: every call here fails its checks,
or has nothing to do, before a launch)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "copenerf.h")
ARG, SHAPE, ALIGN = -1, -2, -3
P = 4096  # a placeholder pointer: aligned, never dereferenced
NEW = ("cn_mesh_raster_workspace_bytes", "cn_mesh_raster", "cn_mesh_visibility", "cn_mesh_select_mask")


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


def _raster_desc(_lib, V=10, T=5, N=2, h=8, w=9):
    d = _lib.MeshRasterDesc()
    d.V, d.T, d.N, d.h, d.w, d.near = V, T, N, h, w, 1e-4
    d.vertices, d.triangles, d.proj, d.depth, d.tri = P, P, P, P, P
    return d


def test_mesh_raster_checks():
    _lib, lib = _load()
    big = 1 << 40
    assert lib.cn_mesh_raster(None, P, big, None) == ARG and b"null descriptor" in _err(lib)
    for kw in (dict(V=-1), dict(T=1 << 31), dict(V=1 << 31), dict(N=-1), dict(h=0), dict(w=0), dict(h=1 << 16, w=1 << 15)):
        assert lib.cn_mesh_raster(ctypes.byref(_raster_desc(_lib, **kw)), P, big, None) == SHAPE, kw
    assert b"h w below 2^31" in _err(lib)
    for near in (0.0, -1.0, float("inf"), float("nan")):
        d = _raster_desc(_lib)
        d.near = near
        assert lib.cn_mesh_raster(ctypes.byref(d), P, big, None) == SHAPE and b"near" in _err(lib)
    d = _raster_desc(_lib)
    d.pixel_budget = -1
    assert lib.cn_mesh_raster(ctypes.byref(d), P, big, None) == SHAPE and b"pixel_budget" in _err(lib)
    d = _raster_desc(_lib)
    d.view_batch = -1
    assert lib.cn_mesh_raster(ctypes.byref(d), P, big, None) == SHAPE and b"view_batch" in _err(lib)
    for field in ("proj", "depth", "tri", "vertices", "triangles"):
        d = _raster_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_mesh_raster(ctypes.byref(d), P, big, None) == ARG and b"null" in _err(lib), field
    d = _raster_desc(_lib)
    d.depth = P + 2
    assert lib.cn_mesh_raster(ctypes.byref(d), P, big, None) == ALIGN
    d = _raster_desc(_lib)
    d.stats = P + 4
    assert lib.cn_mesh_raster(ctypes.byref(d), P, big, None) == ALIGN and b"stats 8-byte" in _err(lib)
    d = _raster_desc(_lib)
    need = lib.cn_mesh_raster_workspace_bytes(10, 5, 2, 8, 9, 0)
    assert lib.cn_mesh_raster(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_mesh_raster(ctypes.byref(d), None, need, None) == SHAPE
    assert lib.cn_mesh_raster(ctypes.byref(d), P + 16, need, None) == ALIGN and b"256-byte" in _err(lib)
    # no views: nothing to do, no launch, no buffers needed
    d = _lib.MeshRasterDesc()
    d.h, d.w, d.near = 4, 4, 1e-4
    assert lib.cn_mesh_raster(ctypes.byref(d), None, 0, None) == 0


def test_mesh_raster_workspace_formula():
    _, lib = _load()

    def want(V, T, N, h, w, batch):
        B = min(batch or 8, N, 65535)
        if T:
            B = min(B, (2 ** 31 - 1) // T)
        B = max(min(B, (2 ** 31 - 1) // (h * w)), 1)
        return rup(8 * B * h * w) + rup(16 * B * V) + rup(8 * B * T) + rup(4)
    for args in ((0, 0, 1, 8, 8, 0), (642, 1280, 3, 64, 96, 0), (642, 1280, 3, 64, 96, 2), (642, 1280, 64, 480, 640, 0),
                 (1_500_000, 3_000_000, 64, 480, 640, 16), (10, 1 << 30, 8, 4, 4, 0), (10, 20, 8, 1 << 14, 1 << 14, 0),
                 (10, 20, 0, 8, 8, 0)):
        assert lib.cn_mesh_raster_workspace_bytes(*args) == want(*args), args
    for bad in ((-1, 0, 1, 8, 8, 0), (0, 1 << 31, 1, 8, 8, 0), (0, 0, 1, 0, 8, 0), (0, 0, 1, 1 << 16, 1 << 16, 0), (0, 0, 1, 8, 8, -1)):
        assert lib.cn_mesh_raster_workspace_bytes(*bad) == 0, bad


def _vis_desc(_lib, Q=10, N=2, h=8, w=9):
    d = _lib.MeshVisibilityDesc()
    d.Q, d.N, d.h, d.w, d.near, d.points, d.proj, d.count = Q, N, h, w, 1e-4, P, P, P
    return d


def test_mesh_visibility_checks():
    _lib, lib = _load()
    assert lib.cn_mesh_visibility(None, None) == ARG and b"null descriptor" in _err(lib)
    for kw in (dict(Q=-1), dict(Q=1 << 31), dict(N=-1), dict(h=0), dict(w=-3)):
        assert lib.cn_mesh_visibility(ctypes.byref(_vis_desc(_lib, **kw)), None) == SHAPE, kw
    for field, value, msg in (("near", 0.0, b"near"), ("near", float("nan"), b"near"), ("tol_abs", -1.0, b"tol_abs"),
                              ("tol_rel", float("nan"), b"tol_rel")):
        d = _vis_desc(_lib)
        setattr(d, field, value)
        assert lib.cn_mesh_visibility(ctypes.byref(d), None) == SHAPE and msg in _err(lib)
    for field in ("points", "count", "proj"):
        d = _vis_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_mesh_visibility(ctypes.byref(d), None) == ARG, field
    d = _vis_desc(_lib)
    d.depth = P + 1
    assert lib.cn_mesh_visibility(ctypes.byref(d), None) == ALIGN
    d = _vis_desc(_lib, Q=0)
    d.points = d.count = None
    assert lib.cn_mesh_visibility(ctypes.byref(d), None) == 0  # nothing to do: no launch


def test_mesh_select_mask_checks():
    _lib, lib = _load()
    big = 1 << 30
    assert lib.cn_mesh_select_mask(None, P, P, big, None) == ARG and b"null descriptor" in _err(lib)
    d = _lib.MeshCleanDesc()
    d.V, d.T, d.triangles, d.counts = 10, 5, P, P
    assert lib.cn_mesh_select_mask(ctypes.byref(d), None, P, big, None) == ARG and b"vmask" in _err(lib)
    need = lib.cn_mesh_clean_workspace_bytes(10, 5)
    assert lib.cn_mesh_select_mask(ctypes.byref(d), P, P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert lib.cn_mesh_select_mask(ctypes.byref(d), P, P + 8, need, None) == ALIGN
    d.counts = None
    assert lib.cn_mesh_select_mask(ctypes.byref(d), P, P, need, None) == ARG and b"counts" in _err(lib)
    d.counts = P + 4
    assert lib.cn_mesh_select_mask(ctypes.byref(d), P, P, need, None) == ALIGN
    d.counts, d.triangles = P, None
    assert lib.cn_mesh_select_mask(ctypes.byref(d), P, P, need, None) == ARG and b"triangles" in _err(lib)
    d.triangles, d.T = P, -1
    assert lib.cn_mesh_select_mask(ctypes.byref(d), P, P, need, None) == SHAPE


def test_struct_layouts_match_header_order():
    from copenerf import _lib
    src = open(HEADER).read()
    for cname, py in (("cn_mesh_raster_desc", _lib.MeshRasterDesc), ("cn_mesh_visibility_desc", _lib.MeshVisibilityDesc)):
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
    R, V = _lib.MeshRasterDesc, _lib.MeshVisibilityDesc
    assert (R.N.offset, R.proj.offset, R.near.offset, R.depth.offset, R.stats.offset, ctypes.sizeof(R)) == (32, 48, 56, 64, 80, 88)
    assert (V.N.offset, V.near.offset, V.proj.offset, V.tol_abs.offset, V.count.offset, ctypes.sizeof(V)) == (16, 28, 32, 48, 56, 64)
