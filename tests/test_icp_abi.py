"""cn_cloud_transform and cn_icp_accumulate are exported, additive to ABI v22, refuse bad arguments
with the right status and a message before anything launches, and their descriptors are laid out as the bindings say
(no device needed: every call here fails its checks, or has nothing to do, before a launch)."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "copenerf.h")
ARG, SHAPE, ALIGN = -1, -2, -3
P = 4096  # a placeholder pointer: aligned, never dereferenced
BIG = 1 << 40
NEW = ("cn_cloud_transform", "cn_icp_accumulate_workspace_bytes", "cn_icp_accumulate")
IDENTITY = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
NONFINITE = (float("nan"), float("inf"), -float("inf"))


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


def _matrix(_lib, at=None, value=0.0):
    m = list(IDENTITY)
    if at is not None:
        m[at] = value
    return (_lib.c_f32 * 12)(*m)


def _transform_desc(_lib, N=5):
    d = _lib.CloudTransformDesc()
    d.N, d.points, d.out, d.matrix = N, P, P, _matrix(_lib)
    return d


def test_cloud_transform_checks():
    _lib, lib = _load()
    assert lib.cn_cloud_transform(None, None) == ARG and b"null descriptor" in _err(lib)
    for N in (-1, 1 << 31):
        assert lib.cn_cloud_transform(ctypes.byref(_transform_desc(_lib, N)), None) == SHAPE and b"[0, 2^31)" in _err(lib)
    for at in (0, 7, 11):
        for bad in NONFINITE:
            d = _transform_desc(_lib)
            d.matrix = _matrix(_lib, at, bad)
            assert lib.cn_cloud_transform(ctypes.byref(d), None) == SHAPE and b"matrix[%d]" % at in _err(lib)
    for field in ("points", "out"):
        d = _transform_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_cloud_transform(ctypes.byref(d), None) == ARG and b"null points / out" in _err(lib)
        d = _transform_desc(_lib)
        setattr(d, field, P + 2)
        assert lib.cn_cloud_transform(ctypes.byref(d), None) == ALIGN and b"4-byte" in _err(lib)
    d = _transform_desc(_lib, N=0)
    d.points = d.out = None
    assert lib.cn_cloud_transform(ctypes.byref(d), None) == 0  # nothing to do: no launch


def _accumulate_desc(_lib, Q=5, N=7, mode=0):
    d = _lib.IcpAccumulateDesc()
    d.Q, d.N, d.mode = Q, N, mode
    d.source, d.targets, d.index, d.out = P, P, P, P
    if mode == 1:
        d.target_normals = P
    d.matrix, d.pivot = _matrix(_lib), (ctypes.c_double * 3)(0.5, 0.5, 0.5)
    return d


def test_icp_accumulate_checks():
    _lib, lib = _load()
    fn = lib.cn_icp_accumulate
    assert fn(None, P, BIG, None) == ARG and b"null descriptor" in _err(lib)
    for kw in (dict(Q=-1), dict(Q=1 << 31), dict(N=-1), dict(N=1 << 31)):
        assert fn(ctypes.byref(_accumulate_desc(_lib, **kw)), P, BIG, None) == SHAPE and b"[0, 2^31)" in _err(lib), kw
    for mode in (-1, 2):
        assert fn(ctypes.byref(_accumulate_desc(_lib, mode=mode)), P, BIG, None) == ARG and b"mode" in _err(lib)
    for bad in NONFINITE:
        d = _accumulate_desc(_lib)
        d.matrix = _matrix(_lib, 5, bad)
        assert fn(ctypes.byref(d), P, BIG, None) == SHAPE and b"matrix[5]" in _err(lib)
        d = _accumulate_desc(_lib)
        d.pivot[1] = bad
        assert fn(ctypes.byref(d), P, BIG, None) == SHAPE and b"pivot[1]" in _err(lib)
    for field in ("source", "index", "targets", "out"):
        d = _accumulate_desc(_lib)
        setattr(d, field, None)
        assert fn(ctypes.byref(d), P, BIG, None) == ARG and b"null" in _err(lib), field
    d = _accumulate_desc(_lib, mode=1)
    d.target_normals = None
    assert fn(ctypes.byref(d), P, BIG, None) == ARG and b"mode 1 without target_normals" in _err(lib)
    for field in ("source", "targets", "target_normals", "index", "out"):
        d = _accumulate_desc(_lib, mode=1)
        setattr(d, field, P + (4 if field == "out" else 2))
        assert fn(ctypes.byref(d), P, BIG, None) == ALIGN and b"aligned" in _err(lib), field
    need = lib.cn_icp_accumulate_workspace_bytes(5)
    assert need == 256 and lib.cn_icp_accumulate_workspace_bytes(1024 * 1024 + 1) == 1024 * 256
    assert lib.cn_icp_accumulate_workspace_bytes(-1) == 0 and lib.cn_icp_accumulate_workspace_bytes(1 << 31) == 0
    d = _accumulate_desc(_lib)
    assert fn(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
    assert fn(ctypes.byref(d), None, need, None) == SHAPE and b"workspace" in _err(lib)
    assert fn(ctypes.byref(d), P + 16, need, None) == ALIGN and b"256-byte" in _err(lib)


STRUCTS = (("cn_cloud_transform_desc", "CloudTransformDesc"), ("cn_icp_accumulate_desc", "IcpAccumulateDesc"))


def _header_fields(cname):
    src = open(HEADER).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        decl = re.sub(r"^(const\s+)?\w+\s*\**", "", decl)
        names += [re.sub(r"\[[\w\s+-]+\]", "", n.strip(" *")) for n in decl.split(",")]
    return names


def test_struct_layouts_match_header_order():
    from copenerf import _lib
    for cname, pyname in STRUCTS:
        py = getattr(_lib, pyname)
        assert _header_fields(cname) == [f[0] for f in py._fields_], cname
        assert ctypes.sizeof(py) % 8 == 0
    # the offsets a C compiler gives (natural alignment)
    T, A = _lib.CloudTransformDesc, _lib.IcpAccumulateDesc
    assert (T.points.offset, T.matrix.offset, T.out.offset, ctypes.sizeof(T)) == (8, 16, 64, 72)
    assert (A.N.offset, A.source.offset, A.index.offset, A.matrix.offset, A.mode.offset, A.pivot.offset, A.out.offset,
            ctypes.sizeof(A)) == (8, 16, 40, 48, 96, 104, 128, 136)


def test_struct_layouts_match_a_c_compiler(tmp_path):
    """offsetof / sizeof of every field as a C compiler lays the header out."""
    from copenerf import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang") or "/opt/rocm/llvm/bin/clang"  # (the build's own)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "copenerf.h"', "int main(void) {"]
    for cname, pyname in STRUCTS:
        for f, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'    printf("{pyname}.{f} %zu\\n", offsetof({cname}, {f}));')
        lines.append(f'    printf("{pyname} %zu\\n", sizeof({cname}));')
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    for line in out.splitlines():
        name, value = line.split()
        if "." in name:
            pyname, f = name.split(".")
            assert getattr(getattr(_lib, pyname), f).offset == int(value), name
        else:
            assert ctypes.sizeof(getattr(_lib, name)) == int(value), name
