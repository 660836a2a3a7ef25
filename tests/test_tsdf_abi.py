"""cn_tsdf_integrate, cn_tsdf_finalize, cn_volume_sample and cn_mesh_count_observed / cn_mesh_emit_observed are
exported, additive to ABI v22, refuse bad arguments with the right status and a message before anything launches, and
their descriptors are laid out as the bindings say (no device needed: every call here fails its checks, or has nothing
to do, before a launch)."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "copenerf.h")
ARG, SHAPE, ALIGN = -1, -2, -3
P = 4096  # a placeholder pointer: aligned, never dereferenced
NEW = ("cn_tsdf_integrate", "cn_tsdf_finalize", "cn_volume_sample", "cn_mesh_count_observed", "cn_mesh_emit_observed")


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


def _tsdf_desc(_lib, dims=(8, 9, 10), N=2, h=6, w=7, color=False):
    d = _lib.TsdfDesc()
    d.nx, d.ny, d.nz = dims
    d.lo, d.hi = (_lib.c_f32 * 3)(-1, -1, -1), (_lib.c_f32 * 3)(1, 1, 1)
    d.N, d.h, d.w = N, h, w
    d.trunc, d.near, d.depth_max = 0.1, 1e-4, float("inf")
    d.proj, d.depth, d.tsum, d.wsum = P, P, P, P
    if color:
        d.color, d.csum = P, P
    return d


def test_tsdf_integrate_checks():
    _lib, lib = _load()
    assert lib.cn_tsdf_integrate(None, None) == ARG and b"null descriptor" in _err(lib)
    for kw in (dict(dims=(1, 9, 10)), dict(dims=(8, 9, 0)), dict(dims=(2048, 2048, 512)), dict(dims=(1 << 16, 1 << 16, 2)),
               dict(N=-1), dict(h=0), dict(w=-2), dict(h=1 << 16, w=1 << 15)):
        assert lib.cn_tsdf_integrate(ctypes.byref(_tsdf_desc(_lib, **kw)), None) == SHAPE, kw
    assert b"h w below 2^31" in _err(lib)
    assert lib.cn_tsdf_integrate(ctypes.byref(_tsdf_desc(_lib, dims=(2048, 2048, 512))), None) == SHAPE
    assert b"below 2^31" in _err(lib)
    for field, values in (("trunc", (0.0, -1.0, float("inf"), float("nan"))), ("near", (0.0, -1.0, float("inf"), float("nan"))),
                          ("depth_max", (0.0, -1.0, float("nan")))):
        for value in values:
            d = _tsdf_desc(_lib)
            setattr(d, field, value)
            assert lib.cn_tsdf_integrate(ctypes.byref(d), None) == SHAPE and field.encode() in _err(lib), (field, value)
    for field in ("proj", "depth", "tsum", "wsum"):
        d = _tsdf_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_tsdf_integrate(ctypes.byref(d), None) == ARG and b"null" in _err(lib), field
    for field in ("color", "csum"):  # one without the other
        d = _tsdf_desc(_lib)
        setattr(d, field, P)
        assert lib.cn_tsdf_integrate(ctypes.byref(d), None) == ARG and b"go together" in _err(lib), field
    for field in ("proj", "depth", "tsum", "wsum", "color", "csum"):
        d = _tsdf_desc(_lib, color=True)
        setattr(d, field, P + 2)
        assert lib.cn_tsdf_integrate(ctypes.byref(d), None) == ALIGN and b"4-byte" in _err(lib), field
    # no views: nothing to do, no launch, no buffers needed
    d = _tsdf_desc(_lib, N=0)
    d.proj = d.depth = d.tsum = d.wsum = None
    assert lib.cn_tsdf_integrate(ctypes.byref(d), None) == 0


def _fin_desc(_lib, dims=(8, 9, 10)):
    d = _lib.TsdfFinalizeDesc()
    d.nx, d.ny, d.nz = dims
    d.min_weight, d.tsum, d.wsum, d.u = 1.0, P, P, P
    return d


def test_tsdf_finalize_checks():
    _lib, lib = _load()
    assert lib.cn_tsdf_finalize(None, None) == ARG and b"null descriptor" in _err(lib)
    assert lib.cn_tsdf_finalize(ctypes.byref(_fin_desc(_lib, (8, 1, 8))), None) == SHAPE
    assert lib.cn_tsdf_finalize(ctypes.byref(_fin_desc(_lib, (2048, 2048, 512))), None) == SHAPE
    for mw in (0.0, 0.5, -1.0, float("nan"), float("inf")):
        d = _fin_desc(_lib)
        d.min_weight = mw
        assert lib.cn_tsdf_finalize(ctypes.byref(d), None) == SHAPE and b"min_weight" in _err(lib), mw
    for field in ("tsum", "wsum", "u"):
        d = _fin_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_tsdf_finalize(ctypes.byref(d), None) == ARG and b"null" in _err(lib), field
    d = _fin_desc(_lib)
    d.rgb = P
    assert lib.cn_tsdf_finalize(ctypes.byref(d), None) == ARG and b"rgb without csum" in _err(lib)
    d = _fin_desc(_lib)
    d.u = P + 1
    assert lib.cn_tsdf_finalize(ctypes.byref(d), None) == ALIGN


def _sample_desc(_lib, dims=(8, 9, 10), C=3, Q=5):
    d = _lib.VolumeSampleDesc()
    d.nx, d.ny, d.nz = dims
    d.C, d.Q = C, Q
    d.lo, d.hi = (_lib.c_f32 * 3)(-1, -1, -1), (_lib.c_f32 * 3)(1, 1, 1)
    d.attr, d.points, d.out = P, P, P
    return d


def test_volume_sample_checks():
    _lib, lib = _load()
    assert lib.cn_volume_sample(None, None) == ARG and b"null descriptor" in _err(lib)
    for kw in (dict(dims=(8, 9, 1)), dict(C=0), dict(C=5), dict(Q=-1), dict(Q=1 << 31)):
        assert lib.cn_volume_sample(ctypes.byref(_sample_desc(_lib, **kw)), None) == SHAPE, kw
    d = _sample_desc(_lib)
    d.hi = (_lib.c_f32 * 3)(1, -1, 1)
    assert lib.cn_volume_sample(ctypes.byref(d), None) == SHAPE and b"hi must exceed lo" in _err(lib)
    for field in ("attr", "points", "out"):
        d = _sample_desc(_lib)
        setattr(d, field, None)
        assert lib.cn_volume_sample(ctypes.byref(d), None) == ARG and b"null" in _err(lib), field
    d = _sample_desc(_lib)
    d.mask = P + 3
    assert lib.cn_volume_sample(ctypes.byref(d), None) == ALIGN
    d = _sample_desc(_lib, Q=0)
    d.points = d.out = None
    assert lib.cn_volume_sample(ctypes.byref(d), None) == 0  # nothing to do: no launch


def test_observed_mesher_checks_are_the_meshers():
    _lib, lib = _load()
    big = 1 << 40
    for name in ("cn_mesh_count_observed", "cn_mesh_emit_observed"):
        fn = getattr(lib, name)
        assert fn(None, P, big, None) == ARG and name.encode() + b": null descriptor" in _err(lib)
        d = _lib.MeshDesc()
        d.nx, d.ny, d.nz, d.u, d.counts = 8, 1, 8, P, P
        assert fn(ctypes.byref(d), P, big, None) == SHAPE and b"each at least 2" in _err(lib)
        d.ny = 8
        need = lib.cn_mesh_workspace_bytes(8, 8, 8)
        assert fn(ctypes.byref(d), P, need - 1, None) == SHAPE and b"workspace" in _err(lib)
        assert fn(ctypes.byref(d), P + 16, need, None) == ALIGN and b"256-byte" in _err(lib)
        d.u = None
        assert fn(ctypes.byref(d), P, need, None) == ARG and b"null u" in _err(lib)
    d = _lib.MeshDesc()
    d.nx, d.ny, d.nz, d.u, d.counts = 8, 8, 8, P, P
    d.max_vertices, d.max_triangles = 4, 4
    assert lib.cn_mesh_emit_observed(ctypes.byref(d), P, big, None) == ARG and b"null vertices" in _err(lib)


STRUCTS = (("cn_tsdf_desc", "TsdfDesc"), ("cn_tsdf_finalize_desc", "TsdfFinalizeDesc"),
           ("cn_volume_sample_desc", "VolumeSampleDesc"))


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
    D, F, S = _lib.TsdfDesc, _lib.TsdfFinalizeDesc, _lib.VolumeSampleDesc
    assert (D.lo.offset, D.N.offset, D.proj.offset, D.color.offset, D.trunc.offset, D.no_reject.offset, D.tsum.offset,
            D.csum.offset, ctypes.sizeof(D)) == (12, 36, 48, 64, 72, 84, 88, 104, 112)
    assert (F.min_weight.offset, F.tsum.offset, F.u.offset, F.rgb.offset, ctypes.sizeof(F)) == (12, 16, 40, 48, 56)
    assert (S.C.offset, S.lo.offset, S.attr.offset, S.Q.offset, S.fill.offset, S.out.offset, ctypes.sizeof(S)) == \
        (12, 16, 40, 56, 72, 80, 88)


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
