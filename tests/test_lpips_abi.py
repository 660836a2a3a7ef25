"""ABI v20 (cn_lpips, its workspace query and the two seam kernels) without a device: the exports exist and are
bound, the descriptor's layout follows the header, the workspace formula, and every refusal fires on the host
before anything launches."""
import ctypes
import re

from test_abi import HEADER, _declared

NAMES = ("cn_lpips_patches", "cn_lpips_head_workspace_bytes", "cn_lpips_head", "cn_lpips_workspace_bytes", "cn_lpips")
P = 4096  # an aligned placeholder, never dereferenced: every call below fails on the host
X6, BF16, F32 = 2, 1, 0


def _rup(n, a=256):
    return (n + a - 1) // a * a


def test_lpips_exports_are_declared_bound_and_versioned():
    from copenerf import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _declared() and name in _lib.SIGNATURES and hasattr(lib, name), name
    m = re.search(r"#define CN_ABI_VERSION (\d+)", open(HEADER).read())
    assert lib.cn_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 20
    assert len(_lib.SIGNATURES["cn_lpips"][1]) == 4 and len(_lib.SIGNATURES["cn_lpips_patches"][1]) == 12
    assert len(_lib.SIGNATURES["cn_lpips_head"][1]) == 9


def test_lpips_desc_layout_matches_header_order():
    from copenerf import _lib
    body = re.search(r"typedef struct cn_lpips_desc \{(.*?)\} cn_lpips_desc;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names, counts = [], {}
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?\w+\s*\**", "", decl.strip())
        for n in filter(None, (x.strip(" *") for x in decl.split(","))):
            m = re.match(r"(\w+)(?:\[(\d+)\])?$", n)
            names.append(m.group(1))
            counts[m.group(1)] = int(m.group(2) or 1)
    assert names == [f[0] for f in _lib.LpipsDesc._fields_]
    assert counts["weights"] == counts["bias"] == _lib.LPIPS_CONVS == 13 and counts["lin"] == _lib.LPIPS_TAPS == 5
    # two pointers, two ints, 31 pointers, two ints, one pointer: no padding
    assert ctypes.sizeof(_lib.LpipsDesc) == 8 * 2 + 4 * 2 + 8 * 31 + 4 * 2 + 8
    assert _lib.LpipsDesc.out.offset == ctypes.sizeof(_lib.LpipsDesc) - 8


def _want_bytes(H, W, band_rows, fmt):
    """The header's formula: two maps of 2 H W 64 floats, the largest band of patches, one partial per 64 pixels
    of each tap."""
    widths = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
    pooled, taps = (2, 4, 7, 10), (1, 3, 6, 9, 12)
    h, w, patch, part = H, W, 0, 0
    for l in range(13):
        if l in pooled:
            h, w = h // 2, w // 2
        kpad = (64 if fmt == BF16 else 32) if l == 0 else 9 * widths[l - 1]
        row = 2 * w * kpad * 4
        most = band_rows if band_rows > 0 else max(1, (576 << 20) // row)
        rows = -(-h // -(-h // most))          # bands of equal height up to one row
        patch = max(patch, _rup(row * rows))
        if l in taps:
            part += _rup(-(-h * w // 64) * 4)
    return 2 * _rup(2 * H * W * 64 * 4) + patch + part


def test_lpips_workspace_formula_and_monotonicity():
    from copenerf import _lib
    lib = _lib.load()
    for H, W, band, fmt in ((16, 16, 0, X6), (37, 53, 0, X6), (37, 53, 5, X6), (37, 53, 1, BF16), (17, 31, 0, F32),
                            (540, 960, 0, X6), (135, 240, 0, BF16), (540, 960, 7, X6)):
        assert lib.cn_lpips_workspace_bytes(H, W, band, fmt) == _want_bytes(H, W, band, fmt), (H, W, band, fmt)
    # the library's choice keeps the patch matrix within 576 MiB at 540 x 960
    assert lib.cn_lpips_workspace_bytes(540, 960, 0, X6) <= 2 * _rup(2 * 540 * 960 * 64 * 4) + (576 << 20) + (1 << 20)
    assert lib.cn_lpips_workspace_bytes(540, 960, 540, X6) > 2 * 540 * 960 * 576 * 4   # a whole-height band
    sizes = [(16, 16), (16, 17), (17, 31), (37, 53), (64, 64), (135, 240), (270, 480), (540, 960), (1080, 1920)]
    got = [lib.cn_lpips_workspace_bytes(h, w, 0, X6) for h, w in sizes]
    assert all(g > 0 for g in got) and got == sorted(got) and len(set(got)) == len(got)
    for bad in ((15, 64, 0, X6), (64, 15, 0, X6), (0, 0, 0, X6), (-1, 64, 0, X6), (64, 64, -1, X6), (64, 64, 0, 3),
                (8193, 8192, 0, X6)):
        assert lib.cn_lpips_workspace_bytes(*bad) == 0, bad
    assert lib.cn_lpips_workspace_bytes(8192, 8192, 0, X6) > 0
    assert lib.cn_lpips_head_workspace_bytes(0) == 0 and lib.cn_lpips_head_workspace_bytes(2 ** 26 + 1) == 0
    assert lib.cn_lpips_head_workspace_bytes(117) == 256 and lib.cn_lpips_head_workspace_bytes(64 * 65) == _rup(65 * 4)


def _desc(_lib, **kw):
    d = _lib.LpipsDesc()
    d.pred = d.gt = d.out = P
    d.H, d.W, d.mfma_dtype = 37, 53, X6
    for l in range(13):
        d.weights[l] = d.bias[l] = P
    for t in range(5):
        d.lin[t] = P
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def test_lpips_argument_checks_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    need = lib.cn_lpips_workspace_bytes(37, 53, 0, X6)

    def call(ws=P, ws_bytes=need, **kw):
        return lib.cn_lpips(ctypes.byref(_desc(_lib, **kw)), ws, ws_bytes, None)

    assert lib.cn_lpips(None, P, need, None) == -2 and b"null desc" in lib.cn_last_error()
    for kw in (dict(H=15), dict(W=15), dict(H=0), dict(W=-3)):
        assert call(**kw) == -2, kw
        assert b"at least 16" in lib.cn_last_error()
    assert call(H=8193, W=8192, ws_bytes=1 << 60) == -2 and b"too large" in lib.cn_last_error()
    assert call(band_rows=-1) == -2 and b"band_rows" in lib.cn_last_error()
    assert call(mfma_dtype=3) == -2 and b"mfma_dtype" in lib.cn_last_error()
    for kw in (dict(pred=None), dict(gt=None), dict(out=None), dict(weights=(0, None)), dict(weights=(12, None)),
               dict(bias=(5, None)), dict(lin=(0, None)), dict(lin=(4, None))):
        assert call(**kw) == -2, kw
        assert b"null" in lib.cn_last_error()
    assert call(ws=None) == -2 and call(ws_bytes=need - 1) == -2 and call(ws_bytes=-1) == -2
    assert b"workspace" in lib.cn_last_error()
    assert call(ws_bytes=lib.cn_lpips_workspace_bytes(37, 53, 1, X6), band_rows=5) == -2  # sized for a thinner band
    assert call(ws=P + 16) == -3 and call(pred=P + 2) == -3 and call(lin=(2, P + 4)) == -3


def test_lpips_seam_argument_checks_without_gpu():
    from copenerf import _lib
    lib = _lib.load()

    def patches(mode=0, n=2, Hs=11, Ws=13, C=64, src=P, src1=None, y0=0, rows=11, kpad=576, out=P):
        return lib.cn_lpips_patches(mode, n, Hs, Ws, C, src, src1, y0, rows, kpad, out, None)

    assert patches(mode=3) == -1 and patches(n=0) == -2 and patches(Hs=0) == -2
    assert patches(y0=5, rows=7) == -2 and b"outside" in lib.cn_last_error()
    assert patches(mode=1, rows=6) == -2    # the pooled map has 5 rows
    assert patches(C=48, kpad=432) == -2 and b"power of two" in lib.cn_last_error()
    assert patches(kpad=572) == -2 and patches(kpad=578) == -2
    assert patches(src=None) == -1 and patches(out=None) == -1 and patches(src=P + 4) == -3 and patches(out=P + 8) == -3
    assert patches(mode=2, C=3, kpad=32, src1=None) == -1    # two images, one pointer
    assert patches(mode=2, C=64, kpad=32, src1=P) == -2 and patches(mode=2, C=3, kpad=24, src1=P) == -2
    assert patches(mode=2, C=3, n=3, kpad=32, src1=P) == -2
    assert patches(rows=0) == 0    # an empty band: nothing to launch

    def head(C=64, Px=117, fx=P, fy=P, lin=P, out=P, ws=P, ws_bytes=256):
        return lib.cn_lpips_head(C, Px, fx, fy, lin, out, ws, ws_bytes, None)

    assert head(C=48) == -2 and head(C=1024) == -2 and head(C=8) == -2 and head(Px=0) == -2
    for k in ("fx", "fy", "lin", "out"):
        assert head(**{k: None}) == -1, k
    assert head(fx=P + 4) == -3 and head(lin=P + 8) == -3 and head(ws=P + 16) == -3
    assert head(ws=None) == -2 and head(ws_bytes=255) == -2 and b"workspace" in lib.cn_last_error()
