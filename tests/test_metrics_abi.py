"""ABI v18 (cn_image_metrics, cn_depth_errors and their workspace queries) without a device: the exports exist
and are bound, the workspace formulas, and every argument check fires on the host before anything launches."""
import ctypes
import re

from test_abi import HEADER, _declared

NAMES = ("cn_image_metrics_workspace_bytes", "cn_image_metrics", "cn_depth_errors_workspace_bytes", "cn_depth_errors")


def _rup(n, a=256):
    return (n + a - 1) // a * a


def test_metric_exports_are_declared_bound_and_versioned():
    from copenerf import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _declared() and name in _lib.SIGNATURES and hasattr(lib, name), name
    m = re.search(r"#define CN_ABI_VERSION (\d+)", open(HEADER).read())
    assert lib.cn_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 18
    assert len(_lib.SIGNATURES["cn_image_metrics"][1]) == 12 and len(_lib.SIGNATURES["cn_depth_errors"][1]) == 15


def test_image_metrics_workspace_formula():
    from copenerf import _lib
    lib = _lib.load()
    # two floats per 64 x 16 tile and (image, channel) plane, rounded up to 256 bytes
    for N, C, H, W in ((1, 1, 7, 9), (4, 3, 37, 53), (1, 3, 70, 130), (8, 3, 540, 960), (2, 1, 16, 64), (2, 1, 17, 65)):
        tiles = -(-W // 64) * -(-H // 16)
        assert lib.cn_image_metrics_workspace_bytes(N, C, H, W) == _rup(N * C * tiles * 8), (N, C, H, W)
    assert lib.cn_image_metrics_workspace_bytes(0, 3, 8, 8) == 0
    for bad in ((-1, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0), (21846, 3, 8, 8), (1, 1, 46341, 46341)):
        assert lib.cn_image_metrics_workspace_bytes(*bad) == 0, bad
    assert 21845 * 3 == 65535 and lib.cn_image_metrics_workspace_bytes(21845, 3, 8, 8) == _rup(65535 * 8)
    assert 46341 ** 2 >= 2 ** 31 > 46340 ** 2 and lib.cn_image_metrics_workspace_bytes(1, 1, 46340, 46340) > 0
    # 256 threads per tile along the grid's x: fewer than 2^24 tiles per plane
    assert lib.cn_image_metrics_workspace_bytes(1, 1, 2 ** 28, 1) == 0 and lib.cn_image_metrics_workspace_bytes(1, 1, 1, 2 ** 30) == 0
    assert lib.cn_image_metrics_workspace_bytes(1, 1, 2 ** 28 - 16, 1) == _rup((2 ** 24 - 1) * 8)


def test_depth_errors_workspace_formula():
    from copenerf import _lib
    lib = _lib.load()
    # eight floats per 2048 ground-truth pixels and image, rounded up to 256 bytes
    for N, H, W in ((1, 12, 16), (3, 37, 53), (2, 32, 64), (2, 32, 65), (16, 540, 960)):
        assert lib.cn_depth_errors_workspace_bytes(N, H, W) == _rup(N * -(-H * W // 2048) * 32), (N, H, W)
    assert lib.cn_depth_errors_workspace_bytes(0, 8, 8) == 0
    for bad in ((-1, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 46341, 46341)):
        assert lib.cn_depth_errors_workspace_bytes(*bad) == 0, bad


def test_image_metrics_argument_checks_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    P = 4096  # an aligned placeholder, never dereferenced: every call below fails on the host
    taps = (ctypes.c_float * 11)(*([1.0 / 11] * 11))
    need = lib.cn_image_metrics_workspace_bytes(4, 3, 37, 53)

    def call(N=4, C=3, H=37, W=53, pred=P, gt=P, taps=taps, out=P, ssim_map=None, ws=P, ws_bytes=need):
        return lib.cn_image_metrics(N, C, H, W, pred, gt, taps, out, ssim_map, ws, ws_bytes, None)

    for k in ("N", "C", "H", "W"):
        assert call(**{k: -1}) == -2, k
    assert call(C=0) == -2 and call(H=0) == -2 and call(W=0) == -2
    assert b"at least 1" in lib.cn_last_error()
    assert call(N=21846) == -2 and b"jobs" in lib.cn_last_error()
    assert call(N=1, C=1, H=46341, W=46341) == -2 and b"too large" in lib.cn_last_error()
    assert call(N=0, pred=None, gt=None, taps=None, out=None, ws=None, ws_bytes=0) == 0  # no images: nothing to do
    for k in ("pred", "gt", "taps", "out"):
        assert call(**{k: None}) == -1, k
        assert b"null" in lib.cn_last_error()
    # a plane the other bounds admit (H W < 2^31) whose tiles the grid cannot hold: 2^24 tiles of 64 x 16
    assert call(N=1, C=1, H=2 ** 28, W=1) == -2 and b"tiles" in lib.cn_last_error()
    assert call(N=1, C=1, H=2 ** 31 - 1, W=1) == -2 and b"tiles" in lib.cn_last_error()
    odd_taps = ctypes.cast(ctypes.addressof(taps) + 2, ctypes.POINTER(ctypes.c_float))  # the host array, misaligned
    for k, v in (("pred", P + 2), ("gt", P + 2), ("out", P + 2), ("ssim_map", P + 2), ("taps", odd_taps)):
        assert call(**{k: v}) == -3, k
        assert b"aligned" in lib.cn_last_error()
    assert call(ws=None) == -2 and call(ws_bytes=need - 1) == -2 and call(ws_bytes=-1) == -2
    assert b"workspace" in lib.cn_last_error()
    assert call(ws=P + 16) == -3


def test_depth_errors_argument_checks_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    P = 4096
    need = lib.cn_depth_errors_workspace_bytes(3, 37, 53)

    def call(N=3, Hg=37, Wg=53, gt=P, Hp=19, Wp=27, pred=P, ratio=P, lo=0.1, hi=80.0, clamp=1, out=P, ws=P,
             ws_bytes=need):
        return lib.cn_depth_errors(N, Hg, Wg, gt, Hp, Wp, pred, ratio, lo, hi, clamp, out, ws, ws_bytes, None)

    assert call(N=-1) == -2 and call(N=65536) == -2
    for k in ("Hg", "Wg", "Hp", "Wp"):
        assert call(**{k: 0}) == -2, k
    assert call(Hg=46341, Wg=46341) == -2 and call(Hp=46341, Wp=46341) == -2
    assert call(N=0, gt=None, pred=None, ratio=None, out=None, ws=None, ws_bytes=0) == 0
    for k in ("gt", "pred", "ratio", "out"):
        assert call(**{k: None}) == -1, k
        assert b"null" in lib.cn_last_error()
        assert call(**{k: P + 2}) == -3, k
    assert call(ws=None) == -2 and call(ws_bytes=need - 1) == -2
    assert b"workspace" in lib.cn_last_error()
    assert call(ws=P + 16) == -3
