"""ABI v17 (cn_refine_workspace_bytes / cn_refine_warp) without a device: the exports exist and are bound,
the workspace formula, and every argument check fires on the host before anything launches."""
import re

from test_abi import HEADER, _declared


def _rup(n, a=256):
    return (n + a - 1) // a * a


def test_refine_exports_are_declared_bound_and_versioned():
    from copenerf import _lib
    lib = _lib.load()
    for name in ("cn_refine_workspace_bytes", "cn_refine_warp"):
        assert name in _declared() and name in _lib.SIGNATURES and hasattr(lib, name)
    m = re.search(r"#define CN_ABI_VERSION (\d+)", open(HEADER).read())
    assert lib.cn_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 17
    assert len(_lib.SIGNATURES["cn_refine_warp"][1]) == 17


def test_refine_workspace_formula():
    from copenerf import _lib
    lib = _lib.load()
    # one 64-byte partial per 64 x 16 pixel tile and job, rounded up to 256 bytes
    for J, H, W in ((1, 3, 5), (8, 37, 53), (6, 70, 130), (32, 540, 960), (2, 16, 64), (2, 17, 65)):
        tiles = -(-W // 64) * -(-H // 16)
        assert lib.cn_refine_workspace_bytes(J, H, W) == _rup(tiles * J * 64), (J, H, W)
    assert lib.cn_refine_workspace_bytes(0, 8, 8) == 0
    # shape errors size to 0: a one-pixel axis (the grid divides by (W-1)/2), 3 H W >= 2^31, too many jobs
    assert lib.cn_refine_workspace_bytes(2, 1, 8) == 0 and lib.cn_refine_workspace_bytes(2, 8, 1) == 0
    assert 3 * 26755 * 26755 >= 2 ** 31 > 3 * 26754 * 26754
    assert lib.cn_refine_workspace_bytes(1, 26755, 26755) == 0
    assert lib.cn_refine_workspace_bytes(1, 26754, 26754) > 0
    assert lib.cn_refine_workspace_bytes(65536, 8, 8) == 0 and lib.cn_refine_workspace_bytes(-1, 8, 8) == 0


def test_refine_warp_argument_checks_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    P = 4096  # an aligned placeholder, never dereferenced: every call below fails on the host
    need = lib.cn_refine_workspace_bytes(4, 37, 53)

    def call(N=5, H=37, W=53, J=4, images=P, depth=P, tgt=P, src=P, pose=P, K=P, Kinv=P, sums=P, dpose=P, warped=None,
             ws=P, ws_bytes=need):
        return lib.cn_refine_warp(N, H, W, J, images, depth, tgt, src, pose, K, Kinv, sums, dpose, warped, ws, ws_bytes,
                                  None)

    assert call(H=1) == -2 and b"at least 2" in lib.cn_last_error()
    assert call(H=26755, W=26755) == -2 and b"too large" in lib.cn_last_error()
    assert call(J=-1) == -2 and call(J=65536) == -2
    assert call(N=0) == -2
    assert call(J=0, images=None, ws=None, ws_bytes=0) == 0  # no jobs: nothing to do
    for k in ("images", "depth", "tgt", "src", "pose", "K", "Kinv", "sums", "dpose"):
        assert call(**{k: None}) == -1, k
        assert b"null" in lib.cn_last_error()
    for k in ("images", "depth", "tgt", "src", "pose", "K", "Kinv", "sums", "warped"):
        assert call(**{k: P + 2}) == -3, k
    assert call(dpose=P + 4) == -3 and b"dpose" in lib.cn_last_error()
    assert call(ws=None) == -2 and call(ws_bytes=need - 1) == -2
    assert b"workspace" in lib.cn_last_error()
    assert call(ws=P + 16) == -3
