"""ABI v19 (cn_ray_visuals, cn_visual_images and their workspace queries) without a device: the exports exist and
are bound, the workspace formulas, and every argument check fires on the host before anything launches."""
import ctypes
import re

from test_abi import HEADER, _declared

NAMES = ("cn_ray_visuals_workspace_bytes", "cn_ray_visuals", "cn_visual_images_workspace_bytes", "cn_visual_images")
P = 4096  # an aligned placeholder, never dereferenced: every call below ends on the host


def _rup(n, a=256):
    return (n + a - 1) // a * a


def test_visual_exports_are_declared_bound_and_versioned():
    from copenerf import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _declared() and name in _lib.SIGNATURES and hasattr(lib, name), name
    m = re.search(r"#define CN_ABI_VERSION (\d+)", open(HEADER).read())
    assert lib.cn_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 19
    assert len(_lib.SIGNATURES["cn_ray_visuals"][1]) == 21 and len(_lib.SIGNATURES["cn_visual_images"][1]) == 17


def test_workspace_formulas():
    from copenerf import _lib
    lib = _lib.load()
    # the image pass: eight floats per 2048 pixels, rounded up to 256 bytes
    for H, W in ((1, 1), (3, 5), (17, 70), (32, 64), (32, 65), (135, 240), (540, 960)):
        assert lib.cn_visual_images_workspace_bytes(H, W) == _rup(-(-H * W // 2048) * 32), (H, W)
    for bad in ((0, 8), (8, 0), (-1, 8), (8, -1), (46341, 46341), (2 ** 30, 2)):
        assert lib.cn_visual_images_workspace_bytes(*bad) == 0, bad
    assert 46341 ** 2 >= 2 ** 31 > 46340 ** 2 and lib.cn_visual_images_workspace_bytes(46340, 46340) > 0
    # the per-ray pass: room for the composed 3 x 4 map when there are Euler steps
    assert [lib.cn_ray_visuals_workspace_bytes(K) for K in (-1, 0, 1, 10, 1024, 1025)] == [0, 0, 256, 256, 256, 0]


def _ray_call(lib, **kw):
    scale = (ctypes.c_float * 2)(16.0, 12.0)
    a = dict(R=5, S=65, pts=P, ld_p=3, normals=P, ld_n=4, weights=P, world=None, K=10, omega=P, vel=P, dt=0.01, proj=P,
             pix=P, scale=scale, normal=P, depth=P, flow=P, ws=P, ws_bytes=256)
    a.update(kw)
    return lib.cn_ray_visuals(a["R"], a["S"], a["pts"], a["ld_p"], a["normals"], a["ld_n"], a["weights"], a["world"],
                              a["K"], a["omega"], a["vel"], a["dt"], a["proj"], a["pix"], a["scale"], a["normal"],
                              a["depth"], a["flow"], a["ws"], a["ws_bytes"], None)


def test_ray_visuals_argument_checks_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    call = lambda **kw: _ray_call(lib, **kw)  # noqa: E731
    assert call(R=-1) == -2 and call(S=0) == -2 and call(S=-3) == -2
    assert b"rays" in lib.cn_last_error()
    assert call(K=-1) == -2 and call(K=1025) == -2 and b"Euler" in lib.cn_last_error()
    assert call(ld_p=2) == -2 and call(ld_n=2) == -2 and call(ld_p=0) == -2
    assert b"leading" in lib.cn_last_error()
    # a flow needs steps, the projection and the pixels
    assert call(K=0) == -1 and b"K = 0" in lib.cn_last_error()
    for k in ("proj", "pix", "scale", "omega", "vel"):
        assert call(**{k: None}) == -1, k
        assert b"null" in lib.cn_last_error()
    # required inputs
    assert call(weights=None) == -1 and b"weights" in lib.cn_last_error()
    assert call(pts=None) == -1 and call(pts=None, flow=None, K=0) == -1 and b"pts" in lib.cn_last_error()
    assert call(normals=None) == -1 and b"normals" in lib.cn_last_error()
    for k in ("pts", "normals", "weights", "world", "omega", "vel", "proj", "pix", "normal", "depth", "flow"):
        assert call(**{k: P + 2}) == -3, k
        assert b"aligned" in lib.cn_last_error()
    assert call(ws=None) == -2 and call(ws_bytes=255) == -2 and call(ws_bytes=-1) == -2
    assert b"workspace" in lib.cn_last_error()
    assert call(ws=P + 16) == -3
    # no rays: nothing to do, whatever the pointers; the shape checks still come first
    assert call(R=0, pts=None, normals=None, weights=None, normal=None, depth=None, flow=None, ws=None, ws_bytes=0,
                K=0, omega=None, vel=None, proj=None, pix=None) == 0
    assert call(R=0) == 0 and call(R=0, S=0) == -2 and call(R=0, K=0) == -1


def test_visual_images_argument_checks_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    need = lib.cn_visual_images_workspace_bytes(17, 70)

    def call(H=17, W=70, rgb=P, depth=P, dmw=P, wz=P, normal=P, flow=P, stats=P, img=P, disp=P, disp_hw=P, nimg=P, fimg=P,
             ws=P, ws_bytes=need):
        return lib.cn_visual_images(H, W, rgb, depth, dmw, wz, normal, flow, stats, img, disp, disp_hw, nimg, fimg, ws,
                                    ws_bytes, None)

    for k in ("H", "W"):
        assert call(**{k: 0}) == -2 and call(**{k: -1}) == -2, k
    assert b"at least 1" in lib.cn_last_error()
    assert call(H=46341, W=46341) == -2 and b"too large" in lib.cn_last_error()
    # the normalised images need the statistics
    for k in ("disp", "disp_hw", "fimg"):
        others = {o: None for o in ("disp", "disp_hw", "fimg") if o != k}
        assert call(stats=None, **others) == -1, k
        assert b"stats" in lib.cn_last_error()
    for k in ("depth", "dmw", "wz"):
        assert call(**{k: None}) == -1, k
        assert b"statistics" in lib.cn_last_error()
    assert call(rgb=None) == -1 and call(normal=None) == -1 and call(flow=None) == -1
    assert b"null flow" in lib.cn_last_error()
    for k in ("rgb", "depth", "dmw", "wz", "normal", "flow", "stats"):
        assert call(**{k: P + 2}) == -3, k
    assert call(ws=None) == -2 and call(ws_bytes=need - 1) == -2 and call(ws_bytes=-1) == -2
    assert b"workspace" in lib.cn_last_error()
    assert call(ws=P + 16) == -3
