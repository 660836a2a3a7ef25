"""ABI v21 (cn_flow_rgb_fwd, cn_flow_rgb_bwd and their workspace query) without a device: the exports exist
and are bound, the workspace formula, and every refusal fires on the host before anything launches."""
import re

import pytest

from test_abi import HEADER, _declared

NAMES = ("cn_flow_rgb_workspace_bytes", "cn_flow_rgb_fwd", "cn_flow_rgb_bwd")
P = 4096  # an aligned placeholder, never dereferenced: every call below fails on the host


def test_flow_rgb_exports_are_declared_bound_and_versioned():
    from copenerf import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _declared() and name in _lib.SIGNATURES and hasattr(lib, name), name
    m = re.search(r"#define CN_ABI_VERSION (\d+)", open(HEADER).read())
    assert lib.cn_abi_version() == int(m.group(1)) == _lib.ABI_VERSION >= 21
    assert len(_lib.SIGNATURES["cn_flow_rgb_fwd"][1]) == 18 and len(_lib.SIGNATURES["cn_flow_rgb_bwd"][1]) == 20


def test_flow_rgb_workspace_formula():
    from copenerf import _lib
    lib = _lib.load()
    rup = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for R, T in ((0, 1), (1, 1), (3, 1), (64, 3), (65, 3), (200, 3), (1000, 3), (4096, 3), (4096, 8), (1 << 20, 8)):
        assert lib.cn_flow_rgb_workspace_bytes(R, T) == rup(-(-max(R, 1) // 64) * T * 48), (R, T)
    for bad in ((-1, 3), (16, 0), (16, 9), (16, -1)):
        assert lib.cn_flow_rgb_workspace_bytes(*bad) == 0, bad


def _args(**kw):
    a = dict(R=200, T=3, N=5, H=37, W=53, ray_acc=P, w2c=P, KS=P, pixn=P, pix=P, rgb_gt=P, images=P, frame=P,
             frame_valid=None)
    a.update(kw)
    return a


def _fwd(lib, sums=P, ws=P, ws_bytes=1 << 20, **kw):
    return lib.cn_flow_rgb_fwd(*_args(**kw).values(), sums, ws, ws_bytes, None)


def _bwd(lib, g_num=P, d_ray_acc=P, d_w2c=P, ws=P, ws_bytes=1 << 20, **kw):
    return lib.cn_flow_rgb_bwd(*_args(**kw).values(), g_num, d_ray_acc, d_w2c, ws, ws_bytes, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["fwd", "bwd"])
def test_flow_rgb_argument_checks_without_gpu(call):
    from copenerf import _lib
    lib = _lib.load()
    err = lib.cn_last_error
    for kw, word in ((dict(T=0), b"reference frames"), (dict(T=9), b"reference frames"), (dict(T=-2), b"reference frames"),
                     (dict(R=-1), b"rays"), (dict(H=0), b"at least 1"), (dict(W=0), b"at least 1"),
                     (dict(W=-5), b"at least 1"), (dict(N=0), b"stack of"), (dict(H=30000, W=30000), b"too large")):
        assert call(lib, **kw) == -2, kw
        assert word in err(), (kw, err())
    for name in ("ray_acc", "w2c", "KS", "pixn", "pix", "rgb_gt", "images", "frame"):
        assert call(lib, **{name: None}) == -1, name
        assert b"null" in err(), (name, err())
    assert call(lib, ray_acc=P + 4) == -3 and b"ray_acc not 16-byte aligned" in err()
    assert call(lib, ray_acc=P + 8) == -3 and call(lib, pix=P + 2) == -3 and call(lib, frame=P + 4) == -3
    need = lib.cn_flow_rgb_workspace_bytes(200, 3)
    assert call(lib, ws=None) == -2 and call(lib, ws_bytes=need - 1) == -2 and call(lib, ws_bytes=-1) == -2
    assert b"workspace" in err()
    assert call(lib, ws=P + 16, ws_bytes=need) == -3 and b"workspace" in err()


def test_flow_rgb_output_checks_without_gpu():
    from copenerf import _lib
    lib = _lib.load()
    assert _fwd(lib, sums=None) == -1 and b"null sums" in lib.cn_last_error()
    assert _fwd(lib, sums=P + 2) == -3
    for name in ("g_num", "d_ray_acc", "d_w2c"):
        assert _bwd(lib, **{name: None}) == -1, name
        assert b"null" in lib.cn_last_error()
    assert _bwd(lib, d_ray_acc=P + 8) == -3 and b"d_ray_acc" in lib.cn_last_error()
    assert _bwd(lib, d_w2c=P + 1) == -3


def test_trainer_refuses_an_unknown_flow_rgb_mode():
    from copenerf.train_step import SyntheticTrainer
    with pytest.raises(ValueError, match="flow_rgb"):
        SyntheticTrainer("cpu", flow_rgb="triton")
