"""ABI v22 without a device: cn_linear_desc.tile = 3 / 4 (the two-per-CU 128x256 and the one-per-CU 256x256 bf16x6
tiles) and the library's own choice of the 128x256 tile, as cn_linear_kernel_name reports it (the launch's own
function decides both)."""
import ctypes

import pytest

TALL2 = "void cn::linear_kernel<2, 2, 2, 4, 16, 2, 2, %d, false, 2>(cn::LinearArgs)"
SQ = "void cn::linear_kernel<4, 2, 2, 4, 16, 1, 2, %d, false, 2>(cn::LinearArgs)"
T128 = "void cn::linear_kernel<2, 2, 2, 2, 16, 2, 2, %d, false, 2>(cn::LinearArgs)"
STORE, SOFTPLUS, RELU, MUL, TANGENT, BWD_SOFTPLUS, BWD_RELU, HEAD = 0, 1, 2, 3, 4, 5, 6, 8
# the epilogue classes the library moves to the 128x256 tile at C2's layer shape (the step A/B)
MOVED = (BWD_SOFTPLUS, MUL, TANGENT, BWD_RELU)


def _desc(epi, tile=0, M=524288, N=256, K=256):
    from copenerf import _lib
    d = _lib.LinearDesc()
    d.M, d.N, d.K, d.K1, d.ldb, d.epilogue, d.tile, d.mfma_dtype = M, N, K, K, 256, epi, tile, 2
    return d


def _name(d):
    from copenerf import _lib, ops
    return ops.kernel_name(_lib.load().cn_linear_kernel_name, d)


def test_abi_version_matches_the_header():
    from copenerf import _lib
    assert _lib.load().cn_abi_version() == _lib.ABI_VERSION == 22


@pytest.mark.parametrize("epi", (STORE, SOFTPLUS, RELU, MUL, TANGENT, BWD_SOFTPLUS, BWD_RELU))
def test_library_choice_at_c2_shape(epi):
    """M = 524,288, N = K = 256: the moved classes on the two-per-CU 128x256 tile, the others where they were."""
    want = TALL2 if epi in MOVED else (T128 if epi == BWD_SOFTPLUS else SQ)
    assert _name(_desc(epi)) == want % epi
    # no second tile per workgroup to overlap with: the earlier tiles
    assert _name(_desc(epi, M=65536)) == (T128 if epi == BWD_SOFTPLUS else SQ) % epi


def test_pinned_launches_keep_their_tile():
    """C2's hidden-layer SOFTPLUS and SOFTPLUS_HEAD on the 256x256 tile, the colour network's RELU with a rank-1
    term on the 256x128 tile, the skip layer's split-output MUL on the 256x256 tile (ragged and at C2's M)."""
    assert _name(_desc(SOFTPLUS)) == SQ % SOFTPLUS
    assert _name(_desc(HEAD)) == SQ % HEAD
    d = _desc(RELU)
    d.rowv = 16
    assert _name(d) == "void cn::linear_kernel<4, 2, 2, 2, 32, 1, 2, 2, true, 2>(cn::LinearArgs)"
    for M in (1537, 524288):
        d = _desc(MUL, M=M)
        d.out_split, d.nsplit = 16, 204
        assert _name(d) == SQ % MUL


def test_forced_tiles():
    """tile 3 / 4 are honoured for every epilogue and any M; outside 128 < N <= 256, with a rank-1 term or
    outside the bf16x6 mode they are CN_ERR_UNSUPPORTED (-5 is not assumed: any negative status but CN_ERR_ARG's
    of tile 5)."""
    from copenerf import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    for epi in (STORE, SOFTPLUS, RELU, MUL, TANGENT, BWD_SOFTPLUS, BWD_RELU, HEAD):
        for M in (1, 1537, 524288):
            assert _name(_desc(epi, tile=3, M=M)) == TALL2 % epi
            assert _name(_desc(epi, tile=4, M=M)) == SQ % epi
    assert _name(_desc(MUL, tile=3, N=204)) == TALL2 % MUL
    bad_arg = lib.cn_linear_kernel_name(_desc(STORE, tile=5), buf, 256)
    assert bad_arg < 0 and lib.cn_linear_kernel_name(_desc(STORE, tile=-1), buf, 256) == bad_arg
    for tile in (3, 4):
        unsupported = lib.cn_linear_kernel_name(_desc(STORE, tile=tile, N=128), buf, 256)
        assert unsupported < 0 and unsupported != bad_arg
        assert lib.cn_linear_kernel_name(_desc(STORE, tile=tile, N=320), buf, 256) == unsupported
        d = _desc(RELU, tile=tile)
        d.rowv = 16
        assert lib.cn_linear_kernel_name(d, buf, 256) == unsupported
        d = _desc(STORE, tile=tile)
        d.mfma_dtype = 0
        assert lib.cn_linear_kernel_name(d, buf, 256) == unsupported


def test_tile_tag_names_the_class():
    from copenerf import ops
    assert ops._tile_tag(TALL2 % MUL, 0) == "tall2"
