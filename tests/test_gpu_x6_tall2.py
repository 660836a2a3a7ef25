"""The two-per-CU 128x256 bf16x6 tile of cn_linear (cn_linear_desc.tile = 3) against the one-per-CU 256x256
tile (tile = 4; BWD_SOFTPLUS: the 128x128 tile, tile = 2): the same six products in the same order into one
accumulation chain, so every output is bitwise equal.  Every epilogue built on the tile, every output (out0,
MUL's split buffer, SOFTPLUS_HEAD's out1 and sdf, direct and scattered), ragged and one-row M, one M at which
every persistent workgroup takes at least two tiles, N = 256 and the 204-wide layer on 256-wide rows, K = 128 /
256 / 512, a virtual concat, both M orders; no write past M rows or nzero columns; repeatable."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD = 264          # output row length: 8 sentinel columns past the 256-wide tile
PAD = 3           # sentinel rows past M
SENT = 7.0
SMALL_M = (1, 127, 128, 129, 1537)
EPIS = ("store", "softplus", "relu", "mul", "mul_split", "tangent", "bwd_softplus", "bwd_relu", "head", "head_idx")


def _rnd(*s, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*s, device=DEV, generator=g) * scale


@functools.lru_cache(maxsize=2)
def _inputs(Mmax):
    """Operands for every case of up to Mmax rows (built once, never written)."""
    from copenerf import ops
    A = _rnd(Mmax, 512, seed=1, scale=0.3)
    W = _rnd(256, 512, seed=2, scale=0.05)
    act = torch.nn.functional.softplus(_rnd(Mmax, 256, seed=3, scale=0.05), beta=100)
    d = dict(A=A, A2=_rnd(Mmax, 64, seed=4, scale=0.3), act=act, relu_src=act - 0.005,
             aux1=_rnd(Mmax, 256, seed=5), aux2=_rnd(Mmax, 256, seed=6), bias=_rnd(256, seed=7, scale=0.3),
             colv=_rnd(256, seed=8), head_w=_rnd(256, seed=9, scale=0.1), head_b=_rnd(1, seed=10),
             perm=torch.randperm(Mmax + PAD, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11)).int())
    for N in (204, 256):
        for K in (128, 256, 320, 512):
            Wn = W[:, :K].clone()
            Wn[N:] = 0  # rows past N are zero padding
            d["B", N, K] = ops.split_bf16x3(Wn)
    return d


def _launch(inp, epi, tile, M, N, K, nzero, flip=0, concat=False):
    """One cn_linear launch on `tile`; every output, sentinel rows and columns included."""
    from copenerf import ops
    full = lambda *s: torch.full(s, SENT, device=DEV)
    outs = {"out0": full(M + PAD, LD)}
    kw = dict(nzero=nzero, tile=tile, M=M)
    A = inp["A"][:M]
    if concat:  # columns k < 256 from A, the rest from A2
        kw.update(A2=inp["A2"][:M], K1=256)
    sg = dict(aux0=inp["act"][:M], aux_beta=100.0)
    if epi == "store":
        code, extra = ops.EPI_STORE, dict(bias=inp["bias"])
    elif epi == "softplus":
        code, extra = ops.EPI_SOFTPLUS, dict(bias=inp["bias"], odiv=ops.SQRT2)
    elif epi == "relu":
        code, extra = ops.EPI_RELU, dict(bias=inp["bias"])
    elif epi == "mul":
        code, extra = ops.EPI_MUL, dict(sg, adiv=ops.SQRT2)
    elif epi == "mul_split":  # columns [nsplit, N) go out raw to the split buffer
        nsplit = N - 52
        outs["split"] = full(M + PAD, 64)
        code, extra = ops.EPI_MUL, dict(sg, adiv=ops.SQRT2, nsplit=nsplit, out_split=outs["split"])
    elif epi == "tangent":
        code, extra = ops.EPI_TANGENT, dict(sg, odiv=ops.SQRT2)
    elif epi == "bwd_softplus":
        code, extra = ops.EPI_BWD_SOFTPLUS, dict(sg, aux1=inp["aux1"][:M], aux2=inp["aux2"][:M], aux2_scale=100.0)
    elif epi == "bwd_relu":
        code, extra = ops.EPI_BWD_RELU, dict(aux0=inp["relu_src"][:M])
    else:  # head: the sdf row-dot in row order; head_idx: scattered through a permutation
        outs["out1"], outs["sdf"] = full(M + PAD, LD), full(M + PAD)
        code = ops.EPI_SOFTPLUS_HEAD
        extra = dict(bias=inp["bias"], colv=inp["colv"], aux_beta=100.0, out1=outs["out1"], head_w=inp["head_w"],
                     head_b=inp["head_b"], head_out=outs["sdf"])
        if epi == "head_idx":
            # M distinct destinations anywhere in the M + PAD elements of the buffer
            extra["head_idx"] = inp["perm"][inp["perm"] < M + PAD][:M].contiguous()
            outs["idx"] = extra["head_idx"]
    ops._flip = 0 if flip else 1  # ops.linear alternates the M order: the launch gets flags = flip
    ops.linear(A, inp["B", N, K], N, K, outs["out0"], code, **kw, **extra)
    return outs


def _check_pair(inp, epi, M, N, K, nzero, flip=0, concat=False):
    ref_tile = 2 if epi == "bwd_softplus" else 4
    got = _launch(inp, epi, 3, M, N, K, nzero, flip, concat)
    again = _launch(inp, epi, 3, M, N, K, nzero, flip, concat)
    ref = _launch(inp, epi, ref_tile, M, N, K, nzero, flip, concat)
    torch.cuda.synchronize()
    where = f"{epi} M={M} N={N} K={K} nzero={nzero} flip={flip} concat={concat}"
    for name in ("out0", "out1", "split", "sdf"):
        if name not in got:
            continue
        assert torch.equal(got[name], ref[name]), f"{where}: {name} differs from tile {ref_tile}"
        assert torch.equal(got[name], again[name]), f"{where}: {name} not repeatable"
    # no stray writes: rows past M, columns past nzero, the zero fill of [N, nzero)
    for name in ("out0", "out1"):
        if name in got:
            o = got[name]
            assert torch.all(o[M:] == SENT) and torch.all(o[:, nzero:] == SENT), f"{where}: {name} sentinels"
            assert torch.all(o[:M, N:nzero] == 0), f"{where}: {name} zero fill"
            assert torch.isfinite(o[:M, :N]).all(), where
    if epi == "mul_split":
        assert torch.all(got["out0"][:M, N - 52:nzero] == 0), f"{where}: out0 under the split columns"
        s = got["split"]
        assert torch.all(s[M:] == SENT) and torch.all(s[:, 52:] == SENT), f"{where}: split sentinels"
        assert not torch.any(s[:M, :52] == SENT), where
    if "sdf" in got:
        s = got["sdf"]
        written = torch.zeros_like(s, dtype=torch.bool)
        written[got["idx"].long() if "idx" in got else torch.arange(M, device=DEV)] = True
        assert torch.all(s[~written] == SENT) and not torch.any(s[written] == SENT), f"{where}: sdf sentinels"


@pytest.mark.parametrize("epi", EPIS)
def test_tall2_equals_the_reference_tile_bitwise(epi):
    """Every small M (one row, one below / at / above a 128-row tile, ragged over 13 tiles) x N = 256 and the
    204-wide layer with nzero = 256 x K = 128, 256, 512; the concat (K1 = 256, K = 320) and the reverse M
    order at M = 1537."""
    inp = _inputs(1537)
    for M in SMALL_M:
        for N, nzero in ((256, 256), (204, 256)):
            for K in (128, 256, 512):
                _check_pair(inp, epi, M, N, K, nzero)
    _check_pair(inp, epi, 1537, 256, 320, 256, concat=True)
    _check_pair(inp, epi, 1537, 256, 256, 256, flip=1)
    _check_pair(inp, epi, 129, 204, 256, 256, flip=1)


@pytest.mark.parametrize("epi", EPIS)
def test_tall2_every_workgroup_takes_two_tiles(epi):
    """M = 2 (2 CUs) 128 + 77 rows: each of the 2 x CUs persistent workgroups walks at least two tiles (the
    prefetch across a tile boundary, the one-set B staging's hand-over) and the last tile is ragged."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = 2 * (2 * cus) * 128 + 77
    _check_pair(_inputs(M), epi, M, 256, 256, 256, flip=(len(epi) & 1))


def test_tall2_forced_where_it_is_not_built():
    """tile = 3 / 4 outside 128 < N <= 256 or with a rank-1 term: CN_ERR_UNSUPPORTED, nothing launched; tile = 5:
    CN_ERR_ARG."""
    from copenerf import ops
    inp = _inputs(1537)
    o = torch.full((200, LD), SENT, device=DEV)
    B128 = ops.split_bf16x3(torch.zeros(256, 256, device=DEV))
    for tile in (3, 4):
        with pytest.raises(RuntimeError):
            ops.linear(inp["A"][:200], B128, 128, 256, o, ops.EPI_STORE, bias=inp["bias"], tile=tile)
        with pytest.raises(RuntimeError):
            ops.linear(inp["A"][:200], inp["B", 256, 256], 256, 256, o, ops.EPI_RELU, bias=inp["bias"],
                       rowv=inp["aux1"][:200, 0].contiguous(), colv=inp["colv"], tile=tile)
    with pytest.raises(RuntimeError):
        ops.linear(inp["A"][:200], inp["B", 256, 256], 256, 256, o, ops.EPI_STORE, bias=inp["bias"], tile=5)
    torch.cuda.synchronize()
    assert torch.all(o == SENT)
