"""Every split-M kernel of cn_wgrad (linear_cases.WGRAD: the ten names cn_wgrad_kernel_name can return) against
float64 Y0^T X0 (+ Y1^T X1) and sum(Y0), with the options no other test sets: accumulate, n_out / k_out at the
padded tile, ld_dw > k_out, M = 0, and the same jobs through ops.WgradQueue; cn_colsum with accumulate and wdiv.

The bars are the existing ones: rtol 1e-4, atol 1e-6 sqrt(M) + 1e-5 (test_wgrad_matches_torch, test_wgrad_bf16;
the bf16 mode against bf16-rounded operands), and for bf16x6 also max error <= 2 x the exact-fp32 kernel's + 1e-7
scale, mean error <= 1.5 x its mean + 1e-8 scale (test_wgrad_x6_matches_fp32_accuracy); cn_colsum rtol 1e-5,
atol 1e-4 (test_row_head_colsum_scale_cols).  The padding columns of Y and X hold finite garbage unless a case
says otherwise: they must not reach dW[:N, :K]."""
import functools

import pytest
import torch

import linear_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = (0, 1, 63, 64, 65, 513, 1025)
SENT = 7.0


def _rnd(*s, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(*s, generator=g) * 2 - 1) * scale).to(DEV)


@functools.lru_cache(maxsize=1)
def _pool():
    return {k: _rnd(max(MS), 256, seed=60 + i) for i, k in enumerate(("Y0", "X0", "Y1", "X1"))}


def _padded(c):
    """(Npad, Kpad): the output tile grid of the case's kernel, as wgrad_geometry (csrc/cn_wgrad.hip) lays it out:
    256x256 tiles on the stage rings (its tile 2), 256x64 on the narrow ring (tile 3), else 128x128 where
    K % 128 == 0 (tile 0) and 128x64 (tile 1)."""
    if c.kernel.startswith(("wgrad_x6r", "wgrad_b16r", "wgrad_b16d")):
        bn, bk = 256, 256
    elif c.kernel.startswith("wgrad_x6n"):
        bn, bk = 256, 64
    else:
        bn, bk = 128, 128 if c.K % 128 == 0 else 64
    return -(-c.N // bn) * bn, -(-c.K // bk) * bk


def _operands(c, M, pairs, zero_pad=False):
    """Y0, X0, Y1, X1 with the case's leading dimensions (at least one row is allocated: M = 0 needs pointers)."""
    p = _pool()
    out = []
    for k, ld, n, img in (("Y0", c.ldy, c.N, c.images[0]), ("X0", c.ldx, c.K, c.images[1]),
                          ("Y1", c.ldy, c.N, c.images[0]), ("X1", c.ldx, c.K, c.images[1])):
        # (a fresh tensor: a one-row slice counts as contiguous and would keep the pool's row length)
        t = torch.empty(max(M, 1), ld, device=DEV).copy_(p[k][:max(M, 1), :ld])
        if zero_pad:
            t[:, n:] = 0
        out.append(t.bfloat16() if img else t)
    return out if pairs == 2 else out[:2] + [None, None]


def _exact(c, M, ops4):
    """(dW, db) in float64; the bf16 mode multiplies bf16-rounded operands, db sums Y0 as stored."""
    r = (lambda t: t.bfloat16().double()) if c.mode == "bf16" else (lambda t: t.double())
    Y0, X0, Y1, X1 = ops4
    dW = r(Y0[:M]).t() @ r(X0[:M])
    if Y1 is not None:
        dW = dW + r(Y1[:M]).t() @ r(X1[:M])
    return dW, Y0[:M].double().sum(0)


def _call(c, M, ops4, dW, db, accumulate=False, mode=None):
    """cn_wgrad over the first M rows (ops.wgrad takes M from Y0: the descriptor is its own, M set here)."""
    from copenerf import _lib, ops
    Y0, X0, Y1, X1 = ops4
    d, ws = ops._wgrad_desc(Y0, X0, c.N, c.K, dW, db, Y1, X1, accumulate, mode or c.mode)
    d.M = M
    if mode is None:
        assert ops.kernel_name(_lib.load().cn_wgrad_kernel_name, d).startswith("void cn::" + c.kernel + "(")
    _lib.check(_lib.load().cn_wgrad(d, ops._stream()), "cn_wgrad")
    return ws


def _close(got, want, M, msg):
    torch.testing.assert_close(got.double(), want, rtol=1e-4, atol=1e-6 * M ** 0.5 + 1e-5, msg=lambda m: f"{msg}: {m}")


@pytest.mark.parametrize("c", LC.WGRAD, ids=[c.kernel.replace(", ", "_") + "-" + c.mode for c in LC.WGRAD])
@pytest.mark.parametrize("pairs", [1, 2])
def test_wgrad_instance_matches_float64(c, pairs):
    Np, Kp = _padded(c)
    for M in MS:
        where = f"{c.kernel} M={M} pairs={pairs}"
        ops4 = _operands(c, M, pairs)
        eW, eb = _exact(c, M, ops4)
        # plain: n_out = N, k_out = K, garbage in the padding columns of Y / X
        dW, db = torch.full((c.N, c.K), float("nan"), device=DEV), torch.full((c.N,), float("nan"), device=DEV)
        _call(c, M, ops4, dW, db)
        if M == 0:
            assert torch.all(dW == 0) and torch.all(db == 0), where
        _close(dW, eW[:c.N, :c.K], M, where + " dW")
        _close(db, eb[:c.N], M, where + " db")
        if c.mode == "bf16x6" and M > 0:
            fW, fb = torch.empty_like(dW), torch.empty_like(db)
            _call(c, M, ops4, fW, fb, mode="fp32")
            e6, e32 = (dW.double() - eW[:c.N, :c.K]).abs(), (fW.double() - eW[:c.N, :c.K]).abs()
            scale = eW.abs().max().item() + 1e-30
            print(f"{where}: fp32 max {e32.max().item():.3e} bf16x6 max {e6.max().item():.3e} (|dW| max {scale:.2f})")
            assert e6.max().item() <= 2.0 * e32.max().item() + 1e-7 * scale, where
            assert e6.mean().item() <= 1.5 * e32.mean().item() + 1e-8 * scale, where
        # accumulate: prefill + gradient, twice from the same prefill bitwise equal (a fixed slab order)
        pW, pb = _rnd(c.N, c.K, seed=70), _rnd(c.N, seed=71)
        aW, ab = pW.clone(), pb.clone()
        _call(c, M, ops4, aW, ab, accumulate=True)
        _close(aW, pW.double() + eW[:c.N, :c.K], M, where + " accumulated dW")
        _close(ab, pb.double() + eb[:c.N], M, where + " accumulated db")
        if M == 0:
            assert torch.equal(aW, pW) and torch.equal(ab, pb), where
        bW, bb = pW.clone(), pb.clone()
        _call(c, M, ops4, bW, bb, accumulate=True)
        assert torch.equal(aW, bW) and torch.equal(ab, bb), where
        # n_out / k_out at the padded tile with zero padding columns: the extra rows and columns are zero;
        # dW is a column slice (ld_dw > k_out) whose sentinel columns stay
        zops = _operands(c, M, pairs, zero_pad=True)
        wide = torch.full((Np, Kp + 8), SENT, device=DEV)
        zb = torch.full((Np,), float("nan"), device=DEV)
        _call(c, M, zops, wide[:, :Kp], zb)
        _close(wide[:c.N, :c.K], eW[:c.N, :c.K], M, where + " padded dW")
        _close(zb[:c.N], eb[:c.N], M, where + " padded db")
        assert torch.all(wide[c.N:, :Kp] == 0) and torch.all(wide[:, c.K:Kp] == 0) and torch.all(zb[c.N:] == 0), where
        assert torch.all(wide[:, Kp:] == SENT), where
        # ld_dw > k_out at n_out = N, k_out = K
        wide = torch.full((c.N, c.K + 8), SENT, device=DEV)
        _call(c, M, ops4, wide[:, :c.K], None)
        assert torch.equal(wide[:, :c.K], dW) and torch.all(wide[:, c.K:] == SENT), where


def test_wgrad_queue_matches_float64():
    """The same jobs through ops.WgradQueue, each against float64: the stage-ring kernels' jobs (named
    ...(cn::WgradBatch)) wait in the queue and share one cn_wgrad_batch launch per kernel, the others launch at
    add().  Every M of the per-kernel test that a tensor can carry (the queue takes M from Y0's rows)."""
    from copenerf import ops
    q = ops.WgradQueue()
    jobs = []
    ring = [c for c in LC.WGRAD if c.kernel.startswith(("wgrad_x6r", "wgrad_b16r", "wgrad_b16d"))]
    assert len(ring) == 3
    for M in MS[1:]:
        for c in LC.WGRAD:
            for pairs in (1, 2):
                ops4 = _operands(c, M, pairs)
                dW, db = torch.full((c.N, c.K), float("nan"), device=DEV), torch.full((c.N,), float("nan"), device=DEV)
                q.add(ops4[0], ops4[1], c.N, c.K, dW, db=db, Y1=ops4[2], X1=ops4[3], mode=c.mode)
                jobs.append((c, M, pairs, ops4, dW, db))
    # the batch path is taken: every ring job is still queued, nothing else is
    assert len(q.jobs) == len(ring) * 2 * len(MS[1:])
    q.flush()
    assert not q.jobs
    for c, M, pairs, ops4, dW, db in jobs:
        eW, eb = _exact(c, M, ops4)
        where = f"queued {c.kernel} M={M} pairs={pairs}"
        _close(dW, eW[:c.N, :c.K], M, where + " dW")
        _close(db, eb[:c.N], M, where + " db")


@pytest.mark.parametrize("M", [1, 1537, 5000])
def test_colsum_accumulates(M):
    """out += (sum_m w[m] X[m]) / wdiv (fields.py's create_graph term of lin8's sdf row), with and without w."""
    from copenerf import ops
    K = 204
    X, w = _rnd(M, 256, seed=80), _rnd(M, seed=81)
    for wv in (w, None):
        pre = _rnd(K, seed=82)
        out = torch.cat([pre, torch.full((4,), SENT, device=DEV)])
        ops.colsum(X, K, out, w=wv, wdiv=2.0, accumulate=True)
        xs = X[:, :K].double() * (1.0 if wv is None else wv.double()[:, None])
        torch.testing.assert_close(out[:K].double(), pre.double() + xs.sum(0) / 2, rtol=1e-5, atol=1e-4)
        assert torch.all(out[K:] == SENT)
        again = torch.cat([pre, torch.full((4,), SENT, device=DEV)])
        ops.colsum(X, K, again, w=wv, wdiv=2.0, accumulate=True)
        assert torch.equal(out, again)
