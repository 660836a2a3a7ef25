"""LPIPS on the device (cn_lpips, its two seam kernels, copenerf.metrics.LPIPS, ABI v20) against the float64
restatement (tests/lpips_ref.py), with full VGG16 widths and seeded random weights.

Shapes: 37 x 53 is odd at three pooling levels (37 -> 18 -> 9 -> 4 -> 2, 53 -> 26 -> 13 -> 6 -> 3); 16 x 16 is
the minimum (the last tap is 1 x 1); a batch of three pairs at 17 x 31.

Bars.  bf16x6 and fp32: each of the five per-block terms within 1e-4 relative of float64.  Measured on the CPU
at these shapes and seeds: the fp32 torch restatement is within 3e-6 of float64 per block, while transposed
taps move a block by at least 1.5e-2, a ceil-mode pool by at least 1.5e-3 and one dropped tap of the last
convolution by 5e-3 -- 1e-4 is about 30 x the rounding and 15 x below the smallest indexing mistake.
bf16: every term within twice the measured error of the restatement with both operands of every convolution
rounded to bf16 (bf16_measured below: 2.66e-2 measured, 5.33e-2 allowed)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
WEIGHT_SEED = 678
BAR = 1e-4
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def ref_weights():
    return R.make_weights(WEIGHT_SEED)


def loaded_weights():
    from copenerf import metrics
    convs, lins = ref_weights()
    return {"conv": [metrics.lpips_conv_matrix(w) for w, _ in convs], "bias": [b for _, b in convs], "lin": list(lins)}


@functools.lru_cache(maxsize=None)
def net(mode="bf16x6", band_rows=0):
    from copenerf import metrics
    return metrics.LPIPS(loaded_weights(), mode=mode, device=DEV, band_rows=band_rows)


@functools.lru_cache(maxsize=None)
def case(shape):
    """(a, b) fp32 on the host and the float64 terms [N, 5], computed once per shape."""
    a, b = R.pair_inputs(shape, seed=1)
    convs, lins = ref_weights()
    return a, b, R.lpips_layers(a, b, convs, lins)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_patches(mode, src, src1, C, Hs, Ws, n, y0, rows, kpad):
    from copenerf import _lib
    Wo = Ws // 2 if mode == 1 else Ws
    out = torch.full((n * rows * Wo, kpad), float("nan"), device=DEV)
    _lib.call("cn_lpips_patches", mode, n, Hs, Ws, C, src.data_ptr(), None if src1 is None else src1.data_ptr(), y0, rows,
              kpad, out.data_ptr(), _stream())
    return out.cpu()


# ---------------------------------------------------------------------------
# the patches kernel alone
@pytest.mark.parametrize("kpad", [576, 608])
def test_patches_plain_and_pool_are_bitwise_the_gather(kpad):
    g = torch.Generator().manual_seed(5)
    src = torch.randn(2, 11, 13, 64, generator=g)
    d = src.to(DEV)
    want = R.patches(src, 0, 11, kpad)
    got = run_patches(0, d, None, 64, 11, 13, 2, 0, 11, kpad)
    assert torch.equal(got, want)
    assert not got[:, 576:].any() and not torch.isnan(got).any()        # the padding columns: written, exactly 0
    # a band that starts and ends inside the image: the same rows of the whole
    band = run_patches(0, d, None, 64, 11, 13, 2, 3, 5, kpad)
    assert torch.equal(band.reshape(2, 5, 13, kpad), want.reshape(2, 11, 13, kpad)[:, 3:8])
    # the 2 x 2 floor max-pool on read: 11 x 13 -> 5 x 6 (the last row and column are dropped)
    pooled = F.max_pool2d(src.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    assert pooled.shape == (2, 5, 6, 64)
    wantp = R.patches(pooled, 0, 5, kpad)
    gotp = run_patches(1, d, None, 64, 11, 13, 2, 0, 5, kpad)
    assert torch.equal(gotp, wantp)
    bandp = run_patches(1, d, None, 64, 11, 13, 2, 1, 3, kpad)
    assert torch.equal(bandp.reshape(2, 3, 6, kpad), wantp.reshape(2, 5, 6, kpad)[:, 1:4])


def test_patches_first_layer_z_scores_with_a_true_division():
    g = torch.Generator().manual_seed(6)
    img = torch.rand(2, 3, 11, 13, generator=g)
    z = (img - torch.tensor(R.MEAN).view(1, 3, 1, 1)) / torch.tensor(R.STD).view(1, 3, 1, 1)   # fp32, IEEE division
    want = R.patches(z.permute(0, 2, 3, 1).contiguous(), 0, 11, 32)
    d0, d1 = img[0].contiguous().to(DEV), img[1].contiguous().to(DEV)
    got = run_patches(2, d0, d1, 3, 11, 13, 2, 0, 11, 32)
    assert torch.equal(got, want) and not got[:, 27:].any()
    band = run_patches(2, d0, d1, 3, 11, 13, 2, 4, 6, 32)
    assert torch.equal(band.reshape(2, 6, 13, 32), want.reshape(2, 11, 13, 32)[:, 4:10])
    wide = run_patches(2, d0, d1, 3, 11, 13, 2, 0, 11, 64)               # the bf16 mode's operand width
    assert torch.equal(wide[:, :32], want) and not wide[:, 27:].any()
    one = run_patches(2, d1, None, 3, 11, 13, 1, 0, 11, 32)
    assert torch.equal(one, want[11 * 13:])


# ---------------------------------------------------------------------------
# the head kernel alone
def run_head(fx, fy, lin):
    from copenerf import _lib
    P, C = fx.shape
    need = int(_lib.load().cn_lpips_head_workspace_bytes(P))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.full((1,), float("nan"), device=DEV)
    _lib.call("cn_lpips_head", C, P, fx.data_ptr(), fy.data_ptr(), lin.data_ptr(), out.data_ptr(), ws.data_ptr(), need,
              _stream())
    return out.cpu()


@pytest.mark.parametrize("C", [64, 512])
def test_head_against_float64(C):
    """9 x 13 = 117 pixels: two workgroups, the second ragged.  Bar from the formats (u = 2^-24): a unit vector
    carries ((C + 1) / 2 + 3) u (the norm's C adds halved by the root, the division), a squared difference
    that times kappa + 1 with kappa = sum lin (|fx^| + |fy^|)^2 / sum lin (fx^ - fy^)^2 the cancellation of
    the difference (computed from the data in float64), and the sums over channels, lanes, waves at most
    (C + 32) u."""
    g = torch.Generator().manual_seed(7 + C)
    fx, fy = torch.randn(117, C, generator=g).abs(), torch.randn(117, C, generator=g).abs()
    fx[5] = fy[5] = 0.0           # a pixel without activations in either image: 0 / (0 + 1e-10)
    lin = torch.rand(C, generator=g)
    nchw = lambda t: t.double().t().reshape(1, C, 9, 13)  # noqa: E731
    want = float(R.head(nchw(fx), nchw(fy), lin.double()))
    nx = fx.double() / (fx.double().pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    ny = fy.double() / (fy.double().pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    kappa = float(((nx + ny).pow(2) * lin.double()).sum() / ((nx - ny).pow(2) * lin.double()).sum())
    bar = (((C + 1) / 2 + 3) * (kappa + 1) + (C + 32)) * U
    dx, dy, dl = fx.to(DEV), fy.to(DEV), lin.to(DEV)
    got = run_head(dx, dy, dl)
    rel = abs(float(got) - want) / want
    print(f"head C={C}: value {want:.6e}, relative error {rel:.3e}, bar {bar:.3e} (kappa {kappa:.2f})")
    assert rel <= bar
    again = run_head(dx, dy, dl)
    assert got.view(torch.int32).equal(again.view(torch.int32))            # equal bits
    assert run_head(dx, dx.clone(), dl).view(torch.int32).item() == 0      # identical inputs: exactly +0


# ---------------------------------------------------------------------------
# end to end
def _check_layers(got, want, bars, what):
    rel = (got.double().cpu() - want).abs() / want
    bars = torch.as_tensor(bars, dtype=torch.float64).expand_as(rel)
    print(f"{what}: relative error per block {[f'{v:.2e}' for v in rel.max(0).values.tolist()]}, "
          f"bars {[f'{v:.2e}' for v in bars.min(0).values.tolist()]}")
    assert (rel <= bars).all(), (what, rel.tolist())


@pytest.mark.parametrize("mode", ["bf16x6", "fp32"])
@pytest.mark.parametrize("shape", [(3, 37, 53), (3, 16, 16)])
def test_layers_against_float64(shape, mode):
    a, b, want = case(shape)
    got = net(mode).layers(a.to(DEV), b.to(DEV))
    assert got.shape == (1, 5) and got.is_cuda
    _check_layers(got, want, BAR, f"{mode} {shape[1]} x {shape[2]}")


BF16_SHAPES = ((3, 37, 53), (3, 16, 16), (3, 3, 17, 31))


@functools.lru_cache(maxsize=None)
def bf16_measured():
    """The measured value of the bf16 bar: the largest per-block relative error, over the test's shapes and
    pairs, of the float64 restatement with both operands of every convolution rounded to bf16 (RNE) against
    the plain float64 restatement.  2.66e-2 (block 5 of the third pair at 17 x 31, a 1 x 1 tap); the bound is
    twice that, 5.33e-2.
    One value, not one per block and pair: past the second block the rounding error is chaotic -- a
    perturbation of 1e-7 (the accumulation's order or width) flips bf16 roundings of later operands, and the
    restatement accumulated in float64, the same in fp32 and the device give unrelated samples of the same
    spread per block (at 16 x 16, block 5: 1.7e-2, 9.6e-4 and 4.1e-2; blocks 1 and 2 agree to three digits).
    Twice one such sample is no bound on another (for two independent normal samples |x| > 2 |y| three times
    in ten), so the bar is taken from the spread: the largest sample."""
    convs, lins = ref_weights()
    worst = 0.0
    for shape in BF16_SHAPES:
        a, b, want = case(shape)
        rounded = R.lpips_layers(a, b, convs, lins, operand=lambda t: t.float().bfloat16().double())
        rel = (rounded - want).abs() / want
        print(f"bf16 restatement {shape}: {[f'{v:.2e}' for v in rel.max(0).values.tolist()]}")
        worst = max(worst, float(rel.max()))
    return worst


@pytest.mark.parametrize("shape", BF16_SHAPES)
def test_layers_bf16_within_twice_the_rounded_restatement(shape):
    a, b, want = case(shape)
    measured = bf16_measured()
    assert 2.6e-2 < measured < 2.7e-2          # the value recorded above
    got = net("bf16").layers(a.to(DEV), b.to(DEV))
    _check_layers(got, want, 2.0 * measured, f"bf16 {tuple(shape)}")


def test_value_is_the_sum_and_identical_images_give_zero():
    a, b, want = case((3, 37, 53))
    n = net()
    da, db = a.to(DEV), b.to(DEV)
    out = n._terms(da, db)
    assert out.shape == (1, 6)
    t = out[0, :5].cpu()
    assert out[0, 5].item() == ((((t[0] + t[1]) + t[2]) + t[3]) + t[4]).item()       # fp32, in block order
    assert torch.equal(n(da, db), out[:, 5]) and torch.equal(n.layers(da, db), out[:, :5])
    assert abs(float(n(da, db)) - float(want.sum())) <= BAR * float(want.sum())
    assert torch.equal(n._terms(da, da.clone()).cpu(), torch.zeros(1, 6))
    assert torch.equal(n._terms(da, db), out)                                         # reproducible


def test_band_rows_do_not_change_a_bit():
    a, b, _ = case((3, 37, 53))
    da, db = a.to(DEV), b.to(DEV)
    outs = [net("bf16x6", band)._terms(da, db).cpu().view(torch.int32) for band in (5, 1, 0)]
    assert outs[0].equal(outs[2]) and outs[1].equal(outs[2])


def test_batch_equals_single_calls():
    a, b, want = case((3, 3, 17, 31))
    n = net()
    da, db = a.to(DEV), b.to(DEV)
    got = n._terms(da, db)
    assert got.shape == (3, 6)
    _check_layers(got[:, :5], want, BAR, "batch of 3 at 17 x 31")
    for i in range(3):
        assert torch.equal(n._terms(da[i], db[i])[0], got[i])
    assert n(da, db).shape == (3,) and n.layers(da, db).shape == (3, 5)


def test_refusals_on_the_host():
    n = net()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        n(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))
    with pytest.raises(ValueError, match="at least 16"):
        n(torch.zeros(3, 15, 40, device=DEV), torch.zeros(3, 15, 40, device=DEV))
    with pytest.raises(RuntimeError, match="fp32"):
        n(torch.zeros(3, 16, 16, device=DEV, dtype=torch.float64), torch.zeros(3, 16, 16, device=DEV, dtype=torch.float64))


# ---------------------------------------------------------------------------
# the evaluator
def test_image_metrics_with_the_device_lpips():
    from copenerf import metrics
    a, b, want = case((3, 3, 17, 31))
    pred = [x.permute(1, 2, 0).contiguous().to(DEV) for x in a]
    gt = [x.permute(1, 2, 0).contiguous().to(DEV) for x in b]
    res = metrics.image_metrics(pred, gt, lpips_fn=net())
    assert list(res) == ["PSNR", "SSIM", "LPIPS"]
    mean = float(want.sum(1).mean())
    print(f"image_metrics LPIPS {res['LPIPS']:.8f}, float64 {mean:.8f}")
    assert abs(res["LPIPS"] - mean) <= BAR * mean
    assert list(metrics.image_metrics(pred, gt)) == ["PSNR", "SSIM"]


def test_evaluate_tool_writes_the_lpips_line(tmp_path):
    """tools/evaluate.py with the two weight files: results.txt has LPIPS in the reference's position (after
    SSIM), with the value metrics.evaluate gives for the same views; without the flags there is no such line and
    every other line is unchanged."""
    from copenerf import metrics
    from copenerf.rays import intrinsics_ndc
    from helpers import GOLDEN
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(GOLDEN.rstrip(os.sep))), "tools"))
    import evaluate as tool
    import extract_mesh
    ckpt = os.path.join(GOLDEN, "ref_checkpoint.pt")
    vgg, lin = R.state_dicts(*ref_weights())
    pv, pl = str(tmp_path / "vgg16.pth"), str(tmp_path / "vgg.pth")
    torch.save(vgg, pv)
    torch.save(lin, pl)
    h, w = 16, 20
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, h, w, generator=g)
    K = intrinsics_ndc(0.9 * w, 0.9 * w, w, h)
    world = torch.eye(4).repeat(2, 1, 1)
    world[1, 0, 3] = 0.03
    times = torch.tensor([-1.0, 1.0])
    files = {}
    for name, arr in (("images", images), ("K", K), ("world", world), ("times", times)):
        files[name] = str(tmp_path / f"{name}.npy")
        np.save(files[name], arr.numpy())
    args = [ckpt, "--images", files["images"], "--K", files["K"], "--world-mats", files["world"], "--times",
            files["times"], "--mode", "fp32", "--chunk", "64"]
    res = tool.main(args + ["--out", str(tmp_path / "with"), "--lpips-vgg", pv, "--lpips-lin", pl])
    assert list(res) == ["PSNR", "SSIM", "LPIPS"] and np.isfinite(res["LPIPS"]) and res["LPIPS"] > 0
    lines = (tmp_path / "with" / "results.txt").read_text().splitlines()
    assert lines == [f"{k}: {v}" for k, v in res.items()] and [l.split(":")[0] for l in lines] == ["PSNR", "SSIM", "LPIPS"]
    plain = tool.main(args + ["--out", str(tmp_path / "without")])
    text = (tmp_path / "without" / "results.txt").read_text()
    assert "LPIPS" not in text and text.splitlines() == [l for l in lines if not l.startswith("LPIPS")]
    assert list(plain) == ["PSNR", "SSIM"]
    with pytest.raises(SystemExit, match="go together"):
        tool.main(args + ["--out", str(tmp_path / "half"), "--lpips-vgg", pv])
    r = extract_mesh.build_renderer(ckpt).to(DEV).set_mfma_dtype("fp32")
    views = [dict(camera_mat=K.to(DEV), world_mat=world[i].to(DEV), time_step=times[i:i + 1],
                  image=images[i].permute(1, 2, 0).contiguous().to(DEV)) for i in range(2)]
    fn = metrics.LPIPS(metrics.load_lpips_weights(pv, pl), device=DEV)
    assert metrics.evaluate(r, views, lpips_fn=fn, chunk=64)["LPIPS"] == res["LPIPS"]
