"""The evaluation metrics on the device (cn_image_metrics, cn_depth_errors, copenerf.metrics, ABI v18) against
the float64 restatement (tests/metrics_ref.py) and the reference's numbers (tests/golden/metrics.npz).

Bars.  The reference's own fp32 formula is off from float64 by an amount that depends on the input (most where
sigma = E[x^2] - mu^2 cancels: smooth and flat images), so no absolute bar is fixed ahead: each case is allowed
4 x the error of the fp32 composition (the same expressions in fp32 torch ops -- numpy for the depth errors
-- on the same input) against float64, and never less than 4 fp32 ulp of the value.  The margin covers the
different summation order of a separable window."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_ref as M
from helpers import REN_CFG, build_modules, fixture_arrays

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = {"7x9": (7, 9), "37x53": (37, 53), "70x130": (70, 130)}  # all halo; ragged tiles; several tiles each way
CONTENTS = ("noise", "smooth", "flat", "black")


def make_images(content, N, C, H, W, seed=0):
    """(pred, gt) float64 [N, C, H, W] holding exactly representable fp32 values."""
    g = torch.Generator().manual_seed(seed + 1000 * N + 100 * C + H)
    r = lambda s=1.0: s * torch.rand(N, C, H, W, generator=g, dtype=torch.float64)  # noqa: E731
    n = lambda s: s * torch.randn(N, C, H, W, generator=g, dtype=torch.float64)  # noqa: E731
    if content == "noise":        # uniform noise against a noisy copy
        gt = r()
        pred = (gt + n(0.1)).clamp(0, 1)
    elif content == "smooth":     # a smooth image against a slightly noisy copy
        y = torch.linspace(0, 1, H, dtype=torch.float64).view(1, 1, H, 1)
        x = torch.linspace(0, 1, W, dtype=torch.float64).view(1, 1, 1, W)
        f = 1.0 + 2.0 * torch.rand(N, C, 1, 1, generator=g, dtype=torch.float64)
        gt = 0.5 + 0.4 * torch.sin(6.2831853 * f * (x + 0.7 * y))
        pred = gt + n(0.005)
    elif content == "flat":       # a flat image with small noise: sigma cancels
        gt = 0.7 + n(0.002)
        pred = 0.7 + n(0.002)
    else:                         # a black image against faint noise
        gt = torch.zeros(N, C, H, W, dtype=torch.float64)
        pred = r(0.02)
    return pred.float().double().numpy(), gt.float().double().numpy()


def composition_fp32(pred, gt):
    """The metric's expressions in fp32 torch ops on the device: ([N, C, 2], map) as float64 numpy."""
    x, y = pred.float(), gt.float()
    C = x.shape[1]
    taps = torch.from_numpy(M.window_taps()).to(x.device)
    win = (taps[:, None] * taps[None, :]).expand(C, 1, 11, 11).contiguous()
    blur = lambda t: F.conv2d(t, win, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    m = ((2 * mu1 * mu2 + M.C1) * (2 * s12 + M.C2)) / ((mu1 * mu1 + mu2 * mu2 + M.C1) * (s1 + s2 + M.C2))
    out = torch.stack([((x - y) ** 2).mean((2, 3)), m.mean((2, 3))], -1)
    return out.double().cpu().numpy(), m.double().cpu().numpy()


def ulp4(v):
    return 4.0 * np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def bar(comp, ref):
    """Elementwise bar: 4 x the composition's worst error in this case, at least 4 fp32 ulp of the value."""
    e = float(np.abs(comp - ref).max())
    return np.maximum(4.0 * e, ulp4(ref)), e


@functools.lru_cache(maxsize=None)
def case(content, size, N, C):
    H, W = SIZES[size]
    pred, gt = make_images(content, N, C, H, W)
    ref_out, ref_map = M.image_metrics(pred, gt)
    dp, dg = torch.from_numpy(pred).float().to(DEV), torch.from_numpy(gt).float().to(DEV)
    comp_out, comp_map = composition_fp32(dp, dg)
    return dict(pred=dp, gt=dg, ref_out=ref_out, ref_map=ref_map, comp_out=comp_out, comp_map=comp_map)


@pytest.mark.parametrize("N,C", [(1, 1), (1, 3), (4, 1), (4, 3)])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("content", CONTENTS)
def test_image_metrics_within_the_fp32_formulas_error(content, size, N, C):
    from copenerf import ops
    c = case(content, size, N, C)
    out, smap = ops.image_metrics(c["pred"], c["gt"], want_map=True)
    out, smap = out.double().cpu().numpy(), smap.double().cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(smap).all()
    report = {}
    for name, got, comp, ref in (("map", smap, c["comp_map"], c["ref_map"]),
                                 ("ssim", out[..., 1], c["comp_out"][..., 1], c["ref_out"][..., 1]),
                                 ("mse", out[..., 0], c["comp_out"][..., 0], c["ref_out"][..., 0])):
        b, e = bar(comp, ref)
        err = np.abs(got - ref)
        report[name] = (float(err.max()), e, float((err / b).max()))
    print(f"{content} {size} N={N} C={C}: (error, composition's error, error / bar) {report}")
    for name, (err, e, frac) in report.items():
        assert frac <= 1.0, (name, err, e, frac)


@pytest.mark.parametrize("size", list(SIZES))
def test_identical_images(size):
    from copenerf import metrics, ops
    H, W = SIZES[size]
    pred, _ = make_images("noise", 2, 3, H, W, seed=5)
    x = torch.from_numpy(pred).float().to(DEV)
    x[1] = 0.0  # a black image too
    out, smap = ops.image_metrics(x, x.clone(), want_map=True)
    assert torch.equal(smap, torch.ones_like(smap))
    assert torch.equal(out[..., 1], torch.ones(2, 3, device=DEV)) and torch.equal(out[..., 0], torch.zeros(2, 3, device=DEV))
    assert torch.isinf(metrics.psnr(x, x.clone())).all() and (metrics.psnr(x, x.clone()) > 0).all()
    assert torch.isinf(metrics.psnr(x[0], x[0].clone())).all()
    assert float(metrics.ssim(x, x.clone())) == 1.0


def test_bitwise_properties():
    from copenerf import ops
    c = case("noise", "70x130", 4, 3)
    a, amap = ops.image_metrics(c["pred"], c["gt"], want_map=True)
    b, bmap = ops.image_metrics(c["pred"], c["gt"], want_map=True)
    assert torch.equal(a, b) and torch.equal(amap, bmap)          # two runs
    nomap, none = ops.image_metrics(c["pred"], c["gt"])
    assert none is None and torch.equal(nomap, a)                 # the means with and without the map
    for n in range(4):                                            # image n alone
        one, onemap = ops.image_metrics(c["pred"][n:n + 1].contiguous(), c["gt"][n:n + 1].contiguous(), want_map=True)
        assert torch.equal(one[0], a[n]) and torch.equal(onemap[0], amap[n])
    ch, _ = ops.image_metrics(c["pred"][:, 1:2].contiguous(), c["gt"][:, 1:2].contiguous())  # one channel alone
    assert torch.equal(ch[:, 0], a[:, 1])


def test_planes_past_two_to_the_31_elements_of_the_stack():
    """Plane base offsets are 64-bit: the last image of a stack of 2050 planes of 1024 x 1024 starts 2049 * 2^20
    elements (8.6 GB) in.  Only the first and last images hold data; the rest are zeros (SSIM 1, error 0)."""
    from copenerf import ops
    H = W = 1024
    N = 2050
    assert (N - 1) * H * W > 2 ** 31
    if torch.cuda.mem_get_info()[0] < 3 * N * H * W * 4 + (1 << 30):
        pytest.skip("three stacks of 8.6 GB each (pred, gt, the map) do not fit on this device")
    try:
        pred, gt = torch.zeros(N, 1, H, W, device=DEV), torch.zeros(N, 1, H, W, device=DEV)
    except torch.OutOfMemoryError:
        pytest.skip("two stacks of 8.6 GB each could not be allocated on this device")
    g = torch.Generator().manual_seed(9)
    small_p, small_g = torch.rand(2, 1, H, W, generator=g).to(DEV), torch.rand(2, 1, H, W, generator=g).to(DEV)
    want, want_map = ops.image_metrics(small_p, small_g, want_map=True)
    for t, s in ((pred, small_p), (gt, small_g)):
        t[0], t[N - 1] = s[0], s[1]
    got, got_map = ops.image_metrics(pred, gt, want_map=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[N - 1], want[1])
    assert torch.equal(got[1:N - 1, 0, 0], torch.zeros(N - 2, device=DEV))
    assert torch.equal(got[1:N - 1, 0, 1], torch.ones(N - 2, device=DEV))
    assert torch.equal(got_map[0], want_map[0]) and torch.equal(got_map[N - 1], want_map[1])


def test_metrics_functions_on_the_fixture():
    from copenerf import metrics
    fx = fixture_arrays("metrics")
    for tag in ("a", "b"):
        p64, g64 = fx[f"img_{tag}_pred"], fx[f"img_{tag}_gt"]
        pred, gt = torch.from_numpy(p64).float().to(DEV), torch.from_numpy(g64).float().to(DEV)
        # the inputs are cast to fp32, which alone moves the float64 values; the bars are taken for the cast inputs
        ref_out, ref_map = M.image_metrics(pred.double().cpu().numpy(), gt.double().cpu().numpy())
        comp_out, _ = composition_fp32(pred, gt)
        cast = np.abs(ref_map.mean(axis=(1, 2, 3)) - fx[f"img_{tag}_ssim_per_image"]).max()
        ref_psnr = M.psnr_of_mse(ref_out[..., 0].mean(1))
        cast_p = max(np.abs(ref_psnr - fx[f"img_{tag}_psnr"][:, 0]).max(),
                     np.abs(M.psnr_of_mse(ref_out[..., 0]) - fx[f"img_{tag}_psnr_unbatched"][..., 0]).max())
        assert cast < 1e-6 and cast_p < 1e-5
        e_ssim = np.abs(comp_out[..., 1] - ref_out[..., 1]).max()
        e_mse = np.abs(comp_out[..., 0] - ref_out[..., 0]).max()
        rel_mse = 4 * max(e_mse / ref_out[..., 0].min(), 2.0 ** -23)  # the bar on the mse, relative
        # d psnr = 10 / ln 10 * d mse / mse, and 4 ulp of a PSNR below 32 for the fp32 sqrt, division and log10
        db = 10 / np.log(10) * rel_mse + 4 * 2.0 ** -23 * 32
        sb = max(4 * e_ssim, 4 * 2.0 ** -23)
        N = pred.shape[0]
        s = metrics.ssim(pred, gt)
        assert s.dim() == 0 and abs(float(s) - ref_map.mean()) <= sb and abs(float(s) - fx[f"img_{tag}_ssim"]) <= sb + cast
        s = metrics.ssim(pred, gt, size_average=False)
        assert s.shape == (N,) and np.abs(s.double().cpu().numpy() - fx[f"img_{tag}_ssim_per_image"]).max() <= sb + cast
        q = metrics.psnr(pred, gt)
        assert q.shape == (N, 1)
        assert np.abs(q[:, 0].double().cpu().numpy() - ref_psnr).max() <= db
        assert np.abs(q.double().cpu().numpy() - fx[f"img_{tag}_psnr"]).max() <= db + cast_p
        for n in range(N):  # unbatched, as eval.py:204-205 calls them: per-channel PSNRs, a scalar SSIM
            q = metrics.psnr(pred[n], gt[n])
            assert q.shape == (3, 1)
            assert np.abs(q.double().cpu().numpy() - fx[f"img_{tag}_psnr_unbatched"][n]).max() <= db + cast_p
            s = metrics.ssim(pred[n], gt[n])
            assert s.dim() == 0 and abs(float(s) - fx[f"img_{tag}_ssim_unbatched"][n]) <= sb + cast
            with pytest.raises(IndexError):
                metrics.ssim(pred[n], gt[n], size_average=False)
        res = metrics.image_metrics(list(pred.permute(0, 2, 3, 1)), list(gt.permute(0, 2, 3, 1)))
        assert list(res) == ["PSNR", "SSIM"]
        assert abs(res["PSNR"] - fx[f"img_{tag}_psnr_unbatched"].mean()) <= db + cast_p  # the mean of per-channel PSNRs
        assert abs(res["SSIM"] - fx[f"img_{tag}_ssim_unbatched"].mean()) <= sb + cast
        res2 = metrics.image_metrics(pred.permute(0, 2, 3, 1), gt.permute(0, 2, 3, 1), lpips_fn=lambda a, b: (a - b).abs().mean())
        assert list(res2) == ["PSNR", "SSIM", "LPIPS"] and res2["PSNR"] == res["PSNR"] and res2["SSIM"] == res["SSIM"]
        assert abs(res2["LPIPS"] - np.abs(pred.double().cpu().numpy() - gt.double().cpu().numpy()).mean()) < 1e-6


# ---------------------------------------------------------------------------
# depth
# per size, three seeds at which no valid pixel's max(gt / pred, pred / gt) lies within 1e-4 of 1.25, 1.25^2 or
# 1.25^3 (searched on the CPU with margin 2e-4, for both prediction sizes and both clamp settings; asserted in
# the test): there a1, a2 and a3 are the same in fp32 and in float64
DEPTH_SEEDS = {(12, 16): (0, 1, 2), (46, 50): (17, 20, 47)}
# test_depth_functions_on_the_fixture only, where the fp32 inputs are themselves casts of the float64 values the
# fixture's numbers belong to and the float64 side took its own median ratio: every per-pixel term carries a handful of fp32 roundings (the cast inputs, the ratio, the
# difference, the logarithms: at most about 4 ulp of a logarithm below 4.4, 1e-6, on log differences whose RMS is
# about 0.3), so 1e-5 of the value
DEPTH_RTOL = 1e-5


def depth_inputs(Hg, Wg, half, seed):
    """gt fp32 [Hg, Wg] with zeros and out-of-range values; pred at the same or at exactly half the size."""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 30.0, (Hg, Wg))
    gt[rng.uniform(size=gt.shape) < 0.15] = 0.0
    gt[rng.uniform(size=gt.shape) < 0.05] = 120.0
    gt[rng.uniform(size=gt.shape) < 0.03] = 0.05
    Hp, Wp = (Hg // 2, Wg // 2) if half else (Hg, Wg)
    base = gt[::2, ::2][:Hp, :Wp] if half else gt
    pred = np.where((base > 0.1) & (base < 80), base, 7.0) / 3.0 * np.exp(0.3 * rng.standard_normal((Hp, Wp)))
    pred.reshape(-1)[rng.permutation(pred.size)[:6]] = [1e-3, 2e-3, 5e-3, 200.0, 400.0, 900.0]  # these clamp
    return gt.astype(np.float32), pred.astype(np.float32)


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("Hg,Wg", list(DEPTH_SEEDS))  # one workgroup; two, the second one ragged
def test_depth_errors(Hg, Wg, half, clamp):
    from copenerf import metrics, ops
    maps = [depth_inputs(Hg, Wg, half, seed) for seed in DEPTH_SEEDS[Hg, Wg]]
    gt = torch.from_numpy(np.stack([m[0] for m in maps])).to(DEV)
    pred = torch.from_numpy(np.stack([m[1] for m in maps])).to(DEV)
    ratio = metrics.median_ratio(gt, pred, 0.1, 80.0)
    out = ops.depth_errors(gt, pred, ratio, 0.1, 80.0, clamp).double().cpu().numpy()
    again = ops.depth_errors(gt, pred, ratio, 0.1, 80.0, clamp).double().cpu().numpy()
    assert np.array_equal(out, again)
    alone = ops.depth_errors(gt[1:2].contiguous(), pred[1:2].contiguous(), ratio[1:2].contiguous(), 0.1, 80.0, clamp)
    assert np.array_equal(alone.double().cpu().numpy()[0], out[1])
    for n, (g, p) in enumerate(maps):
        g64, p64 = g.astype(np.float64), p.astype(np.float64)
        valid = (g >= np.float32(0.1)) & (g <= np.float32(80.0))
        r32 = np.median(g[valid]) / np.median(M.nearest(p, Hg, Wg)[valid])     # fp32, np.median's rule
        assert float(ratio[n]) == r32
        # both sides take the fp32 ratio and the fp32 thresholds as given: the bars are about the seven errors
        ref = M.depth_errors(g64, p64, np.float32(0.1), np.float32(80.0), clamp, ratio=np.float64(r32))
        comp = M.depth_errors(g, p, 0.1, 80.0, clamp, ratio=r32, dtype=np.float32)
        assert out[n, 7] == ref[7] == valid.sum() and 0 < ref[7] < Hg * Wg      # the count: exact
        # a1, a2, a3 are exact provided no pixel sits at a threshold (checked here in float64)
        for k in range(3):
            assert np.abs(ref[8] - 1.25 ** (k + 1)).min() > 1e-4
            assert out[n, 4 + k] == np.float32(ref[4 + k]), (n, k)
        for k, name in enumerate(metrics.DEPTH_KEYS[:4]):
            e = abs(float(comp[k]) - ref[k])
            b = max(4 * e, float(ulp4(np.array(ref[k]))))
            print(f"{Hg}x{Wg} half={half} clamp={clamp} image {n} {name}: error {abs(out[n, k] - ref[k]):.3e}, "
                  f"composition's {e:.3e}, bar {b:.3e}")
            assert abs(out[n, k] - ref[k]) <= b, (n, name, out[n, k], ref[k], e)
        if clamp:
            assert M.depth_errors(g64, p64, 0.1, 80.0, False, ratio=np.float64(r32))[2] != ref[2]  # the clamp acts


def test_depth_errors_without_a_valid_pixel():
    from copenerf import metrics, ops
    gt = torch.zeros(2, 12, 16, device=DEV)
    gt[1] = 5.0
    gt[1, 0, 0] = float("nan")  # never valid
    pred = torch.full((2, 12, 16), 2.0, device=DEV)
    out = ops.depth_errors(gt, pred, torch.ones(2, device=DEV), 0.1, 80.0, True).cpu()
    assert torch.isnan(out[0, :7]).all() and out[0, 7] == 0
    assert out[1, 7] == 12 * 16 - 1 and abs(float(out[1, 0]) - 0.6) < 1e-6 and out[1, 4] == 0 and out[1, 6] == 0
    assert metrics.depth_metrics([-1, -1], [pred[0], pred[1]]) is None
    d = metrics.depth_metrics([gt[1]], [pred[1]])
    assert list(d) == list(metrics.DEPTH_KEYS) and d["abs_rel"] == 0.0 and d["a1"] == 1.0  # the median ratio is 2.5


def test_depth_functions_on_the_fixture():
    from copenerf import metrics
    from copenerf.trainer import Trainer
    fx = fixture_arrays("metrics")
    g, p = fx["depth_gt"].astype(np.float32), fx["depth_pred"].astype(np.float32)
    d = metrics.depth_metrics([torch.from_numpy(g).to(DEV)], [p], clamp=True)  # numpy maps are uploaded
    got = np.array([d[k] for k in metrics.DEPTH_KEYS])
    assert np.abs(got - fx["depth_errors_clamp"]).max() <= DEPTH_RTOL * np.abs(fx["depth_errors_clamp"]).max()
    e = metrics.compute_depth_errors(g, p)
    assert len(e) == 7 and np.abs(np.array(e) - fx["depth_errors_noclamp"]).max() <= DEPTH_RTOL * np.abs(fx["depth_errors_noclamp"]).max()
    assert Trainer.compute_depth_errors(None, g, torch.from_numpy(p).to(DEV)) == e


# ---------------------------------------------------------------------------
# end to end
# the seed of the ground-truth images and depths: the first at which, against the two rendered 16 x 24 depth maps,
# no valid pixel's max(gt / pred, pred / gt) lies within 2e-4 of 1.25, 1.25^2 or 1.25^3 (searched on the CPU on the
# rendered maps; the test asserts a margin of 1e-4)
E2E_SEED = 4


def test_evaluate_end_to_end(tmp_path):
    from copenerf import NeuSRenderer, evaluate, metrics
    from copenerf.inference import render_image
    from copenerf.rays import intrinsics_ndc
    h, w = 16, 24
    sdf, col, dev = build_modules(7, dh_sdf=64, dh_col=64, device=DEV)
    r = NeuSRenderer(None, sdf, dev, col, None, **REN_CFG).to(DEV)
    K = intrinsics_ndc(0.9 * w, 0.9 * w, w, h, device=DEV)
    I = torch.eye(4, device=DEV)
    g = torch.Generator().manual_seed(E2E_SEED)
    views, gt_depths = [], []
    for k in range(2):
        world = I.clone()
        world[0, 3] = 0.05 * k
        views.append(dict(camera_mat=K, world_mat=world, time_step=torch.tensor([0.1 * k]),
                          image=torch.rand(h, w, 3, generator=g).to(DEV)))
        gt_depths.append(torch.rand(h, w, generator=g).to(DEV) * 3.0 + 0.05)
    gt_poses = M.trajectory(6, 2)
    pred_poses = M.apply_sim3(gt_poses, 0.5, M.rodrigues([0.1, 0.2, 0.3]), np.array([1.0, 2.0, 3.0]))
    pred_poses[:, :3, 3] += 0.01 * np.random.default_rng(0).standard_normal((6, 3))
    stub = lambda a, b: (a - b).abs().mean()  # noqa: E731
    res = evaluate(r, views, gt_poses=torch.from_numpy(gt_poses), pred_poses=torch.from_numpy(pred_poses).to(DEV),
                   gt_depths=gt_depths, lpips_fn=stub, chunk=256)
    assert list(res) == ["PSNR", "SSIM", "LPIPS", "rpe_trans", "rpe_rot", "ate"] + list(metrics.DEPTH_KEYS)
    plain = evaluate(r, views, chunk=256)
    assert list(plain) == ["PSNR", "SSIM"] and plain["PSNR"] == res["PSNR"] and plain["SSIM"] == res["SSIM"]
    nodepth = evaluate(r, views, gt_depths=[-1, -1], chunk=256)
    assert list(nodepth) == ["PSNR", "SSIM"]
    # the restatement on the same rendered maps (rendering is deterministic and chunk-invariant)
    with torch.no_grad():
        outs = [render_image(r, K, v["world_mat"], I, (h, w), v["time_step"], chunk=256) for v in views]
    rgb = [o["rgb"] for o in outs]
    want = M.eval_image_metrics([x.double().cpu().numpy() for x in rgb], [v["image"].double().cpu().numpy() for v in views])
    pstack = torch.stack(rgb).permute(0, 3, 1, 2).contiguous()
    gstack = torch.stack([v["image"] for v in views]).permute(0, 3, 1, 2).contiguous()
    comp_out, _ = composition_fp32(pstack, gstack)
    ref_out, _ = M.image_metrics(pstack.double().cpu().numpy(), gstack.double().cpu().numpy())
    sb = max(4 * np.abs(comp_out[..., 1] - ref_out[..., 1]).max(), 4 * 2.0 ** -23)
    rel = 4 * max((np.abs(comp_out[..., 0] - ref_out[..., 0]) / ref_out[..., 0]).max(), 2.0 ** -23)
    assert abs(res["SSIM"] - want["SSIM"]) <= sb
    assert abs(res["PSNR"] - want["PSNR"]) <= 10 / np.log(10) * rel + 4 * 2.0 ** -23 * abs(want["PSNR"])
    assert abs(res["LPIPS"] - np.mean([(a - v["image"]).abs().mean().item() for a, v in zip(rgb, views)])) < 1e-6
    _, rt, rr, ate = M.pose_error(pred_poses, gt_poses)
    assert abs(res["rpe_trans"] - rt) < 1e-9 and abs(res["rpe_rot"] - rr) < 1e-9 and abs(res["ate"] - ate) < 1e-9
    # depth: both sides see the same fp32 maps and the fp32 ratio, so test_depth_errors' rule holds unchanged --
    # per view 4 x the fp32 numpy composition's error against float64, at least 4 fp32 ulp, averaged over the views
    # as the errors are; a1, a2, a3 exact, no pixel of either view sitting at a threshold (E2E_SEED is chosen so)
    rows, bars = [], []
    for o, gd in zip(outs, gt_depths):
        g32, p32 = gd.cpu().numpy(), o["depth"].cpu().numpy()
        valid = (g32 >= np.float32(0.1)) & (g32 <= np.float32(80.0))
        r32 = np.median(g32[valid]) / np.median(p32[valid])
        ref = M.depth_errors(g32.astype(np.float64), p32.astype(np.float64), np.float32(0.1), np.float32(80.0), True,
                             ratio=np.float64(r32))
        comp = M.depth_errors(g32, p32, 0.1, 80.0, True, ratio=r32, dtype=np.float32)
        assert 0 < ref[7] < h * w
        for k in range(3):
            assert np.abs(ref[8] - 1.25 ** (k + 1)).min() > 1e-4
        rows.append(ref[:7])
        bars.append([max(4 * abs(float(comp[k]) - ref[k]), float(ulp4(np.array(ref[k])))) for k in range(4)])
    wantd, bard = np.mean(np.array(rows, dtype=np.float64), 0), np.mean(np.array(bars), 0)
    for k, name in enumerate(metrics.DEPTH_KEYS[:4]):
        print(f"end to end {name}: error {abs(res[name] - wantd[k]):.3e}, bar {bard[k]:.3e}")
        assert abs(res[name] - wantd[k]) <= bard[k], (name, res[name], wantd[k], bard[k])
    for k, name in enumerate(metrics.DEPTH_KEYS[4:], 4):  # the kernel's fp32 fractions, averaged in float64
        assert res[name] == np.mean([np.float64(np.float32(row[k])) for row in rows]), (name, res[name])
    # results.txt round-trips
    path = tmp_path / "results.txt"
    metrics.write_results(path, res)
    back = {l.split(": ")[0]: float(l.split(": ")[1]) for l in path.read_text().splitlines()}
    assert list(back) == list(res) and all(back[k] == float(res[k]) for k in res)


def test_evaluate_tool_writes_results_txt(tmp_path):
    """tools/evaluate.py from the reference's checkpoint and arrays on disk to results.txt: the numbers are
    those of metrics.evaluate on the same views, in the reference's order."""
    import os
    import sys
    from copenerf import metrics
    from copenerf.rays import intrinsics_ndc
    from helpers import GOLDEN
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(GOLDEN.rstrip(os.sep))), "tools"))
    import evaluate as tool
    import extract_mesh
    ckpt = os.path.join(GOLDEN, "ref_checkpoint.pt")
    h, w = 8, 12
    g = torch.Generator().manual_seed(1)
    images = torch.rand(2, 3, h, w, generator=g)
    depths = torch.rand(2, h // 2, w // 2, generator=g) * 3 + 0.2
    K = intrinsics_ndc(0.9 * w, 0.9 * w, w, h)
    world = torch.eye(4).repeat(2, 1, 1)
    world[1, 0, 3] = 0.03
    times = torch.tensor([-1.0, 1.0])
    gt_poses = M.trajectory(5, 4)
    pred_poses = M.apply_sim3(gt_poses, 2.0, M.rodrigues([0.3, 0.1, -0.2]), np.array([0.5, 0.0, -1.0]))
    files = {}
    for name, arr in (("images", images), ("K", K), ("world", world), ("times", times), ("depths", depths),
                      ("gt", torch.from_numpy(gt_poses)), ("pred", torch.from_numpy(pred_poses))):
        files[name] = str(tmp_path / f"{name}.npy")
        np.save(files[name], arr.numpy())
    res = tool.main([ckpt, "--images", files["images"], "--K", files["K"], "--world-mats", files["world"], "--times",
                     files["times"], "--depths", files["depths"], "--gt-poses", files["gt"], "--pred-poses",
                     files["pred"], "--out", str(tmp_path / "out"), "--mode", "fp32", "--chunk", "64"])
    assert list(res) == ["PSNR", "SSIM", "rpe_trans", "rpe_rot", "ate"] + list(metrics.DEPTH_KEYS)
    assert res["ate"] < 1e-5 and np.isfinite(res["PSNR"]) and 0 < res["SSIM"] < 1  # float32 arrays on disk
    lines = (tmp_path / "out" / "results.txt").read_text().splitlines()
    assert lines == [f"{k}: {v}" for k, v in res.items()]
    r = extract_mesh.build_renderer(ckpt).to(DEV).set_mfma_dtype("fp32")
    views = [dict(camera_mat=K.to(DEV), world_mat=world[i].to(DEV), time_step=times[i:i + 1],
                  image=images[i].permute(1, 2, 0).contiguous().to(DEV)) for i in range(2)]
    want = metrics.evaluate(r, views, gt_depths=list(depths.to(DEV)), chunk=64)
    assert np.array_equal([res[k] for k in want], list(want.values()), equal_nan=True)
