"""The fused flow-RGB pass (cn_flow_rgb_fwd / cn_flow_rgb_bwd, motion.flow_rgb_fused, ABI v21) against
motion.project_flow_sums + motion.flow_rgb_loss in float64 on the CPU (pure torch, pinned to the reference by
tests/test_stage1_golden.py), with the same two functions in fp32 on the device as the composition arm.

Cases (H, W, R, T, N): 5 x 7 with 3 rays and one frame (fewer rays than a wavefront), 37 x 53 with 200 rays and
three frames, 70 x 130 with 1000 rays (a ragged last workgroup), frames [1, 4, 4] and the third one masked; and an
empty batch.  Recipe (seeded): pixels from the whole image, K = intrinsics_ndc(0.9 W, 0.9 W, W, H), depth in
[1, 3], p = d (pixn_x / K00, pixn_y / K11, -1), wbar in [0.6, 1], pbar = wbar p, w2c[j] = [Exp(0.03 (j+1) randn) |
0.12 (j+1) randn], random frames and targets.  Rays whose float64 correspondence, in any frame, lies within 1e-3 px
of an integer coordinate (a pixel grid line; the mask's edges 0, W, H are among them) are removed before either
arm runs: a last-ulp move across a grid line flips the bilinear derivative, at the mask's edge the count.

Bars: error against float64 at most max(4 x the composition's error, 4e-6 x the tensor's scale), the rule and
floor of tests/test_gpu_pose_refine.py; the valid counts are exact.

Measured on an MI355X, error against float64 relative to scale, fused pass / fp32 torch composition:
  5x7     3 rays kept of 3, outside 0.333:     num 3.3e-8 / 1.4e-7, d_ray_acc 1.2e-7 / 2.1e-7, d_w2c 1.7e-7 / 2.7e-7
  37x53   195 rays kept of 200, outside 0.214: num 1.6e-7 / 1.7e-7, d_ray_acc 1.5e-6 / 3.5e-6, d_w2c 3.1e-6 / 4.5e-6
  70x130  994 rays kept of 1000, outside 0.250: num 1.2e-7 / 1.4e-7, d_ray_acc 5.5e-6 / 5.7e-6, d_w2c 7.0e-6 / 5.5e-6
  per-frame loss of flow_rgb_fused: 3.3e-8 / 1.4e-7, 2.1e-7 / 2.1e-7, 1.4e-7 / 1.4e-7
(the gradients of both arms carry the correspondence's rounding times the random frames' second differences; the
valid counts were equal to the float64 counts in every case).
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

# name: (H, W, R, T, N, seed, frame, frame_valid)
CASES = {"5x7": (5, 7, 3, 1, 2, 0, None, None),
         "37x53": (37, 53, 200, 3, 5, 0, None, None),
         "70x130": (70, 130, 1000, 3, 5, 1, (1, 4, 4), (1, 1, 0))}
MARGIN = 1e-3
FLOOR = 4e-6


def _so3_exp(v):
    K = torch.zeros(3, 3, dtype=torch.float64)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -v[2], v[1], v[2], -v[0], -v[1], v[0]
    return torch.matrix_exp(K)


def _corr64(c, ray_acc):
    """The float64 correspondences [T, R, 2] of the recipe's rays."""
    from copenerf import motion
    flows = motion.project_flow_sums(ray_acc[:, :3], ray_acc[:, 3:], c.w2c, c.cams, c.I, c.pixn, (c.H, c.W))
    return c.pix[None] + flows


@functools.lru_cache(None)
def _case(name):
    """The recipe (fp32-representable values held in float64) after the conditioning, with its float64
    reference: num, count, per-frame loss, d_ray_acc and d_w2c under a random g_num.  Shared, never modified.
    (The seeds are among 0 and 1 such that the conditions asserted first hold; with 3 rays and one frame the
    outside share can only be 1 / 3.)"""
    from copenerf.rays import intrinsics_ndc, pixels_from_indices
    H, W, R, T, N, seed, frame, fvalid = CASES[name]
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    rndn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    f32 = lambda x: x.float().double()  # noqa: E731  (every input is an fp32 value: both arms see the same numbers)
    c = types.SimpleNamespace(H=H, W=W, T=T, N=N, name=name)
    idx = torch.randint(0, H * W, (R,), generator=g)
    pix, pixn = pixels_from_indices(idx, H, W)
    K = intrinsics_ndc(0.9 * W, 0.9 * W, W, H).double()
    d = 1.0 + 2.0 * rnd(R, 1)
    p = d * torch.cat([pixn[:, :1].double() / K[0, 0], pixn[:, 1:].double() / K[1, 1], -torch.ones(R, 1, dtype=torch.float64)], 1)
    wbar = 0.6 + 0.4 * rnd(R, 1)
    ray_acc = f32(torch.cat([wbar * p, wbar], 1))
    w2c = torch.eye(4, dtype=torch.float64).repeat(T, 1, 1)
    for j in range(T):
        w2c[j, :3, :3] = _so3_exp(0.03 * (j + 1) * rndn(3))
        w2c[j, :3, 3] = 0.12 * (j + 1) * rndn(3)
    c.w2c, c.cams, c.I = f32(w2c), K.expand(T, 4, 4).contiguous(), torch.eye(4, dtype=torch.float64)
    c.images, gt = f32(rnd(N, 3, H, W)), f32(rnd(R, 3))
    c.frame = torch.tensor(frame if frame is not None else list(range(1, T + 1)), dtype=torch.int64)
    c.fvalid = torch.tensor(fvalid if fvalid is not None else [1] * T, dtype=torch.bool)
    c.g_num = f32(0.5 + rnd(T))
    c.pix, c.pixn = pix.double(), pixn.double()
    # conditioning: no correspondence within MARGIN of an integer coordinate, in any frame
    corr = _corr64(c, ray_acc)
    near = ((corr - corr.round()).abs() < MARGIN).any(-1).any(0)
    keep = ~near
    c.removed = float(near.float().mean())
    c.ray_acc, c.pix, c.pixn, c.gt = ray_acc[keep], c.pix[keep], c.pixn[keep], gt[keep]
    c.R = int(keep.sum())
    corr = corr[:, keep]
    inside = (corr[..., 0] >= 0) & (corr[..., 0] < W) & (corr[..., 1] >= 0) & (corr[..., 1] < H)
    c.outside = 1.0 - float(inside.double().mean())
    c.ref = _torch_arm(c, torch.float64, "cpu")
    assert torch.equal(c.ref.count, (inside & c.fvalid[:, None]).sum(1).double())
    return c


def _torch_arm(c, dtype, dev):
    """project_flow_sums + flow_rgb_loss over images.index_select(0, frame): num, count, per, d_ray_acc, d_w2c
    (gradients of sum_t g_num[t] num[t], masked frames dropped), as float64 CPU tensors."""
    from copenerf import motion
    to = lambda x: x.to(dev, dtype)  # noqa: E731
    ra, w2c = to(c.ray_acc).clone().requires_grad_(True), to(c.w2c).clone().requires_grad_(True)  # (the case's stay as they are)
    flows = motion.project_flow_sums(ra[:, :3], ra[:, 3:], w2c, to(c.cams), to(c.I), to(c.pixn), (c.H, c.W))
    per = motion.flow_rgb_loss(flows, to(c.pix), to(c.images).index_select(0, c.frame.to(dev)), to(c.gt))
    with torch.no_grad():
        corr = to(c.pix)[None] + flows
        count = ((corr[..., 0] >= 0) & (corr[..., 0] < c.W) & (corr[..., 1] >= 0) & (corr[..., 1] < c.H)).sum(1)
    fv = c.fvalid.to(dev)
    count = torch.where(fv, count, torch.zeros_like(count)).double()
    per = torch.where(fv, per, torch.zeros_like(per))
    (per * ((count + 1e-10) * to(c.g_num).double()).to(dtype)).sum().backward()
    cpu = lambda x: x.detach().double().cpu()  # noqa: E731
    per = cpu(per)
    return types.SimpleNamespace(num=per * (count.cpu() + 1e-10), count=count.cpu(), per=per, d_ray=cpu(ra.grad),
                                 d_w2c=cpu(w2c.grad)[:, :3, :])


def _fused(c, images=None, frame=None, fvalid="case", rays=slice(None), frames=slice(None)):
    """_FlowRgbTerms on the device: num, count, d_ray_acc, d_w2c[:, :3] (device tensors)."""
    from copenerf import motion
    cu = lambda x: x.to("cuda", torch.float32).contiguous()  # noqa: E731
    ra, w2c = cu(c.ray_acc[rays]).requires_grad_(True), cu(c.w2c[frames]).requires_grad_(True)
    KS = cu((c.I[:3, :3] @ c.cams[:, :3, :3])[frames])
    fv = c.fvalid if isinstance(fvalid, str) else fvalid
    fv = None if fv is None else fv[frames].cuda().view(torch.uint8)
    frame = (c.frame if frame is None else frame)[frames].cuda()
    num, count = motion._FlowRgbTerms.apply(ra, w2c, KS, cu(c.pixn[rays]), cu(c.pix[rays]), cu(c.gt[rays]),
                                            cu(c.images) if images is None else images, frame, fv)
    (num * cu(c.g_num[frames])).sum().backward()
    return types.SimpleNamespace(num=num.detach(), count=count.detach(), d_ray=ra.grad, d_w2c=w2c.grad[:, :3, :],
                                 row3=w2c.grad[:, 3, :])


def _err(got, want):
    return float((got.detach().double().cpu() - want).abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_sums_counts_and_gradients_against_float64(name):
    c = _case(name)
    print(f"{name}: {c.R} rays kept, {c.removed:.4f} removed, outside the mask {c.outside:.3f}")
    assert c.removed <= 0.05
    assert 0.02 <= c.outside <= 0.6
    f, comp = _fused(c), _torch_arm(c, torch.float32, "cuda")
    assert torch.equal(f.count.double().cpu(), c.ref.count), (f.count, c.ref.count)
    assert not f.row3.any()
    for what in ("num", "d_ray", "d_w2c"):
        want = getattr(c.ref, what)
        scale = float(want.abs().max())
        e, ce = _err(getattr(f, what), want), _err(getattr(comp, what), want)
        print(f"  {what}: fused {e / scale:.2e} composition {ce / scale:.2e} of scale {scale:.3g}")
        assert scale > 1e-3
        assert e <= max(4.0 * ce, FLOOR * scale), (what, e, ce, scale)


@pytest.mark.parametrize("name", list(CASES))
def test_flow_rgb_fused_returns_the_per_frame_losses(name):
    from copenerf import motion
    c = _case(name)
    cu = lambda x: x.to("cuda", torch.float32)  # noqa: E731
    per = motion.flow_rgb_fused(cu(c.ray_acc[:, :3]), cu(c.ray_acc[:, 3:]), cu(c.w2c), cu(c.cams), cu(c.I), cu(c.pixn),
                                cu(c.pix), cu(c.images), c.frame.cuda(), cu(c.gt), frame_valid=c.fvalid.cuda())
    comp = _torch_arm(c, torch.float32, "cuda")
    scale = float(c.ref.per.abs().max())
    e, ce = _err(per, c.ref.per), _err(comp.per, c.ref.per)
    print(f"{name}: per-frame loss fused {e / scale:.2e} composition {ce / scale:.2e} of scale {scale:.3g}")
    assert tuple(per.shape) == (c.T,)
    assert e <= max(4.0 * ce, FLOOR * scale)
    assert torch.equal(per.cpu() == 0, ~c.fvalid)


def test_two_runs_are_bitwise_equal_and_frames_are_read_in_place():
    c = _case("70x130")
    a, b = _fused(c), _fused(c)
    for k in ("num", "count", "d_ray", "d_w2c"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    gathered = c.images.index_select(0, c.frame).to("cuda", torch.float32).contiguous()
    g = _fused(c, images=gathered, frame=torch.arange(c.T))
    for k in ("num", "count", "d_ray", "d_w2c"):
        assert torch.equal(getattr(a, k), getattr(g, k)), k


def test_masked_and_out_of_range_frames_are_exact_zeros():
    """Frame 1 masked, or its index outside the stack (either side): zero sums and gradients for it, the bits of
    the other frames unchanged, and d_ray_acc is the sum over the frames that remain."""
    c = _case("37x53")
    full = _fused(c, fvalid=None)
    rest = _fused(c, fvalid=None, frames=[0, 2])
    frame_hi, frame_lo = c.frame.clone(), c.frame.clone()
    frame_hi[1], frame_lo[1] = c.N, -1
    for kw in (dict(fvalid=torch.tensor([True, False, True])), dict(fvalid=None, frame=frame_hi),
               dict(fvalid=None, frame=frame_lo)):
        m = _fused(c, **kw)
        assert not m.num[1].item() and not m.count[1].item() and not m.d_w2c[1].any()
        for t in (0, 2):
            assert torch.equal(m.num[t], full.num[t]) and torch.equal(m.count[t], full.count[t])
            assert torch.equal(m.d_w2c[t], full.d_w2c[t])
        assert torch.equal(m.d_ray, rest.d_ray)
        assert float(full.count[1]) > 0 and not torch.equal(m.d_ray, full.d_ray)
    none = _fused(c, fvalid=torch.zeros(3, dtype=torch.bool))
    for k in ("num", "count", "d_ray", "d_w2c"):
        assert not getattr(none, k).any(), k


def test_a_frame_does_not_depend_on_the_other_frames_or_rays_on_the_launch():
    c = _case("37x53")
    full = _fused(c, fvalid=None)
    for t in range(c.T):
        one = _fused(c, fvalid=None, frames=[t])
        assert torch.equal(one.num[0], full.num[t]) and torch.equal(one.d_w2c[0], full.d_w2c[t]), t
    head = _fused(c, fvalid=None, rays=slice(0, 64))  # the first workgroup's rays alone
    assert torch.equal(head.d_ray, full.d_ray[:64])


def test_a_correspondence_that_is_not_finite_counts_as_invalid():
    c = _case("37x53")
    bad = types.SimpleNamespace(**vars(c))
    bad.ray_acc = c.ray_acc.clone()
    bad.ray_acc[0] = float("nan")
    bad.ray_acc[1] = 0.0  # q2 = 0: 0 / 0
    f = _fused(bad, fvalid=None)
    rest = _fused(c, fvalid=None, rays=slice(2, None))
    assert torch.isfinite(f.num).all() and torch.equal(f.count, rest.count)
    assert not f.d_ray[:2].any() and torch.isfinite(f.d_ray).all() and torch.isfinite(f.d_w2c).all()


def test_empty_batch_gives_zero_sums():
    from copenerf import ops
    c = _case("5x7")
    cu = lambda x: x.to("cuda", torch.float32).contiguous()  # noqa: E731
    e = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
    KS = cu(c.I[:3, :3] @ c.cams[:, :3, :3])
    args = (e(0, 4), cu(c.w2c), KS, e(0, 2), e(0, 2), e(0, 3), cu(c.images), c.frame.cuda(), None)
    sums = ops.flow_rgb_fwd(*args)
    d_ray, d_w2c = ops.flow_rgb_bwd(*args, torch.ones(c.T, device="cuda"))
    assert tuple(sums.shape) == (c.T, 2) and not sums.any()
    assert tuple(d_ray.shape) == (0, 4) and tuple(d_w2c.shape) == (c.T, 3, 4) and not d_w2c.any()
    from copenerf import motion
    per = motion.flow_rgb_fused(e(0, 3), e(0, 1), cu(c.w2c), cu(c.cams), cu(c.I), e(0, 2), e(0, 2), cu(c.images),
                                c.frame.cuda(), e(0, 3))
    assert not per.any()


def test_checked_wrappers_refuse_bad_tensors():
    from copenerf import ops
    c = _case("5x7")
    cu = lambda x: x.to("cuda", torch.float32).contiguous()  # noqa: E731
    KS = cu(c.I[:3, :3] @ c.cams[:, :3, :3])
    good = [cu(c.ray_acc), cu(c.w2c), KS, cu(c.pixn), cu(c.pix), cu(c.gt), cu(c.images), c.frame.cuda(), None]
    ops.flow_rgb_fwd(*good)
    for i, bad in ((0, good[0][:, :3]), (1, good[1][:, :3]), (6, good[6].double()), (6, good[6].cpu()),
                   (7, good[7].int()), (8, torch.ones(c.T, device="cuda")), (1, good[1].repeat(9, 1, 1))):
        a = list(good)
        a[i] = bad
        with pytest.raises(RuntimeError):
            ops.flow_rgb_fwd(*a)


def test_frames_past_two_to_the_31_elements_of_the_stack():
    """Frame base offsets are 64-bit: three frames at the end of a stack of 2734 frames of 512 x 512 (their first
    element is past 2^31 elements, 8.6 GB into the stack) give the bits of the same frames in a stack of three."""
    c = _case("37x53")
    H = W = 512
    N = 2734
    assert (N - 3) * 3 * H * W > 2 ** 31
    small = torch.rand(3, 3, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    big = torch.empty(N, 3, H, W, device="cuda")  # (only the frames the indices name are ever read)
    big[N - 3:] = small
    want = _fused(c, images=small, frame=torch.arange(3))
    got = _fused(c, images=big, frame=torch.arange(3) + (N - 3))
    assert float(want.count.min()) > 0
    for k in ("num", "count", "d_ray", "d_w2c"):
        assert torch.equal(getattr(got, k), getattr(want, k)), k
