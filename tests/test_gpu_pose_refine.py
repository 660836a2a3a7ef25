"""The fused pose-refinement pass (cn_refine_warp, ABI v17) and the loop on the device, against the
float64 restatement tests/pose_refine_ref.py (pinned to the reference by tests/golden/pose_refine.npz).

Sizes: 3 x 5 (fewer pixels than a wavefront), 37 x 53 (ragged tiles, several workgroups per job) and
70 x 130 (many partials per job).  Bars come from the fp32 torch composition of the same expressions
on the device (its error against float64, times 4) with a floor of 4e-6 of scale (a few fp32 ulps
through ~20 operations); the seeds are chosen so that in float64 no pixel lies within 1e-5 of the
mask's edge (asserted first), which makes the valid counts exact.

Measured on an MI355X, error against float64 relative to scale, fused pass / fp32 torch composition:
  sums     3x5 7.4e-8 / 5.5e-8, 37x53 3.6e-8 / 9.2e-8, 70x130 4.3e-8 / 6.2e-8
  warped   3x5 2.2e-7 / 2.1e-7, 37x53 1.5e-6 / 1.5e-6, 70x130 1.5e-6 / 1.4e-6 (the coordinate's rounding
           times the texture's slope: both arms carry it)
  planar   dpose 2.6e-7 .. 3.7e-7 / 3.3e-7 .. 6.8e-7; dr, dt 2.2e-7 .. 7.3e-7 / 2.2e-7 .. 7.2e-7
  taps     (37x53, textured) dpose 2.6e-7 / 7.6e-7, dr 2.5e-7 / 3.7e-7, dt 1.6e-7 / 2.4e-7
  end to end  loss 0.0531 -> 0.0042 (x 0.079) in both loops, worst pose entry error 0.100 -> 0.0616; the fused
           curve is within 3.0e-5 of the composed one over the first 20 epochs and 1.5e-4 over all 100
"""
import functools
import types

import numpy as np
import pytest
import torch

import pose_refine_ref as R

pytestmark = pytest.mark.gpu

CASES = {"3x5": (3, 5, 3, 0), "37x53": (37, 53, 5, 0), "70x130": (70, 130, 4, 2)}  # H, W, N, seed
MARGIN = 1e-5
FLOOR = 4e-6


def _f32(x, dev="cuda"):
    return x.detach().to(dev, torch.float32).contiguous()


def _i32(x, dev="cuda"):
    return x.to(dev, torch.int32)


def _dev_inverse(m):
    from copenerf.rays import inv4x4
    return inv4x4(m)


@functools.lru_cache(None)
def _case(name, planar=False):
    """A recipe with its float64 reference: per-job sums, warped frames, dpose; shared, never modified."""
    H, W, N, seed = CASES[name]
    c = R.recipe(H, W, N, seed, planar)
    tgt, src, pose, K, Kinv = R.recipe_jobs(c)
    pose = pose.clone().requires_grad_(True)
    sums, warped, tuv = R.job_sums(c["images"], c["depth"], tgt, src, pose, K, Kinv)
    (dpose,) = torch.autograd.grad(sums[:, 0].sum(), pose)
    return types.SimpleNamespace(c=c, tgt=tgt, src=src, pose=pose.detach(), K=K, Kinv=Kinv, sums=sums.detach(),
                                 warped=warped.detach(), dpose=dpose[:, :3, :], margin=R.edge_margin(tuv.detach()),
                                 H=H, W=W, N=N)


def _composition(cs):
    """The fp32 torch composition of the same jobs on the device: (sums, warped, dpose)."""
    pose = _f32(cs.pose).requires_grad_(True)
    sums, warped, _ = R.job_sums(_f32(cs.c["images"]), _f32(cs.c["depth"]), cs.tgt.cuda(), cs.src.cuda(), pose,
                                 _f32(cs.K), _f32(cs.Kinv))
    (dpose,) = torch.autograd.grad(sums[:, 0].sum(), pose)
    return sums.detach(), warped.detach(), dpose[:, :3, :]


def _fused(cs, want_warped=False, jobs=None):
    from copenerf import ops
    sel = slice(None) if jobs is None else jobs
    pose = _f32(cs.pose[sel, :3, :]).requires_grad_(True)
    sums, warped = ops.refine_warp(_f32(cs.c["images"]), _f32(cs.c["depth"]), _i32(cs.tgt[sel]), _i32(cs.src[sel]), pose,
                                   _f32(cs.K[sel]), _f32(cs.Kinv[sel]), want_warped=want_warped)
    (dpose,) = torch.autograd.grad(sums[:, 0].sum(), pose)
    return sums.detach(), warped, dpose


def _err(got, want):
    return float((got.detach().double().cpu() - want).abs().max())


def _bar(comp_err, scale):
    return max(4.0 * comp_err, FLOOR * scale)


@pytest.mark.parametrize("name", list(CASES))
def test_counts_sums_and_warped(name):
    cs = _case(name)
    assert cs.margin >= MARGIN, cs.margin  # no pixel at the mask's edge: the counts must be exact
    outside = 1.0 - float(cs.sums[:, 1].sum()) / (len(cs.tgt) * cs.H * cs.W)
    sums, warped, _ = _fused(cs, want_warped=True)
    csums, cwarped, _ = _composition(cs)
    assert torch.equal(sums[:, 1].double().cpu(), cs.sums[:, 1]), (sums[:, 1], cs.sums[:, 1])
    s_scale, w_scale = float(cs.sums[:, 0].abs().max()), float(cs.warped.abs().max())
    e_s, c_s = _err(sums[:, 0], cs.sums[:, 0]), _err(csums[:, 0], cs.sums[:, 0])
    e_w, c_w = _err(warped, cs.warped), _err(cwarped, cs.warped)
    print(f"{name}: outside the mask {outside:.3f}; sums fused {e_s / s_scale:.2e} composition {c_s / s_scale:.2e} "
          f"of scale; warped fused {e_w / w_scale:.2e} composition {c_w / w_scale:.2e} of scale")
    assert 0.02 <= outside <= 0.5
    assert e_s <= _bar(c_s, s_scale), (e_s, c_s, s_scale)
    assert e_w <= _bar(c_w, w_scale), (e_w, c_w, w_scale)


def _rt_grads_ref(cs):
    """Float64 gradients of the batch loss over all pairs with respect to the table's r and t."""
    r, t = cs.c["r"].clone().requires_grad_(True), cs.c["t"].clone().requires_grad_(True)
    idx = torch.arange(cs.N - 1)
    loss = R.pair_loss(cs.c["images"], cs.c["depth"], cs.K[0], cs.Kinv[0], R.stacked_poses(r, t, idx), idx, idx + 1)
    return (loss.detach(),) + torch.autograd.grad(loss, [r, t])


def _rt_grads_composition(cs):
    r, t = _f32(cs.c["r"]).requires_grad_(True), _f32(cs.c["t"]).requires_grad_(True)
    idx = torch.arange(cs.N - 1, device="cuda")
    loss = R.pair_loss(_f32(cs.c["images"]), _f32(cs.c["depth"]), _f32(cs.K[0]), _f32(cs.Kinv[0]),
                       R.stacked_poses(r, t, idx), idx, idx + 1, inverse=_dev_inverse)
    return (loss.detach(),) + torch.autograd.grad(loss, [r, t])


def _rt_grads_fused(cs, depth=None):
    from copenerf import PoseRetriever
    from copenerf.pose_refine import refine_loss
    p = PoseRetriever(cs.N - 1).cuda()
    with torch.no_grad():
        p.r.copy_(_f32(cs.c["r"]))
        p.t.copy_(_f32(cs.c["t"]))
    idx = torch.arange(cs.N - 1, device="cuda")
    depth = _f32(cs.c["depth"] if depth is None else depth)
    loss = refine_loss(_f32(cs.c["images"]), depth, _f32(cs.K[0]), _f32(cs.Kinv[0]), p.poses_at(idx), idx, idx + 1)
    return (loss.detach(),) + torch.autograd.grad(loss, [p.r, p.t])


def _check_grads(cs, tight):
    _, _, dpose = _fused(cs)
    _, _, cdpose = _composition(cs)
    ref = [cs.dpose] + list(_rt_grads_ref(cs)[1:])
    got = [dpose] + list(_rt_grads_fused(cs)[1:])
    comp = [cdpose] + list(_rt_grads_composition(cs)[1:])
    for what, g, c, w in zip(("dpose", "dr", "dt"), got, comp, ref):
        scale = float(w.abs().max())
        e, ce = _err(g, w) / scale, _err(c, w) / scale
        print(f"{what}: fused {e:.2e} composition {ce:.2e} of max |gradient| {scale:.3g}")
        assert scale > 1e-3
        assert e <= (max(4.0 * ce, FLOOR) if tight else 2e-3), (what, e, ce)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_tight_on_planar_frames(name):
    """Frames that are planes in (x, y): the bilinear sample is exact, its derivative does not jump at cell
    edges and sign(warp - I) is constant (odd frames are offset by +0.5), so the gradient is as smooth in
    the inputs as the sums are."""
    cs = _case(name, True)
    assert cs.margin >= MARGIN, cs.margin
    assert float((cs.warped - cs.c["images"][cs.tgt]).abs().min()) > 0.1  # the sign never flips
    _check_grads(cs, tight=True)


def test_gradients_through_the_taps():
    """Textured frames at 37 x 53, at the project's gradient bar of 2e-3 of scale: a last-ulp change may move a
    pixel across a cell edge or flip a sign (O(1 / pixels)); a wrong tap or weight is an O(1) error."""
    cs = _case("37x53")
    assert cs.margin >= MARGIN, cs.margin
    _check_grads(cs, tight=False)


def test_results_are_reproducible_and_independent_of_the_launch():
    cs = _case("37x53")
    a = _fused(cs, want_warped=True)
    b = _fused(cs, want_warped=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    J = len(cs.tgt)
    for j in range(J):
        s, w, d = _fused(cs, want_warped=True, jobs=slice(j, j + 1))
        assert torch.equal(s[0], a[0][j]) and torch.equal(d[0], a[2][j]) and torch.equal(w[0], a[1][j]), j
    # a job whose index is outside the stack reads nothing and sums to zero; its neighbours are unchanged
    from copenerf import ops
    tgt = _i32(cs.tgt).clone()
    tgt[1] = cs.N
    sums, _ = ops.refine_warp(_f32(cs.c["images"]), _f32(cs.c["depth"]), tgt, _i32(cs.src), _f32(cs.pose[:, :3, :]),
                              _f32(cs.K), _f32(cs.Kinv))
    assert torch.equal(sums[1], torch.zeros(2, device="cuda"))
    assert torch.equal(sums[0], a[0][0]) and torch.equal(sums[2:], a[0][2:])


def test_depth_at_another_resolution():
    """Depth maps at 19 x 27 for frames of 37 x 53: brought to the frames' size by nearest interpolation."""
    cs = _case("37x53")
    low = R.recipe(19, 27, cs.N, CASES["37x53"][3])["depth"]
    up = torch.nn.functional.interpolate(low[:, None], (cs.H, cs.W))[:, 0]
    idx = torch.arange(cs.N - 1)
    rel = R.stacked_poses(cs.c["r"], cs.c["t"], idx)
    _, _, tuv = R.job_sums(cs.c["images"], up, cs.tgt, cs.src, cs.pose, cs.K, cs.Kinv)
    assert R.edge_margin(tuv) >= MARGIN
    want = R.pair_loss(cs.c["images"], up, cs.K[0], cs.Kinv[0], rel, idx, idx + 1)
    di = idx.cuda()
    comp = R.pair_loss(_f32(cs.c["images"]), _f32(up), _f32(cs.K[0]), _f32(cs.Kinv[0]), _f32(rel), di, di + 1,
                       inverse=_dev_inverse)
    got = _rt_grads_fused(cs, depth=low)[0]
    e, ce = _err(got, want), _err(comp, want)
    print(f"loss {float(want):.6f}: fused {e:.2e} composition {ce:.2e}")
    assert e <= _bar(ce, float(want))


def test_compat_function_returns_the_reference_pair():
    from copenerf.pose_refine import canonical_uv, compute_loss_and_warp_image
    cs = _case("37x53")
    B = cs.N - 1
    im, d = _f32(cs.c["images"]), _f32(cs.c["depth"])
    uv = canonical_uv(cs.H, cs.W, "cuda")[None].repeat(B, 1, 1, 1)
    loss, warped = compute_loss_and_warp_image(im[:-1], im[1:], d[:-1, None], _f32(cs.K[:B]), uv, _f32(cs.pose[:B]), None)
    want = cs.sums[:B, 0].sum() / cs.sums[:B, 1].sum()
    assert _err(loss, want) <= 1e-5 * float(want)
    assert _err(warped, cs.warped[:B]) <= 1e-5


def test_end_to_end_refinement_recovers_the_plane_scene():
    """A fronto-parallel textured plane at depth 2, 4 frames of 24 x 32, from scratch, lr 1e-3, one batch per
    epoch, 100 epochs: the fused loop and the torch composition on the device both reduce the loss to a
    tenth and the worst pose entry error below 0.7 of the identity's, and their loss curves agree."""
    from copenerf.pose_refine import refine_poses
    images, depth, K, c2w = R.plane_scene()
    res = refine_poses(_f32(images), _f32(depth), _f32(K), pose_refine_lr=1e-3, pose_refine_epochs=100)
    closs, cpred = R.composed_loop(_f32(images), _f32(depth), _f32(K), 100,
                                   inverse=lambda m: _dev_inverse(m) if m.shape[-1] == 4 else torch.inverse(m.cpu()).cuda())
    ident = R.pose_error(torch.eye(4, dtype=torch.float64).expand(4, 4, 4), c2w)
    fl, cl = np.array(res.losses), np.array(closs)
    div = np.abs(fl - cl) / cl
    f_pose, c_pose = R.pose_error(res.pred_poses.double().cpu(), c2w), R.pose_error(cpred.double().cpu(), c2w)
    print(f"fused loss {fl[0]:.4f} -> {fl[-1]:.4f}, composed {cl[0]:.4f} -> {cl[-1]:.4f}; pose error fused {f_pose:.4f} "
          f"composed {c_pose:.4f} identity {ident:.4f}; divergence first 20 epochs {div[:20].max():.2e}, all {div.max():.2e}")
    assert len(fl) == 100 and not res.converged
    for losses, pose in ((fl, f_pose), (cl, c_pose)):
        assert losses[-1] <= 0.1 * losses[0]
        assert pose <= 0.7 * ident
    assert div[:20].max() <= 5e-4 and div.max() <= 5e-3


def test_compat_loop_runs_the_same_refinement(tmp_path):
    """setup_pose_refinement / perform_pose_refinement with the reference's arguments: depth .npz files in
    out_dir/extraction_stage1/depths, the dataset's numpy stacks, a logger and a pose-metric callback."""
    from copenerf import pose_refine as P
    images, depth, K, _ = R.plane_scene(N=3)
    ddir = tmp_path / "extraction_stage1" / "depths"
    ddir.mkdir(parents=True)
    for i in range(3):
        np.savez(ddir / f"{i:03d}.npz", pred=R.np_f32(depth[i]))
    K4 = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    K4[:, :3, :3] = R.np_f32(K)
    cfg = {"training": {"out_dir": str(tmp_path), "resolution": [24, 32], "refine_from_scratch": True,
                        "pose_refine_lr": 1e-3, "pose_refine_epochs": 3}}
    train = {"img": types.SimpleNamespace(imgs=R.np_f32(images), K=K4, i_train=np.arange(3))}
    logged = []
    model = types.SimpleNamespace(logger=types.SimpleNamespace(add_scalar=lambda *a: logged.append(a)))
    ds, loader, retr, opt, sched, uv = P.setup_pose_refinement(cfg, None, train, 3, 10)
    assert len(ds) == 2 and tuple(uv.shape) == (3, 24, 32) and uv.is_cuda
    pred = P.perform_pose_refinement(model, None, None, ds, loader, retr, opt, sched, uv, cfg, None,
                                     lambda p, g: (0.0, 1.0, 2.0, 3.0))
    want = P.refine_poses(_f32(images), _f32(depth), _f32(K), pose_refine_epochs=3)
    assert torch.equal(pred, want.pred_poses)
    assert len(logged) == 5 * 3 and logged[0][0] == "poseRefine/rpe_trans"


def test_frames_past_two_to_the_31_elements_of_the_stack():
    """Frame base offsets are 64-bit: two frames at the end of a stack of 2734 frames of 512 x 512 (their first
    element is past 2^31 elements, 8.6 GB into the stack) give the bits of the same frames in a stack of two."""
    from copenerf import ops
    H = W = 512
    N = 2734
    assert (N - 2) * 3 * H * W > 2 ** 31
    small = _f32(R.recipe(H, W, 2, 1)["images"])
    depth2 = _f32(R.recipe(H, W, 2, 1)["depth"])
    c = _case("37x53")
    pose, K, Kinv = _f32(c.pose[:2, :3, :]), _f32(c.K[:2]), _f32(c.Kinv[:2])
    pair = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    want = ops.refine_warp(small, depth2, pair, 1 - pair, pose, K, Kinv, want_warped=True)
    big = torch.empty(N, 3, H, W, device="cuda")  # (only the frames the jobs name are ever read)
    big[N - 2:] = small
    bdepth = torch.empty(N, H, W, device="cuda")
    bdepth[N - 2:] = depth2
    got = ops.refine_warp(big, bdepth, pair + (N - 2), (1 - pair) + (N - 2), pose, K, Kinv, want_warped=True)
    assert float(want[0][:, 1].min()) > 0.5 * H * W
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
