"""Restatement of the reference's pose refinement in plain torch ops (any dtype, any device): the
photometric warp loss of compute_loss_and_warp_image (utils_poses/pose_refinement.py:34-61) with
Trainer.warp_pixel (train.py:235-244), the batch loss of perform_pose_refinement (lines 118-123) and
its optimisation loop.  In float64 on the CPU it is the tests' reference (pinned to the reference's
own code by tests/golden/pose_refine.npz); in fp32 on the device it is the composed baseline whose
rounding error sets the fused pass's bars.  Also the input recipes of the GPU tests."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from helpers import smooth_frames


def uv_grid(H, W, dtype=torch.float64, device="cpu"):
    """[3, H, W] = (x / ((W-1)/2) - 1, y / ((H-1)/2) - 1, 1)   (pose_refinement.py:93-100)"""
    y, x = torch.meshgrid(torch.arange(H, dtype=dtype, device=device), torch.arange(W, dtype=dtype, device=device),
                          indexing="ij")
    return torch.stack([x / ((W - 1) / 2) - 1, y / ((H - 1) / 2) - 1, torch.ones_like(x)])


def warp_pixel(src_frame, uv):
    coord = torch.stack([uv[:, 0], uv[:, 1]], dim=-1)
    return F.grid_sample(src_frame, coord, mode="bilinear", padding_mode="border", align_corners=True)


def project(depths, K, Kinv, pose, uv):
    """(u', v') [B, 2, H, W] of the canonical grid under depths [B, H, W] and pose [B, >=3, 4]."""
    B, H, W = depths.shape
    xyz = Kinv @ (uv[None] * depths[:, None]).reshape(B, 3, -1)
    xyz = pose[:, :3, :3] @ xyz + pose[:, :3, 3:4]
    q = K @ xyz
    return (q[:, :2] / q[:, 2:3]).reshape(B, 2, H, W)


def warp_sums(images, next_images, depths, K, Kinv, pose):
    """Per pair: (sum |warp - image| over the mask [B], valid pixels [B], warped [B, 3, H, W], (u', v'))."""
    _, _, H, W = images.shape
    tuv = project(depths, K, Kinv, pose, uv_grid(H, W, images.dtype, images.device))
    valid = ((tuv[:, 0] >= -1) & (tuv[:, 0] <= 1) & (tuv[:, 1] >= -1) & (tuv[:, 1] <= 1)).to(images.dtype)[:, None]
    warped = warp_pixel(next_images, tuv)
    num = (torch.abs(warped - images) * valid).sum(dim=(1, 2, 3))
    return num, valid.sum(dim=(1, 2, 3)), warped, tuv


def loss_and_warp(images, next_images, depths, K, Kinv, pose):
    num, cnt, warped, _ = warp_sums(images, next_images, depths, K, Kinv, pose)
    return num.sum() / cnt.sum(), warped


def pair_loss(images, depth, K, Kinv, rel, idx, nxt, inverse=torch.inverse):
    """The batch loss of pose_refinement.py:121-123 on stacks: forward with depth[idx], reverse with
    depth[nxt], inverse(rel) and the same K."""
    pos, _ = loss_and_warp(images[idx], images[nxt], depth[idx], K, Kinv, rel)
    neg, _ = loss_and_warp(images[nxt], images[idx], depth[nxt], K, Kinv, inverse(rel))
    return (pos + neg) / 2


def skew(v):
    z = torch.zeros_like(v[0])
    return torch.stack([torch.stack([z, -v[2], v[1]]), torch.stack([v[2], z, -v[0]]), torch.stack([-v[1], v[0], z])])


def make_c2w(r, t):
    """model/common.py:255-308: Rodrigues with the +1e-15, [R | t; 0 0 0 1]."""
    Kx = skew(r)
    th = r.norm() + 1e-15
    R = torch.eye(3, dtype=r.dtype, device=r.device) + (torch.sin(th) / th) * Kx + ((1 - torch.cos(th)) / th ** 2) * (Kx @ Kx)
    top = torch.cat([R, t[:, None]], 1)
    return torch.cat([top, torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=r.dtype, device=r.device)], 0)


def stacked_poses(r, t, idx):
    return torch.stack([make_c2w(r[int(i)], t[int(i)]) for i in idx])


def world_poses(rel):
    w2c = [torch.eye(4, dtype=rel.dtype, device=rel.device)]
    for p in rel:
        w2c.append(p @ w2c[-1])
    return torch.inverse(torch.stack(w2c))


def composed_loop(images, depth, K, epochs, lr=1e-3, batch_size=16, inverse=torch.inverse):
    """perform_pose_refinement from scratch in torch ops: per-epoch losses and the final world poses."""
    N = images.shape[0]
    dt, dev = images.dtype, images.device
    r = torch.zeros(N - 1, 3, dtype=dt, device=dev, requires_grad=True)
    t = torch.zeros(N - 1, 3, dtype=dt, device=dev, requires_grad=True)
    opt = torch.optim.Adam([r, t], lr=lr)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(range(30, 10000, 10)), gamma=0.9)
    Kinv = inverse(K)
    losses = []
    for _ in range(epochs):
        running = 0.0
        for s in range(0, N - 1, batch_size):
            idx = torch.arange(s, min(s + batch_size, N - 1), device=dev)
            loss = pair_loss(images, depth, K, Kinv, stacked_poses(r, t, idx), idx, idx + 1, inverse)
            running += float(loss.detach()) * len(idx)
            opt.zero_grad()
            loss.backward()
            opt.step()
        sched.step()
        losses.append(running / (N - 1))
    with torch.no_grad():  # (on the host: torch.inverse on a device tensor is a LAPACK-style call)
        pred = world_poses(stacked_poses(r.cpu(), t.cpu(), range(N - 1)))
    return losses, pred


# ---------------------------------------------------------------------------
# Input recipes (float64 on the CPU; the tests cast)
def recipe(H, W, N, seed, planar=False):
    """K = [[f, 0, cx], [0, f W / H, cy], [0, 0, 1]] with f in [1.2, 1.4] and a small principal-point
    offset, depth -(2 + 0.5 sin cos), N - 1 relative poses with |r| <= 0.03 and |t| <= 0.08 per axis;
    frames: helpers.smooth_frames, or (planar) per-channel affine functions of (x, y) with odd frames
    offset by +0.5 (a bilinear sample of a plane is exact and sign(warp - I) is constant)."""
    g = torch.Generator().manual_seed(1000 + seed)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)  # noqa: E731
    f = 1.2 + 0.2 * rnd(1).item()
    cx, cy = (0.04 * rnd(2) - 0.02).tolist()
    K = torch.tensor([[f, 0.0, cx], [0.0, f * W / H, cy], [0.0, 0.0, 1.0]], dtype=torch.float64)
    y = torch.linspace(0, 1, H, dtype=torch.float64).view(1, H, 1)
    x = torch.linspace(0, 1, W, dtype=torch.float64).view(1, 1, W)
    ph = 6.28 * rnd(N, 2).view(N, 2, 1, 1)
    depth = -(2.0 + 0.5 * torch.sin(3.0 * x + ph[:, 0]) * torch.cos(2.0 * y + ph[:, 1]))
    r = 0.06 * rnd(N - 1, 3) - 0.03
    t = 0.16 * rnd(N - 1, 3) - 0.08
    if planar:
        c = rnd(N, 3, 3)
        images = (0.2 + 0.1 * c[..., 0, None, None] * x[None] + 0.1 * c[..., 1, None, None] * y[None] +
                  0.1 * c[..., 2, None, None])  # in [0.2, 0.5]: the +0.5 of odd frames fixes the sign
        images = images + 0.5 * (torch.arange(N) % 2).view(N, 1, 1, 1)
    else:
        images = smooth_frames(N, H, W, seed=seed).double()
    return dict(images=images.contiguous(), depth=depth.contiguous(), K=K, r=r, t=t)


def recipe_jobs(c):
    """The 2 (N - 1) jobs of one batch over all pairs of a recipe: (tgt, src, pose [J, 4, 4], K, Kinv [J, 3, 3])."""
    n = c["images"].shape[0] - 1
    idx = torch.arange(n)
    rel = stacked_poses(c["r"], c["t"], idx)
    pose = torch.cat([rel, torch.inverse(rel)])
    K = c["K"].expand(2 * n, 3, 3).contiguous()
    return torch.cat([idx, idx + 1]), torch.cat([idx + 1, idx]), pose, K, torch.inverse(K)


def job_sums(images, depth, tgt, src, pose, K, Kinv):
    """(sums [J, 2], warped, (u', v')) of jobs in the tensors' dtype, by warp_sums."""
    num, cnt, warped, tuv = warp_sums(images[tgt], images[src], depth[tgt], K, Kinv, pose)
    return torch.stack([num, cnt], 1), warped, tuv


def edge_margin(tuv):
    """min over pixels of | |u'| - 1 | and | |v'| - 1 |: how far the closest pixel is from the mask's edge."""
    return float((tuv.abs() - 1).abs().min())


def plane_scene(N=4, H=24, W=32):
    """The end-to-end scene: a fronto-parallel plane at depth 2 with an analytic sin / cos texture, cameras
    rotated about the optical axis by (0, 0.03, -0.02, 0.04) and shifted in the plane by up to 0.1.
    Returns float64 (images [N, 3, H, W], depth [N, H, W], K, c2w [N, 4, 4])."""
    ang = [0.0, 0.03, -0.02, 0.04][:N]
    sh = [(0.0, 0.0), (0.1, -0.05), (0.02, 0.03), (0.08, 0.1)][:N]
    K = torch.tensor([[1.3, 0.0, 0.0], [0.0, 1.3 * W / H, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    uv = uv_grid(H, W)
    d = -2.0
    cam = torch.inverse(K) @ (uv * d).reshape(3, -1)  # camera-frame points of the plane z = -2
    images, c2w = [], []
    for a, (sx, sy) in zip(ang, sh):
        M = torch.eye(4, dtype=torch.float64)
        M[:2, :2] = torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]], dtype=torch.float64)
        M[0, 3], M[1, 3] = sx, sy
        w = M[:3, :3] @ cam + M[:3, 3:4]
        X, Y = 0.7 * w[0].reshape(H, W), 0.7 * w[1].reshape(H, W)
        images.append(torch.stack([0.5 + 0.3 * torch.sin(2.1 * X + 0.3) * torch.cos(1.7 * Y),
                                   0.5 + 0.3 * torch.cos(1.3 * X - 0.5) * torch.sin(2.3 * Y + 0.2),
                                   0.5 + 0.3 * torch.sin(1.1 * X + 1.9 * Y)]))
        c2w.append(M)
    c2w = torch.stack(c2w)
    c2w = torch.inverse(c2w[0])[None] @ c2w  # the first camera is the world
    return torch.stack(images).contiguous(), torch.full((N, H, W), d, dtype=torch.float64), K, c2w


def pose_error(pred, gt):
    return float((pred - gt).abs().max())


def np_f32(x):
    return np.ascontiguousarray(x.detach().cpu().numpy().astype(np.float32))
