"""Pose refinement between stage 1 and stage 2 (utils_poses/pose_refinement.py:10-149, called at
train.py:369-383): learnable relative poses between consecutive frames, optimised on the photometric
error of each frame warped into its neighbour with the stage-1 depth maps, both directions.

  refine_loss                  one batch's loss: 2B jobs of the fused pass (ops.refine_warp, cn_refine_warp)
  refine_poses                 the loop of perform_pose_refinement on device-resident stacks
  world_poses                  relative poses -> camera-to-world poses (compute_w2c_mappings + inverse)
  PoseRefineDataset, compute_loss_and_warp_image, setup_pose_refinement, perform_pose_refinement
                               the reference's names and signatures, so train.py:25 can import them from
                               here

The per-pixel work (unproject, transform, project, sample, masked L1 and its pose gradient) is one HIP
pass per batch; what stays in torch is 4x4 algebra on B matrices and the optimiser.  The loop never
reads the device inside an epoch: the running loss is a device scalar read once per epoch.
"""
from __future__ import annotations

import os
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from .rays import PoseRetriever, inv4x4

BATCH_SIZE = 16            # DataLoader(batch_size=16, shuffle=False), pose_refinement.py:73
STOP_WINDOW = 50           # pose_refinement.py:144-147
STOP_STD = 1e-5

RefineResult = namedtuple("RefineResult", "pred_poses retriever optimizer scheduler losses converged")


def inv3x3(m):
    """Inverse of 3x3 matrices [..., 3, 3] by cofactors (intrinsics: no LAPACK call on the device)."""
    a, b, c = m[..., 0, 0], m[..., 0, 1], m[..., 0, 2]
    d, e, f = m[..., 1, 0], m[..., 1, 1], m[..., 1, 2]
    g, h, i = m[..., 2, 0], m[..., 2, 1], m[..., 2, 2]
    A, B, C = e * i - f * h, c * h - b * i, b * f - c * e
    det = a * A + d * B + g * C
    adj = torch.stack([A, B, C, f * g - d * i, a * i - c * g, c * d - a * f,
                       d * h - e * g, b * g - a * h, a * e - b * d], -1).reshape(m.shape)
    return adj / det[..., None, None]


def resize_depth(depth, H, W):
    """Depth maps [N, h, w] at the images' size: F.interpolate's default (nearest), as
    pose_refinement.py:113-114, and only when the sizes differ."""
    if tuple(depth.shape[-2:]) == (H, W):
        return depth
    return F.interpolate(depth.unsqueeze(1), (H, W)).squeeze(1)


def _per_pair(K, B):
    return K.expand(B, 3, 3) if K.dim() == 2 else K


def refine_loss(images, depth, K, Kinv, rel_poses, idx, next_idx):
    """The loss of one batch of B frame pairs (pose_refinement.py:118-123) from 2B jobs of the fused pass:
    B forward jobs (target idx, source next_idx, pose rel_poses) and B reverse jobs (target next_idx with
    its own depth, source idx, pose inv(rel_poses), the same K), each direction normalised by its own
    number of valid pixels: (sum num+ / sum cnt+ + sum num- / sum cnt-) / 2.
    images [N, 3, H, W], depth [N, h, w], K / Kinv [B, 3, 3] or [3, 3], rel_poses [B, 4, 4], idx /
    next_idx integer [B]."""
    from . import ops
    B = rel_poses.shape[0]
    depth = resize_depth(depth, images.shape[2], images.shape[3]).contiguous()
    pose = torch.cat([rel_poses[:, :3, :], inv4x4(rel_poses)[:, :3, :]])
    i0, i1 = idx.to(torch.int32), next_idx.to(torch.int32)
    Kj = _per_pair(K, B).repeat(2, 1, 1)
    Kij = _per_pair(Kinv, B).repeat(2, 1, 1)
    sums, _ = ops.refine_warp(images, depth, torch.cat([i0, i1]), torch.cat([i1, i0]), pose, Kj, Kij)
    pos, neg = sums[:B].sum(0), sums[B:].sum(0)
    return (pos[0] / pos[1] + neg[0] / neg[1]) / 2


def world_poses(rel_poses):
    """Camera-to-world poses [n + 1, 4, 4] of n consecutive relative poses, the first camera as the
    world: inverse of w2c[0] = I, w2c[i + 1] = rel[i] w2c[i] (compute_w2c_mappings,
    neus_fields.py:174-186, then torch.inverse, pose_refinement.py:135-136).  On the device the chain
    is one launch (motion.mat4_chain); CPU tensors (host-logic tests) take the products in a loop."""
    eye = torch.eye(4, dtype=rel_poses.dtype, device=rel_poses.device)[None]
    if rel_poses.shape[0] == 0:
        return eye
    if rel_poses.is_cuda:
        from .motion import mat4_chain
        chain = mat4_chain(rel_poses)
    else:
        w2c = [rel_poses[0]]
        for k in range(1, rel_poses.shape[0]):
            w2c.append(rel_poses[k] @ w2c[-1])
        chain = torch.stack(w2c)
    return inv4x4(torch.cat([eye, chain]))


def pair_batches(n_frames, batch_size=BATCH_SIZE):
    """The batches of an epoch: pairs (i, min(i + 1, N - 1)) for i < N - 1 in dataset order, batch_size
    at a time, the last batch ragged (PoseRefineDataset with max_interval 1 under the unshuffled loader)."""
    i = np.arange(max(n_frames - 1, 0))
    nxt = np.minimum(i + 1, n_frames - 1)
    return [(i[s:s + batch_size], nxt[s:s + batch_size]) for s in range(0, len(i), batch_size)]


def make_optimizer(retriever, lr):
    """Adam and the MultiStepLR of pose_refinement.py:88-91 (x 0.9 every 10 epochs from epoch 30)."""
    opt = torch.optim.Adam(retriever.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=list(range(30, 10000, 10)), gamma=0.9, last_epoch=-1)
    return opt, sched


def _check_interval(max_interval):
    if max_interval != 1:
        raise NotImplementedError(f"pose refinement: max_interval={max_interval} is out of scope "
                                  "(the reference runs with consecutive frames, max_interval=1)")


def _refine_loop(images, depth, K, retriever, optimizer, scheduler, epochs, batch_size, on_epoch, loss_fn):
    N = images.shape[0]
    dev = retriever.r.device
    depth = resize_depth(depth, images.shape[2], images.shape[3]).contiguous()
    Kinv = inv3x3(K)
    batches = [(torch.as_tensor(a, device=dev), torch.as_tensor(b, device=dev)) for a, b in pair_batches(N, batch_size)]
    all_idx = torch.arange(N - 1, device=dev)
    loss_fn = refine_loss if loss_fn is None else loss_fn
    window, losses, pred, converged = [], [], None, False
    for epoch in range(epochs):
        running = torch.zeros((), device=dev)
        for idx, nxt in batches:
            rel = retriever.poses_at(idx)
            Kb, Kib = (K, Kinv) if K.dim() == 2 else (K.index_select(0, idx), Kinv.index_select(0, idx))
            loss = loss_fn(images, depth, Kb, Kib, rel, idx, nxt)
            running = running + loss.detach() * len(idx)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        scheduler.step()
        with torch.no_grad():
            pred = world_poses(retriever.poses_at(all_idx))
        epoch_loss = float(running) / (N - 1)  # the epoch's one read of the device
        losses.append(epoch_loss)
        if on_epoch is not None:
            on_epoch(epoch, epoch_loss, pred)
        if len(window) >= STOP_WINDOW:
            window.pop(0)
        window.append(epoch_loss)
        if len(window) == STOP_WINDOW and np.std(window) <= STOP_STD:
            converged = True
            break
    return pred, losses, converged


def refine_poses(images, depth, K, *, pose_refine_lr=1e-3, pose_refine_epochs=2000, batch_size=BATCH_SIZE,
                 refine_from_scratch=True, init_c2c=None, on_epoch=None, loss_fn=None, max_interval=1):
    """perform_pose_refinement (pose_refinement.py:104-149) on device-resident stacks.
    images [N, 3, H, W], depth [N, h, w] (brought to (H, W) once, nearest), K [N, 3, 3] or [3, 3].
    The N - 1 relative poses start from the identity (refine_from_scratch) or from init_c2c [N - 1, 4, 4]
    (the motion network's, setup_pose_refinement); Adam(pose_refine_lr) under make_optimizer's
    schedule; after every epoch the world poses are world_poses(all relative poses) and
    on_epoch(epoch, loss, pred_poses) runs (the reference logs and computes its pose metrics there);
    stops when the last 50 epoch losses have a standard deviation <= 1e-5.
    loss_fn(images, depth, K, Kinv, rel_poses, idx, next_idx) replaces refine_loss (host-logic tests on
    CPU tensors; the fused pass itself has no CPU path).  Returns a RefineResult."""
    _check_interval(max_interval)
    N = images.shape[0]
    if N < 2:
        raise ValueError("pose refinement needs at least two frames")
    if depth.shape[0] != N:
        raise ValueError(f"{N} frames but {depth.shape[0]} depth maps")
    if not refine_from_scratch and init_c2c is None:
        raise ValueError("refine_from_scratch=False needs init_c2c (the motion network's relative poses)")
    init = None if refine_from_scratch else init_c2c.detach().to(images.device, torch.float32)
    retriever = PoseRetriever(N - 1, learn_R=True, learn_t=True, init_c2w=init).to(images.device)
    optimizer, scheduler = make_optimizer(retriever, pose_refine_lr)
    pred, losses, converged = _refine_loop(images, depth, K.to(images.device, torch.float32), retriever, optimizer,
                                           scheduler, pose_refine_epochs, batch_size, on_epoch, loss_fn)
    return RefineResult(pred, retriever, optimizer, scheduler, losses, converged)


# ---------------------------------------------------------------------------
# The reference's names and signatures (utils_poses/pose_refinement.py)
class PoseRefineDataset(torch.utils.data.Dataset):
    """pose_refinement.py:10-32: item idx pairs frame idx with frame idx + 1 (max_interval 1 only)."""

    def __init__(self, image_list, depth_list, K_list, max_interval=1):
        _check_interval(max_interval)
        self.image_list = image_list
        self.depth_list = depth_list
        self.K_list = K_list
        self.max_interval = max_interval

    def __len__(self):
        return len(self.image_list) - 1

    def __getitem__(self, idx):
        nxt = min(idx + 1, len(self.image_list) - 1)
        f = lambda a: torch.as_tensor(a).float()  # noqa: E731
        return (idx, nxt, f(self.image_list[idx]), f(self.image_list[nxt]), f(self.depth_list[idx]),
                f(self.depth_list[nxt]), self.K_list[idx], self.K_list[nxt])


def canonical_uv(H, W, device=None):
    """The pixel grid of pose_refinement.py:93-100: [3, H, W] = (x / ((W-1)/2) - 1, y / ((H-1)/2) - 1, 1)."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([x / ((W - 1) / 2) - 1, y / ((H - 1) / 2) - 1, torch.ones(H, W)]).to(device)


def compute_loss_and_warp_image(images, next_images, depths, K_batch, uv_batch, relative_poses, warp_pixel_fn=None):
    """pose_refinement.py:34-61 through the fused pass: (loss, warped_images [B, 3, H, W]).  The pass
    assumes the canonical pixel grid (canonical_uv, what setup_pose_refinement returns): uv_batch is
    only checked for its shape [B, 3, H, W], and warp_pixel_fn is not called (the pass samples with
    Trainer.warp_pixel's rule, border padding and align_corners=True)."""
    from . import ops
    B, _, H, W = images.shape
    if tuple(uv_batch.shape) != (B, 3, H, W):
        raise ValueError(f"uv_batch {tuple(uv_batch.shape)}: the fused pass takes the canonical grid [B, 3, H, W] = "
                         f"{(B, 3, H, W)}")
    stack = torch.cat([images, next_images]).float().contiguous()
    d = depths.reshape(B, H, W).float()
    d = torch.cat([d, d.new_empty(B, H, W)])  # (only the targets' depth is read)
    tgt = torch.arange(B, device=images.device, dtype=torch.int32)
    K_batch = K_batch.float()
    sums, warped = ops.refine_warp(stack, d, tgt, tgt + B, relative_poses[:, :3, :].float(), K_batch,
                                   inv3x3(K_batch), want_warped=True)
    tot = sums.sum(0)
    return tot[0] / tot[1], warped


def setup_pose_refinement(cfg, motion_network, train_dataset, total_nb_images, nb_sample_timestep):
    """pose_refinement.py:63-101: the stage-1 depth maps (extraction_stage1/depths/*.npz, key 'pred'), the
    pair dataset and its loader, the relative-pose table (from the motion network unless
    refine_from_scratch), its optimiser and schedule, and the canonical pixel grid."""
    tr = cfg["training"]
    H, W = (int(v) for v in tr["resolution"])
    depth_dir = os.path.join(tr["out_dir"], "extraction_stage1", "depths")
    depth_list = load_depth_dir(depth_dir)
    img = train_dataset["img"]
    dataset = PoseRefineDataset(image_list=img.imgs, depth_list=depth_list, K_list=img.K[img.i_train][:, :3, :3])
    loader = torch.utils.data.DataLoader(dataset, batch_size=BATCH_SIZE, shuffle=False)
    c2c_list = None
    if not tr["refine_from_scratch"]:
        with torch.no_grad():
            c2c_list = []
            for a, b in zip(img.i_train[:-1], img.i_train[1:]):
                _, c2c = motion_network.compute_relative_camera_pose(
                    target_cam_idx=a, final_ref_cam_idx=b, total_nb_images=total_nb_images,
                    nb_sample_timestep=nb_sample_timestep)
                c2c_list.append(motion_network.compute_w2c_mappings(c2c)[-1])
            c2c_list = torch.stack(c2c_list)
    dev = next(motion_network.parameters()).device if motion_network is not None else torch.device("cuda")
    retriever = PoseRetriever(len(img.i_train) - 1, learn_R=True, learn_t=True, init_c2w=c2c_list).to(dev)
    optimizer, scheduler = make_optimizer(retriever, tr["pose_refine_lr"])
    return dataset, loader, retriever, optimizer, scheduler, canonical_uv(H, W, dev)


def load_depth_dir(depth_dir):
    """The depth maps render_train_views writes: every .npz of the directory in sorted order, key 'pred'."""
    files = sorted(f for f in os.listdir(depth_dir) if f.endswith(".npz"))
    if not files:
        raise FileNotFoundError(f"no depth .npz files in {depth_dir}")
    return np.stack([np.load(os.path.join(depth_dir, f))["pred"] for f in files])


def perform_pose_refinement(model, motion_network, gt_poses, pose_refine_dataset, pose_refine_dataloader,
                            relative_pose_retriever, relative_pose_optimizer, relative_pose_optimizer_scheduler, uv,
                            cfg, warp_pixel_fn, compute_pose_error_fn):
    """pose_refinement.py:104-149 on the fused pass: the dataset's stacks go to the device once, the
    batches follow the loader's batch size in dataset order, and the per-epoch logging and pose metrics
    run as the loop's callback.  uv must be the canonical grid of setup_pose_refinement (checked by
    shape); warp_pixel_fn is not called."""
    tr = cfg["training"]
    H, W = (int(v) for v in tr["resolution"])
    if tuple(uv.shape) != (3, H, W):
        raise ValueError(f"uv {tuple(uv.shape)}: the fused pass takes the canonical grid [3, {H}, {W}]")
    ds = pose_refine_dataset
    _check_interval(ds.max_interval)
    dev = relative_pose_retriever.r.device
    images = torch.as_tensor(np.asarray(ds.image_list)).float().to(dev).contiguous()
    depth = torch.as_tensor(np.asarray(ds.depth_list)).float().to(dev)
    K = torch.as_tensor(np.asarray(ds.K_list)).float().to(dev)

    def on_epoch(epoch, loss, pred_poses):
        logger = getattr(model, "logger", None)
        if compute_pose_error_fn is not None:
            _, rpe_trans, rpe_rot, ate = compute_pose_error_fn(pred_poses, gt_poses)
            if logger is not None:
                logger.add_scalar("poseRefine/rpe_trans", rpe_trans, epoch)
                logger.add_scalar("poseRefine/rpe_rot", rpe_rot, epoch)
                logger.add_scalar("poseRefine/ate", ate, epoch)
        if logger is not None:
            logger.add_scalar("poseRefine/_loss", loss, epoch)
            logger.add_scalar("poseRefine/lr", relative_pose_optimizer_scheduler.get_last_lr()[0], epoch)

    batch = getattr(pose_refine_dataloader, "batch_size", None) or BATCH_SIZE
    pred, _, converged = _refine_loop(images, depth, K, relative_pose_retriever, relative_pose_optimizer,
                                      relative_pose_optimizer_scheduler, int(tr["pose_refine_epochs"]), batch,
                                      on_epoch, None)
    if converged:
        print("Converged. Stop refining poses.")
    return pred
