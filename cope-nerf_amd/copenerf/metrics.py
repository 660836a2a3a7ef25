"""Evaluation metrics: what the reference's Evaluator computes after rendering (eval.py:190-272).

  image metrics   psnr / ssim with co3d_metric.py's signatures on the fused device pass (cn_image_metrics),
                  image_metrics = Evaluator.image_eval (eval.py:190-221);
  depth metrics   depth_metrics = Evaluator.depth_eval (eval.py:223-244) and compute_depth_errors
                  (model/training.py:126-154) on cn_depth_errors, the median ratio computed on the device;
  pose metrics    align_ate_c2b_use_a2b, compute_ATE, compute_rpe, compute_pose_error (train.py:169-178,
                  utils_poses/align_traj.py, utils_poses/comp_ate.py, ATE/align_trajectory.py) in float64
                  numpy on the host: a few dozen 4 x 4 matrices, control plane;
  evaluate        render the test views (inference.render_image), keep the maps on the device, run the
                  above and merge the dictionaries in eval.py:264-267's order; write_results writes
                  results.txt (eval.py:268-270).

LPIPS needs network weights that are fetched on first use; they are not part of this build.  Pass
lpips_fn(pred, gt) (both [3, H, W]) to have the "LPIPS" key; without it the key is absent.

The image and depth kernels have no CPU path: tensors must live on the device.  Host arrays (numpy, as the
reference's depth loaders give) are uploaded.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

DEPTH_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


# ---------------------------------------------------------------------------
# image metrics
def _batched(img1, img2, who):
    if not (torch.is_tensor(img1) and torch.is_tensor(img2)):
        raise TypeError(f"{who}: tensors expected")
    if img1.shape != img2.shape or img1.dim() not in (3, 4):
        raise ValueError(f"{who}: two [C, H, W] or [N, C, H, W] tensors of one shape expected, got "
                         f"{tuple(img1.shape)} and {tuple(img2.shape)}")
    a, b = (img1, img2) if img1.dim() == 4 else (img1[None], img2[None])
    return a.contiguous(), b.contiguous()


def psnr(img1, img2):
    """co3d_metric.py:14-16: 20 log10(1 / sqrt(mse)) with the mean over everything behind the first axis --
    [N, 1] for a batch, [C, 1] (per channel) for an unbatched [C, H, W] input, which is how eval.py:204
    calls it."""
    a, b = _batched(img1, img2, "psnr")
    mse = ops.image_metrics(a, b)[0][..., 0]  # [N, C]
    mse = mse.mean(1, keepdim=True) if img1.dim() == 4 else mse.reshape(-1, 1)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def ssim(img1, img2, window_size=11, size_average=True):
    """co3d_metric.py:18-48: the mean of the SSIM map (a scalar tensor), or one mean per image of a batch with
    size_average=False."""
    if window_size != 11:
        raise NotImplementedError(f"ssim: only window_size=11 is implemented (got {window_size})")
    a, b = _batched(img1, img2, "ssim")
    means = ops.image_metrics(a, b)[0][..., 1]  # [N, C]
    if size_average:
        return means.mean()
    if img1.dim() != 4:
        raise IndexError("ssim: size_average=False needs a batched [N, C, H, W] input (the reference's "
                         "mean(1).mean(1).mean(1) fails on [C, H, W] too)")
    return means.mean(1)


def _image_stack(x, who):
    """A list of [H, W, 3] maps (what eval.py's lists hold and render_image returns) or a stack
    [N, H, W, 3] -> a list of contiguous [n, 3, H, W] stacks of equal-sized images, in order."""
    if torch.is_tensor(x):
        if x.dim() != 4:
            raise ValueError(f"{who}: a stack must be [N, H, W, C], got {tuple(x.shape)}")
        return [x.permute(0, 3, 1, 2).float().contiguous()]
    groups = []
    for im in x:
        if not torch.is_tensor(im) or im.dim() != 3:
            raise ValueError(f"{who}: [H, W, C] tensors expected")
        im = im.permute(2, 0, 1).float()
        if groups and groups[-1][0].shape == im.shape:
            groups[-1].append(im)
        else:
            groups.append([im])
    return [torch.stack(g).contiguous() for g in groups]


def image_metrics(pred, gt, lpips_fn=None):
    """Evaluator.image_eval (eval.py:190-221): pred and gt are lists of [H, W, 3] maps (or [N, H, W, 3]
    stacks).  Per image the PSNR is the mean of the per-channel PSNRs and the SSIM the mean of the map; the
    per-image values are averaged in float64.  "LPIPS" only with lpips_fn(pred [3, H, W], gt [3, H, W])."""
    P, G = _image_stack(pred, "image_metrics"), _image_stack(gt, "image_metrics")
    if [p.shape for p in P] != [g.shape for g in G]:
        raise ValueError("image_metrics: pred and gt must hold images of the same sizes in the same order")
    psnrs, ssims, lp = [], [], []
    for p, g in zip(P, G):
        out = ops.image_metrics(p, g)[0]
        psnrs.append((20 * torch.log10(1.0 / torch.sqrt(out[..., 0]))).mean(1).double())
        ssims.append(out[..., 1].mean(1).double())
        if lpips_fn is not None:
            for a, b in zip(p, g):
                lp.append(torch.as_tensor(lpips_fn(a, b)).double().mean().reshape(1).to(p.device))
    if not psnrs:
        raise ValueError("image_metrics: no images")
    res = {"PSNR": float(torch.cat(psnrs).mean()), "SSIM": float(torch.cat(ssims).mean())}
    if lpips_fn is not None:
        res["LPIPS"] = float(torch.cat(lp).mean())
    return res


# ---------------------------------------------------------------------------
# depth metrics
def _depth_map(x, who):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x)).to("cuda")
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{who}: [H, W] depth maps expected")
    return x.float()


def median_ratio(gt, pred, min_depth, max_depth):
    """median(gt) / median(pred) over the valid ground-truth pixels of each image (eval.py:234-237), pred
    taken at the nearest-neighbour source pixel the kernel uses, by np.median's rule (the mean of the two
    middle values for an even count), in fp32 on the device: gt [N, Hg, Wg], pred [N, Hp, Wp] -> [N].
    No valid pixel, or a NaN among the valid values: NaN."""
    N, Hg, Wg = gt.shape
    Hp, Wp = pred.shape[1:]
    dev = gt.device
    yi = torch.arange(Hg, device=dev) * Hp // Hg
    xi = torch.arange(Wg, device=dev) * Wp // Wg
    pn = pred[:, yi][:, :, xi]
    valid = ((gt >= min_depth) & (gt <= max_depth)).flatten(1)
    n = valid.sum(1)
    lo = ((n - 1).clamp(min=0) // 2)[:, None]
    hi = (n // 2).clamp(max=Hg * Wg - 1)[:, None]
    nan = torch.full((), float("nan"), device=dev)

    def med(x):
        x = x.flatten(1)
        s = torch.where(valid, x, torch.full((), float("inf"), device=dev)).sort(1).values
        m = ((s.gather(1, lo) + s.gather(1, hi)) / 2)[:, 0]
        return torch.where((n == 0) | (valid & torch.isnan(x)).any(1), nan, m)

    return (med(gt) / med(pn)).contiguous()


def _depth_errors(gt, pred, min_depth, max_depth, clamp):
    ratio = median_ratio(gt, pred, min_depth, max_depth)
    return ops.depth_errors(gt.contiguous(), pred.contiguous(), ratio, min_depth, max_depth, clamp)


def _absent(d):
    if d is None:
        return True
    if isinstance(d, (int, float)):
        return d == -1
    return (torch.is_tensor(d) or isinstance(d, np.ndarray)) and d.ndim == 0 and float(d) == -1


def depth_metrics(gt_depths, pred_depths, min_depth=0.1, max_depth=80.0, clamp=True):
    """Evaluator.depth_eval (eval.py:223-244): per image the prediction is brought to the ground truth's
    size (nearest neighbour), scaled by the ratio of the medians over the valid pixels, clamped (clamp=True,
    as eval.py:239-240) and the seven errors are taken; their means over the images (float64) come back as a
    dict.  None when every ground truth is -1 (no depth in the dataset).  Images without ground truth among
    others that have one are an error, as in the reference."""
    gt_depths, pred_depths = list(gt_depths), list(pred_depths)
    if all(_absent(g) for g in gt_depths):
        return None
    if any(_absent(g) for g in gt_depths) or len(gt_depths) != len(pred_depths):
        raise ValueError("depth_metrics: one ground-truth map per prediction expected")
    rows = []
    for g, p in zip(gt_depths, pred_depths):
        g, p = _depth_map(g, "depth_metrics"), _depth_map(p, "depth_metrics")
        rows.append(_depth_errors(g[None], p[None], min_depth, max_depth, clamp)[0, :7].double())
    mean = torch.stack(rows).mean(0).tolist()
    return dict(zip(DEPTH_KEYS, mean))


def compute_depth_errors(gt_depth_map, pred_depth_map, min_depth=0.1, max_depth=80.0):
    """Trainer.compute_depth_errors (model/training.py:126-154): one map each, the median scaling, no clamp.
    Returns (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3) as floats."""
    g, p = _depth_map(gt_depth_map, "compute_depth_errors"), _depth_map(pred_depth_map, "compute_depth_errors")
    return tuple(_depth_errors(g[None], p[None], min_depth, max_depth, False)[0, :7].tolist())


# ---------------------------------------------------------------------------
# pose metrics (host, float64)
def _np_poses(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3 or x.shape[1] not in (3, 4) or x.shape[2] != 4:
        raise ValueError(f"poses must be [N, 3 or 4, 4], got {x.shape}")
    return x


def umeyama(model, data):
    """(s, R, t) minimising sum |model_i - (s R data_i + t)|^2 over similarities (Umeyama 1991; the
    reference's ATE/align_trajectory.py:28-80), with the reflection fix S[2, 2] = -1 where
    det(U) det(V) < 0.  model, data: [n, 3]."""
    mu_m, mu_d = model.mean(0), data.mean(0)
    mc, dc = model - mu_m, data - mu_d
    n = model.shape[0]
    C = mc.T @ dc / n
    sigma2 = (dc * dc).sum() / n
    U, D, Vt = np.linalg.svd(C)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    s = np.trace(np.diag(D) @ S) / sigma2
    t = mu_m - s * (R @ mu_d)
    return s, R, t


def align_ate_c2b_use_a2b(traj_a, traj_b, traj_c=None):
    """utils_poses/align_traj.py:26-69: align c (default a) to b by the sim(3) that takes the camera
    positions of a to those of b.  The reference computes the quaternions of both trajectories and never
    uses them (ATE/align_utils.py:99-108): the positions alone decide.  [N, 3 or 4, 4] in, [N, 4, 4] out --
    a float64 tensor on traj_a's device for tensor input, else a numpy array."""
    a, b = _np_poses(traj_a), _np_poses(traj_b)
    c = a if traj_c is None else _np_poses(traj_c)
    s, R, t = umeyama(b[:, :3, 3], a[:, :3, 3])
    out = np.tile(np.eye(4), (c.shape[0], 1, 1))
    out[:, :3, :3] = R[None] @ c[:, :3, :3]
    out[:, :3, 3] = s * (c[:, :3, 3] @ R.T) + t
    if torch.is_tensor(traj_a):
        return torch.from_numpy(out).to(traj_a.device)
    return out


def compute_ATE(gt, pred):
    """utils_poses/comp_ate.py:52-73: the RMSE of the camera-position differences."""
    gt, pred = _np_poses(gt), _np_poses(pred)
    d = gt[:, :3, 3] - pred[:, :3, 3]
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


def compute_rpe(gt, pred):
    """utils_poses/comp_ate.py:33-50: the mean translation and rotation (radians) errors of the relative
    poses of consecutive frames."""
    gt, pred = _np_poses(gt), _np_poses(pred)
    if gt.shape[1] != 4 or pred.shape[1] != 4:
        raise ValueError("compute_rpe: [N, 4, 4] poses expected")
    trans, rot = [], []
    for i in range(len(gt) - 1):
        gt_rel = np.linalg.inv(gt[i]) @ gt[i + 1]
        pred_rel = np.linalg.inv(pred[i]) @ pred[i + 1]
        err = np.linalg.inv(gt_rel) @ pred_rel
        trans.append(np.sqrt(np.sum(err[:3, 3] ** 2)))
        rot.append(np.arccos(max(min(0.5 * (err[0, 0] + err[1, 1] + err[2, 2] - 1.0), 1.0), -1.0)))
    return float(np.mean(trans)), float(np.mean(rot))


def compute_pose_error(pred_poses, gt_poses):
    """Trainer.compute_pose_error (train.py:169-178): (aligned poses, rpe_trans * 100, rpe_rot in degrees,
    ate).  The callable perform_pose_refinement takes as compute_pose_error_fn."""
    aligned = align_ate_c2b_use_a2b(pred_poses, gt_poses)
    ate = compute_ATE(gt_poses, aligned)
    rpe_trans, rpe_rot = compute_rpe(gt_poses, aligned)
    return aligned, rpe_trans * 100, rpe_rot * 180 / np.pi, ate


# ---------------------------------------------------------------------------
# the evaluator
def evaluate(renderer, views, *, depth_range=(0.01, 5.0), cos_anneal_ratio=1.0, it=0, gt_poses=None,
             pred_poses=None, gt_depths=None, lpips_fn=None, chunk=65536, min_depth=0.1, max_depth=80.0):
    """Evaluator.eval's metric part (eval.py:258-267).  views: one dict per test view with "camera_mat",
    "world_mat" (the view's optimised pose, world to camera), "time_step", "image" (the ground truth,
    [H, W, 3] on the device) and optionally "scale_mat" (default: identity).  Every view is rendered with
    inference.render_image at its image's size; the colour and depth maps stay on the device.
      image metrics  always ("PSNR", "SSIM", and "LPIPS" with lpips_fn);
      pose metrics   "rpe_trans", "rpe_rot", "ate" when gt_poses and pred_poses (camera to world,
                     [N, 4, 4]) are given;
      depth metrics  the seven depth errors when gt_depths (one map per view) holds depth.
    Returns the merged dict in the reference's order."""
    from .inference import render_image
    rgb, depth, gts = [], [], []
    with torch.no_grad():
        for v in views:
            img = v["image"]
            dev = img.device
            scale = v.get("scale_mat")
            if scale is None:
                scale = torch.eye(4, device=dev)
            out = render_image(renderer, v["camera_mat"], v["world_mat"], scale, tuple(img.shape[:2]),
                               torch.as_tensor(v["time_step"]), depth_range=depth_range,
                               cos_anneal_ratio=cos_anneal_ratio, it=it, chunk=chunk)
            rgb.append(out["rgb"])
            depth.append(out["depth"])
            gts.append(img)
        result = dict(image_metrics(rgb, gts, lpips_fn=lpips_fn))
        if gt_poses is not None and pred_poses is not None:
            _, rpe_trans, rpe_rot, ate = compute_pose_error(pred_poses, gt_poses)
            result.update({"rpe_trans": rpe_trans, "rpe_rot": rpe_rot, "ate": ate})
        if gt_depths is not None:
            d = depth_metrics(gt_depths, depth, min_depth=min_depth, max_depth=max_depth)
            if d is not None:
                result.update(d)
    return result


def write_results(path, result):
    """results.txt as eval.py:268-270 writes it: one "key: value" line per entry, in the dict's order."""
    with open(path, "w") as f:
        for key, value in result.items():
            f.write(f"{key}: {value}\n")
