"""Evaluation metrics: what the reference's Evaluator computes after rendering (eval.py:190-272).

  image metrics   psnr / ssim with co3d_metric.py's signatures on the fused device pass (cn_image_metrics),
                  image_metrics = Evaluator.image_eval (eval.py:190-221);
  LPIPS           co3d_metric.lpips(net_type="vgg") on the device (cn_lpips) from the user's two weight files:
                  load_lpips_weights, LPIPS;
  depth metrics   depth_metrics = Evaluator.depth_eval (eval.py:223-244) and compute_depth_errors
                  (model/training.py:126-154) on cn_depth_errors, the median ratio computed on the device;
  pose metrics    align_ate_c2b_use_a2b, compute_ATE, compute_rpe, compute_pose_error (train.py:169-178,
                  utils_poses/align_traj.py, utils_poses/comp_ate.py, ATE/align_trajectory.py) in float64
                  numpy on the host: a few dozen 4 x 4 matrices, control plane;
  geometry        nearest_distances (exact nearest neighbour between two clouds: cn_nn_grid_build /
                  cn_nn_query) and mesh_geometry_metrics (Chamfer distance in the DTU style, precision /
                  recall / F-score in the Tanks and Temples style) on the device; the reference has none;
  registration    icp_register / icp_register_stages (ICP of a cloud onto a target cloud: cn_cloud_transform,
                  the nearest-neighbour query and cn_icp_accumulate on the device, icp_solve_point /
                  icp_solve_plane in float64 on the host), which mesh_geometry_metrics(icp=...) refines its
                  transform with, as the Tanks and Temples protocol does;
  evaluate        render the test views (inference.render_image), keep the maps on the device, run the
                  above and merge the dictionaries in eval.py:264-267's order; write_results writes
                  results.txt (eval.py:268-270).

LPIPS needs network weights that are not part of this build and are never fetched: the user passes the two
files (a torchvision VGG16 state dict and LPIPS v0.1's vgg.pth) to load_lpips_weights, and LPIPS(weights) is
the lpips_fn(pred, gt) (both [3, H, W]) that gives the "LPIPS" key; without an lpips_fn the key is absent.

The image and depth kernels have no CPU path: tensors must live on the device.  Host arrays (numpy, as the
reference's depth loaders give) are uploaded.
"""
from __future__ import annotations

import numpy as np
import torch

import ctypes
import math

from . import _lib, ops

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
# LPIPS (VGG16 features, the v0.1 linear heads)
LPIPS_WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
LPIPS_TAP_CHANNELS = (64, 128, 256, 512, 512)
_VGG_FEATURES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)  # torchvision's features.N of the 13 convolutions


def _state_dict(path):
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        raise ValueError(f"load_lpips_weights: {path} is not a weights-only state dict ({type(e).__name__}: {e})") from e
    if not isinstance(sd, dict):
        raise ValueError(f"load_lpips_weights: {path} holds a {type(sd).__name__}, not a state dict")
    return sd


def _entry(sd, path, key, shape):
    t = sd.get(key)
    if not torch.is_tensor(t):
        raise KeyError(f"load_lpips_weights: {path} has no tensor {key!r}")
    if tuple(t.shape) != shape:
        raise ValueError(f"load_lpips_weights: {path}: {key!r} is {tuple(t.shape)}, expected {shape}")
    return t.detach().float()


def lpips_conv_matrix(w, kpad=None):
    """A convolution weight [Cout, Cin, 3, 3] as cn_lpips' GEMM operand [Cout, Kpad]: column
    (dy 3 + dx) Cin + c, zero columns up to kpad (default 9 Cin rounded up to 32)."""
    cout, cin = w.shape[:2]
    k = 9 * cin
    kpad = ops.rup(k, 32) if kpad is None else kpad
    out = torch.zeros(cout, kpad, dtype=w.dtype, device=w.device)
    out[:, :k] = w.permute(0, 2, 3, 1).reshape(cout, k)
    return out


def load_lpips_weights(vgg_path, lin_path):
    """The LPIPS network from the user's two files (both loaded with weights_only=True; nothing is fetched):
      vgg_path  torchvision's VGG16 state dict: features.{0, 2, 5, ..., 28}.weight [Cout, Cin, 3, 3] / .bias;
      lin_path  LPIPS v0.1's vgg.pth: lin{0..4}.model.1.weight [1, C, 1, 1].
    Every shape is checked; a missing or mis-shaped entry raises with its key.  Returns host tensors:
    {"conv": 13 x [Cout, Kpad] (lpips_conv_matrix), "bias": 13 x [Cout], "lin": 5 x [C]}."""
    vgg, lin = _state_dict(vgg_path), _state_dict(lin_path)
    conv, bias, cin = [], [], 3
    for i, cout in zip(_VGG_FEATURES, LPIPS_WIDTHS):
        conv.append(lpips_conv_matrix(_entry(vgg, vgg_path, f"features.{i}.weight", (cout, cin, 3, 3))))
        bias.append(_entry(vgg, vgg_path, f"features.{i}.bias", (cout,)).contiguous())
        cin = cout
    lins = [_entry(lin, lin_path, f"lin{t}.model.1.weight", (1, c, 1, 1)).reshape(c).contiguous()
            for t, c in enumerate(LPIPS_TAP_CHANNELS)]
    return {"conv": conv, "bias": bias, "lin": lins}


class LPIPS:
    """co3d_metric.lpips(pred, gt, net_type="vgg") on the device (cn_lpips): images in [0, 1], no rescale.
    weights: load_lpips_weights' dict.  mode: the convolutions' MFMA format, "bf16x6" (fp32 results from bf16
    terms, the default), "bf16" or "fp32".  The weights are packed once; a workspace is kept per image size.
    Usable directly as image_metrics' / evaluate's lpips_fn.  There is no CPU path."""

    def __init__(self, weights, mode="bf16x6", device=None, band_rows=0):
        if mode not in ops.FORMATS:
            raise ValueError(f"LPIPS: mode must be one of {tuple(ops.FORMATS)} (got {mode!r})")
        self.mode, self.band_rows = mode, int(band_rows)
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise RuntimeError(f"LPIPS: needs a HIP device (got {self.device}); the kernels have no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if [tuple(w.shape) for w in weights["conv"]] != [(c, 32 if l == 0 else 9 * LPIPS_WIDTHS[l - 1])
                                                         for l, c in enumerate(LPIPS_WIDTHS)]:
            raise ValueError("LPIPS: weights['conv'] must hold load_lpips_weights' 13 matrices")
        with torch.cuda.device(self.device):
            pk = ops.ImagePacker(mode)
            self.images = []
            for l, w in enumerate(weights["conv"]):
                kpad = 64 if (l == 0 and mode == "bf16") else w.shape[1]
                img = pk.image(ops.rup(w.shape[0], 128), kpad, self.device)
                self.images.append(pk.put(img, w.to(self.device).contiguous()))
            pk.run()
        self.bias = [b.to(self.device).float().contiguous() for b in weights["bias"]]
        self.lin = [v.to(self.device).float().contiguous() for v in weights["lin"]]
        self._ws = {}

    def _workspace(self, H, W):
        ws = self._ws.get((H, W))
        if ws is None:
            need = int(_lib.load().cn_lpips_workspace_bytes(H, W, self.band_rows, ops.FORMATS[self.mode]))
            if need == 0:
                raise ValueError(f"LPIPS: images of {H} x {W} (each side at least 16): {_lib.load().cn_last_error().decode()}")
            ws = self._ws[(H, W)] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def _terms(self, pred, gt):
        a, b = _batched(pred, gt, "LPIPS")
        for t in (a, b):
            if not t.is_cuda or t.device != self.device or t.dtype != torch.float32 or t.shape[1] != 3:
                raise RuntimeError(f"LPIPS: fp32 [3, H, W] or [N, 3, H, W] tensors on {self.device} expected (got "
                                   f"{t.dtype} {tuple(t.shape)} on {t.device}); the kernels have no CPU fallback")
        N, _, H, W = a.shape
        ws = self._workspace(H, W)
        out = torch.empty(N, 6, device=self.device, dtype=torch.float32)
        d = _lib.LpipsDesc()
        d.H, d.W, d.mfma_dtype, d.band_rows = H, W, ops.FORMATS[self.mode], self.band_rows
        for l in range(_lib.LPIPS_CONVS):
            d.weights[l], d.bias[l] = self.images[l].data_ptr(), self.bias[l].data_ptr()
        for t in range(_lib.LPIPS_TAPS):
            d.lin[t] = self.lin[t].data_ptr()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        for i in range(N):  # one pair per call: the pairs share the workspace, in the stream's order
            d.pred, d.gt, d.out = a[i].data_ptr(), b[i].data_ptr(), out[i].data_ptr()
            _lib.call("cn_lpips", ctypes.byref(d), ws.data_ptr(), ws.numel(), stream)
        return out

    def layers(self, pred, gt):
        """The five per-block terms of every pair: [N, 5] on the device."""
        return self._terms(pred, gt)[:, :5]

    def __call__(self, pred, gt):
        """[N] on the device: per pair the fp32 sum of the five terms in block order."""
        return self._terms(pred, gt)[:, 5]


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
# normal metrics
NORMAL_KEYS = ("mean", "median", "rmse", "a11.25", "a22.5", "a30")


def normal_metrics(pred, gt, mask=None):
    """The angular error between normal maps, the table of the surface-normal literature: pred, gt [h, w, 3] or
    [B, h, w, 3] device tensors (the same frame; any length), mask [h, w] / [B, h, w] bool or uint8.  Per image, over
    the pixels where the mask is set and both normals have a finite non-zero length (cn_normal_errors): the mean,
    median and root-mean-square angle in degrees and the share of pixels below 11.25, 22.5 and 30 degrees; the
    median is taken over the kernel's angle buffer on the device by np.median's rule.  Returns the means of the
    per-image values over the images that have a valid pixel, or None when none has one."""
    if pred.dim() == 3:
        pred, gt, mask = pred[None], gt[None], None if mask is None else mask[None]
    if pred.dim() != 4 or pred.shape[-1] != 3 or gt.shape != pred.shape or (mask is not None and mask.shape != pred.shape[:3]):
        raise ValueError(f"normal_metrics: maps [h, w, 3] or [B, h, w, 3] and a mask [h, w] or [B, h, w] (got "
                         f"{tuple(pred.shape)}, {tuple(gt.shape)}, {None if mask is None else tuple(mask.shape)})")
    rows = []
    for b in range(pred.shape[0]):
        m = None if mask is None else mask[b].reshape(-1).contiguous()
        angle, sums = ops.normal_errors(pred[b].reshape(-1, 3).float().contiguous(), gt[b].reshape(-1, 3).float().contiguous(), m)
        s = torch.where(torch.isnan(angle), torch.full((), float("inf"), device=angle.device), angle).sort().values
        n, tot, sq, c11, c22, c30 = sums.tolist()
        n = int(n)
        if n == 0:
            continue
        med = (s[(n - 1) // 2].double() + s[n // 2].double()) / 2
        rows.append([tot / n, float(med), math.sqrt(sq / n), c11 / n, c22 / n, c30 / n])
    if not rows:
        return None
    return dict(zip(NORMAL_KEYS, np.asarray(rows, dtype=np.float64).mean(0).tolist()))


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
# geometry metrics (device)
GEOMETRY_KEYS = ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore", "n_pred", "n_gt",
                 "n_pred_far", "n_gt_far", "area")
NN_TARGETS_PER_CELL = 8
# nearest_distances' default for sort_queries: the arm tools/mesh_eval_bench.py measured as faster
# (profiles/mesh_eval_bench.json)
SORT_QUERIES_DEFAULT = True


def nn_cell_size(lo, hi, n, per_cell=NN_TARGETS_PER_CELL, max_cells=ops.NN_MAX_CELLS):
    """(cell, dims) of the grid nearest_distances lays over n targets in the box lo .. hi: cubic cells that
    hold per_cell targets on average over the box (axes of zero extent count as one cell thick), the edge
    enlarged until the grid has at most max_cells cells.  dims covers the box: hi falls in the last cell."""
    ext = [max(float(h) - float(l), 0.0) for l, h in zip(lo, hi)]
    live = [e for e in ext if e > 0.0]
    if not live:
        return 1.0, (1, 1, 1)
    cell = (math.prod(live) * per_cell / max(int(n), 1)) ** (1.0 / len(live))
    cell = max(cell, max(live) * 2.0 ** -20, 1e-30)
    while True:
        dims = tuple(int(e / cell) + 1 for e in ext)
        cells = dims[0] * dims[1] * dims[2]
        if cells <= max_cells:
            return cell, dims
        cell *= max((cells / max_cells) ** (1.0 / len(live)), 1.0 + 2.0 ** -10)


def nearest_distances(queries, targets, max_dist=math.inf, cell=None, sort_queries=None):
    """(dist fp32 [Q], index int32 [Q]): for every query the distance to and the index of its nearest target,
    exact (a uniform grid over the targets searched in Chebyshev shells: cn_nn_grid_build / cn_nn_query), ties
    to the smaller index; (max_dist, -1) where no target is nearer than max_dist.  queries [Q, 3] and targets
    [N, 3] are fp32 device tensors.  cell: the grid's cell edge, by default nn_cell_size's (about 8 targets per
    cell); the grid covers the targets' bounding box (one 24-byte read-back).  sort_queries (default
    SORT_QUERIES_DEFAULT) bins the queries through the same counting sort on the targets' grid first, so that a
    wave's lanes walk neighbouring cells; the outputs are bitwise the same either way."""
    ops._need_cloud("nearest_distances", queries, "queries")
    ops._need_cloud("nearest_distances", targets, "targets")
    if queries.device != targets.device:
        raise RuntimeError("nearest_distances: queries and targets on different devices")
    if sort_queries is None:
        sort_queries = SORT_QUERIES_DEFAULT
    N, Q = targets.shape[0], queries.shape[0]
    if N == 0:
        return (torch.full((Q,), float(max_dist), dtype=torch.float32, device=queries.device),
                torch.full((Q,), -1, dtype=torch.int32, device=queries.device))
    box = torch.stack([targets.amin(0), targets.amax(0)]).tolist()
    if not all(math.isfinite(x) for x in box[0] + box[1]):
        raise ValueError("nearest_distances: targets must be finite")
    if cell is None:
        cell, dims = nn_cell_size(box[0], box[1], N)
    else:
        cell = float(cell)
        if not cell > 0.0:
            raise ValueError(f"nearest_distances: cell {cell}")
        dims = tuple(int((h - l) / cell) + 1 for l, h in zip(*box))
        if dims[0] * dims[1] * dims[2] > ops.NN_MAX_CELLS:
            raise ValueError(f"nearest_distances: cell {cell} gives {dims} cells, more than 2^26")
    grid = ops.nn_grid(targets, box[0], cell, dims)
    if sort_queries and Q > 0:
        binned = ops.nn_grid(queries, box[0], cell, dims)
        return ops.nn_query(grid, binned.sorted, max_dist, records=True)
    return ops.nn_query(grid, queries, max_dist)


def knn(queries, targets, k, max_dist=math.inf, exclude_self=False):
    """(dist fp32 [Q, k], index int32 [Q, k]): for every query its k nearest targets (1 <= k <= 32), exact, each row
    ascending under (distance, index) and padded with (max_dist, -1) where fewer than k targets are nearer than
    max_dist (cn_knn_query on nearest_distances' grid, the queries binned through it).  exclude_self: queries is
    targets, and no point is its own neighbour (exact duplicates at other indices still are)."""
    ops._need_cloud("knn", queries, "queries")
    ops._need_cloud("knn", targets, "targets")
    if queries.device != targets.device:
        raise RuntimeError("knn: queries and targets on different devices")
    k = int(k)
    if not 1 <= k <= ops.KNN_MAX_K:
        raise ValueError(f"knn: k {k} (in [1, {ops.KNN_MAX_K}])")
    N, Q = targets.shape[0], queries.shape[0]
    if exclude_self and Q != N:
        raise ValueError(f"knn: exclude_self with {Q} queries of {N} targets")
    if N == 0 or Q == 0:
        return (torch.full((Q, k), float(max_dist), dtype=torch.float32, device=queries.device),
                torch.full((Q, k), -1, dtype=torch.int32, device=queries.device))
    box = torch.stack([targets.amin(0), targets.amax(0)]).tolist()
    if not all(math.isfinite(x) for x in box[0] + box[1]):
        raise ValueError("knn: targets must be finite")
    cell, dims = nn_cell_size(box[0], box[1], N)
    grid = ops.nn_grid(targets, box[0], cell, dims)
    binned = grid if queries is targets else ops.nn_grid(queries, box[0], cell, dims)
    dist, index, _ = ops.knn_query(grid, binned.sorted, k, max_dist, exclude_self=exclude_self, records=True)
    return dist, index


def voxel_down_sample(points, voxel, normals=None, colors=None, origin=None):
    """Voxel down-sampling as the Tanks-and-Temples protocol applies it: one point per occupied voxel of edge `voxel`,
    the mean of the voxel's points (and of their colors fp32 [N, 3]; normals are averaged and re-normalised, a zero
    sum staying zero), in ascending voxel-key order (cn_voxel_keys, a stable torch sort, cn_voxel_reduce; double
    sums in ascending original index, bitwise repeatable).  origin (3 numbers) anchors the voxel lattice, by default
    the smallest finite coordinate per axis.  Points that are not finite, or farther than 2^21 voxels from the
    origin, are dropped and counted.  Returns a dict: points, normals, colors (None where not given), counts int32
    [M], n_dropped."""
    ops._need_cloud("voxel_down_sample", points, "points")
    voxel = float(voxel)
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError(f"voxel_down_sample: voxel size {voxel}")
    N = points.shape[0]
    if origin is None:
        finite = torch.where(torch.isfinite(points), points, torch.full_like(points, math.inf))
        origin = finite.amin(0).tolist() if N else [0.0, 0.0, 0.0]
        origin = [x if math.isfinite(x) else 0.0 for x in origin]
    keys, _ = ops.voxel_keys(points, origin, voxel)
    skeys, order = torch.sort(keys, stable=True)
    out = ops.voxel_reduce(skeys, order, points, normals, colors)
    M, dropped = out["totals"].tolist()
    return {"points": out["points"][:M].contiguous(),
            "normals": None if normals is None else out["normals"][:M].contiguous(),
            "colors": None if colors is None else out["colors"][:M].contiguous(),
            "counts": out["counts"][:M].contiguous(), "n_dropped": int(dropped)}


def estimate_normals(points, k=16, max_dist=math.inf, orient_to=None, want_variation=False):
    """Normals of a cloud without them: per point the PCA normal of its k nearest neighbours within max_dist, the
    point itself included (knn over the cloud, cn_cloud_normals).  A point with fewer than 3 neighbours, or a
    collinear neighbourhood, gets the zero normal, which the normal metrics and point-to-plane ICP leave out and
    count.  orient_to: a viewpoint the normals are flipped towards; without it the sign is a convention (the largest
    component positive) -- the normal metrics take |n . n'|, and point-to-plane ICP is sign-free.  Returns normals
    fp32 [N, 3], or (normals, surface variation fp32 [N])."""
    _, index = knn(points, points, k, max_dist)
    normals, variation = ops.cloud_normals(points, index, orient_to, want_variation)
    return (normals, variation) if want_variation else normals


def outlier_cut(sums, std_ratio):
    """(mu, sigma, mu + std_ratio sigma) from cn_knn_mean_stats' three sums (the population standard deviation)."""
    n, s, s2 = (float(x) for x in sums)
    if n < 1:
        return 0.0, 0.0, 0.0
    mu = s / n
    sigma = math.sqrt(max(s2 / n - mu * mu, 0.0))
    return mu, sigma, mu + float(std_ratio) * sigma


def remove_statistical_outliers(points, k=20, std_ratio=2.0):
    """The statistical outlier filter of scan pipelines: a point goes when the mean distance to its k nearest
    neighbours (itself excluded) is above mu + std_ratio sigma of those means over the cloud.  Returns (the kept
    points, the keep mask bool [N])."""
    dist, index = knn(points, points, k, exclude_self=True)
    mean, sums = ops.knn_mean_stats(dist, index)
    _, _, cut = outlier_cut(sums.tolist(), std_ratio)
    keep = mean <= cut
    return points[keep].contiguous(), keep


def _cloud_side(queries, targets, threshold, max_dist, crop_min, crop_max):
    dist, _ = nearest_distances(queries, targets, max_dist)
    return ops.cloud_stats(dist, threshold, max_dist, queries if crop_min is not None else None, crop_min, crop_max)


def _cloud_side_normals(queries, targets, threshold, max_dist, crop_min, crop_max, query_normals, target_normals):
    """_cloud_side's statistics and cloud_normal_stats of the same pairs, from one nearest-neighbour search."""
    dist, index = nearest_distances(queries, targets, max_dist)
    pts = queries if crop_min is not None else None
    return (ops.cloud_stats(dist, threshold, max_dist, pts, crop_min, crop_max),
            ops.cloud_normal_stats(query_normals, target_normals, index, dist, max_dist, pts, crop_min, crop_max))


NORMAL_GEOMETRY_KEYS = ("normal_accuracy", "normal_completeness", "normal_consistency", "n_pred_normal", "n_gt_normal")


def normal_geometry_from_stats(pred, gt):
    """The normal-consistency entries from the two cn_cloud_normal_stats results (pairs counted, sum of |cos|,
    pairs left out), mesh samples first."""
    (cp, sp, _), (cg, sg, _) = pred, gt
    acc = sp / cp if cp else float("nan")
    comp = sg / cg if cg else float("nan")
    return {"normal_accuracy": acc, "normal_completeness": comp, "normal_consistency": 0.5 * (acc + comp),
            "n_pred_normal": int(cp), "n_gt_normal": int(cg)}


def geometry_from_stats(pred, gt, area):
    """The metric dict from the two cn_cloud_stats results (4 numbers each: inside the crop, of those within
    max_dist, the sum of their distances, of those below the threshold), mesh samples first."""
    (np_, npn, sp, hp), (ng, ngn, sg, hg) = pred, gt
    acc = sp / npn if npn else float("nan")
    comp = sg / ngn if ngn else float("nan")
    P = hp / np_ if np_ else 0.0
    R = hg / ng if ng else 0.0
    return {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "precision": P, "recall": R,
            "fscore": 2.0 * P * R / (P + R) if P + R > 0 else 0.0, "n_pred": int(np_), "n_gt": int(ng),
            "n_pred_far": int(np_ - npn), "n_gt_far": int(ng - ngn), "area": area}


# ---------------------------------------------------------------------------
# ICP registration: the solvers (host, float64) and the loop (device passes, one 256-byte read-back each)
ICP_RANK_TOL = 1e-9  # a system whose smallest needed singular / eigen value is below this share of the largest


def icp_solve_point(sums, with_scale=False, pivot=None):
    """The 4 x 4 increment of one point-to-point iteration from cn_icp_accumulate's mode-0 sums (32 numbers; the
    layout is copenerf.h's), taken about `pivot` (3 numbers, default the origin): Kabsch -- with_scale: Umeyama,
    the scale from the source variance -- by a 3 x 3 SVD in float64 with the reflection guard.  The increment
    takes the transformed source p' onto the targets: q ~ s R (p' - pivot - mean_p) + mean_q + pivot.
    ValueError for fewer than 3 pairs and for a source or target set without a plane's worth of spread
    (collinear or coincident points)."""
    s_ = np.asarray(sums, dtype=np.float64).reshape(-1)
    c = np.zeros(3) if pivot is None else np.asarray(pivot, dtype=np.float64).reshape(3)
    n = s_[0]
    if n < 3:
        raise ValueError(f"icp_solve_point: {int(n)} correspondences, at least 3 needed")
    mp, mq = s_[2:5] / n, s_[5:8] / n
    C = s_[8:17].reshape(3, 3) / n - np.outer(mq, mp)
    var = s_[17] / n - mp @ mp
    U, D, Vt = np.linalg.svd(C)
    if not (np.isfinite(D).all() and D[0] > 0.0 and D[1] > ICP_RANK_TOL * D[0] and var > 0.0):
        raise ValueError(f"icp_solve_point: rank-deficient system (singular values {D.tolist()}): the pairs are "
                         "collinear or coincident")
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    scale = float(np.trace(np.diag(D) @ S) / var) if with_scale else 1.0
    M = np.eye(4)
    M[:3, :3] = scale * R
    M[:3, 3] = (mq + c) - scale * (R @ (mp + c))
    return M


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)


def icp_solve_plane(sums, pivot=None):
    """The 4 x 4 increment of one point-to-plane iteration from cn_icp_accumulate's mode-1 sums: the 6 x 6
    normal equations (sum J^T J) x = -(sum J^T r), x = (rotation vector w, translation v), by Cholesky; w is
    turned into an exact rotation (Rodrigues) about `pivot` (default the origin), then v is added:
    p'' = R (p' - pivot) + pivot + v.  ValueError for fewer than 6 pairs and for a rank-deficient system (e.g.
    every normal the same: a single plane fixes 3 of the 6 freedoms)."""
    s_ = np.asarray(sums, dtype=np.float64).reshape(-1)
    c = np.zeros(3) if pivot is None else np.asarray(pivot, dtype=np.float64).reshape(3)
    n = s_[0]
    if n < 6:
        raise ValueError(f"icp_solve_plane: {int(n)} correspondences, at least 6 needed")
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s_[3:24]
    A = A + np.triu(A, 1).T
    b = s_[24:30]
    ev = np.linalg.eigvalsh(A)
    if not (np.isfinite(ev).all() and ev[-1] > 0.0 and ev[0] > ICP_RANK_TOL * ev[-1]):
        raise ValueError(f"icp_solve_plane: rank-deficient system (eigenvalues {ev.tolist()}): the normals do not "
                         "constrain all six freedoms")
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"icp_solve_plane: rank-deficient system ({e})") from None
    x = -np.linalg.solve(L.T, np.linalg.solve(L, b))
    R = _rodrigues(x[:3])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = c - R @ c + x[3:]
    return M


class IcpResult:
    """What icp_register returns: transform (float64 4 x 4 numpy, source frame to target frame), fitness (pairs /
    points used) and inlier_rmse of that transform, iterations (solves applied), converged, and history, the
    (fitness, rmse) every iteration started from."""

    def __init__(self, transform, fitness, inlier_rmse, iterations, converged, history):
        self.transform, self.fitness, self.inlier_rmse = transform, fitness, inlier_rmse
        self.iterations, self.converged, self.history = iterations, converged, history

    def __repr__(self):
        return (f"IcpResult(fitness={self.fitness}, inlier_rmse={self.inlier_rmse}, iterations={self.iterations}, "
                f"converged={self.converged})")


def _mat4(fn, T):
    M = np.array(T.detach().cpu() if torch.is_tensor(T) else T, dtype=np.float64)
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError(f"{fn}: a finite 4 x 4 transform expected, got shape {M.shape}")
    return M


ICP_MODES = {"point": 0, "plane": 1}


def icp_register(source, target, *, max_corr_dist, init=None, mode="point", with_scale=False, target_normals=None,
                 max_iters=50, tol=1e-6, stride=1, cell=None):
    """ICP registration of source fp32 [Q, 3] onto target fp32 [N, 3] (device tensors): the similarity T (rigid
    unless with_scale) that minimises, over the pairs (T p, its nearest target within max_corr_dist), the
    point-to-point distances (mode "point") or the distances to the targets' tangent planes (mode "plane", with
    target_normals fp32 [N, 3], any length).  The target grid is built once (nn_cell_size, as nearest_distances;
    `cell` overrides its edge), the loop starts from `init` (a 4 x 4, default the identity) over source[::stride],
    and an iteration is cloud_transform -> binning the moved cloud on the target's grid -> nn_query on the binned
    records -> icp_accumulate -> one 256-byte read-back -> icp_solve_point / icp_solve_plane about the centre of the
    target's bounding box (a correspondence kernel fused with the transform was measured slower than these three
    calls: DESIGN.md 3.12.6).  T is kept in float64 here and
    composed as T <- dT T; the device gets the fp32 rounding of the current T each time, so rounding does not
    accumulate.  fitness = pairs / points used and inlier_rmse = sqrt(sum |T p - q|^2 / pairs) are those of the
    transform an iteration starts from; the loop stops when both change by less than tol between two consecutive
    iterations (converged, and the transform returned is the one they were measured at), or after max_iters
    solves (then one more pass measures the transform returned).  Returns an IcpResult."""
    fn = "icp_register"
    if mode not in ICP_MODES:
        raise ValueError(f"{fn}: mode {mode!r} (point or plane)")
    if with_scale and mode == "plane":
        raise ValueError(f"{fn}: with_scale needs mode 'point' (the point-to-plane step is rigid)")
    if not max_corr_dist > 0:
        raise ValueError(f"{fn}: max_corr_dist {max_corr_dist}")
    stride, max_iters = int(stride), int(max_iters)
    if stride < 1 or max_iters < 1:
        raise ValueError(f"{fn}: stride {stride}, max_iters {max_iters}")
    ops._need_cloud(fn, source, "source")
    ops._need_cloud(fn, target, "target")
    if mode == "plane":
        if target_normals is None:
            raise ValueError(f"{fn}: mode 'plane' needs target_normals")
        ops._need_cloud(fn, target_normals, "target_normals")
        if target_normals.shape[0] != target.shape[0]:
            raise ValueError(f"{fn}: {target_normals.shape[0]} normals for {target.shape[0]} targets")
    if source.device != target.device:
        raise RuntimeError(f"{fn}: source and target on different devices")
    T = np.eye(4) if init is None else _mat4(fn, init)
    src = source if stride == 1 else source[::stride].contiguous()
    Q, N = src.shape[0], target.shape[0]
    if Q == 0 or N == 0:
        raise ValueError(f"{fn}: {Q} source points and {N} targets")
    box = torch.stack([target.amin(0), target.amax(0)]).tolist()
    if not all(math.isfinite(x) for x in box[0] + box[1]):
        raise ValueError(f"{fn}: the targets must be finite")
    if cell is None:
        cell, dims = nn_cell_size(box[0], box[1], N)
    else:
        cell = float(cell)
        if not cell > 0.0:
            raise ValueError(f"{fn}: cell {cell}")
        dims = tuple(int((h - l) / cell) + 1 for l, h in zip(*box))
        if dims[0] * dims[1] * dims[2] > ops.NN_MAX_CELLS:
            raise ValueError(f"{fn}: cell {cell} gives {dims} cells, more than 2^26")
    grid = ops.nn_grid(target, box[0], cell, dims)
    pivot = [0.5 * (l + h) for l, h in zip(*box)]
    m = ICP_MODES[mode]
    normals = target_normals if m == 1 else None

    def measure(T):
        binned = ops.nn_grid(ops.cloud_transform(src, T), box[0], cell, dims)
        _, index = ops.nn_query(grid, binned.sorted, max_corr_dist, records=True)
        sums = ops.icp_accumulate(src, target, index, T, pivot, m, normals).tolist()
        n = sums[0]
        return sums, n / Q, math.sqrt(sums[1] / n) if n > 0 else float("nan")

    history, converged, iterations = [], False, 0
    while True:
        sums, fitness, rmse = measure(T)
        history.append((fitness, rmse))
        if len(history) > 1 and abs(fitness - history[-2][0]) < tol and abs(rmse - history[-2][1]) < tol:
            converged = True
        if converged or iterations == max_iters:
            break
        try:
            dT = icp_solve_point(sums, with_scale, pivot) if m == 0 else icp_solve_plane(sums, pivot)
        except ValueError as e:
            raise ValueError(f"{fn}: iteration {iterations} ({Q} points, max_corr_dist {max_corr_dist}, fitness "
                             f"{fitness}): {e}") from None
        T = dT @ T
        iterations += 1
    return IcpResult(T, fitness, rmse, iterations, converged, history)


def icp_register_stages(source, target, stages, **common):
    """icp_register once per dict of `stages`, coarse to fine: a stage may override max_corr_dist, stride,
    max_iters and mode, takes everything else from `common`, and starts from the previous stage's transform (the
    first from common's init).  Returns the last stage's IcpResult, its history the stages' histories joined and
    its iterations their sum."""
    stages = list(stages)
    if not stages:
        raise ValueError("icp_register_stages: no stages")
    kw = dict(common)
    history, iterations, res = [], 0, None
    for st in stages:
        extra = set(st) - {"max_corr_dist", "stride", "max_iters", "mode"}
        if extra:
            raise ValueError(f"icp_register_stages: a stage may set max_corr_dist, stride, max_iters and mode, not {sorted(extra)}")
        res = icp_register(source, target, **{**kw, **st})
        kw["init"] = res.transform
        history += res.history
        iterations += res.iterations
    res.history, res.iterations = history, iterations
    return res


ICP_KEYS = ("icp_fitness", "icp_rmse", "icp_iterations", "icp_converged", "transform")


def _apply_transform(vertices, transform, dev):
    M = torch.as_tensor(np.asarray(transform.detach().cpu() if torch.is_tensor(transform) else transform,
                                   dtype=np.float64), dtype=torch.float32).to(dev)
    if M.shape != (4, 4):
        raise ValueError(f"mesh_geometry_metrics: transform must be 4 x 4, got {tuple(M.shape)}")
    return (vertices @ M[:3, :3].T + M[:3, 3]).contiguous()


def _icp_refine(icp, vertices, triangles, gt_points, gt_normals, transform, n_samples, density, seed, dev):
    """mesh_geometry_metrics' registration step: (the composed 4 x 4, the IcpResult).  The registration samples are
    the evaluation sampler's for Philox (seed, offset 4 S), S the evaluation's sample count under the initial
    transform -- the evaluation draws at offset 0, so the two never share a counter."""
    icp = dict(icp)
    stages = icp.pop("stages", None)
    if (stages is None) == ("max_corr_dist" not in icp):
        raise ValueError("mesh_geometry_metrics: icp takes stages or a single max_corr_dist")
    if stages is None:
        stages = [{"max_corr_dist": icp.pop("max_corr_dist")}]
    n_reg = int(icp.pop("n_samples", 0))
    voxel = icp.pop("voxel", None)
    if voxel is not None and not (float(voxel) > 0.0 and math.isfinite(float(voxel))):
        raise ValueError(f"mesh_geometry_metrics: icp voxel {voxel}")
    if n_reg < 1 or n_reg >= 2 ** 31:
        raise ValueError(f"mesh_geometry_metrics: icp n_samples {n_reg}")
    plane = icp.get("mode") == "plane" or any(st.get("mode") == "plane" for st in stages)
    if plane:
        if gt_normals is None:
            raise ValueError("mesh_geometry_metrics: icp mode 'plane' needs gt_normals")
        icp["target_normals"] = gt_normals
    # The mesh is transformed and its area scanned here under the INITIAL transform, for the registration samples, and
    # once more by the caller under the refined one, for the evaluation: two passes over the vertices and triangles,
    # small beside the registration.  With `density` the S that fixes the registration's Philox offset is therefore
    # the initial transform's, while the evaluation's own S comes from the refined area (they differ only when the
    # registration changes the scale).
    base = np.eye(4) if transform is None else _mat4("mesh_geometry_metrics", transform)
    moved = vertices if transform is None else _apply_transform(vertices, transform, dev)
    if triangles.shape[0] == 0:
        raise ValueError("mesh_geometry_metrics: a mesh without triangles")
    handle, area_dev = ops.mesh_area(moved, triangles)
    if n_samples is not None:
        S = int(n_samples)
    else:
        S = int(math.ceil(float(density) * float(area_dev.item())))
    if S < 1 or S >= 2 ** 31:
        raise ValueError(f"mesh_geometry_metrics: {S} samples")
    philox = torch.tensor([int(seed), 4 * S], dtype=torch.uint64, device=dev)
    reg, _ = ops.mesh_sample(handle, n_reg, philox)
    if voxel is not None:
        reg = voxel_down_sample(reg, voxel)["points"]
        down = voxel_down_sample(gt_points, voxel, normals=gt_normals if plane else None)
        gt_points = down["points"]
        if plane:
            icp["target_normals"] = down["normals"]
    res = icp_register_stages(reg, gt_points, stages, **icp)
    return res.transform @ base, res


def _with_icp(res, icp_res, transform):
    if icp_res is not None:
        res.update(zip(ICP_KEYS, (icp_res.fitness, icp_res.inlier_rmse, icp_res.iterations, icp_res.converged,
                                  np.asarray(transform, dtype=np.float64).tolist())))
    return res


def mesh_geometry_metrics(vertices, triangles, gt_points, *, threshold, max_dist=math.inf, n_samples=None,
                          density=None, seed=0, transform=None, crop_min=None, crop_max=None, cull_views=None,
                          cull_resolution=None, cull_gt=False, cull_min_views=1, cull_tol_abs=None, cull_tol_rel=None,
                          gt_normals=None, icp=None, gt_voxel=None, gt_outliers=None, gt_estimate_normals=None):
    """Geometry metrics of a triangle mesh against a ground-truth cloud, all on the device.  vertices fp32
    [V, 3], triangles int32 [T, 3] (NeuSRenderer.extract_geometry's output as it is) and gt_points fp32 [N, 3]
    are device tensors.  The mesh is sampled uniformly by area (cn_mesh_area / cn_mesh_sample, Philox seed
    `seed`) with n_samples points or density points per unit area -- exactly one of the two -- after
    `transform`, a 4 x 4 similarity applied to the vertices (e.g. align_ate_c2b_use_a2b's Sim(3)).  Points
    outside the axis-aligned box crop_min .. crop_max (both or neither) are left out on both sides.
      accuracy      mean distance from the mesh samples to gt_points, over the samples nearer than max_dist;
      completeness  the same from gt_points to the mesh samples;  chamfer = (accuracy + completeness) / 2;
      precision / recall  the share of mesh samples / ground-truth points with distance < threshold (a point
                    farther than max_dist is a miss);  fscore = 2 P R / (P + R), 0 when P + R = 0;
      n_pred, n_gt, n_pred_far, n_gt_far  the points counted on either side and those beyond max_dist;  area.
    The samples and the distances stay on the device; what comes back is the area (8 bytes), the two
    bounding boxes and two double [4] statistics.
    cull_views / cull_resolution (together): the views -- dicts with "camera_mat", "world_mat" and optionally
    "scale_mat", as evaluate takes them, in the mesh's own frame -- and their (h, w).  The mesh is first cut down
    to what at least cull_min_views of them see (mesh.cull_mesh with cull_tol_abs / cull_tol_rel, by default
    cull_mesh's), before `transform` and before sampling, as the ScanNet / DTU / Tanks-and-Temples protocols do.
    cull_gt drops the ground-truth points outside every view's frustum, the cameras taken through `transform`
    into the ground truth's frame.  Without them nothing changes.
    gt_normals fp32 [N, 3] (any length, the ground truth's frame; cull_gt filters them with the points) adds the
    normal consistency: every mesh sample carries the face normal of the (transformed) triangle it was drawn
    from, and over the same pairs as the distance means
      normal_accuracy      mean |n_sample . n_gt[nearest]| from the mesh samples to the ground truth;
      normal_completeness  the same from the ground truth to the mesh samples;  normal_consistency: their mean;
      n_pred_normal, n_gt_normal  the pairs counted (pairs with a zero or non-finite normal are left out).
    Without gt_normals the dict has exactly the keys above.
    icp: a dict with `stages` (a list of icp_register_stages' dicts, coarse to fine) or a single max_corr_dist,
    n_samples (the registration samples) and icp_register's keywords (mode, with_scale, max_iters, tol, stride,
    cell).  After culling and `transform`, n_samples registration samples are drawn from the mesh by the same
    sampler (seed `seed`, Philox offset 4 S with S the evaluation's sample count under `transform`; the evaluation
    draws at offset 0), registered to gt_points (mode "plane" uses gt_normals), the result is composed onto
    `transform`, and everything above goes on with the refined transform.  cull_gt keeps using the initial
    transform: the ground truth is filtered before the registration that refines it.  The dict then gains
    icp_fitness, icp_rmse, icp_iterations, icp_converged and transform (the composed 4 x 4 as nested lists).
    With icp=None nothing changes.
    Preparation of a raw ground-truth scan, all off by default and applied in this order before anything above:
    gt_outliers=(k, ratio) removes its statistical outliers (remove_statistical_outliers; gt_normals follow the
    mask), gt_voxel=V voxel-down-samples it (voxel_down_sample; normals are averaged), gt_estimate_normals=k gives
    a ground truth without normals the PCA normals of its k nearest neighbours (estimate_normals; not together with
    gt_normals), which turns the normal metrics and icp mode "plane" on.  icp's `voxel` down-samples the
    registration samples and the ground truth the registration sees (not the evaluation's) to that voxel size."""
    if gt_estimate_normals is not None and gt_normals is not None:
        raise ValueError("mesh_geometry_metrics: gt_estimate_normals with gt_normals")
    if gt_voxel is not None and not (float(gt_voxel) > 0.0 and math.isfinite(float(gt_voxel))):
        raise ValueError(f"mesh_geometry_metrics: gt_voxel {gt_voxel}")
    if gt_normals is not None:
        ops._need_cloud("mesh_geometry_metrics", gt_normals, "gt_normals")
        if gt_normals.shape[0] != gt_points.shape[0]:
            raise ValueError(f"mesh_geometry_metrics: {gt_normals.shape[0]} normals for {gt_points.shape[0]} points")
    if (n_samples is None) == (density is None):
        raise ValueError("mesh_geometry_metrics: exactly one of n_samples and density")
    if (cull_views is None) != (cull_resolution is None):
        raise ValueError("mesh_geometry_metrics: cull_views and cull_resolution together")
    if cull_gt and cull_views is None:
        raise ValueError("mesh_geometry_metrics: cull_gt needs cull_views")
    if (crop_min is None) != (crop_max is None):
        raise ValueError("mesh_geometry_metrics: crop_min and crop_max together")
    if not threshold > 0 or not max_dist > 0:
        raise ValueError(f"mesh_geometry_metrics: threshold {threshold}, max_dist {max_dist}")
    ops._need_cloud("mesh_geometry_metrics", vertices, "vertices")
    ops._need_cloud("mesh_geometry_metrics", triangles, "triangles", dtype=torch.int32)
    ops._need_cloud("mesh_geometry_metrics", gt_points, "gt_points")
    dev = vertices.device
    if gt_outliers is not None:
        k_out, ratio = gt_outliers
        gt_points, keep = remove_statistical_outliers(gt_points, int(k_out), float(ratio))
        if gt_normals is not None:
            gt_normals = gt_normals[keep].contiguous()
    if gt_voxel is not None:
        down = voxel_down_sample(gt_points, gt_voxel, normals=gt_normals)
        gt_points, gt_normals = down["points"], down["normals"]
    if gt_estimate_normals is not None:
        gt_normals = estimate_normals(gt_points, int(gt_estimate_normals))
    if cull_views is not None:
        from . import mesh
        tol = {k: v for k, v in (("tol_abs", cull_tol_abs), ("tol_rel", cull_tol_rel)) if v is not None}
        vertices, triangles, _ = mesh.cull_mesh(vertices, triangles, cull_views, cull_resolution,
                                                min_views=cull_min_views, **tol)
        if cull_gt:
            h, w = (int(x) for x in cull_resolution)
            seen = ops.mesh_visibility(gt_points, mesh.view_projections(cull_views, (h, w), transform, dev), h, w)
            if gt_normals is not None:
                gt_normals = gt_normals[seen > 0].contiguous()
            gt_points = gt_points[seen > 0].contiguous()
    icp_res = None
    if icp is not None:
        transform, icp_res = _icp_refine(icp, vertices, triangles, gt_points, gt_normals, transform, n_samples, density,
                                         seed, dev)
    if transform is not None:
        vertices = _apply_transform(vertices, transform, dev)
    if triangles.shape[0] == 0:
        raise ValueError("mesh_geometry_metrics: a mesh without triangles")
    handle, area_dev = ops.mesh_area(vertices, triangles)
    area = float(area_dev.item())
    if not area > 0.0:
        raise ValueError("mesh_geometry_metrics: a mesh of zero area")
    S = int(n_samples) if n_samples is not None else int(math.ceil(float(density) * area))
    if S < 1 or S >= 2 ** 31:
        raise ValueError(f"mesh_geometry_metrics: {S} samples")
    philox = torch.tensor([int(seed), 0], dtype=torch.uint64, device=dev)
    samples, sample_tri = ops.mesh_sample(handle, S, philox, want_tri=gt_normals is not None)
    sample_normals = None
    if gt_normals is not None:
        # the face normals at the samples' triangles (cn_cloud_normal_stats normalises them); a sample without a
        # triangle (-1) gets the zero normal and is left out
        corners = vertices[triangles[sample_tri.clamp(min=0).long()].long()]
        sample_normals = torch.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0], dim=-1)
        sample_normals = torch.where((sample_tri >= 0)[:, None], sample_normals, torch.zeros_like(sample_normals)).contiguous()
    if gt_normals is None:
        pred = _cloud_side(samples, gt_points, threshold, max_dist, crop_min, crop_max)
        gt = _cloud_side(gt_points, samples, threshold, max_dist, crop_min, crop_max)
        both = torch.stack([pred, gt]).tolist()
        return _with_icp(geometry_from_stats(both[0], both[1], area), icp_res, transform)
    pred, pred_n = _cloud_side_normals(samples, gt_points, threshold, max_dist, crop_min, crop_max, sample_normals, gt_normals)
    gt, gt_n = _cloud_side_normals(gt_points, samples, threshold, max_dist, crop_min, crop_max, gt_normals, sample_normals)
    both = torch.stack([pred, gt]).tolist()
    res = geometry_from_stats(both[0], both[1], area)
    res.update(normal_geometry_from_stats(*torch.stack([pred_n, gt_n]).tolist()))
    return _with_icp(res, icp_res, transform)


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
