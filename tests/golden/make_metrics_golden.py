"""Generate tests/golden/metrics.npz by running the REFERENCE's metric code.

    python tests/golden/make_metrics_golden.py     # needs the reference checkout (COPENERF_REFERENCE)

co3d_metric.py cannot be imported where the fixtures are made (its LPIPS import needs torchvision), so psnr,
ssim, _ssim, gaussian and create_window are parsed out of its source text and compiled unmodified, as
make_pose_refine_golden.py does; Trainer.compute_depth_errors comes out of train.py the same way.
utils_poses.align_traj and utils_poses.comp_ate import as they are.  Every file is pinned by its sha256.

  image   psnr / ssim in float64 on 2 x 3 x 9 x 13 and 1 x 3 x 23 x 31 images (batched, and unbatched per image
          as eval.py:204-205 calls them); the SSIM map is what _ssim takes the mean of, recorded as it does;
  depth   one 12 x 16 map with zeros and out-of-range values, the masking, median ratio and clamp of
          eval.py:234-240 around the reference's compute_depth_errors, with and without the clamp;
  pose    a 12-pose trajectory seen through a known sim(3) plus noise, through train.py:169-178's lines.
The fixture holds numbers only.
"""
from __future__ import annotations

import ast
import hashlib
import os
import sys
from math import exp
from unittest import mock

import numpy as np
import torch
import torch.nn.functional as F
from torch.autograd import Variable

REF = os.environ.get("COPENERF_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(OUT), os.path.dirname(os.path.dirname(OUT))]  # tests/ and the repository root

PINNED = {
    "co3d_metric.py": "58ff0cd1925608f24d2cc94e423f5886366ad316aa21a9aa2fc7640b21991651",
    "train.py": "145aa03d8103d27fd00ba9e6255fa03b1d78313da3a88b671373e162acc16ab6",
    "utils_poses/align_traj.py": "ea511b282be9feec297e20458061aa45f9a3c8b7628e83c1c2fb3a34562a7c09",
    "utils_poses/comp_ate.py": "31590d86e372696742e32500ff7252d4cd1905ddf76ece745732fbeea49836e2",
    "ATE/align_trajectory.py": "8fd49365755a5d793676b3615f31388c9bcc02978555b327f05369b29b521a6c",
    "ATE/align_utils.py": "dbb398898218142003aba90533bff7f323060e62b8f68b93ef5328df843b27c8",
}


def _ref_text(rel):
    with open(os.path.join(REF, rel), "rb") as f:
        raw = f.read()
    got = hashlib.sha256(raw).hexdigest()
    if got != PINNED[rel]:
        raise SystemExit(f"{rel}: sha256 {got} differs from the pinned snapshot; nothing was run")
    return raw.decode()


def load_reference_functions():
    names = ("psnr", "ssim", "_ssim", "gaussian", "create_window")
    tree = ast.parse(_ref_text("co3d_metric.py"))
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(fns) == len(names)
    cls = next(n for n in ast.parse(_ref_text("train.py")).body if isinstance(n, ast.ClassDef) and n.name == "Trainer")
    dep = next(f for f in cls.body if isinstance(f, ast.FunctionDef) and f.name == "compute_depth_errors")
    ns = {"torch": torch, "np": np, "F": F, "exp": exp, "Variable": Variable}
    exec(compile(ast.fix_missing_locations(ast.Module(body=fns + [dep], type_ignores=[])), REF, "exec"), ns)
    for rel in PINNED:
        _ref_text(rel)
    sys.path.insert(0, REF)
    from utils_poses.align_traj import align_ate_c2b_use_a2b
    from utils_poses.comp_ate import compute_ATE, compute_rpe
    ns.update(align_ate_c2b_use_a2b=align_ate_c2b_use_a2b, compute_ATE=compute_ATE, compute_rpe=compute_rpe)
    return ns


def ssim_with_map(ns, a, b):
    """ssim(a, b) and the map it averaged: Tensor.mean is watched for the call, the reference's text is not
    touched."""
    seen = []
    real = torch.Tensor.mean

    def watch(self, *args, **kw):
        seen.append(self)
        return real(self, *args, **kw)

    with mock.patch.object(torch.Tensor, "mean", watch):
        val = ns["ssim"](a, b)
    assert len(seen) == 1 and seen[0].shape == a.shape
    return val, seen[0]


def image_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(*shape, generator=g, dtype=torch.float64)
    pred = (gt + 0.1 * torch.randn(*shape, generator=g, dtype=torch.float64)).clamp(0, 1)
    return pred, gt


def depth_inputs(seed=5):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 20.0, (12, 16))
    gt[0, :5] = 0.0          # no measurement
    gt[3, 2:6] = 95.0        # beyond max_depth
    gt[7, 9] = 0.05          # below min_depth
    pred = gt / 2.5 * np.exp(0.25 * rng.standard_normal((12, 16)))
    pred[gt == 0.0] = 3.0
    pred[5, 5] = 0.001       # clamps to min_depth after scaling
    pred[6, 6] = 500.0       # clamps to max_depth after scaling
    return gt, pred


def pose_inputs(seed=11):
    import metrics_ref as M
    gt = M.trajectory(12, seed)
    rng = np.random.default_rng(seed + 1)
    R = M.rodrigues([0.4, -0.7, 0.9])
    pred = M.apply_sim3(gt, 1.0 / 2.7, R.T, np.array([0.3, -1.1, 0.6]))
    pred[:, :3, 3] += 0.01 * rng.standard_normal((12, 3))
    for i in range(12):
        pred[i, :3, :3] = pred[i, :3, :3] @ M.rodrigues(0.01 * rng.standard_normal(3))
    return gt, pred


def main():
    ns = load_reference_functions()
    out = {}
    for tag, shape, seed in (("a", (2, 3, 9, 13), 1), ("b", (1, 3, 23, 31), 2)):
        pred, gt = image_inputs(shape, seed)
        val, smap = ssim_with_map(ns, pred, gt)
        out[f"img_{tag}_pred"], out[f"img_{tag}_gt"] = pred, gt
        out[f"img_{tag}_ssim"], out[f"img_{tag}_ssim_map"] = val, smap
        out[f"img_{tag}_ssim_per_image"] = ns["ssim"](pred, gt, size_average=False)
        out[f"img_{tag}_psnr"] = ns["psnr"](pred, gt)                                            # [N, 1]
        out[f"img_{tag}_psnr_unbatched"] = torch.stack([ns["psnr"](p, g) for p, g in zip(pred, gt)])  # [N, 3, 1]
        out[f"img_{tag}_ssim_unbatched"] = torch.stack([ns["ssim"](p, g) for p, g in zip(pred, gt)])  # [N]
    gt, pred = depth_inputs()
    valid = (gt >= 0.1) & (gt <= 80)                      # eval.py:234-240
    g, p = gt[valid], pred[valid]
    ratio = np.median(g) / np.median(p)
    p = p * ratio
    out["depth_gt"], out["depth_pred"], out["depth_ratio"] = gt, pred, np.float64(ratio)
    out["depth_errors_noclamp"] = np.array(ns["compute_depth_errors"](None, g, p), dtype=np.float64)
    p = p.copy()
    p[p < 0.1] = 0.1
    p[p > 80] = 80
    out["depth_errors_clamp"] = np.array(ns["compute_depth_errors"](None, g, p), dtype=np.float64)
    gt_poses, pred_poses = pose_inputs()
    pt, gtt = torch.from_numpy(pred_poses), torch.from_numpy(gt_poses)
    aligned = ns["align_ate_c2b_use_a2b"](pt.detach().cpu(), gtt.detach().cpu())   # train.py:169-178
    ate = ns["compute_ATE"](gtt.cpu().numpy(), aligned.cpu().numpy())
    trans_errors, rot_errors = ns["compute_rpe"](gtt.cpu().numpy(), aligned.cpu().numpy())
    rpe_trans, rpe_rot = np.mean(trans_errors) * 100, np.mean(rot_errors) * 180 / np.pi
    out.update(pose_gt=gt_poses, pose_pred=pred_poses, pose_aligned=aligned, pose_rpe_trans=np.float64(rpe_trans),
               pose_rpe_rot=np.float64(rpe_rot), pose_ate=np.float64(ate))
    arrays = {k: (v.detach().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(OUT, "metrics.npz"), **arrays)
    print("wrote metrics", {k: (v.shape, str(v.dtype)) for k, v in arrays.items()})


if __name__ == "__main__":
    main()
