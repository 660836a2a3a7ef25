"""Evaluate a trained model on its test views and write results.txt (copenerf.metrics.evaluate).

    python tools/evaluate.py CHECKPOINT --images test.npy --K K.npy --world-mats w2c.npy --times t.npy --out OUT
        [--scale-mat S.npy] [--depths depths.npy] [--gt-poses gt.npy --pred-poses pred.npy]
        [--depth-range 0.01 5.0] [--chunk 65536] [--mode fp32|bf16x6|bf16]
        [--lpips-vgg vgg16.pth --lpips-lin vgg.pth]

  CHECKPOINT    one train.py wrote through CheckpointIO (see tools/extract_mesh.py)
  --images      .npy (or .npz with `imgs`): float [N, 3, H, W], the test frames (planar, as the reference's)
  --K           .npy (or .npz with `K`): the camera matrix, [4, 4] (or [3, 3], padded to 4 x 4)
  --world-mats  .npy / .pt [N, 4, 4]: the optimised test poses, world to camera (what eval.py:131 looks up)
  --times       .npy [N]: each view's time step in [-1, 1] (eval.py:110)
  --depths      .npy (or .npz with `depths`) [N, h, w]: ground-truth depth, any resolution; without it no depth
                metrics (the reference's `-1`)
  --gt-poses, --pred-poses   .npy / .pt [M, 4, 4] camera-to-world trajectories for the pose metrics
  --lpips-vgg, --lpips-lin   the two LPIPS weight files (both or neither): torchvision's VGG16 state dict and
                LPIPS v0.1's vgg.pth (copenerf.metrics.load_lpips_weights).  Nothing is ever downloaded.

Writes OUT/results.txt in eval.py:268-270's format: PSNR, SSIM, LPIPS (only with the two weight files), then
rpe_trans, rpe_rot, ate, then the seven depth errors."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT, os.path.join(ROOT, "tools")]


def _load(path, key):
    if path.endswith(".pt"):
        return torch.load(path, map_location="cpu").float()
    a = np.load(path)
    if isinstance(a, np.lib.npyio.NpzFile):
        a = a[key]
    return torch.from_numpy(np.asarray(a)).float()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint")
    ap.add_argument("--images", required=True)
    ap.add_argument("--K", required=True)
    ap.add_argument("--world-mats", required=True)
    ap.add_argument("--times", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--scale-mat", default=None)
    ap.add_argument("--depths", default=None)
    ap.add_argument("--gt-poses", default=None)
    ap.add_argument("--pred-poses", default=None)
    ap.add_argument("--depth-range", type=float, nargs=2, default=[0.01, 5.0])
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--mode", choices=["fp32", "bf16x6", "bf16"], default="bf16x6", help="the MLP GEMMs' MFMA mode")
    ap.add_argument("--lpips-vgg", default=None, help="torchvision VGG16 state dict (features.N.weight / bias)")
    ap.add_argument("--lpips-lin", default=None, help="LPIPS v0.1 vgg.pth (linN.model.1.weight)")
    a = ap.parse_args(argv)
    if (a.lpips_vgg is None) != (a.lpips_lin is None):
        raise SystemExit("--lpips-vgg and --lpips-lin go together")
    if not torch.cuda.is_available():
        raise SystemExit("evaluate: needs a HIP device (the kernels have no CPU fallback)")
    from copenerf import metrics
    from extract_mesh import build_renderer
    dev = torch.device("cuda")
    images = _load(a.images, "imgs").to(dev)
    if images.dim() != 4 or images.shape[1] != 3:
        raise SystemExit(f"--images: expected [N, 3, H, W], got {tuple(images.shape)}")
    N = images.shape[0]
    K = _load(a.K, "K")
    if K.shape[-1] == 3:
        K4 = torch.eye(4)
        K4[:3, :3] = K
        K = K4
    world = _load(a.world_mats, "world_mats")
    times = _load(a.times, "times").reshape(-1)
    if world.shape != (N, 4, 4) or times.shape != (N,):
        raise SystemExit(f"{N} images, but world mats {tuple(world.shape)} and times {tuple(times.shape)}")
    scale = torch.eye(4) if a.scale_mat is None else _load(a.scale_mat, "scale_mat")
    views = [dict(camera_mat=K.to(dev), world_mat=world[i].to(dev), scale_mat=scale.to(dev), time_step=times[i:i + 1],
                  image=images[i].permute(1, 2, 0).contiguous()) for i in range(N)]
    depths = None if a.depths is None else list(_load(a.depths, "depths").to(dev))
    if (a.gt_poses is None) != (a.pred_poses is None):
        raise SystemExit("--gt-poses and --pred-poses go together")
    gt_poses = None if a.gt_poses is None else _load(a.gt_poses, "poses")
    pred_poses = None if a.pred_poses is None else _load(a.pred_poses, "poses")
    lpips_fn = None
    if a.lpips_vgg is not None:
        lpips_fn = metrics.LPIPS(metrics.load_lpips_weights(a.lpips_vgg, a.lpips_lin), device=dev)
    r = build_renderer(a.checkpoint).to(dev).set_mfma_dtype(a.mode)
    res = metrics.evaluate(r, views, depth_range=tuple(a.depth_range), gt_poses=gt_poses, pred_poses=pred_poses,
                           gt_depths=depths, lpips_fn=lpips_fn, chunk=a.chunk)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "results.txt")
    metrics.write_results(path, res)
    print(res)
    print(f"The evaluation result is stored in {path}")
    return res


if __name__ == "__main__":
    main()
