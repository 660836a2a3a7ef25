"""Refine the camera poses of a sequence from its stage-1 depth maps (copenerf.pose_refine.refine_poses).

    python tools/refine_poses.py --depths OUT/extraction_stage1/depths --images imgs.npy --K K.npy --out OUT/models

  --depths  a directory of .npz files with a `pred` array each, in sorted order (what render_train_views
            writes, one per training view), any resolution: brought to the frames' size (nearest)
  --images  .npy (or .npz with `imgs`): float [N, 3, H, W], the dataset's frames (planar, as the reference's
            `imgs`)
  --K       .npy (or .npz with `K`): [3, 3], [4, 4], [N, 3, 3] or [N, 4, 4]; the upper-left 3 x 3 is used
  --init    optional .pt / .npy [N - 1, 4, 4]: the motion network's relative poses (refine_from_scratch off)

Writes OUT/refine_pose.pt: the state_dict of PoseRetriever(N, learn_R=False, learn_t=False,
init_c2w=inv(pred) @ pred[world]), the file train.py:395-398 saves and eval.py:42 loads.  Prints the loss
every --log-every epochs."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]


def _load(path, key):
    if path.endswith(".pt"):
        return torch.load(path, map_location="cpu").float()
    a = np.load(path)
    if isinstance(a, np.lib.npyio.NpzFile):
        a = a[key]
    return torch.from_numpy(np.asarray(a)).float()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depths", required=True)
    ap.add_argument("--images", required=True)
    ap.add_argument("--K", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--init", default=None)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--world-cam-idx", type=int, default=0)
    ap.add_argument("--log-every", type=int, default=50)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("refine_poses: needs a HIP device (the fused pass has no CPU path)")
    from copenerf import PoseRetriever
    from copenerf.pose_refine import load_depth_dir, refine_poses
    from copenerf.rays import inv4x4
    dev = torch.device("cuda")
    images = _load(a.images, "imgs").to(dev).contiguous()
    depth = torch.from_numpy(load_depth_dir(a.depths)).float().to(dev)
    K = _load(a.K, "K")[..., :3, :3].to(dev)
    if images.dim() != 4 or images.shape[1] != 3:
        raise SystemExit(f"--images: expected [N, 3, H, W], got {tuple(images.shape)}")
    if depth.shape[0] != images.shape[0]:
        raise SystemExit(f"{images.shape[0]} frames but {depth.shape[0]} depth maps")
    init = None if a.init is None else _load(a.init, "c2c")

    def on_epoch(epoch, loss, pred):
        if epoch % a.log_every == 0:
            print(f"epoch {epoch}: loss {loss:.6f}", flush=True)

    res = refine_poses(images, depth, K, pose_refine_lr=a.lr, pose_refine_epochs=a.epochs,
                       refine_from_scratch=init is None, init_c2c=init, on_epoch=on_epoch)
    pred = res.pred_poses
    pred = inv4x4(pred) @ pred[a.world_cam_idx].unsqueeze(0)  # train.py:395
    table = PoseRetriever(images.shape[0], learn_R=False, learn_t=False, init_c2w=pred.cpu())
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "refine_pose.pt")
    torch.save(table.state_dict(), path)
    print(f"{'converged' if res.converged else 'stopped'} after {len(res.losses)} epochs, loss {res.losses[-1]:.6f}; "
          f"wrote {path}")
    return path


if __name__ == "__main__":
    main()
