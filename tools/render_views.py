"""Render a trained model's views: the five visualisation images per view, or the stage-1 extraction that
pose refinement reads (copenerf.render_visdata / copenerf.render_train_views).

    python tools/render_views.py CHECKPOINT --K K.npy --times t.npy --resolution H W --out OUT [--extract]
        [--total-images N] [--scale-mat S.npy] [--depth-range 0.01 5.0] [--nb-sample-timestep 10] [--it 0]
        [--anneal-end 0] [--chunk 65536] [--mode fp32|bf16x6|bf16]

  CHECKPOINT  one train.py wrote through CheckpointIO, with its motion network (see tools/extract_mesh.py)
  --K         .npy (or .npz with `K`): the camera matrix, [4, 4] (or [3, 3], padded to 4 x 4)
  --times     .npy [V]: each view's time step in [-1, 1]; view v is image round((t + 1) / 2 (N - 1)) of the
              sequence of N = --total-images frames (default: V, every frame a view)
  --extract   write OUT/extraction_stage1/depths/depth_%06d.npz (key `pred`), the grey depth .jpg and
              images/%06d.png instead: the tree tools/refine_poses.py --depths consumes

Without --extract every view is rendered in its own camera and OUT gets %04d_img.png, %04d_flow.png (the flow
to the next frame; black for the last one), %04d_normal.png, %04d_disparity.png and
%04d_disparity_highest_weight.png."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT, os.path.join(ROOT, "tools")]


def _load(path, key):
    a = np.load(path)
    if isinstance(a, np.lib.npyio.NpzFile):
        a = a[key]
    return torch.from_numpy(np.asarray(a)).float()


def view_indices(times, total):
    """The image index of each time step: t = i / (N - 1) * 2 - 1 (training.py:168)."""
    idx = [int(round((float(t) + 1) / 2 * (total - 1))) for t in times]
    if any(i < 0 or i >= total for i in idx):
        raise SystemExit(f"--times: a time step lies outside [-1, 1] (indices {idx} of {total} images)")
    return idx


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint")
    ap.add_argument("--K", required=True)
    ap.add_argument("--times", required=True)
    ap.add_argument("--resolution", type=int, nargs=2, required=True, metavar=("H", "W"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--extract", action="store_true")
    ap.add_argument("--total-images", type=int, default=None)
    ap.add_argument("--scale-mat", default=None)
    ap.add_argument("--depth-range", type=float, nargs=2, default=[0.01, 5.0])
    ap.add_argument("--nb-sample-timestep", type=int, default=10)
    ap.add_argument("--it", type=int, default=0)
    ap.add_argument("--anneal-end", type=float, default=0.0)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--mode", choices=["fp32", "bf16x6", "bf16"], default="bf16x6", help="the MLP GEMMs' MFMA mode")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("render_views: needs a HIP device (the kernels have no CPU fallback)")
    from copenerf import render_train_views, render_visdata
    from extract_mesh import build_renderer
    dev = torch.device("cuda")
    K = _load(a.K, "K")
    if K.shape[-1] == 3:
        K4 = torch.eye(4)
        K4[:3, :3] = K
        K = K4
    times = _load(a.times, "times").reshape(-1)
    total = len(times) if a.total_images is None else a.total_images
    if total < 2:
        raise SystemExit("render_views: a sequence has at least two images")
    idx = view_indices(times, total)
    scale = torch.eye(4) if a.scale_mat is None else _load(a.scale_mat, "scale_mat")
    r = build_renderer(a.checkpoint).to(dev).set_mfma_dtype(a.mode)
    if r.motion_network is None:
        raise SystemExit("render_views: the checkpoint holds no motion network")
    views = [{"img.camera_mat": K[None].to(dev), "img.scale_mat": scale[None].to(dev), "img.idx": torch.tensor([i]),
              "img.ref_idxs": [torch.tensor([min(i + 1, total - 1)])]} for i in idx]
    common = dict(total_nb_images=total, nb_sample_timestep=a.nb_sample_timestep, depth_range=list(a.depth_range),
                  cfg={"depth_bound_scheduler_milestones": [0], "depth_bound_lr": [0.0]}, chunk=a.chunk)
    os.makedirs(a.out, exist_ok=True)
    if a.extract:
        paths = render_train_views(r, views, idx, a.out, resolution=a.resolution, it=a.it, anneal_end=a.anneal_end, **common)
        print(f"wrote {len(paths)} depth maps under {os.path.dirname(paths[0])}")
        return paths
    with torch.no_grad():
        for v, i in zip(views, idx):  # a rate of 0 keeps the depth range: every view is rendered under the same one
            render_visdata(r, v, None, i, a.resolution, a.it, a.anneal_end, out_render_path=a.out, idx=i, **common)
    print(f"wrote {5 * len(idx)} images under {a.out}")
    return a.out


if __name__ == "__main__":
    main()
