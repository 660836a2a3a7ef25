"""Geometry metrics of a mesh against a ground-truth cloud, on the device: Chamfer distance in the DTU style and
precision / recall / F-score at a threshold in the Tanks and Temples style (metrics.mesh_geometry_metrics).

    python tools/evaluate_mesh.py MESH.ply GT.ply --threshold T [--max-dist D] (--samples S | --density RHO)
        [--seed N] [--crop-min X Y Z --crop-max X Y Z] [--transform T.npy | --align-poses PRED.npy GT.npy]
        [--out results.txt]

MESH.ply is a triangle mesh (tools/extract_mesh.py's output as it is), GT.ply a point cloud (a mesh's vertices are
taken as the cloud).  --transform is a 4 x 4 similarity applied to the mesh first.  --align-poses takes two
camera-to-world trajectories [N, 3 or 4, 4] (.npy) and applies the Sim(3) that aligns the camera centres of PRED
to those of GT (metrics.align_ate_c2b_use_a2b / umeyama, the alignment compute_ATE is measured under): a pose-free
reconstruction lives in its own gauge.  Prints one `name: value` line per metric and with --out writes them in
metrics.write_results' format."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]


def pose_alignment(pred_poses, gt_poses):
    """The 4 x 4 similarity [s R, t] that metrics.align_ate_c2b_use_a2b applies to the camera centres of
    pred_poses to bring them onto gt_poses'."""
    from copenerf import metrics
    a, b = metrics._np_poses(pred_poses), metrics._np_poses(gt_poses)
    if a.shape[0] != b.shape[0]:
        raise SystemExit(f"evaluate_mesh: {a.shape[0]} predicted poses for {b.shape[0]} ground-truth poses")
    s, R, t = metrics.umeyama(b[:, :3, 3], a[:, :3, 3])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = s * R, t
    return M


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("gt")
    ap.add_argument("--threshold", type=float, required=True)
    ap.add_argument("--max-dist", type=float, default=float("inf"))
    n = ap.add_mutually_exclusive_group(required=True)
    n.add_argument("--samples", type=int)
    n.add_argument("--density", type=float)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--crop-min", type=float, nargs=3)
    ap.add_argument("--crop-max", type=float, nargs=3)
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--transform")
    g.add_argument("--align-poses", nargs=2, metavar=("PRED.npy", "GT.npy"))
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_mesh: needs a HIP device; the metrics have no CPU path")
    from copenerf import metrics
    from copenerf.mesh import read_ply
    vertices, triangles, _, _ = read_ply(a.mesh)
    if triangles is None:
        raise SystemExit(f"evaluate_mesh: {a.mesh} has no faces")
    gt = read_ply(a.gt)[0]
    transform = None
    if a.transform:
        transform = np.load(a.transform)
    elif a.align_poses:
        transform = pose_alignment(np.load(a.align_poses[0]), np.load(a.align_poses[1]))
    dev = torch.device("cuda")
    result = metrics.mesh_geometry_metrics(
        torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev), torch.from_numpy(gt).to(dev),
        threshold=a.threshold, max_dist=a.max_dist, n_samples=a.samples, density=a.density, seed=a.seed,
        transform=transform, crop_min=a.crop_min, crop_max=a.crop_max)
    for key, value in result.items():
        print(f"{key}: {value}")
    if a.out:
        metrics.write_results(a.out, result)
    return result


if __name__ == "__main__":
    main()
