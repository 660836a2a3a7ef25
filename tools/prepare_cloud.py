"""Prepare a raw point cloud the way the evaluation protocols do before scoring against it, on the device:
statistical outlier removal, voxel down-sampling and normal estimation (metrics.remove_statistical_outliers,
voxel_down_sample, estimate_normals), applied in that order.

    python tools/prepare_cloud.py IN.ply OUT.ply [--outliers K RATIO] [--voxel V]
        [--estimate-normals K [--orient-to X Y Z]]

IN.ply is a point cloud (a mesh's vertices are taken as the cloud); its normals and colours, where it has them, go
through the filter and are averaged per voxel.  --outliers removes the points whose mean distance to their K nearest
neighbours is above mean + RATIO std over the cloud; --voxel keeps one point per occupied voxel of edge V (the mean of
the voxel's points); --estimate-normals replaces the normals by the PCA normal of the K nearest neighbours, flipped
towards --orient-to where given (otherwise the largest component is positive).  OUT.ply is a cloud PLY without faces,
with nx ny nz when the cloud has normals.  Prints the point counts."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--outliers", nargs=2, metavar=("K", "RATIO"))
    ap.add_argument("--voxel", type=float, metavar="V")
    ap.add_argument("--estimate-normals", type=int, metavar="K")
    ap.add_argument("--orient-to", type=float, nargs=3, metavar=("X", "Y", "Z"))
    a = ap.parse_args(argv)
    if a.outliers is not None:
        try:
            a.outliers = (int(a.outliers[0]), float(a.outliers[1]))
        except ValueError:
            ap.error("--outliers takes a neighbour count K and a ratio")
        if not 1 <= a.outliers[0] <= 32 or not a.outliers[1] > 0:
            ap.error("--outliers takes K in [1, 32] and a positive ratio")
    if a.voxel is not None and not (a.voxel > 0 and a.voxel < float("inf")):
        ap.error("--voxel takes a positive size")
    if a.estimate_normals is not None and not 3 <= a.estimate_normals <= 32:
        ap.error("--estimate-normals takes K in [3, 32]")
    if a.orient_to is not None and a.estimate_normals is None:
        ap.error("--orient-to needs --estimate-normals")
    if a.outliers is None and a.voxel is None and a.estimate_normals is None:
        ap.error("nothing to do: give --outliers, --voxel or --estimate-normals")
    return a


def write_cloud(path, points, normals=None, colors=None):
    """A cloud PLY: mesh.write_ply with no faces."""
    from copenerf.mesh import write_ply
    write_ply(path, points, np.zeros((0, 3), dtype=np.int32), normals=normals, colors=colors)


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("prepare_cloud: needs a HIP device; the passes have no CPU path")
    from copenerf import metrics
    from copenerf.mesh import read_ply
    points, _, normals, colors = read_ply(a.input)
    dev = torch.device("cuda")
    n_in = len(points)
    pts = torch.from_numpy(np.ascontiguousarray(points)).to(dev)
    nrm = None if normals is None or a.estimate_normals is not None else torch.from_numpy(np.ascontiguousarray(normals)).to(dev)
    col = None if colors is None else torch.from_numpy(np.ascontiguousarray(colors)).to(dev).float()
    if a.outliers is not None:
        pts, keep = metrics.remove_statistical_outliers(pts, *a.outliers)
        nrm = None if nrm is None else nrm[keep].contiguous()
        col = None if col is None else col[keep].contiguous()
        print(f"outliers: {n_in - pts.shape[0]} of {n_in} points removed")
    if a.voxel is not None:
        before = pts.shape[0]
        down = metrics.voxel_down_sample(pts, a.voxel, normals=nrm, colors=col)
        pts, nrm, col = down["points"], down["normals"], down["colors"]
        print(f"voxel: {before} points into {pts.shape[0]} voxels, {down['n_dropped']} dropped")
    if a.estimate_normals is not None:
        nrm = metrics.estimate_normals(pts, a.estimate_normals, orient_to=a.orient_to)
        print(f"normals: {int((nrm == 0).all(1).sum())} of {pts.shape[0]} points without one")
    write_cloud(a.output, pts.cpu().numpy(), None if nrm is None else nrm.cpu().numpy(),
                None if col is None else col.round().clamp(0, 255).to(torch.uint8).cpu().numpy())
    print(f"points: {pts.shape[0]}")
    return pts.shape[0]


if __name__ == "__main__":
    main()
