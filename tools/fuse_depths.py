"""Fuse per-view depth maps into a truncated signed distance volume and mesh what the cameras saw, on the device
(mesh.fuse_depths: fusion.TSDFVolume over cn_tsdf_integrate, the observed-only mesher and mesh_clean).

    python tools/fuse_depths.py OUT.ply --depths DIR|depths.npy --K K.npy --world-mats W2C.npy
        [--scale-mat S.npy] [--images imgs.npy]
        --bound-min X Y Z --bound-max X Y Z (--dims NX NY NZ | --voxel-size V)
        [--trunc T (default: 4 voxels)] [--depth-max D] [--min-weight W]
        [--keep-largest] [--min-triangles N] [--views-per-call B]

--depths is a directory of depth_%06d.npz files (key `pred`, read in sorted order with pose_refine.load_depth_dir: what
tools/render_views.py --extract and tools/evaluate_mesh.py --depths-out write) or one .npy array [N, h, w]; a depth
of 0, +inf or NaN means that the pixel saw nothing.  --K holds camera matrices [N, 4, 4] or one [4, 4] for all,
--world-mats world-to-camera matrices [N, 4, 4], --scale-mat optionally scale matrices [N, 4, 4] or one [4, 4]: the
views of tools/evaluate_mesh.py --cull-views, for images of the depth maps' size.  --images: colours [N, h, w, 3],
uint8 or float in [0, 1]; the PLY then carries vertex colours.  The box --bound-min .. --bound-max is divided into
--dims voxels per axis, or into voxels of about --voxel-size.  OUT.ply goes into tools/evaluate_mesh.py as it is."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--depths", required=True)
    ap.add_argument("--K", required=True)
    ap.add_argument("--world-mats", required=True)
    ap.add_argument("--scale-mat")
    ap.add_argument("--images")
    ap.add_argument("--bound-min", type=float, nargs=3, required=True)
    ap.add_argument("--bound-max", type=float, nargs=3, required=True)
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--dims", type=int, nargs=3)
    g.add_argument("--voxel-size", type=float)
    ap.add_argument("--trunc", type=float)
    ap.add_argument("--depth-max", type=float)
    ap.add_argument("--min-weight", type=int, default=1)
    ap.add_argument("--keep-largest", action="store_true")
    ap.add_argument("--min-triangles", type=int, default=0)
    ap.add_argument("--views-per-call", type=int, default=8)
    a = ap.parse_args(argv)
    if not all(h > l for l, h in zip(a.bound_min, a.bound_max)):
        ap.error("--bound-max must exceed --bound-min on every axis")
    if a.voxel_size is not None:
        if not (a.voxel_size > 0 and math.isfinite(a.voxel_size)):
            ap.error("--voxel-size takes a positive size")
        a.dims = [max(int(math.ceil((h - l) / a.voxel_size)) + 1, 2) for l, h in zip(a.bound_min, a.bound_max)]
    if min(a.dims) < 2 or math.prod(a.dims) >= 2 ** 31:
        ap.error(f"dims {a.dims}: each at least 2, and nx ny nz below 2^31")
    if a.trunc is not None and not (a.trunc > 0 and math.isfinite(a.trunc)):
        ap.error("--trunc takes a positive distance")
    if a.depth_max is not None and not a.depth_max > 0:
        ap.error("--depth-max takes a positive depth")
    if a.min_weight < 1 or a.min_triangles < 0 or a.views_per_call < 1:
        ap.error("--min-weight and --views-per-call take at least 1, --min-triangles at least 0")
    return a


def load_depths(path):
    if os.path.isdir(path):
        from copenerf.pose_refine import load_depth_dir
        depths = load_depth_dir(path)
    else:
        depths = np.load(path)
    depths = np.asarray(depths, dtype=np.float32)
    if depths.ndim != 3:
        raise SystemExit(f"fuse_depths: {path}: depth maps [N, h, w], got {depths.shape}")
    return depths


def load_views(k_path, w_path, s_path, n):
    """The views of --K / --world-mats / --scale-mat as the dicts mesh.view_projections takes."""
    W = np.asarray(np.load(w_path), dtype=np.float64)
    if W.ndim != 3 or W.shape[1:] != (4, 4) or W.shape[0] != n:
        raise SystemExit(f"fuse_depths: {w_path}: world-to-camera matrices [{n}, 4, 4], got {W.shape}")
    views = [{"world_mat": w} for w in W]
    for key, p in (("camera_mat", k_path), ("scale_mat", s_path)):
        if p is None:
            continue
        m = np.asarray(np.load(p), dtype=np.float64)
        if m.shape == (4, 4):
            m = np.broadcast_to(m, W.shape)
        if m.shape != W.shape:
            raise SystemExit(f"fuse_depths: {p}: [4, 4] or {W.shape}, got {m.shape}")
        for v, x in zip(views, m):
            v[key] = x
    return views


def main(argv=None):
    a = parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("fuse_depths: needs a HIP device; the fusion has no CPU path")
    from copenerf import mesh
    depths = load_depths(a.depths)
    views = load_views(a.K, a.world_mats, a.scale_mat, depths.shape[0])
    colors = None
    if a.images:
        colors = np.load(a.images)
        if colors.shape != depths.shape + (3,):
            raise SystemExit(f"fuse_depths: {a.images}: images {depths.shape + (3,)}, got {colors.shape}")
    stats = {}
    out = mesh.fuse_depths(depths, views, a.bound_min, a.bound_max, a.dims, a.trunc, colors=colors, depth_max=a.depth_max,
                           min_weight=a.min_weight, keep_largest=a.keep_largest, min_triangles=a.min_triangles,
                           views_per_call=a.views_per_call, stats=stats)
    mesh.write_ply(a.out, out[0], out[1], colors=out[2] if colors is not None else None)
    print(f"{a.out}: {len(out[0])} vertices, {len(out[1])} triangles from {depths.shape[0]} views on a "
          f"{a.dims[0]} x {a.dims[1]} x {a.dims[2]} grid ({stats.get('components_kept', 0)} of {stats.get('components', 0)} "
          "components kept)")
    return out


if __name__ == "__main__":
    main()
