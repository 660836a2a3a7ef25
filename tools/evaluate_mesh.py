"""Geometry metrics of a mesh against a ground-truth cloud, on the device: Chamfer distance in the DTU style and
precision / recall / F-score at a threshold in the Tanks and Temples style (metrics.mesh_geometry_metrics).

    python tools/evaluate_mesh.py MESH.ply GT.ply --threshold T [--max-dist D] (--samples S | --density RHO)
        [--seed N] [--crop-min X Y Z --crop-max X Y Z] [--transform T.npy | --align-poses PRED.npy GT.npy]
        [--cull-views K.npy W2C.npy [SCALE.npy] --cull-resolution H W [--cull-min-views N] [--cull-tol-abs A]
         [--cull-tol-rel R] [--cull-gt]] [--depths-out DIR] [--normal-maps-out DIR] [--culled-out MESH.ply]
        [--normals] [--gt-mesh-samples S] [--out results.txt]
        [--icp D [D ...] [--icp-mode point|plane] [--icp-scale] [--icp-samples S] [--icp-stride K [K ...]]
         [--icp-max-iters N] [--icp-tol E] [--transform-out T.npy] [--icp-voxel V]]
        [--gt-outliers K RATIO] [--gt-voxel V] [--gt-estimate-normals K]

MESH.ply is a triangle mesh (tools/extract_mesh.py's output as it is), GT.ply a point cloud (a mesh's vertices are
taken as the cloud).  --transform is a 4 x 4 similarity applied to the mesh first.  --align-poses takes two
camera-to-world trajectories [N, 3 or 4, 4] (.npy) and applies the Sim(3) that aligns the camera centres of PRED
to those of GT (metrics.align_ate_c2b_use_a2b / umeyama, the alignment compute_ATE is measured under): a pose-free
reconstruction lives in its own gauge.  --cull-views cuts the mesh down to what the cameras saw before it is
measured (mesh.cull_mesh: the ScanNet / DTU / Tanks-and-Temples protocols): camera matrices K [N, 4, 4] or [4, 4],
world-to-camera matrices [N, 4, 4] and optionally scale matrices [N, 4, 4] or [4, 4], in the mesh's own frame, for
images of --cull-resolution; --cull-gt also drops the ground-truth points outside every frustum.  --depths-out
writes the mesh's depth from every view as DIR/depth_%06d.npz (key `pred`, 0 where nothing is seen: what
pose_refine.load_depth_dir reads and metrics.depth_metrics scores against sensor depth), --culled-out the culled
mesh, --normal-maps-out the mesh's camera-frame normal map from every view as DIR/%06d_normal.png
(mesh.render_mesh: the picture tools/render_views.py writes for the model).  --normals adds the normal consistency
(normal_accuracy, normal_completeness, normal_consistency, n_pred_normal, n_gt_normal, after the other entries)
against GT.ply's normals; the file must hold them.  --gt-mesh-samples S: GT.ply is a mesh; S points drawn uniformly
by area on it (seed + 1) and their face normals are the ground-truth cloud.  --icp refines the alignment by ICP
before the mesh is measured (metrics.icp_register_stages, as the Tanks-and-Temples protocol follows its trajectory
alignment): one correspondence distance per stage, coarse to fine, on --icp-samples points drawn from the mesh
(default 200000), every --icp-stride'th of them (one K for all stages or one per stage); --icp-mode plane takes its
normals where --normals does (and so implies it), --icp-scale also fits a scale (point mode).  The icp_* entries and the composed
transform follow the other entries; --transform-out saves the composed 4 x 4 (float64 .npy).  A raw ground-truth scan is prepared
first, in this order: --gt-outliers K RATIO removes its statistical outliers (mean distance to the K nearest
neighbours above mean + RATIO std), --gt-voxel V voxel-down-samples it, --gt-estimate-normals K computes its normals
from the K nearest neighbours -- which satisfies --normals and --icp-mode plane for a ground truth without normals.
--icp-voxel V down-samples both clouds of the registration (not of the evaluation) to voxels of V.  Prints one
`name: value` line per metric and with --out writes them in metrics.write_results' format."""
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


def load_views(paths):
    """The views of --cull-views: camera matrices [N, 4, 4] or one [4, 4] for all, world-to-camera matrices
    [N, 4, 4], and optionally scale matrices [N, 4, 4] or one [4, 4]."""
    mats = [np.asarray(np.load(p), dtype=np.float64) for p in paths]
    W = mats[1]
    if W.ndim != 3 or W.shape[1:] != (4, 4):
        raise SystemExit(f"evaluate_mesh: {paths[1]}: world-to-camera matrices [N, 4, 4], got {W.shape}")
    views = [{"world_mat": w} for w in W]
    for key, m, p in (("camera_mat", mats[0], paths[0]),) + ((("scale_mat", mats[2], paths[2]),) if len(mats) == 3 else ()):
        if m.shape == (4, 4):
            m = np.broadcast_to(m, W.shape)
        if m.shape != W.shape:
            raise SystemExit(f"evaluate_mesh: {p}: [4, 4] or {W.shape}, got {m.shape}")
        for v, x in zip(views, m):
            v[key] = x
    return views


def load_ground_truth(path, normals=False, mesh_samples=None):
    """(points, triangles or None, normals or None) of the ground-truth PLY.  With normals and no mesh sampling the
    file must hold vertex normals; with mesh_samples it must hold faces (the normals are then the faces' own)."""
    from copenerf.mesh import read_ply
    points, triangles, nrm, _ = read_ply(path)
    if mesh_samples is not None:
        if triangles is None or len(triangles) == 0:
            raise SystemExit(f"evaluate_mesh: --gt-mesh-samples needs a mesh, {path} has no faces")
        return points, triangles, None
    if normals and nrm is None:
        raise SystemExit(f"evaluate_mesh: --normals needs vertex normals (nx ny nz), {path} has none")
    return points, None, nrm if normals else None


def sample_ground_truth(points, triangles, S, seed, device):
    """S points uniformly by area on the ground-truth mesh and the normals of the triangles they lie on."""
    from copenerf import ops
    v, f = torch.from_numpy(points).to(device), torch.from_numpy(triangles).to(device)
    handle, _ = ops.mesh_area(v, f)
    philox = torch.tensor([int(seed), 0], dtype=torch.uint64, device=device)
    pts, tri = ops.mesh_sample(handle, int(S), philox, want_tri=True)
    c = v[f[tri.clamp(min=0).long()].long()]
    n = torch.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0], dim=-1)
    return pts, torch.where((tri >= 0)[:, None], n, torch.zeros_like(n)).contiguous()


def parse_args(argv=None):
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
    ap.add_argument("--cull-views", nargs="+", metavar="NPY")
    ap.add_argument("--cull-resolution", type=int, nargs=2, metavar=("H", "W"))
    ap.add_argument("--cull-min-views", type=int, default=1)
    ap.add_argument("--cull-tol-abs", type=float)
    ap.add_argument("--cull-tol-rel", type=float)
    ap.add_argument("--cull-gt", action="store_true")
    ap.add_argument("--depths-out")
    ap.add_argument("--normal-maps-out")
    ap.add_argument("--normals", action="store_true")
    ap.add_argument("--gt-mesh-samples", type=int)
    ap.add_argument("--culled-out")
    ap.add_argument("--out")
    ap.add_argument("--icp", type=float, nargs="+", metavar="D")
    ap.add_argument("--icp-mode", choices=("point", "plane"), default="point")
    ap.add_argument("--icp-scale", action="store_true")
    ap.add_argument("--icp-samples", type=int, default=200000)
    ap.add_argument("--icp-stride", type=int, nargs="+", metavar="K")
    ap.add_argument("--icp-max-iters", type=int, default=50)
    ap.add_argument("--icp-tol", type=float, default=1e-6)
    ap.add_argument("--transform-out")
    ap.add_argument("--gt-outliers", nargs=2, metavar=("K", "RATIO"))
    ap.add_argument("--gt-voxel", type=float, metavar="V")
    ap.add_argument("--gt-estimate-normals", type=int, metavar="K")
    ap.add_argument("--icp-voxel", type=float, metavar="V")
    a = ap.parse_args(argv)
    if a.gt_outliers is not None:
        try:
            a.gt_outliers = (int(a.gt_outliers[0]), float(a.gt_outliers[1]))
        except ValueError:
            ap.error("--gt-outliers takes a neighbour count K and a ratio")
        if not 1 <= a.gt_outliers[0] <= 32 or not a.gt_outliers[1] > 0:
            ap.error("--gt-outliers takes K in [1, 32] and a positive ratio")
    if a.gt_voxel is not None and not (a.gt_voxel > 0 and a.gt_voxel < float("inf")):
        ap.error("--gt-voxel takes a positive size")
    if a.icp_voxel is not None and (a.icp is None or not (a.icp_voxel > 0 and a.icp_voxel < float("inf"))):
        ap.error("--icp-voxel takes a positive size and needs --icp")
    if a.gt_estimate_normals is not None:
        if not 3 <= a.gt_estimate_normals <= 32:
            ap.error("--gt-estimate-normals takes K in [3, 32]")
        if not (a.normals or (a.icp is not None and a.icp_mode == "plane")):
            ap.error("--gt-estimate-normals needs --normals or --icp-mode plane")
    if a.gt_mesh_samples is not None and (a.gt_estimate_normals is not None or a.gt_outliers is not None):
        ap.error("--gt-mesh-samples draws a clean cloud with the faces' normals: not with --gt-estimate-normals or --gt-outliers")
    if a.icp is None and (a.icp_stride is not None or a.icp_scale or a.transform_out or a.icp_mode != "point"):
        ap.error("--icp-mode, --icp-scale, --icp-stride and --transform-out need --icp")
    if a.icp is not None:
        if min(a.icp) <= 0 or a.icp_samples < 1 or a.icp_max_iters < 1:
            ap.error("--icp takes positive distances, --icp-samples and --icp-max-iters positive counts")
        if a.icp_stride is not None and (len(a.icp_stride) not in (1, len(a.icp)) or min(a.icp_stride) < 1):
            ap.error("--icp-stride takes one positive K, or one per --icp stage")
        if a.icp_scale and a.icp_mode == "plane":
            ap.error("--icp-scale needs --icp-mode point")
    if a.cull_views is not None and len(a.cull_views) not in (2, 3):
        ap.error("--cull-views takes K.npy W2C.npy [SCALE.npy]")
    if (a.cull_views is None) != (a.cull_resolution is None):
        ap.error("--cull-views and --cull-resolution go together")
    if a.cull_views is None and (a.cull_gt or a.depths_out or a.culled_out):
        ap.error("--cull-gt, --depths-out and --culled-out need --cull-views")
    if a.cull_views is None and a.normal_maps_out:
        ap.error("--normal-maps-out needs --cull-views")
    if a.gt_mesh_samples is not None and a.gt_mesh_samples < 1:
        ap.error("--gt-mesh-samples takes a positive count")
    return a


def icp_kwargs(a):
    """The `icp` dict mesh_geometry_metrics takes, from the parsed --icp options (None without --icp)."""
    if a.icp is None:
        return None
    strides = a.icp_stride or [1]
    strides = strides * len(a.icp) if len(strides) == 1 else strides
    extra = {} if a.icp_voxel is None else {"voxel": a.icp_voxel}
    return dict(stages=[dict(max_corr_dist=d, stride=k) for d, k in zip(a.icp, strides)], n_samples=a.icp_samples,
                mode=a.icp_mode, with_scale=a.icp_scale, max_iters=a.icp_max_iters, tol=a.icp_tol, **extra)


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_mesh: needs a HIP device; the metrics have no CPU path")
    from copenerf import metrics
    from copenerf.mesh import read_ply
    vertices, triangles, _, _ = read_ply(a.mesh)
    if triangles is None:
        raise SystemExit(f"evaluate_mesh: {a.mesh} has no faces")
    want_normals = a.normals or (a.icp is not None and a.icp_mode == "plane")
    # (--gt-estimate-normals: the ground truth's normals are computed from its points, whatever the file holds)
    gt, gt_triangles, gt_normals = load_ground_truth(a.gt, want_normals and a.gt_estimate_normals is None, a.gt_mesh_samples)
    transform = None
    if a.transform:
        transform = np.load(a.transform)
    elif a.align_poses:
        transform = pose_alignment(np.load(a.align_poses[0]), np.load(a.align_poses[1]))
    dev = torch.device("cuda")
    tv, tf = torch.from_numpy(vertices).to(dev), torch.from_numpy(triangles).to(dev)
    cull = {}
    if a.cull_views:
        from copenerf import mesh
        views = load_views(a.cull_views)
        tol = {k: v for k, v in (("tol_abs", a.cull_tol_abs), ("tol_rel", a.cull_tol_rel)) if v is not None}
        cull = dict(cull_views=views, cull_resolution=tuple(a.cull_resolution), cull_gt=a.cull_gt,
                    cull_min_views=a.cull_min_views, **{"cull_" + k: v for k, v in tol.items()})
        if a.depths_out:
            os.makedirs(a.depths_out, exist_ok=True)
            depth = mesh.render_mesh_depth(tv, tf, views, a.cull_resolution)["depth"]
            depth = torch.where(torch.isinf(depth), torch.zeros_like(depth), depth).cpu().numpy()
            for i, d in enumerate(depth):
                np.savez(os.path.join(a.depths_out, "depth_%06d.npz" % i), pred=d)
        if a.normal_maps_out:
            from PIL import Image
            os.makedirs(a.normal_maps_out, exist_ok=True)
            pictures = mesh.render_mesh(tv, tf, views, a.cull_resolution)["normal_image"].cpu().numpy()
            for i, img in enumerate(pictures):
                Image.fromarray(img).save(os.path.join(a.normal_maps_out, "%06d_normal.png" % i))
        if a.culled_out:
            cv, cf, _ = mesh.cull_mesh(tv, tf, views, a.cull_resolution, min_views=a.cull_min_views, **tol)
            mesh.write_ply(a.culled_out, cv.cpu().numpy(), cf.cpu().numpy())
    gt_points = torch.from_numpy(gt).to(dev)
    if a.gt_mesh_samples is not None:
        gt_points, sampled_normals = sample_ground_truth(gt, gt_triangles, a.gt_mesh_samples, a.seed + 1, dev)
        gt_normals = sampled_normals if want_normals else None
    elif gt_normals is not None:
        gt_normals = torch.from_numpy(np.ascontiguousarray(gt_normals)).to(dev)
    if gt_normals is not None:
        cull["gt_normals"] = gt_normals
    if a.icp is not None:
        cull["icp"] = icp_kwargs(a)
    for key, value in (("gt_outliers", a.gt_outliers), ("gt_voxel", a.gt_voxel), ("gt_estimate_normals", a.gt_estimate_normals)):
        if value is not None:
            cull[key] = value
    result = metrics.mesh_geometry_metrics(
        tv, tf, gt_points, threshold=a.threshold, max_dist=a.max_dist, n_samples=a.samples,
        density=a.density, seed=a.seed, transform=transform, crop_min=a.crop_min, crop_max=a.crop_max, **cull)
    if a.transform_out:
        np.save(a.transform_out, np.asarray(result["transform"], dtype=np.float64))
    for key, value in result.items():
        print(f"{key}: {value}")
    if a.out:
        metrics.write_results(a.out, result)
    return result


if __name__ == "__main__":
    main()
