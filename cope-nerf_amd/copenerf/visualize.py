"""Visualisation renders and the stage-1 view extraction: Trainer.render_visdata (model/training.py:157-374)
and Trainer.render_train_views (train.py:288-305) on the device.

  ray_visuals       cn_ray_visuals: the per-ray tail of the render loop (training.py:236-281) -- the
                    weight-averaged normal, the depth of the highest-weight sample and the forward flow of the
                    advected weight-averaged point -- in one read of the samples;
  visual_images     cn_visual_images: the per-image arithmetic (training.py:292-318, 343-345) -- the five
                    statistics and the uint8 colour, disparity, normal and colour-wheel flow images;
  render_visdata    the reference's method as a function of the renderer (copenerf.Trainer.render_visdata
                    delegates here): render (inference.render_image, ray_visuals="fused"), write the five
                    PNG files, update the adaptive depth range, log the depth errors;
  render_train_views  the depth maps pose refinement reads (extraction_stage1/depths/depth_%06d.npz, key
                    `pred`: what pose_refine.load_depth_dir and setup_pose_refinement load) and the images
                    beside them.

The two kernels have no CPU path: tensors must live on the device.  PNG / JPEG files are written with PIL,
imported on first use.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .ops import _need, _ptr

VIS_FILES = ("%04d_img.png", "%04d_flow.png", "%04d_normal.png", "%04d_disparity.png",
             "%04d_disparity_highest_weight.png")
STAT_KEYS = ("weighted_z_min", "weighted_z_max", "disparity_max", "disparity_highest_weight_max", "flow_norm_max")


def _rows3(t, R, S, name):
    """[R, S, 3] or [R S, 3] (a column slice of the renderer's [M, 4] buffers included) -> ([M, 3] view with
    unit column stride, its leading dimension in elements)."""
    _need(t, name, ndim=0)
    if t.dtype != torch.float32 or t.numel() != R * S * 3:
        raise RuntimeError(f"ray_visuals: {name} must be fp32 with {R} x {S} x 3 elements (got {t.dtype}, "
                           f"shape {tuple(t.shape)})")
    v = t.reshape(-1, 3)
    if v.stride(1) != 1 or (v.shape[0] > 1 and v.stride(0) < 3):
        v = v.contiguous()
    return v, (v.stride(0) if v.shape[0] > 1 else 3)


def _small(t, shape, name, dev):
    if t is None:
        return None
    _need(t, name, ndim=0)
    if t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev:
        raise RuntimeError(f"ray_visuals: {name} must be fp32 {list(shape)} on {dev} (got {t.dtype}, "
                           f"{tuple(t.shape)}, {t.device})")
    return t.contiguous()


def ray_visuals(pts, normals, weights, *, world_mat=None, omega=None, vel=None, dt=0.0, proj=None, pix=None,
                flow_hw=None):
    """cn_ray_visuals for R rays of S samples: pts, normals [R, S, 3] (or [R S, 3]; any row stride), weights
    [R, S].  world_mat: [4, 4] on the device, or None for the identity.  A flow is computed when omega and vel
    ([K, 3], K >= 1 Euler steps of length dt) are given, and then needs proj [3, 3] (scale_mat[:3, :3] @
    camera_mat[:3, :3]), pix [R, 2] and flow_hw = (h, w) of the image (the flow is in pixels).
    Returns {"normal" [R, 3], "depth_max_w" [R]} and, with a flow, "flow" [R, 2]."""
    _need(weights, "weights", ndim=0)
    if weights.dtype != torch.float32 or weights.dim() != 2:
        raise RuntimeError(f"ray_visuals: weights must be fp32 [R, S] (got {weights.dtype}, {tuple(weights.shape)})")
    R, S = weights.shape
    dev = weights.device
    w = weights.contiguous()
    p, ld_p = _rows3(pts, R, S, "pts")
    n, ld_n = _rows3(normals, R, S, "normals")
    world_mat = _small(world_mat, (4, 4), "world_mat", dev)
    flows = omega is not None or vel is not None
    K, scale, ws, need = 0, None, None, 0
    out = {"normal": torch.empty(R, 3, device=dev), "depth_max_w": torch.empty(R, device=dev)}
    if flows:
        if omega is None or vel is None or proj is None or pix is None or flow_hw is None:
            raise RuntimeError("ray_visuals: a flow needs omega, vel, proj, pix and flow_hw")
        K = omega.shape[0]
        omega, vel = _small(omega, (K, 3), "omega", dev), _small(vel, (K, 3), "vel", dev)
        proj, pix = _small(proj, (3, 3), "proj", dev), _small(pix, (R, 2), "pix", dev)
        h, w_ = flow_hw
        scale = (_lib.c_f32 * 2)(w_ / 2, h / 2)
        need = int(_lib.load().cn_ray_visuals_workspace_bytes(K))
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        out["flow"] = torch.empty(R, 2, device=dev)
    _lib.call("cn_ray_visuals", R, S, _ptr(p), ld_p, _ptr(n), ld_n, _ptr(w), _ptr(world_mat), K, _ptr(omega), _ptr(vel),
              float(dt), _ptr(proj), _ptr(pix), scale, _ptr(out["normal"]), _ptr(out["depth_max_w"]),
              _ptr(out.get("flow")), _ptr(ws), need, torch.cuda.current_stream(dev).cuda_stream)
    return out


def visual_images(rgb, depth, depth_max_w, weighted_z, normal, flow=None):
    """cn_visual_images for one h x w render: rgb [h, w, 3], depth, depth_max_w, weighted_z [h, w], normal
    [h, w, 3] (or [h w, 3]), flow [h, w, 2] or None -- contiguous fp32 on the device.  Returns a dict of
    uint8 device tensors "img" [h, w, 3], "disparity", "disparity_highest_weight" [h, w], "normal" [h, w, 3],
    "flow" [h, w, 3] (zeros without a flow, as training.py:303) and "stats", fp32 [5] in STAT_KEYS' order."""
    if depth.dim() != 2:
        raise RuntimeError(f"visual_images: depth must be [h, w] (got {tuple(depth.shape)})")
    h, w = depth.shape
    dev = depth.device
    for t, name, numel in ((rgb, "rgb", 3), (depth, "depth", 1), (depth_max_w, "depth_max_w", 1),
                           (weighted_z, "weighted_z", 1), (normal, "normal", 3), (flow, "flow", 2)):
        if t is None:
            continue
        _need(t, name, ndim=0)
        if t.dtype != torch.float32 or t.numel() != h * w * numel or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"visual_images: {name} must be contiguous fp32 with {h} x {w} x {numel} elements on "
                               f"{dev} (got {t.dtype}, shape {tuple(t.shape)}, strides {t.stride()}, {t.device})")
    u8 = lambda *s: torch.empty(*s, dtype=torch.uint8, device=dev)  # noqa: E731
    out = {"img": u8(h, w, 3), "disparity": u8(h, w), "disparity_highest_weight": u8(h, w), "normal": u8(h, w, 3),
           "flow": u8(h, w, 3) if flow is not None else torch.zeros(h, w, 3, dtype=torch.uint8, device=dev),
           "stats": torch.empty(5, device=dev)}
    need = int(_lib.load().cn_visual_images_workspace_bytes(h, w))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    _lib.call("cn_visual_images", h, w, _ptr(rgb), _ptr(depth), _ptr(depth_max_w), _ptr(weighted_z), _ptr(normal),
              _ptr(flow), _ptr(out["stats"]), _ptr(out["img"]), _ptr(out["disparity"]),
              _ptr(out["disparity_highest_weight"]), _ptr(out["normal"]), _ptr(out["flow"]) if flow is not None else None,
              _ptr(ws), need, torch.cuda.current_stream(dev).cuda_stream)
    return out


# ---------------------------------------------------------------------------
# the adaptive depth range (training.py:339-349)
def depth_bound_lr(it, cfg):
    """The depth_bound_lr of the last milestone `it` has reached (training.py:340-341)."""
    lr = None
    for m, milestone in enumerate(cfg["depth_bound_scheduler_milestones"]):
        if it >= milestone:
            lr = cfg["depth_bound_lr"][m]
    if lr is None:
        raise ValueError(f"iteration {it} lies before the first depth-bound milestone "
                         f"{list(cfg['depth_bound_scheduler_milestones'])} (the reference fails there too)")
    return lr


def update_depth_range(depth_range, it, cfg, z_min, z_max):
    """training.py:340-349: depth_range[1] <- depth_range[1] (1 - lr) + 1.1 z_max lr, in place; the lower
    bound is not updated.  z_min, z_max: the minimum and maximum of the render's weighted z, taken as Python
    floats.  Returns the (min_depth, max_depth) the reference logs as stats/depth_sample_*."""
    lr = depth_bound_lr(it, cfg)
    min_depth = max(depth_range[0], float(z_min) * 0.9)
    max_depth = float(z_max) * 1.1
    depth_range[1] = depth_range[1] * (1 - lr) + max_depth * lr
    return min_depth, max_depth


# ---------------------------------------------------------------------------
# files
def _pil():
    try:
        from PIL import Image
    except ImportError as e:  # pragma: no cover - PIL is a dependency of the visualisation only
        raise RuntimeError("render_visdata / render_train_views write their images with PIL (pillow), which is "
                           "not installed; pass render_only=True to get the arrays without files") from e
    return Image


def vis_paths(out_render_path, idx):
    """The five files render_visdata writes for image `idx` (training.py:329-337), in VIS_FILES' order."""
    return [os.path.join(out_render_path, f % idx) for f in VIS_FILES]


def write_vis_files(out_render_path, idx, images):
    """images: visual_images' dict (device or host uint8 arrays)."""
    Image = _pil()
    host = {k: (v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in images.items() if k != "stats"}
    paths = vis_paths(out_render_path, idx)
    for path, key in zip(paths, ("img", "flow", "normal", "disparity", "disparity_highest_weight")):
        Image.fromarray(host[key]).save(path)
    return paths


def depth_path(out_dir, idx):
    return os.path.join(out_dir, "extraction_stage1", "depths", "depth_%06d.npz" % idx)


def write_train_view(out_dir, idx, render_depth, render_image):
    """train.py:301-305 for one view: depths/depth_%06d.npz (key `pred`, float32 [h, w]), depths/%06d.jpg (the
    depth over its maximum, grey) and images/%06d.png (the colours clipped to [0, 1])."""
    Image = _pil()
    depth = np.ascontiguousarray(render_depth, dtype=np.float32)
    os.makedirs(os.path.join(out_dir, "extraction_stage1", "depths"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "extraction_stage1", "images"), exist_ok=True)
    np.savez(depth_path(out_dir, idx), pred=depth)
    grey = np.clip(np.nan_to_num(depth / np.max(depth)), 0.0, 1.0)
    Image.fromarray((grey * 255.0).astype(np.uint8)).save(
        os.path.join(out_dir, "extraction_stage1", "depths", "%06d.jpg" % idx))
    rgb = np.clip(np.nan_to_num(np.asarray(render_image, dtype=np.float32)), 0.0, 1.0)
    Image.fromarray((rgb * 255.0).astype(np.uint8)).save(
        os.path.join(out_dir, "extraction_stage1", "images", "%06d.png" % idx))


def _nearest(a, h, w):
    """Nearest-neighbour resize by floor(dst * src / dst_size), cn_depth_errors' rule."""
    yi = np.arange(h) * a.shape[0] // h
    xi = np.arange(w) * a.shape[1] // w
    return a[yi][:, xi]


# ---------------------------------------------------------------------------
def render_visdata(renderer, data, world_mat, query_cam_idx, resolution, it, anneal_end, *, total_nb_images,
                   nb_sample_timestep, depth_range, cfg, out_render_path=None, idx=None, render_only=False,
                   gt_depths=None, logger=None, crop_size=0, chunk=65536):
    """Trainer.render_visdata (training.py:157-374).  renderer: the NeuSRenderer (bare or wrapped in
    DataParallel) with its motion_network; data: the loader's batch ("img.camera_mat", "img.scale_mat",
    "img.idx", "img.ref_idxs"); cfg: the training config (depth_bound_scheduler_milestones, depth_bound_lr);
    depth_range: the trainer's [near, far] list, whose far bound is updated in place.

    The image `idx` (default: the batch's) is rendered at the time step of `query_cam_idx`, under world_mat
    or, without one, under the motion network's relative pose between the two frames (identity when they
    coincide), and the flow to the batch's last reference frame is integrated in nb_sample_timestep steps
    per frame interval.  Returns {"render_image" [h, w, 3], "render_depth" [h, w], "render_normal" [h w, 3]}
    as numpy arrays.  Unless render_only: writes VIS_FILES under out_render_path, updates depth_range[1],
    logs the depth statistics and, with gt_depths, both depth maps' errors to `logger` (add_scalar).

    Where the reference fails the behaviour is defined instead: the file names use the image index also when
    idx is None; a reference frame that is not after the image gives no flow and a black flow image."""
    from .inference import relative_world_mat, render_image
    from .metrics import DEPTH_KEYS, compute_depth_errors
    core = getattr(renderer, "module", renderer)
    motion = core.motion_network
    dev = next(core.parameters()).device
    camera_mat = data.get("img.camera_mat").to(dev).reshape(-1, 4, 4)[0].float()
    scale_mat = data.get("img.scale_mat").to(dev).reshape(-1, 4, 4)[0].float()
    batch_idx = int(torch.as_tensor(data.get("img.idx")).reshape(-1)[0])
    image_idx = batch_idx if idx is None else int(idx)
    ref_image_idx = image_idx + (int(torch.as_tensor(data.get("img.ref_idxs")[-1]).reshape(-1)[0]) - batch_idx)
    t_of = lambda i: torch.tensor([i / (total_nb_images - 1) * 2 - 1], dtype=torch.float32, device=dev)  # noqa: E731
    time_step, next_time_step = t_of(image_idx), t_of(ref_image_idx)
    if query_cam_idx is not None and int(query_cam_idx) != image_idx:
        query_time_step = t_of(int(query_cam_idx))
        if world_mat is None:
            with torch.no_grad():
                world_mat = relative_world_mat(motion, int(query_cam_idx), image_idx, total_nb_images,
                                               nb_sample_timestep)
        world_mat = world_mat.to(dev).reshape(4, 4).float()
    else:
        query_time_step = time_step
        world_mat = torch.eye(4, device=dev)
    h, w = (int(v) for v in resolution)
    K = nb_sample_timestep * (ref_image_idx - image_idx)
    car = 1.0 if anneal_end == 0.0 else float(np.min([1.0, it / anneal_end]))
    out = render_image(core, camera_mat, world_mat, scale_mat, (h, w), query_time_step, depth_range=tuple(depth_range),
                       cos_anneal_ratio=car, it=it, chunk=chunk, motion=motion if K >= 1 else None,
                       next_time_step=next_time_step if K >= 1 else None, nb_sample_timestep=K,
                       motion_time_step=time_step, ray_visuals="fused")
    render_pkl = {"render_image": out["rgb"].cpu().numpy(), "render_depth": out["depth"].cpu().numpy(),
                  "render_normal": out["normal"].reshape(h * w, 3).cpu().numpy()}
    if render_only:
        return render_pkl
    images = visual_images(out["rgb"].contiguous(), out["depth"].contiguous(), out["depth_highest_weight"].contiguous(),
                           out["weighted_z"].contiguous(), out["normal"].contiguous(),
                           out["flow"].contiguous() if "flow" in out else None)
    write_vis_files(out_render_path, image_idx, images)
    stats = images["stats"].tolist()
    min_depth, max_depth = update_depth_range(depth_range, it, cfg, stats[0], stats[1])
    if logger is not None:
        logger.add_scalar("stats/depth_running_min", depth_range[0], it)
        logger.add_scalar("stats/depth_running_max", depth_range[1], it)
        logger.add_scalar("stats/depth_sample_min", min_depth, it)
        logger.add_scalar("stats/depth_sample_max", max_depth, it)
    if gt_depths is not None and len(gt_depths) != 0:
        gt_depth = gt_depths[image_idx]
        gt_depth = gt_depth.cpu().numpy() if torch.is_tensor(gt_depth) else np.asarray(gt_depth)
        if crop_size != 0:  # training.py:362-367
            depth_h, depth_w = gt_depth.shape
            crop_w = int(crop_size * depth_w / depth_h)
            gt_depth = _nearest(gt_depth, 484, 648)[crop_size:depth_h - crop_size, crop_w:depth_w - crop_w]
        err = compute_depth_errors(np.ascontiguousarray(gt_depth, dtype=np.float32), out["depth"])
        err_hw = compute_depth_errors(np.ascontiguousarray(gt_depth, dtype=np.float32), out["depth_highest_weight"])
        if logger is not None:
            for d, name in enumerate(DEPTH_KEYS):
                logger.add_scalar(f"depth_eval/{name}", err[d], it)
                logger.add_scalar(f"depth_highW_eval/{name}", err_hw[d], it)
    return render_pkl


def render_train_views(renderer, loader_or_views, image_indices, out_dir, *, resolution, it, anneal_end, total_nb_images,
                       nb_sample_timestep, depth_range, cfg, chunk=65536):
    """Trainer.render_train_views (train.py:288-305): every batch of the loader (or list of batches) is
    rendered in its own frame (image_indices[o] = the dataset's i_train[o] is both the image and the query
    camera) and written under out_dir/extraction_stage1 (write_train_view).  Returns the .npz paths."""
    paths = []
    with torch.no_grad():
        for o, batch in enumerate(loader_or_views):
            image_idx = int(image_indices[o])
            pkl = render_visdata(renderer, batch, None, image_idx, resolution, it, anneal_end, idx=image_idx,
                                 render_only=True, total_nb_images=total_nb_images,
                                 nb_sample_timestep=nb_sample_timestep, depth_range=depth_range, cfg=cfg, chunk=chunk)
            write_train_view(out_dir, image_idx, pkl["render_depth"], pkl["render_image"])
            paths.append(depth_path(out_dir, image_idx))
    return paths
