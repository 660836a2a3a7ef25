"""cn_ray_visuals and cn_visual_images on the device against tests/visuals_ref.py, render_image's fused tail
against its torch tail, and the files render_visdata / render_train_views write.

The per-ray bound is measured, not fixed: on the same inputs the torch fp32 composition of render_image (the
ops of copenerf/inference.py, restated in _torch_tail) has some largest error against the float64 restatement;
the kernel's largest error must stay within 4 x that (another, equally valid summation order and the affine
composition) plus 4 fp32 ulp of the largest magnitude of the result.  Both errors of every case go to
profiles/visuals_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import visuals_ref as V
from helpers import REN_CFG, build_modules, fixture, load_pretrained_sdf

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)


# ---------------------------------------------------------------------------
# per ray
def _torch_tail(pts, normals, wts, world_mat, omegas, vels, dt, proj, pix, hw):
    """The per-chunk tail of render_image(ray_visuals="torch"), op for op (copenerf/inference.py)."""
    dev = pts.device
    normal = (normals * wts[:, :, None]).sum(1)
    amax = wts.argmax(1)
    p_max = pts[torch.arange(pts.shape[0], device=dev), amax]
    if world_mat is None:
        depth_max = -p_max[:, 2]
    else:
        depth_max = -(p_max @ world_mat[:3, :3].T + world_mat[:3, 3])[:, 2]
        normal = normal @ world_mat[:3, :3].T
    out = {"normal": normal, "depth_max_w": depth_max}
    if omegas is not None:
        p = pts.reshape(-1, 3).clone()
        for k in range(omegas.shape[0]):
            p = p + dt * (torch.cross(omegas[k].expand_as(p), p, dim=-1) + vels[k])
        p = (wts[:, :, None] * p.view(wts.shape[0], -1, 3)).sum(1)
        q = (proj @ p.T).T
        f = (q[:, :2] / q[:, 2:] - pix).clone()
        f[..., 0] *= hw[1] / 2
        f[..., 1] *= hw[0] / 2
        out["flow"] = f
    return out


def _ray_case(R, S, K, seed, special):
    """Points in front of the camera (z in [-5, -2], so q.z = -P.z stays above 1), positive weights summing
    to about 0.9, and the special rays: all-zero weights, the maximum at the last sample, the maximum twice."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-1.5, 1.5, (R, S, 3)).astype(np.float32)
    pts[..., 2] = rng.uniform(-5.0, -2.0, (R, S)).astype(np.float32)
    normals = rng.normal(size=(R, S, 3)).astype(np.float32)
    w = rng.random((R, S)).astype(np.float32) + np.float32(0.05)
    w = (w / w.sum(1, keepdims=True) * np.float32(0.9)).astype(np.float32)
    kinds = {}
    for r, kind in ((0, "zeros"), (1, "last"), (2, "twice")) if R >= 3 else ((0, special),):
        if kind == "zeros":
            w[r] = 0.0
        elif kind == "last":
            w[r, S - 1] = w[r].max() * np.float32(1.5)
        elif kind == "twice" and S >= 2:
            a, b = sorted(rng.choice(S, 2, replace=False))
            w[r, a] = w[r, b] = w[r].max() * np.float32(1.25)
        kinds[r] = kind
    ang = rng.uniform(-0.3, 0.3, 3)
    cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
    rot = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
           np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
    world = np.eye(4, dtype=np.float32)
    world[:3, :3] = rot
    world[:3, 3] = rng.uniform(-0.3, 0.3, 3)
    omega = (0.3 * rng.normal(size=(K, 3))).astype(np.float32)
    vel = (0.3 * rng.normal(size=(K, 3))).astype(np.float32)
    proj = np.array([[1.1, 0.0, 0.05], [0.0, 1.4, -0.03], [0.0, 0.0, -1.0]], dtype=np.float32)
    pix = rng.uniform(-1, 1, (R, 2)).astype(np.float32)
    return dict(pts=pts, normals=normals, w=w, world=world, omega=omega, vel=vel, proj=proj, pix=pix, kinds=kinds)


def _padded(a, ld):
    """[R, S, 3] on the device as a column slice of an [R S, ld] buffer (the renderer's layout for ld = 4)."""
    R, S, _ = a.shape
    buf = torch.full((R * S, ld), float("nan"), device=DEV)
    buf[:, :3] = torch.from_numpy(a).to(DEV).reshape(-1, 3)
    return buf[:, :3].reshape(R, S, 3)


def test_ray_visuals_against_float64_and_the_torch_tail():
    from copenerf.visualize import ray_visuals
    hw, dt = (24, 32), 0.02
    rows, case = [], 0
    for R in (1, 3, 5, 257):
        for S in (1, 63, 64, 65, 128, 192):
            for K in (0, 1, 10, 30):
                # every (ld, world) pair meets every K, R and S over the 96 cases
                ld = (3, 4)[(case + case // 4) % 2]
                use_world = bool((case // 2 + case // 8) % 2)
                c = _ray_case(R, S, K, 1000 + case, ("none", "zeros", "last", "twice")[(case // 4) % 4])
                case += 1
                world = c["world"] if use_world else None
                flow_kw = dict(omega=c["omega"], vel=c["vel"], dt=dt, proj=c["proj"], pix=c["pix"], flow_hw=hw) if K else {}
                ref = V.ray_visuals_ref(c["pts"], c["normals"], c["w"], world, **flow_kw)
                pts, normals = _padded(c["pts"], ld), _padded(c["normals"], 7 - ld)
                dv = lambda a: None if a is None else torch.from_numpy(a).to(DEV)  # noqa: E731
                w = dv(c["w"])
                tkw = {k: dv(v) for k, v in flow_kw.items() if k in ("omega", "vel", "proj", "pix")}
                got = ray_visuals(pts, normals, w, world_mat=dv(world), dt=dt, flow_hw=hw if K else None, **tkw)
                tor = _torch_tail(pts, normals, w, dv(world), tkw.get("omega"), tkw.get("vel"), dt, tkw.get("proj"),
                                  tkw.get("pix"), hw)
                assert ("flow" in got) == (K > 0)
                tag = f"R{R} S{S} K{K} ld{ld} world{int(use_world)}"
                # the arg-max: exact everywhere, the first of equal maxima
                p_star = c["pts"][np.arange(R), ref["argmax"]]
                for r, kind in c["kinds"].items():
                    if kind == "zeros":
                        assert ref["argmax"][r] == 0
                    elif kind == "last":
                        assert ref["argmax"][r] == S - 1
                    elif kind == "twice" and S >= 2:
                        assert (c["w"][r] == c["w"][r].max()).sum() == 2 and c["w"][r, ref["argmax"][r]] == c["w"][r].max()
                depth = got["depth_max_w"].cpu().numpy()
                if world is None:
                    assert np.array_equal(depth, -p_star[:, 2]), tag  # bitwise, hence the index
                else:  # the index does not depend on the world matrix: the same call without one shows it
                    plain = ray_visuals(pts, normals, w)["depth_max_w"].cpu().numpy()
                    assert np.array_equal(plain, -p_star[:, 2]), tag
                live = c["w"].sum(1) > 0  # an all-zero ray projects 0 / 0: NaN in every implementation
                row = {"case": tag}
                for key in ("normal", "depth_max_w", "flow"):
                    if key not in got or (key == "depth_max_w" and world is None):
                        continue
                    g, t, r64 = got[key].cpu().numpy().astype(np.float64), tor[key].cpu().numpy().astype(np.float64), ref[key]
                    if key == "flow":
                        assert np.isnan(g[~live]).all() and np.isnan(r64[~live]).all(), tag
                        g, t, r64 = g[live], t[live], r64[live]
                    if r64.size == 0:
                        continue
                    e_torch, e_kernel = float(np.abs(t - r64).max()), float(np.abs(g - r64).max())
                    floor = 4 * EPS * float(np.abs(r64).max())
                    row[key] = {"torch_fp32_max_err": e_torch, "kernel_max_err": e_kernel, "bound": 4 * e_torch + floor}
                    print(tag, key, row[key])
                    assert e_kernel <= 4 * e_torch + floor, (tag, key, row[key])
                rows.append(row)
    assert case == 96
    with open(os.path.join(ROOT, "profiles", "visuals_parity.json"), "w") as fh:
        json.dump({"rule": "kernel_max_err <= 4 torch_fp32_max_err + 4 eps32 max|float64 result|", "cases": rows}, fh, indent=1)
        fh.write("\n")


def test_ray_visuals_refuses_cpu_tensors():
    from copenerf.visualize import ray_visuals, visual_images
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ray_visuals(torch.zeros(2, 4, 3), torch.zeros(2, 4, 3), torch.zeros(2, 4))
    z = torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        visual_images(torch.zeros(2, 3, 3), z, z, z, torch.zeros(2, 3, 3))


# ---------------------------------------------------------------------------
# the image pass
# the seeds were chosen on the CPU (float64 restatement) so that the share asserted below holds
IMAGE_SEEDS = {(1, 1): 0, (3, 5): 2, (17, 70): 1, (135, 240): 0}


def _image_case(h, w, seed):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    c = {"rgb": rng.random((h, w, 3), dtype=f32), "depth": rng.random((h, w), dtype=f32) * f32(4.5) + f32(0.5),
         "depth_max_w": rng.random((h, w), dtype=f32) * f32(4.5) + f32(0.4),
         "weighted_z": rng.random((h, w), dtype=f32) * f32(5) + f32(0.3),
         "normal": (rng.normal(size=(h, w, 3)) * 0.7).astype(f32),  # some components beyond +-1: the clamp
         "flow": (rng.normal(size=(h, w, 2)) * 3).astype(f32)}
    if h * w == 1:
        c["flow"][:] = 0  # one pixel alone is the pixel of the largest norm (below): only a zero field stays out of the band
    return c


def flow_band(flow):
    """(levels, exact, band): the float64 value of every channel before the floor, where it is exactly an integer
    (a channel at 255 in both wheel rows gives exactly 255: held to equality, as is a zero field's white), and
    where it lies within 0.01 of an integer without being one."""
    levels, _ = V.flow_levels_ref(flow)
    dist = np.abs(levels - np.rint(levels))
    return levels, dist == 0, (dist > 0) & (dist <= 0.01)


def band_share_allowed(flow):
    """At most 5 % of the pixels in the band.  The pixel of the largest norm m is always in it when the field is
    not zero: its norm is m / (m + eps) < 1, so the channel that is 0 in both wheel rows (every pair of
    neighbouring rows has one) gives 255 eps / (m + eps), just above 0.  Below 20 pixels that one pixel
    alone is more than 5 %, and it is the only one allowed."""
    hw = flow.shape[0] * flow.shape[1]
    return 0.05 if hw >= 20 or not flow.any() else 1.0 / hw


@pytest.mark.parametrize("h,w", list(IMAGE_SEEDS))
def test_visual_images_against_the_restatement(h, w):
    from copenerf.visualize import visual_images
    c = _image_case(h, w, IMAGE_SEEDS[(h, w)])
    ref = V.images_ref(c["rgb"], c["depth"], c["depth_max_w"], c["weighted_z"], c["normal"], c["flow"])
    dv = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
    got = visual_images(dv["rgb"], dv["depth"], dv["depth_max_w"], dv["weighted_z"], dv["normal"], dv["flow"])
    for key in ("stats", "img", "disparity", "disparity_highest_weight", "normal"):
        g = got[key].cpu().numpy()
        assert g.dtype == ref[key].dtype and g.shape == ref[key].shape, key
        assert np.array_equal(g.view(np.uint32) if key == "stats" else g, ref[key].view(np.uint32) if key == "stats" else ref[key]), key
    assert (ref["normal"] == 0).any() and (ref["normal"] == 255).any() or h * w < 100  # the clamp is exercised
    levels, exact, band = flow_band(c["flow"])
    share = band.any(-1).mean()
    print(f"{h} x {w}: {share:.4f} of the pixels in the band, {exact.mean():.4f} of the values exact")
    assert share <= band_share_allowed(c["flow"])
    fimg = got["flow"].cpu().numpy().astype(np.int64)
    want = np.floor(levels).astype(np.int64)
    assert np.array_equal(fimg[~band], want[~band])
    assert (np.abs(fimg - want)[band] <= 1).all()
    if not c["flow"].any():
        assert (fimg == 255).all()
    # without a flow: the statistic is 0 and the flow image stays black (training.py:303)
    nof = visual_images(dv["rgb"], dv["depth"], dv["depth_max_w"], dv["weighted_z"], dv["normal"], None)
    assert float(nof["stats"][4]) == 0.0 and not nof["flow"].any()
    assert torch.equal(nof["img"], got["img"]) and torch.equal(nof["disparity"], got["disparity"])


# ---------------------------------------------------------------------------
# end to end: 24 x 32, the pretrained SDF, a seeded motion network
H, W = 24, 32
N_IMAGES, NB_STEP = 10, 10


@pytest.fixture(scope="module")
def scene():
    from copenerf import MotionNetwork, NeuSRenderer
    from copenerf.rays import intrinsics_ndc
    from copenerf.train_step import MOTION_CFG
    fx = fixture("render_pretrained")
    sdf, col, dev = build_modules(int(fx["seed"]), device=DEV)
    load_pretrained_sdf(sdf, fx)
    torch.manual_seed(5)
    motion = MotionNetwork(**MOTION_CFG)
    with torch.no_grad():  # non-trivial velocities
        for p in motion.parameters():
            p.add_(0.05 * torch.randn_like(p))
    r = NeuSRenderer(None, sdf, dev, col, motion.to(DEV), **REN_CFG).to(DEV)
    K = intrinsics_ndc(0.9 * W, 0.9 * W, W, H, device=DEV)
    return r, K


def _batch(K, idx):
    return {"img.camera_mat": K[None], "img.scale_mat": torch.eye(4, device=DEV)[None], "img.idx": torch.tensor([idx]),
            "img.ref_idxs": [torch.tensor([idx + 1])]}


def test_render_image_fused_against_torch(scene):
    from copenerf.inference import arange_pixels, relative_world_mat, render_image
    from copenerf.rays import near_far_from_sphere, world_rays
    r, K = scene
    I = torch.eye(4, device=DEV)
    t, t1 = torch.tensor([-1.0 + 2 * 3 / 9], device=DEV), torch.tensor([-1.0 + 2 * 4 / 9], device=DEV)
    _, pixels = arange_pixels(H, W, device=DEV)
    with torch.no_grad():
        world = relative_world_mat(r.motion_network, 2, 3, N_IMAGES, NB_STEP)
        steps = torch.linspace(float(t), float(t1), NB_STEP + 1, device=DEV)[:-1]
        omega, vel = r.motion_network(steps.view(-1, 1))
    dt = (float(t1) - float(t)) / NB_STEP
    for wm in (I, world):
        kw = dict(motion=r.motion_network, next_time_step=t1, nb_sample_timestep=NB_STEP)
        a = render_image(r, K, wm, I, (H, W), t, chunk=H * W, **kw)
        b = render_image(r, K, wm, I, (H, W), t, chunk=H * W, ray_visuals="fused", **kw)
        c = render_image(r, K, wm, I, (H, W), t, chunk=256, ray_visuals="fused", **kw)
        assert set(a) == set(b) == set(c) == {"rgb", "depth", "weighted_z", "normal", "depth_highest_weight", "flow"}
        for k in b:
            assert torch.equal(b[k], c[k]), k  # chunking does not change a bit of the fused result
        for k in ("rgb", "depth", "weighted_z"):
            assert torch.equal(a[k], b[k]), k
        if wm is I:
            assert torch.equal(a["depth_highest_weight"], b["depth_highest_weight"])
        # the float64 restatement on the renderer's own samples, and the rule of the synthetic cases
        with torch.no_grad():
            rays_o, rays_d, norm = world_rays(pixels, K, wm, I)
            near, far = near_far_from_sphere(rays_o, (0.01, 5.0))
            out = r(rays_o, rays_d, norm, t, near, far, cos_anneal_ratio=1.0, it=0, eval=True)
        assert torch.equal(out["color_fine"].view(H, W, 3), a["rgb"])  # the samples render_image saw
        host = lambda x: x.detach().cpu().numpy()  # noqa: E731
        ref = V.ray_visuals_ref(host(out["sampled_points"]), host(out["normals"]), host(out["weights"]),
                                None if wm is I else host(wm), omega=host(omega), vel=host(vel), dt=dt,
                                proj=host(I[:3, :3] @ K[:3, :3]), pix=host(pixels), flow_hw=(H, W))
        for k, rk in (("normal", "normal"), ("flow", "flow"), ("depth_highest_weight", "depth_max_w")):
            r64 = ref[rk].reshape(host(a[k]).shape)
            ta, tb = host(a[k]).astype(np.float64), host(b[k]).astype(np.float64)
            live = np.isfinite(r64)
            assert live.mean() > 0.9 and np.array_equal(np.isfinite(ta), live) and np.array_equal(np.isfinite(tb), live), k
            e_torch, e_fused = np.abs(ta - r64)[live].max(), np.abs(tb - r64)[live].max()
            floor = 4 * EPS * np.abs(r64[live]).max()
            print(k, "identity" if wm is I else "world", "torch", e_torch, "fused", e_fused, "bound", 4 * e_torch + floor)
            assert e_fused <= 4 * e_torch + floor, (k, e_torch, e_fused)


def test_render_visdata_writes_five_files(scene, tmp_path):
    from PIL import Image

    from copenerf import render_visdata
    from copenerf.visualize import vis_paths
    r, K = scene
    cfg = {"depth_bound_scheduler_milestones": [0, 100], "depth_bound_lr": [0.5, 0.25], "nb_sample_timestep": NB_STEP}
    depth_range = [0.01, 5.0]
    log = []

    class Logger:
        def add_scalar(self, name, value, it):
            log.append((name, float(value), it))

    gt = {3: np.full((H, W), 2.0, np.float32)}
    # render_only: the arrays, no files, no update of the range
    only = render_visdata(r, _batch(K, 3), None, 2, (H, W), 150, 0.0, total_nb_images=N_IMAGES, nb_sample_timestep=NB_STEP,
                          depth_range=depth_range, cfg=cfg, render_only=True)
    assert depth_range == [0.01, 5.0] and os.listdir(tmp_path) == []
    pkl = render_visdata(r, _batch(K, 3), None, 2, (H, W), 150, 0.0, total_nb_images=N_IMAGES, nb_sample_timestep=NB_STEP,
                         depth_range=depth_range, cfg=cfg, out_render_path=str(tmp_path), gt_depths=gt, logger=Logger())
    assert pkl["render_image"].shape == (H, W, 3) and pkl["render_depth"].shape == (H, W)
    assert pkl["render_normal"].shape == (H * W, 3)
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 for v in pkl.values())
    shapes = [(H, W, 3), (H, W, 3), (H, W, 3), (H, W), (H, W)]
    for p, s in zip(vis_paths(str(tmp_path), 3), shapes):
        assert np.asarray(Image.open(p)).shape == s, p
    assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p) for p in vis_paths(str(tmp_path), 3))
    img = np.asarray(Image.open(vis_paths(str(tmp_path), 3)[0]))
    assert np.array_equal(img, (np.clip(pkl["render_image"], 0, 1) * np.float32(255)).astype(np.uint8))
    assert np.asarray(Image.open(vis_paths(str(tmp_path), 3)[1])).any()  # a flow was drawn
    # the far bound moved by the second milestone's rate towards 1.1 max(weighted z)
    names = [n for n, _, _ in log]
    assert names[:4] == ["stats/depth_running_min", "stats/depth_running_max", "stats/depth_sample_min",
                         "stats/depth_sample_max"]
    sample_max = log[3][1]
    assert depth_range[0] == 0.01 and depth_range[1] == pytest.approx(5.0 * 0.75 + sample_max * 0.25, rel=1e-12)
    assert log[1][1] == depth_range[1] and 0 < sample_max < 5.0 * 1.1 + 1e-3
    assert sum(n.startswith("depth_eval/") for n in names) == 7 and sum(n.startswith("depth_highW_eval/") for n in names) == 7
    assert all(np.array_equal(only[k], pkl[k]) for k in pkl)  # the same render (the range moved afterwards)


def test_render_train_views_round_trip(scene, tmp_path):
    from copenerf import Trainer, render_train_views
    from copenerf.pose_refine import load_depth_dir
    r, K = scene
    idxs = [0, 4, 7]
    cfg = {"nb_sample_timestep": NB_STEP, "n_training_points": 64, "depth_bound_scheduler_milestones": [0],
           "depth_bound_lr": [0.5], **{k: [1.0, 1.0] for k in (
               "rgb_weight", "eikonal_weight", "sdf_weight", "flow_rgb_weight", "sdf_consistency_weight",
               "edge_aware_smoothness_weight", "smoothness_weight")}}
    tr = Trainer(r, None, None, cfg, device=DEV, total_nb_images=N_IMAGES,
                 cfg_all={"rendering": {"depth_range": [0.01, 5.0]}}, logger=None, gt_depths=[])
    views = [_batch(K, i) for i in idxs]
    paths = render_train_views(r, views, idxs, str(tmp_path), resolution=(H, W), it=0, anneal_end=0.0,
                               total_nb_images=N_IMAGES, nb_sample_timestep=NB_STEP, depth_range=tr.depth_range, cfg=cfg)
    assert [os.path.basename(p) for p in paths] == ["depth_%06d.npz" % i for i in idxs]
    back = load_depth_dir(os.path.join(str(tmp_path), "extraction_stage1", "depths"))
    assert back.shape == (3, H, W) and back.dtype == np.float32
    for k, i in enumerate(idxs):  # the trainer's method renders the same view: bit for bit what was written
        pkl = tr.render_visdata(views[k], None, i, (H, W), 0, 0.0, idx=i, render_only=True)
        assert np.array_equal(back[k], pkl["render_depth"]), i
    assert not np.array_equal(back[0], back[1]) and np.isfinite(back).all()
