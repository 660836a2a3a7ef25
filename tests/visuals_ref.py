"""numpy restatements of the visualisation pass (model/training.py:157-374) for the tests of cn_ray_visuals and
cn_visual_images.

  ray_visuals_ref   the per-ray tail (training.py:236-281) in float64 by the reference's literal loop: every
                    sample point is advected K times, then the weighted sum is taken (not the affine shortcut);
  affine_of_steps   the composed map (A, b) of the K Euler steps, float64 (for the identity the kernel uses);
  images_ref        the image arithmetic (training.py:292-318, 343-345) in float32, numpy ops in the
                    reference's order;
  colour_wheel, flow_levels_ref   torchvision.utils.flow_to_image (training.py:302) restated in float64.
"""
import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)


def ray_visuals_ref(pts, normals, weights, world=None, omega=None, vel=None, dt=0.0, proj=None, pix=None, flow_hw=None):
    """pts, normals [R, S, 3], weights [R, S] -> dict of float64 arrays: normal [R, 3], argmax [R] (the first
    index of the largest weight), depth_max_w [R] and, with omega / vel [K, 3], flow [R, 2]."""
    p = np.asarray(pts, np.float64)
    n = np.asarray(normals, np.float64)
    w = np.asarray(weights, np.float64)
    R = w.shape[0]
    normal = (n * w[:, :, None]).sum(1)
    amax = np.argmax(np.asarray(weights), axis=1)  # numpy, like torch.max, returns the first of equal maxima
    p_max = p[np.arange(R), amax]
    if world is None:
        depth = -p_max[:, 2]
    else:
        W = np.asarray(world, np.float64)
        depth = -(np.concatenate([p_max, np.ones((R, 1))], 1) @ W.T)[:, 2]
        normal = normal @ W[:3, :3].T
    out = {"normal": normal, "argmax": amax, "depth_max_w": depth}
    if omega is not None:
        om, ve = np.asarray(omega, np.float64), np.asarray(vel, np.float64)
        q = p.reshape(-1, 3).copy()
        for k in range(om.shape[0]):  # training.py:271-273
            q = q + dt * (np.cross(np.broadcast_to(om[k], q.shape), q) + ve[k])
        P = (w[:, :, None] * q.reshape(R, -1, 3)).sum(1)
        pr = (np.asarray(proj, np.float64) @ P.T).T
        with np.errstate(divide="ignore", invalid="ignore"):  # a ray without weight projects 0 / 0
            f = pr[:, :2] / pr[:, 2:] - np.asarray(pix, np.float64)
        h, w_ = flow_hw
        out["flow"] = f * np.array([w_ / 2, h / 2])
    return out


def affine_of_steps(omega, vel, dt):
    """(A [3, 3], b [3]) with p^(K) = A p + b for p^(k+1) = p^(k) + dt (omega_k x p^(k) + vel_k), float64."""
    A, b = np.eye(3), np.zeros(3)
    for o, v in zip(np.asarray(omega, np.float64), np.asarray(vel, np.float64)):
        X = np.array([[0.0, -o[2], o[1]], [o[2], 0.0, -o[0]], [-o[1], o[0], 0.0]])  # X p = o x p
        A, b = A + dt * (X @ A), b + dt * (X @ b + v)
    return A, b


def colour_wheel():
    """The 55 x 3 Middlebury wheel of torchvision's _make_colorwheel: segments RY 15, YG 6, GC 4, CB 11,
    BM 13, MR 6 with the ramps floor(255 i / n)."""
    rows = []
    ramp = lambda n: [int(np.floor(255 * i / n)) for i in range(n)]  # noqa: E731
    rows += [(255, r, 0) for r in ramp(15)]
    rows += [(255 - r, 255, 0) for r in ramp(6)]
    rows += [(0, 255, r) for r in ramp(4)]
    rows += [(0, 255 - r, 255) for r in ramp(11)]
    rows += [(r, 0, 255) for r in ramp(13)]
    rows += [(255, 0, 255 - r) for r in ramp(6)]
    return np.array(rows, dtype=np.float64)


def flow_levels_ref(flow):
    """flow [h, w, 2] (float32 values) -> (levels [h, w, 3] float64 = 255 col before the floor, max_norm)."""
    f = np.asarray(flow, np.float64)
    wheel = colour_wheel()
    max_norm = np.sqrt((f ** 2).sum(-1)).max()
    u = f / (max_norm + F32_EPS)
    norm = np.sqrt((u ** 2).sum(-1))
    a = np.arctan2(-u[..., 1], -u[..., 0]) / np.pi
    fk = (a + 1) / 2 * (wheel.shape[0] - 1)
    k0 = np.floor(fk).astype(np.int64)
    k1 = (k0 + 1) % wheel.shape[0]
    fr = (fk - k0)[..., None]
    col = (1 - fr) * (wheel[k0] / 255.0) + fr * (wheel[k1] / 255.0)
    col = 1 - norm[..., None] * (1 - col)
    return 255 * col, max_norm


def flow_image_ref(flow):
    return np.floor(flow_levels_ref(flow)[0]).astype(np.uint8)


def images_ref(rgb, depth, depth_max_w, weighted_z, normal, flow=None):
    """float32 numpy, the reference's order of operations -> dict: stats [5] float32 and the uint8 images img,
    disparity, disparity_highest_weight, normal.  Inputs: positive depths, rgb in [0, 1] (no clamp is needed)."""
    f32 = np.float32
    rgb, depth, dmw, wz, normal = (np.asarray(a, f32) for a in (rgb, depth, depth_max_w, weighted_z, normal))
    h, w = depth.shape
    img = (rgb * f32(255)).astype(np.uint8)                                   # training.py:293
    disp = f32(1) / depth                                                     # :309
    disp_max = disp.max()
    disp_hw = f32(1) / dmw                                                    # :311
    disp_hw_max = disp_hw.max()
    nimg = (normal.reshape(h, w, 3) * f32(128) + f32(128)).clip(0, 255)       # :316-317
    fmax = f32(0)
    if flow is not None:
        fl = np.asarray(flow, f32)
        fmax = np.sqrt(fl[..., 0] * fl[..., 0] + fl[..., 1] * fl[..., 1]).max()
    return {"stats": np.array([wz.min(), wz.max(), disp_max, disp_hw_max, fmax], dtype=f32),
            "img": img,
            "disparity": ((disp / disp_max) * f32(255)).astype(np.uint8),     # :310, 329
            "disparity_highest_weight": ((disp_hw / disp_hw_max) * f32(255)).astype(np.uint8),  # :312, 330
            "normal": nimg.astype(np.uint8)}
