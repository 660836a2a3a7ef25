"""Float64 restatement of the evaluation metrics, written from their formulas (numpy only): what
cn_image_metrics, cn_depth_errors and copenerf.metrics' pose functions are specified to compute
(include/copenerf.h, ABI v18).  tests/test_metrics_host.py holds it to the reference's own numbers
(tests/golden/metrics.npz); the GPU tests hold the kernels to it."""
from __future__ import annotations

import math

import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window_taps():
    """The 11 Gaussian weights (sigma 1.5) as the metric defines them: evaluated in double, stored in fp32,
    divided in fp32 by their sum (the correctly rounded fp32 sum, which is what torch's sum gives for them;
    a left-to-right fp32 sum is one ulp lower)."""
    g = np.array([math.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)], dtype=np.float32)
    return g / np.float32(g.astype(np.float64).sum())


def window_2d():
    """The 11 x 11 window: the outer product of the taps, itself stored in fp32."""
    g = window_taps()
    return (g[:, None] * g[None, :]).astype(np.float32).astype(np.float64)


def blur(img):
    """The window over [..., H, W] with zero padding of 5 (float64)."""
    img = np.asarray(img, dtype=np.float64)
    H, W = img.shape[-2:]
    pad = np.zeros(img.shape[:-2] + (H + 10, W + 10))
    pad[..., 5:5 + H, 5:5 + W] = img
    w = window_2d()
    out = np.zeros_like(img)
    for i in range(11):
        for j in range(11):
            out += w[i, j] * pad[..., i:i + H, j:j + W]
    return out


def ssim_map(x, y):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mu1, mu2 = blur(x), blur(y)
    s1 = blur(x * x) - mu1 * mu1
    s2 = blur(y * y) - mu2 * mu2
    s12 = blur(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def plane_mse(x, y):
    """Mean squared error per [H, W] plane: [..., H, W] -> [...]."""
    d = np.asarray(x, dtype=np.float64) - np.asarray(y, dtype=np.float64)
    return (d * d).mean(axis=(-2, -1))


def psnr_of_mse(mse):
    with np.errstate(divide="ignore"):
        return 20 * np.log10(1.0 / np.sqrt(mse))


def image_metrics(x, y):
    """What cn_image_metrics writes for [N, C, H, W]: ([N, C, 2] (mse, mean ssim), the map)."""
    m = ssim_map(x, y)
    return np.stack([plane_mse(x, y), m.mean(axis=(-2, -1))], -1), m


def eval_image_metrics(preds, gts):
    """The evaluator's PSNR / SSIM over lists of [H, W, 3] maps: per image the mean of the per-channel
    PSNRs and the mean of the map, then the mean over the images."""
    ps, ss = [], []
    for p, g in zip(preds, gts):
        p, g = np.moveaxis(np.asarray(p, np.float64), -1, 0), np.moveaxis(np.asarray(g, np.float64), -1, 0)
        ps.append(psnr_of_mse(plane_mse(p, g)).mean())
        ss.append(ssim_map(p, g).mean())
    return {"PSNR": float(np.mean(ps)), "SSIM": float(np.mean(ss))}


def nearest(pred, Hg, Wg):
    """The nearest-neighbour resize rule of cn_depth_errors: source index floor(dst * src / dst_size)."""
    Hp, Wp = pred.shape
    return pred[(np.arange(Hg) * Hp // Hg)[:, None], (np.arange(Wg) * Wp // Wg)[None, :]]


def depth_errors(gt, pred, min_depth=0.1, max_depth=80.0, clamp=True, ratio=None, dtype=np.float64):
    """(abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, count, thresh) of one map pair in `dtype`: the
    prediction at the ground truth's size, the valid mask, the ratio of medians (unless given), the clamp."""
    gt = np.asarray(gt, dtype=dtype)
    pred = nearest(np.asarray(pred, dtype=dtype), *gt.shape)
    valid = (gt >= min_depth) & (gt <= max_depth)
    g, p = gt[valid], pred[valid]
    if g.size == 0:
        return (float("nan"),) * 7 + (0, g)
    if ratio is None:
        ratio = np.median(g) / np.median(p)
    p = p * dtype(ratio)
    if clamp:
        p = np.where(p < min_depth, dtype(min_depth), p)
        p = np.where(p > max_depth, dtype(max_depth), p)
    thresh = np.maximum(g / p, p / g)
    d = g - p
    return (np.mean(np.abs(d) / g), np.mean(d * d / g), np.sqrt(np.mean(d * d)),
            np.sqrt(np.mean((np.log(g) - np.log(p)) ** 2)), np.mean(thresh < 1.25), np.mean(thresh < 1.25 ** 2),
            np.mean(thresh < 1.25 ** 3), g.size, thresh)


def umeyama(model, data):
    """The similarity (s, R, t) with model ~ s R data + t in the least-squares sense (Umeyama 1991)."""
    model, data = np.asarray(model, np.float64), np.asarray(data, np.float64)
    mm, md = model.mean(0), data.mean(0)
    a, b = model - mm, data - md
    cov = a.T @ b / len(model)
    U, D, Vt = np.linalg.svd(cov)
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ S @ Vt
    s = (D * np.diag(S)).sum() / ((b * b).sum() / len(model))
    return s, R, mm - s * R @ md


def pose_error(pred, gt):
    """(aligned [N, 4, 4], rpe_trans * 100, rpe_rot in degrees, ate): the predicted camera-to-world poses
    aligned to gt by the sim(3) of the camera positions, then the ATE (RMSE of the position differences) and
    the mean relative pose errors of consecutive frames."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    s, R, t = umeyama(gt[:, :3, 3], pred[:, :3, 3])
    al = np.tile(np.eye(4), (len(pred), 1, 1))
    al[:, :3, :3] = R @ pred[:, :3, :3]
    al[:, :3, 3] = s * pred[:, :3, 3] @ R.T + t
    ate = np.sqrt(np.mean(np.sum((gt[:, :3, 3] - al[:, :3, 3]) ** 2, 1)))
    tr, ro = [], []
    for i in range(len(gt) - 1):
        e = np.linalg.inv(np.linalg.inv(gt[i]) @ gt[i + 1]) @ (np.linalg.inv(al[i]) @ al[i + 1])
        tr.append(np.linalg.norm(e[:3, 3]))
        ro.append(np.arccos(np.clip((np.trace(e[:3, :3]) - 1) / 2, -1, 1)))
    return al, np.mean(tr) * 100, np.degrees(np.mean(ro)), ate


def rodrigues(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def trajectory(n, seed):
    """n camera-to-world poses [n, 4, 4] along a curved path with slowly turning cameras."""
    rng = np.random.default_rng(seed)
    T = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        a = i / (n - 1)
        T[i, :3, :3] = rodrigues([0.3 * a, -0.5 * a + 0.05 * rng.standard_normal(), 0.2 * np.sin(3 * a)])
        T[i, :3, 3] = [2 * a, 0.5 * np.sin(4 * a), 0.3 * a * a] + 0.02 * rng.standard_normal(3)
    return T


def apply_sim3(T, s, R, t):
    """The trajectory seen from a frame related by x' = s R x + t."""
    out = T.copy()
    out[:, :3, :3] = R @ T[:, :3, :3]
    out[:, :3, 3] = s * T[:, :3, 3] @ R.T + t
    return out
