"""Pose-refinement timings on the device: one optimiser step over a batch of 16 frame pairs (both
directions, 32 jobs) at 540 x 960 and at 135 x 240, for two arms:

  fused     PoseRetriever.poses_at + pose_refine.refine_loss (cn_refine_warp) + backward + Adam step
  composed  the reference's form in torch ops on the device: the pose batch from stacked forward() calls,
            the expressions of compute_loss_and_warp_image (utils_poses/pose_refinement.py:34-61) with
            motion.warp_pixel, torch.inverse for K and the reverse poses, backward, Adam step

    python tools/pose_refine_bench.py [--sizes 540x960 135x240] [--pairs 16] [--repeats 10] [--out DIR]

Every figure is the median of `repeats` timed steps after three warm-up steps, each step timed with
device events, the two arms alternating inside one process, with the min .. max spread beside it.  The
fused pass alone (ops.refine_warp, forward and pose gradient in one launch plus the reduction) is timed
the same way; its bytes/s are its algorithmic bytes over that time: per job and pixel the depth (4), the
target frame (12) and the source frame once (12).  Prints a markdown table and a JSON line (also written
under --out), stamped with the library's build digest."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]


def _stat(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _alternate(fns, repeats, warmup=3):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            ms[k].append(_timed(fn))
    return [_stat(m) for m in ms]


def make_inputs(H, W, pairs, seed=0, device="cuda"):
    """pairs + 1 smooth frames, depth -(2 + 0.5 sin cos), K = [[f, 0, cx], [0, f W / H, cy], [0, 0, 1]]."""
    N = pairs + 1
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0, 1, H).view(1, 1, H, 1)
    x = torch.linspace(0, 1, W).view(1, 1, 1, W)
    f = torch.rand(N, 3, 2, generator=g) * 2.0 + 0.5
    ph = torch.rand(N, 3, generator=g) * 6.28
    images = 0.5 + 0.4 * torch.sin(6.2831853 * (f[..., 0, None, None] * x + f[..., 1, None, None] * y) + ph[..., None, None])
    dp = torch.rand(N, 2, generator=g).view(N, 2, 1, 1) * 6.28
    depth = -(2.0 + 0.5 * torch.sin(3.0 * x[0] + dp[:, 0]) * torch.cos(2.0 * y[0] + dp[:, 1]))
    K = torch.tensor([[1.3, 0.0, 0.01], [0.0, 1.3 * W / H, -0.01], [0.0, 0.0, 1.0]])
    r = torch.rand(pairs, 3, generator=g) * 0.06 - 0.03
    t = torch.rand(pairs, 3, generator=g) * 0.16 - 0.08
    return images.to(device).contiguous(), depth.to(device).contiguous(), K.to(device), r.to(device), t.to(device)


def composed_loss(images, next_images, depths, K_batch, uv_batch, relative_poses):
    """compute_loss_and_warp_image (pose_refinement.py:34-61) in torch ops, with motion.warp_pixel."""
    from copenerf.motion import warp_pixel
    B = len(images)
    xyz = torch.inverse(K_batch) @ (uv_batch * depths).view(B, 3, -1)
    xyz = relative_poses[:, :3, :3] @ xyz + relative_poses[:, :3, [-1]]
    tuv = K_batch @ xyz
    tuv = (tuv[:, :2] / tuv[:, [-1]]).view(uv_batch[:, :2].shape)
    valid = ((tuv[:, 0] >= -1) & (tuv[:, 0] <= 1) & (tuv[:, 1] >= -1) & (tuv[:, 1] <= 1)).float().unsqueeze(1)
    warped = warp_pixel(src_frame=next_images, uv=tuv, normalize_pix=False)
    return torch.sum(torch.abs(warped - images) * valid) / torch.sum(valid)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["540x960", "135x240"])
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pose_refine_bench: needs a HIP device; nothing is measured without one")
    from copenerf import PoseRetriever, _lib, ops
    from copenerf.pose_refine import canonical_uv, inv3x3, make_optimizer, refine_loss
    from copenerf.rays import inv4x4
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    B = a.pairs
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        images, depth, K, r, t = make_inputs(H, W, B)
        idx = torch.arange(B, device="cuda")
        nxt = idx + 1
        host_idx = list(range(B))
        Kinv = inv3x3(K)
        Kb = K.expand(B, 3, 3).contiguous()
        uv_batch = canonical_uv(H, W, "cuda").unsqueeze(0).repeat(B, 1, 1, 1)
        arms = {}
        for arm in ("fused", "composed"):
            p = PoseRetriever(B).cuda()
            with torch.no_grad():
                p.r.copy_(r)
                p.t.copy_(t)
            arms[arm] = (p,) + make_optimizer(p, 1e-3)

        def fused_step():
            p, opt, _ = arms["fused"]
            loss = refine_loss(images, depth, K, Kinv, p.poses_at(idx), idx, nxt)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()

        def composed_step():
            p, opt, _ = arms["composed"]
            rel = torch.stack([p(i) for i in host_idx])
            pos = composed_loss(images[:-1], images[1:], depth[:-1, None], Kb, uv_batch, rel)
            neg = composed_loss(images[1:], images[:-1], depth[1:, None], Kb, uv_batch, torch.inverse(rel))
            loss = (pos + neg) / 2
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()

        with torch.no_grad():
            rel = arms["fused"][0].poses_at(idx)
            pose = torch.cat([rel[:, :3, :], inv4x4(rel)[:, :3, :]]).contiguous()
        tgt, src = torch.cat([idx, nxt]).int(), torch.cat([nxt, idx]).int()
        K2, Ki2 = K.expand(2 * B, 3, 3).contiguous(), Kinv.expand(2 * B, 3, 3).contiguous()

        def fused_pass():
            return ops.refine_warp(images, depth, tgt, src, pose, K2, Ki2)

        same = abs(float(fused_step()) - float(composed_step()))  # the two arms' first losses (same start)
        fused, composed, kernel = _alternate([fused_step, composed_step, fused_pass], a.repeats)
        nbytes = 2 * B * H * W * 28
        rows.append({"H": H, "W": W, "pairs": B, "jobs": 2 * B, "fused_step": fused, "composed_step": composed,
                     "composed_over_fused": composed["median_ms"] / fused["median_ms"], "fused_pass": kernel,
                     "fused_pass_bytes": nbytes, "fused_pass_GBps": nbytes / (kernel["median_ms"] * 1e-3) / 1e9,
                     "first_loss_abs_diff": same})
        del images, depth, uv_batch, arms
        torch.cuda.empty_cache()
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "rows": rows}
    f = lambda s: f'{s["median_ms"]:.3f} ({s["min_ms"]:.3f} .. {s["max_ms"]:.3f})'  # noqa: E731
    lines = [f"library {stamp}, {res['device']}, median (min .. max) ms of {a.repeats} steps, {B} pairs ({2 * B} jobs)", "",
             "| frames | fused step | composed step | composed / fused | fused pass | algorithmic MB | GB/s |",
             "|---|---|---|---|---|---|---|"]
    for w in rows:
        lines.append(f'| {w["H"]} x {w["W"]} | {f(w["fused_step"])} | {f(w["composed_step"])} | '
                     f'{w["composed_over_fused"]:.2f} | {f(w["fused_pass"])} | {w["fused_pass_bytes"] / 1e6:.1f} | '
                     f'{w["fused_pass_GBps"]:.0f} |')
    table = "\n".join(lines)
    print(table)
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "pose_refine_bench.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.join(a.out, "pose_refine_bench.md"), "w") as fh:
            fh.write(table + "\n")
    return res


if __name__ == "__main__":
    main()
