"""Image-metric timings on the device: 8 image pairs of 3 channels at 540 x 960 and at 135 x 240, two arms:

  fused     ops.image_metrics (cn_image_metrics: one tiled pass and a small reduction), without the map
  composed  the metric's expressions in fp32 torch ops on the device: five depthwise 11 x 11 convolutions and
            the elementwise SSIM expression, the per-plane means, the squared error

    python tools/metrics_bench.py [--sizes 540x960 135x240] [--pairs 8] [--repeats 20] [--out DIR]

Every figure is the median of `repeats` timed calls after three warm-up calls, each call timed with device
events, the two arms alternating inside one process, with the min .. max spread beside it.  The fused pass's
bytes/s are its algorithmic bytes, 2 N C H W 4 (each input read once), over its time.  The depth pass
(ops.depth_errors, 8 maps against half-size predictions) is timed once the same way, for the record.  Prints a
markdown table and a JSON line, and writes both (metrics_bench.json, metrics_bench.md) under --out, by default the
repository's profiles/; stamped with the library's build digest.  The committed profiles/metrics_bench.json is the
output of the command above with no arguments."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def composed(x, y, win):
    C = x.shape[1]
    blur = lambda t: F.conv2d(t, win, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = blur(x), blur(y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = blur(x * x) - mu1_sq, blur(y * y) - mu2_sq, blur(x * y) - mu12
    m = ((2 * mu12 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return torch.stack([((x - y) ** 2).mean((2, 3)), m.mean((2, 3))], -1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["540x960", "135x240"])
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: needs a HIP device; nothing is measured without one")
    from copenerf import _lib, metrics, ops
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    N, C = a.pairs, 3
    taps = ops.ssim_taps().cuda()
    win = (taps[:, None] * taps[None, :]).expand(C, 1, 11, 11).contiguous()
    g = torch.Generator().manual_seed(0)
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        gt = torch.rand(N, C, H, W, generator=g).cuda()
        pred = (gt + 0.05 * torch.randn(N, C, H, W, generator=g).cuda()).clamp(0, 1).contiguous()
        diff = float((ops.image_metrics(pred, gt)[0] - composed(pred, gt, win)).abs().max())
        fused, comp = _alternate([lambda: ops.image_metrics(pred, gt), lambda: composed(pred, gt, win)], a.repeats)
        nbytes = 2 * N * C * H * W * 4
        rows.append({"H": H, "W": W, "pairs": N, "channels": C, "fused": fused, "composed": comp,
                     "composed_over_fused": comp["median_ms"] / fused["median_ms"], "fused_bytes": nbytes,
                     "fused_GBps": nbytes / (fused["median_ms"] * 1e-3) / 1e9, "max_abs_diff": diff})
        del gt, pred
    H, W = 540, 960
    dgt = (torch.rand(N, H, W, generator=g) * 20 + 0.05).cuda()
    dpred = (torch.rand(N, H // 2, W // 2, generator=g) * 8 + 0.05).cuda()
    ratio = metrics.median_ratio(dgt, dpred, 0.1, 80.0)
    (depth,) = _alternate([lambda: ops.depth_errors(dgt, dpred, ratio, 0.1, 80.0, True)], a.repeats)
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "rows": rows,
           "depth_errors": {"N": N, "Hg": H, "Wg": W, "Hp": H // 2, "Wp": W // 2, **depth}}
    f = lambda s: f'{s["median_ms"]:.3f} ({s["min_ms"]:.3f} .. {s["max_ms"]:.3f})'  # noqa: E731
    lines = [f"library {stamp}, {res['device']}, median (min .. max) ms of {a.repeats} calls, {N} pairs x {C} channels", "",
             "| images | fused | composed | composed / fused | algorithmic MB | fused GB/s |", "|---|---|---|---|---|---|"]
    for w in rows:
        lines.append(f'| {w["H"]} x {w["W"]} | {f(w["fused"])} | {f(w["composed"])} | {w["composed_over_fused"]:.2f} | '
                     f'{w["fused_bytes"] / 1e6:.1f} | {w["fused_GBps"]:.0f} |')
    lines += ["", f"depth errors, {N} maps of {H} x {W} against {H // 2} x {W // 2}: {f(depth)} ms"]
    table = "\n".join(lines)
    print(table)
    print(json.dumps(res))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "metrics_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(a.out, "metrics_bench.md"), "w") as fh:
        fh.write(table + "\n")
    return res


if __name__ == "__main__":
    main()
