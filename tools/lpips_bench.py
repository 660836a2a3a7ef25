"""LPIPS timings on the device: one image pair at 540 x 960 and at 135 x 240, two arms on the same seeded random
weights:

  device    copenerf.metrics.LPIPS (cn_lpips: patches + cn_linear per convolution, the fused heads), bf16x6
            by default
  composed  the same network as fp32 torch ops on the device: F.conv2d / relu / max_pool2d, the normalisation
            and the 1 x 1 heads as elementwise ops

    python tools/lpips_bench.py [--sizes 540x960 135x240] [--repeats 10] [--mode bf16x6] [--out DIR]

Every figure is the median of `repeats` timed calls after two warm-up calls, each call timed with device events,
the two arms alternating inside one process, with the min .. max spread beside it.  No speed bar is set: the
file records what was measured, whichever arm is faster.  The value's difference between the arms is printed
too (absolute and relative to the composed value).  Prints a markdown table and a JSON line and writes both
(lpips_bench.json, lpips_bench.md) under --out, by default the repository's profiles/; stamped with the
library's build digest.  The committed profiles/lpips_bench.json is the output of the command above with no
arguments."""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]

WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_BEFORE = (2, 4, 7, 10)
TAP_AFTER = (1, 3, 6, 9, 12)


def make_weights(seed, device):
    """He-normal convolutions, biases 0.05 N(0, 1), lin weights U[0, 1) (the tests' recipe)."""
    g = torch.Generator().manual_seed(seed)
    convs, cin = [], 3
    for cout in WIDTHS:
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        convs.append((w.to(device), (0.05 * torch.randn(cout, generator=g)).to(device)))
        cin = cout
    lins = [torch.rand(WIDTHS[t], generator=g).to(device) for t in TAP_AFTER]
    return convs, lins


def composed(x, y, convs, lins, mean, std):
    """[5] terms of one pair [3, H, W]: both images as a batch of two through torch's own convolutions."""
    f = (torch.stack([x, y]) - mean) / std
    terms = []
    for l, (w, b) in enumerate(convs):
        if l in POOL_BEFORE:
            f = F.max_pool2d(f, 2, 2)
        f = F.relu(F.conv2d(f, w, b, padding=1))
        if l in TAP_AFTER:
            n = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            lin = lins[len(terms)].view(1, -1, 1, 1)
            terms.append((((n[0:1] - n[1:2]) ** 2) * lin).sum(1).mean())
    return torch.stack(terms)


def _stat(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _alternate(fns, repeats, warmup=2):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            ms[k].append(_timed(fn))
    return [_stat(m) for m in ms]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["540x960", "135x240"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--mode", choices=["bf16x6", "bf16", "fp32"], default="bf16x6")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench: needs a HIP device; nothing is measured without one")
    from copenerf import _lib, metrics
    dev = torch.device("cuda")
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    convs, lins = make_weights(678, dev)
    net = metrics.LPIPS({"conv": [metrics.lpips_conv_matrix(w) for w, _ in convs], "bias": [b for _, b in convs],
                         "lin": lins}, mode=a.mode, device=dev)
    mean = torch.tensor([-.030, -.088, -.188], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([.458, .448, .450], device=dev).view(1, 3, 1, 1)
    g = torch.Generator().manual_seed(1)
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        x = torch.rand(3, H, W, generator=g)
        y = (x + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1).to(dev)
        x = x.to(dev)
        with torch.no_grad():
            ours, theirs = net.layers(x, y)[0].double(), composed(x, y, convs, lins, mean, std).double()
            dstat, cstat = _alternate([lambda: net(x, y), lambda: composed(x, y, convs, lins, mean, std)], a.repeats)
        value, ref = float(ours.sum()), float(theirs.sum())
        rows.append({"H": H, "W": W, "device": dstat, "composed": cstat,
                     "composed_over_device": cstat["median_ms"] / dstat["median_ms"], "value_device": value,
                     "value_composed": ref, "abs_diff": abs(value - ref), "rel_diff": abs(value - ref) / ref,
                     "rel_diff_per_block": ((ours - theirs).abs() / theirs).tolist(),
                     "workspace_MiB": net._workspace(H, W).numel() / 2 ** 20})
        print(f"{H} x {W}: device {dstat['median_ms']:.3f} ms, composed {cstat['median_ms']:.3f} ms", flush=True)
    res = {"library": stamp, "gpu": torch.cuda.get_device_name(0), "mode": a.mode, "repeats": a.repeats, "rows": rows}
    f = lambda s: f'{s["median_ms"]:.3f} ({s["min_ms"]:.3f} .. {s["max_ms"]:.3f})'  # noqa: E731
    lines = [f"library {stamp}, {res['gpu']}, mode {a.mode}, median (min .. max) ms of {a.repeats} calls, one pair", "",
             "| image | device | composed (torch) | composed / device | value | rel. difference | workspace MiB |",
             "|---|---|---|---|---|---|---|"]
    for w in rows:
        lines.append(f'| {w["H"]} x {w["W"]} | {f(w["device"])} | {f(w["composed"])} | {w["composed_over_device"]:.2f} | '
                     f'{w["value_device"]:.6f} | {w["rel_diff"]:.2e} | {w["workspace_MiB"]:.0f} |')
    table = "\n".join(lines)
    print(table)
    print(json.dumps(res))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "lpips_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    with open(os.path.join(a.out, "lpips_bench.md"), "w") as fh:
        fh.write(table + "\n")
    return res


if __name__ == "__main__":
    main()
