"""Flow-RGB timings on the device, fused pass (motion.flow_rgb_fused: cn_flow_rgb_fwd / cn_flow_rgb_bwd) against
the torch composition (motion.project_flow_sums + images.index_select + motion.flow_rgb_loss + the mask):

  (a) the term alone, forward plus backward to d ray_acc and d w2c: R rays, T = 3 reference frames out of a
      resident stack of N = 10, at 540 x 960 and at 135 x 240;
  (b) ms_per_step of SyntheticTrainer(stage1=True, mfma_dtype="bf16", start_it=30000, train_cfg=C3_TRAIN) -- the C3
      workload of bench.py -- with flow_rgb="torch" and with flow_rgb="fused".

    python tools/flow_rgb_bench.py [--sizes 540x960 135x240] [--rays 4096] [--repeats 30] [--steps 40] [--out DIR]

Every figure is the median of the timed calls after three warm-up calls, each call timed with device events, the
two arms alternating inside one process, with the min .. max spread beside it.  The term's algorithmic bytes are
what the fused pass must read and write: per ray ray_acc, pixn, pix, rgb_gt (44) and d ray_acc (16), and per ray
and frame 4 taps x 3 channels x 4 bytes, forward and again backward (96) -- an upper bound, rays outside a frame
read no taps.  The pass is latency-bound at that size; the bytes are printed for scale, not as a rate to judge.
Prints a markdown table and a JSON line (also written under --out), stamped with the library's build digest."""
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


def make_inputs(H, W, R, T=3, N=10, seed=0, device="cuda"):
    """Rays of frame 0 with a depth in [1, 3], moved by small relative poses: most correspondences stay inside."""
    from copenerf.rays import intrinsics_ndc, pixels_from_indices
    g = torch.Generator().manual_seed(seed)
    pix, pixn = pixels_from_indices(torch.randint(0, H * W, (R,), generator=g), H, W)
    K = intrinsics_ndc(0.9 * W, 0.9 * W, W, H)
    d = 1.0 + 2.0 * torch.rand(R, 1, generator=g)
    p = d * torch.cat([pixn[:, :1] / K[0, 0], pixn[:, 1:] / K[1, 1], -torch.ones(R, 1)], 1)
    wbar = 0.6 + 0.4 * torch.rand(R, 1, generator=g)
    w2c = torch.eye(4).repeat(T, 1, 1)
    for j in range(T):
        v = 0.01 * (j + 1) * torch.randn(3, generator=g)
        S = torch.tensor([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
        w2c[j, :3, :3] = torch.matrix_exp(S)
        w2c[j, :3, 3] = 0.04 * (j + 1) * torch.randn(3, generator=g)
    to = lambda x: x.to(device).contiguous()  # noqa: E731
    return dict(ray_acc=to(torch.cat([wbar * p, wbar], 1)), w2c=to(w2c), cams=to(K.expand(T, 4, 4)), I=to(torch.eye(4)),
                pixn=to(pixn), pix=to(pix.float()), gt=to(torch.rand(R, 3, generator=g)),
                images=to(torch.rand(N, 3, H, W, generator=g)), frame=to(torch.tensor([3, 4, 5])[:T]),
                valid=to(torch.ones(T, dtype=torch.bool)))


def term_arms(x, H, W):
    """The two forward-plus-backward closures over the same leaves; each returns (per, d ray_acc, d w2c)."""
    from copenerf import motion
    ra, w2c = x["ray_acc"].clone().requires_grad_(True), x["w2c"].clone().requires_grad_(True)

    def done(per):
        ra.grad = w2c.grad = None
        (per.sum() / 3.0).backward()
        return per.detach(), ra.grad, w2c.grad

    def fused():
        return done(motion.flow_rgb_fused(ra[:, :3], ra[:, 3:], w2c, x["cams"], x["I"], x["pixn"], x["pix"], x["images"],
                                          x["frame"], x["gt"], frame_valid=x["valid"]))

    def composed():
        flows = motion.project_flow_sums(ra[:, :3], ra[:, 3:], w2c, x["cams"], x["I"], x["pixn"], (H, W))
        per = motion.flow_rgb_loss(flows, x["pix"], x["images"].index_select(0, x["frame"]), x["gt"])
        return done(torch.where(x["valid"], per, torch.zeros_like(per)))

    return fused, composed


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["540x960", "135x240"])
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40, help="timed training steps per arm (0: skip part (b))")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("flow_rgb_bench: needs a HIP device; nothing is measured without one")
    from bench import C3_TRAIN
    from copenerf import _lib
    from copenerf.train_step import SyntheticTrainer
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    R, T = a.rays, 3
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        x = make_inputs(H, W, R, T)
        fused, composed = term_arms(x, H, W)
        (pf, rf, wf), (pc, rc, wc) = fused(), composed()
        rel = lambda u, v: float((u - v).abs().max() / v.abs().max())  # noqa: E731
        sf, sc = _alternate([fused, composed], a.repeats)
        nbytes = R * (44 + 16) + R * T * 96
        rows.append({"H": H, "W": W, "rays": R, "frames": T, "stack": x["images"].shape[0], "fused": sf, "composed": sc,
                     "composed_over_fused": sc["median_ms"] / sf["median_ms"], "fused_bytes_upper_bound": nbytes,
                     "frames_copied_by_composed_bytes": T * 3 * H * W * 4,
                     "rel_diff": {"per": rel(pf, pc), "d_ray_acc": rel(rf, rc), "d_w2c": rel(wf, wc)}})
        del x, fused, composed
        torch.cuda.empty_cache()
    step = None
    if a.steps > 0:
        kw = dict(stage1=True, mfma_dtype="bf16", start_it=30000, train_cfg=dict(C3_TRAIN))
        arms = {m: SyntheticTrainer("cuda", rays=R, flow_rgb=m, **kw) for m in ("torch", "fused")}
        first = {m: float(tr.step().detach()) for m, tr in arms.items()}  # the same start: the two first losses
        st, sf = _alternate([arms["torch"].step, arms["fused"].step], a.steps)
        for tr in arms.values():
            tr.check_finite()
        step = {"config": "c3", "rays": R, "torch": st, "fused": sf, "torch_minus_fused_ms": st["median_ms"] - sf["median_ms"],
                "rays_per_s": {"torch": R / (st["median_ms"] * 1e-3), "fused": R / (sf["median_ms"] * 1e-3)},
                "first_loss": first}
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "rows": rows, "step": step}
    f = lambda s: f'{s["median_ms"]:.3f} ({s["min_ms"]:.3f} .. {s["max_ms"]:.3f})'  # noqa: E731
    lines = [f"library {stamp}, {res['device']}, median (min .. max) ms, {R} rays, {T} of 10 frames", "",
             "| frames | fused fwd+bwd | composed fwd+bwd | composed / fused | frame copy avoided, MB | fused bytes (bound), MB |",
             "|---|---|---|---|---|---|"]
    for w in rows:
        lines.append(f'| {w["H"]} x {w["W"]} | {f(w["fused"])} | {f(w["composed"])} | {w["composed_over_fused"]:.2f} | '
                     f'{w["frames_copied_by_composed_bytes"] / 1e6:.1f} | {w["fused_bytes_upper_bound"] / 1e6:.2f} |')
    if step:
        d = step["torch_minus_fused_ms"]
        lines += ["", f'C3 step ({a.steps} steps per arm): flow_rgb="torch" {f(step["torch"])} ms, '
                      f'flow_rgb="fused" {f(step["fused"])} ms: the fused step is '
                      f'{"faster" if d > 0 else "NOT faster"} by {abs(d):.3f} ms at the median '
                      f'({step["rays_per_s"]["torch"] / 1e3:.1f} -> {step["rays_per_s"]["fused"] / 1e3:.1f} k rays/s)']
    table = "\n".join(lines)
    print(table)
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "flow_rgb_bench.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.join(a.out, "flow_rgb_bench.md"), "w") as fh:
            fh.write(table + "\n")
    return res


if __name__ == "__main__":
    main()
