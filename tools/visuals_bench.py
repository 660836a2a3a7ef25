"""Visualisation-pass timings on the device, two arms each:

  per ray    fused     visualize.ray_visuals (cn_ray_visuals: one read of the samples)
             composed  the per-chunk tail of inference.render_image(ray_visuals="torch"), op for op: the clone of
                       the points, K passes of cross / add / mul, the weighted sums, the argmax and the gather
             at 65,536 rays x 128 samples and x 192 samples, K = 10 Euler steps, the points and normals as the
             renderer hands them over (column slices of [M, 4] buffers), under a world matrix;
  per image  fused     visualize.visual_images (cn_visual_images)
             composed  training.py:292-318's arithmetic on the host in numpy after copying the maps back, as the
                       reference does (the flow image excluded: torchvision is not part of this build)
             at 540 x 960 and 135 x 240.

    python tools/visuals_bench.py [--rays 65536] [--samples 128 192] [--steps 10] [--sizes 540x960 135x240]
                                  [--repeats 20] [--out DIR]

Every figure is the median of `repeats` timed calls after three warm-up calls, the two arms alternating inside one
process, with the min .. max spread beside it; the device arms are timed with device events, the host arm with
a host clock around work that ends synchronised.  "fused" is the Python call, allocations and both launches
included: at these sizes the host spends longer enqueueing it than the device running it, so a third arm,
"fused_c_call", times the C call alone into preallocated outputs, eight calls per timing (the queue stays full;
the figure is per call).  The per-ray pass's bytes/s are its algorithmic bytes, 28 per sample (three floats of the
point, three of the normal, the weight), over the C call's time; the bytes it touches in the [M, 4] layout are
36 per sample (whole 16-byte rows), reported beside.  Writes visuals_bench.json under
--out, by default the repository's profiles/, stamped with the library's build digest."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak
CALLS = 8  # C calls per timing of the "fused_c_call" arm


def _stat(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def _timed_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _alternate(fns, timers, repeats, warmup=3):
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, (fn, timer) in enumerate(zip(fns, timers)):
            ms[k].append(timer(fn))
    return [_stat(m) for m in ms]


def torch_tail(pts, normals, wts, world_mat, omegas, vels, dt, proj, pix, hw):
    """inference.render_image's per-chunk tail under a world matrix (copenerf/inference.py), with the final
    scaling to pixels."""
    dev = pts.device
    normal = (normals * wts[:, :, None]).sum(1)
    amax = wts.argmax(1)
    p_max = pts[torch.arange(pts.shape[0], device=dev), amax]
    depth_max = -(p_max @ world_mat[:3, :3].T + world_mat[:3, 3])[:, 2]
    normal = normal @ world_mat[:3, :3].T
    p = pts.reshape(-1, 3).clone()
    for k in range(omegas.shape[0]):
        p = p + dt * (torch.cross(omegas[k].expand_as(p), p, dim=-1) + vels[k])
    p = (wts[:, :, None] * p.view(wts.shape[0], -1, 3)).sum(1)
    q = (proj @ p.T).T
    f = (q[:, :2] / q[:, 2:] - pix).clone()
    f[..., 0] *= hw[1] / 2
    f[..., 1] *= hw[0] / 2
    return normal, depth_max, f


def host_images(rgb, depth, depth_max_w, weighted_z, normal):
    """training.py:292-318, 343 on the host after the copies the reference makes."""
    rgb, depth, dmw, wz, normal = (t.cpu().numpy() for t in (rgb, depth, depth_max_w, weighted_z, normal))
    img = (rgb * 255).astype(np.uint8)
    disp = 1 / depth
    disp = disp / disp.max()
    disp_hw = 1 / dmw
    disp_hw = disp_hw / disp_hw.max()
    nimg = (normal * 128 + 128).clip(0, 255).astype(np.uint8)
    return img, (disp * 255.0).astype(np.uint8), (disp_hw * 255.0).astype(np.uint8), nimg, wz.min(), wz.max()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--samples", type=int, nargs="+", default=[128, 192])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--sizes", nargs="+", default=["540x960", "135x240"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("visuals_bench: needs a HIP device; nothing is measured without one")
    from copenerf import _lib
    from copenerf.visualize import ray_visuals, visual_images
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    g = torch.Generator().manual_seed(0)
    dev = "cuda"
    R, K, hw, dt = a.rays, a.steps, (540, 960), 0.02
    world = torch.eye(4)
    world[:3, :3] = torch.tensor([[0.98, -0.17, 0.0], [0.17, 0.98, 0.0], [0.0, 0.0, 1.0]])
    world[:3, 3] = torch.tensor([0.1, -0.2, 0.05])
    world = world.to(dev)
    omega, vel = (0.3 * torch.randn(K, 3, generator=g)).to(dev), (0.3 * torch.randn(K, 3, generator=g)).to(dev)
    proj = torch.tensor([[1.1, 0.0, 0.05], [0.0, 1.4, -0.03], [0.0, 0.0, -1.0]], device=dev)
    pix = (torch.rand(R, 2, generator=g) * 2 - 1).to(dev)
    ray_rows = []
    for S in a.samples:
        pbuf, nbuf = torch.rand(R * S, 4, generator=g).to(dev), torch.randn(R * S, 4, generator=g).to(dev)
        pbuf[:, 2] = -2 - 3 * pbuf[:, 2]
        pts, normals = pbuf[:, :3].reshape(R, S, 3), nbuf[:, :3].reshape(R, S, 3)
        w = torch.rand(R, S, generator=g).to(dev)
        w = w / w.sum(1, keepdim=True) * 0.9
        fused = lambda: ray_visuals(pts, normals, w, world_mat=world, omega=omega, vel=vel, dt=dt, proj=proj,  # noqa: E731
                                    pix=pix, flow_hw=hw)
        comp = lambda: torch_tail(pts, normals, w, world, omega, vel, dt, proj, pix, hw)  # noqa: E731
        o_n, o_d, o_f = torch.empty(R, 3, device=dev), torch.empty(R, device=dev), torch.empty(R, 2, device=dev)
        ws = torch.empty(256, dtype=torch.uint8, device=dev)
        scale = (_lib.c_f32 * 2)(hw[1] / 2, hw[0] / 2)
        stream = torch.cuda.current_stream().cuda_stream

        def calls():  # the C call alone into preallocated outputs, CALLS times: the queue stays full
            for _ in range(CALLS):
                _lib.call("cn_ray_visuals", R, S, pts.data_ptr(), 4, normals.data_ptr(), 4, w.data_ptr(), world.data_ptr(),
                          K, omega.data_ptr(), vel.data_ptr(), dt, proj.data_ptr(), pix.data_ptr(), scale, o_n.data_ptr(),
                          o_d.data_ptr(), o_f.data_ptr(), ws.data_ptr(), 256, stream)

        got, ref = fused(), comp()
        diff = {k: float((got[k] - r).abs().max()) for k, r in zip(("normal", "depth_max_w", "flow"), ref)}
        sf, sc, sk = _alternate([fused, comp, calls], [_timed, _timed, _timed], a.repeats)
        sk = {k: (v / CALLS if k.endswith("_ms") else v) for k, v in sk.items()}
        alg, touched = R * S * 28, R * S * 36
        gbs = alg / (sk["median_ms"] * 1e-3) / 1e9
        ray_rows.append({"R": R, "S": S, "K": K, "fused": sf, "composed": sc, "fused_c_call": sk,
                         "composed_over_fused": sc["median_ms"] / sf["median_ms"], "algorithmic_bytes": alg,
                         "touched_bytes_ld4": touched, "c_call_GBps_algorithmic": gbs,
                         "c_call_GBps_touched": touched / (sk["median_ms"] * 1e-3) / 1e9,
                         "c_call_share_of_hbm_peak_algorithmic": gbs / HBM_PEAK_GBS, "max_abs_diff": diff})
        del pbuf, nbuf, pts, normals, w
    img_rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        rgb = torch.rand(H, W, 3, generator=g).to(dev)
        depth, dmw, wz = (torch.rand(H, W, generator=g).to(dev) * 4.5 + 0.5 for _ in range(3))
        normal = (0.7 * torch.randn(H, W, 3, generator=g)).to(dev)
        flow = (3 * torch.randn(H, W, 2, generator=g)).to(dev)
        fused = lambda: visual_images(rgb, depth, dmw, wz, normal, flow)  # noqa: E731
        fused_host = lambda: {k: v.cpu() for k, v in visual_images(rgb, depth, dmw, wz, normal, flow).items()}  # noqa: E731
        comp = lambda: host_images(rgb, depth, dmw, wz, normal)  # noqa: E731
        same = bool(np.array_equal(fused()["disparity"].cpu().numpy(), comp()[1]))
        sf, sfh, sc = _alternate([fused, fused_host, comp], [_timed, _timed_host, _timed_host], a.repeats)
        img_rows.append({"H": H, "W": W, "fused_device": sf, "fused_with_copies_to_host": sfh, "composed_host": sc,
                         "composed_over_fused_with_copies": sc["median_ms"] / sfh["median_ms"],
                         "disparity_equal": same})
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "hbm_peak_GBps": HBM_PEAK_GBS,
           "per_ray": ray_rows, "per_image": img_rows}
    print(json.dumps(res))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "visuals_bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return res


if __name__ == "__main__":
    main()
