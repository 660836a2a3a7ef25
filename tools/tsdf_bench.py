"""TSDF fusion timings on the device (cn_tsdf_integrate, cn_tsdf_finalize, the observed-only mesher, cn_volume_sample)
on the workload they were written for: the depth of a marching-tetrahedra sphere (radius 0.8 in the box -1 .. 1,
tools/mesh_raster_bench.py's mesh at 256^3) rendered by mesh.render_mesh_depth from cameras on a ring 2.2 away at
480 x 640, fused into a res^3 volume over the same box with a truncation of four voxels.

    python tools/tsdf_bench.py [--res 256 512] [--views 8 64] [--repeats 5] [--out DIR]

Every figure is the median of `repeats` timed calls after two warm-up calls, each timed with device events (the mesher
with a host clock around a synchronise: it reads 16 bytes back), with the min .. max spread beside it; the device's
clocks as rocm-smi reports them before and after are recorded as text (nothing is set).  Per row:
  integrate            ops.tsdf_integrate, all views in one call, alternated call by call in the same process with
  torch_integrate      the same rule as a torch composition on the device (one pass of elementwise ops and a gather
                       per view over the whole volume; `torch_equal`: its volumes are bitwise the kernel's);
  kernel_over_torch    the ratio of the two medians (the condition: at most 1 at every row);
  integrate_no_reject  the kernel with the wavefront-level frustum skip turned off: what the skip saves;
  integrate_by_8_views the same views in calls of 8 (fusion.VIEWS_PER_CALL): the volumes are read and written once per
                       call, and yet the per-view cost of one long call is the higher one;
  voxel_views_per_s    res^3 x views over the kernel's median;
  model_bytes          what the call must move, from shapes: tsum and wsum read once and written once (16 bytes a
                       voxel) and every depth image read once (4 h w a view);
  share_of_hbm         model_bytes / time over 6.29 TB/s, the float4-copy rate of the card;
  finalize, mesher (ops.isosurface(observed=True)), sampler (ops.volume_sample of u at the mesh's vertices, masked).
Prints one JSON line; with --out also writes DIR/tsdf_bench.json (profiles/tsdf_bench.json is one such run)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT, os.path.join(ROOT, "tools")]

from mesh_raster_bench import H, HBM_COPY_BYTES_PER_S, W, _clocks, _host, _stat, ring_views, sphere_mesh  # noqa: E402

MESH_RES = 256
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def _alternate(fn_a, fn_b, repeats, warmup=2):
    """Device-event times of fn_a and fn_b, alternated call by call: ([ms of a], [ms of b])."""
    for _ in range(warmup):
        fn_a()
        fn_b()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(repeats):
        for fn, ms in zip((fn_a, fn_b), out):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    return out


def torch_integrate(tsum, wsum, axes, P_host, depth, trunc, near):
    """cn_tsdf_integrate's rule, view by view, as torch ops over the whole volume (no depth_max, no colours)."""
    x, y, z = axes
    N, h, w = depth.shape
    # (a device scalar: torch divides by a host scalar as a multiplication by its reciprocal, which rounds otherwise)
    trunc = torch.tensor(trunc, dtype=torch.float32, device=depth.device)
    for v in range(N):
        p = P_host[v]
        a = ((p[0][0] * x + p[0][1] * y) + p[0][2] * z) + p[0][3]
        b = ((p[1][0] * x + p[1][1] * y) + p[1][2] * z) + p[1][3]
        c = ((p[2][0] * x + p[2][1] * y) + p[2][2] * z) + p[2][3]
        fx, fy = torch.floor(a / c + 0.5), torch.floor(b / c + 0.5)
        inside = (c >= near) & (fx >= 0) & (fx <= w - 1) & (fy >= 0) & (fy <= h - 1)
        idx = fy.clamp(0, h - 1).long() * w + fx.clamp(0, w - 1).long()
        d = depth[v].reshape(-1)[idx]
        s = d - c
        hit = inside & torch.isfinite(d) & (d > 0) & (s >= -trunc)
        tsum += torch.where(hit, torch.clamp(s / trunc, max=1.0), torch.zeros_like(s))
        wsum += hit.to(torch.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench: needs a HIP device; nothing is measured without one")
    from copenerf import _lib, mesh, ops
    dev = torch.device("cuda")
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W],
           "mesh_res": MESH_RES, "clocks_before": _clocks(), "rows": []}
    mv, mf = sphere_mesh(MESH_RES, dev)
    renders = {}
    for N in a.views:
        views = ring_views(N)
        depth = mesh.render_mesh_depth(mv, mf, views, (H, W))["depth"]
        renders[N] = (mesh.view_projections(views, (H, W), None, dev), depth.contiguous())
    del mv, mf
    for n in a.res:
        trunc = 4.0 * 2.0 / (n - 1)
        # the kernel's voxel map (divided by a device scalar: see torch_integrate)
        ax = torch.arange(n, device=dev, dtype=torch.float32) / torch.tensor(float(n - 1), device=dev) * 2.0 + (-1.0)
        axes = (ax[:, None, None], ax[None, :, None], ax[None, None, :])
        for N in a.views:
            proj, depth = renders[N]
            P_host = proj.cpu().tolist()
            tsum, wsum = torch.zeros(n, n, n, device=dev), torch.zeros(n, n, n, device=dev)
            ops.tsdf_integrate(tsum, wsum, *BOX, proj, depth, trunc)
            t2, w2 = torch.zeros_like(tsum), torch.zeros_like(wsum)
            torch_integrate(t2, w2, axes, P_host, depth, trunc, ops.MESH_NEAR)
            equal = bool(torch.equal(tsum, t2) and torch.equal(wsum, w2))
            differ = int((tsum != t2).sum() + (wsum != w2).sum())
            observed = float((wsum > 0).float().mean())
            del t2, w2
            ka, kb = torch.zeros_like(tsum), torch.zeros_like(wsum)
            ta, tb = torch.zeros_like(tsum), torch.zeros_like(wsum)
            k_ms, t_ms = _alternate(lambda: ops.tsdf_integrate(ka, kb, *BOX, proj, depth, trunc),
                                    lambda: torch_integrate(ta, tb, axes, P_host, depth, trunc, ops.MESH_NEAR), a.repeats)
            del ta, tb
            torch.cuda.empty_cache()
            k2_ms, nr_ms = _alternate(lambda: ops.tsdf_integrate(ka, kb, *BOX, proj, depth, trunc),
                                      lambda: ops.tsdf_integrate(ka, kb, *BOX, proj, depth, trunc, brick_reject=False),
                                      a.repeats)
            by8_ms, _ = _alternate(lambda: [ops.tsdf_integrate(ka, kb, *BOX, proj[i:i + 8], depth[i:i + 8], trunc)
                                            for i in range(0, N, 8)], lambda: None, a.repeats)
            del ka, kb
            kern, tor, kern2, norej, by8 = _stat(k_ms), _stat(t_ms), _stat(k2_ms), _stat(nr_ms), _stat(by8_ms)
            fin = _stat(_alternate(lambda: ops.tsdf_finalize(tsum, wsum), lambda: None, a.repeats)[0])
            u = ops.tsdf_finalize(tsum, wsum)
            mesher = _stat(_host(lambda: ops.isosurface(u, 0.0, *BOX, observed=True), a.repeats))
            v, t = ops.isosurface(u, 0.0, *BOX, observed=True)
            sampler = _stat(_alternate(lambda: ops.volume_sample(u, v, *BOX, mask=u), lambda: None, a.repeats)[0])
            mb = 16 * n ** 3 + 4 * H * W * N
            s = kern["median_ms"] * 1e-3
            row = {"res": n, "views": N, "trunc": trunc, "observed_voxel_share": observed, "integrate": kern,
                   "torch_integrate": tor, "kernel_over_torch": kern["median_ms"] / tor["median_ms"],
                   "torch_equal": equal, "torch_differing_values": differ, "integrate_again": kern2,
                   "integrate_by_8_views": by8, "integrate_no_reject": norej, "reject_saves": 1.0 - kern2["median_ms"] / norej["median_ms"],
                   "voxel_views": n ** 3 * N, "voxel_views_per_s": n ** 3 * N / s, "model_bytes": mb,
                   "model_bytes_per_s": mb / s, "share_of_hbm_copy_rate": mb / s / HBM_COPY_BYTES_PER_S,
                   "finalize": fin, "mesher_observed": mesher, "mesh_vertices": v.shape[0], "mesh_triangles": t.shape[0],
                   "sampler": sampler}
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del tsum, wsum, u, v, t
            torch.cuda.empty_cache()
    res["clocks_after"] = _clocks()
    res["kernel_no_slower_than_torch_at_every_row"] = all(r["kernel_over_torch"] <= 1.0 for r in res["rows"])
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "tsdf_bench.json"), "w") as fh:
            json.dump(res, fh, indent=1)
    return res


if __name__ == "__main__":
    main()
