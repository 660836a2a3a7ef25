"""Mesh depth rendering, visibility and cull timings on the device (cn_mesh_raster, cn_mesh_visibility,
cn_mesh_select_mask + cn_mesh_compact) on the workload they were written for: a marching-tetrahedra sphere (radius
0.8 in the box -1 .. 1, ops.isosurface of the analytic distance on a res^3 grid) seen from cameras on a ring 2.2
away, at 480 x 640.

    python tools/mesh_raster_bench.py [--res 256 512] [--views 8 64] [--repeats 7] [--budgets 16 64 256] [--out DIR]

Every figure is the median of `repeats` timed calls after two warm-up calls, each timed with device events (the cull
with a host clock around a synchronise: it reads 16 bytes back), with the min .. max spread beside it; the device's
clocks as rocm-smi reports them before and after are recorded as text (nothing is set).  Per row:
  pairs_per_s      triangle x views per second of ops.mesh_raster;
  model_bytes      what the passes must move, from shapes: per batch 12 V read + 16 B V written (projection), per view
                   12 T + 48 T read (indices, three projected corners), 8 h w written (clear) and 8 h w read + 8 h w
                   written (unpack); the z-buffer atomics and their reads are NOT in it (they depend on coverage);
  share_of_hbm     model_bytes / time over 6.29 TB/s, the float4-copy rate of the card (8.0 TB/s is the data-sheet peak);
  group_share      the share of rasterised (triangle, view) pairs that took the workgroup path.
--budgets repeats the first row with other pixel budgets.  Prints one JSON line; with --out also writes
DIR/mesh_raster_bench.json (profiles/mesh_raster_bench.json is one such run)."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]

H, W, RADIUS, DIST = 480, 640, 0.8, 2.2
HBM_COPY_BYTES_PER_S = 6.29e12


def _events(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def _host(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def _stat(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def _clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30).stdout
        lines = [ln.strip() for ln in out.splitlines() if "clk" in ln.lower()]
        return lines or "not reported"
    except (OSError, subprocess.SubprocessError):
        return "not measured: rocm-smi is not available"


def sphere_mesh(res, dev):
    """The isosurface |x| = RADIUS of the analytic distance on a res^3 grid over -1 .. 1."""
    from copenerf import ops
    ax = torch.linspace(-1.0, 1.0, res, device=dev)
    u = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - RADIUS
    return ops.isosurface(u.contiguous(), 0.0, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def ring_views(n):
    """n cameras on a tilted ring DIST from the origin, looking at it: x right, y up, looking down -z."""
    views = []
    for i in range(n):
        a = 2 * math.pi * i / n
        eye = DIST * np.array([math.cos(a) * 0.9, math.sin(a) * 0.9, 0.436 * math.cos(2 * a + 0.3)])
        back = eye / np.linalg.norm(eye)
        right = np.cross((0.0, 0.0, 1.0), back)
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(back, right), back])
        Wm = np.eye(4)
        Wm[:3, :3], Wm[:3, 3] = R, -R @ eye
        f = 0.9 * H
        views.append({"camera_mat": np.diag([2 * f / W, -2 * f / H, -1.0, 1.0]), "world_mat": Wm})
    return views


def model_bytes(V, T, N, batch=8):
    batches = -(-N // batch)
    return 12 * V * batches + N * (16 * V + 60 * T + 24 * H * W)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--budgets", type=int, nargs="*", default=[16, 64, 256])
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_raster_bench: needs a HIP device; nothing is measured without one")
    from copenerf import _lib, mesh, ops
    dev = torch.device("cuda")
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W],
           "clocks_before": _clocks(), "rows": [], "budget_rows": []}
    first = None
    for n in a.res:
        v, f = sphere_mesh(n, dev)
        V, T = v.shape[0], f.shape[0]
        for N in a.views:
            proj = mesh.view_projections(ring_views(N), (H, W), None, dev)
            stats = {}
            depth, tri = ops.mesh_raster(v, f, proj, H, W, stats=stats)
            covered = float((tri >= 0).float().mean())
            raster = _stat(_events(lambda: ops.mesh_raster(v, f, proj, H, W), a.repeats))
            vis = _stat(_events(lambda: ops.mesh_visibility(v, proj, H, W, depth=depth, tol_rel=0.01), a.repeats))
            frustum = _stat(_events(lambda: ops.mesh_visibility(v, proj, H, W), a.repeats))
            keep = ops.mesh_visibility(v, proj, H, W, depth=depth, tol_rel=0.01) >= 1
            cull = _stat(_host(lambda: ops.mesh_cull(v, f, keep), a.repeats))
            kept_t = ops.mesh_cull(v, f, keep)[1].shape[0]
            walked = stats["thread_pairs"] + stats["group_pairs"]
            mb = model_bytes(V, T, N)
            s = raster["median_ms"] * 1e-3
            row = {"res": n, "vertices": V, "triangles": T, "views": N, "covered_pixel_share": covered,
                   "raster": raster, "pairs": T * N, "pairs_per_s": T * N / s, "model_bytes": mb,
                   "model_bytes_per_s": mb / s, "share_of_hbm_copy_rate": mb / s / HBM_COPY_BYTES_PER_S,
                   "walked_pairs": walked, "walked_share_of_pairs": walked / (T * N),
                   "group_pairs": stats["group_pairs"], "group_share": stats["group_pairs"] / max(walked, 1),
                   "visibility_with_depth": vis, "visibility_frustum": frustum,
                   "point_views_per_s": V * N / (vis["median_ms"] * 1e-3), "cull": cull, "cull_kept_triangles": kept_t}
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            if first is None:
                first = (n, N)
                for b in a.budgets:
                    st = {}
                    ops.mesh_raster(v, f, proj, H, W, pixel_budget=b, stats=st)
                    t = _stat(_events(lambda: ops.mesh_raster(v, f, proj, H, W, pixel_budget=b), a.repeats))
                    res["budget_rows"].append({"res": n, "views": N, "pixel_budget": b, "raster": t,
                                               "group_pairs": st["group_pairs"], "thread_pairs": st["thread_pairs"]})
        del v, f
        torch.cuda.empty_cache()
    res["clocks_after"] = _clocks()
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "mesh_raster_bench.json"), "w") as fh:
            json.dump(res, fh, indent=1)
    return res


if __name__ == "__main__":
    main()
