"""Mesh shading timings on the device (cn_mesh_shade) on tools/mesh_raster_bench.py's workload: a marching-tetrahedra
sphere (radius 0.8 in the box -1 .. 1 on a res^3 grid) seen from cameras on a ring 2.2 away, at 480 x 640.

    python tools/mesh_shade_bench.py [--res 256 512] [--views 8 64] [--repeats 7] [--out DIR]

Every figure is the median of `repeats` timed calls after two warm-up calls, each timed with device events, with the
min .. max spread beside it; the device's clocks as rocm-smi reports them before and after are recorded as text
(nothing is set).  Per row, for three sets of outputs -- the camera-frame normal map alone ("normal"), the two
pictures with vertex colours ("pictures": what tools/render_mesh.py writes) and everything with C = 3 attributes
("all"):
  shade            ops.mesh_shade alone, on a tri image rendered before the clock starts;
  raster_shade     ops.mesh_raster followed by ops.mesh_shade;
  model_bytes      what the shade pass must move, from shapes: per pixel 4 (tri) read; per covered pixel 12 (indices) +
                   36 (corners) + 12 C (attribute rows) + 36 (vertex normals, when given) read -- a gather that
                   neighbouring pixels share, so most of it comes from the caches, and the model is an upper bound on
                   the traffic to memory; plus the outputs written per pixel, 4 C + 12 + 3 + 3 of those asked for;
  share_of_hbm     model_bytes / time over 6.29 TB/s, the float4-copy rate of the card (8.0 TB/s is the data-sheet peak).
Prints one JSON line; with --out also writes DIR/mesh_shade_bench.json (profiles/mesh_shade_bench.json is one such
run).  Not measured here: counters (cache hit rates, occupancy) and the split of the time between the gather and the
stores."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT, os.path.join(ROOT, "tools")]

from mesh_raster_bench import H, HBM_COPY_BYTES_PER_S, W, _clocks, _events, _stat, ring_views, sphere_mesh  # noqa: E402

NOT_MEASURED = ["hardware counters (cache hit rates, occupancy, memory traffic): the byte model is from shapes",
                "the split of the time between the gather and the output stores",
                "images other than 480 x 640 and meshes other than the sphere"]


def model_bytes(N, covered_share, C, smooth, outputs):
    px = N * H * W
    read = 4 * px + covered_share * px * (12 + 36 + 12 * C + (36 if smooth else 0))
    per_px = {"attr": 4 * C, "normal": 12, "normal_image": 3, "shaded": 3}
    return read + px * sum(per_px[o] for o in outputs)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_shade_bench: needs a HIP device; nothing is measured without one")
    import numpy as np
    from copenerf import _lib, mesh, ops
    dev = torch.device("cuda")
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "image": [H, W],
           "clocks_before": _clocks(), "rows": [], "not_measured": NOT_MEASURED}
    for n in a.res:
        v, f = sphere_mesh(n, dev)
        V, T = v.shape[0], f.shape[0]
        colors = (v.abs() / v.abs().max()).contiguous()
        vn = torch.nn.functional.normalize(v, dim=-1).contiguous()
        for N in a.views:
            views = ring_views(N)
            proj = mesh.view_projections(views, (H, W), None, dev)
            rot = torch.as_tensor(np.stack([x["world_mat"][:3, :3] for x in views]), dtype=torch.float32).to(dev).contiguous()
            tri = ops.mesh_raster(v, f, proj, H, W)[1]
            covered = float((tri >= 0).float().mean())
            row = {"res": n, "vertices": V, "triangles": T, "views": N, "covered_pixel_share": covered, "cases": {}}
            cases = {"normal": dict(want=("normal",), rot=rot),
                     "pictures": dict(want=("normal_image", "shaded"), rot=rot, attr=colors, albedo_from_attr=True),
                     "all": dict(want=("attr", "normal", "normal_image", "shaded"), rot=rot, attr=colors, vnormals=vn,
                                 albedo_from_attr=True)}
            for name, kw in cases.items():
                shade = _stat(_events(lambda: ops.mesh_shade(v, f, proj, tri, **kw), a.repeats))
                both = _stat(_events(lambda: ops.mesh_shade(v, f, proj, ops.mesh_raster(v, f, proj, H, W)[1], **kw), a.repeats))
                C = 3 if "attr" in kw else 0
                mb = model_bytes(N, covered, C, "vnormals" in kw, kw["want"])
                s = shade["median_ms"] * 1e-3
                row["cases"][name] = {"shade": shade, "raster_shade": both, "model_bytes": mb, "model_bytes_per_s": mb / s,
                                      "share_of_hbm_copy_rate": mb / s / HBM_COPY_BYTES_PER_S,
                                      "pixels_per_s": N * H * W / s}
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        del v, f, colors, vn
        torch.cuda.empty_cache()
    res["clocks_after"] = _clocks()
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "mesh_shade_bench.json"), "w") as fh:
            json.dump(res, fh, indent=1)
    return res


if __name__ == "__main__":
    main()
