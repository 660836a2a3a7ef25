"""Point-cloud preparation timings on the device: the k-nearest search (cn_knn_query, the cloud against itself,
the queries binned through the grid), the normals from its rows (cn_cloud_normals) and voxel down-sampling
(cn_voxel_keys + the stable torch sort + cn_voxel_reduce), on tools/mesh_eval_bench.py's noisy sphere shell at 1 M and
4 M points for k = 8, 16 and 32 -- one capacity of the k-best list each; and the three-stage registration of
tools/icp_bench.py with and without a voxel down-sampling of both clouds first (what --icp-voxel does).

    python tools/cloud_bench.py [--sizes 1000000 4000000] [--ks 8 16 32] [--repeats 7] [--voxel 0.01]
        [--baseline-size 1000000] [--out DIR]

Every device figure is the median of `repeats` timed calls after two warm-up calls, each call timed with device
events, with the min .. max spread beside it.  The baseline at --baseline-size points is scipy's cKDTree:
build once, query(k=..., workers=16), wall clock, one run, stated as absent when scipy cannot be imported; its
neighbour indices are compared with the device's on the rows where they can be (no ties).  Prints a JSON line; with
--out also writes DIR/cloud_bench.json (profiles/cloud_bench.json is one such run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT, os.path.join(ROOT, "tools")]

from icp_bench import STAGES, motion  # noqa: E402
from mesh_eval_bench import _events, _stat, cpu_model, shell, sphere_mesh  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--ks", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--voxel", type=float, default=0.01)
    ap.add_argument("--baseline-size", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cloud_bench: needs a HIP device; nothing is measured without one")
    from copenerf import _lib, metrics, ops
    dev = torch.device("cuda")
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    rows = []
    for n in a.sizes:
        pts = shell(n, 2, dev)
        box = torch.stack([pts.amin(0), pts.amax(0)]).tolist()
        cell, dims = metrics.nn_cell_size(box[0], box[1], n)
        row = {"points": n, "cell": cell, "dims": list(dims),
               "grid_build": _stat(_events(lambda: ops.nn_grid(pts, box[0], cell, dims), a.repeats)), "k": {}}
        grid = ops.nn_grid(pts, box[0], cell, dims)
        tree = None
        for k in a.ks:
            entry = {"knn_query": _stat(_events(lambda: ops.knn_query(grid, grid.sorted, k, records=True), a.repeats))}
            dist, index, _ = ops.knn_query(grid, grid.sorted, k, records=True)
            entry["cloud_normals"] = _stat(_events(lambda: ops.cloud_normals(pts, index), a.repeats))
            entry["knn_mean_stats"] = _stat(_events(lambda: ops.knn_mean_stats(dist, index), a.repeats))
            if n == a.baseline_size:
                try:
                    from scipy.spatial import cKDTree
                    host = pts.cpu().numpy()
                    t0 = time.perf_counter()
                    tree = cKDTree(host) if tree is None else tree
                    t1 = time.perf_counter()
                    d_host, i_host = tree.query(host, k=k, workers=16)
                    t2 = time.perf_counter()
                    d_host, i_host = d_host.reshape(n, k), i_host.reshape(n, k)
                    same = (i_host == index.cpu().numpy()).all(1)
                    entry["cpu_baseline"] = {"what": "scipy.spatial.cKDTree.query(k, workers=16), wall clock, one run",
                                             "cpu": cpu_model(), "build_ms": (t1 - t0) * 1e3, "query_ms": (t2 - t1) * 1e3,
                                             "rows_with_equal_indices": float(same.mean()),
                                             "max_abs_distance_difference": float(np.abs(d_host - dist.cpu().numpy()).max())}
                except ImportError:
                    entry["cpu_baseline"] = "absent: scipy cannot be imported"
            row["k"][str(k)] = entry
        def voxel():
            keys, _ = ops.voxel_keys(pts, box[0], a.voxel)
            skeys, order = torch.sort(keys, stable=True)
            return ops.voxel_reduce(skeys, order, pts)
        row["voxel_down_sample"] = dict(_stat(_events(voxel, a.repeats)), voxel=a.voxel, voxels=int(voxel()["totals"][0].item()))
        row["voxel_keys"] = _stat(_events(lambda: ops.voxel_keys(pts, box[0], a.voxel), a.repeats))
        keys, _ = ops.voxel_keys(pts, box[0], a.voxel)
        row["stable_sort"] = _stat(_events(lambda: torch.sort(keys, stable=True), a.repeats))
        skeys, order = torch.sort(keys, stable=True)
        row["voxel_reduce"] = _stat(_events(lambda: ops.voxel_reduce(skeys, order, pts), a.repeats))
        rows.append(row)
        del pts, grid, keys, skeys, order
    # the three-stage registration of icp_bench (200 k mesh samples onto 1 M shell points), with and without voxels
    v, f = sphere_mesh(512, 1024, dev)
    handle, area = ops.mesh_area(v, f)  # (the sampler reads `area` on the device: it has to stay alive with the handle)
    tgt = shell(a.sizes[0], 2, dev)
    samples, _ = ops.mesh_sample(handle, max(a.sizes[0] // 5, 1), torch.tensor([1, 0], dtype=torch.uint64, device=dev))
    M = motion()
    src = ops.cloud_transform(samples, np.linalg.inv(M))

    def plain():
        return metrics.icp_register_stages(src, tgt, STAGES)

    def with_voxel():
        return metrics.icp_register_stages(metrics.voxel_down_sample(src, a.voxel)["points"],
                                           metrics.voxel_down_sample(tgt, a.voxel)["points"], STAGES)
    icp = {"targets": a.sizes[0], "sources": int(src.shape[0]), "voxel": a.voxel, "stages": STAGES}
    for name, fn in (("register_3_stages", plain), ("register_3_stages_voxel", with_voxel)):
        walls, res = [], None
        for _ in range(3):  # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        icp[name] = {"wall_ms": walls, "iterations": res.iterations, "converged": res.converged,
                     "max_abs_transform_error": float(np.abs(res.transform - M).max())}
    out = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "rows": rows, "icp": icp}
    print(json.dumps(out))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "cloud_bench.json"), "w") as fh:
            json.dump(out, fh, indent=1)
    return out


if __name__ == "__main__":
    main()
