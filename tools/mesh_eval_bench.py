"""Mesh geometry metric timings on the device: the area-weighted surface sampler (cn_mesh_area, cn_mesh_sample),
the point grid (cn_nn_grid_build) and the exact nearest-neighbour query (cn_nn_query) in both sort_queries arms,
on a synthetic surface -- a noisy sphere shell (unit sphere, 1 % radial noise), queries and targets drawn alike
with different seeds -- at 1 M x 1 M and 4 M x 4 M points; and a CPU baseline on the same data at 1 M x 1 M:
scipy's cKDTree (build + query on OMP_NUM_THREADS workers, or every core when it is not set), when scipy can be
imported, otherwise stated as absent.

    python tools/mesh_eval_bench.py [--sizes 1000000 4000000] [--repeats 7] [--cell-scales 0.5 0.7 1.4] [--out DIR]

Every device figure is the median of `repeats` timed calls after two warm-up calls, each call timed with device
events, with the min .. max spread beside it.  `query_sorted_total` is what sort_queries=True costs end to end
(binning the queries through the targets' grid, then the query on the binned records); `query_unsorted` is the query
on the queries as they come.  The arm with the smaller total at every size is the default
(metrics.SORT_QUERIES_DEFAULT); the JSON says which, and why.  The two arms' outputs are compared bitwise, and
the device distances against the baseline's.  --cell-scales times the binned query and the grid build again with
the default cell edge (about 8 targets per cell over the box, metrics.nn_cell_size) multiplied by each factor, at
the first size: what the cell choice is worth.  Prints a JSON line; with --out also writes DIR/mesh_eval_bench.json
(profiles/mesh_eval_bench.json is one such run)."""
import argparse
import json
import math
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]


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


def _stat(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def shell(n, seed, dev):
    g = torch.Generator(device="cpu").manual_seed(seed)
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True) * (1.0 + 0.01 * torch.randn(n, 1, generator=g))
    return d.to(dev).contiguous()


def sphere_mesh(n_lat, n_lon, dev):
    """A latitude-longitude sphere: (n_lat + 1) x n_lon vertices, 2 n_lat n_lon triangles (the polar ones of zero
    area: the sampler skips them)."""
    th = torch.linspace(0, math.pi, n_lat + 1)[:, None]
    ph = torch.arange(n_lon)[None, :] * (2 * math.pi / n_lon)
    v = torch.stack([th.sin() * ph.cos(), th.sin() * ph.sin(), th.cos().expand(-1, n_lon)], -1).reshape(-1, 3)
    i = torch.arange(n_lat)[:, None] * n_lon
    j = torch.arange(n_lon)[None, :]
    a, b = i + j, i + (j + 1) % n_lon
    f = torch.cat([torch.stack([a, a + n_lon, b], -1), torch.stack([b, a + n_lon, b + n_lon], -1)]).reshape(-1, 3)
    return v.float().contiguous().to(dev), f.int().contiguous().to(dev)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--baseline-size", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cell-scales", type=float, nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_eval_bench: needs a HIP device; nothing is measured without one")
    from copenerf import _lib, metrics, ops
    dev = torch.device("cuda")
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    rows = []
    v, f = sphere_mesh(512, 1024, dev)
    philox = torch.tensor([1, 0], dtype=torch.uint64, device=dev)
    for n in a.sizes:
        q, t = shell(n, 1, dev), shell(n, 2, dev)
        area = _stat(_events(lambda: ops.mesh_area(v, f), a.repeats))
        handle, _ = ops.mesh_area(v, f)
        sample = _stat(_events(lambda: ops.mesh_sample(handle, n, philox), a.repeats))
        box = torch.stack([t.amin(0), t.amax(0)]).tolist()
        cell, dims = metrics.nn_cell_size(box[0], box[1], n)
        build = _stat(_events(lambda: ops.nn_grid(t, box[0], cell, dims), a.repeats))
        grid = ops.nn_grid(t, box[0], cell, dims)
        binned = ops.nn_grid(q, box[0], cell, dims)
        unsorted = _stat(_events(lambda: ops.nn_query(grid, q), a.repeats))
        sorted_query = _stat(_events(lambda: ops.nn_query(grid, binned.sorted, records=True), a.repeats))
        sorted_total = _stat(_events(
            lambda: ops.nn_query(grid, ops.nn_grid(q, box[0], cell, dims).sorted, records=True), a.repeats))
        du, iu = ops.nn_query(grid, q)
        ds, is_ = ops.nn_query(grid, binned.sorted, records=True)
        occupied = int((grid.cell_start[1:] > grid.cell_start[:-1]).sum())
        row = {"n_queries": n, "n_targets": n, "cell": cell, "dims": list(dims), "occupied_cells": occupied,
               "targets_per_occupied_cell": n / max(occupied, 1), "mesh_triangles": f.shape[0], "mesh_area": area,
               "mesh_sample": sample, "grid_build": build, "query_unsorted": unsorted, "query_sorted": sorted_query,
               "query_sorted_total": sorted_total, "arms_bitwise_equal": bool(torch.equal(du, ds) and torch.equal(iu, is_)),
               "mean_distance": float(du.double().mean())}
        if n == a.baseline_size:
            try:
                from scipy.spatial import cKDTree
            except ImportError:
                row["cpu_baseline"] = "absent: scipy cannot be imported here"
            else:
                qn, tn = q.cpu().numpy(), t.cpu().numpy()
                workers = int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1)
                t0 = time.perf_counter()
                tree = cKDTree(tn)
                t1 = time.perf_counter()
                dk, ik = tree.query(qn, k=1, workers=workers)
                t2 = time.perf_counter()
                row["cpu_baseline"] = {"what": "scipy.spatial.cKDTree, build + query(k=1), one run", "workers": workers,
                                       "build_ms": (t1 - t0) * 1e3, "query_ms": (t2 - t1) * 1e3,
                                       "total_ms": (t2 - t0) * 1e3, "cpu_model": cpu_model(),
                                       "max_abs_distance_diff": float(np.abs(dk - du.cpu().numpy()).max()),
                                       "index_mismatches": int((ik != iu.cpu().numpy()).sum())}
                best = min(unsorted["median_ms"], sorted_total["median_ms"]) + build["median_ms"]
                row["speedup_over_cpu"] = row["cpu_baseline"]["total_ms"] / best
        if n == a.sizes[0] and a.cell_scales:
            row["cell_sweep"] = []
            for k in a.cell_scales:
                c = cell * k
                dm = tuple(int((h - l) / c) + 1 for l, h in zip(*box))
                g = ops.nn_grid(t, box[0], c, dm)
                total = _stat(_events(lambda: ops.nn_query(g, ops.nn_grid(q, box[0], c, dm).sorted, records=True), a.repeats))
                d2, i2 = ops.nn_query(g, ops.nn_grid(q, box[0], c, dm).sorted, records=True)
                row["cell_sweep"].append({"scale": k, "cell": c, "dims": list(dm),
                                          "grid_build": _stat(_events(lambda: ops.nn_grid(t, box[0], c, dm), a.repeats)),
                                          "query_sorted_total": total,
                                          "bitwise_equal_to_default": bool(torch.equal(d2, du) and torch.equal(i2, iu))})
                del g
        rows.append(row)
        del q, t, grid, binned, du, iu, ds, is_
    sorted_wins = all(r["query_sorted_total"]["median_ms"] < r["query_unsorted"]["median_ms"] for r in rows)
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "rows": rows,
           "default_sort_queries": sorted_wins,
           "default_reason": ("binning the queries plus the query on the binned records is faster than the query on "
                              "unordered queries at every size measured" if sorted_wins else
                              "the query on unordered queries is at least as fast as binning plus the binned query "
                              "at some size measured"),
           "library_default": metrics.SORT_QUERIES_DEFAULT}
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "mesh_eval_bench.json"), "w") as fh:
            json.dump(res, fh, indent=1)
    return res


if __name__ == "__main__":
    main()
