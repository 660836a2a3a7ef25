"""ICP registration timings on the device (cn_cloud_transform, the correspondence pass, cn_icp_accumulate,
metrics.icp_register_stages), on tools/mesh_eval_bench.py's synthetic surface: the targets are its noisy sphere shell
(unit sphere, 1 % radial noise), the source is area-weighted samples of its sphere mesh taken through the inverse of a
small rigid motion -- 1 M targets with 200 k source samples and 4 M targets with 1 M.

    python tools/icp_bench.py [--sizes 1000000:200000 4000000:1000000] [--repeats 7] [--baseline-size 1000000] [--out DIR]

Per size, each figure the median of `repeats` calls timed with device events after two warm-up calls, with the
min .. max spread beside it:
  correspond_composed   one iteration's correspondence pass as icp_register makes it: cloud_transform + binning the
                        moved cloud (nn_grid) + cn_nn_query on the binned records;
  accumulate_point / accumulate_plane   cn_icp_accumulate, both modes;
  register_3_stages     metrics.icp_register_stages, three stages (reach 0.1 / 0.03 / 0.01 at stride 8 / 4 / 1, at most
                        20 iterations each), timed with a host clock around the whole call (it ends in read-backs).
At --baseline-size targets the same three stages run on the host for comparison: scipy's cKDTree for the correspondences
(built once; query on OMP_NUM_THREADS workers, or on at most 16 cores when it is not set), numpy for the sums and
metrics.icp_solve_point for the steps, with the same stopping rule -- when scipy can be imported, otherwise stated as
absent.  Prints a JSON line; with --out also writes DIR/icp_bench.json.
profiles/icp_bench.json is the run that decided how the correspondences are made: it was taken while a kernel that fused
the transform into the search (cn_icp_correspond, on records binned once) still existed, has that kernel's figures
(correspond_fused, correspond_fused_raw) beside the composition's, found it slower at both sizes, and the kernel was
removed with its arms of this tool; its register_3_stages figures are with that kernel in the loop."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT, os.path.join(ROOT, "tools")]

from mesh_eval_bench import _stat, cpu_model, shell, sphere_mesh  # noqa: E402

STAGES = [dict(max_corr_dist=0.1, stride=8, max_iters=20), dict(max_corr_dist=0.03, stride=4, max_iters=20),
          dict(max_corr_dist=0.01, stride=1, max_iters=20)]


def motion():
    a = math.radians(2.0)
    M = np.eye(4)
    M[:3, :3] = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
    M[:3, 3] = (0.01, -0.008, 0.012)
    return M


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, repeats, warmup=2):
    """The device-event times of each of fns, called in turn `repeats` times after `warmup` rounds."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            ms[k].append(_timed(fn))
    return [_stat(m) for m in ms]


def host_register(src, tgt, stages, tol=1e-6):
    """The stages of metrics.icp_register_stages (point mode) on the host: (transform, iterations, seconds for the
    tree, seconds for the loop)."""
    from scipy.spatial import cKDTree
    from copenerf import metrics
    workers = int(os.environ.get("OMP_NUM_THREADS") or min(os.cpu_count() or 1, 16))
    t0 = time.perf_counter()
    tree = cKDTree(tgt)
    t1 = time.perf_counter()
    tgt64 = tgt.astype(np.float64)
    pivot = 0.5 * (tgt64.min(0) + tgt64.max(0))
    T, total = np.eye(4), 0
    for st in stages:
        p = src[::st["stride"]].astype(np.float64)
        history, iterations = [], 0
        while True:
            moved = p @ T[:3, :3].T + T[:3, 3]
            dist, idx = tree.query(moved, k=1, distance_upper_bound=st["max_corr_dist"], workers=workers)
            ok = np.isfinite(dist)
            a, b = moved[ok] - pivot, tgt64[idx[ok]] - pivot
            s = np.zeros(32)
            s[0], s[1] = ok.sum(), (dist[ok] ** 2).sum()
            s[2:5], s[5:8], s[8:17], s[17] = a.sum(0), b.sum(0), (b.T @ a).reshape(-1), (a * a).sum()
            fitness, rmse = s[0] / len(p), math.sqrt(s[1] / s[0])
            history.append((fitness, rmse))
            done = len(history) > 1 and abs(fitness - history[-2][0]) < tol and abs(rmse - history[-2][1]) < tol
            if done or iterations == st["max_iters"]:
                break
            T = metrics.icp_solve_point(s, False, pivot) @ T
            iterations += 1
        total += iterations
    return T, total, t1 - t0, time.perf_counter() - t1, workers


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["1000000:200000", "4000000:1000000"], metavar="TARGETS:SOURCES")
    ap.add_argument("--baseline-size", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    sizes = [tuple(int(x) for x in s.split(":")) for s in a.sizes]
    if not torch.cuda.is_available():
        raise SystemExit("icp_bench: needs a HIP device; nothing is measured without one")
    from copenerf import _lib, metrics, ops
    dev = torch.device("cuda")
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    v, f = sphere_mesh(512, 1024, dev)
    handle, area = ops.mesh_area(v, f)  # (the sampler reads `area` on the device: it has to stay alive with the handle)
    M = motion()
    Minv = np.linalg.inv(M)
    rows = []
    for n, q in sizes:
        tgt = shell(n, 2, dev)
        normals = torch.nn.functional.normalize(tgt, dim=1).contiguous()
        samples, _ = ops.mesh_sample(handle, q, torch.tensor([1, 0], dtype=torch.uint64, device=dev))
        src = ops.cloud_transform(samples, Minv)
        box = torch.stack([tgt.amin(0), tgt.amax(0)]).tolist()
        cell, dims = metrics.nn_cell_size(box[0], box[1], n)
        pivot = [0.5 * (l + h) for l, h in zip(*box)]
        grid = ops.nn_grid(tgt, box[0], cell, dims)
        reach = 0.03
        T = M.copy()
        T[:3, 3] += 0.002  # an iterate near, not at, the answer

        def composed():
            moved = ops.cloud_transform(src, T)
            return ops.nn_query(grid, ops.nn_grid(moved, box[0], cell, dims).sorted, reach, records=True)[1]

        (t_composed,) = alternate([composed], a.repeats)
        index = composed()
        t_point, t_plane = alternate([lambda: ops.icp_accumulate(src, tgt, index, T, pivot, 0),
                                      lambda: ops.icp_accumulate(src, tgt, index, T, pivot, 1, normals)], a.repeats)
        walls, res = [], None
        for k in range(3):  # the first run warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = metrics.icp_register_stages(src, tgt, STAGES)
            torch.cuda.synchronize()
            if k:
                walls.append((time.perf_counter() - t0) * 1e3)
        row = {"n_targets": n, "n_source": q, "mesh_area": float(area.item()), "cell": cell, "dims": list(dims), "reach": reach,
               "pairs_found": int((index >= 0).sum()), "correspond_composed": t_composed,
               "accumulate_point": t_point, "accumulate_plane": t_plane,
               "register_3_stages": {"wall_ms": walls, "iterations": res.iterations, "converged": res.converged,
                                     "fitness": res.fitness, "inlier_rmse": res.inlier_rmse,
                                     "translation_error": float(np.abs(res.transform[:3, 3] - M[:3, 3]).max())}}
        if n == a.baseline_size:
            try:
                import scipy  # noqa: F401
            except ImportError:
                row["cpu_baseline"] = "absent: scipy cannot be imported here"
            else:
                Th, its, build_s, loop_s, workers = host_register(src.cpu().numpy(), tgt.cpu().numpy(), STAGES)
                row["cpu_baseline"] = {"what": "scipy.spatial.cKDTree + numpy sums + icp_solve_point, the same stages, one run",
                                       "workers": workers, "tree_build_ms": build_s * 1e3, "loop_ms": loop_s * 1e3,
                                       "total_ms": (build_s + loop_s) * 1e3, "iterations": its, "cpu_model": cpu_model(),
                                       "max_abs_transform_diff": float(np.abs(Th - res.transform).max())}
                row["speedup_over_cpu"] = row["cpu_baseline"]["total_ms"] / min(walls)
        rows.append(row)
        print(f"icp_bench: {n} targets x {q} source points done", file=sys.stderr)
        del tgt, normals, samples, src, grid, index
    out = {"library": stamp, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "stages": STAGES, "rows": rows}
    print(json.dumps(out))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "icp_bench.json"), "w") as fh:
            json.dump(out, fh, indent=1)
    return out


if __name__ == "__main__":
    main()
