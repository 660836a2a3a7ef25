"""Mesh extraction timings on the device: cn_sdf_grid and the mesher's two passes (cn_mesh_count, cn_mesh_emit)
at 256^3 and 512^3 with the C2 network (d_hidden 256) in bf16x6, against the reference-shaped baseline built
from the product API (extract_fields, neus_renderer.py:10-25: 64^3 blocks through SDFNetwork.sdf with a host copy
per block); and, on the extracted mesh, the colour pass (one cn_point_colors call next to the chunked module
composition with the same packs: the same launches, so this measures the per-chunk Python loop, nothing else) and the
clean pass (ops.mesh_clean keep_largest, host clock: it reads the `changed` flag and the counts back).  With --out
the colour and clean figures also go to DIR/mesh_color_bench.json (profiles/mesh_color_bench.json is one such run).

    python tools/mesh_bench.py [--res 256 512] [--repeats 7] [--out DIR]

Every figure is the median of `repeats` timed calls after two warm-up calls, each call timed with device
events (the baseline with a host clock: it ends in host copies), with the min .. max spread beside it.  The
mesher's bytes/s are its algorithmic bytes over the measured time: u once per pass plus the pass's outputs
(count: the edge masks, triangle counts and both offset arrays; emit: the vertices and triangles).  Prints a
JSON line and a markdown table (also written under --out) stamped with the library's build digest."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]

BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


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


def _host(fn, repeats, warmup=1):
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


def baseline_fields(sdf_network, n, t, block=64):
    """extract_fields (neus_renderer.py:10-25) with the (x, y, z, t) query: 64^3 blocks, a host copy per block."""
    import numpy as np
    ax = [torch.linspace(BOX[0][a], BOX[1][a], n).cuda().split(block) for a in range(3)]
    u = np.zeros([n, n, n], dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(ax[0]):
            for yi, ys in enumerate(ax[1]):
                for zi, zs in enumerate(ax[2]):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1),
                                     torch.full((xx.numel(), 1), t, device="cuda")], dim=-1)
                    val = sdf_network.sdf(pts).reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
                    u[xi * block: xi * block + len(xs), yi * block: yi * block + len(ys),
                      zi * block: zi * block + len(zs)] = val
    return u


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--baseline-repeats", type=int, default=3)
    ap.add_argument("--time", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench: needs a HIP device; nothing is measured without one")
    from copenerf import NeuSRenderer, _lib, ops
    from copenerf.fields import RenderingNetwork, SDFNetwork, SingleVarianceNetwork
    from copenerf.train_step import COL_CFG, REN_CFG, SDF_CFG
    torch.manual_seed(0)
    r = NeuSRenderer(None, SDFNetwork(**SDF_CFG), SingleVarianceNetwork(0.3), RenderingNetwork(**COL_CFG), None,
                     **REN_CFG).to("cuda").set_mfma_dtype("bf16x6")
    stamp_path = _lib.LIB_PATH + ".stamp"
    stamp = open(stamp_path).read().strip()[:12] if os.path.exists(stamp_path) else "unstamped"
    dev = torch.device("cuda")
    t = ops.device_scalar(a.time, dev)
    rows, color_rows = [], []
    with torch.no_grad():
        sdf_packed = r.sdf_network.params_and_pack()
        pk = sdf_packed[2]
        net, keep = ops.sdf_net(r.sdf_network.layout(), pk)
        col_packed = r.color_network.params_and_pack(fold_feature=(sdf_packed[0][-1], sdf_packed[1][-1]))
        cnet, ckeep = ops.color_net(r.color_network.layout(), col_packed[2])
        for n in a.res:
            N, C = n ** 3, (n - 1) ** 3
            u = torch.empty(n, n, n, device=dev)
            grid = _stat(_events(lambda: ops.sdf_grid(net, (n, n, n), *BOX, t, out=u), a.repeats))
            d, ws, counts = ops.mesh_count(u, 0.0, *BOX)
            V, T = counts.tolist()
            lib = _lib.load()
            import ctypes
            count = _stat(_events(lambda: _lib.check(lib.cn_mesh_count(ctypes.byref(d), ops._ptr(ws), ws.numel(),
                                                                       ops._stream()), "cn_mesh_count"), a.repeats))
            vert = torch.empty(V, 3, device=dev)
            tri = torch.empty(T, 3, dtype=torch.int32, device=dev)
            emit = _stat(_events(lambda: ops.mesh_emit(d, ws, vert, tri, (V, T)), a.repeats))
            base = _stat(_host(lambda: baseline_fields(r.sdf_network, n, a.time), a.baseline_repeats))
            ub = baseline_fields(r.sdf_network, n, a.time)
            same = float((torch.from_numpy(ub) - u.cpu()).abs().max())
            # the colour pass (one cn_point_colors call) next to the chunked module composition with the same
            # packs, and the clean pass (host clock: it reads `changed` and the counts back)
            rgb = torch.empty(V, 3, device=dev)

            def composed(chunk=1 << 18):
                for i in range(0, V, chunk):
                    v = vert[i:i + chunk]
                    pts = torch.cat([v, t.expand(v.shape[0], 1)], dim=1)
                    _, feat, G = r.sdf_network.field(pts, want_feat="hidden", want_grad=True, packed=sdf_packed)
                    rgb[i:i + chunk] = r.color_network.color(pts, G, ops.vertex_dirs(G), 1, feat, packed=col_packed)
                return rgb

            color = _stat(_events(lambda: ops.point_colors(net, cnet, vert, t), a.repeats))
            color_py = _stat(_events(composed, a.repeats))
            color_same = bool(torch.equal(ops.point_colors(net, cnet, vert, t), composed()))
            cstats = {}
            clean = _stat(_host(lambda: ops.mesh_clean(vert, tri, keep_largest=True, stats=cstats), a.repeats))
            color_rows.append({
                "res": n, "vertices": V, "triangles": T, "point_colors": color, "composition": color_py,
                "composition_bitwise_equal": color_same, "point_colors_rows_per_s": V / (color["median_ms"] * 1e-3),
                "mesh_clean_keep_largest": clean, "components": cstats["components"], "label_rounds": cstats["rounds"],
            })
            count_bytes = 4 * N + N + C + 4 * N + 4 * C + 16
            emit_bytes = 4 * N + 12 * V + 12 * T
            rows.append({
                "res": n, "vertices": V, "triangles": T, "sdf_grid": grid, "mesh_count": count, "mesh_emit": emit,
                "baseline_fields": base, "baseline_max_abs_diff": same,
                "sdf_grid_rows_per_s": N / (grid["median_ms"] * 1e-3),
                "count_bytes": count_bytes, "count_GBps": count_bytes / (count["median_ms"] * 1e-3) / 1e9,
                "emit_bytes": emit_bytes, "emit_GBps": emit_bytes / (emit["median_ms"] * 1e-3) / 1e9,
                "speedup_fields": base["median_ms"] / grid["median_ms"],
            })
            del u, ws, vert, tri
        del keep, ckeep
    res = {"library": stamp, "device": torch.cuda.get_device_name(0), "mode": "bf16x6", "time_step": a.time,
           "repeats": a.repeats, "rows": rows}
    color_res = dict(res, rows=color_rows)
    f = lambda s: f'{s["median_ms"]:.2f} ({s["min_ms"]:.2f} .. {s["max_ms"]:.2f})'  # noqa: E731
    lines = [f"library {stamp}, {res['device']}, bf16x6, median (min .. max) ms of {a.repeats} calls "
             f"(baseline: {a.baseline_repeats})", "",
             "| res | V | T | cn_sdf_grid | Mrows/s | 64^3-block baseline | x | count | GB/s | emit | GB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for w in rows:
        lines.append(f'| {w["res"]}^3 | {w["vertices"]} | {w["triangles"]} | {f(w["sdf_grid"])} | '
                     f'{w["sdf_grid_rows_per_s"] / 1e6:.1f} | {f(w["baseline_fields"])} | {w["speedup_fields"]:.2f} | '
                     f'{f(w["mesh_count"])} | {w["count_GBps"]:.0f} | {f(w["mesh_emit"])} | {w["emit_GBps"]:.0f} |')
    lines += ["", "| res | V | T | cn_point_colors | Mrows/s | chunked composition | bitwise equal | "
              "mesh_clean keep_largest (host clock) | components | label rounds |", "|---|---|---|---|---|---|---|---|---|---|"]
    for w in color_rows:
        lines.append(f'| {w["res"]}^3 | {w["vertices"]} | {w["triangles"]} | {f(w["point_colors"])} | '
                     f'{w["point_colors_rows_per_s"] / 1e6:.1f} | {f(w["composition"])} | '
                     f'{w["composition_bitwise_equal"]} | {f(w["mesh_clean_keep_largest"])} | {w["components"]} | '
                     f'{w["label_rounds"]} |')
    table = "\n".join(lines)
    print(table)
    print(json.dumps(res))
    print(json.dumps(color_res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "mesh_bench.json"), "w") as fh:
            json.dump(res, fh, indent=1)
        with open(os.path.join(a.out, "mesh_color_bench.json"), "w") as fh:
            json.dump(color_res, fh, indent=1)
        with open(os.path.join(a.out, "mesh_bench.md"), "w") as fh:
            fh.write(table + "\n")
    return res


if __name__ == "__main__":
    main()
