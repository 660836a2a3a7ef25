"""Extract the surface a trained model holds at one time value and write it as a PLY file.

    python tools/extract_mesh.py CHECKPOINT OUT.ply [--bound-min X Y Z] [--bound-max X Y Z]
        [--resolution N] [--threshold S] [--time T] [--mode fp32|bf16x6|bf16] [--normals]
        [--colors [--view-dir X Y Z]] [--keep-largest] [--min-triangles N]

The checkpoint is one train.py wrote through CheckpointIO (a DataParallel NeuSRenderer under "model", reference
or this build); the network widths are read from its shapes.  NeuSRenderer.extract_geometry does the work:
the SDF volume, the marching-tetrahedra mesher, floater removal (--keep-largest, --min-triangles) and the vertex
colours (--colors) run on the device."""
import argparse
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT]


def build_renderer(checkpoint):
    """A DataParallel NeuSRenderer with the widths of the checkpoint's networks, loaded strictly from it."""
    from copenerf import CheckpointIO, MotionNetwork, NeuSRenderer, RenderingNetwork, SDFNetwork, SingleVarianceNetwork
    from copenerf.train_step import COL_CFG, MOTION_CFG, REN_CFG, SDF_CFG
    sd = torch.load(checkpoint, map_location="cpu", weights_only=True)["model"]
    width = lambda net: sd[f"module.{net}.lin0.weight_v"].shape[0]  # noqa: E731
    sdf = SDFNetwork(**dict(SDF_CFG, d_hidden=width("sdf_network")))
    col = RenderingNetwork(**dict(COL_CFG, d_hidden=width("color_network"), d_feature=width("sdf_network")))
    motion = None
    if any(k.startswith("module.motion_network.") for k in sd):
        motion = MotionNetwork(**dict(MOTION_CFG, d_hidden=width("motion_network")))
    dp = torch.nn.DataParallel(NeuSRenderer(None, sdf, SingleVarianceNetwork(0.3), col, motion, **REN_CFG))
    with tempfile.TemporaryDirectory() as d:
        CheckpointIO(d, model=dp).load_file(checkpoint, load_model_only=True)
    return dp.module


def main(argv=None):
    from copenerf import write_ply
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint")
    ap.add_argument("out")
    ap.add_argument("--bound-min", type=float, nargs=3, default=[-1.0, -1.0, -1.0])
    ap.add_argument("--bound-max", type=float, nargs=3, default=[1.0, 1.0, 1.0])
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--time", type=float, default=0.0, help="the time value t of the (x, y, z, t) SDF")
    ap.add_argument("--mode", choices=["fp32", "bf16x6", "bf16"], default="bf16x6", help="the MLP GEMMs' MFMA mode")
    ap.add_argument("--normals", action="store_true", help="also write unit normals (the SDF's gradient)")
    ap.add_argument("--colors", action="store_true",
                    help="also write 8-bit vertex colours (the colour network seen along the inward normal)")
    ap.add_argument("--view-dir", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="with --colors: one fixed view direction for every vertex instead of the inward normal")
    ap.add_argument("--keep-largest", action="store_true",
                    help="keep only the connected component with the most triangles")
    ap.add_argument("--min-triangles", type=int, default=0, metavar="N",
                    help="drop every connected component with fewer than N triangles")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("extract_mesh: needs a HIP device (the kernels have no CPU fallback)")
    r = build_renderer(a.checkpoint).to("cuda").set_mfma_dtype(a.mode)
    stats = {}
    res = r.extract_geometry(torch.tensor(a.bound_min), torch.tensor(a.bound_max), a.resolution, a.threshold,
                             time_step=a.time, with_normals=a.normals, with_colors=a.colors, view_dir=a.view_dir,
                             keep_largest=a.keep_largest, min_triangles=a.min_triangles, stats=stats)
    write_ply(a.out, res[0], res[1], normals=res[2] if a.normals else None, colors=res[-1] if a.colors else None)
    line = f"{a.out}: {len(res[0])} vertices, {len(res[1])} triangles"
    if stats:
        line += f", {stats['components']} components found, {stats['components_kept']} kept"
    print(line)
    return res


if __name__ == "__main__":
    main()
