"""Look at a mesh: its depth, its normal map and a shaded picture from every camera, on the device
(mesh.render_mesh: ops.mesh_raster, then ops.mesh_shade).

    python tools/render_mesh.py MESH.ply --K K.npy --world-mats W2C.npy [--scale-mat S.npy] --resolution H W --out DIR
        [--frame camera|world] [--smooth] [--colors] [--transform T.npy]

  MESH.ply      a triangle mesh (tools/extract_mesh.py's output as it is)
  --K           camera matrices [N, 4, 4] or one [4, 4] for every view
  --world-mats  world-to-camera matrices [N, 4, 4], in the mesh's own frame
  --scale-mat   scale matrices [N, 4, 4] or one [4, 4] (default: identity)
  --frame       the frame of the normals: each view's camera frame (default; the frame of tools/render_views.py's
                _normal.png, so the two pictures are the same when the geometry agrees) or the mesh's
  --smooth      interpolate the PLY's vertex normals instead of showing the triangles' own
  --colors      shade with the PLY's vertex colours instead of a constant grey
  --transform   a 4 x 4 similarity applied to the mesh first, the cameras following it

Writes, per view i, DIR/depth_%06d.npz (key `pred`, 0 where nothing is seen: tools/evaluate_mesh.py --depths-out's
format), DIR/%06d_normal.png and DIR/%06d_shaded.png."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "cope-nerf_amd"), ROOT, os.path.join(ROOT, "tools")]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mesh")
    ap.add_argument("--K", required=True)
    ap.add_argument("--world-mats", required=True)
    ap.add_argument("--scale-mat")
    ap.add_argument("--resolution", type=int, nargs=2, required=True, metavar=("H", "W"))
    ap.add_argument("--out", required=True)
    ap.add_argument("--frame", choices=["camera", "world"], default="camera")
    ap.add_argument("--smooth", action="store_true")
    ap.add_argument("--colors", action="store_true")
    ap.add_argument("--transform")
    return ap.parse_args(argv)


def load_mesh(path, smooth=False, colors=False):
    """(vertices, triangles, normals or None, colors or None) of a PLY mesh; normals / colours are returned only when
    asked for, and asking for what the file does not hold ends with a message."""
    from copenerf.mesh import read_ply
    vertices, triangles, normals, cols = read_ply(path)
    if triangles is None:
        raise SystemExit(f"render_mesh: {path} has no faces")
    if smooth and normals is None:
        raise SystemExit(f"render_mesh: --smooth needs vertex normals (nx ny nz), {path} has none")
    if colors and cols is None:
        raise SystemExit(f"render_mesh: --colors needs vertex colours (red green blue), {path} has none")
    return vertices, triangles, normals if smooth else None, cols if colors else None


def main(argv=None):
    a = parse_args(argv)
    vertices, triangles, normals, colors = load_mesh(a.mesh, a.smooth, a.colors)
    if not torch.cuda.is_available():
        raise SystemExit("render_mesh: needs a HIP device (the kernels have no CPU fallback)")
    from PIL import Image
    from copenerf import mesh
    from evaluate_mesh import load_views
    views = load_views([a.K, a.world_mats] + ([a.scale_mat] if a.scale_mat else []))
    dev = torch.device("cuda")
    on = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    out = mesh.render_mesh(on(vertices), on(triangles), views, tuple(a.resolution), normals=on(normals), colors=on(colors),
                           frame=a.frame, transform=None if a.transform is None else np.load(a.transform))
    os.makedirs(a.out, exist_ok=True)
    depth = torch.where(torch.isinf(out["depth"]), torch.zeros_like(out["depth"]), out["depth"]).cpu().numpy()
    normal, shaded = out["normal_image"].cpu().numpy(), out["shaded"].cpu().numpy()
    for i in range(len(views)):
        np.savez(os.path.join(a.out, "depth_%06d.npz" % i), pred=depth[i])
        Image.fromarray(normal[i]).save(os.path.join(a.out, "%06d_normal.png" % i))
        Image.fromarray(shaded[i]).save(os.path.join(a.out, "%06d_shaded.png" % i))
    print(f"wrote {3 * len(views)} files under {a.out}")
    return out


if __name__ == "__main__":
    main()
