"""TSDF fusion on the device: per-view depth maps (rendered from the model, or a sensor's) fused into a truncated
signed distance volume and meshed where the cameras observed it -- the other way NeuS-family and ScanNet-style
evaluations get a mesh.  TSDFVolume keeps the running sums on the device (ops.tsdf_integrate), finalises them into
a volume whose NaN mean "unobserved" (ops.tsdf_finalize), meshes that volume with the observed-only variant of the
marching-tetrahedra mesher (ops.isosurface(observed=True)), removes what no triangle refers to (ops.mesh_clean) and
colours the vertices from the fused colour volume (ops.volume_sample + ops.rgb8_pack).  There is no CPU path: a
missing library or CPU tensors raise."""
from __future__ import annotations

import math

import numpy as np

# Views per cn_tsdf_integrate call.  The volumes are read and written once per call, which argues for long calls; but
# measured (tools/tsdf_bench.py) the per-view cost of a call rises with its length -- 0.08 ms a view
# at 8 views, 0.21 ms at 64, on a 256^3 volume -- and 8 is the fastest of 8 / 16 / 32 / 64 at 256^3 and at 512^3.
VIEWS_PER_CALL = 8


def _as_device(a, name, device, ndim):
    import torch
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32)))
    if t.dim() != ndim:
        raise ValueError(f"TSDFVolume.integrate: {name} must have {ndim} dims (got shape {tuple(t.shape)})")
    return t.to(device=device, dtype=torch.float32).contiguous()


class TSDFVolume:
    """A dims = (nx, ny, nz) grid of voxels over the box bound_min .. bound_max (voxel i of an axis at
    lo + i / (n - 1) (hi - lo): the mesher's vertex map), truncation distance trunc in depth units."""

    def __init__(self, bound_min, bound_max, dims, trunc, device, with_colors=False):
        import torch
        self.lo = [float(v) for v in np.asarray(bound_min, dtype=np.float64).reshape(-1)]
        self.hi = [float(v) for v in np.asarray(bound_max, dtype=np.float64).reshape(-1)]
        if len(self.lo) != 3 or len(self.hi) != 3 or not all(h > l for l, h in zip(self.lo, self.hi)):
            raise ValueError(f"TSDFVolume: bounds {self.lo} .. {self.hi} (three entries each, max above min)")
        dims = (dims,) * 3 if np.isscalar(dims) else tuple(dims)
        self.dims = tuple(int(n) for n in dims)
        if len(self.dims) != 3 or min(self.dims) < 2:
            raise ValueError(f"TSDFVolume: dims {dims} (three entries, each at least 2)")
        if math.prod(self.dims) >= 2 ** 31:
            raise ValueError(f"TSDFVolume: dims {self.dims} too large (nx ny nz below 2^31)")
        self.trunc = float(trunc)
        if not (self.trunc > 0.0 and math.isfinite(self.trunc)):
            raise ValueError(f"TSDFVolume: trunc {trunc} (positive and finite)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"TSDFVolume: device {self.device}; the fusion kernels have no CPU fallback")
        from . import _lib
        _lib.load()  # a missing library raises here, not at the first integrate
        self.tsum = torch.zeros(self.dims, device=self.device)
        self.wsum = torch.zeros(self.dims, device=self.device)
        self.csum = torch.zeros(self.dims + (3,), device=self.device) if with_colors else None
        self.n_views = 0

    def integrate(self, depths, views, resolution=None, colors=None, depth_max=None, near=None, transform=None,
                  views_per_call=VIEWS_PER_CALL):
        """Fuse depths [N, h, w] (a device tensor or numpy; 0, +inf or NaN where nothing is seen) seen from
        `views` -- the dicts mesh.view_projections takes ("camera_mat", "world_mat", optionally "scale_mat") -- in
        render_image's depth convention (mesh.camera_projection's c).  resolution: (h, w) of the images the cameras
        describe, by default the depth maps' own.  colors: [N, h, w, 3] in [0, 1] (uint8 is divided by 255), needed
        exactly when the volume was made with_colors.  depth_max: depths beyond it are no observation.  transform: a
        4 x 4 similarity of the volume's frame against the cameras' (mesh.camera_projection)."""
        import torch
        from . import mesh, ops
        depths = _as_device(depths, "depths", self.device, 3)
        N, h, w = depths.shape
        if len(views) != N:
            raise ValueError(f"TSDFVolume.integrate: {N} depth maps for {len(views)} views")
        if resolution is not None and tuple(int(x) for x in resolution) != (h, w):
            raise ValueError(f"TSDFVolume.integrate: depth maps of {h} x {w} for resolution {tuple(resolution)}")
        if (colors is None) != (self.csum is None):
            raise ValueError("TSDFVolume.integrate: colors are needed exactly when the volume was made with_colors")
        if colors is not None:
            if isinstance(colors, torch.Tensor) and colors.dtype == torch.uint8 or \
                    not isinstance(colors, torch.Tensor) and np.asarray(colors).dtype == np.uint8:
                colors = torch.as_tensor(colors).to(self.device).float() / 255.0
            colors = _as_device(colors, "colors", self.device, 4)
            if tuple(colors.shape) != (N, h, w, 3):
                raise ValueError(f"TSDFVolume.integrate: colors {tuple(colors.shape)} for depths {tuple(depths.shape)}")
        step = max(int(views_per_call), 1)
        proj = mesh.view_projections(views, (h, w), transform, self.device)
        for v0 in range(0, N, step):
            sl = slice(v0, v0 + step)
            ops.tsdf_integrate(self.tsum, self.wsum, self.lo, self.hi, proj[sl].contiguous(), depths[sl], self.trunc,
                               csum=self.csum, color=None if colors is None else colors[sl],
                               near=ops.MESH_NEAR if near is None else near,
                               depth_max=math.inf if depth_max is None else depth_max)
        self.n_views += N
        return self

    def volume(self, min_weight=1):
        """u [nx, ny, nz]: the mean truncated distance over trunc where at least min_weight views observed the
        voxel, NaN elsewhere; with colours (u, rgb [nx, ny, nz, 3])."""
        from . import ops
        return ops.tsdf_finalize(self.tsum, self.wsum, self.csum, min_weight)

    def extract_mesh(self, min_weight=1, keep_largest=False, min_triangles=0, with_colors=False, stats=None):
        """The surface u = 0 of what the cameras observed: numpy (vertices float32 [V, 3], triangles int32 [T, 3])
        and, with_colors, colours uint8 [V, 3].  The observed-only isosurface, then ops.mesh_clean with
        min_triangles at least 1, so no vertex without a triangle survives; normals point towards the cameras."""
        from . import ops
        if with_colors and self.csum is None:
            raise ValueError("TSDFVolume.extract_mesh: with_colors needs a volume made with_colors")
        vol = self.volume(min_weight)
        u, rgb = vol if self.csum is not None else (vol, None)
        v, t = ops.isosurface(u, 0.0, self.lo, self.hi, observed=True)
        if stats is not None:
            stats["vertices_emitted"], stats["triangles_emitted"] = v.shape[0], t.shape[0]
        v, t, _ = ops.mesh_clean(v, t, keep_largest=keep_largest, min_triangles=max(int(min_triangles), 1), stats=stats)
        out = (v.cpu().numpy(), t.cpu().numpy())
        if with_colors:
            c = ops.volume_sample(rgb, v.contiguous(), self.lo, self.hi, mask=u)
            out += (ops.rgb8_pack(c).cpu().numpy(),)
        return out
