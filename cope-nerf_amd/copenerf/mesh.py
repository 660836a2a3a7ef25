"""Mesh files for NeuSRenderer.extract_geometry: a binary little-endian PLY writer (the reference writes its
meshes through trimesh, which this package does not depend on) and the reader the geometry metrics load
meshes and ground-truth clouds with; and what turns a mesh back into per-view depth: camera_projection (the
project's camera convention as one 3 x 4 matrix), render_mesh_depth and cull_mesh (the view-based cull of the
ScanNet / DTU / Tanks-and-Temples protocols) over ops.mesh_raster / mesh_visibility / mesh_cull, render_mesh
(normal maps, vertex attributes and shaded pictures over ops.mesh_shade), and fuse_depths, the way back from
per-view depth to a mesh (fusion.TSDFVolume)."""
from __future__ import annotations

import numpy as np


def write_ply(path, vertices, triangles, normals=None, colors=None):
    """Write a triangle mesh as binary little-endian PLY: vertices float32 [V, 3] (x, y, z), optional unit
    normals float32 [V, 3] (nx, ny, nz), optional colours uint8 [V, 3] (uchar red, green, blue, after the
    normals) and triangles int32 [T, 3] as `list uchar int vertex_indices`."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype="<f4"))
    f = np.ascontiguousarray(np.asarray(triangles, dtype="<i4"))
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"write_ply: vertices [V, 3] and triangles [T, 3] (got {v.shape}, {f.shape})")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("write_ply: triangle index out of range")
    props = ["property float x", "property float y", "property float z"]
    cols = [v]
    if normals is not None:
        n = np.ascontiguousarray(np.asarray(normals, dtype="<f4"))
        if n.shape != v.shape:
            raise ValueError(f"write_ply: normals {n.shape} for vertices {v.shape}")
        props += ["property float nx", "property float ny", "property float nz"]
        cols.append(n)
    rows = np.ascontiguousarray(np.concatenate(cols, axis=1))
    if colors is not None:
        c = np.asarray(colors)
        if c.dtype != np.uint8 or c.shape != v.shape:
            raise ValueError(f"write_ply: colors must be uint8 {v.shape} (got {c.dtype} {c.shape})")
        props += ["property uchar red", "property uchar green", "property uchar blue"]
        rec = np.empty(len(v), dtype=[("f", "<f4", (rows.shape[1],)), ("c", "u1", (3,))])
        rec["f"] = rows
        rec["c"] = c
        rows = rec
    header = "\n".join(["ply", "format binary_little_endian 1.0", "comment copenerf extract_geometry",
                        f"element vertex {len(v)}", *props, f"element face {len(f)}",
                        "property list uchar int vertex_indices", "end_header"]) + "\n"
    faces = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    faces["n"] = 3
    faces["i"] = f
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(rows.tobytes())
        out.write(faces.tobytes())


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(f, path):
    """The elements of a PLY header, in file order: (format, [(name, count, [property, ...])]) with a property
    (name, type) or (name, count type, item type) for a list."""
    if f.readline().strip() != b"ply":
        raise ValueError(f"read_ply: {path} is not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"read_ply: {path}: the header does not end")
        w = line.decode("ascii", "replace").split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property":
            if not elements:
                raise ValueError(f"read_ply: {path}: a property before any element")
            try:
                prop = (w[4], _PLY_TYPES[w[2]], _PLY_TYPES[w[3]]) if w[1] == "list" else (w[2], _PLY_TYPES[w[1]])
            except (KeyError, IndexError):
                raise ValueError(f"read_ply: {path}: cannot read the property line {line!r}") from None
            elements[-1][2].append(prop)
        elif w[0] == "end_header":
            break
    if fmt == "binary_big_endian":
        raise ValueError(f"read_ply: {path} is big-endian; only ascii and binary_little_endian are read")
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"read_ply: {path}: format {fmt!r}")
    return fmt, elements


def _ply_faces(f, path, fmt, count, props, tokens):
    """The face element as int32 [count, 3]: the first list property holds the vertex indices; every face must
    be a triangle."""
    lists = [p for p in props if len(p) == 3]
    if not lists or props[0] is not lists[0] or len(lists) > 1:
        raise ValueError(f"read_ply: {path}: faces must start with their one index list")
    _, ctype, itype = lists[0]
    if ctype not in ("u1", "i1", "i4", "u4", "i2", "u2") or itype not in ("i4", "u4"):
        raise ValueError(f"read_ply: {path}: faces must be `list uchar|int int|uint`")
    tail = [(n, "<" + t) for n, t in props[1:]]
    if fmt == "ascii":
        width = 4 + len(tail)
        rows = np.array(tokens(count * width), dtype=np.float64).reshape(count, width) if count else np.zeros((0, width))
        if count and not np.all(rows[:, 0] == 3):
            raise ValueError(f"read_ply: {path} has a face that is not a triangle")
        return rows[:, 1:4].astype(np.int64).astype(np.int32)
    rec = np.dtype([("n", "<" + ctype), ("i", "<" + itype, (3,))] + tail)
    raw = f.read(rec.itemsize * count)
    # (a face with another count shifts the records: the counts stop reading 3, here or in a later record)
    faces = np.frombuffer(raw[:len(raw) // rec.itemsize * rec.itemsize], dtype=rec)
    if len(faces) != count or not np.all(faces["n"] == 3):
        raise ValueError(f"read_ply: {path} has a face that is not a triangle")
    return faces["i"].astype(np.int32)


def read_ply(path):
    """Read a PLY mesh or point cloud: (vertices float32 [V, 3], triangles int32 [T, 3] or None without a face
    element, normals float32 [V, 3] or None, colors uint8 [V, 3] or None).  ASCII and binary little-endian
    files; x y z (and nx ny nz) float or double; other vertex properties and other elements' scalar properties
    are skipped; faces are `list uchar|int int|uint` and all triangles.  A big-endian file or a face that is
    not a triangle raises a ValueError naming the file.  Reads back what write_ply writes."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f, path)
        words = iter(())
        if fmt == "ascii":
            words = iter(f.read().split())

        def tokens(n):
            out = [w for _, w in zip(range(n), words)]
            if len(out) != n:
                raise ValueError(f"read_ply: {path} ends early")
            return out

        vertices = triangles = normals = colors = None
        for name, count, props in elements:
            if name == "face":
                triangles = _ply_faces(f, path, fmt, count, props, tokens)
                continue
            if any(len(p) == 3 for p in props):
                raise ValueError(f"read_ply: {path}: a list property in element {name!r}")
            if fmt == "ascii":
                cols = np.array(tokens(count * len(props)), dtype=np.float64).reshape(count, len(props))
                table = {p[0]: cols[:, i] for i, p in enumerate(props)}
            else:
                rec = np.dtype([(p[0], "<" + p[1]) for p in props])
                raw = f.read(rec.itemsize * count)
                if len(raw) != rec.itemsize * count:
                    raise ValueError(f"read_ply: {path} ends early")
                table = np.frombuffer(raw, dtype=rec)
            if name != "vertex":
                continue
            have = {p[0] for p in props}
            if not {"x", "y", "z"} <= have:
                raise ValueError(f"read_ply: {path}: vertices without x y z")
            vertices = np.stack([np.asarray(table[k], dtype=np.float32) for k in "xyz"], 1)
            if {"nx", "ny", "nz"} <= have:
                normals = np.stack([np.asarray(table[k], dtype=np.float32) for k in ("nx", "ny", "nz")], 1)
            if {"red", "green", "blue"} <= have:
                colors = np.stack([np.asarray(table[k]).astype(np.uint8) for k in ("red", "green", "blue")], 1)
    if vertices is None:
        raise ValueError(f"read_ply: {path} has no vertex element")
    if triangles is not None and triangles.size and (triangles.min() < 0 or triangles.max() >= len(vertices)):
        raise ValueError(f"read_ply: {path}: triangle index out of range")
    return vertices, triangles, normals, colors


# ---------------------------------------------------------------------------
# depth rendering and view-based culling of a mesh (ops.mesh_raster / mesh_visibility / mesh_cull)
CULL_TOL_ABS, CULL_TOL_REL = 0.0, 0.01


def _mat4(m, name):
    if hasattr(m, "detach"):
        m = m.detach().cpu().numpy()
    m = np.asarray(m, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError(f"{name} must be 4 x 4, got {m.shape}")
    return m


def camera_projection(camera_mat, world_mat, scale_mat, resolution, transform=None):
    """The fp32 [3, 4] projection P of a view, composed in float64: the inverse of rays.world_rays over
    inference.arange_pixels' grid.  With (a, b, c) = P [X, 1] the point X is seen at pixel (a / c, b / c) of the
    (h, w) = resolution image render_image renders (pixel centres at integers, x along the width), and c is the
    depth d with X = o + d v for world_rays' un-normalised ray v through that pixel -- render_image's "depth";
    c > 0 in front of the camera.  scale_mat may be None (identity).  transform: an optional 4 x 4 similarity S
    applied to the geometry (as mesh_geometry_metrics' transform): P S^-1, so that the cameras of the model's
    frame look at geometry in the transformed frame, depths staying in the model's units.  The three matrices
    must be affine (last row 0 0 0 1), as world_rays assumes."""
    h, w = (int(x) for x in resolution)
    if h < 2 or w < 2:
        raise ValueError(f"camera_projection: resolution {resolution}")
    M = _mat4(camera_mat, "camera_mat") @ _mat4(world_mat, "world_mat")
    if scale_mat is not None:
        M = M @ _mat4(scale_mat, "scale_mat")
    if not np.allclose(M[3], (0.0, 0.0, 0.0, 1.0), rtol=0.0, atol=1e-9 * max(1.0, float(np.abs(M).max()))):
        raise ValueError("camera_projection: the camera, world and scale matrices must be affine (last row 0 0 0 1)")
    # M [X, 1] = (d xn, d yn, d, 1) with xn = 2 x / (w - 1) - 1, yn = 2 y / (h - 1) - 1
    P = np.stack([0.5 * (w - 1) * (M[0] + M[2]), 0.5 * (h - 1) * (M[1] + M[2]), M[2]])
    if transform is not None:
        P = P @ np.linalg.inv(_mat4(transform, "transform"))
    return P.astype(np.float32)


def view_projections(views, resolution, transform=None, device=None):
    """camera_projection of every view -- dicts with "camera_mat", "world_mat" and optionally "scale_mat", as
    metrics.evaluate takes them -- as one fp32 [N, 3, 4] tensor on `device`."""
    import torch
    P = np.stack([camera_projection(v["camera_mat"], v["world_mat"], v.get("scale_mat"), resolution, transform)
                  for v in views]) if len(views) else np.zeros((0, 3, 4), np.float32)
    return torch.from_numpy(P).to(device)


def render_mesh_depth(vertices, triangles, views, resolution, transform=None, near=None, stats=None):
    """The depth of a mesh from every view, on the device: {"depth": fp32 [N, h, w] (+inf where the view sees no
    triangle), "tri": int32 [N, h, w] (the triangle seen, -1 where none)} for vertices fp32 [V, 3] / triangles
    int32 [T, 3] device tensors -- ops.mesh_raster under view_projections(views, resolution, transform).  The depth
    is in render_image's convention, so metrics.depth_metrics scores it against sensor depth as it scores a
    rendered one."""
    from . import ops
    h, w = (int(x) for x in resolution)
    proj = view_projections(views, (h, w), transform, vertices.device)
    depth, tri = ops.mesh_raster(vertices, triangles, proj, h, w, near=ops.MESH_NEAR if near is None else near, stats=stats)
    return {"depth": depth, "tri": tri}


def cull_mesh(vertices, triangles, views, resolution, min_views=1, tol_abs=CULL_TOL_ABS, tol_rel=CULL_TOL_REL,
              transform=None, near=None):
    """The mesh cut down to what the cameras saw, as the ScanNet / DTU / Tanks-and-Temples protocols do before
    they measure it: the mesh's depth is rendered from every view (render_mesh_depth), a vertex is kept when at
    least min_views views see it -- inside the image, in front of the camera, and at a depth c <= depth[pixel]
    (1 + tol_rel) + tol_abs of the pixel nearest to it -- and a triangle when its three corners are.  Returns
    (vertices' [V', 3], triangles' int32 [T', 3] renumbered, kept_vertices int32 [V'], the original ids ascending),
    as ops.mesh_clean does; the order of what is kept is unchanged.  The tolerance covers the depth a slanted
    surface gains over half a pixel; the defaults are 1 % relative, nothing absolute."""
    from . import ops
    h, w = (int(x) for x in resolution)
    near = ops.MESH_NEAR if near is None else near
    proj = view_projections(views, (h, w), transform, vertices.device)
    depth, _ = ops.mesh_raster(vertices, triangles, proj, h, w, near=near)
    count = ops.mesh_visibility(vertices, proj, h, w, depth=depth, tol_abs=tol_abs, tol_rel=tol_rel, near=near)
    return ops.mesh_cull(vertices, triangles, count >= int(min_views))


def _similarity(transform, device):
    """(M fp32 [4, 4] on the device, R float64 [3, 3]: the rotation of the similarity M) or (None, None)."""
    import torch
    if transform is None:
        return None, None
    M = _mat4(transform, "transform")
    A = M[:3, :3]
    s = abs(np.linalg.det(A)) ** (1.0 / 3.0)
    if not s > 0.0:
        raise ValueError("transform must be invertible")
    return torch.as_tensor(M, dtype=torch.float32).to(device), A / s


def render_mesh(vertices, triangles, views, resolution, *, normals=None, colors=None, attrs=None, frame="camera",
                light=(0, 0, 1), ambient=0.3, background=(255, 255, 255), transform=None, near=None):
    """A mesh seen from every view, on the device (ops.mesh_raster, then ops.mesh_shade on its triangle image):
      "depth", "tri"   as render_mesh_depth returns them;
      "normal"         fp32 [N, h, w, 3], the unit surface normal turned towards the camera, zero where nothing is
                       seen: the triangles' own normals, or with normals fp32 [V, 3] the interpolated vertex normals;
      "normal_image"   uint8 [N, h, w, 3], normal * 128 + 128: what visualize writes as _normal.png;
      "shaded"         uint8 [N, h, w, 3], albedo (ambient + (1 - ambient) max(0, normal . light)), the albedo from
                       colors (uint8, or float in [0, 1], [V, 3]) or a constant grey; `background` elsewhere;
      "attr"           fp32 [N, h, w, C] with attrs fp32 [V, C] (1 <= C <= 16): perspective-correct interpolation.
    frame="camera" gives the normals in each view's camera frame (world_mat[:3, :3] n, the frame of
    inference.render_image's "normal"), "world" leaves them in the mesh's.  light is normalised here and lives in
    the normals' frame: (0, 0, 1) in the camera frame is a headlight.  transform: a 4 x 4 similarity applied to the
    vertices, and its rotation to normals, before anything else (as metrics.mesh_geometry_metrics does), the cameras
    following it; camera-frame normals are unchanged by it."""
    import torch
    from . import ops
    if frame not in ("camera", "world"):
        raise ValueError(f"render_mesh: frame {frame!r} (camera or world)")
    h, w = (int(x) for x in resolution)
    dev = vertices.device
    M, R = _similarity(transform, dev)
    if M is not None:
        vertices = (vertices @ M[:3, :3].T + M[:3, 3]).contiguous()
        if normals is not None:
            normals = (normals @ torch.as_tensor(R, dtype=torch.float32).to(dev).T).contiguous()
    proj = view_projections(views, (h, w), transform, dev)
    depth, tri = ops.mesh_raster(vertices, triangles, proj, h, w, near=ops.MESH_NEAR if near is None else near)
    rot = None
    if frame == "camera":
        rots = [_mat4(v["world_mat"], "world_mat")[:3, :3] @ (R.T if R is not None else np.eye(3)) for v in views]
        rot = torch.as_tensor(np.stack(rots) if rots else np.zeros((0, 3, 3)), dtype=torch.float32).to(dev).contiguous()
    L = np.asarray(light, dtype=np.float64)
    if L.shape != (3,) or not np.linalg.norm(L) > 0.0:
        raise ValueError(f"render_mesh: light {light}")
    L = L / np.linalg.norm(L)
    albedo = None
    if colors is not None:
        albedo = colors.to(dev)
        albedo = albedo.float() / 255.0 if albedo.dtype == torch.uint8 else albedo.float()
        if albedo.dim() != 2 or tuple(albedo.shape) != (vertices.shape[0], 3):
            raise ValueError(f"render_mesh: colors {tuple(colors.shape)} for {vertices.shape[0]} vertices")
        albedo = albedo.contiguous()
    out = ops.mesh_shade(vertices, triangles, proj, tri, attr=albedo, vnormals=normals, rot=rot,
                         want=("normal", "normal_image", "shaded"), light=L, ambient=ambient,
                         albedo_from_attr=albedo is not None, background=background)
    if attrs is not None:
        out["attr"] = ops.mesh_shade(vertices, triangles, proj, tri, attr=attrs, want=("attr",))["attr"]
    out["depth"], out["tri"] = depth, tri
    return out


# ---------------------------------------------------------------------------
# depth maps back into a mesh (fusion.TSDFVolume)
def fuse_depths(depths, views, bound_min, bound_max, dims, trunc=None, *, colors=None, resolution=None, depth_max=None,
                near=None, transform=None, min_weight=1, keep_largest=False, min_triangles=0, device="cuda",
                views_per_call=None, stats=None):
    """Depth maps to a mesh in one call, on the device: fusion.TSDFVolume(...).integrate(...).extract_mesh(...) --
    depths [N, h, w] (render_image's depth, or a sensor's, 0 / +inf / NaN where nothing is seen) from `views` (the
    dicts view_projections takes) fused into a dims grid over bound_min .. bound_max and meshed where at least
    min_weight views observed it.  trunc defaults to four voxels (of the coarsest axis).  Returns numpy (vertices,
    triangles) and, with colors [N, h, w, 3], the vertex colours uint8 [V, 3]."""
    dims = (dims,) * 3 if np.isscalar(dims) else tuple(int(n) for n in dims)
    if trunc is None:
        lo, hi = np.asarray(bound_min, dtype=np.float64), np.asarray(bound_max, dtype=np.float64)
        trunc = 4.0 * float(np.max((hi - lo) / (np.asarray(dims) - 1)))
    from .fusion import TSDFVolume, VIEWS_PER_CALL
    vol = TSDFVolume(bound_min, bound_max, dims, trunc, device, with_colors=colors is not None)
    vol.integrate(depths, views, resolution=resolution, colors=colors, depth_max=depth_max, near=near,
                  transform=transform, views_per_call=views_per_call or VIEWS_PER_CALL)
    return vol.extract_mesh(min_weight=min_weight, keep_largest=keep_largest, min_triangles=min_triangles,
                            with_colors=colors is not None, stats=stats)
