"""Mesh files for NeuSRenderer.extract_geometry: a binary little-endian PLY writer (the reference writes its
meshes through trimesh, which this package does not depend on)."""
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
