"""Host reference of the isosurface mesher, in numpy, from its specification (include/copenerf.h, ABI v16;
DESIGN.md "Mesh extraction") and independent of the HIP code: marching tetrahedra on the six-tetrahedron
Kuhn split.  Vertex positions are computed in float64 from the fp32 volume; a triangle's orientation is taken
from the midpoint rule, evaluated directly for every triangle (no case table).

Also the mesh properties the tests assert: closedness and consistent orientation, the Euler characteristic,
the signed volume."""
from __future__ import annotations

import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))  # lexicographic


def tet_corners(k):
    """The four corners of tetrahedron k as (x, y, z) offsets in {0, 1}^3."""
    pi = PERMS[k]
    v = [np.zeros(3, dtype=np.int64)]
    for a in pi[:2]:
        w = v[-1].copy()
        w[a] += 1
        v.append(w)
    v.append(np.ones(3, dtype=np.int64))
    return np.stack(v)


def _triangles_of(k, mask):
    """The triangles of (tetrahedron k, mask) as lists of three edges (i, j) of tetrahedron-local corners,
    i the corner in A, oriented by the midpoint rule."""
    inside = [i for i in range(4) if mask >> i & 1]
    outside = [i for i in range(4) if not mask >> i & 1]
    if not inside or not outside:
        return []
    A, B = (inside, outside) if len(inside) <= 2 else (outside, inside)
    if len(A) == 1:
        i, (j, kk, l) = A[0], B
        tris = [[(i, j), (i, kk), (i, l)]]
    else:
        (i, j), (kk, l) = A, B
        tris = [[(i, kk), (i, l), (j, l)], [(i, kk), (j, l), (j, kk)]]
    P = tet_corners(k).astype(np.float64)
    direction = P[outside].mean(axis=0) - P[inside].mean(axis=0)
    out = []
    for tri in tris:
        m = np.stack([(P[a] + P[b]) / 2 for a, b in tri])
        dot = float(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), direction))
        assert abs(dot) > 1e-9, (k, mask)  # the rule decides every case
        out.append(tri if dot > 0 else [tri[0], tri[2], tri[1]])
    return out


def isosurface(u, threshold, lo, hi):
    """(vertices float64 [V, 3], triangles int64 [T, 3]) of the fp32 volume u [nx, ny, nz]."""
    u = np.asarray(u)
    assert u.dtype == np.float32 and u.ndim == 3
    thr = np.float32(threshold)
    nx, ny, nz = u.shape
    dims = np.array([nx, ny, nz])
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)  # the ABI's bounds are fp32
    hi = np.asarray(hi, dtype=np.float32).astype(np.float64)
    inside = u < thr  # strict: a tie is outside
    lin = np.arange(nx * ny * nz).reshape(nx, ny, nz)

    # vertices: one per in-bounds edge (p, slot) whose ends differ, ascending by (linear index of p, slot)
    key_parts, pos_parts = [], []
    for slot in range(7):
        d = np.array([(slot + 1) & 1, (slot + 1) >> 1 & 1, (slot + 1) >> 2 & 1])
        sl_p = tuple(slice(0, n - dd) for n, dd in zip(dims, d))
        sl_q = tuple(slice(dd, n) for n, dd in zip(dims, d))
        cross = inside[sl_p] != inside[sl_q]
        p_lin = lin[sl_p][cross]
        up = u[sl_p][cross].astype(np.float64)
        uq = u[sl_q][cross].astype(np.float64)
        s = (float(thr) - up) / (uq - up)
        p = np.stack(np.unravel_index(p_lin, (nx, ny, nz)), axis=1).astype(np.float64)
        key_parts.append(p_lin * 7 + slot)
        pos_parts.append(p + s[:, None] * d[None, :])
    keys = np.concatenate(key_parts)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    pos = np.concatenate(pos_parts)[order]
    vertices = lo + pos / (dims - 1.0) * (hi - lo)

    # triangles, ascending by (cell, k, triangle)
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    cell_lin = np.arange(cx * cy * cz).reshape(cx, cy, cz)
    rows, sort_keys = [], []
    for k in range(6):
        C = tet_corners(k)
        corner_in = [inside[c[0]:c[0] + cx, c[1]:c[1] + cy, c[2]:c[2] + cz] for c in C]
        corner_lin = [lin[c[0]:c[0] + cx, c[1]:c[1] + cy, c[2]:c[2] + cz] for c in C]
        mask = sum(ci.astype(np.int64) << i for i, ci in enumerate(corner_in))
        for m in range(1, 15):
            sel = mask == m
            if not sel.any():
                continue
            cells = cell_lin[sel]
            for ti, tri in enumerate(_triangles_of(k, m)):
                idx = []
                for a, b in tri:
                    a, b = min(a, b), max(a, b)  # the edge runs from the component-wise lower corner
                    d = C[b] - C[a]
                    slot = d[0] + 2 * d[1] + 4 * d[2] - 1
                    key = corner_lin[a][sel] * 7 + slot
                    j = np.searchsorted(keys, key)
                    assert (keys[j] == key).all()
                    idx.append(j)
                rows.append(np.stack(idx, axis=1))
                sort_keys.append((cells * 6 + k) * 2 + ti)
    if rows:
        tri_all = np.concatenate(rows)
        o = np.argsort(np.concatenate(sort_keys), kind="stable")
        triangles = tri_all[o]
    else:
        triangles = np.zeros((0, 3), dtype=np.int64)
    return vertices.reshape(-1, 3), triangles


# -- mesh properties ---------------------------------------------------------------------------------
def directed_edges(tri):
    t = np.asarray(tri, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_oriented(tri, n_vertices):
    """Every directed edge occurs once and has exactly one opposite."""
    e = directed_edges(tri)
    code = e[:, 0] * n_vertices + e[:, 1]
    rev = e[:, 1] * n_vertices + e[:, 0]
    uniq, cnt = np.unique(code, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(uniq, np.unique(rev)))


def euler_characteristic(tri, n_vertices):
    e = directed_edges(tri)
    und = np.unique(np.minimum(e[:, 0], e[:, 1]) * n_vertices + np.maximum(e[:, 0], e[:, 1]))
    return int(n_vertices - len(und) + len(tri))


def signed_volume(vertices, tri):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# -- analytic volumes (fp32, C order) of the tests ---------------------------------------------------------
def grid(dims, lo, hi):
    ax = [np.linspace(l, h, n) for l, h, n in zip(lo, hi, dims)]
    return np.meshgrid(*ax, indexing="ij")


def sphere_tie(n=33):
    """Sphere of radius 0.5 in the box +-1: the six grid points (+-0.5, 0, 0), ... tie the threshold exactly."""
    x, y, z = grid((n,) * 3, (-1,) * 3, (1,) * 3)
    return (np.sqrt(x * x + y * y + z * z) - 0.5).astype(np.float32)


def sphere_soft(n=33):
    x, y, z = grid((n,) * 3, (-1,) * 3, (1,) * 3)
    return (np.sqrt(x * x + y * y + z * z + 0.09) - 0.5).astype(np.float32)


def two_spheres(n=17):
    x, y, z = grid((n,) * 3, (-1,) * 3, (1,) * 3)
    a = np.sqrt((x - 0.45) ** 2 + (y - 0.45) ** 2 + (z - 0.45) ** 2) - 0.30
    b = np.sqrt((x + 0.45) ** 2 + (y + 0.45) ** 2 + (z + 0.45) ** 2) - 0.25
    return np.minimum(a, b).astype(np.float32)


def torus(n=17):
    x, y, z = grid((n,) * 3, (-1,) * 3, (1,) * 3)
    return (np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z) - 0.22).astype(np.float32)


def sphere_cut(n=17):
    x, y, z = grid((n,) * 3, (-1,) * 3, (1,) * 3)
    return (np.sqrt(x * x + y * y + z * z) - 1.2).astype(np.float32)
