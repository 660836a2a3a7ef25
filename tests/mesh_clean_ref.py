"""Host reference of floater removal (include/copenerf.h, "Connected components of a welded indexed triangle
list"), in numpy, from the specification and independent of the HIP code: a union-find over the triangles'
edges (roots hooked smaller-id-first, paths compressed fully), so every vertex's label is the smallest vertex id of
its connected component; the triangles per component; the kept set; the compacted mesh.

Also the hand-built triangle lists of the tests."""
from __future__ import annotations

import numpy as np


def _find(parent, x):
    """Roots of x with parent[] compressed fully on the way."""
    while True:
        grand = parent[parent]
        if np.array_equal(grand, parent):
            return parent[x]
        parent[:] = grand


def labels(triangles, n_vertices):
    """label int32 [V]: the smallest vertex id of the vertex's component.  Union-find over the edges (c0, c1),
    (c1, c2) of every triangle, all edges at once: the larger root is hooked under the smaller (several hooks of
    one root: the smallest wins, the others are retried), until no edge joins two trees.  A tree's root is its
    smallest id, since a parent is always smaller than its children."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    parent = np.arange(n_vertices, dtype=np.int64)
    a = np.concatenate([t[:, 0], t[:, 1]])
    b = np.concatenate([t[:, 1], t[:, 2]])
    while len(a):
        ra, rb = _find(parent, a), _find(parent, b)
        differ = ra != rb
        if not differ.any():
            break
        a, b, ra, rb = a[differ], b[differ], ra[differ], rb[differ]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
    return _find(parent, np.arange(n_vertices, dtype=np.int64)).astype(np.int32)


def component_sizes(triangles, label):
    """tri_count int32 [V]: triangles per component at its root id (the label of a triangle's first corner)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return np.bincount(label[t[:, 0]], minlength=len(label)).astype(np.int32)


def kept_roots(tri_count, keep_largest=False, min_triangles=0):
    """bool [V]: the roots of the kept components.  Kept: at least min_triangles triangles and, with keep_largest,
    the component with the most triangles (np.argmax takes the first maximum: a tie goes to the smaller root id;
    none when there is no triangle)."""
    keep = tri_count >= min_triangles
    if keep_largest:
        only = np.zeros_like(keep)
        if len(tri_count) and tri_count.max() > 0:
            only[int(np.argmax(tri_count))] = True
        keep &= only
    return keep


def clean(triangles, n_vertices, keep_largest=False, min_triangles=0):
    """(kept_vertices int32 [V'] ascending original ids, triangles' int32 [T', 3] renumbered in their original
    order, label, tri_count)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    lab = labels(t, n_vertices)
    cnt = component_sizes(t, lab)
    keep = kept_roots(cnt, keep_largest, min_triangles)
    vkeep = keep[lab] if n_vertices else np.zeros(0, dtype=bool)
    tkeep = vkeep[t[:, 0]]
    kept = np.flatnonzero(vkeep).astype(np.int32)
    new_id = np.cumsum(vkeep) - 1
    return kept, new_id[t[tkeep]].astype(np.int32).reshape(-1, 3), lab, cnt


def same_partition(a, b):
    """Two labelings split the vertices into the same sets."""
    a, b = np.asarray(a), np.asarray(b)
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


# -- hand-built triangle lists -------------------------------------------------------------------------
def strip(n_vertices, seed=None):
    """triangles[i] = (i, i + 1, i + 2) over n_vertices vertices: one component whose diameter is about
    n_vertices / 2 edges.  seed: the ids permuted by np.random.default_rng(seed), vertex 0 kept in place so the
    smallest id sits at one end and every other label has to travel against the order of the ids."""
    i = np.arange(n_vertices - 2, dtype=np.int64)
    t = np.stack([i, i + 1, i + 2], axis=1)
    if seed is not None:
        perm = np.concatenate([[0], 1 + np.random.default_rng(seed).permutation(n_vertices - 1)])
        t = perm[t]
    return t.astype(np.int32)


def fans(sizes=(5, 5, 3)):
    """Disjoint triangle fans: fan k has a hub and sizes[k] + 1 rim vertices, triangles (hub, rim j, rim j + 1).
    Returns (triangles int32 [sum sizes, 3], the vertex count)."""
    rows, base = [], 0
    for n in sizes:
        rows += [(base, base + 1 + j, base + 2 + j) for j in range(n)]
        base += n + 2
    return np.asarray(rows, dtype=np.int32), base


def disjoint_strips(n_strips, length):
    """n_strips strips of `length` vertices each on consecutive ids: n_strips components of length - 2 triangles."""
    one = strip(length).astype(np.int64)
    t = (one[None, :, :] + (np.arange(n_strips, dtype=np.int64) * length)[:, None, None]).reshape(-1, 3)
    return t.astype(np.int32), n_strips * length
