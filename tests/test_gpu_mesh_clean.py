"""Floater removal on the device: connected components (cn_mesh_label_init / cn_mesh_label_rounds), the triangles
per component (cn_mesh_component_sizes) and the compaction to the kept components (cn_mesh_select /
cn_mesh_compact) against the host reference tests/mesh_clean_ref.py.  Labels, sizes, kept_vertices and the
renumbered triangles are integers: every comparison is exact.  Every case runs twice and the two runs must agree
bit for bit (the labels' fixed point does not depend on the order of the atomics)."""
import numpy as np
import pytest
import torch

import mesh_clean_ref as C
import mesh_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def _positions(V):
    """Vertex positions that name their vertex: (id, 2 id + 1, -id)."""
    i = torch.arange(V, dtype=torch.float32, device=DEV)
    return torch.stack([i, 2 * i + 1, -i], dim=1).contiguous()


def _check(t, V, vertices=None, **kw):
    """ops.mesh_components / mesh_component_sizes / mesh_clean on the list t [T, 3] over V vertices against the host
    reference, twice; returns what the device gave (numpy) and the rounds used."""
    from copenerf import ops
    t = np.ascontiguousarray(t, dtype=np.int32).reshape(-1, 3)
    tri = torch.from_numpy(t).to(DEV)
    vertices = _positions(V) if vertices is None else vertices
    kept_ref, tri_ref, lab_ref, cnt_ref = C.clean(t, V, **kw)
    runs = []
    for _ in range(2):
        label, rounds = ops.mesh_components(tri, V)
        cnt = ops.mesh_component_sizes(tri, label)
        stats = {}
        v2, t2, kept = ops.mesh_clean(vertices, tri, stats=stats, **kw)
        assert label.dtype == cnt.dtype == kept.dtype == t2.dtype == torch.int32 and v2.dtype == vertices.dtype
        assert label.is_cuda and cnt.is_cuda and kept.is_cuda and t2.is_cuda and v2.is_cuda
        assert label.shape == cnt.shape == (V,) and t2.shape == (len(tri_ref), 3) and kept.shape == (len(kept_ref),)
        assert v2.shape == (len(kept_ref), 3)
        assert rounds < ops.mesh_components_cap(V), (rounds, V)
        assert stats["components"] == len(np.unique(lab_ref))
        assert stats["components_kept"] == len(np.unique(lab_ref[kept_ref]))
        runs.append((label, cnt, kept, t2, v2, rounds))
    for a, b in zip(runs[0][:5], runs[1][:5]):
        assert torch.equal(a, b)
    label, cnt, kept, t2, v2, rounds = runs[0]
    assert np.array_equal(label.cpu().numpy(), lab_ref)
    assert np.array_equal(cnt.cpu().numpy(), cnt_ref)
    assert np.array_equal(kept.cpu().numpy(), kept_ref)
    assert np.array_equal(t2.cpu().numpy(), tri_ref)
    assert torch.equal(v2, vertices[kept.long()])
    return kept.cpu().numpy(), t2.cpu().numpy(), v2.cpu().numpy(), rounds


# -- 1. mesher outputs -----------------------------------------------------------------------------------
def _device_mesh(make):
    from copenerf import ops
    u = torch.from_numpy(make()).to(DEV)
    v, t = ops.isosurface(u, 0.0, *BOX)
    return v, t


def test_two_spheres_keep_the_largest_component():
    """Two components; the kept one is a closed, oriented sphere: Euler characteristic 2, positive volume."""
    v, t = _device_mesh(R.two_spheres)
    kept, tri, pos, _ = _check(t.cpu().numpy(), len(v), vertices=v, keep_largest=True)
    assert 0 < len(tri) < len(t) and 0 < len(kept) < len(v)
    assert R.is_closed_oriented(tri, len(kept))
    assert R.euler_characteristic(tri, len(kept)) == 2
    assert R.signed_volume(pos, tri) > 0
    assert (pos > 0).all()  # the larger sphere: radius 0.30 around (+0.45, +0.45, +0.45)
    # min_triangles at the larger sphere's size keeps the same mesh; at the smaller one's, both
    from copenerf import ops
    v1, t1, k1 = ops.mesh_clean(v, t, min_triangles=len(tri))
    assert np.array_equal(k1.cpu().numpy(), kept) and np.array_equal(t1.cpu().numpy(), tri)
    v2, t2, k2 = ops.mesh_clean(v, t, min_triangles=len(t) - len(tri))
    assert torch.equal(v2, v) and torch.equal(t2, t)


def test_torus_is_one_component_and_comes_back_bitwise():
    from copenerf import ops
    v, t = _device_mesh(R.torus)
    kept, tri, pos, _ = _check(t.cpu().numpy(), len(v), vertices=v, keep_largest=True)
    assert np.array_equal(kept, np.arange(len(v)))
    v2, t2, k2 = ops.mesh_clean(v, t, keep_largest=True)
    assert torch.equal(v2, v) and torch.equal(t2, t)
    assert torch.equal(k2, torch.arange(len(v), dtype=torch.int32, device=DEV))


def test_empty_mesh():
    from copenerf import ops
    v = torch.empty(0, 3, device=DEV)
    t = torch.empty(0, 3, dtype=torch.int32, device=DEV)
    for kw in (dict(keep_largest=True), dict(min_triangles=3)):
        stats = {}
        v2, t2, kept = ops.mesh_clean(v, t, stats=stats, **kw)
        assert v2.shape == (0, 3) and t2.shape == (0, 3) and kept.shape == (0,)
        assert t2.dtype == kept.dtype == torch.int32 and stats == dict(components=0, components_kept=0, rounds=0)
    # vertices without triangles: every vertex its own component of no triangles
    kept, tri, _, rounds = _check(np.zeros((0, 3), np.int32), 5, keep_largest=True)
    assert len(kept) == 0 and rounds == 0
    kept, tri, _, _ = _check(np.zeros((0, 3), np.int32), 5, min_triangles=1)
    assert len(kept) == 0


# -- 2. many rounds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [None, 5])
def test_strip_of_4099_vertices_needs_many_rounds(seed):
    """triangles[i] = (i, i + 1, i + 2): one component about 2049 edges across.  With ascending ids the jumps
    double the reach of a label every round; with the ids permuted the labels travel against the id order and the
    rounds run into the hundreds -- always below the cap ops.mesh_components states."""
    from copenerf import ops
    V = 4099
    t = C.strip(V, seed)
    kept, tri, _, rounds = _check(t, V, keep_largest=True)
    print("strip seed", seed, "rounds", rounds, "cap", ops.mesh_components_cap(V))
    assert np.array_equal(kept, np.arange(V)) and np.array_equal(tri, t)
    label, r2 = ops.mesh_components(torch.from_numpy(t).to(DEV), V, rounds_per_call=3)
    assert bool((label == 0).all()) and 0 < r2 < ops.mesh_components_cap(V)


# -- 3. ties and thresholds ------------------------------------------------------------------------------
def test_fans_ties_and_thresholds():
    """Three disjoint fans of 5, 5 and 3 triangles (roots 0, 7, 14)."""
    t, V = C.fans()
    kept, tri, _, _ = _check(t, V, keep_largest=True)
    assert np.array_equal(kept, np.arange(7)) and np.array_equal(tri, t[:5])  # the tie: the smaller root id
    kept, tri, _, _ = _check(t, V, min_triangles=4)
    assert np.array_equal(kept, np.arange(14)) and np.array_equal(tri, t[:10])
    kept, tri, _, _ = _check(t, V, min_triangles=6)
    assert kept.shape == (0,) and tri.shape == (0, 3)
    kept, tri, _, _ = _check(t, V, keep_largest=True, min_triangles=6)
    assert kept.shape == (0,) and tri.shape == (0, 3)
    # the tie again with the equal fans listed the other way round, and with isolated vertices in front
    order = np.concatenate([np.arange(5, 10), np.arange(0, 5), np.arange(10, 13)])
    kept, tri, _, _ = _check(t[order], V, keep_largest=True)
    assert np.array_equal(kept, np.arange(7)) and np.array_equal(tri, t[:5])
    kept, tri, _, _ = _check(t[5:], V, keep_largest=True)
    assert np.array_equal(kept, np.arange(7, 14)) and np.array_equal(tri, t[5:10] - 7)
    kept, tri, _, _ = _check(t[5:], V, min_triangles=3)
    assert np.array_equal(kept, np.arange(7, 19))


# -- 4. buffers smaller than the counts ------------------------------------------------------------------
def test_compact_writes_nothing_into_buffers_smaller_than_the_counts():
    from copenerf import ops
    t, V = C.fans()
    tri = torch.from_numpy(t).to(DEV)
    label, _ = ops.mesh_components(tri, V)
    cnt = ops.mesh_component_sizes(tri, label)
    d, ws, counts = ops.mesh_select(tri, label, cnt, min_triangles=4)
    Vk, Tk = counts.tolist()
    assert (Vk, Tk) == (14, 10)
    i32 = lambda n, *s: torch.full((n, *s), -7, dtype=torch.int32, device=DEV)  # noqa: E731
    with pytest.raises(RuntimeError, match="buffers"):
        ops.mesh_compact(d, ws, i32(Vk - 1), i32(Tk, 3), (Vk, Tk))
    for nv, nt in ((Vk - 1, Tk), (Vk, Tk - 1), (0, Tk), (Vk, 0)):
        kv, to = i32(nv), i32(nt, 3)
        ops.mesh_compact(d, ws, kv, to)  # the kernel's own check against the device counts
        assert bool((kv == -7).all()) and bool((to == -7).all()), (nv, nt)
    kv, to = i32(Vk + 3), i32(Tk + 2, 3)  # larger buffers: the tail stays untouched
    ops.mesh_compact(d, ws, kv, to, (Vk, Tk))
    kept_ref, tri_ref, _, _ = C.clean(t, V, min_triangles=4)
    assert np.array_equal(kv[:Vk].cpu().numpy(), kept_ref) and bool((kv[Vk:] == -7).all())
    assert np.array_equal(to[:Tk].cpu().numpy(), tri_ref) and bool((to[Tk:] == -7).all())


# -- 5. the scans' second level --------------------------------------------------------------------------
def test_more_than_1024_scan_tiles():
    """The compaction reuses the mesher's scan_launch (tiles of 1024 flags, one block over the tile totals, 1024
    totals per round), so one list just past 1024 tiles is enough: 32,769 disjoint strips of 32 triangles behind
    the three fans, T = 1,048,621 and V = 1,114,165, both more than 1024 x 1024.  min_triangles = 6 drops the fans,
    so every kept id moves."""
    f, Vf = C.fans()
    s, Vs = C.disjoint_strips(32769, 34)
    t = np.concatenate([f, s + Vf])
    V = Vf + Vs
    assert len(t) > 1024 * 1024 and V > 1024 * 1024
    kept, tri, _, rounds = _check(t, V, min_triangles=6)
    assert len(kept) == Vs and len(tri) == len(s) and kept[0] == Vf and np.array_equal(tri, s)
