"""cn_nn_grid_build / cn_nn_query against float64 brute force (tests/mesh_eval_ref.py): the distance within the
bound the fp32 arithmetic gives, |d - d64| <= 8 x 2^-24 d64 + 1e-30, and the index equal to the float64 argmin for
every query -- the seeds are such that float64 separates the two nearest distinct distances by more than that
bound, which every case asserts on the reference first; no query is excluded."""
import math

import numpy as np
import pytest
import torch

from mesh_eval_ref import brute_nn, dist_bar

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf


def _cube(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


def _unit(dims, cell=None, origin=(0.0, 0.0, 0.0)):
    return origin, (1.0 / max(dims) if cell is None else cell), dims


# name -> (queries, targets, (origin, cell, dims), max_dist)
def _cases():
    t, q = _cube(777, 1), _cube(1000, 2)
    c = {
        "one_cell": (q, t, _unit((1, 1, 1)), INF),
        "3x5x7": (q, t, _unit((3, 5, 7)), INF),                  # 1/7 cells: x and y targets beyond the grid
        "40^3": (q, t, _unit((40, 40, 40)), INF),                # mostly empty cells
        "n=1": (q, _cube(1, 3), _unit((4, 4, 4)), INF),
        "tails": (_cube(65, 4), _cube(257, 5), _unit((6, 6, 6)), INF),
        "targets_in_one_cell": (q, 0.51 + 0.1 * _cube(300, 6), _unit((8, 8, 8), cell=0.125), INF),
        "targets_outside_grid": (q, t, ((0.25, 0.25, 0.25), 0.1, (5, 5, 5)), INF),
        "max_dist": (q, t, _unit((12, 12, 12)), 0.06),
        "max_dist_sparse": (q, _cube(20, 7), _unit((40, 40, 40)), 0.15),
    }
    dup = t.copy()
    dup[700:750] = dup[:50]                                      # exact duplicates: the smaller index must win
    dup[760:770] = dup[40:50]                                    # (three copies of some)
    c["duplicates"] = (np.concatenate([q[:900], dup[:100] + np.float32(1e-3)]), dup, _unit((10, 10, 10)), INF)
    out = q.copy()
    out[:300, 0] += 1.5                                          # half an extent beyond the +x face
    out[300:600] -= 1.5                                          # beyond a corner
    out[600:620, 1] = 11.0 - out[600:620, 1]                     # ten extents beyond +y
    out[620:640, 2] -= 10.0                                      # ten extents below (the rest stay inside)
    c["queries_outside"] = (out, t, _unit((9, 9, 9)), INF)
    c["queries_outside_max_dist"] = (out, t, _unit((9, 9, 9)), 1.2)
    return c


CASES = _cases()
_REF = {}


def _ref(name):
    if name not in _REF:
        q, t, _, _ = CASES[name]
        _REF[name] = brute_nn(q, t)
    return _REF[name]


def _check(name, ref, dist, index, max_dist):
    d64, i64, second = ref
    bar = dist_bar(d64)
    # the reference separates the nearest from the next distinct distance, and from max_dist, for every query
    assert np.all(second - d64 > bar + dist_bar(np.minimum(second, 1e300))), name  # (inf: no other distance)
    assert np.all(np.abs(d64 - max_dist) > bar), name
    near = d64 < max_dist
    dist, index = dist.cpu().numpy().astype(np.float64), index.cpu().numpy()
    err = np.abs(dist - d64)[near]
    print(f"{name}: {near.sum()} of {len(near)} within max_dist, max err / bar {np.max(err / bar[near], initial=0):.3f}")
    assert np.all(err <= bar[near])
    assert np.array_equal(index[near], i64[near])
    assert np.all(dist[~near] == np.float32(max_dist)) and np.all(index[~near] == -1)


@pytest.mark.parametrize("name", list(CASES))
def test_nn_query_matches_brute_force(name):
    from copenerf import ops
    q, t, (origin, cell, dims), max_dist = CASES[name]
    grid = ops.nn_grid(torch.from_numpy(t).to(DEV), origin, cell, dims)
    dist, index = ops.nn_query(grid, torch.from_numpy(q).to(DEV), max_dist)
    _check(name, _ref(name), dist, index, max_dist)
    if name == "duplicates":
        i = index.cpu().numpy()
        assert np.all((i < 700) | (i >= 770) | ((i >= 750) & (i < 760)))  # never the later copy
    if name == "queries_outside_max_dist":
        assert (index[600:640] == -1).all() and (index[640:] >= 0).all()  # nothing ten extents away, inside all
    # the same through binned queries: bitwise the same outputs, at the queries' own positions
    binned = ops.nn_grid(torch.from_numpy(q).to(DEV), origin, cell, dims)
    dist2, index2 = ops.nn_query(grid, binned.sorted, max_dist, records=True)
    assert torch.equal(dist, dist2) and torch.equal(index, index2)
    d3, none = ops.nn_query(grid, torch.from_numpy(q).to(DEV), max_dist, want_index=False)
    assert none is None and torch.equal(d3, dist)


@pytest.mark.parametrize("name", ["3x5x7", "40^3", "targets_outside_grid", "n=1"])
def test_nn_grid_build_sorts_points_into_cells(name):
    from copenerf import ops
    _, t, (origin, cell, dims), _ = CASES[name]
    grid = ops.nn_grid(torch.from_numpy(t).to(DEV), origin, cell, dims)
    # the cell of every point with the kernel's fp32 arithmetic: floor((p - o) / cell) clamped into the grid
    f = (t - np.asarray(origin, np.float32)) / np.float32(cell)
    ijk = np.clip(np.floor(f), 0, np.asarray(dims) - 1).astype(np.int64)
    ids = (ijk[:, 0] * dims[1] + ijk[:, 1]) * dims[2] + ijk[:, 2]
    ncells = dims[0] * dims[1] * dims[2]
    start = grid.cell_start.cpu().numpy()
    assert np.array_equal(start, np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=ncells))]))
    rec = grid.sorted.cpu().numpy()
    orig = rec[:, 3].copy().view(np.int32)
    assert np.array_equal(np.sort(orig), np.arange(len(t)))          # a permutation
    assert np.array_equal(rec[:, :3], t[orig])                        # every record holds its point
    assert np.all(np.diff(ids[orig]) >= 0)                            # grouped by ascending cell


def _clustered(n, seed):
    rng = np.random.default_rng(seed)
    blob = (0.5 + 0.05 * rng.standard_normal((n * 7 // 10, 3))).astype(np.float32)
    return np.concatenate([blob, rng.random((n - len(blob), 3), dtype=np.float32)])


def test_nearest_distances_clustered_20k_both_arms():
    from copenerf import metrics
    q, t = _clustered(20000, 11), _clustered(20000, 12)
    tq, tt = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    d_s, i_s = metrics.nearest_distances(tq, tt, sort_queries=True)
    d_u, i_u = metrics.nearest_distances(tq, tt, sort_queries=False)
    assert torch.equal(d_s, d_u) and torch.equal(i_s, i_u)  # bitwise
    _check("clustered", brute_nn(q, t), d_s, i_s, INF)
    d_c, i_c = metrics.nearest_distances(tq, tt, cell=0.2)  # a caller's cell size changes nothing
    assert torch.equal(d_c, d_s) and torch.equal(i_c, i_s)
    d_m, i_m = metrics.nearest_distances(tq, tt, max_dist=0.01)
    far = d_s >= 0.01
    assert torch.equal(torch.where(far, torch.full_like(d_s, 0.01), d_s), d_m)
    assert torch.equal(torch.where(far, torch.full_like(i_s, -1), i_s), i_m) and 0 < far.sum().item() < 20000


def test_nearest_distances_without_targets_or_queries():
    from copenerf import metrics
    q = torch.rand(5, 3, device=DEV)
    d, i = metrics.nearest_distances(q, torch.zeros(0, 3, device=DEV), max_dist=2.0)
    assert d.tolist() == [2.0] * 5 and i.tolist() == [-1] * 5
    d, i = metrics.nearest_distances(torch.zeros(0, 3, device=DEV), q)
    assert d.shape == (0,) and i.shape == (0,)
