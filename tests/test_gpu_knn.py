"""cn_knn_query against float64 brute force (tests/cloud_ref.py) on the shapes of test_gpu_nn.py, for k in
{1, 5, 8, 9, 16, 17, 32} (both sides of every capacity), with and without query records.

A row is CLEAR when the reference separates every consecutive pair of its first k + 1 ranks by more than the two
dist_bars (or the two targets are the same point bit for bit: then the order is the index's, on the device as in
the reference), and every rank from max_dist by more than its bar.  On a clear row the index row equals the
reference's and every distance is within dist_bar.  On any other row the returned set must be a valid k-nearest
set within the bar: distinct targets, each at the distance reported, ascending, none farther than the reference's
k-th distance plus the bars.  The share of such rows is capped at 0.5 % per case, asserted on the reference first.

Three cases put queries far from the targets (all targets in one 0.1 cell of the unit cube, and the two with queries
up to ten extents outside the grid).  There dist_bar, which is relative to the distance, grows while the gaps
between consecutive ranks -- set by the targets' own spacing along the line of sight -- shrink, and float64 itself
leaves 0.8 % to 1.6 % of the rows of those cases without a clear gap at k >= 16 (0.2 % to 0.4 % up to k = 9): no
implementation can meet 0.5 % there.  For those cases at k >= 16 the cap is 2 %, the reference's own share with a
margin; every row is checked all the same, and every other case keeps 0.5 %."""
import math

import numpy as np
import pytest
import torch

from cloud_ref import brute_knn
from mesh_eval_ref import dist_bar
from test_gpu_nn import CASES, _cube

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
KS = (1, 5, 8, 9, 16, 17, 32)
RANKS = 33
FAR_CASES = ("targets_in_one_cell", "queries_outside", "queries_outside_max_dist")
_REF = {}


def _ref(name, q, t, exclude_self=False):
    if name not in _REF:
        _REF[name] = brute_knn(q, t, RANKS, exclude_self)
    return _REF[name]


def _same_point(t, ia, ib):
    ok = (ia >= 0) & (ib >= 0)
    return ok & np.all(t[np.maximum(ia, 0)] == t[np.maximum(ib, 0)], axis=-1)


def _check(name, k, q, t, ref, dist, index, count, max_dist, exclude_self=False):
    d64, i64 = ref[0][:, :k + 1], ref[1][:, :k + 1]
    bar = dist_bar(np.where(np.isfinite(d64), d64, 0.0))
    with np.errstate(invalid="ignore"):
        gap = d64[:, 1:] - d64[:, :-1] > bar[:, 1:] + bar[:, :-1]
    gap |= ~np.isfinite(d64[:, 1:]) | _same_point(t, i64[:, :-1], i64[:, 1:])
    with np.errstate(invalid="ignore"):
        clear = gap.all(1) & np.all(~np.isfinite(d64) | (np.abs(d64 - max_dist) > bar), axis=1)
    cap = 0.02 if name in FAR_CASES and k >= 16 else 0.005
    assert (~clear).sum() <= cap * len(q), (name, k, int((~clear).sum()))  # the reference first
    dist, index = dist.cpu().numpy().astype(np.float64), index.cpu().numpy()
    assert dist.shape == index.shape == (len(q), k)
    near = (d64[:, :k] < max_dist) & (i64[:, :k] >= 0)
    # clear rows: the reference's index row, distances within the bar, the padding where the reference has none
    c = clear
    want = np.where(near, i64[:, :k], -1)
    assert np.array_equal(index[c], want[c]), (name, k)
    with np.errstate(invalid="ignore"):
        err = np.abs(dist - d64[:, :k])  # (inf - inf on the padding of both: not looked at)
    with np.errstate(invalid="ignore"):
        worst = np.max(np.where(c[:, None] & near, err / bar[:, :k], 0.0), initial=0.0)
    print(f"{name} k={k}: {int((~clear).sum())} unclear rows of {len(q)}, max err / bar {worst:.3f}")
    assert np.all(err[c][near[c]] <= bar[:, :k][c][near[c]])
    assert np.all(dist[c][~near[c]] == np.float32(max_dist))
    if count is not None:
        assert np.array_equal(count.cpu().numpy()[c], near.sum(1)[c])
    # the other rows: a valid k-nearest set within the bar
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    for r in np.flatnonzero(~clear):
        got = index[r][index[r] >= 0]
        assert len(set(got.tolist())) == len(got) and np.all(index[r][len(got):] == -1)
        assert not (exclude_self and r in got)
        true = np.sqrt(((q64[r] - t64[got]) ** 2).sum(1))
        assert np.all(np.abs(dist[r][:len(got)] - true) <= dist_bar(true)) and np.all(np.diff(dist[r][:len(got)]) >= 0)
        kth = d64[r][:k][np.isfinite(d64[r][:k])]
        if len(got):
            assert true.max() <= kth[-1] + 2 * dist_bar(kth[-1]) and true.max() < max_dist + dist_bar(max_dist)
        assert abs(len(got) - near[r].sum()) <= (np.abs(d64[r] - max_dist) <= bar[r]).sum()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", list(CASES))
def test_knn_query_matches_brute_force(name, k):
    from copenerf import ops
    q, t, (origin, cell, dims), max_dist = CASES[name]
    tq = torch.from_numpy(q).to(DEV)
    grid = ops.nn_grid(torch.from_numpy(t).to(DEV), origin, cell, dims)
    dist, index, count = ops.knn_query(grid, tq, k, max_dist, want_count=True)
    _check(name, k, q, t, _ref(name, q, t), dist, index, count, max_dist)
    # the same through binned queries: bitwise the same outputs, at the queries' own positions
    binned = ops.nn_grid(tq, origin, cell, dims)
    dist2, index2, count2 = ops.knn_query(grid, binned.sorted, k, max_dist, want_count=True, records=True)
    assert torch.equal(dist, dist2) and torch.equal(index, index2) and torch.equal(count, count2)
    # a second run over a rebuilt grid (another order inside the cells, perhaps): bitwise the same
    grid3 = ops.nn_grid(torch.from_numpy(t).to(DEV), origin, cell, dims)
    dist3, index3, none = ops.knn_query(grid3, tq, k, max_dist)
    assert none is None and torch.equal(dist, dist3) and torch.equal(index, index3)
    if k == 1:  # bitwise cn_nn_query's
        d1, i1 = ops.nn_query(grid, tq, max_dist)
        assert torch.equal(dist[:, 0], d1) and torch.equal(index[:, 0], i1)
    if k > len(t):  # the padding of a row longer than the cloud
        assert (index[:, len(t):] == -1).all() and (dist[:, len(t):] == np.float32(max_dist)).all()
    if name == "duplicates":
        # exact duplicates are ordered by index: wherever two neighbours of a row are the same point, the earlier has
        # the smaller index (and at k = 1 it is never the later copy)
        i = index.cpu().numpy()
        same = _same_point(t, i[:, :-1], i[:, 1:])
        assert np.all(i[:, :-1][same] < i[:, 1:][same])
        assert k == 1 or same.sum() > 50


@pytest.mark.parametrize("k", KS)
def test_knn_self_query_exclude_self(k):
    from copenerf import ops
    t = _cube(777, 1)
    dup = t.copy()
    dup[700:750] = dup[:50]  # exact duplicates stay neighbours of one another
    for name, pts in (("self", t), ("self_dup", dup)):
        tt = torch.from_numpy(pts).to(DEV)
        grid = ops.nn_grid(tt, (0.0, 0.0, 0.0), 0.1, (10, 10, 10))
        d_in, i_in, _ = ops.knn_query(grid, tt, k)
        _check(name, k, pts, pts, _ref(name, pts, pts), d_in, i_in, None, INF)
        d_ex, i_ex, _ = ops.knn_query(grid, tt, k, exclude_self=True)
        _check(name + "_ex", k, pts, pts, _ref(name + "_ex", pts, pts, True), d_ex, i_ex, None, INF, exclude_self=True)
        assert not (i_ex == torch.arange(len(pts), device=DEV, dtype=torch.int32)[:, None]).any()
        d_r, i_r, _ = ops.knn_query(grid, grid.sorted, k, exclude_self=True, records=True)  # the grid's own records
        assert torch.equal(d_ex, d_r) and torch.equal(i_ex, i_r)
        if name == "self_dup":
            i = i_ex.cpu().numpy()
            assert np.array_equal(i[:50, 0], np.arange(700, 750)) and np.array_equal(i[700:750, 0], np.arange(50))
            assert np.all(d_ex.cpu().numpy()[:50, 0] == 0.0)
        else:
            assert (i_in[:, 0] == torch.arange(777, device=DEV, dtype=torch.int32)).all() and (d_in[:, 0] == 0).all()


def test_knn_metric_entry_matches_ops_and_handles_empty():
    from copenerf import metrics
    q, t = _cube(1000, 2), _cube(777, 1)
    tq, tt = torch.from_numpy(q).to(DEV), torch.from_numpy(t).to(DEV)
    dist, index = metrics.knn(tq, tt, 9)
    _check("metric", 9, q, t, _ref("3x5x7", q, t), dist, index, None, INF)
    d, i = metrics.knn(tq, torch.zeros(0, 3, device=DEV), 4, max_dist=2.0)
    assert d.shape == (1000, 4) and (d == 2.0).all() and (i == -1).all()
    with pytest.raises(ValueError):
        metrics.knn(tq, tt, 33)
    with pytest.raises(ValueError):
        metrics.knn(tq, tt, 4, exclude_self=True)
