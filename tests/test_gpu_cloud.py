"""csrc/cn_cloud.hip against the float64 numpy reference (tests/cloud_ref.py): the voxel down-sampling passes
(cn_voxel_keys, cn_voxel_reduce), PCA normals from neighbour rows (cn_cloud_normals) and the statistical outlier
filter's sums (cn_knn_mean_stats)."""
import math

import numpy as np
import pytest
import torch

import cloud_ref
from cloud_ref import KEY_NONE, angle, ellipsoid, normals_ref, voxel_keys_ref, voxel_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64).astype(np.float32))).astype(np.float64)


def _voxel_cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3), dtype=np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    col = rng.random((n, 3), dtype=np.float32)
    return p, nrm, col


# voxel sizes: one voxel, about 8 points per voxel, all-singleton voxels
def _voxel_sizes(n):
    return (2.0, max((8.0 / n) ** (1.0 / 3.0), 1e-3), 1e-5)


@pytest.mark.parametrize("n", [1, 255, 257, 5000])
def test_voxel_down_sample_matches_reference(n):
    from copenerf import metrics, ops
    p, nrm, col = _voxel_cloud(n, 20 + n)
    origin = (0.0, 0.0, 0.0)
    for voxel in _voxel_sizes(n):
        ref = voxel_ref(p, origin, voxel, nrm, col)
        keys, valid = ops.voxel_keys(_dev(p), origin, voxel, want_valid=True)
        assert np.array_equal(keys.cpu().numpy(), voxel_keys_ref(p, origin, voxel)) and bool((valid == 1).all())
        skeys, order = torch.sort(keys, stable=True)
        out = ops.voxel_reduce(skeys, order, _dev(p), _dev(nrm), _dev(col))
        M, dropped = out["totals"].tolist()
        assert (M, dropped) == (len(ref["keys"]), 0)
        assert np.array_equal(out["keys"][:M].cpu().numpy(), ref["keys"])
        assert np.array_equal(out["counts"][:M].cpu().numpy(), ref["counts"])
        for name in ("points", "normals", "colors"):
            got = out[name][:M].cpu().numpy().astype(np.float64)
            err = np.abs(got - ref[name]) / _ulp32(ref[name])
            print(f"n={n} voxel={voxel:g} {name}: {M} voxels, max err {err.max():.3f} ulp")
            assert np.all(err <= 1.0)
        length = np.linalg.norm(out["normals"][:M].cpu().numpy().astype(np.float64), axis=1)
        assert np.all(np.abs(length - 1.0) < 1e-6)  # re-normalised
        # bitwise repeatable, and the metric entry returns the same rows
        out2 = ops.voxel_reduce(skeys, order, _dev(p), _dev(nrm), _dev(col))
        assert all(torch.equal(out[k_][:M], out2[k_][:M]) for k_ in ("points", "normals", "colors", "counts", "keys"))
        res = metrics.voxel_down_sample(_dev(p), voxel, _dev(nrm), _dev(col), origin=origin)
        assert torch.equal(res["points"], out["points"][:M]) and torch.equal(res["normals"], out["normals"][:M])
        assert torch.equal(res["colors"], out["colors"][:M]) and res["n_dropped"] == 0
    if n == 1:
        assert M == 1
    if n == 5000:
        assert M == 5000  # the last size: all singletons, each mean its own point
        assert np.array_equal(np.sort(out["points"][:M].cpu().numpy(), axis=0), np.sort(p, axis=0))


def test_voxel_faces_dropped_points_and_zero_normals():
    from copenerf import metrics, ops
    voxel, origin = 0.25, (-1.0, -1.0, -1.0)
    rng = np.random.default_rng(5)
    p = (rng.integers(0, 8, (400, 3)) * 0.25 - 1.0).astype(np.float32)  # every point exactly on voxel faces
    p[100:200] += rng.random((100, 3), dtype=np.float32) * 0.25
    p[7] = (np.nan, 0.0, 0.0)
    p[8] = (0.0, np.inf, 0.0)
    p[9] = (0.0, 0.0, -1.0 + 0.25 * 2 ** 21)       # the first voxel index beyond 21 bits
    p[10] = (-1.0 - 1e-3, 0.0, 0.0)                # below the origin: outside, not clamped into voxel 0
    p[11] = (0.0, 0.0, -1.0 + 0.25 * (2 ** 21 - 1))  # the last voxel inside
    nrm = rng.standard_normal((400, 3)).astype(np.float32)
    nrm[300], nrm[301] = (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)
    p[300] = p[301] = (0.9, 0.9, 0.9)              # a voxel of their own whose normals cancel: a zero normal
    with np.errstate(invalid="ignore"):
        p[np.all(p >= 0.75, axis=1) & (np.arange(400) != 300) & (np.arange(400) != 301)] = (0.0, 0.0, 0.0)
    ref = voxel_ref(p, origin, voxel, nrm)
    assert ref["n_dropped"] == 4
    keys, valid = ops.voxel_keys(_dev(p), origin, voxel, want_valid=True)
    k = keys.cpu().numpy()
    assert np.array_equal(k, voxel_keys_ref(p, origin, voxel))
    assert np.all(k[[7, 8, 9, 10]] == KEY_NONE) and k[11] == (4 << 42) | (4 << 21) | (2 ** 21 - 1)
    assert np.array_equal(valid.cpu().numpy() == 0, k == KEY_NONE)
    res = metrics.voxel_down_sample(_dev(p), voxel, _dev(nrm), origin=origin)
    assert res["n_dropped"] == 4 and res["points"].shape[0] == len(ref["keys"]) == int(res["counts"].shape[0])
    assert int(res["counts"].sum()) == 396 and np.array_equal(res["counts"].cpu().numpy(), ref["counts"])
    got = res["points"].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - ref["points"]) <= _ulp32(ref["points"]))
    gn = res["normals"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(gn - ref["normals"]) <= _ulp32(np.maximum(np.abs(ref["normals"]), 1e-30)))
    zero = np.flatnonzero(np.all(ref["normals"] == 0, axis=1))
    assert len(zero) == 1 and np.all(gn[zero] == 0.0)
    # the default origin is the smallest finite coordinate: the NaN and the infinity do not poison it, and the point
    # below the old origin is now inside
    auto = metrics.voxel_down_sample(_dev(p), voxel)
    assert auto["n_dropped"] == 3 and int(auto["counts"].sum()) == 397
    empty = metrics.voxel_down_sample(torch.zeros(0, 3, device=DEV), voxel)
    assert empty["points"].shape == (0, 3) and empty["n_dropped"] == 0


@pytest.fixture(scope="module")
def ell():
    from copenerf import metrics
    p, analytic = ellipsoid(3000, 11)
    pts = _dev(p)
    _, index = metrics.knn(pts, pts, 16)
    ref_n, eig, valid = normals_ref(p, index.cpu().numpy())
    return {"p": p, "pts": pts, "analytic": analytic, "index": index, "ref_n": ref_n, "eig": eig, "valid": valid}


def test_normals_match_eigh_on_the_same_rows(ell):
    from copenerf import ops
    normals, variation = ops.cloud_normals(ell["pts"], ell["index"], want_variation=True)
    n = normals.cpu().numpy().astype(np.float64)
    eig = ell["eig"]
    # checked on the reference: thin neighbourhoods, every row has a clear smallest eigenvalue
    assert np.all(ell["valid"]) and np.max(eig[:, 0] / eig[:, 1]) < 0.0215  # (0.02123 in float64)
    rows = (eig[:, 1] - eig[:, 0]) / eig[:, 2] >= 1e-3
    assert rows.all()
    a = angle(n, ell["ref_n"])
    print(f"own rows: max angle {a[rows].max():.3e} rad over {rows.sum()} rows (bar 1e-6)")
    assert np.all(a[rows] <= 1e-6)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1.0) < 1e-6)
    var_ref = eig[:, 0] / eig.sum(1)
    assert np.all(np.abs(variation.cpu().numpy() - var_ref) <= 1e-6 * var_ref + 1e-9)
    # against the analytic normal: the device's mean and max angle within 0.01 degree of the reference's
    dev_a, ref_a = np.degrees(angle(n, ell["analytic"])), np.degrees(angle(ell["ref_n"], ell["analytic"]))
    print(f"analytic: device mean {dev_a.mean():.4f} max {dev_a.max():.4f}, reference mean {ref_a.mean():.4f} max {ref_a.max():.4f} deg")
    assert abs(dev_a.mean() - ref_a.mean()) <= 0.01 and abs(dev_a.max() - ref_a.max()) <= 0.01
    # bitwise repeatable; the metric entry is the same composition
    from copenerf import metrics
    again, _ = ops.cloud_normals(ell["pts"], ell["index"])
    assert torch.equal(normals, again) and torch.equal(metrics.estimate_normals(ell["pts"], 16), normals)


def test_normal_sign_rules(ell):
    from copenerf import ops
    n = ops.cloud_normals(ell["pts"], ell["index"])[0].cpu().numpy()
    big = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], axis=1)[:, 0]  # (argmax: the first on a tie)
    assert np.all(big > 0)
    p = ell["p"].astype(np.float64)
    for to in ((0.0, 0.0, 0.0), (3.0, -2.0, 1.0)):
        m = ops.cloud_normals(ell["pts"], ell["index"], orient_to=to)[0].cpu().numpy()
        dots = np.sum(m.astype(np.float64) * (np.asarray(to) - p), axis=1)
        assert np.all(dots >= 0) and np.all(np.abs(m) == np.abs(n))  # the same normals, flipped
    inward = ops.cloud_normals(ell["pts"], ell["index"], orient_to=(0.0, 0.0, 0.0))[0].cpu().numpy()
    assert np.all(np.sum(inward * ell["analytic"], axis=1) < 0)  # towards the centre: against the outward normal


def test_normals_degenerate_rows_and_foreign_indices():
    from copenerf import ops
    rng = np.random.default_rng(3)
    p = rng.random((64, 3), dtype=np.float32)
    p[10:20] = np.linspace(0, 1, 10, dtype=np.float32)[:, None] * np.array([1.0, 2.0, -1.0], dtype=np.float32)  # a line
    p[30] = (np.nan, 0.5, 0.5)
    N, k = len(p), 8
    index = np.stack([rng.permutation(N)[:k] for _ in range(N)]).astype(np.int32)
    index[index == 30] = 31                      # nobody gathers the NaN point ...
    index[5] = (30, 1, 2, 3, 4, 6, 7, 8)         # ... but row 5, and row 30 is the NaN point itself
    index[0] = (0, 1, -1, -1, -1, -1, -1, -1)    # fewer than 3 neighbours
    index[1] = (-1,) * k
    index[12] = (10, 11, 12, 13, 14, 15, 16, 17)  # collinear
    index[40] = (40, 41, 42, 43, N, 2 ** 31 - 1, -7, -1)  # foreign entries: ignored, never gathered
    normals, variation = ops.cloud_normals(_dev(p), _dev(index), want_variation=True)
    torch.cuda.synchronize()
    n = normals.cpu().numpy().astype(np.float64)
    ref_n, eig, valid = normals_ref(p, index)
    assert not valid[[0, 1, 5, 12, 30]].any() and valid[40] and valid.sum() == N - 5
    assert np.all(n[~valid] == 0.0) and np.all(variation.cpu().numpy()[~valid] == 0.0)
    rows = valid & ((eig[:, 1] - eig[:, 0]) / np.maximum(eig[:, 2], 1e-300) >= 1e-3)
    assert rows[40] and rows.sum() > 40
    assert np.all(angle(n[rows], ref_n[rows]) <= 1e-6)
    clean = index[40].copy()
    clean[4:] = -1
    index[40] = clean
    assert np.array_equal(ops.cloud_normals(_dev(p), _dev(index))[0].cpu().numpy()[40], normals.cpu().numpy()[40])


def test_statistical_outliers_match_reference():
    from copenerf import metrics, ops
    p, _ = ellipsoid(2000, 12)
    rng = np.random.default_rng(13)
    far = (rng.standard_normal((20, 3)) * 0.2 + np.array([2.0, 2.0, 2.0])).astype(np.float32)
    pts_np = np.concatenate([p, far])
    pts = _dev(pts_np)
    k, ratio = 20, 2.0
    dist, index = metrics.knn(pts, pts, k, exclude_self=True)
    mean, sums = ops.knn_mean_stats(dist, index)
    # the reference rule on float64 means of the device's own (fp32) neighbour distances, rounded to fp32 as stored
    m_ref = cloud_ref.knn_means_ref(dist.cpu().numpy(), index.cpu().numpy()).astype(np.float32)
    assert np.array_equal(mean.cpu().numpy(), m_ref)
    mu, sigma, cut, keep = cloud_ref.outlier_ref(m_ref, ratio)
    assert np.min(np.abs(m_ref.astype(np.float64) - cut)) > 1e-6 * cut  # no mean sits on the cut
    mu_d, sigma_d, cut_d = metrics.outlier_cut(sums.tolist(), ratio)
    print(f"outliers: mu rel err {abs(mu_d - mu) / mu:.2e}, sigma rel err {abs(sigma_d - sigma) / sigma:.2e} (bar 1e-11)")
    assert sums.tolist()[0] == len(pts_np)
    assert abs(mu_d - mu) <= 1e-11 * mu and abs(sigma_d - sigma) <= 1e-11 * sigma
    kept, mask = metrics.remove_statistical_outliers(pts, k, ratio)
    assert np.array_equal(mask.cpu().numpy(), keep) and torch.equal(kept, pts[mask])
    assert not mask[2000:].any() and mask[:2000].sum().item() > 1900  # the planted points go, the surface stays
    # also against brute-force float64 neighbours: the same mask
    d64, _ = cloud_ref.brute_knn(pts_np, pts_np, k, exclude_self=True)
    assert np.array_equal(cloud_ref.outlier_ref(d64.mean(1), ratio)[3], keep)
    mean2, sums2 = ops.knn_mean_stats(dist, index)
    assert torch.equal(mean, mean2) and torch.equal(sums, sums2)
    # rows without a neighbour: an infinite mean, left out of the sums
    index[3] = -1
    mean3, sums3 = ops.knn_mean_stats(dist, index)
    assert math.isinf(mean3[3].item()) and sums3.tolist()[0] == len(pts_np) - 1
