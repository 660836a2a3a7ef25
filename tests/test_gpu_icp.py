"""cn_cloud_transform, cn_icp_accumulate and metrics.icp_register on the device against the float64
restatement tests/icp_ref.py.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

import icp_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = math.inf
AXIS = (0.3, -0.5, 0.8)
MOTION = dict(degrees=5.0, t=(0.04, -0.03, 0.05))
SIM = icp_ref.similarity(icp_ref.rotation((0.2, 0.9, -0.4), 33.0), (0.31, -1.7, 0.52), 1.37)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _cube(n, seed):
    return np.random.default_rng(seed).random((n, 3), dtype=np.float32)


# ---- the transform ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 255, 257, 5000))
def test_cloud_transform_within_4_ulp_of_the_largest_term(N):
    from copenerf import ops
    p = (4.0 * _cube(N, N) - 2.0).astype(np.float32)
    got = ops.cloud_transform(_dev(p), SIM).cpu().numpy()
    exact, largest = icp_ref.transform_terms(SIM[:3].astype(np.float32), p)
    ulp = np.spacing(largest.astype(np.float32)).astype(np.float64)
    worst = (np.abs(got.astype(np.float64) - exact) / ulp).max()
    # the bound three correctly rounded steps s1 = t + a x, s2 = s1 + b y, s3 = s2 + c z cannot exceed, per element:
    # 2^-24 (|s1| + |s2| + |s3|) -- at most 4.5 x 2^-23 of the largest term, reached only by four like-signed terms of
    # one size.  The result is a fixed function of these seeded inputs (no contraction or ordering is left open), so the
    # figures printed here are the same on every run.
    M, p64 = SIM[:3].astype(np.float32).astype(np.float64), p.astype(np.float64)
    s1 = M[None, :, 3] + M[None, :, 0] * p64[:, None, 0]
    s2 = s1 + M[None, :, 1] * p64[:, None, 1]
    s3 = s2 + M[None, :, 2] * p64[:, None, 2]
    derived = 2.0 ** -24 * (np.abs(s1) + np.abs(s2) + np.abs(s3)) * (1 + 2.0 ** -20)
    share = (np.abs(got.astype(np.float64) - exact) / np.where(derived > 0, derived, 1.0)).max()
    print(f"N {N}: max error {worst:.3f} ulp of the largest term (bar 4), {share:.3f} of the derived rounding bound")
    assert worst <= 4.0
    assert np.all(np.abs(got.astype(np.float64) - exact) <= derived)
    # any float dtype of matrix is rounded to fp32 once, on the host; out may be given
    out = torch.empty(N, 3, device=DEV)
    assert ops.cloud_transform(_dev(p), torch.from_numpy(SIM.astype(np.float32)), out=out) is out
    assert np.array_equal(out.cpu().numpy(), got)


def _box_grid(t, dims):
    lo, hi = t.min(0), t.max(0)
    cell = float(max((hi - lo).max() / max(dims), 1e-3)) * 1.0001
    return tuple(float(x) for x in lo), cell, dims


# ---- the sums -------------------------------------------------------------------------------------------------
SUMS_BAR = 1e-11  # x sum |term| per slot: below the Q 2^-53 sum |term| that reordering exact-in-double terms can move
N_TARGETS = 5000
_SUMS = {}


def _sums_case(Q):
    """Device-made inputs of one Q, shared by the modes and pivots: targets, normals (a few zero and NaN), the source,
    the device's own index (some -1 from max_dist, a few foreign values past N) and cloud_transform output."""
    if Q not in _SUMS:
        from copenerf import ops
        t = (_cube(N_TARGETS, 31) + np.float32([3.0, -2.0, 1.0])).astype(np.float32)
        T = icp_ref.similarity(icp_ref.rotation(AXIS, 4.0), (3.02, -2.01, 0.98), 1.01)
        s = _cube(Q, 32 + Q % 7)
        nrm = np.random.default_rng(33).standard_normal((N_TARGETS, 3)).astype(np.float32) * 3.0
        nrm[::97] = 0.0
        nrm[5::101, 1] = np.nan
        nrm[7::211, 0] = np.inf
        tt, ss = _dev(t), _dev(s)
        grid = ops.nn_grid(tt, *_box_grid(t, (14, 14, 14)))
        index = ops.nn_query(grid, ops.cloud_transform(ss, T), 0.04 if Q > 1 else INF)[1]
        if Q > 100:
            index[3], index[40], index[77] = N_TARGETS, 2 ** 31 - 1, -7  # a foreign array: no pair, nothing read
        moved = ops.cloud_transform(ss, T).cpu().numpy()
        box_centre = (0.5 * (t.min(0).astype(np.float64) + t.max(0))).tolist()
        _SUMS[Q] = (t, tt, ss, nrm, _dev(nrm), T, index, moved, box_centre)
    return _SUMS[Q]


@pytest.mark.parametrize("pivot", ("box_centre", "origin"))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("Q", (1, 255, 257, 262144 + 5))
def test_icp_accumulate_matches_float64(Q, mode, pivot):
    from copenerf import ops
    t, tt, ss, nrm, tn, T, index, moved, centre = _sums_case(Q)
    c = centre if pivot == "box_centre" else [0.0, 0.0, 0.0]
    got = ops.icp_accumulate(ss, tt, index, T, c, mode, tn if mode else None).cpu().numpy()
    idx = index.cpu().numpy()
    want, mag = icp_ref.sums(moved, t, idx, c, mode, nrm)
    rel = np.abs(got - want) / np.where(mag > 0, mag, 1.0)
    print(f"Q {Q} mode {mode} pivot {pivot}: n {int(want[0])}, left out {int(want[30])}, no pair {int((idx < 0).sum())}, "
          f"max |err| / sum |term| = {rel.max():.3e} (bar {SUMS_BAR:.0e}; Q 2^-53 = {Q * 2.0 ** -53:.1e})")
    assert got.dtype == np.float64 and got.shape == (32,)
    assert got[0] == want[0] and got[30] == want[30]  # the counts are exact
    assert np.all(np.abs(got - want) <= SUMS_BAR * mag)
    assert np.all(got[18 if mode == 0 else 31:] == 0.0) and (mode == 1 or got[30] == 0.0)
    if Q > 1:
        assert 0 < want[0] < Q and (idx == -1).any()
    if Q > 1 and mode == 1:
        assert want[30] > 0


@pytest.mark.parametrize("mode", (0, 1))
def test_icp_accumulate_without_pairs_is_all_zero(mode):
    from copenerf import ops
    t, tt, ss, nrm, tn, T, index, moved, centre = _sums_case(257)
    none = torch.full_like(index, -1)
    assert (ops.icp_accumulate(ss, tt, none, T, centre, mode, tn if mode else None) == 0).all()
    empty = torch.empty(0, 3, device=DEV)
    out = ops.icp_accumulate(empty, tt, torch.empty(0, dtype=torch.int32, device=DEV), T, centre, mode, tn if mode else None)
    assert out.shape == (32,) and (out == 0).all()  # Q = 0
    out = ops.icp_accumulate(ss, empty, index, T, centre, mode, empty if mode else None)
    assert (out == 0).all()  # N = 0: every index is past the targets


def test_two_full_builds_give_the_same_sums_bit_for_bit():
    from copenerf import ops
    t, s = _cube(40000, 41), _cube(30000, 42)
    nrm = np.random.default_rng(43).standard_normal((40000, 3)).astype(np.float32)
    T = icp_ref.similarity(icp_ref.rotation(AXIS, 3.0), (0.01, -0.02, 0.015))
    tt, ss, tn = _dev(t), _dev(s), _dev(nrm)
    origin, cell, dims = _box_grid(t, (6, 6, 6))  # ~185 targets per cell: the within-cell order is the atomics'
    runs = []
    for _ in range(2):
        grid = ops.nn_grid(tt, origin, cell, dims)
        records = ops.nn_grid(ops.cloud_transform(ss, T), origin, cell, dims).sorted
        index = ops.nn_query(grid, records, 0.03, records=True)[1]
        runs.append((grid.sorted.clone(), index, [ops.icp_accumulate(ss, tt, index, T, (0.5, 0.5, 0.5), m, tn) for m in (0, 1)]))
    (rec_a, idx_a, sums_a), (rec_b, idx_b, sums_b) = runs
    print(f"records differ between the builds at {int((rec_a != rec_b).any(1).sum())} of {len(t)} slots")
    assert torch.equal(idx_a, idx_b)
    for a, b in zip(sums_a, sums_b):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and a[0] > 0


# ---- end to end -----------------------------------------------------------------------------------------------
T_BAR = 2e-6  # 32 x 2^-24 x 1.2: a few ulp of a coordinate below 1.2, not amplified by a well-conditioned fit
_E2E = {}


def _motion(scale=1.0):
    return icp_ref.similarity(icp_ref.rotation(AXIS, MOTION["degrees"]), MOTION["t"], scale)


def _identical(case):
    """(source, target, normals, T_true, the float64 reference's result) of the identical-clouds case."""
    if ("same", case) not in _E2E:
        tgt, nrm = icp_ref.bumpy_ellipsoid(4000, 11)
        tgt = tgt.astype(np.float32)
        assert np.abs(tgt).max() < 1.2
        T = _motion(1.03 if case == "scale" else 1.0)
        src = icp_ref.apply(np.linalg.inv(T), tgt).astype(np.float32)
        mode = "plane" if case == "plane" else "point"
        ref = icp_ref.register(src, tgt, 0.3, mode=mode, with_scale=case == "scale", target_normals=nrm.astype(np.float32))
        _E2E[("same", case)] = (src, tgt, nrm.astype(np.float32), T, ref)
    return _E2E[("same", case)]


@pytest.mark.parametrize("case", ("point", "scale", "plane"))
def test_icp_register_identical_clouds(case):
    from copenerf import metrics
    src, tgt, nrm, T, ref = _identical(case)
    kw = dict(mode="plane", target_normals=_dev(nrm)) if case == "plane" else dict(with_scale=case == "scale")
    res = metrics.icp_register(_dev(src), _dev(tgt), max_corr_dist=0.3, **kw)
    err, ref_err = np.abs(res.transform - T).max(), np.abs(ref["transform"] - T).max()
    print(f"{case}: max |T - T_true| = {err:.3e} (bar {T_BAR:.0e}; float64 reference {ref_err:.3e}), iterations "
          f"{res.iterations} (reference {ref['iterations']}), fitness {res.fitness}, rmse {res.inlier_rmse:.3e} "
          f"(reference {ref['inlier_rmse']:.3e})")
    assert res.transform.dtype == np.float64 and res.transform.shape == (4, 4)
    assert err <= T_BAR
    assert res.converged and ref["converged"] and res.fitness == 1.0
    assert abs(res.iterations - ref["iterations"]) <= 2
    assert len(res.history) == res.iterations + 1 and res.history[-1] == (res.fitness, res.inlier_rmse)


def _different(mode):
    if ("diff", mode) not in _E2E:
        tgt, nrm = icp_ref.bumpy_ellipsoid(20000, 12)
        srcpts, _ = icp_ref.bumpy_ellipsoid(3000, 13)
        tgt = tgt.astype(np.float32)
        T = _motion()
        src = icp_ref.apply(np.linalg.inv(T), srcpts).astype(np.float32)
        ref = icp_ref.register(src, tgt, 0.3, mode=mode, target_normals=nrm.astype(np.float32))
        _E2E[("diff", mode)] = (src, tgt, nrm.astype(np.float32), T, ref)
    return _E2E[("diff", mode)]


@pytest.mark.parametrize("mode", ("point", "plane"))
def test_icp_register_different_samples(mode):
    from copenerf import metrics
    src, tgt, nrm, T, ref = _different(mode)
    res = metrics.icp_register(_dev(src), _dev(tgt), max_corr_dist=0.3, mode=mode,
                               target_normals=_dev(nrm) if mode == "plane" else None)
    err, ref_err = np.abs(res.transform - T).max(), np.abs(ref["transform"] - T).max()
    print(f"{mode}: rmse {res.inlier_rmse:.6e} (reference {ref['inlier_rmse']:.6e}), max |T - T_true| = {err:.3e} "
          f"(reference {ref_err:.3e}), iterations {res.iterations} (reference {ref['iterations']})")
    assert res.converged and res.fitness == 1.0
    assert res.inlier_rmse <= ref["inlier_rmse"] * (1 + 1e-3)
    if mode == "plane":
        assert err <= 1.25 * ref_err + T_BAR


def test_icp_register_stages_stride_init_and_errors():
    from copenerf import metrics
    src, tgt, nrm, T, _ = _different("plane")
    s, t, n = _dev(src), _dev(tgt), _dev(nrm)
    stages = [dict(max_corr_dist=0.3, stride=4, max_iters=5), dict(max_corr_dist=0.1, stride=2),
              dict(max_corr_dist=0.03, mode="plane")]
    res = metrics.icp_register_stages(s, t, stages, target_normals=n)
    one = metrics.icp_register(s, t, max_corr_dist=0.03, mode="plane", target_normals=n, init=res.transform, max_iters=1)
    print(f"stages: {res.iterations} iterations, rmse {res.inlier_rmse:.3e}, max |T - T_true| = {np.abs(res.transform - T).max():.3e}")
    assert res.converged and np.abs(res.transform - T).max() < 1e-3 and len(res.history) == res.iterations + 3
    # started at the answer, the first measurement is the stages' last
    assert one.history[0] == res.history[-1]
    with pytest.raises(ValueError, match="may set"):
        metrics.icp_register_stages(s, t, [dict(max_corr_dist=0.1, tol=1e-3)])
    with pytest.raises(ValueError, match="correspondences"):
        metrics.icp_register(s, t + 100.0, max_corr_dist=0.01)  # nothing within reach
    with pytest.raises(ValueError, match="target_normals"):
        metrics.icp_register(s, t, max_corr_dist=0.1, mode="plane")
