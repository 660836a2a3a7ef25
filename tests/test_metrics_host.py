"""The evaluation metrics without a device: the float64 restatement (tests/metrics_ref.py) against the
reference's own numbers (tests/golden/metrics.npz, made by tests/golden/make_metrics_golden.py), the host
side of copenerf.metrics (pose metrics, the median rule, results.txt, LPIPS, refusals)."""
import numpy as np
import pytest
import torch

import metrics_ref as M
from helpers import fixture_arrays


@pytest.fixture(scope="module")
def fx():
    return fixture_arrays("metrics")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_equals_the_reference_on_images(fx, tag):
    pred, gt = fx[f"img_{tag}_pred"], fx[f"img_{tag}_gt"]
    out, smap = M.image_metrics(pred, gt)
    assert np.abs(smap - fx[f"img_{tag}_ssim_map"]).max() <= 1e-12
    assert abs(smap.mean() - fx[f"img_{tag}_ssim"]) <= 1e-12
    assert np.abs(smap.mean(axis=(1, 2, 3)) - fx[f"img_{tag}_ssim_per_image"]).max() <= 1e-12
    assert np.abs(out[..., 1].mean(1) - fx[f"img_{tag}_ssim_unbatched"]).max() <= 1e-12
    # batched: one PSNR per image over all channels; unbatched (eval.py:204): one per channel
    assert np.abs(M.psnr_of_mse(out[..., 0].mean(1)) - fx[f"img_{tag}_psnr"][:, 0]).max() <= 1e-12
    assert np.abs(M.psnr_of_mse(out[..., 0]) - fx[f"img_{tag}_psnr_unbatched"][..., 0]).max() <= 1e-12
    ev = M.eval_image_metrics(np.moveaxis(pred, 1, -1), np.moveaxis(gt, 1, -1))
    assert abs(ev["PSNR"] - fx[f"img_{tag}_psnr_unbatched"].mean()) <= 1e-12
    assert abs(ev["SSIM"] - fx[f"img_{tag}_ssim_unbatched"].mean()) <= 1e-12


def test_window_taps_are_the_references():
    from copenerf import ops
    taps = ops.ssim_taps()
    assert taps.dtype == torch.float32 and np.array_equal(taps.numpy(), M.window_taps())
    assert abs(float(taps.double().sum()) - 1.0) < 1e-6


@pytest.mark.parametrize("clamp", [False, True])
def test_restatement_equals_the_reference_on_depth(fx, clamp):
    got = M.depth_errors(fx["depth_gt"], fx["depth_pred"], clamp=clamp)
    want = fx["depth_errors_clamp" if clamp else "depth_errors_noclamp"]
    assert np.abs(np.array(got[:7], dtype=np.float64) - want).max() <= 1e-12
    assert got[7] == 12 * 16 - 5 - 4 - 1
    # the clamp changes something in this fixture, and the out-of-range pixels are really there
    assert np.abs(fx["depth_errors_clamp"] - fx["depth_errors_noclamp"]).max() > 1e-3


def test_pose_metrics_against_the_reference(fx):
    from copenerf import metrics
    for fn in (M.pose_error, metrics.compute_pose_error):
        aligned, rpe_trans, rpe_rot, ate = fn(fx["pose_pred"], fx["pose_gt"])
        # the reference aligns in float32 (align_traj.py:37-39), so float64 cannot equal it to 1e-12.  Measured
        # on the CPU, restatement and copenerf.metrics alike: aligned 4.07e-7 (max abs), rpe_trans 8.02e-6 (value
        # 6.06, in units of 1/100), rpe_rot 2.77e-5 degrees (value 1.16), ate 5.60e-8 (value 0.0385); the bars
        # are 10 x those.
        assert np.abs(np.asarray(aligned) - fx["pose_aligned"]).max() <= 4.07e-6
        assert abs(rpe_trans - fx["pose_rpe_trans"]) <= 8.02e-5
        assert abs(rpe_rot - fx["pose_rpe_rot"]) <= 2.77e-4
        assert abs(ate - fx["pose_ate"]) <= 5.60e-7
    a, b = M.pose_error(fx["pose_pred"], fx["pose_gt"]), metrics.compute_pose_error(fx["pose_pred"], fx["pose_gt"])
    assert np.abs(a[0] - b[0]).max() <= 1e-12 and all(abs(x - y) <= 1e-12 for x, y in zip(a[1:], b[1:]))


def test_compute_pose_error_recovers_a_planted_sim3():
    from copenerf import metrics
    gt = M.trajectory(12, 3)
    R = M.rodrigues([0.9, 0.2, -1.4])
    pred = M.apply_sim3(gt, 0.37, R, np.array([1.0, -2.0, 0.5]))
    aligned, rpe_trans, rpe_rot, ate = metrics.compute_pose_error(torch.from_numpy(pred), torch.from_numpy(gt))
    assert torch.is_tensor(aligned) and aligned.dtype == torch.float64 and aligned.shape == (12, 4, 4)
    assert ate < 1e-9 and rpe_trans < 1e-7 and rpe_rot < 1e-5
    assert np.abs(aligned.numpy() - gt).max() < 1e-9
    # numpy in, numpy out; [N, 3, 4] poses align too
    al2 = metrics.align_ate_c2b_use_a2b(pred[:, :3], gt[:, :3])
    assert isinstance(al2, np.ndarray) and np.abs(al2 - gt).max() < 1e-9
    s, Rr, t = metrics.umeyama(gt[:, :3, 3], pred[:, :3, 3])
    assert abs(s - 1 / 0.37) < 1e-9 and np.abs(Rr - R.T).max() < 1e-9


def test_umeyama_reflection_branch():
    from copenerf import metrics
    rng = np.random.default_rng(0)
    data = rng.standard_normal((12, 3))
    model = data * np.array([1.0, 1.0, -1.0])  # a mirror image: the best orthogonal map is a reflection
    U, _, Vt = np.linalg.svd((model - model.mean(0)).T @ (data - data.mean(0)))
    assert np.linalg.det(U) * np.linalg.det(Vt) < 0  # the branch is taken
    for fn in (metrics.umeyama, M.umeyama):
        s, R, t = fn(model, data)
        assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
        assert 0 < s < 1  # a proper rotation cannot reach the mirror image: the fit shrinks
    a, b = metrics.umeyama(model, data), M.umeyama(model, data)
    assert abs(a[0] - b[0]) < 1e-12 and np.abs(a[1] - b[1]).max() < 1e-12 and np.abs(a[2] - b[2]).max() < 1e-12


def test_ate_and_rpe_of_known_offsets():
    from copenerf import metrics
    gt = M.trajectory(6, 1)
    pred = gt.copy()
    pred[:, :3, 3] += np.array([0.3, 0.0, 0.4])  # a constant offset: ATE 0.5
    assert abs(metrics.compute_ATE(gt, pred) - 0.5) < 1e-12
    tr, ro = metrics.compute_rpe(gt, gt)
    assert tr < 1e-15 and ro < 1e-7
    straight = np.tile(np.eye(4), (6, 1, 1))
    straight[:, 2, 3] = np.arange(6)
    turned = straight.copy()
    for i in range(6):  # frame i turned by 0.1 i about z: each relative pose is off by a turn of 0.1 rad
        turned[i, :3, :3] = M.rodrigues([0, 0, 0.1 * i])
    tr, ro = metrics.compute_rpe(straight, turned)
    assert abs(ro - 0.1) < 1e-9 and tr < 1e-15


@pytest.mark.parametrize("n_valid", [1, 2, 7, 8])
def test_median_ratio_follows_numpys_rule(n_valid):
    from copenerf import metrics
    rng = np.random.default_rng(n_valid)
    gt = np.zeros((2, 3, 5), dtype=np.float32)
    pred = rng.uniform(0.5, 2.0, (2, 3, 5)).astype(np.float32)
    for n in range(2):
        idx = rng.permutation(15)[:n_valid]
        gt[n].reshape(-1)[idx] = rng.uniform(1.0, 9.0, n_valid).astype(np.float32)
    gt[1].reshape(-1)[rng.permutation(15)[0]] = 200.0  # out of range: ignored (or replaces a valid one)
    got = metrics.median_ratio(torch.from_numpy(gt), torch.from_numpy(pred), 0.1, 80.0).numpy()
    for n in range(2):
        v = (gt[n] >= 0.1) & (gt[n] <= 80.0)
        want = np.median(gt[n][v]) / np.median(pred[n][v])
        assert want.dtype == np.float32 and got[n] == want, (n, got[n], want)
    # half-size prediction: the source pixel is (y Hp // Hg, x Wp // Wg); no valid pixel: NaN
    gt4 = rng.uniform(1.0, 9.0, (1, 4, 6)).astype(np.float32)
    p2 = rng.uniform(0.5, 2.0, (1, 2, 3)).astype(np.float32)
    got = metrics.median_ratio(torch.from_numpy(gt4), torch.from_numpy(p2), 0.1, 80.0).numpy()
    assert got[0] == np.median(gt4[0]) / np.median(np.repeat(np.repeat(p2[0], 2, 0), 2, 1))
    assert np.array_equal(M.nearest(p2[0], 4, 6), np.repeat(np.repeat(p2[0], 2, 0), 2, 1))
    assert np.isnan(metrics.median_ratio(torch.zeros(1, 3, 5), torch.ones(1, 3, 5), 0.1, 80.0).numpy()).all()


def test_results_txt_format_and_key_order(tmp_path):
    from copenerf import metrics
    result = {"PSNR": 23.4567891234, "SSIM": 0.81, "LPIPS": 0.25, "rpe_trans": 0.12, "rpe_rot": np.float64(0.034),
              "ate": 0.0021, "abs_rel": 0.1, "sq_rel": 0.02, "rmse": 0.5, "rmse_log": 0.2, "a1": 0.9, "a2": 0.95, "a3": 1.0}
    p = tmp_path / "results.txt"
    metrics.write_results(p, result)
    lines = p.read_text().splitlines()
    assert [l.split(": ")[0] for l in lines] == ["PSNR", "SSIM", "LPIPS", "rpe_trans", "rpe_rot", "ate", "abs_rel",
                                                 "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"]
    assert lines[0] == "PSNR: 23.4567891234" and p.read_text().endswith("a3: 1.0\n")
    assert [float(l.split(": ")[1]) for l in lines] == [float(v) for v in result.values()]
    assert metrics.DEPTH_KEYS == ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


def test_lpips_key_only_with_a_function(monkeypatch):
    from copenerf import metrics, ops
    calls = []

    def fake_kernel(pred, gt, want_map=False):  # the device pass is not what this test is about
        out = torch.stack([((pred - gt) ** 2).mean((2, 3)), torch.ones(pred.shape[:2])], -1)
        return out, None

    monkeypatch.setattr(ops, "image_metrics", fake_kernel)
    imgs = [torch.rand(5, 7, 3) for _ in range(3)]
    gts = [torch.rand(5, 7, 3) for _ in range(3)]
    res = metrics.image_metrics(imgs, gts)
    assert list(res) == ["PSNR", "SSIM"]

    def stub(a, b):
        calls.append((tuple(a.shape), tuple(b.shape)))
        return torch.tensor([[0.25]]) * len(calls)

    res = metrics.image_metrics(imgs, gts, lpips_fn=stub)
    assert list(res) == ["PSNR", "SSIM", "LPIPS"] and calls == [((3, 5, 7), (3, 5, 7))] * 3
    assert abs(res["LPIPS"] - 0.5) < 1e-12 and res["SSIM"] == 1.0
    want = np.mean([M.psnr_of_mse(M.plane_mse(np.moveaxis(a.numpy(), -1, 0), np.moveaxis(b.numpy(), -1, 0))).mean()
                    for a, b in zip(imgs, gts)])
    assert abs(res["PSNR"] - want) < 1e-4


def test_refusals():
    from copenerf import metrics, ops
    a, b = torch.rand(1, 3, 12, 12), torch.rand(1, 3, 12, 12)
    with pytest.raises(NotImplementedError):
        metrics.ssim(a, b, window_size=7)
    for fn in (metrics.ssim, metrics.psnr, ops.image_metrics):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.image_metrics([a[0].permute(1, 2, 0)], [b[0].permute(1, 2, 0)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.depth_errors(torch.rand(1, 4, 4), torch.rand(1, 4, 4), torch.ones(1), 0.1, 80.0, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.depth_metrics([torch.rand(4, 4) + 1], [torch.rand(4, 4) + 1])
    assert metrics.depth_metrics([-1, -1], [torch.rand(4, 4), torch.rand(4, 4)]) is None
    assert metrics.depth_metrics([torch.tensor(-1), None], [torch.rand(4, 4)] * 2) is None
    with pytest.raises(ValueError):
        metrics.psnr(torch.rand(4, 4), torch.rand(4, 4))


def test_exports():
    import copenerf
    import model
    from copenerf import metrics
    from copenerf.trainer import Trainer
    assert copenerf.evaluate is metrics.evaluate is model.evaluate
    assert copenerf.compute_pose_error is metrics.compute_pose_error is model.compute_pose_error
    assert callable(Trainer.compute_depth_errors)
