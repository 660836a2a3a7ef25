"""Pose refinement without a device: the float64 restatement (tests/pose_refine_ref.py) against the
reference's own compute_loss_and_warp_image (tests/golden/pose_refine.npz), and the host logic of
copenerf.pose_refine driven through its loss_fn hook on CPU tensors: pairing and ragged batches, the
learning-rate schedule, the stop rule, the world-pose chain, PoseRetriever.poses_at, the compat names."""
import numpy as np
import pytest
import torch

import pose_refine_ref as R
from helpers import fixture_arrays


def test_restatement_matches_the_reference_function():
    fx = {k: torch.from_numpy(np.asarray(v)) for k, v in fixture_arrays("pose_refine").items()}
    images, depth, K = fx["images"], fx["depth"], fx["K"]
    assert images.dtype == torch.float64 and tuple(images.shape) == (3, 3, 9, 13)
    rel = fx["rel"].clone().requires_grad_(True)
    Kinv = torch.inverse(K)
    pos, wpos = R.loss_and_warp(images[:-1], images[1:], depth[:-1], K, Kinv, rel)
    neg, wneg = R.loss_and_warp(images[1:], images[:-1], depth[1:], K, Kinv, torch.inverse(rel))
    (g,) = torch.autograd.grad((pos + neg) / 2, rel)
    idx = torch.arange(2)
    both = R.pair_loss(images, depth, K, Kinv, rel, idx, idx + 1)
    for name, got, want in (("loss_pos", pos, fx["loss_pos"]), ("loss_neg", neg, fx["loss_neg"]),
                            ("warped_pos", wpos, fx["warped_pos"]), ("warped_neg", wneg, fx["warped_neg"]),
                            ("grad_rel", g, fx["grad_rel"]), ("pair_loss", both, (fx["loss_pos"] + fx["loss_neg"]) / 2)):
        err = float((got.detach() - want).abs().max())
        print(name, "max abs error", err)
        assert err <= 1e-12, (name, err)
    assert float(g.abs().max()) > 1e-3  # non-identity poses: the gradient is not trivially zero


def _const_loss(value=1.0):
    def fn(images, depth, K, Kinv, rel, idx, nxt):
        return rel.sum() * 0 + value
    return fn


def _stacks(N, H=4, W=5):
    return torch.zeros(N, 3, H, W), -torch.ones(N, H, W), torch.eye(3)


@pytest.mark.parametrize("N, sizes", [(2, [1]), (17, [16]), (34, [16, 16, 1])])
def test_pairing_and_ragged_batches(N, sizes):
    from copenerf import pose_refine as P
    seen = []

    def fn(images, depth, K, Kinv, rel, idx, nxt):
        assert rel.shape == (len(idx), 4, 4) and K.shape == (3, 3) and Kinv.shape == (3, 3)
        seen.append((idx.tolist(), nxt.tolist()))
        return (rel ** 2).sum()

    res = P.refine_poses(*_stacks(N), pose_refine_epochs=2, loss_fn=fn)
    assert len(seen) == 2 * len(sizes)
    for e in range(2):
        got = seen[e * len(sizes):(e + 1) * len(sizes)]
        assert [len(i) for i, _ in got] == sizes
        flat_i = [v for i, _ in got for v in i]
        flat_n = [v for _, n in got for v in n]
        assert flat_i == list(range(N - 1))
        assert flat_n == [min(i + 1, N - 1) for i in range(N - 1)]
    assert tuple(res.pred_poses.shape) == (N, 4, 4)
    assert [(len(a), len(b)) for a, b in P.pair_batches(N)] == [(s, s) for s in sizes]


def test_per_frame_intrinsics_follow_the_batch():
    from copenerf import pose_refine as P
    N = 19
    K = torch.eye(3).repeat(N, 1, 1) * torch.arange(1, N + 1).view(N, 1, 1)

    def fn(images, depth, Kb, Kib, rel, idx, nxt):
        assert torch.equal(Kb, K[idx])  # the target frame's K, for both directions
        torch.testing.assert_close(Kib @ Kb, torch.eye(3).expand(len(idx), 3, 3))
        return (rel ** 2).sum()

    images, depth, _ = _stacks(N)
    P.refine_poses(images, depth, K, pose_refine_epochs=1, loss_fn=fn)


@pytest.mark.parametrize("epochs, factor", [(29, 1.0), (30, 0.9), (40, 0.81)])
def test_learning_rate_schedule(epochs, factor):
    from copenerf import pose_refine as P
    k = [0]

    def fn(images, depth, K, Kinv, rel, idx, nxt):
        k[0] += 1
        return rel.sum() * 0 + float(k[0])  # never converges

    res = P.refine_poses(*_stacks(3), pose_refine_lr=1e-3, pose_refine_epochs=epochs, loss_fn=fn)
    assert len(res.losses) == epochs and not res.converged
    assert res.scheduler.get_last_lr()[0] == pytest.approx(1e-3 * factor, rel=1e-12)
    assert isinstance(res.optimizer, torch.optim.Adam)


def test_stop_rule_fires_at_exactly_fifty_equal_losses():
    from copenerf import pose_refine as P
    calls = []
    res = P.refine_poses(*_stacks(5), pose_refine_epochs=200, loss_fn=_const_loss(0.25),
                         on_epoch=lambda e, l, p: calls.append((e, l, tuple(p.shape))))
    assert res.converged and len(res.losses) == 50
    assert calls[-1] == (49, 0.25, (5, 4, 4)) and len(calls) == 50
    short = P.refine_poses(*_stacks(5), pose_refine_epochs=49, loss_fn=_const_loss(0.25))
    assert not short.converged and len(short.losses) == 49
    # 49 equal losses after a different one: the window still holds the first, no stop at epoch 50
    k = [0]

    def fn(images, depth, K, Kinv, rel, idx, nxt):
        k[0] += 1
        return rel.sum() * 0 + (1.0 if k[0] == 1 else 0.25)

    late = P.refine_poses(*_stacks(2), pose_refine_epochs=200, loss_fn=fn)
    assert late.converged and len(late.losses) == 51


def test_epoch_loss_is_the_pair_weighted_mean():
    from copenerf import pose_refine as P
    def fn(images, depth, K, Kinv, rel, idx, nxt):
        return rel.sum() * 0 + float(len(idx))
    res = P.refine_poses(*_stacks(34), pose_refine_epochs=1, loss_fn=fn)
    assert res.losses[0] == pytest.approx((16 * 16 + 16 * 16 + 1) / 33)


def test_world_pose_chain_against_torch_inverse():
    from copenerf import pose_refine as P
    g = torch.Generator().manual_seed(0)
    r = (torch.rand(6, 3, generator=g, dtype=torch.float64) - 0.5) * 0.4
    t = (torch.rand(6, 3, generator=g, dtype=torch.float64) - 0.5)
    rel = R.stacked_poses(r, t, range(6))
    got = P.world_poses(rel)
    want = R.world_poses(rel)
    assert tuple(got.shape) == (7, 4, 4)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got[0], torch.eye(4, dtype=torch.float64))
    torch.testing.assert_close(P.inv3x3(rel[:, :3, :3]), torch.inverse(rel[:, :3, :3]), rtol=1e-12, atol=1e-12)


def test_poses_at_equals_stacked_forward():
    from copenerf import PoseRetriever
    g = torch.Generator().manual_seed(1)
    n = 7
    init = R.stacked_poses((torch.rand(n, 3, generator=g) - 0.5) * 0.2, torch.rand(n, 3, generator=g), range(n)).float()
    for init_c2w in (None, init):
        p = PoseRetriever(n, init_c2w=None if init_c2w is None else init_c2w.clone())
        with torch.no_grad():
            p.r.copy_((torch.rand(n, 3, generator=g) - 0.5) * 0.3)
            p.t.copy_(torch.rand(n, 3, generator=g) - 0.5)
            p.r[2].zero_()  # the zero rotation the refinement starts from
        idx = torch.tensor([3, 0, 2, 6, 2])
        got = p.poses_at(idx)
        want = torch.stack([p(i) for i in idx])
        assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)
        p = p.double()
        w = torch.rand(len(idx), 4, 4, generator=g, dtype=torch.float64)
        ga = torch.autograd.grad((p.poses_at(idx) * w).sum(), [p.r, p.t])
        gb = torch.autograd.grad((torch.stack([p(i) for i in idx]) * w).sum(), [p.r, p.t])
        for a, b in zip(ga, gb):
            assert float((a - b).abs().max()) <= 1e-10


def test_out_of_scope_options_and_cpu_tensors_are_refused():
    from copenerf import pose_refine as P
    images, depth, K = _stacks(3)
    with pytest.raises(NotImplementedError, match="max_interval"):
        P.refine_poses(images, depth, K, max_interval=2, loss_fn=_const_loss())
    with pytest.raises(NotImplementedError, match="max_interval"):
        P.PoseRefineDataset([0, 1], [0, 1], [0, 1], max_interval=3)
    with pytest.raises(ValueError, match="init_c2c"):
        P.refine_poses(images, depth, K, refine_from_scratch=False, loss_fn=_const_loss())
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the fused pass has no CPU path
        P.refine_poses(images, depth, K, pose_refine_epochs=1)
    with pytest.raises(ValueError, match="canonical grid"):
        P.compute_loss_and_warp_image(images[:2], images[1:], depth[:2, None], K.expand(2, 3, 3),
                                      torch.zeros(2, 3, 5, 4), torch.eye(4).expand(2, 4, 4))


def test_init_c2c_starts_the_table():
    from copenerf import pose_refine as P
    init = R.stacked_poses(torch.full((2, 3), 0.1), torch.full((2, 3), 0.2), range(2)).float()
    res = P.refine_poses(*_stacks(3), pose_refine_epochs=1, pose_refine_lr=0.0, refine_from_scratch=False,
                         init_c2c=init, loss_fn=_const_loss())
    torch.testing.assert_close(res.pred_poses, R.world_poses(init))


def test_compat_dataset_grid_and_depth_resize():
    from copenerf import pose_refine as P
    imgs = np.arange(4 * 3 * 2 * 2, dtype=np.float32).reshape(4, 3, 2, 2)
    deps = np.arange(4 * 2 * 2, dtype=np.float32).reshape(4, 2, 2)
    Ks = np.stack([np.eye(3, dtype=np.float32) * (i + 1) for i in range(4)])
    ds = P.PoseRefineDataset(imgs, deps, Ks)
    assert len(ds) == 3
    idx, nxt, im, nim, d, nd, K, nK = ds[2]
    assert (idx, nxt) == (2, 3) and torch.equal(nim, torch.from_numpy(imgs[3])) and torch.equal(d, torch.from_numpy(deps[2]))
    assert np.array_equal(nK, Ks[3])
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=16, shuffle=False)))
    assert batch[0].tolist() == [0, 1, 2] and batch[1].tolist() == [1, 2, 3]
    uv = P.canonical_uv(5, 7)
    assert torch.equal(uv, R.uv_grid(5, 7, torch.float32))
    assert uv[0, 0, 0] == -1 and uv[0, 0, -1] == 1 and uv[1, -1, 0] == 1 and bool((uv[2] == 1).all())
    d = torch.arange(6.0).view(1, 2, 3)
    assert P.resize_depth(d, 2, 3) is d
    up = P.resize_depth(d, 4, 6)
    assert torch.equal(up, torch.nn.functional.interpolate(d[:, None], (4, 6))[:, 0])
