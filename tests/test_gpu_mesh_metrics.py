"""cn_cloud_stats, metrics.mesh_geometry_metrics and tools/evaluate_mesh.py against the float64 restatement
(tests/mesh_eval_ref.py).  Counts are exact; the distance sum is within 1e-12 relative of the float64 sum of the same
fp32 distances and bitwise repeatable; the metric means are within 1e-6 relative of the means of float64
brute-force distances between the same samples (the fp32 distance arithmetic is within 8 x 2^-24 = 4.8e-7).  The
thresholds other than 0.1 and 0.01 (0.0605, and 0.0615 as max_dist) lie 5e-5 relative or more away from every
reference distance, a hundred times the fp32 bound, so the counts are decided."""
import os
import sys

import numpy as np
import pytest
import torch

from mesh_eval_ref import brute_nn, cloud_stats_ref, geometry_ref, icosphere

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("accuracy", "completeness", "chamfer", "precision", "recall", "fscore", "n_pred", "n_gt", "n_pred_far",
        "n_gt_far", "area")
MEANS = ("accuracy", "completeness", "chamfer")
COUNTS = ("n_pred", "n_gt", "n_pred_far", "n_gt_far")
S, SEED = 16000, 5


@pytest.mark.parametrize("Q", [1, 1000, 1_500_000])  # one thread, one block's tail, six strides of 1024 blocks
@pytest.mark.parametrize("crop", [False, True])
def test_cloud_stats_counts_and_sum(Q, crop):
    from copenerf import ops
    rng = np.random.default_rng(Q)
    max_dist, tau = 0.75, 0.3
    d = rng.random(Q, dtype=np.float32)
    d[d >= max_dist] = max_dist  # as cn_nn_query writes them
    p = rng.random((Q, 3), dtype=np.float32)
    box = ((0.1, 0.0, 0.2), (0.9, 1.0, 0.7)) if crop else (None, None)
    want = cloud_stats_ref(d, tau, max_dist, p, *box)
    td, tp = torch.from_numpy(d).to(DEV), torch.from_numpy(p).to(DEV)
    out = ops.cloud_stats(td, tau, max_dist, tp if crop else None, *box)
    again = ops.cloud_stats(td, tau, max_dist, tp if crop else None, *box)
    assert torch.equal(out, again)  # bitwise
    got = out.tolist()
    assert [got[0], got[1], got[3]] == [want[0], want[1], want[3]]
    assert abs(got[2] - want[2]) <= 1e-12 * want[2]
    if Q > 1:
        assert 0 < got[3] < got[1] < got[0] <= Q and (crop or got[0] == Q)
    inf = ops.cloud_stats(td, tau).tolist()  # no max_dist: every distance counts
    assert inf[:2] == [Q, Q] and abs(inf[2] - float(d.astype(np.float64).sum())) <= 1e-12 * inf[2]


def _gt_cloud(n=6000, radius=1.05):
    """A Fibonacci lattice on the sphere: an even cloud without holes."""
    k = np.arange(n) + 0.5
    z = 1 - 2 * k / n
    phi = np.pi * (1 + 5 ** 0.5) * k
    r = np.sqrt(1 - z * z)
    return (radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)).astype(np.float32)


_SHARED = {}


def _shared():
    """The mesh, the cloud, the device sampler's samples for (S, SEED) and the float64 brute-force distances
    between the two clouds, computed once."""
    if not _SHARED:
        from copenerf import ops
        v, f = icosphere(3)
        gt = _gt_cloud()
        tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
        handle, area = ops.mesh_area(tv, tf)
        samples = ops.mesh_sample(handle, S, torch.tensor([SEED, 0], dtype=torch.uint64, device=DEV))[0].cpu().numpy()
        _SHARED.update(v=v, f=f, gt=gt, tv=tv, tf=tf, tgt=torch.from_numpy(gt).to(DEV), samples=samples,
                       area=area.item(), dists=(brute_nn(samples, gt)[0], brute_nn(gt, samples)[0]))
    return _SHARED


def _compare(got, want, rel=1e-6):
    assert tuple(got) == KEYS
    for k in COUNTS:
        assert got[k] == want[k], k
    for k in MEANS:
        assert got[k] == pytest.approx(want[k], rel=rel), k
    for k in ("precision", "recall", "fscore"):
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), k


def test_mesh_geometry_metrics_sphere_against_shell():
    from copenerf import metrics
    s = _shared()
    for tau in (0.1, 0.01, 0.0605):
        got = metrics.mesh_geometry_metrics(s["tv"], s["tf"], s["tgt"], threshold=tau, n_samples=S, seed=SEED)
        want = geometry_ref(s["samples"], s["gt"], tau, area=s["area"], dists=s["dists"])
        print(tau, got)
        _compare(got, want)
        assert got["area"] == s["area"] and got["n_pred"] == S and got["n_gt"] == len(s["gt"])
        if tau == 0.1:
            assert got["precision"] == 1.0 and got["recall"] == 1.0 and got["fscore"] == 1.0
        if tau == 0.01:
            assert got["precision"] == 0.0 and got["recall"] == 0.0 and got["fscore"] == 0.0
        if tau == 0.0605:  # between the nearest and the farthest pair: a real share on both sides
            assert 0 < got["precision"] < 1 and 0 < got["recall"] < 1
    assert 0.05 < got["accuracy"] < 0.08 and 0.05 < got["completeness"] < 0.08
    assert got["area"] == pytest.approx(4 * np.pi, rel=0.01)


def test_mesh_geometry_metrics_max_dist_crop_and_density():
    from copenerf import metrics
    s = _shared()
    # the upper half only, and a max_dist that leaves part of both clouds out of the means
    box = ((-2.0, -2.0, 0.0), (2.0, 2.0, 2.0))
    got = metrics.mesh_geometry_metrics(s["tv"], s["tf"], s["tgt"], threshold=0.0605, max_dist=0.0615, n_samples=S,
                                        seed=SEED, crop_min=box[0], crop_max=box[1])
    want = geometry_ref(s["samples"], s["gt"], 0.0605, 0.0615, box[0], box[1], area=s["area"], dists=s["dists"])
    # (no float64 distance within the fp32 bound of max_dist or the threshold: the counts are decided)
    for d in s["dists"]:
        assert np.all(np.abs(d - 0.0615) > 1e-6 * d) and np.all(np.abs(d - 0.0605) > 1e-6 * d)
    _compare(got, want)
    assert 0 < got["n_pred_far"] < got["n_pred"] < S and 0 < got["n_gt_far"] < got["n_gt"] < len(s["gt"])
    dens = metrics.mesh_geometry_metrics(s["tv"], s["tf"], s["tgt"], threshold=0.1, density=100.0, seed=SEED)
    assert dens["n_pred"] == int(np.ceil(100.0 * s["area"]))
    with pytest.raises(ValueError, match="zero area"):
        metrics.mesh_geometry_metrics(s["tv"], torch.zeros(2, 3, dtype=torch.int32, device=DEV), s["tgt"], threshold=0.1,
                                      n_samples=10)
    with pytest.raises(ValueError, match="without triangles"):
        metrics.mesh_geometry_metrics(s["tv"], torch.zeros(0, 3, dtype=torch.int32, device=DEV), s["tgt"], threshold=0.1,
                                      n_samples=10)


def _sim3(scale=2.0):
    a, b = 0.7, -0.4
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = scale * (Rz @ Rx), (0.3, -1.0, 2.0)
    return M


def test_mesh_geometry_metrics_transform():
    """Scale 2, a rotation and a translation on the mesh, the cloud transformed alike: distances double, counts
    and shares stay.  The transformed vertices round in fp32 (2^-24 relative of coordinates up to 4), which
    moves the cdf by as much relative to the area: of 16000 samples a few may fall in the neighbouring triangle
    and move by up to an edge (0.14), their distance by up to 0.02 -- 1e-5 of the mean; 1e-4 bounds it."""
    from copenerf import metrics
    s = _shared()
    M = _sim3()
    gt2 = (s["gt"].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    base = metrics.mesh_geometry_metrics(s["tv"], s["tf"], s["tgt"], threshold=0.1, n_samples=S, seed=SEED)
    for T in (M, torch.from_numpy(M)):
        got = metrics.mesh_geometry_metrics(s["tv"], s["tf"], torch.from_numpy(gt2).to(DEV), threshold=0.2, n_samples=S,
                                            seed=SEED, transform=T)
        for k in MEANS:
            assert got[k] / 2 == pytest.approx(base[k], rel=1e-4), k
        assert got["area"] / 4 == pytest.approx(base["area"], rel=1e-6)
        for k in COUNTS + ("precision", "recall", "fscore"):
            assert got[k] == base[k], k


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_mesh
    return evaluate_mesh


def _read_results(path):
    return {k: float(v) for k, v in (line.split(": ") for line in open(path).read().splitlines())}


def test_evaluate_mesh_tool(tmp_path, capsys):
    from copenerf import metrics
    from copenerf.mesh import write_ply
    s = _shared()
    mesh, cloud, out = str(tmp_path / "mesh.ply"), str(tmp_path / "gt.ply"), str(tmp_path / "results.txt")
    write_ply(mesh, s["v"], s["f"])
    write_ply(cloud, s["gt"], np.zeros((0, 3), dtype=np.int32))
    res = _tool().main([mesh, cloud, "--threshold", "0.0605", "--samples", str(S), "--seed", str(SEED), "--out", out])
    want = metrics.mesh_geometry_metrics(s["tv"], s["tf"], s["tgt"], threshold=0.0605, n_samples=S, seed=SEED)
    assert res == want and list(_read_results(out)) == list(KEYS)
    assert _read_results(out) == {k: float(v) for k, v in want.items()}
    assert capsys.readouterr().out.splitlines() == open(out).read().splitlines()
    want = metrics.mesh_geometry_metrics(s["tv"], s["tf"], s["tgt"], threshold=0.1, n_samples=S, seed=SEED)
    # a reconstruction in its own gauge: the mesh and the predicted camera centres are the ground truth's pulled
    # back through a Sim(3); --align-poses finds it from the two trajectories and recovers the metrics
    M = _sim3(scale=0.5)
    Minv = np.linalg.inv(M)
    rng = np.random.default_rng(0)
    gt_poses = np.tile(np.eye(4), (12, 1, 1))
    gt_poses[:, :3, 3] = rng.standard_normal((12, 3))
    pred_poses = gt_poses.copy()
    pred_poses[:, :3, 3] = gt_poses[:, :3, 3] @ Minv[:3, :3].T + Minv[:3, 3]
    mesh2 = str(tmp_path / "mesh_gauge.ply")
    write_ply(mesh2, (s["v"].astype(np.float64) @ Minv[:3, :3].T + Minv[:3, 3]).astype(np.float32), s["f"])
    np.save(tmp_path / "pred.npy", pred_poses)
    np.save(tmp_path / "gt.npy", gt_poses[:, :3])
    got = _tool().main([mesh2, cloud, "--threshold", "0.1", "--samples", str(S), "--seed", str(SEED), "--align-poses",
                        str(tmp_path / "pred.npy"), str(tmp_path / "gt.npy")])
    for k in KEYS:
        assert got[k] == pytest.approx(want[k], rel=1e-4), k
    np.save(tmp_path / "T.npy", M)
    got = _tool().main([mesh2, cloud, "--threshold", "0.1", "--density", str(S / want["area"] * 0.9999), "--transform",
                        str(tmp_path / "T.npy"), "--crop-min", "-2", "-2", "-2", "--crop-max", "2", "2", "2"])
    assert got["n_gt"] == len(s["gt"]) and got["accuracy"] == pytest.approx(want["accuracy"], rel=1e-2)
