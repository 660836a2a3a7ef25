"""The host side of the ICP registration, no device: metrics.icp_solve_point / icp_solve_plane on sums built in
float64 from exact correspondences (tests/icp_ref.py), their refusals, and tools/evaluate_mesh.py's --icp options."""
import importlib.util
import math
import os

import numpy as np
import pytest

import icp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXIS = (0.3, -0.5, 0.8)


def _tool():
    spec = importlib.util.spec_from_file_location("evaluate_mesh_tool", os.path.join(ROOT, "tools", "evaluate_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cloud(n=200, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)) * (0.9, 0.6, 0.4)


@pytest.mark.parametrize("degrees", (5.0, 40.0))
@pytest.mark.parametrize("scale", (1.0, 1.03))
@pytest.mark.parametrize("pivot", ((0.0, 0.0, 0.0), (8.0, -6.0, 5.0)))
def test_solve_point_recovers_the_transform(degrees, scale, pivot):
    from copenerf import metrics
    T = icp_ref.similarity(icp_ref.rotation(AXIS, degrees), (0.04, -0.03, 0.05), scale)
    p = _cloud()
    q = icp_ref.apply(T, p)
    s, _ = icp_ref.sums(p, q, np.arange(len(p)), pivot, 0)
    got = metrics.icp_solve_point(s, with_scale=scale != 1.0, pivot=pivot)
    err = np.abs(got - T).max()
    print(f"degrees {degrees} scale {scale} pivot {pivot}: max |T - T_true| = {err:.3e}")
    assert err <= 1e-12
    assert np.abs(got - icp_ref.solve_point(s, scale != 1.0, pivot)).max() <= 1e-12


def test_solve_point_reflection_guard():
    """Nearly planar, noisy pairs whose unconstrained optimum is a reflection: the result is still a rotation."""
    from copenerf import metrics
    rng = np.random.default_rng(3)
    p = rng.uniform(-1, 1, (50, 3)) * (1.0, 1.0, 1e-3)
    q = p * (1.0, 1.0, -1.0) + 1e-5 * rng.standard_normal((50, 3))
    s, _ = icp_ref.sums(p, q, np.arange(50), (0, 0, 0), 0)
    R = metrics.icp_solve_point(s)[:3, :3]
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12


@pytest.mark.parametrize("pivot", ((0.0, 0.0, 0.0), (0.2, -0.1, 0.3)))
def test_solve_plane_recovers_a_small_motion(pivot):
    """One Gauss-Newton step from exact pairs q = T p with the normals at q: the step solves the problem linearised
    in the rotation vector w, whose error is the second-order term -- |R(w) x - (x + w x x)| <= |w|^2 |x| / 2 per
    point, |x| the distance from the pivot -- so the recovered transform is within |w|^2 max|x| of the true one
    (and the exact-rotation step cannot do worse than that by more than the same again)."""
    from copenerf import metrics
    degrees = 0.5
    T = icp_ref.similarity(icp_ref.rotation(AXIS, degrees), (0.004, -0.003, 0.005))
    q, n = icp_ref.bumpy_ellipsoid(400, 1)
    p = icp_ref.apply(np.linalg.inv(T), q)
    s, _ = icp_ref.sums(p, q, np.arange(len(p)), pivot, 1, n.astype(np.float32))
    got = metrics.icp_solve_plane(s, pivot)
    w = math.radians(degrees)
    reach = np.linalg.norm(p - np.asarray(pivot), axis=1).max()
    err = np.abs(got - T).max()
    print(f"pivot {pivot}: max |T - T_true| = {err:.3e}, second-order bound {2 * w * w * reach:.3e}")
    assert err <= 2 * w * w * reach
    R = got[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and got[3].tolist() == [0, 0, 0, 1]
    assert np.abs(got - icp_ref.solve_plane(s, pivot)).max() <= 1e-12


def test_solve_plane_is_exact_at_the_solution():
    """With zero residuals the step is the identity to 1e-12 (and a pure translation along well-spread normals is
    recovered exactly: the problem is linear in it)."""
    from copenerf import metrics
    q, n = icp_ref.bumpy_ellipsoid(400, 2)
    s, _ = icp_ref.sums(q, q, np.arange(len(q)), (0.1, 0.2, 0.3), 1, n.astype(np.float32))
    assert np.abs(metrics.icp_solve_plane(s, (0.1, 0.2, 0.3)) - np.eye(4)).max() <= 1e-12
    t = np.array([0.004, -0.003, 0.005])
    planes = q  # targets: the tangent planes at q; the source sits at q - t
    s, _ = icp_ref.sums(planes - t, planes, np.arange(len(q)), (0.1, 0.2, 0.3), 1, n.astype(np.float32))
    assert np.abs(metrics.icp_solve_plane(s, (0.1, 0.2, 0.3)) - icp_ref.similarity(np.eye(3), t)).max() <= 1e-12


def test_solvers_refuse_too_few_pairs_and_rank_deficient_systems():
    from copenerf import metrics
    p = _cloud(2)
    s, _ = icp_ref.sums(p, p, np.arange(2), (0, 0, 0), 0)
    with pytest.raises(ValueError, match="2 correspondences"):
        metrics.icp_solve_point(s)
    with pytest.raises(ValueError, match="0 correspondences"):
        metrics.icp_solve_point(np.zeros(32))
    line = np.outer(np.linspace(-1, 1, 40), (0.5, 0.2, -0.7)) + (0.3, 0.1, 0.2)
    s, _ = icp_ref.sums(line, line + 0.01, np.arange(40), (0, 0, 0), 0)
    with pytest.raises(ValueError, match="rank-deficient"):
        metrics.icp_solve_point(s)
    q, n = icp_ref.bumpy_ellipsoid(5, 4)
    s, _ = icp_ref.sums(q, q, np.arange(5), (0, 0, 0), 1, n.astype(np.float32))
    with pytest.raises(ValueError, match="5 correspondences"):
        metrics.icp_solve_plane(s)
    plane = _cloud(100, 5) * (1, 1, 0)
    normals = np.tile(np.float32([0, 0, 1]), (100, 1))
    s, _ = icp_ref.sums(plane + (0, 0, 0.01), plane, np.arange(100), (0, 0, 0), 1, normals)
    with pytest.raises(ValueError, match="rank-deficient"):
        metrics.icp_solve_plane(s)


def test_register_argument_errors_need_no_device():
    from copenerf import metrics
    with pytest.raises(ValueError, match="with_scale"):
        metrics.icp_register(None, None, max_corr_dist=0.1, mode="plane", with_scale=True)
    with pytest.raises(ValueError, match="mode"):
        metrics.icp_register(None, None, max_corr_dist=0.1, mode="colour")
    with pytest.raises(ValueError, match="max_corr_dist"):
        metrics.icp_register(None, None, max_corr_dist=0.0)
    with pytest.raises(ValueError, match="no stages"):
        metrics.icp_register_stages(None, None, [])


def test_evaluate_mesh_icp_options():
    tool = _tool()
    base = ["m.ply", "g.ply", "--threshold", "0.01", "--samples", "1000"]
    a = tool.parse_args(base)
    assert a.icp is None and tool.icp_kwargs(a) is None
    a = tool.parse_args(base + ["--icp", "0.3", "0.1", "0.03", "--icp-stride", "8", "4", "1", "--icp-samples", "5000",
                                "--icp-max-iters", "30", "--icp-tol", "1e-7", "--icp-scale", "--transform-out", "T.npy"])
    assert tool.icp_kwargs(a) == dict(
        stages=[dict(max_corr_dist=0.3, stride=8), dict(max_corr_dist=0.1, stride=4), dict(max_corr_dist=0.03, stride=1)],
        n_samples=5000, mode="point", with_scale=True, max_iters=30, tol=1e-7)
    assert a.transform_out == "T.npy"
    a = tool.parse_args(base + ["--icp", "0.2", "0.05", "--icp-stride", "2", "--icp-mode", "plane"])
    kw = tool.icp_kwargs(a)
    assert kw["stages"] == [dict(max_corr_dist=0.2, stride=2), dict(max_corr_dist=0.05, stride=2)]
    assert (kw["mode"], kw["with_scale"], kw["n_samples"], kw["max_iters"], kw["tol"]) == ("plane", False, 200000, 50, 1e-6)
    for bad in (["--icp-stride", "2"], ["--icp-scale"], ["--transform-out", "T.npy"], ["--icp-mode", "plane"],
                ["--icp", "0.1", "--icp-stride", "1", "2"], ["--icp", "-0.1"], ["--icp", "0.1", "--icp-stride", "0"],
                ["--icp", "0.1", "--icp-mode", "plane", "--icp-scale"], ["--icp", "0.1", "--icp-samples", "0"]):
        with pytest.raises(SystemExit):
            tool.parse_args(base + bad)
