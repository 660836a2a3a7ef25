"""The host side of mesh depth rendering and culling, no device needed: mesh.camera_projection inverts
rays.world_rays over inference.arange_pixels' grid, the float64 reference rasteriser (tests/mesh_raster_ref.py)
agrees with an analytic sphere, its undecided share and the fp32 restatement's depth error on the GPU tests' scenes
are what the GPU tests assume, and tools/evaluate_mesh.py refuses --cull-views without --cull-resolution.

Measured here on the CPU: the fp32 restatement's worst relative depth error at decided pixels is 1.037e-6 on
scene_thread and 8.19e-7 on scene_group (17.4 and 13.7 x 2^-24); mesh_raster_ref.F32_WORST pins 1.04e-6 and the GPU
tests' bound is EPS_DEPTH = 4 x that = 4.16e-6.  The reference alone leaves out at most 1.7 % (scene_thread) and
0.7 % (scene_group) of a view's covered pixels as undecided, against the cap of 3 %."""
import os
import sys

import numpy as np
import pytest
import torch

import mesh_raster_ref as R
from mesh_eval_ref import icosphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _P(view, h, w, transform=None):
    from copenerf.mesh import camera_projection
    return camera_projection(view["camera_mat"], view["world_mat"], view.get("scale_mat"), (h, w), transform)


def test_camera_projection_round_trips_world_rays():
    """A point o + d v on pixel (x, y)'s ray (world_rays' un-normalised v) projects to (x, y) with c = d, to float64
    rounding, under a non-trivial world and scale matrix.  P itself is fp32, so the comparison uses the float64
    composition rounded the same way: the fp32 P is checked against it to 2^-24."""
    from copenerf import mesh, rays
    from copenerf.inference import arange_pixels
    h, w = 23, 37
    view = R.make_view((1.1, -0.7, 0.6), (0.1, 0.05, -0.1), 31.0, h, w)
    a = 0.4
    S = np.eye(4)
    S[:3, :3] = 1.7 * np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    S[:3, 3] = (0.2, -0.3, 0.1)
    loc, pn32 = arange_pixels(h, w)
    # arange_pixels' normalised grid in float64 (its own is fp32: 1e-6 pixels of rounding)
    pn = torch.stack([2.0 * loc[:, 0].double() / (w - 1) - 1.0, 2.0 * loc[:, 1].double() / (h - 1) - 1.0], -1)
    assert torch.allclose(pn.float(), pn32, rtol=0, atol=2e-7)
    t64 = [torch.from_numpy(m) for m in (view["camera_mat"], view["world_mat"], S)]
    o, dirs, n = rays.world_rays(pn, *t64)
    v = (dirs * n).numpy()
    d = np.random.default_rng(0).uniform(0.3, 4.0, size=(len(v), 1))
    X = o.numpy() + d * v
    P32 = mesh.camera_projection(view["camera_mat"], view["world_mat"], S, (h, w))
    assert P32.dtype == np.float32 and P32.shape == (3, 4)
    # the float64 composition, as camera_projection forms it
    M = view["camera_mat"] @ view["world_mat"] @ S
    P = np.stack([0.5 * (w - 1) * (M[0] + M[2]), 0.5 * (h - 1) * (M[1] + M[2]), M[2]])
    assert np.all(np.abs(P32 - P) <= 2.0 ** -24 * np.abs(P))
    abc = X @ P[:, :3].T + P[:, 3]
    assert np.all(abc[:, 2] > 0)
    assert np.allclose(abc[:, 2], d[:, 0], rtol=1e-12, atol=0)
    assert np.allclose(abc[:, 0] / abc[:, 2], loc[:, 0].numpy(), rtol=0, atol=1e-9)
    assert np.allclose(abc[:, 1] / abc[:, 2], loc[:, 1].numpy(), rtol=0, atol=1e-9)
    # a point behind the camera has c < 0
    back = o.numpy()[:1] - 0.5 * v[:1]
    assert (back @ P[:, :3].T + P[:, 3])[0, 2] < 0
    # scale_mat None is the identity; tensors are taken as arrays are
    assert np.array_equal(mesh.camera_projection(t64[0], t64[1], None, (h, w)),
                          mesh.camera_projection(view["camera_mat"], view["world_mat"], np.eye(4), (h, w)))
    # a transform S on the geometry: P S^-1 sees S X where P sees X
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = 0.5 * S[:3, :3] / 1.7, (1.0, 2.0, -0.5)
    PT = mesh.camera_projection(view["camera_mat"], view["world_mat"], S, (h, w), transform=T).astype(np.float64)
    XT = X @ T[:3, :3].T + T[:3, 3]
    assert np.allclose(XT @ PT[:, :3].T + PT[:, 3], abc, rtol=0, atol=1e-4)
    with pytest.raises(ValueError, match="affine"):
        proj = np.eye(4)
        proj[3] = (0, 0, -1, 0)
        mesh.camera_projection(proj, view["world_mat"], None, (h, w))


def test_reference_rasteriser_matches_analytic_sphere():
    """raster_ref on an icosphere of 5120 triangles inscribed in a sphere of radius 0.5 against the ray-sphere
    depth: away from the silhouette the inscribed surface lies behind the sphere by at most the sagitta of a
    triangle (edge 0.04: 0.5 (1 - cos(0.04)) / cos(incidence) < 1e-3 at incidences below 60 degrees)."""
    from copenerf import rays
    from copenerf.inference import arange_pixels
    h, w, rad = 48, 64, 0.5
    v, f = icosphere(4, rad)
    view = R.three_views(h, w)[0]
    depth, tri, _ = R.raster_ref(v, f, _P(view, h, w), h, w, 1e-4)
    _, pn = arange_pixels(h, w)
    o, dirs, n = rays.world_rays(pn.double(), torch.from_numpy(view["camera_mat"]), torch.from_numpy(view["world_mat"]),
                                 torch.eye(4, dtype=torch.float64))
    o, vv = o.numpy(), (dirs * n).numpy()
    A, B, C = (vv * vv).sum(1), 2 * (o * vv).sum(1), (o * o).sum(1) - rad * rad
    disc = B * B - 4 * A * C
    hit = disc > 0
    d = np.where(hit, (-B - np.sqrt(np.where(hit, disc, 0))) / (2 * A), np.inf)
    X = o + d[:, None] * vv
    cosi = np.where(hit, -(X * vv).sum(1) / (rad * np.sqrt(A)), 0)  # the ray against the sphere's normal at the hit
    sel = (cosi > 0.5).reshape(h, w)
    assert sel.sum() > 300
    got, want = depth[sel], d.reshape(h, w)[sel]
    assert np.all(tri[sel] >= 0)
    assert np.all(got >= want - 1e-12) and np.all(got - want < 1e-3)
    assert np.all(tri[~hit.reshape(h, w)] == -1)  # the inscribed mesh never reaches outside the sphere


def _measure(scene):
    v, f, views, h, w = scene[:5]
    worst, left = 0.0, 0.0
    for view in views:
        P = _P(view, h, w)
        ref = R.raster_ref(v, f, P, h, w, 1e-4)
        d32, t32 = R.raster_f32(v, f, P, h, w, 1e-4)
        err, lo = R.compare_view(d32, t32, ref)  # (asserts ids and coverage at decided pixels, and the 3 % cap)
        worst, left = max(worst, err), max(left, lo)
    return worst, left


def test_fp32_restatement_error_and_undecided_share():
    """What the GPU tests' depth bound is made of (the module docstring has the figures)."""
    for name, scene in (("scene_thread", R.scene_thread()), ("scene_group", R.scene_group())):
        worst, left = _measure(scene)
        print(name, "worst relative depth error %.3e = %.1f x 2^-24, undecided share %.4f" % (worst, worst * 2 ** 24, left))
        assert 0 < worst <= R.F32_WORST
        assert left <= 0.03
    assert R.EPS_DEPTH == 4 * R.F32_WORST
    v, f, views, h, w, straddler = R.scene_group()
    ref = R.raster_ref(v, f, _P(views[0], h, w), h, w, 1e-4)
    assert not np.any(ref[1] == straddler)                         # skipped, not clipped
    assert np.mean((ref[1] >= 0) & (ref[1] < 4)) > 0.5             # the four large triangles fill most of the image


def test_visibility_reference_on_the_cull_scene():
    """The reference alone on the GPU test's visibility scene: the undecided share is under the cap of 3 %, both
    with the reference's own depth maps and as a frustum test, and the scene has vertices of every kind."""
    v, f, views, h, w = R.scene_cull()
    P = np.stack([_P(view, h, w) for view in views])
    depth = np.stack([R.raster_ref(v, f, p, h, w, 1e-4)[0] for p in P]).astype(np.float32)
    for dm in (depth, None):
        count, decided, stable = R.visibility_ref(v, P, h, w, dm, tol_abs=R.CULL_TOL_ABS, near=1e-4)
        print("undecided share %.4f, unstable %d" % (1.0 - decided.mean(), (~stable).sum()))
        assert 1.0 - decided.mean() <= 0.03
        assert np.all(stable | ~decided)
        assert count.min() == 0 and count.max() == len(views)
    count, _, stable = R.visibility_ref(v, P, h, w, depth, tol_abs=R.CULL_TOL_ABS, near=1e-4)
    assert stable.all()  # (with the reference's own depth maps; the GPU test asserts it for the device's)
    assert 0 < (count >= 1).sum() < len(v) and 0 < (count >= 2).sum() < (count >= 1).sum()


def test_cli_rejects_cull_views_without_resolution(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import evaluate_mesh
    base = ["mesh.ply", "gt.ply", "--threshold", "0.1", "--samples", "10"]
    for extra, msg in ((["--cull-views", "K.npy", "W.npy"], "go together"),
                       (["--cull-resolution", "48", "64"], "go together"),
                       (["--cull-views", "K.npy", "--cull-resolution", "48", "64"], "K.npy W2C.npy"),
                       (["--depths-out", "d"], "need --cull-views"), (["--cull-gt"], "need --cull-views")):
        with pytest.raises(SystemExit) as e:
            evaluate_mesh.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err
