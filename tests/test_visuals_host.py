"""Host side of the visualisation pass (no device): the colour wheel and flow image of the restatement, the
affine identity cn_ray_visuals rests on, the adaptive depth range, and the files render_visdata /
render_train_views write."""
import os

import numpy as np
import pytest

import visuals_ref as V


def test_colour_wheel_rows():
    wheel = V.colour_wheel()
    assert wheel.shape == (55, 3)
    for row, rgb in ((0, (255, 0, 0)), (15, (255, 255, 0)), (21, (0, 255, 0)), (25, (0, 255, 255)), (36, (0, 0, 255)),
                     (49, (255, 0, 255))):
        assert tuple(wheel[row]) == rgb, row
    assert tuple(wheel[1]) == (255, 17, 0) and tuple(wheel[16]) == (213, 255, 0) and tuple(wheel[54]) == (255, 0, 43)
    assert ((wheel == 255).sum(1) >= 1).all() and ((wheel == 0).sum(1) >= 1).all()


def test_zero_flow_is_white():
    img = V.flow_image_ref(np.zeros((3, 5, 2), np.float32))
    assert img.dtype == np.uint8 and (img == 255).all()
    levels, max_norm = V.flow_levels_ref(np.zeros((1, 1, 2), np.float32))
    assert max_norm == 0.0 and (levels == 255.0).all()


def test_flow_image_directions():
    # a unit flow along -x has angle atan2(-0, 1) = 0: fk = 27, between rows 27 and 28 of CB at f = 0
    f = np.zeros((1, 2, 2), np.float32)
    f[0, 0] = (-1.0, 0.0)
    f[0, 1] = (-0.5, 0.0)
    levels, max_norm = V.flow_levels_ref(f)
    assert max_norm == 1.0
    wheel = V.colour_wheel()
    np.testing.assert_allclose(levels[0, 0], wheel[27], atol=1e-3)       # norm ~ 1: the wheel's colour
    np.testing.assert_allclose(levels[0, 1], 255 - 0.5 * (255 - wheel[27]), atol=1e-3)  # half way to white


def test_affine_identity_float64():
    rng = np.random.default_rng(0)
    for R, S, K in ((3, 7, 1), (5, 64, 10), (2, 33, 30)):
        pts = rng.normal(size=(R, S, 3))
        w = rng.random((R, S))
        omega, vel = 0.3 * rng.normal(size=(K, 3)), 0.3 * rng.normal(size=(K, 3))
        dt = 0.01
        proj = np.array([[1.2, 0, 0.1], [0, 1.3, -0.1], [0, 0, -1.0]])
        pts[..., 2] -= 4.0
        pix = rng.uniform(-1, 1, (R, 2))
        ref = V.ray_visuals_ref(pts, np.zeros_like(pts), w, omega=omega, vel=vel, dt=dt, proj=proj, pix=pix,
                                flow_hw=(24, 32))["flow"]
        A, b = V.affine_of_steps(omega, vel, dt)
        P = (w[:, :, None] * pts).sum(1) @ A.T + w.sum(1)[:, None] * b
        q = P @ proj.T
        got = (q[:, :2] / q[:, 2:] - pix) * np.array([16.0, 12.0])
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_depth_range_update_at_every_milestone():
    from copenerf.visualize import depth_bound_lr, update_depth_range
    cfg = {"depth_bound_scheduler_milestones": [0, 1000, 5000], "depth_bound_lr": [0.5, 0.1, 0.01]}
    for it, lr in ((0, 0.5), (999, 0.5), (1000, 0.1), (4999, 0.1), (5000, 0.01), (10 ** 6, 0.01)):
        assert depth_bound_lr(it, cfg) == lr, it
    # by hand: far <- far (1 - lr) + 1.1 z_max lr; the near bound stays
    dr = [0.01, 5.0]
    assert update_depth_range(dr, 0, cfg, 0.5, 2.0) == (0.45, 2.0 * 1.1)
    assert dr[0] == 0.01 and dr[1] == pytest.approx(5.0 * 0.5 + 2.2 * 0.5, abs=1e-15) and dr[1] == pytest.approx(3.6)
    update_depth_range(dr, 1000, cfg, 0.001, 4.0)
    assert dr[1] == pytest.approx(3.6 * 0.9 + 4.4 * 0.1) and dr[1] == pytest.approx(3.68)
    lo, hi = update_depth_range(dr, 5000, cfg, 0.001, 1.0)
    assert lo == 0.01 and hi == pytest.approx(1.1)  # the logged lower bound is floored by the configured near
    assert dr == [0.01, pytest.approx(3.68 * 0.99 + 1.1 * 0.01)] and dr[1] == pytest.approx(3.6542)
    with pytest.raises(ValueError):
        depth_bound_lr(5, {"depth_bound_scheduler_milestones": [10], "depth_bound_lr": [0.5]})


def test_vis_file_names_and_shapes(tmp_path):
    from PIL import Image

    from copenerf.visualize import VIS_FILES, vis_paths, write_vis_files
    assert VIS_FILES == ("%04d_img.png", "%04d_flow.png", "%04d_normal.png", "%04d_disparity.png",
                         "%04d_disparity_highest_weight.png")
    rng = np.random.default_rng(1)
    h, w = 6, 9
    imgs = {"img": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "flow": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            "normal": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "disparity": rng.integers(0, 256, (h, w), dtype=np.uint8),
            "disparity_highest_weight": rng.integers(0, 256, (h, w), dtype=np.uint8), "stats": np.zeros(5, np.float32)}
    paths = write_vis_files(str(tmp_path), 7, imgs)
    assert paths == vis_paths(str(tmp_path), 7)
    assert [os.path.basename(p) for p in paths] == ["0007_img.png", "0007_flow.png", "0007_normal.png", "0007_disparity.png",
                                                    "0007_disparity_highest_weight.png"]
    for p, key in zip(paths, ("img", "flow", "normal", "disparity", "disparity_highest_weight")):
        assert np.array_equal(np.asarray(Image.open(p)), imgs[key]), key  # PNG is lossless


def test_train_view_npz_contract(tmp_path):
    from PIL import Image

    from copenerf.pose_refine import load_depth_dir
    from copenerf.visualize import depth_path, write_train_view
    rng = np.random.default_rng(2)
    h, w = 5, 8
    depths = {i: (rng.random((h, w)) * 3 + 0.1).astype(np.float32) for i in (12, 3, 100)}
    for i, d in depths.items():
        write_train_view(str(tmp_path), i, d, rng.random((h, w, 3)).astype(np.float32) * 1.2 - 0.1)
    ddir = os.path.join(str(tmp_path), "extraction_stage1", "depths")
    assert sorted(os.listdir(ddir)) == ["000003.jpg", "000012.jpg", "000100.jpg", "depth_000003.npz", "depth_000012.npz",
                                        "depth_000100.npz"]
    assert depth_path(str(tmp_path), 3) == os.path.join(ddir, "depth_000003.npz")
    with np.load(depth_path(str(tmp_path), 12)) as f:
        assert f.files == ["pred"] and f["pred"].dtype == np.float32 and f["pred"].shape == (h, w)
    back = load_depth_dir(ddir)  # what tools/refine_poses.py and setup_pose_refinement read
    assert back.dtype == np.float32 and back.shape == (3, h, w)
    for k, i in enumerate(sorted(depths)):
        assert np.array_equal(back[k], depths[i]), i
    assert sorted(os.listdir(os.path.join(str(tmp_path), "extraction_stage1", "images"))) == ["000003.png", "000012.png",
                                                                                          "000100.png"]
    assert np.asarray(Image.open(os.path.join(ddir, "000003.jpg"))).shape == (h, w)
    assert np.asarray(Image.open(os.path.join(str(tmp_path), "extraction_stage1", "images", "000003.png"))).shape == (h, w, 3)


def test_trainer_has_render_visdata_with_the_reference_signature():
    import inspect

    import copenerf
    import model
    sig = inspect.signature(copenerf.Trainer.render_visdata)
    assert list(sig.parameters) == ["self", "data", "world_mat", "query_cam_idx", "resolution", "it", "anneal_end",
                                    "out_render_path", "idx", "render_only"]
    assert [sig.parameters[k].default for k in ("out_render_path", "idx", "render_only")] == [None, None, False]
    assert model.render_visdata is copenerf.render_visdata and model.render_train_views is copenerf.render_train_views
    sig = inspect.signature(copenerf.render_visdata)
    assert list(sig.parameters)[:7] == ["renderer", "data", "world_mat", "query_cam_idx", "resolution", "it", "anneal_end"]
    for k in ("total_nb_images", "nb_sample_timestep", "depth_range", "cfg", "out_render_path", "idx", "render_only",
              "gt_depths", "logger"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert list(inspect.signature(copenerf.render_train_views).parameters)[:4] == ["renderer", "loader_or_views",
                                                                                  "image_indices", "out_dir"]
    from copenerf.inference import render_image
    assert inspect.signature(render_image).parameters["ray_visuals"].default == "torch"
