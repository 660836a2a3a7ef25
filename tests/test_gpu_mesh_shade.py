"""cn_mesh_shade (ops.mesh_shade, mesh.render_mesh) against the float64 restatement tests/mesh_shade_ref.py.  Every
comparison feeds the reference the kernel's own tri image (ops.mesh_raster's), so none depends on a coverage or tie
decision.

Bounds.  On scene_thread and scene_group: mesh_shade_ref.EPS_ATTR / EPS_NORMAL_DEG, four times the fp32 restatement's
worst error against float64, measured on the CPU and pinned (tests/test_mesh_shade_host.py).  The small scenes are
worse conditioned than those two -- triangles of two or three pixels at 37 x 23 divide the same rounding of the screen
coordinates by a smaller area, and interpolated vertex normals differ more across a triangle than positions do: the
restatement alone is off by up to 2.4 times the pinned figure for positions there, and by up to 5.3e-4 degrees for
smooth normals -- so _ref() measures the restatement against float64 on each test's own inputs and the bar is four
times the larger of that and the pinned figure.  The restatement is not the code under test; nothing here comes from
what the kernel gives.  Pictures: exact where the reference's value is farther than 1e-4 from an integer, within one
level elsewhere."""
import numpy as np
import pytest
import torch

import mesh_shade_ref as R
from mesh_eval_ref import icosphere
from mesh_raster_ref import three_views

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEAR = 1e-4


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _shade(v, f, P, want, tri=None, **kw):
    """(outputs as numpy, the tri image used): ops.mesh_shade on ops.mesh_raster's tri unless one is given."""
    from copenerf import ops
    tv, tf, tP = _t(v), _t(f), _t(P)
    if tri is None:
        h, w = kw.pop("hw")
        tri = ops.mesh_raster(tv, tf, tP, h, w, near=NEAR)[1]
    else:
        kw.pop("hw", None)
        tri = _t(tri)
    for k in ("attr", "vnormals", "rot"):
        if k in kw:
            kw[k] = _t(kw[k])
    return _np(ops.mesh_shade(tv, tf, tP, tri, want=want, **kw)), tri.cpu().numpy()


def _ref(v, f, P, tri, pinned=False, **kw):
    """shade_ref of one view with the bounds for it under "eps": the pinned ones, or four times the larger of the
    pinned figure and the fp32 restatement's error against float64 on these very inputs."""
    ref = R.shade_ref(v, f, P, tri, **kw)
    eps = {"attr": R.EPS_ATTR, "normal": R.EPS_NORMAL_DEG}
    if not pinned:
        f32 = R.shade_f32(v, f, P, tri, **kw)
        m = ref["mask"]
        if "attr" in ref and m.any():
            eps["attr"] = R.MARGIN * max(R.ATTR_F32_WORST, float(np.abs(ref["attr"][m] - f32["attr"][m]).max()))
        if m.any():
            eps["normal"] = R.MARGIN * max(R.NORMAL_F32_WORST_DEG, float(R.angle_deg(ref["normal"][m], f32["normal"][m]).max()))
    ref["eps"] = eps
    return ref


def _check(got, ref, what=("attr", "normal")):
    """attr and normal of one view against shade_ref's at every covered pixel, background elsewhere."""
    m = ref["mask"]
    worst = {}
    if "attr" in what:
        worst["attr"] = float(np.abs(got["attr"][m].astype(np.float64) - ref["attr"][m]).max())
        assert worst["attr"] <= ref["eps"]["attr"], (worst, ref["eps"])
        assert np.all(got["attr"][~m] == ref["attr"][~m])
    if "normal" in what:
        worst["normal"] = float(R.angle_deg(got["normal"][m], ref["normal"][m]).max())
        assert worst["normal"] <= ref["eps"]["normal"], (worst, ref["eps"])
        assert np.abs(np.linalg.norm(got["normal"][m].astype(np.float64), axis=1) - 1).max() <= 1e-6
        assert np.all(got["normal"][~m] == 0)
    return worst


def _pinhole(h, w, f=10.0):
    return np.array([[[f, 0, 0.5 * (w - 1), 0], [0, f, 0.5 * (h - 1), 0], [0, 0, 1, 0]]], dtype=np.float32)


def test_one_triangle_reprojection_identity_and_constant():
    """16 x 12, one view: with attr = the vertex positions, proj . [attr_out, 1] gives back (x, y, the rasteriser's
    depth) at every covered pixel; attr = ones gives 1 to rounding."""
    from copenerf import ops
    h, w = 12, 16
    P = _pinhole(h, w, 14.0)
    P[0, 2, :] = [0.1, -0.05, 1.0, 0.2]  # a depth that varies over the image
    v = np.array([[-0.45, -0.32, 1.0], [0.5, -0.25, 1.4], [0.05, 0.36, 0.8]], dtype=np.float32)
    f = np.array([[0, 1, 2]], dtype=np.int32)
    depth, tri = (x.cpu().numpy() for x in ops.mesh_raster(_t(v), _t(f), _t(P), h, w, near=NEAR))
    got, _ = _shade(v, f, P, ("attr",), tri=tri, attr=v)
    m = tri[0] >= 0
    assert m.sum() >= 30
    ys, xs = np.nonzero(m)
    X = np.concatenate([got["attr"][0][m].astype(np.float64), np.ones((m.sum(), 1))], 1) @ P[0].astype(np.float64).T
    # (attr within EPS_ATTR of the exact point; the pixel moves by at most |P| / c times that)
    scale = np.abs(P[0, :, :3]).sum(1).max() / X[:, 2].min()
    assert np.abs(X[:, 0] / X[:, 2] - xs).max() <= R.EPS_ATTR * scale
    assert np.abs(X[:, 1] / X[:, 2] - ys).max() <= R.EPS_ATTR * scale
    assert np.abs(X[:, 2] - depth[0][m]).max() <= R.EPS_ATTR * np.abs(P[0, 2, :3]).sum() + 4.2e-6 * depth[0][m].max()
    _check({"attr": got["attr"][0]}, _ref(v, f, P[0], tri[0], attr=v), ("attr",))
    ones, _ = _shade(v, f, P, ("attr",), tri=tri, attr=np.ones((3, 1), dtype=np.float32), fill=-7.0)
    assert ones["attr"].shape == (1, h, w, 1)
    assert np.abs(ones["attr"][0][m] - 1).max() <= 3 * 2.0 ** -23 and np.all(ones["attr"][0][~m] == -7.0)


@pytest.mark.parametrize("scene", ["scene_thread", "scene_group"])
def test_scenes_attr_normal_and_pictures(scene):
    """96 x 64, three views (scene_group: the two large quads and the skipped straddler): attr_out and normal_out
    against shade_ref at every covered pixel, normal_out . (Cam - X) > 0 everywhere; in the camera frame with vertex
    colours, normal_out and both pictures."""
    sc = getattr(R, scene)()
    v, f, views, h, w = sc[:5]
    P = R.projections(views, h, w)
    got, tri = _shade(v, f, P, ("attr", "normal"), hw=(h, w), attr=v)
    col = (np.abs(v) / np.abs(v).max()).astype(np.float32)
    rot = np.stack([x["world_mat"][:3, :3] for x in views]).astype(np.float32)
    light = np.array([0.3, 0.2, 0.9]) / np.linalg.norm([0.3, 0.2, 0.9])
    cam, _ = _shade(v, f, P, ("normal", "normal_image", "shaded"), tri=tri, attr=col, rot=rot, albedo_from_attr=True,
                    light=light, ambient=0.25, background=(1, 2, 3))
    covered = 0
    for i in range(len(P)):
        ref = _ref(v, f, P[i], tri[i], pinned=True, attr=v)
        m = ref["mask"]
        covered += int(m.sum())
        print(scene, i, _check({k: got[k][i] for k in got}, ref))
        C = R.camera_centre(P[i])
        assert np.all(((C - got["attr"][i][m].astype(np.float64)) * got["normal"][i][m]).sum(1) > 0)
        refc = _ref(v, f, P[i], tri[i], pinned=True, attr=col, rot=rot[i], albedo_from_attr=True, light=light, ambient=0.25)
        _check({"normal": cam["normal"][i]}, refc, ("normal",))
        for key, pre in (("normal_image", "normal_pre"), ("shaded", "shaded_pre")):
            share = R.compare_pictures(cam[key][i][m], refc[pre], share_cap=R.IMAGE_NEAR_SHARE)
            assert np.all(cam[key][i][~m] == np.array([1, 2, 3], dtype=np.uint8)), key
            print(scene, i, key, "near-integer share", share)
    assert covered > 4000
    if scene == "scene_group":
        assert not np.any(tri == sc[5]) and np.mean((tri >= 0) & (tri < 4)) > 0.3


def test_shared_edge_opposite_corner_order():
    """Two triangles sharing an edge, corner indices in opposite order (one wound each way, and the shared edge run from
    the smaller index by one and from the larger by the other): the sign convention."""
    h, w = 20, 24
    P = _pinhole(h, w, 16.0)
    v = np.array([[-0.6, -0.5, 1.0], [0.55, -0.45, 1.3], [0.5, 0.52, 0.9], [-0.58, 0.5, 1.2]], dtype=np.float32)
    for f in (np.array([[0, 1, 2], [0, 2, 3]]), np.array([[0, 1, 2], [3, 2, 0]]), np.array([[2, 1, 0], [0, 2, 3]]),
              np.array([[1, 2, 0], [2, 0, 3]])):
        f = f.astype(np.int32)
        got, tri = _shade(v, f, P, ("attr", "normal"), hw=(h, w), attr=v)
        ref = _ref(v, f, P[0], tri[0], attr=v)
        assert (tri[0] == 0).sum() > 40 and (tri[0] == 1).sum() > 40
        _check({k: got[k][0] for k in got}, ref)
        assert np.all(got["normal"][0][ref["mask"]][:, 2] < 0)  # towards the camera at the origin, looking down +z
        assert ref["lam"].min() > -1e-6  # the weights of a covered pixel are not negative


@pytest.mark.parametrize("C", [1, 3, 4, 7, 8, 16])
def test_channel_counts(C):
    """The load and store paths: rows of a multiple of four channels go as 16-byte vectors."""
    v, f = icosphere(2, 0.5)
    h, w = 23, 37  # an odd image: rows are no multiple of a wave
    P = R.projections(three_views(h, w)[:2], h, w)
    rng = np.random.default_rng(C)  # C linear functions of the position, |value| <= 2
    A = rng.normal(size=(3, C))
    attr = (v.astype(np.float64) @ (A * 2.0 / np.linalg.norm(A, axis=0)) + rng.uniform(-1, 1, size=C)).astype(np.float32)
    assert np.abs(attr).max() <= 2
    got, tri = _shade(v, f, P, ("attr",), hw=(h, w), attr=attr, fill=0.5)
    assert got["attr"].shape == (2, h, w, C) and (tri >= 0).any() and (tri < 0).any()
    for i in range(2):
        _check({"attr": got["attr"][i]}, _ref(v, f, P[i], tri[i], attr=attr, fill=0.5), ("attr",))


def test_nine_views_index_their_own_projection():
    """N = 9 different projections, one more than the rasteriser's batch of 8."""
    v, f = icosphere(2, 0.5)
    h, w = 23, 37
    eyes = [(1.7, 0.6, 0.5), (-0.9, 1.6, -0.7), (0.4, -1.2, 1.5), (-1.5, -0.8, 0.3), (0.2, 0.3, 1.9), (1.0, -1.4, -0.6),
            (-0.3, 1.9, 0.4), (1.3, 1.2, -0.9), (-1.1, -0.2, -1.6)]
    views = [R.make_view(e, (0.01 * i, -0.02, 0.01), (1.0 + 0.05 * i) * h, h, w) for i, e in enumerate(eyes)]
    P = R.projections(views, h, w)
    rot = np.stack([x["world_mat"][:3, :3] for x in views]).astype(np.float32)
    got, tri = _shade(v, f, P, ("attr", "normal"), hw=(h, w), attr=v, rot=rot)
    assert len({tri[i].tobytes() for i in range(9)}) == 9
    for i in range(9):
        _check({k: got[k][i] for k in got}, _ref(v, f, P[i], tri[i], attr=v, rot=rot[i]))


def test_camera_inside_a_box_sees_inward_normals():
    v, f = R.box_mesh(1.5, 6)
    h, w = 32, 48
    view = R.make_view((0.2, -0.1, 0.3), (1.0, 0.4, 0.1), 0.6 * h, h, w)
    P = R.projections([view], h, w)
    got, tri = _shade(v, f, P, ("attr", "normal"), hw=(h, w), attr=v)
    m = tri[0] >= 0
    assert m.mean() > 0.95  # (no clipping: a wall triangle with a corner behind the camera would be skipped)
    ref = _ref(v, f, P[0], tri[0], attr=v)
    _check({k: got[k][0] for k in got}, ref)
    eye = np.array([0.2, -0.1, 0.3])
    pos, n = got["attr"][0][m].astype(np.float64), got["normal"][0][m].astype(np.float64)
    assert np.all(((eye - pos) * n).sum(1) > 0)
    order = np.sort(np.abs(pos), axis=1)
    clear = order[:, 2] - order[:, 1] > 1e-3  # away from the box's edges the wall is the largest coordinate
    wall, ar = np.abs(pos).argmax(1), np.arange(len(pos))
    assert clear.sum() > 0.9 * len(pos)
    assert np.all((n[ar, wall] * pos[ar, wall])[clear] < -0.99 * 1.5)  # the unit normal points straight back into the box


def test_smooth_normals_flip_fallback_and_rotation():
    v, f = icosphere(2, 0.5)
    h, w = 40, 56
    views = three_views(h, w)[:2]
    P = R.projections(views, h, w)
    vn = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    got, tri = _shade(v, f, P, ("normal",), hw=(h, w), vnormals=vn)
    flat, _ = _shade(v, f, P, ("normal",), tri=tri)
    for i in range(2):
        ref = _ref(v, f, P[i], tri[i], vnormals=vn)
        _check({"normal": got["normal"][i]}, ref, ("normal",))
        m = ref["mask"]
        # smooth: a pixel's normal is its own direction from the centre, nearly (chordal error of a level-2 sphere)
        pos, _ = _shade(v, f, P[i:i + 1], ("attr",), tri=tri[i:i + 1], attr=v)
        radial = pos["attr"][0][m] / np.linalg.norm(pos["attr"][0][m], axis=1, keepdims=True)
        assert R.angle_deg(got["normal"][i][m], radial).max() < 1.0 < R.angle_deg(flat["normal"][i][m], radial).max()
    # vertex normals that point away from the face's hemisphere are turned into it; a zero one falls back
    bad = -vn
    bad[::7] = 0.0
    nan_vertex = int(f[tri[0][tri[0] >= 0][0]][0])  # a corner of a triangle the first view sees
    bad[nan_vertex] = np.nan
    got2, _ = _shade(v, f, P, ("normal",), tri=tri, vnormals=bad)
    zero, _ = _shade(v, f, P, ("normal",), tri=tri, vnormals=np.zeros_like(vn))
    assert np.array_equal(zero["normal"], flat["normal"])  # nothing to interpolate: the face normals, bit for bit
    for i in range(2):
        ref = _ref(v, f, P[i], tri[i], vnormals=bad)
        m = ref["mask"]
        _check({"normal": got2["normal"][i]}, ref, ("normal",))
        assert np.all((got2["normal"][i][m].astype(np.float64) * flat["normal"][i][m]).sum(1) > 0)
        nan_px = (f[tri[i][m]] == nan_vertex).any(1)
        assert nan_px.any() or i > 0
        assert np.array_equal(got2["normal"][i][m][nan_px], flat["normal"][i][m][nan_px])
    # a known rotation: the output is the rotated world-frame output
    rot = np.stack([R.rotation((0.3, -0.5, 0.8), 37.0), R.rotation((1.0, 0.2, 0.1), -112.0)]).astype(np.float32)
    turned, _ = _shade(v, f, P, ("normal",), tri=tri, rot=rot)
    for i in range(2):
        m = tri[i] >= 0
        want = flat["normal"][i][m].astype(np.float64) @ rot[i].astype(np.float64).T
        assert R.angle_deg(turned["normal"][i][m], want).max() <= 2 * R.EPS_NORMAL_DEG  # (two roundings of that size)
        _check({"normal": turned["normal"][i]}, _ref(v, f, P[i], tri[i], rot=rot[i]), ("normal",))


def test_background_bad_ids_and_repeatability():
    v, f = icosphere(2, 0.5)
    h, w = 23, 37
    P = R.projections(three_views(h, w)[:2], h, w)
    want = ("attr", "normal", "normal_image", "shaded")
    kw = dict(attr=v, fill=-3.5, background=(9, 8, 250))
    empty, _ = _shade(v, f, P, want, tri=np.full((2, h, w), -1, dtype=np.int32), **kw)
    assert np.all(empty["attr"] == -3.5) and np.all(empty["normal"] == 0)
    for key in ("normal_image", "shaded"):
        assert np.all(empty[key] == np.array([9, 8, 250], dtype=np.uint8))
    # a tri image holding T (and far beyond), and a triangle with a corner index V (and -1): background as documented
    f2 = np.concatenate([f, np.array([[0, 1, len(v)], [-1, 2, 3]], dtype=np.int32)])
    good, tri = _shade(v, f2, P, want, hw=(h, w), **kw)
    forged = tri.copy()
    ys, xs = np.nonzero(tri[0] >= 0)
    forged[0, ys[0], xs[0]] = len(f2)
    forged[0, ys[1], xs[1]] = len(f)       # the triangle with corner index V
    forged[0, ys[2], xs[2]] = len(f) + 1   # the triangle with corner index -1
    forged[0, ys[3], xs[3]] = 2 ** 31 - 1
    forged[1, 0, 0] = -2 ** 31
    got, _ = _shade(v, f2, P, want, tri=forged, **kw)
    changed = forged != tri
    assert changed.sum() == 5
    assert np.all(got["attr"][changed] == -3.5) and np.all(got["normal"][changed] == 0)
    assert np.all(got["shaded"][changed] == np.array([9, 8, 250], dtype=np.uint8))
    for key in want:
        assert np.array_equal(got[key][~changed], good[key][~changed]), key
    again, _ = _shade(v, f2, P, want, tri=forged, **kw)
    for key in want:
        assert np.array_equal(again[key].view(np.uint8), got[key].view(np.uint8)), key  # bitwise
    # no triangles, no vertices: all background
    none, _ = _shade(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), P, ("normal", "shaded"),
                     tri=np.zeros((2, h, w), dtype=np.int32))
    assert np.all(none["normal"] == 0) and np.all(none["shaded"] == 255)


def test_render_mesh_keys_frames_colours_and_transform():
    from copenerf import mesh
    v, f = icosphere(2, 0.5)
    h, w = 24, 32
    views = three_views(h, w)[:2]
    tv, tf = _t(v), _t(f)
    plain = mesh.render_mesh(tv, tf, views, (h, w))
    assert set(plain) == {"depth", "tri", "normal", "normal_image", "shaded"}
    base = mesh.render_mesh_depth(tv, tf, views, (h, w))
    assert torch.equal(plain["depth"], base["depth"]) and torch.equal(plain["tri"], base["tri"])
    world = mesh.render_mesh(tv, tf, views, (h, w), frame="world", attrs=tv)
    assert world["attr"].shape == (2, h, w, 3)
    m = (plain["tri"] >= 0).cpu().numpy()
    for i, view in enumerate(views):
        want = world["normal"][i].cpu().numpy()[m[i]].astype(np.float64) @ view["world_mat"][:3, :3].T
        assert R.angle_deg(plain["normal"][i].cpu().numpy()[m[i]], want).max() <= 2 * R.EPS_NORMAL_DEG  # (two roundings)
        assert np.all(plain["normal"][i].cpu().numpy()[m[i]][:, 2] > 0)  # the camera looks down -z: normals face it
    # the default light is a headlight in the camera frame; a white sphere is bright in the middle, the background white
    img = plain["shaded"].cpu().numpy()
    assert np.all(img[~m] == 255) and img[m].max() > 180 and img[m].min() >= int(0.8 * 0.3 * 255)
    red = np.tile(np.array([[255, 0, 0]], dtype=np.uint8), (len(v), 1))
    for colors in (_t(red), _t(red.astype(np.float32) / 255)):
        c = mesh.render_mesh(tv, tf, views, (h, w), colors=colors)["shaded"].cpu().numpy()
        assert np.all(c[m][:, 1:] == 0) and c[m][:, 0].min() >= 76 and c[m][:, 0].max() > 200
    # a similarity moves the mesh and the cameras together: the same pictures, camera-frame normals to rounding, and
    # world-frame normals turned by its rotation
    Rs = R.rotation((0.2, 0.9, -0.4), 63.0)
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = 1.7 * Rs, (0.3, -1.1, 0.6)
    moved = mesh.render_mesh(tv, tf, views, (h, w), transform=S)
    same = (moved["tri"] == plain["tri"]).cpu().numpy() & m
    assert same.sum() > 0.97 * m.sum()
    assert R.angle_deg(moved["normal"].cpu().numpy()[same], plain["normal"].cpu().numpy()[same]).max() < 0.05
    moved_w = mesh.render_mesh(tv, tf, views, (h, w), transform=S, frame="world")["normal"].cpu().numpy()
    assert R.angle_deg(moved_w[same], world["normal"].cpu().numpy()[same].astype(np.float64) @ Rs.T).max() < 0.05
    with pytest.raises(ValueError, match="frame"):
        mesh.render_mesh(tv, tf, views, (h, w), frame="object")


def test_end_to_end_mesh_normals_against_the_volume_renderer():
    """The geometric-init network's sphere, extracted at 33^3 and rendered with render_mesh(frame="camera"), against
    render_image's normal map from the same view: normal_metrics over the pixels both cover.  Nobody has measured the
    figure before; it is printed here (DESIGN 3.12.4 records it) and only asked to be a finite angle below 90."""
    from copenerf import NeuSRenderer, mesh, metrics
    from copenerf.inference import render_image
    from copenerf.rays import intrinsics_ndc
    from helpers import REN_CFG, build_modules
    sdf, col, dev = build_modules(7, device=DEV)
    r = NeuSRenderer(None, sdf, dev, col, None, **REN_CFG).to(DEV).set_mfma_dtype("bf16x6")
    v, tri = r.extract_geometry(torch.tensor((-1.0, -1.0, -1.0)), torch.tensor((1.0, 1.0, 1.0)), 33, 0.0, time_step=0.3)
    assert len(tri) > 0
    h, w = 24, 32
    K = intrinsics_ndc(1.1 * w, 1.1 * w, w, h, device=DEV)
    W = torch.from_numpy(R.look_at((1.1, 0.7, 1.3), (0.0, 0.0, 0.0))).float().to(DEV)
    view = {"camera_mat": K, "world_mat": W}
    got = mesh.render_mesh(_t(v), _t(tri), [view], (h, w), frame="camera")
    with torch.no_grad():
        vol = render_image(r, K, W, torch.eye(4, device=DEV), (h, w), torch.tensor([0.3], device=DEV), chunk=h * w)
    both = (got["tri"][0] >= 0) & (vol["normal"].norm(dim=-1) > 0.5)
    assert int(both.sum()) > 20
    res = metrics.normal_metrics(got["normal"][0], vol["normal"], both)
    print("mesh against volume normals over %d pixels:" % int(both.sum()), res)
    assert res is not None and np.isfinite(res["mean"]) and 0 <= res["mean"] < 90
