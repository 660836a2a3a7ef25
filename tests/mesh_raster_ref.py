"""Test infrastructure: restatements of the mesh rasteriser and the visibility pass (csrc/cn_mesh_raster.hip).

raster_ref / visibility_ref are the yardstick: float64 numpy from the fp32 inputs, the same coverage rule (edge
functions from the endpoints in vertex-index order, all >= 0 or all <= 0), perspective-correct depth, the
smaller id at equal depth, and the same visibility rule.  raster_ref also returns every pixel's *edge margin*: the
smallest distance, in pixels, from the pixel centre to the line through any edge of any triangle whose box, padded
by PAD pixels, contains the pixel; a pixel is *decided* when its margin exceeds DELTA.  (The kernel's pixel
positions carry fp32 rounding of a few 2^-24 of the image size, 1e-4 pixels at 640 and less here: where it could
tell a pixel from the float64 rule, the pixel lies that close to an edge line -- and inside that triangle's padded
box.)  visibility_ref returns which points are decided: c farther than C_MARGIN, relative, from `near` and from
the tolerance bound, and the pixel position farther than DELTA from a rounding boundary and from the image's rim.

raster_f32 is NOT the yardstick and not the code under test: it restates the kernel's fp32 operation order in
numpy float32 so that the depth bound of the GPU tests can be measured on the CPU against raster_ref
(tests/test_mesh_raster_host.py does, and pins the figures)."""
import numpy as np

DELTA = 1e-3     # pixels
PAD = 0.5        # pixels
C_MARGIN = 1e-5  # relative: forty times the 4 x 2^-24 of the fp32 projection's three products and three sums


def project64(P, X):
    """(sx, sy, c) in float64 of points X [n, 3] under one projection P [3, 4] (fp32 values)."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    abc = X @ P[:, :3].T + P[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        return abc[:, 0] / abc[:, 2], abc[:, 1] / abc[:, 2], abc[:, 2]


def _edges(idx, x, y):
    """Per edge k (opposite corner k): (lx, ly, dx, dy, sign) from the endpoint of the smaller vertex index."""
    out = []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        fwd = idx[i] < idx[j]
        l, h = (i, j) if fwd else (j, i)
        out.append((x[l], y[l], x[h] - x[l], y[h] - y[l], 1.0 if fwd else -1.0))
    return out


def raster_ref(vertices, triangles, P, h, w, near):
    """One view in float64: (depth [h, w], inf where nothing is seen; tri [h, w], -1 where nothing; margin [h, w],
    inf where no padded box reaches)."""
    sx, sy, c = project64(P, vertices)
    V = len(vertices)
    depth = np.full((h, w), np.inf)
    tri = np.full((h, w), -1, dtype=np.int64)
    margin = np.full((h, w), np.inf)
    for t, idx in enumerate(np.asarray(triangles)):
        if idx.min() < 0 or idx.max() >= V:
            continue
        cc = c[idx]
        if not np.all(np.isfinite(cc)) or np.any(cc < near):
            continue
        x, y, iw = sx[idx], sy[idx], 1.0 / cc
        E = _edges(idx, x, y)
        lx, ly, dx, dy, sg = E[2]
        area = sg * (dx * (y[2] - ly) - dy * (x[2] - lx))
        if not abs(area) > 0.0:
            continue
        # the padded box, for the margin
        X0, X1 = max(int(np.floor(x.min() - PAD)), 0), min(int(np.ceil(x.max() + PAD)), w - 1)
        Y0, Y1 = max(int(np.floor(y.min() - PAD)), 0), min(int(np.ceil(y.max() + PAD)), h - 1)
        if X0 > X1 or Y0 > Y1:
            continue
        py, px = np.mgrid[Y0:Y1 + 1, X0:X1 + 1].astype(np.float64)
        e = [sg * (dx * (py - ly) - dy * (px - lx)) for lx, ly, dx, dy, sg in E]
        m = margin[Y0:Y1 + 1, X0:X1 + 1]
        for ek, (_, _, dx, dy, _) in zip(e, E):
            n = np.hypot(dx, dy)
            if n > 0:
                np.minimum(m, np.abs(ek) / n, out=m)
        inbox = (px >= np.ceil(x.min())) & (px <= np.floor(x.max())) & (py >= np.ceil(y.min())) & (py <= np.floor(y.max()))
        cov = inbox & (((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0)))
        with np.errstate(divide="ignore", invalid="ignore"):
            d = ((e[0] + e[1]) + e[2]) / ((e[0] * iw[0] + e[1] * iw[1]) + e[2] * iw[2])
        win = cov & (d > 0) & np.isfinite(d) & (d < depth[Y0:Y1 + 1, X0:X1 + 1])  # (t ascends: a tie keeps the smaller id)
        depth[Y0:Y1 + 1, X0:X1 + 1][win] = d[win]
        tri[Y0:Y1 + 1, X0:X1 + 1][win] = t
    return depth, tri, margin


def raster_f32(vertices, triangles, P, h, w, near):
    """The kernel's operation order in numpy float32, one view: (depth float32 [h, w], tri [h, w])."""
    f = np.float32
    P = np.asarray(P, dtype=f)
    X = np.asarray(vertices, dtype=f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a, b, c = (((P[r, 0] * X[:, 0] + P[r, 1] * X[:, 1]) + P[r, 2] * X[:, 2]) + P[r, 3] for r in range(3))
        sx, sy, iws = a / c, b / c, f(1.0) / c
    assert sx.dtype == f and iws.dtype == f
    V = len(X)
    depth = np.full((h, w), np.inf, dtype=f)
    tri = np.full((h, w), -1, dtype=np.int64)
    for t, idx in enumerate(np.asarray(triangles)):
        if idx.min() < 0 or idx.max() >= V:
            continue
        cc = c[idx]
        if not np.all(cc >= f(near)) or not np.all(cc < np.inf):
            continue
        x, y, iw = sx[idx], sy[idx], iws[idx]
        E = _edges(idx, x, y)
        lx, ly, dx, dy, sg = E[2]
        area = f(sg) * (dx * (y[2] - ly) - dy * (x[2] - lx))
        if not abs(area) > 0.0:
            continue
        x0, x1 = max(np.ceil(x.min()), 0.0), min(np.floor(x.max()), w - 1.0)
        y0, y1 = max(np.ceil(y.min()), 0.0), min(np.floor(y.max()), h - 1.0)
        if not (x0 <= x1 and y0 <= y1):
            continue
        x0, x1, y0, y1 = int(x0), int(x1), int(y0), int(y1)
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(f)
        e = [f(sg) * (dx * (py - ly) - dy * (px - lx)) for lx, ly, dx, dy, sg in E]
        cov = ((e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)) | ((e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0))
        with np.errstate(divide="ignore", invalid="ignore"):
            d = ((e[0] + e[1]) + e[2]) / ((e[0] * iw[0] + e[1] * iw[1]) + e[2] * iw[2])
        assert d.dtype == f
        win = cov & (d > 0) & np.isfinite(d) & (d < depth[y0:y1 + 1, x0:x1 + 1])
        depth[y0:y1 + 1, x0:x1 + 1][win] = d[win]
        tri[y0:y1 + 1, x0:x1 + 1][win] = t
    return depth, tri


def compare_view(got_depth, got_tri, ref, cap=0.03):
    """The criteria of the GPU raster tests for one view: at decided pixels coverage and triangle ids equal the
    reference's exactly; returns (the worst relative depth error there, the share of the reference's covered pixels
    left out as undecided), having asserted the share against the cap."""
    depth, tri, margin = ref
    decided = margin > DELTA
    covered = tri >= 0
    left_out = float((covered & ~decided).sum()) / max(int(covered.sum()), 1)
    assert left_out <= cap, left_out
    got_tri = np.asarray(got_tri)
    assert np.array_equal(got_tri[decided], tri[decided])
    sel = decided & covered
    got_depth = np.asarray(got_depth, dtype=np.float64)
    assert np.all(np.isinf(got_depth[decided & ~covered]))
    err = np.abs(got_depth[sel] - depth[sel]) / depth[sel]
    return (float(err.max()) if err.size else 0.0), left_out


def _seen_at(sx, sy, c, h, w, depth, tol_abs, tol_rel, near):
    """The visibility rule of one view at the given pixel positions: (seen, clear) with clear where c is farther
    than C_MARGIN from `near` and, where a finite depth bound applies, from that bound."""
    front = c >= near
    clear = np.abs(c - near) > C_MARGIN * np.abs(c)
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(sx + 0.5), np.floor(sy + 0.5)
        inside = front & (fx >= 0) & (fx <= w - 1) & (fy >= 0) & (fy <= h - 1)
    if depth is None:
        return inside, clear
    ix, iy = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
    bound = np.asarray(depth, dtype=np.float64)[iy, ix] * (1.0 + float(np.float32(tol_rel))) + float(np.float32(tol_abs))
    with np.errstate(invalid="ignore"):
        clear &= ~(inside & np.isfinite(bound) & (np.abs(c - bound) <= C_MARGIN * np.abs(c)))
    return inside & (c <= bound), clear


def visibility_ref(points, P, h, w, depth=None, tol_abs=0.0, tol_rel=0.0, near=1e-4):
    """(count [Q], decided [Q], stable [Q]) in float64 over the views P [N, 3, 4]; depth [N, h, w] are the fp32 maps
    the pass under test is given as well (they are an input of the rule, not part of it).  decided: in every view c
    is clear of its bounds and, in front of the camera, the pixel position is farther than DELTA from a rounding
    boundary (the image's rim is one).  stable is the weaker condition that decides a cull: in every view the
    outcome is the same, and c clear of its bounds, at the four positions DELTA away in x and y -- a point on a
    rounding boundary is stable when both pixels give the same answer."""
    Q = len(points)
    count = np.zeros(Q, dtype=np.int64)
    decided = np.ones(Q, dtype=bool)
    stable = np.ones(Q, dtype=bool)
    for v in range(len(P)):
        sx, sy, c = project64(P[v], points)
        dm = None if depth is None else depth[v]
        seen, clear = _seen_at(sx, sy, c, h, w, dm, tol_abs, tol_rel, near)
        with np.errstate(invalid="ignore"):
            near_edge = (np.abs(sx + 0.5 - np.round(sx + 0.5)) <= DELTA) | (np.abs(sy + 0.5 - np.round(sy + 0.5)) <= DELTA)
        decided &= clear & ~((c >= near) & near_edge)
        stable &= clear
        for ox in (-DELTA, DELTA):
            for oy in (-DELTA, DELTA):
                s2, c2 = _seen_at(sx + ox, sy + oy, c, h, w, dm, tol_abs, tol_rel, near)
                stable &= c2 & (s2 == seen)
        count += seen
    return count, decided, stable


# ---- scenes ------------------------------------------------------------------------------------------------------

def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """World-to-camera 4 x 4 (float64) of a camera at `eye` looking at `target`: x right, y up, looking down -z,
    the convention rays.intrinsics_ndc's camera matrix goes with."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(back, right), back])
    W = np.eye(4)
    W[:3, :3], W[:3, 3] = R, -R @ eye
    return W


def intrinsics(fx, fy, w, h):
    """rays.intrinsics_ndc in float64."""
    return np.diag([2.0 * fx / w, -2.0 * fy / h, -1.0, 1.0])


def make_view(eye, target, focal, h, w, up=(0.0, 0.0, 1.0), scale_mat=None):
    v = {"camera_mat": intrinsics(focal, focal, w, h), "world_mat": look_at(eye, target, up)}
    if scale_mat is not None:
        v["scale_mat"] = np.asarray(scale_mat, dtype=np.float64)
    return v


def three_views(h, w):
    """Three off-axis cameras around the origin, about 2 away, a sphere of radius 0.5 filling most of the image's
    height."""
    f = 1.4 * h
    return [make_view((1.7, 0.6, 0.5), (0.03, -0.02, 0.01), f, h, w),
            make_view((-0.9, 1.6, -0.7), (-0.02, 0.04, 0.0), f, h, w),
            make_view((0.4, -1.2, 1.5), (0.0, 0.01, -0.03), f, h, w, up=(0.0, 1.0, 0.2))]


def side_views(h, w):
    """Three cameras on the +x side looking towards -x: what scene_group's quads face."""
    f = 0.9 * h
    return [make_view((1.8, 0.3, 0.4), (0.0, 0.02, -0.01), f, h, w),
            make_view((1.7, -0.5, 0.2), (0.02, 0.0, 0.03), f, h, w),
            make_view((1.6, 0.2, -0.6), (-0.01, 0.03, 0.0), f, h, w, up=(0.0, 0.3, 1.0))]


def scene_thread():
    """(vertices, triangles, views, h, w): the icosphere of 1280 triangles, radius 0.5, at 96 x 64 from three
    off-axis cameras -- triangles of a few pixels, all on the one-thread path."""
    from mesh_eval_ref import icosphere
    v, f = icosphere(3, 0.5)
    return v, f, three_views(64, 96), 64, 96


def scene_group():
    """(vertices, triangles, views, h, w, straddler): two large, slightly tilted quads behind one another that fill
    most of the image (four triangles for the workgroup path), the icosphere in front of them (the thread path),
    and one triangle with a corner behind every camera (its id is `straddler`): skipped, no clipping."""
    from mesh_eval_ref import icosphere
    sv, sf = icosphere(3, 0.5)

    def quad(x, tilt):
        c = np.array([[x - tilt, -2.0, -2.0], [x + tilt, 2.0, -2.0], [x + 2 * tilt, 2.0, 2.0], [x, -2.0, 2.0]], dtype=np.float32)
        return c, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    behind = (np.array([[3.0, 0.0, 0.0], [-0.5, 0.3, 0.9], [-0.5, -0.3, 0.9]], dtype=np.float32),
              np.array([[0, 1, 2]], dtype=np.int32))
    v, f = merge(quad(-0.8, 0.05), quad(-1.2, -0.04), (sv, sf), behind)
    return v, f, side_views(64, 96), 64, 96, len(f) - 1


CULL_TOL_ABS = 0.05  # the cull tests' tolerance: no vertex of scene_cull lies within C_MARGIN of its bound (asserted)


def scene_cull():
    """(vertices, triangles, views, h, w): the icosphere inside a closed box of half-edge 2.5 that holds the three
    side cameras too -- sphere vertices seen by all three or by none (the far side), wall vertices in front of some
    cameras' frustums and not others', hidden behind the sphere, or behind the cameras."""
    from mesh_eval_ref import icosphere
    v, f = merge(icosphere(3, 0.5), box_mesh(2.5, 6))
    h, w, foc = 64, 96, 0.9 * 64
    # (side_views nudged: from these eyes no vertex projects within DELTA of a rounding boundary at a silhouette,
    # where the two pixels would disagree -- visibility_ref's `stable`, asserted by the tests that rely on it)
    views = [make_view((1.8, 0.34, 0.4), (0.0, 0.02, -0.01), foc, h, w),
             make_view((1.7, -0.5, 0.24), (0.02, 0.0, 0.03), foc, h, w),
             make_view((1.6, 0.21, -0.63), (-0.01, 0.03, 0.0), foc, h, w, up=(0.0, 0.3, 1.0))]
    return v, f, views, h, w


# The depth bound of the GPU tests.  F32_WORST is the worst relative depth error of raster_f32 -- the kernel's fp32
# operation order restated in numpy -- against raster_ref at the decided pixels of scene_thread and scene_group,
# measured on the CPU (tests/test_mesh_raster_host.py measures it again and pins it); the bound is four times that,
# the margin for the operation-order freedom a compiler keeps (division and reciprocal rounding, reassociation-free
# otherwise under -ffp-contract=off).
F32_WORST = 1.04e-6  # 17.4 x 2^-24 (scene_thread's second view; scene_group's worst is 8.2e-7)
EPS_DEPTH = 4.0 * F32_WORST


def box_mesh(half=1.5, n=6):
    """A closed axis-aligned box of half-edge `half` around the origin, each face an n x n grid of quads split
    into two triangles, vertices welded per face only (12 n^2 triangles)."""
    verts, tris = [], []
    g = np.linspace(-half, half, n + 1)
    for axis in range(3):
        for side in (-half, half):
            base = len(verts)
            for a in g:
                for b in g:
                    p = [0.0, 0.0, 0.0]
                    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, a, b
                    verts.append(p)
            for i in range(n):
                for j in range(n):
                    q = base + i * (n + 1) + j
                    tris += [(q, q + 1, q + n + 2), (q, q + n + 2, q + n + 1)]
    return np.array(verts, dtype=np.float32), np.array(tris, dtype=np.int32)


def merge(*meshes):
    """One mesh from several (vertices float32, triangles int32), indices shifted."""
    vs, ts, off = [], [], 0
    for v, t in meshes:
        vs.append(np.asarray(v, dtype=np.float32))
        ts.append(np.asarray(t, dtype=np.int32) + off)
        off += len(v)
    return np.concatenate(vs), np.concatenate(ts)
