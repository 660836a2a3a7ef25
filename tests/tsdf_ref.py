"""Test infrastructure: restatements of TSDF fusion (csrc/cn_tsdf.hip), the observed-only mesher (cn_mesh.hip's
*_observed entry points) and the trilinear attribute sampler, from include/copenerf.h and independent of the HIP code.

fuse_ref is the yardstick: float64 numpy from the fp32 inputs, the integration rule of cn_tsdf_integrate per voxel
and view.  It also returns which voxels are *undecided*: a voxel is undecided for a view when a pixel coordinate
lies within DELTA pixels of a rounding boundary (the image's rim is one), when c lies within C_MARGIN, relative, of
`near`, or when |s + trunc| < C_MARGIN max(|c|, 1) at the pixel it reads -- there the kernel's fp32 rounding may
take the other branch -- and undecided if any view is.

fuse_f32 is NOT the yardstick and not the code under test: it restates the kernel's fp32 operation order in numpy
float32, so that the bound of the GPU tests can be measured on the CPU against fuse_ref (tests/test_tsdf_host.py
does, and pins the figures).  volume_sample_f32 does the same for the sampler.

isosurface_observed_ref: mesh_ref.isosurface's rules with NaN meaning unobserved -- an edge carries a vertex only
between two observed ends, a cell emits triangles only when its eight corners are observed -- in the same order."""
import numpy as np

import mesh_raster_ref as RR
import mesh_ref as MR

DELTA = 1e-3     # pixels
C_MARGIN = 1e-5  # relative
NEAR = 1e-4      # ops.MESH_NEAR

# The bound of the GPU tests on tsum.  F32_WORST is the worst |tsum32 - tsum64| of fuse_f32 -- the kernel's fp32
# operation order restated in numpy -- against fuse_ref at decided voxels (where the weights are equal) over every
# scene the GPU tests use, measured on the CPU (tests/test_tsdf_host.py measures it again and pins it): 3.53e-6,
# 3.64e-6 and 3.25e-6 on the three sphere cases, 3.83e-6 on the wall scene (2.71e-6 with depth_max).  It is the fp32
# voxel position and projection (a few 2^-24 of values near 2) divided by trunc = 0.12 and summed over up to six
# views.  The bound is four times that, the rasteriser test's precedent for a kernel whose rounding may differ from
# numpy's within the same operation order (division rounding).
F32_WORST = 3.9e-6
EPS_TSUM = 4.0 * F32_WORST
# the same for csum with colours in [0, 1]: 4.2e-7 (sums of up to six fp32 colours picked at equal pixels: the fp32
# restatement differs from float64 only by the roundings of the running sum)
F32_WORST_CSUM = 4.3e-7
EPS_CSUM = 4.0 * F32_WORST_CSUM
# ... and for the sampler over sample_volume / sample_points, values in [-1, 1]: 1.32e-6 without a mask, 6.26e-6 with
# one (the division by a weight sum as small as 0.047)
F32_WORST_SAMPLE = 6.4e-6
EPS_SAMPLE = 4.0 * F32_WORST_SAMPLE
SAMPLE_MIN_WEIGHT, SAMPLE_LEFT_OUT_CAP = 1e-3, 0.01
# The worst distance of a vertex of the float64 reference pipeline (fuse_ref, u = tsum / wsum, isosurface_observed_ref,
# mesh_clean_ref at min_triangles 1) from the radius-0.5 sphere on the first sphere case, measured by
# test_tsdf_host.py: the fused surface bends away from the sphere where views that see it at a grazing angle, or see
# past it, are averaged in.  The GPU pipeline's bar is 1.5 x this: the margin covers the fp32 volume moving a crossing
# along its edge.
PIPELINE_WORST = 0.0288
PIPELINE_BAR = 1.5 * PIPELINE_WORST
UNDECIDED_CAP = 0.05


def voxel_axes(dims, lo, hi, dtype):
    """Per axis X[i] = i / (n - 1) * (hi - lo) + lo in `dtype`, from the fp32 bounds."""
    f = dtype
    lo, hi = np.asarray(lo, dtype=np.float32).astype(f), np.asarray(hi, dtype=np.float32).astype(f)
    return [np.arange(n).astype(f) / f(n - 1) * (hi[a] - lo[a]) + lo[a] for a, n in enumerate(dims)]


def _fuse(dims, lo, hi, P, depth, trunc, near, depth_max, color, f):
    """The integration rule over all voxels at once in dtype f: (tsum, wsum, csum or None, undecided, observed)."""
    ax = voxel_axes(dims, lo, hi, f)
    x, y, z = np.meshgrid(*ax, indexing="ij")
    P = np.asarray(P, dtype=np.float32).astype(f)
    depth = np.asarray(depth, dtype=np.float32)
    N, h, w = depth.shape
    trunc, near, depth_max = (f(np.float32(v)) for v in (trunc, near, depth_max))
    tsum, wsum = np.zeros(dims, dtype=f), np.zeros(dims, dtype=f)
    csum = None if color is None else np.zeros(tuple(dims) + (3,), dtype=f)
    undecided = np.zeros(dims, dtype=bool)
    for v in range(N):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            a, b, c = (((P[v, r, 0] * x + P[v, r, 1] * y) + P[v, r, 2] * z) + P[v, r, 3] for r in range(3))
            front = c >= near
            sx, sy = a / c, b / c
            fx, fy = np.floor(sx + f(0.5)), np.floor(sy + f(0.5))
            inside = front & (fx >= 0) & (fx <= w - 1) & (fy >= 0) & (fy <= h - 1)
            px, py = np.where(inside, fx, 0).astype(np.int64), np.where(inside, fy, 0).astype(np.int64)
            d = depth[v][py, px].astype(f)
            valid = inside & np.isfinite(d) & (d > 0) & (d <= depth_max)
            s = d - c
            hit = valid & ~(s < -trunc)
            val = np.minimum(f(1.0), s / trunc)
            # what the kernel's rounding may decide the other way
            near_edge = (np.abs(sx + 0.5 - np.round(sx + 0.5)) <= DELTA) | (np.abs(sy + 0.5 - np.round(sy + 0.5)) <= DELTA)
            undecided |= (front & near_edge) | (np.abs(c - near) <= C_MARGIN * np.abs(c))
            undecided |= valid & (np.abs(s + trunc) < C_MARGIN * np.maximum(np.abs(c), 1.0))
        assert val.dtype == f
        tsum = tsum + np.where(hit, val, f(0.0))
        wsum = wsum + np.where(hit, f(1.0), f(0.0))
        if color is not None:
            col = np.asarray(color, dtype=np.float32)[v][py, px].astype(f)
            csum = csum + np.where(hit[..., None], col, f(0.0))
    assert tsum.dtype == f and wsum.dtype == f
    return tsum, wsum, csum, undecided


def fuse_ref(dims, lo, hi, P, depth, trunc, near=NEAR, depth_max=np.inf, color=None):
    """The yardstick, float64: (tsum, wsum, csum or None, undecided) over the views P [N, 3, 4] / depth [N, h, w]
    (the fp32 arrays the pass under test is given)."""
    return _fuse(dims, lo, hi, P, depth, trunc, near, depth_max, color, np.float64)


def fuse_f32(dims, lo, hi, P, depth, trunc, near=NEAR, depth_max=np.inf, color=None):
    """The kernel's operation order in numpy float32: (tsum, wsum, csum or None); from zero volumes."""
    return _fuse(dims, lo, hi, P, depth, trunc, near, depth_max, color, np.float32)[:3]


def compare_fusion(got_tsum, got_wsum, ref, eps=EPS_TSUM, cap=UNDECIDED_CAP):
    """The criteria of the fusion tests: at decided voxels wsum equals the reference's exactly and tsum lies within
    eps; at most `cap` of the voxels any view observes are undecided.  Returns (worst |tsum - ref| at decided voxels,
    the undecided share)."""
    tsum, wsum, _, undecided = ref
    observed = wsum > 0
    share = float((undecided & observed).sum()) / max(int(observed.sum()), 1)
    decided = ~undecided
    worst = float(np.abs(np.asarray(got_tsum, dtype=np.float64)[decided] - tsum[decided]).max())
    print("fusion: observed voxels", int(observed.sum()), "undecided share", share, "worst |tsum - ref|", worst, "bar", eps)
    assert share <= cap, share
    assert np.array_equal(np.asarray(got_wsum, dtype=np.float64)[decided], wsum[decided])
    assert worst <= eps, worst
    return worst, share


# ---- the observed-only mesher -----------------------------------------------------------------------------------

def isosurface_observed_ref(u, threshold, lo, hi):
    """(vertices float64 [V, 3], triangles int64 [T, 3]) of the fp32 volume u [nx, ny, nz], NaN = unobserved."""
    u = np.asarray(u)
    assert u.dtype == np.float32 and u.ndim == 3
    thr = np.float32(threshold)
    nx, ny, nz = u.shape
    dims = np.array([nx, ny, nz])
    lo = np.asarray(lo, dtype=np.float32).astype(np.float64)
    hi = np.asarray(hi, dtype=np.float32).astype(np.float64)
    obs = ~np.isnan(u)
    with np.errstate(invalid="ignore"):
        inside = u < thr  # strict; a NaN is outside (and unobserved)
    lin = np.arange(nx * ny * nz).reshape(nx, ny, nz)
    key_parts, pos_parts = [], []
    for slot in range(7):
        d = np.array([(slot + 1) & 1, (slot + 1) >> 1 & 1, (slot + 1) >> 2 & 1])
        sl_p = tuple(slice(0, n - dd) for n, dd in zip(dims, d))
        sl_q = tuple(slice(dd, n) for n, dd in zip(dims, d))
        cross = (inside[sl_p] != inside[sl_q]) & obs[sl_p] & obs[sl_q]
        p_lin = lin[sl_p][cross]
        up = u[sl_p][cross].astype(np.float64)
        uq = u[sl_q][cross].astype(np.float64)
        s = (float(thr) - up) / (uq - up)
        p = np.stack(np.unravel_index(p_lin, (nx, ny, nz)), axis=1).astype(np.float64)
        key_parts.append(p_lin * 7 + slot)
        pos_parts.append(p + s[:, None] * d[None, :])
    keys = np.concatenate(key_parts)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    pos = np.concatenate(pos_parts)[order]
    vertices = lo + pos / (dims - 1.0) * (hi - lo)
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    cell_lin = np.arange(cx * cy * cz).reshape(cx, cy, cz)
    cell_obs = np.ones((cx, cy, cz), dtype=bool)
    for o in range(8):
        c = (o & 1, o >> 1 & 1, o >> 2 & 1)
        cell_obs &= obs[c[0]:c[0] + cx, c[1]:c[1] + cy, c[2]:c[2] + cz]
    rows, sort_keys = [], []
    for k in range(6):
        C = MR.tet_corners(k)
        corner_in = [inside[c[0]:c[0] + cx, c[1]:c[1] + cy, c[2]:c[2] + cz] for c in C]
        corner_lin = [lin[c[0]:c[0] + cx, c[1]:c[1] + cy, c[2]:c[2] + cz] for c in C]
        mask = sum(ci.astype(np.int64) << i for i, ci in enumerate(corner_in))
        for m in range(1, 15):
            sel = (mask == m) & cell_obs
            if not sel.any():
                continue
            cells = cell_lin[sel]
            for ti, tri in enumerate(MR._triangles_of(k, m)):
                idx = []
                for a, b in tri:
                    a, b = min(a, b), max(a, b)
                    d = C[b] - C[a]
                    slot = d[0] + 2 * d[1] + 4 * d[2] - 1
                    key = corner_lin[a][sel] * 7 + slot
                    j = np.searchsorted(keys, key)
                    assert (keys[j] == key).all()
                    idx.append(j)
                rows.append(np.stack(idx, axis=1))
                sort_keys.append((cells * 6 + k) * 2 + ti)
    if rows:
        o = np.argsort(np.concatenate(sort_keys), kind="stable")
        triangles = np.concatenate(rows)[o]
    else:
        triangles = np.zeros((0, 3), dtype=np.int64)
    return vertices.reshape(-1, 3), triangles


def punch(u, how, seed=5):
    """u with NaN punched in: "half" (the half space x index >= 60 % of nx), "slab" (three x planes through the
    middle, through the surface) or "random" (a seeded 10 % of the voxels)."""
    u = np.array(u, dtype=np.float32, copy=True)
    nx, ny, nz = u.shape
    if how == "half":
        u[int(0.6 * nx):] = np.nan
    elif how == "slab":
        u[nx // 2 - 1:nx // 2 + 2] = np.nan
    elif how == "random":
        u[np.random.default_rng(seed).random(u.shape) < 0.1] = np.nan
    else:
        raise ValueError(how)
    return u


# ---- the sampler ---------------------------------------------------------------------------------------------------

def _sample(attr, points, lo, hi, mask, fill, f):
    attr = np.asarray(attr, dtype=np.float32)
    if attr.ndim == 3:
        attr = attr[..., None]
    dims = attr.shape[:3]
    lo, hi = np.asarray(lo, dtype=np.float32).astype(f), np.asarray(hi, dtype=np.float32).astype(f)
    pts = np.asarray(points, dtype=np.float32).astype(f)
    i0, fr = [], []
    for ax in range(3):
        n = dims[ax]
        g = (pts[:, ax] - lo[ax]) / (hi[ax] - lo[ax]) * f(n - 1)
        g = np.minimum(np.maximum(g, f(0.0)), f(n - 1))
        i = np.minimum(np.floor(g).astype(np.int64), n - 2)
        i0.append(i)
        fr.append(g - i.astype(f))
    acc = np.zeros((len(pts), attr.shape[3]), dtype=f)
    wsum = np.zeros(len(pts), dtype=f)
    for o in range(8):
        off = (o & 1, o >> 1 & 1, o >> 2 & 1)
        ix, iy, iz = (i0[ax] + off[ax] for ax in range(3))
        wt = ((fr[0] if off[0] else f(1.0) - fr[0]) * (fr[1] if off[1] else f(1.0) - fr[1])) * (fr[2] if off[2] else f(1.0) - fr[2])
        if mask is not None:
            wt = np.where(np.isnan(np.asarray(mask)[ix, iy, iz]), f(0.0), wt)
        wsum = wsum + wt
        acc = acc + wt[:, None] * np.where(wt[:, None] != 0, attr[ix, iy, iz].astype(f), f(0.0))
    assert acc.dtype == f
    if mask is None:
        return acc, wsum
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(wsum[:, None] > 0, acc / wsum[:, None], f(np.float32(fill)))
    return out, wsum


def volume_sample_ref(attr, points, lo, hi, mask=None, fill=0.0):
    """The yardstick, float64: (out [Q, C], the sum of the observed corners' weights [Q])."""
    return _sample(attr, points, lo, hi, mask, fill, np.float64)


def volume_sample_f32(attr, points, lo, hi, mask=None, fill=0.0):
    """The kernel's operation order in numpy float32: out [Q, C]."""
    return _sample(attr, points, lo, hi, mask, fill, np.float32)[0]


def sample_volume(dims=(9, 7, 11), C=3, seed=2):
    """(attr fp32 [nx, ny, nz, C] in [-1, 1], mask fp32 [nx, ny, nz] with one fully unobserved cell at the low corner
    and a scattered 10 % of NaN, lo, hi)."""
    rng = np.random.default_rng(seed)
    attr = rng.uniform(-1, 1, tuple(dims) + (C,)).astype(np.float32)
    mask = rng.uniform(-1, 1, dims).astype(np.float32)
    mask[rng.random(dims) < 0.1] = np.nan
    mask[:2, :2, :2] = np.nan
    return attr, mask, (-0.7, -1.0, 0.1), (0.9, 0.4, 1.3)


def sample_points(lo, hi, dims, n=700, seed=4):
    """Points inside the box, on its faces, on grid points and outside it (clamped): fp32 [n + 144, 3]."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    inside = lo + rng.random((n, 3)) * (hi - lo)
    faces = lo + rng.random((60, 3)) * (hi - lo)
    k = np.arange(60)
    faces[k, k % 3] = np.where((k % 2)[:, None], hi, lo)[k, k % 3]
    outside = lo + (rng.random((60, 3)) * 1.6 - 0.3) * (hi - lo)
    step = (hi - lo) / (np.asarray(dims) - 1)
    planes = lo + rng.integers(0, np.asarray(dims), (24, 3)) * step
    return np.concatenate([inside, faces, outside, planes]).astype(np.float32)


def unobserved_points(lo, hi, dims, n=40, seed=6):
    """Points strictly inside sample_volume's fully unobserved cell: no observed corner, the sampler's `fill`."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    step = (hi - lo) / (np.asarray(dims) - 1)
    return (lo + (0.05 + 0.9 * np.random.default_rng(seed).random((n, 3))) * step).astype(np.float32)


# ---- scenes ------------------------------------------------------------------------------------------------------------

def projections(views, h, w):
    """mesh.camera_projection of every view, restated: fp32 [N, 3, 4]."""
    out = []
    for v in views:
        M = np.asarray(v["camera_mat"], dtype=np.float64) @ np.asarray(v["world_mat"], dtype=np.float64)
        if v.get("scale_mat") is not None:
            M = M @ np.asarray(v["scale_mat"], dtype=np.float64)
        out.append(np.stack([0.5 * (w - 1) * (M[0] + M[2]), 0.5 * (h - 1) * (M[1] + M[2]), M[2]]))
    return np.stack(out).astype(np.float32)


def _rays(P, h, w):
    """Per pixel the ray X = o + d r with d the depth c: (o [3], r [h, w, 3]) of one projection (float64)."""
    P = np.asarray(P, dtype=np.float64)
    Ai = np.linalg.inv(P[:, :3])
    py, px = np.mgrid[0:h, 0:w].astype(np.float64)
    r = np.stack([px, py, np.ones_like(px)], -1) @ Ai.T
    return -Ai @ P[:, 3], r


def _sphere_depth(o, r, centre, radius):
    oc = o - np.asarray(centre, dtype=np.float64)
    A = (r * r).sum(-1)
    B = 2.0 * (r @ oc)
    C = oc @ oc - radius * radius
    disc = B * B - 4 * A * C
    with np.errstate(invalid="ignore"):
        d = (-B - np.sqrt(disc)) / (2 * A)
    return np.where((disc > 0) & (d > 0), d, np.inf)


def render_sphere(P, h, w, centre=(0.0, 0.0, 0.0), radius=0.5, empty=np.inf):
    """The analytic depth (camera_projection's c) of a sphere from the views P [N, 3, 4]: fp32 [N, h, w], `empty`
    where the ray misses."""
    out = []
    for Pv in P:
        o, r = _rays(Pv, h, w)
        d = _sphere_depth(o, r, centre, radius)
        out.append(np.where(np.isfinite(d), d, empty))
    return np.stack(out).astype(np.float32)


def six_views(h, w):
    return RR.three_views(h, w) + RR.side_views(h, w)


BOX = ((-0.8, -0.8, -0.8), (0.8, 0.8, 0.8))
TRUNC = 0.12
# (dims, (h, w)): the issue's cubic case, the odd-sized one, and a finer image
SPHERE_CASES = (((40, 40, 40), (48, 64)), ((24, 17, 29), (23, 37)), ((33, 33, 33), (64, 96)))


def scene_sphere(dims, hw):
    """(dims, lo, hi, P fp32 [6, 3, 4], depth fp32 [6, h, w] (+inf where nothing is seen), trunc, views)."""
    h, w = hw
    views = six_views(h, w)
    P = projections(views, h, w)
    return dims, BOX[0], BOX[1], P, render_sphere(P, h, w), TRUNC, views


WALL_X, WALL_SPHERE = -0.55, ((0.1, 0.0, 0.0), 0.35)


def scene_wall(h=48, w=64, dims=(32, 32, 32)):
    """A sphere in front of the wall x = WALL_X, seen by the three side cameras: (dims, lo, hi, P, depth, trunc,
    depth_sphere (+inf off the sphere), depth_wall, depth_max between the two)."""
    views = RR.side_views(h, w)
    P = projections(views, h, w)
    ds = render_sphere(P, h, w, *WALL_SPHERE)
    dw = []
    for Pv in P:
        o, r = _rays(Pv, h, w)
        with np.errstate(divide="ignore"):
            d = (WALL_X - o[0]) / r[..., 0]
        dw.append(np.where(d > 0, d, np.inf))
    dw = np.stack(dw).astype(np.float32)
    depth = np.minimum(ds, dw)
    far_sphere, near_wall = float(ds[np.isfinite(ds)].max()), float(dw.min())
    assert far_sphere < near_wall, (far_sphere, near_wall)
    return dims, BOX[0], BOX[1], P, depth, TRUNC, ds, dw, 0.5 * (far_sphere + near_wall)


def pixel_colors(N, h, w):
    """A smooth colour per pixel and view in [0, 1]: fp32 [N, h, w, 3]."""
    py, px = np.mgrid[0:h, 0:w].astype(np.float64)
    out = [np.stack([0.5 + 0.5 * np.sin(0.11 * px + 0.07 * py + v), 0.5 + 0.5 * np.cos(0.05 * px - 0.13 * py + 2 * v),
                     0.5 * (px / w + py / h) * (1.0 - 0.1 * v)], -1) for v in range(N)]
    return np.stack(out).astype(np.float32)
