"""The cases of tests/test_gpu_ray_kernels.py, shared with tests/test_ray_ref.py (which asserts the reference-only
properties -- exclusion caps, the oracle passing its own bars -- on exactly these inputs, without a GPU).
Everything is seeded, fp32 and on the CPU; the references are computed once per case and cached."""
from __future__ import annotations

import functools
import zlib

import torch

import ray_ref as RR

R = 7  # one full block of 4 rays and a ragged one

# compositing
COMP_S = [1, 2, 63, 64, 65, 129, 193, 256]
COMP_INV_S = [20.0, 200.0, 1000.0]
COMP_CAR = [0.0, 0.3, 1.0]
KINK = 1e-4          # |d.n| or |d.n - 1| below this: the sample's gradient is left out
KINK_CAP = 0.01      # at most this share of a case's samples
BWD_SETS = [("dcolor",), ("ddepth",), ("dweights",), ("dcdf",), RR.COTANGENTS]

# up-sampling
UP_N = [2, 3, 17, 64, 65, 66, 129, 130, 193, 240]
UP_NIMP = [1, 2, 15, 16, 63, 64]
UP_INV_S = [64.0, 256.0, 1024.0]
UP_KINDS = ["plain", "dup", "empty"]

# per-point kernels
POINT_M = [1, 37, 64, 65, 300]


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def up_pairs():
    return [(n, k) for n in UP_N for k in UP_NIMP if n + k <= 256]


@functools.lru_cache(maxsize=None)
def composite_case(S, inv_s, car):
    """R = 7 rays: 0-4 cross the surface (0, 1, 4 with a noisy sdf somewhere inside, 2 right after the first sample, 3
    right before the last), 5 is empty (sdf > 0.5), 6 is a steep noise-free crossing (saturated at inv_s = 1000).
    Normals are Gaussian, not unit; the first min(3, S) samples of every ray are
    planted with d.n = 1.5, 0.5 and -0.7 (rotated by ray, so every relu branch runs at S = 1 too), each at least
    0.3 from a kink."""
    g = _gen("comp", S, inv_s, car)
    z = torch.sort(torch.rand(R, S, generator=g) * 2.5 + 0.1, -1)[0]
    cross = 0.6 + 1.4 * torch.rand(R, 1, generator=g)
    sdf = (cross - z) + 0.05 * torch.randn(R, S, generator=g)
    if S >= 2:  # rays 2 and 3 cross between their first / their last two samples: the weight, and with it the
        # backward's suffix sum, sits in the first / the last lane's chunk
        sdf[2] = 0.5 * (z[2, 0] + z[2, 1]) - z[2]
        sdf[3] = 0.5 * (z[3, -2] + z[3, -1]) - z[3]
    sdf[5] = 0.6 + 0.2 * torch.rand(S, generator=g)
    sdf[6] = 3.0 * (cross[6] - z[6])
    rays_d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    normals = 1.3 * torch.randn(R, S, 3, generator=g)
    targets = [1.5, 0.5, -0.7]
    for r in range(R):
        for j in range(min(3, S)):
            d = rays_d[r]
            o = torch.randn(3, generator=g)
            o = o - (o @ d) * d / (d @ d)
            normals[r, j] = targets[(r + j) % 3] * d / (d @ d) + 0.4 * o
    M = R * S
    return dict(S=S, inv_s=inv_s, car=car, z=z, sdf=sdf.reshape(M, 1).contiguous(), normals=normals.reshape(M, 3),
                flow=torch.randn(M, 1, generator=g), rgb=torch.rand(M, 3, generator=g), rays_d=rays_d,
                near=torch.full((R, 1), 0.1), far=torch.full((R, 1), 2.6), n_coarse=64,
                dcolor=torch.randn(R, 3, generator=g), ddepth=torch.randn(R, 1, generator=g),
                dweights=torch.randn(R, S, generator=g), dcdf=torch.randn(R, S, generator=g))


@functools.lru_cache(maxsize=None)
def composite_refs(S, inv_s, car, which):
    """(float64, float32) ray_ref.composite_all of a case for one set of cotangents."""
    c = composite_case(S, inv_s, car)
    return RR.composite_all(c, torch.float64, which), RR.composite_all(c, torch.float32, which)


def kink_mask(tc64):
    """Samples kept in the gradient checks: float64 d.n further than KINK from 0 and from 1."""
    return (tc64.abs() > KINK) & ((tc64 - 1.0).abs() > KINK)


def composite_bar(ref64, ref32, keep=None):
    """4 max|oracle32 - ref64| + 4 * 2^-24 max|ref64| over the kept elements."""
    a, b = ref64.double(), ref32.double()
    if keep is not None:
        a, b = a[keep], b[keep]
    if a.numel() == 0:
        return 0.0
    return 4.0 * (a - b).abs().max().item() + 4.0 * RR.U * a.abs().max().item()


@functools.lru_cache(maxsize=None)
def up_case(n, inv_s, kind):
    """R = 7 rays of n sorted samples.  plain: a surface crossing.  dup: the same with two duplicated z (zero-width
    bins); its odd rays are empty as well, so the uniform pdf puts new samples into those bins and the merge sees
    ties.  empty: sdf > 0.5 everywhere."""
    g = _gen("up", n, inv_s, kind)
    z = torch.sort(torch.rand(R, n, generator=g) * 2.5 + 0.1, -1)[0]
    cross = 0.6 + 1.4 * torch.rand(R, 1, generator=g)
    sdf = (cross - z) + 0.02 * torch.randn(R, n, generator=g)
    empty = 0.6 + 0.2 * torch.rand(R, n, generator=g)
    if kind == "empty":
        sdf = empty
    if kind == "dup":
        sdf[1::2] = empty[1::2]
        for a in sorted({n // 3, (2 * n) // 3}):
            if a + 1 < n:
                z[:, a + 1] = z[:, a]
    return z.contiguous(), sdf.contiguous()


@functools.lru_cache(maxsize=None)
def up_ref32(n, n_imp, inv_s, kind):
    z, sdf = up_case(n, inv_s, kind)
    return RR.up_sample(z, sdf, n_imp, inv_s, torch.float32)


def point_inputs(M, cols, seed, lo=-1.0, hi=1.0):
    g = _gen("pt", M, cols, seed)
    return torch.rand(M, cols, generator=g) * (hi - lo) + lo


# ---------------------------------------------------------------------------
# per-point kernels: every op is (inputs, ref(dtype) -> {name: tensor}, bars -> {name: tensor}); the CPU test
# holds ray_ref at float32 to the bars, the GPU test the kernels.  The bars come from the number formats alone:
#   sin / cos outputs   4 max|CPU fp32 sin / cos - float64| on the same arguments + 2^-23, absolute
#   products and sums   2 * 2^-24 x the sum of the absolute values of the terms
#   reductions          the same, times the number of terms
# plus 2^-40 of the same sum for the second-order terms and the float64 reference's own rounding.
U2 = 2.0 * RR.U
SLACK = 2.0 ** -40


def sincos_bar(args32):
    a = args32.reshape(-1)
    if a.numel() == 0:
        return 2.0 ** -23
    e = max((torch.sin(a).double() - torch.sin(a.double())).abs().max().item(),
            (torch.cos(a).double() - torch.cos(a.double())).abs().max().item())
    return 4.0 * e + 2.0 ** -23


def embed_op(M, multires, scale, kpad):
    x = point_inputs(M, 4, ("embed", multires, scale), -1.5, 1.5)
    args, xs = RR.embed_args(x, multires, scale)
    bar = torch.zeros(M, kpad, dtype=torch.float64)
    bar[:, :4] = (U2 + SLACK) * xs.double().abs()
    bar[:, 4:4 * (1 + 2 * multires)] = sincos_bar(args)
    return dict(x=x), lambda dt: {"U0": RR.embed(x, multires, scale, kpad, dt)}, {"U0": bar}


def _u0(M, multires, kpad, seed):
    return RR.embed(point_inputs(M, 4, ("u0", seed), -1.5, 1.5), multires, 1.0, kpad, torch.float32)


def tangent_op(M, multires, scale, kpad):
    U0 = _u0(M, multires, kpad, "tan")
    v = point_inputs(M, 4, ("v", multires), -2.0, 2.0)
    ref64 = RR.tangent(U0, v, multires, scale, kpad, torch.float64)
    # v scale, then (2^k exact) one product with the stored sin / cos: two rounded operations
    return dict(U0=U0, v=v), lambda dt: {"T0": RR.tangent(U0, v, multires, scale, kpad, dt)}, \
        {"T0": (U2 + SLACK) * ref64.abs()}


def assemble_op(M, multires, scale, with_qe):
    kpad = 64
    U0 = _u0(M, multires, kpad, "asm")
    Q0 = point_inputs(M, kpad, ("q0", multires))
    QE = point_inputs(M, kpad, ("qe", multires)) if with_qe else None
    _, ab = RR.grad_assemble(U0, Q0, QE, multires, scale, torch.float64)
    nterms = 1 + 2 * multires
    return dict(U0=U0, Q0=Q0, QE=QE), lambda dt: {"G": RR.grad_assemble(U0, Q0, QE, multires, scale, dt)[0]}, \
        {"G": (U2 * nterms + SLACK) * ab}


def extras_op(M, dir_div, multires_view, kpad):
    nr = -(-M // dir_div)
    G = point_inputs(M, 4, ("xg", dir_div))
    pts = point_inputs(M, 4, ("xp", dir_div))
    dirs = torch.nn.functional.normalize(point_inputs(nr, 3, ("xd", dir_div, multires_view)), dim=-1)
    bar = torch.zeros(M, kpad, dtype=torch.float64)  # the copied columns and the padding are exact
    bar[:, 11:11 + 6 * multires_view] = sincos_bar(RR.view_args(dirs, multires_view))
    return dict(G=G, pts=pts, dirs=dirs), \
        lambda dt: {"ext": RR.color_extras(G, pts, dirs, dir_div, multires_view, kpad, dt)}, {"ext": bar}


def extras_bwd_op(Rr, rows, multires_view, accumulate):
    ld = 8 + 3 + 6 * multires_view
    d_ext = point_inputs(Rr * rows, ld, ("xb", rows, multires_view))
    dirs = torch.nn.functional.normalize(point_inputs(Rr, 3, ("xbd", rows, multires_view)), dim=-1)
    prev = point_inputs(Rr, 3, ("xbp", rows)) if accumulate else None
    _, gabs, trig = RR.color_extras_bwd(d_ext, dirs, rows, multires_view, torch.float64)
    nterms = rows * (1 + 2 * multires_view) + (1 if accumulate else 0)
    if accumulate:
        gabs = gabs + prev.double().abs()
    bar = (U2 * nterms + SLACK) * gabs + sincos_bar(RR.view_args(dirs, multires_view)) * trig

    def ref(dt):
        g = RR.color_extras_bwd(d_ext, dirs, rows, multires_view, dt)[0]
        return {"ddirs": g + prev.to(dt) if accumulate else g}
    return dict(d_ext=d_ext, dirs=dirs, prev=prev), ref, {"ddirs": bar}


def _near_far(Rr, seed):
    near = 0.1 + 0.5 * (point_inputs(Rr, 1, ("near", seed)) + 1.0)
    far = near + 1.0 + (point_inputs(Rr, 1, ("far", seed)) + 1.0)
    return near, far


def coarse_z_op(n, jitter):
    near, far = _near_far(R, n)
    t_rand = (point_inputs(R, n, ("trand", n)) + 1.0) * 0.5 if jitter else None
    lin = RR.linspace01(n).double()
    A = near.double().abs() * (1.0 - lin[None, :]) + far.double().abs() * lin[None, :]
    if jitter:
        mids = 0.5 * (A[:, 1:] + A[:, :-1])
        upper, lower = torch.cat([mids, A[:, -1:]], -1), torch.cat([A[:, :1], mids], -1)
        A = lower + (upper + lower) * t_rand.double()
    return dict(near=near, far=far, t_rand=t_rand), lambda dt: {"z": RR.coarse_z(near, far, n, t_rand, dt)}, \
        {"z": (U2 + SLACK) * A}


def _rays(seed):
    o = 0.4 * point_inputs(R, 3, ("ro", seed))
    d = torch.nn.functional.normalize(point_inputs(R, 3, ("rd", seed)), dim=-1)
    return o, d


def points_op(n, mid):
    o, d = _rays(n)
    near, far = _near_far(R, ("p", n))
    z = torch.sort((point_inputs(R, n, ("pz", n)) + 1.0) * 1.25 + 0.1, -1)[0].contiguous()
    t = torch.tensor([-0.3])
    n_coarse = 64
    zz = RR.mid_z(z, RR.sample_dist(near, far, n_coarse)) if mid else z  # fp32, as the kernel forms it
    bar = torch.zeros(R * n, 4, dtype=torch.float64)  # the time column is a copy
    bar[:, :3] = (U2 + SLACK) * RR.points_abs(o, d, zz)
    return dict(o=o, d=d, z=z, t=t, near=near, far=far, n_coarse=n_coarse, zz=zz), \
        lambda dt: {"pts": RR.points(o, d, zz, t, dt)}, {"pts": bar}


def points_bwd_op(n, mid, ld_p):
    near, far = _near_far(R, ("pb", n))
    z = torch.sort((point_inputs(R, n, ("pbz", n)) + 1.0) * 1.25 + 0.1, -1)[0].contiguous()
    dP = point_inputs(R * n, ld_p, ("pbd", n, ld_p))
    n_coarse = 64
    zz = RR.mid_z(z, RR.sample_dist(near, far, n_coarse)) if mid else z
    _, _, ao, ad = RR.points_bwd(zz, dP, torch.float64)

    def ref(dt):
        a, b, _, _ = RR.points_bwd(zz, dP, dt)
        return {"drays_o": a, "drays_d": b}
    return dict(z=z, dP=dP, near=near, far=far, n_coarse=n_coarse), ref, \
        {"drays_o": (U2 * n + SLACK) * ao, "drays_d": (U2 * n + SLACK) * ad}


def min_embed_kpad(multires):
    return 4 * (1 + 2 * multires)


def min_extras_kpad(multires_view):
    return (8 + 3 + 6 * multires_view + 3) // 4 * 4


def check_op(got, ref64, bars, label):
    """max error-to-bar ratio per output of a per-point op (exact where the bar is 0); asserts ratio <= 1."""
    worst = {}
    for k, bar in bars.items():
        err = (got[k].double() - ref64[k].double()).abs()
        exact = bar == 0
        assert bool((err[exact] == 0).all()), (label, k, "exact columns differ", err[exact].max().item())
        ratio = (err[~exact] / bar[~exact]).max().item() if bool((~exact).any()) else 0.0
        worst[k] = ratio
        assert ratio <= 1.0, (label, k, ratio)
    return worst
