"""The per-ray and per-point kernels' contract as plain torch functions, generic in dtype.

Each function restates one operation exactly as oracle/neus_oracle.py and the kernels' comments
(csrc/cn_render.hip, csrc/cn_fields.hip) state it, on the CPU, in the dtype it is given: float32 is the
oracle's own arithmetic (tests/test_ray_ref.py pins it bitwise to oracle.neus_oracle), float64 is the value
the kernels are judged against (tests/test_gpu_ray_kernels.py).  Inputs are fp32 tensors and are cast
first, so both runs start from the same bits.  Where the kernel forms a quantity in fp32 that the CPU forms
exactly the same way (the inverse-cdf abscissae u, linspace, the sin / cos arguments fl(fl(x scale) 2^k),
the midpoint z + dist / 2) the float64 run takes that fp32 quantity, so what is left to compare is the
arithmetic after it."""
from __future__ import annotations

import torch
import torch.nn.functional as F

U = 2.0 ** -24  # half a last place of fp32: the relative error of one rounded operation


def f32(x):
    """A host scalar as the kernel receives it: rounded to fp32."""
    return float(torch.tensor(x, dtype=torch.float32))


# ---------------------------------------------------------------------------
# sampling
def exclusive_cumprod(a):
    ones = torch.ones_like(a[:, :1])
    return torch.cumprod(torch.cat([ones, 1.0 - a + 1e-7], -1), -1)[:, :-1]


def linspace_u(n_imp):
    """u_k of sample_pdf(det=True), formed in fp32 (the kernel's linspace is torch's CPU one)."""
    return torch.linspace(0.5 / n_imp, 1.0 - 0.5 / n_imp, steps=n_imp)


def up_sample_weights(z, sdf, inv_s, dtype):
    """cdf [R, n] (leading 0) of the NeuS up-sampling weights between consecutive samples."""
    z, sdf = z.to(dtype), sdf.to(dtype)
    R = z.shape[0]
    s0, s1 = sdf[:, :-1], sdf[:, 1:]
    z0, z1 = z[:, :-1], z[:, 1:]
    mid = (s0 + s1) * 0.5
    cosv = (s1 - s0) / (z1 - z0 + 1e-5)
    prev = torch.cat([torch.zeros(R, 1, dtype=dtype), cosv[:, :-1]], -1)
    cosv = torch.min(torch.stack([prev, cosv], -1), -1)[0].clip(-1e3, 0.0)
    dist = z1 - z0
    pe = mid - cosv * dist * 0.5
    ne = mid + cosv * dist * 0.5
    pc, nc = torch.sigmoid(pe * inv_s), torch.sigmoid(ne * inv_s)
    alpha = (pc - nc + 1e-5) / (pc + 1e-5)
    w = alpha * exclusive_cumprod(alpha) + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    return torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, -1)], -1)


def invert_cdf(z, cdf, u):
    """sample_pdf's inverse: the bin of searchsorted(right=True), linear inside it, denom < 1e-5 -> 1.
    Returns (z_new, bin mass c_hi - c_lo, the denom -> 1 rule's value)."""
    u = u.to(cdf.dtype).expand(cdf.shape[0], u.shape[-1]).contiguous()
    idx = torch.searchsorted(cdf, u, right=True)
    lo = (idx - 1).clamp(min=0)
    hi = idx.clamp(max=cdf.shape[-1] - 1)
    c_lo, c_hi = torch.gather(cdf, 1, lo), torch.gather(cdf, 1, hi)
    b_lo, b_hi = torch.gather(z, 1, lo), torch.gather(z, 1, hi)
    mass = c_hi - c_lo
    den = torch.where(mass < 1e-5, torch.ones_like(mass), mass)
    return b_lo + (u - c_lo) / den * (b_hi - b_lo), mass, b_lo + (u - c_lo) * (b_hi - b_lo)


def up_sample(z, sdf, n_imp, inv_s, dtype):
    """(z_new [R, n_imp], cdf [R, n], u [n_imp] fp32): one up-sampling round at a fixed inv_s."""
    cdf = up_sample_weights(z, sdf, inv_s, dtype)
    u = linspace_u(n_imp)
    return invert_cdf(z.to(dtype), cdf, u)[0], cdf, u


def merge(z, z_new, sdf=None):
    """The stable merge of cat_z_vals: old samples before new ones on ties, new ones among themselves in index
    order.  Returns (z_out [R, n + k], new_dst [R, k] flat positions r (n + k) + p, old_pos [R, n], sdf_out with
    NaN at the new samples' slots or None)."""
    R, n = z.shape
    k = z_new.shape[1]
    zc, idx = torch.sort(torch.cat([z, z_new], -1), dim=-1, stable=True)
    pos = torch.empty_like(idx)
    pos.scatter_(1, idx, torch.arange(n + k).expand(R, n + k).contiguous())
    old_pos, new_pos = pos[:, :n], pos[:, n:]
    new_dst = new_pos + torch.arange(R)[:, None] * (n + k)
    sdf_out = None
    if sdf is not None:
        sdf_out = torch.full((R, n + k), float("nan"), dtype=sdf.dtype)
        sdf_out.scatter_(1, old_pos, sdf)
    return zc, new_dst, old_pos, sdf_out


def cdf_interval(z, cdf, u, tol_cdf):
    """[z_lo, z_hi]: the lowest preimage of u - tol_cdf and the highest of u + tol_cdf under the piecewise-linear
    cdf over the bins (float64; zero-width bins are jumps, flat stretches are intervals)."""
    R, n = cdf.shape
    u = u.to(cdf.dtype).expand(R, u.shape[-1]).contiguous()
    top = cdf[:, -1:]

    def interp(v, j):  # inside bin (j - 1, j), 1 <= j <= n - 1
        c0, c1 = torch.gather(cdf, 1, j - 1), torch.gather(cdf, 1, j)
        b0, b1 = torch.gather(z, 1, j - 1), torch.gather(z, 1, j)
        den = c1 - c0
        t = torch.where(den > 0, (v - c0) / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(den))
        return b0 + t.clamp(0.0, 1.0) * (b1 - b0)

    v = torch.minimum((u - tol_cdf).clamp(min=0.0), top)
    j = torch.searchsorted(cdf, v, right=False)  # first cdf[j] >= v
    z_lo = torch.where(j == 0, z[:, :1].expand_as(v), interp(v, j.clamp(1, n - 1)))
    v = torch.minimum((u + tol_cdf).clamp(min=0.0), top)
    j = torch.searchsorted(cdf, v, right=True)  # first cdf[j] > v
    z_hi = torch.where(j >= n, z[:, -1:].expand_as(v), interp(v, j.clamp(1, n - 1)))
    return z_lo, z_hi


def z_new_ok(z_new, z, sdf, n_imp, inv_s, cdf32):
    """The value check of an up-sampling launch: (ok [R, n_imp] bool, tol_cdf, samples in the ambiguous band).
    tol_cdf = 4 max|cdf32 - cdf64| + 8 * 2^-24, tol_z = 4 * 2^-24 |z|; a sample passes inside
    [z_lo - tol_z, z_hi + tol_z]; where the float64 bin mass is below 1e-5 - 1e-6 it is held to the denom -> 1
    rule's value instead, and within 1e-6 of 1e-5 either rule passes."""
    z64 = z.double()
    cdf64 = up_sample_weights(z, sdf, inv_s, torch.float64)
    u = linspace_u(n_imp)
    tol_cdf = 4.0 * (cdf32.double() - cdf64).abs().max().item() + 8.0 * U
    zn = z_new.double()
    tol_z = 4.0 * U * zn.abs()
    z_lo, z_hi = cdf_interval(z64, cdf64, u, tol_cdf)
    normal = (zn >= z_lo - tol_z) & (zn <= z_hi + tol_z)
    _, mass, rule_val = invert_cdf(z64, cdf64, u)
    width = (z64[:, -1:] - z64[:, :1])
    rule = (zn - rule_val).abs() <= tol_cdf * width + tol_z
    small, band = mass < 1e-5 - 1e-6, (mass - 1e-5).abs() <= 1e-6
    ok = torch.where(small, rule, torch.where(band, normal | rule, normal))
    return ok, tol_cdf, int(band.sum())


# ---------------------------------------------------------------------------
# points
def linspace01(n):
    """linspace(0, 1, n) in fp32 by torch's scalar formula with every operation rounded (the kernel's linspace01,
    built without FMA contraction).  torch's vectorised CPU kernel fuses end - step k, so for n >= 16 a few
    elements of torch.linspace differ from this by one fp32 step."""
    if n == 1:
        return torch.zeros(1)
    step = torch.tensor(1.0) / torch.tensor(float(n - 1))
    i = torch.arange(n, dtype=torch.float32)
    return torch.where(i < n // 2, step * i, 1.0 - step * (n - i - 1.0))


def coarse_z(near, far, n, t_rand, dtype):
    lin = linspace01(n).to(dtype)  # fp32, as the kernel forms it
    near, far = near.to(dtype), far.to(dtype)
    z = near * (1.0 - lin[None, :]) + far * lin[None, :]
    if t_rand is not None:
        mids = 0.5 * (z[..., 1:] + z[..., :-1])
        upper = torch.cat([mids, z[..., -1:]], -1)
        lower = torch.cat([z[..., :1], mids], -1)
        z = lower + (upper - lower) * t_rand.to(dtype)
    return z


def sample_dist(near, far, n_coarse):
    """(far[0] - near[0]) / n_coarse in fp32: the last sample's interval."""
    return (far.reshape(-1)[0] - near.reshape(-1)[0]) / n_coarse


def dists(z, sd):
    return torch.cat([z[..., 1:] - z[..., :-1], sd.to(z.dtype).reshape(1, 1).expand(z.shape[0], 1)], -1)


def mid_z(z, sd):
    """z + dist / 2 in z's dtype (render_core's section midpoints)."""
    return z + dists(z, sd) * 0.5


def points(rays_o, rays_d, zz, t, dtype):
    """[R n, 4]: o + d zz and the time."""
    p = (rays_o.to(dtype)[:, None, :] + rays_d.to(dtype)[:, None, :] * zz.to(dtype)[..., None]).reshape(-1, 3)
    return torch.cat([p, t.to(dtype).reshape(1, 1).expand(p.shape[0], 1)], -1)


def points_abs(rays_o, rays_d, zz):
    """sum of the absolute values of the terms of points' xyz, float64."""
    return (rays_o.double().abs()[:, None, :] + (rays_d.double()[:, None, :] * zz.double()[..., None]).abs()).reshape(-1, 3)


def points_bwd(zz, dP, dtype):
    """(drays_o, drays_d, sum |terms| of each) [R, 3]: sums over a ray's samples of dP and dP zz."""
    R, n = zz.shape
    g = dP.to(dtype).reshape(R, n, -1)[..., :3]
    t = g * zz.to(dtype)[..., None]
    return g.sum(1), t.sum(1), g.abs().sum(1), t.abs().sum(1)


# ---------------------------------------------------------------------------
# encodings
def embed_args(x, multires, scale):
    """fl(fl(x scale) 2^k) [M, L, 4] in fp32, as the kernel forms the sin / cos arguments, and fl(x scale)."""
    xs = x.float() * torch.tensor(scale, dtype=torch.float32)
    f = 2.0 ** torch.arange(multires, dtype=torch.float32)
    return xs[:, None, :] * f[None, :, None], xs


def embed(x, multires, scale, kpad, dtype):
    """[M, kpad]: groups of 4 columns x', sin(2^k x'), cos(2^k x'), ..., zero padding."""
    args, xs = embed_args(x, multires, scale)
    a = args.to(dtype)
    parts = [xs.to(dtype)]
    for k in range(multires):
        parts += [torch.sin(a[:, k]), torch.cos(a[:, k])]
    e = torch.cat(parts, -1)
    return F.pad(e, (0, kpad - e.shape[1]))


def _jac_rows(U0, multires):
    """Per group g >= 1 the factor d enc_g / d x' [M, 4] taken from the stored encoding U0: 2^k cos for a sin
    group (the next group), -2^k sin for a cos group (the previous one)."""
    out = []
    for g in range(1, 1 + 2 * multires):
        k, is_sin = (g - 1) >> 1, ((g - 1) & 1) == 0
        tr = U0[:, 4 * (g + 1):4 * (g + 2)] if is_sin else -U0[:, 4 * (g - 1):4 * g]
        out.append((tr, float(1 << k)))
    return out


def tangent(U0, v, multires, scale, kpad, dtype):
    """T0 [M, kpad]: the tangent of the encoding along v, J_g(x') (scale v)."""
    U0, xd = U0.to(dtype), v.to(dtype) * f32(scale)
    parts = [xd] + [tr * (xd * f) for tr, f in _jac_rows(U0, multires)]
    t = torch.cat(parts, -1)
    return F.pad(t, (0, kpad - t.shape[1]))


def grad_assemble(U0, Q0, QE, multires, scale, dtype):
    """(G [M, 4], sum |terms|): scale * sum_g J_g^T (Q0 + QE)[g]."""
    ng = 1 + 2 * multires
    U0, scale = U0.to(dtype), f32(scale)
    de = Q0.to(dtype)[:, :4 * ng] + (QE.to(dtype)[:, :4 * ng] if QE is not None else 0.0)
    terms = [de[:, :4]] + [de[:, 4 * g:4 * g + 4] * tr * f for g, (tr, f) in enumerate(_jac_rows(U0, multires), 1)]
    t = torch.stack(terms, 0)
    ab = (Q0.to(dtype)[:, :4 * ng].abs() + (QE.to(dtype)[:, :4 * ng].abs() if QE is not None else 0.0))
    jac = [torch.ones_like(ab[:, :4])] + [tr.abs() * f for tr, f in _jac_rows(U0, multires)]
    ta = torch.stack([ab[:, 4 * g:4 * g + 4] * j for g, j in enumerate(jac)], 0)
    return t.sum(0) * scale, ta.sum(0) * abs(scale)


def view_args(dirs, multires_view):
    """fl(d 2^k) [R, L, 3] in fp32."""
    f = 2.0 ** torch.arange(multires_view, dtype=torch.float32)
    return dirs.float()[:, None, :] * f[None, :, None]


def view_embed(dirs, multires_view, dtype):
    """[R, 3 + 6 L]: d, sin(2^k d) (3), cos(2^k d) (3), ..."""
    a = view_args(dirs, multires_view).to(dtype)
    parts = [dirs.to(dtype)]
    for k in range(multires_view):
        parts += [torch.sin(a[:, k]), torch.cos(a[:, k])]
    return torch.cat(parts, -1)


def color_extras(G, pts, dirs, dir_div, multires_view, kpad, dtype):
    """[M, kpad]: rows [g(4) | pts_time(4) | view encoding of the row's ray m // dir_div | 0...]."""
    M = G.shape[0]
    ray = torch.arange(M) // dir_div
    e = torch.cat([G.to(dtype)[:, :4], pts.to(dtype)[:, :4], view_embed(dirs, multires_view, dtype)[ray]], -1)
    return F.pad(e, (0, kpad - e.shape[1]))


def color_extras_bwd(d_ext, dirs, rows, multires_view, dtype):
    """(ddirs [R, 3], sum |terms|, sum_k 2^k (|part_sin| + |part_cos|)): the view encoding's gradient."""
    R = dirs.shape[0]
    nv = 3 + 6 * multires_view
    de = d_ext.to(dtype)[:, 8:8 + nv].reshape(R, rows, nv)
    part, pabs = de.sum(1), de.abs().sum(1)
    a = view_args(dirs, multires_view).to(dtype)
    g, gabs, trig = part[:, :3].clone(), pabs[:, :3].clone(), torch.zeros(R, 3, dtype=dtype)
    for k in range(multires_view):
        f = float(1 << k)
        ps, pc = part[:, 3 + 6 * k:6 + 6 * k], part[:, 6 + 6 * k:9 + 6 * k]
        g = g + f * torch.cos(a[:, k]) * ps - f * torch.sin(a[:, k]) * pc
        qs, qc = pabs[:, 3 + 6 * k:6 + 6 * k], pabs[:, 6 + 6 * k:9 + 6 * k]
        gabs = gabs + f * torch.cos(a[:, k]).abs() * qs + f * torch.sin(a[:, k]).abs() * qc
        trig = trig + f * (ps.abs() + pc.abs())
    return g, gabs, trig


# ---------------------------------------------------------------------------
# compositing
def composite(z, dists_, sdf, normals, rgb, dirs, inv_s, car, dtype=None):
    """oracle.composite with a per-ray inv_s [R, 1] (a [1, 1] one broadcasts as in the oracle), so that autograd
    gives the kernel's per-ray dinv_s_part.  Returns (color, depth, weights, cdf [R S, 1])."""
    if dtype is not None:
        z, dists_, sdf, normals, rgb, dirs, inv_s = (t.to(dtype) for t in (z, dists_, sdf, normals, rgb, dirs, inv_s))
    R, S = z.shape
    if inv_s.shape[0] == R and R > 1:
        inv_s = inv_s.reshape(R, 1, 1).expand(R, S, 1).reshape(-1, 1)
    tc = (dirs * normals).sum(-1, keepdim=True)
    ic = -(F.relu(-tc * 0.5 + 0.5) * (1.0 - car) + F.relu(-tc) * car)
    en = sdf + ic * dists_.reshape(-1, 1) * 0.5
    ep = sdf - ic * dists_.reshape(-1, 1) * 0.5
    pc, nc = torch.sigmoid(ep * inv_s), torch.sigmoid(en * inv_s)
    alpha = ((pc - nc + 1e-5) / (pc + 1e-5)).reshape(R, S).clip(0.0, 1.0)
    w = alpha * exclusive_cumprod(alpha)
    color = (rgb * w[:, :, None]).sum(1)
    depth = (z * w).sum(1).unsqueeze(-1)
    return color, depth, w, pc


COTANGENTS = ("dcolor", "ddepth", "dweights", "dcdf")


def composite_all(case, dtype, which=COTANGENTS):
    """Forward outputs and the gradients for the cotangents named in `which` (the others null) of a compositing
    case (ray_cases.composite_case), in dtype on the CPU.  Returns a dict of fp tensors shaped as the kernels'
    buffers: color [R,3], depth [R,1], weights / cdf [R,S]; dsdf [M,1], dG [M,4], drgb [M,3], dinv_s_part [R],
    drays_d [R,3]; and tc [M] (d . n)."""
    R, S = case["z"].shape
    z = case["z"].to(dtype)
    dd = dists(z, sample_dist(case["near"].to(dtype), case["far"].to(dtype), case["n_coarse"]))
    leaves = {k: case[k].to(dtype).clone().requires_grad_(True) for k in ("sdf", "normals", "rgb", "rays_d")}
    inv = torch.full((R, 1), case["inv_s"], dtype=torch.float32).to(dtype).requires_grad_(True)
    dirs = leaves["rays_d"][:, None, :].expand(R, S, 3).reshape(-1, 3)
    c, d, w, pc = composite(z, dd, leaves["sdf"], leaves["normals"], leaves["rgb"].reshape(R, S, 3), dirs, inv,
                            f32(case["car"]))
    out = {"color": c.detach(), "depth": d.detach(), "weights": w.detach(), "cdf": pc.detach().reshape(R, S),
           "tc": (dirs * leaves["normals"]).sum(-1).detach()}
    if which:
        outs = {"dcolor": c, "ddepth": d, "dweights": w, "dcdf": pc.reshape(R, S)}
        L = sum((case[k].to(dtype) * outs[k]).sum() for k in which)
        g = torch.autograd.grad(L, [leaves["sdf"], leaves["normals"], leaves["rgb"], inv, leaves["rays_d"]],
                                allow_unused=True)
        g = [torch.zeros_like(l) if x is None else x for x, l in
             zip(g, [leaves["sdf"], leaves["normals"], leaves["rgb"], inv, leaves["rays_d"]])]
        out.update(dsdf=g[0], dG=F.pad(g[1], (0, 1)), drgb=g[2], dinv_s_part=g[3].reshape(-1), drays_d=g[4])
    return out
