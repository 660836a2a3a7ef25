"""The hand-written kernels around the GEMMs (csrc/cn_render.hip, csrc/cn_fields.hip) at their own C entry points,
at tiny ragged shapes, against tests/ray_ref.py in float64.

Every bar is derived from the CPU oracle against float64 or from the precision of fp32, never from what the
kernels give (tests/ray_cases.py; tests/test_ray_ref.py holds the fp32 oracle itself to the same bars on the
same inputs):
  compositing   per case and output  max|kernel - ref64| <= 4 max|oracle32 - ref64| + 4 * 2^-24 max|ref64|
  up-sampling   z_new inside the float64 cdf's preimage of u -+ tol_cdf, tol_cdf = 4 max|cdf32 - cdf64| + 8 * 2^-24
                per launch; the merge, its scatter map and the tie rule exactly
  per point     sin / cos: 4 max|CPU fp32 - float64| + 2^-23; products and sums: 2 * 2^-24 x the sum of the absolute
                values of the terms (times the number of terms for the reductions); copies and padding exactly
Every output buffer carries 3 sentinel rows past its last row (and, where the entry takes a leading dimension, is
also run as a column slice with 4 sentinel columns before and 8 after); the sentinels must survive, and every launch
is repeated once and must give the same bits.  Run with -s to see the largest error-to-bar ratio per output
(DESIGN.md records them)."""
import math

import pytest
import torch

import ray_cases as C
import ray_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
R = C.R


def _ops():
    from copenerf import ops
    return ops


class Out:
    """An output buffer of [rows, cols] inside sentinels; init: the values the launch starts from (accumulate)."""

    def __init__(self, rows, cols, sliced=False, dtype=torch.float32, init=None):
        self.rows, self.cols, self.off, self.init = rows, cols, 4 if sliced else 0, init
        self.fill = float("nan") if dtype.is_floating_point else -7
        self.base = torch.empty(rows + 3, cols + (12 if sliced else 0), dtype=dtype, device=DEV)
        self.view = self.base[:rows, self.off:self.off + cols]
        self.reset()

    def reset(self):
        self.base.fill_(self.fill)
        if self.init is not None:
            self.view.copy_(self.init)

    def take(self):
        """The written block on the CPU, after checking that nothing around it was touched."""
        b = self.base.cpu()
        m = torch.ones(b.shape, dtype=torch.bool)
        m[:self.rows, self.off:self.off + self.cols] = False
        s = b[m]
        assert bool(torch.isnan(s).all() if b.dtype.is_floating_point else (s == self.fill).all()), "sentinel overwritten"
        return b[:self.rows, self.off:self.off + self.cols].contiguous()


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _twice(fn, outs):
    """Launch, collect, reset, launch again: the repeat gives the same bits.  None entries stay None."""
    res = []
    for _ in range(2):
        for o in outs:
            if o is not None:
                o.reset()
        fn()
        res.append([None if o is None else o.take() for o in outs])
    for a, b in zip(*res):
        assert a is None or _same_bits(a, b), "a repeated launch differs"
    return res[0]


def _in(t, sliced=False):
    """An operand on the device: contiguous, or a 16-byte-aligned column slice of a wider NaN-filled tensor."""
    if t is None:
        return None
    if not sliced:
        return t.to(DEV).contiguous()
    wide = torch.full((t.shape[0] + 1, t.shape[1] + 12), float("nan"), dtype=t.dtype, device=DEV)
    wide[:t.shape[0], 4:4 + t.shape[1]] = t.to(DEV)
    return wide[:t.shape[0], 4:4 + t.shape[1]]


def _merge_worst(worst, kernel, w):
    for k, v in w.items():
        worst[(kernel, k)] = max(worst.get((kernel, k), 0.0), v)


# ---------------------------------------------------------------------------
# compositing
def _ratio(got, r64, r32, keep=None):
    bar = C.composite_bar(r64, r32, keep)
    a, b = got.double().reshape(r64.shape), r64.double()
    if keep is not None:
        a, b = a[keep], b[keep]
    err = (a - b).abs().max().item() if a.numel() else 0.0
    if bar == 0.0:
        assert err == 0.0, err
        return 0.0
    return err / bar


@pytest.mark.parametrize("S", C.COMP_S)
def test_composite_forward_and_backward(S):
    ops = _ops()
    M = R * S
    worst = {}

    def note(name, v, where):
        worst[name] = max(worst.get(name, (0.0, None)), (v, where))

    for inv_s in C.COMP_INV_S:
        for car in C.COMP_CAR:
            c = C.composite_case(S, inv_s, car)
            z, sdf, rgb, rays_d, near, far = (_in(c[k]) for k in ("z", "sdf", "rgb", "rays_d", "near", "far"))
            inv, car_t = ops.device_scalar(inv_s, z.device), ops.device_scalar(car, z.device)
            G4 = torch.cat([c["normals"], c["flow"]], -1)
            r64, r32 = C.composite_refs(S, inv_s, car, RR.COTANGENTS)
            keep = C.kink_mask(r64["tc"])
            keep_rays = keep.reshape(R, S).all(1)
            for ld_g in (4, 8):
                if ld_g == 4:
                    G = _in(G4)
                else:
                    wide = torch.full((M, 8), float("nan"), device=DEV)
                    wide[:, 4:] = G4.to(DEV)
                    G = wide[:, 4:]
                assert G.stride(0) == ld_g
                where = (inv_s, car, ld_g)
                fwd = None
                for with_cdf in (True, False):
                    o = [Out(R, 3), Out(R, 1), Out(R, S), Out(R, S) if with_cdf else None]
                    got = _twice(lambda: ops.composite_fwd(z, sdf, G, rgb, rays_d, inv, near, far, c["n_coarse"], car_t,
                                                           o[0].view, o[1].view, o[2].view,
                                                           o[3].view if with_cdf else None), o)
                    if fwd is None:
                        fwd = got
                        for name, t in zip(("color", "depth", "weights", "cdf"), got):
                            note(name, _ratio(t, r64[name], r32[name]), where)
                    else:  # a null cdf changes nothing else
                        assert all(_same_bits(a, b) for a, b in zip(got[:3], fwd[:3]))
                for which in C.BWD_SETS:
                    b64, b32 = C.composite_refs(S, inv_s, car, which)
                    cot = [_in(c[k]) if k in which else None for k in RR.COTANGENTS]
                    first = None
                    for want_dd in (False, True):
                        o = [Out(M, 1), Out(M, 4), Out(M, 3), Out(R, 1), Out(R, 3) if want_dd else None]
                        got = _twice(lambda: ops.composite_bwd(z, sdf, G, rgb, rays_d, inv, near, far, c["n_coarse"], car_t,
                                                               *cot, o[0].view, o[1].view, o[2].view, o[3].view,
                                                               o[4].view if want_dd else None), o)
                        if first is not None:  # asking for drays_d changes nothing else
                            assert all(_same_bits(a, b) for a, b in zip(got[:4], first[:4]))
                        first = got
                    dsdf, dG, drgb, dinv, dd = got
                    tag = where + ("+".join(which),)
                    note("dsdf", _ratio(dsdf, b64["dsdf"], b32["dsdf"]), tag)
                    assert bool((dG[:, 3] == 0).all())
                    note("dG", _ratio(dG, b64["dG"], b32["dG"], keep), tag)
                    note("drgb", _ratio(drgb, b64["drgb"], b32["drgb"]), tag)
                    note("dinv_s_part", _ratio(dinv.reshape(-1), b64["dinv_s_part"], b32["dinv_s_part"]), tag)
                    note("drays_d", _ratio(dd, b64["drays_d"], b32["drays_d"], keep_rays), tag)
    print("composite S=%d error/bar:" % S, {k: (round(v, 3), w) for k, (v, w) in worst.items()})
    bad = {k: v for k, v in worst.items() if v[0] > 1.0}
    assert not bad, bad


# ---------------------------------------------------------------------------
# up-sampling and merge
@pytest.mark.parametrize("kind", C.UP_KINDS)
@pytest.mark.parametrize("n", C.UP_N)
def test_up_sample_merge(n, kind):
    ops = _ops()
    tols, ties = [], 0
    for k in [k for k in C.UP_NIMP if n + k <= 256]:
        nt = n + k
        for inv_s in C.UP_INV_S:
            z, sdf = C.up_case(n, inv_s, kind)
            zd, sd = _in(z), _in(sdf)
            o = [Out(R, nt), Out(R, k), Out(R, nt), Out(R, k, dtype=torch.int32)]
            z_out, z_new, sdf_out, dst = _twice(
                lambda: ops.up_sample_merge(zd, sd, k, inv_s, o[0].view, o[1].view, o[2].view, o[3].view), o)
            p = [Out(R, nt), Out(R, k)]
            z_out2, z_new2 = _twice(lambda: ops.up_sample_merge(zd, sd, k, inv_s, p[0].view, p[1].view), p)
            assert _same_bits(z_out, z_out2) and _same_bits(z_new, z_new2)  # null sdf_out / new_dst change nothing
            label = (n, k, inv_s, kind)
            # the merge, exactly
            assert bool((z_out[:, 1:] >= z_out[:, :-1]).all()), label
            assert _same_bits(z_out, torch.sort(torch.cat([z, z_new], -1), -1)[0]), label
            flat = dst.long().reshape(-1)
            assert _same_bits(z_out.reshape(-1)[flat], z_new.reshape(-1)), label
            row = dst.long() - torch.arange(R)[:, None] * nt
            assert bool(((row >= 0) & (row < nt)).all()), label
            assert all(row[r].unique().numel() == k for r in range(R)), label
            new_slot = torch.zeros(R * nt, dtype=torch.bool)
            new_slot[flat] = True
            so = sdf_out.reshape(-1)
            assert bool(torch.isnan(so[new_slot]).all()), label  # the new samples' sdf slots are left for the query
            assert _same_bits(so[~new_slot].reshape(R, n), sdf), label
            want_dst = RR.merge(z, z_new)[1]  # old before new on ties, new ones in index order
            assert torch.equal(dst.long(), want_dst), label
            ties += int((z_new[:, :, None] == z[:, None, :]).any(-1).sum())
            # the values
            _, cdf32, _ = C.up_ref32(n, k, inv_s, kind)
            ok, tol_cdf, _ = RR.z_new_ok(z_new, z, sdf, k, inv_s, cdf32)
            assert bool(ok.all()), (label, int((~ok).sum()))
            tols.append(tol_cdf)
    print("up_sample n=%d %s: tol_cdf %.3g .. %.3g, new-old ties %d" % (n, kind, min(tols), max(tols), ties))


# ---------------------------------------------------------------------------
# per-point kernels
SQRT2 = math.sqrt(2.0)


def _quotient_ok(q, num, div, label):
    """q = num / div, one rounded division of the kernel's own fp32 num (checked against the reference itself)."""
    want = num.double() / RR.f32(div)
    assert bool(((q.double() - want).abs() <= (C.U2 + C.SLACK) * want.abs()).all()), label


@pytest.mark.parametrize("M", C.POINT_M)
def test_sdf_embed(M):
    ops = _ops()
    worst = {}
    for L in (0, 3, 6, 10):
        ng = 1 + 2 * L
        for scale in (1.0, 1.7):
            for kpad in sorted({64, C.min_embed_kpad(L)}):
                if kpad < C.min_embed_kpad(L):
                    continue
                inp, ref, bars = C.embed_op(M, L, scale, kpad)
                for sliced in (False, True):
                    label = ("embed", M, L, scale, kpad, sliced)
                    x = _in(inp["x"], sliced)
                    o = [Out(M, kpad, sliced), Out(M, 4 * ng, sliced)]
                    U0, U4 = _twice(lambda: ops.sdf_embed(x, L, scale, o[0].view, o[1].view, SQRT2), o)
                    _merge_worst(worst, "embed", C.check_op({"U0": U0}, ref(F64), bars, label))
                    _quotient_ok(U4, U0[:, :4 * ng], SQRT2, label)
                    p = [Out(M, kpad, sliced)]
                    assert _same_bits(_twice(lambda: ops.sdf_embed(x, L, scale, p[0].view), p)[0], U0)
                    # the bf16 operand images: RNE of the fp32 launch's values
                    b = [Out(M, kpad, sliced, torch.bfloat16), Out(M, 4 * ng, sliced, torch.bfloat16)]
                    U0b, U4b = _twice(lambda: ops.sdf_embed(x, L, scale, b[0].view, b[1].view, SQRT2), b)
                    assert _same_bits(U0b, U0.to(torch.bfloat16)) and _same_bits(U4b, U4.to(torch.bfloat16)), label
                    m = [Out(M, kpad, sliced), Out(M, 4 * ng, sliced, torch.bfloat16)]
                    U0m, U4m = _twice(lambda: ops.sdf_embed(x, L, scale, m[0].view, m[1].view, SQRT2), m)
                    assert _same_bits(U0m, U0) and _same_bits(U4m, U4b), label
    print("error/bar:", worst)


@pytest.mark.parametrize("M", C.POINT_M)
def test_sdf_tangent_prep_and_grad_assemble(M):
    ops = _ops()
    worst = {}
    for L in (0, 3, 4, 6):
        ng = 1 + 2 * L
        for sliced in (False, True):
            kpad = C.min_embed_kpad(L) if sliced else 64
            inp, ref, bars = C.tangent_op(M, L, 1.7, kpad)
            label = ("tangent", M, L, sliced)
            U0, v = _in(inp["U0"], sliced), _in(inp["v"], sliced)
            o = [Out(M, kpad, sliced), Out(M, 4 * ng, sliced)]
            T0, T4 = _twice(lambda: ops.sdf_tangent_prep(L, 1.7, U0, v, o[0].view, o[1].view, SQRT2), o)
            _merge_worst(worst, "tangent", C.check_op({"T0": T0}, ref(F64), bars, label))
            _quotient_ok(T4, T0[:, :4 * ng], SQRT2, label)
            p = [Out(M, kpad, sliced)]
            assert _same_bits(_twice(lambda: ops.sdf_tangent_prep(L, 1.7, U0, v, p[0].view), p)[0], T0)
            b = [Out(M, kpad, sliced), Out(M, 4 * ng, sliced, torch.bfloat16)]
            T0b, T4b = _twice(lambda: ops.sdf_tangent_prep(L, 1.7, U0, v, b[0].view, b[1].view, SQRT2), b)
            assert _same_bits(T0b, T0) and _same_bits(T4b, T4.to(torch.bfloat16)), label
            for qe in (False, True):
                inp, ref, bars = C.assemble_op(M, L, 1.7, qe)
                label = ("assemble", M, L, qe, sliced)
                U0, Q0, QE = (_in(inp[k], sliced) for k in ("U0", "Q0", "QE"))
                g = [Out(M, 4, sliced)]
                G = _twice(lambda: ops.sdf_grad_assemble(L, 1.7, U0, Q0, QE, g[0].view), g)[0]
                _merge_worst(worst, "assemble", C.check_op({"G": G}, ref(F64), bars, label))
    print("error/bar:", worst)


@pytest.mark.parametrize("M", C.POINT_M)
def test_color_extras(M):
    ops = _ops()
    worst = {}
    for dir_div in (1, 3, 64, 100, 128):
        for mv in (0, 4):
            for sliced in (False, True):
                kpad = C.min_extras_kpad(mv) if sliced else 64
                inp, ref, bars = C.extras_op(M, dir_div, mv, kpad)
                G, pts, dirs = (_in(inp[k], sliced) for k in ("G", "pts", "dirs"))
                o = [Out(M, kpad, sliced)]
                ext = _twice(lambda: ops.color_extras(G, pts, dirs, dir_div, mv, o[0].view), o)[0]
                _merge_worst(worst, "extras", C.check_op({"ext": ext}, ref(F64), bars, ("extras", M, dir_div, mv, sliced)))
    print("error/bar:", worst)


@pytest.mark.parametrize("Rr", [1, 7, 9])
def test_color_extras_bwd(Rr):
    ops = _ops()
    worst = {}
    for rows in (1, 3, 40):
        for mv in (0, 4):
            for acc in (False, True):
                for sliced in (False, True):
                    inp, ref, bars = C.extras_bwd_op(Rr, rows, mv, acc)
                    d_ext, dirs = _in(inp["d_ext"], sliced), _in(inp["dirs"], sliced)
                    o = [Out(Rr, 3, init=_in(inp["prev"]))]
                    dd = _twice(lambda: ops.color_extras_bwd(d_ext, dirs, rows, mv, o[0].view, accumulate=acc), o)[0]
                    _merge_worst(worst, "extras_bwd",
                                 C.check_op({"ddirs": dd}, ref(F64), bars, ("extras_bwd", Rr, rows, mv, acc, sliced)))
    print("error/bar:", worst)


def test_coarse_z_and_points():
    ops = _ops()
    worst = {}
    for n in (1, 2, 5, 64):
        for jitter in (False, True):
            inp, ref, bars = C.coarse_z_op(n, jitter)
            near, far, t_rand = (_in(inp[k]) for k in ("near", "far", "t_rand"))
            o = [Out(R, n)]
            z = _twice(lambda: ops.coarse_z(near, far, n, t_rand, o[0].view), o)[0]
            _merge_worst(worst, "coarse_z", C.check_op({"z": z}, ref(F64), bars, ("coarse_z", n, jitter)))
            assert bool((z[:, 1:] >= z[:, :-1]).all())
    for n in (1, 63, 65, 200):
        for mid in (False, True):
            inp, ref, bars = C.points_op(n, mid)
            ro, rd, z, t, near, far = (_in(inp[k]) for k in ("o", "d", "z", "t", "near", "far"))
            o = [Out(R * n, 4)]
            pts = _twice(lambda: ops.points(ro, rd, z, t, o[0].view, mid=mid, near=near, far=far,
                                            n_coarse=inp["n_coarse"]), o)[0]
            _merge_worst(worst, "points", C.check_op({"pts": pts}, ref(F64), bars, ("points", n, mid)))
            for ld_p in (4, 8):
                inp, ref, bars = C.points_bwd_op(n, mid, ld_p)
                z, dP, near, far = (_in(inp[k]) for k in ("z", "dP", "near", "far"))
                assert dP.stride(0) == ld_p
                full = None
                for want in ((True, True), (True, False), (False, True)):
                    o = [Out(R, 3) if w else None for w in want]
                    got = _twice(lambda: ops.points_bwd(z, dP, o[0].view if want[0] else None,
                                                        o[1].view if want[1] else None, mid=mid, near=near, far=far,
                                                        n_coarse=inp["n_coarse"]), o)
                    if full is None:
                        full = got
                        _merge_worst(worst, "points_bwd", C.check_op({"drays_o": got[0], "drays_d": got[1]}, ref(F64),
                                                                     bars, ("points_bwd", n, mid, ld_p)))
                    else:  # a null output changes nothing in the other
                        assert all(a is None or _same_bits(a, b) for a, b in zip(got, full))
    print("error/bar:", worst)
