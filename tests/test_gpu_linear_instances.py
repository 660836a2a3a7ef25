"""Every linear_kernel<...> instance cn_linear can launch against the float64 contract (linear_ref.py), at the
cases of linear_cases.table(): one test per tile template, mode and rank-1 flag, looping over its epilogues.

Each case runs at M = 1, 127, 128, 129 and a ragged multi-tile M (its virtual-concat twin at M = 129 and the
multi-tile M: linear_cases._rows), from natural buffers and again with every
operand and output a column slice of a wider tensor (leading dimension > width, 16-byte aligned) and the other
value of flags bit 0.  Every output buffer has 3 sentinel rows past M and 8 sentinel columns past the row: nothing
outside [0, M) x [0, nzero) (the split buffer: N - nsplit columns) may change, [N, nzero) is zero, the bf16
images equal the fp32 outputs' RNE bf16 bitwise, and a repeated launch is bitwise equal.

Values leave the easy range of the older tests: the activations the aux-reading epilogues recover sigma from are
softplus_100 of pre-activations over +-0.6 (beta z over +-60), with planted values at beta z = threshold +- a few
fp32 steps, sigma = 0 exactly (and an activation of exactly 0, where BWD_SOFTPLUS's second-order inputs are
garbage that must not be read into the result), sigma = 1 exactly and sigma ~ 1e-6; one row of A is zero, so the
forward epilogues see z = bias exactly, with bias values planted around the threshold; BWD_RELU's gate holds
+0.0, -0.0 and denormal-sized values of both signs.  BWD_SOFTPLUS's aux1 / aux2 are sigma w1, sigma w2 with
|w| <= 1, rounded to the operand format, as include/copenerf.h says they arise.

Tolerances are linear_ref's (derived there).  A bf16x6 instance also meets test_gpu_x6.py's bar on every output:
max error <= 2 x the exact-fp32 mode's max error on the same inputs + 1e-7 scale, mean error <= 1.5 x its mean
error + 1e-8 scale (where the fp32 mode has the instance: SOFTPLUS_HEAD at N > 128 has none).  Each test prints
the largest error-to-tolerance ratio per instance (DESIGN.md records the maxima per template)."""
import functools

import pytest
import torch

import linear_cases as LC
import linear_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD, COLS, OFF, SENT = 3, 8, 8, 7.0
WMAX = 384       # columns of the per-row operand pools (N <= 320)
KMAX = 320
ZERO_ROW = 0     # the row of A that is zero (in every launch, M = 1 too): z = bias exactly
BLOCK = 16384    # rows of a float64 reference block
SQRT2 = 2.0 ** 0.5
BETA = 100.0


def _rnd(*s, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(*s, generator=g) * 2 - 1) * scale).to(DEV)


def _steps(x, ks):
    """fp32 x moved by k units in the last place."""
    b = torch.tensor([x], dtype=torch.float32).view(torch.int32)
    return [(b + k).view(torch.float32).item() for k in ks]


@functools.lru_cache(maxsize=2)
def _pool(Mmax):
    """Operands for every case of up to Mmax rows (built once, never written)."""
    p = {}
    A, A2 = _rnd(Mmax, KMAX, seed=1, scale=0.3), _rnd(Mmax, 64, seed=2, scale=0.3)
    rowv = _rnd(Mmax, seed=3)
    A[ZERO_ROW], A2[ZERO_ROW], rowv[ZERO_ROW] = 0.0, 0.0, 0.0
    p.update(A=A, A2=A2, rowv=rowv, W=_rnd(512, KMAX, seed=4, scale=0.05), colv=_rnd(512, seed=5),
             head_w=_rnd(512, seed=6, scale=0.1), head_b=_rnd(1, seed=7))
    bias = _rnd(512, seed=8, scale=0.6)
    band = _steps(0.2, range(-3, 4))  # beta z = threshold +- 3 fp32 steps
    for j in range(2, 512, 8):
        bias[j] = band[(j // 8) % len(band)]
    p["bias"] = bias
    # pre-activations over +-0.6 with planted values in every fourth column, shifted from row to row
    z = _rnd(Mmax, WMAX, seed=9, scale=0.6)
    special = band + [-0.138, -0.6, 0.6, -0.3, float("nan")]  # nan: an activation of exactly 0
    m = torch.arange(Mmax, device=DEV)[:, None]
    j = torch.arange(1, WMAX, 4, device=DEV)[None, :]
    z[:, 1::4] = torch.tensor(special, device=DEV)[(m + j // 4) % len(special)]
    act = torch.nn.functional.softplus(z.double(), beta=BETA) / SQRT2
    act = torch.nan_to_num(act, nan=0.0).float()
    w1, w2 = _rnd(Mmax, WMAX, seed=10), _rnd(Mmax, WMAX, seed=11)
    for fmt, dt in (("f", torch.float32), ("b", torch.bfloat16)):
        a = act.to(dt)
        sg = LR.sigma(a, BETA * SQRT2)
        dead = a == 0
        p["act", fmt] = a
        # sigma w, garbage where the activation (and so sigma) is exactly 0
        p["aux1", fmt] = torch.where(dead, torch.ones_like(w1), (sg * w1.double()).float()).to(dt)
        p["aux2", fmt] = torch.where(dead, torch.ones_like(w2), (sg * w2.double()).float()).to(dt)
    gate = _rnd(Mmax, WMAX, seed=12)
    zeros = [0.0, -0.0, 1e-40, -1e-40, 1e-30, -1e-30]
    gate[:, 1::4] = torch.tensor(zeros, device=DEV)[(m + j // 4) % len(zeros)]
    p["gate", "f"], p["gate", "b"] = gate, gate.bfloat16()
    p["perm"] = torch.randperm(Mmax + PAD, device=DEV, generator=torch.Generator(device=DEV).manual_seed(13)).int()
    p["A", "b"], p["A2", "b"] = A.bfloat16(), A2.bfloat16()
    return p


def _sliced(p, key):
    """The pool tensor as a column slice (from column OFF) of a wider one (built once per tensor)."""
    k = ("sliced", key)
    if k not in p:
        t = p[key]
        wide = torch.full((t.shape[0], t.shape[1] + 2 * OFF), 3.0, device=DEV, dtype=t.dtype)
        wide[:, OFF:OFF + t.shape[1]] = t
        p[k] = wide[:, OFF:OFF + t.shape[1]]
    return p[k]


def _weights(p, c):
    """(the B operand, its column slice or None, the weight matrix the reference multiplies by)."""
    k = ("B", c.mode, c.N, c.K, c.ldb, c.tile)
    if k not in p:
        from copenerf import ops
        bn = 64 if c.tile == 1 else 128
        rows = c.ldb if c.mode == "x6" else -(-c.N // bn) * bn
        W = p["W"][:rows, :c.K].clone()
        W[c.N:] = 0  # rows past N are zero padding
        if c.mode == "x6":
            p[k] = (ops.split_bf16x3(W), None, W)
        else:
            B = W.bfloat16() if c.mode == "bf16" else W
            wide = torch.zeros(rows, c.K + 2 * OFF, device=DEV, dtype=B.dtype)
            wide[:, OFF:OFF + c.K] = B
            p[k] = (B.contiguous(), wide[:, OFF:OFF + c.K], B)
    return p[k]


def _launch(p, c, M, sliced, flip, mode=None):
    """One cn_linear launch of case c over the first M rows.  Returns (buffers: name -> (whole buffer, column
    offset, written width), the operands the reference needs).  mode "fp32": the exact-fp32 instance of the
    same case (the bf16x6 bar's yardstick)."""
    from copenerf import ops
    mode = mode or c.mode
    if mode != c.mode:
        c = c._replace(mode=mode, tile=1 if c.tile == 1 else 0, ldb=c.K + 8)
    e = LC.EPIS[c.epi]
    get = (lambda key: _sliced(p, key)) if sliced else (lambda key: p[key])
    fa = "b" if (c.mode == "bf16" and c.images[0]) else None
    fx = "b" if (c.mode == "bf16" and c.images[1]) else "f"
    B, Bs, W = _weights(p, c)
    A = get(("A", "b") if fa else "A")[:M]
    off = OFF if sliced else 0
    bufs = {}

    def out(name, width, dtype=torch.float32, cols=None):
        buf = torch.full((M + PAD, off + (cols or width) + COLS), SENT, device=DEV, dtype=dtype)
        bufs[name] = (buf, off, width)
        return buf[:, off:]

    kw = dict(nzero=c.nzero, tile=c.tile, M=M, adiv=SQRT2)
    ref = dict(nzero=c.nzero, adiv=SQRT2, bf16=c.mode == "bf16")
    if c.K1 < c.K:
        kw.update(A2=get(("A2", "b") if fa else "A2")[:M], K1=c.K1)
    both = {}
    if e in (0, 1, 2, 8):
        both["bias"] = p["bias"][:c.N]
    if e in (1, 4):
        both["odiv"] = SQRT2
    if c.rowv:
        both.update(rowv=p["rowv"][:M], colv=p["colv"][:c.N])
    if e in (3, 4, 5):
        both.update(aux0=get(("act", fx))[:M, :c.N], aux_beta=BETA * SQRT2)
    if c.epi == "bwd_softplus":
        both.update(aux1=get(("aux1", fx))[:M, :c.N], aux2=get(("aux2", fx))[:M, :c.N], aux2_scale=BETA * SQRT2)
    if e == 6:
        both["aux0"] = get(("gate", fx))[:M, :c.N]
    if c.epi == "mul_split":
        both["nsplit"] = c.nsplit
        kw["out_split"] = out("split", LC.SPLIT, cols=64)
    if e == 8:
        both.update(colv=p["colv"][:c.N], aux_beta=BETA, head_w=p["head_w"][:c.N], head_b=p["head_b"])
        kw["out1"] = out("out1", c.nzero)
        head = torch.full((M + PAD,), SENT, device=DEV)
        bufs["head"] = (head, 0, 0)
        kw["head_out"] = head
        if c.epi == "head_idx":  # M distinct destinations anywhere in the M + PAD elements of the buffer
            perm = p["perm"]
            kw["head_idx"] = perm[perm < M + PAD][:M].contiguous()
            bufs["idx"] = (kw["head_idx"], 0, 0)
    if c.mode == "bf16":
        kw["out0_b"] = out("out0_b", c.nzero, torch.bfloat16)
        if e == 8:
            kw["out1_b"] = out("out1_b", c.nzero, torch.bfloat16)
    out0 = out("out0", c.nzero)
    ops._flip = 0 if flip else 1  # ops.linear alternates the M order: this launch gets flags = flip
    ops.linear(A, Bs if (sliced and Bs is not None) else B, c.N, c.K, out0, e, **kw, **both)
    ref.update(both, A=A, W=W, A2=kw.get("A2"), K1=kw.get("K1"))
    return bufs, ref


def _reference(c, ref, M, r0, r1, head_act=None):
    """linear_ref over rows [r0, r1) of a launch's operands."""
    kw = dict(ref)
    A, W = kw.pop("A"), kw.pop("W")
    for k in ("A2", "aux0", "aux1", "aux2"):
        if kw.get(k) is not None:
            kw[k] = kw[k][r0:r1]
    if kw.get("rowv") is not None:
        kw["rowv"] = kw["rowv"][r0:r1]
    if head_act is not None:
        kw["head_act"] = head_act[r0:r1]
    return LR.linear_ref(A[r0:r1], W, c.N, c.K, LC.EPIS[c.epi], **kw)


class _Tally:
    """Verdicts kept on the device until a test's end: one synchronisation per test."""

    def __init__(self):
        self.labels, self.flags, self.ratios = [], [], []

    def add(self, label, ok, ratio=None):
        self.labels.append(label)
        self.flags.append(ok.reshape(()))
        self.ratios.append(torch.zeros((), device=DEV, dtype=torch.float64) if ratio is None else ratio.reshape(()).double())

    def finish(self):
        ok = torch.stack(self.flags).cpu()
        r = torch.stack(self.ratios).cpu()
        bad = [(self.labels[i], round(r[i].item(), 3)) for i in range(len(ok)) if not ok[i]]
        assert not bad, f"{len(bad)} of {len(ok)} checks failed, the first: {bad[:6]}"
        return r


def _written(bufs, name, M):
    buf, off, width = bufs[name]
    return buf[:M, off:off + width]


def _check(t, c, M, bufs, ref, where, yard=None):
    """One launch against the reference in row blocks; the sentinels; the bf16 images.  yard: the buffers of the
    exact-fp32 mode's launch on the same inputs (a bf16x6 case).  Returns the largest error / tolerance."""
    worst = torch.zeros((), device=DEV, dtype=torch.float64)
    sums = {}
    for r0 in range(0, M, BLOCK):
        r1 = min(M, r0 + BLOCK)
        act = _written(bufs, "out0", M)[:, :c.N] if "head" in bufs else None
        vals, tols = _reference(c, ref, M, r0, r1, act)
        outs = [("out0", _written(bufs, "out0", M)[r0:r1])]
        if "split" in bufs:
            outs.append(("split", _written(bufs, "split", M)[r0:r1]))
        if "out1" in bufs:
            outs.append(("out1", _written(bufs, "out1", M)[r0:r1]))
        if "head" in bufs:
            h = bufs["head"][0]
            outs.append(("head", h[bufs["idx"][0][r0:r1].long()] if "idx" in bufs else h[r0:r1]))
        for name, got in outs:
            err = (got.double() - vals[name]).abs()
            tol = tols[name]
            t.add(f"{where} {name} rows {r0}:{r1}", (err <= tol).all(), (err / tol.clamp_min(1e-300)).max())
            worst = torch.maximum(worst, torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err)).max())
            # (out1 and the head follow each launch's own activation: the bar is for the GEMM-bearing outputs)
            if yard is not None and name in ("out0", "split"):
                ey = (_written(yard, name, M)[r0:r1].double() - vals[name]).abs()
                s = sums.setdefault(name, [torch.zeros((), device=DEV, dtype=torch.float64) for _ in range(5)] + [0])
                s[0], s[1] = torch.maximum(s[0], err.max()), torch.maximum(s[1], ey.max())
                s[2], s[3] = s[2] + err.sum(), s[3] + ey.sum()
                s[4] = torch.maximum(s[4], vals[name].abs().max())
                s[5] += err.numel()
    for name, (e6, e32, s6, s32, scale, n) in sums.items():
        bar_max, bar_mean = 2.0 * e32 + 1e-7 * scale, 1.5 * s32 / n + 1e-8 * scale
        t.add(f"{where} {name} bf16x6 max error vs the fp32 mode's", e6 <= bar_max, e6 / bar_max)
        t.add(f"{where} {name} bf16x6 mean error vs the fp32 mode's", s6 / n <= bar_mean, s6 / n / bar_mean)
    # nothing outside the written regions: rows past M, columns past nzero (the split buffer: N - nsplit)
    for name, (buf, off, width) in bufs.items():
        if name == "idx":
            continue
        if name == "head":
            written = torch.zeros_like(buf, dtype=torch.bool)
            written[bufs["idx"][0].long() if "idx" in bufs else torch.arange(M, device=DEV)] = True
            t.add(f"{where} head sentinels", (buf[~written] == SENT).all())
            continue
        rest = buf.clone()
        rest[:M, off:off + width] = SENT
        t.add(f"{where} {name} sentinels", (rest == SENT).all())
    for img, src in (("out0_b", "out0"), ("out1_b", "out1")):
        if img in bufs:
            t.add(f"{where} {img} is not the bf16 of {src}",
                  (_written(bufs, img, M) == _written(bufs, src, M).bfloat16()).all())
    return worst


def _same(t, where, a, b):
    for name in a:
        t.add(f"{where} {name} not repeatable", (a[name][0] == b[name][0]).all())


def _run_case(t, p, c, M, both_layouts=True):
    where = f"{c.epi} N={c.N} K={c.K} K1={c.K1} nzero={c.nzero} M={M}"
    assert LC.resolved_name(LC.desc(c, M)) == LC.kernel_name(c), where
    yard = None
    if c.mode == "x6" and not (LC.EPIS[c.epi] == 8 and c.N > (64 if c.tile == 1 else 128)):
        yard, _ = _launch(p, c, M, False, 0, mode="fp32")
    bufs, ref = _launch(p, c, M, False, 0)
    worst = _check(t, c, M, bufs, ref, where, yard)
    # (the second-tile test repeats with the other walk order: results do not depend on flags bit 0)
    again, _ = _launch(p, c, M, False, 0 if both_layouts else 1)
    _same(t, where, bufs, again)
    if both_layouts:
        bufs, ref = _launch(p, c, M, True, 1)
        worst = torch.maximum(worst, _check(t, c, M, bufs, ref, where + " sliced, reversed"))
    return worst


def _group(c):
    return (c.tmpl, LC.mode_bits(c), c.rowv)


GROUPS = sorted(set(_group(c) for c in LC.table()))


def _report(t, ratios):
    """Prints the largest error / tolerance per instance; every check's verdict is asserted first."""
    t.finish()
    worst = {}
    for name, r in ratios:
        worst[name] = max(worst.get(name, 0.0), r.item())
    for name, r in sorted(worst.items()):
        print(f"RATIO {name[len('void cn::'):name.index('(')]} {r:.3f}")
    assert all(r <= 1.0 for r in worst.values())


@pytest.mark.parametrize("tmpl,bits,rowv", GROUPS, ids=[f"{g[0].replace(', ', '_')}-m{g[1]}-r{g[2]}" for g in GROUPS])
def test_instances_match_float64(tmpl, bits, rowv):
    p = _pool(1537)
    t, ratios = _Tally(), []
    for c in LC.table():
        if _group(c) != (tmpl, bits, rowv):
            continue
        for M in c.Ms:
            ratios.append((LC.kernel_name(c), _run_case(t, p, c, M)))
    _report(t, ratios)


TEMPLATES = sorted(set((c.tmpl, c.mode) for c in LC.table()))


@pytest.mark.parametrize("tmpl,mode", TEMPLATES, ids=[f"{g[0].replace(', ', '_')}-{g[1]}" for g in TEMPLATES])
def test_second_tile_of_a_persistent_workgroup(tmpl, mode):
    """M = 2 (workgroups the launch starts) BM + 77: launch_linear_tile_m starts min(tiles, OCC x CUs) workgroups,
    so each walks at least two row tiles and the last tile is ragged; the smallest K, one light epilogue and
    one aux-reading one (where the template has them), against float64 in row blocks."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = 2 * LC.TILE_OCC[tmpl] * cus * LC.TILE_ROWS[tmpl] + 77
    p = _pool(M)
    t, ratios = _Tally(), []
    mine = [c for c in LC.table() if (c.tmpl, c.mode) == (tmpl, mode) and c.K == c.K1 and c.images == (0, 0)]
    ran = 0
    for epis in (("softplus", "store"), ("mul", "bwd_relu")):
        pick = [c for c in mine if c.epi in epis]
        if not pick:
            continue
        # the widest case without a rank-1 term, if there is one
        c = max(pick, key=lambda c: (not c.rowv, c.N <= 256, c.N, c.epi == epis[0]))
        ratios.append((LC.kernel_name(c), _run_case(t, p, c, M, both_layouts=False)))
        ran += 1
    assert ran
    _report(t, ratios)


def test_rejected_instances_launch_nothing():
    """The exclusions of linear_cases.EXCLUDED that the library rejects raise on the device too (a host-side
    check: nothing is launched) and leave the sentinel-filled outputs as they were."""
    from copenerf import ops
    p = _pool(1537)
    M = 200
    full = lambda *s, dt=torch.float32: torch.full(s, SENT, device=DEV, dtype=dt)  # noqa: E731
    o0, o1, sdf, ob = full(M, 384), full(M, 384), full(M), full(M, 384, dt=torch.bfloat16)
    head = dict(bias=p["bias"][:256], head_w=p["head_w"][:256], head_b=p["head_b"], head_out=sdf, out1=o1,
                colv=p["colv"][:256], aux_beta=BETA)
    W = p["W"][:256, :128].contiguous()
    for B in (W, W.bfloat16(), ops.split_bf16x3(W)):
        for tile, N in ((0, 128), (1, 64)):
            # SOFTPLUS_HEAD with a rank-1 term
            with pytest.raises(RuntimeError, match="SOFTPLUS_HEAD"):
                ops.linear(p["A"][:M], B, N, 128, o0, ops.EPI_SOFTPLUS_HEAD, tile=tile, rowv=p["rowv"][:M], **head)
    # SOFTPLUS_HEAD past 256 columns: the only shape that names the one-per-CU 128x256 tile for it
    W5 = p["W"][:512, :128].contiguous()
    with pytest.raises(RuntimeError, match="N <= 256"):
        ops.linear(p["A"][:M], ops.split_bf16x3(W5), 320, 128, o0, ops.EPI_SOFTPLUS_HEAD,
                   **dict(head, bias=p["bias"][:320], head_w=p["head_w"][:320], colv=p["colv"][:320]))
    # a bf16 aux0 image for an epilogue that reads none (STORE, SOFTPLUS, RELU, SOFTPLUS_HEAD; mode bits 9 and 13, on
    # the 128x128 and the 256x256 bf16 tile).  ops.linear refuses the dtype itself, so the descriptor is built here,
    # with every operand real and sized to the case's leading dimensions: the library's own check is what raises
    from copenerf import _lib
    N, K = 256, 128
    o1b = full(M, 384, dt=torch.bfloat16)
    for tile, tmpl in ((2, LC.BF_T0), (0, LC.BF_SQ)):
        for epi in ("store", "softplus", "relu", "head"):
            for a_b in (0, 1):
                c = LC.Case(tmpl, "bf16", tile, epi, 0, (a_b, 0), 128 if (epi == "head" and tile) else N, K, K, K + 8,
                            N, N, 384, (M,))
                t = dict(A=(p["A", "b"] if a_b else p["A"])[:M, :K + 8].contiguous(),
                         B=torch.zeros(256, K + 8, device=DEV, dtype=torch.bfloat16), out0=o0, out0_b=ob, out1=o1,
                         out1_b=o1b, bias=p["bias"], colv=p["colv"], head_w=p["head_w"], head_b=p["head_b"],
                         head_out=sdf)
                d = LC.desc(c, M, ptr=lambda name: t[name].data_ptr())
                d.aux0, d.ld_aux0, d.aux0_bf16 = p["act", "b"].data_ptr(), WMAX, 1
                assert "%d>" % (9 + 4 * a_b) in LC.resolved_name(d)
                with pytest.raises(RuntimeError, match="a bf16 aux0 is for MUL / TANGENT / BWD_SOFTPLUS / BWD_RELU"):
                    _lib.check(_lib.load().cn_linear(d, ops._stream()), "cn_linear")
    torch.cuda.synchronize()
    for o in (o0, o1, sdf, ob, o1b):
        assert torch.all(o == SENT)
