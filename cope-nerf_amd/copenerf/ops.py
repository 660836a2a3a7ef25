"""Tensor-level wrappers over the C ABI (one function per entry point).

Every wrapper checks device, dtype and layout on the host, then launches on
torch's current HIP stream.  Buffers are plain 2-D fp32 row-major tensors whose
leading dimension (stride(0)) is passed explicitly, so column views such as
``buf[:, :256]`` can be handed over without copies.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import (EPI_BWD_RELU, EPI_BWD_SOFTPLUS, EPI_MUL, EPI_RELU, EPI_SOFTPLUS, EPI_SOFTPLUS_HEAD,  # noqa: F401
                   EPI_STORE, EPI_TANGENT)

SQRT2 = float(math.sqrt(2.0))  # torch's x / np.sqrt(2) divides by the fp32 rounding of this


class KernelTimer:
    """Brackets cn_linear / cn_wgrad launches with HIP events on the launching
    stream (torch's current stream) and keeps (key, events, algorithmic FLOPs)."""

    def __init__(self, detail=False):
        self.records = []
        self.detail = detail  # key launches by shape as well
        self.symbols = {}  # launch class -> rocprofv3 symbol of its kernel (named by the library)

    def start(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stop(self, key, e0, flops, nbytes=0.0):
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.records.append((key, e0, e1, flops, nbytes))

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for key, e0, e1, fl, nb in self.records:
            a = agg.setdefault(key, {"launches": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            a["launches"] += 1
            a["ms"] += e0.elapsed_time(e1)
            a["flops"] += fl
            a["bytes"] += nb
        return agg


_timer = None
# cn_linear_desc.flags bit 0 alternated launch to launch (the memory-side cache holds the last
# rows a layer wrote when the next one starts; see include/copenerf.h)
_flip = 0
EPI_NAMES = {0: "store", 1: "softplus", 2: "relu", 3: "mul", 4: "tangent", 5: "bwd_softplus", 6: "bwd_relu",
             8: "softplus_head"}


def set_kernel_timer(t):
    global _timer
    _timer = t


def rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need(t, name, *, ndim=2):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError(f"copenerf: {name} must be a CUDA/HIP tensor (got {t.device}); "
                           "the HIP kernels have no CPU fallback")
    if t.dtype not in (torch.float32, torch.int32, torch.bfloat16):
        raise RuntimeError(f"copenerf: {name} must be float32 (got {t.dtype})")
    if ndim == 2 and (t.dim() != 2 or t.stride(1) != 1):
        raise RuntimeError(f"copenerf: {name} must be a row-major 2-D tensor (shape {tuple(t.shape)}, "
                           f"strides {t.stride()})")


def _ld(t):
    return 0 if t is None else t.stride(0)


def split_bf16x3(W: torch.Tensor) -> torch.Tensor:
    """[N, K] fp32 (K % 16 == 0) -> the chunk-major B image of
    CN_MFMA_F32_BF16X6, bf16 [K/16, N, 48]: entry [c, n, 16 t + j] is term t of
    W[n, 16 c + j], with W = w0 + w1 + w2 (each the RNE bf16 of the remainder;
    |W - Σ| <= 2^-27 |W|)."""
    N, K = W.shape
    if K % 16:
        raise ValueError(f"split_bf16x3: K={K} must be a multiple of 16")
    w0 = W.to(torch.bfloat16)
    r = W - w0.float()
    w1 = r.to(torch.bfloat16)
    w2 = (r - w1.float()).to(torch.bfloat16)
    t = torch.stack([w0, w1, w2], 1).view(N, 3, K // 16, 16)
    return t.permute(2, 0, 1, 3).reshape(K // 16, N, 48).contiguous()


def unsplit_bf16x3(B: torch.Tensor) -> torch.Tensor:
    """The three terms [3, N, K] (bf16) of a split_bf16x3 image."""
    C, N, _ = B.shape
    return B.view(C, N, 3, 16).permute(2, 1, 0, 3).reshape(3, N, C * 16)


FORMATS = {"fp32": 0, "bf16": 1, "bf16x6": 2}


def weight_norm_batch(vs, gs, *, dws=None):
    """cn_weight_norm over lists of (v [rows, cols], g [rows, 1] or [rows]) in one launch:
    forward -> [W]; with dws (the gradients of the W) -> ([dv], [dg])."""
    jobs = (_lib.WnJob * max(1, len(vs)))()
    outs = []
    for i, (v, g) in enumerate(zip(vs, gs)):
        _need(v, "v")
        if not v.is_contiguous() or not g.is_contiguous() or g.numel() != v.shape[0]:
            raise RuntimeError("weight_norm_batch: v [rows, cols] and g [rows] must be contiguous")
        j = jobs[i]
        j.v, j.g, j.rows, j.cols = v.data_ptr(), g.data_ptr(), v.shape[0], v.shape[1]
        if dws is None:
            w = torch.empty_like(v)
            j.w = w.data_ptr()
            outs.append(w)
        else:
            dw = dws[i].contiguous()
            dv, dg = torch.empty_like(v), torch.empty_like(g)
            j.dw, j.dv, j.dg = dw.data_ptr(), dv.data_ptr(), dg.data_ptr()
            outs.append((dv, dg, dw))
    _lib.check(_lib.load().cn_weight_norm(jobs, len(vs), 0 if dws is None else 1, _stream()), "cn_weight_norm")
    if dws is None:
        return outs
    return [o[0] for o in outs], [o[1] for o in outs]


class ImagePacker:
    """Collects cn_pack_job regions of weight images and builds them in one
    cn_pack_weights launch (the per-call weight packing of fields.py)."""

    def __init__(self, mode: str):
        if mode not in FORMATS:
            raise ValueError(f"mode must be one of {tuple(FORMATS)} (got {mode!r})")
        self.mode = mode
        self.jobs = []
        self.keep = []  # sources must stay alive until the launch is queued

    def image(self, rows: int, cols: int, device, fmt: str | None = None) -> torch.Tensor:
        """An uninitialised image of the packer's format: fp32 / bf16 [rows, cols], bf16x6 the
        chunk-major [cols/16, rows, 48] (split_bf16x3's layout)."""
        fmt = fmt or self.mode
        if fmt == "bf16x6":
            if cols % 16:
                raise ValueError(f"pack: bf16x6 image width {cols} must be a multiple of 16")
            return torch.empty(cols // 16, rows, 48, device=device, dtype=torch.bfloat16)
        return torch.empty(rows, cols, device=device, dtype=torch.bfloat16 if fmt == "bf16" else torch.float32)

    def put(self, dst: torch.Tensor, src: torch.Tensor, *, transpose=False, r0=0, r1=None, c0=0, c1=None, fmt=None):
        """Region [r0, r1) x [c0, c1) of dst (default: all of it) = src (or srcᵀ) at (r0, c0), zero elsewhere."""
        fmt = fmt or self.mode
        _need(src, "pack src")
        _need(dst, "pack dst", ndim=dst.dim())
        if src.dtype != torch.float32:
            raise RuntimeError("pack: src must be float32")
        rows, cols = (src.shape[1], src.shape[0]) if transpose else (src.shape[0], src.shape[1])
        j = _lib.PackJob()
        j.src, j.dst = src.data_ptr(), dst.data_ptr()
        j.src_ld = src.stride(0)
        x6 = fmt == "bf16x6"
        d_rows, d_cols = (dst.shape[1], 16 * dst.shape[0]) if x6 else (dst.shape[0], dst.shape[1])
        j.dst_ld = d_rows if x6 else d_cols
        j.rows, j.cols = rows, cols
        j.r0, j.r1 = r0, d_rows if r1 is None else r1
        j.c0, j.c1 = c0, d_cols if c1 is None else c1
        j.transpose, j.format = int(transpose), FORMATS[fmt]
        self.jobs.append(j)
        self.keep.append(src)
        return dst

    def run(self):
        if self.jobs:
            arr = (_lib.PackJob * len(self.jobs))(*self.jobs)
            _lib.check(_lib.load().cn_pack_weights(arr, len(self.jobs), _stream()), "cn_pack_weights")
        self.jobs, self.keep = [], []


# launch-class tags of the kernel timer: linear_kernel<WM, WN, TM, TN, BK, OCC, DEPTH, ...> arguments
# (named by the library itself, cn_linear_kernel_name) -> a short tile name
_TILE_TAGS = {"4, 2, 2, 4, 16, 1, 2": "sq", "4, 2, 1, 4, 32, 1, 2": "tall", "4, 2, 2, 2, 32, 1, 2": "wide",
              "2, 2, 2, 4, 16, 2, 2": "tall2",
              "2, 2, 2, 2, 16, 2, 2": "t128", "4, 1, 1, 2, 16, 2, 2": "t1", "4, 2, 2, 4, 32, 1, 2": "sq",
              "2, 2, 2, 2, 64, 2, 1": "t128", "4, 1, 1, 2, 64, 2, 1": "t1"}


def kernel_name(query, d) -> str:
    """The rocprofv3 symbol of the kernel a cn_linear / cn_wgrad descriptor launches, as the
    library decides it (cn_linear_kernel_name / cn_wgrad_kernel_name)."""
    buf = ctypes.create_string_buffer(256)
    n = query(d, buf, 256)
    if n < 0:
        raise RuntimeError(f"kernel name query failed ({n}): {_lib.load().cn_last_error().decode()}")
    return buf.value.decode()


def _tile_tag(name, tile):
    args = name[name.index("<") + 1:].split(", ")[:7]
    return _TILE_TAGS.get(", ".join(args), tile)


def linear(A, B, N, K, out0, epilogue, *, bias=None, A2=None, K1=None, rowv=None, colv=None, aux0=None,
           aux1=None, aux2=None, out_split=None, nsplit=None, nzero=None, adiv=1.0, odiv=1.0, beta=100.0,
           threshold=20.0, aux_beta=0.0, aux2_scale=0.0, tile=None, M=None, kalg=None, out1=None, head_w=None,
           head_b=None, head_out=None, head_idx=None, out0_b=None, out1_b=None):
    """out = epilogue((A|A2) @ B[:N].T / adiv) -- cn_linear.  MUL / TANGENT /
    BWD_SOFTPLUS read softplus' as sg = 1 - exp(-aux_beta * aux0) from the stored
    softplus output aux0 (include/copenerf.h).  kalg: the unpadded
    inner dimension (for the FLOP count of the kernel timer only).  A bfloat16 B
    selects the bf16 MFMA path (A rounded to bf16 on load, fp32 accumulate); K is
    then rounded up to 64, so A's columns up to that must exist (zero padding).
    A [K/16, N, 48] bfloat16 B (split_bf16x3) selects CN_MFMA_F32_BF16X6: the fp32
    GEMM computed from three bf16 terms per operand on the bf16 MFMA.
    EPI_SOFTPLUS_HEAD (the last SDF hidden layer): out0 = softplus activation (or
    None: not stored), out1 = colv * softplus' (or None), head_out[head_idx[m] or m]
    = out0[m] · head_w + head_b.
    tile: None (the library's choice), 1 (128x64), 2 (128x128 only: tests compare the tiles); bf16x6 only:
    3 (the two-per-CU 128x256 tile), 4 (the 256x256 tile), both for 128 < N <= 256 without rowv.
    bf16 operand images (bf16 MFMA mode only, ABI v10): A (with A2) may be bfloat16 -- the rounded
    operand itself, read instead of rounded on load; aux0 may be bfloat16 for BWD_RELU (its sign) and
    for MUL / TANGENT / BWD_SOFTPLUS (the activation σ is recovered from), BWD_SOFTPLUS's aux1 / aux2
    too (all three in one dtype);
    out0_b / out1_b (bfloat16, or None) receive the RNE bf16 image of every value written to out0 /
    out1, and out0 may then be None."""
    x6 = B.dim() == 3
    if x6 and (B.dtype != torch.bfloat16 or B.shape[2] != 48 or not B.is_contiguous()):
        raise RuntimeError(f"cn_linear: a 3-D B must be split_bf16x3's [K/16, N, 48] bfloat16 image (got "
                           f"{tuple(B.shape)}, {B.dtype}, strides {B.stride()})")
    if out0 is None and out0_b is None and epilogue != EPI_SOFTPLUS_HEAD:
        raise RuntimeError("cn_linear: out0 (or out0_b) is required")
    bf = B.dtype == torch.bfloat16 and not x6
    for t, n in ((A, "A"), (A2, "A2"), (B, "B"), (out0, "out0"), (aux0, "aux0"), (aux1, "aux1"), (aux2, "aux2"),
                 (out_split, "out_split"), (out1, "out1"), (out0_b, "out0_b"), (out1_b, "out1_b")):
        _need(t, n, ndim=3 if (x6 and t is B) else 2)
        if t is None or t is B:
            continue
        want_b = n in ("out0_b", "out1_b")
        may_b = bf and (n in ("A", "A2") or
                        (n == "aux0" and epilogue in (EPI_BWD_RELU, EPI_MUL, EPI_TANGENT, EPI_BWD_SOFTPLUS)) or
                        (n in ("aux1", "aux2") and epilogue == EPI_BWD_SOFTPLUS))
        if (t.dtype == torch.bfloat16) != want_b and not (may_b and t.dtype == torch.bfloat16):
            raise RuntimeError(f"cn_linear: {n} has dtype {t.dtype} (bfloat16 images: A / A2, the aux0 of MUL / "
                               f"TANGENT / BWD_SOFTPLUS / BWD_RELU, BWD_SOFTPLUS's aux1 / aux2 and out0_b / out1_b, "
                               f"in the bf16 MFMA mode only)")
    a_b = A.dtype == torch.bfloat16
    if A2 is not None and (A2.dtype == torch.bfloat16) != a_b:
        raise RuntimeError("cn_linear: A and A2 must have the same dtype")
    if aux1 is not None and aux2 is not None and aux1.dtype != aux2.dtype:
        raise RuntimeError("cn_linear: aux1 and aux2 must have the same dtype")
    if aux1 is not None and aux0 is not None and aux1.dtype != aux0.dtype:
        raise RuntimeError("cn_linear: BWD_SOFTPLUS's aux0, aux1 and aux2 must have the same dtype")
    if bf:
        K = rup(K, 64)
        K1 = rup(K1, 64) if K1 is not None else None
        if (A.stride(0) < (K1 or K)) or (A2 is not None and A2.stride(0) < K - K1):
            raise RuntimeError(f"cn_linear (bf16): A rows too short for K={K}")
    M = A.shape[0] if M is None else M
    # the epilogue reads bias / colv as float4
    bias = bias if bias is None or bias.data_ptr() % 16 == 0 else bias.clone()
    colv = colv if colv is None or colv.data_ptr() % 16 == 0 else colv.clone()
    if tile is None:
        tile = 1 if max(N, nzero or 0) <= 64 else 0
    bn = 64 if tile == 1 else 128
    b_rows, b_k = (B.shape[1], 16 * B.shape[0]) if x6 else (B.shape[0], B.shape[1])
    if b_rows < rup(N, bn) or b_k < K:
        raise RuntimeError(f"cn_linear: B {tuple(B.shape)} too small for N={N}, K={K} (tile {tile})")
    if any(t is not None and t.shape[0] < M for t in (out0, out1, out0_b, out1_b)):
        raise RuntimeError("cn_linear: an output has fewer rows than A")
    if epilogue == EPI_SOFTPLUS_HEAD:
        _need(head_w, "head_w", ndim=1)
        _need(head_b, "head_b", ndim=1)
        _need(head_out, "head_out", ndim=1)
        if not head_out.is_contiguous():
            raise RuntimeError("cn_linear: head_out must be contiguous")
        if head_w.numel() < N or head_w.stride(0) != 1:
            raise RuntimeError("cn_linear: head_w must be a contiguous [N] vector")
        if head_idx is None and head_out.numel() < M:
            raise RuntimeError("cn_linear: head_out has fewer than M elements")
        if head_idx is not None and (head_idx.dtype != torch.int32 or head_idx.numel() < M):
            raise RuntimeError("cn_linear: head_idx must be int32 with M elements")
        head_w = head_w if head_w.data_ptr() % 16 == 0 else head_w.clone()
    d = _lib.LinearDesc()
    d.A, d.A2, d.B, d.bias = _ptr(A), _ptr(A2), _ptr(B), _ptr(bias)
    d.rowv, d.colv, d.aux0, d.aux1 = _ptr(rowv), _ptr(colv), _ptr(aux0), _ptr(aux1)
    d.out0, d.out1, d.out_split = _ptr(out0), _ptr(out1), _ptr(out_split)
    d.head_w, d.head_b, d.head_out, d.head_idx = _ptr(head_w), _ptr(head_b), _ptr(head_out), _ptr(head_idx)
    d.aux2, d.ld_aux2 = _ptr(aux2), _ld(aux2)
    d.aux_beta, d.aux2_scale = aux_beta, aux2_scale
    d.lda, d.lda2, d.ldb = _ld(A), _ld(A2), (B.shape[1] if x6 else _ld(B))
    d.ld_aux0, d.ld_aux1, d.ld_out0, d.ld_out1, d.ld_split = _ld(aux0), _ld(aux1), _ld(out0), _ld(out1), _ld(out_split)
    d.M, d.N, d.K = M, N, K
    d.K1 = K1 if K1 is not None else K
    d.nzero = nzero if nzero is not None else N
    d.nsplit = nsplit if nsplit is not None else N
    d.epilogue, d.tile = epilogue, tile
    d.adiv, d.odiv, d.beta, d.threshold = adiv, odiv, beta, threshold
    d.mfma_dtype = 2 if x6 else (1 if bf else 0)
    d.a_bf16 = 1 if a_b else 0
    d.aux0_bf16 = 1 if (aux0 is not None and aux0.dtype == torch.bfloat16) else 0
    d.aux12_bf16 = 1 if (aux1 is not None and aux1.dtype == torch.bfloat16) else 0
    d.out0_b, d.ld_out0_b, d.out1_b, d.ld_out1_b = _ptr(out0_b), _ld(out0_b), _ptr(out1_b), _ld(out1_b)
    global _flip
    _flip ^= 1  # consecutive launches walk the rows in opposite directions
    d.flags = _flip
    if _timer is not None:
        e0 = _timer.start()
        _lib.check(_lib.load().cn_linear(d, _stream()), "cn_linear")
        name = kernel_name(_lib.load().cn_linear_kernel_name, d)
        tag = _tile_tag(name, tile) if (x6 or bf) else tile
        key = ("linear", tag, EPI_NAMES[epilogue] + ("+rowv" if rowv is not None else "") +
               ("+imgA" if a_b else "")) + (("bf16",) if bf else ("x6",) if x6 else ())
        _timer.symbols[key] = name
        ka = kalg or K
        # algorithmic HBM bytes: A (unpadded K) and every aux row read once, each output
        # element written once, the weight image once (bf16x6: 3 bf16 terms per weight)
        nb = (2.0 if a_b else 4.0) * M * ka + (6.0 if x6 else 2.0 if bf else 4.0) * N * ka
        nb += M * N * sum(t.element_size() for t in (out0, out1, aux0, aux1, aux2, out0_b, out1_b) if t is not None)
        nb += 4.0 * M * ((rowv is not None) + (head_out is not None) + (head_idx is not None))
        _timer.stop(key + ((M, N, K),) if _timer.detail else key, e0, 2.0 * M * N * ka, nb)
    else:
        _lib.check(_lib.load().cn_linear(d, _stream()), "cn_linear")
    return out0


WGRAD_MODES = {"fp32": 0, "bf16": 1, "bf16x6": 2}


def _wgrad_desc(Y0, X0, N, K, dW, db, Y1, X1, accumulate, mode, workspace=True):
    """The cn_wgrad descriptor of one weight gradient and the workspace it points into (workspace=False:
    none yet -- cn_wgrad_batch callers carve every job's slabs out of one buffer).  A bfloat16 Y0 / X0
    (with Y1 / X1 of the same dtype) is a bf16 operand image (bf16 mode)."""
    if mode not in WGRAD_MODES:
        raise ValueError(f"wgrad: mode must be one of {tuple(WGRAD_MODES)} (got {mode!r})")
    for t, n in ((Y0, "Y0"), (X0, "X0"), (Y1, "Y1"), (X1, "X1"), (dW, "dW")):
        _need(t, n)
    yb, xb = Y0.dtype == torch.bfloat16, X0.dtype == torch.bfloat16
    if (Y1 is not None and (Y1.dtype == torch.bfloat16) != yb) or (X1 is not None and (X1.dtype == torch.bfloat16) != xb):
        raise RuntimeError("wgrad: Y0 / Y1 and X0 / X1 must have the same dtype")
    if (yb or xb) and mode != "bf16":
        raise RuntimeError("wgrad: bfloat16 operand images only in the bf16 mode")
    M = Y0.shape[0]
    lib = _lib.load()
    ws = None
    d = _lib.WgradDesc()
    if workspace:
        nbytes = lib.cn_wgrad_workspace_bytes(M, N, K)
        ws = torch.empty(nbytes // 4 + 1, device=Y0.device, dtype=torch.float32)
        d.workspace, d.workspace_bytes = _ptr(ws), ws.numel() * 4
    d.Y0, d.X0, d.Y1, d.X1 = _ptr(Y0), _ptr(X0), _ptr(Y1), _ptr(X1)
    d.dW, d.db = _ptr(dW), _ptr(db)
    d.ldy0, d.ldx0, d.ldy1, d.ldx1, d.ld_dw = _ld(Y0), _ld(X0), _ld(Y1), _ld(X1), _ld(dW)
    d.M, d.N, d.K = M, N, rup(K, 64)
    d.npairs = 2 if Y1 is not None else 1
    d.n_out, d.k_out = dW.shape[0], dW.shape[1]
    d.accumulate = 1 if accumulate else 0
    d.mfma_dtype = WGRAD_MODES[mode]
    d.y_bf16, d.x_bf16 = int(yb), int(xb)
    return d, ws


def _wgrad_bytes(d, ops_):
    """Algorithmic HBM bytes of a weight gradient: every operand row read once."""
    Y0, X0 = ops_[0], ops_[1]
    return float(d.npairs * d.M * (d.n_out * Y0.element_size() + d.k_out * X0.element_size()))


def _wgrad_key(d, mode):
    # one launch class per kernel instance (1- and 2-pair calls share it, as in rocprof's stats)
    name = kernel_name(_lib.load().cn_wgrad_kernel_name, d)
    key = ("wgrad", name[len("void cn::"):name.index("(")].replace(" ", "")) + \
        (("bf16",) if mode == "bf16" else ("x6",) if mode == "bf16x6" else ())
    _timer.symbols[key] = name
    return key


def wgrad(Y0, X0, N, K, dW, *, db=None, Y1=None, X1=None, accumulate=False, mode="fp32"):
    """dW[:n_out, :k_out] (+)= Y0ᵀX0 (+ Y1ᵀX1), db = colsum(Y0) -- cn_wgrad.
    mode: "fp32" (exact fp32 MFMA), "bf16x6" (fp32 from three bf16 terms per
    operand on the bf16 MFMA) or "bf16" (operands rounded to bf16 on load,
    config C3's reduced-precision mode; Y / X may then be bfloat16 operand images)."""
    d, ws = _wgrad_desc(Y0, X0, N, K, dW, db, Y1, X1, accumulate, mode)
    lib = _lib.load()
    if _timer is not None:
        e0 = _timer.start()
        _lib.check(lib.cn_wgrad(d, _stream()), "cn_wgrad")
        key = _wgrad_key(d, mode)
        M = d.M
        _timer.stop(key + ((M, d.n_out, d.k_out),) if _timer.detail else key, e0,
                    2.0 * M * d.n_out * d.k_out * d.npairs, _wgrad_bytes(d, (Y0, X0)))
    else:
        _lib.check(lib.cn_wgrad(d, _stream()), "cn_wgrad")
    return dW


class WgradQueue(object):
    """Collects a backward pass's 256x256 stage-ring weight gradients and runs them with ONE
    cn_wgrad_batch call at flush(): one launch and one slab reduction instead of a launch, a
    full-chip slab write and a reduction each (other tile classes launch at add()).  The
    queue holds the operand tensors, so their memory stays allocated until the flush; the
    gradients are written by the flush (call it before anything reads them).  Every job's slabs
    come out of one workspace allocated at the flush, sized by the batch's own layout
    (cn_wgrad_batch_workspace_bytes: each job's share of the slices, not a full launch's)."""

    def __init__(self):
        self.jobs = []

    def add(self, Y0, X0, N, K, dW, *, db=None, Y1=None, X1=None, mode="fp32"):
        d, _ = _wgrad_desc(Y0, X0, N, K, dW, db, Y1, X1, False, mode, workspace=False)
        if "WgradBatch" not in kernel_name(_lib.load().cn_wgrad_kernel_name, d):
            # not a stage-ring job (e.g. K = 64 first layers): nothing to share, launch it now
            return wgrad(Y0, X0, N, K, dW, db=db, Y1=Y1, X1=X1, mode=mode)
        self.jobs.append((d, mode, (Y0, X0, Y1, X1)))
        return dW

    def flush(self):
        if not self.jobs:
            return
        # the batch layout (each job's share of the CUs) and the stream are the jobs' device's
        with torch.cuda.device(self.jobs[0][2][0].device):
            self._flush()

    def _flush(self):
        lib = _lib.load()
        n = len(self.jobs)
        arr = (_lib.WgradDesc * n)(*[d for d, _, _ in self.jobs])
        offs = (ctypes.c_int64 * n)()
        total = lib.cn_wgrad_batch_workspace_bytes(arr, n, offs)
        ws = torch.empty(total // 4 + 1, device=self.jobs[0][2][0].device, dtype=torch.float32)
        base = ws.data_ptr()
        for i in range(n):
            arr[i].workspace = base + offs[i]
            arr[i].workspace_bytes = total - offs[i]
        if _timer is not None:
            # the batch's time goes to the class of its first job; the FLOPs of all of them
            e0 = _timer.start()
            _lib.check(lib.cn_wgrad_batch(arr, n, _stream()), "cn_wgrad_batch")
            key = _wgrad_key(self.jobs[0][0], self.jobs[0][1])
            fl = sum(2.0 * d.M * d.n_out * d.k_out * d.npairs for d, _, _ in self.jobs)
            nb = sum(_wgrad_bytes(d, t) for d, _, t in self.jobs)
            _timer.stop(key + (("batch", n),) if _timer.detail else key, e0, fl, nb)
        else:
            _lib.check(lib.cn_wgrad_batch(arr, n, _stream()), "cn_wgrad_batch")
        self.jobs = []


def row_head(A, K, W, b, C, act, out, dst_index=None, ld_out=None):
    """out[dst(m)*ld_out + c] = act(A[m] . W[c] + b[c]); ld_out defaults to C (out [M, C])."""
    _need(A, "A")
    _need(W, "W")
    if dst_index is not None and (dst_index.dtype != torch.int32 or not dst_index.is_contiguous()):
        raise RuntimeError("row_head: dst_index must be contiguous int32")
    if not out.is_contiguous():
        raise RuntimeError("row_head: out must be contiguous")
    _lib.call("cn_row_head", A.shape[0], K, _ptr(A), _ld(A), _ptr(W), _ld(W), _ptr(b), C, act, _ptr(out),
              C if ld_out is None else ld_out, _ptr(dst_index), _stream())
    return out


def scale_cols(X, N, w, out, act_beta=0.0, rowv=None):
    """out = f(X) * w (* rowv[m]); f(X) = X (act_beta 0) or 1 - exp(-act_beta X): softplus'
    of stored activations."""
    _need(X, "X")
    _need(out, "out")
    if rowv is not None and (not rowv.is_contiguous() or rowv.numel() != X.shape[0]):
        raise RuntimeError("scale_cols: rowv must be a contiguous [M] tensor")
    _lib.call("cn_scale_cols", X.shape[0], N, _ptr(X), _ld(X), _ptr(w), _ptr(rowv), _ptr(out), _ld(out),
              float(act_beta), _stream())
    return out


def softplus_adjoint(act, N, out, *, act_beta, D=None, rowv=None, colv=None, aux1=None, aux2=None, aux2_scale=0.0,
                     cs_out=None, rs_out=None, cs_div=1.0):
    """out = (D + rowv (x) colv) * sg(act) + aux1 * aux2 * aux2_scale * (1 - sg) / sg -- cn_softplus_adjoint;
    cs_out[n] = Σ_m (rowv[m] act[m][n] + aux2[m][n]) / cs_div when given (lin8's sdf-row gradient),
    rs_out[0] = Σ_m rowv[m] / cs_div (its bias gradient)."""
    for t, n in ((act, "act"), (out, "out"), (D, "D"), (aux1, "aux1"), (aux2, "aux2")):
        _need(t, n)
        if t is not None and t.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError(f"softplus_adjoint: {n} must be float32 or a bfloat16 operand image")
    if aux1 is not None and aux2 is not None and aux1.dtype != aux2.dtype:
        raise RuntimeError("softplus_adjoint: aux1 and aux2 must have the same dtype")
    isb = lambda t: t is not None and t.dtype == torch.bfloat16  # noqa: E731
    in_bf16 = (1 if isb(D) else 0) | (2 if isb(act) else 0) | (4 if isb(aux1) else 0)
    if rowv is not None and (not rowv.is_contiguous() or rowv.numel() != act.shape[0]):
        raise RuntimeError("softplus_adjoint: rowv must be a contiguous [M] tensor")
    M = act.shape[0]
    ws = None
    if cs_out is not None:
        _need(cs_out, "cs_out", ndim=1)
        if not cs_out.is_contiguous() or cs_out.numel() < N:
            raise RuntimeError("softplus_adjoint: cs_out must be a contiguous [N] tensor")
        lib = _lib.load()
        ws = torch.empty(lib.cn_softplus_adjoint_workspace_bytes(M, N) // 4 + 1, device=act.device, dtype=torch.float32)
    _lib.call("cn_softplus_adjoint", M, N, _ptr(D), _ld(D), _ptr(act), _ld(act), float(act_beta),
              _ptr(rowv), _ptr(colv), _ptr(aux1), _ld(aux1), _ptr(aux2), _ld(aux2), float(aux2_scale), _ptr(out),
              _ld(out), int(out.dtype == torch.bfloat16), in_bf16, _ptr(cs_out),
              _ptr(rs_out if cs_out is not None else None), float(cs_div), _ptr(ws),
              0 if ws is None else ws.numel() * 4, _stream())
    return out


def colsum(X, K, out, *, w=None, wdiv=1.0, accumulate=False):
    _need(X, "X")
    M = X.shape[0]
    lib = _lib.load()
    ws = torch.empty(lib.cn_colsum_workspace_bytes(M, K) // 4 + 1, device=X.device, dtype=torch.float32)
    _lib.call("cn_colsum", M, K, _ptr(w), _ptr(X), _ld(X), wdiv, _ptr(out), 1 if accumulate else 0, _ptr(ws),
              ws.numel() * 4, _stream())
    return out


def sdf_embed(x, multires, scale, U0, U4e=None, u4div=1.0):
    """U0 = the encoding of x; U4e = its first columns / u4div; each fp32 or a bfloat16 operand image."""
    _need(x, "x")
    _need(U0, "U0")
    _need(U4e, "U4e")
    flags = int(U4e is not None and U4e.dtype == torch.bfloat16) | (2 if U0.dtype == torch.bfloat16 else 0)
    _lib.call("cn_sdf_embed", x.shape[0], _ptr(x), _ld(x), multires, scale, U0.shape[1], _ptr(U0), _ld(U0),
              _ptr(U4e), _ld(U4e), u4div, flags, _stream())
    return U0


def sdf_mlp(u0b, tail, Ws, biases, head_w, head_b, sdf, *, multires, skip_layer, skip_div, beta, threshold,
            idx=None, debug=None):
    """The sampler's SDF query in one launch (cn_sdf_mlp): sdf[idx[m] or m] from the embedding u0b [M, 64] and
    the skip tail [M, >= E] through lin0 .. lin7 and the head row -- bf16 mode: bf16 images of both and bf16 weight
    images [256][K]; bf16x6 mode (ABI v15, 3-D weight images [K/16, 256, 48]): fp32 inputs, bitwise the
    layer-by-layer bf16x6 query.  Raises if the library does not support the network's shape."""
    x6 = Ws[0].dim() == 3
    for t, n in ((u0b, "u0b"), (tail, "tail")):
        _need(t, n)
        if t.dtype != (torch.float32 if x6 else torch.bfloat16):
            raise RuntimeError(f"sdf_mlp: {n} must be {'fp32' if x6 else 'a bfloat16 image'} in this mode")
    if len(Ws) != 8 or len(biases) != 8:
        raise RuntimeError("sdf_mlp: 8 hidden layers")
    d = _lib.SdfMlpDesc()
    d.u0, d.tail, d.ld_u0, d.ld_t = _ptr(u0b), _ptr(tail), _ld(u0b), _ld(tail)
    d.M, d.n_layers = u0b.shape[0], 8
    d.hidden, d.kpad0 = (Ws[1].shape[1], 16 * Ws[0].shape[0]) if x6 else (Ws[1].shape[0], Ws[0].shape[1])
    d.multires, d.skip_layer = multires, skip_layer
    d.format = FORMATS["bf16x6"] if x6 else 0
    for i, (W, b) in enumerate(zip(Ws, biases)):
        _need(W, f"W{i}", ndim=3 if x6 else 2)
        rows = W.shape[1] if x6 else W.shape[0]
        if W.dtype != torch.bfloat16 or rows != 256 or not b.is_contiguous() or b.dtype != torch.float32 or \
                (x6 and (W.dim() != 3 or W.shape[2] != 48 or not W.is_contiguous())):
            raise RuntimeError(f"sdf_mlp: layer {i} needs a bf16 [256][K] weight image (bf16x6: a [K/16, 256, 48] "
                               f"term image) and an fp32 bias")
        d.W[i], d.ldw[i], d.bias[i] = W.data_ptr(), (256 if x6 else W.stride(0)), b.data_ptr()
    if not (head_w.is_contiguous() and head_w.numel() >= 256 and head_b.numel() >= 1):
        raise RuntimeError("sdf_mlp: head_w [256], head_b [1]")
    if not sdf.is_contiguous() or (idx is None and sdf.numel() < u0b.shape[0]):
        raise RuntimeError("sdf_mlp: sdf must be contiguous with M entries (or idx)")
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() < u0b.shape[0]):
        raise RuntimeError("sdf_mlp: idx must be int32 with M entries")
    d.head_w, d.head_b, d.sdf, d.idx = head_w.data_ptr(), head_b.data_ptr(), sdf.data_ptr(), _ptr(idx)
    d.skip_div, d.beta, d.threshold = skip_div, beta, threshold
    d.debug = _ptr(debug)  # tests: [8][M][256] (bf16; fp32 in the bf16x6 mode), every layer's input
    if _timer is not None:
        e0 = _timer.start()
        _lib.check(_lib.load().cn_sdf_mlp(d, _stream()), "cn_sdf_mlp")
        M = u0b.shape[0]
        ka = [16 * W.shape[0] if x6 else W.shape[1] for W in Ws]
        fl = sum(2.0 * M * 256 * k for k in ka)
        key = ("sdf_mlp",) + (("x6",) if x6 else ())
        _timer.symbols[key] = ("void cn::sdf_mlp_x6_kernel<false>(cn::SdfMlpX6Args)" if x6 else
                               "cn::sdf_mlp_kernel(cn::SdfMlpArgs)")
        _timer.stop(key, e0, fl, u0b.element_size() * M * (64 + tail.shape[1]) + 4.0 * M)
    else:
        _lib.check(_lib.load().cn_sdf_mlp(d, _stream()), "cn_sdf_mlp")
    return sdf


def sdf_net(lay, pk, layered=False):
    """cn_sdf_net of a packed SDF network (fields.SDFLayout + fields.pack_sdf's images), and the tensors
    it points into (hold them while the descriptor is used).  layered: never the fused cn_sdf_mlp query."""
    if lay.n_lin > _lib.SDF_MAX_LIN:
        raise RuntimeError(f"sdf_net: {lay.n_lin} Linear layers (at most {_lib.SDF_MAX_LIN})")
    n, keep = _lib.SdfNet(), []
    n.n_lin, n.skip, n.multires = lay.n_lin, lay.skip, lay.multires
    n.scale, n.beta, n.threshold = lay.scale, lay.beta, lay.threshold
    for l in range(lay.n_lin):
        n.in_dim[l], n.out_dim[l] = lay.in_dim[l], lay.out_dim[l]
    B0 = pk.Bf[0]
    x6 = B0.dim() == 3
    n.mfma_dtype = 2 if x6 else (1 if B0.dtype == torch.bfloat16 else 0)
    n.flags = 1 if layered else 0

    def aligned(t):
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
        keep.append(t)
        return t.data_ptr()

    for l in range(lay.n_lin - 1):
        B = pk.Bf[l]
        if not B.is_contiguous():
            raise RuntimeError(f"sdf_net: layer {l} image must be contiguous")
        keep.append(B)
        n.W[l] = B.data_ptr()
        n.w_rows[l], n.w_cols[l] = (B.shape[1], 16 * B.shape[0]) if x6 else (B.shape[0], B.shape[1])
        n.bias[l] = aligned(pk.b[l])
    n.head_w = aligned(pk.w80.reshape(-1))
    n.head_b = aligned(pk.b80.reshape(-1))
    for l in range(lay.n_lin - 1):  # the transposed images (cn_render_fwd's ∇ pass)
        B = pk.Bt[l]
        if not B.is_contiguous():
            raise RuntimeError(f"sdf_net: layer {l} transposed image must be contiguous")
        keep.append(B)
        n.Wt[l] = B.data_ptr()
        n.wt_rows[l], n.wt_cols[l] = (B.shape[1], 16 * B.shape[0]) if x6 else (B.shape[0], B.shape[1])
    n.head_wp = aligned(pk.w80p)
    return n, keep


def color_net(lay, pk):
    """cn_color_net of a packed RenderingNetwork (fields.ColorLayout + fields.pack_color's images, lin0 folded
    or not), and the tensors it points into."""
    n, keep = _lib.ColorNet(), []
    n.n_lin, n.d_feature, n.multires_view = lay.n_lin, lay.F, lay.multires_view
    for l in range(lay.n_lin):
        n.in_dim[l], n.out_dim[l] = lay.in_dim[l], lay.out_dim[l]
    B0 = pk.Bf[0]
    x6 = B0.dim() == 3
    n.mfma_dtype = 2 if x6 else (1 if B0.dtype == torch.bfloat16 else 0)

    def aligned(t):
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone()
        keep.append(t)
        return t.data_ptr()

    for l in range(lay.n_lin - 1):
        B = pk.Bf[l]
        keep.append(B)
        n.W[l] = B.data_ptr()
        n.w_rows[l], n.w_cols[l] = (B.shape[1], 16 * B.shape[0]) if x6 else (B.shape[0], B.shape[1])
        n.bias[l] = aligned(pk.b[l])
    n.head_w = aligned(pk.W3)
    n.head_b = aligned(pk.b3)

    def image(B):  # (pointer, rows, columns) of a GEMM image as cn_linear reads it
        keep.append(B)
        return (B.data_ptr(),) + ((B.shape[1], 16 * B.shape[0]) if x6 else (B.shape[0], B.shape[1]))

    for l in range(1, lay.n_lin - 1):  # the backward's transposed images (cn_render_bwd)
        n.Wt[l], n.wt_rows[l], n.wt_cols[l] = image(pk.Bt[l])
    n.Wtf, n.wtf_rows, n.wtf_cols = image(pk.Btf)
    n.Wxt, n.wxt_rows, n.wxt_cols = image(pk.Bxt)
    n.Wg = aligned(pk.Wg)
    n.wg_ld = pk.Wg.stride(0)
    return n, keep


_SIZES = {}


def _sized(fn, desc, *extra):
    """lib.<fn>(desc, *extra) memoised on the descriptor's shape key (_lib.shape_key): the composed entry
    points' planners run once per shape, not once more per call (the entry point itself re-plans into the
    caller's buffer and refuses a plan larger than it, so a stale size fails loudly, never silently)."""
    key = (fn, _lib.shape_key(desc), extra)
    n = _SIZES.get(key)
    if n is None:
        if len(_SIZES) > 4096:
            _SIZES.clear()
        n = _SIZES[key] = int(getattr(_lib.load(), fn)(ctypes.byref(desc), *extra))
    return n


def _check_render_inputs(fn, R, rays_o, rays_d, near, far, time_step, inv_s, car, t_rand=None, n_samples=None,
                         z=None):
    """The shapes and types the C side assumes (it takes R from rays_o and S from z): anything else would be
    read out of bounds on the device, so it is refused here with a RuntimeError, as ops.sample does."""
    for t, nm in ((rays_o, "rays_o"), (rays_d, "rays_d"), (near, "near"), (far, "far"), (time_step, "time_step"),
                  (inv_s, "inv_s"), (car, "cos_anneal_ratio"), (t_rand, "t_rand"), (z, "z")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
            raise RuntimeError(f"{fn}: {nm} must be a contiguous fp32 device tensor")
    if rays_o.shape != (R, 3) or rays_d.shape != (R, 3):
        raise RuntimeError(f"{fn}: rays_o and rays_d must be [R, 3] (got {tuple(rays_o.shape)}, {tuple(rays_d.shape)})")
    if near.numel() != R or far.numel() != R:
        raise RuntimeError(f"{fn}: near and far must hold R = {R} entries (got {near.numel()}, {far.numel()})")
    if time_step.numel() < 1 or inv_s.numel() < 1 or car.numel() < 1:
        raise RuntimeError(f"{fn}: time_step, inv_s and cos_anneal_ratio need one element each")
    if t_rand is not None and t_rand.shape != (R, n_samples):
        raise RuntimeError(f"{fn}: t_rand must be [R, n_samples] = [{R}, {n_samples}] (got {tuple(t_rand.shape)})")
    if z is not None and (z.dim() != 2 or z.shape[0] != R):
        raise RuntimeError(f"{fn}: z must be [R, S] with R = {R} rows (got {tuple(z.shape)})")


def render_fwd(sdf_net_, color_net_, rays_o, rays_d, near, far, time_step, inv_s, car, n_samples, n_importance,
               up_sample_steps, t_rand=None, z_in=None, philox=None):
    """NeuSRenderer.forward without gradient in one call (cn_render_fwd): returns z, pts, sdf, grad, rgb, color,
    depth, weights, cdf."""
    R, dev = rays_o.shape[0], rays_o.device
    _check_render_inputs("render_fwd", R, rays_o, rays_d, near, far, time_step, inv_s, car, t_rand=t_rand,
                         n_samples=n_samples, z=z_in)
    if z_in is not None:
        S = z_in.shape[1]
    else:
        k = n_importance // up_sample_steps if n_importance > 0 else 0
        S = n_samples + up_sample_steps * k
    f = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    out = dict(z=f(R, S), pts=f(R * S, 4), sdf=f(R * S), grad=f(R * S, 4), rgb=f(R * S, 3), color=f(R, 3),
               depth=f(R), weights=f(R, S), cdf=f(R, S))
    d = _lib.RenderDesc()
    d.R, d.n_samples, d.n_importance, d.up_sample_steps = R, n_samples, n_importance, up_sample_steps
    d.S_in = S if z_in is not None else 0
    d.rays_o, d.rays_d, d.near, d.far = _ptr(rays_o), _ptr(rays_d), _ptr(near), _ptr(far)
    d.t_rand, d.time_step, d.z_in = _ptr(t_rand), _ptr(time_step), _ptr(z_in)
    d.inv_s, d.cos_anneal_ratio = _ptr(inv_s), _ptr(car)
    d.sdf_net, d.color_net = ctypes.pointer(sdf_net_), ctypes.pointer(color_net_)
    _check_philox(philox)
    d.philox = _ptr(philox)
    for k, v in out.items():
        setattr(d, k, v.data_ptr())
    lib = _lib.load()
    ws = torch.empty(max(_sized("cn_render_fwd_workspace_bytes", d), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.cn_render_fwd(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_render_fwd")
    return out


def render_train_fwd(sdf_net_, color_net_, rays_o, rays_d, near, far, time_step, inv_s, car, n_coarse, z):
    """render_core at the samples z [R, S] keeping its backward's state -- cn_render_train_fwd: returns the outputs
    (pts [M, 4], sdf [M, 1], grad [M, 4], color [R, 3], depth [R, 1], weights, cdf [R, S]), the state buffer and the
    descriptor render_bwd takes (the inputs must stay alive and unchanged until then)."""
    R, S = z.shape
    M, dev = R * S, z.device
    _check_render_inputs("render_train_fwd", rays_o.shape[0], rays_o, rays_d, near, far, time_step, inv_s, car, z=z)
    f = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    out = dict(pts=f(M, 4), sdf=f(M, 1), grad=f(M, 4), color=f(R, 3), depth=f(R, 1), weights=f(R, S), cdf=f(R, S))
    d = _lib.RenderDesc()
    d.R, d.n_samples, d.S_in = R, n_coarse, S
    d.rays_o, d.rays_d, d.near, d.far = _ptr(rays_o), _ptr(rays_d), _ptr(near), _ptr(far)
    d.time_step, d.z_in, d.inv_s, d.cos_anneal_ratio = _ptr(time_step), _ptr(z), _ptr(inv_s), _ptr(car)
    d.sdf_net, d.color_net = ctypes.pointer(sdf_net_), ctypes.pointer(color_net_)
    for k, v in out.items():
        setattr(d, k, v.data_ptr())
    lib = _lib.load()
    state = torch.empty(max(_sized("cn_render_state_bytes", d), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.cn_render_train_fwd(ctypes.byref(d), _ptr(state), state.numel(), _stream()), "cn_render_train_fwd")
    return out, state, d


def render_bwd(d, state, *, dcolor=None, ddepth=None, dweights=None, dcdf=None, dsdf=None, dgrad=None, dpts=None,
               sdf_dWs, sdf_dbs, col_dWs, col_dbs, dinv_s, drays_o=None, drays_d=None):
    """The backward of render_train_fwd -- cn_render_bwd (upstream gradients contiguous float32 or None)."""
    for t in (dcolor, ddepth, dweights, dcdf, dsdf, dgrad, dpts):
        if t is not None and (not t.is_contiguous() or t.dtype != torch.float32):
            raise RuntimeError("render_bwd: upstream gradients must be contiguous float32")
    g = _lib.RenderGrads()
    g.dcolor, g.ddepth, g.dweights, g.dcdf = _ptr(dcolor), _ptr(ddepth), _ptr(dweights), _ptr(dcdf)
    g.dsdf, g.dgrad, g.dpts = _ptr(dsdf), _ptr(dgrad), _ptr(dpts)
    for l, (w, b) in enumerate(zip(sdf_dWs, sdf_dbs)):
        g.sdf_dW[l], g.sdf_db[l] = _ptr(w), _ptr(b)
    for l, (w, b) in enumerate(zip(col_dWs, col_dbs)):
        g.col_dW[l], g.col_db[l] = _ptr(w), _ptr(b)
    g.dinv_s, g.drays_o, g.drays_d = _ptr(dinv_s), _ptr(drays_o), _ptr(drays_d)
    lib = _lib.load()
    nb = _sized("cn_render_bwd_workspace_bytes", d, 1 if drays_o is not None else 0)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=state.device)
    _lib.check(lib.cn_render_bwd(ctypes.byref(d), ctypes.byref(g), _ptr(state), state.numel(), _ptr(ws), ws.numel(),
                                 _stream()), "cn_render_bwd")


def sdf_query(net, x, sdf, idx=None):
    """sdf[idx[m] or m] = SDFNetwork.sdf(x[m]) -- cn_sdf_query (net: sdf_net's descriptor)."""
    _need(x, "x")
    M = x.shape[0]
    if idx is not None and (idx.dtype != torch.int32 or idx.numel() < M or not idx.is_contiguous()):
        raise RuntimeError("sdf_query: idx must be contiguous int32 with M entries")
    if not sdf.is_contiguous() or (idx is None and sdf.numel() < M):
        raise RuntimeError("sdf_query: sdf must be contiguous with M entries (or idx)")
    lib = _lib.load()
    ws = torch.empty(max(int(lib.cn_sdf_query_workspace_bytes(ctypes.byref(net), M)), 1), dtype=torch.uint8,
                     device=x.device)
    _lib.check(lib.cn_sdf_query(ctypes.byref(net), M, _ptr(x), _ld(x), _ptr(sdf), _ptr(idx), _ptr(ws), ws.numel(),
                                _stream()), "cn_sdf_query")
    return sdf


def _mlp_desc(net, M, x=None, sdf=None, dsdf=None, dWs=None, dbs=None, dx=None):
    d = _lib.MlpDesc()
    d.M, d.x, d.net, d.sdf, d.dsdf, d.dx = M, _ptr(x), ctypes.pointer(net), _ptr(sdf), _ptr(dsdf), _ptr(dx)
    for l, (w, b) in enumerate(zip(dWs or [], dbs or [])):
        d.dW[l], d.db[l] = _ptr(w), _ptr(b)
    return d


def mlp_fwd(net, x, sdf):
    """sdf[m] = SDFNetwork.sdf(x[m]) keeping the activations the backward reads -- cn_mlp_fwd; returns the
    state buffer mlp_bwd takes (net: sdf_net's descriptor, with its transposed images)."""
    _need(x, "x")
    M = x.shape[0]
    if x.dim() != 2 or x.shape[1] != 4 or x.stride(0) != 4 or x.dtype != torch.float32:
        raise RuntimeError("mlp_fwd: x must be a contiguous float32 [M, 4]")
    if not sdf.is_contiguous() or sdf.numel() < M:
        raise RuntimeError("mlp_fwd: sdf must be contiguous with M entries")
    lib = _lib.load()
    d = _mlp_desc(net, M, x=x, sdf=sdf)
    state = torch.empty(max(_sized("cn_mlp_state_bytes", d), 1), dtype=torch.uint8, device=x.device)
    _lib.check(lib.cn_mlp_fwd(ctypes.byref(d), _ptr(state), state.numel(), _stream()), "cn_mlp_fwd")
    return state


def mlp_bwd(net, M, state, dsdf, dWs=None, dbs=None, dx=None):
    """The gradients of SDFNetwork.sdf from dsdf [M] -- cn_mlp_bwd: dWs[l] [out_dim, in_dim] / dbs[l]
    (every Linear, or None: dx only) and dx [M, 4] (or None)."""
    _need(dsdf, "dsdf", ndim=1)
    if not dsdf.is_contiguous() or dsdf.numel() < M:
        raise RuntimeError("mlp_bwd: dsdf must be contiguous with M entries")
    for t in list(dWs or []) + list(dbs or []) + [dx]:
        if t is not None and (not t.is_contiguous() or t.dtype != torch.float32):
            raise RuntimeError("mlp_bwd: gradients must be contiguous float32")
    lib = _lib.load()
    d = _mlp_desc(net, M, dsdf=dsdf, dWs=dWs, dbs=dbs, dx=dx)
    ws = torch.empty(max(_sized("cn_mlp_bwd_workspace_bytes", d), 1), dtype=torch.uint8,
                     device=dsdf.device)
    _lib.check(lib.cn_mlp_bwd(ctypes.byref(d), _ptr(state), state.numel(), _ptr(ws), ws.numel(), _stream()),
               "cn_mlp_bwd")


def sample(net, rays_o, rays_d, near, far, t_rand, time_step, n_samples, n_importance, up_sample_steps, z,
           philox=None):
    """z [R, n_samples + up_sample_steps * (n_importance // up_sample_steps)] -- cn_sample: coarse z and the
    up-sampling rounds with their SDF queries in one call (net: sdf_net's descriptor).  philox (with t_rand
    None): a device uint64 [2] (seed, offset) -- the jitter drawn on the device (cn_uniform_philox)."""
    _check_philox(philox)
    for t, nm in ((rays_o, "rays_o"), (rays_d, "rays_d"), (near, "near"), (far, "far"), (t_rand, "t_rand"),
                  (time_step, "time_step"), (z, "z")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise RuntimeError(f"sample: {nm} must be a contiguous fp32 tensor")
    R = z.shape[0]
    k = n_importance // up_sample_steps if n_importance > 0 else 0
    if z.shape[1] != n_samples + up_sample_steps * k or (t_rand is not None and t_rand.shape != (R, n_samples)):
        raise RuntimeError("sample: z [R, n_samples + up_sample_steps * k] and t_rand [R, n_samples]")
    d = _lib.SampleDesc()
    d.R, d.n_samples, d.n_importance, d.up_sample_steps = R, n_samples, n_importance, up_sample_steps
    d.rays_o, d.rays_d, d.near, d.far = _ptr(rays_o), _ptr(rays_d), _ptr(near), _ptr(far)
    d.t_rand, d.time_step, d.z = _ptr(t_rand), _ptr(time_step), _ptr(z)
    d.net, d.philox = ctypes.pointer(net), _ptr(philox)
    lib = _lib.load()
    ws = torch.empty(max(_sized("cn_sample_workspace_bytes", d), 1), dtype=torch.uint8, device=z.device)
    _lib.check(lib.cn_sample(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_sample")
    return z


def sdf_grad_assemble(multires, scale, U0, Q0, QE, G):
    _lib.call("cn_sdf_grad_assemble", U0.shape[0], multires, scale, _ptr(U0), _ld(U0), _ptr(Q0), _ld(Q0),
              _ptr(QE), _ld(QE), _ptr(G), _ld(G), _stream())
    return G


def sdf_tangent_prep(multires, scale, U0, v, T0, T4e=None, t4div=1.0):
    """T0 = the tangent of the encoding along v; T4e (fp32, or a bfloat16 image) = its first columns / t4div."""
    _need(v, "v")
    _need(T4e, "T4e")
    _lib.call("cn_sdf_tangent_prep", U0.shape[0], multires, scale, T0.shape[1], _ptr(U0), _ld(U0), _ptr(v),
              _ld(v), _ptr(T0), _ld(T0), _ptr(T4e), _ld(T4e), t4div, int(T4e is not None and T4e.dtype == torch.bfloat16),
              _stream())
    return T0


def color_extras(G, pts, dirs, dir_div, multires_view, ext):
    for t, n in ((G, "G"), (pts, "pts"), (dirs, "dirs"), (ext, "ext")):
        _need(t, n)
    _lib.call("cn_color_extras", G.shape[0], _ptr(G), _ld(G), _ptr(pts), _ld(pts), _ptr(dirs), _ld(dirs),
              dir_div, multires_view, ext.shape[1], _ptr(ext), _ld(ext), _stream())
    return ext


def rgb_head_bwd(drgb, rgb, H3, K, W3, dZ2, dW3, db3):
    M = rgb.shape[0]
    lib = _lib.load()
    ws = torch.empty(lib.cn_rgb_head_bwd_workspace_bytes(M, K) // 4 + 1, device=rgb.device, dtype=torch.float32)
    _lib.call("cn_rgb_head_bwd", M, K, _ptr(drgb), _ptr(rgb), _ptr(H3), _ld(H3), _ptr(W3), _ptr(dZ2), _ld(dZ2),
              1 if dZ2.dtype == torch.bfloat16 else 0, _ptr(dW3), _ptr(db3), _ptr(ws), ws.numel() * 4, _stream())


def patch_indices(h, w, ps, n_patches, key, out=None):
    """Flat pixel ids [n_patches * ps * ps] (int64) of distinct random patches -- cn_patch_indices;
    key: int32 [4] device tensor."""
    _need(key, "key", ndim=1)
    if key.dtype != torch.int32 or key.numel() < 4:
        raise RuntimeError("patch_indices: key must be an int32 tensor of 4 values")
    if out is None:
        out = torch.empty(n_patches * ps * ps, dtype=torch.int64, device=key.device)
    _lib.call("cn_patch_indices", h, w, ps, n_patches, _ptr(key), _ptr(out), _stream())
    return out


def _check_philox(so):
    if so is not None and (so.dtype != torch.uint64 or so.numel() < 2 or not so.is_contiguous() or not so.is_cuda):
        raise RuntimeError("philox: a contiguous device uint64 tensor [2] = (seed, offset)")


def uniform_philox(n, seed_offset, out=None):
    """out[i] in [0, 1) from Philox4x32-10 (counter (i // 4, offset), key seed) -- cn_uniform_philox; seed_offset
    is a device uint64 [2] read by the kernel (a replayed graph draws with its current value)."""
    _check_philox(seed_offset)
    out = torch.empty(n, device=seed_offset.device) if out is None else out
    _lib.call("cn_uniform_philox", n, _ptr(seed_offset), _ptr(out), _stream())
    return out


def coarse_z(near, far, n, t_rand, z):
    _lib.call("cn_coarse_z", z.shape[0], n, _ptr(near), _ptr(far), _ptr(t_rand), _ptr(z), _stream())
    return z


def points(rays_o, rays_d, z, t, pts, *, mid=False, near=None, far=None, n_coarse=0):
    R, n = z.shape
    _lib.call("cn_points", R, n, _ptr(rays_o), _ptr(rays_d), _ptr(z), _ptr(t), 1 if mid else 0, _ptr(near),
              _ptr(far), n_coarse, _ptr(pts), _stream())
    return pts


def up_sample_merge(z, sdf, n_imp, inv_s, z_out, z_new, sdf_out=None, new_dst=None):
    R, n = z.shape
    _lib.call("cn_up_sample_merge", R, n, n_imp, float(inv_s), _ptr(z), _ptr(sdf), _ptr(z_out), _ptr(z_new),
              _ptr(sdf_out), _ptr(new_dst), _stream())


def device_scalar(x, device) -> torch.Tensor:
    """A float / 0-d tensor as a 1-element fp32 device tensor (the kernels read schedule
    values such as cos_anneal_ratio from device memory, so a replayed graph sees updates)."""
    if isinstance(x, torch.Tensor):
        t = x.reshape(-1)[:1]
        if t.device != device or t.dtype != torch.float32:
            t = t.to(device=device, dtype=torch.float32)
        return t.contiguous()
    return torch.full((1,), float(x), device=device, dtype=torch.float32)


def composite_fwd(z, sdf, G, rgb, rays_d, inv_s, near, far, n_coarse, car, color, depth, weights, cdf):
    """car: cos_anneal_ratio as a 1-element device tensor (device_scalar)."""
    R, S = z.shape
    _lib.call("cn_composite_fwd", R, S, _ptr(z), _ptr(sdf), _ptr(G), G.stride(0), _ptr(rgb), _ptr(rays_d),
              _ptr(inv_s), _ptr(near), _ptr(far), n_coarse, _ptr(car), _ptr(color), _ptr(depth), _ptr(weights),
              _ptr(cdf), _stream())


def composite_bwd(z, sdf, G, rgb, rays_d, inv_s, near, far, n_coarse, car, dcolor, ddepth, dweights, dcdf,
                  dsdf, dG, drgb, dinv_part, drays_d=None):
    R, S = z.shape
    _lib.call("cn_composite_bwd", R, S, _ptr(z), _ptr(sdf), _ptr(G), G.stride(0), _ptr(rgb), _ptr(rays_d),
              _ptr(inv_s), _ptr(near), _ptr(far), n_coarse, _ptr(car), _ptr(dcolor), _ptr(ddepth),
              _ptr(dweights), _ptr(dcdf), _ptr(dsdf), _ptr(dG), _ptr(drgb), _ptr(dinv_part), _ptr(drays_d),
              _stream())


def points_bwd(z, dP, drays_o, drays_d, *, mid=False, near=None, far=None, n_coarse=0):
    """drays_o = sum_i dP_i, drays_d = sum_i dP_i * zz_i per ray -- cn_points_bwd."""
    _need(dP, "dP")
    R, n = z.shape
    _lib.call("cn_points_bwd", R, n, _ptr(z), 1 if mid else 0, _ptr(near), _ptr(far), n_coarse, _ptr(dP), _ld(dP),
              _ptr(drays_o), _ptr(drays_d), _stream())


def color_extras_bwd(d_ext, dirs, dir_div, multires_view, ddirs, accumulate=False):
    """ddirs [R,3] (+)= view-encoding gradient of d_ext -- cn_color_extras_bwd."""
    _need(d_ext, "d_ext")
    _need(dirs, "dirs")
    _lib.call("cn_color_extras_bwd", dirs.shape[0], dir_div, _ptr(d_ext), _ld(d_ext), _ptr(dirs), _ld(dirs),
              multires_view, _ptr(ddirs), 1 if accumulate else 0, _stream())
    return ddirs


def train_loss(color, gt, depth, normals, *, w_rgb=1.0, w_eik=0.1, w_edge=1.0, w_smooth=1e-4, patch=4, gamma=0.1,
               weights=None, nonfinite=None):
    """(loss [], dcolor [R,3], ddepth [R,1], dnormals [M,3]) -- cn_train_loss: the colour
    L1, eikonal, edge-aware and plain smoothness terms and their input gradients.
    normals may be any [M,3] row view (e.g. the first three columns of ∇ₓSDF).
    weights: optional device tensor [4] (w_rgb, w_eik, w_edge, w_smooth) read by the
    kernels (overrides the floats); nonfinite: optional device int32 [1] flag set when
    the loss is not finite."""
    for t, n in ((color, "color"), (gt, "gt"), (normals, "normals")):
        _need(t, n)
    _need(depth.reshape(-1, 1), "depth")
    R, M, dev = color.shape[0], normals.shape[0], color.device
    if not (color.is_contiguous() and gt.is_contiguous() and depth.is_contiguous()):
        raise RuntimeError("train_loss: color, gt and depth must be contiguous")
    lib = _lib.load()
    if weights is None:
        weights = torch.tensor([w_rgb, w_eik, w_edge, w_smooth], dtype=torch.float32).to(dev, non_blocking=True)
    elif weights.dtype != torch.float32 or weights.numel() != 4 or not weights.is_contiguous() or weights.device != dev:
        raise RuntimeError("train_loss: weights must be a contiguous fp32 [4] tensor on the loss device")
    if nonfinite is not None and (nonfinite.dtype != torch.int32 or nonfinite.device != dev):
        raise RuntimeError("train_loss: nonfinite must be an int32 tensor on the loss device")
    ws = torch.empty(lib.cn_train_loss_workspace_bytes(R, patch) // 8 + 1, device=dev, dtype=torch.float64)
    loss = torch.empty((), device=dev)
    dcolor = torch.empty_like(color)
    ddepth = torch.empty(R, 1, device=dev)
    dn = torch.empty(M, 3, device=dev)
    _lib.call("cn_train_loss", R, patch, M, _ptr(color), _ptr(gt), _ptr(depth), _ptr(normals), _ld(normals),
              _ptr(weights), float(gamma), _ptr(loss), _ptr(dcolor), _ptr(ddepth), _ptr(dn), 3, _ptr(nonfinite),
              _ptr(ws), ws.numel() * 8, _stream())
    return loss, dcolor, ddepth, dn


# ---------------------------------------------------------------------------
# Mesh extraction (ABI v16)
def _box(lo, hi):
    lo = [float(v) for v in (lo.tolist() if hasattr(lo, "tolist") else lo)]
    hi = [float(v) for v in (hi.tolist() if hasattr(hi, "tolist") else hi)]
    if len(lo) != 3 or len(hi) != 3:
        raise RuntimeError("copenerf: lo / hi must have three entries")
    return (_lib.c_f32 * 3)(*lo), (_lib.c_f32 * 3)(*hi)


def grid_points(dims, lo, hi, t, m0=0, M=None, out=None):
    """Rows (X[ix], Y[iy], Z[iz], t) of the linear indices [m0, m0 + M) of an nx x ny x nz grid, z fastest;
    every axis is torch.linspace(lo, hi, n) -- cn_grid_points.  t: float or 1-element device tensor."""
    nx, ny, nz = (int(n) for n in dims)
    M = nx * ny * nz - m0 if M is None else int(M)
    if out is None:
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("grid_points: t must be a device tensor (ops.device_scalar) when out is not given")
        out = torch.empty(max(M, 0), 4, device=t.device)
    _need(out, "out")
    if not out.is_contiguous() or out.shape[1] != 4 or out.shape[0] < M:
        raise RuntimeError("grid_points: out must be a contiguous [M, 4] tensor")
    t = device_scalar(t, out.device)
    clo, chi = _box(lo, hi)
    _lib.call("cn_grid_points", nx, ny, nz, clo, chi, _ptr(t), int(m0), M, _ptr(out), _stream())
    return out


def sdf_grid(net, dims, lo, hi, t, chunk_rows=0, out=None):
    """u [nx, ny, nz] = +SDFNetwork.sdf on the grid of grid_points, evaluated in chunks of chunk_rows rows
    (0: 2^20) without leaving the device -- cn_sdf_grid (net: sdf_net's descriptor).  The sign is the
    network's: negative inside.  isosurface orients its triangles toward larger u, so no negation."""
    nx, ny, nz = (int(n) for n in dims)
    if not isinstance(t, torch.Tensor) and out is None:
        raise RuntimeError("sdf_grid: t must be a device tensor (ops.device_scalar) when out is not given")
    dev = out.device if out is not None else t.device
    if out is None:
        out = torch.empty(nx, ny, nz, device=dev)
    _need(out, "out", ndim=3)
    if not out.is_contiguous() or tuple(out.shape) != (nx, ny, nz) or out.dtype != torch.float32:
        raise RuntimeError("sdf_grid: out must be a contiguous fp32 [nx, ny, nz] tensor")
    t = device_scalar(t, dev)
    d = _lib.SdfGridDesc()
    d.net, d.nx, d.ny, d.nz, d.chunk_rows = ctypes.pointer(net), nx, ny, nz, int(chunk_rows)
    d.lo, d.hi = _box(lo, hi)
    d.time_step, d.u = _ptr(t), _ptr(out)
    lib = _lib.load()
    ws = torch.empty(max(int(lib.cn_sdf_grid_workspace_bytes(ctypes.byref(d))), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.cn_sdf_grid(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_sdf_grid")
    return out


def _mesh_desc(u, threshold, lo, hi, counts):
    _need(u, "u", ndim=3)
    if u.dim() != 3 or not u.is_contiguous() or u.dtype != torch.float32:
        raise RuntimeError("isosurface: u must be a contiguous fp32 [nx, ny, nz] tensor")
    d = _lib.MeshDesc()
    d.nx, d.ny, d.nz = u.shape
    d.u, d.threshold, d.counts = _ptr(u), float(threshold), _ptr(counts)
    d.lo, d.hi = _box(lo, hi)
    return d


def mesh_count(u, threshold, lo, hi, observed=False):
    """The count pass of isosurface -- cn_mesh_count: (descriptor, workspace, counts) with counts a device
    int64 [2] = (vertices, triangles); the workspace keeps the edge masks and offsets mesh_emit reads.
    observed: cn_mesh_count_observed -- NaN in u means unobserved (pass the same flag to mesh_emit)."""
    counts = torch.empty(2, dtype=torch.int64, device=u.device if u.is_cuda else None)
    d = _mesh_desc(u, threshold, lo, hi, counts)
    lib = _lib.load()
    ws = torch.empty(max(int(lib.cn_mesh_workspace_bytes(d.nx, d.ny, d.nz)), 1), dtype=torch.uint8, device=u.device)
    fn = "cn_mesh_count_observed" if observed else "cn_mesh_count"
    _lib.check(getattr(lib, fn)(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), fn)
    return d, ws, counts


def mesh_emit(d, ws, vertices, triangles, counts=None, observed=False):
    """The emit pass -- cn_mesh_emit (observed: cn_mesh_emit_observed) into vertices fp32 [V, 3] / triangles int32
    [T, 3] with mesh_count's descriptor and workspace.  counts: the (V, T) read back from mesh_count, checked here
    against the buffers (the kernel checks the device counts again and writes nothing into buffers that are too
    small)."""
    _need(vertices, "vertices")
    _need(triangles, "triangles")
    if (vertices.dtype != torch.float32 or triangles.dtype != torch.int32 or not vertices.is_contiguous() or
            not triangles.is_contiguous() or vertices.shape[1] != 3 or triangles.shape[1] != 3):
        raise RuntimeError("mesh_emit: vertices fp32 [V, 3] and triangles int32 [T, 3], contiguous")
    if counts is not None and (vertices.shape[0] < counts[0] or triangles.shape[0] < counts[1]):
        raise RuntimeError(f"mesh_emit: buffers of {vertices.shape[0]} vertices / {triangles.shape[0]} triangles "
                           f"for counts {tuple(counts)}")
    d.vertices, d.max_vertices = _ptr(vertices) if vertices.shape[0] else None, vertices.shape[0]
    d.triangles, d.max_triangles = _ptr(triangles) if triangles.shape[0] else None, triangles.shape[0]
    _lib.call("cn_mesh_emit_observed" if observed else "cn_mesh_emit", ctypes.byref(d), _ptr(ws), ws.numel(), _stream())


def isosurface(u, threshold, lo, hi, observed=False):
    """The isosurface u = threshold of a device volume u [nx, ny, nz] over the box lo .. hi as a welded triangle
    mesh: (vertices fp32 [V, 3], triangles int32 [T, 3]), device tensors ((0, 3) when empty).  Marching
    tetrahedra on the Kuhn split; vertex and triangle order are fixed by the grid (include/copenerf.h), triangle
    normals point toward larger u.  Count pass, one 16-byte read-back, an exact allocation, emit pass.
    observed: NaN in u means unobserved (tsdf_finalize's volume) -- an edge carries a vertex only between two
    observed ends, a cell emits triangles only when its eight corners are observed; vertices on edges whose every
    cell was skipped remain, unreferenced (mesh_clean with min_triangles >= 1 removes them)."""
    d, ws, counts = mesh_count(u, threshold, lo, hi, observed)
    V, T = (int(c) for c in counts.tolist())
    vertices = torch.empty(V, 3, device=u.device)
    triangles = torch.empty(T, 3, dtype=torch.int32, device=u.device)
    if V or T:
        mesh_emit(d, ws, vertices, triangles, (V, T), observed)
    return vertices, triangles


# ---------------------------------------------------------------------------
# Vertex colours and floater removal (additive to ABI v22)
def vertex_dirs(G, sign=-1.0, out=None):
    """dirs [M, 3] = sign * G[:, :3] / max(|G[:, :3]|, 1e-12) -- cn_vertex_dirs (G: rows of ∇ₓSDF, [M, >= 3]);
    sign -1: the inward unit normals, the view directions of vertex colours."""
    _need(G, "G")
    if G.dtype != torch.float32 or G.shape[1] < 3:
        raise RuntimeError(f"vertex_dirs: G must be fp32 [M, >= 3] (got {G.dtype} {tuple(G.shape)})")
    M = G.shape[0]
    if out is None:
        out = torch.empty(M, 3, device=G.device)
    _need(out, "out")
    if out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (M, 3):
        raise RuntimeError("vertex_dirs: out must be a contiguous fp32 [M, 3] tensor")
    _lib.call("cn_vertex_dirs", M, _ptr(G), _ld(G) if M else 4, float(sign), _ptr(out), _stream())
    return out


def rgb8_pack(rgb, out=None):
    """uint8 floor(clamp(rgb, 0, 1) * 255 + 0.5) of a contiguous fp32 tensor, NaN -> 0 -- cn_rgb8_pack."""
    _need(rgb, "rgb", ndim=0)
    if rgb.dtype != torch.float32 or not rgb.is_contiguous():
        raise RuntimeError("rgb8_pack: rgb must be a contiguous fp32 tensor")
    if out is None:
        out = torch.empty(rgb.shape, dtype=torch.uint8, device=rgb.device)
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.shape != rgb.shape or out.device != rgb.device:
        raise RuntimeError("rgb8_pack: out must be a contiguous uint8 tensor of rgb's shape on its device")
    _lib.call("cn_rgb8_pack", rgb.numel(), _ptr(rgb), _ptr(out), _stream())
    return out


def point_colors(sdf_net_, color_net_, x, t, view_dir=None, chunk_rows=0, want_rgb8=False, want_grad=False):
    """The colour network at the device points x [M, 3] and the time value t (a 1-element device tensor), the
    view direction the inward unit normal of every point or, with view_dir (three host floats), that one
    direction normalised -- cn_point_colors with the networks' descriptors (sdf_net, color_net with the folded
    first layer).  Returns rgb fp32 [M, 3], then rgb8 uint8 [M, 3] and / or grad fp32 [M, 4] where asked."""
    _need(x, "x")
    if x.dtype != torch.float32 or not x.is_contiguous() or x.shape[1] != 3:
        raise RuntimeError(f"point_colors: x must be a contiguous fp32 [M, 3] tensor (got {x.dtype} {tuple(x.shape)})")
    M, dev = x.shape[0], x.device
    t = device_scalar(t, dev)
    rgb = torch.empty(M, 3, device=dev)
    rgb8 = torch.empty(M, 3, dtype=torch.uint8, device=dev) if want_rgb8 else None
    grad = torch.empty(M, 4, device=dev) if want_grad else None
    d = _lib.PointColorsDesc()
    d.M, d.x, d.time_step, d.chunk_rows = M, _ptr(x), _ptr(t), int(chunk_rows)
    d.sdf_net, d.color_net = ctypes.pointer(sdf_net_), ctypes.pointer(color_net_)
    if view_dir is not None:
        v = [float(c) for c in (view_dir.tolist() if hasattr(view_dir, "tolist") else view_dir)]
        if len(v) != 3:
            raise RuntimeError("point_colors: view_dir must have three entries")
        vd = (_lib.c_f32 * 3)(*v)
        d.view_dir = ctypes.cast(vd, ctypes.POINTER(_lib.c_f32))
    d.rgb, d.rgb8, d.grad = _ptr(rgb), _ptr(rgb8), _ptr(grad)
    lib = _lib.load()
    ws = torch.empty(max(int(lib.cn_point_colors_workspace_bytes(ctypes.byref(d))), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.cn_point_colors(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_point_colors")
    out = (rgb,) + ((rgb8,) if want_rgb8 else ()) + ((grad,) if want_grad else ())
    return out[0] if len(out) == 1 else out


# rounds between two reads of the device's `changed` flag: the first call's, doubled call by call up to the cap
LABEL_ROUNDS_PER_CALL, LABEL_ROUNDS_PER_CALL_MAX = 8, 256


def _mesh_clean_desc(fn, triangles, V):
    _need(triangles, "triangles")
    if triangles.dtype != torch.int32 or not triangles.is_contiguous() or triangles.shape[1] != 3:
        raise RuntimeError(f"{fn}: triangles must be a contiguous int32 [T, 3] device tensor")
    d = _lib.MeshCleanDesc()
    d.V, d.T = int(V), triangles.shape[0]
    d.triangles = _ptr(triangles) if d.T else None
    return d


def mesh_components_cap(V):
    """The most rounds mesh_components launches for V vertices."""
    return int(V) + 2 * LABEL_ROUNDS_PER_CALL_MAX


def mesh_components(triangles, V, rounds_per_call=LABEL_ROUNDS_PER_CALL):
    """(label int32 [V], rounds): label[v] = the smallest vertex id of v's connected component in the indexed
    triangle list triangles int32 [T, 3] over V vertices -- cn_mesh_label_init, then cn_mesh_label_rounds in
    calls of rounds_per_call rounds, doubled call by call up to LABEL_ROUNDS_PER_CALL_MAX, until the device's
    `changed` flag reads clear (one 4-byte read-back per call, like isosurface's read of the counts).  rounds
    counts every round launched, the confirming ones included.  The cap is V + 2 LABEL_ROUNDS_PER_CALL_MAX
    rounds: round r settles every vertex within r edges of its component's smallest id, so V rounds always
    suffice; labels still changing at the cap raise a RuntimeError."""
    d = _mesh_clean_desc("mesh_components", triangles, V)
    dev = triangles.device
    label = torch.empty(d.V, dtype=torch.int32, device=dev)
    d.label = _ptr(label) if d.V else None
    _lib.call("cn_mesh_label_init", ctypes.byref(d), _stream())
    rounds, cap, k = 0, mesh_components_cap(d.V), max(int(rounds_per_call), 1)
    if d.V == 0 or d.T == 0:
        return label, rounds
    changed = torch.empty(1, dtype=torch.int32, device=dev)
    while True:
        _lib.call("cn_mesh_label_rounds", ctypes.byref(d), k, _ptr(changed), _stream())
        rounds += k
        if not int(changed.item()):
            return label, rounds
        if rounds >= cap:
            raise RuntimeError(f"mesh_components: labels still changing after {rounds} rounds (cap {cap})")
        k = min(2 * k, LABEL_ROUNDS_PER_CALL_MAX, cap - rounds)


def mesh_component_sizes(triangles, label):
    """tri_count int32 [V]: the triangles of every component at its root id, 0 elsewhere --
    cn_mesh_component_sizes (label: mesh_components')."""
    d = _mesh_clean_desc("mesh_component_sizes", triangles, label.shape[0])
    if label.dtype != torch.int32 or not label.is_contiguous() or label.device != triangles.device:
        raise RuntimeError("mesh_component_sizes: label must be a contiguous int32 [V] tensor on triangles' device")
    tri_count = torch.empty_like(label)
    d.label, d.tri_count = (_ptr(label), _ptr(tri_count)) if d.V else (None, None)
    _lib.call("cn_mesh_component_sizes", ctypes.byref(d), _stream())
    return tri_count


def mesh_select(triangles, label, tri_count, keep_largest=False, min_triangles=0):
    """The select pass of mesh_clean -- cn_mesh_select: (descriptor, workspace, counts) with counts a device
    int64 [2] = (kept vertices, kept triangles); the workspace keeps the flags and offsets mesh_compact reads."""
    d = _mesh_clean_desc("mesh_select", triangles, label.shape[0])
    dev = triangles.device
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    d.label, d.tri_count = (_ptr(label), _ptr(tri_count)) if d.V else (None, None)
    d.keep_largest, d.min_triangles, d.counts = int(bool(keep_largest)), int(min_triangles), _ptr(counts)
    lib = _lib.load()
    ws = torch.empty(max(int(lib.cn_mesh_clean_workspace_bytes(d.V, d.T)), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.cn_mesh_select(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_mesh_select")
    return d, ws, counts


def mesh_compact(d, ws, kept_vertices, triangles_out, counts=None):
    """The compact pass -- cn_mesh_compact into kept_vertices int32 [V'] / triangles_out int32 [T', 3] with
    mesh_select's descriptor and workspace.  counts: the (V', T') read back from mesh_select, checked here against
    the buffers (the kernel checks the device counts again and writes nothing into buffers that are too small)."""
    for t, nm in ((kept_vertices, "kept_vertices"), (triangles_out, "triangles_out")):
        if t.dtype != torch.int32 or not t.is_contiguous() or not t.is_cuda:
            raise RuntimeError(f"mesh_compact: {nm} must be a contiguous int32 device tensor")
    if kept_vertices.dim() != 1 or triangles_out.dim() != 2 or triangles_out.shape[1] != 3:
        raise RuntimeError("mesh_compact: kept_vertices [V'] and triangles_out [T', 3]")
    if counts is not None and (kept_vertices.shape[0] < counts[0] or triangles_out.shape[0] < counts[1]):
        raise RuntimeError(f"mesh_compact: buffers of {kept_vertices.shape[0]} vertices / {triangles_out.shape[0]} "
                           f"triangles for counts {tuple(counts)}")
    d.kept_vertices, d.max_vertices = _ptr(kept_vertices) if kept_vertices.shape[0] else None, kept_vertices.shape[0]
    d.triangles_out, d.max_triangles = _ptr(triangles_out) if triangles_out.shape[0] else None, triangles_out.shape[0]
    _lib.call("cn_mesh_compact", ctypes.byref(d), _ptr(ws), ws.numel(), _stream())


def mesh_clean(vertices, triangles, keep_largest=False, min_triangles=0, stats=None):
    """Floater removal on the device: the mesh without the connected components that are not kept.  A component
    is kept if it has at least min_triangles triangles and, with keep_largest, is the one with the most triangles
    (a tie goes to the smaller smallest-vertex id).  Returns (vertices' [V', 3], triangles' int32 [T', 3]
    renumbered, kept_vertices int32 [V']: the original ids, ascending); kept vertices and triangles keep their
    order.  Labels (mesh_components), sizes, select, one 16-byte read-back, an exact allocation, compact,
    index_select.  stats: an optional dict that receives components / components_kept / rounds."""
    _need(vertices, "vertices")
    V = vertices.shape[0]
    label, rounds = mesh_components(triangles, V)
    tri_count = mesh_component_sizes(triangles, label)
    d, ws, counts = mesh_select(triangles, label, tri_count, keep_largest, min_triangles)
    Vk, Tk = (int(c) for c in counts.tolist())
    kept = torch.empty(Vk, dtype=torch.int32, device=triangles.device)
    tri = torch.empty(Tk, 3, dtype=torch.int32, device=triangles.device)
    mesh_compact(d, ws, kept, tri, (Vk, Tk))
    if stats is not None:
        roots = label == torch.arange(V, dtype=torch.int32, device=label.device)
        stats["components"] = int(roots.sum())
        stats["components_kept"] = int(roots[kept.long()].sum()) if Vk else 0
        stats["rounds"] = rounds
    return vertices.index_select(0, kept.long()), tri, kept


def mesh_select_mask(triangles, vmask):
    """mesh_select from a per-vertex mask -- cn_mesh_select_mask: (descriptor, workspace, counts) as mesh_select
    returns them, for mesh_compact.  vmask: a bool or uint8 [V] device tensor, not 0 where the vertex is kept; a
    triangle is kept when its three corners are."""
    if vmask.dtype == torch.bool:
        vmask = vmask.to(torch.uint8)
    if not vmask.is_cuda or vmask.dtype != torch.uint8 or vmask.dim() != 1 or not vmask.is_contiguous():
        raise RuntimeError("mesh_select_mask: vmask must be a contiguous bool or uint8 [V] device tensor")
    d = _mesh_clean_desc("mesh_select_mask", triangles, vmask.shape[0])
    if triangles.device != vmask.device:
        raise RuntimeError("mesh_select_mask: triangles and vmask on different devices")
    dev = triangles.device
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    d.counts = _ptr(counts)
    lib = _lib.load()
    ws = torch.empty(max(int(lib.cn_mesh_clean_workspace_bytes(d.V, d.T)), 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.cn_mesh_select_mask(ctypes.byref(d), _ptr(vmask) if d.V else None, _ptr(ws), ws.numel(), _stream()),
               "cn_mesh_select_mask")
    # cn_mesh_compact's checks want the two arrays of the component pass; it reads neither
    d.label = d.tri_count = _ptr(ws) if d.V else None
    return d, ws, counts


def mesh_cull(vertices, triangles, keep_mask):
    """The mesh without the vertices whose keep_mask (bool or uint8 [V]) is 0 and without the triangles that had
    one as a corner.  Returns what mesh_clean returns: (vertices' [V', 3], triangles' int32 [T', 3] renumbered,
    kept_vertices int32 [V']: the original ids, ascending); kept vertices and triangles keep their order."""
    _need(vertices, "vertices")
    if keep_mask.shape[0] != vertices.shape[0]:
        raise RuntimeError(f"mesh_cull: a mask of {keep_mask.shape[0]} for {vertices.shape[0]} vertices")
    d, ws, counts = mesh_select_mask(triangles, keep_mask)
    Vk, Tk = (int(c) for c in counts.tolist())
    kept = torch.empty(Vk, dtype=torch.int32, device=triangles.device)
    tri = torch.empty(Tk, 3, dtype=torch.int32, device=triangles.device)
    mesh_compact(d, ws, kept, tri, (Vk, Tk))
    return vertices.index_select(0, kept.long()), tri, kept


# ---------------------------------------------------------------------------
# Mesh geometry metrics (additive to ABI v22): cn_mesh_eval.hip
NN_MAX_CELLS = 1 << 26


def _need_cloud(fn, t, name, cols=3, dtype=torch.float32):
    _need(t, name, ndim=0)
    if t.dtype != dtype or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous():
        raise RuntimeError(f"{fn}: {name} must be a contiguous {dtype} [n, {cols}] device tensor (got {t.dtype}, "
                           f"shape {tuple(t.shape)})")


def _workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def mesh_area(vertices, triangles):
    """The first phase of the surface sampler -- cn_mesh_area: (handle, area) with area a device double [1], the
    mesh's area (the sum of the triangle areas in double from the fp32 vertices), and handle what mesh_sample
    takes: the descriptor, the workspace that keeps the areas' inclusive scan, and the mesh's tensors.  Reading
    area (one host read) lets the caller fix the number of samples by density."""
    _need_cloud("mesh_area", vertices, "vertices")
    _need_cloud("mesh_area", triangles, "triangles", dtype=torch.int32)
    dev = vertices.device
    d = _lib.MeshSampleDesc()
    d.V, d.T = vertices.shape[0], triangles.shape[0]
    d.vertices, d.triangles = _ptr(vertices) if d.V else None, _ptr(triangles) if d.T else None
    area = torch.empty(1, dtype=torch.float64, device=dev)
    d.area = _ptr(area)
    lib = _lib.load()
    ws = _workspace(lib.cn_mesh_sample_workspace_bytes(d.T), dev)
    _lib.check(lib.cn_mesh_area(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_mesh_area")
    return (d, ws, (vertices, triangles)), area


def mesh_sample(handle, S, seed_offset, want_tri=False):
    """S points uniformly by area on the mesh of mesh_area's handle -- cn_mesh_sample: (points fp32 [S, 3],
    tri int32 [S] or None).  seed_offset: a device uint64 [2] = (seed, offset); sample i takes elements
    4 i .. 4 i + 2 of uniform_philox's stream for it."""
    d, ws, _ = handle
    _check_philox(seed_offset)
    dev = ws.device
    S = int(S)
    points = torch.empty(max(S, 0), 3, dtype=torch.float32, device=dev)
    tri = torch.empty(max(S, 0), dtype=torch.int32, device=dev) if want_tri else None
    d.S, d.philox = S, _ptr(seed_offset)
    d.points, d.tri = (_ptr(points), _ptr(tri)) if S > 0 else (None, None)
    _lib.call("cn_mesh_sample", ctypes.byref(d), _ptr(ws), ws.numel(), _stream())
    return points, tri


class NnGrid:
    """A built point grid (nn_grid): the descriptor and the device buffers it points into."""

    def __init__(self, d, points, cell_start, sorted_):
        self.desc, self.points, self.cell_start, self.sorted = d, points, cell_start, sorted_
        self.origin, self.cell, self.dims = tuple(d.origin), float(d.cell), tuple(d.dims)


def nn_grid(points, origin, cell, dims):
    """cn_nn_grid_build: the uniform grid of dims cubic cells of edge `cell` from `origin` over points fp32
    [N, 3]: cell_start int32 [ncells + 1] and the points sorted by cell as 16-byte records (x, y, z, original
    index).  Points outside the grid go to the nearest boundary cell."""
    _need_cloud("nn_grid", points, "points")
    dev = points.device
    dims = tuple(int(x) for x in dims)
    ncells = dims[0] * dims[1] * dims[2]
    if min(dims) < 1 or ncells > NN_MAX_CELLS:
        raise RuntimeError(f"nn_grid: dims {dims} (each at least 1, at most 2^26 cells)")
    d = _lib.NnGridDesc()
    d.N = points.shape[0]
    d.points = _ptr(points) if d.N else None
    d.origin, d.cell, d.dims = (_lib.c_f32 * 3)(*[float(x) for x in origin]), float(cell), (_lib.c_i32 * 3)(*dims)
    cell_start = torch.empty(ncells + 1, dtype=torch.int32, device=dev)
    sorted_ = torch.empty(max(d.N, 1), 4, dtype=torch.float32, device=dev)
    d.cell_start, d.sorted = _ptr(cell_start), _ptr(sorted_)
    lib = _lib.load()
    ws = _workspace(lib.cn_nn_grid_workspace_bytes(d.N, ncells), dev)
    _lib.check(lib.cn_nn_grid_build(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_nn_grid_build")
    return NnGrid(d, points, cell_start, sorted_)


def nn_query(grid, queries, max_dist=math.inf, want_index=True, records=False):
    """cn_nn_query: (dist fp32 [Q], index int32 [Q] or None), the distance to and the original index of the
    nearest point of `grid` for every query, exact, ties to the smaller index; (max_dist, -1) where no point is
    nearer than max_dist.  queries: fp32 [Q, 3], or with records=True the `sorted` records [Q, 4] of an nn_grid
    over the queries -- then every output lands at its query's original position."""
    _need_cloud("nn_query", queries, "queries", cols=4 if records else 3)
    if queries.device != grid.sorted.device:
        raise RuntimeError("nn_query: queries and grid on different devices")
    dev = queries.device
    Q = queries.shape[0]
    dist = torch.empty(Q, dtype=torch.float32, device=dev)
    index = torch.empty(Q, dtype=torch.int32, device=dev) if want_index else None
    d = _lib.NnQueryDesc()
    d.grid = ctypes.pointer(grid.desc)
    d.Q, d.queries, d.query_records, d.max_dist = Q, _ptr(queries) if Q else None, int(bool(records)), float(max_dist)
    d.dist, d.index = (_ptr(dist), _ptr(index)) if Q else (None, None)
    _lib.call("cn_nn_query", ctypes.byref(d), _stream())
    return dist, index


KNN_MAX_K = 32


def knn_query(grid, queries, k, max_dist=math.inf, exclude_self=False, want_count=False, records=False):
    """cn_knn_query: (dist fp32 [Q, k], index int32 [Q, k], count int32 [Q] or None), for every query the exact k
    nearest points of `grid`, each row ascending under (squared distance, original index) and padded with
    (max_dist, -1) where fewer than k points are nearer than max_dist.  queries as in nn_query (records=True: the
    `sorted` records of an nn_grid over the queries).  exclude_self leaves out the target whose original index is the
    query's own; it needs as many queries as the grid has points."""
    _need_cloud("knn_query", queries, "queries", cols=4 if records else 3)
    if queries.device != grid.sorted.device:
        raise RuntimeError("knn_query: queries and grid on different devices")
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise RuntimeError(f"knn_query: k {k} (in [1, {KNN_MAX_K}])")
    dev = queries.device
    Q = queries.shape[0]
    if exclude_self and Q != grid.desc.N:
        raise RuntimeError(f"knn_query: exclude_self with {Q} queries of {grid.desc.N} targets")
    dist = torch.empty(Q, k, dtype=torch.float32, device=dev)
    index = torch.empty(Q, k, dtype=torch.int32, device=dev)
    count = torch.empty(Q, dtype=torch.int32, device=dev) if want_count else None
    d = _lib.KnnQueryDesc()
    d.grid = ctypes.pointer(grid.desc)
    d.Q, d.queries, d.query_records, d.max_dist = Q, _ptr(queries) if Q else None, int(bool(records)), float(max_dist)
    d.k, d.exclude_self = k, int(bool(exclude_self))
    if Q:
        d.dist, d.index, d.count = _ptr(dist), _ptr(index), _ptr(count) if want_count else None
    _lib.call("cn_knn_query", ctypes.byref(d), _stream())
    return dist, index, count


# ---------------------------------------------------------------------------
# Point-cloud preparation (additive to ABI v22): cn_cloud.hip
VOXEL_KEY_NONE = (1 << 63) - 1
VOXEL_AXIS_BITS = 21


def voxel_keys(points, origin, voxel, want_valid=False):
    """cn_voxel_keys: (keys int64 [N], valid int32 [N] or None), the 63-bit voxel key of every point for voxels of
    edge `voxel` from `origin` (three 21-bit indices, x highest); VOXEL_KEY_NONE and valid 0 for a point that is
    not finite or outside the 21-bit range."""
    _need_cloud("voxel_keys", points, "points")
    voxel = float(voxel)
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise RuntimeError(f"voxel_keys: voxel size {voxel}")
    dev = points.device
    N = points.shape[0]
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    valid = torch.empty(N, dtype=torch.int32, device=dev) if want_valid else None
    d = _lib.VoxelKeysDesc()
    d.N, d.origin, d.voxel = N, (_lib.c_f32 * 3)(*[float(x) for x in origin]), voxel
    if N:
        d.points, d.keys, d.valid = _ptr(points), _ptr(keys), _ptr(valid) if want_valid else None
    _lib.call("cn_voxel_keys", ctypes.byref(d), _stream())
    return keys, valid


def voxel_reduce(keys, order, points, normals=None, colors=None):
    """cn_voxel_reduce over the keys sorted ascending by a stable sort and `order`, the original index of every
    sorted element (torch.sort(stable=True)'s two outputs): a dict with points fp32 [N, 3] (the voxel means, the
    first M rows written), normals / colors (where given: the re-normalised mean normal, the mean colour), counts
    int32 [N], keys int64 [N] and totals, a device int32 [2] = (M, points dropped); the voxels are in ascending key
    order.  The caller reads totals (one host read) and keeps the first M rows."""
    _need_cloud("voxel_reduce", points, "points")
    dev = points.device
    N = points.shape[0]
    for t, name in ((keys, "keys"), (order, "order")):
        if t.dtype != torch.int64 or tuple(t.shape) != (N,) or not t.is_contiguous() or t.device != dev:
            raise RuntimeError(f"voxel_reduce: {name} must be a contiguous int64 [{N}] device tensor (got {t.dtype} "
                               f"{tuple(t.shape)})")
    d = _lib.VoxelReduceDesc()
    d.N = N
    out = {"points": torch.empty(N, 3, dtype=torch.float32, device=dev), "normals": None, "colors": None,
           "counts": torch.empty(N, dtype=torch.int32, device=dev), "keys": torch.empty(N, dtype=torch.int64, device=dev),
           "totals": torch.empty(2, dtype=torch.int32, device=dev)}
    for t, name in ((normals, "normals"), (colors, "colors")):
        if t is None:
            continue
        _need_cloud("voxel_reduce", t, name)
        if t.shape[0] != N or t.device != dev:
            raise RuntimeError(f"voxel_reduce: {name} {tuple(t.shape)} for {N} points")
        out[name] = torch.empty(N, 3, dtype=torch.float32, device=dev)
    d.totals = _ptr(out["totals"])
    if N:
        d.keys, d.order, d.points = _ptr(keys), _ptr(order), _ptr(points)
        d.out_points, d.out_counts, d.out_keys = _ptr(out["points"]), _ptr(out["counts"]), _ptr(out["keys"])
        if normals is not None:
            d.normals, d.out_normals = _ptr(normals), _ptr(out["normals"])
        if colors is not None:
            d.colors, d.out_colors = _ptr(colors), _ptr(out["colors"])
    lib = _lib.load()
    ws = _workspace(lib.cn_voxel_reduce_workspace_bytes(N), dev)
    _lib.check(lib.cn_voxel_reduce(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_voxel_reduce")
    return out


def _need_rows(fn, t, name, N, k, dtype):
    _need(t, name, ndim=0)
    if t.dtype != dtype or t.dim() != 2 or t.shape[0] != N or not 1 <= t.shape[1] <= KNN_MAX_K or not t.is_contiguous():
        raise RuntimeError(f"{fn}: {name} must be a contiguous {dtype} [{N}, k] device tensor with k in [1, {KNN_MAX_K}] "
                           f"(got {t.dtype}, shape {tuple(t.shape)})")
    if k is not None and t.shape[1] != k:
        raise RuntimeError(f"{fn}: {name} has {t.shape[1]} columns, {k} expected")


def cloud_normals(points, index, orient_to=None, want_variation=False):
    """cn_cloud_normals: (normals fp32 [N, 3], variation fp32 [N] or None) from every point's neighbour row index
    int32 [N, k] (knn_query's over the cloud itself): the unit eigenvector of the smallest eigenvalue of the
    neighbours' covariance, and the surface variation l0 / (l0 + l1 + l2).  Zero for fewer than 3 valid neighbours,
    non-finite input or a collinear neighbourhood.  orient_to (3 numbers): flipped towards that point; without it
    the component of largest magnitude is positive."""
    _need_cloud("cloud_normals", points, "points")
    N = points.shape[0]
    _need_rows("cloud_normals", index, "index", N, None, torch.int32)
    dev = points.device
    if index.device != dev:
        raise RuntimeError("cloud_normals: tensors on different devices")
    normals = torch.empty(N, 3, dtype=torch.float32, device=dev)
    variation = torch.empty(N, dtype=torch.float32, device=dev) if want_variation else None
    d = _lib.CloudNormalsDesc()
    d.N, d.k = N, index.shape[1]
    if orient_to is not None:
        d.orient, d.orient_to = 1, (_lib.c_f32 * 3)(*[float(x) for x in orient_to])
    if N:
        d.points, d.index, d.normals = _ptr(points), _ptr(index), _ptr(normals)
        d.variation = _ptr(variation) if want_variation else None
    _lib.call("cn_cloud_normals", ctypes.byref(d), _stream())
    return normals, variation


def knn_mean_stats(dist, index):
    """cn_knn_mean_stats: (mean fp32 [N], a device double [3] = (rows with a finite mean, the sum of those means,
    the sum of their squares)) over knn_query's dist fp32 [N, k] / index int32 [N, k]: per row the mean of the
    distances whose index is not -1 (+inf for a row without one)."""
    _need(dist, "dist", ndim=0)
    N = dist.shape[0] if dist.dim() == 2 else -1
    _need_rows("knn_mean_stats", dist, "dist", N, None, torch.float32)
    _need_rows("knn_mean_stats", index, "index", N, dist.shape[1], torch.int32)
    dev = dist.device
    if index.device != dev:
        raise RuntimeError("knn_mean_stats: tensors on different devices")
    mean = torch.empty(N, dtype=torch.float32, device=dev)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    d = _lib.KnnMeanStatsDesc()
    d.N, d.k, d.out = N, dist.shape[1], _ptr(out)
    if N:
        d.dist, d.index, d.mean = _ptr(dist), _ptr(index), _ptr(mean)
    lib = _lib.load()
    ws = _workspace(lib.cn_knn_mean_stats_workspace_bytes(N), dev)
    _lib.check(lib.cn_knn_mean_stats(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_knn_mean_stats")
    return mean, out


def cloud_stats(dist, threshold, max_dist=math.inf, points=None, crop_min=None, crop_max=None):
    """cn_cloud_stats: a device double [4] = (points inside the crop box, those with dist < max_dist, the sum of
    their distances, those of them with dist < threshold) over dist fp32 [Q]; points fp32 [Q, 3] with crop_min /
    crop_max (3 floats each) restrict it to a box, without them every point counts."""
    _need(dist, "dist", ndim=0)
    if dist.dtype != torch.float32 or dist.dim() != 1 or not dist.is_contiguous():
        raise RuntimeError("cloud_stats: dist must be a contiguous fp32 [Q] device tensor")
    dev = dist.device
    d = _lib.CloudStatsDesc()
    d.Q = dist.shape[0]
    d.dist = _ptr(dist) if d.Q else None
    if (crop_min is None) != (crop_max is None) or (crop_min is not None and points is None):
        raise RuntimeError("cloud_stats: a crop box needs crop_min, crop_max and points")
    if crop_min is not None:
        _need_cloud("cloud_stats", points, "points")
        if points.shape[0] != d.Q or points.device != dev:
            raise RuntimeError(f"cloud_stats: points {tuple(points.shape)} for {d.Q} distances")
        d.points = _ptr(points) if d.Q else None
        d.crop_min = (_lib.c_f32 * 3)(*[float(x) for x in crop_min])
        d.crop_max = (_lib.c_f32 * 3)(*[float(x) for x in crop_max])
    d.max_dist, d.threshold = float(max_dist), float(threshold)
    out = torch.empty(4, dtype=torch.float64, device=dev)
    d.out = _ptr(out)
    lib = _lib.load()
    ws = _workspace(lib.cn_cloud_stats_workspace_bytes(d.Q), dev)
    _lib.check(lib.cn_cloud_stats(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_cloud_stats")
    return out


def cloud_normal_stats(query_normals, target_normals, index, dist, max_dist=math.inf, points=None, crop_min=None,
                       crop_max=None):
    """cn_cloud_normal_stats: a device double [3] = (pairs counted, the sum of |q . t[index]| over them, pairs left
    out for a zero or non-finite normal) over query_normals fp32 [Q, 3], target_normals fp32 [N, 3] and nn_query's
    index int32 [Q] / dist fp32 [Q] (with the same max_dist).  A pair is counted when index >= 0, dist < max_dist, the
    query lies inside the crop box (points with crop_min / crop_max, as cloud_stats) and both normals are usable;
    both are normalised in the kernel."""
    _need_cloud("cloud_normal_stats", query_normals, "query_normals")
    _need_cloud("cloud_normal_stats", target_normals, "target_normals")
    dev = query_normals.device
    d = _lib.CloudNormalStatsDesc()
    d.Q, d.N = query_normals.shape[0], target_normals.shape[0]
    _need(index, "index", ndim=0)
    _need(dist, "dist", ndim=0)
    if index.dtype != torch.int32 or tuple(index.shape) != (d.Q,) or not index.is_contiguous() or \
            dist.dtype != torch.float32 or tuple(dist.shape) != (d.Q,) or not dist.is_contiguous():
        raise RuntimeError(f"cloud_normal_stats: index int32 [{d.Q}] and dist fp32 [{d.Q}] contiguous device tensors "
                           f"(got {index.dtype} {tuple(index.shape)}, {dist.dtype} {tuple(dist.shape)})")
    if any(t.device != dev for t in (target_normals, index, dist)):
        raise RuntimeError("cloud_normal_stats: tensors on different devices")
    if (crop_min is None) != (crop_max is None) or (crop_min is not None and points is None):
        raise RuntimeError("cloud_normal_stats: a crop box needs crop_min, crop_max and points")
    if crop_min is not None:
        _need_cloud("cloud_normal_stats", points, "points")
        if points.shape[0] != d.Q or points.device != dev:
            raise RuntimeError(f"cloud_normal_stats: points {tuple(points.shape)} for {d.Q} queries")
        d.points = _ptr(points) if d.Q else None
        d.crop_min = (_lib.c_f32 * 3)(*[float(x) for x in crop_min])
        d.crop_max = (_lib.c_f32 * 3)(*[float(x) for x in crop_max])
    if d.Q:
        d.query_normals, d.index, d.dist = _ptr(query_normals), _ptr(index), _ptr(dist)
    d.target_normals = _ptr(target_normals) if d.N else None
    d.max_dist = float(max_dist)
    out = torch.empty(3, dtype=torch.float64, device=dev)
    d.out = _ptr(out)
    lib = _lib.load()
    ws = _workspace(lib.cn_cloud_normal_stats_workspace_bytes(d.Q), dev)
    _lib.check(lib.cn_cloud_normal_stats(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_cloud_normal_stats")
    return out


# ---------------------------------------------------------------------------
# ICP registration (additive to ABI v22): cn_mesh_eval.hip
ICP_SUMS = 32


def _sim12(fn, T):
    """The 12 fp32 numbers of a 4 x 4 similarity (numpy or tensor, any float dtype): its top three rows, rounded
    to fp32 once, here."""
    M = np.asarray(T.detach().cpu() if torch.is_tensor(T) else T, dtype=np.float64)
    if M.shape != (4, 4):
        raise RuntimeError(f"{fn}: the transform must be 4 x 4, got {M.shape}")
    return (_lib.c_f32 * 12)(*M[:3].astype(np.float32).reshape(-1).tolist())


def cloud_transform(points, T, out=None):
    """cn_cloud_transform: fp32 [N, 3] = the 4 x 4 similarity T applied to points fp32 [N, 3], by the one device
    function icp_accumulate applies it with (an ICP iteration's correspondences are nn_query over this output)."""
    _need_cloud("cloud_transform", points, "points")
    if out is None:
        out = torch.empty_like(points)
    else:
        _need_cloud("cloud_transform", out, "out")
        if out.shape != points.shape or out.device != points.device:
            raise RuntimeError("cloud_transform: out must match points")
    d = _lib.CloudTransformDesc()
    d.N, d.matrix = points.shape[0], _sim12("cloud_transform", T)
    d.points, d.out = (_ptr(points), _ptr(out)) if d.N else (None, None)
    _lib.call("cn_cloud_transform", ctypes.byref(d), _stream())
    return out


def icp_accumulate(source, targets, index, T, pivot, mode, target_normals=None):
    """cn_icp_accumulate: a device double [32], the sums of one ICP iteration over the pairs (source[i],
    targets[index[i]]) with index[i] >= 0 (nn_query's index over cloud_transform(source, T)), the source taken through
    the 4 x 4 similarity T, relative to pivot
    (3 numbers).  mode 0: point-to-point, mode 1: point-to-plane with target_normals fp32 [N, 3]; the slots are
    laid out in copenerf.h."""
    _need_cloud("icp_accumulate", source, "source")
    _need_cloud("icp_accumulate", targets, "targets")
    _need(index, "index", ndim=0)
    dev = source.device
    d = _lib.IcpAccumulateDesc()
    d.Q, d.N = source.shape[0], targets.shape[0]
    if index.dtype != torch.int32 or tuple(index.shape) != (d.Q,) or not index.is_contiguous():
        raise RuntimeError(f"icp_accumulate: index must be a contiguous int32 [{d.Q}] device tensor (got {index.dtype} "
                           f"{tuple(index.shape)})")
    if mode not in (0, 1):
        raise RuntimeError(f"icp_accumulate: mode {mode} (0 point-to-point, 1 point-to-plane)")
    if mode == 1:
        if target_normals is None:
            raise RuntimeError("icp_accumulate: mode 1 needs target_normals")
        _need_cloud("icp_accumulate", target_normals, "target_normals")
        if target_normals.shape[0] != d.N:
            raise RuntimeError(f"icp_accumulate: {target_normals.shape[0]} normals for {d.N} targets")
        d.target_normals = _ptr(target_normals) if d.N else None
    if any(t.device != dev for t in (targets, index) + ((target_normals,) if mode == 1 else ())):
        raise RuntimeError("icp_accumulate: tensors on different devices")
    if d.Q:
        d.source, d.index = _ptr(source), _ptr(index)
    d.targets = _ptr(targets) if d.N else None
    d.matrix, d.mode = _sim12("icp_accumulate", T), int(mode)
    d.pivot = (ctypes.c_double * 3)(*[float(x) for x in pivot])
    out = torch.empty(ICP_SUMS, dtype=torch.float64, device=dev)
    d.out = _ptr(out)
    lib = _lib.load()
    ws = _workspace(lib.cn_icp_accumulate_workspace_bytes(d.Q), dev)
    _lib.check(lib.cn_icp_accumulate(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_icp_accumulate")
    return out


# ---------------------------------------------------------------------------
# Mesh depth rendering and visibility (additive to ABI v22): cn_mesh_raster.hip
MESH_NEAR = 1e-4  # the default near bound on a corner's (or a point's) depth c


def _need_proj(fn, proj, dev):
    _need(proj, "proj", ndim=0)
    if proj.dtype != torch.float32 or proj.dim() != 3 or tuple(proj.shape[1:]) != (3, 4) or not proj.is_contiguous():
        raise RuntimeError(f"{fn}: proj must be a contiguous fp32 [N, 3, 4] device tensor (got {proj.dtype}, "
                           f"shape {tuple(proj.shape)})")
    if proj.device != dev:
        raise RuntimeError(f"{fn}: proj on another device")


def mesh_raster(vertices, triangles, proj, h, w, near=MESH_NEAR, view_batch=0, pixel_budget=0, stats=None):
    """Depth rendering of an indexed triangle mesh -- cn_mesh_raster: (depth fp32 [N, h, w], +inf where nothing is
    seen; tri int32 [N, h, w], the triangle seen, -1 where none) of vertices fp32 [V, 3] / triangles int32 [T, 3]
    under the projections proj fp32 [N, 3, 4] (copenerf.mesh.camera_projection).  Two-sided inclusive coverage of
    pixel centres without cracks along shared edges, perspective-correct depth, the nearest triangle wins and equal
    depths go to the smaller id; a triangle with a corner at depth < near is skipped (no clipping).  view_batch /
    pixel_budget: 0 for the library's defaults (8 views per pass; boxes of up to 64 pixels walked by one thread).
    stats: an optional dict that receives thread_pairs / group_pairs, the (triangle, view) pairs each path walked
    (one 16-byte read-back)."""
    _need_cloud("mesh_raster", vertices, "vertices")
    _need_cloud("mesh_raster", triangles, "triangles", dtype=torch.int32)
    dev = vertices.device
    if triangles.device != dev:
        raise RuntimeError("mesh_raster: vertices and triangles on different devices")
    _need_proj("mesh_raster", proj, dev)
    d = _lib.MeshRasterDesc()
    d.V, d.T, d.N, d.h, d.w = vertices.shape[0], triangles.shape[0], proj.shape[0], int(h), int(w)
    d.view_batch, d.near, d.pixel_budget = int(view_batch), float(near), int(pixel_budget)
    if d.h < 1 or d.w < 1:
        raise RuntimeError(f"mesh_raster: image {d.h} x {d.w}")
    d.vertices, d.triangles = _ptr(vertices) if d.V else None, _ptr(triangles) if d.T else None
    depth = torch.empty(d.N, d.h, d.w, dtype=torch.float32, device=dev)
    tri = torch.empty(d.N, d.h, d.w, dtype=torch.int32, device=dev)
    counters = torch.zeros(2, dtype=torch.int64, device=dev) if stats is not None else None
    d.proj, d.depth, d.tri, d.stats = (_ptr(proj), _ptr(depth), _ptr(tri), _ptr(counters)) if d.N else (None,) * 4
    lib = _lib.load()
    ws = _workspace(lib.cn_mesh_raster_workspace_bytes(d.V, d.T, d.N, d.h, d.w, d.view_batch), dev)
    _lib.check(lib.cn_mesh_raster(ctypes.byref(d), _ptr(ws), ws.numel(), _stream()), "cn_mesh_raster")
    if stats is not None:
        stats["thread_pairs"], stats["group_pairs"] = (int(c) for c in counters.tolist())
    return depth, tri


def mesh_visibility(points, proj, h, w, depth=None, tol_abs=0.0, tol_rel=0.0, near=MESH_NEAR):
    """count int32 [Q]: the views that see each of points fp32 [Q, 3] -- cn_mesh_visibility.  A view sees a point
    at depth c >= near whose pixel (rounded to the nearest centre) lies inside the h x w image and, with depth
    fp32 [N, h, w] (mesh_raster's), c <= depth[pixel] (1 + tol_rel) + tol_abs.  Without depth: the frustum test."""
    _need_cloud("mesh_visibility", points, "points")
    dev = points.device
    _need_proj("mesh_visibility", proj, dev)
    d = _lib.MeshVisibilityDesc()
    d.Q, d.N, d.h, d.w, d.near = points.shape[0], proj.shape[0], int(h), int(w), float(near)
    d.tol_abs, d.tol_rel = float(tol_abs), float(tol_rel)
    if depth is not None:
        _need(depth, "depth", ndim=0)
        if depth.dtype != torch.float32 or tuple(depth.shape) != (d.N, d.h, d.w) or not depth.is_contiguous() or \
                depth.device != dev:
            raise RuntimeError(f"mesh_visibility: depth must be a contiguous fp32 [{d.N}, {d.h}, {d.w}] tensor on the "
                               f"points' device (got {depth.dtype}, shape {tuple(depth.shape)})")
        d.depth = _ptr(depth) if d.N else None
    count = torch.empty(d.Q, dtype=torch.int32, device=dev)
    d.points, d.count = (_ptr(points), _ptr(count)) if d.Q else (None, None)
    d.proj = _ptr(proj) if d.N else None
    _lib.call("cn_mesh_visibility", ctypes.byref(d), _stream())
    return count


# ---------------------------------------------------------------------------
# TSDF fusion (additive to ABI v22): cn_tsdf.hip
def _need_volume(fn, t, name, shape):
    _need(t, name, ndim=0)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError(f"{fn}: {name} must be a contiguous fp32 {list(shape)} device tensor (got {t.dtype}, "
                           f"shape {tuple(t.shape)})")


def tsdf_integrate(tsum, wsum, lo, hi, proj, depth, trunc, *, csum=None, color=None, near=MESH_NEAR,
                   depth_max=math.inf, brick_reject=True):
    """Fuse the views proj fp32 [N, 3, 4] / depth fp32 [N, h, w] (and color fp32 [N, h, w, 3]) into the running
    volumes tsum, wsum fp32 [nx, ny, nz] (and csum [nx, ny, nz, 3]) over the box lo .. hi, in place --
    cn_tsdf_integrate.  A voxel that projects, at depth c >= near, onto a pixel with a finite depth d in
    (0, depth_max] and d - c >= -trunc adds min(1, (d - c) / trunc) to tsum, 1 to wsum and the pixel's colour to
    csum.  Bitwise repeatable, and equal to any split of the views over several calls; the volumes are read and
    written once per call (fusion.VIEWS_PER_CALL: the batch measured fastest).  brick_reject=False turns the
    wavefront-level frustum skip off (it never changes a result; for measurement)."""
    _need_volume("tsdf_integrate", tsum, "tsum", tsum.shape)
    if tsum.dim() != 3:
        raise RuntimeError(f"tsdf_integrate: tsum must be [nx, ny, nz] (got shape {tuple(tsum.shape)})")
    dev, dims = tsum.device, tuple(tsum.shape)
    _need_volume("tsdf_integrate", wsum, "wsum", dims)
    _need_proj("tsdf_integrate", proj, dev)
    _need(depth, "depth", ndim=0)
    if depth.dtype != torch.float32 or depth.dim() != 3 or depth.shape[0] != proj.shape[0] or not depth.is_contiguous():
        raise RuntimeError(f"tsdf_integrate: depth must be a contiguous fp32 [{proj.shape[0]}, h, w] device tensor (got "
                           f"{depth.dtype}, shape {tuple(depth.shape)})")
    if (csum is None) != (color is None):
        raise RuntimeError("tsdf_integrate: csum and color go together (both or neither)")
    if csum is not None:
        _need_volume("tsdf_integrate", csum, "csum", dims + (3,))
        _need_volume("tsdf_integrate", color, "color", tuple(depth.shape) + (3,))
    for t, nm in ((wsum, "wsum"), (depth, "depth"), (csum, "csum"), (color, "color")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"tsdf_integrate: {nm} on another device")
    d = _lib.TsdfDesc()
    d.nx, d.ny, d.nz = dims
    d.lo, d.hi = _box(lo, hi)
    d.N, d.h, d.w = depth.shape
    d.trunc, d.near, d.depth_max, d.no_reject = float(trunc), float(near), float(depth_max), int(not brick_reject)
    d.tsum, d.wsum, d.csum = _ptr(tsum), _ptr(wsum), _ptr(csum)
    d.proj, d.depth, d.color = (_ptr(proj), _ptr(depth), _ptr(color)) if d.N else (None, None, _ptr(color))
    _lib.call("cn_tsdf_integrate", ctypes.byref(d), _stream())


def tsdf_finalize(tsum, wsum, csum=None, min_weight=1.0):
    """u fp32 [nx, ny, nz] = tsum / wsum where wsum >= min_weight (>= 1), NaN elsewhere (unobserved) --
    cn_tsdf_finalize; with csum also rgb fp32 [nx, ny, nz, 3] = csum / wsum there, 0 elsewhere: (u, rgb)."""
    _need_volume("tsdf_finalize", tsum, "tsum", tsum.shape)
    if tsum.dim() != 3:
        raise RuntimeError(f"tsdf_finalize: tsum must be [nx, ny, nz] (got shape {tuple(tsum.shape)})")
    dims = tuple(tsum.shape)
    _need_volume("tsdf_finalize", wsum, "wsum", dims)
    if csum is not None:
        _need_volume("tsdf_finalize", csum, "csum", dims + (3,))
    u = torch.empty_like(tsum)
    rgb = torch.empty_like(csum) if csum is not None else None
    d = _lib.TsdfFinalizeDesc()
    d.nx, d.ny, d.nz = dims
    d.min_weight = float(min_weight)
    d.tsum, d.wsum, d.csum, d.u, d.rgb = _ptr(tsum), _ptr(wsum), _ptr(csum), _ptr(u), _ptr(rgb)
    _lib.call("cn_tsdf_finalize", ctypes.byref(d), _stream())
    return u if csum is None else (u, rgb)


def volume_sample(attr, points, lo, hi, mask=None, fill=0.0):
    """out fp32 [Q, C]: the trilinear interpolation of attr fp32 [nx, ny, nz, C] (C 1 .. 4; [nx, ny, nz] counts as
    C = 1) over the box lo .. hi at points fp32 [Q, 3] -- cn_volume_sample; a point outside the box samples the
    nearest face.  mask: a u volume [nx, ny, nz] whose NaN mean unobserved -- such corners get weight 0, the rest
    are renormalised, and a point whose observed corners carry no weight gets `fill`."""
    _need(attr, "attr", ndim=0)
    if attr.dtype != torch.float32 or attr.dim() not in (3, 4) or not attr.is_contiguous():
        raise RuntimeError(f"volume_sample: attr must be a contiguous fp32 [nx, ny, nz, C] device tensor (got {attr.dtype}, "
                           f"shape {tuple(attr.shape)})")
    dims, C = tuple(attr.shape[:3]), attr.shape[3] if attr.dim() == 4 else 1
    _need_cloud("volume_sample", points, "points")
    if mask is not None:
        _need_volume("volume_sample", mask, "mask", dims)
    if points.device != attr.device or (mask is not None and mask.device != attr.device):
        raise RuntimeError("volume_sample: attr, points and mask on different devices")
    out = torch.empty(points.shape[0], C, device=attr.device)
    d = _lib.VolumeSampleDesc()
    d.nx, d.ny, d.nz = dims
    d.C, d.Q, d.fill = C, points.shape[0], float(fill)
    d.lo, d.hi = _box(lo, hi)
    d.attr, d.mask = _ptr(attr), _ptr(mask)
    d.points, d.out = (_ptr(points), _ptr(out)) if d.Q else (None, None)
    _lib.call("cn_volume_sample", ctypes.byref(d), _stream())
    return out


MESH_SHADE_GREY = 0.8  # the albedo of a mesh shaded without colours


def mesh_shade(vertices, triangles, proj, tri, *, attr=None, vnormals=None, rot=None, want=("normal",), fill=0.0,
               light=(0.0, 0.0, 1.0), ambient=0.3, grey=MESH_SHADE_GREY, albedo_from_attr=False, background=(255, 255, 255)):
    """What mesh_raster's tri int32 [N, h, w] shows -- cn_mesh_shade: a dict with the outputs named in `want`:
      "attr"          fp32 [N, h, w, C]: attr fp32 [V, C] (1 <= C <= 16) interpolated perspective-correctly, `fill`
                      where nothing is seen;
      "normal"        fp32 [N, h, w, 3]: the unit normal turned towards the camera -- the triangle's own, or with
                      vnormals fp32 [V, 3] the interpolated vertex normal -- rotated by rot fp32 [N, 3, 3] when given;
                      zero where nothing is seen;
      "normal_image"  uint8 [N, h, w, 3]: normal * 128 + 128, visualize's picture of a normal map;
      "shaded"        uint8 [N, h, w, 3]: albedo (ambient + (1 - ambient) max(0, normal . light)) * 255, the albedo
                      `grey` or, with albedo_from_attr, the first three channels of the interpolated attr ([0, 1]);
    the pictures show `background` (three uint8) where nothing is seen.  light is used as given (a unit vector in
    the normals' frame).  One thread per pixel, no atomics: given tri the result is bitwise repeatable."""
    _need_cloud("mesh_shade", vertices, "vertices")
    _need_cloud("mesh_shade", triangles, "triangles", dtype=torch.int32)
    dev = vertices.device
    if triangles.device != dev:
        raise RuntimeError("mesh_shade: vertices and triangles on different devices")
    _need_proj("mesh_shade", proj, dev)
    _need(tri, "tri", ndim=0)
    if tri.dtype != torch.int32 or tri.dim() != 3 or tri.shape[0] != proj.shape[0] or not tri.is_contiguous() or tri.device != dev:
        raise RuntimeError(f"mesh_shade: tri must be a contiguous int32 [{proj.shape[0]}, h, w] tensor on the vertices' "
                           f"device (got {tri.dtype}, shape {tuple(tri.shape)})")
    want = tuple(want)
    unknown = set(want) - {"attr", "normal", "normal_image", "shaded"}
    if unknown or not want:
        raise RuntimeError(f"mesh_shade: want {want} (of attr, normal, normal_image, shaded)")
    d = _lib.MeshShadeDesc()
    d.V, d.T, d.N, d.h, d.w = vertices.shape[0], triangles.shape[0], tri.shape[0], tri.shape[1], tri.shape[2]
    if d.h < 1 or d.w < 1:
        raise RuntimeError(f"mesh_shade: image {d.h} x {d.w}")
    d.vertices, d.triangles = _ptr(vertices) if d.V else None, _ptr(triangles) if d.T else None

    keep = []  # placeholders that must outlive the call

    def per_vertex(t, name, cols):
        _need_cloud("mesh_shade", t, name, cols=cols)
        if t.shape[0] != d.V or t.device != dev:
            raise RuntimeError(f"mesh_shade: {name} {tuple(t.shape)} for {d.V} vertices")
        if not d.V:  # (no vertex, so every pixel is background: the library still wants a pointer)
            keep.append(torch.zeros(1, cols, dtype=torch.float32, device=dev))
        return _ptr(t) if d.V else _ptr(keep[-1])

    if attr is not None:
        if attr.dim() != 2 or not 1 <= attr.shape[1] <= 16:
            raise RuntimeError(f"mesh_shade: attr must be [V, C] with 1 <= C <= 16 (got {tuple(attr.shape)})")
        d.C = attr.shape[1]
        d.attr = per_vertex(attr, "attr", d.C)
    elif "attr" in want or albedo_from_attr:
        raise RuntimeError("mesh_shade: the attr output and albedo_from_attr need attr")
    if albedo_from_attr and d.C < 3:
        raise RuntimeError(f"mesh_shade: albedo_from_attr needs at least 3 channels, attr has {d.C}")
    if vnormals is not None:
        d.vnormals = per_vertex(vnormals, "vnormals", 3)
    if rot is not None:
        _need(rot, "rot", ndim=0)
        if rot.dtype != torch.float32 or tuple(rot.shape) != (d.N, 3, 3) or not rot.is_contiguous() or rot.device != dev:
            raise RuntimeError(f"mesh_shade: rot must be a contiguous fp32 [{d.N}, 3, 3] tensor on the vertices' device "
                               f"(got {rot.dtype}, shape {tuple(rot.shape)})")
        d.rot = _ptr(rot) if d.N else None
    d.fill, d.ambient, d.grey, d.albedo_from_attr = float(fill), float(ambient), float(grey), int(bool(albedo_from_attr))
    d.light = (_lib.c_f32 * 3)(*[float(x) for x in light])
    d.background = (ctypes.c_uint8 * 3)(*[int(x) for x in background])
    out = {}
    if "attr" in want:
        out["attr"] = torch.empty(d.N, d.h, d.w, d.C, dtype=torch.float32, device=dev)
    if "normal" in want:
        out["normal"] = torch.empty(d.N, d.h, d.w, 3, dtype=torch.float32, device=dev)
    if "normal_image" in want:
        out["normal_image"] = torch.empty(d.N, d.h, d.w, 3, dtype=torch.uint8, device=dev)
    if "shaded" in want:
        out["shaded"] = torch.empty(d.N, d.h, d.w, 3, dtype=torch.uint8, device=dev)
    if d.N:
        d.proj, d.tri = _ptr(proj), _ptr(tri)
        for key, field in (("attr", "attr_out"), ("normal", "normal_out"), ("normal_image", "normal_img"), ("shaded", "shaded_img")):
            if key in out:
                setattr(d, field, _ptr(out[key]))
    _lib.call("cn_mesh_shade", ctypes.byref(d), _stream())
    return out


# ---------------------------------------------------------------------------
# Pose refinement (ABI v17)
class _RefineWarp(torch.autograd.Function):
    """cn_refine_warp: the forward launches the fused pass and keeps dpose = d sums[:, 0] / d pose; the
    backward is g_sums[:, 0, None] * dpose for the poses alone (the valid counts carry no gradient)."""

    @staticmethod
    def forward(ctx, pose, images, depth, tgt, src, K, Kinv, want_warped):
        N, _, H, W = images.shape
        J = tgt.shape[0]
        dev = images.device
        sums = torch.empty(J, 2, device=dev, dtype=torch.float32)
        dpose = torch.empty(J, 12, device=dev, dtype=torch.float32)
        warped = torch.empty(J, 3, H, W, device=dev, dtype=torch.float32) if want_warped else None
        lib = _lib.load()
        need = int(lib.cn_refine_workspace_bytes(J, H, W))
        if J and need == 0:
            _lib.check(lib.cn_refine_warp(N, H, W, J, None, None, None, None, None, None, None, None, None, None,
                                          None, 0, None), "cn_refine_warp")
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        p = pose.detach().reshape(J, 12).contiguous()
        _lib.call("cn_refine_warp", N, H, W, J, _ptr(images), _ptr(depth), _ptr(tgt), _ptr(src), _ptr(p), _ptr(K),
                  _ptr(Kinv), _ptr(sums), _ptr(dpose), _ptr(warped), _ptr(ws), ws.numel(),
                  torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(dpose)
        ctx.pose_shape = pose.shape
        if warped is None:
            warped = sums.new_empty(0)
        ctx.mark_non_differentiable(warped)
        return sums, warped

    @staticmethod
    def backward(ctx, g_sums, _g_warped):
        (dpose,) = ctx.saved_tensors
        return ((g_sums[:, 0, None] * dpose).reshape(ctx.pose_shape),) + (None,) * 7


def refine_warp(images, depth, tgt, src, pose, K, Kinv, want_warped=False):
    """The photometric warp of pose refinement for J (target, source) jobs -- cn_refine_warp.
    images fp32 [N, 3, H, W], depth fp32 [N, H, W] (contiguous), tgt / src int32 [J], pose [J, 3, 4] (or
    [J, 12]; the only differentiable input), K / Kinv fp32 [J, 3, 3].  Returns (sums [J, 2], warped):
    sums[:, 0] = the masked L1 sum, sums[:, 1] = the number of valid pixels (no gradient); warped
    [J, 3, H, W] when want_warped, else None."""
    for t, name in ((images, "images"), (depth, "depth"), (tgt, "tgt"), (src, "src"), (pose, "pose"), (K, "K"),
                    (Kinv, "Kinv")):
        _need(t, name, ndim=0)
    J = tgt.shape[0]
    if (images.dim() != 4 or images.shape[1] != 3 or images.dtype != torch.float32 or not images.is_contiguous()):
        raise RuntimeError("refine_warp: images must be a contiguous fp32 [N, 3, H, W] tensor")
    if (tuple(depth.shape) != (images.shape[0],) + tuple(images.shape[2:]) or depth.dtype != torch.float32 or
            not depth.is_contiguous()):
        raise RuntimeError("refine_warp: depth must be a contiguous fp32 [N, H, W] tensor of the images' size")
    if tgt.dtype != torch.int32 or src.dtype != torch.int32 or tuple(src.shape) != (J,) or tgt.dim() != 1:
        raise RuntimeError("refine_warp: tgt / src must be int32 [J] tensors")
    if pose.numel() != 12 * J or pose.dtype != torch.float32:
        raise RuntimeError("refine_warp: pose must be fp32 [J, 3, 4]")
    for t, name in ((K, "K"), (Kinv, "Kinv")):
        if tuple(t.shape) != (J, 3, 3) or t.dtype != torch.float32:
            raise RuntimeError(f"refine_warp: {name} must be fp32 [J, 3, 3]")
    sums, warped = _RefineWarp.apply(pose, images, depth, tgt.contiguous(), src.contiguous(), K.contiguous(),
                                     Kinv.contiguous(), bool(want_warped))
    return sums, (warped if want_warped else None)


# ---------------------------------------------------------------------------
# The flow-RGB term of stage 1 (ABI v21)
def _flow_rgb_args(fn, ray_acc, w2c, KS, pixn, pix, rgb_gt, images, frame, frame_valid):
    """Check the common inputs of cn_flow_rgb_fwd / _bwd; returns (R, T, N, H, W, the pointer arguments)."""
    for t, name in ((ray_acc, "ray_acc"), (w2c, "w2c"), (KS, "KS"), (pixn, "pixn"), (pix, "pix"), (rgb_gt, "rgb_gt"),
                    (images, "images")):
        _need(t, name, ndim=0)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != images.device:
            raise RuntimeError(f"{fn}: {name} must be a contiguous fp32 tensor on the images' device")
    if images.dim() != 4 or images.shape[1] != 3:
        raise RuntimeError(f"{fn}: images must be [N, 3, H, W] (got {tuple(images.shape)})")
    N, _, H, W = images.shape
    R, T = ray_acc.shape[0], w2c.shape[0]
    for t, name, shape in ((ray_acc, "ray_acc", (R, 4)), (w2c, "w2c", (T, 4, 4)), (KS, "KS", (T, 3, 3)),
                           (pixn, "pixn", (R, 2)), (pix, "pix", (R, 2)), (rgb_gt, "rgb_gt", (R, 3))):
        if tuple(t.shape) != shape:
            raise RuntimeError(f"{fn}: {name} must be {list(shape)} (got {list(t.shape)})")
    if (frame.dtype != torch.int64 or tuple(frame.shape) != (T,) or not frame.is_contiguous() or
            frame.device != images.device):
        raise RuntimeError(f"{fn}: frame must be a contiguous int64 [{T}] tensor on the images' device")
    if frame_valid is not None and (frame_valid.dtype != torch.uint8 or tuple(frame_valid.shape) != (T,) or
                                    not frame_valid.is_contiguous() or frame_valid.device != images.device):
        raise RuntimeError(f"{fn}: frame_valid must be a contiguous uint8 [{T}] tensor on the images' device")
    return R, T, N, H, W, (_ptr(ray_acc), _ptr(w2c), _ptr(KS), _ptr(pixn), _ptr(pix), _ptr(rgb_gt), _ptr(images),
                           _ptr(frame), _ptr(frame_valid))


def _flow_rgb_workspace(fn, R, T, dev):
    need = int(_lib.load().cn_flow_rgb_workspace_bytes(R, T))
    if need == 0:  # a shape the library refuses: let it say why
        _lib.check(_lib.load().cn_flow_rgb_fwd(R, T, 1, 1, 1, *([None] * 11), 0, None), fn)
    return torch.empty(need, dtype=torch.uint8, device=dev), need


def flow_rgb_fwd(ray_acc, w2c, KS, pixn, pix, rgb_gt, images, frame, frame_valid=None):
    """cn_flow_rgb_fwd: ray_acc [R, 4], w2c [T, 4, 4], KS [T, 3, 3], pixn / pix [R, 2], rgb_gt [R, 3], images
    [N, 3, H, W] (fp32, contiguous, one device), frame int64 [T], frame_valid uint8 [T] or None.  Returns sums
    fp32 [T, 2]: the masked L1 sum and the number of valid rays of each reference frame."""
    R, T, N, H, W, ptrs = _flow_rgb_args("flow_rgb_fwd", ray_acc, w2c, KS, pixn, pix, rgb_gt, images, frame, frame_valid)
    dev = images.device
    ws, need = _flow_rgb_workspace("cn_flow_rgb_fwd", R, T, dev)
    sums = torch.empty(T, 2, device=dev, dtype=torch.float32)
    _lib.call("cn_flow_rgb_fwd", R, T, N, H, W, *ptrs, _ptr(sums), _ptr(ws), need,
              torch.cuda.current_stream(dev).cuda_stream)
    return sums


def flow_rgb_bwd(ray_acc, w2c, KS, pixn, pix, rgb_gt, images, frame, frame_valid, g_num):
    """cn_flow_rgb_bwd: the inputs of flow_rgb_fwd and g_num fp32 [T] = d loss / d sums[:, 0].  Returns
    (d_ray_acc [R, 4], d_w2c [T, 3, 4])."""
    R, T, N, H, W, ptrs = _flow_rgb_args("flow_rgb_bwd", ray_acc, w2c, KS, pixn, pix, rgb_gt, images, frame, frame_valid)
    dev = images.device
    if (g_num.dtype != torch.float32 or tuple(g_num.shape) != (T,) or not g_num.is_contiguous() or
            g_num.device != dev):
        raise RuntimeError(f"flow_rgb_bwd: g_num must be a contiguous fp32 [{T}] tensor on the images' device")
    ws, need = _flow_rgb_workspace("cn_flow_rgb_bwd", R, T, dev)
    d_ray = torch.empty(R, 4, device=dev, dtype=torch.float32)
    d_w2c = torch.empty(T, 3, 4, device=dev, dtype=torch.float32)
    _lib.call("cn_flow_rgb_bwd", R, T, N, H, W, *ptrs, _ptr(g_num), _ptr(d_ray), _ptr(d_w2c), _ptr(ws), need,
              torch.cuda.current_stream(dev).cuda_stream)
    return d_ray, d_w2c


# ---------------------------------------------------------------------------
# Evaluation metrics (ABI v18)
def ssim_taps():
    """The 11 window weights by the reference's own expression (co3d_metric.py:49-51): exp in Python
    doubles, to fp32, divided by the fp32 sum."""
    from math import exp
    g = torch.tensor([exp(-(x - 11 // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    return g / g.sum()


_SSIM_TAPS_HOST = None  # the 11 taps as a host array, built on first use (cn_image_metrics copies them per call)


def _ssim_taps_host():
    global _SSIM_TAPS_HOST
    if _SSIM_TAPS_HOST is None:
        _SSIM_TAPS_HOST = (_lib.c_f32 * 11)(*ssim_taps().tolist())
    return _SSIM_TAPS_HOST


def _need_plane_stack(fn, t, name, ndim):
    _need(t, name, ndim=0)
    if t.dtype != torch.float32 or t.dim() != ndim or not t.is_contiguous():
        raise RuntimeError(f"{fn}: {name} must be a contiguous fp32 {ndim}-D tensor (got {t.dtype}, shape "
                           f"{tuple(t.shape)}, strides {t.stride()})")


def image_metrics(pred, gt, want_map=False):
    """cn_image_metrics on contiguous fp32 [N, C, H, W] device tensors.  Returns (out, ssim_map): out
    [N, C, 2] = (mean squared error, mean SSIM) per image and channel; ssim_map [N, C, H, W] when want_map,
    else None."""
    _need_plane_stack("image_metrics", pred, "pred", 4)
    _need_plane_stack("image_metrics", gt, "gt", 4)
    if pred.shape != gt.shape or pred.device != gt.device:
        raise RuntimeError(f"image_metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must agree")
    N, C, H, W = pred.shape
    dev = pred.device
    out = torch.empty(N, C, 2, device=dev, dtype=torch.float32)
    smap = torch.empty(N, C, H, W, device=dev, dtype=torch.float32) if want_map else None
    lib = _lib.load()
    need = int(lib.cn_image_metrics_workspace_bytes(N, C, H, W))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    _lib.call("cn_image_metrics", N, C, H, W, _ptr(pred), _ptr(gt), _ssim_taps_host(), _ptr(out), _ptr(smap), _ptr(ws), need,
              torch.cuda.current_stream(dev).cuda_stream)
    return out, smap


def depth_errors(gt, pred, ratio, min_depth, max_depth, clamp):
    """cn_depth_errors: gt fp32 [N, Hg, Wg], pred fp32 [N, Hp, Wp], ratio fp32 [N] (all on the device,
    contiguous).  Returns fp32 [N, 8]: abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, the valid count."""
    _need_plane_stack("depth_errors", gt, "gt", 3)
    _need_plane_stack("depth_errors", pred, "pred", 3)
    _need_plane_stack("depth_errors", ratio, "ratio", 1)
    N, Hg, Wg = gt.shape
    if pred.shape[0] != N or ratio.shape[0] != N or pred.device != gt.device or ratio.device != gt.device:
        raise RuntimeError(f"depth_errors: gt {tuple(gt.shape)}, pred {tuple(pred.shape)} and ratio "
                           f"{tuple(ratio.shape)} must hold the same number of images on one device")
    dev = gt.device
    out = torch.empty(N, 8, device=dev, dtype=torch.float32)
    lib = _lib.load()
    need = int(lib.cn_depth_errors_workspace_bytes(N, Hg, Wg))
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    _lib.call("cn_depth_errors", N, Hg, Wg, _ptr(gt), pred.shape[1], pred.shape[2], _ptr(pred), _ptr(ratio),
              float(min_depth), float(max_depth), int(bool(clamp)), _ptr(out), _ptr(ws), need,
              torch.cuda.current_stream(dev).cuda_stream)
    return out


def normal_errors(pred, gt, mask=None):
    """cn_normal_errors: (angle fp32 [n], sums double [6]) for two normal maps pred, gt fp32 [n, 3] and an optional
    uint8 / bool mask [n], all contiguous on one device.  angle: the angle between the two normals in degrees,
    atan2(|p x g|, p . g) of the normalised vectors, NaN where the mask is 0 or a normal has a zero or non-finite
    length; sums = (valid pixels, sum angle, sum angle^2, count < 11.25, count < 22.5, count < 30 degrees)."""
    _need_cloud("normal_errors", pred, "pred")
    _need_cloud("normal_errors", gt, "gt")
    n, dev = pred.shape[0], pred.device
    if gt.shape[0] != n or gt.device != dev:
        raise RuntimeError(f"normal_errors: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} on one device")
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
        if not mask.is_cuda or mask.dtype != torch.uint8 or tuple(mask.shape) != (n,) or not mask.is_contiguous() or \
                mask.device != dev:
            raise RuntimeError(f"normal_errors: mask must be a contiguous bool or uint8 [{n}] tensor on the maps' device")
    angle = torch.empty(n, dtype=torch.float32, device=dev)
    sums = torch.empty(6, dtype=torch.float64, device=dev)
    lib = _lib.load()
    ws = _workspace(lib.cn_normal_errors_workspace_bytes(n), dev)
    _lib.call("cn_normal_errors", n, _ptr(pred) if n else None, _ptr(gt) if n else None,
              _ptr(mask) if n and mask is not None else None, _ptr(angle) if n else None, _ptr(sums), _ptr(ws), ws.numel(),
              _stream())
    return angle, sums
