"""Float64 restatement of LPIPS (VGG16 features, the v0.1 linear heads), written from its description (torch
on the CPU): what cn_lpips is specified to compute (include/copenerf.h, ABI v20).

  1. z-score per channel;  2. thirteen 3 x 3 convolutions (zero padding 1, bias, ReLU) in five blocks with a
  2 x 2 stride-2 floor max-pool between the blocks, tapped after each block;  3. every tap divided by its
  channel norm + 1e-10;  4. per block the mean over the pixels of sum_c lin[c] (fx^ - fy^)^2.

A fixture made by the reference's own code is not possible: its networks.py builds the feature stack from
torchvision, which is not installed where this suite runs, and the trained weights are never fetched.  The
weights here are random (make_weights), in the two real key layouts (state_dicts)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

WIDTHS = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
POOL_BEFORE = (2, 4, 7, 10)          # convolutions that read the pooled map
TAP_AFTER = (1, 3, 6, 9, 12)         # relu1_2, 2_2, 3_3, 4_3, 5_3
TAP_CHANNELS = (64, 128, 256, 512, 512)
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # torchvision's features.N of each convolution
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)


def make_weights(seed, widths=WIDTHS, dtype=torch.float32):
    """Seeded random weights: He-normal convolutions (std sqrt(2 / (9 Cin))), biases 0.05 N(0, 1), lin
    weights U[0, 1).  Returns (convs [(w [Cout, Cin, 3, 3], b [Cout])], lins [[C]])."""
    g = torch.Generator().manual_seed(seed)
    convs, cin = [], 3
    for cout in widths:
        w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * math.sqrt(2.0 / (9 * cin))
        b = 0.05 * torch.randn(cout, generator=g, dtype=torch.float64)
        convs.append((w.to(dtype), b.to(dtype)))
        cin = cout
    lins = [torch.rand(widths[t], generator=g, dtype=torch.float64).to(dtype) for t in TAP_AFTER]
    return convs, lins


def state_dicts(convs, lins):
    """The two files' key layouts: torchvision's VGG16 (features.N.weight / bias) and LPIPS v0.1's vgg.pth
    (linN.model.1.weight, [1, C, 1, 1])."""
    vgg = {}
    for i, (w, b) in zip(FEATURE_INDEX, convs):
        vgg[f"features.{i}.weight"], vgg[f"features.{i}.bias"] = w.clone(), b.clone()
    lin = {f"lin{t}.model.1.weight": v.reshape(1, -1, 1, 1).clone() for t, v in enumerate(lins)}
    return vgg, lin


def features(x, convs, dtype=torch.float64, ceil_mode=False, operand=None):
    """The five taps of [N, 3, H, W] images.  operand: a rounding applied to both operands of every
    convolution (the bf16 measurement of the GPU test), else none."""
    rnd = operand or (lambda t: t)
    x = x.to(dtype)
    x = (x - torch.tensor(MEAN, dtype=dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    taps = []
    for l, (w, b) in enumerate(convs):
        if l in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2, ceil_mode=ceil_mode)
        x = F.relu(F.conv2d(rnd(x), rnd(w.to(dtype)), b.to(dtype), padding=1))
        if l in TAP_AFTER:
            taps.append(x)
    return taps


def head(fx, fy, lin):
    """One block's term for taps [N, C, h, w]: [N]."""
    nx = fx / (fx.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    ny = fy / (fy.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((nx - ny).pow(2) * lin.to(fx.dtype).view(1, -1, 1, 1)).sum(1).mean((1, 2))


def lpips_layers(x, y, convs, lins, dtype=torch.float64, **kw):
    """[N, 5]: the five terms of each pair of [N, 3, H, W] (or [3, H, W]) images."""
    if x.dim() == 3:
        x, y = x[None], y[None]
    fx, fy = features(x, convs, dtype, **kw), features(y, convs, dtype, **kw)
    return torch.stack([head(a, b, l) for a, b, l in zip(fx, fy, lins)], 1)


def lpips(x, y, convs, lins, dtype=torch.float64):
    return lpips_layers(x, y, convs, lins, dtype).sum(1)


def patches(src, y0, rows, kpad):
    """The operand rows of output rows [y0, y0 + rows) of NHWC maps [n, H, W, C] by gathers:
    [n rows W, kpad], column (dy 3 + dx) C + c."""
    n, H, W, C = src.shape
    pad = torch.zeros(n, H + 2, W + 2, C, dtype=src.dtype)
    pad[:, 1:H + 1, 1:W + 1] = src
    ys = torch.arange(y0, y0 + rows)
    xs = torch.arange(W)
    out = torch.zeros(n, rows, W, kpad, dtype=src.dtype)
    for dy in range(3):
        for dx in range(3):
            t = dy * 3 + dx
            out[..., t * C:(t + 1) * C] = pad[:, (ys + dy)[:, None], (xs + dx)[None, :]]
    return out.reshape(n * rows * W, kpad)


def pair_inputs(shape, seed=1):
    """a ~ U[0, 1), b = clip(a + 0.1 N(0, 1), 0, 1), fp32."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(*shape, generator=g)
    b = (a + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
    return a, b
