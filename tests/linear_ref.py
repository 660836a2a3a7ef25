"""cn_linear's contract (include/copenerf.h) restated in plain float64 torch, with an elementwise tolerance.

linear_ref takes the operands a launch takes (as tensors; the weight as the [>= N, >= K] matrix the B image was
built from) and returns {"out0", "split", "out1", "head"} in float64 and a dictionary of the same keys holding
the largest |kernel - reference| each element may show.  MUL's split columns hold the raw product: the rank-1
term is not added to them (include/copenerf.h).  The tolerances are derived, none is measured:

* the GEMM term v: the project's bar for these operand scales, 1e-5 + 1e-5 |v| (test_gpu_kernels.py,
  test_gpu_bf16.py); every epilogue passes it on with a Lipschitz constant <= 1 (times sigma, times 1 / odiv);
* softplus: 2^-21 / beta + 2^-21 |a| -- one rounding each of beta z log2(e), 1 + e, the v_log result and the
  ln2 / beta product (a 1-ulp hardware transcendental: one bit over the 2^-22 of a correctly rounded one);
* sigma = 1 - exp(-aux_beta aux0): 2^-21 absolute (v_exp result, argument product, the subtraction), times |v|
  where sigma scales v;
* BWD_SOFTPLUS's second-order term aux1 aux2 aux2_scale (1 - sigma) / sigma: the kernel divides by its own
  sigma (off by <= 2^-21); with aux1 = sigma w1 and aux2 = sigma w2 the term's error is aux2_scale |w1 w2|
  2^-21 to first order, and two further bits cover sigma < 2^-20 where the term itself is below aux2_scale
  2^-20: aux2_scale 2^-19 |w1 w2|, with |w1 w2| = |aux1 aux2| / sigma^2 recovered from the operands;
* SOFTPLUS_HEAD's out1 = colv sigma(a): the sigma bar times |colv|; its head, an fp32 row-dot of N terms and
  the bias in a fixed order: (N + 1) roundings of at most 2^-24 of the sum of the terms' magnitudes."""
import torch

STORE, SOFTPLUS, RELU, MUL, TANGENT, BWD_SOFTPLUS, BWD_RELU, SOFTPLUS_HEAD = 0, 1, 2, 3, 4, 5, 6, 8
V_RTOL = V_ATOL = 1e-5
EPS_SP = 2.0 ** -21
EPS_SG = 2.0 ** -21
EPS_T2 = 2.0 ** -19


def sigma(aux0, aux_beta):
    """softplus' recovered from a stored activation, as test_gpu_kernels._sg."""
    return -torch.expm1(-aux_beta * aux0.double())


def softplus(z, beta, threshold):
    """torch.nn.Softplus(beta, threshold) in the precision of z."""
    return torch.where(z * beta > threshold, z, torch.log1p(torch.exp(torch.clamp(z * beta, max=threshold))) / beta)


def linear_ref(A, W, N, K, epilogue, *, M=None, A2=None, K1=None, bias=None, rowv=None, colv=None, aux0=None,
               aux1=None, aux2=None, nsplit=None, nzero=None, adiv=1.0, odiv=1.0, beta=100.0, threshold=20.0,
               aux_beta=0.0, aux2_scale=0.0, head_w=None, head_b=None, head_act=None, bf16=False):
    """(values, tolerances) of one cn_linear call.  bf16: the CN_MFMA_BF16 mode -- A (and A2) rounded to bf16
    (RNE) here, W the bf16 weights; aux images are read as given.  head_act: the activation SOFTPLUS_HEAD's
    out1 and head are computed from (the kernel's own out0, as the kernel does; default: the reference's)."""
    M = A.shape[0] if M is None else M
    K1 = K if (K1 is None or A2 is None) else K1
    nzero = max(N, N if nzero is None else nzero)
    nsplit = N if nsplit is None else nsplit
    f64 = lambda t: None if t is None else t.double()  # noqa: E731
    a = A[:M, :K1]
    if A2 is not None:
        a = torch.cat([a, A2[:M, :K - K1]], 1)
    if bf16:
        a = a.bfloat16()
    raw = a.double() @ W[:N, :K].double().t() / float(adiv)
    v = raw
    if rowv is not None:
        v = raw + f64(rowv)[:M, None] * f64(colv)[None, :N]
    tv = V_ATOL + V_RTOL * v.abs()
    b = 0.0 if bias is None else f64(bias)[None, :N]
    vals, tols = {}, {}
    if epilogue in (MUL, TANGENT, BWD_SOFTPLUS):
        sg = sigma(aux0[:M, :N], aux_beta)
    if epilogue == STORE:
        o, t = v + b, tv
    elif epilogue in (SOFTPLUS, SOFTPLUS_HEAD):
        act = softplus(v + b, float(beta), float(threshold))
        o = act / float(odiv)
        t = (tv + EPS_SP / beta + EPS_SP * act.abs()) / float(odiv)
    elif epilogue == RELU:
        o, t = torch.clamp(v + b, min=0.0), tv
    elif epilogue == MUL:
        o, t = v * sg, tv * sg + EPS_SG * v.abs()
    elif epilogue == TANGENT:
        o, t = v * sg / float(odiv), (tv * sg + EPS_SG * v.abs()) / float(odiv)
    elif epilogue == BWD_SOFTPLUS:
        o, t = v * sg, tv * sg + EPS_SG * v.abs()
        if aux1 is not None:
            p = f64(aux1)[:M, :N] * f64(aux2)[:M, :N]
            live = sg > 0
            safe = torch.where(live, sg, torch.ones_like(sg))
            term = torch.where(live, p * float(aux2_scale) * (1 - sg) / safe, torch.zeros_like(sg))
            w1w2 = torch.where(live, p.abs() / (safe * safe), torch.zeros_like(sg))
            o, t = o + term, t + float(aux2_scale) * EPS_T2 * w1w2
    elif epilogue == BWD_RELU:
        gate = f64(aux0)[:M, :N] > 0
        o, t = torch.where(gate, v, torch.zeros_like(v)), torch.where(gate, tv, torch.zeros_like(tv))
    else:
        raise ValueError(f"epilogue {epilogue}")
    out0 = torch.zeros(M, nzero, dtype=torch.float64, device=v.device)
    tol0 = torch.zeros_like(out0)
    nmain = min(N, nsplit) if epilogue == MUL else N
    out0[:, :nmain], tol0[:, :nmain] = o[:, :nmain], t[:, :nmain]
    vals["out0"], tols["out0"] = out0, tol0
    if epilogue == MUL and nsplit < N:
        # the raw product: no rank-1 term on the split columns
        vals["split"], tols["split"] = raw[:, nsplit:], V_ATOL + V_RTOL * raw[:, nsplit:].abs()
    if epilogue == SOFTPLUS_HEAD:
        act = out0[:, :N] if head_act is None else head_act[:M, :N].double()
        if colv is not None and aux_beta > 0:
            o1 = torch.zeros_like(out0)
            t1 = torch.zeros_like(out0)
            cv = f64(colv)[None, :N]
            o1[:, :N] = cv * sigma(act, aux_beta)
            t1[:, :N] = cv.abs() * EPS_SG
            vals["out1"], tols["out1"] = o1, t1
        hw = f64(head_w)[:N]
        vals["head"] = act @ hw + f64(head_b)[0]
        # an fp32 row-dot of N terms and the bias: (N + 1) roundings of at most 2^-24 of the sum of magnitudes
        tols["head"] = (N + 1) * 2.0 ** -24 * (act.abs() @ hw.abs() + f64(head_b)[0].abs())
        if head_act is None:
            tols["head"] = tols["head"] + tol0[:, :N] @ hw.abs()
    return vals, tols
