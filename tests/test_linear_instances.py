"""Without a device: the float64 restatement of cn_linear's contract (linear_ref.py) against torch autograd, and
the coverage of the per-instance case table (linear_cases.py) -- every linear_kernel<...> instance name of
test_linear_tiles' grid is the resolved name of a table case that cn_linear accepts (M = 0: linear_plan runs, then
the call returns before any launch), or stands in linear_cases.EXCLUDED and is rejected for every grid case that
resolves to it; the weight-gradient table resolves to every kernel cn_wgrad_kernel_name can return."""
import ctypes
import functools

import torch

import linear_cases as LC
import linear_ref as LR
import test_linear_tiles as LT


def test_reference_matches_autograd():
    """h = softplus_100(x W^T + b) / c in float64, sdf = h . w2, G = d sdf / dx with create_graph, and the loss
    L = sum(G R) + sum(h D): fed the quantities include/copenerf.h names, the reference's MUL gives the
    gradient pass's adjoint s = (w2 / c) sigma, STORE on it G, TANGENT the stored tangent u' = sigma z' / c2 (the
    derivative of h along R), and BWD_SOFTPLUS dL/dz = (D / c) sigma + beta s (1 - sigma) z' with
    aux2_scale = beta c2 -- autograd's values to 1e-12."""
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1  # noqa: E731
    M, K, N, beta, c = 37, 5, 12, 100.0, 2.0 ** 0.5
    x = (rnd(M, K) * 0.3).requires_grad_()
    W, b, w2 = rnd(N, K) * 0.05, rnd(N) * 0.02, rnd(N)
    R, D = rnd(M, K), rnd(M, N)
    z = x @ W.t() + b
    h = torch.nn.functional.softplus(z, beta=beta) / c
    G, = torch.autograd.grad((h @ w2).sum(), x, create_graph=True)
    dz, = torch.autograd.grad((G * R).sum() + (h * D).sum(), z, retain_graph=True)
    u_auto = torch.autograd.functional.jvp(lambda t: torch.nn.functional.softplus(t @ W.t() + b, beta=beta) / c,
                                           x.detach(), R)[1]
    hd, ab = h.detach(), beta * c
    close = functools.partial(torch.testing.assert_close, rtol=1e-12, atol=1e-12)
    # the adjoint of the pre-activation in the gradient pass: v = 1 (x) w2 / c through a K = 1 product
    s = LR.linear_ref(torch.ones(M, 1, dtype=torch.float64), w2[:, None], N, 1, LR.MUL, aux0=hd, aux_beta=ab,
                      adiv=c)[0]["out0"]
    close(s, (w2 / c) * torch.sigmoid(beta * z.detach()))
    close(LR.linear_ref(s, W.t().contiguous(), K, N, LR.STORE)[0]["out0"], G.detach())
    u = LR.linear_ref(R, W, N, K, LR.TANGENT, aux0=hd, aux_beta=ab, odiv=c)[0]["out0"]
    close(u, u_auto)
    got = LR.linear_ref(D, torch.eye(N, dtype=torch.float64), N, N, LR.BWD_SOFTPLUS, adiv=c, aux0=hd, aux_beta=ab,
                        aux1=s, aux2=u, aux2_scale=beta * c)[0]["out0"]
    close(got, dz)
    # the forward epilogue itself, and the first-order adjoint alone
    close(LR.linear_ref(x.detach(), W, N, K, LR.SOFTPLUS, bias=b, odiv=c)[0]["out0"], hd)
    first, = torch.autograd.grad((h * D).sum(), z)
    close(LR.linear_ref(D, torch.eye(N, dtype=torch.float64), N, N, LR.BWD_SOFTPLUS, adiv=c, aux0=hd,
                        aux_beta=ab)[0]["out0"], first)


def test_reference_layout_and_edges():
    """Columns [N, nzero) are zero, MUL's split columns go out raw to a buffer of N - nsplit columns, the head is
    the row-dot of the activation, BWD_RELU's gate is > 0 (both zeros closed), and the second-order term is 0
    where sigma is 0."""
    g = torch.Generator().manual_seed(1)
    A = torch.rand(7, 8, generator=g, dtype=torch.float64)
    W = torch.rand(12, 8, generator=g, dtype=torch.float64)
    v = A @ W.t()
    act = torch.rand(7, 12, generator=g, dtype=torch.float64)
    o, _ = LR.linear_ref(A, W, 12, 8, LR.MUL, aux0=act, aux_beta=3.0, nsplit=8, nzero=16)
    assert o["out0"].shape == (7, 16) and torch.all(o["out0"][:, 8:] == 0)
    assert torch.equal(o["split"], v[:, 8:])
    torch.testing.assert_close(o["out0"][:, :8], (v * (1 - torch.exp(-3.0 * act)))[:, :8], rtol=1e-14, atol=0)
    gate = act.clone()
    gate[0, 0], gate[0, 1], gate[0, 2] = 0.0, -0.0, -1.0
    o, t = LR.linear_ref(A, W, 12, 8, LR.BWD_RELU, aux0=gate)
    assert torch.all(o["out0"][0, :3] == 0) and torch.all(t["out0"][0, :3] == 0) and o["out0"][0, 3] == v[0, 3]
    z0 = torch.zeros_like(act)
    o, _ = LR.linear_ref(A, W, 12, 8, LR.BWD_SOFTPLUS, aux0=z0, aux_beta=3.0, aux1=act, aux2=act, aux2_scale=5.0)
    assert torch.all(o["out0"] == 0)
    hw, hb, cv = torch.rand(12, generator=g, dtype=torch.float64), torch.tensor([0.25], dtype=torch.float64), W[:, 0]
    o, _ = LR.linear_ref(A, W, 12, 8, LR.SOFTPLUS_HEAD, colv=cv, aux_beta=100.0, head_w=hw, head_b=hb)
    a = torch.nn.functional.softplus(v, beta=100.0)
    torch.testing.assert_close(o["out0"], a, rtol=1e-14, atol=0)
    torch.testing.assert_close(o["head"], a @ hw + 0.25, rtol=1e-14, atol=0)
    torch.testing.assert_close(o["out1"], cv * torch.where(v > 0.2, torch.ones_like(v), torch.sigmoid(100 * v)),
                               rtol=1e-9, atol=1e-12)


@functools.lru_cache(maxsize=1)
def _grid():
    """name -> the grid cases resolving to it (at any M of the grid)."""
    names = {}
    for case in LT.cases():
        for r in set(x for x in LT.outcome(case) if isinstance(x, str)):
            names.setdefault(r, []).append(case)
    return names


@functools.lru_cache(maxsize=1)
def _table_names():
    """name -> the table cases that resolve to it and that cn_linear accepts."""
    got = {}
    for c in LC.table():
        if LC.accepted(LC.desc(c, 0)):
            got.setdefault(LC.resolved_name(LC.desc(c, c.Ms[0])), []).append(c)
    return got


def test_every_table_case_is_accepted_and_launches_the_named_instance():
    from copenerf import _lib
    bad = []
    for c in LC.table():
        if not LC.accepted(LC.desc(c, 0)):
            bad.append((c, _lib.load().cn_last_error().decode()))
            continue
        for M in c.Ms:
            r = LC.resolved_name(LC.desc(c, M))
            if r != LC.kernel_name(c):
                bad.append((c, M, r))
    assert not bad, f"{len(bad)} table cases rejected or on another instance, the first: {bad[:3]}"


def test_every_grid_instance_has_an_accepted_case_or_a_proven_exclusion():
    grid, table = _grid(), _table_names()
    assert len(grid) == 256
    missing = sorted(n for n in grid if n not in table and LC.excluded_reason(n) is None)
    assert not missing, f"{len(missing)} instances without a table case or an exclusion: {missing}"
    both = sorted(n for n in grid if n in table and LC.excluded_reason(n) is not None)
    assert not both, f"excluded although a table case launches it: {both}"
    # every rule of the exclusion list names an instance of the grid
    for rule, why in LC.EXCLUDED:
        assert any(LC.excluded_reason(n) == why for n in grid), rule


def _grid_desc(case, name):
    """The most permissive descriptor of a grid case: every operand its epilogue and flags ask for, legal leading
    dimensions and B rows (where that keeps the instance), the grid's own flags."""
    f = dict(zip(LT.FIELDS, case))
    e, split = f["epilogue"], f["split"]
    key = {0: "store", 1: "softplus", 2: "relu", 3: "mul_split" if split & 1 else "mul", 4: "tangent",
           5: "bwd_softplus" if (f["aux12_bf16"] or not f["aux0_bf16"]) else "bwd_softplus1", 6: "bwd_relu",
           8: "head"}[e]
    mode = ("fp32", "bf16", "x6")[f["mfma_dtype"]]
    N, K = f["N"], f["K"]
    bn = 64 if f["tile"] == 1 else 128
    for ldb in ((max(f["ldb"], -(-N // bn) * bn), f["ldb"]) if mode == "x6" else (K + 8,)):
        c = LC.Case(None, mode, f["tile"], key, f["rowv"], (f["a_bf16"], 0), N, K, K, ldb, N,
                    N - LC.SPLIT if split & 2 else N, N + 8, ())
        d = LC.desc(c, 0)
        d.aux0_bf16, d.aux12_bf16 = f["aux0_bf16"], f["aux12_bf16"]
        if f["aux0_bf16"] and not d.aux0:
            d.aux0, d.ld_aux0 = LC.FAKE, N + 8
        d.M = 1
        if LC.resolved_name(d) == name:
            d.M = 0
            return d
    return None


def test_excluded_instances_are_rejected_for_every_grid_case():
    """The exclusion list cannot hide something launchable: each excluded name's grid cases, given every operand
    they could ask for, are all rejected -- by the CN_REQUIRE the list names wherever no earlier check of the
    shape (a K the mode does not take, say) refuses the case first, and by it at least once per name."""
    from copenerf import _lib
    lib = _lib.load()
    n = 0
    for name, cases in _grid().items():
        why = LC.excluded_reason(name)
        if why is None:
            continue
        want = why[why.rindex("rejected: ") + len("rejected: "):]
        named = 0
        for case in cases:
            d = _grid_desc(case, name)
            assert d is not None, (name, case)
            rc = lib.cn_linear(d, None)
            assert rc < 0, (name, case, rc)
            named += lib.cn_last_error().decode().startswith(want)
            n += 1
        assert named > 0, (name, want)
    assert n > 0


def test_unreachable_head_on_the_tall_tile():
    """SOFTPLUS_HEAD never reaches the one-per-CU 128x256 bf16x6 tile: over every N the head accepts, with every
    K, tile and B-image height of the grid, the library picks another tile."""
    c0 = next(c for c in LC.table() if c.tmpl == LC.X6_SQ and c.epi == "head")
    for N in range(4, 257, 4):
        for K in LT.KS:
            for tile in range(5):
                for ldb in (128, 256, 384):
                    d = LC.desc(c0._replace(N=N, K=K, K1=K, tile=tile, ldb=ldb, nzero=N, nsplit=N, ld=N + 8), 1)
                    r = LC.resolved_name(d)
                    assert isinstance(r, int) or LC.X6_TALL not in r, (N, K, tile, ldb, r)


def test_wgrad_table_resolves_to_every_kernel():
    from copenerf import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    got = set()
    for c in LC.WGRAD:
        for M in (0, 1, 1025):
            for pairs in (1, 2):
                assert lib.cn_wgrad_kernel_name(LC.wgrad_desc(c, M, pairs), buf, 256) > 0
                name = buf.value.decode()
                assert name.startswith("void cn::" + c.kernel + "("), (c, M, pairs, name)
                got.add(name)
    assert len(got) == LC.WGRAD_KERNELS == len(LC.WGRAD)
