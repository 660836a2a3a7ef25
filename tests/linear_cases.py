"""The case table of the per-instance cn_linear tests: every linear_kernel<...> instance the library can launch,
at the smallest shapes at which its mechanisms can fail, and a builder from a case to an _lib.LinearDesc.

A case is reached at small M: the tiles the library picks only at large M are forced through cn_linear_desc.tile
(3 the two-per-CU 128x256 tile, 4 the 256x256 tile, 2 the 128x128 tile, 1 the 128x64 tile) -- the kernel is the
same.  test_linear_instances.py checks without a device that the table covers every instance name of
test_linear_tiles' grid (or that the name is in EXCLUDED and the library rejects it);
test_gpu_linear_instances.py launches every case.

MUL's split output together with a rank-1 term is in the table on every tile that takes a rank-1 term: the
split columns take the raw product (include/copenerf.h).  Not in the table: SOFTPLUS_HEAD on the 256x256 tiles
below K = 128 (no network has such a layer).

EPIS maps the table's epilogue keys to cn_epilogue codes: mul_split is MUL with the split output
(nsplit = N - 52), bwd_softplus1 is BWD_SOFTPLUS without aux1 / aux2, head_idx is SOFTPLUS_HEAD scattered."""
import collections
import ctypes

EPIS = {"store": 0, "softplus": 1, "relu": 2, "mul": 3, "mul_split": 3, "tangent": 4, "bwd_softplus": 5,
        "bwd_softplus1": 5, "bwd_relu": 6, "head": 8, "head_idx": 8}
ALL = tuple(EPIS)
AUX = ("mul", "mul_split", "tangent", "bwd_softplus", "bwd_softplus1", "bwd_relu")  # the aux0-reading epilogues
MODES = {"fp32": 0, "bf16": 1, "x6": 2}
SMALL_M = (1, 127, 128, 129)
SPLIT = 52  # columns of MUL's split output (the skip layer's embedding columns)

# mode: fp32 / bf16 / x6; tile: cn_linear_desc.tile; images: (a_bf16, aux_bf16) of the bf16 mode (aux_bf16: every
# aux operand the epilogue reads is a bf16 image); ldb: rows of the bf16x6 term image, else B's leading dimension;
# ld: row length of the aux and output buffers (elements; the strided launches add to it); Ms: the rows launched;
# tmpl: the tile's template arguments in the kernel name
Case = collections.namedtuple("Case", "tmpl mode tile epi rowv images N K K1 ldb nzero nsplit ld Ms")

# tile templates: (WM, WN, TM, TN, BK, OCC, DEPTH) as the kernel name prints them, and the rows of a tile
F_T0_D2, F_T0_D1 = "2, 2, 2, 2, 32, 2, 2", "2, 2, 2, 2, 32, 2, 1"
F_T1_D2, F_T1_D1 = "4, 1, 1, 2, 32, 2, 2", "4, 1, 1, 2, 32, 2, 1"
BF_SQ, BF_T0, BF_T1 = "4, 2, 2, 4, 32, 1, 2", "2, 2, 2, 2, 64, 2, 1", "4, 1, 1, 2, 64, 2, 1"
X6_SQ, X6_TALL2, X6_TALL = "4, 2, 2, 4, 16, 1, 2", "2, 2, 2, 4, 16, 2, 2", "4, 2, 1, 4, 32, 1, 2"
X6_WIDE, X6_T128, X6_T1 = "4, 2, 2, 2, 32, 1, 2", "2, 2, 2, 2, 16, 2, 2", "4, 1, 1, 2, 16, 2, 2"
TILE_ROWS = {F_T0_D2: 128, F_T0_D1: 128, F_T1_D2: 128, F_T1_D1: 128, BF_SQ: 256, BF_T0: 128, BF_T1: 128,
             X6_SQ: 256, X6_TALL2: 128, X6_TALL: 128, X6_WIDE: 256, X6_T128: 128, X6_T1: 128}
# workgroups per CU of the persistent grid (OCC)
TILE_OCC = {t: int(t.split(", ")[5]) for t in TILE_ROWS}

# (N, nzero) at the tile's edges
G64 = ((52, 64), (64, 64))
G128 = ((128, 128), (132, 256), (204, 256), (256, 256), (320, 320))
GSPAN = G128[1:4]  # one tile spans every column: 128 < N <= 256
HEAD128 = ((128, 128),)
HEAD64 = ((64, 64),)


def _rows(tmpl, mode, tile, K, images, sets):
    """The cases of one tile template: sets = ((epilogues, rowv, geometries), ...).  Every instance at every
    geometry with the smallest K, over every M; once more with a virtual concat (K1 = 256 and one more chunk)."""
    out = []
    step = 64 if mode == "bf16" or tmpl in (X6_TALL, X6_WIDE, F_T0_D2, F_T1_D2) else 32
    multi = 1537 if TILE_ROWS[tmpl] == 256 else 641
    for epis, rowv, geoms in sets:
        for epi in epis:
            for i, (N, nzero) in enumerate(geoms):
                nsplit = N - SPLIT if epi == "mul_split" else N
                ldb = -(-N // (64 if tile == 1 else 128)) * (64 if tile == 1 else 128)
                if mode == "x6":
                    ldb = max(ldb, 256 if N > 128 else ldb)
                ld = nzero + 8
                mk = lambda k, k1, ms: Case(tmpl, mode, tile, epi, rowv, images, N, k, k1,  # noqa: E731
                                            ldb if mode == "x6" else k + 8, nzero, nsplit, ld, ms)
                out.append(mk(K, K, SMALL_M + (multi,)))
                if i == len(geoms) - 1:
                    out.append(mk(256 + step, 256, (129, multi)))
    return out


def _family(tmpl_t0, tmpl_t1, mode, t0, K, images=(0, 0)):
    """The 128x128 and 128x64 tiles of a mode: every epilogue, with and without the rank-1 term."""
    norowv = tuple(e for e in ALL if not e.startswith("head"))
    rowv_ok = norowv
    heads = ("head", "head_idx")
    return (_rows(tmpl_t0, mode, t0, K, images, ((norowv, 0, G128), (heads, 0, HEAD128), (rowv_ok, 1, G128[1:3]))) +
            _rows(tmpl_t1, mode, 1, K, images, ((norowv, 0, G64), (heads, 0, HEAD64), (rowv_ok, 1, G64[:1]))))


def _aux_family(tmpl_t0, tmpl_t1, t0, K, images):
    """bf16 aux images: the aux-reading epilogues only, no rank-1 term."""
    return _rows(tmpl_t0, "bf16", t0, K, images, ((AUX, 0, G128),)) + _rows(tmpl_t1, "bf16", 1, K, images, ((AUX, 0, G64),))


def table():
    t = []
    # exact-fp32 MFMA: the depth-2 prefetch at K % 64 == 0, depth 1 otherwise
    t += _family(F_T0_D2, F_T1_D2, "fp32", 0, 64)
    t += _family(F_T0_D1, F_T1_D1, "fp32", 0, 32)
    t += _rows(F_T0_D1, "fp32", 0, 96, (0, 0), ((("store", "softplus", "bwd_softplus"), 0, G128[2:3]),))
    # bf16 MFMA: fp32 / image A (mode bits 1 / 5), fp32 / image aux (+ 8); tile 2 keeps the 128x128 tile
    for a_b in (0, 1):
        t += _family(BF_T0, BF_T1, "bf16", 2, 64, (a_b, 0))
        t += _aux_family(BF_T0, BF_T1, 2, 64, (a_b, 1))
        t += _rows(BF_SQ, "bf16", 0, 128, (a_b, 0), ((ALL, 0, GSPAN),))
        t += _rows(BF_SQ, "bf16", 0, 128, (a_b, 1), ((AUX, 0, GSPAN),))
    # bf16x6
    t += _family(X6_T128, X6_T1, "x6", 2, 32)
    t += _rows(X6_SQ, "x6", 4, 128, (0, 0), ((ALL, 0, GSPAN),))
    t += _rows(X6_TALL2, "x6", 3, 128, (0, 0), ((ALL, 0, GSPAN),))
    # the one-per-CU 128x256 tile: MUL / TANGENT where one tile does not span the row (N > 256) or with rowv
    t += _rows(X6_TALL, "x6", 0, 128, (0, 0), ((("mul", "mul_split", "tangent"), 0, G128[4:]),
                                                  (("mul", "mul_split", "tangent"), 1, G128[1:])))
    # the 256x128 tile: the light epilogues where the 256-wide tiles do not apply
    light = ("store", "softplus", "relu")
    t += _rows(X6_WIDE, "x6", 0, 128, (0, 0), ((light, 0, (G128[0], G128[4])),
                                                  (("mul", "mul_split", "tangent"), 0, ((64, 128), (128, 128))),
                                                  (light, 1, G128), (("mul", "mul_split", "tangent"), 1, G128[:1])))
    return t


def mode_bits(c):
    return 1 + 4 * c.images[0] + 8 * c.images[1] if c.mode == "bf16" else MODES[c.mode]


def kernel_name(c):
    """The instance the table says a case launches."""
    return "void cn::linear_kernel<%s, %d, %s, %d>(cn::LinearArgs)" % (
        c.tmpl, EPIS[c.epi], "true" if c.rowv else "false", mode_bits(c))


FAKE = 1 << 20  # a 16-byte aligned non-null pointer value that is never dereferenced (M = 0, name queries)


def desc(c, M, ptr=None, flags=0):
    """The descriptor of a case with M rows.  ptr: name -> address (default: FAKE for every operand the case
    uses); leading dimensions are the case's."""
    from copenerf import _lib
    p = (lambda name: FAKE) if ptr is None else ptr
    e = EPIS[c.epi]
    d = _lib.LinearDesc()
    d.M, d.N, d.K, d.K1 = M, c.N, c.K, c.K1
    d.mfma_dtype, d.tile, d.epilogue, d.flags = MODES[c.mode], c.tile, e, flags
    d.nzero, d.nsplit, d.ldb = c.nzero, c.nsplit, c.ldb
    d.A, d.B, d.out0 = p("A"), p("B"), p("out0")
    d.lda, d.ld_out0 = c.K1 + 8, c.ld
    if c.K1 < c.K:
        d.A2, d.lda2 = p("A2"), c.K - c.K1 + 8
    d.beta, d.threshold, d.adiv, d.odiv = 100.0, 20.0, 2.0 ** 0.5, 1.0
    if e in (0, 1, 2, 8):
        d.bias = p("bias")
    if e in (1, 4):
        d.odiv = 2.0 ** 0.5
    if c.rowv:
        d.rowv, d.colv = p("rowv"), p("colv")
    if e in (3, 4, 5, 6):
        d.aux0, d.ld_aux0, d.aux_beta = p("aux0"), c.ld, 100.0 * 2.0 ** 0.5
    if c.epi == "bwd_softplus":
        d.aux1, d.aux2, d.ld_aux1, d.ld_aux2, d.aux2_scale = p("aux1"), p("aux2"), c.ld, c.ld, 100.0 * 2.0 ** 0.5
    if c.epi == "mul_split":
        d.out_split, d.ld_split = p("split"), 64
    if e == 8:
        d.out1, d.ld_out1, d.colv, d.aux_beta = p("out1"), c.ld, p("colv"), 100.0
        d.head_w, d.head_b, d.head_out = p("head_w"), p("head_b"), p("head_out")
        if c.epi == "head_idx":
            d.head_idx = p("head_idx")
    if c.mode == "bf16":
        d.a_bf16 = c.images[0]
        d.aux0_bf16 = int(bool(c.images[1] and d.aux0))
        d.aux12_bf16 = int(bool(c.images[1] and d.aux1))
        d.out0_b, d.ld_out0_b = p("out0_b"), c.ld
        if e == 8:
            d.out1_b, d.ld_out1_b = p("out1_b"), c.ld
    return d


def resolved_name(d):
    """cn_linear_kernel_name's answer for a descriptor, or its negative status."""
    from copenerf import _lib
    buf = ctypes.create_string_buffer(256)
    n = _lib.load().cn_linear_kernel_name(d, buf, 256)
    return buf.value.decode() if n >= 0 else n


def accepted(d):
    """Whether cn_linear takes the descriptor: with M = 0 it validates (linear_plan) and returns before any
    launch or device access."""
    from copenerf import _lib
    assert d.M == 0
    return _lib.load().cn_linear(d, None) == 0


# Instance names of the grid that no descriptor can launch: (tile templates, epilogue codes, rowv, mode bits)
# -> why.  "rejected": the CN_REQUIRE of linear_plan that refuses every descriptor resolving to the name.
ANY_TMPL = None
EXCLUDED = (
    ((ANY_TMPL, (8,), "true", ANY_TMPL),
     "rejected: cn_linear: SOFTPLUS_HEAD needs head_w (16B aligned), head_b, head_out and no rowv"),
    ((ANY_TMPL, (0, 1, 2, 8), "false", (9, 13)),
     "rejected: cn_linear: a bf16 aux0 is for MUL / TANGENT / BWD_SOFTPLUS / BWD_RELU"),
    (((X6_TALL,), (8,), "false", (2,)),
     "compiled but unreachable: SOFTPLUS_HEAD needs N <= 256, where the 256x256 tile is chosen first; the name "
     "appears at N = 320 only, which is rejected: cn_linear: SOFTPLUS_HEAD needs N <= 256"),
)


def excluded_reason(name):
    """The EXCLUDED reason of an instance name, or None."""
    inner = name[name.index("<") + 1:name.index(">")].split(", ")
    tmpl, e, rowv, mode = ", ".join(inner[:7]), int(inner[7]), inner[8], int(inner[9])
    for (tmpls, epis, rv, modes), why in EXCLUDED:
        if (tmpls is None or tmpl in tmpls) and e in epis and rv == rowv and (modes is None or mode in modes):
            return why
    return None


# ----------------------------------------------------------------------------- cn_wgrad
# One case per split-M kernel cn_wgrad_kernel_name can return: kernel, mode, N, K, the operand rows' lengths
# (256-padded rows select the 256x256 stage ring, or the narrow ring at K <= 64) and (y_bf16, x_bf16).
WCase = collections.namedtuple("WCase", "kernel mode N K ldy ldx images")
WGRAD = (
    WCase("wgrad_kernel<2, 2, 2, 2>", "fp32", 132, 128, 256, 128, (0, 0)),
    WCase("wgrad_kernel<2, 2, 2, 1>", "fp32", 52, 192, 128, 192, (0, 0)),
    WCase("wgrad_x6r_kernel<2>", "bf16x6", 204, 256, 256, 256, (0, 0)),
    WCase("wgrad_x6n_kernel<3>", "bf16x6", 204, 64, 256, 64, (0, 0)),
    WCase("wgrad_x6_kernel<2, 2>", "bf16x6", 132, 128, 256, 128, (0, 0)),
    WCase("wgrad_x6_kernel<2, 1>", "bf16x6", 52, 192, 128, 192, (0, 0)),
    WCase("wgrad_bf16_kernel<2, 2, 2, 2>", "bf16", 132, 128, 256, 128, (0, 0)),
    WCase("wgrad_bf16_kernel<2, 2, 2, 1>", "bf16", 52, 192, 128, 192, (0, 0)),
    WCase("wgrad_b16r_kernel<2>", "bf16", 204, 256, 256, 256, (0, 0)),
    WCase("wgrad_b16d_kernel<4>", "bf16", 204, 256, 256, 256, (1, 1)),
)
WGRAD_MODES = {"fp32": 0, "bf16": 1, "bf16x6": 2}
WGRAD_KERNELS = 10  # the names cn_wgrad_kernel_name can return


def wgrad_desc(c, M, npairs=1):
    """The descriptor of a weight-gradient case with fake operand pointers (name queries only)."""
    from copenerf import _lib
    d = _lib.WgradDesc()
    d.Y0 = d.X0 = d.dW = d.workspace = FAKE
    if npairs == 2:
        d.Y1 = d.X1 = FAKE
    d.ldy0 = d.ldy1 = c.ldy
    d.ldx0 = d.ldx1 = c.ldx
    d.M, d.N, d.K, d.npairs = M, c.N, c.K, npairs
    d.n_out, d.k_out, d.ld_dw = c.N, c.K, c.K
    d.mfma_dtype = WGRAD_MODES[c.mode]
    d.y_bf16, d.x_bf16 = c.images
    return d
