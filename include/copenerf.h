/* copenerf.h — C ABI of libcopenerf.so, the MI355X (gfx950) kernels behind the
 * cope-nerf NeuS volumetric-rendering hot path.
 *
 * The reference (HoangChuongNguyen/cope-nerf) is pure PyTorch: it has no FFI.
 * Each entry point below replaces one group of aten calls on the hot path and
 * cites the reference lines it restates (paths relative to the reference root).
 * The host side that binds these symbols is cope-nerf_amd/copenerf/_lib.py
 * (ctypes); INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - All pointers are device pointers (fp32 unless typed otherwise), row-major,
 *    with explicit leading dimensions in ELEMENTS.  The caller owns all memory.
 *  - `stream` is a hipStream_t (passed as void* so that this header needs no HIP
 *    headers).  Nothing here allocates, synchronises, or uses the null stream:
 *    any sequence of calls is hipGraph-capturable and re-entrant across devices
 *    (torch.nn.DataParallel runs one host thread per GPU, train.py:54).
 *  - Return 0 on success, a negative cn_status on a bad argument or a failed
 *    launch; cn_last_error() holds the message (thread-local).  Asynchronous
 *    device faults surface at the caller's next synchronisation.
 */
#ifndef COPENERF_H_
#define COPENERF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CN_ABI_VERSION 22

typedef void* cn_stream_t; /* hipStream_t */

typedef enum cn_status {
    CN_OK = 0,
    CN_ERR_ARG = -1,         /* null pointer / bad enum */
    CN_ERR_SHAPE = -2,       /* inconsistent sizes or leading dimensions */
    CN_ERR_ALIGN = -3,       /* pointer / leading dimension not 16-byte aligned */
    CN_ERR_LAUNCH = -4,      /* hipLaunchKernel failed */
    CN_ERR_UNSUPPORTED = -5  /* configuration outside what the kernels implement */
} cn_status;

int cn_abi_version(void);
const char* cn_last_error(void);

/* ------------------------------------------------------------------------ *
 * Fully-connected layers: out = epilogue((A · Bᵀ) / adiv [+ rowv ⊗ colv])
 * Replaces every nn.Linear of SDFNetwork (model/neus_fields.py:273-283) and
 * RenderingNetwork (model/neus_fields.py:364-370), the first-order backward of
 * those layers (autograd of the same lines), the ∇ₓSDF pass of
 * SDFNetwork.gradient (neus_fields.py:291-303) and its create_graph double
 * backward.  Computed with v_mfma_f32_32x32x2_f32 (exact fp32 products).
 *
 *   A   : [M][>=K] (lda), optionally a virtual concat: columns k < K1 come from
 *         A, columns k >= K1 from A2 (column k-K1).  K, K1 multiples of 32.
 *   B   : [Npad][K] (ldb), Npad = N rounded up to the tile width (128, or 64
 *         when tile == 1); rows >= N must be readable (zero-padded weights).
 *   Columns [0, N) of out0 get the epilogue value, columns [N, nzero) get 0.
 * ------------------------------------------------------------------------ */
/* sg(x) = 1 - exp(-aux_beta * x): softplus'(z) recovered from a stored softplus
 * output x = softplus_beta(z) / c (aux_beta = beta * c), since exp(beta a) = 1 +
 * exp(beta z).  The derivative is never stored (ABI v4): the backward reads the
 * activations it already keeps. */
typedef enum cn_epilogue {
    CN_EPI_STORE = 0,        /* out0 = v + bias                                      */
    CN_EPI_SOFTPLUS = 1,     /* z = v + bias; out0 = softplus_beta(z)/odiv           */
    CN_EPI_RELU = 2,         /* out0 = relu(v + bias)                                */
    CN_EPI_MUL = 3,          /* out0 = v * sg(aux0) (cols < nsplit); out_split = v (cols >= nsplit; the raw
                                product: the split columns take no rank-1 term) */
    CN_EPI_TANGENT = 4,      /* out0 = v * sg(aux0) / odiv                           */
    CN_EPI_BWD_SOFTPLUS = 5, /* out0 = v*sg(aux0) + aux1*aux2*aux2_scale*(1-sg)/sg (0 where sg = 0;
                                aux1, aux2 both NULL or both set): with aux1 = s (the ∇-pass
                                adjoint), aux2 = u' = sg*z'/c2 and aux2_scale = beta*c2 this is
                                softplus' double-backward term beta*s*(1-sg)*z'  */
    CN_EPI_BWD_RELU = 6,     /* out0 = aux0 > 0 ? v : 0                              */
    CN_EPI_SOFTPLUS_HEAD = 8 /* the last SDF hidden layer with the sdf head fused (ABI v5):
                                a = softplus_beta(v + bias) (odiv 1); out0 = a (or NULL: not
                                stored); out1 = colv * sg(a) (or NULL: the ∇-pass seed
                                s = w80 ⊙ softplus', aux_beta > 0); head_out[head_idx ?
                                head_idx[m] : m] = Σ_n a[m][n] head_w[n] + head_b[0]
                                (neus_fields.py:279-283, the sdf column of lin8); needs the
                                whole row in one tile: N <= 256 (bf16x6) or N <= 128 */
} cn_epilogue;

typedef struct cn_linear_desc {
    const void* A;       /* fp32, or bf16 when a_bf16 (A2 likewise) */
    const void* A2;
    const float* B;
    const float* bias;   /* [N] or NULL (N <= 512 with a bias or colv) */
    const float* rowv;   /* [M] or NULL : rank-1 term rowv[m]*colv[n] added to v */
    const float* colv;   /* [N] or NULL */
    const void* aux0;    /* fp32, or bf16 when aux0_bf16 */
    const float* aux1;
    float* out0;
    float* out1;         /* SOFTPLUS_HEAD only (else NULL) */
    float* out_split;
    int64_t lda, lda2, ldb, ld_aux0, ld_aux1, ld_out0, ld_out1, ld_split;
    int32_t M, N, K, K1;
    int32_t nzero, nsplit;
    int32_t epilogue;    /* cn_epilogue */
    int32_t tile;        /* 0: the library's tile choice (up to 256x256), 1: 128x64, 2: 128x128 only
                            (tests compare the tiles: every tile gives the same bits); bf16x6 only
                            (ABI v22): 3 the two-per-CU 128x256 tile, 4 the one-per-CU 256x256 tile,
                            both for 128 < N <= 256, no rowv, ldb >= 256 (else CN_ERR_UNSUPPORTED);
                            above 4: CN_ERR_ARG */
    float adiv, odiv;    /* divisors applied to A·Bᵀ and to the activation (0 means 1),
                            applied as multiplies by their fp32 reciprocals */
    float beta, threshold; /* Softplus(beta, threshold) of neus_fields.py:266 */
    int32_t mfma_dtype;  /* CN_MFMA_F32: A, B fp32, exact fp32 products (v_mfma_f32_32x32x2_f32);
                            CN_MFMA_BF16: A fp32 rounded to bf16 (RNE) on load, B bf16 [N][ldb]
                            (ldb in bf16 elements), fp32 accumulate (v_mfma_f32_32x32x16_bf16);
                            K and K1 multiples of 64 (config C3's bf16 MLP MFMA);
                            CN_MFMA_F32_BF16X6: fp32 GEMM on the bf16 MFMA: A fp32 split on load
                            into three bf16 terms, B pre-split and chunk-major: bf16
                            [K/16][ldb][3][16], term t of element (n, k) at
                            B + ((k/16) ldb + n) 48 + 16 t + k%16, ldb = image rows >= the N
                            tiles; six term products accumulated in fp32 (error at the level
                            of fp32 accumulation; K, K1 multiples of 32) */
    float aux_beta;      /* sg() scale of MUL / TANGENT / BWD_SOFTPLUS (> 0 for those) */
    const float* aux2;   /* BWD_SOFTPLUS second-order input u' (or NULL) */
    int64_t ld_aux2;
    float aux2_scale;
    int32_t flags;       /* bit 0: visit the M-tiles last to first (a chain's consecutive launches
                            alternate it so a layer first reads the rows its producer wrote last,
                            still in the memory-side cache); results do not depend on it */
    const float* head_w;       /* SOFTPLUS_HEAD: [N] row-dot weights, head_b: [1] */
    const float* head_b;
    float* head_out;           /* [M] (or indexed by head_idx) */
    const int32_t* head_idx;   /* [M] destination rows or NULL */
    /* ABI v10 -- bf16 operand images (CN_MFMA_BF16 only, config C3's bf16 MLP MFMA): a GEMM operand
       is rounded to bf16 (RNE) when it is staged, so a tensor whose consumers are GEMM operands can be
       stored as that rounded image (2 bytes instead of 4) with bitwise-identical results.
       a_bf16: A and A2 are bf16 row-major (lda / lda2 in bf16 elements, multiples of 8).
       aux0_bf16: aux0 is bf16 -- BWD_RELU's sign source (bf16 RNE keeps the sign, and a positive
       value rounds to 0 only below 2^-133), or the activation MUL / TANGENT / BWD_SOFTPLUS recover
       softplus' σ from (config C3 stores the SDF's hidden activations as bf16 images only; σ from
       the bf16 activation is within the mode's bf16 operand rounding).
       aux12_bf16: BWD_SOFTPLUS's aux1 and aux2 (the second-order term's s and u') are bf16 (config
       C3 stores the ∇-pass adjoints and the tangents, read only by GEMMs and by this term, in bf16).
       BWD_SOFTPLUS with aux1 / aux2 takes all three aux operands in one format: aux0_bf16 ==
       aux12_bf16.
       out0_b (ld_out0_b): the bf16 image of every value written to out0 (columns [0, nzero),
       including the zero fill); out0 itself may then be NULL.  out1_b: the same for SOFTPLUS_HEAD's
       out1 (colv and aux_beta set; out1 may then be NULL).  Leading dimensions in bf16 elements, multiples of 8; 16-byte aligned. */
    int32_t a_bf16;
    int32_t aux0_bf16;
    int32_t aux12_bf16;
    void* out0_b;
    int64_t ld_out0_b;
    void* out1_b;
    int64_t ld_out1_b;
} cn_linear_desc;

enum cn_mfma_dtype { CN_MFMA_F32 = 0, CN_MFMA_BF16 = 1, CN_MFMA_F32_BF16X6 = 2 };

int cn_linear(const cn_linear_desc* d, cn_stream_t stream);

/* The rocprofv3 symbol of the kernel cn_linear would launch for *d (no launch, no device
 * access; the tile choice is the launch's own function): NUL-terminated into buf[len].
 * Returns the name's length, or a negative cn_status.  For profilers and the bench's
 * roofline (bench.py names the launch class it reports). */
int cn_linear_kernel_name(const cn_linear_desc* d, char* buf, int32_t len);

/* ------------------------------------------------------------------------ *
 * Weight images for cn_linear (the per-call `pack` of the effective weights,
 * neus_fields.py:273-283 / 364-373 weight_norm outputs): one launch builds
 * every padded / transposed / column-permuted B image of a network.  Job j
 * writes the region [r0, r1) x [c0, c1) of its image: the source matrix
 * S (rows x cols; S[r][c] = src[r*src_ld + c], or src[c*src_ld + r] when
 * transpose) lands at (r0, c0), the rest of the region is zero.  format is a
 * cn_mfma_dtype: CN_MFMA_F32 copies fp32 (element (r, c) at dst[r*dst_ld + c]),
 * CN_MFMA_BF16 rounds to bf16 (RNE, same indexing), CN_MFMA_F32_BF16X6 writes
 * the three bf16 terms of each value into cn_linear's chunk-major image (term t
 * at dst[((c/16)*dst_ld + r)*48 + 16t + c%16]; dst_ld = the image's rows).
 * ------------------------------------------------------------------------ */
typedef struct cn_pack_job {
    const float* src;
    void* dst;
    int64_t src_ld, dst_ld;
    int32_t rows, cols;
    int32_t r0, r1, c0, c1;
    int32_t transpose;
    int32_t format;
} cn_pack_job;

int cn_pack_weights(const cn_pack_job* jobs, int32_t njobs, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Weight normalisation of every Linear of a network in one launch
 * (torch.nn.utils.weight_norm, dim 0, as the reference wraps every layer:
 * model/neus_fields.py:84-140, 336-360): per output row i,
 *   forward   W_i = v_i (g_i / |v_i|)
 *   backward  dg_i = (dW_i . v_i) / |v_i|,  dv_i = (g_i / |v_i|) (dW_i - v_i dg_i / |v_i|)
 * v, w, dw, dv row-major contiguous [rows][cols]; g, dg [rows].  One wavefront per
 * row (fixed-order reductions).
 * ------------------------------------------------------------------------ */
typedef struct cn_wn_job {
    const float* v;
    const float* g;
    float* w;            /* forward output */
    const float* dw;     /* backward input */
    float* dv;           /* backward outputs */
    float* dg;
    int32_t rows, cols;
} cn_wn_job;

int cn_weight_norm(const cn_wn_job* jobs, int32_t njobs, int32_t backward, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Weight gradient: dW[n][k] = sum_m ( Y0[m][n]*X0[m][k] + Y1[m][n]*X1[m][k] ),
 * db[n] = sum_m Y0[m][n].  Reduction over the M = R*S sample rows is split
 * over workgroups into fp32 slabs (workspace) and summed in a fixed order, so
 * the result is bitwise reproducible.  Replaces the dW/db of the autograd of
 * every Linear above, including the create_graph term of neus_fields.py:296.
 * ------------------------------------------------------------------------ */
typedef struct cn_wgrad_desc {
    const void* Y0;      /* fp32, or bf16 when y_bf16 (Y1 likewise) */
    const void* X0;      /* fp32, or bf16 when x_bf16 (X1 likewise) */
    const void* Y1;      /* NULL when npairs == 1 */
    const void* X1;
    float* workspace;    /* cn_wgrad_workspace_bytes() */
    float* dW;           /* [n_out][k_out] (ld_dw) */
    float* db;           /* [n_out] or NULL */
    int64_t ldy0, ldx0, ldy1, ldx1, ld_dw;
    int64_t workspace_bytes;
    int32_t M, N, K;     /* N, K: valid columns of Y and X (Y/X readable up to the padded tile) */
    int32_t npairs;
    int32_t n_out, k_out;
    int32_t accumulate;  /* 1: dW += result (db too), 0: dW = result; M = 0 is an empty sum: dW = db = 0,
                            or both unchanged when accumulating */
    int32_t mfma_dtype;  /* CN_MFMA_F32, or CN_MFMA_BF16: Y and X rounded to bf16 (RNE) on load,
                            v_mfma_f32_32x32x16_bf16, fp32 accumulation and slab reduction;
                            db is summed from the fp32 values either way;
                            CN_MFMA_F32_BF16X6: fp32 gradient from three bf16 terms per operand
                            (six products) */
    /* ABI v10 (CN_MFMA_BF16 only): the Y side (Y0, Y1) / the X side (X0, X1) are bf16 operand images
       (see cn_linear_desc.a_bf16; leading dimensions in bf16 elements, multiples of 8): the products
       are the same bits as from the fp32 tensors they round; db then sums the bf16 values of Y0. */
    int32_t y_bf16;
    int32_t x_bf16;
} cn_wgrad_desc;

size_t cn_wgrad_workspace_bytes(int32_t M, int32_t N, int32_t K);
int cn_wgrad(const cn_wgrad_desc* d, cn_stream_t stream);
/* As cn_linear_kernel_name for cn_wgrad's split-M kernel (cn::slab_reduce_kernel follows it). */
int cn_wgrad_kernel_name(const cn_wgrad_desc* d, char* buf, int32_t len);
/* Several independent weight gradients (ABI v9).  The descriptors that cn_wgrad would run on a
 * 256x256 stage-ring kernel (bf16x6, or bf16 since ABI v10) share ONE launch of it (each takes a share of the workgroups
 * proportional to its rows x pairs x output tiles, its own M-slices and slabs in its own
 * workspace) and ONE cn::slab_reduce_kernel launch; any other descriptor is run as by cn_wgrad.
 * Results equal cn_wgrad's up to the slice count (fixed-order sums: bitwise reproducible).
 * Replaces the per-layer dW of neus_fields.py:291-303 (SDF) and 364-373 (colour) as one call. */
int cn_wgrad_batch(const cn_wgrad_desc* descs, int32_t n, cn_stream_t stream);
/* ABI v10: the workspace a cn_wgrad_batch call over descs[0..n) needs (n <= 64), and each
 * descriptor's byte offset into one buffer of that size (offsets may be NULL): a batched job takes
 * only its share of the slabs, so this is less than the sum of cn_wgrad_workspace_bytes.  The
 * layout follows the CU count of the current device: query and launch on the same device. */
size_t cn_wgrad_batch_workspace_bytes(const cn_wgrad_desc* descs, int32_t n, int64_t* offsets);

/* ------------------------------------------------------------------------ *
 * Per-row heads (neus_fields.py:279-283 last Linear row 0 = sdf;
 * neus_fields.py:367-373 last colour Linear + sigmoid):
 *   out[dst(m)][c] = act( sum_k A[m][k]*W[c][k] + b[c] ),  c < C (C <= 4)
 * act: 0 none, 1 sigmoid.  dst(m) = dst_index ? dst_index[m] : m.
 * ------------------------------------------------------------------------ */
int cn_row_head(int32_t M, int32_t K, const float* A, int64_t lda, const float* W, int64_t ldw,
                const float* b, int32_t C, int32_t act, float* out, int64_t ld_out,
                const int32_t* dst_index, cn_stream_t stream);

/* out[k] (+)= (sum_m (w ? w[m] : 1) * X[m][k]) / wdiv, k < K: the sdf row of the
 * last SDF Linear's weight gradient (neus_fields.py:283, row 0 of lin8) and its
 * create_graph term; fixed-order slab reduction. */
size_t cn_colsum_workspace_bytes(int32_t M, int32_t K);
int cn_colsum(int32_t M, int32_t K, const float* w, const float* X, int64_t ldx, float wdiv, float* out,
              int32_t accumulate, float* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* out[m][n] = f(X[m][n]) * w[n] (* rowv[m] when rowv != NULL) for n < N: the seed of the
 * ∇ₓSDF pass (neus_fields.py:295-302), and the sdf-only adjoint of the last hidden layer
 * (d sdf / d z_7 = dsdf[m] w80[n] softplus'(z_7), no feature gradient: no GEMM needed);
 * f(x) = x when act_beta == 0, else softplus' from the softplus output, 1 - exp(-act_beta x). */
int cn_scale_cols(int32_t M, int32_t N, const float* X, int64_t ldx, const float* w, const float* rowv,
                  float* out, int64_t ld_out, float act_beta, cn_stream_t stream);

/* Adjoint of a softplus layer from the gradient of its output, without a GEMM (the
 * SDF's last hidden layer when the feature head is folded into the colour network's
 * first layer: the colour backward already yields d/d(hidden)):
 *   out[m][n] = ((D ? D[m][n] : 0) + (rowv ? rowv[m] colv[n] : 0)) * sg
 *             + (aux1 ? aux1[m][n] aux2[m][n] aux2_scale (1 - sg) / sg : 0),   0 where sg = 0,
 *   sg = 1 - exp(-act_beta act[m][n]) (softplus' from the activation, as cn_linear's epilogues). */
/* With cs_out != NULL it also produces the sdf row of lin8's weight gradient from the
 * operands it already streams (the fused form of cn_colsum's calls):
 *   cs_out[n] = (sum_m (rowv ? rowv[m] act[m][n] : 0) + (aux2 ? aux2[m][n] : 0)) / cs_div,
 *   rs_out[0] = (sum_m rowv[m]) / cs_div (the sdf head's bias gradient; rs_out may be NULL),
 * fixed-order slab reductions through workspace (cn_softplus_adjoint_workspace_bytes). */
size_t cn_softplus_adjoint_workspace_bytes(int32_t M, int32_t N);
/* out_bf16 (ABI v10): out is written as its bf16 operand image (RNE; ld_out in bf16 elements, % 4 == 0).
 * in_bf16 (ABI v10): bit 0: D, bit 1: act, bit 2: aux1 and aux2 are bf16 operand images (config C3's
 * bf16 mode; leading dimensions in bf16 elements, % 4 == 0, 8-byte aligned). */
int cn_softplus_adjoint(int32_t M, int32_t N, const void* D, int64_t ldd, const void* act, int64_t lda,
                        float act_beta, const float* rowv, const float* colv, const void* aux1, int64_t ld1,
                        const void* aux2, int64_t ld2, float aux2_scale, void* out, int64_t ld_out, int32_t out_bf16,
                        int32_t in_bf16, float* cs_out, float* rs_out, float cs_div, float* workspace,
                        int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Positional encoding of the SDF input (neus_embedder.py:6-51 with
 * include_input, log-sampled bands 2^0..2^(multires-1), [sin, cos]; applied at
 * neus_fields.py:269-271 to x*scale):
 *   U0[m][0..4+8*multires) = embed(scale * x[m][0..4)),  zeros up to kpad.
 *   If U4e != NULL also U4e[m][j] = U0[m][j] / u4_scale (the skip-connection
 *   copy of neus_fields.py:276-277).  flags bit 0 (ABI v10): U4e is a bf16
 *   operand image (RNE; ld_u4 in bf16 elements, 8-byte aligned); bit 1 (ABI
 *   v11): U0 is one too (the operand of cn_sdf_mlp; 8-byte aligned).
 * ------------------------------------------------------------------------ */
int cn_sdf_embed(int32_t M, const float* x, int64_t ldx, int32_t multires, float scale, int32_t kpad,
                 void* U0, int64_t ld_u0, void* U4e, int64_t ld_u4, float u4_scale, int32_t flags,
                 cn_stream_t stream);

/* ∇ₓSDF from the embedding adjoint: G[m][i] = scale * J_embed(x)ᵀ (Q0[m] + QE[m])
 * (neus_fields.py:291-303; the chain rule through neus_embedder.py:20-22). */
int cn_sdf_grad_assemble(int32_t M, int32_t multires, float scale, const float* U0, int64_t ld_u0,
                         const float* Q0, int64_t ld_q0, const float* QE, int64_t ld_qe,
                         float* G, int64_t ld_g, cn_stream_t stream);

/* Tangent of the embedding along v = dL/d(∇ₓSDF) (forward-over-reverse form
 * of the double backward of neus_fields.py:296):
 *   T0[m] = scale * J_embed(x) v[m] (zeros up to kpad);  T4e[m] = T0[m] / t4_scale
 *   (t4_bf16, ABI v10: T4e a bf16 operand image, as cn_sdf_embed's U4e). */
int cn_sdf_tangent_prep(int32_t M, int32_t multires, float scale, int32_t kpad, const float* U0,
                        int64_t ld_u0, const float* v, int64_t ld_v, float* T0, int64_t ld_t0,
                        void* T4e, int64_t ld_t4, float t4_scale, int32_t t4_bf16, cn_stream_t stream);

/* Colour-network input extras (neus_fields.py:346-356, mode 'idr'):
 *   ext[m] = [ G[m][0..4), pts[m][0..4), embed_view(dirs[m / dir_div]) (3+6*multires_view), 0... ]
 * The 256 feature columns are read in place by cn_linear through A/A2. */
int cn_color_extras(int32_t M, const float* G, int64_t ld_g, const float* pts, int64_t ld_p,
                    const float* dirs, int64_t ld_d, int32_t dir_div, int32_t multires_view,
                    int32_t kpad, float* ext, int64_t ld_ext, cn_stream_t stream);

/* Ray-direction gradient through the view encoding of cn_color_extras (the
 * autograd of neus_embedder.py:17-36 on dirs, neus_renderer.py:345, 354):
 * with d_ext [M][>=8+3+6L] the gradient of ext, rows r*dir_div .. r*dir_div +
 * dir_div-1 sharing dirs[r],
 *   ddirs[r][c] (+)= sum_rows d_ext[.][8+c]
 *                  + sum_k 2^k (cos(2^k d_c) d_ext[.][11+6k+c] - sin(2^k d_c) d_ext[.][14+6k+c]). */
int cn_color_extras_bwd(int32_t R, int32_t dir_div, const float* d_ext, int64_t ld_ext, const float* dirs,
                        int64_t ld_d, int32_t multires_view, float* ddirs, int32_t accumulate,
                        cn_stream_t stream);

/* Backward of the colour head (sigmoid(Linear 256->3), neus_fields.py:367-373):
 *   dz3 = drgb*rgb*(1-rgb);  dZ2[m][k] = (H3[m][k] > 0) * sum_c dz3[m][c]*W3[c][k];
 *   dW3 = sum_m dz3ᵀ H3, db3 = sum_m dz3 (fixed-order slab reduction). */
size_t cn_rgb_head_bwd_workspace_bytes(int32_t M, int32_t K);
int cn_rgb_head_bwd(int32_t M, int32_t K, const float* drgb, const float* rgb, const float* H3,
                    int64_t ld_h, const float* W3, void* dZ2, int64_t ld_dz, int32_t dz_bf16, float* dW3,
                    float* db3, float* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Patch sampling (model/training.py:413-436 on the device): idx[p*ps*ps + a*ps + b] =
 * (row_p + a) * w + col_p + b for n_patches distinct corners (row_p, col_p) of the
 * (h-ps+1) x (w-ps+1) grid -- the first n_patches values of a keyed pseudo-random
 * permutation of the corner ids (4-round Feistel network with cycle walking; key:
 * 4 int32 on the device, e.g. from torch.randint), the device counterpart of
 * randperm(n)[:n_patches] without a sort.
 * ------------------------------------------------------------------------ */
int cn_patch_indices(int32_t h, int32_t w, int32_t ps, int32_t n_patches, const int32_t* key, int64_t* idx,
                     cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Stage-1 relative poses (neus_fields.py:142-161, every interval at once): for
 * interval k < K with its n time steps, A_s = EulerXYZ(omega_s dt_k) (pytorch3d
 * convention, Rx Ry Rz), V_s = vel_s dt_k, T <- A_s T + V_s, Q <- Q A_s from
 * Q = I, T = 0; P[k] = [Q T; 0 0 0 1] (row-major 4x4).  omega / vel rows
 * k*n + s with leading dimensions ld_o / ld_v (floats).  The backward maps dP
 * [K][4][4] to domega, dvel ([K*n][3] contiguous) by the reverse recurrence.
 * One thread per interval (n <= 64).
 * ------------------------------------------------------------------------ */
int cn_euler_chain(int32_t K, int32_t n, const float* omega, int64_t ld_o, const float* vel, int64_t ld_v,
                   const float* dt, float* P, cn_stream_t stream);
int cn_euler_chain_bwd(int32_t K, int32_t n, const float* omega, int64_t ld_o, const float* vel, int64_t ld_v,
                       const float* dt, const float* dP, float* domega, float* dvel, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Sampling along rays (neus_renderer.py:453-525).
 * ------------------------------------------------------------------------ */
/* Uniform jitter from a counter-based generator (ABI v14; the §8(b) device Philox seed): out[i] =
 * (word i % 4 of Philox4x32-10(counter = (i / 4 as 64 bits, offset), key = seed)) >> 8, x 2^-24, in [0, 1).
 * seed_offset: DEVICE uint64 [2] = (seed, offset), read by the kernel, so a captured launch replays with
 * the current values (the caller advances offset by ceil(n / 4) per draw to keep streams disjoint). */
int cn_uniform_philox(int64_t n, const uint64_t* seed_offset, float* out, cn_stream_t stream);

/* z[r][i] = near*(1-lin_i) + far*lin_i, lin = linspace(0,1,n); stratified
 * jitter with t_rand [R][n] when t_rand != NULL (neus_renderer.py:466-483). */
int cn_coarse_z(int32_t R, int32_t n, const float* near, const float* far, const float* t_rand,
                float* z, cn_stream_t stream);

/* pts_time[r*n+i] = [o_r + d_r * zz_i, t]: zz = z (mid == 0) or the section
 * midpoints z + dists/2 with the last dist = (far[0]-near[0])/n_coarse
 * (neus_renderer.py:337-350, 495-498, 286-291). */
int cn_points(int32_t R, int32_t n, const float* rays_o, const float* rays_d, const float* z,
              const float* t, int32_t mid, const float* near, const float* far, int32_t n_coarse,
              float* pts_time, cn_stream_t stream);

/* Backward of cn_points for ray / pose gradients (the autograd of
 * neus_renderer.py:343-350, pts = rays_o + rays_d * mid_z): with dP [R*n][>=3]
 * (row stride ld_p) the upstream gradient of pts_time,
 *   drays_o[r] = sum_i dP[r*n+i][0..3),  drays_d[r] = sum_i dP[r*n+i][0..3) * zz_i
 * (zz as in cn_points).  One wavefront per ray, fixed-order double sums. */
int cn_points_bwd(int32_t R, int32_t n, const float* z, int32_t mid, const float* near, const float* far,
                  int32_t n_coarse, const float* dP, int64_t ld_p, float* drays_o, float* drays_d,
                  cn_stream_t stream);

/* One NeuS up-sampling round + merge (neus_renderer.py:178-224 up_sample,
 * 39-70 sample_pdf det=True, 282-298 cat_z_vals).  One wavefront per ray.
 *   z_out = sorted merge of z and the n_imp new samples;
 *   z_new = the new samples [R][n_imp];
 *   if sdf_out: sdf_out[r][pos(old i)] = sdf[r][i] and new_dst[r*n_imp+j] =
 *   r*(n+n_imp) + pos(new j) (cn_row_head scatters the new SDF there). */
int cn_up_sample_merge(int32_t R, int32_t n, int32_t n_imp, float inv_s, const float* z,
                       const float* sdf, float* z_out, float* z_new, float* sdf_out, int32_t* new_dst,
                       cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Alpha compositing (neus_renderer.py:337-420, render_core).  One wavefront
 * per ray; transmittance as an exclusive product scan across the wave.
 * G holds ∇ₓSDF rows (normals = G[m][0..3)), sdf/G/rgb are indexed m = r*S+i.
 * inv_s and cos_anneal_ratio are device scalars (training.py:120-124 ramps the
 * ratio every iteration: a replayed hipGraph reads the current value). 
 * ------------------------------------------------------------------------ */
int cn_composite_fwd(int32_t R, int32_t S, const float* z, const float* sdf, const float* G,
                     int64_t ld_g, const float* rgb, const float* rays_d, const float* inv_s,
                     const float* near, const float* far, int32_t n_coarse, const float* cos_anneal_ratio,
                     float* color, float* depth, float* weights, float* cdf, cn_stream_t stream);

/* Backward of cn_composite_fwd.  drays_d (nullable, [R][3]) receives the ray
 * direction gradient of true_cos = rays_d . normals (neus_renderer.py:362);
 * the normals are those of the detached-input gradient pass
 * (neus_renderer.py:356), so no second-order term reaches the points. */
int cn_composite_bwd(int32_t R, int32_t S, const float* z, const float* sdf, const float* G,
                     int64_t ld_g, const float* rgb, const float* rays_d, const float* inv_s,
                     const float* near, const float* far, int32_t n_coarse, const float* cos_anneal_ratio,
                     const float* dcolor, const float* ddepth, const float* dweights,
                     const float* dcdf, float* dsdf, float* dG, float* drgb, float* dinv_s_part,
                     float* drays_d, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Training losses in one pass: the loss value and its input gradients
 * (model/training.py:506-509 colour L1, train.py:526 eikonal, model/losses.py:7-38
 * with train.py:519-525 edge-aware and plain depth smoothness on patch x patch
 * ray patches, patch in 1..4; R rays, M samples):
 *   loss = w_rgb sum|color - gt| / R + w_eik mean_m (|n_m| - 1)^2
 *        + w_edge EdgePreservingSmoothness(depth, gt; gamma) + w_smooth Smoothness(depth)
 *   weights: DEVICE [4] = (w_rgb, w_eik, w_edge, w_smooth), read by the kernels, so the
 *   annealed weights of train.py:246-263, 401-405 change without re-capturing a graph;
 *   nonfinite (nullable, device int32): set to 1 when the loss is not finite -- the
 *   NaN assert of model/training.py:532-533 without a host sync;
 *   color, gt [R][3]; depth [R]; normals [M][ld_n] (columns 0..2); loss [1];
 *   dcolor [R][3], ddepth [R], dnormals [M][ld_dn] (columns 0..2) = d loss / d input.
 * Partial sums are reduced in double in a fixed order (bitwise reproducible).
 * ------------------------------------------------------------------------ */
size_t cn_train_loss_workspace_bytes(int32_t R, int32_t patch);
int cn_train_loss(int32_t R, int32_t patch, int64_t M, const float* color, const float* gt, const float* depth,
                  const float* normals, int64_t ld_n, const float* weights, float gamma, float* loss,
                  float* dcolor, float* ddepth, float* dnormals, int64_t ld_dn, int32_t* nonfinite,
                  void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Stage-1 per-sample terms (train.py:467-505), R rays of S samples, M = R*S,
 * in one pass each way (replaces the ~40 torch ops of train.py:468-477, the
 * per-ray sums the flow projection reduces to (train.py:484-495) and the
 * point transform of the SDF-consistency term (train.py:502-504)):
 *   pts [M][ld_p], normals [M][ld_n] (columns 0..2), flows [M] (stride ld_f),
 *   weights [R][S]; mv: DEVICE [6] = (angular_velocity, velocity);
 *   cw2: DEVICE [4][4] (row-major) or null -- camera-of-frame -> world-camera;
 * forward:
 *   sums [2]       = (sum_m |(w x p_m + v) . n_m + f_m| w_m, sum_m w_m)
 *   ray_acc [R][4] = (sum_s w p, sum_s w) per ray (16B aligned)
 *   x_out [M][ld_x] (nullable, needs cw2) = (cw2 (p_m, 1))[0..2], t_world
 * backward (g_num: DEVICE [1] = dL/d sums[0]; the weights are detached there,
 * as in the reference; d_ray [R][4] and dx [M][ld_dx] (columns 0..2) nullable):
 *   dnormals [M][ld_dn], dflows [M] (stride ld_df): written;
 *   dweights [R][S] (nullable) = d_ray . (p, 1);
 *   dpts [M][ld_dp] (nullable): written;
 *   dmv_dcw2 [18] = (dL/d mv [6], dL/d cw2 rows 0..2 [12]).
 * The cross-ray sums are per-workgroup partials reduced in a fixed order
 * (bitwise reproducible); workspace: cn_stage1_workspace_bytes(R).
 * ------------------------------------------------------------------------ */
size_t cn_stage1_workspace_bytes(int32_t R);
int cn_stage1_fwd(int32_t R, int32_t S, const float* pts, int64_t ld_p, const float* normals, int64_t ld_n,
                  const float* flows, int64_t ld_f, const float* weights, const float* mv, const float* cw2,
                  float t_world, float* ray_acc, float* x_out, int64_t ld_x, float* sums, float* workspace,
                  cn_stream_t stream);
int cn_stage1_bwd(int32_t R, int32_t S, const float* pts, int64_t ld_p, const float* normals, int64_t ld_n,
                  const float* flows, int64_t ld_f, const float* weights, const float* mv, const float* cw2,
                  const float* g_num, const float* d_ray, const float* dx, int64_t ld_dx, float* dnormals,
                  int64_t ld_dn, float* dflows, int64_t ld_df, float* dweights, float* dpts, int64_t ld_dp,
                  float* dmv_dcw2, float* workspace, cn_stream_t stream);

/* Running products of n 4x4 matrices (row-major [n][4][4]), ABI v8: C_0 = A_0,
 * C_j = A_j C_{j-1} -- the relative-pose chains of stage 1 (compute_w2c_mappings,
 * model/neus_fields.py:171-183; the world-camera chain of train.py:498-501) -- and the
 * adjoint: dA from dC (every C_j may carry a gradient).  One lane walks the chain. */
int cn_mat4_chain_fwd(int32_t n, const float* A, float* C, cn_stream_t stream);
int cn_mat4_chain_bwd(int32_t n, const float* A, const float* C, const float* dC, float* dA, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * The sampler's SDF query in one launch (ABI v11): SDFNetwork.sdf(x) with no
 * gradient, as NeuSRenderer.up_sample calls it (model/neus_renderer.py:492-525,
 * the coarse samples and each round's new ones; neus_fields.py:268-283) -- eight
 * softplus layers with the skip concat and the sdf row of the last Linear -- for
 * the bf16 MLP MFMA mode (config C3), from the embedding's bf16 images that
 * cn_sdf_embed writes (flags 3).  Activations stay on chip: per sample 128 + 2E
 * bytes are read and the sdf (4 B) written.  Bitwise equal to the
 * layer-by-layer bf16 path (cn_linear on bf16 weight images, SOFTPLUS /
 * SOFTPLUS_HEAD epilogues).
 *   u0      [M][ld_u0] bf16: the embedding, 64 columns (lin0's input; zero past E),
 *           ld_u0 % 8 == 0, 16-byte aligned;
 *   tail    [M][ld_t] bf16: the embedding / skip_div, E = 4 (1 + 2 multires)
 *           columns (the skip concat's tail), ld_t % 4 == 0, 8-byte aligned;
 *   W[l]    bf16 weight images [256][ldw[l]] of lin0 .. lin7, K = 64 (lin0) or 256,
 *           rows past a layer's width zero (as cn_pack_weights builds them);
 *   bias[l] fp32 [width]; the skip layer (feeding the skip concat) has width
 *           256 - E, its output divided by skip_div;
 *   head_w  [256] = lin8.weight[0] / scale, head_b [1] = lin8.bias[0] / scale;
 *   sdf     written at idx[m] (idx NULL: m).
 * Supported: n_layers 8, hidden 256, kpad0 64, multires <= 7; else
 * CN_ERR_UNSUPPORTED (the caller composes cn_linear launches instead).
 * ------------------------------------------------------------------------ */
typedef struct cn_sdf_mlp_desc {
    const void* u0;   /* bf16 */
    const void* tail; /* bf16 */
    int64_t ld_u0, ld_t;
    int32_t M, n_layers, hidden, kpad0, multires, skip_layer;
    const void* W[8]; /* bf16 */
    int64_t ldw[8];
    const float* bias[8];
    const float* head_w;
    const float* head_b;
    float* sdf;
    const int32_t* idx;
    float skip_div, beta, threshold;
    void* debug; /* NULL, or [8][M][256] (bf16; fp32 in the bf16x6 format): every layer's input as the kernel holds it (tests) */
    int32_t format; /* 0: the bf16 mode (u0 / tail bf16 images, W bf16 [256][K]); CN_MFMA_F32_BF16X6 (ABI v15): the
                       fp32-class mode -- u0 / tail fp32, W the chunk-major term images [K/16][256][48] of
                       cn_pack_weights (ldw = 256, their rows), bitwise the layer-by-layer bf16x6 query */
} cn_sdf_mlp_desc;
int cn_sdf_mlp(const cn_sdf_mlp_desc* d, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Composed entry points (ABI v12): the sampler of NeuSRenderer.render
 * (neus_renderer.py:466-525) and the SDF query it makes (SDFNetwork.sdf,
 * neus_fields.py:268-283, 286-287), each one C call over the kernels above --
 * no host code between the launches, all on the caller's stream, scratch from
 * a caller-owned workspace (size from the *_workspace_bytes function; 256-byte
 * aligned; it may be reused as soon as the stream has passed the call).
 * Results are bitwise those of the same kernels composed one by one
 * (copenerf.fields.sdf_forward / copenerf.renderer.sample_z).
 *
 * cn_sdf_net describes SDFNetwork's weights as cn_pack_weights images
 * (copenerf.fields.pack_sdf): for lin0 .. lin(n_lin-2) the forward image
 * W[l] (rows w_rows[l] >= the output width rounded up to 128, columns w_cols[l]:
 * KE = 64-rounded encoding width for lin0, the 32- (bf16: 64-) rounded input
 * width after; CN_MFMA_F32_BF16X6 images are chunk-major [w_cols/16][w_rows][48]),
 * bias[l] fp32 [out_dim[l]] (16-byte aligned); the sdf row of the last Linear
 * as head_w [in_dim[n_lin-1]] = weight[0] / scale (16-byte aligned) and head_b
 * [1] = bias[0] / scale.  skip: the layer whose input is cat([h, embed(x)]) / sqrt 2
 * (SDFNetwork skip_in, one entry) or -1; the layer before it has width
 * out_dim = d_hidden - E.  Inputs are (x, y, z, t) points (d_in = 4), E = 4 (1 + 2 multires).
 * flags bit 0 (CN_SDF_LAYERED): never the fused cn_sdf_mlp query (tests compare the two).
 * ------------------------------------------------------------------------ */
#define CN_SDF_MAX_LIN 16
#define CN_SDF_LAYERED 1
typedef struct cn_sdf_net {
    int32_t n_lin;                      /* Linear layers (SDFNetwork n_layers + 1), 2 .. 16 */
    int32_t in_dim[CN_SDF_MAX_LIN];     /* lin_l.weight.shape[1] */
    int32_t out_dim[CN_SDF_MAX_LIN];    /* lin_l.weight.shape[0] */
    int32_t skip;
    int32_t multires;
    float scale, beta, threshold;       /* SDFNetwork scale, Softplus(beta, threshold) */
    int32_t mfma_dtype;                 /* cn_mfma_dtype of the images */
    int32_t flags;
    const void* W[CN_SDF_MAX_LIN - 1];
    int32_t w_rows[CN_SDF_MAX_LIN - 1];
    int32_t w_cols[CN_SDF_MAX_LIN - 1];
    const float* bias[CN_SDF_MAX_LIN - 1];
    const float* head_w;
    const float* head_b;
    /* ABI v13 (cn_render_fwd's ∇ₓSDF pass only): the transposed images Wt[l] (fields.pack_sdf's Bt:
       rows >= the input width rounded up to 128, columns the output width rounded up to 32 / 64) and
       head_wp [HL] = head_w zero-padded to the hidden buffers' width (16-byte aligned) */
    const void* Wt[CN_SDF_MAX_LIN - 1];
    int32_t wt_rows[CN_SDF_MAX_LIN - 1];
    int32_t wt_cols[CN_SDF_MAX_LIN - 1];
    const float* head_wp;
} cn_sdf_net;

/* sdf[idx ? idx[m] : m] = SDFNetwork.sdf(x[m]) for M points x [M][ldx >= 4] (no gradient):
 * cn_sdf_embed + cn_sdf_mlp (bf16 images, the fused shape) or cn_sdf_embed + one cn_linear per
 * layer (SOFTPLUS, the last with the SOFTPLUS_HEAD epilogue where one tile spans the row) +
 * cn_row_head otherwise. */
size_t cn_sdf_query_workspace_bytes(const cn_sdf_net* net, int32_t M);
int cn_sdf_query(const cn_sdf_net* net, int32_t M, const float* x, int64_t ldx, float* sdf,
                 const int32_t* idx, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* The sampler: z [R][n_samples + up_sample_steps k] (k = n_importance / up_sample_steps >= 1, or
 * [R][n_samples] when n_importance == 0) = the coarse samples (stratified with
 * t_rand [R][n_samples], or none when t_rand is NULL -- eval) and, when n_importance > 0,
 * up_sample_steps rounds of k new samples each, round i with
 * inv_s = 64 * 2^i from the SDF of the current samples (the coarse SDF query, then one query per
 * round's new samples scattered into the merged order; no query after the last round).
 * rays_o / rays_d [R][3], near / far [R], time_step [1] (the frame's time value; points are
 * (o + d z, t)).  The caller picks n_samples / n_importance by the iteration (the
 * importance_sampling_start switch of neus_renderer.py:455-459). */
typedef struct cn_sample_desc {
    int32_t R, n_samples, n_importance, up_sample_steps;
    const float* rays_o;
    const float* rays_d;
    const float* near;
    const float* far;
    const float* t_rand;
    const float* time_step;
    const cn_sdf_net* net;
    float* z;
    /* ABI v14: with t_rand NULL and philox != NULL (DEVICE uint64 [2] = (seed, offset)), the jitter is
       drawn on the device: t_rand = cn_uniform_philox(R n_samples, philox) in the workspace */
    const uint64_t* philox;
} cn_sample_desc;
size_t cn_sample_workspace_bytes(const cn_sample_desc* d);
int cn_sample(const cn_sample_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * The rendering forward in one call (ABI v13): NeuSRenderer.forward of the
 * eval path (neus_renderer.py:453-584 with render_core 307-450, no gradient):
 * the sampler (cn_sample, or the caller's z), the section midpoints, the SDF
 * field with its ∇ₓSDF pass and the feature head folded into the colour
 * network (copenerf.renderer's fold: the colour network's first layer reads
 * the SDF's last hidden activation), the colour network, the compositing.
 * Bitwise equal to copenerf's renderer with the same packs.
 *
 * cn_color_net: RenderingNetwork (mode idr, squeeze_out) as its images
 * (copenerf.fields.pack_color with the folded first layer): W[0] is lin0's
 * image over [feature (F) | gradient | pts | emb(dirs) | 0] (K = F + KX,
 * KX = 64-rounded 4 + 4 + 3 (1 + 2 multires_view)), W[l] the hidden layers';
 * head_w [3][in_dim[n_lin-1]] fp32 and head_b [3] the sigmoid head.
 * ------------------------------------------------------------------------ */
typedef struct cn_color_net {
    int32_t n_lin;                      /* Linear layers, 2 .. 16 */
    int32_t in_dim[CN_SDF_MAX_LIN];
    int32_t out_dim[CN_SDF_MAX_LIN];
    int32_t d_feature, multires_view;
    int32_t mfma_dtype;
    const void* W[CN_SDF_MAX_LIN - 1];
    int32_t w_rows[CN_SDF_MAX_LIN - 1];
    int32_t w_cols[CN_SDF_MAX_LIN - 1];
    const float* bias[CN_SDF_MAX_LIN - 1];
    const float* head_w;
    const float* head_b;
    /* ABI v14 (cn_render_bwd only): the transposed images of the backward (copenerf.fields.pack_color):
       Wt[l] for the hidden layers l >= 1 (rows >= the input width rounded up to 128, columns the output
       width rounded up to 32 / 64); lin0's feature columns transposed Wtf; its gradient columns
       transposed Wg [4][wg_ld] fp32; its extras columns [g | pts | emb(dirs)] transposed Wxt (rows 64). */
    const void* Wt[CN_SDF_MAX_LIN - 1];
    int32_t wt_rows[CN_SDF_MAX_LIN - 1];
    int32_t wt_cols[CN_SDF_MAX_LIN - 1];
    const void* Wtf;
    int32_t wtf_rows, wtf_cols;
    const float* Wg;
    int32_t wg_ld;
    const void* Wxt;
    int32_t wxt_rows, wxt_cols;
} cn_color_net;

/* z_in: [R][S] sample positions (the renderer's z_vals hook), or NULL: cn_sample's
 * (t_rand as there; NULL: eval).  inv_s, cos_anneal_ratio: device scalars [1].
 * Outputs (all required): z [R][S] (S = n_samples + up_sample_steps k, or z_in's S),
 * pts [R S][4] (the midpoints, (x, t)), sdf [R S], grad [R S][4] (∇ₓSDF: normals and the
 * sdf flow), rgb [R S][3], color [R][3], depth [R] (weighted z), weights [R][S], cdf [R][S]. */
typedef struct cn_render_desc {
    int32_t R, n_samples, n_importance, up_sample_steps, S_in;
    const float* rays_o;
    const float* rays_d;
    const float* near;
    const float* far;
    const float* t_rand;
    const float* time_step;
    const float* z_in;
    const float* inv_s;
    const float* cos_anneal_ratio;
    const cn_sdf_net* sdf_net;
    const cn_color_net* color_net;
    float* z;
    float* pts;
    float* sdf;
    float* grad;
    float* rgb;
    float* color;
    float* depth;
    float* weights;
    float* cdf;
    const uint64_t* philox;             /* ABI v14: as cn_sample_desc.philox (the sampler's jitter) */
} cn_render_desc;
size_t cn_render_fwd_workspace_bytes(const cn_render_desc* d);
int cn_render_fwd(const cn_render_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * The rendering step under autograd (ABI v14): render_core of NeuSRenderer.forward
 * (neus_renderer.py:307-450) at given samples, with everything its backward needs kept
 * in the caller's `state` buffer, and the backward in one call.
 * cn_render_train_fwd takes the descriptor of cn_render_fwd with z_in required (the
 * samples: cn_sample's, drawn without gradient as in the reference) and writes pts, sdf,
 * grad, color, depth, weights, cdf (rgb, z unused: the colour values stay in the state);
 * z_in, rays, near / far, time_step, inv_s, cos_anneal_ratio, the networks and those
 * outputs must stay unchanged until cn_render_bwd has run.
 * cn_render_bwd takes the gradients of the outputs (NULL: none) and writes
 *   the SDF network's effective-weight gradients sdf_dW[l] [out][in] / sdf_db[l]
 *     (the last Linear's feature rows zero: the colour network's folded lin0 carries them),
 *   the colour network's col_dW[l] / col_db[l] (lin0 over the folded input in the
 *     reference column order [pts | emb(dirs) | gradient | feature]),
 *   dinv_s [R] (per-ray parts of dL/d inv_s; the caller sums them),
 *   drays_o / drays_d [R][3] (both or neither: the pose gradient through the points,
 *     the view directions and the compositing's cosine).
 * Gradients that reach one buffer from several consumers are summed in the order
 * autograd sums them for copenerf's composition (the sdf / ∇ₓSDF / point outputs' own
 * consumers first, then the compositing's, then the colour network's, then the SDF
 * network's), so the results are bitwise those of the composition
 * (copenerf.renderer with RENDER_NATIVE off).  state: cn_render_state_bytes; workspace:
 * cn_render_bwd_workspace_bytes (pose or not); both 256-byte aligned.
 * ------------------------------------------------------------------------ */
typedef struct cn_render_grads {
    const float* dcolor;                /* [R][3] */
    const float* ddepth;                /* [R] */
    const float* dweights;              /* [R][S] */
    const float* dcdf;                  /* [R][S] */
    const float* dsdf;                  /* [R S] */
    const float* dgrad;                 /* [R S][4] */
    const float* dpts;                  /* [R S][4] */
    float* sdf_dW[CN_SDF_MAX_LIN];
    float* sdf_db[CN_SDF_MAX_LIN];
    float* col_dW[CN_SDF_MAX_LIN];
    float* col_db[CN_SDF_MAX_LIN];
    float* dinv_s;
    float* drays_o;
    float* drays_d;
} cn_render_grads;
size_t cn_render_state_bytes(const cn_render_desc* d);
size_t cn_render_bwd_workspace_bytes(const cn_render_desc* d, int32_t pose);
int cn_render_train_fwd(const cn_render_desc* d, void* state, int64_t state_bytes, cn_stream_t stream);
int cn_render_bwd(const cn_render_desc* d, const cn_render_grads* g, const void* state, int64_t state_bytes,
                  void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * The SDF query under autograd (ABI v14): SDFNetwork.sdf(x) with gradients to the
 * network's parameters and to x -- the stage-1 consistency re-query of
 * train.py:502-505 (neus_fields.py:268-283 and its autograd backward; the §8(b)
 * cn_mlp_fwd / cn_mlp_bwd) -- as two calls.  cn_mlp_fwd writes sdf [M] and keeps the
 * layer activations in the caller's `state` buffer (cn_mlp_state_bytes; unchanged until
 * cn_mlp_bwd has run).  cn_mlp_bwd takes dsdf [M] = dL/dsdf and that state and writes
 *   dW[l] [out_dim[l]][in_dim[l]] (row-major) and db[l] [out_dim[l]], l = 0 .. n_lin-1:
 *     the gradients of the effective weights (weight-norm's backward stays the caller's);
 *     the last Linear's rows past the sdf row (the feature head, unused by sdf()) are zero;
 *   dx [M][4] (16-byte aligned) = dL/dx when dx != NULL;
 *   dW[0] == NULL: dx only, no parameter gradients.
 * The network needs the transposed images (Wt, head_wp; cn_sdf_net ABI v13).  Scratch
 * from workspace (cn_mlp_bwd_workspace_bytes); state and workspace 256-byte aligned.
 * Bitwise equal to copenerf.fields.sdf_forward (keep) and sdf_backward (sdf only, first
 * order) / sdf_input_grad with the same packs.  M = 0: nothing is written.
 * ------------------------------------------------------------------------ */
typedef struct cn_mlp_desc {
    int32_t M;
    const float* x;                     /* [M][4] (x, y, z, t) -- cn_mlp_fwd */
    const cn_sdf_net* net;
    float* sdf;                         /* [M] -- cn_mlp_fwd */
    const float* dsdf;                  /* [M] -- cn_mlp_bwd */
    float* dW[CN_SDF_MAX_LIN];
    float* db[CN_SDF_MAX_LIN];
    float* dx;
} cn_mlp_desc;
size_t cn_mlp_state_bytes(const cn_mlp_desc* d);
size_t cn_mlp_bwd_workspace_bytes(const cn_mlp_desc* d);
int cn_mlp_fwd(const cn_mlp_desc* d, void* state, int64_t state_bytes, cn_stream_t stream);
int cn_mlp_bwd(const cn_mlp_desc* d, const void* state, int64_t state_bytes, void* workspace,
               int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Mesh extraction (ABI v16): NeuSRenderer.extract_geometry (neus_renderer.py:10-37,
 * 588-591) on the device: the grid points of a bounding box at one time value, the SDF
 * volume over them, and the isosurface of a volume as a welded triangle mesh.  The
 * reference's extract_fields queries 3-column points in 64^3 blocks with a host copy
 * each and meshes with PyMCubes; here the points are (x, y, z, t) rows, the volume
 * stays on the device and the mesher is marching tetrahedra on the six-tetrahedron
 * Kuhn split (DESIGN.md "Mesh extraction").
 *
 * cn_grid_points: pts [M][4] (16-byte aligned) = rows (X[ix], Y[iy], Z[iz], t) of the
 * linear indices [m0, m0 + M) of an nx x ny x nz grid in C order (z fastest: the
 * reference's u[xi, yi, zi]).  Each axis is torch.linspace(lo, hi, n) by its fp32 rule:
 * step = (hi - lo) / (n - 1); lo + i step for i < n / 2, hi - (n - 1 - i) step otherwise.
 * lo, hi: HOST float [3] (read during the call); time_step: device scalar [1].
 * ------------------------------------------------------------------------ */
int cn_grid_points(int32_t nx, int32_t ny, int32_t nz, const float* lo, const float* hi,
                   const float* time_step, int64_t m0, int32_t M, float* pts, cn_stream_t stream);

/* u [nx][ny][nz] = +SDFNetwork.sdf at the grid points: cn_grid_points + cn_sdf_query over
 * chunks of chunk_rows rows (0: 2^20) on the caller's stream, bitwise the same for every
 * chunk_rows.  The sign is the network's (negative inside): cn_mesh_* orient triangles by
 * the volume's values, so no negation is needed (the reference meshes -sdf).
 * chunk_rows x 256 bytes must stay below 2^31 (the fused bf16x6 query's row bound):
 * larger is CN_ERR_SHAPE before anything launches.  Workspace (256-byte aligned):
 * cn_sdf_grid_workspace_bytes = chunk x 16 bytes rounded up to 256 (one chunk's points)
 * + cn_sdf_query_workspace_bytes(net, chunk), chunk = min(chunk_rows or 2^20, nx ny nz). */
typedef struct cn_sdf_grid_desc {
    const cn_sdf_net* net;
    int32_t nx, ny, nz;
    float lo[3], hi[3];
    const float* time_step;
    float* u;
    int32_t chunk_rows;
} cn_sdf_grid_desc;
size_t cn_sdf_grid_workspace_bytes(const cn_sdf_grid_desc* d);
int cn_sdf_grid(const cn_sdf_grid_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* The isosurface u = threshold of a volume u [nx][ny][nz] (fp32, device).
 *  - Cells in C order over (nx-1, ny-1, nz-1); tetrahedron k = 0..5 of a cell belongs to the
 *    k-th permutation pi of (x, y, z) in lexicographic order, corners v0 = (0,0,0),
 *    v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = (1,1,1); bit i of its mask is u[vi] < threshold
 *    (strict: a tie is outside).
 *  - Every tetrahedron edge runs from a grid vertex p to p + d, d in {0,1}^3 \ {0}, owned by
 *    p in slot dx + 2 dy + 4 dz - 1.  An edge whose ends differ in the mask bit carries one
 *    mesh vertex; vertex ids ascend by (linear index of p, slot).  Position: p + s d in index
 *    space, s = (threshold - u_p) / (u_{p+d} - u_p), then per axis
 *    pos / (n - 1) * (hi - lo) + lo, all in fp32.
 *  - Triangles: A = the inside corners if at most two, else the outside corners, B the
 *    others, both ascending.  A = {i}: (E_ij, E_ik, E_il); A = {i,j}: (E_ik, E_il, E_jl),
 *    (E_ik, E_jl, E_jk); second and third index swapped where the midpoint triangle's normal
 *    points from the outside corners' centroid toward the inside corners': normals point
 *    toward larger u, out of the surface for an SDF.  Order: (cell, k, triangle).
 * cn_mesh_count writes counts = (V, T) (DEVICE int64 [2]) and leaves the edge masks and the
 * scanned offsets in the workspace; cn_mesh_emit, with the same volume, descriptor and
 * workspace, writes vertices [V][3] and triangles [T][3].  The host cannot see counts
 * without synchronising, so cn_mesh_emit checks max_vertices / max_triangles against them on
 * the device: with a buffer smaller than the counts it writes nothing at all.  Deterministic:
 * no atomics, no waits between workgroups.
 * Workspace (256-byte aligned), every piece rounded up to 256 bytes, N = nx ny nz,
 * C = (nx-1)(ny-1)(nz-1): N (edge masks) + 4 N (vertex offsets) + C (triangle counts) + 4 C
 * (triangle offsets) + 4 ceil(N / 1024) + 4 ceil(C / 1024) (the scans' tile totals).
 * Any dim below 2, 7 N >= 2^31 or 12 C >= 2^31: CN_ERR_SHAPE (workspace_bytes: 0). */
typedef struct cn_mesh_desc {
    int32_t nx, ny, nz;
    const float* u;
    float threshold;
    float lo[3], hi[3];
    float* vertices;            /* [max_vertices][3] -- cn_mesh_emit */
    int64_t max_vertices;
    int32_t* triangles;         /* [max_triangles][3] -- cn_mesh_emit */
    int64_t max_triangles;
    int64_t* counts;            /* device [2]: V, T */
} cn_mesh_desc;
size_t cn_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int cn_mesh_count(const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);
int cn_mesh_emit(const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);
/* cn_mesh_count_observed / cn_mesh_emit_observed (additive to ABI v22): the same mesher over a
 * volume in which NaN means "unobserved" (cn_tsdf_finalize's u) -- the same descriptor, the same
 * workspace layout and size, the same vertex and triangle order.  An owned edge carries a vertex
 * only when both its ends are observed (and differ in the mask bit); a cell emits triangles only
 * when all eight corners are observed.  No vertex coordinate is ever NaN.  A vertex on an edge
 * whose every surrounding cell was skipped is still emitted and no triangle refers to it: drop
 * such vertices with cn_mesh_select / cn_mesh_compact at min_triangles >= 1 (a vertex without a
 * triangle is a component of none).  With no NaN in u the results are bitwise those of
 * cn_mesh_count / cn_mesh_emit. */
int cn_mesh_count_observed(const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);
int cn_mesh_emit_observed(const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Vertex colours (additive to ABI v22): the colour network at surface points, with the
 * view direction set to the inward unit normal of every point (the usual convention of
 * NeuS-family exporters; the reference's extract_geometry stops at the geometry).
 *
 * cn_vertex_dirs: dirs [M][3] = sign * G[m][0:3] / max(|G[m][0:3]|, 1e-12) for rows
 * G [M][ldg >= 3] (the first three columns of ∇ₓSDF), the norm
 * sqrtf((gx gx + gy gy) + gz gz) without FMA contraction; one thread per row.  A zero row
 * gives exact zeros.
 *
 * cn_rgb8_pack: out[i] = floorf(fminf(fmaxf(rgb[i], 0), 1) * 255 + 0.5) as uint8 for n
 * values, NaN -> 0.
 *
 * cn_point_colors: rgb [M][3] = RenderingNetwork(x, t, dir, ∇ₓSDF, feature) at the DEVICE
 * points x [M][3] and the device scalar time_step, dir = -n̂ (cn_vertex_dirs, sign -1) or,
 * with view_dir != NULL (HOST float [3], read during the call, not zero), the row
 * (float)(v / |v|) (the quotient in double, |v| = sqrt((x x + y y) + z z)) on every point.
 * Per chunk of chunk_rows rows (0: 2^18): the rows (x, t), the SDF field with its ∇ₓSDF
 * pass, cn_vertex_dirs (or the fixed row), the colour network with dir_div = 1 -- the
 * launches of cn_render_fwd's field part, so the networks must satisfy its conditions (the
 * folded feature head: CN_ERR_UNSUPPORTED otherwise; equal GEMM modes) and the results are
 * bitwise copenerf's composition SDFNetwork.field / ops.vertex_dirs / RenderingNetwork.color,
 * the same for every chunk_rows.  Optional outputs: rgb8 [M][3] (cn_rgb8_pack of rgb) and
 * grad [M][4] (∇ₓSDF, 16-byte aligned).  M = 0 writes nothing.  A chunk of
 * chunk x (widest buffer row) bytes >= 2^31 is CN_ERR_SHAPE before anything launches.
 * Workspace (256-byte aligned): cn_point_colors_workspace_bytes (one chunk's rows, sdf,
 * ∇ₓSDF, dirs and the two networks' buffers; 0 for a descriptor the call would refuse).
 * ------------------------------------------------------------------------ */
int cn_vertex_dirs(int64_t M, const float* G, int64_t ldg, float sign, float* dirs, cn_stream_t stream);
int cn_rgb8_pack(int64_t n, const float* rgb, uint8_t* out, cn_stream_t stream);
typedef struct cn_point_colors_desc {
    int64_t M;
    const float* x;                     /* [M][3] */
    const float* time_step;             /* device [1] */
    const cn_sdf_net* sdf_net;
    const cn_color_net* color_net;
    const float* view_dir;              /* HOST [3], or NULL: the inward normals */
    int32_t chunk_rows;
    float* rgb;                         /* [M][3] */
    uint8_t* rgb8;                      /* [M][3], or NULL */
    float* grad;                        /* [M][4], or NULL */
} cn_point_colors_desc;
size_t cn_point_colors_workspace_bytes(const cn_point_colors_desc* d);
int cn_point_colors(const cn_point_colors_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Connected components of a welded indexed triangle list and its compaction to the kept
 * components (additive to ABI v22): floater removal without leaving the device.  triangles
 * [T][3] are DEVICE int32 indices into V vertices (any such list, the mesher's or not).
 *
 * cn_mesh_label_init: label[v] = v.  cn_mesh_label_rounds: *changed = 0, then k rounds of
 *   (1) every triangle takes the minimum label of its corners and atomicMins it into all
 *       three, (2) every vertex jumps, label[v] = label[label[v]];
 * a round that lowers any label sets *changed (DEVICE int32) to 1.  Labels only fall and
 * stay vertex ids of the vertex's own component, so the fixed point -- every vertex holds
 * the smallest vertex id of its component -- is unique and does not depend on the order
 * of the atomics.  No kernel waits for another workgroup: the caller repeats the call
 * until *changed reads 0 (a host read; at most V rounds are ever needed, since round r
 * reaches every vertex within r edges of its component's smallest id).
 * cn_mesh_component_sizes: tri_count [V] = the triangles of every component at its root
 * id (the label of a triangle's first corner), 0 elsewhere; integer atomics, exact.
 * cn_mesh_select: a component is kept if it has at least min_triangles triangles and,
 * with keep_largest, is the one with the most triangles (a tie goes to the smaller root
 * id; none when T = 0).  Writes counts = (V', T') (DEVICE int64 [2]: the vertices whose
 * component is kept, the triangles whose first corner's is) and leaves the 0/1 flags and
 * their exclusive scans in the workspace.  cn_mesh_compact, with the same descriptor and
 * workspace, writes kept_vertices [V'] (the original ids, ascending) and triangles_out
 * [T'][3] (renumbered, in their original order); like cn_mesh_emit it checks
 * max_vertices / max_triangles against the device counts and writes nothing at all into
 * buffers that are too small.
 * Workspace (256-byte aligned), every piece rounded up to 256 bytes: V + T (flags) + 4 V
 * + 4 T (offsets) + 4 max(1, ceil(V / 1024)) + 4 max(1, ceil(T / 1024)) (the scans' tile
 * totals) + 8 (the largest component).  V < 0 or T < 0: CN_ERR_SHAPE (workspace_bytes: 0).
 * ------------------------------------------------------------------------ */
typedef struct cn_mesh_clean_desc {
    int32_t V, T;
    const int32_t* triangles;           /* [T][3] */
    int32_t* label;                     /* [V] */
    int32_t* tri_count;                 /* [V] -- cn_mesh_component_sizes, read by cn_mesh_select */
    int32_t keep_largest, min_triangles;
    int64_t* counts;                    /* device [2]: V', T' */
    int32_t* kept_vertices;             /* [max_vertices] -- cn_mesh_compact */
    int64_t max_vertices;
    int32_t* triangles_out;             /* [max_triangles][3] -- cn_mesh_compact */
    int64_t max_triangles;
} cn_mesh_clean_desc;
int cn_mesh_label_init(const cn_mesh_clean_desc* d, cn_stream_t stream);
int cn_mesh_label_rounds(const cn_mesh_clean_desc* d, int32_t k, int32_t* changed, cn_stream_t stream);
int cn_mesh_component_sizes(const cn_mesh_clean_desc* d, cn_stream_t stream);
size_t cn_mesh_clean_workspace_bytes(int32_t V, int32_t T);
int cn_mesh_select(const cn_mesh_clean_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);
int cn_mesh_compact(const cn_mesh_clean_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);
/* cn_mesh_select_mask (additive to ABI v22): cn_mesh_select's workspace and counts from a
 * caller's per-vertex mask instead of components: vertex v is kept when vmask[v] (DEVICE
 * uint8 [V]) is not 0, a triangle when all three corners are inside [0, V) and kept.  The
 * same scans, the same counts = (V', T'), the same workspace layout, so cn_mesh_compact
 * finishes it unchanged (its checks still want label and tri_count non-NULL and 4-byte
 * aligned; it reads neither, and neither does this entry).  Reads V, T, triangles, counts. */
int cn_mesh_select_mask(const cn_mesh_clean_desc* d, const uint8_t* vmask, void* workspace, int64_t workspace_bytes,
                        cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Mesh geometry metrics (additive to ABI v22): Chamfer distance and precision / recall /
 * F-score between a mesh and a point cloud without leaving the device.  The reference has no
 * geometry metric; the yardstick is float64 brute force.  Sizes are int64 so that a size at
 * or above 2^31 is refused (CN_ERR_SHAPE) instead of wrapping: V, T, S, N, Q < 2^31, and a
 * grid has at most 2^26 cells.  All checks run before any launch.
 *
 * cn_mesh_area / cn_mesh_sample: S points uniformly by area on vertices [V][3] fp32 /
 * triangles [T][3] int32.  cn_mesh_area computes every triangle's area in double from the
 * fp32 corners (0 for a corner index outside [0, V) or a non-finite area), leaves their
 * inclusive scan cdf [T] (double) in the workspace and writes area (DEVICE double [1]) =
 * cdf[T - 1] (0 when T = 0): the caller may read it -- one host read -- before fixing S.
 * The scan is a nest of sequential sums (4 triangles per thread, 64 threads per wave in
 * lane order, 4 waves per 1024-triangle tile, the tiles in order by one wave): bitwise
 * repeatable, never falling, and a zero-area triangle repeats its predecessor exactly.
 * cn_mesh_sample, with the same descriptor and workspace, draws sample i from
 * (u0, u1, u2) = elements 4 i, 4 i + 1, 4 i + 2 of cn_uniform_philox's stream for philox
 * (DEVICE uint64 [2] = (seed, offset)), i.e. words 0, 1, 2 of Philox4x32-10(counter
 * (i, offset), key seed), word 3 unused (the caller advances offset by S per draw of S
 * samples): tri[i] = the first t with cdf[t] > u0 area in double, by binary search (never
 * a zero-area triangle), points[i] = ((1 - r) a + r (1 - u2) b) + r u2 c in fp32 with
 * r = sqrtf(u1) and (a, b, c) the triangle's corners.  tri may be NULL.  With area = 0 the
 * points are zeros and tri is -1.  S > 0 with T = 0 is CN_ERR_SHAPE.
 * Workspace (256-byte aligned): 8 T (the cdf) + 8 max(1, ceil(T / 1024)) (the tile totals),
 * each rounded up to 256 bytes.
 * ------------------------------------------------------------------------ */
typedef struct cn_mesh_sample_desc {
    int64_t V, T;
    const float* vertices;              /* [V][3] */
    const int32_t* triangles;           /* [T][3] */
    double* area;                       /* device [1] -- written by cn_mesh_area, read by cn_mesh_sample */
    int64_t S;                          /* cn_mesh_sample only, as are the fields below */
    const uint64_t* philox;             /* device [2] = (seed, offset) */
    float* points;                      /* [S][3] */
    int32_t* tri;                       /* [S], or NULL */
} cn_mesh_sample_desc;
size_t cn_mesh_sample_workspace_bytes(int64_t T);
int cn_mesh_area(const cn_mesh_sample_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);
int cn_mesh_sample(const cn_mesh_sample_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* cn_nn_grid_build: a uniform grid of dims[0] x dims[1] x dims[2] cubic cells of edge `cell`
 * from `origin` (HOST values) over points [N][3].  The cell of a point is, per axis,
 * floor((p - origin) / cell) clamped into the grid (a point outside goes to the nearest
 * boundary cell, a NaN to cell 0); the cell id is (ix dims[1] + iy) dims[2] + iz.  An
 * integer-atomic histogram and an exclusive int32 scan give cell_start [ncells + 1]
 * (cell_start[ncells] = N); the points are scattered into sorted [N][4]: 16-byte records
 * (x, y, z, the original index as int32 bits), cell c's at [cell_start[c],
 * cell_start[c + 1]).  The order inside a cell is the atomics'; nothing below depends on it.
 * Workspace (256-byte aligned): 4 N (cell ids) + 4 ncells (counts) + 4 ceil(ncells / 1024)
 * (the scan's tile totals), each rounded up to 256 bytes.
 *
 * cn_nn_query: for each of Q queries the exact nearest point of a built grid, one lane per
 * query: dist [Q] and, unless NULL, index [Q] (the original index; the smaller one where
 * squared distances tie).  d^2 = ((dx dx + dy dy) + dz dz) and dist = sqrtf(d^2) in fp32.
 * Cells are visited in Chebyshev shells around the query's (clamped) cell until no unvisited
 * cell can hold a nearer point (the bound holds for queries and points outside the grid:
 * csrc/cn_mesh_eval.hip), until the bound reaches max_dist, or until the shell has left the
 * grid on every side; at most max(dims) shells.  A query with no point at a distance below
 * max_dist gets dist = max_dist, index = -1; max_dist = +inf searches everywhere.
 * query_records = 0: queries [Q][3] floats, outputs in query order.  query_records = 1:
 * queries are the `sorted` records [Q][4] of a cn_nn_grid_build over the queries (16-byte
 * aligned), and every output goes to its record's original index -- binning the queries
 * through the points' grid keeps a wave's lanes in neighbouring cells; the outputs are
 * bitwise the same either way.  No workspace. */
typedef struct cn_nn_grid_desc {
    int64_t N;
    const float* points;                /* [N][3] -- cn_nn_grid_build only */
    float origin[3];
    float cell;
    int32_t dims[3];
    int32_t* cell_start;                /* [ncells + 1] */
    float* sorted;                      /* [N][4], 16-byte aligned */
} cn_nn_grid_desc;
size_t cn_nn_grid_workspace_bytes(int64_t N, int64_t ncells);
int cn_nn_grid_build(const cn_nn_grid_desc* g, void* workspace, int64_t workspace_bytes, cn_stream_t stream);
typedef struct cn_nn_query_desc {
    const cn_nn_grid_desc* grid;        /* HOST: a grid cn_nn_grid_build has filled */
    int64_t Q;
    const float* queries;               /* [Q][3], or [Q][4] records */
    int32_t query_records;
    float max_dist;                     /* >= 0, +inf allowed */
    float* dist;                        /* [Q] */
    int32_t* index;                     /* [Q], or NULL */
} cn_nn_query_desc;
int cn_nn_query(const cn_nn_query_desc* d, cn_stream_t stream);

/* cn_knn_query (additive to ABI v22): for each of Q queries the exact k nearest points of a
 * built grid, 1 <= k <= 32, one lane per query: dist [Q][k] and index [Q][k].  A row is
 * ascending under the total order (squared distance in fp32 as cn_nn_query forms it, original
 * index) and holds exactly the k smallest pairs of that order among the targets with
 * dist = sqrtf(d^2) < max_dist; a row with fewer such targets is padded with (max_dist, -1).
 * count [Q] (or NULL) = the number found.  The shells and the stop rule are cn_nn_query's with
 * the k-th best pair in place of the best (the proof: csrc/cn_mesh_eval.hip); at k = 1 the
 * outputs are bitwise cn_nn_query's.  query_records as in cn_nn_query, with bitwise the same
 * outputs either way.  exclude_self = 1 skips the target whose original index is the query's
 * own (the query's position, or its record's index) -- exact duplicates at other indices are
 * kept; it needs Q = N (CN_ERR_SHAPE otherwise).  A lane's list is kept in LDS as [slot][lane]
 * (256 lanes x capacity x 8 bytes, capacity 8, 16 or 32: the smallest that holds k).
 * No workspace. */
typedef struct cn_knn_query_desc {
    const cn_nn_grid_desc* grid;        /* HOST: a grid cn_nn_grid_build has filled */
    int64_t Q;
    const float* queries;               /* [Q][3], or [Q][4] records */
    int32_t query_records;
    float max_dist;                     /* >= 0, +inf allowed */
    int32_t k;                          /* 1 .. 32 */
    int32_t exclude_self;
    float* dist;                        /* [Q][k] */
    int32_t* index;                     /* [Q][k] */
    int32_t* count;                     /* [Q], or NULL */
} cn_knn_query_desc;
int cn_knn_query(const cn_knn_query_desc* d, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Point-cloud preparation (additive to ABI v22, csrc/cn_cloud.hip): what the protocols do to
 * a raw scan before scoring -- voxel down-sampling, normals from the k nearest neighbours,
 * and the sums of the statistical outlier filter.  No pass uses an atomic; each is bitwise
 * repeatable.
 *
 * cn_voxel_keys: one thread per point.  Per axis f = fl(fl(p - origin) / voxel) in fp32
 * (origin, voxel: HOST values, voxel > 0 and finite); where 0 <= f < 2^21 on all three axes
 * keys[i] = (ix << 42) | (iy << 21) | iz with i = floor(f), valid[i] = 1; otherwise (a NaN or
 * infinite coordinate, or one outside the 21-bit range) keys[i] = CN_VOXEL_KEY_NONE, which
 * sorts after every voxel, and valid[i] = 0: such a point is dropped, never clamped into a
 * voxel.  valid may be NULL.
 *
 * cn_voxel_reduce: keys [N] are cn_voxel_keys' sorted ascending by a STABLE sort and order [N]
 * (int64) the original index of each sorted element.  Run heads are flagged and scanned (int32,
 * the three-launch block scan of the point grid); one thread per voxel walks its run -- in
 * ascending original index, the sort being stable -- and sums positions and, where given,
 * normals and colors (fp32 [N][3] each) in double.  Voxel v, in ascending key order, gets
 * out_points[v] = the fp32 of sum / count, out_colors[v] likewise, out_normals[v] = the fp32 of
 * sum / |sum| in double (a zero or non-finite |sum|: a zero normal), out_counts[v], out_keys[v]
 * (or NULL); totals (DEVICE int32 [2]) = (the number of voxels M, the points dropped).  The
 * outputs are sized for N voxels; rows from M on are not written.  An order entry outside
 * [0, N) gathers nothing.
 * Workspace (256-byte aligned): 4 N (run starts) + 4 max(1, ceil(N / 1024)) (tile totals),
 * each rounded up to 256 bytes.
 *
 * cn_cloud_normals: one thread per point over its neighbour row index [N][k] (cn_knn_query's
 * over the cloud itself; 1 <= k <= 32).  Entries of -1 are skipped and entries outside [0, N)
 * are skipped and never gathered.  The centroid, then the 3 x 3 covariance about it, of the
 * valid neighbours in row order in double; the eigenvector of the smallest eigenvalue by
 * cyclic Jacobi in double (at most 12 sweeps); normals [N][3] = that vector, unit, in fp32,
 * and variation [N] (or NULL) = l0 / (l0 + l1 + l2).  The normal (and the variation) is zero
 * with fewer than 3 valid neighbours, with a non-finite point or neighbour, and when
 * l1 <= 1e-12 l2 (a collinear neighbourhood) -- what cn_cloud_normal_stats and
 * cn_icp_accumulate leave out and count.  Sign: orient = 1 flips it so that
 * n . (orient_to - p) >= 0 (orient_to: HOST, finite); orient = 0 makes the fp32 component of
 * the largest magnitude positive, the first such component on a tie.  No workspace.
 *
 * cn_knn_mean_stats: mean [N] = per point the mean of the row's valid distances (dist [N][k]
 * where index [N][k] >= 0) in row order in double, stored in fp32 (+inf for a row without
 * one); out (DEVICE double [3]) = (the rows with a finite mean, the sum of those stored means,
 * the sum of their squares) in cn_cloud_stats' fixed two-launch tree.  The host forms
 * mu + ratio sigma.  Workspace (256-byte aligned): 24 blocks, rounded up to 256 bytes, blocks
 * as cn_cloud_stats'.
 * ------------------------------------------------------------------------ */
#define CN_VOXEL_KEY_NONE INT64_MAX
typedef struct cn_voxel_keys_desc {
    int64_t N;
    const float* points;                /* [N][3] */
    float origin[3];
    float voxel;
    int64_t* keys;                      /* [N] */
    int32_t* valid;                     /* [N], or NULL */
} cn_voxel_keys_desc;
int cn_voxel_keys(const cn_voxel_keys_desc* d, cn_stream_t stream);
typedef struct cn_voxel_reduce_desc {
    int64_t N;
    const int64_t* keys;                /* [N], sorted */
    const int64_t* order;               /* [N] */
    const float* points;                /* [N][3] */
    const float* normals;               /* [N][3], or NULL */
    const float* colors;                /* [N][3], or NULL */
    float* out_points;                  /* [N][3] */
    float* out_normals;                 /* [N][3], with normals */
    float* out_colors;                  /* [N][3], with colors */
    int64_t* out_keys;                  /* [N], or NULL */
    int32_t* out_counts;                /* [N] */
    int32_t* totals;                    /* device [2] */
} cn_voxel_reduce_desc;
size_t cn_voxel_reduce_workspace_bytes(int64_t N);
int cn_voxel_reduce(const cn_voxel_reduce_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);
typedef struct cn_cloud_normals_desc {
    int64_t N;
    const float* points;                /* [N][3] */
    const int32_t* index;               /* [N][k] */
    int32_t k;
    int32_t orient;
    float orient_to[3];
    float* normals;                     /* [N][3] */
    float* variation;                   /* [N], or NULL */
} cn_cloud_normals_desc;
int cn_cloud_normals(const cn_cloud_normals_desc* d, cn_stream_t stream);
typedef struct cn_knn_mean_stats_desc {
    int64_t N;
    int32_t k;
    const float* dist;                  /* [N][k] */
    const int32_t* index;               /* [N][k] */
    float* mean;                        /* [N] */
    double* out;                        /* device [3] */
} cn_knn_mean_stats_desc;
size_t cn_knn_mean_stats_workspace_bytes(int64_t N);
int cn_knn_mean_stats(const cn_knn_mean_stats_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* cn_cloud_stats: out (DEVICE double [4]) over dist [Q] (cn_nn_query's, with the same
 * max_dist) = (0) the points inside the crop box crop_min <= p <= crop_max (HOST values; all
 * Q when points is NULL), (1) those of them with dist < max_dist, (2) the sum of the
 * distances of (1), (3) those of (1) with dist < threshold.  The counts are exact; the sum
 * is a fixed-order double reduction (thread t of block b adds elements b 256 + t + j 256
 * blocks for j = 0, 1, ..., a fixed tree per block, one block over the block partials),
 * bitwise repeatable.  blocks = min(1024, max(1, ceil(Q / 1024))).
 * Workspace (256-byte aligned): 32 blocks, rounded up to 256 bytes. */
typedef struct cn_cloud_stats_desc {
    int64_t Q;
    const float* dist;                  /* [Q] */
    const float* points;                /* [Q][3], or NULL: no crop */
    float crop_min[3];
    float crop_max[3];
    float max_dist;
    float threshold;
    double* out;                        /* device [4] */
} cn_cloud_stats_desc;
size_t cn_cloud_stats_workspace_bytes(int64_t Q);
int cn_cloud_stats(const cn_cloud_stats_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* cn_cloud_normal_stats: the normal-consistency sums of one direction.  Over Q queries with
 * query_normals [Q][3], cn_nn_query's index / dist [Q] into N targets with target_normals
 * [N][3]: out (DEVICE double [3]) = (0) the pairs counted, (1) the sum of |q . t[index]| over
 * them, (2) the pairs left out because a normal has a zero or non-finite length.  A pair is
 * counted when the query is inside the crop box (cn_cloud_stats' rule; points NULL: no crop),
 * 0 <= index < N, dist < max_dist and both normals are usable -- the population of
 * cn_cloud_stats' distance mean.  Both normals are normalised in fp32 (v / sqrt((x x + y y) +
 * z z)); the dot product is taken in absolute value (orientation is a convention).  The
 * reduction is cn_cloud_stats' (the same blocks, fixed order, double): bitwise repeatable.
 * Workspace (256-byte aligned): 24 blocks, rounded up to 256 bytes. */
typedef struct cn_cloud_normal_stats_desc {
    int64_t Q, N;
    const float* query_normals;         /* [Q][3] */
    const float* target_normals;        /* [N][3] */
    const int32_t* index;               /* [Q] */
    const float* dist;                  /* [Q] */
    const float* points;                /* [Q][3], or NULL: no crop */
    float crop_min[3];
    float crop_max[3];
    float max_dist;
    double* out;                        /* device [3] */
} cn_cloud_normal_stats_desc;
size_t cn_cloud_normal_stats_workspace_bytes(int64_t Q);
int cn_cloud_normal_stats(const cn_cloud_normal_stats_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * ICP registration of a cloud to a target cloud (additive to ABI v22): what the
 * Tanks-and-Temples protocol refines the trajectory alignment with.  The device does the
 * passes of an iteration -- cn_cloud_transform, then cn_nn_grid_build / cn_nn_query over the
 * moved cloud for the correspondences, then cn_icp_accumulate; the closed-form solve of 32
 * doubles is the host's (copenerf.metrics.icp_register).  A correspondence kernel fused with
 * the transform was measured slower than that composition and is not kept.
 *
 * A similarity is `matrix`, 12 floats (HOST values): row-major 3 x 4, s R in the left 3 x 3
 * and t in the last column.  One device function applies it everywhere, row (a, b, c, t) as
 *   p'_r = fmaf(c, z, fmaf(b, y, fmaf(a, x, t)))
 * so the same point under the same matrix is the same three floats in both entries below:
 * the sums are over the very points the search saw.  A non-finite matrix entry is CN_ERR_SHAPE.
 *
 * cn_cloud_transform: out [N][3] = the transform of points [N][3], one thread per point (out
 * may be points).
 *
 * cn_icp_accumulate: out (DEVICE double [32]) = the sums over the pairs (i, index[i]) (index:
 * cn_nn_query's over cn_cloud_transform's output, -1 where no target is within reach) with
 * 0 <= index[i] < N (any other index is no pair: nothing is gathered), walked in the source's
 * order in cn_cloud_stats' fixed two-launch tree (the same blocks rule): bitwise repeatable,
 * and independent of the grid's within-cell order.  p' is recomputed by the shared transform,
 * q = targets[index[i]]; every term is formed in double from the fp32 p', q and unit normal,
 * relative to pivot c (HOST doubles, finite; the target box's centre keeps the covariance
 * from cancelling far from the origin).
 *   mode 0 (point-to-point):  [0] n   [1] sum |p' - q|^2   [2..4] sum (p' - c)
 *     [5..7] sum (q - c)   [8..16] sum (q - c)(p' - c)^T, row-major (row: q's axis)
 *     [17] sum |p' - c|^2   [18..31] 0
 *   mode 1 (point-to-plane; n^ = target_normals[index[i]] normalised in fp32 as
 *     cn_cloud_normal_stats does, a pair with a zero or non-finite normal is left out):
 *     [0] n   [1] sum |p' - q|^2   [2] sum r^2, r = (p' - q) . n^
 *     [3..23] the upper triangle of sum J^T J row by row ((0,0) (0,1) .. (0,5) (1,1) .. (5,5)),
 *     J = [(p' - c) x n^, n^]   [24..29] sum J^T r   [30] the pairs left out   [31] 0
 * Q = 0 or N = 0: all zeros.  Workspace (256-byte aligned): 256 blocks bytes.
 * ------------------------------------------------------------------------ */
typedef struct cn_cloud_transform_desc {
    int64_t N;
    const float* points;                /* [N][3] */
    float matrix[12];
    float* out;                         /* [N][3] */
} cn_cloud_transform_desc;
int cn_cloud_transform(const cn_cloud_transform_desc* d, cn_stream_t stream);
typedef struct cn_icp_accumulate_desc {
    int64_t Q, N;
    const float* source;                /* [Q][3] */
    const float* targets;               /* [N][3] */
    const float* target_normals;        /* [N][3]; mode 1 only */
    const int32_t* index;               /* [Q] */
    float matrix[12];
    int32_t mode;
    double pivot[3];
    double* out;                        /* device [32] */
} cn_icp_accumulate_desc;
size_t cn_icp_accumulate_workspace_bytes(int64_t Q);
int cn_icp_accumulate(const cn_icp_accumulate_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Mesh depth rendering and visibility (additive to ABI v22): what the ScanNet / DTU /
 * Tanks-and-Temples protocols cull a predicted mesh with before they measure it.  The
 * reference has no rasteriser; the yardstick is a float64 restatement.  A camera is a 3 x 4
 * projection P (fp32, row-major): (a, b, c) = P [X, 1] puts X at pixel (a / c, b / c), pixel
 * centres at integers, at depth c (> 0 in front of the camera).
 *
 * cn_mesh_raster: depth [N][h][w] (+inf where nothing is seen) and tri [N][h][w] (the
 * triangle seen, -1 where none) of vertices [V][3] fp32 / triangles [T][3] int32 under proj
 * [N][3][4].  Per vertex, in fp32 and this order: a = ((P00 x + P01 y) + P02 z) + P03 (b, c
 * alike), sx = a / c, sy = b / c, iw = 1 / c.  The edge function of an edge at pixel p is
 * E = (hx - lx)(py - ly) - (hy - ly)(px - lx) with l its corner of the smaller vertex index,
 * negated for the triangle that runs the edge from the larger index: two triangles that share
 * an edge get the same value with opposite signs, so no pixel centre falls between them.  A
 * pixel centre is covered when the three edge values e0, e1, e2 (ek opposite corner k) are all
 * >= 0 or all <= 0 (two-sided, inclusive); its depth is ((e0 + e1) + e2) / ((e0 iw0 + e1 iw1)
 * + e2 iw2), i.e. 1 / c interpolated linearly in screen space.  The smallest depth wins, equal
 * depths go to the smaller triangle id (a 64-bit atomicMin over (depth bits, id)): the images
 * do not depend on scheduling.  A triangle with a corner index outside [0, V), zero screen
 * area, or any corner at c < near (or not finite) is skipped in that view -- there is no
 * clipping.  The bounding box is clamped to the image.  A triangle whose box holds at most
 * pixel_budget pixels (0: 64) is walked by one thread; a larger one goes onto a list and is
 * walked by a whole workgroup in a second launch.  Views are processed view_batch (0: 8) at a
 * time, fewer where T x batch or h w x batch would reach 2^31.  stats (DEVICE int64 [2], or
 * NULL) receives the (triangle, view) pairs walked by a thread and by a workgroup.
 * Workspace (256-byte aligned), with B the batch, each rounded up to 256 bytes: 8 B h w (the
 * z-buffer) + 16 B V (projected vertices) + 8 B T (the list: room for every pair, it cannot
 * overflow) + 4.  V, T, h w < 2^31; near > 0.
 * ------------------------------------------------------------------------ */
typedef struct cn_mesh_raster_desc {
    int64_t V, T;
    const float* vertices;              /* [V][3] */
    const int32_t* triangles;           /* [T][3] */
    int32_t N, h, w;
    int32_t view_batch;                 /* 0: 8 */
    const float* proj;                  /* [N][3][4] */
    float near;
    int32_t pixel_budget;               /* 0: 64 */
    float* depth;                       /* [N][h][w] */
    int32_t* tri;                       /* [N][h][w] */
    int64_t* stats;                     /* device [2], or NULL */
} cn_mesh_raster_desc;
size_t cn_mesh_raster_workspace_bytes(int64_t V, int64_t T, int32_t N, int32_t h, int32_t w, int32_t view_batch);
int cn_mesh_raster(const cn_mesh_raster_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* cn_mesh_visibility: count [Q] = the views that see each of points [Q][3], one thread per
 * point, no atomics.  A view sees a point when c >= near, the pixel (floor(a / c + 0.5),
 * floor(b / c + 0.5)) lies inside the h x w image and, with depth [N][h][w] given (cn_mesh_raster's),
 * c <= depth[pixel] (1 + tol_rel) + tol_abs (fp32: one product, one sum; a pixel that shows
 * nothing, +inf, hides nothing).  depth = NULL: the frustum test alone.  No workspace. */
typedef struct cn_mesh_visibility_desc {
    int64_t Q;
    const float* points;                /* [Q][3] */
    int32_t N, h, w;
    float near;
    const float* proj;                  /* [N][3][4] */
    const float* depth;                 /* [N][h][w], or NULL */
    float tol_abs, tol_rel;
    int32_t* count;                     /* [Q] */
} cn_mesh_visibility_desc;
int cn_mesh_visibility(const cn_mesh_visibility_desc* d, cn_stream_t stream);

/* cn_mesh_shade: what cn_mesh_raster's tri [N][h][w] shows, one thread per pixel, no atomics,
 * bitwise repeatable; it takes the rasteriser's tri image and decides no coverage itself.  For
 * a pixel whose tri is t the three corners are projected and the edge values e_k formed
 * exactly as cn_mesh_raster documents (the same fp32 operation order), and the
 * perspective-correct weights are lambda_k = e_k iw_k / ((e_0 iw_0 + e_1 iw_1) + e_2 iw_2).
 * Outputs, each optional (NULL):
 *   attr_out [N][h][w][C] = (lambda_0 A_0 + lambda_1 A_1) + lambda_2 A_2 of attr [V][C], 1 <= C <= 16;
 *   normal_out [N][h][w][3]: the unit geometric normal (X_1 - X_0) x (X_2 - X_0), turned
 *     towards the camera (two-sided rendering): as wound it faces the camera iff (signed
 *     screen area of the projected corners) x det(proj[:, :3]) < 0.  With vnormals [V][3]:
 *     the normalised interpolation of the vertex normals, negated into the oriented face
 *     normal's hemisphere; a zero or non-finite interpolation leaves the face normal.  With
 *     rot [N][3][3]: rot[view] . n (e.g. the world-to-camera rotation);
 *   normal_img uint8 [N][h][w][3] = to_u8(n 128 + 128), cn_visual_images' rule (NaN and
 *     negatives 0, truncation, saturation at 255);
 *   shaded_img uint8 [N][h][w][3] = to_u8(albedo (ambient + (1 - ambient) max(0, n . light))
 *     255), albedo the first three channels of the interpolated attributes with
 *     albedo_from_attr (C >= 3; colours in [0, 1]), else grey; light: a unit vector in
 *     normal_out's frame (HOST values).
 * Background -- tri outside [0, T) or a corner index outside [0, V): fill in attr_out, the zero
 * vector in normal_out, background in both pictures; nothing else is read for such a pixel.
 * V, T, h w < 2^31; no workspace. */
typedef struct cn_mesh_shade_desc {
    int64_t V, T;
    const float* vertices;              /* [V][3] */
    const int32_t* triangles;           /* [T][3] */
    int32_t N, h, w;
    int32_t C;                          /* 1 .. 16 with attr */
    const float* proj;                  /* [N][3][4] */
    const int32_t* tri;                 /* [N][h][w], cn_mesh_raster's */
    const float* attr;                  /* [V][C], or NULL */
    const float* vnormals;              /* [V][3], or NULL: face normals */
    const float* rot;                   /* [N][3][3], or NULL */
    float fill;
    float ambient;                      /* in [0, 1] */
    float light[3];
    float grey;
    int32_t albedo_from_attr;
    uint8_t background[3];
    float* attr_out;                    /* [N][h][w][C], or NULL */
    float* normal_out;                  /* [N][h][w][3], or NULL */
    uint8_t* normal_img;                /* [N][h][w][3], or NULL */
    uint8_t* shaded_img;                /* [N][h][w][3], or NULL */
} cn_mesh_shade_desc;
int cn_mesh_shade(const cn_mesh_shade_desc* d, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * TSDF fusion (additive to ABI v22): per-view depth maps fused into a truncated signed
 * distance volume, the other way NeuS-family and ScanNet-style evaluations get a mesh (render
 * or read a depth per view, fuse, mesh what the cameras saw).  The reference has no fusion
 * code; the yardstick is a float64 restatement.  Cameras are cn_mesh_raster's 3 x 4
 * projections, depths are its c.
 *
 * cn_tsdf_integrate: the running volumes tsum [nx][ny][nz], wsum [nx][ny][nz] and, with colours,
 * csum [nx][ny][nz][3] (fp32, read and written; zero them before the first call) take in the N
 * views proj [N][3][4], depth [N][h][w] and color [N][h][w][3] (or NULL, exactly when csum is).
 * One thread per voxel, z fastest; no workspace, no allocation, no synchronisation.  Voxel
 * (ix, iy, iz) sits at X_ax = (float)i / (float)(n - 1) * (hi - lo) + lo, all in fp32: the
 * mesher's vertex map at integer positions, so mesh and volume agree (not cn_grid_points'
 * linspace rule).  Per view, in view order, in fp32 and in this order:
 *   1. a = ((P00 x + P01 y) + P02 z) + P03, b and c alike;
 *   2. skip unless c >= near;
 *   3. pixel (floor(a / c + 0.5), floor(b / c + 0.5)), as cn_mesh_visibility; skip outside the image;
 *   4. d = depth[view][py][px]; skip unless d is finite, d > 0 and d <= depth_max ("0 where
 *      nothing is seen" and "+inf where nothing is seen" both mean no observation; so does NaN);
 *   5. s = d - c; skip if s < -trunc;
 *   6. tsum += fminf(1, s / trunc), wsum += 1, csum += color[view][py][px].
 * A voxel's result depends on nothing but its own sequence of views: there are no atomics, the
 * result is bitwise repeatable, and one call with N views is bitwise equal to any split of the
 * same views, in the same order, over several calls (each volume is read once and written once
 * per call; the batch that was measured fastest: DESIGN.md 3.12.5).  A wavefront's 64 voxels may skip a view as a whole
 * when their bounding box lies, with a margin far above the fp32 error, behind `near` or off
 * one side of the image; the skip never changes a result (no_reject = 1 turns it off, for
 * measurement).  N = 0 is a no-op without a launch.  Any dim below 2, nx ny nz or h w >= 2^31:
 * CN_ERR_SHAPE; trunc, near > 0 and finite; depth_max > 0, +inf for none.
 * ------------------------------------------------------------------------ */
typedef struct cn_tsdf_desc {
    int32_t nx, ny, nz;
    float lo[3], hi[3];
    int32_t N, h, w;
    const float* proj;                  /* [N][3][4] */
    const float* depth;                 /* [N][h][w] */
    const float* color;                 /* [N][h][w][3], or NULL */
    float trunc, near, depth_max;
    int32_t no_reject;                  /* 1: no wavefront skips a view (measurement) */
    float* tsum;                        /* [nx][ny][nz] */
    float* wsum;                        /* [nx][ny][nz] */
    float* csum;                        /* [nx][ny][nz][3], NULL exactly when color is */
} cn_tsdf_desc;
int cn_tsdf_integrate(const cn_tsdf_desc* d, cn_stream_t stream);

/* cn_tsdf_finalize: u [nx][ny][nz] = tsum / wsum where wsum >= min_weight (min_weight >= 1), NaN
 * elsewhere ("unobserved": what cn_mesh_*_observed and cn_volume_sample's mask read); with rgb
 * (optional, needs csum) rgb [nx][ny][nz][3] = csum / wsum there and 0 elsewhere.  The sign is
 * the mesher's: positive in front of the surface, so triangle normals point out of it.  One
 * thread per voxel, no workspace. */
typedef struct cn_tsdf_finalize_desc {
    int32_t nx, ny, nz;
    float min_weight;
    const float* tsum;
    const float* wsum;
    const float* csum;                  /* or NULL */
    float* u;
    float* rgb;                         /* or NULL */
} cn_tsdf_finalize_desc;
int cn_tsdf_finalize(const cn_tsdf_finalize_desc* d, cn_stream_t stream);

/* cn_volume_sample: out [Q][C] (1 <= C <= 4) = the trilinear interpolation of attr
 * [nx][ny][nz][C] at points [Q][3], one thread per point, no atomics, no workspace.  Index
 * position per axis, in fp32: g = (x - lo) / (hi - lo) * (n - 1), clamped to [0, n - 1] (a point
 * outside the box samples its nearest face); i0 = min((int)floorf(g), n - 2); f = g - i0.  Corner
 * o = ox + 2 oy + 4 oz has weight (wx wy) wz with w = f where the offset is 1, 1 - f where it is
 * 0; out = the sum over o = 0 .. 7, in that order, of weight x attr.  With mask [nx][ny][nz] (a u
 * volume, NaN meaning unobserved) a corner that is unobserved gets weight 0 and is not read,
 * and the sum is divided by the sum of the remaining weights; a point whose observed corners
 * carry no weight (none is observed, or only corners of weight 0) gets `fill` in every channel.
 * hi > lo on every axis; Q < 2^31. */
typedef struct cn_volume_sample_desc {
    int32_t nx, ny, nz;
    int32_t C;
    float lo[3], hi[3];
    const float* attr;                  /* [nx][ny][nz][C] */
    const float* mask;                  /* [nx][ny][nz], or NULL */
    int64_t Q;
    const float* points;                /* [Q][3] */
    float fill;
    float* out;                         /* [Q][C] */
} cn_volume_sample_desc;
int cn_volume_sample(const cn_volume_sample_desc* d, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Pose refinement (ABI v17): compute_loss_and_warp_image
 * (utils_poses/pose_refinement.py:34-61) for J (target, source) jobs over one image
 * stack, with the pose gradient in the same pass -- the per-batch work of
 * perform_pose_refinement (pose_refinement.py:104-128) in one launch and one
 * fixed-order reduction instead of a dozen full-image torch ops each way and
 * grid_sample's backward.
 *   images [N][3][H][W] planar (the reference's imgs), depth [N][H][W];
 *   tgt [J], src [J]: int32 frame indices (the depth used is depth[tgt[j]]); a job with
 *     an index outside [0, N) reads nothing and gives zero sums;
 *   pose [J][12]: row-major 3 x 4 [R | t], the target camera's frame to the source's;
 *   K [J][9], Kinv [J][9]: row-major 3 x 3.
 * Per pixel (row i, column c) of the target, all fp32 without contraction:
 *   u = c / ((W-1)/2) - 1, v = i / ((H-1)/2) - 1              (pose_refinement.py:93-100)
 *   X = Kinv (u d, v d, d), Y = R X + t, q = K Y, (u', v') = (q0, q1) / q2
 *   valid = u' and v' in [-1, 1] (the only test, as pose_refinement.py:50-53)
 *   warp  = the bilinear sample of images[src] at (u', v'), border padding,
 *           align_corners=True (Trainer.warp_pixel, train.py:235-244)
 *   sums [J][2]   = (sum over valid pixels and the 3 channels of |warp - target|,
 *                    the number of valid pixels)
 *   dpose [J][12] = d sums[j][0] / d pose[j] (16-byte aligned): sign(warp - target) with
 *                   sign(0) = 0, the bilinear derivative zero where the coordinate is
 *                   clamped (torch's border rule), no gradient through the mask
 *   warped        : NULL, or [J][3][H][W] = warp at every pixel (the reference's
 *                   second return value)
 * Reduction: one partial per 64 x 16 pixel tile and job, summed over a job's tiles in
 * a fixed order; no atomics.  Bitwise reproducible, and a job's results do not depend
 * on the other jobs of the call.  The valid counts are exact (below 2^24 per frame).
 * Frame base offsets are 64-bit; H, W >= 2 and 3 H W < 2^31, J <= 65535 (else
 * CN_ERR_SHAPE; cn_refine_workspace_bytes: 0).  Workspace (256-byte aligned):
 * ceil(W / 64) ceil(H / 16) J x 64 bytes, rounded up to 256.  J = 0: nothing is written.
 * ------------------------------------------------------------------------ */
size_t cn_refine_workspace_bytes(int32_t J, int32_t H, int32_t W);
int cn_refine_warp(int32_t N, int32_t H, int32_t W, int32_t J, const float* images, const float* depth,
                   const int32_t* tgt, const int32_t* src, const float* pose, const float* K,
                   const float* Kinv, float* sums, float* dpose, float* warped, void* workspace,
                   int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Evaluation metrics (ABI v18).
 *
 * cn_image_metrics: co3d_metric.py's psnr (lines 14-16) and ssim / _ssim (lines 18-48)
 * for N x C (image, channel) planes in one fused pass: the reference runs five depthwise
 * 11 x 11 convolutions and about fifteen full-image elementwise launches per pair
 * (eval.py:190-221, after copying the rendered maps to the host and back).
 *   pred, gt [N][C][H][W] contiguous fp32;
 *   taps: HOST pointer to the 11 fp32 window weights (co3d_metric.py:49-51, built by the
 *     caller; the library derives nothing).  Only window 11 exists.
 *   out [N][C][2]  = (mean of (pred - gt)^2, mean of the SSIM map) per image and channel
 *     (eval.py:204 calls psnr on an unbatched [3, H, W] tensor, so the reference's PSNR
 *     is the mean of three per-channel PSNRs: the caller needs the channels apart);
 *   ssim_map: NULL, or [N][C][H][W] = the SSIM map.
 * Semantics, all fp32 without contraction (co3d_metric.py:28-43): the window applied to
 * x, y, x x, y y, x y with zero padding of 5 on every side (separably: along x, then
 * along y, taps in ascending order); sigma = E[.] - mu^2; C1 = 0.01^2, C2 = 0.03^2;
 *   ssim = (2 mu1 mu2 + C1)(2 sigma12 + C2) / ((mu1^2 + mu2^2 + C1)(sigma1 + sigma2 + C2)),
 * no clamping.  An image smaller than the window is legal.  Identical inputs give a map
 * of exactly 1 and a squared error of exactly 0.
 * Reduction: one fp32 partial per 64 x 16 tile and plane (lanes, then waves, in a fixed
 * order); a second kernel sums a plane's tiles in a fixed order in double, divides by
 * H W and rounds once.  No atomics: bitwise reproducible, and a plane's result does not
 * depend on the rest of the batch.  Plane base offsets are 64-bit.
 * C, H or W < 1, N < 0, N C > 65535, H W >= 2^31, 2^24 or more tiles per plane (more
 * workgroups than the grid holds) or a workspace that is too small:
 * CN_ERR_SHAPE (cn_image_metrics_workspace_bytes: 0).  N = 0: nothing is written, 0.
 * Workspace (256-byte aligned): N C ceil(W / 64) ceil(H / 16) x 8 bytes, rounded up to 256.
 *
 * cn_depth_errors: Evaluator.depth_eval's per-image work (eval.py:233-241) and
 * Trainer.compute_depth_errors (train.py:180-193; model/training.py:126-154 is the same
 * without the clamp).  For each of N images, every ground-truth pixel (y, x) with
 * min_depth <= gt <= max_depth takes
 *   p = pred[y Hp / Hg][x Wp / Wg] * ratio[n]      (integer division; ratio: DEVICE [N]),
 * clamped to [min_depth, max_depth] when clamp != 0, and with d = gt - p,
 * thresh = max(gt / p, p / gt):
 *   out [N][8] = mean |d| / gt, mean d^2 / gt, sqrt(mean d^2), sqrt(mean (log gt - log p)^2),
 *                mean(thresh < 1.25), mean(thresh < 1.25^2), mean(thresh < 1.25^3), count.
 * No valid pixel: seven NaN and count 0.  The counts are summed exactly (per-workgroup
 * integers, then double) and rounded to fp32 once, like the other sums.
 * The nearest-neighbour rule is floor(dst * src_size / dst_size); the reference uses
 * cv2.resize(INTER_NEAREST), which was not available to compare against: the rule is
 * unambiguous (and tested) for equal sizes and integer ratios only.
 * The median ratio (eval.py:237) is the caller's: copenerf.metrics computes it on the device.
 * N < 0, N > 65535, any size < 1, Hg Wg or Hp Wp >= 2^31, or a workspace that is too small:
 * CN_ERR_SHAPE.  Workspace (256-byte aligned): N ceil(Hg Wg / 2048) x 32 bytes, rounded
 * up to 256.
 * ------------------------------------------------------------------------ */
size_t cn_image_metrics_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int cn_image_metrics(int32_t N, int32_t C, int32_t H, int32_t W, const float* pred, const float* gt,
                     const float* taps, float* out, float* ssim_map, void* workspace,
                     int64_t workspace_bytes, cn_stream_t stream);
size_t cn_depth_errors_workspace_bytes(int32_t N, int32_t Hg, int32_t Wg);
int cn_depth_errors(int32_t N, int32_t Hg, int32_t Wg, const float* gt, int32_t Hp, int32_t Wp,
                    const float* pred, const float* ratio, float min_depth, float max_depth, int32_t clamp,
                    float* out, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* cn_normal_errors (additive to ABI v22): the angle between two normal maps pred, gt fp32
 * [n][3] (any frame, the same for both; any length).  Pixel i is valid when mask (uint8 [n], or
 * NULL: all) is not 0 and both normals have a finite, non-zero length.  Both are normalised
 * in fp32 (v / sqrt((x x + y y) + z z)) and
 *   angle[i] = atan2(|p x g|, p . g) in degrees (fp32; NaN where invalid),
 * not acos of the dot product, which loses half its digits near 0 degrees.  Identical maps
 * give 0 exactly, antiparallel ones 180.
 *   out (DEVICE double [6]) = valid pixels, sum angle, sum angle^2, and the counts of
 *   angle < 11.25, < 22.5, < 30 degrees.
 * Fixed-order double reduction (thread t of block b takes pixels b 256 + t + j 256 blocks, a
 * fixed tree per block, one block over the block partials): bitwise repeatable.  blocks =
 * min(1024, max(1, ceil(n / 2048))).  n = 0: six zeros.  n < 0 or n >= 2^31: CN_ERR_SHAPE.
 * Workspace (256-byte aligned): 48 blocks, rounded up to 256 bytes. */
size_t cn_normal_errors_workspace_bytes(int64_t n);
int cn_normal_errors(int64_t n, const float* pred, const float* gt, const uint8_t* mask, float* angle, double* out,
                     void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Visualisation renders (ABI v19): Trainer.render_visdata (model/training.py:157-374).
 *
 * cn_ray_visuals: the per-ray tail of the render loop (training.py:236-281) for R rays of
 * S samples in one read of the samples (28 bytes each), instead of a clone of the points,
 * K passes of cross / add / mul over [R S, 3], weighted sums, an argmax and a gather.
 *   pts [R S][ld_p], normals [R S][ld_n]: columns 0..2 are used (ld in elements, >= 3;
 *     when both have rows of a multiple of 4 floats on a 16-byte boundary, a row is one
 *     16-byte load: its fourth float is read and must lie inside the caller's buffer);
 *   weights [R][S] contiguous;
 *   world_mat: DEVICE [4][4] row-major, or NULL for the identity;
 *   omega [K][3], vel [K][3]: DEVICE, the K Euler steps' angular and linear velocities;
 *     dt: the HOST step length;  0 <= K <= 1024;
 *   proj: DEVICE [3][3] = scale_mat[:3,:3] @ camera_mat[:3,:3] (the caller's product);
 *   pix [R][2]: the rays' normalised pixel coordinates;
 *   flow_scale: HOST [2] = (w / 2, h / 2).
 * Outputs, each may be NULL (an input only a NULL output reads may be NULL as well):
 *   normal [R][3]   = sum_s w n, multiplied by world_mat[:3,:3] when world_mat is given
 *                     (training.py:255-260);
 *   depth_max_w [R] = -(world_mat (p*, 1))[2] with p* the sample of the largest weight,
 *                     the lowest index among equal weights (torch.max, training.py:236-243);
 *                     with a NULL world_mat exactly -p*[2].  All weights NaN: sample 0;
 *   flow [R][2]     = ((q.xy / q.z) - pix) * flow_scale, q = proj P, P = sum_s w_s p_s^(K),
 *                     p^(k+1) = p^(k) + dt (omega_k x p^(k) + vel_k)   (training.py:269-281,
 *                     299-300).  IEEE results propagate when q.z = 0.
 * Every Euler step is affine in p, so the K steps compose into one map p -> A p + b and
 * sum_s w (A p + b) = A sum_s w p + b sum_s w: a one-wavefront kernel composes (A | b)
 * from omega and vel on the device (no host synchronisation) into the workspace, and the
 * main kernel forms sum w p, sum w, sum w n and the arg-max per ray -- one wavefront per
 * ray, lane l taking samples l, l + 64, ... in ascending order, the lanes combined in a
 * fixed order.  A ray's results depend on that ray alone and are bitwise reproducible.
 * The sums are fp32 (fused multiply-adds); they differ from the reference's per-sample
 * composition by rounding only.  Row offsets are 64-bit.
 * R < 0, S < 1, K outside [0, 1024], ld_p or ld_n < 3, a workspace that is too small:
 * CN_ERR_SHAPE.  flow with K = 0, or without proj / pix / flow_scale / omega / vel; NULL
 * weights; NULL pts with flow or depth_max_w; NULL normals with normal: CN_ERR_ARG.
 * Everything is checked before the first launch.  R = 0: nothing is written, 0.
 * Workspace (256-byte aligned, needed for a flow only): cn_ray_visuals_workspace_bytes(K)
 * = 256 for 1 <= K <= 1024, else 0.
 *
 * cn_visual_images: the per-image arithmetic of training.py:292-318, 343-345 for one
 * H x W render: a statistics pass (one partial per 2048 pixels, then one wavefront over
 * the partials in a fixed order), then one pass that writes the images.  No atomics; min
 * and max do not depend on the order, so the statistics are exact.
 *   rgb [HW][3], depth [HW], depth_max_w [HW], weighted_z [HW], normal [HW][3],
 *   flow [HW][2] (may be NULL): contiguous fp32.
 *   stats [5] fp32 (DEVICE) = min weighted_z, max weighted_z, max 1 / depth,
 *     max 1 / depth_max_w, max |flow| = sqrt(fx fx + fy fy) (0 without a flow).  A NaN
 *     input gives a NaN statistic (numpy's min / max).  stats may be NULL when no
 *     disparity or flow image is asked for; with stats, depth, depth_max_w and
 *     weighted_z are required.
 *   uint8 images, each may be NULL (an image needs its input); trunc() toward zero, NaN
 *   gives 0, every value clamped to [0, 255]; fp32, each operation rounded, none fused:
 *     img [H][W][3]        = trunc(rgb * 255)                         (training.py:293);
 *     disparity [H][W]     = trunc(((1 / depth) / stats[2]) * 255)    (training.py:309-310, 329);
 *     disparity_hw [H][W]  = trunc(((1 / depth_max_w) / stats[3]) * 255)   (311-312, 330);
 *       the contract is positive depths;
 *     normal_img [H][W][3] = trunc(normal * 128 + 128)                (training.py:314-318);
 *     flow_img [H][W][3]   = torchvision.utils.flow_to_image (training.py:302), that is:
 *       the wheel has 55 rows from the segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 with
 *       the ramps floor(255 i / n):  RY (255, r, 0), YG (255 - r, 255, 0), GC (0, 255, r),
 *       CB (0, 255 - r, 255), BM (r, 0, 255), MR (255, 0, 255 - r);
 *       u = flow / (stats[4] + FLT_EPSILON), norm = |u|, a = atan2(-u.y, -u.x) / pi,
 *       fk = (a + 1) / 2 * 54, k0 = floor(fk), k1 = (k0 + 1) mod 55, f = fk - k0;
 *       per channel col = (1 - f) wheel[k0] / 255 + f wheel[k1] / 255,
 *       col = 1 - norm (1 - col), pixel = floor(255 col).
 *       A zero flow field gives an all-white image exactly.
 * H or W < 1, H W >= 2^31, a workspace that is too small: CN_ERR_SHAPE
 * (cn_visual_images_workspace_bytes: 0).  NULL stats with a disparity or flow image, an
 * image without its input: CN_ERR_ARG.  Workspace (256-byte aligned, needed with stats):
 * ceil(H W / 2048) x 32 bytes, rounded up to 256.
 * ------------------------------------------------------------------------ */
size_t cn_ray_visuals_workspace_bytes(int32_t K);
int cn_ray_visuals(int32_t R, int32_t S, const float* pts, int64_t ld_p, const float* normals, int64_t ld_n,
                   const float* weights, const float* world_mat, int32_t K, const float* omega,
                   const float* vel, float dt, const float* proj, const float* pix, const float* flow_scale,
                   float* normal, float* depth_max_w, float* flow, void* workspace, int64_t workspace_bytes,
                   cn_stream_t stream);
size_t cn_visual_images_workspace_bytes(int32_t H, int32_t W);
int cn_visual_images(int32_t H, int32_t W, const float* rgb, const float* depth, const float* depth_max_w,
                     const float* weighted_z, const float* normal, const float* flow, float* stats,
                     uint8_t* img, uint8_t* disparity, uint8_t* disparity_hw, uint8_t* normal_img,
                     uint8_t* flow_img, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * LPIPS (VGG16, the v0.1 linear heads) from user-supplied weights (ABI v20): what
 * co3d_metric.lpips(pred, gt, net_type="vgg") computes for eval.py:190-221
 * (lpipsPyTorch/modules/{lpips,networks,utils}.py), for one pair of [3][H][W] images in
 * [0, 1] (no 2x - 1 rescale), instead of 26 library convolutions and about sixty
 * elementwise launches per pair:
 *   1. z = (x - mean) / std per channel, mean (-.030, -.088, -.188), std (.458, .448, .450);
 *   2. VGG16 features[0:30]: thirteen 3 x 3 convolutions (stride 1, zero padding 1, bias,
 *      ReLU) of widths 64 64 | 128 128 | 256 256 256 | 512 512 512 | 512 512 512, a 2 x 2
 *      stride-2 max-pool between the five blocks (floor: an odd last row / column is
 *      dropped); the last activation of each block is tapped;
 *   3. each tap unit-normalised over its channels: f^ = f / (sqrt(sum_c f^2) + 1e-10);
 *   4. term_b = mean over the block's pixels of sum_c lin_b[c] (fx^ - fy^)^2.
 * The library ships and fetches no weights: the caller passes them.
 *
 * cn_lpips_patches: the convolution's operand rows.  For output rows [y0, y0 + rows) of n
 * maps, out [n rows Wo][kpad], row (i rows + r) Wo + x, column (dy 3 + dx) C + c = the
 * source at (y0 + r + dy - 1, x + dx - 1, c) of map i, zero outside the map; columns
 * [9 C, kpad) are zero.  mode 0: src is an NHWC map [n][Hs][Ws][C] (Ho = Hs, Wo = Ws);
 * mode 1: the source is the 2 x 2 floor max-pool of that stored map, taken on read
 * (Ho = Hs / 2, Wo = Ws / 2); mode 2 (C = 3, n <= 2): src and src1 are planar images
 * [3][Hs][Ws], z-scored on read with a true fp32 division.  C a power of two in
 * [4, 4096] (modes 0, 1), kpad a multiple of 4; loads along c and stores are 16 bytes
 * (src, out 16-byte aligned); row offsets are 64-bit.
 *
 * cn_lpips_head: one block's term from its two NHWC taps fx, fy [P][C] (P pixels, C a
 * power of two in [16, 512]) and lin [C]: out[0] = (sum_p sum_c lin[c] (fx^ - fy^)^2) / P.
 * min(64, C / 4) lanes per pixel, one pass; one fp32 partial per workgroup of 64 pixels
 * (lanes, then waves, in a fixed order); a second kernel sums the partials in a fixed
 * order in double, divides by P and rounds once.  No atomics: bitwise reproducible;
 * fx == fy gives exactly 0.  Workspace (256-byte aligned): ceil(P / 64) x 4 bytes,
 * rounded up to 256.
 *
 * cn_lpips: the whole metric for one pair.  Each convolution is cn_lpips_patches into the
 * workspace, then cn_linear (CN_EPI_RELU) on the caller's packed weights; both images are
 * one batch of two, so a weight image is read once per band.
 *   weights[l]: the image cn_pack_weights builds (format = mfma_dtype) from the layer's
 *     [Cout][Kpad] matrix with columns (dy 3 + dx) Cin + c, padded with zero rows to a
 *     multiple of 128 rows; Kpad = 9 Cin, and for the first layer 32 (CN_MFMA_BF16: 64);
 *   bias[l] [Cout], lin[b] [C_b] fp32, 16-byte aligned;
 *   mfma_dtype: CN_MFMA_F32_BF16X6 (the default of the Python side), CN_MFMA_BF16 or
 *     CN_MFMA_F32;
 *   band_rows: the patch matrix holds at most this many output rows of a layer at a time
 *     (both images); 0 = the library's choice: per layer the most rows that keep the patch
 *     matrix within 576 MiB (at least one row).  A layer's bands are of equal height up
 *     to one row (540 x 960: conv1_2 in four bands of 135 rows, conv2_2 in two, every
 *     other layer in one).  Only the
 *     patch matrix is banded, the maps are whole, and a GEMM row depends on its own
 *     operand row alone: out does not depend on band_rows, bit for bit;
 *   out [6] (DEVICE): the five terms in block order, then their fp32 sum in that order.
 * The terms are part of the contract (a test localises an error with them).
 * Workspace (256-byte aligned): two maps of 2 H W 64 floats, the patch matrix, the heads'
 * partials, each rounded up to 256 bytes.  Nothing is allocated, nothing synchronises.
 * H or W < 16 (a block would be empty), H W > 2^26, band_rows < 0, a bad mfma_dtype, a
 * NULL pointer anywhere in the descriptor, a workspace that is NULL or too small:
 * CN_ERR_SHAPE (cn_lpips_workspace_bytes: 0 for the first four).
 * ------------------------------------------------------------------------ */
typedef struct cn_lpips_desc {
    const float* pred;        /* [3][H][W] */
    const float* gt;          /* [3][H][W] */
    int32_t H, W;
    const void* weights[13];
    const float* bias[13];
    const float* lin[5];
    int32_t mfma_dtype;
    int32_t band_rows;
    float* out;               /* [6] */
} cn_lpips_desc;

int cn_lpips_patches(int32_t mode, int32_t n, int32_t Hs, int32_t Ws, int32_t C, const float* src,
                     const float* src1, int32_t y0, int32_t rows, int32_t kpad, float* out, cn_stream_t stream);
size_t cn_lpips_head_workspace_bytes(int64_t P);
int cn_lpips_head(int32_t C, int64_t P, const float* fx, const float* fy, const float* lin, float* out,
                  void* workspace, int64_t workspace_bytes, cn_stream_t stream);
size_t cn_lpips_workspace_bytes(int32_t H, int32_t W, int32_t band_rows, int32_t mfma_dtype);
int cn_lpips(const cn_lpips_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

/* ------------------------------------------------------------------------ *
 * The flow-RGB term of stage 1 (ABI v21): the flow projection of train.py:484-495 from
 * the per-ray sums of cn_stage1_fwd, warp_pixel (train.py:235-244) and the masked L1 of
 * train.py:506-515 for T reference frames, one launch and one fixed-order reduction each
 * way instead of a chain of torch ops and a copy of T frames out of the image stack.
 *   ray_acc [R][4]    (sum_s w p, sum_s w) per ray (cn_stage1_fwd's), 16-byte aligned;
 *   w2c [T][4][4]     the relative poses (row 3 is not read);
 *   KS [T][3][3]      scale_mat[:3,:3] ref_camera_mat[t][:3,:3];
 *   pixn, pix [R][2]  the rays' normalised and pixel coordinates (x, y); rgb_gt [R][3];
 *   images [N][3][H][W] planar; frame [T]: int64 indices into the stack, read on the
 *     device (a captured launch follows their current values);
 *   frame_valid [T]: NULL, or one byte per frame (0: masked).
 * Per frame t and ray r, all fp32 without contraction:
 *   wp = w2c[t][:3,:3] pbar + wbar w2c[t][:3,3],  q = KS[t] wp,  n = (q0, q1) / q2
 *   corr  = pix + (n - pixn) * (W/2, H/2)
 *   valid = 0 <= corr.x < W and 0 <= corr.y < H
 *   warp  = the bilinear sample of images[frame[t]] at corr, border padding,
 *           align_corners=True (sampled at corr itself: the reference normalises to
 *           [-1, 1] and grid_sample un-normalises, which differs by rounding)
 *   sums [T][2] = (sum over valid rays and the 3 channels of |warp - rgb_gt|, the number
 *                  of valid rays)
 * A frame with frame_valid[t] = 0 or an index outside [0, N) is never read and gives
 * exact zeros (sums, d_w2c[t], its share of d_ray_acc).  A ray whose correspondence is
 * not finite (q2 = 0, a NaN input) fails every comparison of the mask and counts as
 * invalid; torch's composition would carry the NaN into the sum instead.
 * cn_flow_rgb_bwd: g_num [T] (device) = d loss / d sums[t][0];
 *   d_ray_acc [R][4] (16-byte aligned) = sum over t = 0 .. T-1, in that order, of the
 *     ray's gradient; d_w2c [T][12] = row-major d / d w2c[t][:3,:].
 *   sign(warp - gt) with sign(0) = 0, the bilinear derivative zero where the coordinate
 *   was clamped (torch's border rule), the quotient rule, KS^T, then w2c^T / the outer
 *   product with (pbar, wbar).  No gradient through the mask, KS, pix, pixn, rgb_gt or
 *   the images.  The backward recomputes the projection and re-reads the taps.
 * Reduction: one partial per 64 rays and frame, summed in a fixed order; no atomics.
 * Bitwise reproducible; a frame's sums and d_w2c do not depend on the other frames.
 * The valid counts are exact.  Frame base offsets are 64-bit.
 * T outside 1 .. 8, R < 0, N < 1, H or W < 1, 3 H W >= 2^31, a workspace that is NULL or
 * too small: CN_ERR_SHAPE (cn_flow_rgb_workspace_bytes: 0 for the first two).  Workspace
 * (256-byte aligned): ceil(max(R, 1) / 64) T x 48 bytes, rounded up to 256, for either
 * call.  R = 0: the ray arrays may be NULL, nothing reads them, the sums / d_w2c are
 * written as zeros.
 * ------------------------------------------------------------------------ */
size_t cn_flow_rgb_workspace_bytes(int32_t R, int32_t T);
int cn_flow_rgb_fwd(int32_t R, int32_t T, int32_t N, int32_t H, int32_t W, const float* ray_acc, const float* w2c,
                    const float* KS, const float* pixn, const float* pix, const float* rgb_gt, const float* images,
                    const int64_t* frame, const uint8_t* frame_valid, float* sums, void* workspace,
                    int64_t workspace_bytes, cn_stream_t stream);
int cn_flow_rgb_bwd(int32_t R, int32_t T, int32_t N, int32_t H, int32_t W, const float* ray_acc, const float* w2c,
                    const float* KS, const float* pixn, const float* pix, const float* rgb_gt, const float* images,
                    const int64_t* frame, const uint8_t* frame_valid, const float* g_num, float* d_ray_acc,
                    float* d_w2c, void* workspace, int64_t workspace_bytes, cn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* COPENERF_H_ */
