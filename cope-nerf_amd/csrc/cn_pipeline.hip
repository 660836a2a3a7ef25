// cn_pipeline.hip — composed entry points (ABI v12 - v14): the sampler's SDF query and the whole sampler
// of NeuSRenderer.render (v12), the no-gradient rendering forward (v13), the SDF query under autograd and the
// training render with its backward (v14), each as single C calls over the kernels of this library.
//
// Reference: neus_renderer.py:466-525 (coarse z, up_sample rounds, cat_z_vals with the new samples' SDF),
// 307-450 (render_core) and neus_fields.py:268-303 (SDFNetwork.forward / .sdf / .gradient), 352-373
// (RenderingNetwork), train.py:502-505 (the stage-1 re-query).  Each composition follows copenerf's Python
// composition (fields.sdf_forward / sdf_backward / sdf_input_grad, renderer.sample_z, the autograd Functions
// of renderer.py and fields.py) launch for launch, so the results are the same bits; host code only plans
// buffers in the caller's workspace and fills descriptors -- nothing synchronises, allocates or touches the
// default stream, so a caller may capture any of these calls in a hipGraph.
#include <algorithm>
#include <cmath>

#include "cn_common.h"

namespace {

constexpr size_t kAlign = 256;

size_t rup_sz(size_t v, size_t a) { return (v + a - 1) / a * a; }
int rup_i(int v, int a) { return (v + a - 1) / a * a; }

// A bump planner over the caller's workspace: the same walk sizes it (base == nullptr) and
// hands out the pieces.
struct Plan {
    char* base;
    size_t used = 0;
    explicit Plan(void* b) : base(static_cast<char*>(b)) {}
    void* take(size_t bytes) {
        void* p = base ? base + used : nullptr;
        used += rup_sz(bytes, kAlign);
        return p;
    }
};

// The network's buffer geometry (copenerf.fields.SDFNetwork.layout / SDFLayout).
struct NetShape {
    int L8, E, KE, HL, sk;
    bool bf, x6, img, fuse_head, fused;
};

int net_shape(const cn_sdf_net* n, NetShape* s) {
    CN_REQUIRE(n, CN_ERR_ARG, "cn_sdf_net: null");
    CN_REQUIRE(n->n_lin >= 2 && n->n_lin <= CN_SDF_MAX_LIN, CN_ERR_SHAPE, "cn_sdf_net: n_lin %d (2 .. %d)", n->n_lin,
               CN_SDF_MAX_LIN);
    CN_REQUIRE(n->mfma_dtype >= CN_MFMA_F32 && n->mfma_dtype <= CN_MFMA_F32_BF16X6, CN_ERR_ARG,
               "cn_sdf_net: mfma_dtype %d", n->mfma_dtype);
    CN_REQUIRE(n->multires >= 0 && n->multires <= 12, CN_ERR_SHAPE, "cn_sdf_net: multires %d", n->multires);
    const int L8 = n->n_lin - 1;
    s->L8 = L8;
    s->E = 4 * (1 + 2 * n->multires);
    s->KE = rup_i(s->E, 64);
    s->sk = n->skip;
    CN_REQUIRE(s->sk == -1 || (s->sk >= 1 && s->sk <= L8), CN_ERR_SHAPE, "cn_sdf_net: skip %d", s->sk);
    int hl = 0;
    for (int l = 0; l <= L8; ++l) {
        CN_REQUIRE(n->in_dim[l] >= 1 && n->out_dim[l] >= 1, CN_ERR_SHAPE, "cn_sdf_net: layer %d dims", l);
        if (l >= 1) hl = n->in_dim[l] > hl ? n->in_dim[l] : hl;
        if (l < L8) hl = n->out_dim[l] > hl ? n->out_dim[l] : hl;
    }
    s->HL = rup_i(hl, 128);
    CN_REQUIRE(n->in_dim[0] == s->E, CN_ERR_SHAPE, "cn_sdf_net: lin0 takes %d inputs, the encoding has %d",
               n->in_dim[0], s->E);
    for (int l = 1; l <= L8; ++l) {
        const int want = n->out_dim[l - 1] + (l == s->sk ? s->E : 0);
        CN_REQUIRE(n->in_dim[l] == want, CN_ERR_SHAPE, "cn_sdf_net: lin%d takes %d inputs, expected %d", l,
                   n->in_dim[l], want);
    }
    s->x6 = n->mfma_dtype == CN_MFMA_F32_BF16X6;
    s->bf = n->mfma_dtype == CN_MFMA_BF16;
    const int kq = s->bf ? 64 : 32;
    for (int l = 0; l < L8; ++l) {
        const int kp = l == 0 ? s->KE : rup_i(n->in_dim[l], kq);
        CN_REQUIRE(n->W[l] && n->bias[l], CN_ERR_ARG, "cn_sdf_net: layer %d weights / bias null", l);
        CN_REQUIRE(((uintptr_t)n->bias[l] & 15) == 0 && ((uintptr_t)n->W[l] & 15) == 0, CN_ERR_ALIGN,
                   "cn_sdf_net: layer %d weights / bias not 16-byte aligned", l);
        CN_REQUIRE(n->w_rows[l] >= rup_i(n->out_dim[l], 128) && n->w_cols[l] >= kp && n->w_cols[l] % kq == 0,
                   CN_ERR_SHAPE, "cn_sdf_net: layer %d image [%d][%d] too small for %d x %d", l, n->w_rows[l],
                   n->w_cols[l], n->out_dim[l], kp);
    }
    CN_REQUIRE(n->head_w && n->head_b, CN_ERR_ARG, "cn_sdf_net: head null");
    CN_REQUIRE(((uintptr_t)n->head_w & 15) == 0, CN_ERR_ALIGN, "cn_sdf_net: head_w not 16-byte aligned");
    // bf16 operand images for the hidden activations (fields._img_mode)
    s->img = s->bf && s->HL % 256 == 0;
    // the sdf head in the last hidden layer's epilogue (fields._fuse_head)
    {
        const int N = n->out_dim[L8 - 1];
        const bool shape_ok = n->in_dim[L8] == N && N % 4 == 0 && L8 != s->sk && L8 - 1 != 0;
        s->fuse_head = shape_ok && (N <= 128 ||
                                    (s->x6 && N <= 256 && n->w_rows[L8 - 1] >= 256 &&
                                     rup_i(n->in_dim[L8 - 1], 32) % 64 == 0) ||
                                    (s->bf && N <= 256 && n->w_rows[L8 - 1] >= 256));
    }
    // cn_sdf_mlp's shape (fields._fused_query_ok)
    // (bf16 images, or the bf16x6 mode's fp32 inputs and term images: sdf_mlp_x6_kernel, ABI v15)
    bool f = !(n->flags & CN_SDF_LAYERED) && (s->img || s->x6) && n->n_lin == 9 && s->HL == 256 && s->KE == 64 &&
             s->sk >= 2 && s->sk <= 7;
    if (f) f = s->E + n->out_dim[s->sk - 1] == 256 && n->in_dim[8] == 256;
    for (int l = 0; f && l < 8; ++l)
        f = (l == s->sk - 1 || n->out_dim[l] == 256) && n->w_rows[l] == 256;
    s->fused = f;
    return CN_OK;
}

int sdf_query_plan(const cn_sdf_net* n, const NetShape& s, int M, const float* x, int64_t ldx, float* sdf,
                   const int32_t* idx, Plan& ws, hipStream_t st, bool run) {
    const float kSqrt2 = (float)std::sqrt(2.0);
    if (s.fused) {
        // cn_sdf_embed's bf16 images (lin0's input; the skip concat's tail / sqrt 2) -- fp32 rows in the bf16x6
        // mode -- then one cn_sdf_mlp
        const size_t esz = s.x6 ? 4 : 2;
        void* u0b = ws.take((size_t)M * 64 * esz);
        void* tail = ws.take((size_t)M * 64 * esz);
        if (!run) return CN_OK;
        int rc = cn_sdf_embed(M, x, ldx, n->multires, n->scale, 64, u0b, 64, tail, 64, kSqrt2, s.x6 ? 0 : 3, st);
        if (rc) return rc;
        cn_sdf_mlp_desc d{};
        d.u0 = u0b;
        d.tail = tail;
        d.ld_u0 = 64;
        d.ld_t = 64;
        d.M = M;
        d.n_layers = 8;
        d.hidden = 256;
        d.kpad0 = 64;
        d.multires = n->multires;
        d.skip_layer = s.sk - 1;
        for (int l = 0; l < 8; ++l) {
            d.W[l] = n->W[l];
            d.ldw[l] = s.x6 ? n->w_rows[l] : n->w_cols[l];  // (a term image's leading dimension: its rows)
            d.bias[l] = n->bias[l];
        }
        d.format = s.x6 ? CN_MFMA_F32_BF16X6 : 0;
        d.head_w = n->head_w;
        d.head_b = n->head_b;
        d.sdf = sdf;
        d.idx = idx;
        d.skip_div = kSqrt2;
        d.beta = n->beta;
        d.threshold = n->threshold;
        return cn_sdf_mlp(&d, st);
    }
    // layer by layer (fields.sdf_forward): U0 fp32 [M][KE]; the skip layer's input Usk (bf16 image in the
    // image mode, its tail written by the embedding); two ping-pong activation buffers
    const int L8 = s.L8, HL = s.HL, sk = s.sk;
    const bool usk_b = s.img && sk >= 1 && sk < L8;
    const size_t pp_elem = (s.img && s.fuse_head) ? 2 : 4;  // only bf16 images (and no stored U_8) then
    float* U0 = static_cast<float*>(ws.take((size_t)M * s.KE * 4));
    char* Usk = sk >= 0 ? static_cast<char*>(ws.take((size_t)M * HL * (usk_b ? 2 : 4))) : nullptr;
    char* pp[2] = {static_cast<char*>(ws.take((size_t)M * HL * pp_elem)),
                   static_cast<char*>(ws.take((size_t)M * HL * pp_elem))};
    if (!run) return CN_OK;
    void* e_view = nullptr;
    if (sk >= 0) e_view = Usk + (size_t)n->out_dim[sk - 1] * (usk_b ? 2 : 4);
    int rc = cn_sdf_embed(M, x, ldx, n->multires, n->scale, s.KE, U0, s.KE, e_view, e_view ? HL : 0, kSqrt2,
                          usk_b ? 1 : 0, st);
    if (rc) return rc;
    const void* A = U0;
    int64_t lda = s.KE;
    bool a_b = false;
    const void* U8 = nullptr;
    for (int l = 0; l < L8; ++l) {
        const bool into = (l + 1) == sk;
        int K = l == 0 ? s.KE : rup_i(n->in_dim[l], 32);
        if (s.bf) K = rup_i(K, 64);
        cn_linear_desc d{};
        d.A = A;
        d.lda = lda;
        d.a_bf16 = a_b ? 1 : 0;
        d.B = static_cast<const float*>(n->W[l]);
        d.ldb = s.x6 ? n->w_rows[l] : n->w_cols[l];
        d.bias = n->bias[l];
        d.M = M;
        d.N = n->out_dim[l];
        d.K = d.K1 = K;
        d.nsplit = d.N;
        d.adiv = 1.0f;
        d.odiv = 1.0f;
        d.beta = n->beta;
        d.threshold = n->threshold;
        d.mfma_dtype = n->mfma_dtype;
        d.flags = l & 1;  // consecutive launches walk the rows in opposite directions (results do not depend on it)
        void* out = nullptr;
        void* outb = nullptr;
        if (l == L8 - 1 && s.fuse_head) {
            d.epilogue = CN_EPI_SOFTPLUS_HEAD;
            d.nzero = HL;
            d.head_w = n->head_w;
            d.head_b = n->head_b;
            d.head_out = sdf;
            d.head_idx = idx;
        } else {
            d.epilogue = CN_EPI_SOFTPLUS;
            d.nzero = into ? n->out_dim[l] : HL;
            if (into) d.odiv = kSqrt2;
            char* dst = into ? Usk : pp[l & 1];
            if (s.img && l + 1 < L8) {  // the next layer's operand image, the activation's only copy
                outb = dst;
                d.out0_b = outb;
                d.ld_out0_b = HL;
            } else {
                out = dst;
                d.out0 = static_cast<float*>(out);
                d.ld_out0 = HL;
            }
        }
        d.tile = (d.N <= 64 && d.nzero <= 64) ? 1 : 0;
        rc = cn_linear(&d, st);
        if (rc) return rc;
        A = out ? out : outb;
        a_b = outb != nullptr;
        lda = HL;
        if (l == L8 - 1) U8 = out;
    }
    if (!s.fuse_head)
        return cn_row_head(M, n->in_dim[L8], static_cast<const float*>(U8), HL, n->head_w, n->in_dim[L8],
                           n->head_b, 1, 0, sdf, 1, idx, st);
    return CN_OK;
}

int query_check(const cn_sdf_net* n, int32_t M, const float* x, int64_t ldx, float* sdf) {
    CN_REQUIRE(M >= 0, CN_ERR_SHAPE, "cn_sdf_query: M = %d", M);
    CN_REQUIRE(M == 0 || (x && sdf), CN_ERR_ARG, "cn_sdf_query: null x / sdf");
    CN_REQUIRE(ldx >= 4, CN_ERR_SHAPE, "cn_sdf_query: ldx %lld < 4", (long long)ldx);
    (void)n;
    return CN_OK;
}

// The sampler's buffers: two ping-pong z / sdf rows of the final width, the points of the widest
// query, the new samples and their scatter targets, then the query's own workspace (reused by
// every round: the stream orders them).
struct SamplePlan {
    float* jitter;  // the device-drawn t_rand (philox), or null
    float *z[2], *sdf[2], *pts, *z_new;
    int32_t* dst;
    int k, width, qmax;
};

bool sample_draws(const cn_sample_desc* d) { return !d->t_rand && d->philox; }

int sample_plan(const cn_sample_desc* d, const NetShape& s, Plan& ws, SamplePlan* p) {
    const int R = d->R, ns = d->n_samples;
    p->jitter = sample_draws(d) ? static_cast<float*>(ws.take((size_t)R * ns * 4)) : nullptr;
    p->k = d->n_importance > 0 ? d->n_importance / d->up_sample_steps : 0;
    p->width = ns + d->up_sample_steps * p->k;
    p->qmax = ns > p->k ? ns : p->k;
    const size_t rows = (size_t)R * p->width;
    for (int i = 0; i < 2; ++i) {
        p->z[i] = static_cast<float*>(ws.take(rows * 4));
        p->sdf[i] = static_cast<float*>(ws.take(rows * 4));
    }
    p->pts = static_cast<float*>(ws.take((size_t)R * p->qmax * 16));
    p->z_new = static_cast<float*>(ws.take((size_t)R * (p->k > 0 ? p->k : 1) * 4));
    p->dst = static_cast<int32_t*>(ws.take((size_t)R * (p->k > 0 ? p->k : 1) * 4));
    (void)s;
    return CN_OK;
}

int sample_check(const cn_sample_desc* d) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_sample: null descriptor");
    CN_REQUIRE(d->R >= 0 && d->n_samples >= 1 && d->n_importance >= 0, CN_ERR_SHAPE,
               "cn_sample: R %d n_samples %d n_importance %d", d->R, d->n_samples, d->n_importance);
    CN_REQUIRE(d->n_importance == 0 || (d->up_sample_steps >= 1 && d->n_importance >= d->up_sample_steps),
               CN_ERR_SHAPE, "cn_sample: n_importance %d over %d up-sample steps", d->n_importance, d->up_sample_steps);
    CN_REQUIRE(d->near && d->far && d->z, CN_ERR_ARG, "cn_sample: null near / far / z");
    CN_REQUIRE(d->n_importance == 0 || (d->rays_o && d->rays_d && d->time_step && d->net), CN_ERR_ARG,
               "cn_sample: null rays / time_step / net");
    CN_REQUIRE((int64_t)d->R * ((int64_t)d->n_samples + d->n_importance) < ((int64_t)1 << 31), CN_ERR_SHAPE,
               "cn_sample: R = %d too large", d->R);
    return CN_OK;
}

}  // namespace

extern "C" size_t cn_sdf_query_workspace_bytes(const cn_sdf_net* net, int32_t M) {
    NetShape s;
    if (M < 0 || net_shape(net, &s) != CN_OK) return 0;
    Plan ws(nullptr);
    sdf_query_plan(net, s, M, nullptr, 4, nullptr, nullptr, ws, nullptr, false);
    return ws.used;
}

extern "C" int cn_sdf_query(const cn_sdf_net* net, int32_t M, const float* x, int64_t ldx, float* sdf,
                            const int32_t* idx, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    NetShape s;
    int rc = net_shape(net, &s);
    if (rc) return rc;
    if ((rc = query_check(net, M, x, ldx, sdf))) return rc;
    if (M == 0) return CN_OK;
    const size_t need = cn_sdf_query_workspace_bytes(net, M);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_sdf_query: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_sdf_query: workspace not 256-byte aligned");
    Plan ws(workspace);
    return sdf_query_plan(net, s, M, x, ldx, sdf, idx, ws, (hipStream_t)stream, true);
}

extern "C" size_t cn_sample_workspace_bytes(const cn_sample_desc* d) {
    if (sample_check(d) != CN_OK) return 0;
    if (d->n_importance == 0) return sample_draws(d) ? rup_sz((size_t)d->R * d->n_samples * 4, kAlign) : 0;
    NetShape s;
    if (net_shape(d->net, &s) != CN_OK) return 0;
    Plan ws(nullptr);
    SamplePlan p;
    sample_plan(d, s, ws, &p);
    return ws.used + cn_sdf_query_workspace_bytes(d->net, d->R * p.qmax);
}

extern "C" int cn_sample(const cn_sample_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int rc = sample_check(d);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int R = d->R, ns = d->n_samples;
    if (d->n_importance == 0) {
        const float* t_rand = d->t_rand;
        if (sample_draws(d) && R > 0) {  // the jitter drawn on the device into the workspace
            CN_REQUIRE(workspace && workspace_bytes >= (int64_t)R * ns * 4 && ((uintptr_t)workspace & (kAlign - 1)) == 0,
                       CN_ERR_SHAPE, "cn_sample: workspace for the drawn jitter");
            if ((rc = cn_uniform_philox((int64_t)R * ns, d->philox, static_cast<float*>(workspace), stream))) return rc;
            t_rand = static_cast<const float*>(workspace);
        }
        return cn_coarse_z(R, ns, d->near, d->far, t_rand, d->z, stream);
    }
    NetShape s;
    if ((rc = net_shape(d->net, &s))) return rc;
    if (R == 0) return CN_OK;
    const size_t need = cn_sample_workspace_bytes(d);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_sample: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_sample: workspace not 256-byte aligned");
    Plan ws(workspace);
    SamplePlan p;
    sample_plan(d, s, ws, &p);
    char* qws = ws.base + ws.used;
    const int64_t qbytes = workspace_bytes - (int64_t)ws.used;
    // coarse samples and their SDF (neus_renderer.py:466-498)
    float* z = p.z[0];
    float* sdf = p.sdf[0];
    const float* t_rand = d->t_rand;
    if (p.jitter) {
        if ((rc = cn_uniform_philox((int64_t)R * ns, d->philox, p.jitter, stream))) return rc;
        t_rand = p.jitter;
    }
    if ((rc = cn_coarse_z(R, ns, d->near, d->far, t_rand, z, stream))) return rc;
    if ((rc = cn_points(R, ns, d->rays_o, d->rays_d, z, d->time_step, 0, nullptr, nullptr, 0, p.pts, stream)))
        return rc;
    if ((rc = cn_sdf_query(d->net, R * ns, p.pts, 4, sdf, nullptr, qws, qbytes, stream))) return rc;
    // up_sample + cat_z_vals rounds (neus_renderer.py:500-520)
    int n = ns;
    for (int i = 0; i < d->up_sample_steps; ++i) {
        const bool last = i + 1 == d->up_sample_steps;
        float* z_out = last ? d->z : p.z[(i + 1) & 1];
        float* sdf_out = last ? nullptr : p.sdf[(i + 1) & 1];
        const float inv_s = 64.0f * (float)(1 << i);
        if ((rc = cn_up_sample_merge(R, n, p.k, inv_s, z, sdf, z_out, p.z_new, sdf_out, last ? nullptr : p.dst, stream)))
            return rc;
        if (!last) {
            if ((rc = cn_points(R, p.k, d->rays_o, d->rays_d, p.z_new, d->time_step, 0, nullptr, nullptr, 0, p.pts,
                                stream)))
                return rc;
            if ((rc = cn_sdf_query(d->net, R * p.k, p.pts, 4, sdf_out, p.dst, qws, qbytes, stream))) return rc;
        }
        z = z_out;
        sdf = sdf_out;
        n += p.k;
    }
    (void)st;
    return CN_OK;
}

// ---------------------------------------------------------------------------------------------
// cn_render_fwd: NeuSRenderer.forward without gradient (neus_renderer.py:453-584, render_core
// 307-450) composed from the launches copenerf's renderer makes in eval mode with the folded
// feature head: cn_sample, cn_points (midpoints), the SDF field (fields.sdf_forward with
// want_feat "hidden", want_grad, keep False), the colour field (_ColorFieldFn.forward) and
// cn_composite_fwd -- descriptor for descriptor, so the same bits.
namespace {

struct ColorShape {
    int KX, HL;
    bool bf, x6, img;
};

int color_shape(const cn_color_net* c, ColorShape* s) {
    CN_REQUIRE(c, CN_ERR_ARG, "cn_color_net: null");
    CN_REQUIRE(c->n_lin >= 2 && c->n_lin <= CN_SDF_MAX_LIN, CN_ERR_SHAPE, "cn_color_net: n_lin %d", c->n_lin);
    CN_REQUIRE(c->mfma_dtype >= CN_MFMA_F32 && c->mfma_dtype <= CN_MFMA_F32_BF16X6, CN_ERR_ARG, "cn_color_net: mfma_dtype");
    CN_REQUIRE(c->multires_view >= 0 && c->multires_view <= 12 && c->d_feature % 32 == 0 && c->d_feature > 0,
               CN_ERR_SHAPE, "cn_color_net: multires_view %d / d_feature %d", c->multires_view, c->d_feature);
    const int n = c->n_lin;
    s->KX = rup_i(4 + 4 + 3 * (1 + 2 * c->multires_view), 64);
    CN_REQUIRE(c->out_dim[n - 1] == 3 && c->in_dim[0] == 4 + 3 * (1 + 2 * c->multires_view) + 4 + c->d_feature,
               CN_ERR_SHAPE, "cn_color_net: lin0 takes %d inputs, the head gives %d", c->in_dim[0], c->out_dim[n - 1]);
    int hl = 0;
    for (int l = 0; l < n - 1; ++l) hl = c->out_dim[l] > hl ? c->out_dim[l] : hl;
    for (int l = 1; l < n; ++l)
        CN_REQUIRE(c->in_dim[l] == c->out_dim[l - 1], CN_ERR_SHAPE, "cn_color_net: lin%d widths", l);
    s->HL = rup_i(hl, 128);
    s->x6 = c->mfma_dtype == CN_MFMA_F32_BF16X6;
    s->bf = c->mfma_dtype == CN_MFMA_BF16;
    s->img = s->bf && s->HL % 256 == 0;
    const int kq = s->bf ? 64 : 32;
    for (int l = 0; l < n - 1; ++l) {
        const int kp = l == 0 ? c->d_feature + s->KX : rup_i(c->in_dim[l], kq);
        CN_REQUIRE(c->W[l] && c->bias[l] && ((uintptr_t)c->W[l] & 15) == 0 && ((uintptr_t)c->bias[l] & 15) == 0,
                   CN_ERR_ALIGN, "cn_color_net: layer %d weights / bias null or not 16-byte aligned", l);
        CN_REQUIRE(c->w_rows[l] >= rup_i(c->out_dim[l], 128) && c->w_cols[l] >= kp, CN_ERR_SHAPE,
                   "cn_color_net: layer %d image [%d][%d] too small", l, c->w_rows[l], c->w_cols[l]);
    }
    CN_REQUIRE(c->head_w && c->head_b, CN_ERR_ARG, "cn_color_net: head null");
    return CN_OK;
}

// copenerf.ops.linear's descriptor for these arguments (K rounded to 64 in the bf16 mode, the tile by
// the widths, ldb by the image format)
struct LinCall {
    const void* A = nullptr;
    bool a_b = false;
    int64_t lda = 0;
    const void* A2 = nullptr;
    int64_t lda2 = 0;
    int K1 = -1;
    const void* B = nullptr;
    int b_rows = 0, b_cols = 0;
    int N = 0, K = 0, nzero = -1, nsplit = -1, epi = CN_EPI_STORE;
    const float* bias = nullptr;
    const float* colv = nullptr;
    const void* aux0 = nullptr;
    bool aux0_b = false;
    int64_t ld_aux0 = 0;
    const void* aux1 = nullptr;  // BWD_SOFTPLUS's second-order operands (fp32, or images with aux12_b)
    const void* aux2 = nullptr;
    int64_t ld_aux1 = 0, ld_aux2 = 0;
    float aux2_scale = 0.0f;
    bool aux12_b = false;
    float aux_beta = 0.0f, adiv = 1.0f, odiv = 1.0f, beta = 100.0f, threshold = 20.0f;
    float* out0 = nullptr;
    int64_t ld_out0 = 0;
    void* out0_b = nullptr;
    int64_t ld_out0_b = 0;
    float* out1 = nullptr;
    int64_t ld_out1 = 0;
    void* out1_b = nullptr;
    int64_t ld_out1_b = 0;
    float* out_split = nullptr;
    int64_t ld_split = 0;
    const float* head_w = nullptr;
    const float* head_b = nullptr;
    float* head_out = nullptr;
    int M = 0;
};

int run_linear(int mode, const LinCall& c, int flip, hipStream_t st) {
    const bool x6 = mode == CN_MFMA_F32_BF16X6, bf = mode == CN_MFMA_BF16;
    cn_linear_desc d{};
    int K = c.K, K1 = c.K1 < 0 ? -1 : c.K1;
    if (bf) {
        K = rup_i(K, 64);
        if (K1 >= 0) K1 = rup_i(K1, 64);
    }
    d.A = c.A;
    d.A2 = c.A2;
    d.B = static_cast<const float*>(c.B);
    d.bias = c.bias;
    d.colv = c.colv;
    d.aux0 = c.aux0;
    d.aux1 = static_cast<const float*>(c.aux1);
    d.aux2 = static_cast<const float*>(c.aux2);
    d.ld_aux1 = c.ld_aux1;
    d.ld_aux2 = c.ld_aux2;
    d.aux2_scale = c.aux2_scale;
    d.aux12_bf16 = c.aux12_b ? 1 : 0;
    d.out0 = c.out0;
    d.out1 = c.out1;
    d.out_split = c.out_split;
    d.head_w = c.head_w;
    d.head_b = c.head_b;
    d.head_out = c.head_out;
    d.aux_beta = c.aux_beta;
    d.lda = c.lda;
    d.lda2 = c.lda2;
    d.ldb = x6 ? c.b_rows : c.b_cols;
    d.ld_aux0 = c.ld_aux0;
    d.ld_out0 = c.ld_out0;
    d.ld_out1 = c.ld_out1;
    d.ld_split = c.ld_split;
    d.M = c.M;
    d.N = c.N;
    d.K = K;
    d.K1 = K1 >= 0 ? K1 : K;
    d.nzero = c.nzero >= 0 ? c.nzero : c.N;
    d.nsplit = c.nsplit >= 0 ? c.nsplit : c.N;
    d.epilogue = c.epi;
    const int nz = c.nzero >= 0 ? c.nzero : 0;
    d.tile = (c.N > nz ? c.N : nz) <= 64 ? 1 : 0;
    d.adiv = c.adiv;
    d.odiv = c.odiv;
    d.beta = c.beta;
    d.threshold = c.threshold;
    d.mfma_dtype = mode;
    d.a_bf16 = c.a_b ? 1 : 0;
    d.aux0_bf16 = c.aux0_b ? 1 : 0;
    d.out0_b = c.out0_b;
    d.ld_out0_b = c.ld_out0_b;
    d.out1_b = c.out1_b;
    d.ld_out1_b = c.ld_out1_b;
    d.flags = flip & 1;
    return cn_linear(&d, st);
}

// softplus' σ_l's aux_beta as fields.sig_beta computes it (in double, then to float)
float sig_beta(const cn_sdf_net* n, int l) {
    return (float)((double)n->beta * ((l + 1) == n->skip ? std::sqrt(2.0) : 1.0));
}

// What the training forward keeps for the backward (fields.sdf_forward keep=True): the activations U_l (bf16
// images where ub[l]) and the ∇ pass's adjoints s_l (fp32 S[l] and / or the image Sb[l]).
struct SdfKeep {
    float* U0;
    char* U[CN_SDF_MAX_LIN];
    bool ub[CN_SDF_MAX_LIN];
    float* S[CN_SDF_MAX_LIN];
    void* Sb[CN_SDF_MAX_LIN];
    bool sf[CN_SDF_MAX_LIN];   // S[l] kept (the pointers are null in a sizing pass: these say what exists)
    bool sbf[CN_SDF_MAX_LIN];  // Sb[l] kept
};

// The SDF field with its ∇ₓSDF pass (fields.sdf_forward, want_feat "hidden", want_grad; keep False, or True
// with `keep` != nullptr: every s_l in its own buffer, recorded there): sdf [M], U8 (the last hidden
// activation, fp32 [M][HL]: the colour network's operand) and G [M][4].
int sdf_field_plan(const cn_sdf_net* n, const NetShape& s, int M, const float* x, float* sdf, float** U8_out,
                   float* G, Plan& ws, hipStream_t st, bool run, SdfKeep* keep = nullptr) {
    const float kSqrt2 = (float)std::sqrt(2.0);
    const int L8 = s.L8, HL = s.HL, sk = s.sk, KE = s.KE;
    const size_t eh = s.img ? 2 : 4;  // the hidden activations' element size (bf16 images in the image mode)
    const bool usk_b = s.img && sk >= 1 && sk < L8;
    float* U0 = static_cast<float*>(ws.take((size_t)M * KE * 4));
    // U[1 .. L8]: every activation is kept (σ's source in the ∇ pass); U[sk] is the skip input
    char* U[CN_SDF_MAX_LIN] = {};
    bool ub[CN_SDF_MAX_LIN] = {};
    for (int l = 1; l <= L8; ++l) {
        ub[l] = (l == sk) ? usk_b : (s.img && l < L8);
        U[l] = static_cast<char*>(ws.take((size_t)M * HL * (ub[l] ? 2 : 4)));
    }
    const bool fp32_s7 = !s.img;  // the image mode with the folded head keeps s_7 as its image only
    // (fp32 s_7 also from cn_scale_cols where the head is not fused)
    float* S7 = (fp32_s7 || !s.fuse_head) ? static_cast<float*>(ws.take((size_t)M * HL * 4)) : nullptr;
    void* S7b = s.img ? ws.take((size_t)M * HL * 2) : nullptr;
    // the ∇ pass: two ping-pong adjoints (images in the image mode), s_0 also fp32, QE, Q0; kept: s_0 .. s_{L8-2}
    // each in its own buffer (fp32 where not the image mode or l = 0, the image in the image mode)
    char* Sp[2] = {nullptr, nullptr};
    float* S0 = nullptr;
    float* Sk[CN_SDF_MAX_LIN] = {};
    void* Sbk[CN_SDF_MAX_LIN] = {};
    if (keep) {
        for (int l = 0; l + 1 < L8; ++l) {
            Sbk[l] = s.img ? ws.take((size_t)M * HL * 2) : nullptr;
            Sk[l] = (!s.img || l == 0) ? static_cast<float*>(ws.take((size_t)M * HL * 4)) : nullptr;
        }
        S0 = Sk[0];
    } else {
        Sp[0] = static_cast<char*>(ws.take((size_t)M * HL * eh));
        Sp[1] = static_cast<char*>(ws.take((size_t)M * HL * eh));
        S0 = static_cast<float*>(ws.take((size_t)M * HL * 4));
    }
    float* QE = sk >= 0 ? static_cast<float*>(ws.take((size_t)M * KE * 4)) : nullptr;
    float* Q0 = static_cast<float*>(ws.take((size_t)M * KE * 4));
    if (keep) {  // (fields.sdf_forward keep: st["U"], st["Ub"], st["S"], st["Sb"])
        keep->U0 = U0;
        keep->U[0] = nullptr;
        keep->ub[0] = false;
        for (int l = 1; l <= L8; ++l) {
            keep->U[l] = U[l];
            keep->ub[l] = ub[l];
        }
        for (int l = 0; l + 1 < L8; ++l) {
            keep->S[l] = Sk[l];
            keep->sf[l] = !s.img || l == 0;
            keep->Sb[l] = Sbk[l];
            keep->sbf[l] = s.img;
        }
        // s_7: fp32 from the head epilogue (not the image mode) or cn_scale_cols (no fused head); its image
        // from the head epilogue in the image mode
        keep->S[L8 - 1] = S7;
        keep->sf[L8 - 1] = fp32_s7 || !s.fuse_head;
        keep->Sb[L8 - 1] = (s.img && s.fuse_head) ? S7b : nullptr;
        keep->sbf[L8 - 1] = s.img && s.fuse_head;
    }
    if (!run) return CN_OK;
    void* e_view = nullptr;
    if (sk >= 0) e_view = U[sk] + (size_t)n->out_dim[sk - 1] * (usk_b ? 2 : 4);
    int rc = cn_sdf_embed(M, x, 4, n->multires, n->scale, KE, U0, KE, e_view, e_view ? HL : 0, kSqrt2, usk_b ? 1 : 0, st);
    if (rc) return rc;
    int flip = 0;
    bool have_s7 = false, have_s7b = false;
    for (int l = 0; l < L8; ++l) {
        const bool into = (l + 1) == sk;
        LinCall c;
        c.A = l == 0 ? static_cast<const void*>(U0) : U[l];
        c.a_b = l > 0 && ub[l];
        c.lda = l == 0 ? KE : HL;
        c.B = n->W[l];
        c.b_rows = n->w_rows[l];
        c.b_cols = n->w_cols[l];
        c.N = n->out_dim[l];
        c.K = l == 0 ? KE : rup_i(n->in_dim[l], 32);
        c.bias = n->bias[l];
        c.beta = n->beta;
        c.threshold = n->threshold;
        c.M = M;
        if (l == L8 - 1 && s.fuse_head) {
            c.epi = CN_EPI_SOFTPLUS_HEAD;
            c.out0 = reinterpret_cast<float*>(U[L8]);
            c.ld_out0 = HL;
            c.nzero = HL;
            if (fp32_s7) {
                c.out1 = S7;
                c.ld_out1 = HL;
                have_s7 = true;
            }
            if (S7b) {
                c.out1_b = S7b;
                c.ld_out1_b = HL;
                have_s7b = true;
            }
            c.colv = n->head_wp;
            c.aux_beta = sig_beta(n, l);
            c.head_w = n->head_w;
            c.head_b = n->head_b;
            c.head_out = sdf;
        } else {
            c.epi = CN_EPI_SOFTPLUS;
            c.nzero = into ? n->out_dim[l] : HL;
            if (into) c.odiv = kSqrt2;
            if (ub[l + 1]) {
                c.out0_b = U[l + 1];
                c.ld_out0_b = HL;
            } else {
                c.out0 = reinterpret_cast<float*>(U[l + 1]);
                c.ld_out0 = HL;
            }
        }
        if ((rc = run_linear(n->mfma_dtype, c, flip++, st))) return rc;
    }
    float* U8 = reinterpret_cast<float*>(U[L8]);
    *U8_out = U8;
    if (!s.fuse_head &&
        (rc = cn_row_head(M, n->in_dim[L8], U8, HL, n->head_w, n->in_dim[L8], n->head_b, 1, 0, sdf, 1, nullptr, st)))
        return rc;
    if (!have_s7 && !have_s7b) {
        if ((rc = cn_scale_cols(M, HL, U8, HL, n->head_wp, nullptr, S7, HL, sig_beta(n, L8 - 1), st))) return rc;
        have_s7 = true;
    }
    // ∇ pass: s_{l-1} = (W_lᵀ s_l) ⊙ σ_{l-1}, l = L8-1 .. 1 (the skip layer's embedding columns to QE)
    const void* A = have_s7b ? S7b : static_cast<const void*>(S7);
    bool a_b = have_s7b;
    for (int l = L8 - 1; l >= 1; --l) {
        LinCall c;
        c.A = A;
        c.a_b = a_b;
        c.lda = HL;
        c.B = n->Wt[l];
        c.b_rows = n->wt_rows[l];
        c.b_cols = n->wt_cols[l];
        c.K = rup_i(n->out_dim[l], 32);
        c.epi = CN_EPI_MUL;
        c.aux0 = U[l];
        c.aux0_b = ub[l];
        c.ld_aux0 = HL;
        c.aux_beta = sig_beta(n, l - 1);
        c.nzero = HL;
        c.M = M;
        c.beta = n->beta;
        c.threshold = n->threshold;
        if (l == sk) {
            c.N = n->in_dim[l];
            c.nsplit = n->out_dim[l - 1];
            c.out_split = QE;
            c.ld_split = KE;
            c.adiv = kSqrt2;
        } else {
            c.N = n->out_dim[l - 1];
        }
        char* dst = keep ? static_cast<char*>(s.img ? Sbk[l - 1] : static_cast<void*>(Sk[l - 1])) : Sp[l & 1];
        if (s.img) {
            c.out0_b = dst;
            c.ld_out0_b = HL;
            if (l - 1 == 0) {
                c.out0 = S0;
                c.ld_out0 = HL;
            }
        } else {
            c.out0 = l - 1 == 0 ? S0 : reinterpret_cast<float*>(dst);
            c.ld_out0 = HL;
        }
        if ((rc = run_linear(n->mfma_dtype, c, flip++, st))) return rc;
        A = s.img ? static_cast<const void*>(dst) : static_cast<const void*>(c.out0);
        a_b = s.img;
    }
    {  // Q0 = W_0ᵀ s_0 (the embedding's adjoint), then ∇ₓSDF
        LinCall c;
        c.A = A;
        c.a_b = a_b;
        c.lda = HL;
        c.B = n->Wt[0];
        c.b_rows = n->wt_rows[0];
        c.b_cols = n->wt_cols[0];
        c.N = s.E;
        c.K = rup_i(n->out_dim[0], 32);
        c.epi = CN_EPI_STORE;
        c.out0 = Q0;
        c.ld_out0 = KE;
        c.nzero = KE;
        c.M = M;
        c.beta = n->beta;
        c.threshold = n->threshold;
        if ((rc = run_linear(n->mfma_dtype, c, flip++, st))) return rc;
    }
    return cn_sdf_grad_assemble(M, n->multires, n->scale, U0, KE, Q0, KE, QE, QE ? KE : 0, G, 4, st);
}

// the colour network (_ColorFieldFn.forward): rgb [M][3]
// What the colour network's training forward keeps: the extras and every hidden activation (bf16 images
// where the image mode stores images only).
struct ColorKeep {
    float* ext;
    char* H[CN_SDF_MAX_LIN];
    bool hb[CN_SDF_MAX_LIN];
};

int color_field_plan(const cn_color_net* c, const ColorShape& s, int M, const float* G, const float* pts,
                     const float* dirs, int dir_div, const float* feat, int64_t ld_feat, float* rgb, Plan& ws,
                     hipStream_t st, bool run, ColorKeep* keep = nullptr) {
    const int n = c->n_lin, HL = s.HL;
    float* ext = static_cast<float*>(ws.take((size_t)M * s.KX * 4));
    char* H[2] = {nullptr, nullptr};
    char* Hk[CN_SDF_MAX_LIN] = {};
    if (keep) {
        keep->ext = ext;
        for (int l = 0; l < n - 1; ++l) {
            keep->hb[l] = s.img && l < n - 2;
            Hk[l] = keep->H[l] = static_cast<char*>(ws.take((size_t)M * HL * (keep->hb[l] ? 2 : 4)));
        }
    } else {
        H[0] = static_cast<char*>(ws.take((size_t)M * HL * 4));
        H[1] = static_cast<char*>(ws.take((size_t)M * HL * 4));
    }
    if (!run) return CN_OK;
    int rc = cn_color_extras(M, G, 4, pts, 4, dirs, 3, dir_div, c->multires_view, s.KX, ext, s.KX, st);
    if (rc) return rc;
    const void* A = feat;
    bool a_b = false;
    int64_t lda = ld_feat;
    const float* last = nullptr;
    for (int l = 0; l < n - 1; ++l) {
        LinCall k;
        k.A = A;
        k.a_b = a_b;
        k.lda = lda;
        if (l == 0) {
            k.A2 = ext;
            k.lda2 = s.KX;
            k.K1 = c->d_feature;
            k.K = c->d_feature + s.KX;
        } else {
            k.K = rup_i(c->out_dim[l - 1], 32);
        }
        k.B = c->W[l];
        k.b_rows = c->w_rows[l];
        k.b_cols = c->w_cols[l];
        k.N = c->out_dim[l];
        k.epi = CN_EPI_RELU;
        k.bias = c->bias[l];
        k.nzero = HL;
        k.M = M;
        char* dst = keep ? Hk[l] : H[l & 1];
        const bool img = s.img && l < n - 2;  // the next layer's operand image, the activation's only copy
        if (img) {
            k.out0_b = dst;
            k.ld_out0_b = HL;
        } else {
            k.out0 = reinterpret_cast<float*>(dst);
            k.ld_out0 = HL;
        }
        if ((rc = run_linear(c->mfma_dtype, k, l, st))) return rc;
        A = dst;
        a_b = img;
        lda = HL;
        last = reinterpret_cast<const float*>(dst);
    }
    return cn_row_head(M, c->in_dim[n - 1], last, HL, c->head_w, c->in_dim[n - 1], c->head_b, 3, 1, rgb, 3, nullptr, st);
}

// What the field part of the rendering forward (sdf_field_plan + color_field_plan) asks of the two networks
int fold_check(const char* who, const cn_sdf_net* n, const cn_color_net* c, NetShape* s, ColorShape* cs) {
    int rc = net_shape(n, s);
    if (rc) return rc;
    if ((rc = color_shape(c, cs))) return rc;
    CN_REQUIRE(n->mfma_dtype == c->mfma_dtype, CN_ERR_ARG, "%s: the networks' GEMM modes differ", who);
    // the folded feature head (copenerf.renderer's fold): the colour network reads the SDF's last hidden layer
    CN_REQUIRE(n->in_dim[s->L8] == s->HL && s->HL == c->d_feature && n->out_dim[s->L8] == 1 + c->d_feature,
               CN_ERR_UNSUPPORTED, "%s: needs the folded feature head (SDF hidden width == d_feature)", who);
    for (int l = 0; l < s->L8; ++l) {
        const int kq = s->bf ? 64 : 32;
        CN_REQUIRE(n->Wt[l] && ((uintptr_t)n->Wt[l] & 15) == 0 && n->wt_rows[l] >= rup_i(n->in_dim[l], 128) &&
                       n->wt_cols[l] >= rup_i(n->out_dim[l], kq),
                   CN_ERR_SHAPE, "%s: transposed image %d missing or too small", who, l);
    }
    CN_REQUIRE(n->head_wp && ((uintptr_t)n->head_wp & 15) == 0, CN_ERR_ALIGN, "%s: head_wp [HL] (16-byte aligned)", who);
    return CN_OK;
}

int render_check(const cn_render_desc* d, NetShape* s, ColorShape* cs, bool train = false) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_render_fwd: null descriptor");
    int rc = fold_check("cn_render_fwd", d->sdf_net, d->color_net, s, cs);
    if (rc) return rc;
    CN_REQUIRE(d->R >= 0 && d->rays_o && d->rays_d && d->near && d->far && d->time_step && d->inv_s &&
                   d->cos_anneal_ratio,
               CN_ERR_ARG, "cn_render_fwd: null input");
    CN_REQUIRE((train || (d->z && d->rgb)) && d->pts && d->sdf && d->grad && d->color && d->depth && d->weights &&
                   d->cdf,
               CN_ERR_ARG, "cn_render_fwd: null output");
    CN_REQUIRE(((uintptr_t)d->pts & 15) == 0 && ((uintptr_t)d->grad & 15) == 0, CN_ERR_ALIGN,
               "cn_render_fwd: pts / grad 16-byte aligned");
    if (d->z_in)
        CN_REQUIRE(d->S_in >= 1 && d->n_samples >= 1, CN_ERR_SHAPE, "cn_render_fwd: z_in needs S_in and n_samples");
    else
        CN_REQUIRE(d->n_samples >= 1 && d->n_importance >= 0 &&
                       (d->n_importance == 0 || (d->up_sample_steps >= 1 && d->n_importance >= d->up_sample_steps)),
                   CN_ERR_SHAPE, "cn_render_fwd: n_samples %d, n_importance %d over %d up-sample steps", d->n_samples,
                   d->n_importance, d->up_sample_steps);
    const int64_t S = d->z_in ? d->S_in
                              : d->n_samples + (d->n_importance > 0 ? (int64_t)d->up_sample_steps *
                                                                          (d->n_importance / d->up_sample_steps)
                                                                    : 0);
    CN_REQUIRE((int64_t)d->R * S < ((int64_t)1 << 31), CN_ERR_SHAPE, "cn_render_fwd: R x S = %lld too large",
               (long long)d->R * S);
    return CN_OK;
}

int render_S(const cn_render_desc* d) {
    if (d->z_in) return d->S_in;
    const int k = d->n_importance > 0 ? d->n_importance / d->up_sample_steps : 0;
    return d->n_samples + d->up_sample_steps * k;
}

cn_sample_desc render_sample_desc(const cn_render_desc* d) {
    cn_sample_desc sd{};
    sd.R = d->R;
    sd.n_samples = d->n_samples;
    sd.n_importance = d->n_importance;
    sd.up_sample_steps = d->up_sample_steps;
    sd.rays_o = d->rays_o;
    sd.rays_d = d->rays_d;
    sd.near = d->near;
    sd.far = d->far;
    sd.t_rand = d->t_rand;
    sd.philox = d->philox;
    sd.time_step = d->time_step;
    sd.net = d->sdf_net;
    sd.z = d->z;
    return sd;
}

}  // namespace

extern "C" size_t cn_render_fwd_workspace_bytes(const cn_render_desc* d) {
    NetShape s;
    ColorShape cs;
    if (render_check(d, &s, &cs) != CN_OK) return 0;
    const int M = d->R * render_S(d);
    Plan ws(nullptr);
    float* U8 = nullptr;
    sdf_field_plan(d->sdf_net, s, M, nullptr, nullptr, &U8, nullptr, ws, nullptr, false);
    color_field_plan(d->color_net, cs, M, nullptr, nullptr, nullptr, 1, nullptr, 0, nullptr, ws, nullptr, false);
    size_t bytes = ws.used;
    if (!d->z_in) {
        const cn_sample_desc sd = render_sample_desc(d);
        const size_t sb = cn_sample_workspace_bytes(&sd);
        bytes = bytes > sb ? bytes : sb;  // the sampler's workspace is free again once z is written
    }
    return bytes;
}

extern "C" int cn_render_fwd(const cn_render_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    NetShape s;
    ColorShape cs;
    int rc = render_check(d, &s, &cs);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int R = d->R, S = render_S(d);  // (R x S < 2^31: render_check)
    if (R == 0) return CN_OK;
    const size_t need = cn_render_fwd_workspace_bytes(d);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_render_fwd: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_render_fwd: workspace not 256-byte aligned");
    // the samples (neus_renderer.py:466-525), or the caller's
    if (d->z_in) {
        CN_REQUIRE(hipMemcpyAsync(d->z, d->z_in, (size_t)R * S * 4, hipMemcpyDeviceToDevice, st) == hipSuccess,
                   CN_ERR_LAUNCH, "cn_render_fwd: z copy failed");
    } else {
        const cn_sample_desc sd = render_sample_desc(d);
        if ((rc = cn_sample(&sd, workspace, workspace_bytes, stream))) return rc;
    }
    const int M = R * S;
    // render_core (neus_renderer.py:337-420): the midpoints, the fields, the compositing
    if ((rc = cn_points(R, S, d->rays_o, d->rays_d, d->z, d->time_step, 1, d->near, d->far, d->n_samples, d->pts, stream)))
        return rc;
    Plan ws(workspace);
    float* U8 = nullptr;
    if ((rc = sdf_field_plan(d->sdf_net, s, M, d->pts, d->sdf, &U8, d->grad, ws, st, true))) return rc;
    if ((rc = color_field_plan(d->color_net, cs, M, d->grad, d->pts, d->rays_d, S, U8, s.HL, d->rgb, ws, st, true)))
        return rc;
    return cn_composite_fwd(R, S, d->z, d->sdf, d->grad, 4, d->rgb, d->rays_d, d->inv_s, d->near, d->far, d->n_samples,
                            d->cos_anneal_ratio, d->color, d->depth, d->weights, d->cdf, stream);
}

// ---------------------------------------------------------------------------------------------
// cn_point_colors: the colour network at surface points (vertex colours of an extracted mesh), the view
// direction the inward unit normal -- NeuSRenderer.vertex_colors' composition (SDFNetwork.field with the
// hidden activation and ∇ₓSDF, ops.vertex_dirs, RenderingNetwork.color with dir_div 1) in row chunks: the
// field part of cn_render_fwd at points the caller gives, the same launches, the same bits.
namespace {

constexpr int32_t kColorChunk = 1 << 18;

// pts [M][4] = (x[m], t): the rows torch.cat([x, t.expand(M, 1)], 1) holds; dirs [M][3] = one fixed row
__global__ void __launch_bounds__(256) point_rows_kernel(int M, const float* __restrict__ x, const float* __restrict__ t,
                                                         float* __restrict__ pts, float vx, float vy, float vz,
                                                         float* __restrict__ dirs) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    cn::floatx4 o;
    o[0] = x[3 * (int64_t)m];
    o[1] = x[3 * (int64_t)m + 1];
    o[2] = x[3 * (int64_t)m + 2];
    o[3] = t[0];
    reinterpret_cast<cn::floatx4*>(pts)[m] = o;
    if (dirs) {
        dirs[3 * (int64_t)m] = vx;
        dirs[3 * (int64_t)m + 1] = vy;
        dirs[3 * (int64_t)m + 2] = vz;
    }
}

struct ColorsPlan {
    float* pts;
    float* sdf;
    float* G;
    float* dirs;
};

// one chunk of Mc rows: its own buffers, then the two networks' (run: launch; else size only)
int point_colors_chunk(const cn_point_colors_desc* d, const NetShape& s, const ColorShape& cs, int Mc, int64_t m0,
                       const float* vd, Plan& ws, hipStream_t st, bool run) {
    ColorsPlan p;
    p.pts = static_cast<float*>(ws.take((size_t)Mc * 16));
    p.sdf = static_cast<float*>(ws.take((size_t)Mc * 4));
    p.G = static_cast<float*>(ws.take((size_t)Mc * 16));  // (also when grad is given: the plan does not depend on it)
    p.dirs = static_cast<float*>(ws.take((size_t)Mc * 12));
    float* G = run && d->grad ? d->grad + 4 * m0 : p.G;
    float* rgb = run ? d->rgb + 3 * m0 : nullptr;
    int rc;
    if (run) {
        point_rows_kernel<<<(Mc + 255) / 256, 256, 0, st>>>(Mc, d->x + 3 * m0, d->time_step, p.pts, vd ? vd[0] : 0.0f,
                                                             vd ? vd[1] : 0.0f, vd ? vd[2] : 0.0f,
                                                             vd ? p.dirs : nullptr);
        if ((rc = cn::check_launch("cn_point_colors"))) return rc;
    }
    float* U8 = nullptr;
    if ((rc = sdf_field_plan(d->sdf_net, s, Mc, p.pts, p.sdf, &U8, G, ws, st, run))) return rc;
    if (run && !vd && (rc = cn_vertex_dirs(Mc, G, 4, -1.0f, p.dirs, st))) return rc;
    if ((rc = color_field_plan(d->color_net, cs, Mc, G, p.pts, p.dirs, 1, U8, s.HL, rgb, ws, st, run))) return rc;
    if (run && d->rgb8) return cn_rgb8_pack((int64_t)Mc * 3, rgb, d->rgb8 + 3 * m0, st);
    return CN_OK;
}

int point_colors_check(const cn_point_colors_desc* d, NetShape* s, ColorShape* cs, int32_t* chunk) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_point_colors: null descriptor");
    int rc = fold_check("cn_point_colors", d->sdf_net, d->color_net, s, cs);
    if (rc) return rc;
    CN_REQUIRE(d->M >= 0 && d->chunk_rows >= 0, CN_ERR_SHAPE, "cn_point_colors: M %lld, chunk_rows %d", (long long)d->M,
               d->chunk_rows);
    const int64_t c = d->chunk_rows ? d->chunk_rows : kColorChunk;
    *chunk = (int32_t)(c < d->M ? c : d->M);
    // every buffer of a chunk is addressed with 32-bit element offsets: the widest row bounds the chunk
    int row = s->HL > cs->HL ? s->HL : cs->HL;
    row = row > s->KE ? row : s->KE;
    row = row > cs->KX ? row : cs->KX;
    CN_REQUIRE((int64_t)*chunk * row * 4 < ((int64_t)1 << 31), CN_ERR_SHAPE,
               "cn_point_colors: a chunk of %d rows x %d bytes reaches 2^31 (lower chunk_rows)", *chunk, row * 4);
    return CN_OK;
}

}  // namespace

extern "C" size_t cn_point_colors_workspace_bytes(const cn_point_colors_desc* d) {
    NetShape s;
    ColorShape cs;
    int32_t chunk;
    if (point_colors_check(d, &s, &cs, &chunk) != CN_OK) return 0;
    Plan ws(nullptr);
    point_colors_chunk(d, s, cs, chunk, 0, nullptr, ws, nullptr, false);
    return ws.used;
}

extern "C" int cn_point_colors(const cn_point_colors_desc* d, void* workspace, int64_t workspace_bytes,
                               cn_stream_t stream) {
    NetShape s;
    ColorShape cs;
    int32_t chunk;
    int rc = point_colors_check(d, &s, &cs, &chunk);
    if (rc) return rc;
    float vd[3];
    if (d->view_dir) {
        const double x = d->view_dir[0], y = d->view_dir[1], z = d->view_dir[2];
        const double n = std::sqrt((x * x + y * y) + z * z);
        CN_REQUIRE(n > 0.0 && std::isfinite(n), CN_ERR_ARG, "cn_point_colors: view_dir (%g, %g, %g) has no direction", x,
                   y, z);
        vd[0] = (float)(x / n);
        vd[1] = (float)(y / n);
        vd[2] = (float)(z / n);
    }
    if (d->M == 0) return CN_OK;
    CN_REQUIRE(d->x && d->time_step && d->rgb, CN_ERR_ARG, "cn_point_colors: null x / time_step / rgb");
    CN_REQUIRE(((uintptr_t)d->x & 3) == 0 && ((uintptr_t)d->rgb & 3) == 0 && ((uintptr_t)d->grad & 15) == 0, CN_ERR_ALIGN,
               "cn_point_colors: x / rgb 4-byte, grad 16-byte aligned");
    const size_t need = cn_point_colors_workspace_bytes(d);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_point_colors: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_point_colors: workspace not 256-byte aligned");
    for (int64_t m0 = 0; m0 < d->M; m0 += chunk) {
        const int Mc = (int)(d->M - m0 < chunk ? d->M - m0 : chunk);
        Plan ws(workspace);
        if ((rc = point_colors_chunk(d, s, cs, Mc, m0, d->view_dir ? vd : nullptr, ws, (hipStream_t)stream, true)))
            return rc;
    }
    return CN_OK;
}

// ---------------------------------------------------------------------------------------------
// cn_mlp_fwd / cn_mlp_bwd (ABI v14): SDFNetwork.sdf(x) under autograd -- the stage-1 consistency
// re-query of train.py:502-505 (neus_fields.py:268-283 and its backward) -- composed from the
// launches copenerf.fields.sdf_forward (keep, want_feat / want_grad False) and sdf_backward (dsdf
// only, first order, want_dx) or sdf_input_grad (no parameter gradients) make, descriptor for
// descriptor: the same bits.
namespace {

// Zero fill of n floats (the feature rows of lin8's gradient).  A kernel, not hipMemsetAsync: with
// the memsets, replays of a captured training step left those rows differing from the eager step
// from the second replay on (tests/test_gpu_configs.py::test_c5_graph_stage1_joint_pose_replays).
// Isolated in ab/memset_graph.py (profiles/r6_ab.txt r6e): a captured ~1 KB hipMemsetAsync at a
// 4-byte offset (db8 + 1) takes effect on the graph's first replay only (19 of 20 replays stale); the
// 256 KB one beside it, and this kernel in its place, are right on every replay.
__global__ void __launch_bounds__(256) zero_kernel(float* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0.0f;
}

int zero_fill(float* p, int64_t n, hipStream_t stream) {
    if (n <= 0) return CN_OK;
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 1024);
    zero_kernel<<<blocks, 256, 0, stream>>>(p, n);
    CN_REQUIRE(hipGetLastError() == hipSuccess, CN_ERR_LAUNCH, "cn_mlp_bwd: zero fill launch failed");
    return CN_OK;
}

// The forward's kept activations in the caller's state buffer: U_0 (fp32 [M][KE]) and U_1 .. U_L8
// ([M][HL]; bf16 operand images where fields.sdf_forward keeps images only: the image mode's hidden
// layers and the skip input below L8).
struct MlpState {
    float* U0;
    char* U[CN_SDF_MAX_LIN];
    bool ub[CN_SDF_MAX_LIN];
};

void mlp_state_plan(const NetShape& s, int M, Plan& p, MlpState* st) {
    const int L8 = s.L8, sk = s.sk;
    const bool usk_b = s.img && sk >= 1 && sk < L8;
    st->U0 = static_cast<float*>(p.take((size_t)M * s.KE * 4));
    st->U[0] = nullptr;
    st->ub[0] = false;
    for (int l = 1; l <= L8; ++l) {
        st->ub[l] = (l == sk) ? usk_b : (s.img && l < L8);
        st->U[l] = static_cast<char*>(p.take((size_t)M * s.HL * (st->ub[l] ? 2 : 4)));
    }
}

int mlp_check(const cn_mlp_desc* d, NetShape* s, bool bwd) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_mlp: null descriptor");
    int rc = net_shape(d->net, s);
    if (rc) return rc;
    CN_REQUIRE(d->M >= 0 && d->M < (1 << 30), CN_ERR_SHAPE, "cn_mlp: M = %d", d->M);
    if (!bwd) {
        CN_REQUIRE(d->M == 0 || (d->x && d->sdf), CN_ERR_ARG, "cn_mlp_fwd: null x / sdf");
        return CN_OK;
    }
    const cn_sdf_net* n = d->net;
    CN_REQUIRE(d->M == 0 || d->dsdf, CN_ERR_ARG, "cn_mlp_bwd: null dsdf");
    CN_REQUIRE(d->dW[0] || d->dx, CN_ERR_ARG, "cn_mlp_bwd: neither parameter gradients (dW) nor dx asked for");
    if (d->dW[0])
        for (int l = 0; l <= s->L8; ++l)
            CN_REQUIRE(d->dW[l] && d->db[l], CN_ERR_ARG, "cn_mlp_bwd: dW[%d] / db[%d] null", l, l);
    CN_REQUIRE(!d->dx || ((uintptr_t)d->dx & 15) == 0, CN_ERR_ALIGN, "cn_mlp_bwd: dx [M][4] 16-byte aligned");
    const int kq = s->bf ? 64 : 32;
    for (int l = 0; l < s->L8; ++l)
        CN_REQUIRE(n->Wt[l] && ((uintptr_t)n->Wt[l] & 15) == 0 && n->wt_rows[l] >= rup_i(n->in_dim[l], 128) &&
                       n->wt_cols[l] >= rup_i(n->out_dim[l], kq),
                   CN_ERR_SHAPE, "cn_mlp_bwd: transposed image %d missing or too small", l);
    CN_REQUIRE(n->head_wp && ((uintptr_t)n->head_wp & 15) == 0, CN_ERR_ALIGN, "cn_mlp_bwd: head_wp [HL] (16-byte aligned)");
    return CN_OK;
}

int mlp_fwd_run(const cn_mlp_desc* d, const NetShape& s, const MlpState& st, hipStream_t stream) {
    const cn_sdf_net* n = d->net;
    const float kSqrt2 = (float)std::sqrt(2.0);
    const int L8 = s.L8, HL = s.HL, sk = s.sk, M = d->M;
    const bool usk_b = s.img && sk >= 1 && sk < L8;
    void* e_view = nullptr;
    if (sk >= 0) e_view = st.U[sk] + (size_t)n->out_dim[sk - 1] * (usk_b ? 2 : 4);
    int rc = cn_sdf_embed(M, d->x, 4, n->multires, n->scale, s.KE, st.U0, s.KE, e_view, e_view ? HL : 0, kSqrt2,
                          usk_b ? 1 : 0, stream);
    if (rc) return rc;
    for (int l = 0; l < L8; ++l) {
        const bool into = (l + 1) == sk;
        LinCall c;
        c.A = l == 0 ? static_cast<const void*>(st.U0) : st.U[l];
        c.a_b = st.ub[l];
        c.lda = l == 0 ? s.KE : HL;
        c.B = n->W[l];
        c.b_rows = n->w_rows[l];
        c.b_cols = n->w_cols[l];
        c.N = n->out_dim[l];
        c.K = l == 0 ? s.KE : rup_i(n->in_dim[l], 32);
        c.bias = n->bias[l];
        c.beta = n->beta;
        c.threshold = n->threshold;
        c.M = M;
        if (l == L8 - 1 && s.fuse_head) {  // the sdf head in the epilogue, the activation stored (kept)
            c.epi = CN_EPI_SOFTPLUS_HEAD;
            c.out0 = reinterpret_cast<float*>(st.U[L8]);
            c.ld_out0 = HL;
            c.nzero = HL;
            c.head_w = n->head_w;
            c.head_b = n->head_b;
            c.head_out = d->sdf;
        } else {
            c.epi = CN_EPI_SOFTPLUS;
            c.nzero = into ? n->out_dim[l] : HL;
            if (into) c.odiv = kSqrt2;
            if (st.ub[l + 1]) {
                c.out0_b = st.U[l + 1];
                c.ld_out0_b = HL;
            } else {
                c.out0 = reinterpret_cast<float*>(st.U[l + 1]);
                c.ld_out0 = HL;
            }
        }
        if ((rc = run_linear(n->mfma_dtype, c, l, stream))) return rc;
    }
    if (!s.fuse_head)
        return cn_row_head(M, n->in_dim[L8], reinterpret_cast<const float*>(st.U[L8]), HL, n->head_w, n->in_dim[L8],
                           n->head_b, 1, 0, d->sdf, 1, nullptr, stream);
    return CN_OK;
}

// The adjoint chain's MUL launch (fields.sdf_backward / sdf_input_grad): Z_{l-1} = (W_lᵀ Z_l) ⊙ σ_{l-1}
// (+ the skip layer's embedding columns to PE when split)
int mlp_mul(const cn_sdf_net* n, const NetShape& s, const MlpState& st, int M, int l, const void* A, bool a_b,
            void* out, bool out_b, float* PE, bool split, bool skip_div, hipStream_t stream) {
    const float kSqrt2 = (float)std::sqrt(2.0);
    LinCall c;
    c.A = A;
    c.a_b = a_b;
    c.lda = s.HL;
    c.B = n->Wt[l];
    c.b_rows = n->wt_rows[l];
    c.b_cols = n->wt_cols[l];
    c.K = rup_i(n->out_dim[l], 32);
    c.epi = CN_EPI_MUL;
    c.aux0 = st.U[l];
    c.aux0_b = st.ub[l];
    c.ld_aux0 = s.HL;
    c.aux_beta = sig_beta(n, l - 1);
    c.nzero = s.HL;
    c.M = M;
    c.beta = n->beta;
    c.threshold = n->threshold;
    if (split) {
        c.N = n->in_dim[l];
        c.nsplit = n->out_dim[l - 1];
        c.out_split = PE;
        c.ld_split = s.KE;
        c.adiv = kSqrt2;
    } else {
        c.N = n->out_dim[l - 1];
        if (skip_div) c.adiv = kSqrt2;
    }
    if (out_b) {
        c.out0_b = out;
        c.ld_out0_b = s.HL;
    } else {
        c.out0 = static_cast<float*>(out);
        c.ld_out0 = s.HL;
    }
    return run_linear(n->mfma_dtype, c, l, stream);
}

// dx from the embedding adjoint: P0 = W_0ᵀ Z_0, then the assembly with the skip columns PE
int mlp_dx(const cn_sdf_net* n, const NetShape& s, const MlpState& st, int M, const float* Z0, float* P0,
           const float* PE, float* dx, hipStream_t stream) {
    LinCall c;
    c.A = Z0;
    c.lda = s.HL;
    c.B = n->Wt[0];
    c.b_rows = n->wt_rows[0];
    c.b_cols = n->wt_cols[0];
    c.N = s.E;
    c.K = rup_i(n->out_dim[0], 32);
    c.epi = CN_EPI_STORE;
    c.out0 = P0;
    c.ld_out0 = s.KE;
    c.nzero = s.KE;
    c.M = M;
    c.beta = n->beta;
    c.threshold = n->threshold;
    int rc = run_linear(n->mfma_dtype, c, 0, stream);
    if (rc) return rc;
    return cn_sdf_grad_assemble(M, n->multires, n->scale, st.U0, s.KE, P0, s.KE, PE, PE ? s.KE : 0, dx, 4, stream);
}

// The backward's plan over the workspace (run false: sizing only).  With parameter gradients
// (fields.sdf_backward, sdf only, first order, want_dx = dx != NULL): Z_7 .. Z_0 each kept until the
// weight gradients' batch (Z_l a bf16 image where sdf_backward's z_img keeps one), PE, P0, the
// colsum / adjoint column-sum slabs and the cn_wgrad_batch workspace.  Without (sdf_input_grad): two
// fp32 ping-pong adjoints, PE, P0.
int mlp_bwd_plan(const cn_mlp_desc* d, const NetShape& s, const MlpState& st, Plan& ws, hipStream_t stream,
                 bool run) {
    const cn_sdf_net* n = d->net;
    const int L8 = s.L8, HL = s.HL, sk = s.sk, M = d->M;
    const bool params = d->dW[0] != nullptr;
    int rc = CN_OK;
    if (!params) {  // dx only: sdf_input_grad with dsdf alone
        float* P[2] = {static_cast<float*>(ws.take((size_t)M * HL * 4)), static_cast<float*>(ws.take((size_t)M * HL * 4))};
        float* PE = sk >= 0 ? static_cast<float*>(ws.take((size_t)M * s.KE * 4)) : nullptr;
        float* P0 = static_cast<float*>(ws.take((size_t)M * s.KE * 4));
        if (!run) return CN_OK;
        const float* U8 = reinterpret_cast<const float*>(st.U[L8]);
        if ((rc = cn_scale_cols(M, HL, U8, HL, n->head_wp, d->dsdf, P[0], HL, sig_beta(n, L8 - 1), stream))) return rc;
        int cur = 0;
        for (int l = L8 - 1; l >= 1; --l) {
            if ((rc = mlp_mul(n, s, st, M, l, P[cur], false, P[cur ^ 1], false, PE, l == sk, false, stream))) return rc;
            cur ^= 1;
        }
        return mlp_dx(n, s, st, M, P[cur], P0, PE, d->dx, stream);
    }
    const int i8 = n->in_dim[L8], o8 = n->out_dim[L8];
    const bool fused_cs = i8 == HL;
    const bool share = d->dx != nullptr;
    auto z_img = [&](int l) { return s.img && l >= 1 && l < L8 && st.ub[l]; };
    // Z[l]: the parameter adjoint of layer l's output (Z[L8 - 1] the elementwise seed)
    void* Z[CN_SDF_MAX_LIN] = {};
    bool zb[CN_SDF_MAX_LIN] = {};
    zb[L8 - 1] = z_img(L8 - 1) && fused_cs;
    Z[L8 - 1] = ws.take((size_t)M * HL * (zb[L8 - 1] ? 2 : 4));
    for (int l = L8 - 1; l >= 1; --l) {
        zb[l - 1] = z_img(l - 1);
        Z[l - 1] = ws.take((size_t)M * HL * (zb[l - 1] ? 2 : 4));
    }
    float* PE = (share && sk >= 0) ? static_cast<float*>(ws.take((size_t)M * s.KE * 4)) : nullptr;
    float* P0 = share ? static_cast<float*>(ws.take((size_t)M * s.KE * 4)) : nullptr;
    const size_t cs_bytes = fused_cs ? cn_softplus_adjoint_workspace_bytes(M, HL)
                                     : std::max(cn_colsum_workspace_bytes(M, i8), cn_colsum_workspace_bytes(M, 1));
    float* cs_ws = static_cast<float*>(ws.take(cs_bytes));
    // the hidden layers' weight gradients, in sdf_backward's queue order (l = L8-1 .. 0)
    cn_wgrad_desc wd[CN_SDF_MAX_LIN] = {};
    for (int l = L8 - 1; l >= 0; --l) {
        cn_wgrad_desc& w = wd[L8 - 1 - l];
        const bool xb = st.ub[l];
        w.Y0 = Z[l];
        w.X0 = l == 0 ? static_cast<const void*>(st.U0) : st.U[l];
        w.dW = d->dW[l];
        w.db = d->db[l];
        w.ldy0 = HL;
        w.ldx0 = l == 0 ? s.KE : HL;
        w.ld_dw = n->in_dim[l];
        w.M = M;
        w.N = n->out_dim[l];
        w.K = rup_i(n->in_dim[l], 64);
        w.npairs = 1;
        w.n_out = n->out_dim[l];
        w.k_out = n->in_dim[l];
        w.mfma_dtype = n->mfma_dtype;
        w.y_bf16 = zb[l] ? 1 : 0;
        w.x_bf16 = xb ? 1 : 0;
    }
    int64_t offs[CN_SDF_MAX_LIN];
    const size_t wg_bytes = cn_wgrad_batch_workspace_bytes(wd, L8, offs);
    char* wg_ws = static_cast<char*>(ws.take(wg_bytes));
    if (!run) return CN_OK;
    const float* U8 = reinterpret_cast<const float*>(st.U[L8]);
    float* dW8 = d->dW[L8];
    float* db8 = d->db[L8];
    // lin8's rows past the sdf row (the feature head sdf() does not read): zero
    if ((rc = zero_fill(dW8 + i8, (int64_t)(o8 - 1) * i8, stream)) || (rc = zero_fill(db8 + 1, o8 - 1, stream)))
        return rc;
    const float beta7 = sig_beta(n, L8 - 1);
    if (fused_cs) {  // Z_7 = dsdf[m] w80[n] σ_7 with lin8's sdf row / bias gradients from the same pass
        if ((rc = cn_softplus_adjoint(M, HL, nullptr, 0, U8, HL, beta7, d->dsdf, n->head_wp, nullptr, 0, nullptr, 0, 0.0f,
                                      Z[L8 - 1], HL, zb[L8 - 1] ? 1 : 0, 0, dW8, db8, n->scale, cs_ws,
                                      (int64_t)cs_bytes, stream)))
            return rc;
    } else {
        if ((rc = cn_colsum(M, i8, d->dsdf, U8, HL, n->scale, dW8, 0, cs_ws, (int64_t)cs_bytes, stream))) return rc;
        if ((rc = cn_colsum(M, 1, nullptr, d->dsdf, 1, n->scale, db8, 0, cs_ws, (int64_t)cs_bytes, stream))) return rc;
        if ((rc = cn_scale_cols(M, HL, U8, HL, n->head_wp, d->dsdf, static_cast<float*>(Z[L8 - 1]), HL, beta7, stream)))
            return rc;
    }
    for (int l = L8 - 1; l >= 1; --l) {
        if ((rc = mlp_mul(n, s, st, M, l, Z[l], zb[l], Z[l - 1], zb[l - 1], PE, share && l == sk, l == sk, stream)))
            return rc;
    }
    for (int i = 0; i < L8; ++i) {
        wd[i].workspace = reinterpret_cast<float*>(wg_ws + offs[i]);
        wd[i].workspace_bytes = (int64_t)wg_bytes - offs[i];
    }
    if ((rc = cn_wgrad_batch(wd, L8, stream))) return rc;
    if (!share) return CN_OK;
    return mlp_dx(n, s, st, M, static_cast<const float*>(Z[0]), P0, PE, d->dx, stream);
}

}  // namespace

extern "C" size_t cn_mlp_state_bytes(const cn_mlp_desc* d) {
    NetShape s;
    if (mlp_check(d, &s, false) != CN_OK) return 0;
    Plan p(nullptr);
    MlpState st;
    mlp_state_plan(s, d->M, p, &st);
    return p.used;
}

extern "C" size_t cn_mlp_bwd_workspace_bytes(const cn_mlp_desc* d) {
    NetShape s;
    if (mlp_check(d, &s, true) != CN_OK) return 0;
    Plan p(nullptr);
    MlpState st;
    mlp_state_plan(s, d->M, p, &st);
    Plan ws(nullptr);
    mlp_bwd_plan(d, s, st, ws, nullptr, false);
    return ws.used;
}

extern "C" int cn_mlp_fwd(const cn_mlp_desc* d, void* state, int64_t state_bytes, cn_stream_t stream) {
    NetShape s;
    int rc = mlp_check(d, &s, false);
    if (rc) return rc;
    if (d->M == 0) return CN_OK;
    const size_t need = cn_mlp_state_bytes(d);
    CN_REQUIRE(state && state_bytes >= 0 && (size_t)state_bytes >= need, CN_ERR_SHAPE,
               "cn_mlp_fwd: state %lld bytes, %zu needed", (long long)state_bytes, need);
    CN_REQUIRE(((uintptr_t)state & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_mlp_fwd: state not 256-byte aligned");
    Plan p(state);
    MlpState st;
    mlp_state_plan(s, d->M, p, &st);
    return mlp_fwd_run(d, s, st, (hipStream_t)stream);
}

extern "C" int cn_mlp_bwd(const cn_mlp_desc* d, const void* state, int64_t state_bytes, void* workspace,
                          int64_t workspace_bytes, cn_stream_t stream) {
    NetShape s;
    int rc = mlp_check(d, &s, true);
    if (rc) return rc;
    if (d->M == 0) return CN_OK;  // (M = 0: nothing to sum; the caller's gradients are left as they are)
    const size_t need_st = cn_mlp_state_bytes(d);
    CN_REQUIRE(state && state_bytes >= 0 && (size_t)state_bytes >= need_st, CN_ERR_SHAPE,
               "cn_mlp_bwd: state %lld bytes, %zu needed", (long long)state_bytes, need_st);
    const size_t need = cn_mlp_bwd_workspace_bytes(d);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_mlp_bwd: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)state & (kAlign - 1)) == 0 && ((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN,
               "cn_mlp_bwd: state / workspace not 256-byte aligned");
    Plan p(const_cast<void*>(state));
    MlpState st;
    mlp_state_plan(s, d->M, p, &st);
    Plan ws(workspace);
    return mlp_bwd_plan(d, s, st, ws, (hipStream_t)stream, true);
}

// ---------------------------------------------------------------------------------------------
// cn_render_train_fwd / cn_render_bwd (ABI v14): render_core under autograd (neus_renderer.py:307-450) --
// the training forward keeping its state, and the backward of copenerf's composition: _CompositeFn,
// _ColorFieldFn, _SDFFieldFn (fields.sdf_backward with the folded feature head: second order, dh) and
// _PointsFn, with the gradient sums autograd makes between them, in its order.
namespace {

// out[m][c] = a[m][c] + b[m][c], c < C <= 4 (strided rows; one thread per row): autograd's sum of two
// gradients (one fp32 add each, the bits of torch's add)
__global__ void __launch_bounds__(256) add2_kernel(int M, int C, const float* __restrict__ a, int64_t lda,
                                                   const float* __restrict__ b, int64_t ldb, float* __restrict__ out,
                                                   int64_t ldo) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float v[4];
    for (int c = 0; c < C; ++c) v[c] = a[(int64_t)m * lda + c] + b[(int64_t)m * ldb + c];
    for (int c = 0; c < C; ++c) out[(int64_t)m * ldo + c] = v[c];
}

int add2(int M, int C, const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t ldo,
         hipStream_t stream) {
    if (M <= 0) return CN_OK;
    CN_REQUIRE(C >= 1 && C <= 4, CN_ERR_ARG, "cn_render_bwd: add of %d columns", C);
    add2_kernel<<<(M + 255) / 256, 256, 0, stream>>>(M, C, a, lda, b, ldb, out, ldo);
    CN_REQUIRE(hipGetLastError() == hipSuccess, CN_ERR_LAUNCH, "cn_render_bwd: add launch failed");
    return CN_OK;
}

// dst[r][c] = src[r][c], c < C: the colour lin0 gradient's columns into the reference order
__global__ void __launch_bounds__(256) copy_cols_kernel(int R, int C, const float* __restrict__ src, int64_t lds,
                                                        float* __restrict__ dst, int64_t ldd) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < R * C) dst[(int64_t)(i / C) * ldd + i % C] = src[(int64_t)(i / C) * lds + i % C];
}

int copy_cols(int R, int C, const float* src, int64_t lds, float* dst, int64_t ldd, hipStream_t stream) {
    if (R <= 0 || C <= 0) return CN_OK;
    copy_cols_kernel<<<(R * C + 255) / 256, 256, 0, stream>>>(R, C, src, lds, dst, ldd);
    CN_REQUIRE(hipGetLastError() == hipSuccess, CN_ERR_LAUNCH, "cn_render_bwd: copy launch failed");
    return CN_OK;
}

struct TrainState {
    SdfKeep sk;
    ColorKeep ck;
    float* rgb;
};

int train_check(const cn_render_desc* d, NetShape* s, ColorShape* cs) {
    int rc = render_check(d, s, cs, true);
    if (rc) return rc;
    CN_REQUIRE(d->z_in && d->S_in >= 1, CN_ERR_ARG, "cn_render_train_fwd / bwd: the samples z_in [R][S_in] are required");
    return CN_OK;
}

// The state's plan (and, run, the training forward): the points, the SDF field keeping its activations and
// adjoints, the colour network keeping its hidden activations, the compositing.
int train_fwd_plan(const cn_render_desc* d, const NetShape& s, const ColorShape& cs, Plan& p, TrainState* t,
                   hipStream_t st, bool run) {
    const int R = d->R, S = d->S_in, M = R * S;
    t->rgb = static_cast<float*>(p.take((size_t)M * 12));
    float* U8 = nullptr;
    int rc = CN_OK;
    if (run && (rc = cn_points(R, S, d->rays_o, d->rays_d, d->z_in, d->time_step, 1, d->near, d->far, d->n_samples,
                               d->pts, st)))
        return rc;
    if ((rc = sdf_field_plan(d->sdf_net, s, M, d->pts, d->sdf, &U8, d->grad, p, st, run, &t->sk))) return rc;
    if ((rc = color_field_plan(d->color_net, cs, M, d->grad, d->pts, d->rays_d, S, U8, s.HL, t->rgb, p, st, run,
                               &t->ck)))
        return rc;
    if (!run) return CN_OK;
    return cn_composite_fwd(R, S, d->z_in, d->sdf, d->grad, 4, t->rgb, d->rays_d, d->inv_s, d->near, d->far,
                            d->n_samples, d->cos_anneal_ratio, d->color, d->depth, d->weights, d->cdf, st);
}

// a wgrad descriptor as ops._wgrad_desc builds it (K rounded to 64; ld_dw the destination's)
// (npairs explicit: a sizing pass has null operand pointers)
cn_wgrad_desc wgrad_job(int npairs, const void* Y0, bool yb, int64_t ldy, const void* X0, bool xb, int64_t ldx,
                        const void* Y1, int64_t ldy1, const void* X1, int64_t ldx1, int M, int N, int K, float* dW,
                        int64_t ld_dw, float* db, int mode) {
    cn_wgrad_desc w{};
    w.Y0 = Y0;
    w.X0 = X0;
    w.Y1 = Y1;
    w.X1 = X1;
    w.dW = dW;
    w.db = db;
    w.ldy0 = ldy;
    w.ldx0 = ldx;
    w.ldy1 = npairs == 2 ? ldy1 : 0;
    w.ldx1 = npairs == 2 ? ldx1 : 0;
    w.ld_dw = ld_dw;
    w.M = M;
    w.N = N;
    w.K = rup_i(K, 64);
    w.npairs = npairs;
    w.n_out = N;
    w.k_out = K;
    w.mfma_dtype = mode;
    w.y_bf16 = yb ? 1 : 0;
    w.x_bf16 = xb ? 1 : 0;
    return w;
}

// Runs a weight-gradient batch out of a workspace piece (sizing pass: only takes the piece).
int wgrad_batch_run(cn_wgrad_desc* w, int n, Plan& ws, hipStream_t stream, bool run) {
    int64_t offs[2 * CN_SDF_MAX_LIN];
    const size_t bytes = cn_wgrad_batch_workspace_bytes(w, n, offs);
    char* base = static_cast<char*>(ws.take(bytes));
    if (!run) return CN_OK;
    for (int i = 0; i < n; ++i) {
        w[i].workspace = reinterpret_cast<float*>(base + offs[i]);
        w[i].workspace_bytes = (int64_t)bytes - offs[i];
    }
    return cn_wgrad_batch(w, n, stream);
}

// The backward's plan (run false: sizing; the buffers are taken in the same order either way).
int render_bwd_plan(const cn_render_desc* d, const cn_render_grads* g, const NetShape& s, const ColorShape& cs,
                    const TrainState& t, bool pose, Plan& ws, hipStream_t st, bool run) {
    const cn_sdf_net* n = d->sdf_net;
    const cn_color_net* c = d->color_net;
    const float kSqrt2 = (float)std::sqrt(2.0);
    const int R = d->R, S = d->S_in, M = R * S;
    const int L8 = s.L8, HL = s.HL, sk = s.sk, KE = s.KE;
    const int nc = c->n_lin, CHL = cs.HL;
    const int P = 4, Gd = 4, V = 3 * (1 + 2 * c->multires_view), F = c->d_feature, o0 = c->out_dim[0];
    int rc = CN_OK;
    // --- _CompositeFn.backward
    float* dsdf_c = static_cast<float*>(ws.take((size_t)M * 4));
    float* dG_c = static_cast<float*>(ws.take((size_t)M * 16));
    float* drgb = static_cast<float*>(ws.take((size_t)M * 12));
    float* drd_c = pose ? static_cast<float*>(ws.take((size_t)R * 12)) : nullptr;
    if (run && (rc = cn_composite_bwd(R, S, d->z_in, d->sdf, d->grad, 4, t.rgb, d->rays_d, d->inv_s, d->near, d->far,
                                      d->n_samples, d->cos_anneal_ratio, g->dcolor, g->ddepth, g->dweights, g->dcdf,
                                      dsdf_c, dG_c, drgb, g->dinv_s, drd_c, st)))
        return rc;
    // --- _ColorFieldFn.backward (drgb): dZ[l] the adjoint of hidden layer l's output (an image where the
    // image mode reads it only as an operand, l >= 1)
    const ColorKeep& ck = t.ck;
    char* dZ[CN_SDF_MAX_LIN] = {};
    bool dzb[CN_SDF_MAX_LIN] = {};
    for (int l = nc - 2; l >= 0; --l) {
        dzb[l] = cs.img && l >= 1;
        dZ[l] = static_cast<char*>(ws.take((size_t)M * CHL * (dzb[l] ? 2 : 4)));
    }
    const size_t rh_bytes = cn_rgb_head_bwd_workspace_bytes(M, c->in_dim[nc - 1]);
    float* rh_ws = static_cast<float*>(ws.take(rh_bytes));
    if (run && (rc = cn_rgb_head_bwd(M, c->in_dim[nc - 1], drgb, t.rgb, reinterpret_cast<const float*>(ck.H[nc - 2]),
                                     CHL, c->head_w, dZ[nc - 2], CHL, dzb[nc - 2] ? 1 : 0, g->col_dW[nc - 1],
                                     g->col_db[nc - 1], rh_ws, (int64_t)rh_bytes, st)))
        return rc;
    cn_wgrad_desc cw[CN_SDF_MAX_LIN] = {};
    int ncw = 0;
    for (int l = nc - 2; l >= 1; --l) {
        cw[ncw++] = wgrad_job(1, dZ[l], dzb[l], CHL, ck.H[l - 1], ck.hb[l - 1], CHL, nullptr, 0, nullptr, 0, M,
                              c->out_dim[l], c->in_dim[l], g->col_dW[l], c->in_dim[l], g->col_db[l], c->mfma_dtype);
        LinCall k;
        k.A = dZ[l];
        k.a_b = dzb[l];
        k.lda = CHL;
        k.B = c->Wt[l];
        k.b_rows = c->wt_rows[l];
        k.b_cols = c->wt_cols[l];
        k.N = c->out_dim[l - 1];
        k.K = rup_i(c->out_dim[l], 32);
        k.epi = CN_EPI_BWD_RELU;
        k.aux0 = ck.H[l - 1];
        k.aux0_b = ck.hb[l - 1];
        k.ld_aux0 = CHL;
        k.nzero = CHL;
        k.M = M;
        if (dzb[l - 1]) {
            k.out0_b = dZ[l - 1];
            k.ld_out0_b = CHL;
        } else {
            k.out0 = reinterpret_cast<float*>(dZ[l - 1]);
            k.ld_out0 = CHL;
        }
        if (run && (rc = run_linear(c->mfma_dtype, k, l, st))) return rc;
    }
    const float* U8 = reinterpret_cast<const float*>(t.sk.U[L8]);
    const float* dZ0 = reinterpret_cast<const float*>(dZ[0]);
    // lin0's feature columns to dWf, its extras columns to dWx: then both into the reference column order
    float* dW0 = g->col_dW[0];
    const int64_t ld0 = c->in_dim[0];
    // (a buffer of its own, as fields' dWf: the weight gradient's tile choice reads the destination's alignment)
    float* dWf = static_cast<float*>(ws.take((size_t)o0 * F * 4));
    cw[ncw++] = wgrad_job(1, dZ0, false, CHL, U8, false, HL, nullptr, 0, nullptr, 0, M, o0, F, dWf, F, g->col_db[0],
                          c->mfma_dtype);
    float* dWx = static_cast<float*>(ws.take((size_t)o0 * cs.KX * 4));
    {
        cn_wgrad_desc w = wgrad_job(1, dZ0, false, CHL, ck.ext, false, cs.KX, nullptr, 0, nullptr, 0, M, o0, cs.KX, dWx,
                                    cs.KX, nullptr, c->mfma_dtype);
        const size_t b = cn_wgrad_workspace_bytes(M, o0, w.K);
        w.workspace = static_cast<float*>(ws.take(b));
        w.workspace_bytes = (int64_t)b;
        if (run && (rc = cn_wgrad(&w, st))) return rc;
    }
    if ((rc = wgrad_batch_run(cw, ncw, ws, st, run))) return rc;
    if (run) {  // [pts | emb(dirs) | gradient] from dWx's [gradient | pts | emb(dirs)]
        if ((rc = copy_cols(o0, P, dWx + Gd, cs.KX, dW0, ld0, st)) ||
            (rc = copy_cols(o0, V, dWx + Gd + P, cs.KX, dW0 + P, ld0, st)) ||
            (rc = copy_cols(o0, Gd, dWx, cs.KX, dW0 + P + V, ld0, st)) ||
            (rc = copy_cols(o0, F, dWf, F, dW0 + P + V + Gd, ld0, st)))
            return rc;
    }
    float* dfeat = static_cast<float*>(ws.take((size_t)M * F * 4));
    {
        LinCall k;
        k.A = dZ0;
        k.lda = CHL;
        k.B = c->Wtf;
        k.b_rows = c->wtf_rows;
        k.b_cols = c->wtf_cols;
        k.N = F;
        k.K = rup_i(o0, 32);
        k.epi = CN_EPI_STORE;
        k.out0 = dfeat;
        k.ld_out0 = F;
        k.nzero = F;
        k.M = M;
        if (run && (rc = run_linear(c->mfma_dtype, k, 0, st))) return rc;
    }
    const float* dG_col = nullptr;
    int64_t ld_gcol = 4;
    const float* dpts_col = nullptr;
    float* ddirs = nullptr;
    if (pose) {  // d ext = dZ0 W0[:, ext] in one GEMM, ext = [g | pts | emb(dirs)]
        float* d_ext = static_cast<float*>(ws.take((size_t)M * 64 * 4));
        ddirs = static_cast<float*>(ws.take((size_t)R * 12));
        LinCall k;
        k.A = dZ0;
        k.lda = CHL;
        k.B = c->Wxt;
        k.b_rows = c->wxt_rows;
        k.b_cols = c->wxt_cols;
        k.N = rup_i(Gd + P + V, 4);
        k.K = rup_i(o0, 32);
        k.epi = CN_EPI_STORE;
        k.out0 = d_ext;
        k.ld_out0 = 64;
        k.nzero = 64;
        k.M = M;
        if (run && (rc = run_linear(c->mfma_dtype, k, 0, st))) return rc;
        dG_col = d_ext;
        ld_gcol = 64;
        dpts_col = d_ext + Gd;
        if (run && (rc = cn_color_extras_bwd(R, S, d_ext, 64, d->rays_d, 3, c->multires_view, ddirs, 0, st))) return rc;
    } else {
        float* dg = static_cast<float*>(ws.take((size_t)M * 16));
        if (run && (rc = cn_row_head(M, o0, dZ0, CHL, c->Wg, c->wg_ld, nullptr, Gd, 0, dg, Gd, nullptr, st))) return rc;
        dG_col = dg;
    }
    // --- the sums into the SDF field's outputs: ∇ₓSDF = (its own consumers + the compositing's) + the colour
    // network's; sdf = its own consumers + the compositing's
    float* dG = static_cast<float*>(ws.take((size_t)M * 16));
    float* dsdf = dsdf_c;
    if (run) {
        if (g->dgrad) {
            if ((rc = add2(M, 4, g->dgrad, 4, dG_c, 4, dG, 4, st)) || (rc = add2(M, 4, dG, 4, dG_col, ld_gcol, dG, 4, st)))
                return rc;
        } else if ((rc = add2(M, 4, dG_c, 4, dG_col, ld_gcol, dG, 4, st))) {
            return rc;
        }
    }
    // (taken whether or not there is an upstream dsdf: the sizing pass does not see the gradients)
    float* dsdf_sum = static_cast<float*>(ws.take((size_t)M * 4));
    if (g->dsdf) {
        if (run && (rc = add2(M, 1, g->dsdf, 1, dsdf_c, 1, dsdf_sum, 1, st))) return rc;
        dsdf = dsdf_sum;
    }
    // --- _SDFFieldFn.backward: fields.sdf_backward(dsdf, dfeat None, dG, dh = the colour network's dfeat)
    const SdfKeep& k8 = t.sk;
    const bool img = s.img;
    const bool top_img = img && k8.sbf[L8 - 1];  // (fused_cs: the fold makes in_dim[L8] == HL)
    auto act = [&](int l) { return static_cast<const void*>(l == 0 ? static_cast<void*>(k8.U0) : k8.U[l]); };
    // the tangent pass u̇
    float* Ud[CN_SDF_MAX_LIN] = {};
    void* Udb[CN_SDF_MAX_LIN] = {};
    bool udb[CN_SDF_MAX_LIN] = {};  // u̇_l kept as its image
    Ud[0] = static_cast<float*>(ws.take((size_t)M * KE * 4));
    char* Usk_d = nullptr;
    bool usk_db = false;
    if (sk >= 0) {
        usk_db = img && 1 <= sk && sk < L8;
        Usk_d = static_cast<char*>(ws.take((size_t)M * HL * (usk_db ? 2 : 4)));
    }
    for (int l = 0; l < L8; ++l) {
        const bool into = (l + 1) == sk;
        const bool ob = img && (l + 1 < L8 || top_img);
        char* dst = into ? Usk_d : static_cast<char*>(ws.take((size_t)M * HL * (ob ? 2 : 4)));
        udb[l + 1] = ob;
        if (ob)
            Udb[l + 1] = dst;
        else
            Ud[l + 1] = reinterpret_cast<float*>(dst);
    }
    // s_{L8-1} in fp32 where a consumer reads it so and the forward kept only the image
    float* S7f = k8.S[L8 - 1];
    const bool need_s7f = !k8.sf[L8 - 1] && !top_img;
    if (need_s7f) S7f = static_cast<float*>(ws.take((size_t)M * HL * 4));
    auto s_fp32 = [&](int l) -> const float* { return l == L8 - 1 ? S7f : k8.S[l]; };
    auto z_img = [&](int l) { return img && l >= 1 && l < L8 && k8.sbf[l] && k8.ub[l]; };
    void* Z[CN_SDF_MAX_LIN] = {};
    bool zb[CN_SDF_MAX_LIN] = {};
    zb[L8 - 1] = z_img(L8 - 1);
    Z[L8 - 1] = ws.take((size_t)M * HL * (zb[L8 - 1] ? 2 : 4));
    for (int l = L8 - 1; l >= 1; --l) {
        zb[l - 1] = z_img(l - 1);
        Z[l - 1] = ws.take((size_t)M * HL * (zb[l - 1] ? 2 : 4));
    }
    const size_t sa_bytes = cn_softplus_adjoint_workspace_bytes(M, HL);
    float* sa_ws = static_cast<float*>(ws.take(sa_bytes));
    if (run) {
        void* e_view = nullptr;
        if (sk >= 0) e_view = Usk_d + (size_t)n->out_dim[sk - 1] * (usk_db ? 2 : 4);
        if ((rc = cn_sdf_tangent_prep(M, n->multires, n->scale, KE, k8.U0, KE, dG, 4, Ud[0], KE, e_view,
                                      e_view ? HL : 0, kSqrt2, usk_db ? 1 : 0, st)))
            return rc;
        for (int l = 0; l < L8; ++l) {
            const bool into = (l + 1) == sk;
            LinCall k;
            k.A = udb[l] ? Udb[l] : static_cast<const void*>(Ud[l]);
            k.a_b = udb[l];
            k.lda = l == 0 ? KE : HL;
            k.B = n->W[l];
            k.b_rows = n->w_rows[l];
            k.b_cols = n->w_cols[l];
            k.N = n->out_dim[l];
            k.K = l == 0 ? KE : rup_i(n->in_dim[l], 32);
            k.epi = CN_EPI_TANGENT;
            k.aux0 = act(l + 1);
            k.aux0_b = k8.ub[l + 1];
            k.ld_aux0 = HL;
            k.aux_beta = sig_beta(n, l);
            k.nzero = into ? n->out_dim[l] : HL;
            if (into) k.odiv = kSqrt2;
            k.beta = n->beta;
            k.threshold = n->threshold;
            k.M = M;
            if (udb[l + 1]) {
                k.out0_b = Udb[l + 1];
                k.ld_out0_b = HL;
            } else {
                k.out0 = Ud[l + 1];
                k.ld_out0 = HL;
            }
            if ((rc = run_linear(n->mfma_dtype, k, l, st))) return rc;
        }
        if (need_s7f && (rc = cn_scale_cols(M, HL, U8, HL, n->head_wp, nullptr, S7f, HL, sig_beta(n, L8 - 1), st)))
            return rc;
        // lin8's feature rows: the fold carries them (dW8[1:], db8[1:] zero)
        const int i8 = n->in_dim[L8], o8 = n->out_dim[L8];
        if ((rc = zero_fill(g->sdf_dW[L8] + i8, (int64_t)(o8 - 1) * i8, st)) ||
            (rc = zero_fill(g->sdf_db[L8] + 1, o8 - 1, st)))
            return rc;
    }
    // the second-order term's operands of layer l (fields.sdf_backward.second_order)
    struct Second {
        const void* a1;
        const void* a2;
        bool b;
        float scale;
    };
    auto second = [&](int l) {
        const bool img2 = (l < L8 - 1 || top_img) && k8.sbf[l] && udb[l + 1];
        Second r;
        r.a1 = img2 ? k8.Sb[l] : static_cast<const void*>(s_fp32(l));
        r.a2 = img2 ? Udb[l + 1] : static_cast<const void*>(Ud[l + 1]);
        r.b = img2;
        r.scale = n->beta * ((l + 1) == sk ? kSqrt2 : 1.0f);
        return r;
    };
    if (run) {  // Z_7 = (dh + dsdf w80) σ_7 + the second-order term, lin8's sdf row / bias gradients beside
        const Second so = second(L8 - 1);
        if ((rc = cn_softplus_adjoint(M, HL, dfeat, F, U8, HL, sig_beta(n, L8 - 1), dsdf, n->head_wp, so.a1, HL, so.a2,
                                      HL, so.scale, Z[L8 - 1], HL, zb[L8 - 1] ? 1 : 0, so.b ? 4 : 0, g->sdf_dW[L8],
                                      g->sdf_db[L8], n->scale, sa_ws, (int64_t)sa_bytes, st)))
            return rc;
    }
    cn_wgrad_desc sw[CN_SDF_MAX_LIN] = {};
    for (int l = L8 - 1; l >= 0; --l) {
        if (l > 0 && run) {
            const Second so = second(l - 1);
            LinCall k;
            k.A = Z[l];
            k.a_b = zb[l];
            k.lda = HL;
            k.B = n->Wt[l];
            k.b_rows = n->wt_rows[l];
            k.b_cols = n->wt_cols[l];
            k.N = n->out_dim[l - 1];
            k.K = rup_i(n->out_dim[l], 32);
            k.epi = CN_EPI_BWD_SOFTPLUS;
            k.aux0 = act(l);
            k.aux0_b = k8.ub[l];
            k.ld_aux0 = HL;
            k.aux_beta = sig_beta(n, l - 1);
            k.nzero = HL;
            if (l == sk) k.adiv = kSqrt2;
            k.aux1 = so.a1;
            k.aux2 = so.a2;
            k.ld_aux1 = HL;
            k.ld_aux2 = HL;
            k.aux2_scale = so.scale;
            k.aux12_b = so.b;
            k.beta = n->beta;
            k.threshold = n->threshold;
            k.M = M;
            if (zb[l - 1]) {
                k.out0_b = Z[l - 1];
                k.ld_out0_b = HL;
            } else {
                k.out0 = static_cast<float*>(Z[l - 1]);
                k.ld_out0 = HL;
            }
            if ((rc = run_linear(n->mfma_dtype, k, l, st))) return rc;
        }
        const bool xb = k8.ub[l] && udb[l];
        const int64_t ldx = l == 0 ? KE : HL;
        sw[L8 - 1 - l] = wgrad_job(2, Z[l], zb[l], HL, xb ? act(l) : act(l), xb, ldx, zb[l] ? k8.Sb[l] : s_fp32(l), HL,
                                   xb ? Udb[l] : static_cast<const void*>(Ud[l]), ldx, M, n->out_dim[l], n->in_dim[l],
                                   g->sdf_dW[l], n->in_dim[l], g->sdf_db[l], n->mfma_dtype);
    }
    if ((rc = wgrad_batch_run(sw, L8, ws, st, run))) return rc;
    if (!pose) return CN_OK;
    // --- dx (fields.sdf_input_grad with dh): the first-order adjoint chain P in fp32
    float* Pp[2] = {static_cast<float*>(ws.take((size_t)M * HL * 4)), static_cast<float*>(ws.take((size_t)M * HL * 4))};
    float* PE = sk >= 0 ? static_cast<float*>(ws.take((size_t)M * KE * 4)) : nullptr;
    float* P0 = static_cast<float*>(ws.take((size_t)M * KE * 4));
    float* dx = static_cast<float*>(ws.take((size_t)M * 16));
    float* dpts = static_cast<float*>(ws.take((size_t)M * 16));
    float* drd_p = static_cast<float*>(ws.take((size_t)R * 12));
    if (!run) return CN_OK;
    if ((rc = cn_softplus_adjoint(M, HL, dfeat, F, U8, HL, sig_beta(n, L8 - 1), dsdf, n->head_wp, nullptr, 0, nullptr, 0,
                                  0.0f, Pp[0], HL, 0, 0, nullptr, nullptr, 1.0f, nullptr, 0, st)))
        return rc;
    MlpState ms;
    ms.U0 = k8.U0;
    for (int l = 0; l <= L8; ++l) {
        ms.U[l] = k8.U[l];
        ms.ub[l] = k8.ub[l];
    }
    int cur = 0;
    for (int l = L8 - 1; l >= 1; --l) {
        if ((rc = mlp_mul(n, s, ms, M, l, Pp[cur], false, Pp[cur ^ 1], false, PE, l == sk, false, st))) return rc;
        cur ^= 1;
    }
    if ((rc = mlp_dx(n, s, ms, M, Pp[cur], P0, PE, dx, st))) return rc;
    // --- _PointsFn.backward: the points' gradient = (their own consumers + the colour network's) + the SDF's
    if (g->dpts) {
        if ((rc = add2(M, 4, g->dpts, 4, dpts_col, 64, dpts, 4, st)) || (rc = add2(M, 4, dpts, 4, dx, 4, dpts, 4, st)))
            return rc;
    } else if ((rc = add2(M, 4, dpts_col, 64, dx, 4, dpts, 4, st))) {
        return rc;
    }
    if ((rc = cn_points_bwd(R, S, d->z_in, 1, d->near, d->far, d->n_samples, dpts, 4, g->drays_o, drd_p, st))) return rc;
    // rays_d: (the compositing's + the view directions') + the points'
    if ((rc = add2(R, 3, drd_c, 3, ddirs, 3, g->drays_d, 3, st))) return rc;
    return add2(R, 3, g->drays_d, 3, drd_p, 3, g->drays_d, 3, st);
}

int train_bwd_check(const cn_render_desc* d, const cn_render_grads* g, const NetShape& s) {
    CN_REQUIRE(g, CN_ERR_ARG, "cn_render_bwd: null gradients");
    CN_REQUIRE((g->drays_o == nullptr) == (g->drays_d == nullptr), CN_ERR_ARG,
               "cn_render_bwd: drays_o and drays_d both or neither");
    CN_REQUIRE(g->dinv_s, CN_ERR_ARG, "cn_render_bwd: dinv_s [R] required");
    for (int l = 0; l <= s.L8; ++l)
        CN_REQUIRE(g->sdf_dW[l] && g->sdf_db[l], CN_ERR_ARG, "cn_render_bwd: sdf_dW[%d] / sdf_db[%d] null", l, l);
    const cn_color_net* c = d->color_net;
    for (int l = 0; l < c->n_lin; ++l)
        CN_REQUIRE(g->col_dW[l] && g->col_db[l], CN_ERR_ARG, "cn_render_bwd: col_dW[%d] / col_db[%d] null", l, l);
    const int kq = s.bf ? 64 : 32;
    for (int l = 1; l + 1 < c->n_lin; ++l)
        CN_REQUIRE(c->Wt[l] && ((uintptr_t)c->Wt[l] & 15) == 0 && c->wt_rows[l] >= rup_i(c->in_dim[l], 128) &&
                       c->wt_cols[l] >= rup_i(c->out_dim[l], kq),
                   CN_ERR_SHAPE, "cn_render_bwd: colour transposed image %d missing or too small", l);
    CN_REQUIRE(c->Wtf && c->Wg && c->Wxt && c->wg_ld >= c->out_dim[0] && c->wtf_rows >= rup_i(c->d_feature, 128) &&
                   c->wxt_rows >= 64,
               CN_ERR_SHAPE, "cn_render_bwd: colour lin0's transposed images missing or too small");
    return CN_OK;
}

}  // namespace

extern "C" size_t cn_render_state_bytes(const cn_render_desc* d) {
    NetShape s;
    ColorShape cs;
    if (train_check(d, &s, &cs) != CN_OK) return 0;
    Plan p(nullptr);
    TrainState t;
    train_fwd_plan(d, s, cs, p, &t, nullptr, false);
    return p.used;
}

extern "C" size_t cn_render_bwd_workspace_bytes(const cn_render_desc* d, int32_t pose) {
    NetShape s;
    ColorShape cs;
    if (train_check(d, &s, &cs) != CN_OK) return 0;
    Plan p(nullptr);
    TrainState t;
    train_fwd_plan(d, s, cs, p, &t, nullptr, false);
    cn_render_grads g{};
    Plan ws(nullptr);
    render_bwd_plan(d, &g, s, cs, t, pose != 0, ws, nullptr, false);
    return ws.used;
}

extern "C" int cn_render_train_fwd(const cn_render_desc* d, void* state, int64_t state_bytes, cn_stream_t stream) {
    NetShape s;
    ColorShape cs;
    int rc = train_check(d, &s, &cs);
    if (rc) return rc;
    if (d->R == 0) return CN_OK;
    const size_t need = cn_render_state_bytes(d);
    CN_REQUIRE(state && state_bytes >= 0 && (size_t)state_bytes >= need, CN_ERR_SHAPE,
               "cn_render_train_fwd: state %lld bytes, %zu needed", (long long)state_bytes, need);
    CN_REQUIRE(((uintptr_t)state & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_render_train_fwd: state not 256-byte aligned");
    Plan p(state);
    TrainState t;
    return train_fwd_plan(d, s, cs, p, &t, (hipStream_t)stream, true);
}

extern "C" int cn_render_bwd(const cn_render_desc* d, const cn_render_grads* g, const void* state, int64_t state_bytes,
                             void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    NetShape s;
    ColorShape cs;
    int rc = train_check(d, &s, &cs);
    if (rc) return rc;
    if ((rc = train_bwd_check(d, g, s))) return rc;
    if (d->R == 0) return CN_OK;
    const bool pose = g->drays_o != nullptr;
    const size_t need_st = cn_render_state_bytes(d);
    const size_t need = cn_render_bwd_workspace_bytes(d, pose ? 1 : 0);
    CN_REQUIRE(state && state_bytes >= 0 && (size_t)state_bytes >= need_st, CN_ERR_SHAPE,
               "cn_render_bwd: state %lld bytes, %zu needed", (long long)state_bytes, need_st);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_render_bwd: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)state & (kAlign - 1)) == 0 && ((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN,
               "cn_render_bwd: state / workspace not 256-byte aligned");
    Plan p(const_cast<void*>(state));
    TrainState t;
    train_fwd_plan(d, s, cs, p, &t, nullptr, false);  // the state's layout (pointers only)
    Plan dry(nullptr);  // the plan with these gradients must fit what was sized (nothing launched yet)
    render_bwd_plan(d, g, s, cs, t, pose, dry, nullptr, false);
    CN_REQUIRE(dry.used <= need, CN_ERR_SHAPE, "cn_render_bwd: internal plan %zu bytes > sized %zu", dry.used, need);
    Plan ws(workspace);
    return render_bwd_plan(d, g, s, cs, t, pose, ws, (hipStream_t)stream, true);
}
