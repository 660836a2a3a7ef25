// cn_mesh_shade.hip — what a rasterised mesh looks like (additive to ABI v22): per pixel of cn_mesh_raster's triangle
// image the perspective-correct interpolation of per-vertex attributes, the surface normal, and the normal and
// shaded pictures.  The reference has no rasteriser; the yardstick is a float64 restatement (tests/mesh_shade_ref.py).
//
// One thread per pixel, x fastest.  The pass takes the rasteriser's own tri image, so it decides no coverage: given
// tri it is a pure function of its inputs, without atomics, bitwise repeatable.  A pixel whose id is outside [0, T),
// or whose triangle has a corner index outside [0, V), is background and reads nothing more.
//
// Arithmetic (fp32, -ffp-contract=off; tests/mesh_shade_ref.py restates it in numpy float32 to set the bounds).  The
// corners are projected and the edge functions formed exactly as cn_mesh_raster.hip documents:
//   a = ((P00 x + P01 y) + P02 z) + P03, b and c alike;  sx = a / c, sy = b / c, iw = 1 / c       (per corner)
//   e_k = sg_k ((hx - lx) (py - ly) - (hy - ly) (px - lx))   the edge opposite corner k, from its endpoint of the
//         smaller vertex index, negated when the triangle runs it from the larger
//   g_k = e_k iw_k;   lambda_k = g_k / ((g_0 + g_1) + g_2)                                 (perspective-correct weights)
//   attr_out[c] = (lambda_0 A_0[c] + lambda_1 A_1[c]) + lambda_2 A_2[c]
// Normal: f = (X_1 - X_0) x (X_2 - X_0), each component u_i w_j - u_j w_i; it faces the camera as wound iff
//   (signed screen area of the projected corners, as wound) x det(P[:, :3]) < 0
// and is negated otherwise (rendering is two-sided, as coverage is), then divided by sqrt((fx fx + fy fy) + fz fz).
// With vertex normals m = (lambda_0 N_0 + lambda_1 N_1) + lambda_2 N_2, normalised the same way and negated when
// (m . f) < 0; a zero or non-finite m leaves f.  With rot: n_i = (R_i0 n_0 + R_i1 n_1) + R_i2 n_2.
// Pictures: normal_img = to_u8(n 128 + 128) (cn_visuals.hip's rule), shaded_img = to_u8((albedo (ambient +
// (1 - ambient) max(0, (n_0 l_0 + n_1 l_1) + n_2 l_2))) 255).
//
// Memory: a gather over indices and vertices that neighbouring pixels share (a wave's 64 pixels of a row see a handful
// of triangles: the 12 + 36 + 12 C bytes per covered pixel come from the caches after the first touch) and a stream of
// outputs, 4 (tri) read and 12 C + 12 + 3 + 3 written per pixel with everything asked for.  Attribute rows of a
// multiple of four channels are read and written as 16-byte vectors.
#include "cn_common.h"

#include <cmath>

namespace cn {
namespace {

constexpr int64_t kMaxCount = ((int64_t)1 << 31) - 1;  // V, T, h w < 2^31
constexpr int kMaxChannels = 16;
constexpr int kMaxGridY = 65535;

struct ShadeArgs {
    int64_t V, T;
    const float* vtx;
    const int32_t* tris;
    const float* proj;      // the chunk's first view
    const int32_t* tri;     // the chunk's first view (as every per-view array below)
    const float* attr;
    const float* vnormals;
    const float* rot;
    int h, w, C;
    float fill, ambient, grey;
    float light[3];
    int albedo_from_attr;
    uint8_t bg[3];
    float* attr_out;
    float* normal_out;
    uint8_t* normal_img;
    uint8_t* shaded_img;
};

// cn_visuals.hip's conversion: NaN and negatives to 0, truncation, saturation at 255
__device__ __forceinline__ uint8_t to_u8(float v) {
    if (!(v > 0.0f)) return 0;
    return (uint8_t)(int)(v < 255.0f ? v : 255.0f);
}

template <bool kVec4>
__global__ void __launch_bounds__(256) mesh_shade_kernel(ShadeArgs a) {
    const int64_t hw = (int64_t)a.h * a.w;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;  // the pixel inside the view
    if (p >= hw) return;
    const int v = blockIdx.y;
    const int64_t i = (int64_t)v * hw + p;  // the pixel inside the chunk: below B h w, the arrays' extent
    const int32_t t = a.tri[i];
    int32_t id[3] = {0, 0, 0};
    bool live = t >= 0 && t < a.T;
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            id[k] = a.tris[(int64_t)t * 3 + k];
            live = live && id[k] >= 0 && id[k] < a.V;
        }
    }
    if (!live) {
        if (a.attr_out) {
            float* o = a.attr_out + i * a.C;
            for (int c = 0; c < a.C; ++c) o[c] = a.fill;  // bound: C <= 16
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (a.normal_out) a.normal_out[i * 3 + c] = 0.0f;
            if (a.normal_img) a.normal_img[i * 3 + c] = a.bg[c];
            if (a.shaded_img) a.shaded_img[i * 3 + c] = a.bg[c];
        }
        return;
    }
    const float* __restrict__ P = a.proj + (int64_t)v * 12;
    float X[3][3], sx[3], sy[3], iw[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) X[k][c] = a.vtx[(int64_t)id[k] * 3 + c];
        const float pa = ((P[0] * X[k][0] + P[1] * X[k][1]) + P[2] * X[k][2]) + P[3];
        const float pb = ((P[4] * X[k][0] + P[5] * X[k][1]) + P[6] * X[k][2]) + P[7];
        const float pc = ((P[8] * X[k][0] + P[9] * X[k][1]) + P[10] * X[k][2]) + P[11];
        sx[k] = pa / pc;
        sy[k] = pb / pc;
        iw[k] = 1.0f / pc;
    }
    const int y = (int)(p / a.w), x = (int)(p - (int64_t)y * a.w);
    const float px = (float)x, py = (float)y;
    float g[3], area = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int ci = (k + 1) % 3, cj = (k + 2) % 3;  // this triangle runs the edge ci -> cj
        const bool fwd = id[ci] < id[cj];
        const int l = fwd ? ci : cj, hgh = fwd ? cj : ci;
        const float sg = fwd ? 1.0f : -1.0f;
        const float dx = sx[hgh] - sx[l], dy = sy[hgh] - sy[l];
        g[k] = (sg * (dx * (py - sy[l]) - dy * (px - sx[l]))) * iw[k];
        if (k == 2) area = sg * (dx * (sy[2] - sy[l]) - dy * (sx[2] - sx[l]));  // twice the screen area, as wound
    }
    const float den = (g[0] + g[1]) + g[2];
    const float l0 = g[0] / den, l1 = g[1] / den, l2 = g[2] / den;

    if (a.attr_out) {
        const float* __restrict__ A0 = a.attr + (int64_t)id[0] * a.C;
        const float* __restrict__ A1 = a.attr + (int64_t)id[1] * a.C;
        const float* __restrict__ A2 = a.attr + (int64_t)id[2] * a.C;
        float* o = a.attr_out + i * a.C;
        if (kVec4) {
            for (int c = 0; c < a.C; c += 4) {  // bound: C / 4 <= 4 rounds
                const floatx4 r0 = *reinterpret_cast<const floatx4*>(A0 + c), r1 = *reinterpret_cast<const floatx4*>(A1 + c),
                              r2 = *reinterpret_cast<const floatx4*>(A2 + c);
                floatx4 r;
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = (l0 * r0[j] + l1 * r1[j]) + l2 * r2[j];
                *reinterpret_cast<floatx4*>(o + c) = r;
            }
        } else {
            for (int c = 0; c < a.C; ++c) o[c] = (l0 * A0[c] + l1 * A1[c]) + l2 * A2[c];  // bound: C <= 16
        }
    }
    if (!(a.normal_out || a.normal_img || a.shaded_img)) return;

    // the face normal, turned towards the camera
    const float u[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
    const float w[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
    float n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    const float det = (P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8])) +
                      P[2] * (P[4] * P[9] - P[5] * P[8]);
    const float turn = area * det < 0.0f ? 1.0f : -1.0f;
    const float flen = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool fok = flen > 0.0f && flen < INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = fok ? (turn * n[c]) / flen : 0.0f;
    if (a.vnormals) {
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            m[c] = (l0 * a.vnormals[(int64_t)id[0] * 3 + c] + l1 * a.vnormals[(int64_t)id[1] * 3 + c]) +
                   l2 * a.vnormals[(int64_t)id[2] * 3 + c];
        const float mlen = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
        if (mlen > 0.0f && mlen < INFINITY) {
            const float side = ((m[0] * n[0] + m[1] * n[1]) + m[2] * n[2]) < 0.0f ? -1.0f : 1.0f;
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] = (side * m[c]) / mlen;
        }
    }
    if (a.rot) {
        const float* __restrict__ R = a.rot + (int64_t)v * 9;
        const float r0 = (R[0] * n[0] + R[1] * n[1]) + R[2] * n[2];
        const float r1 = (R[3] * n[0] + R[4] * n[1]) + R[5] * n[2];
        const float r2 = (R[6] * n[0] + R[7] * n[1]) + R[8] * n[2];
        n[0] = r0;
        n[1] = r1;
        n[2] = r2;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.normal_out) a.normal_out[i * 3 + c] = n[c];
        if (a.normal_img) a.normal_img[i * 3 + c] = to_u8(n[c] * 128.0f + 128.0f);
    }
    if (a.shaded_img) {
        const float lam = fmaxf(0.0f, (n[0] * a.light[0] + n[1] * a.light[1]) + n[2] * a.light[2]);
        const float s = a.ambient + (1.0f - a.ambient) * lam;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float alb = a.grey;
            if (a.albedo_from_attr)  // (C >= 3 by the entry point's checks)
                alb = (l0 * a.attr[(int64_t)id[0] * a.C + c] + l1 * a.attr[(int64_t)id[1] * a.C + c]) +
                      l2 * a.attr[(int64_t)id[2] * a.C + c];
            a.shaded_img[i * 3 + c] = to_u8((alb * s) * 255.0f);
        }
    }
}

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" int cn_mesh_shade(const cn_mesh_shade_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_mesh_shade: null descriptor");
    CN_REQUIRE(d->V >= 0 && d->V <= kMaxCount && d->T >= 0 && d->T <= kMaxCount, CN_ERR_SHAPE,
               "cn_mesh_shade: V %lld, T %lld (each below 2^31)", (long long)d->V, (long long)d->T);
    CN_REQUIRE(d->N >= 0, CN_ERR_SHAPE, "cn_mesh_shade: N %d", d->N);
    CN_REQUIRE(d->h >= 1 && d->w >= 1 && (int64_t)d->h * d->w <= kMaxCount, CN_ERR_SHAPE,
               "cn_mesh_shade: image %d x %d (h w below 2^31)", d->h, d->w);
    const bool attrs = d->attr || d->attr_out || d->albedo_from_attr;
    CN_REQUIRE(!attrs || (d->C >= 1 && d->C <= kMaxChannels), CN_ERR_SHAPE, "cn_mesh_shade: C %d (1 .. 16 channels)", d->C);
    CN_REQUIRE(!d->albedo_from_attr || d->C >= 3, CN_ERR_SHAPE, "cn_mesh_shade: albedo_from_attr with C %d (at least 3)", d->C);
    CN_REQUIRE(d->ambient >= 0.0f && d->ambient <= 1.0f, CN_ERR_SHAPE, "cn_mesh_shade: ambient %g (in [0, 1])", (double)d->ambient);
    CN_REQUIRE(std::isfinite(d->light[0]) && std::isfinite(d->light[1]) && std::isfinite(d->light[2]) && std::isfinite(d->grey),
               CN_ERR_SHAPE, "cn_mesh_shade: light / grey not finite");
    if (d->N == 0) return CN_OK;
    CN_REQUIRE(d->proj && d->tri, CN_ERR_ARG, "cn_mesh_shade: null proj / tri");
    CN_REQUIRE((d->V == 0 || d->vertices) && (d->T == 0 || d->triangles), CN_ERR_ARG, "cn_mesh_shade: null vertices / triangles");
    CN_REQUIRE(d->attr_out || d->normal_out || d->normal_img || d->shaded_img, CN_ERR_ARG, "cn_mesh_shade: null outputs (none asked for)");
    CN_REQUIRE(!(d->attr_out || d->albedo_from_attr) || d->attr, CN_ERR_ARG,
               "cn_mesh_shade: null attr with attr_out / albedo_from_attr");
    CN_REQUIRE((((uintptr_t)d->vertices | (uintptr_t)d->triangles | (uintptr_t)d->proj | (uintptr_t)d->tri | (uintptr_t)d->attr |
                 (uintptr_t)d->vnormals | (uintptr_t)d->rot | (uintptr_t)d->attr_out | (uintptr_t)d->normal_out) & 3) == 0,
               CN_ERR_ALIGN, "cn_mesh_shade: every fp32 / int32 array 4-byte aligned");
    ShadeArgs a{};
    a.V = d->V;
    a.T = d->T;
    a.vtx = d->vertices;
    a.tris = d->triangles;
    a.attr = d->attr;
    a.vnormals = d->vnormals;
    a.h = d->h;
    a.w = d->w;
    a.C = attrs ? d->C : 0;
    a.fill = d->fill;
    a.ambient = d->ambient;
    a.grey = d->grey;
    a.albedo_from_attr = d->albedo_from_attr ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
        a.light[c] = d->light[c];
        a.bg[c] = d->background[c];
    }
    const bool vec4 = a.C > 0 && a.C % 4 == 0 && (((uintptr_t)d->attr | (uintptr_t)d->attr_out) & 15) == 0;
    const int64_t hw = (int64_t)d->h * d->w;
    hipStream_t st = (hipStream_t)stream;
    for (int v0 = 0; v0 < d->N; v0 += kMaxGridY) {  // (one round up to 65535 views)
        const int B = d->N - v0 < kMaxGridY ? d->N - v0 : kMaxGridY;
        a.proj = d->proj + (int64_t)v0 * 12;
        a.tri = d->tri + v0 * hw;
        a.rot = d->rot ? d->rot + (int64_t)v0 * 9 : nullptr;
        a.attr_out = d->attr_out ? d->attr_out + v0 * hw * a.C : nullptr;
        a.normal_out = d->normal_out ? d->normal_out + v0 * hw * 3 : nullptr;
        a.normal_img = d->normal_img ? d->normal_img + v0 * hw * 3 : nullptr;
        a.shaded_img = d->shaded_img ? d->shaded_img + v0 * hw * 3 : nullptr;
        const dim3 grid((unsigned)((hw + 255) / 256), (unsigned)B);
        if (vec4)
            mesh_shade_kernel<true><<<grid, 256, 0, st>>>(a);
        else
            mesh_shade_kernel<false><<<grid, 256, 0, st>>>(a);
        if (int rc = check_launch("cn_mesh_shade")) return rc;
    }
    return CN_OK;
}
