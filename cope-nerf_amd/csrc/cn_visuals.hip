// cn_visuals.hip — the visualisation pass of Trainer.render_visdata (ABI v19).
//
// cn_ray_visuals: the per-ray tail of the render loop (model/training.py:236-281) in one read of the
// samples.  The reference advects every sample point through K Euler steps p <- p + dt (omega_k x p + v_k)
// and then takes the weighted sum: K full passes over [R S, 3].  Every step is affine in p, so the K steps
// compose into one map p -> A p + b, and
//     sum_s w_s (A p_s + b) = A (sum_s w_s p_s) + b (sum_s w_s).
// A one-wavefront kernel composes (A | b) from omega and vel on the device (lane j < 3 advects the basis
// vector e_j with v = 0, lane 3 advects the origin: the columns of A and b), and the main kernel needs only
// sum w p, sum w, sum w n and the arg-max of w per ray.  One wavefront per ray: lane l takes the samples
// l, l + 64, ... in ascending order, then the lanes combine by xor-butterflies (a fixed order, so a ray's
// result depends on nothing but the ray: chunking the image does not change a bit).  Rows of a multiple of
// four floats on a 16-byte boundary (the renderer's [M, 4] buffers) are read as one 16-byte load per lane,
// any other layout as one 12-byte load.  28 bytes per sample are needed; nothing intermediate is written.
//
// cn_visual_images: the per-image arithmetic of training.py:292-318, 343-345.  A first pass over the pixels
// writes one (min, max, max, max, max) partial per workgroup, a single wavefront reduces the partials in a
// fixed order (min and max do not depend on the order: the statistics are exact), and a second pass over
// the pixels writes the five uint8 images.  No atomics.
//
// Compiled like cn_metrics.hip: no fast-math, no contraction; every product-sum written as fmaf() below is a
// deliberate fused operation in a result that is specified to a tolerance, never in one specified exactly.
#include "cn_common.h"

#include <cfloat>

namespace cn {
namespace {

constexpr int kRaysPerBlock = 4;        // one wavefront each
constexpr int kMaxSteps = 1024;         // Euler steps composed per call
constexpr int kPixPerBlock = 2048;      // pixels per workgroup of the statistics pass
constexpr int kStatFloats = 8;          // floats per partial (5 used; 32-byte records)
constexpr size_t kAlign = 256;

struct RayArgs {
    int R, S;
    int64_t ld_p, ld_n;
    const float* pts;
    const float* normals;
    const float* weights;
    const float* world;   // [4][4] or null
    const float* affine;  // [12] = (A | b) row-major 3 x 4, in the workspace (K > 0)
    const float* proj;    // [3][3]
    const float* pix;     // [R][2]
    float sx, sy;
    float* normal;
    float* depth_max_w;
    float* flow;
};

// (A | b) of the K composed Euler steps: lane j holds column j.  c <- c + dt (omega_k x c + [j == 3] v_k).
__global__ void __launch_bounds__(64) compose_kernel(int K, const float* omega, const float* vel, float dt, float* affine) {
    const int j = threadIdx.x;
    if (j >= 4) return;
    float c0 = j == 0 ? 1.0f : 0.0f, c1 = j == 1 ? 1.0f : 0.0f, c2 = j == 2 ? 1.0f : 0.0f;
    for (int k = 0; k < K; ++k) {
        const float ox = omega[3 * k], oy = omega[3 * k + 1], oz = omega[3 * k + 2];
        const float f0 = (oy * c2 - oz * c1) + (j == 3 ? vel[3 * k] : 0.0f);
        const float f1 = (oz * c0 - ox * c2) + (j == 3 ? vel[3 * k + 1] : 0.0f);
        const float f2 = (ox * c1 - oy * c0) + (j == 3 ? vel[3 * k + 2] : 0.0f);
        c0 = c0 + dt * f0;
        c1 = c1 + dt * f1;
        c2 = c2 + dt * f2;
    }
    affine[j] = c0;
    affine[4 + j] = c1;
    affine[8 + j] = c2;
}

struct __attribute__((packed, aligned(4))) Row3 {
    float x, y, z;
};

template <bool kVec4>
__device__ __forceinline__ void load_row(const float* base, int64_t row, int64_t ld, float& x, float& y, float& z) {
    if (kVec4) {
        const floatx4 v = *reinterpret_cast<const floatx4*>(base + row * ld);
        x = v[0];
        y = v[1];
        z = v[2];
    } else {
        const Row3 v = *reinterpret_cast<const Row3*>(base + row * ld);
        x = v.x;
        y = v.y;
        z = v.z;
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// kVec: both row layouts take 16-byte loads; kFlow / kNormal: which sums are formed (their inputs exist).
template <bool kVec, bool kFlow, bool kNormal>
__global__ void __launch_bounds__(64 * kRaysPerBlock) ray_visuals_kernel(RayArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6);
    if (r >= a.R) return;  // the whole wavefront leaves: no shuffle below sees a missing lane
    const int S = a.S;
    const int64_t row0 = r * S;
    const float* __restrict__ w = a.weights + row0;
    constexpr bool want_p = kFlow, want_n = kNormal;
    const bool want_d = a.depth_max_w != nullptr;

    float sw = 0.0f, p0 = 0.0f, p1 = 0.0f, p2 = 0.0f, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    for (int s = lane; s < S; s += 64) {
        const float ws = w[s];
        if (ws > best) {  // strict: the lowest index of a lane's equal maxima stays
            best = ws;
            best_i = s;
        }
        if (want_p) {
            float x, y, z;
            load_row<kVec>(a.pts, row0 + s, a.ld_p, x, y, z);
            sw += ws;
            p0 = fmaf(ws, x, p0);
            p1 = fmaf(ws, y, p1);
            p2 = fmaf(ws, z, p2);
        }
        if (want_n) {
            float x, y, z;
            load_row<kVec>(a.normals, row0 + s, a.ld_n, x, y, z);
            n0 = fmaf(ws, x, n0);
            n1 = fmaf(ws, y, n1);
            n2 = fmaf(ws, z, n2);
        }
    }

    const float* W = a.world;
    if (want_d) {
        // (value, index) arg-max over the lanes: the larger value, the lower index among equals.  A lane
        // without a sample holds (-inf, INT_MAX); weights that are all -inf or NaN give index 0.
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(best, o, 64);
            const int oi = __shfl_xor(best_i, o, 64);
            const bool take = ov > best || (ov == best && oi < best_i);
            best = take ? ov : best;
            best_i = take ? oi : best_i;
        }
        if (lane == 0) {
            const int i = best_i < S ? best_i : 0;
            float x, y, z;
            load_row<false>(a.pts, row0 + i, a.ld_p, x, y, z);
            a.depth_max_w[r] = W ? -(fmaf(W[8], x, fmaf(W[9], y, fmaf(W[10], z, W[11])))) : -z;
        }
    }
    if (want_n) {
        n0 = wave_sum(n0);
        n1 = wave_sum(n1);
        n2 = wave_sum(n2);
        if (lane == 0) {
            float* o = a.normal + r * 3;
            if (W) {
                o[0] = fmaf(W[0], n0, fmaf(W[1], n1, W[2] * n2));
                o[1] = fmaf(W[4], n0, fmaf(W[5], n1, W[6] * n2));
                o[2] = fmaf(W[8], n0, fmaf(W[9], n1, W[10] * n2));
            } else {
                o[0] = n0;
                o[1] = n1;
                o[2] = n2;
            }
        }
    }
    if (want_p) {
        sw = wave_sum(sw);
        p0 = wave_sum(p0);
        p1 = wave_sum(p1);
        p2 = wave_sum(p2);
        if (lane == 0) {
            const float* A = a.affine;
            const float P0 = fmaf(A[0], p0, fmaf(A[1], p1, fmaf(A[2], p2, A[3] * sw)));
            const float P1 = fmaf(A[4], p0, fmaf(A[5], p1, fmaf(A[6], p2, A[7] * sw)));
            const float P2 = fmaf(A[8], p0, fmaf(A[9], p1, fmaf(A[10], p2, A[11] * sw)));
            const float* M = a.proj;
            const float q0 = fmaf(M[0], P0, fmaf(M[1], P1, M[2] * P2));
            const float q1 = fmaf(M[3], P0, fmaf(M[4], P1, M[5] * P2));
            const float q2 = fmaf(M[6], P0, fmaf(M[7], P1, M[8] * P2));
            a.flow[r * 2] = (q0 / q2 - a.pix[r * 2]) * a.sx;
            a.flow[r * 2 + 1] = (q1 / q2 - a.pix[r * 2 + 1]) * a.sy;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// the image pass

// numpy's min / max: a NaN on either side stays
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }
__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }

struct Stats {
    float zmin, zmax, disp, disp_hw, fnorm;
};

__device__ __forceinline__ Stats stats_identity() { return {INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0f}; }

__device__ __forceinline__ Stats stats_merge(Stats a, Stats b) {
    return {nan_min(a.zmin, b.zmin), nan_max(a.zmax, b.zmax), nan_max(a.disp, b.disp), nan_max(a.disp_hw, b.disp_hw),
            nan_max(a.fnorm, b.fnorm)};
}

__device__ __forceinline__ Stats stats_wave(Stats s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Stats t;
        t.zmin = __shfl_xor(s.zmin, o, 64);
        t.zmax = __shfl_xor(s.zmax, o, 64);
        t.disp = __shfl_xor(s.disp, o, 64);
        t.disp_hw = __shfl_xor(s.disp_hw, o, 64);
        t.fnorm = __shfl_xor(s.fnorm, o, 64);
        s = stats_merge(s, t);
    }
    return s;
}

__device__ __forceinline__ void stats_store(float* p, Stats s) {
    p[0] = s.zmin;
    p[1] = s.zmax;
    p[2] = s.disp;
    p[3] = s.disp_hw;
    p[4] = s.fnorm;
}

__device__ __forceinline__ Stats stats_load(const float* p) { return {p[0], p[1], p[2], p[3], p[4]}; }

struct ImageArgs {
    int HW;
    const float* rgb;
    const float* depth;
    const float* depth_max_w;
    const float* weighted_z;
    const float* normal;
    const float* flow;
    float* part;          // [blocks][kStatFloats]
    const float* stats;   // [5]
    uint8_t* img;
    uint8_t* disparity;
    uint8_t* disparity_hw;
    uint8_t* normal_img;
    uint8_t* flow_img;
};

__global__ void __launch_bounds__(256) image_stats_kernel(ImageArgs a) {
    __shared__ float red[4][kStatFloats];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Stats s = stats_identity();
    const int64_t first = (int64_t)blockIdx.x * kPixPerBlock;
#pragma unroll
    for (int k = 0; k < kPixPerBlock / 256; ++k) {
        const int64_t i = first + k * 256 + tid;
        if (i >= a.HW) break;
        Stats t;
        t.zmin = t.zmax = a.weighted_z[i];
        t.disp = 1.0f / a.depth[i];
        t.disp_hw = 1.0f / a.depth_max_w[i];
        t.fnorm = 0.0f;
        if (a.flow) {
            const float fx = a.flow[2 * i], fy = a.flow[2 * i + 1];
            t.fnorm = sqrtf(fx * fx + fy * fy);
        }
        s = stats_merge(s, t);
    }
    s = stats_wave(s);
    if (lane == 0) stats_store(red[wave], s);
    __syncthreads();
    if (tid == 0) {
        s = stats_load(red[0]);
        for (int v = 1; v < 4; ++v) s = stats_merge(s, stats_load(red[v]));
        stats_store(a.part + (int64_t)blockIdx.x * kStatFloats, s);
    }
}

__global__ void __launch_bounds__(64) image_stats_reduce_kernel(const float* part, int blocks, float* stats) {
    const int lane = threadIdx.x;
    Stats s = stats_identity();
    for (int b = lane; b < blocks; b += 64) s = stats_merge(s, stats_load(part + (int64_t)b * kStatFloats));
    s = stats_wave(s);
    if (lane == 0) stats_store(stats, s);
}

// The Middlebury colour wheel as torchvision.utils.flow_to_image builds it: 55 rows from the segments
// RY 15, YG 6, GC 4, CB 11, BM 13, MR 6 with the ramps floor(255 i / n), written out by hand.
__constant__ uint8_t kWheel[55][3] = {
    // RY: (255, floor(255 i / 15), 0)
    {255, 0, 0}, {255, 17, 0}, {255, 34, 0}, {255, 51, 0}, {255, 68, 0}, {255, 85, 0}, {255, 102, 0}, {255, 119, 0},
    {255, 136, 0}, {255, 153, 0}, {255, 170, 0}, {255, 187, 0}, {255, 204, 0}, {255, 221, 0}, {255, 238, 0},
    // YG: (255 - floor(255 i / 6), 255, 0)
    {255, 255, 0}, {213, 255, 0}, {170, 255, 0}, {128, 255, 0}, {85, 255, 0}, {43, 255, 0},
    // GC: (0, 255, floor(255 i / 4))
    {0, 255, 0}, {0, 255, 63}, {0, 255, 127}, {0, 255, 191},
    // CB: (0, 255 - floor(255 i / 11), 255)
    {0, 255, 255}, {0, 232, 255}, {0, 209, 255}, {0, 186, 255}, {0, 163, 255}, {0, 140, 255}, {0, 116, 255},
    {0, 93, 255}, {0, 70, 255}, {0, 47, 255}, {0, 24, 255},
    // BM: (floor(255 i / 13), 0, 255)
    {0, 0, 255}, {19, 0, 255}, {39, 0, 255}, {58, 0, 255}, {78, 0, 255}, {98, 0, 255}, {117, 0, 255}, {137, 0, 255},
    {156, 0, 255}, {176, 0, 255}, {196, 0, 255}, {215, 0, 255}, {235, 0, 255},
    // MR: (255, 0, 255 - floor(255 i / 6))
    {255, 0, 255}, {255, 0, 213}, {255, 0, 170}, {255, 0, 128}, {255, 0, 85}, {255, 0, 43},
};

// trunc(clamp(v, 0, 255)) as a byte; NaN gives 0
__device__ __forceinline__ uint8_t to_u8(float v) {
    if (!(v > 0.0f)) return 0;
    return (uint8_t)(int)(v < 255.0f ? v : 255.0f);
}

__global__ void __launch_bounds__(256) image_map_kernel(ImageArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.HW) return;
    if (a.img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.img[3 * i + c] = to_u8(a.rgb[3 * i + c] * 255.0f);
    }
    if (a.normal_img) {
#pragma unroll
        for (int c = 0; c < 3; ++c) a.normal_img[3 * i + c] = to_u8(a.normal[3 * i + c] * 128.0f + 128.0f);
    }
    if (a.disparity) a.disparity[i] = to_u8(((1.0f / a.depth[i]) / a.stats[2]) * 255.0f);
    if (a.disparity_hw) a.disparity_hw[i] = to_u8(((1.0f / a.depth_max_w[i]) / a.stats[3]) * 255.0f);
    if (a.flow_img) {
        const float den = a.stats[4] + FLT_EPSILON;
        const float ux = a.flow[2 * i] / den, uy = a.flow[2 * i + 1] / den;
        const float norm = sqrtf(ux * ux + uy * uy);
        const float ang = atan2f(-uy, -ux) / 3.14159265358979323846f;
        const float fk = (ang + 1.0f) / 2.0f * 54.0f;
        const float fl = floorf(fk);
        int k0 = fl >= 0.0f ? (int)(fl < 54.0f ? fl : 54.0f) : 0;  // NaN: row 0
        const int k1 = k0 == 54 ? 0 : k0 + 1;
        const float f = fk - fl;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float c0 = (float)kWheel[k0][c] / 255.0f, c1 = (float)kWheel[k1][c] / 255.0f;
            float col = (1.0f - f) * c0 + f * c1;
            col = 1.0f - norm * (1.0f - col);
            a.flow_img[3 * i + c] = to_u8(floorf(255.0f * col));
        }
    }
}

int64_t stat_blocks(int64_t HW) { return (HW + kPixPerBlock - 1) / kPixPerBlock; }

size_t round_up(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

int image_shape_check(const char* who, int H, int W) {
    CN_REQUIRE(H >= 1 && W >= 1, CN_ERR_SHAPE, "%s: image of %d x %d (each at least 1)", who, H, W);
    CN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), CN_ERR_SHAPE, "%s: image of %d x %d too large (H W must stay below 2^31)",
               who, H, W);
    return CN_OK;
}

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" size_t cn_ray_visuals_workspace_bytes(int32_t K) { return (K >= 1 && K <= kMaxSteps) ? kAlign : 0; }

extern "C" int cn_ray_visuals(int32_t R, int32_t S, const float* pts, int64_t ld_p, const float* normals, int64_t ld_n,
                              const float* weights, const float* world_mat, int32_t K, const float* omega,
                              const float* vel, float dt, const float* proj, const float* pix,
                              const float* flow_scale, float* normal, float* depth_max_w, float* flow,
                              void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    CN_REQUIRE(R >= 0 && S >= 1, CN_ERR_SHAPE, "cn_ray_visuals: %d rays of %d samples (R >= 0, S >= 1)", R, S);
    CN_REQUIRE(K >= 0 && K <= kMaxSteps, CN_ERR_SHAPE, "cn_ray_visuals: %d Euler steps (0 .. %d)", K, kMaxSteps);
    CN_REQUIRE(ld_p >= 3 && ld_n >= 3, CN_ERR_SHAPE, "cn_ray_visuals: leading dimensions %lld, %lld (at least 3)",
               (long long)ld_p, (long long)ld_n);
    CN_REQUIRE(!(flow && K == 0), CN_ERR_ARG, "cn_ray_visuals: a flow needs at least one Euler step (K = 0)");
    CN_REQUIRE(!flow || (proj && pix && flow_scale), CN_ERR_ARG, "cn_ray_visuals: a flow needs proj, pix and flow_scale (null)");
    CN_REQUIRE(!flow || (omega && vel), CN_ERR_ARG, "cn_ray_visuals: a flow needs omega and vel (null)");
    if (R == 0) return CN_OK;
    CN_REQUIRE(weights, CN_ERR_ARG, "cn_ray_visuals: null weights");
    CN_REQUIRE(pts || !(flow || depth_max_w), CN_ERR_ARG, "cn_ray_visuals: null pts with a flow or depth_max_w output");
    CN_REQUIRE(normals || !normal, CN_ERR_ARG, "cn_ray_visuals: null normals with a normal output");
    const uintptr_t all4 = (uintptr_t)pts | (uintptr_t)normals | (uintptr_t)weights | (uintptr_t)world_mat |
                           (uintptr_t)omega | (uintptr_t)vel | (uintptr_t)proj | (uintptr_t)pix | (uintptr_t)normal |
                           (uintptr_t)depth_max_w | (uintptr_t)flow;
    CN_REQUIRE((all4 & 3) == 0, CN_ERR_ALIGN, "cn_ray_visuals: every array 4-byte aligned");
    float* affine = nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (flow) {
        const size_t need = cn_ray_visuals_workspace_bytes(K);
        CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
                   "cn_ray_visuals: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
        CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_ray_visuals: workspace not 256-byte aligned");
        affine = static_cast<float*>(workspace);
        compose_kernel<<<1, 64, 0, st>>>(K, omega, vel, dt, affine);
        if (int rc = check_launch("cn_ray_visuals (compose)")) return rc;
    }
    if (!(normal || depth_max_w || flow)) return CN_OK;
    RayArgs a{R, S, ld_p, ld_n, pts, normals, weights, world_mat, affine, proj, pix, flow ? flow_scale[0] : 0.0f,
              flow ? flow_scale[1] : 0.0f, normal, depth_max_w, flow};
    // 16-byte row loads when both layouts allow them (an input that is not read does not matter)
    const bool vp = !(flow || depth_max_w) || (ld_p % 4 == 0 && ((uintptr_t)pts & 15) == 0);
    const bool vn = !normal || (ld_n % 4 == 0 && ((uintptr_t)normals & 15) == 0);
    const dim3 grid((unsigned)(((int64_t)R + kRaysPerBlock - 1) / kRaysPerBlock)), block(64 * kRaysPerBlock);
    using Kernel = void (*)(RayArgs);
    static const Kernel kernels[8] = {
        ray_visuals_kernel<false, false, false>, ray_visuals_kernel<false, false, true>,
        ray_visuals_kernel<false, true, false>,  ray_visuals_kernel<false, true, true>,
        ray_visuals_kernel<true, false, false>,  ray_visuals_kernel<true, false, true>,
        ray_visuals_kernel<true, true, false>,   ray_visuals_kernel<true, true, true>};
    kernels[(vp && vn ? 4 : 0) + (flow ? 2 : 0) + (normal ? 1 : 0)]<<<grid, block, 0, st>>>(a);
    return check_launch("cn_ray_visuals");
}

extern "C" size_t cn_visual_images_workspace_bytes(int32_t H, int32_t W) {
    if (image_shape_check("cn_visual_images_workspace_bytes", H, W) != CN_OK) return 0;
    return round_up((size_t)stat_blocks((int64_t)H * W) * kStatFloats * sizeof(float));
}

extern "C" int cn_visual_images(int32_t H, int32_t W, const float* rgb, const float* depth, const float* depth_max_w,
                                const float* weighted_z, const float* normal, const float* flow, float* stats,
                                uint8_t* img, uint8_t* disparity, uint8_t* disparity_hw, uint8_t* normal_img,
                                uint8_t* flow_img, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    if (int rc = image_shape_check("cn_visual_images", H, W)) return rc;
    CN_REQUIRE(stats || !(disparity || disparity_hw || flow_img), CN_ERR_ARG,
               "cn_visual_images: null stats with a disparity or flow image (they are normalised by it)");
    CN_REQUIRE(!stats || (depth && depth_max_w && weighted_z), CN_ERR_ARG,
               "cn_visual_images: the statistics need depth, depth_max_w and weighted_z (null)");
    CN_REQUIRE(!img || rgb, CN_ERR_ARG, "cn_visual_images: null rgb with an img output");
    CN_REQUIRE(!normal_img || normal, CN_ERR_ARG, "cn_visual_images: null normal with a normal_img output");
    CN_REQUIRE(!flow_img || flow, CN_ERR_ARG, "cn_visual_images: null flow with a flow_img output");
    const uintptr_t all4 = (uintptr_t)rgb | (uintptr_t)depth | (uintptr_t)depth_max_w | (uintptr_t)weighted_z |
                           (uintptr_t)normal | (uintptr_t)flow | (uintptr_t)stats;
    CN_REQUIRE((all4 & 3) == 0, CN_ERR_ALIGN, "cn_visual_images: every fp32 array 4-byte aligned");
    const int HW = H * W;
    hipStream_t st = (hipStream_t)stream;
    ImageArgs a{HW, rgb, depth, depth_max_w, weighted_z, normal, flow, nullptr, stats, img, disparity, disparity_hw, normal_img,
                flow_img};
    if (stats) {
        const size_t need = cn_visual_images_workspace_bytes(H, W);
        CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
                   "cn_visual_images: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
        CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_visual_images: workspace not 256-byte aligned");
        a.part = static_cast<float*>(workspace);
        const int blocks = (int)stat_blocks(HW);
        image_stats_kernel<<<dim3((unsigned)blocks), 256, 0, st>>>(a);
        if (int rc = check_launch("cn_visual_images (statistics)")) return rc;
        image_stats_reduce_kernel<<<1, 64, 0, st>>>(a.part, blocks, stats);
        if (int rc = check_launch("cn_visual_images (reduce)")) return rc;
    }
    if (!(img || disparity || disparity_hw || normal_img || flow_img)) return CN_OK;
    image_map_kernel<<<dim3((unsigned)(((int64_t)HW + 255) / 256)), 256, 0, st>>>(a);
    return check_launch("cn_visual_images");
}
