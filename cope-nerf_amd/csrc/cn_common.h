// cn_common.h — shared definitions for the cope-nerf MI355X (gfx950) kernels.
//
// Error model (include/copenerf.h): every extern "C" entry point validates its
// arguments on the host, launches on the caller's stream and returns 0 or a
// negative cn_status.  The message of the last failure on the calling thread is
// kept in a thread_local buffer (cn_last_error).  No entry point allocates,
// synchronises or touches the default stream, so a caller may capture any
// sequence of them into a hipGraph.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdarg>

#include "../../include/copenerf.h"

namespace cn {

void set_error(const char* fmt, ...);

// Check a launch; converts a HIP launch error into CN_ERR_LAUNCH.
int check_launch(const char* what);

typedef float floatx4 __attribute__((ext_vector_type(4)));

// Column group g (4 columns) of the SDF positional encoding of x' = scale * x (neus_embedder.py:17-36:
// include_input, log bands, periodic_fns [sin, cos], d = 4): g 0 = x', g 1 + 2k = sin(2^k x'), g 2 + 2k
// = cos(2^k x') for k < L, zero for g >= 1 + 2L.  The one definition of the encoding: cn_sdf_embed and
// the first layer's fused operand load (cn_linear with emb_x) give the same bits.
__device__ __forceinline__ floatx4 sdf_embed_group(floatx4 xv, int g, int L, float scale) {
    floatx4 xs, o = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < 4; ++c) xs[c] = xv[c] * scale;
    if (g == 0) {
        o = xs;
    } else if (g < 1 + 2 * L) {
        const int k = (g - 1) >> 1;
        const float f = (float)(1 << k);
        const bool is_sin = ((g - 1) & 1) == 0;
        for (int c = 0; c < 4; ++c) {
            const float t = xs[c] * f;
            o[c] = is_sin ? sinf(t) : cosf(t);
        }
    }
    return o;
}
typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;

__device__ __forceinline__ float sigmoidf_ref(float x) {
    // torch CPU sigmoid: 1 / (1 + exp(-x))
    return 1.0f / (1.0f + expf(-x));
}

// torch.nn.Softplus(beta, threshold): x if x*beta > threshold else log1p(exp(x*beta))/beta
__device__ __forceinline__ float softplus_ref(float x, float beta, float thr) {
    const float bx = x * beta;
    return bx > thr ? x : log1pf(expf(bx)) / beta;
}

// torch softplus_backward factor: 1 if x*beta > threshold else e/(e+1), e = exp(x*beta).
// For x*beta > ~16.6 the fp32 value is exactly 1, so the threshold branch and the
// sigmoid agree bit for bit; we keep torch's form.
__device__ __forceinline__ float softplus_grad_ref(float x, float beta, float thr) {
    const float bx = x * beta;
    if (bx > thr) return 1.0f;
    const float e = expf(bx);
    return e / (e + 1.0f);
}

__host__ __device__ __forceinline__ int cdiv(int a, int b) { return (a + b - 1) / b; }

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123
// constants): ten rounds of two 32x32 -> 64-bit multiplies, the key bumped by the Weyl constants between rounds.
// Shared by cn_uniform_philox (cn_render.hip) and the surface sampler (cn_mesh_eval.hip).
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
    }
}

// The integer scans of the mesher (cn_mesh.hip) and of the point grid (cn_mesh_eval.hip): 256 threads of
// 4 elements, reduce per 1024-element tile, one block scans the tile totals, a third launch adds back.
constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;
constexpr int kScanTile = kScanThreads * kScanItems;  // elements per block of the reduce / add-back launches

__device__ __forceinline__ int wave_incl_scan_add_i(int x, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

// Exclusive scan of one value per thread over the block's 256 threads; *total = the block's sum.
__device__ __forceinline__ int block_excl_scan(int x, int* total) {
    __shared__ int wsum[kScanThreads / kWave];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int incl = wave_incl_scan_add_i(x, lane);
    __syncthreads();  // (a previous round's readers are done)
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kScanThreads / kWave; ++i) {
        if (i < w) before += wsum[i];
        all += wsum[i];
    }
    *total = all;
    return before + incl - x;
}

// The fixed-order double reductions of the cloud statistics (cn_mesh_eval.hip, cn_cloud.hip): launch 1 of
// stats_blocks(Q) blocks of 256 threads, thread t of block b taking elements (b 256 + t) + j (blocks 256), a fixed
// tree per block; launch 2 of one block over the block partials.
constexpr int kStatsThreads = 256;
constexpr int kStatsMaxBlocks = 1024;

inline int stats_blocks(int64_t Q) {
    int64_t b = (Q + 1023) / 1024;
    return (int)(b < 1 ? 1 : (b > kStatsMaxBlocks ? kStatsMaxBlocks : b));
}

// the sum over the block of one value per thread, in a fixed tree; valid in thread 0
__device__ __forceinline__ double block_sum_fixed(double x, double* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = x + __shfl_down(x, off, kWave);
    __syncthreads();  // (a previous call's readers are done)
    if (lane == 0) sh[w] = x;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kStatsThreads / kWave; ++i) s = s + sh[i];
    return s;
}

// grid_sample's border clip of an unnormalised coordinate (GridSampler.h clip_coordinates_set_grad):
// the clamped coordinate, *mult = 0 where it was clamped (the borders count as clamped).  Shared by the
// two bilinear warps (cn_refine.hip, cn_flow_rgb.hip).
__device__ __forceinline__ float clip_border(float x, float maxv, float* mult) {
    if (!(x > 0.0f)) {  // (a NaN coordinate samples texel 0, as fmax(x, 0))
        *mult = 0.0f;
        return 0.0f;
    }
    if (x >= maxv) {
        *mult = 0.0f;
        return maxv;
    }
    *mult = 1.0f;
    return x;
}

}  // namespace cn

#define CN_REQUIRE(cond, code, ...)           \
    do {                                      \
        if (!(cond)) {                        \
            ::cn::set_error(__VA_ARGS__);     \
            return (code);                    \
        }                                     \
    } while (0)
