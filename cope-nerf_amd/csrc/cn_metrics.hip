// cn_metrics.hip — the evaluation metrics (ABI v18).
//
// cn_image_metrics: co3d_metric.py's psnr / ssim (lines 14-48) for N x C (image, channel) jobs in one fused
// pass, instead of five depthwise 11 x 11 convolutions and about fifteen full-image elementwise launches per
// pair.  One workgroup per 64 x 16 output tile of one job:
//   1. the tile and its 5-pixel halo of both images go to LDS once (74 x 26 floats each; pixels outside the
//      image are the convolution's zero padding) -- each input pixel is read 74 * 26 / (64 * 16) = 1.88 times;
//   2. row pass: the 11 taps along x of the five moment images x, y, x x, y y, x y, for the 26 rows, into LDS;
//   3. column pass: the 11 taps along y; then the SSIM expression (co3d_metric.py:32-43, fp32, no clamping)
//      and (x - y)^2 on the same pixels.
// A wavefront always works on 64 consecutive floats of one LDS row (ds_read_b32 / ds_write_b32 bank = dword
// address mod 32 within a 32-lane half: consecutive lanes never share a bank), so no pass has a bank conflict
// and no row needs padding.  Nothing intermediate goes to global memory.
//
// cn_depth_errors: the seven depth errors of train.py:180-193 after the nearest-neighbour resize, the scale
// by a device scalar and the optional clamp of eval.py:233-240 (training.py:126-154 without the clamp).
//
// Both: a workgroup's sums are one fp32 partial (lanes by shuffles, then waves 0..3 in order), and a second
// kernel sums a job's partials in a fixed order in double and rounds once.  No atomics: bitwise
// reproducible, and a job's result does not depend on the other jobs of the launch.
#include "cn_mfma.h"

namespace cn {
namespace {

constexpr int kTileW = 64;                  // columns per tile: one wavefront's lanes
constexpr int kTileH = 16;                  // four rows for each of the four wavefronts
constexpr int kWin = 11;                    // the only window
constexpr int kHalo = kWin / 2;
constexpr int kInW = kTileW + 2 * kHalo;    // 74
constexpr int kInH = kTileH + 2 * kHalo;    // 26
constexpr int kDepthPerBlock = 2048;        // ground-truth pixels per workgroup of cn_depth_errors
constexpr size_t kAlign = 256;

struct ImageArgs {
    int H, W, tiles_x, tiles;
    const float* pred;   // [jobs][H][W]
    const float* gt;     // [jobs][H][W]
    float* ssim_map;     // [jobs][H][W] or null
    float* part;         // [jobs][tiles][2]: sum (x - y)^2, sum ssim
    float w[kWin];
};

__global__ void __launch_bounds__(256) image_metrics_kernel(ImageArgs a) {
    __shared__ float sx[kInH * kInW];
    __shared__ float sy[kInH * kInW];
    __shared__ float mom[5][kInH * kTileW];
    __shared__ float red[4 * 2];
    const int job = blockIdx.y, tile = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int H = a.H, W = a.W;
    const int x0 = (tile % a.tiles_x) * kTileW, y0 = (tile / a.tiles_x) * kTileH;
    const int64_t base = (int64_t)job * H * W;
    const float* __restrict__ px = a.pred + base;
    const float* __restrict__ py = a.gt + base;

    // 1. the tile with its halo; zero outside the image
    for (int i = tid; i < kInH * kInW; i += 256) {
        const int r = i / kInW, c = i - r * kInW;
        const int gy = y0 - kHalo + r, gx = x0 - kHalo + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const int o = in ? gy * W + gx : 0;
        sx[i] = in ? px[o] : 0.0f;
        sy[i] = in ? py[o] : 0.0f;
    }
    __syncthreads();

    // 2. row pass: a wavefront takes the 64 columns of one row per step; taps in ascending order
    for (int i = tid; i < kInH * kTileW; i += 256) {
        const int r = i >> 6, c = i & 63;
        const float* rx = sx + r * kInW + c;
        const float* ry = sy + r * kInW + c;
        float m0 = 0.0f, m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const float xv = rx[k], yv = ry[k], wk = a.w[k];
            m0 += wk * xv;
            m1 += wk * yv;
            m2 += wk * (xv * xv);
            m3 += wk * (yv * yv);
            m4 += wk * (xv * yv);
        }
        mom[0][i] = m0;
        mom[1][i] = m1;
        mom[2][i] = m2;
        mom[3][i] = m3;
        mom[4][i] = m4;
    }
    __syncthreads();

    // 3. column pass: lane = column, the wavefront's four consecutive rows share their 14 input rows
    const int r0 = wave * 4;
    float out[5][4];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        float v[kWin + 3];
#pragma unroll
        for (int k = 0; k < kWin + 3; ++k) v[k] = mom[m][(r0 + k) * kTileW + lane];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < kWin; ++k) s += a.w[k] * v[o + k];
            out[m][o] = s;
        }
    }
    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
    float se = 0.0f, ss = 0.0f;
    const int gx = x0 + lane;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = y0 + r0 + o;
        if (gx < W && gy < H) {
            const float mu1 = out[0][o], mu2 = out[1][o];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
            const float s1 = out[2][o] - mu1_sq, s2 = out[3][o] - mu2_sq, s12 = out[4][o] - mu1_mu2;
            const float v = ((2.0f * mu1_mu2 + C1) * (2.0f * s12 + C2)) /
                            (((mu1_sq + mu2_sq) + C1) * ((s1 + s2) + C2));
            if (a.ssim_map) a.ssim_map[base + (int64_t)gy * W + gx] = v;
            ss += v;
            const int li = (r0 + o + kHalo) * kInW + lane + kHalo;
            const float d = sx[li] - sy[li];
            se += d * d;
        }
    }
    // the tile's partial: lanes by shuffles, then waves 0..3 in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        se += __shfl_xor(se, o, 64);
        ss += __shfl_xor(ss, o, 64);
    }
    if (lane == 0) {
        red[wave * 2] = se;
        red[wave * 2 + 1] = ss;
    }
    __syncthreads();
    if (tid < 2)
        a.part[((int64_t)job * a.tiles + tile) * 2 + tid] = ((red[tid] + red[2 + tid]) + red[4 + tid]) + red[6 + tid];
}

// out[job][0..1] = (sum over the job's tiles) / (H W): one wavefront per job, lane l takes tiles l, l + 64, ...
// in double, then the lanes by shuffles; rounded to fp32 once.
__global__ void __launch_bounds__(64) image_reduce_kernel(const float* part, int tiles, double count, float* out) {
    const int job = blockIdx.x, lane = threadIdx.x;
    const float* p = part + (int64_t)job * tiles * 2;
    double s0 = 0.0, s1 = 0.0;
    for (int t = lane; t < tiles; t += 64) {
        s0 += (double)p[2 * (int64_t)t];
        s1 += (double)p[2 * (int64_t)t + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
    }
    if (lane == 0) {
        out[(int64_t)job * 2] = (float)(s0 / count);
        out[(int64_t)job * 2 + 1] = (float)(s1 / count);
    }
}

struct DepthArgs {
    int Hg, Wg, Hp, Wp, blocks, clamp;
    const float* gt;      // [N][Hg][Wg]
    const float* pred;    // [N][Hp][Wp]
    const float* ratio;   // [N]
    float min_depth, max_depth;
    float* part;          // [N][blocks][8]
};

__global__ void __launch_bounds__(256) depth_errors_kernel(DepthArgs a) {
    __shared__ float red[4 * 8];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int HW = a.Hg * a.Wg;
    const float* __restrict__ g = a.gt + (int64_t)n * HW;
    const float* __restrict__ p = a.pred + (int64_t)n * a.Hp * a.Wp;
    const float ratio = a.ratio[n];
    // abs_rel, sq_rel, sq, sq_log, a1, a2, a3, count: at most 8 pixels per lane, so the four counts are exact
    float acc[8] = {};
    const int64_t first = (int64_t)blockIdx.x * kDepthPerBlock;
#pragma unroll
    for (int k = 0; k < kDepthPerBlock / 256; ++k) {
        const int64_t i = first + k * 256 + tid;
        if (i >= HW) break;
        const float gv = g[i];
        if (!(gv >= a.min_depth && gv <= a.max_depth)) continue;
        const int y = (int)(i / a.Wg), x = (int)(i - (int64_t)y * a.Wg);
        const int sy = (int)((int64_t)y * a.Hp / a.Hg), sx = (int)((int64_t)x * a.Wp / a.Wg);
        float pv = p[(int64_t)sy * a.Wp + sx] * ratio;
        if (a.clamp) {  // eval.py:239-240 (a NaN stays)
            if (pv < a.min_depth) pv = a.min_depth;
            if (pv > a.max_depth) pv = a.max_depth;
        }
        const float q0 = gv / pv, q1 = pv / gv;
        const float thresh = q0 > q1 ? q0 : q1;
        const float d = gv - pv, sq = d * d;
        const float dl = logf(gv) - logf(pv);
        acc[0] += fabsf(d) / gv;
        acc[1] += sq / gv;
        acc[2] += sq;
        acc[3] += dl * dl;
        acc[4] += thresh < 1.25f ? 1.0f : 0.0f;
        acc[5] += thresh < 1.5625f ? 1.0f : 0.0f;
        acc[6] += thresh < 1.953125f ? 1.0f : 0.0f;
        acc[7] += 1.0f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += __shfl_xor(acc[i], o, 64);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 8; ++i) red[wave * 8 + i] = acc[i];
    __syncthreads();
    if (tid < 8)
        a.part[((int64_t)n * a.blocks + blockIdx.x) * 8 + tid] =
            ((red[tid] + red[8 + tid]) + red[16 + tid]) + red[24 + tid];
}

// one wavefront per image: the eight sums over its workgroups in double (every count is an integer far
// below 2^53: exact), then the seven errors and the count, each rounded to fp32 once.  A zero count: 0 / 0.
__global__ void __launch_bounds__(64) depth_reduce_kernel(const float* part, int blocks, float* out) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const float* p = part + (int64_t)n * blocks * 8;
    double s[8] = {};
    for (int b = lane; b < blocks; b += 64)
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] += (double)p[(int64_t)b * 8 + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] += __shfl_xor(s[i], o, 64);
    if (lane == 0) {
        float* r = out + (int64_t)n * 8;
        const double cnt = s[7];
        r[0] = (float)(s[0] / cnt);
        r[1] = (float)(s[1] / cnt);
        r[2] = (float)sqrt(s[2] / cnt);
        r[3] = (float)sqrt(s[3] / cnt);
        r[4] = (float)(s[4] / cnt);
        r[5] = (float)(s[5] / cnt);
        r[6] = (float)(s[6] / cnt);
        r[7] = (float)cnt;
    }
}

// in 64 bits: H or W near 2^31 must reach the shape check, not wrap in the rounding
int64_t image_tiles(int H, int W) {
    return (((int64_t)W + kTileW - 1) / kTileW) * (((int64_t)H + kTileH - 1) / kTileH);
}

int image_shape_check(const char* who, int N, int C, int H, int W) {
    CN_REQUIRE(N >= 0 && C >= 1 && H >= 1 && W >= 1, CN_ERR_SHAPE, "%s: %d images of %d x %d x %d (each at least 1)",
               who, N, C, H, W);
    CN_REQUIRE((int64_t)N * C <= 65535, CN_ERR_SHAPE, "%s: %lld (image, channel) jobs (0 .. 65535)", who,
               (long long)N * C);
    // offsets inside one plane are 32-bit; the plane's base offset in the stack is 64-bit
    CN_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), CN_ERR_SHAPE, "%s: planes of %d x %d too large (H W must stay below 2^31)",
               who, H, W);
    // one workgroup of 256 threads per tile along the grid's x: its thread count must fit 32 bits
    CN_REQUIRE(image_tiles(H, W) < ((int64_t)1 << 24), CN_ERR_SHAPE,
               "%s: planes of %d x %d give %lld tiles, more than the grid holds (below 2^24)", who, H, W,
               (long long)image_tiles(H, W));
    return CN_OK;
}

int64_t depth_blocks(int Hg, int Wg) { return ((int64_t)Hg * Wg + kDepthPerBlock - 1) / kDepthPerBlock; }

int depth_shape_check(const char* who, int N, int Hg, int Wg) {
    CN_REQUIRE(N >= 0 && N <= 65535, CN_ERR_SHAPE, "%s: %d images (0 .. 65535)", who, N);
    CN_REQUIRE(Hg >= 1 && Wg >= 1, CN_ERR_SHAPE, "%s: ground truth of %d x %d (each at least 1)", who, Hg, Wg);
    CN_REQUIRE((int64_t)Hg * Wg < ((int64_t)1 << 31), CN_ERR_SHAPE,
               "%s: ground truth of %d x %d too large (Hg Wg must stay below 2^31)", who, Hg, Wg);
    return CN_OK;
}

// cn_normal_errors: the angle between two normal maps, per pixel and summed.
constexpr int kNormalPerBlock = 2048;  // pixels per workgroup
constexpr int kNormalMaxBlocks = 1024;

int normal_blocks(int64_t n) {
    int64_t b = (n + kNormalPerBlock - 1) / kNormalPerBlock;
    return (int)(b < 1 ? 1 : (b > kNormalMaxBlocks ? kNormalMaxBlocks : b));
}

struct NormalArgs {
    int64_t n;
    const float* pred;
    const float* gt;
    const uint8_t* mask;
    float* angle;
    double* part;  // [blocks][6]
};

__device__ __forceinline__ bool unit3(const float* __restrict__ v, float* o) {
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(len > 0.0f && len < INFINITY)) return false;
    o[0] = v[0] / len;
    o[1] = v[1] / len;
    o[2] = v[2] / len;
    return true;
}

// the sum over the block of one double per thread in a fixed tree (lanes by shuffles, then the four waves in order)
__device__ __forceinline__ double block_sum_d(double x, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = x + __shfl_down(x, o, 64);
    __syncthreads();  // (a previous call's readers are done)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// thread t of block b takes pixels (b 256 + t) + j (blocks 256), j ascending: angle = atan2(|p x g|, p . g) of the
// normalised vectors in fp32, in degrees (the radians scaled in double, rounded once); the six sums in double.
__global__ void __launch_bounds__(256) normal_errors_kernel(NormalArgs a) {
    __shared__ double sh[4];
    const int64_t stride = (int64_t)gridDim.x * 256;
    double s[6] = {};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {  // bound: ceil(n / stride)
        float p[3], g[3], ang = NAN;
        if ((!a.mask || a.mask[i]) && unit3(a.pred + i * 3, p) && unit3(a.gt + i * 3, g)) {
            const float cx = p[1] * g[2] - p[2] * g[1], cy = p[2] * g[0] - p[0] * g[2], cz = p[0] * g[1] - p[1] * g[0];
            const float cr = sqrtf((cx * cx + cy * cy) + cz * cz);
            const float dt = (p[0] * g[0] + p[1] * g[1]) + p[2] * g[2];
            ang = (float)((double)atan2f(cr, dt) * 57.29577951308232);
            s[0] += 1.0;
            s[1] = s[1] + (double)ang;
            s[2] = s[2] + (double)ang * (double)ang;
            s[3] += ang < 11.25f ? 1.0 : 0.0;
            s[4] += ang < 22.5f ? 1.0 : 0.0;
            s[5] += ang < 30.0f ? 1.0 : 0.0;
        }
        a.angle[i] = ang;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double r = block_sum_d(s[k], sh);
        if (threadIdx.x == 0) a.part[(int64_t)blockIdx.x * 6 + k] = r;
    }
}

// one block: the block partials, thread t takes blocks t, t + 256, ...
__global__ void __launch_bounds__(256) normal_reduce_kernel(int nb, const double* __restrict__ part, double* __restrict__ out) {
    __shared__ double sh[4];
    double s[6] = {};
    for (int b = threadIdx.x; b < nb; b += 256)  // bound: ceil(nb / 256) <= 4
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = s[k] + part[(int64_t)b * 6 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double r = block_sum_d(s[k], sh);
        if (threadIdx.x == 0) out[k] = r;
    }
}

size_t round_up(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" size_t cn_image_metrics_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (image_shape_check("cn_image_metrics_workspace_bytes", N, C, H, W) != CN_OK) return 0;
    return round_up((size_t)N * C * (size_t)image_tiles(H, W) * 2 * sizeof(float));
}

extern "C" int cn_image_metrics(int32_t N, int32_t C, int32_t H, int32_t W, const float* pred, const float* gt,
                                const float* taps, float* out, float* ssim_map, void* workspace,
                                int64_t workspace_bytes, cn_stream_t stream) {
    if (int rc = image_shape_check("cn_image_metrics", N, C, H, W)) return rc;
    if (N == 0) return CN_OK;
    CN_REQUIRE(pred && gt && taps && out, CN_ERR_ARG, "cn_image_metrics: null pred / gt / taps / out");
    const uintptr_t all4 = (uintptr_t)pred | (uintptr_t)gt | (uintptr_t)taps | (uintptr_t)out | (uintptr_t)ssim_map;
    CN_REQUIRE((all4 & 3) == 0, CN_ERR_ALIGN, "cn_image_metrics: every array 4-byte aligned");
    const size_t need = cn_image_metrics_workspace_bytes(N, C, H, W);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_image_metrics: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN,
               "cn_image_metrics: workspace not 256-byte aligned");
    const int64_t tiles = image_tiles(H, W);
    const int jobs = N * C;
    hipStream_t st = (hipStream_t)stream;
    ImageArgs a{H, W, cdiv(W, kTileW), (int)tiles, pred, gt, ssim_map, static_cast<float*>(workspace), {}};
    for (int k = 0; k < kWin; ++k) a.w[k] = taps[k];
    image_metrics_kernel<<<dim3((unsigned)tiles, (unsigned)jobs), 256, 0, st>>>(a);
    if (int rc = check_launch("cn_image_metrics")) return rc;
    image_reduce_kernel<<<dim3((unsigned)jobs), 64, 0, st>>>(a.part, (int)tiles, (double)H * (double)W, out);
    return check_launch("cn_image_metrics (reduce)");
}

extern "C" size_t cn_depth_errors_workspace_bytes(int32_t N, int32_t Hg, int32_t Wg) {
    if (depth_shape_check("cn_depth_errors_workspace_bytes", N, Hg, Wg) != CN_OK) return 0;
    return round_up((size_t)N * (size_t)depth_blocks(Hg, Wg) * 8 * sizeof(float));
}

extern "C" int cn_depth_errors(int32_t N, int32_t Hg, int32_t Wg, const float* gt, int32_t Hp, int32_t Wp,
                               const float* pred, const float* ratio, float min_depth, float max_depth, int32_t clamp,
                               float* out, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    if (int rc = depth_shape_check("cn_depth_errors", N, Hg, Wg)) return rc;
    CN_REQUIRE(Hp >= 1 && Wp >= 1 && (int64_t)Hp * Wp < ((int64_t)1 << 31), CN_ERR_SHAPE,
               "cn_depth_errors: prediction of %d x %d (each at least 1, Hp Wp below 2^31)", Hp, Wp);
    if (N == 0) return CN_OK;
    CN_REQUIRE(gt && pred && ratio && out, CN_ERR_ARG, "cn_depth_errors: null gt / pred / ratio / out");
    const uintptr_t all4 = (uintptr_t)gt | (uintptr_t)pred | (uintptr_t)ratio | (uintptr_t)out;
    CN_REQUIRE((all4 & 3) == 0, CN_ERR_ALIGN, "cn_depth_errors: every array 4-byte aligned");
    const size_t need = cn_depth_errors_workspace_bytes(N, Hg, Wg);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_depth_errors: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN,
               "cn_depth_errors: workspace not 256-byte aligned");
    const int blocks = (int)depth_blocks(Hg, Wg);
    hipStream_t st = (hipStream_t)stream;
    DepthArgs a{Hg, Wg, Hp, Wp, blocks, clamp, gt, pred, ratio, min_depth, max_depth, static_cast<float*>(workspace)};
    depth_errors_kernel<<<dim3((unsigned)blocks, (unsigned)N), 256, 0, st>>>(a);
    if (int rc = check_launch("cn_depth_errors")) return rc;
    depth_reduce_kernel<<<dim3((unsigned)N), 64, 0, st>>>(a.part, blocks, out);
    return check_launch("cn_depth_errors (reduce)");
}

extern "C" size_t cn_normal_errors_workspace_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31)) return 0;
    return round_up((size_t)normal_blocks(n) * 6 * sizeof(double));
}

extern "C" int cn_normal_errors(int64_t n, const float* pred, const float* gt, const uint8_t* mask, float* angle, double* out,
                                void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    CN_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), CN_ERR_SHAPE, "cn_normal_errors: n %lld (in [0, 2^31))", (long long)n);
    CN_REQUIRE(out && (n == 0 || (pred && gt && angle)), CN_ERR_ARG, "cn_normal_errors: null pred / gt / angle / out");
    CN_REQUIRE((((uintptr_t)pred | (uintptr_t)gt | (uintptr_t)angle) & 3) == 0 && ((uintptr_t)out & 7) == 0, CN_ERR_ALIGN,
               "cn_normal_errors: pred / gt / angle 4-byte, out 8-byte aligned");
    const size_t need = cn_normal_errors_workspace_bytes(n);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_normal_errors: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_normal_errors: workspace not 256-byte aligned");
    const int nb = normal_blocks(n);
    hipStream_t st = (hipStream_t)stream;
    NormalArgs a{n, pred, gt, mask, angle, static_cast<double*>(workspace)};
    normal_errors_kernel<<<nb, 256, 0, st>>>(a);
    if (int rc = check_launch("cn_normal_errors")) return rc;
    normal_reduce_kernel<<<1, 256, 0, st>>>(nb, a.part, out);
    return check_launch("cn_normal_errors (reduce)");
}
