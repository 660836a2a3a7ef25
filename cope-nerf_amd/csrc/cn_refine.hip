// cn_refine.hip — the pose-refinement photometric pass (ABI v17): compute_loss_and_warp_image
// (utils_poses/pose_refinement.py:34-61) for J (target, source) jobs over one image stack, forward and
// the pose gradient in the same pass, instead of a dozen full-image torch launches each way:
//
//   per pixel (row i, column c) of the target frame, with its depth d
//     (u, v)  = (c / ((W-1)/2) - 1, i / ((H-1)/2) - 1)          pose_refinement.py:93-100
//     X = Kinv (u d, v d, d),  Y = R X + t,  q = K Y,  (u', v') = (q0, q1) / q2
//     valid   = u', v' in [-1, 1]                                pose_refinement.py:50-53
//     warp    = grid_sample(source, (u', v'), bilinear, border, align_corners=True)   train.py:235-244
//   sums[j]  = (sum over valid pixels and channels of |warp - target|, number of valid pixels)
//   dpose[j] = d sums[j][0] / d (R | t): sign(warp - target) through the bilinear derivative (zero
//              where the coordinate is clamped, as torch's), the projection and K.
//
// One workgroup per 64 x 16 pixel tile of one job: a wavefront takes 64 consecutive columns of a row (the
// target and depth loads coalesce, the four taps of neighbouring lanes fall in the same two source rows),
// the four wavefronts take four consecutive rows, four times.  The 14 sums of a tile are a per-workgroup
// partial (wave shuffles, then the four waves in order through LDS); slab_reduce_kernel sums a job's tiles
// in a fixed order.  No atomics: bitwise reproducible, and a job's result does not depend on the other
// jobs of the launch.
#include "cn_mfma.h"

namespace cn {
namespace {

constexpr int kTileW = 64;          // columns per tile: one wavefront's lanes
constexpr int kRowsPerWave = 4;
constexpr int kTileH = 4 * kRowsPerWave;
constexpr int kPart = 16;           // floats per (tile, job) partial: dpose 12, sums 2, 2 unused
constexpr size_t kAlign = 256;

struct RefineArgs {
    int N, H, W, J;
    const float* images;   // [N][3][H][W]
    const float* depth;    // [N][H][W]
    const int32_t* tgt;    // [J]
    const int32_t* src;    // [J]
    const float* pose;     // [J][12]
    const float* K;        // [J][9]
    const float* Kinv;     // [J][9]
    float* warped;         // [J][3][H][W] or null
    float* part;           // [tiles][J][kPart]
    int tiles_x;
};

__global__ void __launch_bounds__(256) refine_warp_kernel(RefineArgs a) {
    __shared__ float smem[4 * 14];
    const int j = blockIdx.y;
    const int tile = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (tile % a.tiles_x) * kTileW + lane;
    const int row0 = (tile / a.tiles_x) * kTileH + wave;
    const int H = a.H, W = a.W, HW = H * W;
    const int it = a.tgt[j], is = a.src[j];
    // an index outside the stack: the job reads nothing and sums to zero
    const bool job_ok = it >= 0 && it < a.N && is >= 0 && is < a.N;
    float acc[14] = {};  // dR (9, row-major) and dt (3) as pose[12] = [R | t] rows; then sum |.|, count
    if (job_ok && col < W) {
        float P[12], Km[9], Ki[9];
#pragma unroll
        for (int i = 0; i < 12; ++i) P[i] = a.pose[(int64_t)j * 12 + i];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            Km[i] = a.K[(int64_t)j * 9 + i];
            Ki[i] = a.Kinv[(int64_t)j * 9 + i];
        }
        const float* __restrict__ tg = a.images + (int64_t)it * 3 * HW;
        const float* __restrict__ sr = a.images + (int64_t)is * 3 * HW;
        const float* __restrict__ dp = a.depth + (int64_t)it * HW;
        float* wo = a.warped ? a.warped + (int64_t)j * 3 * HW : nullptr;
        const float hw = (float)(W - 1) * 0.5f, hh = (float)(H - 1) * 0.5f;
        const float xmax = (float)(W - 1), ymax = (float)(H - 1);
        const float u = (float)col / hw - 1.0f;
#pragma unroll
        for (int k = 0; k < kRowsPerWave; ++k) {
            const int row = row0 + 4 * k;
            if (row >= H) break;
            const int p = row * W + col;
            const float d = dp[p];
            const float v = (float)row / hh - 1.0f;
            const float ud = u * d, vd = v * d;
            const float X0 = (Ki[0] * ud + Ki[1] * vd) + Ki[2] * d;
            const float X1 = (Ki[3] * ud + Ki[4] * vd) + Ki[5] * d;
            const float X2 = (Ki[6] * ud + Ki[7] * vd) + Ki[8] * d;
            const float Y0 = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3];
            const float Y1 = ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7];
            const float Y2 = ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11];
            const float q0 = (Km[0] * Y0 + Km[1] * Y1) + Km[2] * Y2;
            const float q1 = (Km[3] * Y0 + Km[4] * Y1) + Km[5] * Y2;
            const float q2 = (Km[6] * Y0 + Km[7] * Y1) + Km[8] * Y2;
            const float up = q0 / q2, vp = q1 / q2;
            const bool valid = up >= -1.0f && up <= 1.0f && vp >= -1.0f && vp <= 1.0f;
            if (!valid && !wo) continue;  // contributes nothing
            // grid_sample: unnormalise (align_corners), clip to the border, the four taps
            float mx, my;
            const float x = clip_border((up + 1.0f) * 0.5f * xmax, xmax, &mx);
            const float y = clip_border((vp + 1.0f) * 0.5f * ymax, ymax, &my);
            const float xf = floorf(x), yf = floorf(y);
            const int x0 = (int)xf, y0 = (int)yf;  // in [0, W-1] x [0, H-1] after the clip
            const bool hx = x0 + 1 < W, hy = y0 + 1 < H;  // the east / south taps are inside the image
            const float fx1 = x - xf, fx0 = (xf + 1.0f) - x;  // weights of the east / west columns
            const float fy1 = y - yf, fy0 = (yf + 1.0f) - y;
            const float wnw = fx0 * fy0, wne = fx1 * fy0, wsw = fx0 * fy1, wse = fx1 * fy1;
            const int o00 = y0 * W + x0;
            const int o01 = hx ? o00 + 1 : o00, o10 = hy ? o00 + W : o00, o11 = o10 + (hx ? 1 : 0);
            float gx = 0.0f, gy = 0.0f, sabs = 0.0f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float* s = sr + ch * HW;
                const float nw = s[o00];
                const float ne = hx ? s[o01] : 0.0f;
                const float sw = hy ? s[o10] : 0.0f;
                const float se = (hx && hy) ? s[o11] : 0.0f;
                const float wv = ((nw * wnw + ne * wne) + sw * wsw) + se * wse;
                if (wo) wo[ch * HW + p] = wv;
                if (valid) {
                    const float e = wv - tg[ch * HW + p];
                    sabs += fabsf(e);
                    const float sg = e > 0.0f ? 1.0f : (e < 0.0f ? -1.0f : 0.0f);
                    // d wv / dx, d wv / dy (grid_sampler_2d_backward's tap order)
                    gx += sg * (((ne * fy0 - nw * fy0) - sw * fy1) + se * fy1);
                    gy += sg * (((sw * fx0 - nw * fx0) - ne * fx1) + se * fx1);
                }
            }
            if (!valid) continue;
            acc[12] += sabs;
            acc[13] += 1.0f;
            const float gu = gx * mx * (xmax * 0.5f), gv = gy * my * (ymax * 0.5f);  // d / du', d / dv'
            const float dq0 = gu / q2, dq1 = gv / q2;
            const float dq2 = -(gu * up + gv * vp) / q2;
            const float dY0 = (Km[0] * dq0 + Km[3] * dq1) + Km[6] * dq2;
            const float dY1 = (Km[1] * dq0 + Km[4] * dq1) + Km[7] * dq2;
            const float dY2 = (Km[2] * dq0 + Km[5] * dq1) + Km[8] * dq2;
            acc[0] += dY0 * X0; acc[1] += dY0 * X1; acc[2] += dY0 * X2; acc[3] += dY0;
            acc[4] += dY1 * X0; acc[5] += dY1 * X1; acc[6] += dY1 * X2; acc[7] += dY1;
            acc[8] += dY2 * X0; acc[9] += dY2 * X1; acc[10] += dY2 * X2; acc[11] += dY2;
        }
    }
    // the tile's partial: lanes by shuffles, then waves 0..3 in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < 14; ++i) acc[i] += __shfl_xor(acc[i], o, 64);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < 14; ++i) smem[wave * 14 + i] = acc[i];
    __syncthreads();
    if (threadIdx.x < 14) {
        const int i = threadIdx.x;
        a.part[((int64_t)tile * a.J + j) * kPart + i] = ((smem[i] + smem[14 + i]) + smem[28 + i]) + smem[42 + i];
    }
}

int shape_check(const char* who, int J, int H, int W) {
    CN_REQUIRE(J >= 0 && J <= 65535, CN_ERR_SHAPE, "%s: %d jobs (0 .. 65535)", who, J);
    CN_REQUIRE(H >= 2 && W >= 2, CN_ERR_SHAPE, "%s: frames of %d x %d (each at least 2)", who, H, W);
    // offsets inside one frame (3 planes) are 32-bit; the frame's base offset in the stack is 64-bit
    CN_REQUIRE((int64_t)H * W * 3 < ((int64_t)1 << 31), CN_ERR_SHAPE,
               "%s: frames of %d x %d too large (3 H W must stay below 2^31)", who, H, W);
    return CN_OK;
}

int64_t tiles_of(int H, int W) { return (int64_t)cdiv(W, kTileW) * cdiv(H, kTileH); }

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" size_t cn_refine_workspace_bytes(int32_t J, int32_t H, int32_t W) {
    if (shape_check("cn_refine_workspace_bytes", J, H, W) != CN_OK) return 0;
    const size_t b = (size_t)tiles_of(H, W) * (size_t)J * kPart * sizeof(float);
    return (b + kAlign - 1) / kAlign * kAlign;
}

extern "C" int cn_refine_warp(int32_t N, int32_t H, int32_t W, int32_t J, const float* images, const float* depth,
                              const int32_t* tgt, const int32_t* src, const float* pose, const float* K,
                              const float* Kinv, float* sums, float* dpose, float* warped, void* workspace,
                              int64_t workspace_bytes, cn_stream_t stream) {
    if (int rc = shape_check("cn_refine_warp", J, H, W)) return rc;
    CN_REQUIRE(N >= 1, CN_ERR_SHAPE, "cn_refine_warp: a stack of %d frames", N);
    if (J == 0) return CN_OK;
    CN_REQUIRE(images && depth && tgt && src && pose && K && Kinv, CN_ERR_ARG,
               "cn_refine_warp: null images / depth / tgt / src / pose / K / Kinv");
    CN_REQUIRE(sums && dpose, CN_ERR_ARG, "cn_refine_warp: null sums / dpose");
    const uintptr_t all4 = (uintptr_t)images | (uintptr_t)depth | (uintptr_t)tgt | (uintptr_t)src | (uintptr_t)pose |
                           (uintptr_t)K | (uintptr_t)Kinv | (uintptr_t)sums | (uintptr_t)warped;
    CN_REQUIRE((all4 & 3) == 0, CN_ERR_ALIGN, "cn_refine_warp: every array 4-byte aligned");
    CN_REQUIRE(al16(dpose), CN_ERR_ALIGN, "cn_refine_warp: dpose not 16-byte aligned");
    const size_t need = cn_refine_workspace_bytes(J, H, W);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_refine_warp: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_refine_warp: workspace not 256-byte aligned");
    const int64_t tiles = tiles_of(H, W);
    CN_REQUIRE(tiles < ((int64_t)1 << 31), CN_ERR_SHAPE, "cn_refine_warp: %lld tiles", (long long)tiles);
    hipStream_t st = (hipStream_t)stream;
    RefineArgs a{N, H, W, J, images, depth, tgt, src, pose, K, Kinv, warped, static_cast<float*>(workspace),
                 cdiv(W, kTileW)};
    refine_warp_kernel<<<dim3((unsigned)tiles, (unsigned)J), 256, 0, st>>>(a);
    if (int rc = check_launch("cn_refine_warp")) return rc;
    // per job: dpose from columns 0 .. 11 of its partials, sums from columns 12, 13, over the tiles in order
    const int64_t stride = (int64_t)J * kPart;
    return launch_slab_jobs(slab_job(a.part, (int)tiles, stride, J, 12, kPart, dpose, 12, 1.0f, 0),
                            slab_job(a.part + 12, (int)tiles, stride, J, 2, kPart, sums, 2, 1.0f, 0), st);
}
