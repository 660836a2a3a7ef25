// cn_lpips.hip — LPIPS (VGG16, v0.1 linear heads) of one image pair from user-supplied weights (ABI v20).
//
// The network (lpipsPyTorch/modules/{lpips,networks,utils}.py, restated): z-score per channel, the thirteen
// 3 x 3 convolutions (+ bias, ReLU) of VGG16 in five blocks with a 2 x 2 floor max-pool between blocks, the
// last activation of each block unit-normalised over its channels, and
//   sum over the blocks of mean over the pixels of sum_c lin[c] (fx^ - fy^)^2.
//
// A convolution is patches x weights on the existing GEMM (cn_linear, CN_EPI_RELU):
//   patches_kernel  writes the operand rows [n rows Wo][Kpad] of a band of output rows from the NHWC map
//                   [n][Hs][Ws][C] (column (dy 3 + dx) C + c = the source at (y + dy - 1, x + dx - 1, c),
//                   zero outside the map and in the columns [9 C, Kpad)).  Mode pool takes the 2 x 2 floor
//                   max-pool of the stored map on read (no pooled map is stored); mode first reads the two
//                   planar [3][H][W] images and z-scores them on read (a true fp32 division).  One 16-byte
//                   store per thread, 16-byte loads along c; row offsets are 64-bit.
//   cn_linear       [n rows Wo][Kpad] x [Cout][Kpad]^T + bias, ReLU: the rows of the next NHWC map.  Both
//                   images are one batch (n = 2): a weight image is read once per band.
// Only the patch matrix is banded; the maps are whole (two buffers, written alternately: the stream's order
// keeps a block's last map alive until its head has read it).  A GEMM row depends on its own operand row
// alone, so the result does not depend on the banding.
//
//   head_kernel     one block's term: L = min(64, C / 4) lanes per pixel, each lane 4 (C = 512: 8) channels
//                   of both images in registers; the two channel norms and the weighted squared difference
//                   by xor-shuffles inside the lane group (all its lanes end with the sum); a wavefront's
//                   pixels are added in ascending order, the lane groups by shuffles, waves 0..3 in order:
//                   one fp32 partial per workgroup of 64 pixels.
//   reduce_kernel   one wavefront: per block the partials in a fixed order in double, divided by the pixel
//                   count, rounded once; then the fp32 sum of the five terms in block order.
// No atomics: bitwise reproducible.  Identical images give identical maps, so every difference and every
// term is exactly 0.
#include "cn_common.h"

#include <algorithm>

namespace cn {
namespace {

constexpr int kConvs = 13, kTaps = 5;
constexpr int kCout[kConvs] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int kPooled[kConvs] = {0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0};   // reads the pooled previous map
constexpr int kTapOf[kConvs] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};
constexpr float kMean[3] = {-.030f, -.088f, -.188f};
constexpr float kStd[3] = {.458f, .448f, .450f};
constexpr int kMinSize = 16;                 // four pools: the last block still has a pixel
constexpr int64_t kMaxPixels = (int64_t)1 << 26;
// the library's band choice keeps the patch matrix within this: at 540 x 960 blocks 3 to 5 are one band each (a
// long-K GEMM of few rows takes as long as one that fills the chip), conv1_2 is four bands
constexpr size_t kPatchCap = (size_t)576 << 20;
constexpr int kHeadPix = 64;                 // pixels per workgroup of the head: 16 per wavefront
constexpr size_t kAlign = 256;

enum { kPlain = 0, kPool = 1, kFirst = 2 };

struct PatchArgs {
    const float* src;    // plain / pool: [n][Hst][Wst][C];  first: image 0 [3][Ho][Wo]
    const float* src1;   // first: image 1
    float* out;          // [n rows Wo][kpad]
    int n, Hst, Wst, Ho, Wo, C, logC, kpad, y0, rows;
};

template <int MODE>
__global__ void __launch_bounds__(256) patches_kernel(PatchArgs a) {
    const int K4 = a.kpad >> 2;
    const int64_t total = (int64_t)a.n * a.rows * a.Wo * K4;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += stride) {
        const int64_t m = idx / K4;
        const int k = (int)(idx - m * K4) * 4;
        const int64_t t = m / a.Wo;
        const int x = (int)(m - t * a.Wo);
        const int i = (int)(t / a.rows);
        const int y = a.y0 + (int)(t - (int64_t)i * a.rows);
        floatx4 v = {0.f, 0.f, 0.f, 0.f};
        if (MODE == kFirst) {
            const float* __restrict__ img = i ? a.src1 : a.src;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int kk = k + e;
                const int tap = kk / 3, c = kk - 3 * tap;
                const int dy = tap / 3, dx = tap - 3 * dy;
                const int sy = y + dy - 1, sx = x + dx - 1;
                if (kk < 27 && sy >= 0 && sy < a.Ho && sx >= 0 && sx < a.Wo) {
                    const float mean = c == 0 ? kMean[0] : c == 1 ? kMean[1] : kMean[2];
                    const float sd = c == 0 ? kStd[0] : c == 1 ? kStd[1] : kStd[2];
                    v[e] = (img[((int64_t)c * a.Ho + sy) * a.Wo + sx] - mean) / sd;
                }
            }
        } else if (k < 9 * a.C) {
            const int tap = k >> a.logC, c = k & (a.C - 1);
            const int dy = tap / 3, dx = tap - 3 * dy;
            const int sy = y + dy - 1, sx = x + dx - 1;
            if (sy >= 0 && sy < a.Ho && sx >= 0 && sx < a.Wo) {
                if (MODE == kPlain) {
                    v = *reinterpret_cast<const floatx4*>(a.src + (((int64_t)i * a.Hst + sy) * a.Wst + sx) * a.C + c);
                } else {  // Ho = Hst / 2, Wo = Wst / 2: rows 2 sy, 2 sy + 1 and columns 2 sx, 2 sx + 1 exist
                    const float* p = a.src + (((int64_t)i * a.Hst + 2 * sy) * a.Wst + 2 * sx) * a.C + c;
                    const int64_t down = (int64_t)a.Wst * a.C;
                    const floatx4 v00 = *reinterpret_cast<const floatx4*>(p);
                    const floatx4 v01 = *reinterpret_cast<const floatx4*>(p + a.C);
                    const floatx4 v10 = *reinterpret_cast<const floatx4*>(p + down);
                    const floatx4 v11 = *reinterpret_cast<const floatx4*>(p + down + a.C);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(fmaxf(v00[e], v01[e]), fmaxf(v10[e], v11[e]));
                }
            }
        }
        *reinterpret_cast<floatx4*>(a.out + m * a.kpad + k) = v;
    }
}

struct HeadArgs {
    const float* fx;   // [P][C]
    const float* fy;   // [P][C]
    const float* lin;  // [C]
    float* part;       // [ceil(P / 64)]
    int64_t P;
    int C;
};

// V float4 chunks per lane: chunk v of lane j (of the pixel's L lanes) holds channels 4 (v L + j) .. + 3
template <int V>
__global__ void __launch_bounds__(256) head_kernel(HeadArgs a) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.C / (4 * V);          // lanes per pixel: 4 .. 64, a power of two
    const int G = 64 / L;                 // pixels per wavefront and step
    const int g = lane / L, j = lane - g * L;
    floatx4 w[V];
#pragma unroll
    for (int v = 0; v < V; ++v) w[v] = *reinterpret_cast<const floatx4*>(a.lin + 4 * (v * L + j));
    const int64_t p0 = (int64_t)blockIdx.x * kHeadPix + wave * (kHeadPix / 4);
    float acc = 0.0f;
    for (int s = 0; s < kHeadPix / 4; s += G) {
        const int64_t p = p0 + s + g;
        floatx4 x[V], y[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            x[v] = y[v] = floatx4{0.f, 0.f, 0.f, 0.f};
            if (p < a.P) {
                x[v] = *reinterpret_cast<const floatx4*>(a.fx + p * a.C + 4 * (v * L + j));
                y[v] = *reinterpret_cast<const floatx4*>(a.fy + p * a.C + 4 * (v * L + j));
            }
        }
        float nx = 0.0f, ny = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                nx += x[v][e] * x[v][e];
                ny += y[v][e] * y[v][e];
            }
        for (int o = L >> 1; o > 0; o >>= 1) {
            nx += __shfl_xor(nx, o, 64);
            ny += __shfl_xor(ny, o, 64);
        }
        const float dx = sqrtf(nx) + 1e-10f, dy = sqrtf(ny) + 1e-10f;
        float d2 = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = x[v][e] / dx - y[v][e] / dy;
                d2 += w[v][e] * (d * d);
            }
        for (int o = L >> 1; o > 0; o >>= 1) d2 += __shfl_xor(d2, o, 64);
        acc += d2;   // a pixel past P: exactly 0
    }
    // every lane of a group holds the group's sum: the groups by the remaining butterfly steps
    for (int o = 32; o >= L; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (tid == 0) a.part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

struct ReduceArgs {
    const float* part[kTaps];
    int64_t blocks[kTaps];
    double count[kTaps];
    int terms;      // 1 .. 5
    int want_sum;   // out[terms] = the fp32 sum of the terms in order
    float* out;
};

__global__ void __launch_bounds__(64) reduce_kernel(ReduceArgs a) {
    const int lane = threadIdx.x;
    float total = 0.0f;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        if (t >= a.terms) break;
        double s = 0.0;
        for (int64_t b = lane; b < a.blocks[t]; b += 64) s += (double)a.part[t][b];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const float v = (float)(s / a.count[t]);
        total += v;
        if (lane == 0) a.out[t] = v;
    }
    if (lane == 0 && a.want_sum) a.out[a.terms] = total;
}

size_t round_up(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }
bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int64_t head_blocks(int64_t P) { return (P + kHeadPix - 1) / kHeadPix; }

int first_kpad(int mfma_dtype) { return mfma_dtype == CN_MFMA_BF16 ? 64 : 32; }

int launch_patches(const char* who, int mode, const PatchArgs& a, hipStream_t st) {
    const int64_t total = (int64_t)a.n * a.rows * a.Wo * (a.kpad >> 2);
    if (total == 0) return CN_OK;
    const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
    if (mode == kPlain) patches_kernel<kPlain><<<grid, 256, 0, st>>>(a);
    else if (mode == kPool) patches_kernel<kPool><<<grid, 256, 0, st>>>(a);
    else patches_kernel<kFirst><<<grid, 256, 0, st>>>(a);
    return check_launch(who);
}

int launch_head(const char* who, const HeadArgs& a, hipStream_t st) {
    const unsigned grid = (unsigned)head_blocks(a.P);
    if (a.C == 512) head_kernel<2><<<grid, 256, 0, st>>>(a);
    else head_kernel<1><<<grid, 256, 0, st>>>(a);
    return check_launch(who);
}

bool head_channels_ok(int C) { return C >= 16 && C <= 512 && (C & (C - 1)) == 0; }

// What one call needs, from the sizes alone.
struct Plan {
    int Ho[kConvs], Wo[kConvs], kpad[kConvs], rows[kConvs];
    size_t map_bytes, patch_bytes, part_off[kTaps], bytes;
};

int make_plan(const char* who, int H, int W, int band_rows, int mfma_dtype, Plan& p) {
    CN_REQUIRE(H >= kMinSize && W >= kMinSize, CN_ERR_SHAPE,
               "%s: image of %d x %d (each at least %d: the last block would be empty)", who, H, W, kMinSize);
    CN_REQUIRE((int64_t)H * W <= kMaxPixels, CN_ERR_SHAPE, "%s: image of %d x %d too large (H W up to 2^26)", who, H, W);
    CN_REQUIRE(band_rows >= 0, CN_ERR_SHAPE, "%s: band_rows %d (0: the library's choice)", who, band_rows);
    CN_REQUIRE(mfma_dtype == CN_MFMA_F32 || mfma_dtype == CN_MFMA_BF16 || mfma_dtype == CN_MFMA_F32_BF16X6, CN_ERR_SHAPE,
               "%s: bad mfma_dtype %d", who, mfma_dtype);
    int h = H, w = W;
    p.patch_bytes = 0;
    size_t off = 0;
    for (int l = 0; l < kConvs; ++l) {
        if (kPooled[l]) h /= 2, w /= 2;
        p.Ho[l] = h;
        p.Wo[l] = w;
        p.kpad[l] = l == 0 ? first_kpad(mfma_dtype) : 9 * kCout[l - 1];
        const size_t row_bytes = (size_t)2 * w * p.kpad[l] * sizeof(float);
        const int64_t most = band_rows > 0 ? band_rows : (int64_t)std::max<size_t>(1, kPatchCap / row_bytes);
        const int64_t bands = (h + most - 1) / most;   // of equal height up to one row: no thin last band
        p.rows[l] = (int)((h + bands - 1) / bands);
        p.patch_bytes = std::max(p.patch_bytes, round_up(row_bytes * p.rows[l]));
        if (kTapOf[l] >= 0) {
            p.part_off[kTapOf[l]] = off;
            off += round_up((size_t)head_blocks((int64_t)h * w) * sizeof(float));
        }
    }
    p.map_bytes = round_up((size_t)2 * H * W * 64 * sizeof(float));   // the two widest maps: block 1's
    for (int t = 0; t < kTaps; ++t) p.part_off[t] += 2 * p.map_bytes + p.patch_bytes;
    p.bytes = 2 * p.map_bytes + p.patch_bytes + off;
    return CN_OK;
}

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" int cn_lpips_patches(int32_t mode, int32_t n, int32_t Hs, int32_t Ws, int32_t C, const float* src,
                                const float* src1, int32_t y0, int32_t rows, int32_t kpad, float* out,
                                cn_stream_t stream) {
    CN_REQUIRE(mode == kPlain || mode == kPool || mode == kFirst, CN_ERR_ARG, "cn_lpips_patches: bad mode %d", mode);
    CN_REQUIRE(n >= 1 && Hs >= 1 && Ws >= 1 && (int64_t)Hs * Ws <= kMaxPixels, CN_ERR_SHAPE,
               "cn_lpips_patches: %d maps of %d x %d (each at least 1, Hs Ws up to 2^26)", n, Hs, Ws);
    const int Ho = mode == kPool ? Hs / 2 : Hs, Wo = mode == kPool ? Ws / 2 : Ws;
    CN_REQUIRE(y0 >= 0 && rows >= 0 && (int64_t)y0 + rows <= Ho, CN_ERR_SHAPE,
               "cn_lpips_patches: rows [%d, %d + %d) outside the %d output rows", y0, y0, rows, Ho);
    CN_REQUIRE((int64_t)n * rows * Wo < ((int64_t)1 << 31), CN_ERR_SHAPE, "cn_lpips_patches: %lld operand rows (below 2^31)",
               (long long)n * rows * Wo);
    if (mode == kFirst) {
        CN_REQUIRE(C == 3 && n <= 2 && kpad >= 28 && kpad % 4 == 0, CN_ERR_SHAPE,
                   "cn_lpips_patches: the first layer takes one or two images of 3 channels, kpad >= 28 and a multiple of 4 "
                   "(n=%d C=%d kpad=%d)", n, C, kpad);
        CN_REQUIRE(src && (n == 1 || src1) && out, CN_ERR_ARG, "cn_lpips_patches: null image / out");
        CN_REQUIRE((((uintptr_t)src | (uintptr_t)src1) & 3) == 0 && al16(out), CN_ERR_ALIGN,
                   "cn_lpips_patches: images 4-byte, out 16-byte aligned");
    } else {
        CN_REQUIRE(C >= 4 && C <= 4096 && (C & (C - 1)) == 0 && kpad >= 9 * C && kpad % 4 == 0, CN_ERR_SHAPE,
                   "cn_lpips_patches: C=%d must be a power of two in [4, 4096] and kpad=%d >= 9 C, a multiple of 4", C, kpad);
        CN_REQUIRE(src && out, CN_ERR_ARG, "cn_lpips_patches: null src / out");
        CN_REQUIRE(al16(src) && al16(out), CN_ERR_ALIGN, "cn_lpips_patches: src and out 16-byte aligned");
    }
    CN_REQUIRE(kpad < (1 << 20), CN_ERR_SHAPE, "cn_lpips_patches: kpad=%d (below 2^20)", kpad);
    int logC = 0;
    while ((1 << logC) < C) ++logC;
    const PatchArgs a{src, src1, out, n, Hs, Ws, Ho, Wo, C, logC, kpad, y0, rows};
    return launch_patches("cn_lpips_patches", mode, a, (hipStream_t)stream);
}

extern "C" size_t cn_lpips_head_workspace_bytes(int64_t P) {
    if (P < 1 || P > kMaxPixels) return 0;
    return round_up((size_t)head_blocks(P) * sizeof(float));
}

extern "C" int cn_lpips_head(int32_t C, int64_t P, const float* fx, const float* fy, const float* lin, float* out,
                             void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    CN_REQUIRE(head_channels_ok(C), CN_ERR_SHAPE, "cn_lpips_head: C=%d must be a power of two in [16, 512]", C);
    CN_REQUIRE(P >= 1 && P <= kMaxPixels, CN_ERR_SHAPE, "cn_lpips_head: %lld pixels (1 .. 2^26)", (long long)P);
    CN_REQUIRE(fx && fy && lin && out, CN_ERR_ARG, "cn_lpips_head: null fx / fy / lin / out");
    CN_REQUIRE(al16(fx) && al16(fy) && al16(lin) && ((uintptr_t)out & 3) == 0, CN_ERR_ALIGN,
               "cn_lpips_head: fx, fy and lin 16-byte, out 4-byte aligned");
    const size_t need = cn_lpips_head_workspace_bytes(P);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_lpips_head: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_lpips_head: workspace not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const HeadArgs a{fx, fy, lin, static_cast<float*>(workspace), P, C};
    if (int rc = launch_head("cn_lpips_head", a, st)) return rc;
    ReduceArgs r{};
    r.part[0] = a.part;
    r.blocks[0] = head_blocks(P);
    r.count[0] = (double)P;
    r.terms = 1;
    r.out = out;
    reduce_kernel<<<1, 64, 0, st>>>(r);
    return check_launch("cn_lpips_head (reduce)");
}

extern "C" size_t cn_lpips_workspace_bytes(int32_t H, int32_t W, int32_t band_rows, int32_t mfma_dtype) {
    Plan p;
    if (make_plan("cn_lpips_workspace_bytes", H, W, band_rows, mfma_dtype, p) != CN_OK) return 0;
    return p.bytes;
}

extern "C" int cn_lpips(const cn_lpips_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_SHAPE, "cn_lpips: null desc");
    Plan p;
    if (int rc = make_plan("cn_lpips", d->H, d->W, d->band_rows, d->mfma_dtype, p)) return rc;
    CN_REQUIRE(d->pred && d->gt && d->out, CN_ERR_SHAPE, "cn_lpips: null pred / gt / out");
    for (int l = 0; l < kConvs; ++l)
        CN_REQUIRE(d->weights[l] && d->bias[l], CN_ERR_SHAPE, "cn_lpips: null weights[%d] / bias[%d]", l, l);
    for (int t = 0; t < kTaps; ++t) CN_REQUIRE(d->lin[t], CN_ERR_SHAPE, "cn_lpips: null lin[%d]", t);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= p.bytes, CN_ERR_SHAPE,
               "cn_lpips: workspace %lld bytes, %zu needed", (long long)workspace_bytes, p.bytes);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_lpips: workspace not 256-byte aligned");
    uintptr_t all4 = (uintptr_t)d->pred | (uintptr_t)d->gt | (uintptr_t)d->out;
    CN_REQUIRE((all4 & 3) == 0, CN_ERR_ALIGN, "cn_lpips: pred, gt and out 4-byte aligned");
    for (int t = 0; t < kTaps; ++t) CN_REQUIRE(al16(d->lin[t]), CN_ERR_ALIGN, "cn_lpips: lin[%d] not 16-byte aligned", t);

    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    float* maps[2] = {reinterpret_cast<float*>(ws), reinterpret_cast<float*>(ws + p.map_bytes)};
    float* patch = reinterpret_cast<float*>(ws + 2 * p.map_bytes);
    const bool x6 = d->mfma_dtype == CN_MFMA_F32_BF16X6;
    ReduceArgs r{};
    int Hst = d->H, Wst = d->W;
    for (int l = 0; l < kConvs; ++l) {
        const int Ho = p.Ho[l], Wo = p.Wo[l], kpad = p.kpad[l], N = kCout[l];
        const float* src = l == 0 ? d->pred : maps[(l - 1) & 1];
        float* dst = maps[l & 1];
        const int mode = l == 0 ? kFirst : kPooled[l] ? kPool : kPlain;
        cn_linear_desc g{};
        g.B = static_cast<const float*>(d->weights[l]);
        g.bias = d->bias[l];
        g.lda = kpad;
        g.ldb = x6 ? (N + 127) / 128 * 128 : kpad;   // bf16x6: the chunk-major image's rows
        g.ld_out0 = N;
        g.N = N;
        g.K = kpad;
        g.epilogue = CN_EPI_RELU;
        g.mfma_dtype = d->mfma_dtype;
        for (int y0 = 0; y0 < Ho; y0 += p.rows[l]) {
            const int rows = std::min(p.rows[l], Ho - y0);
            const PatchArgs a{src, d->gt, patch, 2, Hst, Wst, Ho, Wo, l == 0 ? 3 : kCout[l - 1],
                              l == 0 ? 0 : __builtin_ctz(kCout[l - 1]), kpad, y0, rows};
            if (int rc = launch_patches("cn_lpips (patches)", mode, a, st)) return rc;
            // the band's rows of image i are contiguous in the map; a band of the whole height is one GEMM
            const int calls = rows == Ho ? 1 : 2;
            for (int i = 0; i < calls; ++i) {
                g.A = patch + (int64_t)i * rows * Wo * kpad;
                g.out0 = dst + ((int64_t)i * Ho + y0) * Wo * N;
                g.M = (calls == 1 ? 2 : 1) * rows * Wo;
                if (int rc = cn_linear(&g, stream)) return rc;
            }
        }
        Hst = Ho;
        Wst = Wo;
        const int t = kTapOf[l];
        if (t >= 0) {
            const int64_t P = (int64_t)Ho * Wo;
            const HeadArgs h{dst, dst + P * N, d->lin[t], reinterpret_cast<float*>(ws + p.part_off[t]), P, N};
            if (int rc = launch_head("cn_lpips (head)", h, st)) return rc;
            r.part[t] = h.part;
            r.blocks[t] = head_blocks(P);
            r.count[t] = (double)P;
        }
    }
    r.terms = kTaps;
    r.want_sum = 1;
    r.out = d->out;
    reduce_kernel<<<1, 64, 0, st>>>(r);
    return check_launch("cn_lpips (reduce)");
}
