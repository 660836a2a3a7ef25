// cn_flow_rgb.hip — the flow-RGB term of stage 1 (ABI v21): the flow projection of train.py:484-495
// from the per-ray sums of cn_stage1_fwd, warp_pixel (train.py:235-244) and the masked L1 of
// train.py:506-515 for T reference frames in one launch each way, instead of ~25 torch launches
// forward, as many autograd nodes back and a copy of T whole frames out of the image stack:
//
//   per frame t and ray r, with (pbar, wbar) = ray_acc[r] = (sum_s w p, sum_s w)
//     wp   = w2c[t][:3,:3] pbar + wbar w2c[t][:3,3],  q = KS[t] wp,  n = (q0, q1) / q2
//     corr = pix + (n - pixn) * (W/2, H/2)
//     valid = 0 <= corr.x < W and 0 <= corr.y < H            (false for a NaN / Inf correspondence)
//     warp = the bilinear sample of images[frame[t]] at corr, border padding, align_corners=True
//   sums[t] = (sum over valid rays and channels of |warp - rgb_gt|, number of valid rays)
//   backward: g_num[t] sign(warp - gt) -> the bilinear derivative (zero where clamped) -> the quotient
//     rule -> KS^T -> d w2c[t][:3,:] (outer products with (pbar, wbar)) and d ray_acc (through w2c^T).
//
// One wavefront per 64 rays.  Forward: a workgroup per (64 rays, frame); backward: a workgroup per 64
// rays that walks the frames in order, so d ray_acc is summed over t = 0 .. T-1 in a register.  The
// sums and d w2c are per-workgroup partials (wave shuffles) that slab_reduce_kernel adds in a fixed
// order: no atomics, bitwise reproducible, and a frame's result does not depend on the other frames.
// The backward recomputes the projection and re-reads the taps (48 bytes per valid ray and frame)
// instead of keeping a Jacobian: nothing is saved between the two calls.
#include "cn_mfma.h"

namespace cn {
namespace {

constexpr int kRays = 64;       // rays per workgroup: one wavefront
constexpr int kMaxFrames = 8;
constexpr int kFwdPart = 2;     // floats per (workgroup, frame) partial, forward: sum |.|, count
constexpr int kBwdPart = 12;    // backward: d w2c[t][:3,:]
constexpr size_t kAlign = 256;

struct FlowArgs {
    int R, T, N, H, W;
    const float* ray_acc;     // [R][4]
    const float* w2c;         // [T][4][4]
    const float* KS;          // [T][3][3]
    const float* pixn;        // [R][2]
    const float* pix;         // [R][2]
    const float* gt;          // [R][3]
    const float* images;      // [N][3][H][W]
    const int64_t* frame;     // [T]
    const uint8_t* fvalid;    // [T] or null
};

// the frame of reference t, or false: masked, or an index outside the stack (nothing of it is read)
__device__ __forceinline__ bool frame_of(const FlowArgs& a, int t, int64_t* f) {
    if (a.fvalid && a.fvalid[t] == 0) return false;
    const int64_t i = a.frame[t];
    if (i < 0 || i >= (int64_t)a.N) return false;
    *f = i;
    return true;
}

struct Proj {
    float q2, nx, ny, cx, cy;
    bool valid;
};

// project_flow_sums and the mask of flow_rgb_loss for one ray: M = w2c[t] (rows of 4), Ks = KS[t]
__device__ __forceinline__ Proj project(const float* M, const float* Ks, const float (&pa)[4], float pnx, float pny,
                                        float px, float py, int H, int W) {
    float wp[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        wp[i] = ((M[4 * i] * pa[0] + M[4 * i + 1] * pa[1]) + M[4 * i + 2] * pa[2]) + pa[3] * M[4 * i + 3];
    const float q0 = (Ks[0] * wp[0] + Ks[1] * wp[1]) + Ks[2] * wp[2];
    const float q1 = (Ks[3] * wp[0] + Ks[4] * wp[1]) + Ks[5] * wp[2];
    Proj p;
    p.q2 = (Ks[6] * wp[0] + Ks[7] * wp[1]) + Ks[8] * wp[2];
    p.nx = q0 / p.q2;
    p.ny = q1 / p.q2;
    p.cx = px + (p.nx - pnx) * ((float)W * 0.5f);
    p.cy = py + (p.ny - pny) * ((float)H * 0.5f);
    // (every comparison is false for a NaN: a correspondence that is not finite is invalid)
    p.valid = p.cx >= 0.0f && p.cx < (float)W && p.cy >= 0.0f && p.cy < (float)H;
    return p;
}

// sum_c |warp_c - gt_c| of the bilinear sample of one frame (fr: its three planes) at (cx, cy), and with
// GRAD its derivative by (cx, cy): sign(e) through the taps (grid_sampler_2d_backward's order), zero
// where the coordinate was clamped.  The taps stay inside the frame for any (cx, cy), a NaN included.
template <bool GRAD>
__device__ __forceinline__ float warp_l1(const float* __restrict__ fr, int H, int W, float cx, float cy,
                                         const float (&gt)[3], float* gcx, float* gcy) {
    const int HW = H * W;
    float mx, my;
    const float x = clip_border(cx, (float)(W - 1), &mx);
    const float y = clip_border(cy, (float)(H - 1), &my);
    const float xf = floorf(x), yf = floorf(y);
    const int x0 = (int)xf, y0 = (int)yf;  // in [0, W-1] x [0, H-1] after the clip
    const bool hx = x0 + 1 < W, hy = y0 + 1 < H;  // the east / south taps are inside the image
    const float fx1 = x - xf, fx0 = (xf + 1.0f) - x;
    const float fy1 = y - yf, fy0 = (yf + 1.0f) - y;
    const float wnw = fx0 * fy0, wne = fx1 * fy0, wsw = fx0 * fy1, wse = fx1 * fy1;
    const int o00 = y0 * W + x0;
    const int o01 = hx ? o00 + 1 : o00, o10 = hy ? o00 + W : o00, o11 = o10 + (hx ? 1 : 0);
    float gx = 0.0f, gy = 0.0f, sabs = 0.0f;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* s = fr + ch * HW;
        const float nw = s[o00];
        const float ne = hx ? s[o01] : 0.0f;
        const float sw = hy ? s[o10] : 0.0f;
        const float se = (hx && hy) ? s[o11] : 0.0f;
        const float wv = ((nw * wnw + ne * wne) + sw * wsw) + se * wse;
        const float e = wv - gt[ch];
        sabs += fabsf(e);
        if (GRAD) {
            const float sg = e > 0.0f ? 1.0f : (e < 0.0f ? -1.0f : 0.0f);
            gx += sg * (((ne * fy0 - nw * fy0) - sw * fy1) + se * fy1);
            gy += sg * (((sw * fx0 - nw * fx0) - ne * fx1) + se * fx1);
        }
    }
    if (GRAD) {
        *gcx = gx * mx;
        *gcy = gy * my;
    }
    return sabs;
}

template <int N>
__device__ __forceinline__ void wave_total(float (&v)[N]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], o, 64);
}

struct Ray {
    float pa[4], pnx, pny, px, py, gt[3];
};

__device__ __forceinline__ Ray load_ray(const FlowArgs& a, int r) {
    Ray y;
    const floatx4 v = *reinterpret_cast<const floatx4*>(a.ray_acc + (int64_t)r * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) y.pa[i] = v[i];
    y.pnx = a.pixn[(int64_t)r * 2];
    y.pny = a.pixn[(int64_t)r * 2 + 1];
    y.px = a.pix[(int64_t)r * 2];
    y.py = a.pix[(int64_t)r * 2 + 1];
#pragma unroll
    for (int i = 0; i < 3; ++i) y.gt[i] = a.gt[(int64_t)r * 3 + i];
    return y;
}

// grid (ceil(R / 64), T): part[(block * T + t) * 2 + (0, 1)] = the block's L1 sum and valid count of frame t
__global__ void __launch_bounds__(kRays) flow_rgb_fwd_kernel(FlowArgs a, float* part) {
    const int t = blockIdx.y;
    const int r = blockIdx.x * kRays + threadIdx.x;
    float s[kFwdPart] = {0.0f, 0.0f};
    int64_t f;
    if (frame_of(a, t, &f) && r < a.R) {
        const Ray y = load_ray(a, r);
        const Proj p = project(a.w2c + t * 16, a.KS + t * 9, y.pa, y.pnx, y.pny, y.px, y.py, a.H, a.W);
        if (p.valid) {
            s[0] = warp_l1<false>(a.images + f * 3 * ((int64_t)a.H * a.W), a.H, a.W, p.cx, p.cy, y.gt, nullptr, nullptr);
            s[1] = 1.0f;
        }
    }
    wave_total<kFwdPart>(s);
    if (threadIdx.x == 0) {
        float* o = part + ((int64_t)blockIdx.x * a.T + t) * kFwdPart;
        o[0] = s[0];
        o[1] = s[1];
    }
}

// grid ceil(R / 64): d_ray[r] = sum over t in order of the ray's gradient; part[(block * T + t) * 12 + i] =
// the block's d w2c[t][:3,:] (row-major 3 x 4)
__global__ void __launch_bounds__(kRays) flow_rgb_bwd_kernel(FlowArgs a, const float* g_num, float* d_ray,
                                                             float* part) {
    const int r = blockIdx.x * kRays + threadIdx.x;
    const bool live = r < a.R;
    Ray y = {};
    if (live) y = load_ray(a, r);
    float dr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int t = 0; t < a.T; ++t) {
        float acc[kBwdPart] = {};
        int64_t f;
        const bool ok = frame_of(a, t, &f);  // the same for every lane
        if (ok && live) {
            const float* M = a.w2c + t * 16;
            const float* Ks = a.KS + t * 9;
            const Proj p = project(M, Ks, y.pa, y.pnx, y.pny, y.px, y.py, a.H, a.W);
            if (p.valid) {
                float gcx, gcy;
                warp_l1<true>(a.images + f * 3 * ((int64_t)a.H * a.W), a.H, a.W, p.cx, p.cy, y.gt, &gcx, &gcy);
                const float g = g_num[t];
                const float gnx = (g * gcx) * ((float)a.W * 0.5f), gny = (g * gcy) * ((float)a.H * 0.5f);
                const float dq0 = gnx / p.q2, dq1 = gny / p.q2;
                const float dq2 = -(gnx * p.nx + gny * p.ny) / p.q2;
                float dwp[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) dwp[j] = (Ks[j] * dq0 + Ks[3 + j] * dq1) + Ks[6 + j] * dq2;
#pragma unroll
                for (int j = 0; j < 4; ++j) dr[j] += (M[j] * dwp[0] + M[4 + j] * dwp[1]) + M[8 + j] * dwp[2];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[4 * i + j] = dwp[i] * y.pa[j];
            }
        }
        if (ok) wave_total<kBwdPart>(acc);
        if (threadIdx.x == 0) {
            float* o = part + ((int64_t)blockIdx.x * a.T + t) * kBwdPart;
#pragma unroll
            for (int i = 0; i < kBwdPart; ++i) o[i] = acc[i];
        }
    }
    if (live) {
        floatx4 v = {dr[0], dr[1], dr[2], dr[3]};
        *reinterpret_cast<floatx4*>(d_ray + (int64_t)r * 4) = v;
    }
}

int blocks_of(int R) { return cdiv(R, kRays); }

int shape_check(const char* who, int R, int T) {
    CN_REQUIRE(R >= 0, CN_ERR_SHAPE, "%s: %d rays", who, R);
    CN_REQUIRE(T >= 1 && T <= kMaxFrames, CN_ERR_SHAPE, "%s: %d reference frames (1 .. %d)", who, T, kMaxFrames);
    return CN_OK;
}

// every check of the two entry points that does not concern their outputs
int args_check(const char* who, const FlowArgs& a, const void* workspace, int64_t workspace_bytes) {
    if (int rc = shape_check(who, a.R, a.T)) return rc;
    CN_REQUIRE(a.N >= 1, CN_ERR_SHAPE, "%s: a stack of %d frames", who, a.N);
    CN_REQUIRE(a.H >= 1 && a.W >= 1, CN_ERR_SHAPE, "%s: frames of %d x %d (each at least 1)", who, a.H, a.W);
    // offsets inside one frame (3 planes) are 32-bit; the frame's base offset in the stack is 64-bit
    CN_REQUIRE((int64_t)a.H * a.W * 3 < ((int64_t)1 << 31), CN_ERR_SHAPE,
               "%s: frames of %d x %d too large (3 H W must stay below 2^31)", who, a.H, a.W);
    CN_REQUIRE(a.w2c && a.KS && a.images && a.frame, CN_ERR_ARG, "%s: null w2c / KS / images / frame", who);
    CN_REQUIRE(a.R == 0 || (a.ray_acc && a.pixn && a.pix && a.gt), CN_ERR_ARG,
               "%s: null ray_acc / pixn / pix / rgb_gt", who);
    const uintptr_t all4 = (uintptr_t)a.w2c | (uintptr_t)a.KS | (uintptr_t)a.images | (uintptr_t)a.pixn |
                           (uintptr_t)a.pix | (uintptr_t)a.gt;
    CN_REQUIRE((all4 & 3) == 0 && al8(a.frame), CN_ERR_ALIGN, "%s: fp32 arrays 4-byte, frame 8-byte aligned", who);
    CN_REQUIRE(al16(a.ray_acc), CN_ERR_ALIGN, "%s: ray_acc not 16-byte aligned", who);
    const size_t need = cn_flow_rgb_workspace_bytes(a.R, a.T);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "%s: workspace %lld bytes, %zu needed", who, (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "%s: workspace not 256-byte aligned", who);
    return CN_OK;
}

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" size_t cn_flow_rgb_workspace_bytes(int32_t R, int32_t T) {
    if (R < 0 || T < 1 || T > kMaxFrames) return 0;
    const size_t b = (size_t)blocks_of(R > 0 ? R : 1) * (size_t)T * kBwdPart * sizeof(float);
    return (b + kAlign - 1) / kAlign * kAlign;
}

extern "C" int cn_flow_rgb_fwd(int32_t R, int32_t T, int32_t N, int32_t H, int32_t W, const float* ray_acc,
                               const float* w2c, const float* KS, const float* pixn, const float* pix,
                               const float* rgb_gt, const float* images, const int64_t* frame,
                               const uint8_t* frame_valid, float* sums, void* workspace, int64_t workspace_bytes,
                               cn_stream_t stream) {
    const FlowArgs a{R, T, N, H, W, ray_acc, w2c, KS, pixn, pix, rgb_gt, images, frame, frame_valid};
    if (int rc = args_check("cn_flow_rgb_fwd", a, workspace, workspace_bytes)) return rc;
    CN_REQUIRE(sums, CN_ERR_ARG, "cn_flow_rgb_fwd: null sums");
    CN_REQUIRE(((uintptr_t)sums & 3) == 0, CN_ERR_ALIGN, "cn_flow_rgb_fwd: sums not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* part = static_cast<float*>(workspace);
    const int nblk = blocks_of(R);  // R = 0: no partials, the reduction writes zero sums
    if (R > 0) {
        flow_rgb_fwd_kernel<<<dim3((unsigned)nblk, (unsigned)T), kRays, 0, st>>>(a, part);
        if (int rc = check_launch("cn_flow_rgb_fwd")) return rc;
    }
    return launch_slab_reduce(part, nblk, (int64_t)T * kFwdPart, T, kFwdPart, kFwdPart, sums, kFwdPart, 1.0f, 0, st);
}

extern "C" int cn_flow_rgb_bwd(int32_t R, int32_t T, int32_t N, int32_t H, int32_t W, const float* ray_acc,
                               const float* w2c, const float* KS, const float* pixn, const float* pix,
                               const float* rgb_gt, const float* images, const int64_t* frame,
                               const uint8_t* frame_valid, const float* g_num, float* d_ray_acc, float* d_w2c,
                               void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    const FlowArgs a{R, T, N, H, W, ray_acc, w2c, KS, pixn, pix, rgb_gt, images, frame, frame_valid};
    if (int rc = args_check("cn_flow_rgb_bwd", a, workspace, workspace_bytes)) return rc;
    CN_REQUIRE(g_num && d_w2c && (R == 0 || d_ray_acc), CN_ERR_ARG, "cn_flow_rgb_bwd: null g_num / d_ray_acc / d_w2c");
    CN_REQUIRE((((uintptr_t)g_num | (uintptr_t)d_w2c) & 3) == 0, CN_ERR_ALIGN,
               "cn_flow_rgb_bwd: g_num / d_w2c not 4-byte aligned");
    CN_REQUIRE(al16(d_ray_acc), CN_ERR_ALIGN, "cn_flow_rgb_bwd: d_ray_acc not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float* part = static_cast<float*>(workspace);
    const int nblk = blocks_of(R);
    if (R > 0) {
        flow_rgb_bwd_kernel<<<nblk, kRays, 0, st>>>(a, g_num, d_ray_acc, part);
        if (int rc = check_launch("cn_flow_rgb_bwd")) return rc;
    }
    return launch_slab_reduce(part, nblk, (int64_t)T * kBwdPart, T, kBwdPart, kBwdPart, d_w2c, kBwdPart, 1.0f, 0, st);
}
