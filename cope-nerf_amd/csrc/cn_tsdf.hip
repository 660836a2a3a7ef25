// cn_tsdf.hip — fusion of per-view depth maps into a truncated signed distance volume (additive to ABI v22):
// cn_tsdf_integrate / cn_tsdf_finalize, and the trilinear attribute sampler cn_volume_sample.  The mesher that
// leaves out unobserved space (cn_mesh_count_observed / cn_mesh_emit_observed) is a variant of cn_mesh.hip's kernels
// and lives there.  The reference has no fusion code; the yardstick is a float64 restatement (tests/tsdf_ref.py).
// Cameras are 3 x 4 projections as in cn_mesh_raster.hip: (a, b, c) = P [X, 1], pixel (a / c, b / c), depth c.
//
// cn_tsdf_integrate: one thread per voxel, z the fastest thread index, so a wavefront covers 64 consecutive
// voxels of the volumes and its reads and writes of tsum / wsum / csum are one coalesced access each.  The sums
// live in registers across all views of a call: every volume is read once and written once per call, whatever N.
// Arithmetic per view (fp32, -ffp-contract=off; tests/tsdf_ref.py restates it in numpy float32):
//   X_ax = (float)i / (float)(n - 1) * (hi - lo) + lo                        (the mesher's vertex map at integers)
//   a = ((P00 x + P01 y) + P02 z) + P03, b and c alike;   skip unless c >= near
//   pixel (floor(a / c + 0.5), floor(b / c + 0.5)), skip outside the image;   d = depth[view][py][px]
//   skip unless d finite, d > 0, d <= depth_max;   s = d - c, skip if s < -trunc
//   tsum += fminf(1, s / trunc), wsum += 1, csum += color[view][py][px]
// A voxel's result depends on nothing but its own sequence of views: no atomics, bitwise repeatable, and N views in
// one call equal any split of them, in the same order, over several calls.
//
// The projection rows are the same in every lane: they are read at a wave-uniform address (the loop counter), which
// the compiler turns into scalar loads.  The projection is evaluated afresh for every voxel, never incrementally
// along z: the rounding above is the contract.
//
// Brick rejection.  The 64 voxels of a wavefront lie in an index box (a stretch of one z row, or whole rows, or
// whole planes); lane l holds corner l & 7 of that box.  Per view the eight corners are projected once and the view
// is skipped for the whole wave, by a wave-uniform branch, when at every corner one and the same of these holds:
//   c + m_c < near                       (behind the near bound)
//   a + 0.5 c < -m,   a - (w - 0.5) c > m,   b + 0.5 c < -m,   b - (h - 0.5) c > m      (off one side of the image)
// Each left side is linear in X, so what holds at the corners holds, with its margin, at every voxel between them
// (the voxel map is monotone in i, so every voxel lies in the corners' box); for c >= near > 0 the four side tests
// are floor(a / c + 0.5) < 0, >= w, ... multiplied out.  The margins are 1e-4 (S_a + w S_c) with S the sum of the
// absolute terms of a row at that corner (convex in X, so the corners bound it too): several hundred times the fp32
// error of the evaluation at corner and voxel, so a rejected view is one that every lane would have skipped.
#include "cn_common.h"

#include <cmath>

namespace cn {
namespace {

constexpr int64_t kMaxCount = ((int64_t)1 << 31) - 1;  // nx ny nz, h w, Q < 2^31
constexpr float kBrickMargin = 1e-4f;

struct TsdfArgs {
    int nx, ny, nz;
    float lo[3], hi[3];
    int N, h, w;
    const float* proj;
    const float* depth;
    const float* color;
    float trunc, near, depth_max;
    int no_reject;
    float* tsum;
    float* wsum;
    float* csum;
};

__device__ __forceinline__ float voxel_at(int i, int n, float lo, float hi) {
    return (float)i / (float)(n - 1) * (hi - lo) + lo;
}

__device__ __forceinline__ void unravel(int p, int ny, int nz, int* ix, int* iy, int* iz) {
    *iz = p % nz;
    const int r = p / nz;
    *iy = r % ny;
    *ix = r / ny;
}

template <bool COLOR>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(TsdfArgs a) {
    const int nvox = a.nx * a.ny * a.nz;  // < 2^31 (checked)
    const int lane = threadIdx.x & 63;
    const int64_t w0 = (int64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane);  // the wave's first voxel
    if (w0 >= nvox) return;                                                      // (the whole wave)
    const bool live = w0 + lane < nvox;
    const int p0 = (int)w0;
    const int p1 = (int)(w0 + 63 < nvox ? w0 + 63 : nvox - 1);
    const int p = live ? p0 + lane : p1;  // (a lane past the end works on the last voxel and writes nothing)
    int ix, iy, iz;
    unravel(p, a.ny, a.nz, &ix, &iy, &iz);
    const float x = voxel_at(ix, a.nx, a.lo[0], a.hi[0]);
    const float y = voxel_at(iy, a.ny, a.lo[1], a.hi[1]);
    const float z = voxel_at(iz, a.nz, a.lo[2], a.hi[2]);

    // the wave's index box and this lane's corner of it
    int x0, y0, z0, x1, y1, z1;
    unravel(p0, a.ny, a.nz, &x0, &y0, &z0);
    unravel(p1, a.ny, a.nz, &x1, &y1, &z1);
    if (x0 != x1) {
        y0 = 0;
        y1 = a.ny - 1;
    }
    if (x0 != x1 || y0 != y1) {
        z0 = 0;
        z1 = a.nz - 1;
    }
    const float cx = voxel_at((lane & 1) ? x1 : x0, a.nx, a.lo[0], a.hi[0]);
    const float cy = voxel_at((lane & 2) ? y1 : y0, a.ny, a.lo[1], a.hi[1]);
    const float cz = voxel_at((lane & 4) ? z1 : z0, a.nz, a.lo[2], a.hi[2]);
    const float wf = (float)a.w - 0.5f, hf = (float)a.h - 0.5f;

    float ts = a.tsum[p], ws = a.wsum[p];
    float cs[3] = {0.0f, 0.0f, 0.0f};
    if (COLOR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) cs[k] = a.csum[(int64_t)p * 3 + k];
    }
    const int64_t hw = (int64_t)a.h * a.w;
    for (int v = 0; v < a.N; ++v) {  // bound: the views of the call
        const float* __restrict__ P = a.proj + (int64_t)v * 12;  // the same address in every lane
        const float p00 = P[0], p01 = P[1], p02 = P[2], p03 = P[3];
        const float p10 = P[4], p11 = P[5], p12 = P[6], p13 = P[7];
        const float p20 = P[8], p21 = P[9], p22 = P[10], p23 = P[11];
        if (!a.no_reject) {
            const float ca = ((p00 * cx + p01 * cy) + p02 * cz) + p03;
            const float cb = ((p10 * cx + p11 * cy) + p12 * cz) + p13;
            const float cc = ((p20 * cx + p21 * cy) + p22 * cz) + p23;
            const float sa = ((fabsf(p00 * cx) + fabsf(p01 * cy)) + fabsf(p02 * cz)) + fabsf(p03);
            const float sb = ((fabsf(p10 * cx) + fabsf(p11 * cy)) + fabsf(p12 * cz)) + fabsf(p13);
            const float sc = ((fabsf(p20 * cx) + fabsf(p21 * cy)) + fabsf(p22 * cz)) + fabsf(p23);
            const float ma = kBrickMargin * (sa + (float)a.w * sc), mb = kBrickMargin * (sb + (float)a.h * sc);
            // (a NaN anywhere fails its comparison: no rejection)
            const bool behind = cc + kBrickMargin * sc < a.near;
            const bool left = ca + 0.5f * cc < -ma, right = ca - wf * cc > ma;
            const bool top = cb + 0.5f * cc < -mb, bottom = cb - hf * cc > mb;
            if (__all(behind) || __all(left) || __all(right) || __all(top) || __all(bottom)) continue;
        }
        const float pa = ((p00 * x + p01 * y) + p02 * z) + p03;
        const float pb = ((p10 * x + p11 * y) + p12 * z) + p13;
        const float pc = ((p20 * x + p21 * y) + p22 * z) + p23;
        if (!(pc >= a.near)) continue;
        const float fx = floorf(pa / pc + 0.5f), fy = floorf(pb / pc + 0.5f);
        if (!(fx >= 0.0f && fx <= (float)(a.w - 1) && fy >= 0.0f && fy <= (float)(a.h - 1))) continue;  // (NaN: outside)
        const int64_t px = v * hw + (int64_t)(int)fy * a.w + (int)fx;  // in range by the test above
        const float d = a.depth[px];
        if (!(d > 0.0f && d < INFINITY && d <= a.depth_max)) continue;  // (NaN fails d > 0)
        const float s = d - pc;
        if (s < -a.trunc) continue;
        ts += fminf(1.0f, s / a.trunc);
        ws += 1.0f;
        if (COLOR) {
#pragma unroll
            for (int k = 0; k < 3; ++k) cs[k] += a.color[px * 3 + k];
        }
    }
    if (!live) return;
    a.tsum[p] = ts;
    a.wsum[p] = ws;
    if (COLOR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a.csum[(int64_t)p * 3 + k] = cs[k];
    }
}

__global__ void tsdf_finalize_kernel(int n, const float* __restrict__ tsum, const float* __restrict__ wsum,
                                     const float* __restrict__ csum, float min_weight, float* __restrict__ u,
                                     float* __restrict__ rgb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float w = wsum[i];
    const bool seen = w >= min_weight;  // (min_weight >= 1: never a division by zero)
    u[i] = seen ? tsum[i] / w : __uint_as_float(0x7FC00000u);
    if (rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[(int64_t)i * 3 + k] = seen ? csum[(int64_t)i * 3 + k] / w : 0.0f;
    }
}

struct SampleArgs {
    int nx, ny, nz, C;
    float lo[3], hi[3];
    const float* attr;
    const float* mask;
    int64_t Q;
    const float* points;
    float fill;
    float* out;
};

// index position along one axis: the cell's lower index and the fraction inside it
__device__ __forceinline__ void axis_cell(float x, float lo, float hi, int n, int* i0, float* f) {
    float g = (x - lo) / (hi - lo) * (float)(n - 1);
    g = fminf(fmaxf(g, 0.0f), (float)(n - 1));  // (a NaN coordinate samples index 0, as fmaxf(NaN, 0))
    const int i = min((int)floorf(g), n - 2);
    *i0 = i;
    *f = g - (float)i;
}

__global__ void volume_sample_kernel(SampleArgs a) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.Q) return;
    int i0[3];
    float f[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
        axis_cell(a.points[q * 3 + ax], a.lo[ax], a.hi[ax], ax == 0 ? a.nx : ax == 1 ? a.ny : a.nz, &i0[ax], &f[ax]);
    const int64_t base = ((int64_t)i0[0] * a.ny + i0[1]) * a.nz + i0[2];  // the cell's corners are inside the grid
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wsum = 0.0f;
#pragma unroll
    for (int o = 0; o < 8; ++o) {  // corner o = ox + 2 oy + 4 oz, the mesher's numbering
        const int64_t idx = base + ((o & 1) ? (int64_t)a.ny * a.nz : 0) + ((o & 2) ? a.nz : 0) + ((o & 4) ? 1 : 0);
        if (a.mask && a.mask[idx] != a.mask[idx]) continue;  // NaN: unobserved, weight 0, attr not read
        const float wt = (((o & 1) ? f[0] : 1.0f - f[0]) * ((o & 2) ? f[1] : 1.0f - f[1])) * ((o & 4) ? f[2] : 1.0f - f[2]);
        wsum += wt;
        for (int c = 0; c < a.C; ++c) acc[c] += wt * a.attr[idx * a.C + c];  // bound: C <= 4
    }
    for (int c = 0; c < a.C; ++c) {
        float r = acc[c];
        if (a.mask) r = wsum > 0.0f ? r / wsum : a.fill;
        a.out[q * a.C + c] = r;
    }
}

int tsdf_dims(const char* who, int nx, int ny, int nz) {
    CN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, CN_ERR_SHAPE, "%s: dims %d x %d x %d (each at least 2)", who, nx, ny, nz);
    CN_REQUIRE((int64_t)nx * ny <= kMaxCount && (int64_t)nx * ny * nz <= kMaxCount, CN_ERR_SHAPE,
               "%s: dims %d x %d x %d too large (nx ny nz below 2^31)", who, nx, ny, nz);
    return CN_OK;
}

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" int cn_tsdf_integrate(const cn_tsdf_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_tsdf_integrate: null descriptor");
    int rc = tsdf_dims("cn_tsdf_integrate", d->nx, d->ny, d->nz);
    if (rc) return rc;
    CN_REQUIRE(d->N >= 0, CN_ERR_SHAPE, "cn_tsdf_integrate: N %d", d->N);
    CN_REQUIRE(d->h >= 1 && d->w >= 1 && (int64_t)d->h * d->w <= kMaxCount, CN_ERR_SHAPE,
               "cn_tsdf_integrate: image %d x %d (h w below 2^31)", d->h, d->w);
    CN_REQUIRE(d->trunc > 0.0f && d->trunc < INFINITY, CN_ERR_SHAPE, "cn_tsdf_integrate: trunc %g (positive and finite)",
               (double)d->trunc);
    CN_REQUIRE(d->near > 0.0f && d->near < INFINITY, CN_ERR_SHAPE, "cn_tsdf_integrate: near %g (positive and finite)",
               (double)d->near);
    CN_REQUIRE(d->depth_max > 0.0f, CN_ERR_SHAPE, "cn_tsdf_integrate: depth_max %g (positive, +inf for none)",
               (double)d->depth_max);
    if (d->N == 0) return CN_OK;
    CN_REQUIRE((d->color == nullptr) == (d->csum == nullptr), CN_ERR_ARG,
               "cn_tsdf_integrate: color and csum go together (both or neither)");
    CN_REQUIRE(d->proj && d->depth && d->tsum && d->wsum, CN_ERR_ARG, "cn_tsdf_integrate: null proj / depth / tsum / wsum");
    CN_REQUIRE((((uintptr_t)d->proj | (uintptr_t)d->depth | (uintptr_t)d->color | (uintptr_t)d->tsum | (uintptr_t)d->wsum |
                 (uintptr_t)d->csum) & 3) == 0,
               CN_ERR_ALIGN, "cn_tsdf_integrate: proj / depth / color / tsum / wsum / csum 4-byte aligned");
    TsdfArgs a{};
    a.nx = d->nx;
    a.ny = d->ny;
    a.nz = d->nz;
    for (int i = 0; i < 3; ++i) {
        a.lo[i] = d->lo[i];
        a.hi[i] = d->hi[i];
    }
    a.N = d->N;
    a.h = d->h;
    a.w = d->w;
    a.proj = d->proj;
    a.depth = d->depth;
    a.color = d->color;
    a.trunc = d->trunc;
    a.near = d->near;
    a.depth_max = d->depth_max;
    a.no_reject = d->no_reject;
    a.tsum = d->tsum;
    a.wsum = d->wsum;
    a.csum = d->csum;
    const int64_t nvox = (int64_t)d->nx * d->ny * d->nz;
    const unsigned blocks = (unsigned)((nvox + 255) / 256);
    if (d->color)
        tsdf_integrate_kernel<true><<<blocks, 256, 0, (hipStream_t)stream>>>(a);
    else
        tsdf_integrate_kernel<false><<<blocks, 256, 0, (hipStream_t)stream>>>(a);
    return check_launch("cn_tsdf_integrate");
}

extern "C" int cn_tsdf_finalize(const cn_tsdf_finalize_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_tsdf_finalize: null descriptor");
    int rc = tsdf_dims("cn_tsdf_finalize", d->nx, d->ny, d->nz);
    if (rc) return rc;
    CN_REQUIRE(d->min_weight >= 1.0f && d->min_weight < INFINITY, CN_ERR_SHAPE, "cn_tsdf_finalize: min_weight %g (at least 1)",
               (double)d->min_weight);
    CN_REQUIRE(d->tsum && d->wsum && d->u, CN_ERR_ARG, "cn_tsdf_finalize: null tsum / wsum / u");
    CN_REQUIRE(!d->rgb || d->csum, CN_ERR_ARG, "cn_tsdf_finalize: rgb without csum");
    CN_REQUIRE((((uintptr_t)d->tsum | (uintptr_t)d->wsum | (uintptr_t)d->csum | (uintptr_t)d->u | (uintptr_t)d->rgb) & 3) == 0,
               CN_ERR_ALIGN, "cn_tsdf_finalize: tsum / wsum / csum / u / rgb 4-byte aligned");
    const int n = d->nx * d->ny * d->nz;
    tsdf_finalize_kernel<<<(unsigned)(((int64_t)n + 255) / 256), 256, 0, (hipStream_t)stream>>>(n, d->tsum, d->wsum, d->csum,
                                                                                             d->min_weight, d->u, d->rgb);
    return check_launch("cn_tsdf_finalize");
}

extern "C" int cn_volume_sample(const cn_volume_sample_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_volume_sample: null descriptor");
    int rc = tsdf_dims("cn_volume_sample", d->nx, d->ny, d->nz);
    if (rc) return rc;
    CN_REQUIRE(d->C >= 1 && d->C <= 4, CN_ERR_SHAPE, "cn_volume_sample: C %d (1 to 4)", d->C);
    CN_REQUIRE(d->Q >= 0 && d->Q <= kMaxCount, CN_ERR_SHAPE, "cn_volume_sample: Q %lld (below 2^31)", (long long)d->Q);
    CN_REQUIRE(d->hi[0] > d->lo[0] && d->hi[1] > d->lo[1] && d->hi[2] > d->lo[2], CN_ERR_SHAPE,
               "cn_volume_sample: hi must exceed lo on every axis");
    if (d->Q == 0) return CN_OK;
    CN_REQUIRE(d->attr && d->points && d->out, CN_ERR_ARG, "cn_volume_sample: null attr / points / out");
    CN_REQUIRE((((uintptr_t)d->attr | (uintptr_t)d->mask | (uintptr_t)d->points | (uintptr_t)d->out) & 3) == 0, CN_ERR_ALIGN,
               "cn_volume_sample: attr / mask / points / out 4-byte aligned");
    SampleArgs a{};
    a.nx = d->nx;
    a.ny = d->ny;
    a.nz = d->nz;
    a.C = d->C;
    for (int i = 0; i < 3; ++i) {
        a.lo[i] = d->lo[i];
        a.hi[i] = d->hi[i];
    }
    a.attr = d->attr;
    a.mask = d->mask;
    a.Q = d->Q;
    a.points = d->points;
    a.fill = d->fill;
    a.out = d->out;
    volume_sample_kernel<<<(unsigned)((d->Q + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
    return check_launch("cn_volume_sample");
}
