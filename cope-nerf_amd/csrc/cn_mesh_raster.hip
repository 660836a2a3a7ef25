// cn_mesh_raster.hip — depth rendering of an indexed triangle mesh and the visibility of points under the rendered
// depth (additive to ABI v22): cn_mesh_raster / cn_mesh_visibility.  The reference has no rasteriser; the yardstick
// is a float64 restatement (tests/mesh_raster_ref.py).  The kernels see cameras only as 3 x 4 projections P with
// (a, b, c) = P [X, 1]: pixel (a / c, b / c), pixel centres at integers, depth c (copenerf.mesh.camera_projection).
//
// Arithmetic (fp32, -ffp-contract=off; tests/mesh_raster_ref.py restates it in numpy float32 to set the depth bound):
//   a = ((P00 x + P01 y) + P02 z) + P03, b and c alike;  sx = a / c, sy = b / c, iw = 1 / c          (per vertex)
//   E(l, h; p) = (hx - lx) (py - ly) - (hy - ly) (px - lx)   with l the corner of the SMALLER vertex index:
//   the edge function of an edge is evaluated from its endpoints in vertex-index order and negated for the triangle
//   that runs it from the larger index, so the two triangles of a shared edge get the same value with opposite
//   signs at every pixel and no pixel centre falls between them.  e_k is the edge opposite corner k.
//   covered: e_0, e_1, e_2 all >= 0 or all <= 0 (two-sided, inclusive)
//   depth = ((e_0 + e_1) + e_2) / ((e_0 iw_0 + e_1 iw_1) + e_2 iw_2)     (1 / c linear in screen space)
// Z-buffer: one 64-bit word per pixel, (depth bits << 32) | triangle id, resolved with a 64-bit atomicMin on global
// memory (a vector atomic): positive floats order like their bits, so the image does not depend on the order of
// arrival and equal depths go to the smaller triangle id.  There are no other atomics on the image.
//
// Two paths.  One thread per (triangle, view) sets the triangle up and walks its clamped bounding box when the box has
// at most pixel_budget pixels; a larger box is appended to the batch's deferred list -- one atomicAdd per wave (the
// ballot's population count), every lane writing at its rank -- and a second launch gives each listed triangle to a
// whole workgroup.  The list has room for every (triangle, view) of the batch, so it cannot overflow.
#include "cn_common.h"

#include <cmath>

namespace cn {
namespace {

constexpr size_t kAlign = 256;
size_t rup_sz(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

constexpr int64_t kMaxCount = ((int64_t)1 << 31) - 1;  // V, T, Q, h w, T x batch < 2^31
constexpr int kDefaultBatch = 8;
constexpr int kDefaultBudget = 64;
constexpr int kMaxGridY = 65535;
constexpr int kGroupBlocks = 4096;  // the workgroup path's grid: blocks stride over the deferred list
constexpr unsigned long long kEmpty = ((unsigned long long)0x7F800000u << 32) | 0xFFFFFFFFull;  // (+inf, -1)

struct RasterArgs {
    int64_t V, T;
    const float* vtx;
    const int32_t* tri;
    const float* proj;  // the batch's first view
    int B, h, w;
    float near;
    int budget;
    float4* pv;                 // [B][V]: (sx, sy, c, 1 / c)
    unsigned long long* z;      // [B][h][w]
    int2* list;                 // [T B]
    int32_t* n_deferred;
    unsigned long long* stats;  // [2] or null
    float* depth;               // the batch's first view
    int32_t* tri_out;
};

// (a, b, c) = P [x, y, z, 1] in the documented order
__device__ __forceinline__ void project(const float* __restrict__ P, float x, float y, float z, float* a, float* b, float* c) {
    *a = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    *b = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    *c = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
}

// the batch's z-buffer cleared, its deferred counter zeroed (and, before the first batch, the statistics)
__global__ void raster_fill_kernel(RasterArgs a, int clear_stats) {
    const int64_t n = (int64_t)a.B * a.h * a.w;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a.z[i] = kEmpty;
    if (i == 0) {
        *a.n_deferred = 0;
        if (clear_stats && a.stats) a.stats[0] = a.stats[1] = 0;
    }
}

__global__ void raster_project_kernel(RasterArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int v = blockIdx.y;
    if (i >= a.V) return;
    float pa, pb, pc;
    project(a.proj + (int64_t)v * 12, a.vtx[i * 3], a.vtx[i * 3 + 1], a.vtx[i * 3 + 2], &pa, &pb, &pc);
    a.pv[(int64_t)v * a.V + i] = make_float4(pa / pc, pb / pc, pc, 1.0f / pc);
}

// A triangle in one view: per edge k (opposite corner k) the corner of the smaller vertex index (lx, ly), the
// difference to the other (dx, dy) and the sign for this triangle's direction; the corners' 1 / c; the box.
struct TriSetup {
    float lx[3], ly[3], dx[3], dy[3], sg[3], iw[3];
    int x0, x1, y0, y1;
};

// false: the triangle is skipped in this view (a corner index outside [0, V), a corner at c < near or not finite,
// zero screen area, or a box that holds no pixel centre of the image)
__device__ __forceinline__ bool tri_setup(const RasterArgs& a, int64_t t, int v, TriSetup& s) {
    int32_t id[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        id[k] = a.tri[t * 3 + k];
        if (id[k] < 0 || id[k] >= a.V) return false;
    }
    float x[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float4 p = a.pv[(int64_t)v * a.V + id[k]];
        if (!(p.z >= a.near) || !(p.z < INFINITY)) return false;
        x[k] = p.x;
        y[k] = p.y;
        s.iw[k] = p.w;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;  // this triangle runs the edge i -> j
        const bool fwd = id[i] < id[j];
        const int l = fwd ? i : j, hgh = fwd ? j : i;
        s.lx[k] = x[l];
        s.ly[k] = y[l];
        s.dx[k] = x[hgh] - x[l];
        s.dy[k] = y[hgh] - y[l];
        s.sg[k] = fwd ? 1.0f : -1.0f;
    }
    // the screen area (twice, signed): edge 2 at corner 2
    const float area = s.sg[2] * (s.dx[2] * (y[2] - s.ly[2]) - s.dy[2] * (x[2] - s.lx[2]));
    if (!(fabsf(area) > 0.0f)) return false;  // (a NaN area too)
    const float fx0 = fmaxf(ceilf(fminf(x[0], fminf(x[1], x[2]))), 0.0f);
    const float fx1 = fminf(floorf(fmaxf(x[0], fmaxf(x[1], x[2]))), (float)(a.w - 1));
    const float fy0 = fmaxf(ceilf(fminf(y[0], fminf(y[1], y[2]))), 0.0f);
    const float fy1 = fminf(floorf(fmaxf(y[0], fmaxf(y[1], y[2]))), (float)(a.h - 1));
    if (!(fx0 <= fx1) || !(fy0 <= fy1)) return false;  // (NaN or infinite coordinates end here as well)
    s.x0 = (int)fx0;  // 0 <= fx0 <= fx1 <= w - 1: the conversions are in range
    s.x1 = (int)fx1;
    s.y0 = (int)fy0;
    s.y1 = (int)fy1;
    return true;
}

// pixel (x, y) of view v against triangle t: x in [0, w), y in [0, h) by tri_setup's clamped box
__device__ __forceinline__ void raster_pixel(const RasterArgs& a, const TriSetup& s, int v, int64_t t, int x, int y) {
    const float px = (float)x, py = (float)y;
    float e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) e[k] = s.sg[k] * (s.dx[k] * (py - s.ly[k]) - s.dy[k] * (px - s.lx[k]));
    const bool pos = e[0] >= 0.0f && e[1] >= 0.0f && e[2] >= 0.0f;
    const bool neg = e[0] <= 0.0f && e[1] <= 0.0f && e[2] <= 0.0f;
    if (!(pos || neg)) return;
    const float sum = (e[0] + e[1]) + e[2];
    const float num = (e[0] * s.iw[0] + e[1] * s.iw[1]) + e[2] * s.iw[2];
    const float d = sum / num;
    if (!(d > 0.0f) || !(d < INFINITY)) return;  // (0 / 0 where all three vanish)
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (uint32_t)t;
    unsigned long long* z = a.z + ((int64_t)v * a.h + y) * a.w + x;
    // (a plain read first: most fragments of a closed surface lose, and a load is cheaper than an atomic; the
    // word only ever falls, so a stale value costs an atomic, never a result)
    if (key < __atomic_load_n(z, __ATOMIC_RELAXED)) atomicMin(z, key);
}

__global__ void raster_thread_kernel(RasterArgs a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int v = blockIdx.y;
    const int lane = threadIdx.x & 63;
    TriSetup s;
    const bool live = t < a.T && tri_setup(a, t, v, s);  // (no early return: every lane reaches the ballots)
    bool defer = false;
    if (live) {
        const int bw = s.x1 - s.x0 + 1, bh = s.y1 - s.y0 + 1;
        defer = (int64_t)bw * bh > a.budget;
        if (!defer)
            for (int y = s.y0; y <= s.y1; ++y)        // bound: at most budget pixels
                for (int x = s.x0; x <= s.x1; ++x) raster_pixel(a, s, v, t, x, y);
    }
    const unsigned long long m = __ballot(defer);
    if (m) {  // (the same in every lane of the wave)
        const int leader = __ffsll(m) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(a.n_deferred, (int)__popcll(m));
        base = __shfl(base, leader, kWave);
        // base + rank < T B: every (triangle, view) of the batch is appended at most once
        if (defer) a.list[base + __popcll(m & ((1ull << lane) - 1))] = make_int2((int)t, v);
    }
    if (a.stats) {
        const unsigned long long r = __ballot(live && !defer);
        if (r && lane == __ffsll(r) - 1) atomicAdd(a.stats, (unsigned long long)__popcll(r));
    }
}

__global__ void raster_group_kernel(RasterArgs a) {
    const int n = *a.n_deferred;  // (at most T B: the list's size)
    if (a.stats && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(a.stats + 1, (unsigned long long)n);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const int2 e = a.list[i];
        TriSetup s;
        if (!tri_setup(a, e.x, e.y, s)) continue;  // (never: it passed in the first launch)
        const int bw = s.x1 - s.x0 + 1;
        const int npx = bw * (s.y1 - s.y0 + 1);  // <= h w < 2^31
        for (int p = threadIdx.x; p < npx; p += blockDim.x) raster_pixel(a, s, e.y, e.x, s.x0 + p % bw, s.y0 + p / bw);
    }
}

__global__ void raster_unpack_kernel(RasterArgs a) {
    const int64_t n = (int64_t)a.B * a.h * a.w;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = a.z[i];
    a.depth[i] = __uint_as_float((uint32_t)(k >> 32));
    a.tri_out[i] = (int32_t)(uint32_t)k;
}

struct RasterPlan {
    int B;
    float4* pv;
    unsigned long long* z;
    int2* list;
    int32_t* n_deferred;
    size_t bytes;
};

// views per pass: view_batch (0: 8), at most N, at most 65535 (the grid's y) and small enough for T B < 2^31 (the
// deferred list's counter) and B h w < 2^31 (the pixel launches' grids)
int raster_batch(int64_t T, int N, int64_t hw, int view_batch) {
    int64_t B = view_batch ? view_batch : kDefaultBatch;
    if (B > N) B = N;
    if (B > kMaxGridY) B = kMaxGridY;
    if (T > 0 && B > kMaxCount / T) B = kMaxCount / T;
    if (B > kMaxCount / hw) B = kMaxCount / hw;
    return B < 1 ? 1 : (int)B;
}

RasterPlan raster_plan(int64_t V, int64_t T, int N, int h, int w, int view_batch, void* ws) {
    RasterPlan p{};
    p.B = raster_batch(T, N, (int64_t)h * w, view_batch);
    char* b = static_cast<char*>(ws);
    size_t used = 0;
    auto take = [&](size_t n) {
        char* q = b ? b + used : nullptr;
        used += rup_sz(n);
        return q;
    };
    p.z = reinterpret_cast<unsigned long long*>(take((size_t)p.B * h * w * 8));
    p.pv = reinterpret_cast<float4*>(take((size_t)p.B * V * 16));
    p.list = reinterpret_cast<int2*>(take((size_t)p.B * T * 8));
    p.n_deferred = reinterpret_cast<int32_t*>(take(4));
    p.bytes = used;
    return p;
}

int raster_sizes(const char* who, int64_t V, int64_t T, int N, int h, int w, int view_batch) {
    CN_REQUIRE(V >= 0 && V <= kMaxCount && T >= 0 && T <= kMaxCount, CN_ERR_SHAPE, "%s: V %lld, T %lld (each below 2^31)", who,
               (long long)V, (long long)T);
    CN_REQUIRE(N >= 0, CN_ERR_SHAPE, "%s: N %d", who, N);
    CN_REQUIRE(h >= 1 && w >= 1 && (int64_t)h * w <= kMaxCount, CN_ERR_SHAPE, "%s: image %d x %d (h w below 2^31)", who, h, w);
    CN_REQUIRE(view_batch >= 0, CN_ERR_SHAPE, "%s: view_batch %d", who, view_batch);
    return CN_OK;
}

__global__ void visibility_kernel(int64_t Q, const float* __restrict__ pts, int N, int h, int w, float near,
                                  const float* __restrict__ proj, const float* __restrict__ depth, float tol_abs, float tol_rel,
                                  int32_t* __restrict__ count) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= Q) return;
    const float x = pts[q * 3], y = pts[q * 3 + 1], z = pts[q * 3 + 2];
    const float one_rel = 1.0f + tol_rel;
    int n = 0;
    for (int v = 0; v < N; ++v) {  // bound: the views
        float pa, pb, pc;
        project(proj + (int64_t)v * 12, x, y, z, &pa, &pb, &pc);
        if (!(pc >= near)) continue;
        const float fx = floorf(pa / pc + 0.5f), fy = floorf(pb / pc + 0.5f);
        if (!(fx >= 0.0f && fx <= (float)(w - 1) && fy >= 0.0f && fy <= (float)(h - 1))) continue;  // (NaN: outside)
        if (depth) {
            const float d = depth[((int64_t)v * h + (int)fy) * w + (int)fx];  // in range by the test above
            if (!(pc <= d * one_rel + tol_abs)) continue;
        }
        ++n;
    }
    count[q] = n;
}

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" size_t cn_mesh_raster_workspace_bytes(int64_t V, int64_t T, int32_t N, int32_t h, int32_t w, int32_t view_batch) {
    if (raster_sizes("cn_mesh_raster_workspace_bytes", V, T, N, h, w, view_batch) != CN_OK) return 0;
    return raster_plan(V, T, N, h, w, view_batch, nullptr).bytes;
}

extern "C" int cn_mesh_raster(const cn_mesh_raster_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_mesh_raster: null descriptor");
    int rc = raster_sizes("cn_mesh_raster", d->V, d->T, d->N, d->h, d->w, d->view_batch);
    if (rc) return rc;
    CN_REQUIRE(d->near > 0.0f && d->near < INFINITY, CN_ERR_SHAPE, "cn_mesh_raster: near %g (positive and finite)", (double)d->near);
    CN_REQUIRE(d->pixel_budget >= 0, CN_ERR_SHAPE, "cn_mesh_raster: pixel_budget %d", d->pixel_budget);
    if (d->N == 0) return CN_OK;
    CN_REQUIRE(d->proj && d->depth && d->tri, CN_ERR_ARG, "cn_mesh_raster: null proj / depth / tri");
    CN_REQUIRE((d->V == 0 || d->vertices) && (d->T == 0 || d->triangles), CN_ERR_ARG, "cn_mesh_raster: null vertices / triangles");
    CN_REQUIRE((((uintptr_t)d->vertices | (uintptr_t)d->triangles | (uintptr_t)d->proj | (uintptr_t)d->depth | (uintptr_t)d->tri) & 3) == 0 &&
                   ((uintptr_t)d->stats & 7) == 0,
               CN_ERR_ALIGN, "cn_mesh_raster: vertices / triangles / proj / depth / tri 4-byte, stats 8-byte aligned");
    const RasterPlan p = raster_plan(d->V, d->T, d->N, d->h, d->w, d->view_batch, workspace);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= p.bytes, CN_ERR_SHAPE,
               "cn_mesh_raster: workspace %lld bytes, %zu needed", (long long)workspace_bytes, p.bytes);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_mesh_raster: workspace not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    RasterArgs a{};
    a.V = d->V;
    a.T = d->T;
    a.vtx = d->vertices;
    a.tri = d->triangles;
    a.h = d->h;
    a.w = d->w;
    a.near = d->near;
    a.budget = d->pixel_budget ? d->pixel_budget : kDefaultBudget;
    a.pv = p.pv;
    a.z = p.z;
    a.list = p.list;
    a.n_deferred = p.n_deferred;
    a.stats = reinterpret_cast<unsigned long long*>(d->stats);
    const int64_t hw = (int64_t)d->h * d->w;
    for (int v0 = 0; v0 < d->N; v0 += p.B) {
        a.B = d->N - v0 < p.B ? d->N - v0 : p.B;
        a.proj = d->proj + (int64_t)v0 * 12;
        a.depth = d->depth + v0 * hw;
        a.tri_out = d->tri + v0 * hw;
        const unsigned px_blocks = (unsigned)((a.B * hw + 255) / 256);  // B h w < 2^31 (raster_batch)
        raster_fill_kernel<<<px_blocks, 256, 0, st>>>(a, v0 == 0);
        if ((rc = check_launch("cn_mesh_raster"))) return rc;
        if (d->V > 0 && d->T > 0) {
            raster_project_kernel<<<dim3((unsigned)((d->V + 255) / 256), a.B), 256, 0, st>>>(a);
            if ((rc = check_launch("cn_mesh_raster"))) return rc;
            raster_thread_kernel<<<dim3((unsigned)((d->T + 255) / 256), a.B), 256, 0, st>>>(a);
            if ((rc = check_launch("cn_mesh_raster"))) return rc;
            const int64_t pairs = d->T * a.B;
            raster_group_kernel<<<(unsigned)(pairs < kGroupBlocks ? pairs : kGroupBlocks), 256, 0, st>>>(a);
            if ((rc = check_launch("cn_mesh_raster"))) return rc;
        }
        raster_unpack_kernel<<<px_blocks, 256, 0, st>>>(a);
        if ((rc = check_launch("cn_mesh_raster"))) return rc;
    }
    return CN_OK;
}

extern "C" int cn_mesh_visibility(const cn_mesh_visibility_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_mesh_visibility: null descriptor");
    CN_REQUIRE(d->Q >= 0 && d->Q <= kMaxCount, CN_ERR_SHAPE, "cn_mesh_visibility: Q %lld (below 2^31)", (long long)d->Q);
    CN_REQUIRE(d->N >= 0, CN_ERR_SHAPE, "cn_mesh_visibility: N %d", d->N);
    CN_REQUIRE(d->h >= 1 && d->w >= 1 && (int64_t)d->h * d->w <= kMaxCount, CN_ERR_SHAPE,
               "cn_mesh_visibility: image %d x %d (h w below 2^31)", d->h, d->w);
    CN_REQUIRE(d->near > 0.0f && d->near < INFINITY, CN_ERR_SHAPE, "cn_mesh_visibility: near %g (positive and finite)",
               (double)d->near);
    CN_REQUIRE(d->tol_abs >= 0.0f && d->tol_rel >= 0.0f, CN_ERR_SHAPE, "cn_mesh_visibility: tol_abs %g, tol_rel %g",
               (double)d->tol_abs, (double)d->tol_rel);
    if (d->Q == 0) return CN_OK;
    CN_REQUIRE(d->points && d->count && (d->N == 0 || d->proj), CN_ERR_ARG, "cn_mesh_visibility: null points / count / proj");
    CN_REQUIRE((((uintptr_t)d->points | (uintptr_t)d->count | (uintptr_t)d->proj | (uintptr_t)d->depth) & 3) == 0, CN_ERR_ALIGN,
               "cn_mesh_visibility: points / count / proj / depth 4-byte aligned");
    visibility_kernel<<<(unsigned)((d->Q + 255) / 256), 256, 0, (hipStream_t)stream>>>(d->Q, d->points, d->N, d->h, d->w, d->near,
                                                                                     d->proj, d->depth, d->tol_abs, d->tol_rel,
                                                                                     d->count);
    return check_launch("cn_mesh_visibility");
}
