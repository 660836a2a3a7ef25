// cn_mesh_eval.hip — mesh geometry metrics (additive to ABI v22): points drawn uniformly by area on an indexed
// triangle list (cn_mesh_area / cn_mesh_sample), the exact nearest neighbour between two point clouds through a
// uniform grid (cn_nn_grid_build / cn_nn_query) and the statistics Chamfer distance and F-score are made of
// (cn_cloud_stats).  The reference has no geometry metric; the yardstick is float64 brute force (tests/mesh_eval_ref.py).
// ICP registration of a cloud to the targets of such a grid sits on the same search: a similarity applied by one
// device function (cn_cloud_transform; the correspondences are cn_nn_query over its output) and the reduction of the
// pairs into the 32 sums of a closed-form step (cn_icp_accumulate); the yardstick is tests/icp_ref.py.
// The exact k nearest neighbours on the same grid (cn_knn_query, the k-best list in LDS) feed the point-cloud
// preparation passes of cn_cloud.hip; the yardstick is tests/cloud_ref.py.
//
// Determinism.  The area scan is a nest of SEQUENTIAL sums, not a tree: a thread sums its 4 triangles in order,
// a wave its 64 threads in lane order, a tile its 4 waves in order, and one wave the tile totals in order; every
// level's running base is the sequential sum of the level below's totals, and an entry is
//   cdf[t] = B_tile + (W_wave + (P_lane + partial_j)).
// A total is the last inclusive value of its level, so the value at a boundary is the next unit's base bit for
// bit: cdf never falls, and a zero-area triangle repeats its predecessor exactly (x + 0 = x at every level).
// "The first t with cdf[t] > x" therefore never names a zero-area triangle, and area = cdf[T - 1].  There are no
// floating-point atomics anywhere; the grid's histogram and scatter use integer atomics, which make the counts
// exact and leave only the order inside a cell to scheduling -- cn_nn_query's (distance, index) minimum does
// not depend on that order.  cn_cloud_stats reduces in a fixed order (strided per thread, a fixed tree per
// block, one block over the block partials).
#include "cn_common.h"

#include <cmath>

namespace cn {
namespace {

constexpr size_t kAlign = 256;
size_t rup_sz(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

constexpr int64_t kMaxCount = ((int64_t)1 << 31) - 1;  // N, Q, S, T < 2^31
constexpr int64_t kMaxCells = (int64_t)1 << 26;

// ---- area-weighted surface sampling ---------------------------------------------------------------------

// The area of triangle t in double from its fp32 corners; 0 for a corner index outside [0, V) and for an area
// that is not finite (a NaN corner), so neither is ever drawn.
__device__ __forceinline__ double tri_area(const float* __restrict__ v, const int32_t* __restrict__ tri, int64_t V,
                                           int64_t t) {
    const int32_t i0 = tri[t * 3], i1 = tri[t * 3 + 1], i2 = tri[t * 3 + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return 0.0;
    const double ax = v[(int64_t)i0 * 3], ay = v[(int64_t)i0 * 3 + 1], az = v[(int64_t)i0 * 3 + 2];
    const double ux = (double)v[(int64_t)i1 * 3] - ax, uy = (double)v[(int64_t)i1 * 3 + 1] - ay,
                 uz = (double)v[(int64_t)i1 * 3 + 2] - az;
    const double wx = (double)v[(int64_t)i2 * 3] - ax, wy = (double)v[(int64_t)i2 * 3 + 1] - ay,
                 wz = (double)v[(int64_t)i2 * 3 + 2] - az;
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    const double a = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    return (a == a && a < INFINITY) ? a : 0.0;
}

// carry + s_0 + ... + s_(lane - 1), added one lane at a time in lane order (64 steps; the same value in every
// lane of p); *total = carry + all 64.
__device__ __forceinline__ double wave_seq_scan(double s, int lane, double carry, double* total) {
    double p = carry, mine = carry;
    for (int l = 0; l < kWave; ++l) {  // bound: the wave's 64 lanes
        if (lane == l) mine = p;
        p = p + __shfl(s, l, kWave);
    }
    *total = p;
    return mine;
}

// launch 1: cdf[t] = the inclusive sum inside t's tile, tot[b] = the sum of tile b
__global__ void __launch_bounds__(kScanThreads) area_tile_kernel(int64_t V, int64_t T, const float* __restrict__ v,
                                                                 const int32_t* __restrict__ tri,
                                                                 double* __restrict__ cdf, double* __restrict__ tot) {
    __shared__ double wtot[kScanThreads / kWave];
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    double part[kScanItems], run = 0.0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        run = run + (i0 + j < T ? tri_area(v, tri, V, i0 + j) : 0.0);
        part[j] = run;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double wave_total;
    const double P = wave_seq_scan(run, lane, 0.0, &wave_total);
    if (lane == 0) wtot[w] = wave_total;
    __syncthreads();
    double W = 0.0, all = 0.0;
#pragma unroll
    for (int i = 0; i < kScanThreads / kWave; ++i) {
        if (i == w) W = all;
        all = all + wtot[i];
    }
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (i0 + j < T) cdf[i0 + j] = W + (P + part[j]);
    if (threadIdx.x == 0) tot[blockIdx.x] = all;
}

// launch 2 (one wave): tot[] -> its exclusive sequential sums in place, *area = the grand total
__global__ void __launch_bounds__(kWave) area_totals_kernel(double* __restrict__ tot, int nt, double* __restrict__ area) {
    const int lane = threadIdx.x;
    double carry = 0.0;
    for (int base = 0; base < nt; base += kWave) {  // bound: ceil(nt / 64) rounds
        const int i = base + lane;
        const double x = i < nt ? tot[i] : 0.0;
        double next;
        const double mine = wave_seq_scan(x, lane, carry, &next);
        if (i < nt) tot[i] = mine;
        carry = next;
    }
    if (lane == 0) *area = carry;
}

// launch 3: cdf[t] = tot[tile of t] + cdf[t]
__global__ void __launch_bounds__(kScanThreads) area_apply_kernel(int64_t T, const double* __restrict__ tot,
                                                                  double* __restrict__ cdf) {
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    const double B = tot[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (i0 + j < T) cdf[i0 + j] = B + cdf[i0 + j];
}

struct SampleArgs {
    int64_t V, T, S;
    const float* v;
    const int32_t* tri;
    const double* cdf;
    const double* area;
    const uint64_t* philox;
    float* points;
    int32_t* tri_out;
};

// Sample i: (u0, u1, u2) = words 0, 1, 2 of Philox4x32-10(counter (i, offset), key seed), each >> 8, x 2^-24 --
// elements 4 i, 4 i + 1, 4 i + 2 of cn_uniform_philox's stream for the same (seed, offset); word 3 is unused.
__global__ void __launch_bounds__(256) mesh_sample_kernel(SampleArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.S) return;
    const uint64_t seed = a.philox[0], off = a.philox[1];
    uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u0 = (float)(c[0] >> 8) * (1.0f / 16777216.0f), u1 = (float)(c[1] >> 8) * (1.0f / 16777216.0f),
                u2 = (float)(c[2] >> 8) * (1.0f / 16777216.0f);
    const double A = *a.area;
    const double x = (double)u0 * A;
    // the first t with cdf[t] > x; u0 < 1 and A = cdf[T - 1] > 0 give x < cdf[T - 1], so there is one
    int64_t lo = 0, hi = a.T;
    for (int it = 0; it < 32 && lo < hi; ++it) {  // bound: T < 2^31 halves to nothing in 31 steps
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.cdf[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    int64_t t = lo < a.T ? lo : a.T - 1;
    int32_t i0 = 0, i1 = 0, i2 = 0;
    bool ok = A > 0.0 && t >= 0;
    if (ok) {
        i0 = a.tri[t * 3];
        i1 = a.tri[t * 3 + 1];
        i2 = a.tri[t * 3 + 2];
        ok = i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < a.V && i1 < a.V && i2 < a.V;
    }
    float p[3] = {0.f, 0.f, 0.f};
    if (ok) {
        const float r = sqrtf(u1);
        const float w0 = 1.0f - r, w1 = r * (1.0f - u2), w2 = r * u2;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
            p[ax] = (w0 * a.v[(int64_t)i0 * 3 + ax] + w1 * a.v[(int64_t)i1 * 3 + ax]) + w2 * a.v[(int64_t)i2 * 3 + ax];
    }
    // (a mesh of zero area has nothing to draw from: zeros and triangle -1)
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) a.points[i * 3 + ax] = p[ax];
    if (a.tri_out) a.tri_out[i] = ok ? (int32_t)t : -1;
}

struct SamplePlan {
    double* cdf;
    double* tot;
    int nt;
    size_t bytes;
};

SamplePlan sample_plan(int64_t T, void* ws) {
    SamplePlan p{};
    p.nt = (int)((T + kScanTile - 1) / kScanTile);
    if (p.nt < 1) p.nt = 1;
    char* b = static_cast<char*>(ws);
    const size_t cdf_bytes = rup_sz((size_t)T * 8);
    p.cdf = reinterpret_cast<double*>(b);
    p.tot = reinterpret_cast<double*>(b ? b + cdf_bytes : nullptr);
    p.bytes = cdf_bytes + rup_sz((size_t)p.nt * 8);
    return p;
}

int sample_check(const char* who, const cn_mesh_sample_desc* d, const void* ws, int64_t ws_bytes, bool draw) {
    CN_REQUIRE(d, CN_ERR_ARG, "%s: null descriptor", who);
    CN_REQUIRE(d->V >= 0 && d->T >= 0 && d->V <= kMaxCount && d->T <= kMaxCount, CN_ERR_SHAPE,
               "%s: V %lld, T %lld (each in [0, 2^31))", who, (long long)d->V, (long long)d->T);
    CN_REQUIRE((d->V == 0 || d->vertices) && (d->T == 0 || d->triangles) && d->area, CN_ERR_ARG,
               "%s: null vertices / triangles / area", who);
    CN_REQUIRE(((uintptr_t)d->vertices & 3) == 0 && ((uintptr_t)d->triangles & 3) == 0 && ((uintptr_t)d->area & 7) == 0,
               CN_ERR_ALIGN, "%s: vertices / triangles 4-byte, area 8-byte aligned", who);
    if (draw) {
        CN_REQUIRE(d->S >= 0 && d->S <= kMaxCount, CN_ERR_SHAPE, "%s: S %lld (in [0, 2^31))", who, (long long)d->S);
        CN_REQUIRE(d->S == 0 || d->T > 0, CN_ERR_SHAPE, "%s: %lld samples of a mesh without triangles", who,
                   (long long)d->S);
        CN_REQUIRE(d->S == 0 || (d->philox && d->points), CN_ERR_ARG, "%s: null philox / points", who);
        CN_REQUIRE(((uintptr_t)d->philox & 7) == 0 && ((uintptr_t)d->points & 3) == 0 && ((uintptr_t)d->tri & 3) == 0,
                   CN_ERR_ALIGN, "%s: philox 8-byte, points / tri 4-byte aligned", who);
    }
    const size_t need = sample_plan(d->T, nullptr).bytes;
    CN_REQUIRE(ws && ws_bytes >= 0 && (size_t)ws_bytes >= need, CN_ERR_SHAPE, "%s: workspace %lld bytes, %zu needed", who,
               (long long)ws_bytes, need);
    CN_REQUIRE(((uintptr_t)ws & (kAlign - 1)) == 0, CN_ERR_ALIGN, "%s: workspace not 256-byte aligned", who);
    return CN_OK;
}

// ---- the uniform grid and the nearest-neighbour search ---------------------------------------------------

struct Grid {
    float o[3];
    float cell;
    int d[3];
};

// The cell index of coordinate p on one axis: floor((p - o) / cell) clamped into [0, dim) -- a point outside
// the grid goes to the nearest boundary cell, a NaN to cell 0.  fl(fl(p - o) / cell) never falls as p grows.
__device__ __forceinline__ int axis_cell(float p, float o, float cell, int dim) {
    const float f = (p - o) / cell;
    return f >= 0.0f ? (f < (float)dim ? (int)f : dim - 1) : 0;
}

__device__ __forceinline__ int cell_id(const Grid& g, float x, float y, float z) {
    const int ix = axis_cell(x, g.o[0], g.cell, g.d[0]), iy = axis_cell(y, g.o[1], g.cell, g.d[1]),
              iz = axis_cell(z, g.o[2], g.cell, g.d[2]);
    return (ix * g.d[1] + iy) * g.d[2] + iz;
}

__global__ void zero_cells_kernel(int n, int32_t* __restrict__ p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

__global__ void grid_count_kernel(Grid g, int64_t N, const float* __restrict__ pts, int32_t* __restrict__ id,
                                  int32_t* count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int c = cell_id(g, pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]);
    id[i] = c;
    atomicAdd(count + c, 1);
}

__global__ void cells_reduce_kernel(const int32_t* __restrict__ c, int n, int32_t* __restrict__ tot) {
    const int i0 = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int x = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) x += i0 + j < n ? c[i0 + j] : 0;
    int all;
    block_excl_scan(x, &all);
    if (threadIdx.x == 0) tot[blockIdx.x] = all;
}

// one block: tot[] -> its exclusive scan in place, *total (cell_start[ncells]) = the grand total
__global__ void cells_totals_kernel(int32_t* __restrict__ tot, int nt, int32_t* __restrict__ total) {
    int carry = 0;
    for (int base = 0; base < nt; base += kScanTile) {  // bound: ceil(nt / 1024) rounds
        const int i0 = base + threadIdx.x * kScanItems;
        int v[kScanItems], x = 0;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            v[j] = i0 + j < nt ? tot[i0 + j] : 0;
            x += v[j];
        }
        int all;
        int run = carry + block_excl_scan(x, &all);
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            if (i0 + j < nt) tot[i0 + j] = run;
            run += v[j];
        }
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ void cells_apply_kernel(const int32_t* __restrict__ c, int n, const int32_t* __restrict__ tot,
                                   int32_t* __restrict__ start) {
    const int i0 = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int v[kScanItems], x = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        v[j] = i0 + j < n ? c[i0 + j] : 0;
        x += v[j];
    }
    int all;
    int run = tot[blockIdx.x] + block_excl_scan(x, &all);
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (i0 + j < n) start[i0 + j] = run;
        run += v[j];
    }
}

// Point i takes one of its cell's slots: the count falls from the cell's size to 0, so the slots handed out
// are exactly [start, start + size), in an order that is the atomics'.
__global__ void grid_scatter_kernel(int64_t N, const float* __restrict__ pts, const int32_t* __restrict__ id,
                                    const int32_t* __restrict__ start, int32_t* count, floatx4* __restrict__ sorted) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int c = id[i];
    const int64_t slot = (int64_t)start[c] + atomicSub(count + c, 1) - 1;
    if (slot < 0 || slot >= N) return;  // (never: the counts are this launch sequence's own)
    floatx4 r;
    r[0] = pts[i * 3];
    r[1] = pts[i * 3 + 1];
    r[2] = pts[i * 3 + 2];
    r[3] = __int_as_float((int)i);
    sorted[slot] = r;
}

struct GridPlan {
    int32_t* id;
    int32_t* count;
    int32_t* tot;
    int nt;
    size_t bytes;
};

GridPlan grid_plan(int64_t N, int64_t ncells, void* ws) {
    GridPlan p{};
    p.nt = (int)((ncells + kScanTile - 1) / kScanTile);
    char* b = static_cast<char*>(ws);
    size_t used = 0;
    auto take = [&](size_t n) {
        char* q = b ? b + used : nullptr;
        used += rup_sz(n);
        return q;
    };
    p.id = reinterpret_cast<int32_t*>(take((size_t)N * 4));
    p.count = reinterpret_cast<int32_t*>(take((size_t)ncells * 4));
    p.tot = reinterpret_cast<int32_t*>(take((size_t)p.nt * 4));
    p.bytes = used;
    return p;
}

// the grid's own fields (no device pointer is read): *ncells = the number of cells
int grid_check(const char* who, const cn_nn_grid_desc* g, int64_t* ncells) {
    CN_REQUIRE(g, CN_ERR_ARG, "%s: null grid descriptor", who);
    CN_REQUIRE(g->N >= 0 && g->N <= kMaxCount, CN_ERR_SHAPE, "%s: N %lld (in [0, 2^31))", who, (long long)g->N);
    CN_REQUIRE(g->dims[0] >= 1 && g->dims[1] >= 1 && g->dims[2] >= 1, CN_ERR_SHAPE, "%s: dims %d x %d x %d", who,
               g->dims[0], g->dims[1], g->dims[2]);
    // (each factor is below 2^31, so the first product fits 64 bits and is checked before the second)
    const int64_t xy = (int64_t)g->dims[0] * g->dims[1];
    CN_REQUIRE(xy <= kMaxCells && xy * g->dims[2] <= kMaxCells, CN_ERR_SHAPE,
               "%s: dims %d x %d x %d are more than 2^26 cells", who, g->dims[0], g->dims[1], g->dims[2]);
    CN_REQUIRE(g->cell > 0.0f && g->cell < INFINITY, CN_ERR_SHAPE, "%s: cell size %g", who, (double)g->cell);
    for (int i = 0; i < 3; ++i)
        CN_REQUIRE(std::isfinite(g->origin[i]), CN_ERR_SHAPE, "%s: origin[%d] is not finite", who, i);
    CN_REQUIRE(g->cell_start && (g->N == 0 || g->sorted), CN_ERR_ARG, "%s: null cell_start / sorted", who);
    CN_REQUIRE(((uintptr_t)g->cell_start & 3) == 0 && ((uintptr_t)g->sorted & 15) == 0, CN_ERR_ALIGN,
               "%s: cell_start 4-byte, sorted 16-byte aligned", who);
    *ncells = xy * g->dims[2];
    return CN_OK;
}

Grid grid_of(const cn_nn_grid_desc* g) {
    Grid o{};
    for (int i = 0; i < 3; ++i) {
        o.o[i] = g->origin[i];
        o.d[i] = g->dims[i];
    }
    o.cell = g->cell;
    return o;
}

struct QueryArgs {
    Grid g;
    int64_t N, Q;
    const float* q;
    int records;
    const floatx4* sorted;
    const int32_t* start;
    float max_dist;
    float* dist;
    int32_t* index;
    int maxdim;
};

// The records [s, e) against the best (squared distance, original index) so far, the smaller index on a tie.
__device__ __forceinline__ void scan_records(const QueryArgs& a, int s, int e, float qx, float qy, float qz,
                                             float* best, int* bi) {
    s = s < 0 ? 0 : s;
    e = (int64_t)e > a.N ? (int)a.N : e;  // (cell_start is the build's: the clamps only bound a foreign array)
    for (int j = s; j < e; ++j) {         // bound: e - s <= N records
        const floatx4 r = a.sorted[j];    // one 16-byte load per record
        const float dx = r[0] - qx, dy = r[1] - qy, dz = r[2] - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int idx = __float_as_int(r[3]);
        if (d2 < *best || (d2 == *best && idx < *bi)) {
            *best = d2;
            *bi = idx;
        }
    }
}

// One lane per query.  Shell k is the cells at Chebyshev index distance k from the query's (clamped) cell c;
// after shells 0 .. k an unvisited target p has, on some axis a, either
//   cell_a(p) >= c_a + k + 1  (only if c_a + k + 1 <= dim_a - 1), or  cell_a(p) <= c_a - k - 1  (only if >= 0).
// cell_a(p) = clamp(floor(f(p))) with f(p) = fl(fl(p_a - o_a) / cell), which never falls as p_a grows.  In the
// first case f(p) >= m = c_a + k + 1 >= 1 (a cell clamped from above has f >= dim_a > m), so, with e = 2^-24,
// p_a - o_a >= m cell (1 - 2 e): p_a - q_a >= (o_a + m cell) - q_a - 2 e m cell.  In the second f(p) < c_a - k
// (a cell clamped from below has f < 0), so q_a - p_a > q_a - (o_a + (c_a - k) cell) - 2 e dim_a cell.
// Nothing here asks that q lie inside the grid: its own cell only chooses where the shells start, and the two
// walls are compared with q_a itself, so a query outside sees the (larger) true gaps.  The walls and the gaps
// are computed in fp32, each step within e of its operands: in all within 6 e (|o_a| + |q_a| + dim_a cell) of
// the exact values.  lb = (the smallest gap over the sides that still have cells) - slack, slack = 16 e times
// the largest such sum, times (1 - 16 e), is therefore below every unvisited target's true distance by more
// than the few e that the fp32 distance arithmetic can lose, and
//   best < lb^2  =>  no unvisited target reaches, or ties, the best squared distance as this kernel computes it;
//   lb >= max_dist  =>  no unvisited target is within max_dist.
// No side with cells left: every cell has been visited.  Targets outside the grid sit in boundary cells and are
// covered by the same argument (the clamped cases above).  A query far outside the grid of a cloud that also has
// targets outside it cannot stop before the shells leave the grid, since such targets may lie anywhere: it costs
// a full scan, exact all the same; a finite max_dist stops it at once.
__global__ void __launch_bounds__(256) nn_query_kernel(QueryArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.Q) return;
    float q[3];
    int64_t out = i;
    if (a.records) {
        const floatx4 r = reinterpret_cast<const floatx4*>(a.q)[i];
        q[0] = r[0];
        q[1] = r[1];
        q[2] = r[2];
        out = __float_as_int(r[3]);
        if (out < 0 || out >= a.Q) return;  // (never for cn_nn_grid_build's records)
    } else {
        q[0] = a.q[i * 3];
        q[1] = a.q[i * 3 + 1];
        q[2] = a.q[i * 3 + 2];
    }
    int c[3];
    float slack = 0.0f;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        c[ax] = axis_cell(q[ax], a.g.o[ax], a.g.cell, a.g.d[ax]);
        slack = fmaxf(slack, (fabsf(a.g.o[ax]) + fabsf(q[ax]) + (float)a.g.d[ax] * a.g.cell) * (1.0f / 1048576.0f));
    }
    const int ny = a.g.d[1], nz = a.g.d[2];
    float best = INFINITY;
    int bi = -1;
    // bound: the grid's largest dimension -- shell maxdim - 1 around any cell holds every cell of the grid
    for (int k = 0; k < a.maxdim; ++k) {
        const int x0 = max(c[0] - k, 0), x1 = min(c[0] + k, a.g.d[0] - 1);
        const int y0 = max(c[1] - k, 0), y1 = min(c[1] + k, ny - 1);
        const int z0 = max(c[2] - k, 0), z1 = min(c[2] + k, nz - 1);
        for (int x = x0; x <= x1; ++x) {      // bound: 2 k + 1
            for (int y = y0; y <= y1; ++y) {  // bound: 2 k + 1
                const int row = (x * ny + y) * nz;
                if (abs(x - c[0]) == k || abs(y - c[1]) == k) {
                    // a face row of the shell: its cells z0 .. z1 are one run of records (z is the fastest index)
                    scan_records(a, a.start[row + z0], a.start[row + z1 + 1], q[0], q[1], q[2], &best, &bi);
                } else {
                    // an inner row: the two end cells, where they are inside the grid
                    const int za = c[2] - k, zb = c[2] + k;
                    if (za >= 0) scan_records(a, a.start[row + za], a.start[row + za + 1], q[0], q[1], q[2], &best, &bi);
                    if (zb < nz) scan_records(a, a.start[row + zb], a.start[row + zb + 1], q[0], q[1], q[2], &best, &bi);
                }
            }
        }
        float lb = INFINITY;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (c[ax] + k + 1 <= a.g.d[ax] - 1) lb = fminf(lb, (a.g.o[ax] + (float)(c[ax] + k + 1) * a.g.cell) - q[ax]);
            if (c[ax] - k - 1 >= 0) lb = fminf(lb, q[ax] - (a.g.o[ax] + (float)(c[ax] - k) * a.g.cell));
        }
        if (lb == INFINITY) break;  // the shell left the grid on every side
        lb = (lb - slack) * (1.0f - 1.0f / 1048576.0f);
        if (lb > 0.0f && (best < lb * lb || lb >= a.max_dist)) break;
    }
    const float d = sqrtf(best);
    const bool found = bi >= 0 && d < a.max_dist;
    a.dist[out] = found ? d : a.max_dist;
    if (a.index) a.index[out] = found ? bi : -1;
}

// ---- the k nearest neighbours ------------------------------------------------------------------------------

struct KnnArgs {
    QueryArgs q;  // dist / index are [Q][k]
    int k;
    int exclude_self;
    int32_t* count;
};

// A lane's k-best list lives in LDS as [slot][lane]: slot j of lane t is word j 256 + t of each array, so whatever
// slots the lanes of a wave are at, lane t is in bank t mod 64 -- no conflicts, and no runtime-indexed private array
// (which would go to scratch).  Slots 0 .. n - 1 are ascending under (squared distance, original index).
template <int K>
struct KnnList {
    float (*d)[256];
    int (*i)[256];
    int t, k;
    int n;     // slots in use, <= k
    float wd;  // the current worst pair once the list is full; (inf, -1) before: any finite distance enters, and
    int wi;    // an infinite or NaN one never does -- nn_query_kernel's (best, bi) start
};

// The records [s, e) against the list: a record enters when its pair is below the worst pair (one compare for one
// that cannot), by an insertion that shifts the larger pairs up one slot.
template <int K>
__device__ __forceinline__ void knn_scan_records(const KnnArgs& a, int s, int e, float qx, float qy, float qz, int self,
                                                 KnnList<K>& L) {
    s = s < 0 ? 0 : s;
    e = (int64_t)e > a.q.N ? (int)a.q.N : e;  // (cell_start is the build's: the clamps only bound a foreign array)
    for (int j = s; j < e; ++j) {             // bound: e - s <= N records
        const floatx4 r = a.q.sorted[j];      // one 16-byte load per record
        const float dx = r[0] - qx, dy = r[1] - qy, dz = r[2] - qz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;  // scan_records' expression
        const int idx = __float_as_int(r[3]);
        if (!(d2 < L.wd || (d2 == L.wd && idx < L.wi))) continue;
        if (a.exclude_self && idx == self) continue;
        int p = L.n < L.k ? L.n : L.k - 1;  // the slot that opens: a new one, or the worst pair's
        for (int m = 1; m < K && p > 0; ++m) {  // bound: K - 1 shifts
            const float pd = L.d[p - 1][L.t];
            const int pi = L.i[p - 1][L.t];
            if (pd < d2 || (pd == d2 && pi < idx)) break;
            L.d[p][L.t] = pd;
            L.i[p][L.t] = pi;
            --p;
        }
        L.d[p][L.t] = d2;
        L.i[p][L.t] = idx;
        if (L.n < L.k) ++L.n;
        if (L.n == L.k) {
            L.wd = L.d[L.k - 1][L.t];
            L.wi = L.i[L.k - 1][L.t];
        }
    }
}

// One lane per query, nn_query_kernel's shells with the k-th best pair in place of the best.  After shells 0 .. s
// every unvisited target lies, by the argument above nn_query_kernel, at a true distance above lb (by more than the
// fp32 distance arithmetic can lose), so its squared distance as this kernel forms it is >= lb^2.  The list holds
// the k smallest pairs among the visited targets (an insertion only ever drops the largest of k + 1), and:
//   list full and worst < lb^2  =>  every unvisited target's pair is above the list's worst pair: none of them is
//     among the k smallest pairs of all targets, so the list is final;
//   lb >= max_dist  =>  no unvisited target is within max_dist; those of the list that are stay its prefix;
//   no side with cells left  =>  every cell has been visited.
// A list that is not full has worst = +inf and never stops on the first rule.  Rows are cut at max_dist when they
// are written: sqrtf never falls, so the pairs with sqrtf(d^2) < max_dist are a prefix of the ascending list, and
// the k smallest pairs of all targets cut there are the k smallest among the targets within max_dist.
// exclude_self leaves out the one target whose original index is the query's own (the lane's position, or its
// record's index): the argument is the same over the remaining targets.  K is the capacity (k <= K); the LDS is
// 256 lanes x K slots x 8 bytes.
template <int K>
__global__ void __launch_bounds__(256) knn_query_kernel(KnnArgs a) {
    __shared__ float sd[K][256];
    __shared__ int si[K][256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.q.Q) return;  // (no barrier below: a lane only ever touches its own column of the LDS)
    float q[3];
    int64_t out = i;
    if (a.q.records) {
        const floatx4 r = reinterpret_cast<const floatx4*>(a.q.q)[i];
        q[0] = r[0];
        q[1] = r[1];
        q[2] = r[2];
        out = __float_as_int(r[3]);
        if (out < 0 || out >= a.q.Q) return;  // (never for cn_nn_grid_build's records)
    } else {
        q[0] = a.q.q[i * 3];
        q[1] = a.q.q[i * 3 + 1];
        q[2] = a.q.q[i * 3 + 2];
    }
    const Grid& g = a.q.g;
    int c[3];
    float slack = 0.0f;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        c[ax] = axis_cell(q[ax], g.o[ax], g.cell, g.d[ax]);
        slack = fmaxf(slack, (fabsf(g.o[ax]) + fabsf(q[ax]) + (float)g.d[ax] * g.cell) * (1.0f / 1048576.0f));
    }
    const int ny = g.d[1], nz = g.d[2];
    KnnList<K> L{sd, si, (int)threadIdx.x, a.k, 0, INFINITY, -1};
    const int self = (int)out;
    // bound: the grid's largest dimension -- shell maxdim - 1 around any cell holds every cell of the grid
    for (int s = 0; s < a.q.maxdim; ++s) {
        const int x0 = max(c[0] - s, 0), x1 = min(c[0] + s, g.d[0] - 1);
        const int y0 = max(c[1] - s, 0), y1 = min(c[1] + s, ny - 1);
        const int z0 = max(c[2] - s, 0), z1 = min(c[2] + s, nz - 1);
        for (int x = x0; x <= x1; ++x) {      // bound: 2 s + 1
            for (int y = y0; y <= y1; ++y) {  // bound: 2 s + 1
                const int row = (x * ny + y) * nz;
                if (abs(x - c[0]) == s || abs(y - c[1]) == s) {
                    // a face row of the shell: its cells z0 .. z1 are one run of records (z is the fastest index)
                    knn_scan_records<K>(a, a.q.start[row + z0], a.q.start[row + z1 + 1], q[0], q[1], q[2], self, L);
                } else {
                    // an inner row: the two end cells, where they are inside the grid
                    const int za = c[2] - s, zb = c[2] + s;
                    if (za >= 0)
                        knn_scan_records<K>(a, a.q.start[row + za], a.q.start[row + za + 1], q[0], q[1], q[2], self, L);
                    if (zb < nz)
                        knn_scan_records<K>(a, a.q.start[row + zb], a.q.start[row + zb + 1], q[0], q[1], q[2], self, L);
                }
            }
        }
        float lb = INFINITY;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (c[ax] + s + 1 <= g.d[ax] - 1) lb = fminf(lb, (g.o[ax] + (float)(c[ax] + s + 1) * g.cell) - q[ax]);
            if (c[ax] - s - 1 >= 0) lb = fminf(lb, q[ax] - (g.o[ax] + (float)(c[ax] - s) * g.cell));
        }
        if (lb == INFINITY) break;  // the shell left the grid on every side
        lb = (lb - slack) * (1.0f - 1.0f / 1048576.0f);
        if (lb > 0.0f && (L.wd < lb * lb || lb >= a.q.max_dist)) break;
    }
    int found = 0;
    for (int j = 0; j < a.k; ++j) {  // bound: k <= K slots
        float d = a.q.max_dist;
        int idx = -1;
        if (j < L.n) {
            const float dj = sqrtf(sd[j][threadIdx.x]);
            if (dj < a.q.max_dist) {
                d = dj;
                idx = si[j][threadIdx.x];
                ++found;
            }
        }
        a.q.dist[out * a.k + j] = d;
        a.q.index[out * a.k + j] = idx;
    }
    if (a.count) a.count[out] = found;
}

// ---- statistics -----------------------------------------------------------------------------------------

struct StatsArgs {
    int64_t Q;
    const float* dist;
    const float* pts;
    float lo[3], hi[3];
    float max_dist, tau;
    double* part;  // [blocks][4]
    double* out;   // [4]
};

// launch 1: thread t of block b takes elements (b 256 + t) + j (blocks 256), j ascending
__global__ void __launch_bounds__(kStatsThreads) stats_partial_kernel(StatsArgs a) {
    __shared__ double sh[kStatsThreads / kWave];
    const int64_t stride = (int64_t)gridDim.x * kStatsThreads;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x; i < a.Q; i += stride) {  // bound: ceil(Q / stride)
        bool in = true;
        if (a.pts) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float p = a.pts[i * 3 + ax];
                in = in && p >= a.lo[ax] && p <= a.hi[ax];
            }
        }
        const float d = a.dist[i];
        const bool near = in && d < a.max_dist;
        v[0] += in ? 1.0 : 0.0;
        v[1] += near ? 1.0 : 0.0;
        v[2] = v[2] + (near ? (double)d : 0.0);
        v[3] += (near && d < a.tau) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s = block_sum_fixed(v[k], sh);
        if (threadIdx.x == 0) a.part[(int64_t)blockIdx.x * 4 + k] = s;
    }
}

// launch 2 (one block): the block partials, thread t takes blocks t, t + 256, ...
__global__ void __launch_bounds__(kStatsThreads) stats_final_kernel(int nb, const double* __restrict__ part,
                                                                    double* __restrict__ out) {
    __shared__ double sh[kStatsThreads / kWave];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += kStatsThreads)  // bound: ceil(nb / 256) <= 4
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] + part[(int64_t)b * 4 + k];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double s = block_sum_fixed(v[k], sh);
        if (threadIdx.x == 0) out[k] = s;
    }
}

// ---- normal statistics ----------------------------------------------------------------------------------

struct NormalStatsArgs {
    int64_t Q, N;
    const float* qn;
    const float* tn;
    const int32_t* index;
    const float* dist;
    const float* pts;
    float lo[3], hi[3];
    float max_dist;
    double* part;  // [blocks][3]
    double* out;   // [3]
};

// v / |v| in fp32, |v| = sqrt((x x + y y) + z z); false for a zero or non-finite length
__device__ __forceinline__ bool unit3(const float* __restrict__ v, float* o) {
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(len > 0.0f && len < INFINITY)) return false;
    o[0] = v[0] / len;
    o[1] = v[1] / len;
    o[2] = v[2] / len;
    return true;
}

// launch 1, laid out as stats_partial_kernel: (pairs counted, the sum of |q . t|, pairs left out for a normal)
__global__ void __launch_bounds__(kStatsThreads) normal_stats_partial_kernel(NormalStatsArgs a) {
    __shared__ double sh[kStatsThreads / kWave];
    const int64_t stride = (int64_t)gridDim.x * kStatsThreads;
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x; i < a.Q; i += stride) {  // bound: ceil(Q / stride)
        bool in = true;
        if (a.pts) {
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float p = a.pts[i * 3 + ax];
                in = in && p >= a.lo[ax] && p <= a.hi[ax];
            }
        }
        const int32_t j = a.index[i];
        if (!(in && j >= 0 && j < a.N && a.dist[i] < a.max_dist)) continue;  // (an index past the targets reads nothing)
        float q[3], t[3];
        if (unit3(a.qn + i * 3, q) && unit3(a.tn + (int64_t)j * 3, t)) {
            v[0] += 1.0;
            v[1] = v[1] + (double)fabsf((q[0] * t[0] + q[1] * t[1]) + q[2] * t[2]);
        } else {
            v[2] += 1.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double s = block_sum_fixed(v[k], sh);
        if (threadIdx.x == 0) a.part[(int64_t)blockIdx.x * 3 + k] = s;
    }
}

// launch 2 (one block): the block partials, thread t takes blocks t, t + 256, ...
__global__ void __launch_bounds__(kStatsThreads) normal_stats_final_kernel(int nb, const double* __restrict__ part,
                                                                           double* __restrict__ out) {
    __shared__ double sh[kStatsThreads / kWave];
    double v[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nb; b += kStatsThreads)  // bound: ceil(nb / 256) <= 4
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = v[k] + part[(int64_t)b * 3 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double s = block_sum_fixed(v[k], sh);
        if (threadIdx.x == 0) out[k] = s;
    }
}

// ---- ICP registration: the transform -------------------------------------------------------------------

struct Sim {
    float m[12];  // row-major 3 x 4: s R in the left 3 x 3, t in the last column
};

// The ONLY place a similarity is applied to a point: row r of m is (a, b, c, t) and
//   o_r = fmaf(c, z, fmaf(b, y, fmaf(a, x, t)))
// -- t first, then x, y, z, each step one rounding.  cloud_transform_kernel and icp_partial_kernel both call it, so
// the same point under the same matrix is the same three floats in each: the sums are over the points the search saw.
__device__ __forceinline__ void sim_apply(const Sim& s, float x, float y, float z, float* o) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
        o[r] = fmaf(s.m[r * 4 + 2], z, fmaf(s.m[r * 4 + 1], y, fmaf(s.m[r * 4], x, s.m[r * 4 + 3])));
}

// one thread per point; a thread reads its point before it writes it, so out may be points
__global__ void __launch_bounds__(256) cloud_transform_kernel(int64_t N, const float* pts, Sim s, float* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float o[3];
    sim_apply(s, pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2], o);
    out[i * 3] = o[0];
    out[i * 3 + 1] = o[1];
    out[i * 3 + 2] = o[2];
}

// ---- ICP registration: the sums of a closed-form solve ---------------------------------------------------

constexpr int kIcpSums = 32;

struct IcpArgs {
    int64_t Q, N;
    const float* src;
    const float* tgt;
    const float* nrm;
    const int32_t* index;
    Sim sim;
    double c[3];
    double* part;  // [blocks][32]
    double* out;   // [32]
};

// launch 1, laid out as stats_partial_kernel over the source in its ORIGINAL order.  Every term is formed in
// double from the fp32 p' = sim_apply(source[i]), q = targets[index[i]] and (MODE 1) the fp32 unit normal,
// relative to the pivot c.  An index outside [0, N) -- -1, or anything a foreign array holds -- gathers nothing.
// The slots (copenerf.h):  MODE 0: 0 n, 1 sum |p' - q|^2, 2..4 sum (p' - c), 5..7 sum (q - c),
// 8..16 sum (q - c)(p' - c)^T row-major, 17 sum |p' - c|^2.  MODE 1: 0 n, 1 sum |p' - q|^2, 2 sum r^2,
// 3..23 the upper triangle of sum J^T J row by row, 24..29 sum J^T r, 30 the pairs left out for their normal.
// The two counts are per-thread integers (a thread sees fewer than 2^31 / 256 points): 29 doubles at most per
// thread, no atomics, no LDS but block_sum_fixed's.
template <int MODE>
__global__ void __launch_bounds__(kStatsThreads) icp_partial_kernel(IcpArgs a) {
    __shared__ double sh[kStatsThreads / kWave];
    constexpr int kAcc = MODE == 0 ? 17 : 29;  // the double sums: slot k + 1 is v[k] (slots 1 .. 17, or 1 .. 29)
    const int64_t stride = (int64_t)gridDim.x * kStatsThreads;
    double v[kAcc];
#pragma unroll
    for (int k = 0; k < kAcc; ++k) v[k] = 0.0;
    int n = 0, left = 0;
    for (int64_t i = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x; i < a.Q; i += stride) {  // bound: ceil(Q / stride)
        const int32_t j = a.index[i];
        if (j < 0 || j >= a.N) continue;  // (no pair, or an index past the targets: nothing is read)
        float pf[3];
        sim_apply(a.sim, a.src[i * 3], a.src[i * 3 + 1], a.src[i * 3 + 2], pf);
        double p[3], q[3], e[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const float qf = a.tgt[(int64_t)j * 3 + ax];
            e[ax] = (double)pf[ax] - (double)qf;
            p[ax] = (double)pf[ax] - a.c[ax];
            q[ax] = (double)qf - a.c[ax];
        }
        const double e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        if (MODE == 0) {
            n += 1;
            v[0] = v[0] + e2;
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                v[1 + ax] = v[1 + ax] + p[ax];
                v[4 + ax] = v[4 + ax] + q[ax];
#pragma unroll
                for (int bx = 0; bx < 3; ++bx) v[7 + ax * 3 + bx] = v[7 + ax * 3 + bx] + q[ax] * p[bx];
            }
            v[16] = v[16] + ((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]);
        } else {
            float nf[3];
            if (!unit3(a.nrm + (int64_t)j * 3, nf)) {
                left += 1;
                continue;
            }
            const double nx = nf[0], ny = nf[1], nz = nf[2];
            double J[6];
            J[0] = p[1] * nz - p[2] * ny;
            J[1] = p[2] * nx - p[0] * nz;
            J[2] = p[0] * ny - p[1] * nx;
            J[3] = nx;
            J[4] = ny;
            J[5] = nz;
            const double r = (e[0] * nx + e[1] * ny) + e[2] * nz;
            n += 1;
            v[0] = v[0] + e2;
            v[1] = v[1] + r * r;
            int k = 2;
#pragma unroll
            for (int x = 0; x < 6; ++x)
#pragma unroll
                for (int y = x; y < 6; ++y) {
                    v[k] = v[k] + J[x] * J[y];
                    ++k;
                }
#pragma unroll
            for (int x = 0; x < 6; ++x) v[23 + x] = v[23 + x] + J[x] * r;  // (k ended at 23)
        }
    }
    double* part = a.part + (int64_t)blockIdx.x * kIcpSums;
    double s = block_sum_fixed((double)n, sh);
    if (threadIdx.x == 0) part[0] = s;
#pragma unroll
    for (int k = 0; k < kAcc; ++k) {
        s = block_sum_fixed(v[k], sh);
        if (threadIdx.x == 0) part[1 + k] = s;
    }
    s = block_sum_fixed((double)left, sh);
    if (threadIdx.x == 0) {
        for (int k = 1 + kAcc; k < kIcpSums; ++k) part[k] = 0.0;  // bound: at most 14 unused slots
        if (MODE == 1) part[30] = s;
    }
}

// launch 2 (one block): per slot, thread t adds the partials of blocks t, t + 256, ..., then the fixed tree
__global__ void __launch_bounds__(kStatsThreads) icp_final_kernel(int nb, const double* __restrict__ part,
                                                                  double* __restrict__ out) {
    __shared__ double sh[kStatsThreads / kWave];
    for (int k = 0; k < kIcpSums; ++k) {  // bound: the 32 slots
        double v = 0.0;
        for (int b = threadIdx.x; b < nb; b += kStatsThreads) v = v + part[(int64_t)b * kIcpSums + k];  // bound: <= 4
        const double s = block_sum_fixed(v, sh);
        if (threadIdx.x == 0) out[k] = s;
    }
}

int sim_check(const char* who, const float* m, Sim* s) {
    for (int i = 0; i < 12; ++i) {
        CN_REQUIRE(std::isfinite(m[i]), CN_ERR_SHAPE, "%s: matrix[%d] is not finite", who, i);
        s->m[i] = m[i];
    }
    return CN_OK;
}

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" size_t cn_mesh_sample_workspace_bytes(int64_t T) {
    if (T < 0 || T > kMaxCount) return 0;
    return sample_plan(T, nullptr).bytes;
}

extern "C" int cn_mesh_area(const cn_mesh_sample_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int rc = sample_check("cn_mesh_area", d, workspace, workspace_bytes, false);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const SamplePlan p = sample_plan(d->T, workspace);
    const int tiles = (int)((d->T + kScanTile - 1) / kScanTile);
    if (tiles > 0) {
        area_tile_kernel<<<tiles, kScanThreads, 0, st>>>(d->V, d->T, d->vertices, d->triangles, p.cdf, p.tot);
        if ((rc = check_launch("cn_mesh_area"))) return rc;
    }
    area_totals_kernel<<<1, kWave, 0, st>>>(p.tot, tiles, d->area);  // (no triangles: area = 0)
    if ((rc = check_launch("cn_mesh_area")) || tiles == 0) return rc;
    area_apply_kernel<<<tiles, kScanThreads, 0, st>>>(d->T, p.tot, p.cdf);
    return check_launch("cn_mesh_area");
}

extern "C" int cn_mesh_sample(const cn_mesh_sample_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int rc = sample_check("cn_mesh_sample", d, workspace, workspace_bytes, true);
    if (rc || d->S == 0) return rc;
    SampleArgs a{};
    a.V = d->V;
    a.T = d->T;
    a.S = d->S;
    a.v = d->vertices;
    a.tri = d->triangles;
    a.cdf = sample_plan(d->T, workspace).cdf;
    a.area = d->area;
    a.philox = d->philox;
    a.points = d->points;
    a.tri_out = d->tri;
    mesh_sample_kernel<<<(unsigned)((d->S + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
    return check_launch("cn_mesh_sample");
}

extern "C" size_t cn_nn_grid_workspace_bytes(int64_t N, int64_t ncells) {
    if (N < 0 || N > kMaxCount || ncells < 1 || ncells > kMaxCells) return 0;
    return grid_plan(N, ncells, nullptr).bytes;
}

extern "C" int cn_nn_grid_build(const cn_nn_grid_desc* g, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int64_t ncells;
    int rc = grid_check("cn_nn_grid_build", g, &ncells);
    if (rc) return rc;
    CN_REQUIRE(g->N == 0 || g->points, CN_ERR_ARG, "cn_nn_grid_build: null points");
    CN_REQUIRE(((uintptr_t)g->points & 3) == 0, CN_ERR_ALIGN, "cn_nn_grid_build: points not 4-byte aligned");
    const size_t need = grid_plan(g->N, ncells, nullptr).bytes;
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_nn_grid_build: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_nn_grid_build: workspace not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const GridPlan p = grid_plan(g->N, ncells, workspace);
    const Grid gr = grid_of(g);
    const int nc = (int)ncells;
    const unsigned pblocks = (unsigned)((g->N + 255) / 256);
    zero_cells_kernel<<<(nc + 255) / 256, 256, 0, st>>>(nc, p.count);
    if ((rc = check_launch("cn_nn_grid_build"))) return rc;
    if (g->N > 0) {
        grid_count_kernel<<<pblocks, 256, 0, st>>>(gr, g->N, g->points, p.id, p.count);
        if ((rc = check_launch("cn_nn_grid_build"))) return rc;
    }
    cells_reduce_kernel<<<p.nt, kScanThreads, 0, st>>>(p.count, nc, p.tot);
    if ((rc = check_launch("cn_nn_grid_build"))) return rc;
    cells_totals_kernel<<<1, kScanThreads, 0, st>>>(p.tot, p.nt, g->cell_start + nc);
    if ((rc = check_launch("cn_nn_grid_build"))) return rc;
    cells_apply_kernel<<<p.nt, kScanThreads, 0, st>>>(p.count, nc, p.tot, g->cell_start);
    if ((rc = check_launch("cn_nn_grid_build")) || g->N == 0) return rc;
    grid_scatter_kernel<<<pblocks, 256, 0, st>>>(g->N, g->points, p.id, g->cell_start, p.count,
                                                 reinterpret_cast<floatx4*>(g->sorted));
    return check_launch("cn_nn_grid_build");
}

extern "C" int cn_nn_query(const cn_nn_query_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_nn_query: null descriptor");
    int64_t ncells;
    int rc = grid_check("cn_nn_query", d->grid, &ncells);
    if (rc) return rc;
    CN_REQUIRE(d->Q >= 0 && d->Q <= kMaxCount, CN_ERR_SHAPE, "cn_nn_query: Q %lld (in [0, 2^31))", (long long)d->Q);
    CN_REQUIRE(d->query_records == 0 || d->query_records == 1, CN_ERR_ARG, "cn_nn_query: query_records %d",
               d->query_records);
    CN_REQUIRE(!(d->max_dist != d->max_dist) && d->max_dist >= 0.0f, CN_ERR_SHAPE, "cn_nn_query: max_dist %g",
               (double)d->max_dist);
    if (d->Q == 0) return CN_OK;
    CN_REQUIRE(d->queries && d->dist, CN_ERR_ARG, "cn_nn_query: null queries / dist");
    CN_REQUIRE(((uintptr_t)d->queries & (d->query_records ? 15 : 3)) == 0 && ((uintptr_t)d->dist & 3) == 0 &&
                   ((uintptr_t)d->index & 3) == 0,
               CN_ERR_ALIGN, "cn_nn_query: queries %d-byte, dist / index 4-byte aligned", d->query_records ? 16 : 4);
    QueryArgs a{};
    a.g = grid_of(d->grid);
    a.N = d->grid->N;
    a.Q = d->Q;
    a.q = d->queries;
    a.records = d->query_records;
    a.sorted = reinterpret_cast<const floatx4*>(d->grid->sorted);
    a.start = d->grid->cell_start;
    a.max_dist = d->max_dist;
    a.dist = d->dist;
    a.index = d->index;
    a.maxdim = a.g.d[0] > a.g.d[1] ? a.g.d[0] : a.g.d[1];
    a.maxdim = a.maxdim > a.g.d[2] ? a.maxdim : a.g.d[2];
    nn_query_kernel<<<(unsigned)((d->Q + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
    return check_launch("cn_nn_query");
}

extern "C" int cn_knn_query(const cn_knn_query_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_knn_query: null descriptor");
    int64_t ncells;
    int rc = grid_check("cn_knn_query", d->grid, &ncells);
    if (rc) return rc;
    CN_REQUIRE(d->Q >= 0 && d->Q <= kMaxCount, CN_ERR_SHAPE, "cn_knn_query: Q %lld (in [0, 2^31))", (long long)d->Q);
    CN_REQUIRE(d->k >= 1 && d->k <= 32, CN_ERR_SHAPE, "cn_knn_query: k %d (in [1, 32])", d->k);
    CN_REQUIRE(d->query_records == 0 || d->query_records == 1, CN_ERR_ARG, "cn_knn_query: query_records %d",
               d->query_records);
    CN_REQUIRE(d->exclude_self == 0 || d->exclude_self == 1, CN_ERR_ARG, "cn_knn_query: exclude_self %d", d->exclude_self);
    CN_REQUIRE(!d->exclude_self || d->Q == d->grid->N, CN_ERR_SHAPE,
               "cn_knn_query: exclude_self with Q %lld queries of N %lld targets (a self-query has Q = N)", (long long)d->Q,
               (long long)d->grid->N);
    CN_REQUIRE(!(d->max_dist != d->max_dist) && d->max_dist >= 0.0f, CN_ERR_SHAPE, "cn_knn_query: max_dist %g",
               (double)d->max_dist);
    if (d->Q == 0) return CN_OK;
    CN_REQUIRE(d->queries && d->dist && d->index, CN_ERR_ARG, "cn_knn_query: null queries / dist / index");
    CN_REQUIRE(((uintptr_t)d->queries & (d->query_records ? 15 : 3)) == 0 && ((uintptr_t)d->dist & 3) == 0 &&
                   ((uintptr_t)d->index & 3) == 0 && ((uintptr_t)d->count & 3) == 0,
               CN_ERR_ALIGN, "cn_knn_query: queries %d-byte, dist / index / count 4-byte aligned", d->query_records ? 16 : 4);
    KnnArgs a{};
    a.q.g = grid_of(d->grid);
    a.q.N = d->grid->N;
    a.q.Q = d->Q;
    a.q.q = d->queries;
    a.q.records = d->query_records;
    a.q.sorted = reinterpret_cast<const floatx4*>(d->grid->sorted);
    a.q.start = d->grid->cell_start;
    a.q.max_dist = d->max_dist;
    a.q.dist = d->dist;
    a.q.index = d->index;
    a.q.maxdim = a.q.g.d[0] > a.q.g.d[1] ? a.q.g.d[0] : a.q.g.d[1];
    a.q.maxdim = a.q.maxdim > a.q.g.d[2] ? a.q.maxdim : a.q.g.d[2];
    a.k = d->k;
    a.exclude_self = d->exclude_self;
    a.count = d->count;
    const unsigned blocks = (unsigned)((d->Q + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    // the smallest capacity that holds k: 16, 32 or 64 KB of LDS per block
    if (d->k <= 8) knn_query_kernel<8><<<blocks, 256, 0, st>>>(a);
    else if (d->k <= 16) knn_query_kernel<16><<<blocks, 256, 0, st>>>(a);
    else knn_query_kernel<32><<<blocks, 256, 0, st>>>(a);
    return check_launch("cn_knn_query");
}

extern "C" size_t cn_cloud_stats_workspace_bytes(int64_t Q) {
    if (Q < 0 || Q > kMaxCount) return 0;
    return rup_sz((size_t)stats_blocks(Q) * 4 * sizeof(double));
}

extern "C" int cn_cloud_stats(const cn_cloud_stats_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_cloud_stats: null descriptor");
    CN_REQUIRE(d->Q >= 0 && d->Q <= kMaxCount, CN_ERR_SHAPE, "cn_cloud_stats: Q %lld (in [0, 2^31))", (long long)d->Q);
    CN_REQUIRE((d->Q == 0 || d->dist) && d->out, CN_ERR_ARG, "cn_cloud_stats: null dist / out");
    CN_REQUIRE(((uintptr_t)d->dist & 3) == 0 && ((uintptr_t)d->points & 3) == 0 && ((uintptr_t)d->out & 7) == 0, CN_ERR_ALIGN,
               "cn_cloud_stats: dist / points 4-byte, out 8-byte aligned");
    const size_t need = cn_cloud_stats_workspace_bytes(d->Q);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_cloud_stats: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_cloud_stats: workspace not 256-byte aligned");
    StatsArgs a{};
    a.Q = d->Q;
    a.dist = d->dist;
    a.pts = d->points;
    for (int i = 0; i < 3; ++i) {
        a.lo[i] = d->crop_min[i];
        a.hi[i] = d->crop_max[i];
    }
    a.max_dist = d->max_dist;
    a.tau = d->threshold;
    a.part = static_cast<double*>(workspace);
    a.out = d->out;
    hipStream_t st = (hipStream_t)stream;
    const int nb = stats_blocks(d->Q);
    stats_partial_kernel<<<nb, kStatsThreads, 0, st>>>(a);
    int rc = check_launch("cn_cloud_stats");
    if (rc) return rc;
    stats_final_kernel<<<1, kStatsThreads, 0, st>>>(nb, a.part, a.out);
    return check_launch("cn_cloud_stats");
}

extern "C" size_t cn_cloud_normal_stats_workspace_bytes(int64_t Q) {
    if (Q < 0 || Q > kMaxCount) return 0;
    return rup_sz((size_t)stats_blocks(Q) * 3 * sizeof(double));
}

extern "C" int cn_cloud_normal_stats(const cn_cloud_normal_stats_desc* d, void* workspace, int64_t workspace_bytes,
                                     cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_cloud_normal_stats: null descriptor");
    CN_REQUIRE(d->Q >= 0 && d->Q <= kMaxCount && d->N >= 0 && d->N <= kMaxCount, CN_ERR_SHAPE,
               "cn_cloud_normal_stats: Q %lld, N %lld (each in [0, 2^31))", (long long)d->Q, (long long)d->N);
    CN_REQUIRE(!(d->max_dist != d->max_dist), CN_ERR_SHAPE, "cn_cloud_normal_stats: max_dist is NaN");
    CN_REQUIRE(d->out, CN_ERR_ARG, "cn_cloud_normal_stats: null out");
    CN_REQUIRE(d->Q == 0 || (d->query_normals && d->index && d->dist), CN_ERR_ARG,
               "cn_cloud_normal_stats: null query_normals / index / dist");
    CN_REQUIRE(d->Q == 0 || d->N == 0 || d->target_normals, CN_ERR_ARG, "cn_cloud_normal_stats: null target_normals");
    CN_REQUIRE((((uintptr_t)d->query_normals | (uintptr_t)d->target_normals | (uintptr_t)d->index | (uintptr_t)d->dist |
                 (uintptr_t)d->points) & 3) == 0 && ((uintptr_t)d->out & 7) == 0,
               CN_ERR_ALIGN, "cn_cloud_normal_stats: normals / index / dist / points 4-byte, out 8-byte aligned");
    const size_t need = cn_cloud_normal_stats_workspace_bytes(d->Q);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_cloud_normal_stats: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_cloud_normal_stats: workspace not 256-byte aligned");
    NormalStatsArgs a{};
    a.Q = d->Q;
    a.N = d->N;
    a.qn = d->query_normals;
    a.tn = d->target_normals;
    a.index = d->index;
    a.dist = d->dist;
    a.pts = d->points;
    for (int i = 0; i < 3; ++i) {
        a.lo[i] = d->crop_min[i];
        a.hi[i] = d->crop_max[i];
    }
    a.max_dist = d->max_dist;
    a.part = static_cast<double*>(workspace);
    a.out = d->out;
    hipStream_t st = (hipStream_t)stream;
    const int nb = stats_blocks(d->Q);
    normal_stats_partial_kernel<<<nb, kStatsThreads, 0, st>>>(a);
    int rc = check_launch("cn_cloud_normal_stats");
    if (rc) return rc;
    normal_stats_final_kernel<<<1, kStatsThreads, 0, st>>>(nb, a.part, a.out);
    return check_launch("cn_cloud_normal_stats");
}

extern "C" int cn_cloud_transform(const cn_cloud_transform_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_cloud_transform: null descriptor");
    CN_REQUIRE(d->N >= 0 && d->N <= kMaxCount, CN_ERR_SHAPE, "cn_cloud_transform: N %lld (in [0, 2^31))", (long long)d->N);
    Sim s{};
    int rc = sim_check("cn_cloud_transform", d->matrix, &s);
    if (rc || d->N == 0) return rc;
    CN_REQUIRE(d->points && d->out, CN_ERR_ARG, "cn_cloud_transform: null points / out");
    CN_REQUIRE(((uintptr_t)d->points & 3) == 0 && ((uintptr_t)d->out & 3) == 0, CN_ERR_ALIGN,
               "cn_cloud_transform: points / out 4-byte aligned");
    cloud_transform_kernel<<<(unsigned)((d->N + 255) / 256), 256, 0, (hipStream_t)stream>>>(d->N, d->points, s, d->out);
    return check_launch("cn_cloud_transform");
}

extern "C" size_t cn_icp_accumulate_workspace_bytes(int64_t Q) {
    if (Q < 0 || Q > kMaxCount) return 0;
    return rup_sz((size_t)stats_blocks(Q) * kIcpSums * sizeof(double));
}

extern "C" int cn_icp_accumulate(const cn_icp_accumulate_desc* d, void* workspace, int64_t workspace_bytes,
                                 cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_icp_accumulate: null descriptor");
    CN_REQUIRE(d->Q >= 0 && d->Q <= kMaxCount && d->N >= 0 && d->N <= kMaxCount, CN_ERR_SHAPE,
               "cn_icp_accumulate: Q %lld, N %lld (each in [0, 2^31))", (long long)d->Q, (long long)d->N);
    CN_REQUIRE(d->mode == 0 || d->mode == 1, CN_ERR_ARG, "cn_icp_accumulate: mode %d (0 point-to-point, 1 point-to-plane)",
               d->mode);
    IcpArgs a{};
    int rc = sim_check("cn_icp_accumulate", d->matrix, &a.sim);
    if (rc) return rc;
    for (int i = 0; i < 3; ++i) {
        CN_REQUIRE(std::isfinite(d->pivot[i]), CN_ERR_SHAPE, "cn_icp_accumulate: pivot[%d] is not finite", i);
        a.c[i] = d->pivot[i];
    }
    CN_REQUIRE(d->out, CN_ERR_ARG, "cn_icp_accumulate: null out");
    CN_REQUIRE(d->Q == 0 || (d->source && d->index), CN_ERR_ARG, "cn_icp_accumulate: null source / index");
    CN_REQUIRE(d->Q == 0 || d->N == 0 || d->targets, CN_ERR_ARG, "cn_icp_accumulate: null targets");
    CN_REQUIRE(d->mode == 0 || d->Q == 0 || d->N == 0 || d->target_normals, CN_ERR_ARG,
               "cn_icp_accumulate: mode 1 without target_normals");
    CN_REQUIRE((((uintptr_t)d->source | (uintptr_t)d->targets | (uintptr_t)d->target_normals | (uintptr_t)d->index) & 3) == 0 &&
                   ((uintptr_t)d->out & 7) == 0,
               CN_ERR_ALIGN, "cn_icp_accumulate: source / targets / target_normals / index 4-byte, out 8-byte aligned");
    const size_t need = cn_icp_accumulate_workspace_bytes(d->Q);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_icp_accumulate: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_icp_accumulate: workspace not 256-byte aligned");
    a.Q = d->Q;
    a.N = d->N;
    a.src = d->source;
    a.tgt = d->targets;
    a.nrm = d->target_normals;
    a.index = d->index;
    a.part = static_cast<double*>(workspace);
    a.out = d->out;
    hipStream_t st = (hipStream_t)stream;
    const int nb = stats_blocks(d->Q);
    if (d->mode == 0) icp_partial_kernel<0><<<nb, kStatsThreads, 0, st>>>(a);
    else icp_partial_kernel<1><<<nb, kStatsThreads, 0, st>>>(a);
    if ((rc = check_launch("cn_icp_accumulate"))) return rc;
    icp_final_kernel<<<1, kStatsThreads, 0, st>>>(nb, a.part, a.out);
    return check_launch("cn_icp_accumulate");
}
