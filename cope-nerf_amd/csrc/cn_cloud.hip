// cn_cloud.hip — point-cloud preparation around the k-nearest search (additive to ABI v22): what the evaluation
// protocols do to a raw scan before they score against it.  Voxel down-sampling (cn_voxel_keys, a stable sort
// by the caller, cn_voxel_reduce), PCA normals from cn_knn_query's neighbour rows (cn_cloud_normals) and the
// statistics of the statistical outlier filter (cn_knn_mean_stats).  The reference has none of these; the
// yardstick is float64 numpy (tests/cloud_ref.py).
//
// Determinism.  No floating-point atomics and no integer atomics either: a voxel's sums are one thread's walk of
// its run in the order of the caller's stable sort (ascending original index), a normal is one thread's walk of its
// row, and the outlier sums go through cn_cloud_stats' fixed two-launch tree.  Every pass is bitwise repeatable.
#include "cn_common.h"

#include <cmath>

namespace cn {
namespace {

constexpr size_t kAlign = 256;
size_t rup_sz(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

constexpr int64_t kMaxCount = ((int64_t)1 << 31) - 1;  // N < 2^31
constexpr int64_t kKeyNone = INT64_MAX;                // CN_VOXEL_KEY_NONE: sorts after every voxel
constexpr float kVoxelRange = 2097152.0f;              // 2^21 voxels per axis

// ---- voxel keys ------------------------------------------------------------------------------------------

// One thread per point.  Per axis f = fl(fl(p - o) / voxel), axis_cell's form; the voxel index is floor(f) when
// 0 <= f < 2^21 -- a NaN or infinite coordinate fails both comparisons -- and the key packs the three 21-bit
// indices, x highest.  A point that fails on any axis gets kKeyNone and valid = 0: it is never clamped into a voxel.
__global__ void __launch_bounds__(256) voxel_keys_kernel(int64_t N, const float* __restrict__ pts, float ox, float oy,
                                                         float oz, float voxel, int64_t* __restrict__ keys,
                                                         int32_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float fx = (pts[i * 3] - ox) / voxel, fy = (pts[i * 3 + 1] - oy) / voxel, fz = (pts[i * 3 + 2] - oz) / voxel;
    const bool ok = fx >= 0.0f && fx < kVoxelRange && fy >= 0.0f && fy < kVoxelRange && fz >= 0.0f && fz < kVoxelRange;
    keys[i] = ok ? (((int64_t)(int)fx << 42) | ((int64_t)(int)fy << 21) | (int64_t)(int)fz) : kKeyNone;
    if (valid) valid[i] = ok ? 1 : 0;
}

// ---- voxel reduce ----------------------------------------------------------------------------------------

// element i of the sorted keys starts a voxel's run
__device__ __forceinline__ int run_head(const int64_t* __restrict__ keys, int64_t N, int64_t i) {
    if (i >= N) return 0;
    const int64_t k = keys[i];
    return (k != kKeyNone && k >= 0 && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

// launch 1: tot[b] = the heads of tile b
__global__ void __launch_bounds__(kScanThreads) heads_reduce_kernel(const int64_t* __restrict__ keys, int64_t N,
                                                                    int32_t* __restrict__ tot) {
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int x = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) x += run_head(keys, N, i0 + j);
    int all;
    block_excl_scan(x, &all);
    if (threadIdx.x == 0) tot[blockIdx.x] = all;
}

// launch 2 (one block): tot[] -> its exclusive scan in place; totals = (the number of voxels, 0 dropped so far)
__global__ void __launch_bounds__(kScanThreads) heads_totals_kernel(int32_t* __restrict__ tot, int nt,
                                                                    int32_t* __restrict__ totals) {
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
    if (threadIdx.x == 0) {
        totals[0] = carry;
        totals[1] = 0;
    }
}

// launch 3: start[v] = the first element of voxel v's run; the first element that is no voxel's (the sorted keys
// end with the dropped points') sets totals[1] = N - its position -- one thread at most, a plain store.
__global__ void __launch_bounds__(kScanThreads) heads_apply_kernel(const int64_t* __restrict__ keys, int64_t N,
                                                                   const int32_t* __restrict__ tot,
                                                                   int32_t* __restrict__ start,
                                                                   int32_t* __restrict__ totals) {
    const int64_t i0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int h[kScanItems], x = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        h[j] = run_head(keys, N, i0 + j);
        x += h[j];
    }
    int all;
    int run = tot[blockIdx.x] + block_excl_scan(x, &all);
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        const int64_t i = i0 + j;
        if (h[j] && run >= 0 && run < N) start[run] = (int32_t)i;
        run += h[j];
        if (i < N) {
            const bool none = keys[i] == kKeyNone || keys[i] < 0;
            const bool prev_none = i > 0 && (keys[i - 1] == kKeyNone || keys[i - 1] < 0);
            if (none && !prev_none) totals[1] = (int32_t)(N - i);
        }
    }
}

struct VoxelArgs {
    int64_t N;
    const int64_t* keys;
    const int64_t* order;
    const float* pts;
    const float* nrm;
    const float* col;
    const int32_t* start;
    const int32_t* totals;
    float* out_pts;
    float* out_nrm;
    float* out_col;
    int64_t* out_keys;
    int32_t* out_counts;
};

// launch 4: one thread per voxel walks its run [start[v], start[v + 1]) (the last voxel's ends where the dropped
// points begin) in the sorted order -- ascending original index inside a run, the caller's sort being stable --
// and sums in double.  An order entry outside [0, N) gathers nothing and is not counted.
__global__ void __launch_bounds__(256) voxel_means_kernel(VoxelArgs a) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t M = a.totals[0];
    if (v >= M || v >= a.N) return;
    int64_t s = a.start[v], e = v + 1 < M ? (int64_t)a.start[v + 1] : a.N - a.totals[1];
    s = s < 0 ? 0 : s;
    e = e > a.N ? a.N : e;  // (start and totals are this launch sequence's own: the clamps only bound the walk)
    double p[3] = {0.0, 0.0, 0.0}, n[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    for (int64_t j = s; j < e; ++j) {  // bound: e - s <= N
        const int64_t i = a.order[j];
        if (i < 0 || i >= a.N) continue;
        ++cnt;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            p[ax] = p[ax] + (double)a.pts[i * 3 + ax];
            if (a.nrm) n[ax] = n[ax] + (double)a.nrm[i * 3 + ax];
            if (a.col) c[ax] = c[ax] + (double)a.col[i * 3 + ax];
        }
    }
    const double w = cnt > 0 ? (double)cnt : 1.0;
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const bool unit = len > 0.0 && len < INFINITY;  // a zero (or non-finite) sum: a zero normal
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        a.out_pts[v * 3 + ax] = (float)(p[ax] / w);
        if (a.nrm) a.out_nrm[v * 3 + ax] = unit ? (float)(n[ax] / len) : 0.0f;
        if (a.col) a.out_col[v * 3 + ax] = (float)(c[ax] / w);
    }
    a.out_counts[v] = cnt;
    if (a.out_keys) a.out_keys[v] = s < a.N ? a.keys[s] : kKeyNone;
}

struct VoxelPlan {
    int32_t* start;
    int32_t* tot;
    int nt;
    size_t bytes;
};

VoxelPlan voxel_plan(int64_t N, void* ws) {
    VoxelPlan p{};
    p.nt = (int)((N + kScanTile - 1) / kScanTile);
    if (p.nt < 1) p.nt = 1;
    char* b = static_cast<char*>(ws);
    const size_t start_bytes = rup_sz((size_t)N * 4);
    p.start = reinterpret_cast<int32_t*>(b);
    p.tot = reinterpret_cast<int32_t*>(b ? b + start_bytes : nullptr);
    p.bytes = start_bytes + rup_sz((size_t)p.nt * 4);
    return p;
}

// ---- normals ---------------------------------------------------------------------------------------------

// One Jacobi rotation of the symmetric A (its upper triangle is what is read) that zeroes A[P][Q], accumulated
// into the columns of V.  P, Q and the third index R are compile-time, so A and V stay in registers.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&A)[3][3], double (&V)[3][3]) {
    constexpr int R = 3 - P - Q;
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    // the smaller root of t^2 + 2 theta t - 1: |t| <= 1; a theta whose square overflows gives t = 0
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] = A[P][P] - t * apq;
    A[Q][Q] = A[Q][Q] + t * apq;
    A[P][Q] = 0.0;
    A[Q][P] = 0.0;
    const double arp = A[R][P], arq = A[R][Q];
    A[R][P] = c * arp - s * arq;
    A[R][Q] = s * arp + c * arq;
    A[P][R] = A[R][P];
    A[Q][R] = A[R][Q];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double vp = V[r][P], vq = V[r][Q];
        V[r][P] = c * vp - s * vq;
        V[r][Q] = s * vp + c * vq;
    }
}

constexpr int kJacobiSweeps = 12;  // cyclic Jacobi on 3 x 3 converges quadratically: 5 or 6 sweeps reach double's floor

struct NormalsArgs {
    int64_t N;
    int k;
    int orient;
    const float* pts;
    const int32_t* index;
    float to[3];
    float* normals;
    float* variation;
};

// One thread per point: the centroid, then the covariance about it, of the row's valid neighbours in row order in
// double; the eigenvector of the smallest eigenvalue by cyclic Jacobi.
__global__ void __launch_bounds__(256) cloud_normals_kernel(NormalsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const int32_t* row = a.index + i * a.k;
    double c[3] = {0.0, 0.0, 0.0};
    int cnt = 0;
    for (int j = 0; j < a.k; ++j) {  // bound: k <= 32
        const int32_t t = row[j];
        if (t < 0 || t >= a.N) continue;  // (-1: no neighbour; anything else outside: never gathered)
        ++cnt;
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) c[ax] = c[ax] + (double)a.pts[(int64_t)t * 3 + ax];
    }
    double A[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    const double w = cnt > 0 ? (double)cnt : 1.0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) c[ax] = c[ax] / w;
    for (int j = 0; j < a.k; ++j) {  // bound: k <= 32
        const int32_t t = row[j];
        if (t < 0 || t >= a.N) continue;
        double d[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) d[ax] = (double)a.pts[(int64_t)t * 3 + ax] - c[ax];
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = x; y < 3; ++y) A[x][y] = A[x][y] + d[x] * d[y];
    }
    bool ok = cnt >= 3;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = x; y < 3; ++y) {
            A[x][y] = A[x][y] / w;
            A[y][x] = A[x][y];
            ok = ok && fabs(A[x][y]) < INFINITY;  // (a NaN or infinite input reaches every sum it is part of)
        }
    const float px = a.pts[i * 3], py = a.pts[i * 3 + 1], pz = a.pts[i * 3 + 2];
    ok = ok && fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY;
    float n[3] = {0.0f, 0.0f, 0.0f};
    float var = 0.0f;
    if (ok) {
        for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {  // bound: kJacobiSweeps
            if (A[0][1] == 0.0 && A[0][2] == 0.0 && A[1][2] == 0.0) break;
            jacobi_rotate<0, 1>(A, V);
            jacobi_rotate<0, 2>(A, V);
            jacobi_rotate<1, 2>(A, V);
        }
        const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
        // the column of the smallest eigenvalue (the first on a tie), and the middle and largest values
        const int m = (e0 <= e1 && e0 <= e2) ? 0 : (e1 <= e2 ? 1 : 2);
        const double l0 = m == 0 ? e0 : (m == 1 ? e1 : e2);
        const double ra = m == 0 ? e1 : e0, rb = m == 2 ? e1 : e2;
        const double l1 = ra < rb ? ra : rb, l2 = ra < rb ? rb : ra;
        double v[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) v[r] = m == 0 ? V[r][0] : (m == 1 ? V[r][1] : V[r][2]);
        const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        if (l1 > 1e-12 * l2 && len > 0.0) {  // (a collinear neighbourhood, l2 = 0 included, has no normal)
#pragma unroll
            for (int r = 0; r < 3; ++r) n[r] = (float)(v[r] / len);
            bool flip;
            if (a.orient) {
                const double dot = ((double)n[0] * ((double)a.to[0] - (double)px) + (double)n[1] * ((double)a.to[1] - (double)py)) +
                                   (double)n[2] * ((double)a.to[2] - (double)pz);
                flip = dot < 0.0;
            } else {
                const float ax = fabsf(n[0]), ay = fabsf(n[1]), az = fabsf(n[2]);
                const float big = (ax >= ay && ax >= az) ? n[0] : (ay >= az ? n[1] : n[2]);
                flip = big < 0.0f;
            }
            if (flip) {
#pragma unroll
                for (int r = 0; r < 3; ++r) n[r] = -n[r];
            }
            const double lz = l0 > 0.0 ? l0 : 0.0;
            var = (float)(lz / ((lz + l1) + l2));
        }
    }
    a.normals[i * 3] = n[0];
    a.normals[i * 3 + 1] = n[1];
    a.normals[i * 3 + 2] = n[2];
    if (a.variation) a.variation[i] = var;
}

// ---- the statistical outlier filter's sums -------------------------------------------------------------------

struct MeanStatsArgs {
    int64_t N;
    int k;
    const float* dist;
    const int32_t* index;
    float* mean;
    double* part;  // [blocks][3]
    double* out;   // [3]
};

// launch 1, laid out as cn_cloud_stats' first launch: per point the mean of the row's valid distances (index >= 0)
// in row order in double, stored in fp32 (+inf for a row without one); the sums are of the STORED fp32 means, so
// the host's cut and its comparison see the very numbers that were summed.
__global__ void __launch_bounds__(kStatsThreads) knn_mean_partial_kernel(MeanStatsArgs a) {
    __shared__ double sh[kStatsThreads / kWave];
    const int64_t stride = (int64_t)gridDim.x * kStatsThreads;
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x; i < a.N; i += stride) {  // bound: ceil(N / stride)
        double s = 0.0;
        int cnt = 0;
        for (int j = 0; j < a.k; ++j) {  // bound: k <= 32
            if (a.index[i * a.k + j] < 0) continue;
            s = s + (double)a.dist[i * a.k + j];
            ++cnt;
        }
        const float m = cnt > 0 ? (float)(s / (double)cnt) : INFINITY;
        a.mean[i] = m;
        if (cnt > 0 && fabsf(m) < INFINITY) {
            v[0] += 1.0;
            v[1] = v[1] + (double)m;
            v[2] = v[2] + (double)m * (double)m;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double s = block_sum_fixed(v[k], sh);
        if (threadIdx.x == 0) a.part[(int64_t)blockIdx.x * 3 + k] = s;
    }
}

// launch 2 (one block): the block partials, thread t takes blocks t, t + 256, ...
__global__ void __launch_bounds__(kStatsThreads) knn_mean_final_kernel(int nb, const double* __restrict__ part,
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

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" int cn_voxel_keys(const cn_voxel_keys_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_voxel_keys: null descriptor");
    CN_REQUIRE(d->N >= 0 && d->N <= kMaxCount, CN_ERR_SHAPE, "cn_voxel_keys: N %lld (in [0, 2^31))", (long long)d->N);
    CN_REQUIRE(d->voxel > 0.0f && d->voxel < INFINITY, CN_ERR_SHAPE, "cn_voxel_keys: voxel size %g", (double)d->voxel);
    for (int i = 0; i < 3; ++i)
        CN_REQUIRE(std::isfinite(d->origin[i]), CN_ERR_SHAPE, "cn_voxel_keys: origin[%d] is not finite", i);
    if (d->N == 0) return CN_OK;
    CN_REQUIRE(d->points && d->keys, CN_ERR_ARG, "cn_voxel_keys: null points / keys");
    CN_REQUIRE(((uintptr_t)d->points & 3) == 0 && ((uintptr_t)d->keys & 7) == 0 && ((uintptr_t)d->valid & 3) == 0, CN_ERR_ALIGN,
               "cn_voxel_keys: points / valid 4-byte, keys 8-byte aligned");
    voxel_keys_kernel<<<(unsigned)((d->N + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        d->N, d->points, d->origin[0], d->origin[1], d->origin[2], d->voxel, d->keys, d->valid);
    return check_launch("cn_voxel_keys");
}

extern "C" size_t cn_voxel_reduce_workspace_bytes(int64_t N) {
    if (N < 0 || N > kMaxCount) return 0;
    return voxel_plan(N, nullptr).bytes;
}

extern "C" int cn_voxel_reduce(const cn_voxel_reduce_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_voxel_reduce: null descriptor");
    CN_REQUIRE(d->N >= 0 && d->N <= kMaxCount, CN_ERR_SHAPE, "cn_voxel_reduce: N %lld (in [0, 2^31))", (long long)d->N);
    CN_REQUIRE(d->totals, CN_ERR_ARG, "cn_voxel_reduce: null totals");
    CN_REQUIRE(d->N == 0 || (d->keys && d->order && d->points && d->out_points && d->out_counts), CN_ERR_ARG,
               "cn_voxel_reduce: null keys / order / points / out_points / out_counts");
    CN_REQUIRE((d->normals == nullptr) == (d->out_normals == nullptr) && (d->colors == nullptr) == (d->out_colors == nullptr),
               CN_ERR_ARG, "cn_voxel_reduce: normals / colors and their outputs go together");
    CN_REQUIRE((((uintptr_t)d->points | (uintptr_t)d->normals | (uintptr_t)d->colors | (uintptr_t)d->out_points |
                 (uintptr_t)d->out_normals | (uintptr_t)d->out_colors | (uintptr_t)d->out_counts | (uintptr_t)d->totals) & 3) == 0 &&
                   (((uintptr_t)d->keys | (uintptr_t)d->order | (uintptr_t)d->out_keys) & 7) == 0,
               CN_ERR_ALIGN, "cn_voxel_reduce: float / int32 arrays 4-byte, keys / order / out_keys 8-byte aligned");
    const size_t need = voxel_plan(d->N, nullptr).bytes;
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_voxel_reduce: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_voxel_reduce: workspace not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const VoxelPlan p = voxel_plan(d->N, workspace);
    const int tiles = (int)((d->N + kScanTile - 1) / kScanTile);
    int rc;
    if (tiles > 0) {
        heads_reduce_kernel<<<tiles, kScanThreads, 0, st>>>(d->keys, d->N, p.tot);
        if ((rc = check_launch("cn_voxel_reduce"))) return rc;
    }
    heads_totals_kernel<<<1, kScanThreads, 0, st>>>(p.tot, tiles, d->totals);  // (no points: totals = (0, 0))
    if ((rc = check_launch("cn_voxel_reduce")) || tiles == 0) return rc;
    heads_apply_kernel<<<tiles, kScanThreads, 0, st>>>(d->keys, d->N, p.tot, p.start, d->totals);
    if ((rc = check_launch("cn_voxel_reduce"))) return rc;
    VoxelArgs a{};
    a.N = d->N;
    a.keys = d->keys;
    a.order = d->order;
    a.pts = d->points;
    a.nrm = d->normals;
    a.col = d->colors;
    a.start = p.start;
    a.totals = d->totals;
    a.out_pts = d->out_points;
    a.out_nrm = d->out_normals;
    a.out_col = d->out_colors;
    a.out_keys = d->out_keys;
    a.out_counts = d->out_counts;
    voxel_means_kernel<<<(unsigned)((d->N + 255) / 256), 256, 0, st>>>(a);
    return check_launch("cn_voxel_reduce");
}

extern "C" int cn_cloud_normals(const cn_cloud_normals_desc* d, cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_cloud_normals: null descriptor");
    CN_REQUIRE(d->N >= 0 && d->N <= kMaxCount, CN_ERR_SHAPE, "cn_cloud_normals: N %lld (in [0, 2^31))", (long long)d->N);
    CN_REQUIRE(d->k >= 1 && d->k <= 32, CN_ERR_SHAPE, "cn_cloud_normals: k %d (in [1, 32])", d->k);
    CN_REQUIRE(d->orient == 0 || d->orient == 1, CN_ERR_ARG, "cn_cloud_normals: orient %d", d->orient);
    if (d->orient)
        for (int i = 0; i < 3; ++i)
            CN_REQUIRE(std::isfinite(d->orient_to[i]), CN_ERR_SHAPE, "cn_cloud_normals: orient_to[%d] is not finite", i);
    if (d->N == 0) return CN_OK;
    CN_REQUIRE(d->points && d->index && d->normals, CN_ERR_ARG, "cn_cloud_normals: null points / index / normals");
    CN_REQUIRE((((uintptr_t)d->points | (uintptr_t)d->index | (uintptr_t)d->normals | (uintptr_t)d->variation) & 3) == 0,
               CN_ERR_ALIGN, "cn_cloud_normals: points / index / normals / variation 4-byte aligned");
    NormalsArgs a{};
    a.N = d->N;
    a.k = d->k;
    a.orient = d->orient;
    a.pts = d->points;
    a.index = d->index;
    for (int i = 0; i < 3; ++i) a.to[i] = d->orient_to[i];
    a.normals = d->normals;
    a.variation = d->variation;
    cloud_normals_kernel<<<(unsigned)((d->N + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
    return check_launch("cn_cloud_normals");
}

extern "C" size_t cn_knn_mean_stats_workspace_bytes(int64_t N) {
    if (N < 0 || N > kMaxCount) return 0;
    return rup_sz((size_t)stats_blocks(N) * 3 * sizeof(double));
}

extern "C" int cn_knn_mean_stats(const cn_knn_mean_stats_desc* d, void* workspace, int64_t workspace_bytes,
                                 cn_stream_t stream) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_knn_mean_stats: null descriptor");
    CN_REQUIRE(d->N >= 0 && d->N <= kMaxCount, CN_ERR_SHAPE, "cn_knn_mean_stats: N %lld (in [0, 2^31))", (long long)d->N);
    CN_REQUIRE(d->k >= 1 && d->k <= 32, CN_ERR_SHAPE, "cn_knn_mean_stats: k %d (in [1, 32])", d->k);
    CN_REQUIRE(d->out, CN_ERR_ARG, "cn_knn_mean_stats: null out");
    CN_REQUIRE(d->N == 0 || (d->dist && d->index && d->mean), CN_ERR_ARG, "cn_knn_mean_stats: null dist / index / mean");
    CN_REQUIRE((((uintptr_t)d->dist | (uintptr_t)d->index | (uintptr_t)d->mean) & 3) == 0 && ((uintptr_t)d->out & 7) == 0,
               CN_ERR_ALIGN, "cn_knn_mean_stats: dist / index / mean 4-byte, out 8-byte aligned");
    const size_t need = cn_knn_mean_stats_workspace_bytes(d->N);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_knn_mean_stats: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_knn_mean_stats: workspace not 256-byte aligned");
    MeanStatsArgs a{};
    a.N = d->N;
    a.k = d->k;
    a.dist = d->dist;
    a.index = d->index;
    a.mean = d->mean;
    a.part = static_cast<double*>(workspace);
    a.out = d->out;
    hipStream_t st = (hipStream_t)stream;
    const int nb = stats_blocks(d->N);
    knn_mean_partial_kernel<<<nb, kStatsThreads, 0, st>>>(a);
    int rc = check_launch("cn_knn_mean_stats");
    if (rc) return rc;
    knn_mean_final_kernel<<<1, kStatsThreads, 0, st>>>(nb, a.part, a.out);
    return check_launch("cn_knn_mean_stats");
}
