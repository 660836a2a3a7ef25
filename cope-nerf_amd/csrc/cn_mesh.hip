// cn_mesh.hip — mesh extraction (ABI v16): the grid points of a bounding box, the SDF volume over them
// (cn_grid_points + cn_sdf_query in row chunks) and the isosurface of a volume as a welded triangle mesh
// by marching tetrahedra on the six-tetrahedron Kuhn split (cn_mesh_count / cn_mesh_emit); and floater removal
// on any indexed triangle list: connected components by label propagation with pointer jumping
// (cn_mesh_label_init / cn_mesh_label_rounds), the triangles per component (cn_mesh_component_sizes) and the
// compaction to the kept components through the mesher's scans (cn_mesh_select / cn_mesh_compact).
// cn_mesh_count_observed / cn_mesh_emit_observed (additive to ABI v22) are the two mesher kernels compiled with
// OBS = true: NaN in u means unobserved, an edge carries a vertex only between two observed ends and a cell emits
// triangles only with its eight corners observed (the volumes of cn_tsdf.hip).
//
// Reference: NeuSRenderer.extract_geometry / extract_fields (neus_renderer.py:10-37): the interface and the
// grid (torch.linspace per axis, u[xi, yi, zi], vertices / (resolution - 1) * (max - min) + min).  The
// reference's mesher (PyMCubes on 3-column points) is replaced, see DESIGN.md "Mesh extraction".
//
// Ordering never depends on atomics or on scheduling: a count pass writes one byte per grid vertex (the
// 7-bit mask of the edges it owns that cross the threshold) and one byte per cell (its triangle count),
// both are scanned (reduce per 1024-element tile, one block scans the tile totals, a third launch adds
// back -- no workgroup waits for another), and the emit pass writes every vertex and triangle at its
// scanned offset.  All kernels run one thread per grid vertex with z the fastest thread index, so the
// loads of u coalesce and the stencil's reuse of the neighbouring rows and planes is the cache's.
#include "cn_common.h"
#include "cn_mesh_table.h"

namespace cn {
namespace {

__constant__ TetTable kTet = make_tet_table();

// (the scans' block_excl_scan and tile constants: cn_common.h)

// torch.linspace(lo, hi, n)[i] on fp32 (RangeFactoriesKernel.cpp): from lo below the middle, from hi above
__device__ __forceinline__ float linspace_at(float lo, float hi, int n, int i) {
    if (n == 1) return lo;
    const float step = (hi - lo) / (float)(n - 1);
    return i < n / 2 ? lo + (float)i * step : hi - (float)(n - 1 - i) * step;
}

struct Box {
    float lo[3], hi[3];
};

__global__ void grid_points_kernel(int nx, int ny, int nz, Box b, const float* __restrict__ t, int64_t m0, int M,
                                   float* __restrict__ pts) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int64_t idx = m0 + m;
    const int iz = (int)(idx % nz);
    const int64_t r = idx / nz;
    const int iy = (int)(r % ny), ix = (int)(r / ny);
    floatx4 o;
    o[0] = linspace_at(b.lo[0], b.hi[0], nx, ix);
    o[1] = linspace_at(b.lo[1], b.hi[1], ny, iy);
    o[2] = linspace_at(b.lo[2], b.hi[2], nz, iz);
    o[3] = t[0];
    reinterpret_cast<floatx4*>(pts)[m] = o;
}

struct MeshArgs {
    int nx, ny, nz;
    const float* u;
    float thr;
    Box box;
    uint8_t* emask;     // [N] the owned-edge mask of every grid vertex
    int32_t* voff;      // [N] exclusive scan of popcount(emask)
    uint8_t* tcount;    // [C] triangles of every cell
    int32_t* toff;      // [C] exclusive scan of tcount
    float* vertices;
    int32_t* triangles;
    int64_t max_vertices, max_triangles;
    const int64_t* counts;
};

// The thread's grid vertex p = (ix, iy, iz), the values at p + o for the eight offsets o = ox + 2 oy + 4 oz
// (p's own value where p + o is outside the grid) and which of them are inside the grid.  OBS (the *_observed
// entry points): a NaN value is an unobserved grid vertex, and `have` keeps only the observed ones.
struct Stencil {
    int ix, iy, iz, p;
    float v[8];
    int have;  // bit o: p + o is a grid vertex (OBS: and observed)
    int grid;  // OBS only -- bit o: p + o is a grid vertex
};

template <bool OBS>
__device__ __forceinline__ bool load_stencil(const MeshArgs& a, Stencil* s) {
    const int N = a.nx * a.ny * a.nz;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return false;
    s->p = p;
    s->iz = p % a.nz;
    const int r = p / a.nz;
    s->iy = r % a.ny;
    s->ix = r / a.ny;
    const bool hx = s->ix + 1 < a.nx, hy = s->iy + 1 < a.ny, hz = s->iz + 1 < a.nz;
    s->have = 0;
    if (OBS) s->grid = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        const bool ok = (!(o & 1) || hx) && (!(o & 2) || hy) && (!(o & 4) || hz);
        const int q = p + ((o & 1) ? a.ny * a.nz : 0) + ((o & 2) ? a.nz : 0) + ((o & 4) ? 1 : 0);
        s->v[o] = a.u[ok ? q : p];
        if (OBS) {
            s->grid |= ok ? 1 << o : 0;
            s->have |= ok && s->v[o] == s->v[o] ? 1 << o : 0;
        } else {
            s->have |= ok ? 1 << o : 0;
        }
    }
    return true;
}

// bit o: the value at p + o is below the threshold (strictly: a tie is outside, and so is a NaN)
__device__ __forceinline__ int inside_bits(const Stencil& s, float thr) {
    int in = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) in |= s.v[o] < thr ? 1 << o : 0;
    return in;
}

// the 7-bit mask of p's owned edges (slot d - 1, d = dx + 2 dy + 4 dz) whose ends differ (OBS: and are both observed)
template <bool OBS>
__device__ __forceinline__ int edge_mask(const Stencil& s, int in) {
    const int differ = (in ^ ((in & 1) ? 0xff : 0)) & s.have;
    if (OBS && !(s.have & 1)) return 0;
    return differ >> 1;
}

// the 4-bit mask of tetrahedron k from the cell's 8 inside bits
__device__ __forceinline__ int tet_mask(int in, int k) {
    const uint32_t c = kTet.corner[k];
    return (in & 1) | ((in >> ((c >> 3) & 7)) & 1) << 1 | ((in >> ((c >> 6) & 7)) & 1) << 2 | ((in >> 7) & 1) << 3;
}

template <bool OBS>
__global__ void mesh_count_kernel(MeshArgs a) {
    Stencil s;
    if (!load_stencil<OBS>(a, &s)) return;
    const int in = inside_bits(s, a.thr);
    a.emask[s.p] = (uint8_t)edge_mask<OBS>(s, in);
    if ((OBS ? s.grid : s.have) == 0xff) {
        int n = 0;
        if (in != 0 && in != 0xff && (!OBS || s.have == 0xff)) {  // OBS: a cell with an unobserved corner has no triangle
#pragma unroll
            for (int k = 0; k < 6; ++k) n += kTet.entry[k * 16 + tet_mask(in, k)] & 3;
        }
        const int cell = (s.ix * (a.ny - 1) + s.iy) * (a.nz - 1) + s.iz;
        a.tcount[cell] = (uint8_t)n;
    }
}

template <bool POPC>
__device__ __forceinline__ int scan_item(const uint8_t* __restrict__ c, int i, int n) {
    if (i >= n) return 0;
    const int v = c[i];
    return POPC ? __popc(v) : v;
}

// launch 1: tot[b] = the sum of tile b
template <bool POPC>
__global__ void scan_reduce_kernel(const uint8_t* __restrict__ c, int n, int32_t* __restrict__ tot) {
    const int i0 = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int x = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) x += scan_item<POPC>(c, i0 + j, n);
    int all;
    block_excl_scan(x, &all);
    if (threadIdx.x == 0) tot[blockIdx.x] = all;
}

// launch 2 (one block): tot[] -> its exclusive scan in place, *total = the grand total
__global__ void scan_totals_kernel(int32_t* __restrict__ tot, int nt, int64_t* __restrict__ total) {
    int carry = 0;
    for (int base = 0; base < nt; base += kScanTile) {
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

// launch 3: off[i] = tot[tile of i] + the exclusive scan inside the tile
template <bool POPC>
__global__ void scan_apply_kernel(const uint8_t* __restrict__ c, int n, const int32_t* __restrict__ tot,
                                  int32_t* __restrict__ off) {
    const int i0 = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int v[kScanItems], x = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        v[j] = scan_item<POPC>(c, i0 + j, n);
        x += v[j];
    }
    int all;
    int run = tot[blockIdx.x] + block_excl_scan(x, &all);
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (i0 + j < n) off[i0 + j] = run;
        run += v[j];
    }
}

template <bool OBS>
__global__ void mesh_emit_kernel(MeshArgs a) {
    // output buffers smaller than the counts: nothing is written (the decision is the same in every thread)
    const int64_t V = a.counts[0], T = a.counts[1];
    if (V > a.max_vertices || T > a.max_triangles) return;
    Stencil s;
    if (!load_stencil<OBS>(a, &s)) return;
    const int in = inside_bits(s, a.thr);
    const int em = edge_mask<OBS>(s, in);
    if (em) {
        // the vertices on p's owned edges, ascending by slot
        int id = a.voff[s.p];
        const float pf[3] = {(float)s.ix, (float)s.iy, (float)s.iz};
        const float den[3] = {(float)(a.nx - 1), (float)(a.ny - 1), (float)(a.nz - 1)};
#pragma unroll
        for (int slot = 0; slot < 7; ++slot) {
            if (!(em >> slot & 1) || id >= a.max_vertices) continue;  // (the bound holds whenever u is count's)
            const int d = slot + 1;
            const float t = (a.thr - s.v[0]) / (s.v[d] - s.v[0]);
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const float pos = (d >> ax & 1) ? pf[ax] + t : pf[ax];
                a.vertices[(int64_t)id * 3 + ax] = pos / den[ax] * (a.box.hi[ax] - a.box.lo[ax]) + a.box.lo[ax];
            }
            ++id;
        }
    }
    if (s.have != 0xff || in == 0 || in == 0xff) return;
    // the cell's triangles, ascending by (tetrahedron, triangle); a vertex id is its owner's offset plus the
    // number of the owner's crossing edges in lower slots
    const int cell = (s.ix * (a.ny - 1) + s.iy) * (a.nz - 1) + s.iz;
    int64_t t = a.toff[cell];
    int base[8], qm[8];
#pragma unroll
    for (int o = 0; o < 7; ++o) {  // (corner 7 owns no edge of this cell)
        const int q = s.p + ((o & 1) ? a.ny * a.nz : 0) + ((o & 2) ? a.nz : 0) + ((o & 4) ? 1 : 0);
        base[o] = a.voff[q];
        qm[o] = o == 0 ? em : a.emask[q];
    }
    base[7] = qm[7] = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const uint32_t c = kTet.corner[k];
        const uint32_t e = kTet.entry[k * 16 + tet_mask(in, k)];
        const int nt = e & 3;
        for (int tt = 0; tt < nt && t < a.max_triangles; ++tt) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t ed = e >> (4 + 12 * tt + 4 * j);
                const int oa = (c >> (3 * (ed & 3))) & 7, ob = (c >> (3 * ((ed >> 2) & 3))) & 7;
                const int slot = (oa ^ ob) - 1;
                int bq = 0, mq = 0;
#pragma unroll
                for (int o = 0; o < 7; ++o) {  // (a select chain keeps base / qm in registers)
                    bq = oa == o ? base[o] : bq;
                    mq = oa == o ? qm[o] : mq;
                }
                a.triangles[t * 3 + j] = bq + __popc(mq & ((1 << slot) - 1));
            }
            ++t;
        }
    }
}

int dims_check(const char* who, int nx, int ny, int nz) {
    CN_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, CN_ERR_SHAPE, "%s: dims %d x %d x %d (each at least 2)", who, nx, ny, nz);
    const int64_t N = (int64_t)nx * ny * nz, C = (int64_t)(nx - 1) * (ny - 1) * (nz - 1);
    CN_REQUIRE(nx < (1 << 20) && ny < (1 << 20) && nz < (1 << 20) && 7 * N < ((int64_t)1 << 31) &&
                   12 * C < ((int64_t)1 << 31),
               CN_ERR_SHAPE, "%s: dims %d x %d x %d too large (7 x vertices and 12 x cells must stay below 2^31)", who, nx,
               ny, nz);
    return CN_OK;
}

constexpr size_t kAlign = 256;
size_t rup_sz(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct MeshPlan {
    uint8_t* emask;
    int32_t* voff;
    uint8_t* tcount;
    int32_t* toff;
    int32_t* vtot;
    int32_t* ttot;
    int N, C, vt, ct;
    size_t bytes;
};

MeshPlan mesh_plan(int nx, int ny, int nz, void* ws) {
    MeshPlan p{};
    p.N = nx * ny * nz;
    p.C = (nx - 1) * (ny - 1) * (nz - 1);
    p.vt = (p.N + kScanTile - 1) / kScanTile;
    p.ct = (p.C + kScanTile - 1) / kScanTile;
    char* b = static_cast<char*>(ws);
    size_t used = 0;
    auto take = [&](size_t n) {
        char* q = b ? b + used : nullptr;
        used += rup_sz(n);
        return q;
    };
    p.emask = reinterpret_cast<uint8_t*>(take((size_t)p.N));
    p.voff = reinterpret_cast<int32_t*>(take((size_t)p.N * 4));
    p.tcount = reinterpret_cast<uint8_t*>(take((size_t)p.C));
    p.toff = reinterpret_cast<int32_t*>(take((size_t)p.C * 4));
    p.vtot = reinterpret_cast<int32_t*>(take((size_t)p.vt * 4));
    p.ttot = reinterpret_cast<int32_t*>(take((size_t)p.ct * 4));
    p.bytes = used;
    return p;
}

int mesh_check(const char* who, const cn_mesh_desc* d, const void* ws, int64_t ws_bytes, bool emit) {
    CN_REQUIRE(d, CN_ERR_ARG, "%s: null descriptor", who);
    int rc = dims_check(who, d->nx, d->ny, d->nz);
    if (rc) return rc;
    CN_REQUIRE(d->u && d->counts, CN_ERR_ARG, "%s: null u / counts", who);
    CN_REQUIRE(((uintptr_t)d->u & 3) == 0 && ((uintptr_t)d->counts & 7) == 0, CN_ERR_ALIGN,
               "%s: u 4-byte, counts 8-byte aligned", who);
    const size_t need = cn_mesh_workspace_bytes(d->nx, d->ny, d->nz);
    CN_REQUIRE(ws && ws_bytes >= 0 && (size_t)ws_bytes >= need, CN_ERR_SHAPE, "%s: workspace %lld bytes, %zu needed", who,
               (long long)ws_bytes, need);
    CN_REQUIRE(((uintptr_t)ws & (kAlign - 1)) == 0, CN_ERR_ALIGN, "%s: workspace not 256-byte aligned", who);
    if (emit) {
        CN_REQUIRE(d->max_vertices >= 0 && d->max_triangles >= 0, CN_ERR_SHAPE, "%s: max_vertices %lld / max_triangles %lld",
                   who, (long long)d->max_vertices, (long long)d->max_triangles);
        CN_REQUIRE((d->max_vertices == 0 || d->vertices) && (d->max_triangles == 0 || d->triangles), CN_ERR_ARG,
                   "%s: null vertices / triangles", who);
        CN_REQUIRE(((uintptr_t)d->vertices & 3) == 0 && ((uintptr_t)d->triangles & 3) == 0, CN_ERR_ALIGN,
                   "%s: vertices / triangles 4-byte aligned", who);
    }
    return CN_OK;
}

MeshArgs mesh_args(const cn_mesh_desc* d, const MeshPlan& p) {
    MeshArgs a{};
    a.nx = d->nx;
    a.ny = d->ny;
    a.nz = d->nz;
    a.u = d->u;
    a.thr = d->threshold;
    for (int i = 0; i < 3; ++i) {
        a.box.lo[i] = d->lo[i];
        a.box.hi[i] = d->hi[i];
    }
    a.emask = p.emask;
    a.voff = p.voff;
    a.tcount = p.tcount;
    a.toff = p.toff;
    a.vertices = d->vertices;
    a.triangles = d->triangles;
    a.max_vertices = d->max_vertices;
    a.max_triangles = d->max_triangles;
    a.counts = d->counts;
    return a;
}

template <bool POPC>
int scan_launch(const char* who, const uint8_t* c, int n, int tiles, int32_t* tot, int32_t* off, int64_t* total,
                hipStream_t st) {
    scan_reduce_kernel<POPC><<<tiles, kScanThreads, 0, st>>>(c, n, tot);
    int rc = check_launch(who);
    if (rc) return rc;
    scan_totals_kernel<<<1, kScanThreads, 0, st>>>(tot, tiles, total);
    if ((rc = check_launch(who))) return rc;
    scan_apply_kernel<POPC><<<tiles, kScanThreads, 0, st>>>(c, n, tot, off);
    return check_launch(who);
}

// -- connected components of an indexed triangle list, and its compaction to the kept ones -----------------
// Labels are vertex ids of the vertex's own component and only ever fall (atomicMin, or a jump to a label
// that is itself a lower id), so whatever order the atomics land in, the only fixed point is the smallest id
// of every component.  A round is two launches; nothing waits for another workgroup.
struct CleanArgs {
    int V, T;
    const int32_t* tri;
    int32_t* label;
    int32_t* tri_count;
    int keep_largest, min_triangles;
    uint8_t* vflag;     // [V] 1: the vertex's component is kept
    int32_t* voff;      // [V] exclusive scan of vflag
    uint8_t* tflag;     // [T]
    int32_t* toff;      // [T]
    uint64_t* best;     // the largest component: (triangles << 32) | ~root
    const int64_t* counts;
    int32_t* kept_vertices;
    int32_t* tri_out;
    int64_t max_vertices, max_triangles;
};

__device__ __forceinline__ int label_at(const int32_t* label, int v) {
    return __atomic_load_n(label + v, __ATOMIC_RELAXED);  // (other threads lower it meanwhile)
}

__global__ void label_init_kernel(int V, int32_t* __restrict__ label) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < V) label[v] = v;
}

__global__ void clear_flag_kernel(int32_t* changed) { *changed = 0; }

__global__ void label_hook_kernel(int V, int T, const int32_t* __restrict__ tri, int32_t* label, int32_t* changed) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    int c[3], l[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        c[j] = tri[(int64_t)t * 3 + j];
        if ((unsigned)c[j] >= (unsigned)V) return;  // an index outside the vertex list joins nothing
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) l[j] = label_at(label, c[j]);
    const int m = min(l[0], min(l[1], l[2]));
    bool lowered = false;
#pragma unroll
    for (int j = 0; j < 3; ++j)
        if (l[j] > m) lowered |= atomicMin(label + c[j], m) > m;
    if (lowered) *changed = 1;
}

__global__ void label_jump_kernel(int V, int32_t* label, int32_t* changed) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int l = label_at(label, v);
    if ((unsigned)l >= (unsigned)V) return;  // (never after cn_mesh_label_init: labels start as ids and fall to ids)
    const int ll = label_at(label, l);
    if (ll < l) {
        atomicMin(label + v, ll);
        *changed = 1;
    }
}

__global__ void zero_i32_kernel(int n, int32_t* __restrict__ p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

// root of triangle t: the label of its first corner, or -1 where that index is outside the vertex list
__device__ __forceinline__ int tri_root(const CleanArgs& a, int t) {
    const int c = a.tri[(int64_t)t * 3];
    return (unsigned)c < (unsigned)a.V ? a.label[c] : -1;
}

__global__ void component_sizes_kernel(CleanArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T) return;
    const int r = tri_root(a, t);
    if ((unsigned)r < (unsigned)a.V) atomicAdd(a.tri_count + r, 1);
}

__global__ void best_clear_kernel(uint64_t* best) { *best = 0; }

// the largest component, a tie to the smaller root: the maximum of (count, ~root) does not depend on the order
__global__ void best_component_kernel(CleanArgs a) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.V) return;
    const int n = a.tri_count[v];
    if (n > 0) atomicMax((unsigned long long*)a.best, ((unsigned long long)n << 32) | (uint32_t)~(uint32_t)v);
}

__device__ __forceinline__ bool root_kept(const CleanArgs& a, int r) {
    if ((unsigned)r >= (unsigned)a.V) return false;
    const int n = a.tri_count[r];
    if (n < a.min_triangles) return false;
    if (!a.keep_largest) return true;
    const uint64_t b = *a.best;
    return b != 0 && (uint32_t)~(uint32_t)b == (uint32_t)r;
}

// one thread per index of max(V, T): the vertex's flag and the triangle's
__global__ void select_flags_kernel(CleanArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.V) a.vflag[i] = root_kept(a, a.label[i]) ? 1 : 0;
    if (i < a.T) a.tflag[i] = root_kept(a, tri_root(a, i)) ? 1 : 0;
}

// the same flags from a caller's per-vertex mask: a triangle is kept when its three corners are
__global__ void select_mask_flags_kernel(CleanArgs a, const uint8_t* __restrict__ vmask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.V) a.vflag[i] = vmask[i] ? 1 : 0;
    if (i < a.T) {
        bool keep = true;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int c = a.tri[(int64_t)i * 3 + j];
            keep = keep && (unsigned)c < (unsigned)a.V && vmask[c];
        }
        a.tflag[i] = keep ? 1 : 0;
    }
}

__global__ void compact_kernel(CleanArgs a) {
    // output buffers smaller than the counts: nothing is written (the decision is the same in every thread)
    if (a.counts[0] > a.max_vertices || a.counts[1] > a.max_triangles) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.V && a.vflag[i]) {
        const int o = a.voff[i];
        if (o < a.max_vertices) a.kept_vertices[o] = i;
    }
    if (i < a.T && a.tflag[i]) {
        const int64_t o = a.toff[i];
        if (o >= a.max_triangles) return;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // (a kept triangle's corners share its component only in a well-formed list: an index outside the
            // vertex list, or a corner that was not kept, is written as -1, never read out of bounds)
            const int c = a.tri[(int64_t)i * 3 + j];
            a.tri_out[o * 3 + j] = ((unsigned)c < (unsigned)a.V && a.vflag[c]) ? a.voff[c] : -1;
        }
    }
}

struct CleanPlan {
    uint8_t* vflag;
    uint8_t* tflag;
    int32_t* voff;
    int32_t* toff;
    int32_t* vtot;
    int32_t* ttot;
    uint64_t* best;
    int vt, tt;
    size_t bytes;
};

CleanPlan clean_plan(int V, int T, void* ws) {
    CleanPlan p{};
    p.vt = V ? (V + kScanTile - 1) / kScanTile : 1;
    p.tt = T ? (T + kScanTile - 1) / kScanTile : 1;
    char* b = static_cast<char*>(ws);
    size_t used = 0;
    auto take = [&](size_t n) {
        char* q = b ? b + used : nullptr;
        used += rup_sz(n);
        return q;
    };
    p.vflag = reinterpret_cast<uint8_t*>(take((size_t)V));
    p.tflag = reinterpret_cast<uint8_t*>(take((size_t)T));
    p.voff = reinterpret_cast<int32_t*>(take((size_t)V * 4));
    p.toff = reinterpret_cast<int32_t*>(take((size_t)T * 4));
    p.vtot = reinterpret_cast<int32_t*>(take((size_t)p.vt * 4));
    p.ttot = reinterpret_cast<int32_t*>(take((size_t)p.tt * 4));
    p.best = reinterpret_cast<uint64_t*>(take(8));
    p.bytes = used;
    return p;
}

// the descriptor's sizes and the pointers every entry reads
int clean_check(const char* who, const cn_mesh_clean_desc* d, bool need_label) {
    CN_REQUIRE(d, CN_ERR_ARG, "%s: null descriptor", who);
    CN_REQUIRE(d->V >= 0 && d->T >= 0, CN_ERR_SHAPE, "%s: V %d, T %d", who, d->V, d->T);
    CN_REQUIRE(d->T == 0 || d->triangles, CN_ERR_ARG, "%s: null triangles", who);
    CN_REQUIRE(!need_label || d->V == 0 || d->label, CN_ERR_ARG, "%s: null label", who);
    CN_REQUIRE(((uintptr_t)d->triangles & 3) == 0 && ((uintptr_t)d->label & 3) == 0, CN_ERR_ALIGN,
               "%s: triangles / label 4-byte aligned", who);
    return CN_OK;
}

int clean_ws_check(const char* who, const cn_mesh_clean_desc* d, const void* ws, int64_t ws_bytes) {
    int rc = clean_check(who, d, true);
    if (rc) return rc;
    CN_REQUIRE(d->V == 0 || d->tri_count, CN_ERR_ARG, "%s: null tri_count", who);
    CN_REQUIRE(d->counts, CN_ERR_ARG, "%s: null counts", who);
    CN_REQUIRE(((uintptr_t)d->tri_count & 3) == 0 && ((uintptr_t)d->counts & 7) == 0, CN_ERR_ALIGN,
               "%s: tri_count 4-byte, counts 8-byte aligned", who);
    CN_REQUIRE(d->min_triangles >= 0, CN_ERR_SHAPE, "%s: min_triangles %d", who, d->min_triangles);
    const size_t need = clean_plan(d->V, d->T, nullptr).bytes;
    CN_REQUIRE(ws && ws_bytes >= 0 && (size_t)ws_bytes >= need, CN_ERR_SHAPE, "%s: workspace %lld bytes, %zu needed", who,
               (long long)ws_bytes, need);
    CN_REQUIRE(((uintptr_t)ws & (kAlign - 1)) == 0, CN_ERR_ALIGN, "%s: workspace not 256-byte aligned", who);
    return CN_OK;
}

CleanArgs clean_args(const cn_mesh_clean_desc* d, const CleanPlan& p) {
    CleanArgs a{};
    a.V = d->V;
    a.T = d->T;
    a.tri = d->triangles;
    a.label = d->label;
    a.tri_count = d->tri_count;
    a.keep_largest = d->keep_largest;
    a.min_triangles = d->min_triangles;
    a.vflag = p.vflag;
    a.voff = p.voff;
    a.tflag = p.tflag;
    a.toff = p.toff;
    a.best = p.best;
    a.counts = d->counts;
    a.kept_vertices = d->kept_vertices;
    a.tri_out = d->triangles_out;
    a.max_vertices = d->max_vertices;
    a.max_triangles = d->max_triangles;
    return a;
}

}  // namespace
}  // namespace cn

using namespace cn;

extern "C" int cn_grid_points(int32_t nx, int32_t ny, int32_t nz, const float* lo, const float* hi,
                              const float* time_step, int64_t m0, int32_t M, float* pts, cn_stream_t stream) {
    CN_REQUIRE(lo && hi, CN_ERR_ARG, "cn_grid_points: null lo / hi");
    CN_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1, CN_ERR_SHAPE, "cn_grid_points: dims %d x %d x %d", nx, ny, nz);
    const int64_t total = (int64_t)nx * ny * nz;
    CN_REQUIRE(M >= 0 && m0 >= 0 && m0 <= total && M <= total - m0, CN_ERR_SHAPE,
               "cn_grid_points: rows [%lld, %lld + %d) of %lld", (long long)m0, (long long)m0, M, (long long)total);
    if (M == 0) return CN_OK;
    CN_REQUIRE(time_step && pts, CN_ERR_ARG, "cn_grid_points: null time_step / pts");
    CN_REQUIRE(((uintptr_t)pts & 15) == 0, CN_ERR_ALIGN, "cn_grid_points: pts not 16-byte aligned");
    Box b;
    for (int i = 0; i < 3; ++i) {
        b.lo[i] = lo[i];
        b.hi[i] = hi[i];
    }
    grid_points_kernel<<<(M + 255) / 256, 256, 0, (hipStream_t)stream>>>(nx, ny, nz, b, time_step, m0, M, pts);
    return check_launch("cn_grid_points");
}

namespace {

constexpr int32_t kDefaultChunk = 1 << 20;

int sdf_grid_check(const cn_sdf_grid_desc* d, int32_t* chunk) {
    CN_REQUIRE(d, CN_ERR_ARG, "cn_sdf_grid: null descriptor");
    CN_REQUIRE(d->net, CN_ERR_ARG, "cn_sdf_grid: null net");
    CN_REQUIRE(d->nx >= 1 && d->ny >= 1 && d->nz >= 1, CN_ERR_SHAPE, "cn_sdf_grid: dims %d x %d x %d", d->nx, d->ny,
               d->nz);
    CN_REQUIRE(d->chunk_rows >= 0, CN_ERR_SHAPE, "cn_sdf_grid: chunk_rows %d", d->chunk_rows);
    // every chunk is one cn_sdf_query: below the fused bf16x6 query's row bound (M x 64 x 4 bytes < 2^31)
    CN_REQUIRE((int64_t)d->chunk_rows * 64 * 4 < ((int64_t)1 << 31), CN_ERR_SHAPE,
               "cn_sdf_grid: chunk_rows %d too large (chunk_rows x 256 bytes must stay below 2^31)", d->chunk_rows);
    const int64_t total = (int64_t)d->nx * d->ny * d->nz;
    const int64_t c = d->chunk_rows ? d->chunk_rows : kDefaultChunk;
    *chunk = (int32_t)(c < total ? c : total);
    return CN_OK;
}

}  // namespace

extern "C" size_t cn_sdf_grid_workspace_bytes(const cn_sdf_grid_desc* d) {
    int32_t chunk;
    if (sdf_grid_check(d, &chunk) != CN_OK) return 0;
    const size_t q = cn_sdf_query_workspace_bytes(d->net, chunk);
    if (q == 0) return 0;
    return rup_sz((size_t)chunk * 16) + q;
}

extern "C" int cn_sdf_grid(const cn_sdf_grid_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int32_t chunk;
    int rc = sdf_grid_check(d, &chunk);
    if (rc) return rc;
    CN_REQUIRE(d->time_step && d->u, CN_ERR_ARG, "cn_sdf_grid: null time_step / u");
    const size_t need = cn_sdf_grid_workspace_bytes(d);
    // (a network cn_sdf_query refuses sizes to 0: report its own message)
    if (need == 0) return cn_sdf_query(d->net, chunk, nullptr, 4, nullptr, nullptr, nullptr, 0, stream);
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_sdf_grid: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_sdf_grid: workspace not 256-byte aligned");
    float* pts = static_cast<float*>(workspace);
    const size_t pbytes = rup_sz((size_t)chunk * 16);
    char* qws = static_cast<char*>(workspace) + pbytes;
    const int64_t qbytes = workspace_bytes - (int64_t)pbytes;
    const int64_t total = (int64_t)d->nx * d->ny * d->nz;
    for (int64_t m0 = 0; m0 < total; m0 += chunk) {
        const int32_t M = (int32_t)(total - m0 < chunk ? total - m0 : chunk);
        if ((rc = cn_grid_points(d->nx, d->ny, d->nz, d->lo, d->hi, d->time_step, m0, M, pts, stream))) return rc;
        if ((rc = cn_sdf_query(d->net, M, pts, 4, d->u + m0, nullptr, qws, qbytes, stream))) return rc;
    }
    return CN_OK;
}

extern "C" size_t cn_mesh_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (dims_check("cn_mesh_workspace_bytes", nx, ny, nz) != CN_OK) return 0;
    return mesh_plan(nx, ny, nz, nullptr).bytes;
}

namespace {

template <bool OBS>
int mesh_count_launch(const char* who, const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int rc = mesh_check(who, d, workspace, workspace_bytes, false);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const MeshPlan p = mesh_plan(d->nx, d->ny, d->nz, workspace);
    const MeshArgs a = mesh_args(d, p);
    mesh_count_kernel<OBS><<<(p.N + 255) / 256, 256, 0, st>>>(a);
    if ((rc = check_launch(who))) return rc;
    if ((rc = scan_launch<true>(who, p.emask, p.N, p.vt, p.vtot, p.voff, d->counts, st))) return rc;
    return scan_launch<false>(who, p.tcount, p.C, p.ct, p.ttot, p.toff, d->counts + 1, st);
}

template <bool OBS>
int mesh_emit_launch(const char* who, const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int rc = mesh_check(who, d, workspace, workspace_bytes, true);
    if (rc) return rc;
    const MeshPlan p = mesh_plan(d->nx, d->ny, d->nz, workspace);
    const MeshArgs a = mesh_args(d, p);
    mesh_emit_kernel<OBS><<<(p.N + 255) / 256, 256, 0, (hipStream_t)stream>>>(a);
    return check_launch(who);
}

}  // namespace

extern "C" int cn_mesh_count(const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    return mesh_count_launch<false>("cn_mesh_count", d, workspace, workspace_bytes, stream);
}

extern "C" int cn_mesh_emit(const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    return mesh_emit_launch<false>("cn_mesh_emit", d, workspace, workspace_bytes, stream);
}

extern "C" int cn_mesh_count_observed(const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    return mesh_count_launch<true>("cn_mesh_count_observed", d, workspace, workspace_bytes, stream);
}

extern "C" int cn_mesh_emit_observed(const cn_mesh_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    return mesh_emit_launch<true>("cn_mesh_emit_observed", d, workspace, workspace_bytes, stream);
}

extern "C" int cn_mesh_label_init(const cn_mesh_clean_desc* d, cn_stream_t stream) {
    int rc = clean_check("cn_mesh_label_init", d, true);
    if (rc || d->V == 0) return rc;
    label_init_kernel<<<(d->V + 255) / 256, 256, 0, (hipStream_t)stream>>>(d->V, d->label);
    return check_launch("cn_mesh_label_init");
}

extern "C" int cn_mesh_label_rounds(const cn_mesh_clean_desc* d, int32_t k, int32_t* changed, cn_stream_t stream) {
    int rc = clean_check("cn_mesh_label_rounds", d, true);
    if (rc) return rc;
    CN_REQUIRE(k >= 1, CN_ERR_SHAPE, "cn_mesh_label_rounds: k %d", k);
    CN_REQUIRE(changed, CN_ERR_ARG, "cn_mesh_label_rounds: null changed");
    CN_REQUIRE(((uintptr_t)changed & 3) == 0, CN_ERR_ALIGN, "cn_mesh_label_rounds: changed 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    clear_flag_kernel<<<1, 1, 0, st>>>(changed);
    if ((rc = check_launch("cn_mesh_label_rounds"))) return rc;
    if (d->V == 0 || d->T == 0) return CN_OK;
    for (int i = 0; i < k; ++i) {
        label_hook_kernel<<<(d->T + 255) / 256, 256, 0, st>>>(d->V, d->T, d->triangles, d->label, changed);
        if ((rc = check_launch("cn_mesh_label_rounds"))) return rc;
        label_jump_kernel<<<(d->V + 255) / 256, 256, 0, st>>>(d->V, d->label, changed);
        if ((rc = check_launch("cn_mesh_label_rounds"))) return rc;
    }
    return CN_OK;
}

extern "C" int cn_mesh_component_sizes(const cn_mesh_clean_desc* d, cn_stream_t stream) {
    int rc = clean_check("cn_mesh_component_sizes", d, true);
    if (rc || d->V == 0) return rc;
    CN_REQUIRE(d->tri_count, CN_ERR_ARG, "cn_mesh_component_sizes: null tri_count");
    CN_REQUIRE(((uintptr_t)d->tri_count & 3) == 0, CN_ERR_ALIGN, "cn_mesh_component_sizes: tri_count 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    zero_i32_kernel<<<(d->V + 255) / 256, 256, 0, st>>>(d->V, d->tri_count);
    if ((rc = check_launch("cn_mesh_component_sizes")) || d->T == 0) return rc;
    component_sizes_kernel<<<(d->T + 255) / 256, 256, 0, st>>>(clean_args(d, CleanPlan{}));
    return check_launch("cn_mesh_component_sizes");
}

extern "C" size_t cn_mesh_clean_workspace_bytes(int32_t V, int32_t T) {
    if (V < 0 || T < 0) return 0;
    return clean_plan(V, T, nullptr).bytes;
}

extern "C" int cn_mesh_select(const cn_mesh_clean_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int rc = clean_ws_check("cn_mesh_select", d, workspace, workspace_bytes);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const CleanPlan p = clean_plan(d->V, d->T, workspace);
    const CleanArgs a = clean_args(d, p);
    best_clear_kernel<<<1, 1, 0, st>>>(p.best);
    if ((rc = check_launch("cn_mesh_select"))) return rc;
    if (d->keep_largest && d->V > 0) {
        best_component_kernel<<<(d->V + 255) / 256, 256, 0, st>>>(a);
        if ((rc = check_launch("cn_mesh_select"))) return rc;
    }
    const int n = d->V > d->T ? d->V : d->T;
    if (n > 0) {
        select_flags_kernel<<<(n + 255) / 256, 256, 0, st>>>(a);
        if ((rc = check_launch("cn_mesh_select"))) return rc;
    }
    // (an empty list scans one empty tile: the counts are written as zeros)
    if ((rc = scan_launch<false>("cn_mesh_select", p.vflag, d->V, p.vt, p.vtot, p.voff, d->counts, st))) return rc;
    return scan_launch<false>("cn_mesh_select", p.tflag, d->T, p.tt, p.ttot, p.toff, d->counts + 1, st);
}

extern "C" int cn_mesh_select_mask(const cn_mesh_clean_desc* d, const uint8_t* vmask, void* workspace, int64_t workspace_bytes,
                                   cn_stream_t stream) {
    int rc = clean_check("cn_mesh_select_mask", d, false);
    if (rc) return rc;
    CN_REQUIRE(d->V == 0 || vmask, CN_ERR_ARG, "cn_mesh_select_mask: null vmask");
    CN_REQUIRE(d->counts, CN_ERR_ARG, "cn_mesh_select_mask: null counts");
    CN_REQUIRE(((uintptr_t)d->counts & 7) == 0, CN_ERR_ALIGN, "cn_mesh_select_mask: counts 8-byte aligned");
    const size_t need = clean_plan(d->V, d->T, nullptr).bytes;
    CN_REQUIRE(workspace && workspace_bytes >= 0 && (size_t)workspace_bytes >= need, CN_ERR_SHAPE,
               "cn_mesh_select_mask: workspace %lld bytes, %zu needed", (long long)workspace_bytes, need);
    CN_REQUIRE(((uintptr_t)workspace & (kAlign - 1)) == 0, CN_ERR_ALIGN, "cn_mesh_select_mask: workspace not 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const CleanPlan p = clean_plan(d->V, d->T, workspace);
    const int n = d->V > d->T ? d->V : d->T;
    if (n > 0) {
        select_mask_flags_kernel<<<(n + 255) / 256, 256, 0, st>>>(clean_args(d, p), vmask);
        if ((rc = check_launch("cn_mesh_select_mask"))) return rc;
    }
    if ((rc = scan_launch<false>("cn_mesh_select_mask", p.vflag, d->V, p.vt, p.vtot, p.voff, d->counts, st))) return rc;
    return scan_launch<false>("cn_mesh_select_mask", p.tflag, d->T, p.tt, p.ttot, p.toff, d->counts + 1, st);
}

extern "C" int cn_mesh_compact(const cn_mesh_clean_desc* d, void* workspace, int64_t workspace_bytes, cn_stream_t stream) {
    int rc = clean_ws_check("cn_mesh_compact", d, workspace, workspace_bytes);
    if (rc) return rc;
    CN_REQUIRE(d->max_vertices >= 0 && d->max_triangles >= 0, CN_ERR_SHAPE, "cn_mesh_compact: max_vertices %lld / max_triangles %lld",
               (long long)d->max_vertices, (long long)d->max_triangles);
    CN_REQUIRE((d->max_vertices == 0 || d->kept_vertices) && (d->max_triangles == 0 || d->triangles_out), CN_ERR_ARG,
               "cn_mesh_compact: null kept_vertices / triangles_out");
    CN_REQUIRE(((uintptr_t)d->kept_vertices & 3) == 0 && ((uintptr_t)d->triangles_out & 3) == 0, CN_ERR_ALIGN,
               "cn_mesh_compact: kept_vertices / triangles_out 4-byte aligned");
    const int n = d->V > d->T ? d->V : d->T;
    if (n == 0) return CN_OK;
    compact_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(clean_args(d, clean_plan(d->V, d->T, workspace)));
    return check_launch("cn_mesh_compact");
}
