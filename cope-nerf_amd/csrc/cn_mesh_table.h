// cn_mesh_table.h — the marching-tetrahedra case table of the six-tetrahedron Kuhn split, generated at
// compile time from its two-line rule (DESIGN.md "Mesh extraction"); nothing here is typed by hand.
//
// Tetrahedron k of a cell belongs to the k-th permutation π of the axes (x, y, z) in lexicographic order;
// its corners are v0 = (0,0,0), v1 = v0 + e_π0, v2 = v1 + e_π1, v3 = (1,1,1), as cube-corner codes
// x + 2 y + 4 z.  Bit i of a mask is "corner i is inside".  With A the smaller of the inside / outside
// sets (the inside set on a 2 : 2 split) and B the other, both ascending:
//   A = {i},   B = {j,k,l}: (E_ij, E_ik, E_il)
//   A = {i,j}, B = {k,l}:   (E_ik, E_il, E_jl) and (E_ik, E_jl, E_jk)
// and a triangle's second and third index are swapped where, with every crossing at its edge's midpoint,
// its normal has a negative dot product with (centroid of the outside corners - centroid of the inside
// corners): normals point toward larger values.  The orientation depends on (k, mask) only.
//
// Entry layout (uint32): bits 0-1 the triangle count; triangle t in bits 4 + 12 t .. 15 + 12 t as three
// 4-bit edges (a | b << 2), a < b the tetrahedron-local corners of the edge's ends.  Along the Kuhn path
// a < b means corner a is component-wise below corner b, so the edge runs from a to b.
#pragma once

#include <cstdint>

namespace cn {

struct TetTable {
    uint32_t corner[6];   // the four cube-corner codes of tetrahedron k, 3 bits each (corner i in bits 3i ..)
    uint32_t entry[6 * 16];
};

constexpr int kTetPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

constexpr TetTable make_tet_table() {
    TetTable t{};
    for (int k = 0; k < 6; ++k) {
        int code[4] = {0, 1 << kTetPerm[k][0], (1 << kTetPerm[k][0]) | (1 << kTetPerm[k][1]), 7};
        t.corner[k] = (uint32_t)(code[0] | code[1] << 3 | code[2] << 6 | code[3] << 9);
        // corner coordinates, doubled so that edge midpoints are integers
        int P[4][3] = {};
        for (int i = 0; i < 4; ++i)
            for (int a = 0; a < 3; ++a) P[i][a] = 2 * ((code[i] >> a) & 1);
        for (int mask = 1; mask < 15; ++mask) {
            int in[4] = {}, out[4] = {}, nin = 0, nout = 0;
            for (int i = 0; i < 4; ++i) {
                if (mask >> i & 1) in[nin++] = i;
                else out[nout++] = i;
            }
            const bool a_in = nin <= 2;
            const int* A = a_in ? in : out;
            const int* B = a_in ? out : in;
            const int na = a_in ? nin : nout;
            int tri[2][3][2] = {};
            int ntri = 0;
            if (na == 1) {
                ntri = 1;
                for (int e = 0; e < 3; ++e) {
                    tri[0][e][0] = A[0];
                    tri[0][e][1] = B[e];
                }
            } else {
                ntri = 2;
                const int i = A[0], j = A[1], kk = B[0], l = B[1];
                const int q[2][3][2] = {{{i, kk}, {i, l}, {j, l}}, {{i, kk}, {j, l}, {j, kk}}};
                for (int tt = 0; tt < 2; ++tt)
                    for (int e = 0; e < 3; ++e) {
                        tri[tt][e][0] = q[tt][e][0];
                        tri[tt][e][1] = q[tt][e][1];
                    }
            }
            // nin * nout * (centroid of the outside corners - centroid of the inside corners)
            int dir[3] = {};
            for (int a = 0; a < 3; ++a) {
                int so = 0, si = 0;
                for (int i = 0; i < nout; ++i) so += P[out[i]][a];
                for (int i = 0; i < nin; ++i) si += P[in[i]][a];
                dir[a] = nin * so - nout * si;
            }
            uint32_t e32 = (uint32_t)ntri;
            for (int tt = 0; tt < ntri; ++tt) {
                int m[3][3] = {};  // the midpoints, doubled
                for (int e = 0; e < 3; ++e)
                    for (int a = 0; a < 3; ++a) m[e][a] = (P[tri[tt][e][0]][a] + P[tri[tt][e][1]][a]) / 2;
                int u[3] = {}, v[3] = {};
                for (int a = 0; a < 3; ++a) {
                    u[a] = m[1][a] - m[0][a];
                    v[a] = m[2][a] - m[0][a];
                }
                const int n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
                const int dot = n[0] * dir[0] + n[1] * dir[1] + n[2] * dir[2];
                const int order[3] = {0, dot < 0 ? 2 : 1, dot < 0 ? 1 : 2};
                for (int e = 0; e < 3; ++e) {
                    int a = tri[tt][order[e]][0], b = tri[tt][order[e]][1];
                    if (a > b) {
                        const int s = a;
                        a = b;
                        b = s;
                    }
                    e32 |= (uint32_t)(a | b << 2) << (4 + 12 * tt + 4 * e);
                }
            }
            t.entry[k * 16 + mask] = e32;
        }
    }
    return t;
}

}  // namespace cn
