// drt_hull.h -- the visual hull of a capture's silhouette masks ("the visual hull"): the silhouette field of one
// grid corner, and marching tetrahedra on the Kuhn subdivision of a cell.  Plain C++ like the other device math headers, so that
// tests/hostsim/hull.cpp runs the same bodies on the host against the numpy restatement (tests/hull_ref.py) with tolerance 0: every
// float64 expression below is one rounding per operation in the stated association (the library is built with -ffp-contract=off).
#pragma once
#include "drt_common.h"

namespace drt {

struct HullGrid {
    double lo[3];       // position of corner (0, 0, 0)
    double h;           // cell size
    int nx, ny, nz;     // corner counts; corner (i, j, k) has the linear index (i * ny + j) * nz + k
};

constexpr double kHullSMin = 1.0 / 1024.0;     // s of a crossing is clamped to [2^-10, 1 - 2^-10]: no two vertices coincide

DRT_HD int64_t hull_corners(const HullGrid& g) { return (int64_t)g.nx * g.ny * g.nz; }
DRT_HD double hull_coord(const HullGrid& g, int axis, int i) { return g.lo[axis] + g.h * (double)i; }
DRT_HD bool hull_on_boundary(const HullGrid& g, int i, int j, int k) {
    return i == 0 || j == 0 || k == 0 || i == g.nx - 1 || j == g.ny - 1 || k == g.nz - 1;
}

// One view: does it see the point, and the bilinear sample of its mask there.  P = K R[:3, :] row-major [3][4]; pixel centres at integer
// coordinates (views.generate_ray); a nonzero byte is 1.0.  A NaN or infinite projection fails the comparisons: not seen.
DRT_HD bool hull_view_sample(const double* __restrict__ P, const uint8_t* __restrict__ mask, int H, int W, double x, double y, double z, double& val) {
    const double hx = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const double hy = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const double hz = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    if (!(hz > 0.0)) return false;
    const double u = hx / hz, w = hy / hz;
    if (!(u >= 0.0 && u <= (double)(W - 1) && w >= 0.0 && w <= (double)(H - 1))) return false;
    double x0 = floor(u), y0 = floor(w);
    if (x0 > (double)(W - 2)) x0 = (double)(W - 2);
    if (y0 > (double)(H - 2)) y0 = (double)(H - 2);
    const double fx = u - x0, fy = w - y0;
    const uint8_t* row = mask + (int64_t)y0 * W + (int64_t)x0;       // 0 <= x0 <= W - 2, 0 <= y0 <= H - 2: all four reads inside the image
    const double m00 = row[0] ? 1.0 : 0.0, m01 = row[1] ? 1.0 : 0.0, m10 = row[W] ? 1.0 : 0.0, m11 = row[W + 1] ? 1.0 : 0.0;
    val = ((m00 * (1.0 - fx) + m01 * fx) * (1.0 - fy)) + ((m10 * (1.0 - fx) + m11 * fx) * fy);
    return true;
}

// The running minimum of one corner over the views, in order.  m starts at +infinity ("no view has contributed").  A view that does not
// see the corner contributes 0 (carve) or nothing (keep).  Once m is 0 no later view can change it.
DRT_HD void hull_accumulate(double& m, const double* __restrict__ P, const uint8_t* __restrict__ mask, int H, int W, double x, double y, double z, bool keep) {
    double val;
    if (hull_view_sample(P, mask, H, W, x, y, z, val)) m = val < m ? val : m;
    else if (!keep) m = 0.0;
}
DRT_HD float hull_finish(double m) { return m == INFINITY ? 0.0f : (float)m; }

// The whole field value of corner (i, j, k): what k_hull_field computes with the view loop spread over LDS chunks.
DRT_HD float hull_corner_field(const HullGrid& g, int i, int j, int k, const uint8_t* __restrict__ masks, int n_views, int H, int W,
                               const double* __restrict__ P, bool keep) {
    if (hull_on_boundary(g, i, j, k)) return 0.0f;          // the surface closes inside the grid
    const double x = hull_coord(g, 0, i), y = hull_coord(g, 1, j), z = hull_coord(g, 2, k);
    double m = INFINITY;
    for (int v = 0; v < n_views && m > 0.0; ++v) hull_accumulate(m, P + 12 * v, masks + (int64_t)v * H * W, H, W, x, y, z, keep);
    return hull_finish(m);
}

// ---- marching tetrahedra on the Kuhn subdivision ---------------------------------------------------------------------------------
// Offsets inside a cell are coded 4 dx + 2 dy + dz.  Tetrahedron t belongs to the t-th permutation (a, b, c) of the axes in
// lexicographic order; its vertices are c0, c0 + e_a, c0 + e_a + e_b, c0 + (1, 1, 1): a chain of codes, each a superset of the one before,
// so the edge of tetrahedron vertices p < q is the lattice edge (corner + code[p], offset code[q] ^ code[p]).
struct HullTet { uint8_t code[4]; uint8_t odd; };
constexpr HullTet kHullTets[6] = {
    {{0, 4, 6, 7}, 0},      // x y z
    {{0, 4, 5, 7}, 1},      // x z y
    {{0, 2, 6, 7}, 1},      // y x z
    {{0, 2, 3, 7}, 0},      // y z x
    {{0, 1, 5, 7}, 0},      // z x y
    {{0, 1, 3, 7}, 1},      // z y x
};
// Case = bit p set when tetrahedron vertex p is inside.  Edges as (p << 2) | q, three per triangle, for an EVEN permutation with the
// normal pointing from inside to outside; an odd permutation is the mirror image: swap the last two vertices of every triangle.
// One inside vertex p: its three edges by increasing q; three inside: the same around the outside vertex; two inside {a, b}, two outside
// {c, d}: the quad (ac, ad, bd, bc) as (ac, ad, bd), (ac, bd, bc).
struct HullCase { uint8_t n; uint8_t edge[6]; };
constexpr HullCase kHullCases[16] = {
    {0, {0x0, 0x0, 0x0, 0x0, 0x0, 0x0}},
    {1, {0x1, 0x2, 0x3, 0x0, 0x0, 0x0}},
    {1, {0x1, 0x7, 0x6, 0x0, 0x0, 0x0}},
    {2, {0x2, 0x3, 0x7, 0x2, 0x7, 0x6}},
    {1, {0x2, 0x6, 0xb, 0x0, 0x0, 0x0}},
    {2, {0x1, 0xb, 0x3, 0x1, 0x6, 0xb}},
    {2, {0x1, 0x7, 0xb, 0x1, 0xb, 0x2}},
    {1, {0x3, 0x7, 0xb, 0x0, 0x0, 0x0}},
    {1, {0x3, 0xb, 0x7, 0x0, 0x0, 0x0}},
    {2, {0x1, 0x2, 0xb, 0x1, 0xb, 0x7}},
    {2, {0x1, 0xb, 0x6, 0x1, 0x3, 0xb}},
    {1, {0x2, 0xb, 0x6, 0x0, 0x0, 0x0}},
    {2, {0x2, 0x6, 0x7, 0x2, 0x7, 0x3}},
    {1, {0x1, 0x6, 0x7, 0x0, 0x0, 0x0}},
    {1, {0x1, 0x3, 0x2, 0x0, 0x0, 0x0}},
    {0, {0x0, 0x0, 0x0, 0x0, 0x0, 0x0}},
};

DRT_HD bool hull_inside(float f, float level) { return f > level; }          // a corner exactly on the level is outside
DRT_HD int64_t hull_step(const HullGrid& g, int code) {
    return (int64_t)((code >> 2) & 1) * g.ny * g.nz + (int64_t)((code >> 1) & 1) * g.nz + (code & 1);
}
DRT_HD int hull_popcount8(unsigned m) {
    m = (m & 0x55u) + ((m >> 1) & 0x55u);
    m = (m & 0x33u) + ((m >> 2) & 0x33u);
    return (int)((m + (m >> 4)) & 0x0fu);
}

// Inside flags of the eight corners of the cell that starts at (i, j, k), bit = offset code.  The cell must exist (i < nx - 1, ...).
DRT_HD unsigned hull_cell_bits(const HullGrid& g, const float* __restrict__ field, int64_t lin, float level) {
    unsigned bits = 0;
    for (int c = 0; c < 8; ++c) bits |= (unsigned)hull_inside(field[lin + hull_step(g, c)], level) << c;
    return bits;
}
DRT_HD int hull_tet_case(unsigned cell_bits, int t) {
    const HullTet& T = kHullTets[t];
    return (int)(((cell_bits >> T.code[0]) & 1u) | (((cell_bits >> T.code[1]) & 1u) << 1) | (((cell_bits >> T.code[2]) & 1u) << 2) |
                 (((cell_bits >> T.code[3]) & 1u) << 3));
}
DRT_HD int hull_cell_triangles(unsigned cell_bits) {
    if (cell_bits == 0u || cell_bits == 0xffu) return 0;
    int n = 0;
    for (int t = 0; t < 6; ++t) n += kHullCases[hull_tet_case(cell_bits, t)].n;
    return n;
}

// What k_hull_mark stores for a corner: bit (code - 1) of the edge mask is set when the lattice edge (corner, code) lies in the grid and
// changes sign -- the corner owns one vertex per set bit, numbered by ascending code -- and the triangle count of the cell that starts here.
DRT_HD void hull_mark_corner(const HullGrid& g, const float* __restrict__ field, int i, int j, int k, float level, unsigned& edge_mask, int& n_tri) {
    const int64_t lin = ((int64_t)i * g.ny + j) * g.nz + k;
    const bool here = hull_inside(field[lin], level);
    edge_mask = 0;
    for (int code = 1; code < 8; ++code) {
        if (i + ((code >> 2) & 1) >= g.nx || j + ((code >> 1) & 1) >= g.ny || k + (code & 1) >= g.nz) continue;
        if (hull_inside(field[lin + hull_step(g, code)], level) != here) edge_mask |= 1u << (code - 1);
    }
    n_tri = (i < g.nx - 1 && j < g.ny - 1 && k < g.nz - 1) ? hull_cell_triangles(hull_cell_bits(g, field, lin, level)) : 0;
}

// The vertex on the lattice edge (corner (i, j, k), code): lo + h ((i, j, k) + s off), s = (level - fa) / (fb - fa) in float64 from the
// two float32 values (fa at the lower corner), clamped.
DRT_HD void hull_edge_vertex(const HullGrid& g, const float* __restrict__ field, int i, int j, int k, int code, float level, double out[3]) {
    const int64_t lin = ((int64_t)i * g.ny + j) * g.nz + k;
    const double fa = (double)field[lin], fb = (double)field[lin + hull_step(g, code)];
    double s = ((double)level - fa) / (fb - fa);
    s = s < kHullSMin ? kHullSMin : s;
    s = s > 1.0 - kHullSMin ? 1.0 - kHullSMin : s;
    out[0] = g.lo[0] + g.h * ((double)i + s * (double)((code >> 2) & 1));
    out[1] = g.lo[1] + g.h * ((double)j + s * (double)((code >> 1) & 1));
    out[2] = g.lo[2] + g.h * ((double)k + s * (double)(code & 1));
}

// Index of the vertex on the lattice edge (corner lin, code): vertices are numbered by ascending (corner, code), so it is the number of
// vertices of all earlier corners plus the set bits below this one.  v_inc = INCLUSIVE prefix sum of the per-corner vertex counts.
DRT_HD int32_t hull_vertex_index(const uint8_t* __restrict__ edge_mask, const int32_t* __restrict__ v_inc, int64_t lin, int code) {
    const int32_t base = lin > 0 ? v_inc[lin - 1] : 0;
    return base + hull_popcount8(edge_mask[lin] & ((1u << (code - 1)) - 1u));
}

// Triangles of the cell that starts at corner lin, by tetrahedron and then in table order, written to faces[3 * first ...]; returns how many.
// Nothing is written at or beyond n_faces.
DRT_HD int hull_emit_cell(const HullGrid& g, unsigned cell_bits, int64_t lin, const uint8_t* __restrict__ edge_mask, const int32_t* __restrict__ v_inc,
                          int64_t first, int64_t n_faces, int32_t* __restrict__ faces) {
    int n = 0;
    for (int t = 0; t < 6; ++t) {
        const HullTet& T = kHullTets[t];
        const HullCase& C = kHullCases[hull_tet_case(cell_bits, t)];
        for (int r = 0; r < C.n; ++r) {
            int32_t v[3];
            for (int e = 0; e < 3; ++e) {
                const int p = C.edge[3 * r + e] >> 2, q = C.edge[3 * r + e] & 3;
                v[e] = hull_vertex_index(edge_mask, v_inc, lin + hull_step(g, T.code[p]), T.code[q] ^ T.code[p]);
            }
            const int64_t row = first + n;
            if (row < n_faces) {
                faces[3 * row] = v[0];
                faces[3 * row + 1] = T.odd ? v[2] : v[1];
                faces[3 * row + 2] = T.odd ? v[1] : v[2];
            }
            ++n;
        }
    }
    return n;
}

}  // namespace drt
