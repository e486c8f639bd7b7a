// tests/hostsim/hull.cpp -- drt_amd/csrc/drt_hull.h compiled for the host (g++ -ffp-contract=off): the per-corner and per-cell bodies of
// k_hull_field / k_hull_mark / k_hull_emit run over a whole grid in plain loops, with the two prefix sums between them.  Test-only.
#include "../../drt_amd/csrc/drt_hull.h"

using namespace drt;

namespace {
HullGrid grid(const double* lo3, double h, const int* dims) { return HullGrid{{lo3[0], lo3[1], lo3[2]}, h, dims[0], dims[1], dims[2]}; }
}  // namespace

extern "C" {

void hull_field(const uint8_t* masks, int n_views, int H, int W, const double* P, const double* lo3, double h, const int* dims, int keep, float* field) {
    const HullGrid g = grid(lo3, h, dims);
    for (int i = 0; i < g.nx; ++i)
        for (int j = 0; j < g.ny; ++j)
            for (int k = 0; k < g.nz; ++k)
                field[((int64_t)i * g.ny + j) * g.nz + k] = hull_corner_field(g, i, j, k, masks, n_views, H, W, P, keep != 0);
}

// edge_mask uint8 [N], v_inc / t_inc int32 [N] (inclusive sums); totals[0] = vertices, totals[1] = triangles
void hull_mark(const float* field, const int* dims, float level, uint8_t* edge_mask, int32_t* v_inc, int32_t* t_inc, int64_t* totals) {
    const double lo3[3] = {0.0, 0.0, 0.0};
    const HullGrid g = grid(lo3, 1.0, dims);
    int32_t nv = 0, nt = 0;
    for (int i = 0; i < g.nx; ++i)
        for (int j = 0; j < g.ny; ++j)
            for (int k = 0; k < g.nz; ++k) {
                const int64_t lin = ((int64_t)i * g.ny + j) * g.nz + k;
                unsigned em;
                int n;
                hull_mark_corner(g, field, i, j, k, level, em, n);
                edge_mask[lin] = (uint8_t)em;
                nv += hull_popcount8(em);
                nt += n;
                v_inc[lin] = nv;
                t_inc[lin] = nt;
            }
    totals[0] = nv;
    totals[1] = nt;
}

void hull_emit(const float* field, const int* dims, const double* lo3, double h, float level, const uint8_t* edge_mask, const int32_t* v_inc,
               const int32_t* t_inc, int64_t n_verts, int64_t n_faces, double* verts, int32_t* faces) {
    const HullGrid g = grid(lo3, h, dims);
    for (int i = 0; i < g.nx; ++i)
        for (int j = 0; j < g.ny; ++j)
            for (int k = 0; k < g.nz; ++k) {
                const int64_t lin = ((int64_t)i * g.ny + j) * g.nz + k;
                int64_t row = lin > 0 ? v_inc[lin - 1] : 0;
                for (int code = 1; code < 8; ++code)
                    if ((edge_mask[lin] >> (code - 1)) & 1) {
                        if (row < n_verts) hull_edge_vertex(g, field, i, j, k, code, level, verts + 3 * row);
                        ++row;
                    }
                if (i >= g.nx - 1 || j >= g.ny - 1 || k >= g.nz - 1) continue;
                const int64_t first = lin > 0 ? t_inc[lin - 1] : 0;
                if (t_inc[lin] != first) hull_emit_cell(g, hull_cell_bits(g, field, lin, level), lin, edge_mask, v_inc, first, n_faces, faces);
            }
}

}  // extern "C"
