// drt_hull.hip -- the visual hull of a capture's silhouette masks on the device (drt_hull.h holds the law): the silhouette field of a
// dense corner grid, the per-corner edge masks and triangle counts, and -- after two prefix sums on the caller's side -- the vertices
// and triangles of the marching-tetrahedra surface.  No sort and no atomics: the same inputs give the same bits.
#include "drt_device.h"
#include "drt_hull.h"

namespace {

constexpr int kHullBlock = 256;                  // four waves, one 4 x 4 x 4 brick of corners each
constexpr int kHullChunk = 64;                   // views whose 3 x 4 matrices are staged in LDS at a time (6 KB)
constexpr int kHullMaxDim = 1024;

// Brick b of the grid (bricks numbered with z fastest) and lane l of its wave -> the corner; false when it falls outside the grid.
__device__ __forceinline__ bool brick_corner(const HullGrid& g, int64_t brick, int lane, int& i, int& j, int& k) {
    const int by = (g.ny + 3) >> 2, bz = (g.nz + 3) >> 2;
    const int64_t bi = brick / ((int64_t)by * bz), rem = brick - bi * by * bz;
    i = (int)(bi << 2) + (lane >> 4);
    j = (int)((rem / bz) << 2) + ((lane >> 2) & 3);
    k = (int)((rem % bz) << 2) + (lane & 3);
    return i < g.nx && j < g.ny && k < g.nz;
}

}  // namespace

// One thread per corner.  The 64 lanes of a wave hold a 4 x 4 x 4 brick: their projections fall on neighbouring pixels of every view (the
// mask bytes of a wave come from a few cache lines) and bricks outside the silhouette of some view are at 0 in all lanes together, so the
// wave leaves the view loop.  The trip count over the LDS chunks is block-uniform (barriers); a finished wave only skips the work.
__global__ void __launch_bounds__(kHullBlock) k_hull_field(HullGrid g, int64_t n_bricks, const uint8_t* __restrict__ masks, int n_views, int H, int W,
                                                           const double* __restrict__ proj, int keep, float* __restrict__ field) {
    __shared__ double s_proj[kHullChunk * 12];
    const int lane = threadIdx.x & 63;
    const int64_t brick = (int64_t)blockIdx.x * (kHullBlock / 64) + (threadIdx.x >> 6);
    int i = 0, j = 0, k = 0;
    const bool in_grid = brick < n_bricks && brick_corner(g, brick, lane, i, j, k);
    const bool live = in_grid && !hull_on_boundary(g, i, j, k);
    const double x = hull_coord(g, 0, i), y = hull_coord(g, 1, j), z = hull_coord(g, 2, k);
    double m = live ? INFINITY : 0.0;
    bool wave_done = __ballot(m > 0.0) == 0ull;
    const int64_t image = (int64_t)H * W;
    for (int v0 = 0; v0 < n_views; v0 += kHullChunk) {
        const int nv = n_views - v0 < kHullChunk ? n_views - v0 : kHullChunk;
        __syncthreads();                                           // the previous chunk has been read by every wave
        for (int e = threadIdx.x; e < 12 * nv; e += kHullBlock) s_proj[e] = proj[(int64_t)12 * v0 + e];
        __syncthreads();
        if (wave_done) continue;
        for (int v = 0; v < nv; ++v) {
            if (m > 0.0) hull_accumulate(m, s_proj + 12 * v, masks + (v0 + v) * image, H, W, x, y, z, keep != 0);
            if (__ballot(m > 0.0) == 0ull) { wave_done = true; break; }
        }
    }
    if (in_grid) field[((int64_t)i * g.ny + j) * g.nz + k] = hull_finish(m);
}

__global__ void __launch_bounds__(kHullBlock) k_hull_mark(HullGrid g, const float* __restrict__ field, float level, uint8_t* __restrict__ edge_mask,
                                                          uint8_t* __restrict__ n_vert, uint8_t* __restrict__ n_tri) {
    const int64_t lin = (int64_t)blockIdx.x * kHullBlock + threadIdx.x;
    if (lin >= hull_corners(g)) return;
    const int k = (int)(lin % g.nz), j = (int)((lin / g.nz) % g.ny), i = (int)(lin / ((int64_t)g.nz * g.ny));
    unsigned em;
    int nt;
    hull_mark_corner(g, field, i, j, k, level, em, nt);
    edge_mask[lin] = (uint8_t)em;
    n_vert[lin] = (uint8_t)hull_popcount8(em);
    n_tri[lin] = (uint8_t)nt;
}

// v_inc / t_inc: inclusive prefix sums of k_hull_mark's two counts.  A corner writes the vertices of its own edges and the triangles of
// the cell that starts at it, at the places the sums give: the output order is the law's, whatever order the threads run in.
__global__ void __launch_bounds__(kHullBlock) k_hull_emit(HullGrid g, const float* __restrict__ field, float level, const uint8_t* __restrict__ edge_mask,
                                                          const int32_t* __restrict__ v_inc, const int32_t* __restrict__ t_inc, int64_t n_verts,
                                                          int64_t n_faces, double* __restrict__ verts, int32_t* __restrict__ faces) {
    const int64_t lin = (int64_t)blockIdx.x * kHullBlock + threadIdx.x;
    if (lin >= hull_corners(g)) return;
    const int k = (int)(lin % g.nz), j = (int)((lin / g.nz) % g.ny), i = (int)(lin / ((int64_t)g.nz * g.ny));
    const unsigned em = edge_mask[lin];
    if (em) {
        int64_t row = lin > 0 ? v_inc[lin - 1] : 0;
        for (int code = 1; code < 8; ++code) {
            if (!((em >> (code - 1)) & 1u)) continue;
            if (row >= 0 && row < n_verts) {                      // (sums that disagree with the masks never write outside the output)
                double p[3];
                hull_edge_vertex(g, field, i, j, k, code, level, p);
                verts[3 * row] = p[0]; verts[3 * row + 1] = p[1]; verts[3 * row + 2] = p[2];
            }
            ++row;
        }
    }
    if (i >= g.nx - 1 || j >= g.ny - 1 || k >= g.nz - 1) return;
    const int64_t first = lin > 0 ? t_inc[lin - 1] : 0;
    if (t_inc[lin] == first || first < 0) return;                                  // no triangle in this cell
    hull_emit_cell(g, hull_cell_bits(g, field, lin, level), lin, edge_mask, v_inc, first, n_faces, faces);
}

namespace {

int check_grid(double lo_x, double lo_y, double lo_z, double cell, int nx, int ny, int nz, HullGrid& g) {
    if (nx < 3 || nx > kHullMaxDim) return fail(DRT_E_INVALID, "nx = %d: corner counts must be in [3, %d]", nx, kHullMaxDim);
    if (ny < 3 || ny > kHullMaxDim) return fail(DRT_E_INVALID, "ny = %d: corner counts must be in [3, %d]", ny, kHullMaxDim);
    if (nz < 3 || nz > kHullMaxDim) return fail(DRT_E_INVALID, "nz = %d: corner counts must be in [3, %d]", nz, kHullMaxDim);
    if (!(cell > 0.0) || !std::isfinite(cell)) return fail(DRT_E_INVALID, "cell = %g: the cell size must be positive and finite", cell);
    if (!std::isfinite(lo_x) || !std::isfinite(lo_y) || !std::isfinite(lo_z)) return fail(DRT_E_INVALID, "lo: the grid origin must be finite");
    g = HullGrid{{lo_x, lo_y, lo_z}, cell, nx, ny, nz};
    return DRT_OK;
}

int check_level(double level) {
    if (!(level > 0.0 && level < 1.0) || !((float)level > 0.0f && (float)level < 1.0f)) return fail(DRT_E_INVALID, "level = %g: must be inside (0, 1)", level);
    return DRT_OK;
}

}  // namespace

extern "C" {

int drt_hull_field(const uint8_t* d_masks, int n_views, int height, int width, const double* d_proj, double lo_x, double lo_y, double lo_z,
                   double cell, int nx, int ny, int nz, int keep_outside, float* d_field, void* stream) {
    HullGrid g;
    { int rc = check_grid(lo_x, lo_y, lo_z, cell, nx, ny, nz, g); if (rc) return rc; }
    if (n_views < 1) return fail(DRT_E_INVALID, "n_views = %d: at least one view is needed", n_views);
    if (height < 2 || width < 2) return fail(DRT_E_INVALID, "height x width = %d x %d: masks must be at least 2 x 2", height, width);
    if (keep_outside != 0 && keep_outside != 1) return fail(DRT_E_INVALID, "keep_outside = %d: 0 (carve) or 1 (keep)", keep_outside);
    if (!d_masks) return fail(DRT_E_INVALID, "d_masks is null");
    if (!d_proj) return fail(DRT_E_INVALID, "d_proj is null");
    if (!d_field) return fail(DRT_E_INVALID, "d_field is null");
    const int64_t n_bricks = (int64_t)((nx + 3) >> 2) * ((ny + 3) >> 2) * ((nz + 3) >> 2);
    const int64_t blocks = (n_bricks + kHullBlock / 64 - 1) / (kHullBlock / 64);
    k_hull_field<<<(unsigned)blocks, kHullBlock, 0, (hipStream_t)stream>>>(g, n_bricks, d_masks, n_views, height, width, d_proj, keep_outside, d_field);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

int drt_hull_mark(const float* d_field, int nx, int ny, int nz, double level, uint8_t* d_edge_mask, uint8_t* d_n_vert, uint8_t* d_n_tri, void* stream) {
    HullGrid g;
    { int rc = check_grid(0.0, 0.0, 0.0, 1.0, nx, ny, nz, g); if (rc) return rc; }
    { int rc = check_level(level); if (rc) return rc; }
    if (!d_field) return fail(DRT_E_INVALID, "d_field is null");
    if (!d_edge_mask) return fail(DRT_E_INVALID, "d_edge_mask is null");
    if (!d_n_vert) return fail(DRT_E_INVALID, "d_n_vert is null");
    if (!d_n_tri) return fail(DRT_E_INVALID, "d_n_tri is null");
    k_hull_mark<<<(unsigned)((hull_corners(g) + kHullBlock - 1) / kHullBlock), kHullBlock, 0, (hipStream_t)stream>>>(g, d_field, (float)level, d_edge_mask,
                                                                                                                    d_n_vert, d_n_tri);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

int drt_hull_emit(const float* d_field, int nx, int ny, int nz, double lo_x, double lo_y, double lo_z, double cell, double level,
                  const uint8_t* d_edge_mask, const int32_t* d_v_inc, const int32_t* d_t_inc, int64_t n_verts, int64_t n_faces,
                  double* d_verts, int32_t* d_faces, void* stream) {
    HullGrid g;
    { int rc = check_grid(lo_x, lo_y, lo_z, cell, nx, ny, nz, g); if (rc) return rc; }
    { int rc = check_level(level); if (rc) return rc; }
    if (n_verts < 0 || n_verts > INT32_MAX) return fail(DRT_E_INVALID, "n_verts = %lld: must be in [0, 2^31)", (long long)n_verts);
    if (n_faces < 0 || n_faces > INT32_MAX) return fail(DRT_E_INVALID, "n_faces = %lld: must be in [0, 2^31)", (long long)n_faces);
    if (!d_field) return fail(DRT_E_INVALID, "d_field is null");
    if (!d_edge_mask) return fail(DRT_E_INVALID, "d_edge_mask is null");
    if (!d_v_inc) return fail(DRT_E_INVALID, "d_v_inc is null");
    if (!d_t_inc) return fail(DRT_E_INVALID, "d_t_inc is null");
    if (n_verts && !d_verts) return fail(DRT_E_INVALID, "d_verts is null");
    if (n_faces && !d_faces) return fail(DRT_E_INVALID, "d_faces is null");
    k_hull_emit<<<(unsigned)((hull_corners(g) + kHullBlock - 1) / kHullBlock), kHullBlock, 0, (hipStream_t)stream>>>(
        g, d_field, (float)level, d_edge_mask, d_v_inc, d_t_inc, n_verts, n_faces, d_verts, d_faces);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

}  // extern "C"
