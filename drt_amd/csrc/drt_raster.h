// drt_raster.h -- primary visibility of pinhole ray grids by projection instead of BVH traversal.
//
// The first traversal of Scene.render_transparent (reference DiffRender.py:537-540: `Dintersect` of the camera rays)
// answers, for every pixel of a view, "closest triangle along this ray".  When the rays of an image ARE a pinhole grid
// -- generate_ray, reference captured_data.py:23-40: origin = R^-1[:3,3] for every pixel, direction ~ M (x, y, 1)^T with
// M = R^-1[:3,:3] K^-1 -- the set of pixels whose ray can hit a triangle is the projection of that triangle, so each
// triangle is tested only against the handful of pixels of its projected bounding box, with the SAME float32
// ray/triangle test (drt_tri.h) on the SAME float32 ray the traversal would use, and the closest hit per pixel is kept
// by a 64-bit atomic minimum of (t bits, face id) -- i.e. the contract of oracle/tracer.c (minimum t, ties -> lowest
// face id) without walking a tree: ~3 tests per (view, triangle) instead of ~14 node visits per candidate ray.
//
// A caller that presents the SAME, unchanged ray tensors again (a capture's views are constants of the optimisation) can
// keep the verdict: a call in DRT_GRID_ESTABLISH mode records the fitted models and, per image, whether every single ray
// verified, in a caller-owned cache; later calls in DRT_GRID_TRUST mode then neither re-fit nor re-read the rays of
// pixels no projected triangle touches (nine out of ten): k_cull writes their zeros without loading anything.
//
// Nothing is assumed about the caller's rays: the model (origin, M^-1) of every image is FITTED on the device from four
// of its rays, every single ray is then VERIFIED against it in k_cull (origin bit-equal, pixel position within
// kRasterVerifyTol), and a ray that does not verify -- calibrated per-pixel rays of a real capture, arbitrary ray
// lists -- takes the BVH path as before.  Conservative by construction: the box is grown by kRasterPad = 1/16 pixel.  What
// it has to cover, in pixels of a 1024-wide image of a ~500 mm distant object: the float32 projection of the vertices
// (~2e-4), the distance a verified ray may be from its pixel centre (kRasterVerifyTol = 1e-3) and how far outside a
// triangle the float32 test can still accept a ray (rounding of dot(s, p) against the pixel pitch, ~3e-4) -- together
// ~1.5e-3 px, ~3e-3 px at 4096 wide: a factor 20-40 below the pad.  (It was 1/4 px at first: the boxes of 2-3 pixel
// triangles then held a third more pixel centres, all of them misses.)
#pragma once
#include "drt_common.h"
#include "drt_tri.h"

namespace drt {

struct ViewModel {
    double o[3];        // common origin of the image's rays
    double minv[9];     // (x, y, 1) ~ minv * direction, row-major
    int32_t ok;         // 1: pinhole grid; 0: take the BVH path for every ray of this image
    int32_t all;        // 1: EVERY ray of the image verified against the model (established by a call in DRT_GRID_ESTABLISH mode)
};

static_assert(sizeof(ViewModel) == 104, "DRT_GRID_CACHE_BYTES of include/drt_hip.h");

constexpr double kRasterPad = 0.0625;         // pixels added on every side of a projected triangle's bounding box
constexpr double kRasterVerifyTol = 1e-3;    // a ray belongs to the grid if its direction projects within this of its pixel
#ifndef DRT_RASTER_MAX_PER_LANE
#define DRT_RASTER_MAX_PER_LANE 48
#endif
constexpr int kRasterMaxPerLane = DRT_RASTER_MAX_PER_LANE;        // larger boxes are handed to k_raster_big (one wave per band of rows of the box)
constexpr int kRasterBandPixels = 1024;      // pixel centres per band (a band is at least one row)

// Solve the model from the rays of the four image corners (unit or not, only their directions matter):
// d(x, y) ~ x m0 + y m1 + m2.  Returns false when the corner directions are degenerate.
DRT_HD bool fit_view_model(d3 o, d3 d00, d3 dW0, d3 d0H, d3 dWH, double wm1, double hm1, ViewModel& vm) {
    // beta dW0 + gamma d0H - eps dWH = d00   (from (W-1) m0 = beta dW0 - d00, (H-1) m1 = gamma d0H - d00, m2 = d00)
    const d3 c0 = dW0, c1 = d0H, c2 = -dWH;
    const double det = dot(c0, cross(c1, c2));
    vm.ok = 0; vm.all = 0;
    vm.o[0] = o.x; vm.o[1] = o.y; vm.o[2] = o.z;
    for (int k = 0; k < 9; ++k) vm.minv[k] = 0.0;
    if (!(fabs(det) > 1e-300) || !(wm1 > 0.0) || !(hm1 > 0.0)) return false;
    const double beta = dot(d00, cross(c1, c2)) / det, gamma = dot(c0, cross(d00, c2)) / det;
    const d3 m0 = (beta * dW0 - d00) / wm1, m1 = (gamma * d0H - d00) / hm1, m2 = d00;
    // inverse of M = [m0 m1 m2] (columns): rows of M^-1 are cross products / det(M)
    const double dm = dot(m0, cross(m1, m2));
    if (!(fabs(dm) > 1e-300)) return false;
    const d3 r0 = cross(m1, m2) / dm, r1 = cross(m2, m0) / dm, r2 = cross(m0, m1) / dm;
    vm.minv[0] = r0.x; vm.minv[1] = r0.y; vm.minv[2] = r0.z;
    vm.minv[3] = r1.x; vm.minv[4] = r1.y; vm.minv[5] = r1.z;
    vm.minv[6] = r2.x; vm.minv[7] = r2.y; vm.minv[8] = r2.z;
    bool fin = true;
    for (int k = 0; k < 9; ++k) fin = fin && (fabs(vm.minv[k]) < 1e300);
    return fin;
}

// (px, py, pz) = minv * v: the pixel position is (px / pz, py / pz), pz > 0 in front of the camera.
DRT_HD d3 view_project(const ViewModel& vm, d3 v) {
    return d3{(vm.minv[0] * v.x + vm.minv[1] * v.y) + vm.minv[2] * v.z,
              (vm.minv[3] * v.x + vm.minv[4] * v.y) + vm.minv[5] * v.z,
              (vm.minv[6] * v.x + vm.minv[7] * v.y) + vm.minv[8] * v.z};
}

// Is (o, d) the ray of pixel (x, y) of this image?
DRT_HD bool view_verify(const ViewModel& vm, d3 o, d3 d, double x, double y) {
    if (!(o.x == vm.o[0] && o.y == vm.o[1] && o.z == vm.o[2])) return false;
    const d3 p = view_project(vm, d);
    if (!(p.z > 0.0)) return false;
    return fabs(p.x - x * p.z) <= kRasterVerifyTol * p.z && fabs(p.y - y * p.z) <= kRasterVerifyTol * p.z;
}

struct PixelBox {
    int x0, x1, y0, y1;     // inclusive; empty when x0 > x1 or y0 > y1
    bool unsafe;            // a vertex at or behind the camera plane (or a non-finite projection): no projection bound
};

// Padded pixel bounding box of the triangle record `t` seen from the image's origin, in float32 (|error| ~1e-4 px at these
// magnitudes; the pad is 1/16 px).  Used by k_raster and by the host-side unit test alike.
DRT_HD PixelBox project_tri_box(const ViewModel& vm, f3 o32, const TriRec& t, int w, int h) {
    PixelBox r{0, -1, 0, -1, false};
    const f3 a{t.v0x - o32.x, t.v0y - o32.y, t.v0z - o32.z};
    const f3 b{a.x + t.e1x, a.y + t.e1y, a.z + t.e1z}, c{a.x + t.e2x, a.y + t.e2y, a.z + t.e2z};
    const float m0 = (float)vm.minv[0], m1 = (float)vm.minv[1], m2 = (float)vm.minv[2], m3 = (float)vm.minv[3], m4 = (float)vm.minv[4],
                m5 = (float)vm.minv[5], m6 = (float)vm.minv[6], m7 = (float)vm.minv[7], m8 = (float)vm.minv[8];
    const float az = fmaf(m6, a.x, fmaf(m7, a.y, m8 * a.z)), bz = fmaf(m6, b.x, fmaf(m7, b.y, m8 * b.z)), cz = fmaf(m6, c.x, fmaf(m7, c.y, m8 * c.z));
    if (!(fminf(az, fminf(bz, cz)) > 1e-20f)) { r.unsafe = true; return r; }      // at or behind the camera plane
    const float ra = 1.0f / az, rb = 1.0f / bz, rc = 1.0f / cz;
    const float ax = fmaf(m0, a.x, fmaf(m1, a.y, m2 * a.z)) * ra, ay = fmaf(m3, a.x, fmaf(m4, a.y, m5 * a.z)) * ra;
    const float bx = fmaf(m0, b.x, fmaf(m1, b.y, m2 * b.z)) * rb, by = fmaf(m3, b.x, fmaf(m4, b.y, m5 * b.z)) * rb;
    const float cx = fmaf(m0, c.x, fmaf(m1, c.y, m2 * c.z)) * rc, cy = fmaf(m3, c.x, fmaf(m4, c.y, m5 * c.z)) * rc;
    const float pad = (float)kRasterPad;
    const float lox = fminf(ax, fminf(bx, cx)) - pad, hix = fmaxf(ax, fmaxf(bx, cx)) + pad;
    const float loy = fminf(ay, fminf(by, cy)) - pad, hiy = fmaxf(ay, fmaxf(by, cy)) + pad;
    if (!(fabsf(lox) < 1e9f && fabsf(hix) < 1e9f && fabsf(loy) < 1e9f && fabsf(hiy) < 1e9f)) { r.unsafe = true; return r; }
    const float fx0 = fmaxf(ceilf(lox), 0.0f), fx1 = fminf(floorf(hix), (float)(w - 1));
    const float fy0 = fmaxf(ceilf(loy), 0.0f), fy1 = fminf(floorf(hiy), (float)(h - 1));
    if (fx0 > fx1 || fy0 > fy1) return r;
    r.x0 = (int)fx0; r.x1 = (int)fx1; r.y0 = (int)fy0; r.y1 = (int)fy1;
    return r;
}

// Camera-facing?  (k_raster handles these in its first launch, the others in the second: see there.)
DRT_HD bool tri_faces_away(f3 o32, const TriRec& t) {
    const f3 a{t.v0x - o32.x, t.v0y - o32.y, t.v0z - o32.z};
    return dot(a, cross(f3{t.e1x, t.e1y, t.e1z}, f3{t.e2x, t.e2y, t.e2z})) > 0.0f;
}

// 64-bit key of a hit: t > 0, so its bit pattern orders like an unsigned integer; equal t -> lowest face id wins.
DRT_HD unsigned long long raster_key(float t, int32_t face) {
    uint32_t tb;
    memcpy(&tb, &t, 4);
    return ((unsigned long long)tb << 32) | (unsigned long long)(uint32_t)face;
}
constexpr unsigned long long kRasterEmpty = ~0ull;

// Where the key of the ray in column x of (sub-batch-global) row gy lives: 4 x 4-pixel tiles, 16 keys = one 128-byte cache line each.
// The chip serves memory requests -- and atomics above all -- per cache line, not per lane (tools/ubench/atomic_pattern.hip); the pixels a
// triangle of one to three pixels touches, and those of its neighbours in the wave, share a tile far more often than a 16-pixel run of
// one image row.  A bijection of [0, rows * w) whenever w and the row count are multiples of 4 (whole 64 x 4 patches: the
// precondition of the projection pass).
DRT_HD int64_t raster_slot(unsigned x, unsigned gy, unsigned w) {
    return (((int64_t)(gy >> 2) * (w >> 2) + (x >> 2)) << 4) | ((gy & 3u) << 2) | (x & 3u);
}

// ---- the deal of k_raster's runs by the test counts of the previous call ---------------------------------------------------------------
// k_raster's unit of work is a run (image, 64 consecutive triangles); a run holds anything from no (triangle, pixel) test to
// 64 * kRasterMaxPerLane of them, and how many it held in the previous call on the same rays is nearly how many it holds now.  The
// line of all work -- run after run, each `c_fixed + cost[run]` long: what a run costs without a test (record load, facing test,
// projection, prefix sum) in units of one test, then its tests -- is cut into V pieces of equal length, one per wave.  A boundary is a
// position (run, item): a cut that falls into a run's fixed part moves to the run's start (item 0), one that falls among its tests
// splits the run between waves, each of which projects the run again and works its own items.
struct DealPos { uint32_t run, item; };
constexpr uint32_t kRasterDealFixed = 64;    // c_fixed (profiles/raster_deal.txt section 4: 16, 64 and 256 measured alike, 1 024 and more slower)

DRT_HD uint64_t raster_deal_weight(uint32_t cost, uint32_t c_fixed) { return (uint64_t)c_fixed + cost; }
DRT_HD uint64_t raster_deal_target(uint64_t total, uint32_t n_waves, uint32_t v) {      // floor(v C / V) (< C for v < V), without the product v C
    return (total / n_waves) * v + (total % n_waves) * v / n_waves;
}
DRT_HD uint32_t raster_deal_item(uint64_t off, uint32_t c_fixed) { return off > c_fixed ? (uint32_t)(off - c_fixed) : 0u; }      // a cut `off` into a run's weight

// Boundary v of V over `n_runs` runs, from the INCLUSIVE prefix sums of raster_deal_weight: B[0] = (0, 0), B[V] = (n_runs, 0), and B[v]
// where the running sum reaches floor(v C / V), C the grand total.  Non-decreasing in v in the order of (run, item).
DRT_HD DealPos raster_deal_boundary(const uint64_t* prefix, uint32_t n_runs, uint32_t n_waves, uint32_t v, uint32_t c_fixed) {
    if (v == 0 || n_runs == 0) return DealPos{0, 0};
    if (v >= n_waves) return DealPos{n_runs, 0};
    const uint64_t total = prefix[n_runs - 1];
    const uint64_t target = raster_deal_target(total, n_waves, v);
    uint32_t lo = 0, hi = n_runs - 1;                                                     // first run whose inclusive sum exceeds the target
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] > target) hi = mid; else lo = mid + 1;
    }
    return DealPos{lo, raster_deal_item(target - (lo ? prefix[lo - 1] : 0), c_fixed)};
}

// The same boundaries from the runs' side, without a search (k_raster_deal: a thread per run): the boundaries that fall into a run whose
// weights before it sum to `before` and with it to `with` are those of the waves [first_wave(before), first_wave(with)) --
// floor(v C / V) >= X exactly when v >= ceil(X V / C) -- and boundary v of them is (run, raster_deal_item(target(v) - before)).
DRT_HD uint32_t raster_deal_first_wave(uint64_t sum, uint64_t total, uint32_t n_waves) {
    const uint64_t q = (sum * n_waves + total - 1) / total;
    return q > n_waves ? n_waves : (uint32_t)q;
}
// What k_raster_deal's thread of run `run` does once it knows the sums: write the boundaries inside its run.  Over all runs every entry
// [0, V) is written exactly once (total > 0); entry V = (n_runs, 0) is the caller's.
DRT_HD void raster_deal_place(DealPos* table, uint32_t run, uint64_t before, uint64_t with, uint64_t total, uint32_t n_waves, uint32_t c_fixed) {
    if (!(with > before) || total == 0) return;
    const uint32_t v1 = raster_deal_first_wave(with, total, n_waves);
    for (uint32_t v = raster_deal_first_wave(before, total, n_waves); v < v1; ++v)
        table[v] = DealPos{run, raster_deal_item(raster_deal_target(total, n_waves, v) - before, c_fixed)};
}

// What a table may hold that describes another launch (more runs, a graph replayed behind a call of another shape): nothing past the end.
DRT_HD DealPos raster_deal_clamp(DealPos b, uint32_t n_runs) { return b.run >= n_runs ? DealPos{n_runs, 0} : b; }

// The runs of the wave between boundaries b0 <= b1: first .. last, the last one only if b1 cuts into it; none when b0 == b1.
DRT_HD uint32_t raster_deal_end(DealPos b0, DealPos b1) {
    if (b0.run == b1.run && b0.item == b1.item) return b0.run;
    return b1.run + (b1.item > 0 ? 1u : 0u);
}

// The wave's items [lo, hi) of run r of its range (whatever the run's actual total is: a slice past it is empty, the last slice of a run
// is open-ended), and whether the wave OWNS the run: its range contains (r, 0).  Every run has exactly one owner.
struct DealSlice { uint32_t lo, hi; bool owner; };
DRT_HD DealSlice raster_deal_slice(DealPos b0, DealPos b1, uint32_t r) {
    DealSlice s;
    s.lo = b0.run == r ? b0.item : 0u;
    s.hi = b1.run == r ? b1.item : 0xFFFFFFFFu;
    s.owner = (b0.run < r || (b0.run == r && b0.item == 0)) && (r < b1.run || (r == b1.run && b1.item > 0));
    return s;
}


// The same slices as a wave walks its range: only its first run can start past item 0 -- and is then not the wave's own --, only its
// last can end early.  Four scalars of loop state instead of two boundaries and a run number (k_raster has none to spare).
struct DealRange { uint32_t run, end, lo, last_hi; };
DRT_HD DealRange raster_deal_range(DealPos b0, DealPos b1) { return DealRange{b0.run, raster_deal_end(b0, b1), b0.item, b1.item ? b1.item : 0xFFFFFFFFu}; }
DRT_HD DealSlice raster_deal_slice(const DealRange& g) { return DealSlice{g.lo, g.run + 1 == g.end ? g.last_hi : 0xFFFFFFFFu, g.lo == 0}; }      // of run g.run < g.end
DRT_HD void raster_deal_next(DealRange& g) { ++g.run; g.lo = 0; }

}  // namespace drt
