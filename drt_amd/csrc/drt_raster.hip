// drt_raster.hip -- kernels of the projected primary-visibility pass (drt_raster.h) and their launcher.
#include "drt_device.h"

// One block per image: lane 0 fits the pinhole model from the four corner rays, then 64 lanes check an 8x8 lattice of
// the image's rays against it; an image that is not a pinhole grid keeps ok = 0 and takes the BVH path entirely
// (k_raster skips it; k_cull verifies every ray once more anyway).
__global__ void __launch_bounds__(64) k_fit_views(const double* __restrict__ origin, const double* __restrict__ dir, int w, int h,
                                                  ViewModel* __restrict__ views) {
    __shared__ ViewModel vm;
    const int64_t base = (int64_t)blockIdx.x * w * h;
    if (threadIdx.x == 0) {
        const int64_t i00 = base, iW0 = base + (w - 1), i0H = base + (int64_t)(h - 1) * w, iWH = i0H + (w - 1);
        if (fit_view_model(load_d3(origin, i00), load_d3(dir, i00), load_d3(dir, iW0), load_d3(dir, i0H), load_d3(dir, iWH),
                           (double)(w - 1), (double)(h - 1), vm))
            vm.ok = 1;
    }
    __syncthreads();
    bool good = vm.ok != 0;
    if (good) {
        const int sx = (int)(threadIdx.x & 7), sy = (int)(threadIdx.x >> 3);
        const int x = (int)(((int64_t)(w - 1) * sx) / 7), y = (int)(((int64_t)(h - 1) * sy) / 7);
        const int64_t i = base + (int64_t)y * w + x;
        good = view_verify(vm, load_d3(origin, i), load_d3(dir, i), (double)x, (double)y);
    }
    const bool all_good = __ballot(good) == ~0ull;
    if (threadIdx.x == 0) {
        vm.ok = all_good ? 1 : 0;
        vm.all = vm.ok;              // k_cull clears it when a ray of the image does not verify
        views[blockIdx.x] = vm;
    }
}

// DRT_GRID_TRUST: the models come from the caller's cache -- but a trusted image is not taken on faith entirely: the 8x8 lattice of
// its rays (the 64 rays k_fit_views samples) is read again and checked against the cached model, so that ray tensors that were
// replaced wholesale behind the cache's back (a write through `.data` or a raw pointer, which no version counter sees) are caught for
// the price of 64 ray loads per image.  An image that fails is re-fitted from its corner rays on the spot and loses `all` -- in the
// working copy AND in the cache -- so that every one of its rays is verified individually (k_cull_listed's general path), in this
// call and in every later one, exactly as in a call without a cache.
// The CANARY (`salt` != 0): besides the fixed lattice every lane re-verifies one more ray of the image at a pseudo-random pixel that changes
// from call to call (a hash of the call's salt, the image and the lane): 64 rays per image and call that a partial overwrite behind the
// version counter's back (a block of rows written through a raw pointer, `t.data[...] = ...`) cannot avoid for long -- a fraction f of
// modified rays survives a call with probability (1 - f)^64 per image.  Same consequence as a lattice mismatch.
__device__ __forceinline__ uint32_t canary_hash(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA6Bu ^ (c + 0x165667B1u) * 0xC2B2AE35u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    return h;
}
__global__ void __launch_bounds__(64) k_check_views(const double* __restrict__ origin, const double* __restrict__ dir, int w, int h,
                                                    ViewModel* __restrict__ cache, ViewModel* __restrict__ views, unsigned salt, unsigned* __restrict__ salt_ctr) {
    __shared__ ViewModel vm;
    __shared__ unsigned s_ctr;
    const int64_t base = (int64_t)blockIdx.x * w * h;
    if (threadIdx.x == 0) {
        vm = cache[blockIdx.x];
        // The call's salt is a HOST counter: baked into a captured graph, every replay would re-check the same 64 pixels.  A DEVICE counter that
        // every launch bumps is mixed in, so that replays move on like eager calls do (which value a block happens to read does not matter:
        // any pixel is a legitimate canary).
        s_ctr = salt_ctr ? __hip_atomic_load(salt_ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        if (salt_ctr && blockIdx.x == 0) atomicAdd(salt_ctr, 1u);
    }
    __syncthreads();
    if (salt) salt = (salt ^ (s_ctr * 0x9E3779B1u)) | 1u;
    const bool trusted = vm.ok && vm.all;              // (k_store_models stores ok == all)
    const int sx = (int)(threadIdx.x & 7), sy = (int)(threadIdx.x >> 3);
    const int x = (int)(((int64_t)(w - 1) * sx) / 7), y = (int)(((int64_t)(h - 1) * sy) / 7);
    const int64_t i = base + (int64_t)y * w + x;
    bool good = trusted && view_verify(vm, load_d3(origin, i), load_d3(dir, i), (double)x, (double)y);
    if (good && salt) {
        const uint32_t hx = canary_hash(salt, blockIdx.x, threadIdx.x), hy = canary_hash(salt ^ 0xA5A5A5A5u, threadIdx.x, blockIdx.x);
        const int cx = (int)(((uint64_t)hx * (uint64_t)w) >> 32), cy = (int)(((uint64_t)hy * (uint64_t)h) >> 32);
        const int64_t ci = base + (int64_t)cy * w + cx;
        good = view_verify(vm, load_d3(origin, ci), load_d3(dir, ci), (double)cx, (double)cy);
    }
    if (__ballot(good) == ~0ull) {                     // wave-uniform: the usual case
        if (threadIdx.x == 0) views[blockIdx.x] = vm;
        return;
    }
    // not (or no longer) a trusted grid: fit it like a call without a cache would
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t i00 = base, iW0 = base + (w - 1), i0H = base + (int64_t)(h - 1) * w, iWH = i0H + (w - 1);
        if (fit_view_model(load_d3(origin, i00), load_d3(dir, i00), load_d3(dir, iW0), load_d3(dir, i0H), load_d3(dir, iWH),
                           (double)(w - 1), (double)(h - 1), vm))
            vm.ok = 1;
    }
    __syncthreads();
    good = vm.ok != 0 && view_verify(vm, load_d3(origin, i), load_d3(dir, i), (double)x, (double)y);
    const bool all_good = __ballot(good) == ~0ull;
    if (threadIdx.x == 0) {
        vm.ok = all_good ? 1 : 0;
        vm.all = 0;                                    // never trusted again: per-ray verification from now on
        views[blockIdx.x] = vm;
        if (trusted) { cache[blockIdx.x].ok = 0; cache[blockIdx.x].all = 0; }
    }
}

// Test one (triangle, pixel) pair and fold a hit into the pixel's key.  The plain read of the current key may be stale
// (the L1 is not coherent with the atomics at L2) but keys only ever decrease, so a stale value is >= the true one:
// skipping when the new key is not smaller than what was read can never drop a winner.
__device__ __forceinline__ void raster_test(const TriRec& t, f3 o32, const double* __restrict__ dir, int64_t i, int64_t slot,
                                            unsigned long long* __restrict__ zbuf, uint32_t* __restrict__ zmask) {
    const f3 d32 = to_f32(load_d3(dir, i));
    float tt;
    // (tri_hit's conditions with the cheap ones first: the barycentric test, "would this key win", and only then the hit-point test)
    if (!tri_hit_mt(o32, d32, f3{t.v0x, t.v0y, t.v0z}, f3{t.e1x, t.e1y, t.e1z}, f3{t.e2x, t.e2y, t.e2z}, tt)) return;
    const unsigned long long key = raster_key(tt, t.face);
    if (key >= zbuf[slot]) return;
    if (!hit_point_in_box(o32, d32, tt, f3{t.v0x, t.v0y, t.v0z}, f3{t.e1x, t.e1y, t.e1z}, f3{t.e2x, t.e2y, t.e2z}, t.margin)) return;
    atomicMin(&zbuf[slot], key);
    // one bit per 64 consecutive rays: k_cull reads keys only there.  Thousands of hits share a word, and atomics on ONE
    // address are served one at a time: set the bit only when a (possibly stale) read does not show it yet
    const uint32_t bit = 1u << ((i >> 6) & 31);
    if (!(zmask[i >> 11] & bit)) atomicOr(&zmask[i >> 11], bit);
}

struct BigItem { int32_t view, tri, x0, y0, nx, ny; };

// The unit of work is a RUN: (image, 64 consecutive triangles in Morton order), image-major.  A lane projects its triangle (float32
// is ample: the box is padded by 1/16 pixel) and counts the pixel centres inside the padded box -- 0 for most sub-pixel triangles, a
// handful typically, dozens for a few.  The (triangle, pixel) tests of the run are then dealt to the wave's lanes 64 at a time (wave
// prefix sum of the counts, owner found by bisection in LDS), so that one fat triangle does not hold 63 idle lanes.
//
// The grid is what is resident (8 blocks per CU) and every WAVE loops over runs on its own: under the STATIC deal wave v of V takes runs
// v, v + V, ... (the first call on a set of rays, small launches, DRT_RASTER_DEAL=0; for the other deal see DEAL below).
// About half the runs of a launch hold nothing (Morton neighbours face the same way, and a launch handles one facing), the others up
// to several thousand tests; with a block per 256 triangles, a block -- and its 16 KB of LDS -- lived as long as its slowest wave,
// and the chip's wave slots were half empty (profiles/raster_runs.txt).  No block barrier anywhere: a wave's slice of s_lane is its
// own; a wave barrier separates its writes from its reads, and one run's reads from the next run's writes.  (Runs dealt by cursor
// words instead, as k_cull_listed's are, doubled the launch: same file.)
struct RasterLane {            // what a lane publishes for the wave: its triangle and its box
    TriRec tri;
    int32_t x0, y0, nx, end;   // `end` = inclusive prefix sum of the counts (first work item NOT of this lane)
};

__device__ __forceinline__ float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// DEAL: the wave's runs are instead the contiguous range between two boundaries of a table made from the test counts every run had in the
// previous call (drt_raster.h, k_raster_deal below): ranges of equal predicted work, a heavy run cut between several waves.  Two
// wave-uniform loads, no atomic, no block barrier.  The result does not depend on what the table holds: every (run, item) is worked by
// exactly one wave for ANY non-decreasing table (a slice past the run's actual total is empty, a run's last slice is open-ended; the two
// ends are fixed here, and a boundary past the last run is clamped), every wave that shares a run projects it again and counts alike, and
// what must happen once per run -- listing a large triangle, demoting the image, recording the run's tests for the next table -- is done
// by the run's one OWNER, the wave whose range holds the run's start.  Under the static deal every wave owns its runs.
//
// RECORD: the owner writes the run's number of tests for the next table.  The kernel has no scalar register to spare for another pointer
// that lives across the run loop (it spills a dozen vector registers with one), so the counts lie behind the big list's counter, in the
// same allocation: word kRasterCostAt + 2 * run + pass of `big_count`.  A recording launch has no early exit for an image that is not
// `ok`: it goes on to the (empty) count.  A launch that neither deals nor records -- k_raster<false, false, .> -- is the loop as it was.
constexpr int kRasterCostAt = 32;
template <bool DEAL, bool RECORD, int pass>
__global__ void __launch_bounds__(256, 8) k_raster(const TriRec* __restrict__ tris, int n_tris, ViewModel* views, int n_views,
                                                   const double* __restrict__ dir, int w, int h,
                                                   unsigned long long* __restrict__ zbuf, uint32_t* __restrict__ zmask,
                                                   BigItem* __restrict__ big, unsigned* big_count,
                                                   const DealPos* __restrict__ table /* DEAL: this pass's boundaries [n_waves + 1] */) {
    constexpr unsigned big_cap = drt_scene::kBigCap;
    __shared__ RasterLane s_lane[256];
    const int lane = threadIdx.x & 63;
    RasterLane* const wl = s_lane + (threadIdx.x & ~63);      // this wave's slice
    const unsigned n_waves = gridDim.x * 4u, wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const unsigned runs_per_view = ((unsigned)n_tris + 63u) / 64u, n_runs = runs_per_view * (unsigned)n_views;
    int cur_view = -1;
    float minv32[9] = {};
    f3 o32{0.0f, 0.0f, 0.0f};
    DealRange g{wave, n_runs, 0u, 0xFFFFFFFFu};
    if (DEAL) {
        const DealPos b0 = wave == 0 ? DealPos{0, 0} : raster_deal_clamp(table[wave], n_runs);
        const DealPos b1 = wave + 1 >= n_waves ? DealPos{n_runs, 0} : raster_deal_clamp(table[wave + 1], n_runs);
        g = raster_deal_range(b0, b1);
        g.end = min(g.end, n_runs);
    }
    for (; g.run < g.end; DEAL ? raster_deal_next(g) : (void)(g.run += n_waves)) {
        const unsigned run = g.run;
        const int view = (int)(run / runs_per_view);
        const int k = (int)(run - (unsigned)view * runs_per_view) * 64 + lane;
        const DealSlice sl = DEAL ? raster_deal_slice(g) : DealSlice{0u, 0xFFFFFFFFu, true};
        // wave-uniform; read per run: an image that a run demoted is left alone by the later ones.  (A recording launch goes on to the
        // count, which is then 0, instead of leaving the loop here: a store on this path costs the kernel a dozen spilled registers.)
        const bool ok = __hip_atomic_load(&views[view].ok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        if (!RECORD && !ok) continue;
        if (ok && view != cur_view) {                               // the model, as the float32 values project_tri_box uses, in scalar registers while the image lasts
            cur_view = view;
            for (int q = 0; q < 9; ++q) minv32[q] = wave_uniform((float)views[view].minv[q]);
            o32 = f3{wave_uniform((float)views[view].o[0]), wave_uniform((float)views[view].o[1]), wave_uniform((float)views[view].o[2])};
        }
        int count = 0;
        __builtin_amdgcn_wave_barrier();                      // the last run's reads of the slice are through
        if ((!RECORD || ok) && k < n_tris) {
            const TriRec tri = tris[k];
            // Two launches: triangles facing the camera first (pass 0), the others second (pass 1).  Every triangle is handled in
            // exactly one of them, so the result is the same minimum; but a pixel's closest hit is nearly always a front face,
            // and the second launch sees the finished keys of the first: its read-before-atomic check then skips almost every
            // back face, which cuts the 64-bit atomics -- what bounds this kernel -- by more than half.
            if ((pass == 1) == tri_faces_away(o32, tri)) {
                ViewModel vm;                                 // (project_tri_box rounds the matrix to float32 first: the same values)
                for (int q = 0; q < 9; ++q) vm.minv[q] = (double)minv32[q];
                const PixelBox box = project_tri_box(vm, o32, tri, w, h);
                if (box.unsafe) {          // the camera plane cuts (or touches) this triangle: no projection bound for this image
                    if (sl.owner) __hip_atomic_store(&views[view].ok, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } else if (box.x0 <= box.x1 && box.y0 <= box.y1) {
                    const int nx = box.x1 - box.x0 + 1, ny = box.y1 - box.y0 + 1;
                    const int64_t cnt = (int64_t)nx * ny;
                    if (cnt > kRasterMaxPerLane) {
                        // listed for k_raster_big, one WAVE per entry: in bands of whole rows of at most kRasterBandPixels pixel centres
                        // (by the run's owner: a wave that only shares the run counts nothing for this triangle, like the owner)
                        const int rows_per = max(1, kRasterBandPixels / nx), n_bands = (ny + rows_per - 1) / rows_per;
                        const unsigned slot = sl.owner ? atomicAdd(big_count, (unsigned)n_bands) : 0u;
                        if (!sl.owner) {
                        } else if (slot <= big_cap && (unsigned)n_bands <= big_cap - slot) {
                            for (int b = 0; b < n_bands; ++b)
                                big[slot + b] = BigItem{view, k, box.x0, box.y0 + b * rows_per, nx, min(rows_per, ny - b * rows_per)};
                        } else {
                            __hip_atomic_store(&views[view].ok, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // list full: BVH path for this image
                            for (unsigned q = slot; q < big_cap; ++q) big[q] = BigItem{view, k, 0, 0, 0, 0};      // (what was reserved below the cap: empty entries)
                        }
                    } else {
                        count = (int)cnt;
                        wl[lane].tri = tri;                   // published for the wave (a lane without tests is never an owner: only its `end` is read)
                        wl[lane].x0 = box.x0; wl[lane].y0 = box.y0; wl[lane].nx = nx;
                    }
                }
            }
        }
        // inclusive prefix sum of the counts over the wave
        int end = count;
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(end, off);
            if (lane >= off) end += v;
        }
        const int total = __builtin_amdgcn_readlane(end, 63);  // (a scalar: the loop's state stays in scalar registers only while its branches are wave-uniform)
        if (RECORD && sl.owner && lane == 0) big_count[kRasterCostAt + 2 * run + pass] = (unsigned)total;   // what the next call's table is made from
        const int stop = (int)min((unsigned)total, sl.hi);     // this wave's items: [sl.lo, stop)
        if (sl.lo >= (unsigned)stop) continue;                 // most runs of a view see nothing but background
        wl[lane].end = end;                                    // read back by the lanes of this wave only: no block barrier needed
        __builtin_amdgcn_wave_barrier();
        const int64_t base = (int64_t)view * w * h;
        for (int item0 = (int)sl.lo; item0 < stop; item0 += 64) {
            const int item = item0 + lane;
            if (item >= stop) break;
            int lo = 0, hi = 63;                               // first lane whose `end` exceeds item
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (wl[mid].end > item) hi = mid; else lo = mid + 1;
            }
            const RasterLane& ow = wl[lo];
            const int local = item - (lo == 0 ? 0 : wl[lo - 1].end);
            const int row = (int)(((float)local + 0.5f) / (float)ow.nx);     // exact for these small integers
            const int x = ow.x0 + (local - row * ow.nx), y = ow.y0 + row;
            raster_test(ow.tri, o32, dir, base + (int64_t)y * w + x, raster_slot((unsigned)x, (unsigned)(view * h + y), (unsigned)w), zbuf, zmask);
        }
    }
}

// The table of the NEXT call's launches from the counts this call's launches recorded.  A thread per run, blocks of 1 024 runs, grid.y the
// pass.  Every block sums ALL counts of its pass (coalesced, a few dozen loads per thread: cheaper than a second launch or a hand-over
// between blocks) for the grand total and for what lies before its own runs, scans its own 1 024 weights, and every run then places
// the boundaries that fall into it (raster_deal_first_wave: no search).  The first form -- one block per pass, a bisection over the prefix
// sums per boundary -- was a chain of 120 dependent loads per thread and took 140 - 165 us, more than the launches it balances
// (profiles/raster_deal.txt section 3); this one takes 15 - 17 us at 28 296 runs.  Enqueued behind the projection pass on the sub-batch's own stream: nothing of this call reads
// the table any more, and the next call's launch is behind it in stream order.
constexpr int kDealBlock = 1024;
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int off) {
    return ((uint64_t)(uint32_t)__shfl_up((int)(v >> 32), off) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, off);
}
__global__ void __launch_bounds__(kDealBlock) k_raster_deal(const unsigned* __restrict__ counts /* k_raster's `big_count` */, DealPos* __restrict__ table,
                                                            unsigned n_runs, unsigned n_waves, uint32_t c_fixed) {
    __shared__ uint64_t s_all[kDealBlock / 64], s_before[kDealBlock / 64], s_own[kDealBlock / 64];
    const unsigned pass = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    DealPos* const tab = table + pass * (n_waves + 1);
    const unsigned* const cost = counts + kRasterCostAt + pass;      // (the passes interleaved)
    const unsigned first = blockIdx.x * kDealBlock, run = first + tid;
    constexpr unsigned kMost = 64u * (unsigned)kRasterMaxPerLane;    // what a run can hold: the sums below stay far inside 64 bits whatever the words hold
    uint64_t all = 0, before = 0, own = 0;
    for (unsigned base = 0; base < n_runs; base += kDealBlock) {
        const unsigned r = base + tid;
        const uint64_t wgt = r < n_runs ? raster_deal_weight(min(cost[2 * r], kMost), c_fixed) : 0;
        all += wgt;
        if (base < first) before += wgt;
        if (base == first) own = wgt;
    }
    // inclusive scan of `own` over the wave; wave sums of all three
    uint64_t incl = own;
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t v = shfl_up_u64(incl, off), va = shfl_up_u64(all, off), vb = shfl_up_u64(before, off);
        if ((int)lane >= off) { incl += v; all += va; before += vb; }
    }
    if (lane == 63) { s_all[wid] = all; s_before[wid] = before; s_own[wid] = incl; }
    __syncthreads();
    uint64_t total = 0, start = 0;
    for (unsigned q = 0; q < kDealBlock / 64; ++q) {
        total += s_all[q];
        start += s_before[q];
        if (q < wid) start += s_own[q];
    }
    const uint64_t with = start + incl;
    if (run < n_runs) raster_deal_place(tab, run, with - own, with, total, n_waves, c_fixed);
    if (run == 0) tab[n_waves] = DealPos{n_runs, 0};
}

// Triangles whose box holds more pixels than one lane should loop over: one WAVE per list entry (a band of rows of the box).  With the object
// filling the image a third of the camera-facing triangles are such entries, 50-300 pixel centres each: one BLOCK per entry on 2 blocks per
// CU -- the first form, written for the odd large triangle -- kept 512 entries in flight and took 0.4-0.7 ms per launch, twice the main
// kernel; a wave per entry on a full grid keeps 8192.
__global__ void __launch_bounds__(256) k_raster_big(const TriRec* __restrict__ tris, const ViewModel* __restrict__ views,
                                                    const double* __restrict__ dir, int w, int h,
                                                    unsigned long long* __restrict__ zbuf, uint32_t* __restrict__ zmask,
                                                    const BigItem* __restrict__ big, const unsigned* __restrict__ big_count, unsigned big_cap) {
    const unsigned n = min(*big_count, big_cap);          // (an overfull list was cut at an entry boundary: k_raster wrote whole triangles only)
    const unsigned n_waves = gridDim.x * 4u;
    const int lane = threadIdx.x & 63;
    for (unsigned e = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6)); e < n; e += n_waves) {
        const BigItem it = big[e];
        const ViewModel& vm = views[it.view];
        const TriRec t = tris[it.tri];
        const f3 o32 = to_f32(d3{vm.o[0], vm.o[1], vm.o[2]});
        const int64_t base = (int64_t)it.view * w * h;
        const int cnt = it.nx * it.ny;
        for (int p = lane; p < cnt; p += 64) {
            const int row = (int)(((float)p + 0.5f) / (float)it.nx);        // exact for p < 2^22
            int y = it.y0 + row, x = it.x0 + (p - row * it.nx);
            if (x >= it.x0 + it.nx) { x -= it.nx; ++y; } else if (x < it.x0) { x += it.nx; --y; }     // (belt and braces for bands of one very long row)
            raster_test(t, o32, dir, base + (int64_t)y * w + x, raster_slot((unsigned)x, (unsigned)(it.view * h + y), (unsigned)w), zbuf, zmask);
        }
    }
}

__global__ void k_fill_u64(unsigned long long* __restrict__ p, int64_t n, unsigned long long v) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

constexpr int64_t kRasterDealMaxRuns = (int64_t)1 << 18;   // every block of k_raster_deal reads all counts: launches of more runs keep the static deal
static int64_t raster_runs(int64_t n_tris, int n_views) { return (n_tris + 63) / 64 * n_views; }

// Workspace of the raster pass of one internal stream: keys [cap] (kept all-empty between calls: k_cull resets every
// key it consumes), group bits, image models, the big-triangle list.
int ensure_raster(drt_scene* s, drt_scene::Sub& w, int64_t n_rays, int n_views, hipStream_t st) {
    if (n_rays > w.z_cap) {
        (void)hipFree(w.zbuf); (void)hipFree(w.zmask);
        w.zbuf = nullptr; w.zmask = nullptr; w.z_cap = 0;
        const int64_t words = (n_rays + 2047) / 2048 + 1;
        HIP_TRY(hipMalloc(&w.zbuf, sizeof(unsigned long long) * n_rays));
        HIP_TRY(hipMalloc(&w.zmask, sizeof(uint32_t) * words));
        k_fill_u64<<<4 * s->n_cu, 256, 0, st>>>(w.zbuf, n_rays, kRasterEmpty);
        HIP_TRY(hipMemsetAsync(w.zmask, 0, sizeof(uint32_t) * words, st));
        w.z_cap = n_rays;
    }
    if (n_views > w.vm_cap) {
        (void)hipFree(w.vmodel); w.vmodel = nullptr; w.vm_cap = 0;
        HIP_TRY(hipMalloc(&w.vmodel, sizeof(ViewModel) * n_views));
        w.vm_cap = n_views;
    }
    if (!w.big) HIP_TRY(hipMalloc(&w.big, sizeof(BigItem) * drt_scene::kBigCap));
    // the deal of k_raster's runs: counts per run (behind the big list's counter: k_raster), boundaries per resident wave, for either pass
    drt_scene::Sub::Deal& dl = w.deal;
    // Allocated ONCE, for the most runs a launch may deal (2 MB) and the scene's grid: a captured graph holds both pointers, and unlike
    // the key buffer they never move.
    if (!w.big_count) {
        const int n_waves = 8 * s->n_cu * 4;
        HIP_TRY(hipMalloc(&w.big_count, sizeof(unsigned) * (kRasterCostAt + (s->raster_deal ? 2 * kRasterDealMaxRuns : 0))));
        if (s->raster_deal) {
            HIP_TRY(hipMalloc(&dl.table, sizeof(DealPos) * 2 * (n_waves + 1)));
            dl.cap_runs = kRasterDealMaxRuns; dl.cap_waves = n_waves;
        }
    }
    return DRT_OK;
}

// Fit the image models and rasterise every triangle into the key buffer of `w` (rays [0, n_views * w * h) of the sub-batch).
int launch_raster(drt_scene* s, drt_scene::Sub& w, hipStream_t st, const double* d_origin, const double* d_dir, int n_views, int iw, int ih,
                  ViewModel* trusted) {
    const int n = (int)s->n_faces;
    HIP_TRY(hipMemsetAsync(w.big_count, 0, sizeof(unsigned), st));
    if (trusted) k_check_views<<<n_views, 64, 0, st>>>(d_origin, d_dir, iw, ih, trusted, w.vmodel,           // models of an earlier call: lattice re-checked,
                                                        s->grid_canary ? (++s->canary_salt ? s->canary_salt : ++s->canary_salt) : 0u,    // + 64 rays at this call's random pixels
                                                        s->vcount + 3);                                                                  //   (device counter: moves on under graph replay too)
    else k_fit_views<<<n_views, 64, 0, st>>>(d_origin, d_dir, iw, ih, w.vmodel);
    if (n > 0) {
        // The deal: from the table when it describes THIS launch (the same rays, image shape, triangle count and grid as the launch whose
        // counts it was made from), statically otherwise -- the first call, another sub-batch on this workspace, a new topology.
        drt_scene::Sub::Deal& dl = w.deal;
        const int grid = 8 * s->n_cu;
        const int64_t n_runs = raster_runs(n, n_views);
        // Launches of fewer runs than `raster_deal_min_runs` keep the static deal and record nothing: with less than about two runs per
        // resident wave there is little to balance, and k_raster_deal's 15 us on the sub-batch's chain cost more than the shorter
        // launches gave (9 views, 7 074 runs: +1.5 % per step; profiles/raster_deal.txt section 6).
        const bool record = s->raster_deal && dl.table && n_runs > 0 && n_runs >= s->raster_deal_min_runs && n_runs <= dl.cap_runs && grid * 4 == dl.cap_waves;
        const bool dealt = record && dl.complete && dl.dir == d_dir && dl.n_views == n_views && dl.iw == iw && dl.ih == ih && dl.n_tris == n && dl.grid == grid;
        s->raster_deal_counts[dealt ? 0 : 1] += 2;
        for (int pass = 0; pass < 2; ++pass) {
            auto* const kern = pass == 0 ? (dealt ? k_raster<true, true, 0> : record ? k_raster<false, true, 0> : k_raster<false, false, 0>)
                                         : (dealt ? k_raster<true, true, 1> : record ? k_raster<false, true, 1> : k_raster<false, false, 1>);
            kern<<<grid, 256, 0, st>>>(s->tris_flat, n, w.vmodel, n_views, d_dir, iw, ih, w.zbuf, w.zmask, reinterpret_cast<BigItem*>(w.big), w.big_count,
                                       dealt ? dl.table + pass * (dl.cap_waves + 1) : nullptr);
            if (pass == 0) {   // the large triangles of the first launch before the second one reads the keys
                k_raster_big<<<8 * s->n_cu, 256, 0, st>>>(s->tris_flat, w.vmodel, d_dir, iw, ih, w.zbuf, w.zmask,
                                                           reinterpret_cast<const BigItem*>(w.big), w.big_count, drt_scene::kBigCap);
                HIP_TRY(hipMemsetAsync(w.big_count, 0, sizeof(unsigned), st));
            }
        }
        k_raster_big<<<8 * s->n_cu, 256, 0, st>>>(s->tris_flat, w.vmodel, d_dir, iw, ih, w.zbuf, w.zmask,
                                                   reinterpret_cast<const BigItem*>(w.big), w.big_count, drt_scene::kBigCap);
        dl.complete = false;
        if (record) {
            k_raster_deal<<<dim3((unsigned)((n_runs + kDealBlock - 1) / kDealBlock), 2), kDealBlock, 0, st>>>(w.big_count, dl.table, (unsigned)n_runs, (unsigned)(grid * 4), s->raster_deal_fixed);
            dl.dir = d_dir; dl.n_views = n_views; dl.iw = iw; dl.ih = ih; dl.n_tris = n; dl.grid = grid;
            dl.complete = true;
        }
    }
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}
