// drt_pathsink.h -- what the path kernels of more than one translation unit share (drt_pipeline.hip: the two-bounce pipeline;
// drt_paths.hip: paths of up to K interactions; drt_image.hip / drt_image_loss.hip: the refracted image and its loss): the compact
// ray list, the staged list append, the LDS hash sink of the vertex gradients, the small pieces of the K-interaction backward kernels and
// the pass of every gradient kernel over its list through that sink (sink_pass).
#pragma once
#include "drt_device.h"

struct RayList {
    int32_t* idx;     // ray index within the chunk
    float* ray;       // [cap,6] float32 origin, direction -- exactly what the tracer sees
    int32_t* face;    // [cap] traversal result
};

// Staged list append.  A returning atomic on one counter word is served at ~90 per microsecond, and the 2048 resident
// blocks of a shading kernel all arrive at it together: one push per 256-entry block iteration made k_shade1/2 and
// k_finish wait on the counter for more than half of their time.  A block therefore collects its survivors in LDS
// (index + float32 ray) and reserves list space once per ~500-700 of them; the copy-out is fully coalesced.
constexpr int kStageCap = 768;                       // 21.5 KB: six blocks per CU keep their LDS
struct StageMem {
    int32_t idx[kStageCap];
    float ray[kStageCap * 6];
    unsigned n, base, wtot[kPathWaves];
};
__device__ __forceinline__ void stage_init(StageMem& m) {
    if (threadIdx.x == 0) m.n = 0u;
    __syncthreads();
}
// whole block; m.n must be stable (a barrier since its last update)
__device__ __forceinline__ void stage_flush(StageMem& m, const RayList& out, unsigned* counter) {
    const unsigned cnt = m.n;
    if (threadIdx.x == 0) m.base = cnt ? atomicAdd(counter, cnt) : 0u;
    __syncthreads();
    const unsigned base = m.base;
    for (unsigned k = threadIdx.x; k < cnt; k += kPathBlock) out.idx[base + k] = m.idx[k];
    if (out.ray) for (unsigned k = threadIdx.x; k < 6u * cnt; k += kPathBlock) out.ray[6 * (int64_t)base + k] = m.ray[k];
    __syncthreads();
    if (threadIdx.x == 0) m.n = 0u;
    __syncthreads();
}
// whole block, once per block iteration (<= kPathBlock new entries)
__device__ __forceinline__ void stage_push(StageMem& m, bool pred, int32_t i, f3 o, f3 d, const RayList& out, unsigned* counter) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long mask = __ballot(pred);
    if (lane == 0) m.wtot[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    unsigned slot = m.n, tot = 0;
    for (int w = 0; w < kPathWaves; ++w) { const unsigned c = m.wtot[w]; if (w < wave) slot += c; tot += c; }
    if (pred) {
        slot += (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
        m.idx[slot] = i;
        if (out.ray) { float* e = m.ray + 6 * slot; e[0] = o.x; e[1] = o.y; e[2] = o.z; e[3] = d.x; e[4] = d.y; e[5] = d.z; }
    }
    __syncthreads();
    if (threadIdx.x == 0) m.n += tot;
    __syncthreads();
    if (m.n > kStageCap - kPathBlock) stage_flush(m, out, counter);
}

// Vertex-gradient accumulation through an LDS hash table.  The float64 scatter is bound by the
// chip's atomic rate (measured 22.6 G global_atomic_add_f64 per second, tools/ubench/atomic_scope.hip,
// independent of scope or per-XCD privatisation), and neighbouring rays hit neighbouring triangles
// that share vertices: a block first sums its contributions per vertex in LDS (ds_add_f64 after a
// compare-and-swap probe on the key) and then issues three global atomics per DISTINCT vertex.
#ifndef DRT_HASH_BITS
#define DRT_HASH_BITS 11
#endif
#ifndef DRT_BWD_BATCH
#define DRT_BWD_BATCH 1024
#endif
#ifndef DRT_BWD_BPC
#define DRT_BWD_BPC 2
#endif
constexpr int kHashBits = DRT_HASH_BITS, kHashSize = 1 << kHashBits;      // 2048 slots: 8 KB keys + 48 KB sums
constexpr int kBwdBatch = DRT_BWD_BATCH;                                 // rays per table fill (6 vertex refs each)

struct HashAdd3 {
    int32_t* keys;      // LDS [kHashSize]
    double* sums;       // LDS [kHashSize * 3]
    double* g;          // global fallback / final target
    __device__ __forceinline__ void operator()(int32_t v, d3 a) const {
        // slot = low bits of the vertex id: neighbouring slots then hold neighbouring ids, and the flush below walks the
        // table as flat doubles, so that a wave's atomics fall on runs of consecutive addresses -- see hash_flush
        unsigned h = (unsigned)v & (kHashSize - 1);
        // (ids come in runs of neighbours, and so do the occupied slots: a colliding id leaves the run in one odd stride that
        // depends on its high bits instead of walking through it slot by slot)
        const unsigned step = ((((unsigned)v >> kHashBits) << 1) + 97u) | 1u;
#pragma unroll 1
        for (int probe = 0; probe < 24; ++probe) {
            int32_t k = keys[h];
            if (k == -1) k = atomicCAS(&keys[h], -1, v);
            if (k == -1 || k == v) {
                __hip_atomic_fetch_add(&sums[3 * h + 0], a.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&sums[3 * h + 1], a.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&sums[3 * h + 2], a.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                return;
            }
            h = (h + step) & (kHashSize - 1);
        }
        AtomicAdd3{g}(v, a);     // table crowded: straight to memory
    }
};

__device__ __forceinline__ void hash_clear(int32_t* keys, double* sums) {
    for (int i = threadIdx.x; i < kHashSize; i += blockDim.x) keys[i] = -1;
    for (int i = threadIdx.x; i < 3 * kHashSize; i += blockDim.x) sums[i] = 0.0;
    __syncthreads();
}
__device__ __forceinline__ void hash_flush(int32_t* keys, double* sums, double* g) {
    __syncthreads();
    // The chip's atomic units work per cache-line REQUEST, not per lane (tools/ubench/atomic_pattern.hip: 23 G float64 atomics/s on
    // random addresses, 57 G/s when the 64 lanes of an instruction cover consecutive 24-byte rows, 141 G/s on 64 consecutive doubles).
    // With the table indexed by the low bits of the vertex id and the flush walking it as flat doubles (lane j -> component j % 3 of
    // slot j / 3), the vertices of a batch -- a compact patch of the surface, numbered by the mesher with some coherence -- give runs of
    // consecutive addresses: the backward kernel 0.33 -> 0.27 ms against a multiplicative hash flushed slot by slot.
    for (int j = threadIdx.x; j < 3 * kHashSize; j += blockDim.x) {
        const int32_t v = keys[j / 3];
        if (v >= 0) unsafeAtomicAdd(g + 3 * (int64_t)v + (j % 3), sums[j]);
    }
    __syncthreads();
}

// The same table for the deterministic mode (drt_fixed.h): the slots hold 128-bit fixed-point sums -- low and high words as two 64-bit
// integer LDS atomics, the carry owned by the addition that wrapped the low word -- and the flush adds each occupied slot to its FxCell in
// memory with two more.  Integer sums are exact, so WHICH contributions meet in a table (batch composition, probe order, overflow to
// memory) cannot change a bit of the result; the table only cuts the global atomics from 36 per path to 6 per distinct vertex and batch
// (measured round 6, 72 x 1024^2: without it the loss + gradient pass took 4.4 ms instead of 0.3).  Same LDS footprint as the float64
// table: half the slots, twice the bytes per sum.
constexpr int kFxHashSize = kHashSize / 2;
struct FxHashAdd3 {
    int32_t* keys;                    // LDS [kFxHashSize]
    unsigned long long* lo;           // LDS [3 * kFxHashSize]
    unsigned long long* hi;           // LDS [3 * kFxHashSize]
    double* g;                        // the FxCell array in memory
    __device__ __forceinline__ void operator()(int32_t v, d3 a) const {
        Fx128 t[3];
        const double comp[3] = {a.x, a.y, a.z};
        FxCell* cell = reinterpret_cast<FxCell*>(g) + 3 * (int64_t)v;
        bool any = false;
        for (int c = 0; c < 3; ++c) {
            const uint32_t f = fx_from_double(comp[c], t[c]);
            if (f) fx_atomic_add(cell + c, t[c], f);          // (rare: sticky flags go straight to memory; t[c] is zero then)
            any |= (t[c].hi | (int64_t)t[c].lo) != 0;
        }
        if (!any) return;
        unsigned h = (unsigned)v & (kFxHashSize - 1);
        const unsigned step = ((((unsigned)v >> (kHashBits - 1)) << 1) + 97u) | 1u;
#pragma unroll 1
        for (int probe = 0; probe < 24; ++probe) {
            int32_t k = keys[h];
            if (k == -1) k = atomicCAS(&keys[h], -1, v);
            if (k == -1 || k == v) {
                for (int c = 0; c < 3; ++c) {
                    if (!(t[c].hi | (int64_t)t[c].lo)) continue;
                    unsigned long long carry = 0;
                    if (t[c].lo) {
                        const unsigned long long old = atomicAdd(&lo[3 * h + c], (unsigned long long)t[c].lo);
                        carry = old + (unsigned long long)t[c].lo < old ? 1ull : 0ull;
                    }
                    const unsigned long long add_hi = (unsigned long long)t[c].hi + carry;
                    if (add_hi) atomicAdd(&hi[3 * h + c], add_hi);
                }
                return;
            }
            h = (h + step) & (kFxHashSize - 1);
        }
        for (int c = 0; c < 3; ++c) fx_atomic_add(cell + c, t[c], 0u);     // table crowded: straight to memory
    }
};
__device__ __forceinline__ void fx_hash_clear(int32_t* keys, unsigned long long* lo, unsigned long long* hi) {
    for (int i = threadIdx.x; i < kFxHashSize; i += blockDim.x) keys[i] = -1;
    for (int i = threadIdx.x; i < 3 * kFxHashSize; i += blockDim.x) { lo[i] = 0ull; hi[i] = 0ull; }
    __syncthreads();
}
__device__ __forceinline__ void fx_hash_flush(int32_t* keys, unsigned long long* lo, unsigned long long* hi, double* g) {
    __syncthreads();
    for (int j = threadIdx.x; j < 3 * kFxHashSize; j += blockDim.x) {
        const int32_t v = keys[j / 3];
        if (v >= 0) fx_atomic_add(reinterpret_cast<FxCell*>(g) + 3 * (int64_t)v + (j % 3), Fx128{(int64_t)hi[j], (uint64_t)lo[j]}, 0u);
    }
    __syncthreads();
}

// The vertex-gradient sink of the path kernels in the two accumulation modes (drt_device.h GradAdd3) over ONE block of LDS (keys [kHashSize]
// int32, sums [3 kHashSize] float64 -- or, deterministic, half as many slots of two 64-bit words): clear() before a batch, flush() after it.
template <bool DET>
struct PathSink {
    int32_t* keys;
    double* sums;
    double* g;
    __device__ __forceinline__ unsigned long long* lo() const { return reinterpret_cast<unsigned long long*>(sums); }
    __device__ __forceinline__ unsigned long long* hi() const { return reinterpret_cast<unsigned long long*>(sums) + 3 * kFxHashSize; }
    __device__ __forceinline__ void operator()(int32_t v, d3 a) const {
        if (DET) FxHashAdd3{keys, lo(), hi(), g}(v, a); else HashAdd3{keys, sums, g}(v, a);
    }
    __device__ __forceinline__ void clear() const { if (DET) fx_hash_clear(keys, lo(), hi()); else hash_clear(keys, sums); }
    __device__ __forceinline__ void flush() const { if (DET) fx_hash_flush(keys, lo(), hi(), g); else hash_flush(keys, sums, g); }
};

// The backward kernels of the K-interaction law (drt_paths.hip, drt_image_loss.hip).  A ray brings up to 3 * K vertex references (24 at
// K = 8, against 6 of the two-bounce path), so a table fill takes a quarter of k_render_bwd's rays.
constexpr int kPathsBwdBatch = 256;
// The sink of a call that wants no vertex gradient: the kernel has no table in LDS and the compiler drops the vertex chains of the adjoints.
struct DiscardAdd3 {
    __device__ __forceinline__ void operator()(int32_t, d3) const {}
};
// Element k of an IOR-gradient target in the two accumulation modes: float64, or, deterministic, an FxCell.
template <bool DET>
__device__ __forceinline__ double* ior_slot(double* ior, int k) {
    return DET ? reinterpret_cast<double*>(reinterpret_cast<FxCell*>(ior) + k) : ior + k;
}

// One pass of a gradient kernel over its list of n items (whole grid, whole blocks), body(k, add) per item k; the index type is n's.
// VERTS: the LDS table and its PathSink live here.  Block b takes the BATCH-sized batches b, b + gridDim.x, ...; thread t of a batch its
// items base + t, base + t + blockDim.x, ...; clear() before and flush() after every batch.  Without: no table, a grid-stride loop, and
// the body gets a DiscardAdd3 -- so a body written once, as a generic lambda, serves both.
template <bool DET, int BATCH, bool VERTS = true, typename Index, typename Body>
__device__ __forceinline__ void sink_pass(Index n, double* grad_verts, Body body) {
    if constexpr (VERTS) {
        __shared__ int32_t hkeys[kHashSize];
        __shared__ double hsums[3 * kHashSize];
        const PathSink<DET> add{hkeys, hsums, grad_verts};
        for (Index base = blockIdx.x * (Index)BATCH; base < n; base += (Index)gridDim.x * BATCH) {
            add.clear();
            const Index end = base + BATCH < n ? base + BATCH : n;
            for (Index k = base + threadIdx.x; k < end; k += blockDim.x) body(k, add);
            add.flush();
        }
    } else {
        for (Index k = blockIdx.x * (Index)blockDim.x + threadIdx.x; k < n; k += (Index)gridDim.x * blockDim.x) body(k, DiscardAdd3{});
    }
}
