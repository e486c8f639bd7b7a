// drt_pathws.h -- what the translation units that run the K-interaction wavefront loop share (drt_paths.hip: the path calls; drt_image.hip:
// the forward renderer): the workspace behind drt_scene::paths_ws, the per-ray state byte, the counter block and the block runs that keep
// a staged append in input order.
#pragma once
#include "drt_device.h"
#include "drt_paths.h"

// per-ray state byte while a call is in flight: refractions made so far (<= 8) | kPathDone once the path has ended valid
constexpr uint8_t kPathDone = 0x80;
// words of the counter block: sizes of lists 0 .. K, the second-pass counts of the K + 1 traversals, k_trace's retired-workgroup counter,
// the number of valid rays
constexpr int kCntList = 0, kCntRedo = 16, kCntDone = 32, kCntValid = 33, kCntWords = 40;
static_assert(kMaxBounces + 1 <= kCntRedo - kCntList && kMaxBounces + 1 <= kCntDone - kCntRedo, "counter block layout");

struct PathsWs {
    int64_t cap = 0;
    int32_t* idx[2] = {nullptr, nullptr};
    float* ray[2] = {nullptr, nullptr};
    int32_t* face[2] = {nullptr, nullptr};
    int32_t* redo = nullptr;
    uint8_t* state = nullptr;
    unsigned* cnt = nullptr;
    int32_t* slow_stack = nullptr;       // overflow area of k_trace's second pass: [kPathBlock * kStackSlowDev]
    // the one-pass form only (ensure_paths_fused_ws): float64 ray in flight [2][fused_cap,3], face tape [kMaxBounces, fused_cap], hit counts
    int64_t fused_cap = 0;
    double* park = nullptr;
    int32_t* tape = nullptr;
    uint8_t* hits = nullptr;
    // the forward renderer only (drt_image.hip), beside the rows of the one-pass form: one float64 throughput per sample
    int64_t thr_cap = 0;
    double* thr = nullptr;
};

// each block takes one contiguous run of [0, n), so that what it appends stays in input order
__device__ __forceinline__ void block_run(unsigned n, unsigned& first, unsigned& last) {
    const unsigned per_block = ((n + gridDim.x - 1) / gridDim.x + kPathBlock - 1) / kPathBlock * kPathBlock;
    first = blockIdx.x * per_block;
    last = min(n, first + per_block);
    if (first > last) first = last;
}

inline PathsWs* paths_ws_of(drt_scene* s) { return static_cast<PathsWs*>(s->paths_ws); }
// defined in drt_paths.hip: the ray lists, grown to n entries (never inside a stream capture).  `who`: the entry point, for messages.
int ensure_paths_ws(drt_scene* s, int64_t n, hipStream_t st, const char* who);
// ... and the workspace rows of the one-pass form (parked float64 rays, face tape, hit counts); needs ensure_paths_ws first
int ensure_paths_fused_ws(drt_scene* s, int64_t n, hipStream_t st, const char* who);
