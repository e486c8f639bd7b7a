// drt_pathws.h -- what the translation units that run the K-interaction wavefront loop share (drt_paths.hip: the path calls; drt_image.hip:
// the forward wavefront of the refracted image; drt_image_loss.hip: its loss): the workspace behind drt_scene::paths_ws, the per-ray state
// byte, the counter block, the block runs that keep a staged append in input order, the pass loop and the launcher of k_paths_collect.
#pragma once
#include "drt_device.h"
#include "drt_trace_kernel.h"
#include "drt_pathsink.h"
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
    // the forward wavefront of the image only (drt_image.hip image_forward), beside the rows of the one-pass form: one float64 throughput per sample
    int64_t thr_cap = 0;
    double* thr = nullptr;
    // ... and, under absorption only (drt_image_absorb.hip), one float64 interior length per sample, grown like the throughputs
    int64_t len_cap = 0;
    double* len = nullptr;
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
// defined in drt_paths.hip: k_paths_collect -- the rays whose state byte says that the path completed -> index list done_idx, its size in *n_done
void launch_paths_collect(int grid, hipStream_t st, unsigned n, const uint8_t* state, int32_t* done_idx, unsigned* n_done);

// The wavefront loop behind list 0: trace list k (closest hit; any hit at k = K, where every interaction is used up), shade it into list
// k + 1 (the other ping-pong buffer), K + 1 times.  shade(k, in, n_in, out, n_out) launches the caller's shade kernel of round k on `st`.
template <typename Shade>
inline void trace_lists(const drt_scene* s, const PathsWs& w, const TraceCtx& tc, hipStream_t st, int max_bounces, Shade shade) {
    const RayList l0{w.idx[0], w.ray[0], w.face[0]}, l1{w.idx[1], w.ray[1], w.face[1]};
    for (int k = 0; k <= max_bounces; ++k) {
        const RayList& in = (k & 1) ? l1 : l0;
        const RayList& out = (k & 1) ? l0 : l1;
        launch_trace_list(k < max_bounces ? kTraceClosest : kTraceAny, s->grid_path, st, tc, in.ray, w.cnt + kCntList + k,
                          TraceOut{in.face, nullptr, nullptr, nullptr}, w.redo, w.cnt + kCntRedo + k, w.cnt + kCntDone, s->refill_min, s->inner_min, nullptr);
        shade(k, in, w.cnt + kCntList + k, out, w.cnt + kCntList + k + 1);
    }
}
