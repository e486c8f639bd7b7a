// drt_paths.hip -- refraction paths of up to K surface interactions with optional internal reflection (drt_paths.h: the law) as a
// wavefront loop over compact ray lists, and their backward.
//
//   k_paths_start   all rays : top-box test; candidates -> list 0 (index + float32 ray), their float64 ray parked in rows of out_ori / out_dir
//   per interaction k = 0 .. K:
//     k_trace       list k   : closest hit (k < K) or any hit (k = K: every interaction is used up) -> face per list slot
//     k_paths_shade list k   : miss -> the path ends (valid iff an even, non-zero number of refractions); hit -> face into the tape,
//                              float64 bounce_forward / bounce_reflect on the parked ray, survivors -> list k + 1 (the other ping-pong buffer)
//   k_paths_finish  all rays : dead values on invalid rows, valid rows -> the list the backward walks
// The float64 state of a ray in flight lives in ITS rows of out_ori / out_dir (as k_shade2's `parked` mode of the two-bounce pipeline), so
// the exit ray of a completed path is in place when the path ends.  Every list size stays on the device, grids are sized from N, and all
// launches go to the caller's stream: the call can be captured in a hipGraph.  k_trace is the two-bounce pipeline's (launch_trace_list,
// instantiated in drt_trace.hip); the staged list append and the gradient sink are shared with it (drt_pathsink.h).
//
// The one-pass form (drt_render_paths_ray_loss_fused: loss + vertex gradient of one view, nothing dense written) runs the same loop with
// the ray in flight, the face tape and the hit counts in the scene's workspace instead of caller tensors:
//   k_paths_start_fused all rays : as k_paths_start, but a ray without a target is no candidate; one state byte per ray, nothing else
//   k_trace / k_paths_shade      : unchanged (they are handed the workspace rows)
//   k_paths_collect     all rays : reads the state byte, completed paths -> index list
//   k_paths_loss_bwd    that list: ray_loss term on the parked exit ray + adjoint (path_loss_backward_k), LossAcc / PathSink
//   k_paths_loss_bwd_ior that list: in place of k_paths_loss_bwd when the IOR partials are asked for (drt_render_paths_law_ray_loss_ior_fused);
//                                 VERTS = false: no vertex gradient, no table in LDS
// The tape needs no -1 preset there: hits[i], written with the last face of a path, bounds what the last kernel reads.
#include "drt_device.h"
#include "drt_trace_kernel.h"
#include "drt_pathsink.h"
#include "drt_paths.h"
#include "drt_pathws.h"

__global__ void __launch_bounds__(kPathBlock) k_paths_start(const Node4Q* __restrict__ nodes, int n_tris, const double* __restrict__ origin,
                                                             const double* __restrict__ dir, unsigned n, double* __restrict__ out_ori,
                                                             double* __restrict__ out_dir, uint8_t* __restrict__ state, uint8_t* __restrict__ hits,
                                                             RayList out, unsigned* count) {
    __shared__ StageMem stage;
    stage_init(stage);
    unsigned first, last;
    block_run(n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned i = base + threadIdx.x;
        bool cand = false;
        f3 o32{0.f, 0.f, 0.f}, d32{0.f, 0.f, 1.f};
        if (i < n) {
            const d3 o = load_d3(origin, i), d = load_d3(dir, i);
            o32 = to_f32(o); d32 = to_f32(d);
            cand = n_tris > 0 && hits_top_boxes(nodes, o32, d32);
            state[i] = 0;
            hits[i] = 0;
            if (cand) { store_d3(out_ori, i, o); store_d3(out_dir, i, d); }
        }
        stage_push(stage, cand, (int32_t)i, o32, d32, out, count);
    }
    stage_flush(stage, out, count);
}

// k_paths_start of the one-pass form: a ray without a target cannot contribute and is never traced; the float64 ray parks in the workspace;
// per camera ray one state byte is written and origin / dir / valid are read once.
__global__ void __launch_bounds__(kPathBlock) k_paths_start_fused(const Node4Q* __restrict__ nodes, int n_tris, const double* __restrict__ origin,
                                                                   const double* __restrict__ dir, const uint8_t* __restrict__ valid, unsigned n,
                                                                   double* __restrict__ park_ori, double* __restrict__ park_dir,
                                                                   uint8_t* __restrict__ state, RayList out, unsigned* count) {
    __shared__ StageMem stage;
    stage_init(stage);
    unsigned first, last;
    block_run(n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned i = base + threadIdx.x;
        bool cand = false;
        f3 o32{0.f, 0.f, 0.f}, d32{0.f, 0.f, 1.f};
        if (i < n) {
            state[i] = 0;
            if (n_tris > 0 && valid[i]) {
                const d3 o = load_d3(origin, i), d = load_d3(dir, i);
                o32 = to_f32(o); d32 = to_f32(d);
                cand = hits_top_boxes(nodes, o32, d32);
                if (cand) { store_d3(park_ori, i, o); store_d3(park_dir, i, d); }
            }
        }
        stage_push(stage, cand, (int32_t)i, o32, d32, out, count);
    }
    stage_flush(stage, out, count);
}

// list k -> list k + 1.  k == max_bounces: every interaction is used up, the list was traced in the any-hit form and nothing continues.
// SNELL (here and in the two backward kernels): the refraction formula of the law (drt_paths.h), chosen on the host per launch.
template <bool SNELL>
__global__ void __launch_bounds__(kPathBlock) k_paths_shade(PathCtx c, int64_t n_rays, int k, int max_bounces, bool reflect, RayList in,
                                                             const unsigned* __restrict__ n_in, RayList out, unsigned* n_out,
                                                             double* __restrict__ out_ori, double* __restrict__ out_dir,
                                                             uint8_t* __restrict__ state, uint8_t* __restrict__ hits, int32_t* __restrict__ tape) {
    __shared__ StageMem stage;
    stage_init(stage);
    const unsigned n = *n_in;
    const bool last_stage = k >= max_bounces;
    unsigned first, last;
    block_run(n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned e = base + threadIdx.x;
        bool go = false;
        int64_t i = 0;
        f3 o32{0.f, 0.f, 0.f}, d32{0.f, 0.f, 1.f};
        if (e < n) {
            i = in.idx[e];
            const int32_t f = in.face[e];
            if (i >= 0 && i < n_rays) {
                int n_refr = state[i];
                if (f < 0) {
                    if (path_exit_valid(n_refr)) state[i] = (uint8_t)n_refr | kPathDone;
                } else if (!last_stage) {
                    tape[(int64_t)k * n_rays + i] = f;
                    hits[i] = (uint8_t)(k + 1);
                    d3 o = load_d3(out_ori, i), d = load_d3(out_dir, i);
                    go = path_interact<SNELL>(c, f, reflect, o, d, n_refr);
                    if (go) {
                        store_d3(out_ori, i, o); store_d3(out_dir, i, d);
                        state[i] = (uint8_t)n_refr;
                        o32 = to_f32(o); d32 = to_f32(d);
                    }
                }
            }
        }
        if (!last_stage) stage_push(stage, go, (int32_t)i, o32, d32, out, n_out);
    }
    if (!last_stage) stage_flush(stage, out, n_out);
}

// Dead values on the rows whose path did not complete (their rows may hold a parked ray), flags on the others, valid rows -> valid_idx.
__global__ void __launch_bounds__(kPathBlock) k_paths_finish(unsigned n, double* __restrict__ out_ori, double* __restrict__ out_dir, uint8_t* __restrict__ mask,
                                                              const uint8_t* __restrict__ state, uint8_t* __restrict__ hits, int32_t* __restrict__ valid_idx,
                                                              unsigned* n_valid) {
    __shared__ StageMem stage;
    stage_init(stage);
    const RayList out{valid_idx, nullptr, nullptr};              // index-only list
    unsigned first, last;
    block_run(n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned i = base + threadIdx.x;
        bool keep = false;
        if (i < n) {
            keep = (state[i] & kPathDone) != 0;
            const uint8_t m = keep ? 1 : 0;
            mask[3 * (int64_t)i] = m; mask[3 * (int64_t)i + 1] = m; mask[3 * (int64_t)i + 2] = m;
            if (!keep) {
                const d3 z{0.0, 0.0, 0.0};
                store_d3(out_ori, i, z);
                store_d3(out_dir, i, z);
                hits[i] = 0;
            }
        }
        stage_push(stage, keep, (int32_t)i, f3{0.f, 0.f, 0.f}, f3{0.f, 0.f, 0.f}, out, n_valid);
    }
    stage_flush(stage, out, n_valid);
}

__global__ void k_paths_count(const unsigned* __restrict__ count, int64_t* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out = (int64_t)*count;
}

// Backward over the list of valid rays: recompute every interaction from the camera ray and the face tape, reverse, scatter the vertex
// gradients through the LDS hash sink, kPathsBwdBatch rays per table fill (drt_pathsink.h); neighbouring rays still share most of their
// vertices.
template <bool DET, bool SNELL>
__global__ void __launch_bounds__(256) k_paths_bwd(PathCtx c, const double* __restrict__ origin, const double* __restrict__ dir, int64_t n_rays,
                                                   int max_bounces, const int32_t* __restrict__ tape, const uint8_t* __restrict__ hits,
                                                   const double* __restrict__ g_out_ori, const double* __restrict__ g_out_dir, double* grad_verts,
                                                   const int32_t* __restrict__ list, const int64_t* __restrict__ n_list) {
    int64_t n = *n_list;
    if (n > n_rays) n = n_rays;
    sink_pass<DET, kPathsBwdBatch>(n, grad_verts, [&](int64_t k, const PathSink<DET>& add) {
        const int64_t i = list[k];
        if (i < 0 || i >= n_rays) return;
        const d3 z{0.0, 0.0, 0.0};
        const d3 g_ori = g_out_ori ? load_d3(g_out_ori, i) : z;
        const d3 g_dir = g_out_dir ? load_d3(g_out_dir, i) : z;
        path_recompute_backward_k<SNELL>(c, load_d3(origin, i), load_d3(dir, i), tape + i, n_rays, min((int)hits[i], max_bounces), g_ori, g_dir, add);
    });
}

// The one-pass form: the rays whose path completed (state byte) -> index list; order does not matter to the sums.
__global__ void __launch_bounds__(kPathBlock) k_paths_collect(unsigned n, const uint8_t* __restrict__ state, int32_t* __restrict__ done_idx, unsigned* n_done) {
    __shared__ StageMem stage;
    stage_init(stage);
    const RayList out{done_idx, nullptr, nullptr};              // index-only list
    unsigned first, last;
    block_run(n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned i = base + threadIdx.x;
        const bool keep = i < n && (state[i] & kPathDone) != 0;
        stage_push(stage, keep, (int32_t)i, f3{0.f, 0.f, 0.f}, f3{0.f, 0.f, 0.f}, out, n_done);
    }
    stage_flush(stage, out, n_done);
}

// Loss AND vertex gradient (unit seed) over the list of completed paths: the ray_loss term on the exit ray the forward parked -- the bits a
// recompute would give -- then recompute, reverse, scatter as k_paths_bwd does (same table fill).  Every listed ray has a target:
// k_paths_start_fused admits no other.
template <bool DET, bool SNELL>
__global__ void __launch_bounds__(256) k_paths_loss_bwd(PathCtx c, const double* __restrict__ origin, const double* __restrict__ dir,
                                                        const double* __restrict__ screen_pixel, int64_t n_rays, int max_bounces,
                                                        const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                        const int32_t* __restrict__ tape, const uint8_t* __restrict__ hits,
                                                        const int32_t* __restrict__ list, const unsigned* __restrict__ n_list, double* loss,
                                                        double* grad_verts, unsigned long long* n_valid) {
    int64_t n = *n_list;
    if (n > n_rays) n = n_rays;
    LossAcc<DET> acc;
    unsigned cnt = 0;
    sink_pass<DET, kPathsBwdBatch>(n, grad_verts, [&](int64_t k, const PathSink<DET>& add) {
        const int64_t i = list[k];
        if (i < 0 || i >= n_rays) return;
        acc.add(path_loss_backward_k<SNELL>(c, load_d3(origin, i), load_d3(dir, i), tape + i, n_rays, min((int)hits[i], max_bounces),
                                     load_d3(park_ori, i), load_d3(park_dir, i), load_d3(screen_pixel, i), add));
        ++cnt;
    });
    acc.flush(loss);
    if (n_valid && cnt) atomicAdd(n_valid, (unsigned long long)cnt);
}

// k_paths_loss_bwd that also sums d loss / d (ior_int, ior_ext) (path_loss_backward_ior_k): two more LossAcc, summed per
// thread and per wave and flushed with one atomic per wave into grad_ior[0] / [1] -- float64, or, deterministic, two FxCells (exact, as the
// loss).  VERTS = false is the calibration mode of a fixed mesh: no vertex gradient is wanted, `add` discards, the kernel has no table in
// LDS and the compiler drops the vertex chains of the adjoints.
template <bool DET, bool SNELL, bool VERTS>
__global__ void __launch_bounds__(256) k_paths_loss_bwd_ior(PathCtx c, const double* __restrict__ origin, const double* __restrict__ dir,
                                                            const double* __restrict__ screen_pixel, int64_t n_rays, int max_bounces,
                                                            const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                            const int32_t* __restrict__ tape, const uint8_t* __restrict__ hits,
                                                            const int32_t* __restrict__ list, const unsigned* __restrict__ n_list, double* loss,
                                                            double* grad_verts, double* grad_ior, unsigned long long* n_valid) {
    int64_t n = *n_list;
    if (n > n_rays) n = n_rays;
    LossAcc<DET> acc, acc_int, acc_ext;
    unsigned cnt = 0;
    sink_pass<DET, kPathsBwdBatch, VERTS>(n, grad_verts, [&](int64_t k, auto add) {
        const int64_t i = list[k];
        if (i < 0 || i >= n_rays) return;
        double gi, ge;
        acc.add(path_loss_backward_ior_k<SNELL>(c, load_d3(origin, i), load_d3(dir, i), tape + i, n_rays, min((int)hits[i], max_bounces),
                                                load_d3(park_ori, i), load_d3(park_dir, i), load_d3(screen_pixel, i), add, gi, ge));
        acc_int.add(gi); acc_ext.add(ge);
        ++cnt;
    });
    acc.flush(loss);
    acc_int.flush(ior_slot<DET>(grad_ior, 0));
    acc_ext.flush(ior_slot<DET>(grad_ior, 1));
    if (n_valid && cnt) atomicAdd(n_valid, (unsigned long long)cnt);
}

static PathsWs* ws_of(drt_scene* s) { return paths_ws_of(s); }

int ensure_paths_ws(drt_scene* s, int64_t n, hipStream_t st, const char* who) {
    PathsWs* w = ws_of(s);
    if (w && n <= w->cap) return DRT_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(DRT_E_INVALID, "%s: the first call of this size allocates its ray lists and cannot run inside a stream "
                                   "capture: issue one such call eagerly before capturing", who);
    if (!w) {
        w = new (std::nothrow) PathsWs();
        if (!w) return fail(DRT_E_NOMEM, "host allocation failed");
        s->paths_ws = w;
        HIP_TRY(hipMalloc(&w->cnt, sizeof(unsigned) * kCntWords));
        HIP_TRY(hipMalloc(&w->slow_stack, sizeof(int32_t) * (size_t)kPathBlock * kStackSlowDev));
    }
    for (int k = 0; k < 2; ++k) {
        (void)hipFree(w->idx[k]); (void)hipFree(w->ray[k]); (void)hipFree(w->face[k]);
        w->idx[k] = nullptr; w->ray[k] = nullptr; w->face[k] = nullptr;
    }
    (void)hipFree(w->redo); (void)hipFree(w->state);
    w->redo = nullptr; w->state = nullptr; w->cap = 0;
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipMalloc(&w->idx[k], sizeof(int32_t) * n));
        HIP_TRY(hipMalloc(&w->ray[k], sizeof(float) * 6 * n));
        HIP_TRY(hipMalloc(&w->face[k], sizeof(int32_t) * n));
    }
    HIP_TRY(hipMalloc(&w->redo, sizeof(int32_t) * n));
    HIP_TRY(hipMalloc(&w->state, (size_t)n));
    w->cap = n;
    return DRT_OK;
}

// the workspace rows of the one-pass form, grown like the ray lists
int ensure_paths_fused_ws(drt_scene* s, int64_t n, hipStream_t st, const char* who) {
    PathsWs* w = ws_of(s);
    if (n <= w->fused_cap) return DRT_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(DRT_E_INVALID, "%s: the first call of this size allocates its parked rays and face tape and cannot "
                                   "run inside a stream capture: issue one such call eagerly before capturing", who);
    (void)hipFree(w->park); (void)hipFree(w->tape); (void)hipFree(w->hits);
    w->park = nullptr; w->tape = nullptr; w->hits = nullptr; w->fused_cap = 0;
    HIP_TRY(hipMalloc(&w->park, sizeof(double) * 6 * (size_t)n));
    HIP_TRY(hipMalloc(&w->tape, sizeof(int32_t) * (size_t)kMaxBounces * (size_t)n));
    HIP_TRY(hipMalloc(&w->hits, (size_t)n));
    w->fused_cap = n;
    return DRT_OK;
}

static int check_law(int max_bounces, int reflect) {
    if (max_bounces < 2 || max_bounces > kMaxBounces) return fail(DRT_E_INVALID, "max_bounces = %d: must be 2 .. %d", max_bounces, kMaxBounces);
    if (reflect != 0 && reflect != 1) return fail(DRT_E_INVALID, "reflect = %d: must be 0 (a TIR hit ends the path) or 1 (the ray is mirrored)", reflect);
    return DRT_OK;
}

// law_flags of the drt_render_paths_law_* entry points (include/drt_hip.h: DRT_LAW_REFLECT | DRT_LAW_SNELL)
static int check_law_flags(int max_bounces, int law_flags) {
    if (max_bounces < 2 || max_bounces > kMaxBounces) return fail(DRT_E_INVALID, "max_bounces = %d: must be 2 .. %d", max_bounces, kMaxBounces);
    if (law_flags & ~(DRT_LAW_REFLECT | DRT_LAW_SNELL))
        return fail(DRT_E_INVALID, "law_flags = %d: must be a combination of DRT_LAW_REFLECT (%d) and DRT_LAW_SNELL (%d)", law_flags,
                    DRT_LAW_REFLECT, DRT_LAW_SNELL);
    return DRT_OK;
}

// DET_LAUNCH for the kernels whose second template parameter is the refraction formula of the law
#define DET_LAW_LAUNCH(kern, snell, grid, block, st, ...)                                 \
    do {                                                                                  \
        const bool det_ = det_mode();                                                     \
        if (snell) {                                                                      \
            if (det_) kern<true, true><<<grid, block, 0, st>>>(__VA_ARGS__);              \
            else kern<false, true><<<grid, block, 0, st>>>(__VA_ARGS__);                  \
        } else {                                                                          \
            if (det_) kern<true, false><<<grid, block, 0, st>>>(__VA_ARGS__);             \
            else kern<false, false><<<grid, block, 0, st>>>(__VA_ARGS__);                 \
        }                                                                                 \
    } while (0)

// ... and for k_paths_loss_bwd_ior, whose third is whether the vertex gradient is computed.  Without the table the calibration mode is
// limited by its registers: kPathsIorBpc blocks per CU fill the waves the compiler's report allows.
constexpr int kPathsIorBpc = 4;
#define DET_LAW_VERTS_LAUNCH(kern, snell, verts, grid, block, st, ...)                    \
    do {                                                                                  \
        const bool det_ = det_mode();                                                     \
        const int sel_ = (det_ ? 4 : 0) | ((snell) ? 2 : 0) | ((verts) ? 1 : 0);          \
        switch (sel_) {                                                                   \
        case 0: kern<false, false, false><<<grid, block, 0, st>>>(__VA_ARGS__); break;    \
        case 1: kern<false, false, true><<<grid, block, 0, st>>>(__VA_ARGS__); break;     \
        case 2: kern<false, true, false><<<grid, block, 0, st>>>(__VA_ARGS__); break;     \
        case 3: kern<false, true, true><<<grid, block, 0, st>>>(__VA_ARGS__); break;      \
        case 4: kern<true, false, false><<<grid, block, 0, st>>>(__VA_ARGS__); break;     \
        case 5: kern<true, false, true><<<grid, block, 0, st>>>(__VA_ARGS__); break;      \
        case 6: kern<true, true, false><<<grid, block, 0, st>>>(__VA_ARGS__); break;      \
        default: kern<true, true, true><<<grid, block, 0, st>>>(__VA_ARGS__); break;      \
        }                                                                                 \
    } while (0)

void paths_free(drt_scene* s) {
    PathsWs* w = ws_of(s);
    if (!w) return;
    for (int k = 0; k < 2; ++k) { (void)hipFree(w->idx[k]); (void)hipFree(w->ray[k]); (void)hipFree(w->face[k]); }
    (void)hipFree(w->redo); (void)hipFree(w->state); (void)hipFree(w->cnt); (void)hipFree(w->slow_stack);
    (void)hipFree(w->park); (void)hipFree(w->tape); (void)hipFree(w->hits);
    (void)hipFree(w->thr);
    (void)hipFree(w->len);
    delete w;
    s->paths_ws = nullptr;
}

// The pass loop (drt_pathws.h trace_lists) with k_paths_shade.  ray_ori / ray_dir [N,3]: the rows the float64 ray in flight parks in;
// hits [N], tape [K,N]: written per list item.
static void paths_rounds(drt_scene* s, const PathsWs& w, const PathCtx& pc, hipStream_t st, int gs, int64_t n_rays, int max_bounces, bool reflect,
                         bool snell, double* ray_ori, double* ray_dir, uint8_t* hits, int32_t* tape) {
    trace_lists(s, w, pc.tc, st, max_bounces, [&](int k, const RayList& in, const unsigned* n_in, const RayList& out, unsigned* n_out) {
        if (snell)
            k_paths_shade<true><<<gs, kPathBlock, 0, st>>>(pc, n_rays, k, max_bounces, reflect, in, n_in, out, n_out, ray_ori, ray_dir, w.state, hits, tape);
        else
            k_paths_shade<false><<<gs, kPathBlock, 0, st>>>(pc, n_rays, k, max_bounces, reflect, in, n_in, out, n_out, ray_ori, ray_dir, w.state, hits, tape);
    });
}

void launch_paths_collect(int grid, hipStream_t st, unsigned n, const uint8_t* state, int32_t* done_idx, unsigned* n_done) {
    k_paths_collect<<<grid, kPathBlock, 0, st>>>(n, state, done_idx, n_done);
}

// The bodies behind the entry points; the law has been checked.  `who`: the entry point, for messages.
static int paths_forward(drt_scene* s, const double* d_verts, const double* d_origin, const double* d_dir, int64_t n_rays,
                         double ior_int, double ior_ext, int max_bounces, bool reflect, bool snell,
                         double* d_out_ori, double* d_out_dir, uint8_t* d_mask, int32_t* d_tape, uint8_t* d_hits,
                         int32_t* d_valid_idx, int64_t* d_n_valid, void* stream, const char* who) {
    if (n_rays < 0 || n_rays > INT32_MAX) return fail(DRT_E_INVALID, "ray count out of range");
    hipStream_t st = (hipStream_t)stream;
    if (n_rays == 0) {
        if (d_n_valid) HIP_TRY(hipMemsetAsync(d_n_valid, 0, sizeof(int64_t), st));
        return DRT_OK;
    }
    if (!d_verts || !d_origin || !d_dir || !d_out_ori || !d_out_dir || !d_mask || !d_tape || !d_hits || !d_valid_idx || !d_n_valid)
        return fail(DRT_E_INVALID, "null pointer argument");
    { int rc = ensure_paths_ws(s, n_rays, st, who); if (rc) return rc; }
    { int rc = wait_build(s, st); if (rc) return rc; }
    const PathsWs& w = *ws_of(s);
    PathCtx pc = path_ctx(s, d_verts, ior_int, ior_ext);
    pc.tc.slow_stack = w.slow_stack;
    const unsigned n = (unsigned)n_rays;
    const int gs = grid_for(n_rays, kPathBlock, 8 * s->n_cu);
    HIP_TRY(hipMemsetAsync(w.cnt, 0, sizeof(unsigned) * kCntWords, st));
    HIP_TRY(hipMemsetAsync(d_tape, 0xFF, sizeof(int32_t) * (size_t)max_bounces * (size_t)n_rays, st));
    const RayList l0{w.idx[0], w.ray[0], w.face[0]};
    k_paths_start<<<gs, kPathBlock, 0, st>>>(pc.tc.nodes, pc.tc.n_tris, d_origin, d_dir, n, d_out_ori, d_out_dir, w.state, d_hits, l0, w.cnt + kCntList);
    paths_rounds(s, w, pc, st, gs, n_rays, max_bounces, reflect, snell, d_out_ori, d_out_dir, d_hits, d_tape);
    k_paths_finish<<<gs, kPathBlock, 0, st>>>(n, d_out_ori, d_out_dir, d_mask, w.state, d_hits, d_valid_idx, w.cnt + kCntValid);
    k_paths_count<<<1, 64, 0, st>>>(w.cnt + kCntValid, d_n_valid);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

static int paths_backward(drt_scene* s, const double* d_verts, const double* d_origin, const double* d_dir, int64_t n_rays,
                          double ior_int, double ior_ext, int max_bounces, bool snell,
                          const int32_t* d_tape, const uint8_t* d_hits, const int32_t* d_valid_idx, const int64_t* d_n_valid,
                          const double* d_grad_out_ori, const double* d_grad_out_dir, double* d_grad_verts, void* stream) {
    if (n_rays < 0 || n_rays > INT32_MAX) return fail(DRT_E_INVALID, "ray count out of range");
    if (n_rays == 0 || (!d_grad_out_ori && !d_grad_out_dir)) return DRT_OK;
    if (!d_verts || !d_origin || !d_dir || !d_tape || !d_hits || !d_valid_idx || !d_n_valid || !d_grad_verts) return fail(DRT_E_INVALID, "null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    const PathCtx pc = path_ctx(s, d_verts, ior_int, ior_ext);
    DET_LAW_LAUNCH(k_paths_bwd, snell, DRT_BWD_BPC * s->n_cu, 256, st, pc, d_origin, d_dir, n_rays, max_bounces, d_tape, d_hits, d_grad_out_ori, d_grad_out_dir, d_grad_verts,
               d_valid_idx, d_n_valid);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

static int paths_ray_loss_fused(drt_scene* s, const double* d_verts, const double* d_origin, const double* d_dir,
                                const double* d_screen_pixel, const uint8_t* d_valid, int64_t n_rays, double ior_int, double ior_ext,
                                int max_bounces, bool reflect, bool snell, double* d_loss, double* d_grad_verts, double* d_grad_ior,
                                int64_t* d_n_valid, void* stream, const char* who) {
    if (n_rays < 0 || n_rays > INT32_MAX) return fail(DRT_E_INVALID, "ray count out of range");
    if (n_rays == 0) return DRT_OK;
    // (d_grad_ior: the call that also differentiates the IORs, k_paths_loss_bwd_ior; only there may the vertex gradient be left out)
    if (!d_verts || !d_origin || !d_dir || !d_screen_pixel || !d_valid || !d_loss || (!d_grad_verts && !d_grad_ior)) return fail(DRT_E_INVALID, "null pointer argument");
    hipStream_t st = (hipStream_t)stream;
    { int rc = ensure_paths_ws(s, n_rays, st, who); if (rc) return rc; }
    { int rc = ensure_paths_fused_ws(s, n_rays, st, who); if (rc) return rc; }
    { int rc = wait_build(s, st); if (rc) return rc; }
    const PathsWs& w = *ws_of(s);
    PathCtx pc = path_ctx(s, d_verts, ior_int, ior_ext);
    pc.tc.slow_stack = w.slow_stack;
    const unsigned n = (unsigned)n_rays;
    const int gs = grid_for(n_rays, kPathBlock, 8 * s->n_cu);
    double* const park_ori = w.park;
    double* const park_dir = w.park + 3 * w.fused_cap;
    HIP_TRY(hipMemsetAsync(w.cnt, 0, sizeof(unsigned) * kCntWords, st));
    const RayList l0{w.idx[0], w.ray[0], w.face[0]};
    k_paths_start_fused<<<gs, kPathBlock, 0, st>>>(pc.tc.nodes, pc.tc.n_tris, d_origin, d_dir, d_valid, n, park_ori, park_dir, w.state, l0, w.cnt + kCntList);
    paths_rounds(s, w, pc, st, gs, n_rays, max_bounces, reflect, snell, park_ori, park_dir, w.hits, w.tape);
    int32_t* const done = w.idx[0];          // (both ping-pong lists are free once the loop has ended)
    launch_paths_collect(gs, st, n, w.state, done, w.cnt + kCntValid);
    if (d_grad_ior)
        DET_LAW_VERTS_LAUNCH(k_paths_loss_bwd_ior, snell, d_grad_verts != nullptr, (d_grad_verts ? DRT_BWD_BPC : kPathsIorBpc) * s->n_cu, 256, st, pc, d_origin, d_dir,
                             d_screen_pixel, n_rays, max_bounces, park_ori, park_dir, w.tape, w.hits, done, w.cnt + kCntValid, d_loss, d_grad_verts, d_grad_ior,
                             reinterpret_cast<unsigned long long*>(d_n_valid));
    else
        DET_LAW_LAUNCH(k_paths_loss_bwd, snell, DRT_BWD_BPC * s->n_cu, 256, st, pc, d_origin, d_dir, d_screen_pixel, n_rays, max_bounces, park_ori, park_dir, w.tape, w.hits,
                       done, w.cnt + kCntValid, d_loss, d_grad_verts, reinterpret_cast<unsigned long long*>(d_n_valid));
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

extern "C" {

int drt_render_paths_forward(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir, int64_t n_rays,
                             double ior_int, double ior_ext, int max_bounces, int reflect,
                             double* d_out_ori, double* d_out_dir, uint8_t* d_mask, int32_t* d_tape, uint8_t* d_hits,
                             int32_t* d_valid_idx, int64_t* d_n_valid, void* stream) {
    CHECK_BUILT(s);
    { int rc = check_law(max_bounces, reflect); if (rc) return rc; }
    return paths_forward(s, d_verts, d_origin, d_dir, n_rays, ior_int, ior_ext, max_bounces, reflect != 0, false, d_out_ori, d_out_dir, d_mask,
                         d_tape, d_hits, d_valid_idx, d_n_valid, stream, "drt_render_paths_forward");
}

int drt_render_paths_backward(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir, int64_t n_rays,
                              double ior_int, double ior_ext, int max_bounces, int reflect,
                              const int32_t* d_tape, const uint8_t* d_hits, const int32_t* d_valid_idx, const int64_t* d_n_valid,
                              const double* d_grad_out_ori, const double* d_grad_out_dir, double* d_grad_verts, void* stream) {
    CHECK_BUILT(s);
    { int rc = check_law(max_bounces, reflect); if (rc) return rc; }
    return paths_backward(s, d_verts, d_origin, d_dir, n_rays, ior_int, ior_ext, max_bounces, false, d_tape, d_hits, d_valid_idx, d_n_valid,
                          d_grad_out_ori, d_grad_out_dir, d_grad_verts, stream);
}

int drt_render_paths_ray_loss_fused(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir,
                                    const double* d_screen_pixel, const uint8_t* d_valid, int64_t n_rays, double ior_int, double ior_ext,
                                    int max_bounces, int reflect, double* d_loss, double* d_grad_verts, int64_t* d_n_valid, void* stream) {
    CHECK_BUILT(s);
    { int rc = check_law(max_bounces, reflect); if (rc) return rc; }
    return paths_ray_loss_fused(s, d_verts, d_origin, d_dir, d_screen_pixel, d_valid, n_rays, ior_int, ior_ext, max_bounces, reflect != 0, false,
                                d_loss, d_grad_verts, nullptr, d_n_valid, stream, "drt_render_paths_ray_loss_fused");
}

int drt_render_paths_law_forward(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir, int64_t n_rays,
                                 double ior_int, double ior_ext, int max_bounces, int law_flags,
                                 double* d_out_ori, double* d_out_dir, uint8_t* d_mask, int32_t* d_tape, uint8_t* d_hits,
                                 int32_t* d_valid_idx, int64_t* d_n_valid, void* stream) {
    CHECK_BUILT(s);
    { int rc = check_law_flags(max_bounces, law_flags); if (rc) return rc; }
    return paths_forward(s, d_verts, d_origin, d_dir, n_rays, ior_int, ior_ext, max_bounces, (law_flags & DRT_LAW_REFLECT) != 0,
                         (law_flags & DRT_LAW_SNELL) != 0, d_out_ori, d_out_dir, d_mask, d_tape, d_hits, d_valid_idx, d_n_valid, stream,
                         "drt_render_paths_law_forward");
}

int drt_render_paths_law_backward(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir, int64_t n_rays,
                                  double ior_int, double ior_ext, int max_bounces, int law_flags,
                                  const int32_t* d_tape, const uint8_t* d_hits, const int32_t* d_valid_idx, const int64_t* d_n_valid,
                                  const double* d_grad_out_ori, const double* d_grad_out_dir, double* d_grad_verts, void* stream) {
    CHECK_BUILT(s);
    { int rc = check_law_flags(max_bounces, law_flags); if (rc) return rc; }
    return paths_backward(s, d_verts, d_origin, d_dir, n_rays, ior_int, ior_ext, max_bounces, (law_flags & DRT_LAW_SNELL) != 0, d_tape, d_hits,
                          d_valid_idx, d_n_valid, d_grad_out_ori, d_grad_out_dir, d_grad_verts, stream);
}

int drt_render_paths_law_ray_loss_fused(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir,
                                        const double* d_screen_pixel, const uint8_t* d_valid, int64_t n_rays, double ior_int, double ior_ext,
                                        int max_bounces, int law_flags, double* d_loss, double* d_grad_verts, int64_t* d_n_valid, void* stream) {
    CHECK_BUILT(s);
    { int rc = check_law_flags(max_bounces, law_flags); if (rc) return rc; }
    return paths_ray_loss_fused(s, d_verts, d_origin, d_dir, d_screen_pixel, d_valid, n_rays, ior_int, ior_ext, max_bounces,
                                (law_flags & DRT_LAW_REFLECT) != 0, (law_flags & DRT_LAW_SNELL) != 0, d_loss, d_grad_verts, nullptr, d_n_valid, stream,
                                "drt_render_paths_law_ray_loss_fused");
}

int drt_render_paths_law_ray_loss_ior_fused(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir,
                                            const double* d_screen_pixel, const uint8_t* d_valid, int64_t n_rays, double ior_int, double ior_ext,
                                            int max_bounces, int law_flags, double* d_loss, double* d_grad_verts, double* d_grad_ior,
                                            int64_t* d_n_valid, void* stream) {
    CHECK_BUILT(s);
    { int rc = check_law_flags(max_bounces, law_flags); if (rc) return rc; }
    if (!d_grad_ior) return fail(DRT_E_INVALID, "d_grad_ior is NULL: this call differentiates the IORs (drt_render_paths_law_ray_loss_fused does not)");
    return paths_ray_loss_fused(s, d_verts, d_origin, d_dir, d_screen_pixel, d_valid, n_rays, ior_int, ior_ext, max_bounces,
                                (law_flags & DRT_LAW_REFLECT) != 0, (law_flags & DRT_LAW_SNELL) != 0, d_loss, d_grad_verts, d_grad_ior, d_n_valid, stream,
                                "drt_render_paths_law_ray_loss_ior_fused");
}

}  // extern "C"
