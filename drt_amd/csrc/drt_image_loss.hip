// drt_image_loss.hip -- the photometric loss of the refracted image with its vertex and IOR gradients (drt_image_loss.h holds the law;
// DESIGN.md 10.3), one band of rows per call: the forward wavefront of drt_image.hip with the face tape kept, then the adjoint over the
// compact list of through samples.  A translation unit of its own: drt_image.hip, drt_paths.hip and k_trace compile from unchanged text,
// so the kernels of the forward wavefront are restated here under names of their own (a kernel cannot be shared between translation units).
//
//   k_image_loss_start    all samples : k_image_start: sample ray, top-box test, candidates -> list 0, float64 ray and T = 1 parked
//   per interaction k = 0 .. K:
//     k_trace             list k      : drt_trace.hip's, through launch_trace_list, unchanged
//     k_image_loss_shade  list k      : k_image_shade that also records the face of the interaction in the tape [K, n] of the workspace
//   k_image_loss_resolve  all pixels  : k_image_resolve's walk over the s x s samples of its pixel; the float64 mean I, the residual against
//                                       the target, the loss term (LossAcc), the seed g_c = 2 w r / s^2 of the pixel's samples [n_pix, C]
//                                       (a workspace buffer), optionally the float32 image -- the bits drt_render_image writes
//   k_image_loss_collect  all samples : through samples (state byte) -> index list (staged append)
//   k_image_loss_bwd      that list   : image_sample_backward per sample: camera ray formed again (image_sample_ray), exit ray and T from
//                                       the parked rows, g_c of pixel i / s^2; vertex gradients through PathSink in kPathsBwdBatch-sized
//                                       fills, the IOR partials through two LossAcc; VERTS = false: no table in LDS
// Everything runs on the caller's stream, nothing is read back, every list size stays on the device.
#include "drt_device.h"
#include "drt_trace_kernel.h"
#include "drt_pathsink.h"
#include "drt_pathws.h"
#include "drt_image_loss.h"

struct LossBand {
    int width, y0, s;              // image width, first row of the band, supersampling
    unsigned n;                    // samples of the band: rows * width * s * s
};

// sample i of the band -> its pixel and its number within the pixel
__device__ __forceinline__ void loss_band_sample(const LossBand& b, unsigned i, int& x, int& y, int& j) {
    const unsigned s2 = (unsigned)(b.s * b.s), pix = i / s2;
    j = (int)(i - pix * s2);
    y = b.y0 + (int)(pix / (unsigned)b.width);
    x = (int)(pix % (unsigned)b.width);
}

struct LossFill { double c_void[kImageMaxChannels], c_invalid[kImageMaxChannels]; };

struct ImageLossWs {
    int64_t cap = 0;               // doubles of g_c
    double* g_c = nullptr;         // [n_pix, C] of the band in flight
};

namespace {

constexpr int kPathsBwdBatch = 256;        // samples per table fill, as k_paths_loss_bwd_ior (drt_paths.hip)
constexpr int kImageLossBpc = 4;           // blocks per CU of the kernel without the table (registers bound it: DESIGN.md 10.3)

struct DiscardAdd3 {
    __device__ __forceinline__ void operator()(int32_t, d3) const {}
};
template <bool DET>
__device__ __forceinline__ double* ior_slot(double* ior, int k) {
    return DET ? reinterpret_cast<double*>(reinterpret_cast<FxCell*>(ior) + k) : ior + k;
}

}  // namespace

__global__ void __launch_bounds__(kPathBlock) k_image_loss_start(const Node4Q* __restrict__ nodes, int n_tris, ImageCam cam, LossBand band,
                                                                  double* __restrict__ park_ori, double* __restrict__ park_dir,
                                                                  double* __restrict__ thr, uint8_t* __restrict__ state, uint8_t* __restrict__ hits,
                                                                  RayList out, unsigned* count) {
    __shared__ StageMem stage;
    stage_init(stage);
    unsigned first, last;
    block_run(band.n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned i = base + threadIdx.x;
        bool cand = false;
        f3 o32{0.f, 0.f, 0.f}, d32{0.f, 0.f, 1.f};
        if (i < band.n) {
            state[i] = 0;
            hits[i] = 0;
            if (n_tris > 0) {
                int x, y, j;
                loss_band_sample(band, i, x, y, j);
                d3 o, d;
                image_sample_ray(cam, band.s, x, y, j, o, d);
                o32 = to_f32(o); d32 = to_f32(d);
                cand = hits_top_boxes(nodes, o32, d32);
                if (cand) { store_d3(park_ori, i, o); store_d3(park_dir, i, d); thr[i] = 1.0; }
            }
        }
        stage_push(stage, cand, (int32_t)i, o32, d32, out, count);
    }
    stage_flush(stage, out, count);
}

// list k -> list k + 1: k_image_shade (drt_image.hip) with the face of the interaction written to tape[k, i]
template <bool SNELL, bool FRESNEL>
__global__ void __launch_bounds__(kPathBlock) k_image_loss_shade(PathCtx c, int64_t n_rays, int k, int max_bounces, bool reflect, RayList in,
                                                                  const unsigned* __restrict__ n_in, RayList out, unsigned* n_out,
                                                                  double* __restrict__ park_ori, double* __restrict__ park_dir,
                                                                  double* __restrict__ thr, uint8_t* __restrict__ state, uint8_t* __restrict__ hits,
                                                                  int32_t* __restrict__ tape) {
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
                    d3 o = load_d3(park_ori, i), d = load_d3(park_dir, i);
                    double T = FRESNEL ? thr[i] : 1.0;
                    go = image_interact<SNELL, FRESNEL>(c, f, reflect, o, d, n_refr, T);
                    if (go) {
                        store_d3(park_ori, i, o); store_d3(park_dir, i, d);
                        if (FRESNEL) thr[i] = T;
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

// One thread per pixel of the band.  weight / image may be null.
template <bool DET>
__global__ void __launch_bounds__(kPathBlock) k_image_loss_resolve(ImageCam cam, LossBand band, int64_t n_pix, ImageScreen sc, ImageTex tx, LossFill fill,
                                                                    bool fresnel, const double* __restrict__ park_ori,
                                                                    const double* __restrict__ park_dir, const double* __restrict__ thr,
                                                                    const uint8_t* __restrict__ state, const uint8_t* __restrict__ hits,
                                                                    const float* __restrict__ target, const float* __restrict__ weight,
                                                                    double* __restrict__ g_c, float* __restrict__ image, double* loss) {
    const int64_t pix = (int64_t)blockIdx.x * kPathBlock + threadIdx.x;
    LossAcc<DET> acc;
    if (pix < n_pix) {
        const int s2 = band.s * band.s;
        const int y = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
        double sum[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            const int cls = image_class(hits[i] != 0, (state[i] & kPathDone) != 0);
            d3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 1.0};
            double T = 1.0;
            if (cls == kImageDirect) {
                image_sample_ray(cam, band.s, x, y, j, o, d);
            } else if (cls == kImageThrough) {
                o = load_d3(park_ori, i); d = load_d3(park_dir, i);
                if (fresnel) T = thr[i];
            }
            double c[kImageMaxChannels];
            image_sample_colour(sc, tx, cls, o, d, T, fill.c_void, fill.c_invalid, c);
            for (int ch = 0; ch < tx.c; ++ch) sum[ch] = j == 0 ? c[ch] : sum[ch] + c[ch];
        }
        const int64_t row = (int64_t)y * band.width + x;
        double mean[kImageMaxChannels], g[kImageMaxChannels];
        for (int ch = 0; ch < tx.c; ++ch) {
            mean[ch] = sum[ch] / (double)s2;
            if (image) image[row * tx.c + ch] = (float)mean[ch];
        }
        acc.add(image_loss_pixel(mean, tx.c, s2, target + row * tx.c, weight ? (double)weight[row] : 1.0, g));
        for (int ch = 0; ch < tx.c; ++ch) g_c[pix * tx.c + ch] = g[ch];
    }
    acc.flush(loss);
}

// the samples whose path completed (state byte) -> index list; order does not matter to the sums
__global__ void __launch_bounds__(kPathBlock) k_image_loss_collect(unsigned n, const uint8_t* __restrict__ state, int32_t* __restrict__ done_idx,
                                                                    unsigned* n_done) {
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

// The adjoint of one listed sample (image_sample_backward) with the sink of the caller's choice.
template <bool SNELL, bool FRESNEL, typename Add>
__device__ __forceinline__ bool loss_bwd_sample(const PathCtx& c, const ImageCam& cam, const LossBand& band, const ImageScreen& sc, const ImageTex& tx,
                                                int max_bounces, const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                const double* __restrict__ thr, const int32_t* __restrict__ tape, const uint8_t* __restrict__ hits,
                                                const double* __restrict__ g_c, int64_t i, Add add, double& gi, double& ge) {
    int x, y, j;
    loss_band_sample(band, (unsigned)i, x, y, j);
    d3 o, d;
    image_sample_ray(cam, band.s, x, y, j, o, d);
    const int64_t pix = i / (band.s * band.s);
    double g[kImageMaxChannels] = {0.0, 0.0, 0.0};
    for (int ch = 0; ch < tx.c; ++ch) g[ch] = g_c[pix * tx.c + ch];
    return image_sample_backward<SNELL, FRESNEL>(c, o, d, tape + i, (int64_t)band.n, min((int)hits[i], max_bounces), load_d3(park_ori, i),
                                                 load_d3(park_dir, i), FRESNEL ? thr[i] : 1.0, sc, tx, g, add, gi, ge);
}

// grad_verts (VERTS), grad_ior and count may each be null.
template <bool DET, bool SNELL, bool FRESNEL, bool VERTS>
__global__ void __launch_bounds__(256) k_image_loss_bwd(PathCtx c, ImageCam cam, LossBand band, ImageScreen sc, ImageTex tx, int max_bounces,
                                                        const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                        const double* __restrict__ thr, const int32_t* __restrict__ tape,
                                                        const uint8_t* __restrict__ hits, const int32_t* __restrict__ list,
                                                        const unsigned* __restrict__ n_list, const double* __restrict__ g_c, double* grad_verts,
                                                        double* grad_ior, unsigned long long* count) {
    int64_t n = *n_list;
    if (n > (int64_t)band.n) n = band.n;
    LossAcc<DET> acc_int, acc_ext;
    unsigned cnt = 0;
    if constexpr (VERTS) {
        __shared__ int32_t hkeys[kHashSize];
        __shared__ double hsums[3 * kHashSize];
        const PathSink<DET> add{hkeys, hsums, grad_verts};
        for (int64_t base = blockIdx.x * (int64_t)kPathsBwdBatch; base < n; base += (int64_t)gridDim.x * kPathsBwdBatch) {
            add.clear();
            const int64_t end = base + kPathsBwdBatch < n ? base + kPathsBwdBatch : n;
            for (int64_t k = base + threadIdx.x; k < end; k += blockDim.x) {
                const int64_t i = list[k];
                if (i < 0 || i >= (int64_t)band.n) continue;
                double gi, ge;
                if (loss_bwd_sample<SNELL, FRESNEL>(c, cam, band, sc, tx, max_bounces, park_ori, park_dir, thr, tape, hits, g_c, i, add, gi, ge)) {
                    acc_int.add(gi); acc_ext.add(ge);
                    ++cnt;
                }
            }
            add.flush();
        }
    } else {
        for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
            const int64_t i = list[k];
            if (i < 0 || i >= (int64_t)band.n) continue;
            double gi, ge;
            if (loss_bwd_sample<SNELL, FRESNEL>(c, cam, band, sc, tx, max_bounces, park_ori, park_dir, thr, tape, hits, g_c, i, DiscardAdd3{}, gi, ge)) {
                acc_int.add(gi); acc_ext.add(ge);
                ++cnt;
            }
        }
    }
    if (grad_ior) {
        acc_int.flush(ior_slot<DET>(grad_ior, 0));
        acc_ext.flush(ior_slot<DET>(grad_ior, 1));
    }
    if (count && cnt) atomicAdd(count, (unsigned long long)cnt);
}

namespace {

// the throughputs (PathsWs::thr, shared with drt_render_image) and the pixel seeds, grown like the rows of the one-pass form
int ensure_image_loss_ws(drt_scene* s, int64_t n, int64_t n_seed, hipStream_t st) {
    PathsWs* w = paths_ws_of(s);
    ImageLossWs* lw = static_cast<ImageLossWs*>(s->image_loss_ws);
    if (n <= w->thr_cap && lw && n_seed <= lw->cap) return DRT_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(DRT_E_INVALID, "drt_render_image_loss: the first call of this size allocates its throughputs and pixel seeds and cannot run "
                                   "inside a stream capture: issue one such call eagerly before capturing");
    if (n > w->thr_cap) {
        (void)hipFree(w->thr);
        w->thr = nullptr; w->thr_cap = 0;
        HIP_TRY(hipMalloc(&w->thr, sizeof(double) * (size_t)n));
        w->thr_cap = n;
    }
    if (!lw) {
        lw = new (std::nothrow) ImageLossWs();
        if (!lw) return fail(DRT_E_NOMEM, "host allocation failed");
        s->image_loss_ws = lw;
    }
    if (n_seed > lw->cap) {
        (void)hipFree(lw->g_c);
        lw->g_c = nullptr; lw->cap = 0;
        HIP_TRY(hipMalloc(&lw->g_c, sizeof(double) * (size_t)n_seed));
        lw->cap = n_seed;
    }
    return DRT_OK;
}

template <bool SNELL>
void launch_loss_shade(bool fresnel, int gs, hipStream_t st, const PathCtx& pc, int64_t n, int k, int max_bounces, bool reflect, const RayList& in,
                       const unsigned* n_in, const RayList& out, unsigned* n_out, double* park_ori, double* park_dir, const PathsWs& w) {
    if (fresnel) k_image_loss_shade<SNELL, true><<<gs, kPathBlock, 0, st>>>(pc, n, k, max_bounces, reflect, in, n_in, out, n_out, park_ori, park_dir, w.thr, w.state, w.hits, w.tape);
    else k_image_loss_shade<SNELL, false><<<gs, kPathBlock, 0, st>>>(pc, n, k, max_bounces, reflect, in, n_in, out, n_out, park_ori, park_dir, w.thr, w.state, w.hits, w.tape);
}

// k_image_loss_bwd under (deterministic, snell, fresnel, verts)
#define IMAGE_LOSS_BWD_LAUNCH(det, snell, fresnel, verts, grid, st, ...)                                              \
    do {                                                                                                              \
        const int sel_ = ((det) ? 8 : 0) | ((snell) ? 4 : 0) | ((fresnel) ? 2 : 0) | ((verts) ? 1 : 0);               \
        switch (sel_) {                                                                                               \
        case 0: k_image_loss_bwd<false, false, false, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;               \
        case 1: k_image_loss_bwd<false, false, false, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 2: k_image_loss_bwd<false, false, true, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 3: k_image_loss_bwd<false, false, true, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 4: k_image_loss_bwd<false, true, false, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 5: k_image_loss_bwd<false, true, false, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 6: k_image_loss_bwd<false, true, true, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 7: k_image_loss_bwd<false, true, true, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                  \
        case 8: k_image_loss_bwd<true, false, false, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 9: k_image_loss_bwd<true, false, false, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 10: k_image_loss_bwd<true, false, true, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 11: k_image_loss_bwd<true, false, true, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 12: k_image_loss_bwd<true, true, false, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 13: k_image_loss_bwd<true, true, false, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 14: k_image_loss_bwd<true, true, true, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        default: k_image_loss_bwd<true, true, true, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                  \
        }                                                                                                             \
    } while (0)

}  // namespace

void image_loss_free(drt_scene* s) {
    ImageLossWs* lw = static_cast<ImageLossWs*>(s->image_loss_ws);
    if (!lw) return;
    (void)hipFree(lw->g_c);
    delete lw;
    s->image_loss_ws = nullptr;
}

extern "C" {

int drt_render_image_loss(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                          double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                          const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                          const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                          int64_t* d_count, void* stream) {
    CHECK_BUILT(s);
    if (max_bounces < 2 || max_bounces > kMaxBounces) return fail(DRT_E_INVALID, "max_bounces = %d: must be 2 .. %d", max_bounces, kMaxBounces);
    if (law_flags & ~(DRT_LAW_REFLECT | DRT_LAW_SNELL))
        return fail(DRT_E_INVALID, "law_flags = %d: must be a combination of DRT_LAW_REFLECT (%d) and DRT_LAW_SNELL (%d)", law_flags, DRT_LAW_REFLECT, DRT_LAW_SNELL);
    if (fresnel != 0 && fresnel != 1) return fail(DRT_E_INVALID, "fresnel = %d: 0 (geometry only) or 1 (weight refractions by 1 - R)", fresnel);
    if (supersample < 1 || supersample > kImageMaxSuper) return fail(DRT_E_INVALID, "supersample = %d: must be 1 .. %d", supersample, kImageMaxSuper);
    if (channels != 1 && channels != 3) return fail(DRT_E_INVALID, "channels = %d: must be 1 or 3", channels);
    if (tex_h < 2 || tex_w < 2) return fail(DRT_E_INVALID, "tex_h x tex_w = %d x %d: the texture must be at least 2 x 2", tex_h, tex_w);
    if (height < 1 || width < 1) return fail(DRT_E_INVALID, "height x width = %d x %d: the image must have at least one pixel", height, width);
    if (y0 < 0 || y1 > height || y0 >= y1) return fail(DRT_E_INVALID, "band [y0, y1) = [%d, %d): must be a non-empty range of rows inside [0, %d)", y0, y1, height);
    if (!camera21 || !screen9 || !fill_void || !fill_invalid) return fail(DRT_E_INVALID, "null host pointer argument (camera21, screen9, fill_void, fill_invalid)");
    if (!d_texture || !d_target || !d_loss || (s->n_faces > 0 && !d_verts))
        return fail(DRT_E_INVALID, "null device pointer argument (d_verts, d_texture, d_target, d_loss)");
    ImageCam cam;
    memcpy(cam.kinv, camera21, sizeof(double) * 9);
    memcpy(cam.rinv, camera21 + 9, sizeof(double) * 12);
    const ImageScreen sc{d3{screen9[0], screen9[1], screen9[2]}, d3{screen9[3], screen9[4], screen9[5]}, d3{screen9[6], screen9[7], screen9[8]}};
    if (!image_screen_ok(sc)) return fail(DRT_E_INVALID, "screen9: the axes eu, ev must be finite, non-zero and orthogonal (|eu . ev| <= 1e-12 |eu| |ev|)");
    const int s2 = supersample * supersample;
    const int64_t n_pix = (int64_t)(y1 - y0) * width, n = n_pix * s2;
    if (n > INT32_MAX) return fail(DRT_E_INVALID, "the band has %lld samples: at most 2^31 - 1 per call (render fewer rows)", (long long)n);
    hipStream_t st = (hipStream_t)stream;
    { int rc = ensure_paths_ws(s, n, st, "drt_render_image_loss"); if (rc) return rc; }
    { int rc = ensure_paths_fused_ws(s, n, st, "drt_render_image_loss"); if (rc) return rc; }
    { int rc = ensure_image_loss_ws(s, n, n_pix * channels, st); if (rc) return rc; }
    { int rc = wait_build(s, st); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    const ImageLossWs& lw = *static_cast<ImageLossWs*>(s->image_loss_ws);
    PathCtx pc = path_ctx(s, d_verts, ior_int, ior_ext);
    pc.tc.slow_stack = w.slow_stack;
    const LossBand band{width, y0, supersample, (unsigned)n};
    const ImageTex tx{d_texture, tex_h, tex_w, channels};
    LossFill fill{};
    for (int ch = 0; ch < channels; ++ch) { fill.c_void[ch] = fill_void[ch]; fill.c_invalid[ch] = fill_invalid[ch]; }
    const int gs = grid_for(n, kPathBlock, 8 * s->n_cu);
    double* const park_ori = w.park;
    double* const park_dir = w.park + 3 * w.fused_cap;
    const bool reflect = (law_flags & DRT_LAW_REFLECT) != 0, snell = (law_flags & DRT_LAW_SNELL) != 0;
    HIP_TRY(hipMemsetAsync(w.cnt, 0, sizeof(unsigned) * kCntWords, st));
    const RayList l0{w.idx[0], w.ray[0], w.face[0]}, l1{w.idx[1], w.ray[1], w.face[1]};
    k_image_loss_start<<<gs, kPathBlock, 0, st>>>(pc.tc.nodes, pc.tc.n_tris, cam, band, park_ori, park_dir, w.thr, w.state, w.hits, l0, w.cnt + kCntList);
    if (s->n_faces > 0) {
        for (int k = 0; k <= max_bounces; ++k) {
            const RayList& in = (k & 1) ? l1 : l0;
            const RayList& out = (k & 1) ? l0 : l1;
            launch_trace_list(k < max_bounces ? kTraceClosest : kTraceAny, s->grid_path, st, pc.tc, in.ray, w.cnt + kCntList + k,
                              TraceOut{in.face, nullptr, nullptr, nullptr}, w.redo, w.cnt + kCntRedo + k, w.cnt + kCntDone, s->refill_min, s->inner_min, nullptr);
            if (snell) launch_loss_shade<true>(fresnel != 0, gs, st, pc, n, k, max_bounces, reflect, in, w.cnt + kCntList + k, out, w.cnt + kCntList + k + 1, park_ori, park_dir, w);
            else launch_loss_shade<false>(fresnel != 0, gs, st, pc, n, k, max_bounces, reflect, in, w.cnt + kCntList + k, out, w.cnt + kCntList + k + 1, park_ori, park_dir, w);
        }
    }
    const bool det = det_mode();
    const unsigned pix_grid = (unsigned)((n_pix + kPathBlock - 1) / kPathBlock);
    if (det) k_image_loss_resolve<true><<<pix_grid, kPathBlock, 0, st>>>(cam, band, n_pix, sc, tx, fill, fresnel != 0, park_ori, park_dir, w.thr, w.state, w.hits,
                                                                          d_target, d_weight, lw.g_c, d_image, d_loss);
    else k_image_loss_resolve<false><<<pix_grid, kPathBlock, 0, st>>>(cam, band, n_pix, sc, tx, fill, fresnel != 0, park_ori, park_dir, w.thr, w.state, w.hits,
                                                                       d_target, d_weight, lw.g_c, d_image, d_loss);
    if (s->n_faces > 0 && (d_grad_verts || d_grad_ior || d_count)) {
        int32_t* const done = w.idx[0];          // (both ping-pong lists are free once the loop has ended)
        k_image_loss_collect<<<gs, kPathBlock, 0, st>>>((unsigned)n, w.state, done, w.cnt + kCntValid);
        const int grid = (d_grad_verts ? DRT_BWD_BPC : kImageLossBpc) * s->n_cu;
        IMAGE_LOSS_BWD_LAUNCH(det, snell, fresnel != 0, d_grad_verts != nullptr, grid, st, pc, cam, band, sc, tx, max_bounces, park_ori, park_dir, w.thr, w.tape, w.hits,
                              done, w.cnt + kCntValid, lw.g_c, d_grad_verts, d_grad_ior, reinterpret_cast<unsigned long long*>(d_count));
    }
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

}  // extern "C"
