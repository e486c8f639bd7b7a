// drt_image_loss.hip -- the photometric loss of the refracted image with its vertex and IOR gradients (drt_image_loss.h holds the law;
// DESIGN.md 10.3), one band of rows per call: the forward wavefront of drt_image.hip with the face tape kept (image_forward, declared in
// drt_image_wave.h), then the adjoint over the compact list of through samples.
//
//   image_forward         all samples : k_image_start, then per interaction k_trace and k_image_shade<., ., tape>, which also records the
//                                       face of the interaction in the tape [K, n] of the workspace
//   k_image_loss_resolve  all pixels  : k_image_resolve's walk over the s x s samples of its pixel (image_pixel_walk); the float64 mean I, the
//                                       residual against the target, the loss term (LossAcc), the seed g_c = 2 w r / s^2 of the pixel's samples
//                                       [n_pix, C] (a workspace buffer), optionally the float32 image -- the bits drt_render_image writes
//   k_paths_collect       all samples : drt_paths.hip's, through launch_paths_collect: through samples (state byte) -> index list
//   k_image_loss_bwd      that list   : image_sample_backward per sample: camera ray formed again (image_sample_ray), exit ray and T from
//                                       the parked rows, g_c of pixel i / s^2; vertex gradients through PathSink in kPathsBwdBatch-sized
//                                       fills, the IOR partials through two LossAcc; VERTS = false: no table in LDS
//   k_image_screen_bwd    all pixels  : drt_render_image_loss_screen only (drt_image_screen.hip, through launch_image_screen_bwd): the screen-pose
//                                       and texture gradients from the same seeds
// Everything runs on the caller's stream, nothing is read back, every list size stays on the device.
#include "drt_image_wave.h"
#include "drt_image_loss.h"

struct ImageLossWs {
    int64_t cap = 0;               // doubles of g_c
    double* g_c = nullptr;         // [n_pix, C] of the band in flight
};

constexpr int kImageLossBpc = 4;           // blocks per CU of the kernel without the table (registers bound it: DESIGN.md 10.3)

// One thread per pixel of the band.  weight / image may be null.
template <bool DET>
__global__ void __launch_bounds__(kPathBlock) k_image_loss_resolve(ImageCam cam, ImageBand band, int64_t n_pix, ImageScreen sc, ImageTex tx, ImageFill fill,
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
        int n_hit, n_through;          // (not wanted here)
        image_pixel_walk(cam, band, pix, x, y, sc, tx, fill, fresnel, park_ori, park_dir, thr, state, hits, sum, n_hit, n_through);
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

// The adjoint of one listed sample (image_sample_backward) with the sink of the caller's choice.
template <bool SNELL, bool FRESNEL, typename Add>
__device__ __forceinline__ bool loss_bwd_sample(const PathCtx& c, const ImageCam& cam, const ImageBand& band, const ImageScreen& sc, const ImageTex& tx,
                                                int max_bounces, const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                const double* __restrict__ thr, const int32_t* __restrict__ tape, const uint8_t* __restrict__ hits,
                                                const double* __restrict__ g_c, int64_t i, Add add, double& gi, double& ge) {
    int x, y, j;
    band_sample(band, (unsigned)i, x, y, j);
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
__global__ void __launch_bounds__(256) k_image_loss_bwd(PathCtx c, ImageCam cam, ImageBand band, ImageScreen sc, ImageTex tx, int max_bounces,
                                                        const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                        const double* __restrict__ thr, const int32_t* __restrict__ tape,
                                                        const uint8_t* __restrict__ hits, const int32_t* __restrict__ list,
                                                        const unsigned* __restrict__ n_list, const double* __restrict__ g_c, double* grad_verts,
                                                        double* grad_ior, unsigned long long* count) {
    int64_t n = *n_list;
    if (n > (int64_t)band.n) n = band.n;
    LossAcc<DET> acc_int, acc_ext;
    unsigned cnt = 0;
    sink_pass<DET, kPathsBwdBatch, VERTS>(n, grad_verts, [&](int64_t k, auto add) {
        const int64_t i = list[k];
        if (i < 0 || i >= (int64_t)band.n) return;
        double gi, ge;
        if (loss_bwd_sample<SNELL, FRESNEL>(c, cam, band, sc, tx, max_bounces, park_ori, park_dir, thr, tape, hits, g_c, i, add, gi, ge)) {
            acc_int.add(gi); acc_ext.add(ge);
            ++cnt;
        }
    });
    if (grad_ior) {
        acc_int.flush(ior_slot<DET>(grad_ior, 0));
        acc_ext.flush(ior_slot<DET>(grad_ior, 1));
    }
    if (count && cnt) atomicAdd(count, (unsigned long long)cnt);
}

namespace {

// the pixel seeds [n_seed], grown like the throughputs they sit beside (drt_image.hip)
int ensure_image_loss_ws(drt_scene* s, int64_t n_seed, hipStream_t st, const char* who) {
    ImageLossWs* lw = static_cast<ImageLossWs*>(s->image_loss_ws);
    if (lw && n_seed <= lw->cap) return DRT_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(DRT_E_INVALID, "%s: the first call of this size allocates its pixel seeds and cannot run "
                                   "inside a stream capture: issue one such call eagerly before capturing", who);
    if (!lw) {
        lw = new (std::nothrow) ImageLossWs();
        if (!lw) return fail(DRT_E_NOMEM, "host allocation failed");
        s->image_loss_ws = lw;
    }
    (void)hipFree(lw->g_c);
    lw->g_c = nullptr; lw->cap = 0;
    HIP_TRY(hipMalloc(&lw->g_c, sizeof(double) * (size_t)n_seed));
    lw->cap = n_seed;
    return DRT_OK;
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

namespace {

// The one host body of drt_render_image_loss and drt_render_image_loss_screen (`who`, for messages): the former hands no screen and no
// texture accumulator and enqueues what it always has.
int image_loss_call(drt_scene* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample, double ior_int,
                    double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9, const float* d_texture, int tex_h, int tex_w,
                    int channels, const double* fill_void, const double* fill_invalid, const float* d_target, const float* d_weight, double* d_loss,
                    double* d_grad_verts, double* d_grad_ior, float* d_image, int64_t* d_count, double* d_grad_screen, double* d_grad_texture, void* stream,
                    const char* who) {
    CHECK_BUILT(s);
    ImageCall c;
    { int rc = image_call_check(camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h, tex_w,
                                channels, fill_void, fill_invalid, d_texture && d_target && d_loss && (s->n_faces == 0 || d_verts),
                                "null device pointer argument (d_verts, d_texture, d_target, d_loss)", c); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    if (d_grad_texture && (int64_t)tex_h * tex_w > INT32_MAX)
        return fail(DRT_E_INVALID, "tex_h x tex_w = %d x %d: a texture gradient takes at most 2^31 - 1 texels", tex_h, tex_w);
    { int rc = ensure_image_loss_ws(s, c.n_pix * channels, st, who); if (rc) return rc; }
    { int rc = image_forward(s, d_verts, c, true, st, who); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    const ImageLossWs& lw = *static_cast<ImageLossWs*>(s->image_loss_ws);
    const PathCtx pc = image_path_ctx(s, d_verts, c);
    double* const park_ori = w.park;
    double* const park_dir = w.park + 3 * w.fused_cap;
    const bool det = det_mode();
    const unsigned pix_grid = (unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock);
    if (det) k_image_loss_resolve<true><<<pix_grid, kPathBlock, 0, st>>>(c.cam, c.band, c.n_pix, c.sc, c.tx, c.fill, c.fresnel, park_ori, park_dir, w.thr, w.state, w.hits,
                                                                          d_target, d_weight, lw.g_c, d_image, d_loss);
    else k_image_loss_resolve<false><<<pix_grid, kPathBlock, 0, st>>>(c.cam, c.band, c.n_pix, c.sc, c.tx, c.fill, c.fresnel, park_ori, park_dir, w.thr, w.state, w.hits,
                                                                       d_target, d_weight, lw.g_c, d_image, d_loss);
    if (s->n_faces > 0 && (d_grad_verts || d_grad_ior || d_count)) {
        int32_t* const done = w.idx[0];          // (both ping-pong lists are free once the loop has ended)
        launch_paths_collect(grid_for(c.n, kPathBlock, 8 * s->n_cu), st, (unsigned)c.n, w.state, done, w.cnt + kCntValid);
        const int grid = (d_grad_verts ? DRT_BWD_BPC : kImageLossBpc) * s->n_cu;
        IMAGE_LOSS_BWD_LAUNCH(det, c.snell, c.fresnel, d_grad_verts != nullptr, grid, st, pc, c.cam, c.band, c.sc, c.tx, c.max_bounces, park_ori, park_dir, w.thr, w.tape,
                              w.hits, done, w.cnt + kCntValid, lw.g_c, d_grad_verts, d_grad_ior, reinterpret_cast<unsigned long long*>(d_count));
    }
    HIP_TRY(hipGetLastError());
    if (d_grad_screen || d_grad_texture) return launch_image_screen_bwd(s, c, lw.g_c, d_grad_screen, d_grad_texture, st);
    return DRT_OK;
}

}  // namespace

extern "C" {

int drt_render_image_loss(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                          double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                          const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                          const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                          int64_t* d_count, void* stream) {
    return image_loss_call(s, d_verts, camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h,
                           tex_w, channels, fill_void, fill_invalid, d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, nullptr, nullptr,
                           stream, "drt_render_image_loss");
}

int drt_render_image_loss_screen(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                 double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                 const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                 const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                 int64_t* d_count, double* d_grad_screen, double* d_grad_texture, void* stream) {
    return image_loss_call(s, d_verts, camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h,
                           tex_w, channels, fill_void, fill_invalid, d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, d_grad_screen,
                           d_grad_texture, stream, "drt_render_image_loss_screen");
}

}  // extern "C"
