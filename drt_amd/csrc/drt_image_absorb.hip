// drt_image_absorb.hip -- absorbing glass (drt_image_absorb.h holds the law): the refracted image and its photometric loss
// with Beer-Lambert attenuation along the interior length of every sample, one band of rows per call.  The forward wavefront is
// drt_image.hip's (image_forward_from) with this unit's shade kernel; everything else is a form of a kernel of drt_image.hip /
// drt_image_loss.hip that also reads the interior length.  A unit of its own for the reason drt_image_loss_bwd.h gives: the existing
// instantiations keep their register figures.
//
//   k_image_start                all samples : drt_image.hip's, unchanged (image_start_call)
//   per interaction k = 0 .. K:
//     k_trace                    list k      : drt_trace.hip's, through trace_lists, unchanged
//     k_image_absorb_shade       list k      : k_image_shade plus the interior length len[i], one more float64 per sample: stored at k = 0, added to
//                                              afterwards (no memset); o, d, T and n_refr have image_interact's bits
//   k_image_absorb_resolve       all pixels  : k_image_resolve's walk with A_ch = exp(-(sigma_ch L)) on the lit samples; optionally the plane
//                                              `length`, the mean of L over the pixel's through samples
//   k_image_absorb_loss_resolve  all pixels  : k_image_loss_resolve likewise; also the C sigma partials -g_c[ch] sum_j L_j c_j[ch], which need
//                                              forward values only (LossAcc x 3 through block_flush)
//   k_paths_collect              all samples : drt_paths.hip's, through launch_paths_collect
//   k_image_absorb_loss_bwd      that list   : k_image_loss_bwd without CAMERA over image_sample_backward_absorb, which reads len[i] beside thr[i]
// Everything runs on the caller's stream, nothing is read back, every list size stays on the device.
#include "drt_image_wave.h"
#include "drt_image_absorb.h"

struct ImageSigma { double v[kImageMaxChannels]; };

// list k -> list k + 1: k_image_shade (drt_image.hip) with image_absorb_interact, which also carries the interior length of the sample.
template <bool SNELL, bool FRESNEL, bool TAPE>
__global__ void __launch_bounds__(kPathBlock) k_image_absorb_shade(PathCtx c, int64_t n_rays, int k, int max_bounces, bool reflect, RayList in,
                                                                    const unsigned* __restrict__ n_in, RayList out, unsigned* n_out,
                                                                    double* __restrict__ park_ori, double* __restrict__ park_dir,
                                                                    double* __restrict__ thr, double* __restrict__ len, uint8_t* __restrict__ state,
                                                                    uint8_t* __restrict__ hits, int32_t* __restrict__ tape) {
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
                    if constexpr (TAPE) tape[(int64_t)k * n_rays + i] = f;
                    hits[i] = (uint8_t)(k + 1);
                    d3 o = load_d3(park_ori, i), d = load_d3(park_dir, i);
                    double T = FRESNEL ? thr[i] : 1.0;
                    // (the length of a sample whose path dies here is stored too: nothing reads it)
                    go = image_absorb_interact<SNELL, FRESNEL>(c, f, reflect, o, d, n_refr, T,
                                                               [&](const Bounce& b) { len[i] = image_absorb_length(b, k == 0 ? 0.0 : len[i]); });
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

// image_pixel_walk (drt_image_wave.h) with the attenuation: sum[0 .. tx.c) is the ordered float64 sum of the colours; lc[0 .. tx.c) that of
// L_j c_j[ch] over the through samples on the screen (what the sigma partials need), l_sum that of L over the through samples.
__device__ __forceinline__ void image_absorb_pixel_walk(const ImageCam& cam, const ImageBand& band, int64_t pix, int x, int y, const ImageScreen& sc,
                                                        const ImageTex& tx, const ImageFill& fill, bool fresnel, const ImageSigma& sigma,
                                                        const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                        const double* __restrict__ thr, const double* __restrict__ len,
                                                        const uint8_t* __restrict__ state, const uint8_t* __restrict__ hits, double* sum, double* lc,
                                                        double& l_sum, int& n_hit, int& n_through) {
    const int s2 = band.s * band.s;
    n_hit = 0; n_through = 0;
    l_sum = 0.0;
    for (int j = 0; j < s2; ++j) {
        const int64_t i = pix * s2 + j;
        const bool was_hit = hits[i] != 0, done = (state[i] & kPathDone) != 0;
        const int cls = image_class(was_hit, done);
        n_hit += was_hit ? 1 : 0;
        d3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 1.0};
        double T = 1.0, L = 0.0;
        if (cls == kImageDirect) {
            image_sample_ray(cam, band.s, x, y, j, o, d);
        } else if (cls == kImageThrough) {
            o = load_d3(park_ori, i); d = load_d3(park_dir, i);
            if (fresnel) T = thr[i];
            L = len[i];
            l_sum = n_through == 0 ? L : l_sum + L;
            ++n_through;
        }
        double c[kImageMaxChannels];
        const bool lit = image_absorb_sample_colour(sc, tx, cls, o, d, T, L, sigma.v, fill.c_void, fill.c_invalid, c);
#pragma unroll
        for (int ch = 0; ch < kImageMaxChannels; ++ch) {
            if (ch >= tx.c) continue;
            sum[ch] = j == 0 ? c[ch] : sum[ch] + c[ch];
            if (lit && cls == kImageThrough) lc[ch] = lc[ch] + L * c[ch];
        }
    }
}

// One thread per pixel of the band.  hit / through / length may be null.
__global__ void __launch_bounds__(kPathBlock) k_image_absorb_resolve(ImageCam cam, ImageBand band, int64_t n_pix, ImageScreen sc, ImageTex tx, ImageFill fill,
                                                                      bool fresnel, ImageSigma sigma, const double* __restrict__ park_ori,
                                                                      const double* __restrict__ park_dir, const double* __restrict__ thr,
                                                                      const double* __restrict__ len, const uint8_t* __restrict__ state,
                                                                      const uint8_t* __restrict__ hits, float* __restrict__ image, float* __restrict__ hit,
                                                                      float* __restrict__ through, float* __restrict__ length) {
    const int64_t pix = (int64_t)blockIdx.x * kPathBlock + threadIdx.x;
    if (pix >= n_pix) return;
    const int s2 = band.s * band.s;
    const int y = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
    double acc[kImageMaxChannels] = {0.0, 0.0, 0.0}, lc[kImageMaxChannels] = {0.0, 0.0, 0.0}, l_sum;
    int n_hit, n_through;
    image_absorb_pixel_walk(cam, band, pix, x, y, sc, tx, fill, fresnel, sigma, park_ori, park_dir, thr, len, state, hits, acc, lc, l_sum, n_hit, n_through);
    const int64_t row = (int64_t)y * band.width + x;
    for (int ch = 0; ch < tx.c; ++ch) image[row * tx.c + ch] = (float)(acc[ch] / (double)s2);
    if (hit) hit[row] = (float)((double)n_hit / (double)s2);
    if (through) through[row] = (float)((double)n_through / (double)s2);
    if (length) length[row] = n_through ? (float)(l_sum / (double)n_through) : 0.f;
}

// One thread per pixel of the band.  weight / image / grad_sigma may be null.
template <bool DET>
__global__ void __launch_bounds__(kPathBlock) k_image_absorb_loss_resolve(ImageCam cam, ImageBand band, int64_t n_pix, ImageScreen sc, ImageTex tx, ImageFill fill,
                                                                           bool fresnel, ImageSigma sigma, const double* __restrict__ park_ori,
                                                                           const double* __restrict__ park_dir, const double* __restrict__ thr,
                                                                           const double* __restrict__ len, const uint8_t* __restrict__ state,
                                                                           const uint8_t* __restrict__ hits, const float* __restrict__ target,
                                                                           const float* __restrict__ weight, double* __restrict__ g_c,
                                                                           float* __restrict__ image, double* loss, double* grad_sigma) {
    const int64_t pix = (int64_t)blockIdx.x * kPathBlock + threadIdx.x;
    LossAcc<DET> acc, sig[kImageMaxChannels];
    if (pix < n_pix) {
        const int s2 = band.s * band.s;
        const int y = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
        double sum[kImageMaxChannels] = {0.0, 0.0, 0.0}, lc[kImageMaxChannels] = {0.0, 0.0, 0.0}, l_sum;
        int n_hit, n_through;          // (not wanted here)
        image_absorb_pixel_walk(cam, band, pix, x, y, sc, tx, fill, fresnel, sigma, park_ori, park_dir, thr, len, state, hits, sum, lc, l_sum, n_hit, n_through);
        const int64_t row = (int64_t)y * band.width + x;
        double mean[kImageMaxChannels] = {0.0, 0.0, 0.0}, g[kImageMaxChannels] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int ch = 0; ch < kImageMaxChannels; ++ch) {
            if (ch >= tx.c) continue;
            mean[ch] = sum[ch] / (double)s2;
            if (image) image[row * tx.c + ch] = (float)mean[ch];
        }
        acc.add(image_loss_pixel(mean, tx.c, s2, target + row * tx.c, weight ? (double)weight[row] : 1.0, g));
#pragma unroll
        for (int ch = 0; ch < kImageMaxChannels; ++ch) {
            if (ch >= tx.c) continue;
            g_c[pix * tx.c + ch] = g[ch];
            sig[ch].add(image_absorb_sigma_term(g[ch], lc[ch]));
        }
    }
    acc.flush(loss);
    if (grad_sigma) {                  // (the same in every thread; tx.c accumulators, never more)
        if (tx.c == kImageMaxChannels) block_flush<DET, kImageMaxChannels>(sig, grad_sigma);
        else block_flush<DET, 1>(sig, grad_sigma);
    }
}

// grad_verts (VERTS), grad_ior and count may each be null: k_image_loss_bwd (drt_image_loss_bwd.h) without CAMERA, over the absorbing adjoint.
template <bool DET, bool SNELL, bool FRESNEL, bool VERTS>
__global__ void __launch_bounds__(256, VERTS ? 2 : 1) k_image_absorb_loss_bwd(PathCtx c, ImageCam cam, ImageBand band, ImageScreen sc, ImageTex tx, ImageSigma sigma,
                                                               int max_bounces, const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                               const double* __restrict__ thr, const double* __restrict__ len,
                                                               const int32_t* __restrict__ tape, const uint8_t* __restrict__ hits,
                                                               const int32_t* __restrict__ list, const unsigned* __restrict__ n_list,
                                                               const double* __restrict__ g_c, double* grad_verts, double* grad_ior,
                                                               unsigned long long* count) {
    int64_t n = *n_list;
    if (n > (int64_t)band.n) n = band.n;
    LossAcc<DET> acc_int, acc_ext;
    unsigned cnt = 0;
    sink_pass<DET, kPathsBwdBatch, VERTS>(n, grad_verts, [&](int64_t k, auto add) {
        const int64_t i = list[k];
        if (i < 0 || i >= (int64_t)band.n) return;
        int x, y, j;
        band_sample(band, (unsigned)i, x, y, j);
        d3 o, d;
        image_sample_ray(cam, band.s, x, y, j, o, d);
        const int64_t pix = i / (band.s * band.s);
        double g[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int ch = 0; ch < tx.c; ++ch) g[ch] = g_c[pix * tx.c + ch];
        double gi, ge;
        if (image_sample_backward_absorb<SNELL, FRESNEL>(c, o, d, tape + i, (int64_t)band.n, min((int)hits[i], max_bounces), load_d3(park_ori, i),
                                                         load_d3(park_dir, i), FRESNEL ? thr[i] : 1.0, len[i], sigma.v, sc, tx, g, add, gi, ge)) {
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

// one interior length per sample, grown like the throughputs it sits beside (drt_image.hip ensure_image_thr)
int ensure_image_len(drt_scene* s, int64_t n, hipStream_t st, const char* who) {
    PathsWs* w = paths_ws_of(s);
    if (n <= w->len_cap) return DRT_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(DRT_E_INVALID, "%s: the first call of this size allocates its throughputs and cannot run inside a stream "
                                   "capture: issue one such call eagerly before capturing", who);
    (void)hipFree(w->len);
    w->len = nullptr; w->len_cap = 0;
    HIP_TRY(hipMalloc(&w->len, sizeof(double) * (size_t)n));
    w->len_cap = n;
    return DRT_OK;
}

// the host array sigma[channels] of an entry point, after image_call_check
int absorb_sigma_check(const double* sigma, int channels, ImageSigma& out) {
    if (!sigma) return fail(DRT_E_INVALID, "null host pointer argument (sigma)");
    out = ImageSigma{{0.0, 0.0, 0.0}};
    for (int ch = 0; ch < channels; ++ch) {
        if (!(sigma[ch] >= 0.0) || !(sigma[ch] < INFINITY))
            return fail(DRT_E_INVALID, "sigma[%d] = %g: an absorption coefficient must be finite and >= 0", ch, sigma[ch]);
        out.v[ch] = sigma[ch];
    }
    return DRT_OK;
}

// k_image_absorb_shade under (snell, fresnel, tape) as the shade hook of image_forward_from; `src`: the lengths
using AbsorbShade = void (*)(PathCtx, int64_t, int, int, bool, RayList, const unsigned*, RayList, unsigned*, double*, double*, double*, double*, uint8_t*, uint8_t*,
                             int32_t*);
void absorb_shade(const ImageShadeArgs& a, const void* src) {
    static const AbsorbShade kernels[8] = {k_image_absorb_shade<false, false, false>, k_image_absorb_shade<false, false, true>,
                                           k_image_absorb_shade<false, true, false>,  k_image_absorb_shade<false, true, true>,
                                           k_image_absorb_shade<true, false, false>,  k_image_absorb_shade<true, false, true>,
                                           k_image_absorb_shade<true, true, false>,   k_image_absorb_shade<true, true, true>};
    const AbsorbShade kern = kernels[(a.snell ? 4 : 0) | (a.fresnel ? 2 : 0) | (a.tape ? 1 : 0)];
    kern<<<a.grid, kPathBlock, 0, a.st>>>(a.pc, a.n_rays, a.k, a.max_bounces, a.reflect, a.in, a.n_in, a.out, a.n_out, a.park_ori, a.park_dir, a.thr,
                                          static_cast<double*>(const_cast<void*>(src)), a.state, a.hits, a.tape);
}

// The forward wavefront of an absorbing call: the workspace grown (the lengths too), then image_forward_from with this unit's shade kernel.
int absorb_forward(drt_scene* s, const double* d_verts, const ImageCall& c, bool keep_tape, hipStream_t st, const char* who) {
    { int rc = ensure_paths_ws(s, c.n, st, who); if (rc) return rc; }
    { int rc = ensure_image_len(s, c.n, st, who); if (rc) return rc; }
    return image_forward_from(s, d_verts, c, keep_tape, st, who, image_start_call, &c, absorb_shade, paths_ws_of(s)->len);
}

// k_image_absorb_loss_bwd under (deterministic, snell, fresnel, verts)
#define IMAGE_ABSORB_BWD_LAUNCH(det, snell, fresnel, verts, grid, st, ...)                                              \
    do {                                                                                                                \
        const int sel_ = ((det) ? 8 : 0) | ((snell) ? 4 : 0) | ((fresnel) ? 2 : 0) | ((verts) ? 1 : 0);                 \
        switch (sel_) {                                                                                                 \
        case 0: k_image_absorb_loss_bwd<false, false, false, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;          \
        case 1: k_image_absorb_loss_bwd<false, false, false, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;           \
        case 2: k_image_absorb_loss_bwd<false, false, true, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;           \
        case 3: k_image_absorb_loss_bwd<false, false, true, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;            \
        case 4: k_image_absorb_loss_bwd<false, true, false, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;           \
        case 5: k_image_absorb_loss_bwd<false, true, false, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;            \
        case 6: k_image_absorb_loss_bwd<false, true, true, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;            \
        case 7: k_image_absorb_loss_bwd<false, true, true, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;             \
        case 8: k_image_absorb_loss_bwd<true, false, false, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;           \
        case 9: k_image_absorb_loss_bwd<true, false, false, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;            \
        case 10: k_image_absorb_loss_bwd<true, false, true, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;           \
        case 11: k_image_absorb_loss_bwd<true, false, true, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;            \
        case 12: k_image_absorb_loss_bwd<true, true, false, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;           \
        case 13: k_image_absorb_loss_bwd<true, true, false, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;            \
        case 14: k_image_absorb_loss_bwd<true, true, true, false><<<grid, 256, 0, st>>>(__VA_ARGS__); break;            \
        default: k_image_absorb_loss_bwd<true, true, true, true><<<grid, 256, 0, st>>>(__VA_ARGS__); break;             \
        }                                                                                                               \
    } while (0)

}  // namespace

extern "C" {

int drt_render_image_absorb(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                            double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                            const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                            float* d_image, float* d_hit, float* d_through, const double* sigma, float* d_length, void* stream) {
    CHECK_BUILT(s);
    ImageCall c;
    { int rc = image_call_check(camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h, tex_w,
                                channels, fill_void, fill_invalid, d_texture && d_image && (s->n_faces == 0 || d_verts),
                                "null device pointer argument (d_verts, d_texture, d_image)", c); if (rc) return rc; }
    ImageSigma sg;
    { int rc = absorb_sigma_check(sigma, channels, sg); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    { int rc = absorb_forward(s, d_verts, c, false, st, "drt_render_image_absorb"); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    k_image_absorb_resolve<<<(unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock), kPathBlock, 0, st>>>(
        c.cam, c.band, c.n_pix, c.sc, c.tx, c.fill, c.fresnel, sg, w.park, w.park + 3 * w.fused_cap, w.thr, w.len, w.state, w.hits, d_image, d_hit, d_through, d_length);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

int drt_render_image_loss_absorb(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                 double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                 const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                 const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                 int64_t* d_count, const double* sigma, double* d_grad_sigma, void* stream) {
    const char* const who = "drt_render_image_loss_absorb";
    CHECK_BUILT(s);
    ImageCall c;
    { int rc = image_call_check(camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h, tex_w,
                                channels, fill_void, fill_invalid, d_texture && d_target && d_loss && (s->n_faces == 0 || d_verts),
                                "null device pointer argument (d_verts, d_texture, d_target, d_loss)", c); if (rc) return rc; }
    ImageSigma sg;
    { int rc = absorb_sigma_check(sigma, channels, sg); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    { int rc = ensure_image_loss_ws(s, c.n_pix * channels, 0, st, who); if (rc) return rc; }
    { int rc = absorb_forward(s, d_verts, c, true, st, who); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    const ImageLossWs& lw = *static_cast<ImageLossWs*>(s->image_loss_ws);
    const PathCtx pc = image_path_ctx(s, d_verts, c);
    double* const park_ori = w.park;
    double* const park_dir = w.park + 3 * w.fused_cap;
    const bool det = det_mode();
    const unsigned pix_grid = (unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock);
    DET_LAUNCH(k_image_absorb_loss_resolve, pix_grid, kPathBlock, st, c.cam, c.band, c.n_pix, c.sc, c.tx, c.fill, c.fresnel, sg, park_ori, park_dir, w.thr, w.len,
               w.state, w.hits, d_target, d_weight, lw.g_c, d_image, d_loss, d_grad_sigma);
    if (s->n_faces > 0 && (d_grad_verts || d_grad_ior || d_count)) {
        int32_t* const done = w.idx[0];          // (both ping-pong lists are free once the loop has ended)
        launch_paths_collect(grid_for(c.n, kPathBlock, 8 * s->n_cu), st, (unsigned)c.n, w.state, done, w.cnt + kCntValid);
        const int grid = (d_grad_verts ? DRT_BWD_BPC : kImageLossBpc) * s->n_cu;
        IMAGE_ABSORB_BWD_LAUNCH(det, c.snell, c.fresnel, d_grad_verts != nullptr, grid, st, pc, c.cam, c.band, c.sc, c.tx, sg, c.max_bounces, park_ori, park_dir,
                                w.thr, w.len, w.tape, w.hits, done, w.cnt + kCntValid, lw.g_c, d_grad_verts, d_grad_ior,
                                reinterpret_cast<unsigned long long*>(d_count));
    }
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

}  // extern "C"
