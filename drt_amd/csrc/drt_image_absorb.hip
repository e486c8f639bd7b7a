// drt_image_absorb.hip -- absorbing glass (drt_image_absorb.h states the law): the refracted image and its
// photometric loss with Beer-Lambert attenuation along the interior length of every sample, one band of rows per call.  The forward
// wavefront is drt_image.hip's (image_forward_from) with this unit's shade kernels; every kernel is the family's template
// (drt_image_wave.h, drt_image_loss_bwd.h) under the payload ImageAbsorb, and this unit holds those forms.  A unit of its own for the
// reason drt_image_loss_bwd.h gives: the clear instantiations keep their register figures.
//
//   k_image_start         all samples : drt_image.hip's (image_start_call)
//   per interaction k = 0 .. K:
//     k_trace             list k      : drt_trace.hip's, through trace_lists, unchanged
//     k_image_shade       list k      : <., ., ., ImageAbsorb>: also the interior length len[i], one more float64 per sample
//   k_image_resolve       all pixels  : <ImageAbsorb>: A_ch = exp(-(sigma_ch L)) on the lit samples; optionally the plane `length`, the mean of
//                                       L over the pixel's through samples
//   k_image_loss_resolve  all pixels  : <., ImageOneView, ImageAbsorb>: likewise; also the C sigma partials
//   k_paths_collect       all samples : drt_paths.hip's, through launch_paths_collect
//   k_image_loss_bwd      that list   : <.., ImageOneView, ImageAbsorb> without CAMERA: reads len[i] beside thr[i]
// Everything runs on the caller's stream, nothing is read back, every list size stays on the device.
#include "drt_image_loss_bwd.h"

// the host array sigma[channels] of an entry point, after image_call_check (drt_image_views_absorb.hip uses it too)
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

namespace {

// k_image_shade<., ., ., ImageAbsorb> as the shade hook of image_forward_from; `src`: the payload
void absorb_shade(const ImageShadeArgs& a, const void* src) { image_shade_launch(a, *static_cast<const ImageAbsorb*>(src)); }

// The forward wavefront of an absorbing call: the workspace grown (the lengths too, which completes the payload), then image_forward_from
// with this unit's shade kernel.
int absorb_forward(drt_scene* s, const double* d_verts, const ImageCall& c, bool keep_tape, ImageAbsorb& pay, hipStream_t st, const char* who) {
    { int rc = ensure_paths_ws(s, c.n, st, who); if (rc) return rc; }
    PathsWs* w = paths_ws_of(s);
    { int rc = grow_doubles(w->len, w->len_cap, c.n, st, who, "interior lengths"); if (rc) return rc; }
    pay.len = w->len;
    return image_forward_from(s, d_verts, c, keep_tape, st, who, image_start_call, &c, absorb_shade, &pay);
}

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
    ImageAbsorb pay{};
    { int rc = absorb_sigma_check(sigma, channels, pay.sigma); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    { int rc = absorb_forward(s, d_verts, c, false, pay, st, "drt_render_image_absorb"); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    k_image_resolve<<<(unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock), kPathBlock, 0, st>>>(
        c.cam, c.band, c.n_pix, c.sc, c.tx, c.fill, c.fresnel, pay, w.park, w.park + 3 * w.fused_cap, w.thr, w.state, w.hits, d_image, d_hit, d_through, d_length);
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
    ImageAbsorb pay{};
    { int rc = absorb_sigma_check(sigma, channels, pay.sigma); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    return image_loss_run(s, d_verts, c, ImageOneView{c.cam, c.sc}, pay, [&](ImageAbsorb& p) { return absorb_forward(s, d_verts, c, true, p, st, who); },
                          image_loss_bwd_launch<ImageOneView, ImageAbsorb, false>,
                          ImageLossOut{d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, d_grad_sigma}, 0, st, who);
}

}  // extern "C"
