// drt_image_views_absorb.hip -- absorbing glass in the photometric image term of up to 16 views, in front of their screens, of ONE
// environment map, or of both, with the optional reflection off the outer surface.  The law is nothing new per sample:
// the result is the sum over the listed views of one view's loss under 10.7's law, with the environment attenuated exactly like the
// texture and the reflection -- light that never entered the object -- not attenuated.  This unit holds the forms of the family's
// templates under the product ImageViewTable x ImageAbsorb x {ImageScreenOnly, ImageScreenEnv, ImageScreenEnvReflect}; a unit of its own
// for the reason drt_image_loss_bwd.h gives (the forms of the five units it borrows from keep their register figures).
//
//   image_forward_from    all samples : drt_image.hip's wavefront with the table's start kernel (image_start_views, drt_image_views.hip's)
//                                       and k_image_shade<., ., ., ImageAbsorb>: also the interior length len[i]; the face tape kept
//   reflection_pass       all samples : drt_image_env_loss.h's <ImageViewTable>, with `reflection`
//   k_image_loss_resolve  all pixels  : <., ImageViewTable, ImageAbsorb, BG>: A_ch = exp(-(sigma_ch L)) on the transmitted colour of the lit
//                                       samples, from the screen or from the environment; the C sigma partials from that part alone;
//                                       optionally the float32 pixel of every listed view, at its view's row of the stack
//   k_paths_collect       all samples : drt_paths.hip's
//   k_image_loss_bwd      that list   : <.., ImageViewTable, ImageAbsorb, no CAMERA, ImageScreenOnly | ImageScreenEnv>: reads len[i] beside
//                                       thr[i]; to the environment through image_env_sample_backward<.., LENGTH>
//   k_image_reflect_bwd   that list   : <DET, SNELL, VERTS, ImageViewTable>, with `reflection`, unchanged
// Without an environment the sequence is image_loss_run's (drt_image_loss_bwd.h), with one env_loss_run's (drt_image_env_loss.h).
// Everything runs on the caller's stream, nothing is read back, every list size stays on the device.
#include "drt_image_env_loss.h"

namespace {

// k_image_shade<., ., ., ImageAbsorb> as the shade hook of image_forward_from; `src`: the payload
void views_absorb_shade(const ImageShadeArgs& a, const void* src) { image_shade_launch(a, *static_cast<const ImageAbsorb*>(src)); }

// The forward wavefront of the call: the workspace grown (the lengths too, which completes the payload), then image_forward_from with
// the table's start kernel and this unit's shade kernel, the tape kept.
int views_absorb_forward(drt_scene* s, const double* d_verts, const ImageCall& c, const ViewsStart& vs, ImageAbsorb& pay, hipStream_t st, const char* who) {
    { int rc = ensure_paths_ws(s, c.n, st, who); if (rc) return rc; }
    PathsWs* w = paths_ws_of(s);
    { int rc = grow_doubles(w->len, w->len_cap, c.n, st, who, "interior lengths"); if (rc) return rc; }
    pay.len = w->len;
    return image_forward_from(s, d_verts, c, true, st, who, image_start_views, &vs, views_absorb_shade, &pay);
}

}  // namespace

extern "C" {

int drt_render_image_loss_views_absorb(drt_scene_t* s, const double* d_verts, const drt_image_views_t* views, const int* view_ids, int k, int r0, int r1,
                                       int supersample, double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const float* d_texture,
                                       int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid, const float* d_targets,
                                       const float* d_weights, double* d_loss, double* d_grad_verts, double* d_grad_ior, int64_t* d_count, const double* sigma,
                                       double* d_grad_sigma, const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection, float* d_images,
                                       void* stream) {
    const char* const who = "drt_render_image_loss_views_absorb";
    CHECK_BUILT(s);
    if (!views) return fail(DRT_E_INVALID, "views is null: make the view table with drt_image_views_create");
    if (views->scene != s) return fail(DRT_E_INVALID, "views: the view table belongs to another scene");
    if (k < 1 || k > kImageViewsMax) return fail(DRT_E_INVALID, "k = %d: a call lists 1 .. %d views", k, kImageViewsMax);
    if (!view_ids) return fail(DRT_E_INVALID, "null host pointer argument (view_ids)");
    ImageViewIds ids{};
    ids.height = views->height; ids.k = k;
    for (int j = 0; j < k; ++j) {
        if (view_ids[j] < 0 || view_ids[j] >= views->n_views)
            return fail(DRT_E_INVALID, "view_ids[%d] = %d: the view table has views 0 .. %d", j, view_ids[j], views->n_views - 1);
        ids.id[j] = view_ids[j];
    }
    const bool has_env = d_env != nullptr, has_screen = d_texture != nullptr;
    ImageCall c;          // (its camera and screen are the first listed view's and are not used: every kernel reads the table)
    if (!has_env) {
        int rc = image_call_check(views->cam21 + 21 * (size_t)ids.id[0], k * views->height, views->width, r0, r1, supersample, ior_int, ior_ext, max_bounces, law_flags,
                                  fresnel, views->scr9 + 9 * (size_t)ids.id[0], d_texture, tex_h, tex_w, channels, fill_void, fill_invalid,
                                  d_texture && d_targets && d_loss && (s->n_faces == 0 || d_verts),
                                  "null device pointer argument (d_verts, d_texture, d_targets, d_loss)", c);
        if (rc) return rc;
    } else {          // (without a screen d_env stands in for the texture that the check wants non-null, as in drt_render_image_loss_views_env)
        int rc = image_call_check(views->cam21 + 21 * (size_t)ids.id[0], k * views->height, views->width, r0, r1, supersample, ior_int, ior_ext, max_bounces, law_flags,
                                  fresnel, views->scr9 + 9 * (size_t)ids.id[0], has_screen ? d_texture : d_env, has_screen ? tex_h : 2, has_screen ? tex_w : 2, channels,
                                  fill_void, fill_invalid, d_targets && d_loss && (s->n_faces == 0 || d_verts),
                                  "null device pointer argument (d_verts, d_targets, d_loss)", c);
        if (rc) return rc;
    }
    ImageAbsorb pay{};
    { int rc = absorb_sigma_check(sigma, channels, pay.sigma); if (rc) return rc; }
    ImageScreenEnv bg{};
    if (has_env) { int rc = env_args_check(d_env, env_h, env_w, env_rot9, reflection, fresnel, channels, has_screen, bg); if (rc) return rc; }
    else if (reflection) return fail(DRT_E_INVALID, "reflection = %d: the reflection needs an environment (d_env is null)", reflection);
    hipStream_t st = (hipStream_t)stream;
    const ViewsStart vs{ImageViewTable{views->d_rows, ids}, c.band};
    const ImageLossOut out{d_targets, d_weights, d_loss, d_grad_verts, d_grad_ior, d_images, d_count, d_grad_sigma};
    if (!has_env)
        return image_loss_run(s, d_verts, c, vs.view, pay, [&](ImageAbsorb& p) { return views_absorb_forward(s, d_verts, c, vs, p, st, who); },
                              image_loss_bwd_launch<ImageViewTable, ImageAbsorb, false>, out, 0, st, who);
    return env_loss_run(s, d_verts, c, vs.view, [&](ImageAbsorb& p) { return views_absorb_forward(s, d_verts, c, vs, p, st, who); }, bg, reflection != 0, out, st,
                        who, pay);
}

}  // extern "C"
