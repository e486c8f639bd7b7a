// drt_image_views_env.hip -- the photometric image term of up to 16 views in front of ONE environment map, with the optional reflection off the
// outer surface, as ONE forward wavefront, ONE reflection pass and ONE adjoint pass.  The law is nothing new: the result
// is the sum over the listed views of what drt_render_image_loss_env gives for each; the per-sample device functions are that call's, the
// mapping of a row of the band to (view, y) is drt_image_views.h's.  This unit holds the forms of the family's templates under the product
// ImageViewTable x ImageScreenEnv[Reflect]; a unit of its own for the reason drt_image_loss_bwd.h gives (the forms of drt_image_views.hip
// and drt_image_env.hip keep their register figures).
//
//   image_forward_from    all samples : drt_image.hip's wavefront with the table's start kernel (image_start_views, drt_image_views.hip's:
//                                       no second copy of k_image_start<ImageViewTable>), the face tape kept
//   k_image_reflect_list  all samples : <SNELL, ImageViewTable>, with `reflection`: the camera ray formed again with the camera of the row's
//                                       view and the row WITHIN that view
//   k_trace, k_image_reflect_mark     : drt_trace.hip's and drt_image_env.hip's, unchanged
//   k_image_loss_resolve  all pixels  : <., ImageViewTable, ImageClear, ImageScreenEnv[Reflect]>
//   k_paths_collect       all samples : drt_paths.hip's
//   k_image_loss_bwd      that list   : <.., ImageViewTable, ImageClear, no CAMERA, ImageScreenEnv>
//   k_image_reflect_bwd   that list   : <DET, SNELL, VERTS, ImageViewTable>, with `reflection`
// The sequence is env_loss_run's (drt_image_env_loss.h).  No workspace of its own: tape row 0, the bit kImageReflectSeen, words 34 and 35 of
// the counter block.  The id list reaches every kernel by value (ImageViewIds) and is resolved by the unrolled select.  Everything runs on
// the caller's stream, nothing is read back.
#include "drt_image_env_loss.h"

extern "C" {

int drt_render_image_loss_views_env(drt_scene_t* s, const double* d_verts, const drt_image_views_t* views, const int* view_ids, int k, int r0, int r1,
                                    int supersample, double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const float* d_texture,
                                    int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid, const float* d_targets,
                                    const float* d_weights, double* d_loss, double* d_grad_verts, double* d_grad_ior, int64_t* d_count, const float* d_env,
                                    int env_h, int env_w, const double* env_rot9, int reflection, void* stream) {
    const char* const who = "drt_render_image_loss_views_env";
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
    // (before image_call_check, as in env_loss_call: without a screen d_env stands in for the texture that the check wants non-null)
    if (!d_env) return fail(DRT_E_INVALID, "null device pointer argument (d_env)");
    const bool has_screen = d_texture != nullptr;          // (without one the table's screens are never read: ImageScreenEnv::screen is false)
    ImageCall c;          // (its camera and screen are the first listed view's and are not used: every kernel reads the table)
    { int rc = image_call_check(views->cam21 + 21 * (size_t)ids.id[0], k * views->height, views->width, r0, r1, supersample, ior_int, ior_ext, max_bounces, law_flags,
                                fresnel, views->scr9 + 9 * (size_t)ids.id[0], has_screen ? d_texture : d_env, has_screen ? tex_h : 2, has_screen ? tex_w : 2, channels,
                                fill_void, fill_invalid, d_targets && d_loss && (s->n_faces == 0 || d_verts),
                                "null device pointer argument (d_verts, d_targets, d_loss)", c); if (rc) return rc; }
    ImageScreenEnv bg{};
    { int rc = env_args_check(d_env, env_h, env_w, env_rot9, reflection, fresnel, channels, has_screen, bg); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    const ViewsStart vs{ImageViewTable{views->d_rows, ids}, c.band};
    return env_loss_run(s, d_verts, c, vs.view, [&] { return image_forward_from(s, d_verts, c, true, st, who, image_start_views, &vs); }, bg, reflection != 0,
                        ImageLossOut{d_targets, d_weights, d_loss, d_grad_verts, d_grad_ior, nullptr, d_count, nullptr}, st, who);
}

}  // extern "C"
