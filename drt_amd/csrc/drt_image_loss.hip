// drt_image_loss.hip -- the photometric loss of the refracted image with its vertex and IOR gradients (drt_image_loss.h holds the law;
// DESIGN.md 10.3), one band of rows per call: the forward wavefront of drt_image.hip with the face tape kept (image_forward, declared in
// drt_image_wave.h), then the adjoint over the compact list of through samples.  The kernels are drt_image_loss_bwd.h's templates and the
// host body of the call is its image_loss_run; this unit holds the forms <ImageOneView, ImageClear> without CAMERA.
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
//   k_image_camera_bwd    all pixels  : drt_render_image_loss_camera only (drt_image_camera.hip, through launch_image_camera_bwd): the 21
//                                       camera partials; k_image_loss_bwd is then that unit's, with CAMERA (launch_image_loss_bwd_camera)
// Everything runs on the caller's stream, nothing is read back, every list size stays on the device.
#include "drt_image_loss_bwd.h"

// the pixel seeds [n_seed], grown like the throughputs they sit beside (drt_image.hip); the camera-ray seeds [n_cam] (0: none wanted) likewise
int ensure_image_loss_ws(drt_scene* s, int64_t n_seed, int64_t n_cam, hipStream_t st, const char* who) {
    ImageLossWs* lw = static_cast<ImageLossWs*>(s->image_loss_ws);
    if (!lw) {
        lw = new (std::nothrow) ImageLossWs();
        if (!lw) return fail(DRT_E_NOMEM, "host allocation failed");
        s->image_loss_ws = lw;
    }
    { int rc = grow_doubles(lw->g_c, lw->cap, n_seed, st, who, "pixel seeds"); if (rc) return rc; }
    return grow_doubles(lw->seeds, lw->seed_cap, n_cam, st, who, "camera-ray seeds");
}

void image_loss_free(drt_scene* s) {
    ImageLossWs* lw = static_cast<ImageLossWs*>(s->image_loss_ws);
    if (!lw) return;
    (void)hipFree(lw->g_c);
    (void)hipFree(lw->seeds);
    delete lw;
    s->image_loss_ws = nullptr;
}

namespace {

// The one host body of drt_render_image_loss, drt_render_image_loss_screen and drt_render_image_loss_camera (`who`, for messages): the
// first hands no screen, no texture and no camera accumulator and enqueues what it always has; so does the second without a camera
// accumulator.
int image_loss_call(drt_scene* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample, double ior_int,
                    double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9, const float* d_texture, int tex_h, int tex_w,
                    int channels, const double* fill_void, const double* fill_invalid, const float* d_target, const float* d_weight, double* d_loss,
                    double* d_grad_verts, double* d_grad_ior, float* d_image, int64_t* d_count, double* d_grad_screen, double* d_grad_texture,
                    double* d_grad_camera, void* stream, const char* who) {
    CHECK_BUILT(s);
    ImageCall c;
    { int rc = image_call_check(camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h, tex_w,
                                channels, fill_void, fill_invalid, d_texture && d_target && d_loss && (s->n_faces == 0 || d_verts),
                                "null device pointer argument (d_verts, d_texture, d_target, d_loss)", c); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    if (d_grad_texture && (int64_t)tex_h * tex_w > INT32_MAX)
        return fail(DRT_E_INVALID, "tex_h x tex_w = %d x %d: a texture gradient takes at most 2^31 - 1 texels", tex_h, tex_w);
    const bool seeds_wanted = d_grad_camera && s->n_faces > 0;          // (a scene without triangles has direct samples only)
    { int rc = image_loss_run(s, d_verts, c, ImageOneView{c.cam, c.sc}, ImageClear{}, [&](ImageClear&) { return image_forward(s, d_verts, c, true, st, who); },
                              d_grad_camera ? launch_image_loss_bwd_camera : image_loss_bwd_launch<ImageOneView, ImageClear, false>,
                              ImageLossOut{d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, nullptr}, seeds_wanted ? 6 * c.n : 0, st, who);
      if (rc) return rc; }
    const ImageLossWs& lw = *static_cast<ImageLossWs*>(s->image_loss_ws);
    if (d_grad_screen || d_grad_texture) { int rc = launch_image_screen_bwd(s, c, lw.g_c, d_grad_screen, d_grad_texture, st); if (rc) return rc; }
    if (d_grad_camera) return launch_image_camera_bwd(s, c, lw.g_c, seeds_wanted ? lw.seeds : nullptr, d_grad_camera, st);
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
                           nullptr, stream, "drt_render_image_loss");
}

int drt_render_image_loss_screen(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                 double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                 const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                 const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                 int64_t* d_count, double* d_grad_screen, double* d_grad_texture, void* stream) {
    return image_loss_call(s, d_verts, camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h,
                           tex_w, channels, fill_void, fill_invalid, d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, d_grad_screen,
                           d_grad_texture, nullptr, stream, "drt_render_image_loss_screen");
}

int drt_render_image_loss_camera(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                 double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                 const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                 const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                 int64_t* d_count, double* d_grad_screen, double* d_grad_texture, double* d_grad_camera, void* stream) {
    return image_loss_call(s, d_verts, camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h,
                           tex_w, channels, fill_void, fill_invalid, d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, d_grad_screen,
                           d_grad_texture, d_grad_camera, stream, "drt_render_image_loss_camera");
}

}  // extern "C"
