// drt_image_env.hip -- the refracted image in front of an environment map (drt_image_env.h states the law): a screen or
// none, and a lat-long panorama at infinity where the screen is not, one band of rows per call.  The forward wavefront is drt_image.hip's
// (image_forward), unchanged: the paths do not know what they will look at.  This unit holds the forms of the family's templates under
// the background policy ImageScreenEnv.  A unit of its own for the reason drt_image_loss_bwd.h gives: the forms without an environment
// keep their register figures.
//
//   image_forward         all samples : k_image_start, then per interaction k_trace and k_image_shade, drt_image.hip's
//   k_image_resolve       all pixels  : <ImageClear, ImageScreenEnv>: a direct or through sample that the screen does not catch looks up
//                                       the environment along its exit direction (acos, atan2 and a wrapped bilinear fetch, for those
//                                       samples only); no sample receives `void`
// With `reflection` the forward wavefront keeps its face tape, whose row 0 is the first face of every sample, and between it
// and the resolve kernel runs the reflection pass (reflection_pass, drt_image_env_loss.h: k_image_reflect_list and k_image_reflect_bwd are
// stated there once over the view policy, for this unit's ImageOneView and for drt_image_views_env.hip's ImageViewTable):
//   k_image_reflect_list  all samples : a sample that met the mesh forms its camera ray again, recomputes the Bounce of its first face and, where
//                                       that is an entering, non-TIR interaction, appends the float32 reflected ray to a list of its own (the
//                                       staged append of drt_pathsink.h into ping-pong list 0, free once the loop has ended; its size and its
//                                       second-pass count in two spare words of the counter block, zeroed with it)
//   k_trace               that list   : any hit (launch_trace_list(kTraceAny, ...)), drt_trace.hip's, unchanged
//   k_image_reflect_mark  that list   : a reflected ray that found nothing sets the bit kImageReflectSeen in its sample's state byte (a sample is
//                                       listed at most once: no two threads write one byte)
//   k_image_resolve       all pixels  : <ImageClear, ImageScreenEnvReflect>: a through sample with the bit recomputes (ro, wr, R1) and adds
//                                       R1 * B(ro, wr); also the plane `reflect`
// The loss (drt_render_image_loss_env; the loss itself is drt_image_loss.h's):
//   image_forward         all samples : with the face tape kept; then, with `reflection`, the reflection pass above
//   k_image_loss_resolve  all pixels  : <., ImageOneView, ImageClear, ImageScreenEnv[Reflect]>: the walk of the resolve form, the loss, the seeds g_c
//   k_paths_collect       all samples : drt_paths.hip's: through samples -> index list
//   k_image_loss_bwd      that list   : <.., ImageOneView, ImageClear, no CAMERA, ImageScreenEnv>: image_env_sample_backward -- the exit ray's seed is
//                                       the screen's where it lands there, g_o = 0 and g_d from the lookup otherwise; every listed sample counts
//   k_image_reflect_bwd   that list   : with `reflection`: a listed sample with the bit kImageReflectSeen (exactly those whose reflection was added)
//                                       forms its camera ray again and runs image_reflect_backward: one triangle, one Bounce; vertex gradients
//                                       through PathSink, the IOR partials through two LossAcc.  A kernel of its own: k_image_loss_bwd sits at
//                                       197 to 256 VGPRs
//   k_image_env_param_bwd all pixels  : drt_render_image_loss_env_param with an accumulator for the environment's texels or rotation
//                                       (DESIGN.md 10.9): drt_image_env_param.hip's, last on the stream
// No workspace of its own: the first face is the tape's row 0 (4 B per sample, already there for the loss) and the bit sits in the state
// byte.  The list's order is never read, so two runs give the same bits.
// Everything runs on the caller's stream, nothing is read back, every list size stays on the device.
#include "drt_image_env_loss.h"

namespace {

// entry e of the traced reflection list: face < 0 = nothing in the way
__global__ void __launch_bounds__(kPathBlock) k_image_reflect_mark(RayList list, const unsigned* __restrict__ n_list, unsigned n_samples, uint8_t* __restrict__ state) {
    unsigned n = *n_list;
    if (n > n_samples) n = n_samples;
    for (unsigned e = blockIdx.x * kPathBlock + threadIdx.x; e < n; e += gridDim.x * kPathBlock) {
        const int32_t i = list.idx[e];
        if (i >= 0 && (unsigned)i < n_samples && list.face[e] < 0) state[i] = state[i] | kImageReflectSeen;
    }
}

// a screen that stands for none: never evaluated (ImageScreenEnv::screen is false), it only has to pass image_call_check
const double kNoScreen[9] = {0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0};

// The one host body of drt_render_image_loss_env and drt_render_image_loss_env_param (`who`); the former hands two null pointers.
int env_loss_call(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample, double ior_int,
                  double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9, const float* d_texture, int tex_h, int tex_w, int channels,
                  const double* fill_void, const double* fill_invalid, const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts,
                  double* d_grad_ior, float* d_image, int64_t* d_count, const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection,
                  double* d_grad_env, double* d_grad_env_rot, void* stream, const char* who) {
    CHECK_BUILT(s);
    if ((screen9 == nullptr) != (d_texture == nullptr))
        return fail(DRT_E_INVALID, "screen9 and d_texture must be given together or both be NULL (no screen: every ray sees the environment)");
    if (!d_env) return fail(DRT_E_INVALID, "null device pointer argument (d_env)");
    const bool has_screen = screen9 != nullptr;
    ImageCall c;
    { int rc = image_call_check(camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, has_screen ? screen9 : kNoScreen,
                                has_screen ? d_texture : d_env, has_screen ? tex_h : 2, has_screen ? tex_w : 2, channels, fill_void, fill_invalid,
                                d_target && d_loss && (s->n_faces == 0 || d_verts), "null device pointer argument (d_verts, d_target, d_loss)", c); if (rc) return rc; }
    ImageScreenEnv bg{};
    { int rc = env_args_check(d_env, env_h, env_w, env_rot9, reflection, fresnel, channels, has_screen, bg); if (rc) return rc; }
    if (d_grad_env && (int64_t)env_h * env_w > INT32_MAX)
        return fail(DRT_E_INVALID, "env_h x env_w = %d x %d: an environment texel gradient (d_grad_env) takes at most 2^31 - 1 texels", env_h, env_w);
    hipStream_t st = (hipStream_t)stream;
    const ImageLossOut out{d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, nullptr};
    const ImageOneView view{c.cam, c.sc};
    { int rc = env_loss_run(s, d_verts, c, view, [&] { return image_forward(s, d_verts, c, true, st, who); }, bg, reflection != 0, out, st, who); if (rc) return rc; }
    // grad_env / grad_env_rot (drt_render_image_loss_env_param; either may be null): the pass of drt_image_env_param.hip over the pixels of
    // the band comes last, behind what env_loss_run left in the workspace
    if (d_grad_env || d_grad_env_rot)
        return launch_image_env_param_bwd(s, image_path_ctx(s, d_verts, c), c, bg, reflection != 0, static_cast<ImageLossWs*>(s->image_loss_ws)->g_c, d_grad_env,
                                          d_grad_env_rot, st);
    return DRT_OK;
}

}  // namespace

// The arguments an environment call adds, after image_call_check: fills `bg`.
int env_args_check(const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection, int fresnel, int channels, bool has_screen,
                   ImageScreenEnv& bg) {
    if (!d_env) return fail(DRT_E_INVALID, "null device pointer argument (d_env)");
    if (env_h < 2 || env_w < 2) return fail(DRT_E_INVALID, "env_h x env_w = %d x %d: the environment must be at least 2 x 2", env_h, env_w);
    if (!env_rot9) return fail(DRT_E_INVALID, "null host pointer argument (env_rot9)");
    if (!image_env_rot_ok(env_rot9)) return fail(DRT_E_INVALID, "env_rot9: the rotation must be orthonormal (max |R R^T - I| <= 1e-12)");
    if (reflection != 0 && reflection != 1) return fail(DRT_E_INVALID, "reflection = %d: 0 (the reflected light is dropped) or 1 (add the outer-surface reflection)", reflection);
    if (reflection && !fresnel) return fail(DRT_E_INVALID, "reflection = 1 needs fresnel = 1: the reflected share R1 is the complement of what the Fresnel term transmits");
    bg.screen = has_screen;
    bg.env = ImageEnv{d_env, env_h, env_w, channels, {}};
    memcpy(bg.env.rot, env_rot9, sizeof(double) * 9);
    return DRT_OK;
}

void launch_image_reflect_mark(int grid, hipStream_t st, RayList list, const unsigned* n_list, unsigned n_samples, uint8_t* state) {
    k_image_reflect_mark<<<grid, kPathBlock, 0, st>>>(list, n_list, n_samples, state);
}

extern "C" {

int drt_render_image_env(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                         double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                         const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                         float* d_image, float* d_hit, float* d_through, const float* d_env, int env_h, int env_w, const double* env_rot9,
                         int reflection, float* d_reflect, void* stream) {
    CHECK_BUILT(s);
    if ((screen9 == nullptr) != (d_texture == nullptr))
        return fail(DRT_E_INVALID, "screen9 and d_texture must be given together or both be NULL (no screen: every ray sees the environment)");
    if (!d_env) return fail(DRT_E_INVALID, "null device pointer argument (d_env)");
    const bool has_screen = screen9 != nullptr;
    ImageCall c;
    { int rc = image_call_check(camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, has_screen ? screen9 : kNoScreen,
                                has_screen ? d_texture : d_env, has_screen ? tex_h : 2, has_screen ? tex_w : 2, channels, fill_void, fill_invalid,
                                d_image && (s->n_faces == 0 || d_verts), "null device pointer argument (d_verts, d_image)", c); if (rc) return rc; }
    ImageScreenEnv bg{};
    { int rc = env_args_check(d_env, env_h, env_w, env_rot9, reflection, fresnel, channels, has_screen, bg); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    { int rc = image_forward(s, d_verts, c, reflection != 0, st, "drt_render_image_env"); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    const unsigned pix_grid = (unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock);
    if (reflection) {
        const PathCtx pc = image_path_ctx(s, d_verts, c);
        reflection_pass(s, pc, c, ImageOneView{c.cam, c.sc}, st);
        const ImageScreenEnvReflect bgr{bg.screen, bg.env, pc, c.snell, w.tape, d_reflect};
        k_image_resolve<ImageClear, ImageScreenEnvReflect><<<pix_grid, kPathBlock, 0, st>>>(
            c.cam, c.band, c.n_pix, c.sc, c.tx, c.fill, c.fresnel, ImageClear{}, w.park, w.park + 3 * w.fused_cap, w.thr, w.state, w.hits, d_image, d_hit, d_through,
            nullptr, bgr);
        HIP_TRY(hipGetLastError());
        return DRT_OK;
    }
    k_image_resolve<ImageClear, ImageScreenEnv><<<pix_grid, kPathBlock, 0, st>>>(
        c.cam, c.band, c.n_pix, c.sc, c.tx, c.fill, c.fresnel, ImageClear{}, w.park, w.park + 3 * w.fused_cap, w.thr, w.state, w.hits, d_image, d_hit, d_through, nullptr,
        bg);
    HIP_TRY(hipGetLastError());
    // without the reflection no sample has one: the plane is 0 on the rows of the band
    if (d_reflect) HIP_TRY(hipMemsetAsync(d_reflect + (int64_t)y0 * width, 0, sizeof(float) * (size_t)c.n_pix, st));
    return DRT_OK;
}

int drt_render_image_loss_env(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                              double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                              const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                              const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                              int64_t* d_count, const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection, void* stream) {
    return env_loss_call(s, d_verts, camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h, tex_w,
                         channels, fill_void, fill_invalid, d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, d_env, env_h, env_w, env_rot9,
                         reflection, nullptr, nullptr, stream, "drt_render_image_loss_env");
}

int drt_render_image_loss_env_param(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                    double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                    const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                    const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                    int64_t* d_count, const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection, double* d_grad_env,
                                    double* d_grad_env_rot, void* stream) {
    return env_loss_call(s, d_verts, camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h, tex_w,
                         channels, fill_void, fill_invalid, d_target, d_weight, d_loss, d_grad_verts, d_grad_ior, d_image, d_count, d_env, env_h, env_w, env_rot9,
                         reflection, d_grad_env, d_grad_env_rot, stream, "drt_render_image_loss_env_param");
}

}  // extern "C"
