// drt_image.hip -- the forward renderer (drt_image.h holds the law): the refracted image of the mesh in front of a textured planar
// screen, one band of rows per call, as the wavefront loop of drt_paths.hip with the rays made in the kernel.  The forward wavefront
// (image_forward / image_forward_from, declared in drt_image_wave.h) is also what every loss call of the family starts with.  The kernels
// are drt_image_wave.h's templates; this unit holds the clear single-view forms: k_image_start<ImageOneView>,
// k_image_shade<., ., ., ImageClear>, k_image_resolve<ImageClear>.
//
//   k_image_start   all samples : forms the sample ray (image_sample_ray), top-box test; candidates -> list 0 (index + float32 ray), their
//                                 float64 ray and a throughput of 1 parked in the workspace; one state byte and one hit count per sample
//   per interaction k = 0 .. K (drt_pathws.h trace_lists):
//     k_trace       list k      : drt_trace.hip's, through launch_trace_list, unchanged
//     k_image_shade list k      : k_paths_shade plus the throughput update (image_interact); TAPE: the loss's form, which records the face of
//                                 the interaction in the tape of the workspace -- the renderer's own form leaves the tape alone
//   k_image_resolve all pixels  : walks the s x s contiguous samples of its pixel in order (image_pixel_walk): class, screen plane, bilinear
//                                 fetch, weight, mean
// Sample i of a band belongs to pixel i / s^2 (pixel-major, sample-minor: a wave covers neighbouring pixels).  No origin / dir tensor
// exists at any point: a sample without interaction has its camera ray formed again by the resolve kernel -- the same function, the same
// bits.  Every list size stays on the device, nothing is read back, all launches go to the caller's stream.  The only atomics are the
// list appends' reservations; a list's ORDER is never read (every value is stored under its sample index), so two runs give the same bits.
#include "drt_image_wave.h"

int grow_doubles(double*& buf, int64_t& cap, int64_t n, hipStream_t st, const char* who, const char* what) {
    if (n <= cap) return DRT_OK;
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &capturing) == hipSuccess && capturing != hipStreamCaptureStatusNone)
        return fail(DRT_E_INVALID, "%s: the first call of this size allocates its %s and cannot run "
                                   "inside a stream capture: issue one such call eagerly before capturing", who, what);
    (void)hipFree(buf);
    buf = nullptr; cap = 0;
    HIP_TRY(hipMalloc(&buf, sizeof(double) * (size_t)n));
    cap = n;
    return DRT_OK;
}

int image_call_check(const double* camera21, int height, int width, int y0, int y1, int supersample, double ior_int, double ior_ext, int max_bounces,
                     int law_flags, int fresnel, const double* screen9, const float* d_texture, int tex_h, int tex_w, int channels,
                     const double* fill_void, const double* fill_invalid, bool device_ok, const char* device_msg, ImageCall& call) {
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
    if (!device_ok) return fail(DRT_E_INVALID, "%s", device_msg);
    memcpy(call.cam.kinv, camera21, sizeof(double) * 9);
    memcpy(call.cam.rinv, camera21 + 9, sizeof(double) * 12);
    call.sc = ImageScreen{d3{screen9[0], screen9[1], screen9[2]}, d3{screen9[3], screen9[4], screen9[5]}, d3{screen9[6], screen9[7], screen9[8]}};
    if (!image_screen_ok(call.sc)) return fail(DRT_E_INVALID, "screen9: the axes eu, ev must be finite, non-zero and orthogonal (|eu . ev| <= 1e-12 |eu| |ev|)");
    const int s2 = supersample * supersample;
    call.n_pix = (int64_t)(y1 - y0) * width;
    call.n = call.n_pix * s2;
    if (call.n > INT32_MAX) return fail(DRT_E_INVALID, "the band has %lld samples: at most 2^31 - 1 per call (render fewer rows)", (long long)call.n);
    call.tx = ImageTex{d_texture, tex_h, tex_w, channels};
    call.fill = ImageFill{};
    for (int ch = 0; ch < channels; ++ch) { call.fill.c_void[ch] = fill_void[ch]; call.fill.c_invalid[ch] = fill_invalid[ch]; }
    call.band = ImageBand{width, y0, supersample, (unsigned)call.n};
    call.ior_int = ior_int; call.ior_ext = ior_ext;
    call.max_bounces = max_bounces;
    call.reflect = (law_flags & DRT_LAW_REFLECT) != 0; call.snell = (law_flags & DRT_LAW_SNELL) != 0; call.fresnel = fresnel != 0;
    return DRT_OK;
}

// image_forward's own start: k_image_start with the camera of the call (`src`)
void image_start_call(const ImageStartArgs& a, const void* src) {
    const ImageCall& c = *static_cast<const ImageCall*>(src);
    k_image_start<<<a.grid, kPathBlock, 0, a.st>>>(a.nodes, a.n_tris, ImageOneView{c.cam, c.sc}, c.band, a.park_ori, a.park_dir, a.thr, a.state, a.hits, a.out,
                                                   a.count);
}

// image_forward_from's default shade: the clear forms, what every call without a shade hook launches
static void image_shade_clear(const ImageShadeArgs& a, const void*) { image_shade_launch(a, ImageClear{}); }

int image_forward_from(drt_scene* s, const double* d_verts, const ImageCall& c, bool keep_tape, hipStream_t st, const char* who, ImageStartFn start,
                       const void* src, ImageShadeFn shade_fn, const void* shade_src) {
    { int rc = ensure_paths_ws(s, c.n, st, who); if (rc) return rc; }
    { int rc = ensure_paths_fused_ws(s, c.n, st, who); if (rc) return rc; }
    { PathsWs* w = paths_ws_of(s); int rc = grow_doubles(w->thr, w->thr_cap, c.n, st, who, "throughputs"); if (rc) return rc; }
    { int rc = wait_build(s, st); if (rc) return rc; }
    if (!shade_fn) shade_fn = image_shade_clear;
    const PathsWs& w = *paths_ws_of(s);
    const PathCtx pc = image_path_ctx(s, d_verts, c);
    const int gs = grid_for(c.n, kPathBlock, 8 * s->n_cu);
    double* const park_ori = w.park;                 // the rows of the one-pass form: scratch to every call
    double* const park_dir = w.park + 3 * w.fused_cap;
    HIP_TRY(hipMemsetAsync(w.cnt, 0, sizeof(unsigned) * kCntWords, st));
    const RayList l0{w.idx[0], w.ray[0], w.face[0]};
    start(ImageStartArgs{pc.tc.nodes, pc.tc.n_tris, park_ori, park_dir, w.thr, w.state, w.hits, l0, w.cnt + kCntList, gs, st}, src);
    if (s->n_faces > 0) {
        int32_t* const tape = keep_tape ? w.tape : nullptr;
        trace_lists(s, w, pc.tc, st, c.max_bounces, [&](int k, const RayList& in, const unsigned* n_in, const RayList& out, unsigned* n_out) {
            shade_fn(ImageShadeArgs{pc, (int64_t)c.n, k, c.max_bounces, c.reflect, c.snell, c.fresnel, in, n_in, out, n_out, park_ori, park_dir, w.thr, w.state,
                                    w.hits, tape, gs, st}, shade_src);
        });
    }
    return DRT_OK;
}

int image_forward(drt_scene* s, const double* d_verts, const ImageCall& c, bool keep_tape, hipStream_t st, const char* who) {
    return image_forward_from(s, d_verts, c, keep_tape, st, who, image_start_call, &c);
}

extern "C" {

int drt_render_image(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                     double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                     const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                     float* d_image, float* d_hit, float* d_through, void* stream) {
    CHECK_BUILT(s);
    ImageCall c;
    { int rc = image_call_check(camera21, height, width, y0, y1, supersample, ior_int, ior_ext, max_bounces, law_flags, fresnel, screen9, d_texture, tex_h, tex_w,
                                channels, fill_void, fill_invalid, d_texture && d_image && (s->n_faces == 0 || d_verts),
                                "null device pointer argument (d_verts, d_texture, d_image)", c); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    { int rc = image_forward(s, d_verts, c, false, st, "drt_render_image"); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    k_image_resolve<<<(unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock), kPathBlock, 0, st>>>(
        c.cam, c.band, c.n_pix, c.sc, c.tx, c.fill, c.fresnel, ImageClear{}, w.park, w.park + 3 * w.fused_cap, w.thr, w.state, w.hits, d_image, d_hit, d_through, nullptr);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

}  // extern "C"
