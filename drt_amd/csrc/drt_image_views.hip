// drt_image_views.hip -- the photometric image term of up to 16 views as ONE forward wavefront and ONE adjoint pass (drt_image_views.h
// holds the mapping).  The result is the sum over the listed views of what drt_render_image_loss gives for each; the
// per-sample device functions are that call's.  The kernels are the family's templates (drt_image_wave.h, drt_image_loss_bwd.h) under
// the view policy ImageViewTable; this unit holds those forms.  A unit of its own because a kernel's register allocation depends on the
// other kernels of its unit (drt_image_loss_bwd.h): the single-view instantiations keep their figures.
//
//   view table                      : ImageViewRow [n_views] in device memory, made once per capture (drt_image_views_create)
//   image_forward_from  all samples : drt_image.hip's wavefront with k_image_start<ImageViewTable>: the sample's camera read from its
//                                     view's table row
//   k_image_loss_resolve            : <., ImageViewTable, ImageClear>: the pixel's camera and screen read from its view's table row; target
//                                     and weight are the capture's stacks, addressed at ((view * H + y) * W + x)
//   k_paths_collect                 : drt_paths.hip's, unchanged
//   k_image_loss_bwd                : <.., ImageViewTable, ImageClear> without CAMERA: the sample's camera and screen are references into the
//                                     table, read where image_sample_ray and the plane adjoint use them
// A band is rows [r0, r1) of the tall image of k * H rows and may straddle a view border; inside it everything is indexed as in the
// single-view call (sample i -> band pixel i / s^2; seeds under the band pixel; parked rows, state, hits and tape under i).
// The slot -> view id list reaches the kernels by value (ImageViewIds) and is resolved by an unrolled select (image_views_id): the call
// stays capturable and copies nothing to the device per step.
#include "drt_image_loss_bwd.h"
#include "drt_image_views_host.h"

namespace {

void views_release(drt_image_views* v) {
    (void)hipFree(v->d_rows);
    delete[] v->cam21;
    delete[] v->scr9;
    delete v;
}

}  // namespace

void image_start_views(const ImageStartArgs& a, const void* src) {
    const ViewsStart& v = *static_cast<const ViewsStart*>(src);
    k_image_start<<<a.grid, kPathBlock, 0, a.st>>>(a.nodes, a.n_tris, v.view, v.band, a.park_ori, a.park_dir, a.thr, a.state, a.hits, a.out, a.count);
}

void image_views_free(drt_scene* s) {
    drt_image_views* v = static_cast<drt_image_views*>(s->image_views);
    while (v) {
        drt_image_views* const next = v->next;
        views_release(v);
        v = next;
    }
    s->image_views = nullptr;
}

extern "C" {

int drt_image_views_check(int n_views, const double* cameras21, const double* screens9, int height, int width) {
    if (n_views < 1) return fail(DRT_E_INVALID, "n_views = %d: a view table has at least one view", n_views);
    if (height < 1 || width < 1) return fail(DRT_E_INVALID, "height x width = %d x %d: the image must have at least one pixel", height, width);
    if (height > INT32_MAX / kImageViewsMax) return fail(DRT_E_INVALID, "height = %d: %d views of it must stack into fewer than 2^31 rows", height, kImageViewsMax);
    if (!cameras21 || !screens9) return fail(DRT_E_INVALID, "null host pointer argument (cameras21, screens9)");
    for (int k = 0; k < n_views; ++k) {
        const double* q = screens9 + 9 * (size_t)k;
        if (!image_screen_ok(ImageScreen{d3{q[0], q[1], q[2]}, d3{q[3], q[4], q[5]}, d3{q[6], q[7], q[8]}}))
            return fail(DRT_E_INVALID, "screens9 row %d: the axes eu, ev must be finite, non-zero and orthogonal (|eu . ev| <= 1e-12 |eu| |ev|)", k);
    }
    return DRT_OK;
}

int drt_image_views_create(drt_scene_t* s, int n_views, const double* cameras21, const double* screens9, int height, int width, drt_image_views_t** out) {
    CHECK_SCENE(s);
    if (!out) return fail(DRT_E_INVALID, "out is null");
    { int rc = drt_image_views_check(n_views, cameras21, screens9, height, width); if (rc) return rc; }
    drt_image_views* v = new (std::nothrow) drt_image_views();
    ImageViewRow* rows = new (std::nothrow) ImageViewRow[n_views];
    if (v) { v->cam21 = new (std::nothrow) double[(size_t)n_views * 21]; v->scr9 = new (std::nothrow) double[(size_t)n_views * 9]; }
    if (!v || !rows || !v->cam21 || !v->scr9) {
        delete[] rows;
        if (v) views_release(v);
        return fail(DRT_E_NOMEM, "host allocation failed");
    }
    for (int k = 0; k < n_views; ++k) {
        const double* c = cameras21 + 21 * (size_t)k;
        const double* q = screens9 + 9 * (size_t)k;
        memcpy(rows[k].cam.kinv, c, sizeof(double) * 9);
        memcpy(rows[k].cam.rinv, c + 9, sizeof(double) * 12);
        rows[k].sc = ImageScreen{d3{q[0], q[1], q[2]}, d3{q[3], q[4], q[5]}, d3{q[6], q[7], q[8]}};
    }
    memcpy(v->cam21, cameras21, sizeof(double) * 21 * (size_t)n_views);
    memcpy(v->scr9, screens9, sizeof(double) * 9 * (size_t)n_views);
    hipError_t e = hipMalloc(&v->d_rows, sizeof(ImageViewRow) * (size_t)n_views);
    if (e == hipSuccess) e = hipMemcpy(v->d_rows, rows, sizeof(ImageViewRow) * (size_t)n_views, hipMemcpyHostToDevice);
    delete[] rows;
    if (e != hipSuccess) {
        views_release(v);
        return fail(DRT_E_HIP, "drt_image_views_create: %s", hipGetErrorString(e));
    }
    v->scene = s; v->n_views = n_views; v->height = height; v->width = width;
    v->next = static_cast<drt_image_views*>(s->image_views);
    s->image_views = v;
    *out = v;
    return DRT_OK;
}

void drt_image_views_destroy(drt_image_views_t* v) {
    if (!v) return;
    if (v->scene) {
        void** link = &v->scene->image_views;
        while (*link && *link != v) link = reinterpret_cast<void**>(&static_cast<drt_image_views*>(*link)->next);
        if (*link == v) *link = v->next;
    }
    views_release(v);
}

int drt_render_image_loss_views(drt_scene_t* s, const double* d_verts, const drt_image_views_t* views, const int* view_ids, int k, int r0, int r1,
                                int supersample, double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const float* d_texture,
                                int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid, const float* d_targets,
                                const float* d_weights, double* d_loss, double* d_grad_verts, double* d_grad_ior, int64_t* d_count, void* stream) {
    const char* const who = "drt_render_image_loss_views";
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
    ImageCall c;          // (its camera and screen are the first listed view's and are not used: every kernel reads the table)
    { int rc = image_call_check(views->cam21 + 21 * (size_t)ids.id[0], k * views->height, views->width, r0, r1, supersample, ior_int, ior_ext, max_bounces, law_flags,
                                fresnel, views->scr9 + 9 * (size_t)ids.id[0], d_texture, tex_h, tex_w, channels, fill_void, fill_invalid,
                                d_texture && d_targets && d_loss && (s->n_faces == 0 || d_verts),
                                "null device pointer argument (d_verts, d_texture, d_targets, d_loss)", c); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;
    const ViewsStart vs{ImageViewTable{views->d_rows, ids}, c.band};
    return image_loss_run(s, d_verts, c, vs.view, ImageClear{}, [&](ImageClear&) { return image_forward_from(s, d_verts, c, true, st, who, image_start_views, &vs); },
                          image_loss_bwd_launch<ImageViewTable, ImageClear, false>,
                          ImageLossOut{d_targets, d_weights, d_loss, d_grad_verts, d_grad_ior, nullptr, d_count, nullptr}, 0, st, who);
}

}  // extern "C"
