// drt_image_views.hip -- the photometric image term of up to 16 views as ONE forward wavefront and ONE adjoint pass (drt_image_views.h
// holds the mapping).  The result is the sum over the listed views of what drt_render_image_loss gives for each; the
// per-sample device functions are that call's, unchanged.  A unit of its own because a kernel's register allocation depends on the
// other kernels of its unit (drt_image_loss_bwd.h): the single-view instantiations keep their figures.
//
//   view table                      : ImageViewRow [n_views] in device memory, made once per capture (drt_image_views_create)
//   image_forward_from  all samples : drt_image.hip's wavefront with k_image_views_start in the place of k_image_start
//   k_image_views_start             : k_image_start with the sample's camera read from its view's table row
//   k_image_views_loss_resolve      : k_image_loss_resolve with the pixel's camera and screen read from its view's table row; target and
//                                     weight are the capture's stacks, addressed at ((view * H + y) * W + x)
//   k_paths_collect                 : drt_paths.hip's, unchanged
//   k_image_views_loss_bwd          : k_image_loss_bwd (without CAMERA) whose sample hands loss_bwd_sample the table row's camera and screen
// A band is rows [r0, r1) of the tall image of k * H rows and may straddle a view border; inside it everything is indexed as in the
// single-view call (sample i -> band pixel i / s^2; seeds under the band pixel; parked rows, state, hits and tape under i).
// The slot -> view id list reaches the kernels by value (ImageViewIds) and is resolved by an unrolled select (image_views_id): the call
// stays capturable and copies nothing to the device per step.
#include "drt_image_loss_bwd.h"
#include "drt_image_views.h"

struct drt_image_views {
    drt_scene* scene = nullptr;
    int n_views = 0, height = 0, width = 0;
    ImageViewRow* d_rows = nullptr;
    double* cam21 = nullptr;               // host copies [n_views, 21] / [n_views, 9]: what image_call_check reads of the first listed view
    double* scr9 = nullptr;
    drt_image_views* next = nullptr;       // the scene's list (drt_scene::image_views)
};

// sample i of the band -> pixel column, row within its view, sample number, the view's table row
__device__ __forceinline__ const ImageViewRow& views_sample(const ImageViewRow* __restrict__ rows, const ImageViewIds& ids, const ImageBand& band, unsigned i,
                                                            int& x, int& y, int& j) {
    int r, slot, view;
    band_sample(band, i, x, r, j);
    image_views_row(ids, r, slot, view, y);
    return rows[view];
}

__global__ void __launch_bounds__(kPathBlock) k_image_views_start(const Node4Q* __restrict__ nodes, int n_tris, const ImageViewRow* __restrict__ rows,
                                                                   ImageViewIds ids, ImageBand band, double* __restrict__ park_ori,
                                                                   double* __restrict__ park_dir, double* __restrict__ thr, uint8_t* __restrict__ state,
                                                                   uint8_t* __restrict__ hits, RayList out, unsigned* count) {
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
                const ImageViewRow& row = views_sample(rows, ids, band, i, x, y, j);
                d3 o, d;
                image_sample_ray(row.cam, band.s, x, y, j, o, d);
                o32 = to_f32(o); d32 = to_f32(d);
                cand = hits_top_boxes(nodes, o32, d32);
                if (cand) { store_d3(park_ori, i, o); store_d3(park_dir, i, d); thr[i] = 1.0; }
            }
        }
        stage_push(stage, cand, (int32_t)i, o32, d32, out, count);
    }
    stage_flush(stage, out, count);
}

// One thread per pixel of the band.  target [n_views, H, W, C] and weight [n_views, H, W] (may be null) are the capture's stacks.
template <bool DET>
__global__ void __launch_bounds__(kPathBlock) k_image_views_loss_resolve(const ImageViewRow* __restrict__ rows, ImageViewIds ids, ImageBand band, int64_t n_pix,
                                                                          ImageTex tx, ImageFill fill, bool fresnel, const double* __restrict__ park_ori,
                                                                          const double* __restrict__ park_dir, const double* __restrict__ thr,
                                                                          const uint8_t* __restrict__ state, const uint8_t* __restrict__ hits,
                                                                          const float* __restrict__ target, const float* __restrict__ weight,
                                                                          double* __restrict__ g_c, double* loss) {
    const int64_t pix = (int64_t)blockIdx.x * kPathBlock + threadIdx.x;
    LossAcc<DET> acc;
    if (pix < n_pix) {
        const int s2 = band.s * band.s;
        const int r = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
        int slot, view, y;
        image_views_row(ids, r, slot, view, y);
        const ImageViewRow& vr = rows[view];
        double sum[kImageMaxChannels] = {0.0, 0.0, 0.0};
        int n_hit, n_through;          // (not wanted here)
        image_pixel_walk(vr.cam, band, pix, x, y, vr.sc, tx, fill, fresnel, park_ori, park_dir, thr, state, hits, sum, n_hit, n_through);
        const int64_t row = ((int64_t)view * ids.height + y) * band.width + x;
        double mean[kImageMaxChannels], g[kImageMaxChannels];
        for (int ch = 0; ch < tx.c; ++ch) mean[ch] = sum[ch] / (double)s2;
        acc.add(image_loss_pixel(mean, tx.c, s2, target + row * tx.c, weight ? (double)weight[row] : 1.0, g));
        for (int ch = 0; ch < tx.c; ++ch) g_c[pix * tx.c + ch] = g[ch];
    }
    acc.flush(loss);
}

// k_image_loss_bwd<DET, SNELL, FRESNEL, VERTS, false> with the table lookup in front of loss_bwd_sample: the sample's band is the call's
// with its first row moved to the top of the sample's slot, so that band_sample gives the row within the view; camera and screen are
// handed over as references into the table, read where image_sample_ray and the plane adjoint use them.
template <bool DET, bool SNELL, bool FRESNEL, bool VERTS>
__global__ void __launch_bounds__(256) k_image_views_loss_bwd(PathCtx c, const ImageViewRow* __restrict__ rows, ImageViewIds ids, ImageBand band, ImageTex tx,
                                                              int max_bounces, const double* __restrict__ park_ori, const double* __restrict__ park_dir,
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
        int x, r, j, slot, view, y;
        band_sample(band, (unsigned)i, x, r, j);
        image_views_row(ids, r, slot, view, y);
        ImageBand in_view = band;
        in_view.y0 = band.y0 - slot * ids.height;
        const ImageViewRow& row = rows[view];
        double gi, ge;
        if (loss_bwd_sample<SNELL, FRESNEL>(c, row.cam, in_view, row.sc, tx, max_bounces, park_ori, park_dir, thr, tape, hits, g_c, i, add, gi, ge)) {
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

using ViewsBwd = void (*)(PathCtx, const ImageViewRow*, ImageViewIds, ImageBand, ImageTex, int, const double*, const double*, const double*, const int32_t*,
                          const uint8_t*, const int32_t*, const unsigned*, const double*, double*, double*, unsigned long long*);
// k_image_views_loss_bwd under (deterministic, snell, fresnel, verts)
ViewsBwd views_bwd_kernel(bool det, bool snell, bool fresnel, bool verts) {
#define VB(D, S) k_image_views_loss_bwd<D, S, false, false>, k_image_views_loss_bwd<D, S, false, true>, k_image_views_loss_bwd<D, S, true, false>, \
                 k_image_views_loss_bwd<D, S, true, true>
    static const ViewsBwd kernels[16] = {VB(false, false), VB(false, true), VB(true, false), VB(true, true)};
#undef VB
    return kernels[(det ? 8 : 0) | (snell ? 4 : 0) | (fresnel ? 2 : 0) | (verts ? 1 : 0)];
}

struct ViewsStart {
    const ImageViewRow* rows;
    ImageViewIds ids;
    ImageBand band;
};
void image_start_views(const ImageStartArgs& a, const void* src) {
    const ViewsStart& v = *static_cast<const ViewsStart*>(src);
    k_image_views_start<<<a.grid, kPathBlock, 0, a.st>>>(a.nodes, a.n_tris, v.rows, v.ids, v.band, a.park_ori, a.park_dir, a.thr, a.state, a.hits, a.out, a.count);
}

void views_release(drt_image_views* v) {
    (void)hipFree(v->d_rows);
    delete[] v->cam21;
    delete[] v->scr9;
    delete v;
}

}  // namespace

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
    { int rc = ensure_image_loss_ws(s, c.n_pix * channels, 0, st, who); if (rc) return rc; }
    const ViewsStart vs{views->d_rows, ids, c.band};
    { int rc = image_forward_from(s, d_verts, c, true, st, who, image_start_views, &vs); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    const ImageLossWs& lw = *static_cast<ImageLossWs*>(s->image_loss_ws);
    const PathCtx pc = image_path_ctx(s, d_verts, c);
    double* const park_ori = w.park;
    double* const park_dir = w.park + 3 * w.fused_cap;
    const bool det = det_mode();
    const unsigned pix_grid = (unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock);
    DET_LAUNCH(k_image_views_loss_resolve, pix_grid, kPathBlock, st, views->d_rows, ids, c.band, c.n_pix, c.tx, c.fill, c.fresnel, park_ori, park_dir, w.thr, w.state,
               w.hits, d_targets, d_weights, lw.g_c, d_loss);
    if (s->n_faces > 0 && (d_grad_verts || d_grad_ior || d_count)) {
        int32_t* const done = w.idx[0];          // (both ping-pong lists are free once the loop has ended)
        launch_paths_collect(grid_for(c.n, kPathBlock, 8 * s->n_cu), st, (unsigned)c.n, w.state, done, w.cnt + kCntValid);
        const int grid = (d_grad_verts ? DRT_BWD_BPC : kImageLossBpc) * s->n_cu;
        views_bwd_kernel(det, c.snell, c.fresnel, d_grad_verts != nullptr)<<<grid, 256, 0, st>>>(
            pc, views->d_rows, ids, c.band, c.tx, c.max_bounces, park_ori, park_dir, w.thr, w.tape, w.hits, done, w.cnt + kCntValid, lw.g_c, d_grad_verts, d_grad_ior,
            reinterpret_cast<unsigned long long*>(d_count));
    }
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}

}  // extern "C"
