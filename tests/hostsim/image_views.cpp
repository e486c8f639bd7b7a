// tests/hostsim/image_views.cpp -- drt_amd/csrc/drt_image_views.h compiled for the host (g++ -ffp-contract=off): the mapping of a band of
// the tall image of k stacked views to (view, x, y, sample) and the lookup of the view's table row, and the image loss of a list of views
// through that mapping in plain loops -- per sample what k_image_start / k_image_loss_resolve / k_image_loss_bwd do under ImageViewTable
// (drt_image_wave.h), with the classes and the face tapes handed in as in tests/hostsim/image_loss.cpp (no tracer takes part).  Test-only.
#include "../../drt_amd/csrc/drt_image_loss.h"
#include "../../drt_amd/csrc/drt_image_views.h"

using namespace drt;

namespace {

void fill_rows(const double* cams21, const double* screens9, int n_views, ImageViewRow* rows) {
    for (int k = 0; k < n_views; ++k) {
        const double* c = cams21 + 21 * k;
        const double* q = screens9 + 9 * k;
        memcpy(rows[k].cam.kinv, c, sizeof(double) * 9);
        memcpy(rows[k].cam.rinv, c + 9, sizeof(double) * 12);
        rows[k].sc = ImageScreen{d3{q[0], q[1], q[2]}, d3{q[3], q[4], q[5]}, d3{q[6], q[7], q[8]}};
    }
}

ImageViewIds ids_of(const int* view_ids, int k, int H) {
    ImageViewIds ids{};
    ids.height = H; ids.k = k;
    for (int j = 0; j < k; ++j) ids.id[j] = view_ids[j];
    return ids;
}

// sample i of the band that starts at row r0 -> (x, r, j), the arithmetic of band_sample (drt_image_wave.h)
void band_of(int W, int r0, int s, unsigned i, int& x, int& r, int& j) {
    const unsigned s2 = (unsigned)(s * s), pix = i / s2;
    j = (int)(i - pix * s2);
    r = r0 + (int)(pix / (unsigned)W);
    x = (int)(pix % (unsigned)W);
}

template <bool SNELL, bool FRESNEL>
double views_loss(const ImageViewRow* rows, const ImageViewIds& ids, int W, int s, const ImageTex& tx, const PathCtx& c, const int32_t* cls,
                  const int32_t* tape, const uint8_t* hits, const double* fill_void, const double* fill_invalid, const float* targets, const float* weights,
                  double* grad_verts, double* g_ior, int64_t* count) {
    const int s2 = s * s, H = ids.height;
    const int64_t n_pix = (int64_t)ids.k * H * W, n = n_pix * s2;
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    double loss = 0.0;
    for (int64_t pix = 0; pix < n_pix; ++pix) {
        int x, r, j0, slot, view, y;
        band_of(W, 0, s, (unsigned)(pix * s2), x, r, j0);
        image_views_row(ids, r, slot, view, y);
        const ImageViewRow& row = rows[view];
        d3 eo[kImageMaxSuper * kImageMaxSuper], ed[kImageMaxSuper * kImageMaxSuper];
        double eT[kImageMaxSuper * kImageMaxSuper];
        double acc[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            d3 o, d;
            image_sample_ray(row.cam, s, x, y, j, o, d);
            double T = 1.0;
            if (cls[i] == kImageThrough) {
                int n_refr = 0;
                for (int k = 0; k < (int)hits[i]; ++k) image_interact<SNELL, FRESNEL>(c, tape[(int64_t)k * n + i], true, o, d, n_refr, T);
            }
            eo[j] = o; ed[j] = d; eT[j] = T;
            double col[kImageMaxChannels];
            image_sample_colour(row.sc, tx, cls[i], o, d, T, fill_void, fill_invalid, col);
            for (int ch = 0; ch < tx.c; ++ch) acc[ch] = j == 0 ? col[ch] : acc[ch] + col[ch];
        }
        const int64_t at = ((int64_t)view * H + y) * W + x;
        double mean[kImageMaxChannels], g_c[kImageMaxChannels];
        for (int ch = 0; ch < tx.c; ++ch) mean[ch] = acc[ch] / (double)s2;
        loss += image_loss_pixel(mean, tx.c, s2, targets + at * tx.c, weights ? (double)weights[at] : 1.0, g_c);
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            if (cls[i] != kImageThrough) continue;
            d3 o, d;
            image_sample_ray(row.cam, s, x, y, j, o, d);
            double gi, ge;
            if (image_sample_backward<SNELL, FRESNEL>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], row.sc, tx, g_c, add, gi, ge)) {
                g_ior[0] += gi; g_ior[1] += ge;
                ++*count;
            }
        }
    }
    return loss;
}

}  // namespace

extern "C" {

int iv_row_bytes() { return (int)sizeof(ImageViewRow); }

// Every sample i of the band [r0, r1) of k stacked views: x, y, j, slot, view [n]; mark [n]: rinv[3] of the table row the view selects
// (the camera's x position, as the test set it), at [n, 2] the row of the target stack and the band pixel.
void iv_map(const double* cams21, const double* screens9, int n_views, const int* view_ids, int k, int H, int W, int s, int r0, int r1, int32_t* x, int32_t* y,
            int32_t* j, int32_t* slot, int32_t* view, double* mark, int64_t* at) {
    ImageViewRow* rows = new ImageViewRow[n_views];
    fill_rows(cams21, screens9, n_views, rows);
    const ImageViewIds ids = ids_of(view_ids, k, H);
    const unsigned n = (unsigned)((r1 - r0) * W * s * s);
    for (unsigned i = 0; i < n; ++i) {
        int xx, r, jj, sl, vw, yy;
        band_of(W, r0, s, i, xx, r, jj);
        image_views_row(ids, r, sl, vw, yy);
        x[i] = xx; y[i] = yy; j[i] = jj; slot[i] = sl; view[i] = vw;
        mark[i] = rows[vw].cam.rinv[3];
        at[2 * i] = ((int64_t)vw * H + yy) * W + xx;
        at[2 * i + 1] = i / (unsigned)(s * s);
    }
    delete[] rows;
}

// image_sample_ray of every sample of view `view` (H x W, s) through the table row, o and d [n, 3] each, and through a by-value camera
void iv_rays(const double* cams21, const double* screens9, int n_views, int view, int H, int W, int s, double* via_table, double* by_value) {
    ImageViewRow* rows = new ImageViewRow[n_views];
    fill_rows(cams21, screens9, n_views, rows);
    const int ids1[1] = {view};
    const ImageViewIds ids = ids_of(ids1, 1, H);
    ImageCam cam;
    memcpy(cam.kinv, cams21 + 21 * view, sizeof(double) * 9);
    memcpy(cam.rinv, cams21 + 21 * view + 9, sizeof(double) * 12);
    const int64_t n = (int64_t)H * W * s * s;
    for (int64_t i = 0; i < n; ++i) {
        int x, r, j, slot, vw, y;
        band_of(W, 0, s, (unsigned)i, x, r, j);
        image_views_row(ids, r, slot, vw, y);
        d3 o, d;
        image_sample_ray(rows[vw].cam, s, x, y, j, o, d);
        store_d3(via_table, i, o); store_d3(via_table + 3 * n, i, d);
        image_sample_ray(cam, s, x, r, j, o, d);
        store_d3(by_value, i, o); store_d3(by_value + 3 * n, i, d);
    }
    delete[] rows;
}

// The loss of the listed views (returned) with its adjoint, over the whole tall image: grad_verts [V, 3], g_ior [2] and *count are added
// into.  cls int32 [n], tape int32 [K, n], hits uint8 [n] with n = k H W s^2, the listed views' one after the other; targets
// [n_views, H, W, C] and weights [n_views, H, W] (may be null) are indexed by view id.
double iv_views_loss(const double* cams21, const double* screens9, int n_views, const int* view_ids, int k, int H, int W, int s, const float* texel, int th,
                     int tw, int ch, const int32_t* faces, const double* verts, double ior_int, double ior_ext, int snell, int fresnel, const int32_t* cls,
                     const int32_t* tape, const uint8_t* hits, const double* fill_void, const double* fill_invalid, const float* targets,
                     const float* weights, double* grad_verts, double* g_ior, int64_t* count) {
    ImageViewRow* rows = new ImageViewRow[n_views];
    fill_rows(cams21, screens9, n_views, rows);
    const ImageViewIds ids = ids_of(view_ids, k, H);
    const ImageTex tx{texel, th, tw, ch};
    const PathCtx c{TraceCtx{nullptr, nullptr, 0, nullptr}, faces, verts, ior_int, ior_ext};
    double loss;
#define IV(SN, FR) views_loss<SN, FR>(rows, ids, W, s, tx, c, cls, tape, hits, fill_void, fill_invalid, targets, weights, grad_verts, g_ior, count)
    if (snell) loss = fresnel ? IV(true, true) : IV(true, false);
    else loss = fresnel ? IV(false, true) : IV(false, false);
#undef IV
    delete[] rows;
    return loss;
}

}  // extern "C"
