// tests/hostsim/image_views_env.cpp -- the image term of several views in front of one environment, compiled for the host (g++
// -ffp-contract=off): drt_amd/csrc/drt_image_views.h's mapping of a band of the tall image to (view, y) and drt_image_env.h's law in plain
// loops -- per sample what k_image_reflect_list, k_image_loss_resolve, k_image_loss_bwd and k_image_reflect_bwd do under ImageViewTable
// (drt_image_env_loss.h, drt_image_loss_bwd.h), with the classes, the face tapes and the occlusion verdicts handed in as in
// tests/hostsim/image_env.cpp (no tracer takes part).  Test-only.
#include "../../drt_amd/csrc/drt_image_env.h"
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

ImageEnv env_of(const float* texel, int eh, int ew, int c, const double* R9) {
    ImageEnv e{texel, eh, ew, c, {}};
    memcpy(e.rot, R9, sizeof(double) * 9);
    return e;
}

// tests/hostsim/image_env.cpp's env_view over the tall image: camera, screen and the row within the view come from the table row of the
// sample's band row; target and weight are addressed at ((view * H + y) * W + x).
template <bool SNELL>
double views_env_loss(const ImageViewRow* rows, const ImageViewIds& ids, int W, int s, const ImageTex& tx, bool has_screen, const ImageEnv& env, const PathCtx& c,
                      const int32_t* cls, const int32_t* tape, const uint8_t* hits, const uint8_t* seen, bool reflection, const double* fill_invalid,
                      const float* targets, const float* weights, double* grad_verts, double* g_ior, int64_t* count) {
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
            d3 o, d, co, cd;
            image_sample_ray(row.cam, s, x, y, j, o, d);
            co = o; cd = d;
            double T = 1.0;
            if (cls[i] == kImageThrough) {
                int n_refr = 0;
                for (int k = 0; k < (int)hits[i]; ++k) image_interact<SNELL, true>(c, tape[(int64_t)k * n + i], true, o, d, n_refr, T);
            }
            eo[j] = o; ed[j] = d; eT[j] = T;
            double col[kImageMaxChannels];
            image_env_sample_colour(row.sc, tx, has_screen, env, cls[i], o, d, T, fill_invalid, col);
            if (reflection && cls[i] == kImageThrough && seen[i]) {
                d3 ro, wr;
                double R1;
                if (image_reflect_first<SNELL>(c, tape[i], co, cd, ro, wr, R1)) image_env_add_reflection(row.sc, tx, has_screen, env, ro, wr, R1, col);
            }
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
            if (image_env_sample_backward<SNELL, true>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], row.sc, tx, has_screen, env, g_c, add, gi, ge)) {
                g_ior[0] += gi; g_ior[1] += ge;
                ++*count;
            }
            if (reflection && seen[i] && image_reflect_backward<SNELL>(c, tape[i], o, d, row.sc, tx, has_screen, env, g_c, add, gi, ge)) {
                g_ior[0] += gi; g_ior[1] += ge;
            }
        }
    }
    return loss;
}

}  // namespace

extern "C" {

// What the reflection list forms for every sample i of the band [r0, r1) of k stacked views, THROUGH THE TABLE ROW of the sample's band row:
// the camera ray (cam_ray float64 [2, n, 3]: origins, then directions) and, from first_face[i] (< 0: none), qual uint8 [n], ro / wr
// float64 [n, 3], R1 float64 [n] (written where qual).
void ive_reflect_band(const double* cams21, const double* screens9, int n_views, const int* view_ids, int k, int H, int W, int s, int r0, int r1,
                      const int32_t* faces, const double* verts, int n_tris, double ior_ext, double ior_int, int snell, const int32_t* first_face,
                      double* cam_ray, uint8_t* qual, double* ro, double* wr, double* R1) {
    ImageViewRow* rows = new ImageViewRow[n_views];
    fill_rows(cams21, screens9, n_views, rows);
    const ImageViewIds ids = ids_of(view_ids, k, H);
    PathCtx c{};
    c.tc.n_tris = n_tris; c.faces = faces; c.verts = verts; c.ior_int = ior_int; c.ior_ext = ior_ext;
    const int64_t n = (int64_t)(r1 - r0) * W * s * s;
    for (int64_t i = 0; i < n; ++i) {
        int x, r, j, slot, view, y;
        band_of(W, r0, s, (unsigned)i, x, r, j);
        image_views_row(ids, r, slot, view, y);
        d3 o, d, a, b;
        double q = 0.0;
        image_sample_ray(rows[view].cam, s, x, y, j, o, d);
        store_d3(cam_ray, i, o); store_d3(cam_ray + 3 * n, i, d);
        qual[i] = snell ? image_reflect_first<true>(c, first_face[i], o, d, a, b, q) : image_reflect_first<false>(c, first_face[i], o, d, a, b, q);
        if (qual[i]) { store_d3(ro, i, a); store_d3(wr, i, b); R1[i] = q; }
    }
    delete[] rows;
}

// The same of every sample of ONE view of H x W at supersampling s through its by-value camera (tests/hostsim/image_env.cpp's env_reflect,
// with the camera ray handed out): the single-view call.
void ive_reflect_view(const double* cam21, int H, int W, int s, const int32_t* faces, const double* verts, int n_tris, double ior_ext, double ior_int, int snell,
                      const int32_t* first_face, double* cam_ray, uint8_t* qual, double* ro, double* wr, double* R1) {
    PathCtx c{};
    c.tc.n_tris = n_tris; c.faces = faces; c.verts = verts; c.ior_int = ior_int; c.ior_ext = ior_ext;
    ImageCam cam;
    memcpy(cam.kinv, cam21, sizeof(double) * 9);
    memcpy(cam.rinv, cam21 + 9, sizeof(double) * 12);
    const int64_t n = (int64_t)H * W * s * s;
    int64_t i = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int j = 0; j < s * s; ++j, ++i) {
                d3 o, d, a, b;
                double q = 0.0;
                image_sample_ray(cam, s, x, y, j, o, d);
                store_d3(cam_ray, i, o); store_d3(cam_ray + 3 * n, i, d);
                qual[i] = snell ? image_reflect_first<true>(c, first_face[i], o, d, a, b, q) : image_reflect_first<false>(c, first_face[i], o, d, a, b, q);
                if (qual[i]) { store_d3(ro, i, a); store_d3(wr, i, b); R1[i] = q; }
            }
}

// The loss of the listed views in front of the environment (returned) with its adjoint, over the whole tall image, Fresnel on: grad_verts
// [V, 3], g_ior [2] and *count are added into.  cls int32 [n], tape int32 [K, n], hits / seen uint8 [n] with n = k H W s^2, the listed
// views' one after the other; targets [n_views, H, W, C] and weights [n_views, H, W] (may be null) are indexed by view id.  tex null: no
// screen (the table's screens are then never read).
double ive_views_loss(const double* cams21, const double* screens9, int n_views, const int* view_ids, int k, int H, int W, int s, const float* tex, int th, int tw,
                      int ch, const float* texel, int eh, int ew, const double* R9, const int32_t* faces, const double* verts, int n_tris, double ior_int,
                      double ior_ext, int snell, int reflection, const int32_t* cls, const int32_t* tape, const uint8_t* hits, const uint8_t* seen,
                      const double* fill_invalid, const float* targets, const float* weights, double* grad_verts, double* g_ior, int64_t* count) {
    ImageViewRow* rows = new ImageViewRow[n_views];
    fill_rows(cams21, screens9, n_views, rows);
    const ImageViewIds ids = ids_of(view_ids, k, H);
    const bool has_screen = tex != nullptr;
    const ImageTex tx{has_screen ? tex : nullptr, has_screen ? th : 2, has_screen ? tw : 2, ch};
    const ImageEnv e = env_of(texel, eh, ew, ch, R9);
    const PathCtx c{TraceCtx{nullptr, nullptr, n_tris, nullptr}, faces, verts, ior_int, ior_ext};
    const double loss = snell ? views_env_loss<true>(rows, ids, W, s, tx, has_screen, e, c, cls, tape, hits, seen, reflection != 0, fill_invalid, targets, weights,
                                                     grad_verts, g_ior, count)
                              : views_env_loss<false>(rows, ids, W, s, tx, has_screen, e, c, cls, tape, hits, seen, reflection != 0, fill_invalid, targets, weights,
                                                      grad_verts, g_ior, count);
    delete[] rows;
    return loss;
}

}  // extern "C"
