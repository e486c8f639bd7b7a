// tests/hostsim/image_views_absorb.cpp -- absorbing glass in the image term of several views, in front of their screens, of one
// environment, or of both, compiled for the host (g++ -ffp-contract=off): drt_amd/csrc/drt_image_views.h's mapping of a
// band of the tall image to (view, y), drt_image_absorb.h's law and drt_image_env.h's with ABSORB / LENGTH in plain loops -- per sample what
// k_image_shade<.., ImageAbsorb>, k_image_loss_resolve<., ImageViewTable, ImageAbsorb, BG>, k_image_loss_bwd<.., ImageViewTable, ImageAbsorb,
// ., BG> and k_image_reflect_bwd do, with the classes, the face tapes and the occlusion verdicts handed in as in
// tests/hostsim/image_views_env.cpp (no tracer takes part).  Test-only.
#include "../../drt_amd/csrc/drt_image_absorb.h"
#include "../../drt_amd/csrc/drt_image_env.h"
#include "../../drt_amd/csrc/drt_image_views.h"

using namespace drt;

namespace {

ImageCam cam_of(const double* cam21) {
    ImageCam c;
    memcpy(c.kinv, cam21, sizeof(double) * 9);
    memcpy(c.rinv, cam21 + 9, sizeof(double) * 12);
    return c;
}
ImageScreen screen_of(const double* q) { return ImageScreen{d3{q[0], q[1], q[2]}, d3{q[3], q[4], q[5]}, d3{q[6], q[7], q[8]}}; }

void fill_rows(const double* cams21, const double* screens9, int n_views, ImageViewRow* rows) {
    for (int k = 0; k < n_views; ++k) {
        rows[k].cam = cam_of(cams21 + 21 * k);
        rows[k].sc = screen_of(screens9 + 9 * k);
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
    if (R9) memcpy(e.rot, R9, sizeof(double) * 9);
    return e;
}

// what the forward leaves of one sample: exit ray, throughput and interior length from its tape (k_image_shade<.., ImageAbsorb>)
template <bool SNELL>
void sample_path(const PathCtx& c, int cls, const int32_t* tape, int64_t stride, int hits, d3& o, d3& d, double& T, double& L) {
    T = 1.0; L = 0.0;
    if (cls != kImageThrough) return;
    int n_refr = 0;
    for (int k = 0; k < hits; ++k)
        image_absorb_interact<SNELL, true>(c, tape[(int64_t)k * stride], true, o, d, n_refr, T, [&L](const Bounce& b) { L = image_absorb_length(b, L); });
}

// the transmitted colour (A T) B of one sample, image_pixel_walk's absorbing branch; true: lit (a function of T and L)
bool sample_colour(const ImageScreen& sc, const ImageTex& tx, bool has_screen, bool has_env, const ImageEnv& env, int cls, d3 o, d3 d, double T, double L,
                   const double* sigma, const double* fill_void, const double* fill_invalid, double* col) {
    if (has_env) return image_env_sample_colour<true>(sc, tx, has_screen, env, cls, o, d, T, fill_invalid, col, L, sigma) != kImageBgFill;
    return image_sample_colour<true>(sc, tx, cls, o, d, T, fill_void, fill_invalid, col, L, sigma);
}

struct Outs {
    double *grad_verts, *g_ior, *g_sigma;
    int64_t* count;
    float* images;
};

template <bool SNELL>
double views_loss(const ImageViewRow* rows, const ImageViewIds& ids, int W, int s, const ImageTex& tx, bool has_screen, bool has_env, const ImageEnv& env,
                  const PathCtx& c, const int32_t* cls, const int32_t* tape, const uint8_t* hits, const uint8_t* seen, bool reflection, const double* sigma,
                  const double* fill_void, const double* fill_invalid, const float* targets, const float* weights, const Outs& out) {
    const int s2 = s * s, H = ids.height;
    const int64_t n_pix = (int64_t)ids.k * H * W, n = n_pix * s2;
    double* gv = out.grad_verts;
    auto add = [gv](int32_t v, d3 a) { store_d3(gv, v, load_d3(gv, v) + a); };
    double loss = 0.0;
    for (int64_t pix = 0; pix < n_pix; ++pix) {
        int x, r, j0, slot, view, y;
        band_of(W, 0, s, (unsigned)(pix * s2), x, r, j0);
        image_views_row(ids, r, slot, view, y);
        const ImageViewRow& row = rows[view];
        d3 eo[kImageMaxSuper * kImageMaxSuper], ed[kImageMaxSuper * kImageMaxSuper];
        double eT[kImageMaxSuper * kImageMaxSuper], eL[kImageMaxSuper * kImageMaxSuper];
        double acc[kImageMaxChannels] = {0.0, 0.0, 0.0}, lc[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            d3 o, d, co, cd;
            image_sample_ray(row.cam, s, x, y, j, o, d);
            co = o; cd = d;
            double T, L;
            sample_path<SNELL>(c, cls[i], tape + i, n, (int)hits[i], o, d, T, L);
            eo[j] = o; ed[j] = d; eT[j] = T; eL[j] = L;
            double col[kImageMaxChannels];
            const bool lit = sample_colour(row.sc, tx, has_screen, has_env, env, cls[i], o, d, T, L, sigma, fill_void, fill_invalid, col);
            for (int ch = 0; ch < tx.c; ++ch)          // (before the reflection: that light never entered the object)
                if (lit && cls[i] == kImageThrough) lc[ch] = lc[ch] + L * col[ch];
            if (reflection && cls[i] == kImageThrough && seen[i]) {
                d3 ro, wr;
                double R1;
                if (image_reflect_first<SNELL>(c, tape[i], co, cd, ro, wr, R1)) image_env_add_reflection(row.sc, tx, has_screen, env, ro, wr, R1, col);
            }
            for (int ch = 0; ch < tx.c; ++ch) acc[ch] = j == 0 ? col[ch] : acc[ch] + col[ch];
        }
        const int64_t at = ((int64_t)view * H + y) * W + x;
        double mean[kImageMaxChannels], g_c[kImageMaxChannels];
        for (int ch = 0; ch < tx.c; ++ch) {
            mean[ch] = acc[ch] / (double)s2;
            if (out.images) out.images[at * tx.c + ch] = (float)mean[ch];
        }
        loss += image_loss_pixel(mean, tx.c, s2, targets + at * tx.c, weights ? (double)weights[at] : 1.0, g_c);
        for (int ch = 0; ch < tx.c; ++ch) out.g_sigma[ch] += image_absorb_sigma_term(g_c[ch], lc[ch]);
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            if (cls[i] != kImageThrough) continue;
            d3 o, d;
            image_sample_ray(row.cam, s, x, y, j, o, d);
            double gi, ge;
            const bool carried = has_env ? image_env_sample_backward<SNELL, true, true>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], row.sc, tx, has_screen, env,
                                                                                        g_c, add, gi, ge, eL[j], sigma)
                                         : image_sample_backward_absorb<SNELL, true>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], eL[j], sigma, row.sc, tx, g_c,
                                                                                     add, gi, ge);
            if (carried) {
                out.g_ior[0] += gi; out.g_ior[1] += ge;
                ++*out.count;
            }
            if (reflection && seen[i] && image_reflect_backward<SNELL>(c, tape[i], o, d, row.sc, tx, has_screen, env, g_c, add, gi, ge)) {
                out.g_ior[0] += gi; out.g_ior[1] += ge;
            }
        }
    }
    return loss;
}

// the clear loss of the same views (tests/hostsim/image_views_env.cpp's body, and the screen-only one): what sigma = 0 is held against
template <bool SNELL>
double views_loss_clear(const ImageViewRow* rows, const ImageViewIds& ids, int W, int s, const ImageTex& tx, bool has_screen, bool has_env, const ImageEnv& env,
                        const PathCtx& c, const int32_t* cls, const int32_t* tape, const uint8_t* hits, const uint8_t* seen, bool reflection,
                        const double* fill_void, const double* fill_invalid, const float* targets, const float* weights, const Outs& out) {
    const int s2 = s * s, H = ids.height;
    const int64_t n_pix = (int64_t)ids.k * H * W, n = n_pix * s2;
    double* gv = out.grad_verts;
    auto add = [gv](int32_t v, d3 a) { store_d3(gv, v, load_d3(gv, v) + a); };
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
            if (has_env) image_env_sample_colour(row.sc, tx, has_screen, env, cls[i], o, d, T, fill_invalid, col);
            else image_sample_colour(row.sc, tx, cls[i], o, d, T, fill_void, fill_invalid, col);
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
            const bool carried = has_env ? image_env_sample_backward<SNELL, true>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], row.sc, tx, has_screen, env, g_c,
                                                                                  add, gi, ge)
                                         : image_sample_backward<SNELL, true>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], row.sc, tx, g_c, add, gi, ge);
            if (carried) {
                out.g_ior[0] += gi; out.g_ior[1] += ge;
                ++*out.count;
            }
            if (reflection && seen[i] && image_reflect_backward<SNELL>(c, tape[i], o, d, row.sc, tx, has_screen, env, g_c, add, gi, ge)) {
                out.g_ior[0] += gi; out.g_ior[1] += ge;
            }
        }
    }
    return loss;
}

}  // namespace

extern "C" {

// L [n], A [n, C] and the transmitted colour col [n, C] of every sample i of the band [r0, r1) of k stacked views, formed THROUGH THE TABLE
// ROW of the sample's band row.  cls / hits [n] and tape [K, n] are the band's.  tex null: no screen; texel null: no environment.
void iva_band(const double* cams21, const double* screens9, int n_views, const int* view_ids, int k, int H, int W, int s, int r0, int r1, const float* tex, int th,
              int tw, int ch, const float* texel, int eh, int ew, const double* R9, const int32_t* faces, const double* verts, int n_tris, double ior_int,
              double ior_ext, int snell, const int32_t* cls, const int32_t* tape, const uint8_t* hits, const double* sigma, const double* fill_void,
              const double* fill_invalid, double* L_out, double* A_out, double* col_out) {
    ImageViewRow* rows = new ImageViewRow[n_views];
    fill_rows(cams21, screens9, n_views, rows);
    const ImageViewIds ids = ids_of(view_ids, k, H);
    const bool has_screen = tex != nullptr, has_env = texel != nullptr;
    const ImageTex tx{has_screen ? tex : nullptr, has_screen ? th : 2, has_screen ? tw : 2, ch};
    const ImageEnv e = env_of(texel, eh, ew, ch, R9);
    const PathCtx c{TraceCtx{nullptr, nullptr, n_tris, nullptr}, faces, verts, ior_int, ior_ext};
    const int64_t n = (int64_t)(r1 - r0) * W * s * s;
    for (int64_t i = 0; i < n; ++i) {
        int x, r, j, slot, view, y;
        band_of(W, r0, s, (unsigned)i, x, r, j);
        image_views_row(ids, r, slot, view, y);
        d3 o, d;
        double T, L;
        image_sample_ray(rows[view].cam, s, x, y, j, o, d);
        if (snell) sample_path<true>(c, cls[i], tape + i, n, (int)hits[i], o, d, T, L);
        else sample_path<false>(c, cls[i], tape + i, n, (int)hits[i], o, d, T, L);
        L_out[i] = L;
        for (int q = 0; q < ch; ++q) A_out[i * ch + q] = image_absorb_factor(sigma[q], L);
        sample_colour(rows[view].sc, tx, has_screen, has_env, e, cls[i], o, d, T, L, sigma, fill_void, fill_invalid, col_out + i * ch);
    }
    delete[] rows;
}

// The same of every sample of ONE view of H x W through its by-value camera and screen: the single-view call.
void iva_view(const double* cam21, const double* screen9, int H, int W, int s, const float* tex, int th, int tw, int ch, const float* texel, int eh, int ew,
              const double* R9, const int32_t* faces, const double* verts, int n_tris, double ior_int, double ior_ext, int snell, const int32_t* cls,
              const int32_t* tape, const uint8_t* hits, const double* sigma, const double* fill_void, const double* fill_invalid, double* L_out, double* A_out,
              double* col_out) {
    const ImageCam cam = cam_of(cam21);
    const ImageScreen sc = screen_of(screen9);
    const bool has_screen = tex != nullptr, has_env = texel != nullptr;
    const ImageTex tx{has_screen ? tex : nullptr, has_screen ? th : 2, has_screen ? tw : 2, ch};
    const ImageEnv e = env_of(texel, eh, ew, ch, R9);
    const PathCtx c{TraceCtx{nullptr, nullptr, n_tris, nullptr}, faces, verts, ior_int, ior_ext};
    const int64_t n = (int64_t)H * W * s * s;
    int64_t i = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int j = 0; j < s * s; ++j, ++i) {
                d3 o, d;
                double T, L;
                image_sample_ray(cam, s, x, y, j, o, d);
                if (snell) sample_path<true>(c, cls[i], tape + i, n, (int)hits[i], o, d, T, L);
                else sample_path<false>(c, cls[i], tape + i, n, (int)hits[i], o, d, T, L);
                L_out[i] = L;
                for (int q = 0; q < ch; ++q) A_out[i * ch + q] = image_absorb_factor(sigma[q], L);
                sample_colour(sc, tx, has_screen, has_env, e, cls[i], o, d, T, L, sigma, fill_void, fill_invalid, col_out + i * ch);
            }
}

// The loss of the listed views (returned) with its adjoint, over the whole tall image, Fresnel on: grad_verts [V, 3], g_ior [2], g_sigma [C]
// and *count are added into; images float32 [n_views, H, W, C] (may be null) receives the listed views' pixels.  cls int32 [n], tape int32
// [K, n], hits / seen uint8 [n] with n = k H W s^2, the listed views' one after the other; targets [n_views, H, W, C] and weights [n_views,
// H, W] (may be null) are indexed by view id.  tex null: no screen; texel null: no environment (then no reflection).  sigma null: the
// CLEAR loss of the same views (g_sigma is then left alone).
double iva_views_loss(const double* cams21, const double* screens9, int n_views, const int* view_ids, int k, int H, int W, int s, const float* tex, int th, int tw,
                      int ch, const float* texel, int eh, int ew, const double* R9, const int32_t* faces, const double* verts, int n_tris, double ior_int,
                      double ior_ext, int snell, int reflection, const int32_t* cls, const int32_t* tape, const uint8_t* hits, const uint8_t* seen,
                      const double* sigma, const double* fill_void, const double* fill_invalid, const float* targets, const float* weights, double* grad_verts,
                      double* g_ior, double* g_sigma, int64_t* count, float* images) {
    ImageViewRow* rows = new ImageViewRow[n_views];
    fill_rows(cams21, screens9, n_views, rows);
    const ImageViewIds ids = ids_of(view_ids, k, H);
    const bool has_screen = tex != nullptr, has_env = texel != nullptr;
    const ImageTex tx{has_screen ? tex : nullptr, has_screen ? th : 2, has_screen ? tw : 2, ch};
    const ImageEnv e = env_of(texel, eh, ew, ch, R9);
    const PathCtx c{TraceCtx{nullptr, nullptr, n_tris, nullptr}, faces, verts, ior_int, ior_ext};
    const Outs out{grad_verts, g_ior, g_sigma, count, images};
    const bool refl = reflection != 0 && has_env;
    double loss;
    if (sigma)
        loss = snell ? views_loss<true>(rows, ids, W, s, tx, has_screen, has_env, e, c, cls, tape, hits, seen, refl, sigma, fill_void, fill_invalid, targets, weights, out)
                     : views_loss<false>(rows, ids, W, s, tx, has_screen, has_env, e, c, cls, tape, hits, seen, refl, sigma, fill_void, fill_invalid, targets, weights, out);
    else
        loss = snell ? views_loss_clear<true>(rows, ids, W, s, tx, has_screen, has_env, e, c, cls, tape, hits, seen, refl, fill_void, fill_invalid, targets, weights, out)
                     : views_loss_clear<false>(rows, ids, W, s, tx, has_screen, has_env, e, c, cls, tape, hits, seen, refl, fill_void, fill_invalid, targets, weights, out);
    delete[] rows;
    return loss;
}

// The adjoint of sum over the selected through samples of sum_ch g_c[ch] c[ch], c the transmitted colour (A T) B of an ENVIRONMENT-going
// sample of one view without a screen: image_env_sample_backward<.., LENGTH> per sample, which hands g_L to bounce_t_backward at every
// interaction with sg < 0.  grad_verts [V, 3] and g_ior [2] are added into; returns the sum itself.
double iva_env_adjoint(const double* cam21, int H, int W, int s, int ch, const float* texel, int eh, int ew, const double* R9, const int32_t* faces,
                       const double* verts, int n_tris, double ior_int, double ior_ext, int snell, const int32_t* cls, const int32_t* tape, const uint8_t* hits,
                       const uint8_t* sel, const double* sigma, const double* g_c, double* grad_verts, double* g_ior) {
    const ImageCam cam = cam_of(cam21);
    const ImageScreen sc{};
    const ImageTex tx{nullptr, 2, 2, ch};
    const ImageEnv e = env_of(texel, eh, ew, ch, R9);
    const PathCtx c{TraceCtx{nullptr, nullptr, n_tris, nullptr}, faces, verts, ior_int, ior_ext};
    const int64_t n = (int64_t)H * W * s * s;
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    const double fill[kImageMaxChannels] = {0.0, 0.0, 0.0};
    double total = 0.0;
    int64_t i = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int j = 0; j < s * s; ++j, ++i) {
                if (!sel[i] || cls[i] != kImageThrough) continue;
                d3 o, d, eo, ed;
                double T, L, col[kImageMaxChannels], gi, ge;
                image_sample_ray(cam, s, x, y, j, o, d);
                eo = o; ed = d;
                if (snell) sample_path<true>(c, cls[i], tape + i, n, (int)hits[i], eo, ed, T, L);
                else sample_path<false>(c, cls[i], tape + i, n, (int)hits[i], eo, ed, T, L);
                image_env_sample_colour<true>(sc, tx, false, e, cls[i], eo, ed, T, fill, col, L, sigma);
                for (int q = 0; q < ch; ++q) total += g_c[q] * col[q];
                if (snell) image_env_sample_backward<true, true, true>(c, o, d, tape + i, n, (int)hits[i], eo, ed, T, sc, tx, false, e, g_c, add, gi, ge, L, sigma);
                else image_env_sample_backward<false, true, true>(c, o, d, tape + i, n, (int)hits[i], eo, ed, T, sc, tx, false, e, g_c, add, gi, ge, L, sigma);
                g_ior[0] += gi; g_ior[1] += ge;
            }
    return total;
}

}  // extern "C"
