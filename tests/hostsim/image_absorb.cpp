// tests/hostsim/image_absorb.cpp -- drt_amd/csrc/drt_image_absorb.h compiled for the host (g++ -ffp-contract=off): the absorbing refracted
// image, its photometric loss and the adjoint, run over a whole view in plain loops.  The classes and the face tape are handed in (the
// restatement's, from the oracle's tracer): a through sample's exit ray, throughput and interior length are recomputed from its tape with
// the function k_image_absorb_shade runs (image_absorb_interact), its adjoint is image_sample_backward_absorb -- what
// k_image_absorb_loss_bwd runs --, and the sigma partials are summed per pixel as k_image_absorb_loss_resolve sums them.  Test-only.
#include "../../drt_amd/csrc/drt_image_absorb.h"

using namespace drt;

namespace {
ImageCam cam_of(const double* cam21) {
    ImageCam c;
    memcpy(c.kinv, cam21, sizeof(double) * 9);
    memcpy(c.rinv, cam21 + 9, sizeof(double) * 12);
    return c;
}
ImageScreen screen_of(const double* s9) { return ImageScreen{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}}; }

template <bool SNELL, bool FRESNEL>
double view(const ImageCam& cam, int H, int W, int s, const ImageScreen& sc, const ImageTex& tx, const PathCtx& c, const int32_t* cls, const int32_t* tape,
            const uint8_t* hits, const double* fill_void, const double* fill_invalid, const double* sigma, const float* target, const float* weight,
            double* grad_verts, double* g_ior, double* g_sigma, int64_t* count, float* image, float* length, double* L_out, double* A_out) {
    const int s2 = s * s;
    const int64_t n = (int64_t)H * W * s2;
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    double loss = 0.0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t pix = (int64_t)y * W + x;
            d3 eo[kImageMaxSuper * kImageMaxSuper], ed[kImageMaxSuper * kImageMaxSuper];
            double eT[kImageMaxSuper * kImageMaxSuper], eL[kImageMaxSuper * kImageMaxSuper];
            double acc[kImageMaxChannels] = {0.0, 0.0, 0.0}, lc[kImageMaxChannels] = {0.0, 0.0, 0.0};
            double l_sum = 0.0;
            int n_through = 0;
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                d3 o, d;
                image_sample_ray(cam, s, x, y, j, o, d);
                double T = 1.0, L = 0.0;
                if (cls[i] == kImageThrough) {
                    int n_refr = 0;
                    for (int k = 0; k < (int)hits[i]; ++k)
                        image_absorb_interact<SNELL, FRESNEL>(c, tape[(int64_t)k * n + i], true, o, d, n_refr, T, [&L](const Bounce& b) { L = image_absorb_length(b, L); });
                    l_sum = n_through == 0 ? L : l_sum + L;
                    ++n_through;
                }
                eo[j] = o; ed[j] = d; eT[j] = T; eL[j] = L;
                if (L_out) L_out[i] = L;
                if (A_out) for (int ch = 0; ch < tx.c; ++ch) A_out[i * tx.c + ch] = image_absorb_factor(sigma[ch], L);
                double col[kImageMaxChannels];
                const bool lit = image_absorb_sample_colour(sc, tx, cls[i], o, d, T, L, sigma, fill_void, fill_invalid, col);
                for (int ch = 0; ch < tx.c; ++ch) {
                    acc[ch] = j == 0 ? col[ch] : acc[ch] + col[ch];
                    if (lit && cls[i] == kImageThrough) lc[ch] = lc[ch] + L * col[ch];
                }
            }
            double mean[kImageMaxChannels], g_c[kImageMaxChannels];
            for (int ch = 0; ch < tx.c; ++ch) {
                mean[ch] = acc[ch] / (double)s2;
                if (image) image[pix * tx.c + ch] = (float)mean[ch];
            }
            if (length) length[pix] = n_through ? (float)(l_sum / (double)n_through) : 0.f;
            loss += image_loss_pixel(mean, tx.c, s2, target + pix * tx.c, weight ? (double)weight[pix] : 1.0, g_c);
            for (int ch = 0; ch < tx.c; ++ch) g_sigma[ch] += image_absorb_sigma_term(g_c[ch], lc[ch]);
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                if (cls[i] != kImageThrough) continue;
                d3 o, d;
                image_sample_ray(cam, s, x, y, j, o, d);
                double gi, ge;
                if (image_sample_backward_absorb<SNELL, FRESNEL>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], eL[j], sigma, sc, tx, g_c, add, gi, ge)) {
                    g_ior[0] += gi; g_ior[1] += ge;
                    ++*count;
                }
            }
        }
    return loss;
}
}  // namespace

extern "C" {

// Per row: law_forward<snell> on (o, d, triangle), its t and sg written out, then bounce_t_backward with the seed g_t [n] into zeros:
// gv [n, 3, 3] (v0, v1, v2), g_o, g_d [n, 3].  t_plain / sg_plain: what bounce_forward itself leaves, for the comparison of the two laws.
void ia_t_backward(const double* o, const double* d, const double* tri, double ior_ext, double ior_int, int snell, const double* g_t, int64_t n, double* t,
                   double* sg, double* t_plain, double* sg_plain, double* gv, double* g_o, double* g_d) {
    for (int64_t i = 0; i < n; ++i) {
        const d3 oo = load_d3(o, i), dd = load_d3(d, i), v0 = load_d3(tri, 3 * i), v1 = load_d3(tri, 3 * i + 1), v2 = load_d3(tri, 3 * i + 2);
        Bounce b, p;
        if (snell) law_forward<true>(oo, dd, v0, v1, v2, ior_ext, ior_int, b);
        else law_forward<false>(oo, dd, v0, v1, v2, ior_ext, ior_int, b);
        bounce_forward(oo, dd, v0, v1, v2, ior_ext, ior_int, p);
        t[i] = b.t; sg[i] = b.sg; t_plain[i] = p.t; sg_plain[i] = p.sg;
        d3 a{0.0, 0.0, 0.0}, bb = a, cc = a, go = a, gd = a;
        bounce_t_backward(b, g_t[i], a, bb, cc, go, gd);
        store_d3(gv, 3 * i, a); store_d3(gv, 3 * i + 1, bb); store_d3(gv, 3 * i + 2, cc);
        store_d3(g_o, i, go); store_d3(g_d, i, gd);
    }
}

// The loss of one view (returned) with its adjoint: grad_verts [V, 3], g_ior [2] (ior_int, ior_ext), g_sigma [C] and *count (through
// samples on the screen) are added into; image float32 [H, W, C], length float32 [H, W], L [n] and A [n, C] (each may be null) are
// written.  cls int32 [n], tape int32 [K, n], hits uint8 [n], sigma float64 [C].
double ia_view(const double* cam21, int H, int W, int s, const double* s9, const float* texel, int th, int tw, int ch, const int32_t* faces,
               const double* verts, double ior_int, double ior_ext, int snell, int fresnel, const int32_t* cls, const int32_t* tape, const uint8_t* hits,
               const double* fill_void, const double* fill_invalid, const double* sigma, const float* target, const float* weight, double* grad_verts,
               double* g_ior, double* g_sigma, int64_t* count, float* image, float* length, double* L_out, double* A_out) {
    const ImageCam cam = cam_of(cam21);
    const ImageScreen sc = screen_of(s9);
    const ImageTex tx{texel, th, tw, ch};
    const PathCtx c{TraceCtx{nullptr, nullptr, 0, nullptr}, faces, verts, ior_int, ior_ext};
#define IA_VIEW(SN, FR) view<SN, FR>(cam, H, W, s, sc, tx, c, cls, tape, hits, fill_void, fill_invalid, sigma, target, weight, grad_verts, g_ior, g_sigma, count, \
                                     image, length, L_out, A_out)
    if (snell) return fresnel ? IA_VIEW(true, true) : IA_VIEW(true, false);
    return fresnel ? IA_VIEW(false, true) : IA_VIEW(false, false);
#undef IA_VIEW
}

}  // extern "C"
