// tests/hostsim/image_loss.cpp -- drt_amd/csrc/drt_image_loss.h compiled for the host (g++ -ffp-contract=off): the photometric loss of the
// refracted image and its adjoint, run over a whole view in plain loops.  The classes and the face tape are handed in (the restatement's,
// from the oracle's tracer), so that no tracer takes part: a through sample's exit ray and throughput are recomputed from its tape with the
// functions k_image_shade runs (image_interact), its adjoint is image_sample_backward -- what k_image_loss_bwd runs.  Test-only.
#include "../../drt_amd/csrc/drt_image_loss.h"

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
            const uint8_t* hits, const double* fill_void, const double* fill_invalid, const float* target, const float* weight, double* grad_verts,
            double* g_ior, int64_t* count, float* image, double* T_out) {
    const int s2 = s * s;
    const int64_t n = (int64_t)H * W * s2;
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    double loss = 0.0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t pix = (int64_t)y * W + x;
            d3 eo[kImageMaxSuper * kImageMaxSuper], ed[kImageMaxSuper * kImageMaxSuper];
            double eT[kImageMaxSuper * kImageMaxSuper];
            double acc[kImageMaxChannels] = {0.0, 0.0, 0.0};
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                d3 o, d;
                image_sample_ray(cam, s, x, y, j, o, d);
                double T = 1.0;
                if (cls[i] == kImageThrough) {
                    int n_refr = 0;
                    for (int k = 0; k < (int)hits[i]; ++k) image_interact<SNELL, FRESNEL>(c, tape[(int64_t)k * n + i], true, o, d, n_refr, T);
                }
                eo[j] = o; ed[j] = d; eT[j] = T;
                if (T_out) T_out[i] = T;
                double col[kImageMaxChannels];
                image_sample_colour(sc, tx, cls[i], o, d, T, fill_void, fill_invalid, col);
                for (int ch = 0; ch < tx.c; ++ch) acc[ch] = j == 0 ? col[ch] : acc[ch] + col[ch];
            }
            double mean[kImageMaxChannels], g_c[kImageMaxChannels];
            for (int ch = 0; ch < tx.c; ++ch) {
                mean[ch] = acc[ch] / (double)s2;
                if (image) image[pix * tx.c + ch] = (float)mean[ch];
            }
            loss += image_loss_pixel(mean, tx.c, s2, target + pix * tx.c, weight ? (double)weight[pix] : 1.0, g_c);
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                if (cls[i] != kImageThrough) continue;
                d3 o, d;
                image_sample_ray(cam, s, x, y, j, o, d);
                double gi, ge;
                if (image_sample_backward<SNELL, FRESNEL>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], sc, tx, g_c, add, gi, ge)) {
                    g_ior[0] += gi; g_ior[1] += ge;
                    ++*count;
                }
            }
        }
    return loss;
}
}  // namespace

extern "C" {

// g_ci, g_eta_i, g_eta_t [n] of fresnel_R_backward with the seed g_R [n] (into zeros)
void il_fresnel_backward(const double* ci, const double* eta_i, const double* eta_t, const double* g_R, int64_t n, double* g_ci, double* g_ei, double* g_et) {
    for (int64_t i = 0; i < n; ++i) {
        g_ci[i] = 0.0; g_ei[i] = 0.0; g_et[i] = 0.0;
        fresnel_R_backward(ci[i], eta_i[i], eta_t[i], g_R[i], g_ci[i], g_ei[i], g_et[i]);
    }
}

// The loss of one view (returned) with its adjoint: grad_verts [V, 3], g_ior [2] (ior_int, ior_ext) and *count (through samples on the
// screen) are added into, image float32 [H, W, C] and T [n] (both may be null) are written.  cls int32 [n], tape int32 [K, n], hits uint8 [n].
double il_view(const double* cam21, int H, int W, int s, const double* s9, const float* texel, int th, int tw, int ch, const int32_t* faces,
               const double* verts, double ior_int, double ior_ext, int snell, int fresnel, const int32_t* cls, const int32_t* tape, const uint8_t* hits,
               const double* fill_void, const double* fill_invalid, const float* target, const float* weight, double* grad_verts, double* g_ior,
               int64_t* count, float* image, double* T_out) {
    const ImageCam cam = cam_of(cam21);
    const ImageScreen sc = screen_of(s9);
    const ImageTex tx{texel, th, tw, ch};
    const PathCtx c{TraceCtx{nullptr, nullptr, 0, nullptr}, faces, verts, ior_int, ior_ext};
#define IL_VIEW(SN, FR) view<SN, FR>(cam, H, W, s, sc, tx, c, cls, tape, hits, fill_void, fill_invalid, target, weight, grad_verts, g_ior, count, image, T_out)
    if (snell) return fresnel ? IL_VIEW(true, true) : IL_VIEW(true, false);
    return fresnel ? IL_VIEW(false, true) : IL_VIEW(false, false);
#undef IL_VIEW
}

}  // extern "C"
