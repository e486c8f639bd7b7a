// tests/hostsim/image_screen.cpp -- drt_amd/csrc/drt_image_screen.h compiled for the host (g++ -ffp-contract=off): the photometric loss of
// the refracted image and its adjoint w.r.t. the screen's pose and the texture, run over a whole view in plain loops.  Every sample's
// class, ray (the camera ray of a direct sample, the exit ray of a through one) and throughput are handed in -- the restatement's
// constants -- so that no tracer and no path takes part: the forward is image_sample_colour and image_loss_pixel, the adjoint is
// image_sample_backward_screen -- what k_image_screen_bwd runs.  Test-only.
#include "../../drt_amd/csrc/drt_image_screen.h"

using namespace drt;

extern "C" {

// The loss of one view (returned) with its adjoint: g_screen [9] (p0, eu, ev), g_texture [th, tw, ch] and *count (samples that carried a
// gradient) are added into; g_screen / g_texture may be null.  cls int32 [n], ori / dir float64 [n, 3], T float64 [n], n = H W s^2.
double is_view(int H, int W, int s, const double* s9, const float* texel, int th, int tw, int ch, const int32_t* cls, const double* ori,
               const double* dir, const double* T, const double* fill_void, const double* fill_invalid, const float* target, const float* weight,
               double* g_screen, double* g_texture, int64_t* count) {
    const ImageScreen sc{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}};
    const ImageTex tx{texel, th, tw, ch};
    const int s2 = s * s;
    auto tex_add = [g_texture, ch](int32_t cell, const double* g) {
        if (g_texture) for (int k = 0; k < ch; ++k) g_texture[(int64_t)cell * ch + k] += g[k];
    };
    const d3 z{0.0, 0.0, 0.0};
    d3 g_p0 = z, g_eu = z, g_ev = z;
    double loss = 0.0;
    for (int64_t pix = 0; pix < (int64_t)H * W; ++pix) {
        double acc[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            double col[kImageMaxChannels];
            image_sample_colour(sc, tx, cls[i], load_d3(ori, i), load_d3(dir, i), T[i], fill_void, fill_invalid, col);
            for (int k = 0; k < ch; ++k) acc[k] = j == 0 ? col[k] : acc[k] + col[k];
        }
        double mean[kImageMaxChannels], g_c[kImageMaxChannels];
        for (int k = 0; k < ch; ++k) mean[k] = acc[k] / (double)s2;
        loss += image_loss_pixel(mean, ch, s2, target + pix * ch, weight ? (double)weight[pix] : 1.0, g_c);
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            if (cls[i] == kImageInvalid) continue;
            if (image_sample_backward_screen(sc, tx, load_d3(ori, i), load_d3(dir, i), T[i], g_c, tex_add, g_p0, g_eu, g_ev)) ++*count;
        }
    }
    if (g_screen) {
        const double g[9] = {g_p0.x, g_p0.y, g_p0.z, g_eu.x, g_eu.y, g_eu.z, g_ev.x, g_ev.y, g_ev.z};
        for (int k = 0; k < 9; ++k) g_screen[k] += g[k];
    }
    return loss;
}

}  // extern "C"
