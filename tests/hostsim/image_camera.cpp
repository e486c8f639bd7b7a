// tests/hostsim/image_camera.cpp -- drt_amd/csrc/drt_image_camera.h compiled for the host (g++ -ffp-contract=off): the photometric loss of
// the refracted image and its adjoint w.r.t. the camera's 21 numbers, run over a whole view in plain loops.  The classes and the face tape
// are handed in (the restatement's, from the oracle's tracer), so that no tracer takes part: the forward is tests/hostsim/image_loss.cpp's
// -- a through sample's exit ray and throughput recomputed from its tape with image_interact -- and the adjoint is what the two kernels of
// drt_image_camera.hip run: image_sample_backward with its seed outputs (k_image_loss_bwd with CAMERA) or image_direct_seeds, then
// image_sample_ray_backward (k_image_camera_bwd).  Test-only.
#include "../../drt_amd/csrc/drt_image_camera.h"

using namespace drt;

namespace {
template <bool SNELL, bool FRESNEL>
double view(const ImageCam& cam, int H, int W, int s, const ImageScreen& sc, const ImageTex& tx, const PathCtx& c, const int32_t* cls, const int32_t* tape,
            const uint8_t* hits, const double* fill_void, const double* fill_invalid, const float* target, const float* weight, double* g_cam,
            int64_t* count, int64_t* through) {
    const int s2 = s * s;
    const int64_t n = (int64_t)H * W * s2;
    auto add = [](int32_t, d3) {};
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
                double col[kImageMaxChannels];
                image_sample_colour(sc, tx, cls[i], o, d, T, fill_void, fill_invalid, col);
                for (int ch = 0; ch < tx.c; ++ch) acc[ch] = j == 0 ? col[ch] : acc[ch] + col[ch];
            }
            double mean[kImageMaxChannels], g_c[kImageMaxChannels];
            for (int ch = 0; ch < tx.c; ++ch) mean[ch] = acc[ch] / (double)s2;
            loss += image_loss_pixel(mean, tx.c, s2, target + pix * tx.c, weight ? (double)weight[pix] : 1.0, g_c);
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                if (cls[i] == kImageInvalid) continue;
                d3 o, d, g_o, g_d;
                image_sample_ray(cam, s, x, y, j, o, d);
                if (cls[i] == kImageThrough) {
                    double gi, ge;
                    if (!image_sample_backward<SNELL, FRESNEL>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], sc, tx, g_c, add, gi, ge, &g_o, &g_d))
                        continue;
                    if (!image_through_on_screen(sc, tx, eo[j], ed[j])) return -1.0;          // (the second kernel's verdict is the first's)
                    ++*through;
                } else if (!image_direct_seeds(sc, tx, o, d, g_c, g_o, g_d)) {
                    continue;
                }
                image_sample_ray_backward(cam, s, x, y, j, g_o, g_d, g_cam, g_cam + 9);
                ++*count;
            }
        }
    return loss;
}
}  // namespace

extern "C" {

// The loss of one view (returned) with its adjoint: g_cam [21] (kinv, then rinv), *count (samples that carried a gradient) and *through
// (the through samples among them) are added into.  cls int32 [n], tape int32 [K, n], hits uint8 [n], n = H W s^2.
double ic_view(const double* cam21, int H, int W, int s, const double* s9, const float* texel, int th, int tw, int ch, const int32_t* faces,
               const double* verts, double ior_int, double ior_ext, int snell, int fresnel, const int32_t* cls, const int32_t* tape, const uint8_t* hits,
               const double* fill_void, const double* fill_invalid, const float* target, const float* weight, double* g_cam, int64_t* count,
               int64_t* through) {
    ImageCam cam;
    memcpy(cam.kinv, cam21, sizeof(double) * 9);
    memcpy(cam.rinv, cam21 + 9, sizeof(double) * 12);
    const ImageScreen sc{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}};
    const ImageTex tx{texel, th, tw, ch};
    const PathCtx c{TraceCtx{nullptr, nullptr, 0, nullptr}, faces, verts, ior_int, ior_ext};
#define IC_VIEW(SN, FR) view<SN, FR>(cam, H, W, s, sc, tx, c, cls, tape, hits, fill_void, fill_invalid, target, weight, g_cam, count, through)
    if (snell) return fresnel ? IC_VIEW(true, true) : IC_VIEW(true, false);
    return fresnel ? IC_VIEW(false, true) : IC_VIEW(false, false);
#undef IC_VIEW
}

}  // extern "C"
