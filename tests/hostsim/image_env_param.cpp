// tests/hostsim/image_env_param.cpp -- drt_amd/csrc/drt_image_env_param.h compiled for the host (g++ -ffp-contract=off): the loss of one view in
// front of an environment with the gradients of the environment's texels and rotation, run over arrays in plain loops.  Test-only.
#include "../../drt_amd/csrc/drt_image_env_param.h"

using namespace drt;

namespace {
// What k_image_loss_resolve<.., ImageScreenEnv[Reflect]> and k_image_env_param_bwd run, on classes, exit rays, throughputs and occlusion
// verdicts that are handed in: per pixel the colours (image_env_sample_colour, + image_env_add_reflection where the reflection was seen),
// the mean, the loss term and the seeds g_c; then per sample image_env_ray_backward along the exit (direct: camera) ray with w = T and,
// where the reflection was seen, along the reflected ray recomputed from the first face with w = R1.  g_env / g_R null: the loss alone.
template <bool SNELL>
double param_view(const ImageCam& cam, int H, int W, int s, const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& env, const PathCtx& c,
                  const int32_t* cls, const double* exit_o, const double* exit_d, const double* T, const int32_t* first_face, const uint8_t* seen, bool reflection,
                  const double* fill_invalid, const float* target, const float* weight, double* g_env, double* g_R, double* stats) {
    const int s2 = s * s;
    double loss = 0.0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t pix = (int64_t)y * W + x;
            double acc[kImageMaxChannels] = {0.0, 0.0, 0.0};
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                double col[kImageMaxChannels];
                image_env_sample_colour(sc, tx, has_screen, env, cls[i], load_d3(exit_o, i), load_d3(exit_d, i), T[i], fill_invalid, col);
                if (reflection && cls[i] == kImageThrough && seen[i]) {
                    d3 co, cd, ro, wr;
                    double R1;
                    image_sample_ray(cam, s, x, y, j, co, cd);
                    if (image_reflect_first<SNELL>(c, first_face[i], co, cd, ro, wr, R1)) image_env_add_reflection(sc, tx, has_screen, env, ro, wr, R1, col);
                }
                for (int ch = 0; ch < tx.c; ++ch) acc[ch] = j == 0 ? col[ch] : acc[ch] + col[ch];
            }
            double mean[kImageMaxChannels], g_c[kImageMaxChannels];
            for (int ch = 0; ch < tx.c; ++ch) mean[ch] = acc[ch] / (double)s2;
            loss += image_loss_pixel(mean, tx.c, s2, target + pix * tx.c, weight ? (double)weight[pix] : 1.0, g_c);
            if (!g_env && !g_R) continue;
            auto add_texel = [&](int32_t texel, const double* gt) {
                if (g_env) for (int ch = 0; ch < tx.c; ++ch) g_env[(int64_t)texel * tx.c + ch] += gt[ch];
            };
            auto read = [&](d3 o, d3 d, double w) {
                double r[9];
                if (!image_env_ray_backward(sc, tx, has_screen, env, o, d, w, g_c, add_texel, r)) return;
                if (g_R) for (int k = 0; k < 9; ++k) g_R[k] += r[k];
                if (stats) {
                    for (int ch = 0; ch < tx.c; ++ch) { stats[ch] += w * g_c[ch]; stats[3] += fabs(w * g_c[ch]); }
                    stats[4] += 1.0;
                }
            };
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                if (cls[i] == kImageInvalid) continue;
                read(load_d3(exit_o, i), load_d3(exit_d, i), T[i]);
                if (reflection && cls[i] == kImageThrough && seen[i]) {
                    d3 co, cd, ro, wr;
                    double R1;
                    image_sample_ray(cam, s, x, y, j, co, cd);
                    if (image_reflect_first<SNELL>(c, first_face[i], co, cd, ro, wr, R1)) read(ro, wr, R1);
                }
            }
        }
    return loss;
}
}  // namespace

extern "C" {

// The loss of one view (returned).  g_env float64 [eh, ew, ch], g_R [9] and stats [5] (sum over the reads of w g_c[ch] per channel, of
// |w g_c[ch]|, and the number of reads) are added into; each may be null.  s9 / tex null: no screen.  cls int32 [n], exit_o / exit_d
// float64 [n, 3], T float64 [n] (1 for a direct sample, whose exit ray is its camera ray), first_face int32 [n], seen uint8 [n].
double env_param_view(const double* cam21, int H, int W, int s, const double* s9, const float* tex, int th, int tw, int ch, const float* texel, int eh, int ew,
                      const double* R9, const int32_t* faces, const double* verts, int n_tris, double ior_int, double ior_ext, int snell, int reflection,
                      const int32_t* cls, const double* exit_o, const double* exit_d, const double* T, const int32_t* first_face, const uint8_t* seen,
                      const double* fill_invalid, const float* target, const float* weight, double* g_env, double* g_R, double* stats) {
    ImageCam cam;
    memcpy(cam.kinv, cam21, sizeof(double) * 9);
    memcpy(cam.rinv, cam21 + 9, sizeof(double) * 12);
    const bool has_screen = s9 != nullptr;
    ImageScreen sc{d3{0, 0, 0}, d3{1, 0, 0}, d3{0, 1, 0}};
    if (has_screen) sc = ImageScreen{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}};
    const ImageTex tx{has_screen ? tex : nullptr, has_screen ? th : 2, has_screen ? tw : 2, ch};
    ImageEnv e{texel, eh, ew, ch, {}};
    memcpy(e.rot, R9, sizeof(double) * 9);
    const PathCtx c{TraceCtx{nullptr, nullptr, n_tris, nullptr}, faces, verts, ior_int, ior_ext};
    if (snell) return param_view<true>(cam, H, W, s, sc, tx, has_screen, e, c, cls, exit_o, exit_d, T, first_face, seen, reflection != 0, fill_invalid, target, weight, g_env, g_R, stats);
    return param_view<false>(cam, H, W, s, sc, tx, has_screen, e, c, cls, exit_o, exit_d, T, first_face, seen, reflection != 0, fill_invalid, target, weight, g_env, g_R, stats);
}

}  // extern "C"
