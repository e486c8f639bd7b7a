// drt_image_env_param.hip -- the environment's texel and rotation gradients of the photometric loss of the refracted image
// (drt_image_env_param.h holds the law): one more pass of drt_render_image_loss_env_param (drt_image_env.hip) over the
// pixels of the band, behind k_image_loss_resolve<., ., ., ImageScreenEnv[Reflect]>, which has written the pixel seeds g_c.  A unit of its
// own for the reason drt_image_screen.hip gives: a kernel's register allocation depends on the other kernels of its unit (DESIGN.md
// section 4), and the kernels of drt_image_env.hip are to stay what they are.
//
//   k_image_env_param_bwd  all pixels : image_pixel_walk's walk over the s x s samples of its pixel -- a direct sample's camera ray formed again,
//                                       a through sample's exit ray and throughput from the parked rows -- and image_env_ray_backward per
//                                       sample that the screen does not catch; REFLECT: a through sample with the bit kImageReflectSeen
//                                       forms its camera ray again, recomputes (ro, wr, R1) from the tape's first face (image_reflect_first,
//                                       as the resolve kernel does) and runs image_env_ray_backward on the reflected ray with w = R1.  The
//                                       nine rotation partials through nine LossAcc summed over the block (block_flush: one atomic per block
//                                       and partial), the four texel contributions of a read through PathSink in kImageEnvParamBatch-sized
//                                       fills (sink_pass); TEXELS = false: no table in LDS
// The texel gradient in the sink is packed as drt_image_screen.hip packs the texture's: with three channels the texel number is the id and
// the channels are the d3; with one channel the id is texel / 3 and one component is non-zero, which is why the accumulator is padded to a
// multiple of three values.  The refraction law of the one recomputed Bounce is a run-time branch, as in image_pixel_walk (the first
// Bounce's t, n, ci and flags are bounce_forward's under either law): profiles/image_env_param_resources.txt has the figures of both
// spellings.  No tree is read and no path recomputed.  Everything runs on the caller's stream, nothing is read back.
#include "drt_image_wave.h"
#include "drt_image_env_param.h"

// Pixels per table fill, as kImageScreenBatch: the 256 neighbouring pixels of a fill look at neighbouring texels of the environment (a
// panorama is coarser in texels per pixel than a screen), and a table that does fill up sends the rest straight to memory.
constexpr int kImageEnvParamBatch = kPathsBwdBatch;
constexpr int kImageEnvParamBpc = DRT_BWD_BPC;       // 56 KB of table per block

// grad_env (TEXELS) and grad_rot (nine accumulators, row-major) may each be null.
template <bool DET, bool TEXELS, bool REFLECT>
__global__ void __launch_bounds__(256) k_image_env_param_bwd(ImageCam cam, ImageBand band, int64_t n_pix, ImageScreen sc, ImageTex tx, bool fresnel, ImageScreenEnv bg,
                                                             PathCtx pc, bool snell, const int32_t* __restrict__ first_face,
                                                             const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                             const double* __restrict__ thr, const uint8_t* __restrict__ state,
                                                             const uint8_t* __restrict__ hits, const double* __restrict__ g_c, double* grad_env,
                                                             double* grad_rot) {
    LossAcc<DET> acc[9];
    const int s2 = band.s * band.s;
    sink_pass<DET, kImageEnvParamBatch, TEXELS>(n_pix, grad_env, [&](int64_t pix, auto add) {
        const int y = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
        double g[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int ch = 0; ch < tx.c; ++ch) g[ch] = g_c[pix * tx.c + ch];
        const bool rgb = tx.c == 3;
        auto add_texel = [&](int32_t texel, const double* gt) {
            if (rgb) { add(texel, d3{gt[0], gt[1], gt[2]}); return; }
            const int32_t id = texel / 3;
            const int k = texel - 3 * id;
            add(id, d3{k == 0 ? gt[0] : 0.0, k == 1 ? gt[0] : 0.0, k == 2 ? gt[0] : 0.0});
        };
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            const int cls = image_class(hits[i] != 0, (state[i] & kPathDone) != 0);
            if (cls == kImageInvalid) continue;
            d3 o, d;
            double T = 1.0;
            if (cls == kImageDirect) {
                image_sample_ray(cam, band.s, x, y, j, o, d);
            } else {
                o = load_d3(park_ori, i); d = load_d3(park_dir, i);
                if (fresnel) T = thr[i];
            }
            double g_R[9];
            if (image_env_ray_backward(sc, tx, bg.screen, bg.env, o, d, T, g, add_texel, g_R)) {
#pragma unroll
                for (int k = 0; k < 9; ++k) acc[k].add(g_R[k]);
            }
            if constexpr (REFLECT) {
                if (cls == kImageThrough && (state[i] & kImageReflectSeen)) {
                    d3 co, cd, ro, wr;
                    double R1;
                    image_sample_ray(cam, band.s, x, y, j, co, cd);
                    const bool seen = snell ? image_reflect_first<true>(pc, first_face[i], co, cd, ro, wr, R1)
                                            : image_reflect_first<false>(pc, first_face[i], co, cd, ro, wr, R1);
                    if (seen && image_env_ray_backward(sc, tx, bg.screen, bg.env, ro, wr, R1, g, add_texel, g_R)) {
#pragma unroll
                        for (int k = 0; k < 9; ++k) acc[k].add(g_R[k]);
                    }
                }
            }
        }
    });
    if (grad_rot) block_flush<DET, 9>(acc, grad_rot);
}

template <int... I>
static auto env_param_kernel(int sel, std::integer_sequence<int, I...>) {
    using Kernel = decltype(&k_image_env_param_bwd<false, false, false>);
    static const Kernel kernels[] = {k_image_env_param_bwd<(I & 4) != 0, (I & 2) != 0, (I & 1) != 0>...};
    return kernels[sel];
}

int launch_image_env_param_bwd(const drt_scene* s, const PathCtx& pc, const ImageCall& c, const ImageScreenEnv& bg, bool reflection, const double* g_c,
                               double* d_grad_env, double* d_grad_env_rot, hipStream_t st) {
    const PathsWs& w = *static_cast<const PathsWs*>(s->paths_ws);
    const double* const park_ori = w.park;
    const double* const park_dir = w.park + 3 * w.fused_cap;
    const bool reflect = reflection && s->n_faces > 0;          // (a scene without triangles has direct samples only, and no tape)
    const int grid = grid_for(c.n_pix, d_grad_env ? kImageEnvParamBatch : 256, kImageEnvParamBpc * s->n_cu);
    const auto kern = env_param_kernel((det_mode() ? 4 : 0) | (d_grad_env ? 2 : 0) | (reflect ? 1 : 0), std::make_integer_sequence<int, 8>{});
    kern<<<grid, 256, 0, st>>>(c.cam, c.band, c.n_pix, c.sc, c.tx, c.fresnel, bg, pc, c.snell, reflect ? w.tape : nullptr, park_ori, park_dir, w.thr, w.state, w.hits,
                               g_c, d_grad_env, d_grad_env_rot);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}
