// drt_image_loss_bwd.h -- k_image_loss_bwd, the adjoint of the photometric image loss over the compact list of through samples, as a
// template two units instantiate: drt_image_loss.hip the sixteen kernels without CAMERA (drt_render_image_loss), and
// drt_image_camera.hip the sixteen with it, which also park every sample's camera-ray seeds for k_image_camera_bwd.
// Two units because a kernel's register allocation depends on the other kernels of its unit.
#pragma once
#include "drt_image_wave.h"
#include "drt_image_loss.h"

// The adjoint of one listed sample (image_sample_backward) with the sink of the caller's choice.
template <bool SNELL, bool FRESNEL, typename Add>
__device__ __forceinline__ bool loss_bwd_sample(const PathCtx& c, const ImageCam& cam, const ImageBand& band, const ImageScreen& sc, const ImageTex& tx,
                                                int max_bounces, const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                const double* __restrict__ thr, const int32_t* __restrict__ tape, const uint8_t* __restrict__ hits,
                                                const double* __restrict__ g_c, int64_t i, Add add, double& gi, double& ge, d3* seed_o = nullptr,
                                                d3* seed_d = nullptr) {
    int x, y, j;
    band_sample(band, (unsigned)i, x, y, j);
    d3 o, d;
    image_sample_ray(cam, band.s, x, y, j, o, d);
    const int64_t pix = i / (band.s * band.s);
    double g[kImageMaxChannels] = {0.0, 0.0, 0.0};
    for (int ch = 0; ch < tx.c; ++ch) g[ch] = g_c[pix * tx.c + ch];
    return image_sample_backward<SNELL, FRESNEL>(c, o, d, tape + i, (int64_t)band.n, min((int)hits[i], max_bounces), load_d3(park_ori, i),
                                                 load_d3(park_dir, i), FRESNEL ? thr[i] : 1.0, sc, tx, g, add, gi, ge, seed_o, seed_d);
}

// grad_verts (VERTS), grad_ior and count may each be null.  CAMERA: seeds [2, band.n, 3] receives (g_o; g_d) of every listed sample that
// lands on the screen, under its sample index; the other rows are left as they are.
template <bool DET, bool SNELL, bool FRESNEL, bool VERTS, bool CAMERA>
__global__ void __launch_bounds__(256) k_image_loss_bwd(PathCtx c, ImageCam cam, ImageBand band, ImageScreen sc, ImageTex tx, int max_bounces,
                                                        const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                        const double* __restrict__ thr, const int32_t* __restrict__ tape,
                                                        const uint8_t* __restrict__ hits, const int32_t* __restrict__ list,
                                                        const unsigned* __restrict__ n_list, const double* __restrict__ g_c, double* grad_verts,
                                                        double* grad_ior, unsigned long long* count, double* seeds) {
    int64_t n = *n_list;
    if (n > (int64_t)band.n) n = band.n;
    LossAcc<DET> acc_int, acc_ext;
    unsigned cnt = 0;
    sink_pass<DET, kPathsBwdBatch, VERTS>(n, grad_verts, [&](int64_t k, auto add) {
        const int64_t i = list[k];
        if (i < 0 || i >= (int64_t)band.n) return;
        double gi, ge;
        if constexpr (CAMERA) {
            d3 so, sd;
            if (loss_bwd_sample<SNELL, FRESNEL>(c, cam, band, sc, tx, max_bounces, park_ori, park_dir, thr, tape, hits, g_c, i, add, gi, ge, &so, &sd)) {
                acc_int.add(gi); acc_ext.add(ge);
                ++cnt;
                store_d3(seeds, i, so);
                store_d3(seeds + 3 * (int64_t)band.n, i, sd);
            }
        } else {
            if (loss_bwd_sample<SNELL, FRESNEL>(c, cam, band, sc, tx, max_bounces, park_ori, park_dir, thr, tape, hits, g_c, i, add, gi, ge)) {
                acc_int.add(gi); acc_ext.add(ge);
                ++cnt;
            }
        }
    });
    if (grad_ior) {
        acc_int.flush(ior_slot<DET>(grad_ior, 0));
        acc_ext.flush(ior_slot<DET>(grad_ior, 1));
    }
    if (count && cnt) atomicAdd(count, (unsigned long long)cnt);
}

// k_image_loss_bwd<., ., ., ., CAMERA> under (deterministic, snell, fresnel, verts); CAMERA is a literal
#define IMAGE_LOSS_BWD_LAUNCH(CAMERA, det, snell, fresnel, verts, grid, st, ...)                                              \
    do {                                                                                                                      \
        const int sel_ = ((det) ? 8 : 0) | ((snell) ? 4 : 0) | ((fresnel) ? 2 : 0) | ((verts) ? 1 : 0);                       \
        switch (sel_) {                                                                                                       \
        case 0: k_image_loss_bwd<false, false, false, false, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;               \
        case 1: k_image_loss_bwd<false, false, false, true, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 2: k_image_loss_bwd<false, false, true, false, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 3: k_image_loss_bwd<false, false, true, true, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 4: k_image_loss_bwd<false, true, false, false, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 5: k_image_loss_bwd<false, true, false, true, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 6: k_image_loss_bwd<false, true, true, false, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 7: k_image_loss_bwd<false, true, true, true, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                  \
        case 8: k_image_loss_bwd<true, false, false, false, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 9: k_image_loss_bwd<true, false, false, true, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 10: k_image_loss_bwd<true, false, true, false, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 11: k_image_loss_bwd<true, false, true, true, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 12: k_image_loss_bwd<true, true, false, false, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                \
        case 13: k_image_loss_bwd<true, true, false, true, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        case 14: k_image_loss_bwd<true, true, true, false, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                 \
        default: k_image_loss_bwd<true, true, true, true, CAMERA><<<grid, 256, 0, st>>>(__VA_ARGS__); break;                  \
        }                                                                                                                     \
    } while (0)
