// drt_image_camera.hip -- the camera gradient of the photometric loss of the refracted image (drt_image_camera.h holds the law; DESIGN.md
// 10.5): what drt_render_image_loss_camera (drt_image_loss.hip) enqueues beyond drt_render_image_loss_screen.  A unit of its own: a kernel's
// register allocation depends on the other kernels of its unit, and the kernels of drt_image_loss.hip and
// drt_image_screen.hip are to stay what they are.
//
//   k_image_loss_bwd<.., CAMERA>  the list : drt_image_loss_bwd.h's template <ImageOneView, ImageClear> with the flag on, in place of drt_image_loss.hip's launch: the same
//                                            vertex and IOR gradients and count, and the camera-ray seeds (g_o, g_d) that image_path_backward
//                                            ends with, stored under the sample index (48 bytes per sample of the band)
//   k_image_camera_bwd            all pixels : behind k_image_loss_resolve and the kernel above; image_pixel_walk's classes over the s x s
//                                            samples of its pixel: a direct sample's camera ray formed again and image_direct_seeds on it, a
//                                            through sample's on-screen verdict recomputed from its parked exit ray and its seeds read back;
//                                            image_sample_ray_backward per contributing sample into 21 LossAcc, summed over the block
//                                            (block_flush: one atomic per block and partial)
// No tree is read and no path recomputed by the second kernel.  Everything runs on the caller's stream, nothing is read back.
#include "drt_image_loss_bwd.h"
#include "drt_image_camera.h"

constexpr int kImageCameraBpc = 4;         // blocks per CU of k_image_camera_bwd (a grid-stride loop over the pixels; registers bound it)

// grad_camera: 21 accumulators (kinv, then rinv).  seeds may be null when no sample of the band is a through sample (a scene without
// triangles): it is read only for through samples.
template <bool DET>
__global__ void __launch_bounds__(256) k_image_camera_bwd(ImageCam cam, ImageBand band, int64_t n_pix, ImageScreen sc, ImageTex tx,
                                                          const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                          const uint8_t* __restrict__ state, const uint8_t* __restrict__ hits,
                                                          const double* __restrict__ g_c, const double* __restrict__ seeds, double* grad_camera) {
    LossAcc<DET> acc[kImageCamParams];
    const int s2 = band.s * band.s;
    for (int64_t pix = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; pix < n_pix; pix += (int64_t)gridDim.x * blockDim.x) {
        const int y = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
        double g[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int ch = 0; ch < tx.c; ++ch) g[ch] = g_c[pix * tx.c + ch];
        for (int j = 0; j < s2; ++j) {
            const int64_t i = pix * s2 + j;
            const int cls = image_class(hits[i] != 0, (state[i] & kPathDone) != 0);
            if (cls == kImageInvalid) continue;
            d3 g_o, g_d;
            if (cls == kImageDirect) {
                d3 o, d;
                image_sample_ray(cam, band.s, x, y, j, o, d);
                if (!image_direct_seeds(sc, tx, o, d, g, g_o, g_d)) continue;
            } else {
                if (!seeds || !image_through_on_screen(sc, tx, load_d3(park_ori, i), load_d3(park_dir, i))) continue;
                g_o = load_d3(seeds, i);
                g_d = load_d3(seeds + 3 * (int64_t)band.n, i);
            }
            double part[kImageCamParams];
#pragma unroll
            for (int k = 0; k < kImageCamParams; ++k) part[k] = 0.0;
            image_sample_ray_backward(cam, band.s, x, y, j, g_o, g_d, part, part + 9);
#pragma unroll
            for (int k = 0; k < kImageCamParams; ++k) acc[k].add(part[k]);
        }
    }
    block_flush<DET, kImageCamParams>(acc, grad_camera);
}

int launch_image_loss_bwd_camera(const drt_scene* s, const PathCtx& pc, const ImageCall& c, const ImageOneView& view, const ImageClear& pay, int grid,
                                 const int32_t* list, const unsigned* n_list, const double* g_c, const ImageLossOut& out, double* seeds, hipStream_t st) {
    return image_loss_bwd_launch<ImageOneView, ImageClear, true>(s, pc, c, view, pay, grid, list, n_list, g_c, out, seeds, st);
}

int launch_image_camera_bwd(const drt_scene* s, const ImageCall& c, const double* g_c, const double* seeds, double* d_grad_camera, hipStream_t st) {
    const PathsWs& w = *static_cast<const PathsWs*>(s->paths_ws);
    const double* const park_ori = w.park;
    const double* const park_dir = w.park + 3 * w.fused_cap;
    const int grid = grid_for(c.n_pix, 256, kImageCameraBpc * s->n_cu);
    if (det_mode()) k_image_camera_bwd<true><<<grid, 256, 0, st>>>(c.cam, c.band, c.n_pix, c.sc, c.tx, park_ori, park_dir, w.state, w.hits, g_c, seeds, d_grad_camera);
    else k_image_camera_bwd<false><<<grid, 256, 0, st>>>(c.cam, c.band, c.n_pix, c.sc, c.tx, park_ori, park_dir, w.state, w.hits, g_c, seeds, d_grad_camera);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}
