// drt_image_screen.hip -- the screen-pose and texture gradients of the photometric loss of the refracted image (drt_image_screen.h holds
// the law): one more pass of drt_render_image_loss_screen (drt_image_loss.hip) over the pixels of the band, behind
// k_image_loss_resolve, which has written the pixel seeds g_c.  A unit of its own: a kernel's register allocation depends on the other
// kernels of its unit, and the kernels of drt_image_loss.hip are to stay what they are.
//
//   k_image_screen_bwd  all pixels : image_pixel_walk's walk over the s x s samples of its pixel -- a direct sample's camera ray formed again,
//                                    a through sample's exit ray and throughput from the parked rows -- and image_sample_backward_screen per
//                                    sample that lands on the screen: the nine screen partials through nine LossAcc summed over the block
//                                    (block_flush, drt_image_wave.h: one atomic per block and partial), the four texel contributions through PathSink in
//                                    kImageScreenBatch-sized fills (sink_pass); TEXTURE = false: no table in LDS
// The texture gradient in the sink: with three channels the texel number is the id and the channels are the d3; with one channel the id is
// texel / 3 and one component is non-zero, which is why the accumulator is padded to a multiple of three values.  No tree is read and no
// path recomputed.  Everything runs on the caller's stream, nothing is read back.
#include "drt_image_wave.h"
#include "drt_image_screen.h"

// Pixels per table fill.  A pixel brings up to 4 s^2 <= 64 texel references, but the 256 neighbouring pixels of a fill look at neighbouring
// texels: direct samples, nine in ten, revisit the cells of their neighbours, and the distinct texels of a fill are about two texture rows
// of 256 * (texels per pixel) -- what kPathsBwdBatch paths of up to 24 vertex references each bring to the same table.  A table that does
// fill up sends the rest straight to memory (HashAdd3 / FxHashAdd3), so the batch only bounds the cost, never the result.
constexpr int kImageScreenBatch = kPathsBwdBatch;
constexpr int kImageScreenBpc = DRT_BWD_BPC;       // 56 KB of table per block

// grad_screen (nine accumulators: p0, eu, ev) and grad_texture (TEXTURE) may each be null.
template <bool DET, bool TEXTURE>
__global__ void __launch_bounds__(256) k_image_screen_bwd(ImageCam cam, ImageBand band, int64_t n_pix, ImageScreen sc, ImageTex tx, bool fresnel,
                                                          const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                          const double* __restrict__ thr, const uint8_t* __restrict__ state,
                                                          const uint8_t* __restrict__ hits, const double* __restrict__ g_c, double* grad_screen,
                                                          double* grad_texture) {
    LossAcc<DET> acc[9];
    const int s2 = band.s * band.s;
    sink_pass<DET, kImageScreenBatch, TEXTURE>(n_pix, grad_texture, [&](int64_t pix, auto add) {
        const int y = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
        double g[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int ch = 0; ch < tx.c; ++ch) g[ch] = g_c[pix * tx.c + ch];
        const bool rgb = tx.c == 3;
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
            const d3 z{0.0, 0.0, 0.0};
            d3 g_p0 = z, g_eu = z, g_ev = z;
            const bool on = image_sample_backward_screen(sc, tx, o, d, T, g, [&](int32_t texel, const double* gt) {
                if (rgb) { add(texel, d3{gt[0], gt[1], gt[2]}); return; }
                const int32_t id = texel / 3;
                const int k = texel - 3 * id;
                add(id, d3{k == 0 ? gt[0] : 0.0, k == 1 ? gt[0] : 0.0, k == 2 ? gt[0] : 0.0});
            }, g_p0, g_eu, g_ev);
            if (!on) continue;
            acc[0].add(g_p0.x); acc[1].add(g_p0.y); acc[2].add(g_p0.z);
            acc[3].add(g_eu.x); acc[4].add(g_eu.y); acc[5].add(g_eu.z);
            acc[6].add(g_ev.x); acc[7].add(g_ev.y); acc[8].add(g_ev.z);
        }
    });
    if (grad_screen) block_flush<DET, 9>(acc, grad_screen);
}

int launch_image_screen_bwd(const drt_scene* s, const ImageCall& c, const double* g_c, double* d_grad_screen, double* d_grad_texture, hipStream_t st) {
    const PathsWs& w = *static_cast<const PathsWs*>(s->paths_ws);
    const double* const park_ori = w.park;
    const double* const park_dir = w.park + 3 * w.fused_cap;
    const int grid = grid_for(c.n_pix, d_grad_texture ? kImageScreenBatch : 256, kImageScreenBpc * s->n_cu);
    const bool det = det_mode();
    const auto kern = d_grad_texture ? (det ? k_image_screen_bwd<true, true> : k_image_screen_bwd<false, true>)
                                     : (det ? k_image_screen_bwd<true, false> : k_image_screen_bwd<false, false>);
    kern<<<grid, 256, 0, st>>>(c.cam, c.band, c.n_pix, c.sc, c.tx, c.fresnel, park_ori, park_dir, w.thr, w.state, w.hits, g_c, d_grad_screen, d_grad_texture);
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}
