// drt_image_loss_bwd.h -- the loss half of the refracted-image family (drt_image_wave.h holds the forward half and the two policies),
// each kernel once as a template: k_image_loss_resolve<DET, VIEW, PAYLOAD> and k_image_loss_bwd<DET, SNELL, FRESNEL, VERTS, VIEW, PAYLOAD,
// CAMERA>, the adjoint over the compact list of through samples, with the one selector of its sixteen forms and the one host body of a
// loss call.  Four units instantiate them: drt_image_loss.hip <ImageOneView, ImageClear> (drt_render_image_loss),
// drt_image_camera.hip the same with CAMERA, which also parks every sample's camera-ray seeds for k_image_camera_bwd (10.5),
// drt_image_views.hip <ImageViewTable, ImageClear> (10.6) and drt_image_absorb.hip <ImageOneView, ImageAbsorb> (10.7).
// Four units because a kernel's register allocation depends on the other kernels of its unit.  For the same reason the
// forms under an environment have units of their own: drt_image_env.hip <ImageOneView, ImageClear, ., ImageScreenEnv[Reflect]> (10.8) and
// drt_image_views_env.hip <ImageViewTable, ImageClear, ., ImageScreenEnv[Reflect]> (10.10), through env_loss_run (drt_image_env_loss.h);
// and drt_image_views_absorb.hip <ImageViewTable, ImageAbsorb> under all three backgrounds (10.13).
#pragma once
#include "drt_image_wave.h"
#include "drt_image_loss.h"

// One thread per pixel of the band: k_image_resolve's walk over the s x s samples of its pixel (image_pixel_walk); the float64 mean I, the
// residual against the target, the loss term (LossAcc), the seed g_c = 2 w r / s^2 of the pixel's samples [n_pix, C]; optionally the
// float32 image -- the bits k_image_resolve writes.  target and weight are addressed at the view's row (ImageViewAt::row).  ImageAbsorb:
// also the C sigma partials -g_c[ch] sum_j L_j c_j[ch], which need forward values only (LossAcc x 3 through block_flush).
// weight / image / grad_sigma may be null.  (The channel loops are spelt per payload, as in image_pixel_walk.)  BACKGROUND: the walk's
// (drt_image_wave.h); the default is the screen alone, the text of before.
template <bool DET, typename VIEW, typename PAYLOAD, typename BACKGROUND = ImageScreenOnly>
__global__ void __launch_bounds__(kPathBlock) k_image_loss_resolve(VIEW view, ImageBand band, int64_t n_pix, ImageTex tx, ImageFill fill, bool fresnel, PAYLOAD pay,
                                                                    const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                                    const double* __restrict__ thr, const uint8_t* __restrict__ state,
                                                                    const uint8_t* __restrict__ hits, const float* __restrict__ target,
                                                                    const float* __restrict__ weight, double* __restrict__ g_c,
                                                                    float* __restrict__ image, double* loss, double* grad_sigma,
                                                                    BACKGROUND bg = BACKGROUND{}) {
    static_assert(!(PAYLOAD::kAbsorb && BACKGROUND::kEnv) || std::is_same_v<VIEW, ImageViewTable>, "absorbing glass in a room: under the view table only");
    const int64_t pix = (int64_t)blockIdx.x * kPathBlock + threadIdx.x;
    LossAcc<DET> acc;
    [[maybe_unused]] LossAcc<DET> sig[kImageMaxChannels];
    if (pix < n_pix) {
        const int s2 = band.s * band.s;
        const int r = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
        const ImageViewAt v = view.at(r);
        double sum[kImageMaxChannels] = {0.0, 0.0, 0.0};
        typename PAYLOAD::Sums more;
        int n_hit, n_through;          // (not wanted here)
        image_pixel_walk(v.cam, band, pix, x, v.y, v.sc, tx, fill, fresnel, pay, park_ori, park_dir, thr, state, hits, sum, more, n_hit, n_through, bg);
        const int64_t row = v.row * band.width + x;
        if constexpr (PAYLOAD::kAbsorb) {
            double mean[kImageMaxChannels] = {0.0, 0.0, 0.0}, g[kImageMaxChannels] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int ch = 0; ch < kImageMaxChannels; ++ch) {
                if (ch >= tx.c) continue;
                mean[ch] = sum[ch] / (double)s2;
                if (image) image[row * tx.c + ch] = (float)mean[ch];
            }
            acc.add(image_loss_pixel(mean, tx.c, s2, target + row * tx.c, weight ? (double)weight[row] : 1.0, g));
#pragma unroll
            for (int ch = 0; ch < kImageMaxChannels; ++ch) {
                if (ch >= tx.c) continue;
                g_c[pix * tx.c + ch] = g[ch];
                sig[ch].add(image_absorb_sigma_term(g[ch], more.lc[ch]));
            }
        } else {
            double mean[kImageMaxChannels], g[kImageMaxChannels];
            for (int ch = 0; ch < tx.c; ++ch) {
                mean[ch] = sum[ch] / (double)s2;
                if (image) image[row * tx.c + ch] = (float)mean[ch];
            }
            acc.add(image_loss_pixel(mean, tx.c, s2, target + row * tx.c, weight ? (double)weight[row] : 1.0, g));
            for (int ch = 0; ch < tx.c; ++ch) g_c[pix * tx.c + ch] = g[ch];
        }
    }
    acc.flush(loss);
    if constexpr (PAYLOAD::kAbsorb) {
        if (grad_sigma) {              // (the same in every thread; tx.c accumulators, never more)
            if (tx.c == kImageMaxChannels) block_flush<DET, kImageMaxChannels>(sig, grad_sigma);
            else block_flush<DET, 1>(sig, grad_sigma);
        }
    }
}

// The adjoint of every listed sample (image_sample_backward): the camera ray formed again with the camera of the sample's row
// (image_sample_ray), exit ray and T -- ImageAbsorb: and L -- from the parked rows, g_c of pixel i / s^2; vertex gradients through PathSink
// in kPathsBwdBatch-sized fills, the IOR partials through two LossAcc; VERTS = false: no table in LDS.  grad_verts (VERTS), grad_ior and
// count may each be null.  CAMERA: seeds [2, band.n, 3] receives (g_o; g_d) of every listed sample that lands on the screen, under its
// sample index; the other rows are left as they are.  The absorbing forms with the table ask for two blocks per CU: without that bound
// they drop to one wave (profiles/image_absorb_resources.txt); in front of an environment they do not ask for it: under that bound the
// forms with the table spill 35 to 157 VGPRs, without it they run one wave and spill at most 4 (profiles/image_views_absorb_resources.txt).
// BACKGROUND with an environment (no CAMERA; ImageAbsorb under the view
// table only, drt_image_views_absorb.hip): every listed
// sample carries a gradient, through the screen where its exit ray lands on it and through the environment lookup otherwise
// (image_env_sample_backward); the reflection's adjoint is a kernel of its own (drt_image_env.hip).
template <bool DET, bool SNELL, bool FRESNEL, bool VERTS, typename VIEW, typename PAYLOAD, bool CAMERA, typename BACKGROUND = ImageScreenOnly>
__global__ void __launch_bounds__(256, PAYLOAD::kAbsorb && VERTS && !BACKGROUND::kEnv ? 2 : 1)
    k_image_loss_bwd(PathCtx c, VIEW view, ImageBand band, ImageTex tx, PAYLOAD pay, int max_bounces, const double* __restrict__ park_ori,
                     const double* __restrict__ park_dir, const double* __restrict__ thr, const int32_t* __restrict__ tape,
                     const uint8_t* __restrict__ hits, const int32_t* __restrict__ list, const unsigned* __restrict__ n_list,
                     const double* __restrict__ g_c, double* grad_verts, double* grad_ior, unsigned long long* count, double* seeds,
                     BACKGROUND bg = BACKGROUND{}) {
    int64_t n = *n_list;
    if (n > (int64_t)band.n) n = band.n;
    LossAcc<DET> acc_int, acc_ext;
    unsigned cnt = 0;
    sink_pass<DET, kPathsBwdBatch, VERTS>(n, grad_verts, [&](int64_t k, auto add) {
        const int64_t i = list[k];
        if (i < 0 || i >= (int64_t)band.n) return;
        int x, r, j;
        band_sample(band, (unsigned)i, x, r, j);
        const ImageViewAt v = view.at(r);
        d3 o, d;
        image_sample_ray(v.cam, band.s, x, v.y, j, o, d);
        const int64_t pix = i / (band.s * band.s);
        double g[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int ch = 0; ch < tx.c; ++ch) g[ch] = g_c[pix * tx.c + ch];
        double L = 0.0;
        const double* sigma = nullptr;
        if constexpr (PAYLOAD::kAbsorb) { L = pay.len[i]; sigma = pay.sigma.v; }
        [[maybe_unused]] d3 so, sd;
        double gi, ge;
        bool carried;
        if constexpr (BACKGROUND::kEnv) {
            static_assert(!CAMERA, "an environment goes without camera seeds");
            static_assert(!PAYLOAD::kAbsorb || std::is_same_v<VIEW, ImageViewTable>, "absorbing glass in a room: under the view table only");
            carried = image_env_sample_backward<SNELL, FRESNEL, PAYLOAD::kAbsorb>(c, o, d, tape + i, (int64_t)band.n, min((int)hits[i], max_bounces),
                                                                                  load_d3(park_ori, i), load_d3(park_dir, i), FRESNEL ? thr[i] : 1.0, v.sc, tx,
                                                                                  bg.screen, bg.env, g, add, gi, ge, L, sigma);
        } else {
            carried = image_sample_backward<SNELL, FRESNEL, PAYLOAD::kAbsorb>(c, o, d, tape + i, (int64_t)band.n, min((int)hits[i], max_bounces), load_d3(park_ori, i),
                                                                              load_d3(park_dir, i), FRESNEL ? thr[i] : 1.0, v.sc, tx, g, add, gi, ge,
                                                                              CAMERA ? &so : nullptr, CAMERA ? &sd : nullptr, L, sigma);
        }
        if (carried) {
            acc_int.add(gi); acc_ext.add(ge);
            ++cnt;
            if constexpr (CAMERA) {
                store_d3(seeds, i, so);
                store_d3(seeds + 3 * (int64_t)band.n, i, sd);
            }
        }
    });
    if (grad_ior) {
        acc_int.flush(ior_slot<DET>(grad_ior, 0));
        acc_ext.flush(ior_slot<DET>(grad_ior, 1));
    }
    if (count && cnt) atomicAdd(count, (unsigned long long)cnt);
}

// k_image_loss_bwd<., ., ., ., VIEW, PAYLOAD, CAMERA> under (deterministic, snell, fresnel, verts), from a table of the sixteen
template <typename VIEW, typename PAYLOAD, bool CAMERA, typename BACKGROUND, int... I>
auto image_loss_bwd_kernel(int sel, std::integer_sequence<int, I...>) {
    using Kernel = decltype(&k_image_loss_bwd<false, false, false, false, VIEW, PAYLOAD, CAMERA, BACKGROUND>);
    static const Kernel kernels[] = {k_image_loss_bwd<(I & 8) != 0, (I & 4) != 0, (I & 2) != 0, (I & 1) != 0, VIEW, PAYLOAD, CAMERA, BACKGROUND>...};
    return kernels[sel];
}
template <typename VIEW, typename PAYLOAD, bool CAMERA, typename BACKGROUND = ImageScreenOnly>
auto image_loss_bwd_kernel(bool det, bool snell, bool fresnel, bool verts) {
    return image_loss_bwd_kernel<VIEW, PAYLOAD, CAMERA, BACKGROUND>((det ? 8 : 0) | (snell ? 4 : 0) | (fresnel ? 2 : 0) | (verts ? 1 : 0), std::make_integer_sequence<int, 16>{});
}

// The adjoint launch of a loss call on `st`, behind the resolve kernel (g_c) and launch_paths_collect (list, n_list): k_image_loss_bwd
// of the caller's policies over the workspace image_forward filled.  seeds: CAMERA only.
template <typename VIEW, typename PAYLOAD, bool CAMERA>
int image_loss_bwd_launch(const drt_scene* s, const PathCtx& pc, const ImageCall& c, const VIEW& view, const PAYLOAD& pay, int grid, const int32_t* list,
                          const unsigned* n_list, const double* g_c, const ImageLossOut& out, double* seeds, hipStream_t st) {
    const PathsWs& w = *static_cast<const PathsWs*>(s->paths_ws);
    image_loss_bwd_kernel<VIEW, PAYLOAD, CAMERA>(det_mode(), c.snell, c.fresnel, out.grad_verts != nullptr)<<<grid, 256, 0, st>>>(
        pc, view, c.band, c.tx, pay, c.max_bounces, w.park, w.park + 3 * w.fused_cap, w.thr, w.tape, w.hits, list, n_list, g_c, out.grad_verts, out.grad_ior,
        reinterpret_cast<unsigned long long*>(out.count), seeds, ImageScreenOnly{});
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}
template <typename VIEW, typename PAYLOAD>
using ImageLossBwdLaunch = decltype(&image_loss_bwd_launch<VIEW, PAYLOAD, false>);
// The one host body of a loss call after its argument checks: the workspace of the loss grown (n_cam doubles of camera-ray seeds; 0: none
// wanted), the forward wavefront (`forward(pay)`: the caller's, with the face tape kept; it may complete the payload), the loss resolve,
// and -- on a scene with triangles, when a gradient, the count or the seeds are wanted -- the list of through samples and the adjoint
// (`bwd`: image_loss_bwd_launch of the caller's unit, or launch_image_loss_bwd_camera).  A unit instantiates it with its own policies, so
// the kernels it launches are emitted there.
template <typename VIEW, typename PAYLOAD, typename Forward>
int image_loss_run(drt_scene* s, const double* d_verts, const ImageCall& c, const VIEW& view, PAYLOAD pay, Forward forward, ImageLossBwdLaunch<VIEW, PAYLOAD> bwd,
                   const ImageLossOut& out, int64_t n_cam, hipStream_t st, const char* who) {
    { int rc = ensure_image_loss_ws(s, c.n_pix * c.tx.c, n_cam, st, who); if (rc) return rc; }
    { int rc = forward(pay); if (rc) return rc; }
    const PathsWs& w = *paths_ws_of(s);
    const ImageLossWs& lw = *static_cast<ImageLossWs*>(s->image_loss_ws);
    const unsigned pix_grid = (unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock);
    auto resolve = det_mode() ? k_image_loss_resolve<true, VIEW, PAYLOAD> : k_image_loss_resolve<false, VIEW, PAYLOAD>;
    resolve<<<pix_grid, kPathBlock, 0, st>>>(view, c.band, c.n_pix, c.tx, c.fill, c.fresnel, pay, w.park, w.park + 3 * w.fused_cap, w.thr, w.state, w.hits, out.target,
                                             out.weight, lw.g_c, out.image, out.loss, out.grad_sigma, ImageScreenOnly{});
    if (s->n_faces > 0 && (out.grad_verts || out.grad_ior || out.count || n_cam)) {
        int32_t* const done = w.idx[0];          // (both ping-pong lists are free once the loop has ended)
        launch_paths_collect(grid_for(c.n, kPathBlock, 8 * s->n_cu), st, (unsigned)c.n, w.state, done, w.cnt + kCntValid);
        const int grid = (out.grad_verts ? DRT_BWD_BPC : kImageLossBpc) * s->n_cu;
        int rc = bwd(s, image_path_ctx(s, d_verts, c), c, view, pay, grid, done, w.cnt + kCntValid, lw.g_c, out, n_cam ? lw.seeds : nullptr, st);
        if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}
