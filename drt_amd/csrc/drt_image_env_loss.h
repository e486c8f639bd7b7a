// drt_image_env_loss.h -- what the two loss calls in front of an environment share (drt_image_env.hip: one view, DESIGN.md 10.8;
// drt_image_views_env.hip: up to 16 views): the reflection pass and the host body of the loss, each stated once over the
// view policy (drt_image_wave.h), and the host-side pieces the multi-view unit takes from drt_image_env.hip -- the check of the environment
// arguments and the launcher of k_image_reflect_mark (the view table's handle and its start launcher: drt_image_views_host.h).  A unit
// instantiates the forms it launches and no others.
//   k_image_reflect_list<SNELL, VIEW>            all samples : a sample that met the mesh forms its camera ray again with the camera of its ROW'S
//                                                              VIEW (view.at(r): band_sample's row is the row of the band, under ImageViewTable the
//                                                              row of the tall image, not of the view), recomputes the Bounce of its first face
//                                                              and, where that is an entering, non-TIR interaction, appends the float32 reflected ray
//                                                              to a list of its own
//   k_image_reflect_mark                         that list   : a reflected ray that found nothing sets kImageReflectSeen in its sample's state byte
//   k_image_reflect_bwd<DET, SNELL, VERTS, VIEW> the through list : a listed sample with the bit forms its camera ray again the same way and runs
//                                                              image_reflect_backward with the screen of its row's view
#pragma once
#include "drt_image_loss_bwd.h"
#include "drt_image_views_host.h"

// The arguments an environment call adds, after image_call_check: fills `bg` (defined in drt_image_env.hip).
int env_args_check(const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection, int fresnel, int channels, bool has_screen,
                   ImageScreenEnv& bg);

// k_image_reflect_mark over the traced reflection list on `st` (defined in drt_image_env.hip, which holds the kernel).
void launch_image_reflect_mark(int grid, hipStream_t st, RayList list, const unsigned* n_list, unsigned n_samples, uint8_t* state);

constexpr int kCntReflect = 34, kCntReflectRedo = 35;          // spare words of the counter block (drt_pathws.h): list size, second-pass count
static_assert(kCntReflectRedo < kCntWords && kCntReflect > kCntValid, "counter block layout");

template <bool SNELL, typename VIEW>
__global__ void __launch_bounds__(kPathBlock) k_image_reflect_list(PathCtx c, VIEW view, ImageBand band, const uint8_t* __restrict__ hits,
                                                                    const int32_t* __restrict__ first_face, RayList out, unsigned* count) {
    __shared__ StageMem stage;
    stage_init(stage);
    unsigned first, last;
    block_run(band.n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned i = base + threadIdx.x;
        bool go = false;
        f3 o32{0.f, 0.f, 0.f}, d32{0.f, 0.f, 1.f};
        if (i < band.n && hits[i] != 0) {
            int x, r, j;
            band_sample(band, i, x, r, j);
            const ImageViewAt v = view.at(r);
            d3 o, d, ro, wr;
            double R1;
            image_sample_ray(v.cam, band.s, x, v.y, j, o, d);
            go = image_reflect_first<SNELL>(c, first_face[i], o, d, ro, wr, R1);
            if (go) { o32 = to_f32(ro); d32 = to_f32(wr); }
        }
        stage_push(stage, go, (int32_t)i, o32, d32, out, count);
    }
    stage_flush(stage, out, count);
}

// The adjoint of the reflection term of every listed (through) sample whose reflection was added.
template <bool DET, bool SNELL, bool VERTS, typename VIEW>
__global__ void __launch_bounds__(256) k_image_reflect_bwd(PathCtx c, VIEW view, ImageBand band, ImageTex tx, ImageScreenEnv bg,
                                                           const int32_t* __restrict__ first_face, const uint8_t* __restrict__ state,
                                                           const int32_t* __restrict__ list, const unsigned* __restrict__ n_list,
                                                           const double* __restrict__ g_c, double* grad_verts, double* grad_ior) {
    int64_t n = *n_list;
    if (n > (int64_t)band.n) n = band.n;
    LossAcc<DET> acc_int, acc_ext;
    sink_pass<DET, kPathsBwdBatch, VERTS>(n, grad_verts, [&](int64_t k, auto add) {
        const int64_t i = list[k];
        if (i < 0 || i >= (int64_t)band.n || !(state[i] & kImageReflectSeen)) return;
        int x, r, j;
        band_sample(band, (unsigned)i, x, r, j);
        const ImageViewAt v = view.at(r);
        d3 o, d;
        image_sample_ray(v.cam, band.s, x, v.y, j, o, d);
        const int64_t pix = i / (band.s * band.s);
        double g[kImageMaxChannels] = {0.0, 0.0, 0.0};
        for (int ch = 0; ch < tx.c; ++ch) g[ch] = g_c[pix * tx.c + ch];
        double gi, ge;
        if (image_reflect_backward<SNELL>(c, first_face[i], o, d, v.sc, tx, bg.screen, bg.env, g, add, gi, ge)) { acc_int.add(gi); acc_ext.add(ge); }
    });
    if (grad_ior) {
        acc_int.flush(ior_slot<DET>(grad_ior, 0));
        acc_ext.flush(ior_slot<DET>(grad_ior, 1));
    }
}

template <typename VIEW, int... I>
auto reflect_bwd_kernel(int sel, std::integer_sequence<int, I...>) {
    using Kernel = decltype(&k_image_reflect_bwd<false, false, false, VIEW>);
    static const Kernel kernels[] = {k_image_reflect_bwd<(I & 4) != 0, (I & 2) != 0, (I & 1) != 0, VIEW>...};
    return kernels[sel];
}

// The reflection pass on `st`, behind the forward wavefront with the tape kept (a scene without triangles has direct samples only: nothing
// to do).
template <typename VIEW>
void reflection_pass(drt_scene* s, const PathCtx& pc, const ImageCall& c, const VIEW& view, hipStream_t st) {
    if (s->n_faces == 0) return;
    const PathsWs& w = *paths_ws_of(s);
    const RayList list{w.idx[0], w.ray[0], w.face[0]};          // (both ping-pong lists are free once the loop has ended)
    const int gs = grid_for(c.n, kPathBlock, 8 * s->n_cu);
    auto fill = c.snell ? k_image_reflect_list<true, VIEW> : k_image_reflect_list<false, VIEW>;
    fill<<<gs, kPathBlock, 0, st>>>(pc, view, c.band, w.hits, w.tape, list, w.cnt + kCntReflect);
    launch_trace_list(kTraceAny, s->grid_path, st, pc.tc, list.ray, w.cnt + kCntReflect, TraceOut{list.face, nullptr, nullptr, nullptr}, w.redo,
                      w.cnt + kCntReflectRedo, w.cnt + kCntDone, s->refill_min, s->inner_min, nullptr);
    launch_image_reflect_mark(gs, st, list, w.cnt + kCntReflect, (unsigned)c.n, w.state);
}

// The host body of an environment loss call behind its checks, image_loss_run's steps under a background: workspace, forward (`forward()`:
// the caller's wavefront, with the face tape kept), reflection pass, loss resolve, and -- on a scene with triangles, when a gradient or the
// count is wanted -- the list of through samples, the adjoint and the reflection's adjoint.  Afterwards the pixel seeds g_c, the state
// bytes, the parked rows, the throughputs and the tape are what the resolve read: between it and the return only w.idx[0] and the counter
// kCntValid are written (the through list).  PAYLOAD: ImageClear, or (drt_image_views_absorb.hip) an ImageAbsorb, taken
// by value and handed to `forward(pay)`, which completes it (the lengths' address), as image_loss_run does; its resolve also adds the
// sigma partials into out.grad_sigma.  The reflection's pass and adjoint are the same under both payloads: the reflected light never
// entered the object.
template <typename VIEW, typename Forward, typename PAYLOAD = ImageClear>
int env_loss_run(drt_scene* s, const double* d_verts, const ImageCall& c, const VIEW& view, Forward forward, const ImageScreenEnv& bg, bool reflection,
                 const ImageLossOut& out, hipStream_t st, const char* who, PAYLOAD pay = PAYLOAD{}) {
    { int rc = ensure_image_loss_ws(s, c.n_pix * c.tx.c, 0, st, who); if (rc) return rc; }
    if constexpr (std::is_invocable_v<Forward, PAYLOAD&>) { int rc = forward(pay); if (rc) return rc; }
    else { int rc = forward(); if (rc) return rc; }
    double* const grad_sigma = PAYLOAD::kAbsorb ? out.grad_sigma : nullptr;
    const PathCtx pc = image_path_ctx(s, d_verts, c);
    if (reflection) reflection_pass(s, pc, c, view, st);
    const PathsWs& w = *paths_ws_of(s);
    const ImageLossWs& lw = *static_cast<ImageLossWs*>(s->image_loss_ws);
    const unsigned pix_grid = (unsigned)((c.n_pix + kPathBlock - 1) / kPathBlock);
    if (reflection) {          // (the tape's address is read here, behind the forward that may have grown it)
        const ImageScreenEnvReflect bgr{bg.screen, bg.env, pc, c.snell, w.tape, nullptr};
        auto resolve = det_mode() ? k_image_loss_resolve<true, VIEW, PAYLOAD, ImageScreenEnvReflect>
                                  : k_image_loss_resolve<false, VIEW, PAYLOAD, ImageScreenEnvReflect>;
        resolve<<<pix_grid, kPathBlock, 0, st>>>(view, c.band, c.n_pix, c.tx, c.fill, c.fresnel, pay, w.park, w.park + 3 * w.fused_cap, w.thr, w.state,
                                                 w.hits, out.target, out.weight, lw.g_c, out.image, out.loss, grad_sigma, bgr);
    } else {
        auto resolve = det_mode() ? k_image_loss_resolve<true, VIEW, PAYLOAD, ImageScreenEnv>
                                  : k_image_loss_resolve<false, VIEW, PAYLOAD, ImageScreenEnv>;
        resolve<<<pix_grid, kPathBlock, 0, st>>>(view, c.band, c.n_pix, c.tx, c.fill, c.fresnel, pay, w.park, w.park + 3 * w.fused_cap, w.thr, w.state,
                                                 w.hits, out.target, out.weight, lw.g_c, out.image, out.loss, grad_sigma, bg);
    }
    if (s->n_faces > 0 && (out.grad_verts || out.grad_ior || out.count)) {
        int32_t* const done = w.idx[0];          // (the reflection list is no longer needed: its verdicts are in the state bytes)
        launch_paths_collect(grid_for(c.n, kPathBlock, 8 * s->n_cu), st, (unsigned)c.n, w.state, done, w.cnt + kCntValid);
        const int grid = (out.grad_verts ? DRT_BWD_BPC : kImageLossBpc) * s->n_cu;
        image_loss_bwd_kernel<VIEW, PAYLOAD, false, ImageScreenEnv>(det_mode(), c.snell, c.fresnel, out.grad_verts != nullptr)<<<grid, 256, 0, st>>>(
            pc, view, c.band, c.tx, pay, c.max_bounces, w.park, w.park + 3 * w.fused_cap, w.thr, w.tape, w.hits, done, w.cnt + kCntValid, lw.g_c,
            out.grad_verts, out.grad_ior, reinterpret_cast<unsigned long long*>(out.count), nullptr, bg);
        if (reflection && (out.grad_verts || out.grad_ior))
            reflect_bwd_kernel<VIEW>((det_mode() ? 4 : 0) | (c.snell ? 2 : 0) | (out.grad_verts ? 1 : 0), std::make_integer_sequence<int, 8>{})<<<grid, 256, 0, st>>>(
                pc, view, c.band, c.tx, bg, w.tape, w.state, done, w.cnt + kCntValid, lw.g_c, out.grad_verts, out.grad_ior);
    }
    HIP_TRY(hipGetLastError());
    return DRT_OK;
}
