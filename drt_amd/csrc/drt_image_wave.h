// drt_image_wave.h -- what the calls on the refracted image share (drt_image.hip, drt_image_loss.hip, drt_image_screen.hip,
// drt_image_camera.hip, drt_image_views.hip, drt_image_absorb.hip, drt_image_env.hip, drt_image_env_param.hip, drt_image_views_env.hip): the band of rows of one call, the checked call, the two policies a
// kernel of the family is stated over, and the forward half of the family, each kernel once as a template -- k_image_start<VIEW>,
// k_image_shade<SNELL, FRESNEL, TAPE, PAYLOAD>, image_pixel_walk<PAYLOAD, BACKGROUND>, k_image_resolve<PAYLOAD, BACKGROUND> -- with the forward
// wavefront that launches them (defined in drt_image.hip, as launch_trace_list is in drt_trace.hip).  drt_image_loss_bwd.h holds the loss half.
//   VIEW        where a row of the band finds its camera and screen: ImageOneView (by value, the call's own) or ImageViewTable (the capture's
//               table in device memory and the call's id list)
//   PAYLOAD     what a sample carries beside its throughput: ImageClear (nothing) or ImageAbsorb (the interior length and sigma)
//   BACKGROUND  what a sample's exit ray looks at: ImageScreenOnly (the screen, `void` beside it: the default, and the text of before) or
//               ImageScreenEnv (a screen or none, and an environment map where the screen is not: drt_image_env.h)
// A unit instantiates the forms it launches and no others, so a kernel stays in the unit that held it before there was a template
// (a kernel's register allocation depends on the other kernels of its unit: DESIGN.md section 4).
#pragma once
#include <type_traits>
#include <utility>
#include "drt_device.h"
#include "drt_pathws.h"
#include "drt_image.h"
#include "drt_image_env.h"
#include "drt_image_views.h"

struct ImageBand {
    int width, y0, s;              // image width, first row of the band, supersampling
    unsigned n;                    // samples of the band: rows * width * s * s
};

// sample i of the band -> its pixel and its number within the pixel
__device__ __forceinline__ void band_sample(const ImageBand& b, unsigned i, int& x, int& y, int& j) {
    const unsigned s2 = (unsigned)(b.s * b.s), pix = i / s2;
    j = (int)(i - pix * s2);
    y = b.y0 + (int)(pix / (unsigned)b.width);
    x = (int)(pix % (unsigned)b.width);
}

struct ImageFill { double c_void[kImageMaxChannels], c_invalid[kImageMaxChannels]; };

// ---- the view policy: row r of the band (band_sample's y; of a pixel, band.y0 + pix / width) -> whose row it is
struct ImageViewAt {
    const ImageCam& cam;
    const ImageScreen& sc;
    int y;                         // the row within the view
    int64_t row;                   // the row of the target / weight planes: pixel (x, y) of the view is at row * width + x
};
// the camera and the screen of the call, by value
struct ImageOneView {
    ImageCam cam;
    ImageScreen sc;
    __device__ __forceinline__ ImageViewAt at(int r) const { return ImageViewAt{cam, sc, r, (int64_t)r}; }
};
// a band of the tall image of the listed views (drt_image_views.h): camera and screen are references into the table, read where
// image_sample_ray and the plane use them; target and weight are the capture's stacks, addressed at ((view * H + y) * W + x)
struct ImageViewTable {
    const ImageViewRow* __restrict__ rows;
    ImageViewIds ids;
    __device__ __forceinline__ ImageViewAt at(int r) const {
        int slot, view, y;
        image_views_row(ids, r, slot, view, y);
        const ImageViewRow& vr = rows[view];
        return ImageViewAt{vr.cam, vr.sc, y, (int64_t)view * ids.height + y};
    }
};

// ---- the payload policy: what a sample carries beside its throughput, and what a pixel sums beside its colours
struct ImageSigma { double v[kImageMaxChannels]; };
struct ImageClear {
    static constexpr bool kAbsorb = false;
    struct Sums {};
};
struct ImageAbsorb {
    static constexpr bool kAbsorb = true;
    double* __restrict__ len;      // the interior length of every sample of the band (PathsWs::len)
    ImageSigma sigma;
    struct Sums {
        double lc[kImageMaxChannels] = {0.0, 0.0, 0.0};          // that of L_j c_j[ch] over the lit through samples, transmitted part only (the sigma partials)
        double l_sum;                                            // that of L over the through samples
    };
};

// ---- the background policy: where the colour of a direct or through sample comes from.  A form without an environment holds no trace of
// it (`if constexpr (BACKGROUND::kEnv)`, as kAbsorb).  With ImageAbsorb it goes under ImageViewTable only (drt_image_views_absorb.hip,
// DESIGN.md 10.13): the single-view pair is never instantiated.
struct ImageScreenOnly { static constexpr bool kEnv = false; };
struct ImageScreenEnv {
    static constexpr bool kEnv = true, kReflect = false;
    bool screen;                   // false: the call has no screen (and no texture); every ray sees the environment
    ImageEnv env;
};
// ... with the reflection off the outer surface added to a through sample whose reflected ray was seen to leave unoccluded (the bit
// kImageReflectSeen of its state byte, set by drt_image_env.hip's reflection pass): the walk forms the camera ray again and recomputes the
// one Bounce of the first face (tape row 0), as it does the camera ray of a direct sample
constexpr uint8_t kImageReflectSeen = 0x40;          // beside the refraction count (<= 8) and kPathDone (0x80)
struct ImageScreenEnvReflect {
    static constexpr bool kEnv = true, kReflect = true;
    bool screen;
    ImageEnv env;
    PathCtx pc;
    bool snell;
    const int32_t* __restrict__ first_face;          // tape row 0: the face of every sample's first interaction
    float* __restrict__ reflect;                     // the plane `reflect` [height, width], may be null
};

// One call after image_call_check: the arguments the two entry points have in common, unpacked.
struct ImageCall {
    ImageCam cam;
    ImageScreen sc;
    ImageTex tx;
    ImageFill fill;
    ImageBand band;
    int64_t n_pix, n;              // pixels and samples of the band
    double ior_int, ior_ext;
    int max_bounces;
    bool reflect, snell, fresnel;
};

// The argument checks of the two entry points (after CHECK_BUILT), in the order in which their errors win: scalars, host pointers, the
// entry point's own device pointers (device_ok, and device_msg when not), the screen, the sample count.  Fills `call` on DRT_OK.
int image_call_check(const double* camera21, int height, int width, int y0, int y1, int supersample, double ior_int, double ior_ext, int max_bounces,
                     int law_flags, int fresnel, const double* screen9, const float* d_texture, int tex_h, int tex_w, int channels,
                     const double* fill_void, const double* fill_invalid, bool device_ok, const char* device_msg, ImageCall& call);

// The forward wavefront on `st`: the workspace grown to the band (ray lists, rows of the one-pass form, throughputs; never inside a stream
// capture), the build waited for, the counters zeroed, k_image_start, then K + 1 rounds of k_trace and k_image_shade.  Afterwards the
// workspace holds per sample the state byte, the hit count, the parked exit ray and the throughput; with keep_tape also the face tape
// [K, n] -- without it the tape is left untouched.  `who`: the entry point, for messages.
int image_forward(drt_scene* s, const double* d_verts, const ImageCall& call, bool keep_tape, hipStream_t st, const char* who);

// image_forward with the start and shade kernels of the caller's choice, so that a kernel form is emitted in the unit that asks for it:
// `start` launches k_image_start<VIEW> on a.st, with a.grid blocks of kPathBlock threads; `shade` launches for list k the form of
// k_image_shade of its payload (image_shade_launch).  `src` / `shade_src` are handed through to them.  Null `shade`, the default:
// k_image_shade<., ., ., ImageClear> from drt_image.hip.  image_forward is this with image_start_call and the default shade.
struct ImageStartArgs {
    const Node4Q* nodes;
    int n_tris;
    double *park_ori, *park_dir, *thr;
    uint8_t *state, *hits;
    RayList out;
    unsigned* count;
    int grid;
    hipStream_t st;
};
using ImageStartFn = void (*)(const ImageStartArgs& a, const void* src);
struct ImageShadeArgs {
    PathCtx pc;
    int64_t n_rays;
    int k, max_bounces;
    bool reflect, snell, fresnel;
    RayList in;
    const unsigned* n_in;
    RayList out;
    unsigned* n_out;
    double *park_ori, *park_dir, *thr;
    uint8_t *state, *hits;
    int32_t* tape;                 // null: no tape is kept
    int grid;
    hipStream_t st;
};
using ImageShadeFn = void (*)(const ImageShadeArgs& a, const void* shade_src);
int image_forward_from(drt_scene* s, const double* d_verts, const ImageCall& call, bool keep_tape, hipStream_t st, const char* who, ImageStartFn start,
                       const void* src, ImageShadeFn shade = nullptr, const void* shade_src = nullptr);
// image_forward's own start (k_image_start<ImageOneView> with the camera of the call, `src` = the ImageCall), for callers that bring a
// shade kernel only
void image_start_call(const ImageStartArgs& a, const void* src);

// One buffer of a workspace grown to n doubles (defined in drt_image.hip): never inside a stream capture (`what`, for the message).
int grow_doubles(double*& buf, int64_t& cap, int64_t n, hipStream_t st, const char* who, const char* what);

// The host array sigma[channels] of an absorbing entry point, after image_call_check (defined in drt_image_absorb.hip).
int absorb_sigma_check(const double* sigma, int channels, ImageSigma& out);

// The workspace of the loss calls behind drt_scene::image_loss_ws (drt_image_loss.hip; drt_image_views.hip shares the pixel seeds), and its
// growth to n_seed doubles of pixel seeds and n_cam doubles of camera-ray seeds (0: none wanted) -- never inside a stream capture.
struct ImageLossWs {
    int64_t cap = 0;               // doubles of g_c
    double* g_c = nullptr;         // [n_pix, C] of the band in flight
    int64_t seed_cap = 0;          // doubles of seeds
    double* seeds = nullptr;       // [2, n, 3] of the band in flight: the camera-ray seeds of drt_render_image_loss_camera
};
int ensure_image_loss_ws(drt_scene* s, int64_t n_seed, int64_t n_cam, hipStream_t st, const char* who);

constexpr int kImageLossBpc = 4;           // blocks per CU of the adjoint without the table (registers bound it: DESIGN.md 10.3)

// Defined in drt_image_screen.hip: k_image_screen_bwd on `st` over the pixels of the band, behind image_forward and the resolve kernel
// of the loss, whose pixel seeds g_c [n_pix, C] it reads.  d_grad_screen (nine accumulators: p0, eu, ev) and d_grad_texture
// ([tex_h, tex_w, C] accumulators, padded to a multiple of three values) are accumulated into; one of them may be null.
int launch_image_screen_bwd(const drt_scene* s, const ImageCall& call, const double* g_c, double* d_grad_screen, double* d_grad_texture, hipStream_t st);

// Defined in drt_image_env_param.hip: k_image_env_param_bwd on `st` over the pixels of the band, behind image_forward with
// the tape kept, the reflection pass (with `reflection`) and the resolve kernel of the environment loss, whose pixel seeds g_c it reads
// with the state bytes, the parked rows and the tape's row 0 as that kernel read them.  d_grad_env ([env_h, env_w, C] accumulators, padded
// to a multiple of three values) and d_grad_env_rot (nine accumulators, row-major) are accumulated into; one of them may be null.
int launch_image_env_param_bwd(const drt_scene* s, const PathCtx& pc, const ImageCall& call, const ImageScreenEnv& bg, bool reflection, const double* g_c,
                               double* d_grad_env, double* d_grad_env_rot, hipStream_t st);

// What a loss call hands out: the planes it compares against and the accumulators it adds into.  Only target and loss must be there.
struct ImageLossOut {
    const float *target, *weight;
    double *loss, *grad_verts, *grad_ior;
    float* image;
    int64_t* count;
    double* grad_sigma;            // ImageAbsorb only
};

// Defined in drt_image_camera.hip (drt_render_image_loss_camera).  launch_image_loss_bwd_camera: the adjoint launch of a
// loss call (image_loss_bwd_launch, drt_image_loss_bwd.h) with CAMERA on -- what image_loss_call hands image_loss_run in place of its own
// unit's launch --, which also stores the camera-ray seeds `seeds` [2, band.n, 3] float64 (g_o rows, then g_d rows, under the sample index).
// launch_image_camera_bwd: k_image_camera_bwd over the pixels of the band, behind the resolve kernel (g_c) and, on a scene with
// triangles, behind launch_image_loss_bwd_camera (seeds; not read on a scene without); d_grad_camera: 21 accumulators, kinv then rinv.
int launch_image_loss_bwd_camera(const drt_scene* s, const PathCtx& pc, const ImageCall& c, const ImageOneView& view, const ImageClear& pay, int grid,
                                 const int32_t* list, const unsigned* n_list, const double* g_c, const ImageLossOut& out, double* seeds, hipStream_t st);
int launch_image_camera_bwd(const drt_scene* s, const ImageCall& call, const double* g_c, const double* seeds, double* d_grad_camera, hipStream_t st);

// The N sums of a block of 256 threads into their accumulators grad[0 .. N) (whole block): a wave sum each, the four waves' sums added in
// LDS, then ONE atomic (pair) per block and accumulator.  LossAcc::flush's one atomic per wave was measured first
// (profiles/render_image_loss_screen.txt): accumulators that share a cache line are served one after the other -- with nine of them,
// 18 432 atomics of a launch, 0.2 ms of a pass that otherwise takes 0.1.  In either mode the sums are those LossAcc::flush would add:
// exact integers (DET), or float64 in a fixed order.
template <bool DET, int N>
__device__ __forceinline__ void block_flush(LossAcc<DET>* acc, double* grad) {
    constexpr int kWaves = 256 / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, k = threadIdx.x;
    if constexpr (DET) {
        __shared__ long long part_hi[kWaves][N];
        __shared__ unsigned long long part_lo[kWaves][N];
        __shared__ unsigned part_flags[kWaves][N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const FxAcc a = fx_wave_sum(acc[j].a);
            if (lane == 0) { part_hi[wave][j] = a.v.hi; part_lo[wave][j] = a.v.lo; part_flags[wave][j] = a.flags; }
        }
        __syncthreads();
        if (k < N) {
            Fx128 v{part_hi[0][k], part_lo[0][k]};
            unsigned flags = part_flags[0][k];
            for (int w = 1; w < kWaves; ++w) { v = fx_add(v, Fx128{part_hi[w][k], part_lo[w][k]}); flags |= part_flags[w][k]; }
            fx_atomic_add(reinterpret_cast<FxCell*>(grad) + k, v, flags);
        }
    } else {
        __shared__ double part[kWaves][N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const double v = wave_sum(acc[j].v);
            if (lane == 0) part[wave][j] = v;
        }
        __syncthreads();
        if (k < N) {
            double v = part[0][k];
            for (int w = 1; w < kWaves; ++w) v += part[w][k];
            if (v != 0.0) unsafeAtomicAdd(grad + k, v);
        }
    }
}

// The context image_forward traced with (the same for the adjoint of the loss).
inline PathCtx image_path_ctx(const drt_scene* s, const double* d_verts, const ImageCall& call) {
    PathCtx pc = path_ctx(s, d_verts, call.ior_int, call.ior_ext);
    pc.tc.slow_stack = static_cast<const PathsWs*>(s->paths_ws)->slow_stack;
    return pc;
}


// ---- the forward kernels of the family, each once

// All samples of the band: forms the sample ray (image_sample_ray) with the camera of the sample's row, top-box test; candidates -> list 0
// (index + float32 ray), their float64 ray and a throughput of 1 parked in the workspace; one state byte and one hit count per sample.
template <typename VIEW>
__global__ void __launch_bounds__(kPathBlock) k_image_start(const Node4Q* __restrict__ nodes, int n_tris, VIEW view, ImageBand band,
                                                             double* __restrict__ park_ori, double* __restrict__ park_dir, double* __restrict__ thr,
                                                             uint8_t* __restrict__ state, uint8_t* __restrict__ hits, RayList out, unsigned* count) {
    __shared__ StageMem stage;
    stage_init(stage);
    unsigned first, last;
    block_run(band.n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned i = base + threadIdx.x;
        bool cand = false;
        f3 o32{0.f, 0.f, 0.f}, d32{0.f, 0.f, 1.f};
        if (i < band.n) {
            state[i] = 0;
            hits[i] = 0;
            if (n_tris > 0) {
                int x, r, j;
                band_sample(band, i, x, r, j);
                const ImageViewAt v = view.at(r);
                d3 o, d;
                image_sample_ray(v.cam, band.s, x, v.y, j, o, d);
                o32 = to_f32(o); d32 = to_f32(d);
                cand = hits_top_boxes(nodes, o32, d32);
                if (cand) { store_d3(park_ori, i, o); store_d3(park_dir, i, d); thr[i] = 1.0; }
            }
        }
        stage_push(stage, cand, (int32_t)i, o32, d32, out, count);
    }
    stage_flush(stage, out, count);
}

// list k -> list k + 1, as k_paths_shade (drt_paths.hip); FRESNEL: a refracting interaction multiplies the sample's throughput by 1 - R;
// TAPE: the face of the interaction is written to tape[k, i] (without it `tape` is never touched and may be null); ImageAbsorb: the
// interior length pay.len[i], one more float64 per sample, stored at k = 0 and added to afterwards (no memset) -- o, d, T and n_refr
// have the clear form's bits.
template <bool SNELL, bool FRESNEL, bool TAPE, typename PAYLOAD>
__global__ void __launch_bounds__(kPathBlock) k_image_shade(PathCtx c, int64_t n_rays, int k, int max_bounces, bool reflect, RayList in,
                                                             const unsigned* __restrict__ n_in, RayList out, unsigned* n_out,
                                                             double* __restrict__ park_ori, double* __restrict__ park_dir, double* __restrict__ thr,
                                                             uint8_t* __restrict__ state, uint8_t* __restrict__ hits, int32_t* __restrict__ tape,
                                                             PAYLOAD pay) {
    __shared__ StageMem stage;
    stage_init(stage);
    const unsigned n = *n_in;
    const bool last_stage = k >= max_bounces;
    unsigned first, last;
    block_run(n, first, last);
    for (unsigned base = first; base < last; base += kPathBlock) {
        const unsigned e = base + threadIdx.x;
        bool go = false;
        int64_t i = 0;
        f3 o32{0.f, 0.f, 0.f}, d32{0.f, 0.f, 1.f};
        if (e < n) {
            i = in.idx[e];
            const int32_t f = in.face[e];
            if (i >= 0 && i < n_rays) {
                int n_refr = state[i];
                if (f < 0) {
                    if (path_exit_valid(n_refr)) state[i] = (uint8_t)n_refr | kPathDone;
                } else if (!last_stage) {
                    if constexpr (TAPE) tape[(int64_t)k * n_rays + i] = f;
                    hits[i] = (uint8_t)(k + 1);
                    d3 o = load_d3(park_ori, i), d = load_d3(park_dir, i);
                    double T = FRESNEL ? thr[i] : 1.0;
                    // (the length of a sample whose path dies here is stored too: nothing reads it)
                    go = image_interact<SNELL, FRESNEL>(c, f, reflect, o, d, n_refr, T, [&](const Bounce& b) {
                        if constexpr (PAYLOAD::kAbsorb) pay.len[i] = image_absorb_length(b, k == 0 ? 0.0 : pay.len[i]);
                    });
                    if (go) {
                        store_d3(park_ori, i, o); store_d3(park_dir, i, d);
                        if (FRESNEL) thr[i] = T;
                        state[i] = (uint8_t)n_refr;
                        o32 = to_f32(o); d32 = to_f32(d);
                    }
                }
            }
        }
        if (!last_stage) stage_push(stage, go, (int32_t)i, o32, d32, out, n_out);
    }
    if (!last_stage) stage_flush(stage, out, n_out);
}

// k_image_shade<., ., ., PAYLOAD> under (snell, fresnel, tape) from a table of the eight, launched as a shade hook of image_forward_from is to
template <typename PAYLOAD, int... I>
void image_shade_launch(const ImageShadeArgs& a, const PAYLOAD& pay, std::integer_sequence<int, I...>) {
    using Kernel = decltype(&k_image_shade<false, false, false, PAYLOAD>);
    static const Kernel kernels[] = {k_image_shade<(I & 4) != 0, (I & 2) != 0, (I & 1) != 0, PAYLOAD>...};
    kernels[(a.snell ? 4 : 0) | (a.fresnel ? 2 : 0) | (a.tape ? 1 : 0)]<<<a.grid, kPathBlock, 0, a.st>>>(
        a.pc, a.n_rays, a.k, a.max_bounces, a.reflect, a.in, a.n_in, a.out, a.n_out, a.park_ori, a.park_dir, a.thr, a.state, a.hits, a.tape, pay);
}
template <typename PAYLOAD>
void image_shade_launch(const ImageShadeArgs& a, const PAYLOAD& pay) { image_shade_launch(a, pay, std::make_integer_sequence<int, 8>{}); }

// The s x s contiguous samples of pixel `pix` = (x, y) of the band, in order: class, the camera ray formed again (direct) or the parked
// exit ray and throughput (through), colour; sum[0 .. tx.c) is the ordered float64 sum of the colours, n_hit / n_through count the
// samples that met the mesh / completed their path.  ImageAbsorb: the colours are attenuated along the interior length, and `more`
// receives the ordered sums the sigma partials and the length plane need.  (The channel loop and the count of the through samples are
// spelt per payload, here and in k_image_loss_resolve: under the clear spelling the absorbing kernels keep their per-channel arrays in
// LDS, 8 to 18 KiB a block, instead of registers -- profiles/image_family_resources.txt.)
template <typename PAYLOAD, typename BACKGROUND = ImageScreenOnly>
__device__ __forceinline__ void image_pixel_walk(const ImageCam& cam, const ImageBand& band, int64_t pix, int x, int y, const ImageScreen& sc, const ImageTex& tx,
                                                 const ImageFill& fill, bool fresnel, const PAYLOAD& pay, const double* __restrict__ park_ori,
                                                 const double* __restrict__ park_dir, const double* __restrict__ thr,
                                                 const uint8_t* __restrict__ state, const uint8_t* __restrict__ hits, double* sum,
                                                 typename PAYLOAD::Sums& more, int& n_hit, int& n_through, const BACKGROUND& bg = BACKGROUND{},
                                                 int* n_reflect = nullptr) {
    const int s2 = band.s * band.s;
    n_hit = 0; n_through = 0;
    if constexpr (PAYLOAD::kAbsorb) more.l_sum = 0.0;
    for (int j = 0; j < s2; ++j) {
        const int64_t i = pix * s2 + j;
        const bool was_hit = hits[i] != 0, done = (state[i] & kPathDone) != 0;
        const int cls = image_class(was_hit, done);
        n_hit += was_hit ? 1 : 0;
        if constexpr (!PAYLOAD::kAbsorb) n_through += cls == kImageThrough ? 1 : 0;
        d3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 1.0};
        double T = 1.0;
        [[maybe_unused]] double L = 0.0;
        if (cls == kImageDirect) {
            image_sample_ray(cam, band.s, x, y, j, o, d);
        } else if (cls == kImageThrough) {
            o = load_d3(park_ori, i); d = load_d3(park_dir, i);
            if (fresnel) T = thr[i];
            if constexpr (PAYLOAD::kAbsorb) {
                L = pay.len[i];
                more.l_sum = n_through == 0 ? L : more.l_sum + L;
                ++n_through;
            }
        }
        double c[kImageMaxChannels];
        if constexpr (PAYLOAD::kAbsorb) {
            if constexpr (BACKGROUND::kEnv) {
                // Absorbing glass in a room: the environment is attenuated like the texture.  lc takes the transmitted
                // colour BEFORE the reflection is added into c: that light never entered the object and carries no sigma partial.
                const bool lit = image_env_sample_colour<true>(sc, tx, bg.screen, bg.env, cls, o, d, T, fill.c_invalid, c, L, pay.sigma.v) != kImageBgFill;
#pragma unroll
                for (int ch = 0; ch < kImageMaxChannels; ++ch) {
                    if (ch >= tx.c) continue;
                    if (lit && cls == kImageThrough) more.lc[ch] = more.lc[ch] + L * c[ch];
                }
                if constexpr (BACKGROUND::kReflect) {
                    if (cls == kImageThrough && (state[i] & kImageReflectSeen)) {
                        d3 co, cd, ro, wr;
                        double R1;
                        image_sample_ray(cam, band.s, x, y, j, co, cd);
                        const bool seen = bg.snell ? image_reflect_first<true>(bg.pc, bg.first_face[i], co, cd, ro, wr, R1)
                                                   : image_reflect_first<false>(bg.pc, bg.first_face[i], co, cd, ro, wr, R1);
                        if (seen) {
                            image_env_add_reflection(sc, tx, bg.screen, bg.env, ro, wr, R1, c);
                            if (n_reflect) ++*n_reflect;
                        }
                    }
                }
#pragma unroll
                for (int ch = 0; ch < kImageMaxChannels; ++ch) {
                    if (ch >= tx.c) continue;
                    sum[ch] = j == 0 ? c[ch] : sum[ch] + c[ch];
                }
            } else {
                const bool lit = image_sample_colour<true>(sc, tx, cls, o, d, T, fill.c_void, fill.c_invalid, c, L, pay.sigma.v);
#pragma unroll
                for (int ch = 0; ch < kImageMaxChannels; ++ch) {
                    if (ch >= tx.c) continue;
                    sum[ch] = j == 0 ? c[ch] : sum[ch] + c[ch];
                    if (lit && cls == kImageThrough) more.lc[ch] = more.lc[ch] + L * c[ch];
                }
            }
        } else {
            if constexpr (BACKGROUND::kEnv) {
                image_env_sample_colour(sc, tx, bg.screen, bg.env, cls, o, d, T, fill.c_invalid, c);
                if constexpr (BACKGROUND::kReflect) {
                    if (cls == kImageThrough && (state[i] & kImageReflectSeen)) {
                        d3 co, cd, ro, wr;
                        double R1;
                        image_sample_ray(cam, band.s, x, y, j, co, cd);
                        const bool seen = bg.snell ? image_reflect_first<true>(bg.pc, bg.first_face[i], co, cd, ro, wr, R1)
                                                   : image_reflect_first<false>(bg.pc, bg.first_face[i], co, cd, ro, wr, R1);
                        if (seen) {
                            image_env_add_reflection(sc, tx, bg.screen, bg.env, ro, wr, R1, c);
                            if (n_reflect) ++*n_reflect;
                        }
                    }
                }
            } else image_sample_colour(sc, tx, cls, o, d, T, fill.c_void, fill.c_invalid, c);
            for (int ch = 0; ch < tx.c; ++ch) sum[ch] = j == 0 ? c[ch] : sum[ch] + c[ch];
        }
    }
}

// One thread per pixel of the band: the mean of its samples' colours.  hit / through may be null; so may `length` (ImageAbsorb only: the
// mean of L over the pixel's through samples).
template <typename PAYLOAD, typename BACKGROUND = ImageScreenOnly>
__global__ void __launch_bounds__(kPathBlock) k_image_resolve(ImageCam cam, ImageBand band, int64_t n_pix, ImageScreen sc, ImageTex tx, ImageFill fill, bool fresnel,
                                                               PAYLOAD pay, const double* __restrict__ park_ori, const double* __restrict__ park_dir,
                                                               const double* __restrict__ thr, const uint8_t* __restrict__ state,
                                                               const uint8_t* __restrict__ hits, float* __restrict__ image, float* __restrict__ hit,
                                                               float* __restrict__ through, float* __restrict__ length, BACKGROUND bg = BACKGROUND{}) {
    static_assert(!(PAYLOAD::kAbsorb && BACKGROUND::kEnv), "one view: an environment goes with clear glass only");
    const int64_t pix = (int64_t)blockIdx.x * kPathBlock + threadIdx.x;
    if (pix >= n_pix) return;
    const int s2 = band.s * band.s;
    const int y = band.y0 + (int)(pix / band.width), x = (int)(pix % band.width);
    double acc[kImageMaxChannels] = {0.0, 0.0, 0.0};
    typename PAYLOAD::Sums more;
    int n_hit, n_through;
    [[maybe_unused]] int n_reflect = 0;
    image_pixel_walk(cam, band, pix, x, y, sc, tx, fill, fresnel, pay, park_ori, park_dir, thr, state, hits, acc, more, n_hit, n_through, bg, &n_reflect);
    const int64_t row = (int64_t)y * band.width + x;
    if constexpr (BACKGROUND::kEnv) {
        if constexpr (BACKGROUND::kReflect) {
            if (bg.reflect) bg.reflect[row] = (float)((double)n_reflect / (double)s2);
        }
    }
    for (int ch = 0; ch < tx.c; ++ch) image[row * tx.c + ch] = (float)(acc[ch] / (double)s2);
    if (hit) hit[row] = (float)((double)n_hit / (double)s2);
    if (through) through[row] = (float)((double)n_through / (double)s2);
    if constexpr (PAYLOAD::kAbsorb) {
        if (length) length[row] = n_through ? (float)(more.l_sum / (double)n_through) : 0.f;
    }
}
