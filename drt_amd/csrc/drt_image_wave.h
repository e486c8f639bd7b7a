// drt_image_wave.h -- what the two calls on the refracted image share (drt_image.hip: drt_render_image; drt_image_loss.hip:
// drt_render_image_loss): the band of rows of one call, the checked call, the forward wavefront (defined in drt_image.hip, as
// launch_trace_list is in drt_trace.hip) and the walk over the samples of a pixel that both resolve kernels make.
#pragma once
#include "drt_device.h"
#include "drt_pathws.h"
#include "drt_image.h"

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

// image_forward with the start kernel of the caller's choice (drt_image_views.hip: the samples of several views in one band): `start`
// launches on a.st, with a.grid blocks of kPathBlock threads, a kernel that does for every sample of the band what k_image_start does;
// `src` is handed through to it.  image_forward is this with k_image_start and the camera of the call.
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
// ... and with the shade kernel of the caller's choice (drt_image_absorb.hip: k_image_shade plus the interior length): `shade` launches on
// a.st, with a.grid blocks of kPathBlock threads, a kernel that does for list k what k_image_shade<snell, fresnel, tape != null> does;
// `shade_src` is handed through to it.  Null, the default: k_image_shade from drt_image.hip's own table, what every call launched before.
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
// image_forward's own start (k_image_start with the camera of the call, `src` = the ImageCall), for callers that bring a shade kernel only
void image_start_call(const ImageStartArgs& a, const void* src);

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

// Defined in drt_image_camera.hip (drt_render_image_loss_camera).  launch_image_loss_bwd_camera: k_image_loss_bwd with
// CAMERA on -- what image_loss_call launches over the list of through samples, which here also stores the camera-ray seeds
// `seeds` [2, band.n, 3] float64 (g_o rows, then g_d rows, under the sample index); d_grad_verts, d_grad_ior and d_count may be null.
// launch_image_camera_bwd: k_image_camera_bwd over the pixels of the band, behind the resolve kernel (g_c) and, on a scene with
// triangles, behind launch_image_loss_bwd_camera (seeds; not read on a scene without); d_grad_camera: 21 accumulators, kinv then rinv.
int launch_image_loss_bwd_camera(const drt_scene* s, const PathCtx& pc, const ImageCall& call, int grid, const int32_t* list, const unsigned* n_list,
                                 const double* g_c, double* d_grad_verts, double* d_grad_ior, unsigned long long* d_count, double* seeds, hipStream_t st);
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

// The s x s contiguous samples of pixel `pix` = (x, y) of the band, in order: class, the camera ray formed again (direct) or the parked
// exit ray and throughput (through), colour; sum[0 .. tx.c) is the ordered float64 sum of the colours, n_hit / n_through count the
// samples that met the mesh / completed their path.
__device__ __forceinline__ void image_pixel_walk(const ImageCam& cam, const ImageBand& band, int64_t pix, int x, int y, const ImageScreen& sc, const ImageTex& tx,
                                                 const ImageFill& fill, bool fresnel, const double* __restrict__ park_ori,
                                                 const double* __restrict__ park_dir, const double* __restrict__ thr,
                                                 const uint8_t* __restrict__ state, const uint8_t* __restrict__ hits, double* sum, int& n_hit,
                                                 int& n_through) {
    const int s2 = band.s * band.s;
    n_hit = 0; n_through = 0;
    for (int j = 0; j < s2; ++j) {
        const int64_t i = pix * s2 + j;
        const bool was_hit = hits[i] != 0, done = (state[i] & kPathDone) != 0;
        const int cls = image_class(was_hit, done);
        n_hit += was_hit ? 1 : 0;
        n_through += cls == kImageThrough ? 1 : 0;
        d3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 1.0};
        double T = 1.0;
        if (cls == kImageDirect) {
            image_sample_ray(cam, band.s, x, y, j, o, d);
        } else if (cls == kImageThrough) {
            o = load_d3(park_ori, i); d = load_d3(park_dir, i);
            if (fresnel) T = thr[i];
        }
        double c[kImageMaxChannels];
        image_sample_colour(sc, tx, cls, o, d, T, fill.c_void, fill.c_invalid, c);
        for (int ch = 0; ch < tx.c; ++ch) sum[ch] = j == 0 ? c[ch] : sum[ch] + c[ch];
    }
}
