// tests/hostsim/image_env.cpp -- drt_amd/csrc/drt_image_env.h compiled for the host (g++ -ffp-contract=off): the environment lookup, its
// cell and bilinear fetch, a sample's colour in front of a screen and an environment and the outer-surface reflection, run over arrays
// in plain loops.  Test-only.
#include "../../drt_amd/csrc/drt_image_env.h"

using namespace drt;

namespace {
ImageEnv env_of(const float* texel, int eh, int ew, int c, const double* R9) {
    ImageEnv e{texel, eh, ew, c, {}};
    memcpy(e.rot, R9, sizeof(double) * 9);
    return e;
}
// The loss of one view in front of an environment with its adjoint (Fresnel on), as tests/hostsim/image_loss.cpp runs the clear law: classes,
// tape and occlusion verdicts are handed in; a through sample's exit ray and throughput are recomputed from its tape with image_interact,
// its colour is image_env_sample_colour (+ image_env_add_reflection where its reflection was seen), its adjoint image_env_sample_backward
// (+ image_reflect_backward) -- what k_image_loss_bwd<.., ImageScreenEnv> and k_image_reflect_bwd run.
template <bool SNELL>
double env_view(const ImageCam& cam, int H, int W, int s, const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& env, const PathCtx& c,
                const int32_t* cls, const int32_t* tape, const uint8_t* hits, const uint8_t* seen, bool reflection, const double* fill_invalid,
                const float* target, const float* weight, double* grad_verts, double* g_ior, int64_t* count, float* image) {
    const int s2 = s * s;
    const int64_t n = (int64_t)H * W * s2;
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    double loss = 0.0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const int64_t pix = (int64_t)y * W + x;
            d3 eo[kImageMaxSuper * kImageMaxSuper], ed[kImageMaxSuper * kImageMaxSuper];
            double eT[kImageMaxSuper * kImageMaxSuper];
            double acc[kImageMaxChannels] = {0.0, 0.0, 0.0};
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                d3 o, d, co, cd;
                image_sample_ray(cam, s, x, y, j, o, d);
                co = o; cd = d;
                double T = 1.0;
                if (cls[i] == kImageThrough) {
                    int n_refr = 0;
                    for (int k = 0; k < (int)hits[i]; ++k) image_interact<SNELL, true>(c, tape[(int64_t)k * n + i], true, o, d, n_refr, T);
                }
                eo[j] = o; ed[j] = d; eT[j] = T;
                double col[kImageMaxChannels];
                image_env_sample_colour(sc, tx, has_screen, env, cls[i], o, d, T, fill_invalid, col);
                if (reflection && cls[i] == kImageThrough && seen[i]) {
                    d3 ro, wr;
                    double R1;
                    if (image_reflect_first<SNELL>(c, tape[i], co, cd, ro, wr, R1)) image_env_add_reflection(sc, tx, has_screen, env, ro, wr, R1, col);
                }
                for (int ch = 0; ch < tx.c; ++ch) acc[ch] = j == 0 ? col[ch] : acc[ch] + col[ch];
            }
            double mean[kImageMaxChannels], g_c[kImageMaxChannels];
            for (int ch = 0; ch < tx.c; ++ch) {
                mean[ch] = acc[ch] / (double)s2;
                if (image) image[pix * tx.c + ch] = (float)mean[ch];
            }
            loss += image_loss_pixel(mean, tx.c, s2, target + pix * tx.c, weight ? (double)weight[pix] : 1.0, g_c);
            for (int j = 0; j < s2; ++j) {
                const int64_t i = pix * s2 + j;
                if (cls[i] != kImageThrough) continue;
                d3 o, d;
                image_sample_ray(cam, s, x, y, j, o, d);
                double gi, ge;
                if (image_env_sample_backward<SNELL, true>(c, o, d, tape + i, n, (int)hits[i], eo[j], ed[j], eT[j], sc, tx, has_screen, env, g_c, add, gi, ge)) {
                    g_ior[0] += gi; g_ior[1] += ge;
                    ++*count;
                }
                if (reflection && seen[i] && image_reflect_backward<SNELL>(c, tape[i], o, d, sc, tx, has_screen, env, g_c, add, gi, ge)) {
                    g_ior[0] += gi; g_ior[1] += ge;
                }
            }
        }
    return loss;
}
}  // namespace

extern "C" {

int env_rot_ok(const double* R9) { return image_env_rot_ok(R9) ? 1 : 0; }

// uv float64 [n, 2], ey float64 [n]
void env_uv(const double* R9, int eh, int ew, const double* d, int64_t n, double* uv, double* ey) {
    const ImageEnv e = env_of(nullptr, eh, ew, 1, R9);
    for (int64_t i = 0; i < n; ++i) ey[i] = image_env_uv(e, load_d3(d, i), uv[2 * i], uv[2 * i + 1]);
}

// the bilinear fetch at GIVEN (u, v): out float64 [n, c]; cell int32 [n, 3] = xa, xb, y0
void env_fetch(const float* texel, int eh, int ew, int c, const double* uv, int64_t n, double* out, int32_t* cell) {
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const ImageEnv e = env_of(texel, eh, ew, c, eye);
    for (int64_t i = 0; i < n; ++i) {
        const ImageEnvCell k = image_env_cell(e, uv[2 * i], uv[2 * i + 1]);
        cell[3 * i] = k.xa; cell[3 * i + 1] = k.xb; cell[3 * i + 2] = k.y0;
        for (int ch = 0; ch < c; ++ch) out[i * c + ch] = image_env_bilinear(e, k, ch);
    }
}

// per sample: cls int32, exit ray, throughput -> colour float64 [n, c], src int32 [n] (0 fill, 1 screen, 2 environment); s9 / tex null: no screen
void env_colours(const double* s9, const float* tex, int th, int tw, int c, const float* texel, int eh, int ew, const double* R9, const int32_t* cls,
                 const double* o, const double* d, const double* T, int64_t n, const double* fill_invalid, double* colour, int32_t* src) {
    const bool has_screen = s9 != nullptr;
    ImageScreen sc{d3{0, 0, 0}, d3{1, 0, 0}, d3{0, 1, 0}};
    if (has_screen) sc = ImageScreen{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}};
    const ImageTex tx{has_screen ? tex : nullptr, has_screen ? th : 2, has_screen ? tw : 2, c};
    const ImageEnv e = env_of(texel, eh, ew, c, R9);
    for (int64_t i = 0; i < n; ++i)
        src[i] = image_env_sample_colour(sc, tx, has_screen, e, cls[i], load_d3(o, i), load_d3(d, i), T[i], fill_invalid, colour + i * c);
}

// d (sum_ch g_c[ch] E(d)[ch]) / d d: g_d float64 [n, 3]
void env_lookup_backward(const float* texel, int eh, int ew, int c, const double* R9, const double* d, const double* g_c, int64_t n, double* g_d) {
    const ImageEnv e = env_of(texel, eh, ew, c, R9);
    for (int64_t i = 0; i < n; ++i) {
        double u, v;
        image_env_uv(e, load_d3(d, i), u, v);
        const ImageEnvCell k = image_env_cell(e, u, v);
        double s_x = 0.0, s_y = 0.0;
        for (int ch = 0; ch < c; ++ch) {
            double bx, by;
            image_env_bilinear_grad(e, k, ch, bx, by);
            s_x = ch == 0 ? g_c[i * c + ch] * bx : s_x + g_c[i * c + ch] * bx;
            s_y = ch == 0 ? g_c[i * c + ch] * by : s_y + g_c[i * c + ch] * by;
        }
        d3 g;
        image_env_uv_backward(e, load_d3(d, i), s_x, k.v_inside ? s_y : 0.0, g);
        store_d3(g_d, i, g);
    }
}

// image_sample_colour, the clear function, on the same arguments (fill_void where the screen does not catch the ray)
void env_clear_colours(const double* s9, const float* tex, int th, int tw, int c, const int32_t* cls, const double* o, const double* d, const double* T,
                       int64_t n, const double* fill_void, const double* fill_invalid, double* colour) {
    const ImageScreen sc{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}};
    const ImageTex tx{tex, th, tw, c};
    for (int64_t i = 0; i < n; ++i) image_sample_colour(sc, tx, cls[i], load_d3(o, i), load_d3(d, i), T[i], fill_void, fill_invalid, colour + i * c);
}

// The outer-surface reflection of every sample of an H x W image at supersampling s whose first face is first_face[i] (< 0: none):
// qual uint8 [n], ro / wr float64 [n, 3], R1 float64 [n] (written where qual)
void env_reflect(const int32_t* faces, const double* verts, int n_tris, const double* cam21, int H, int W, int s, double ior_ext, double ior_int, int snell,
                 const int32_t* first_face, uint8_t* qual, double* ro, double* wr, double* R1) {
    PathCtx c{};
    c.tc.n_tris = n_tris; c.faces = faces; c.verts = verts; c.ior_int = ior_int; c.ior_ext = ior_ext;
    ImageCam cam;
    memcpy(cam.kinv, cam21, sizeof(double) * 9);
    memcpy(cam.rinv, cam21 + 9, sizeof(double) * 12);
    int64_t i = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int j = 0; j < s * s; ++j, ++i) {
                d3 o, d, a, b;
                double r = 0.0;
                image_sample_ray(cam, s, x, y, j, o, d);
                qual[i] = snell ? image_reflect_first<true>(c, first_face[i], o, d, a, b, r) : image_reflect_first<false>(c, first_face[i], o, d, a, b, r);
                if (qual[i]) { store_d3(ro, i, a); store_d3(wr, i, b); R1[i] = r; }
            }
}

// c[n, ch] += R1 * B(ro, wr) on the rows with add[i] != 0
void env_add_reflection(const double* s9, const float* tex, int th, int tw, int ch, const float* texel, int eh, int ew, const double* R9, const uint8_t* add,
                        const double* ro, const double* wr, const double* R1, int64_t n, double* colour) {
    const bool has_screen = s9 != nullptr;
    ImageScreen sc{d3{0, 0, 0}, d3{1, 0, 0}, d3{0, 1, 0}};
    if (has_screen) sc = ImageScreen{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}};
    const ImageTex tx{has_screen ? tex : nullptr, has_screen ? th : 2, has_screen ? tw : 2, ch};
    const ImageEnv e = env_of(texel, eh, ew, ch, R9);
    for (int64_t i = 0; i < n; ++i)
        if (add[i]) image_env_add_reflection(sc, tx, has_screen, e, load_d3(ro, i), load_d3(wr, i), R1[i], colour + i * ch);
}

// The loss of one view (returned) with its adjoint: grad_verts [V, 3], g_ior [2] (ior_int, ior_ext) and *count (through samples) are added
// into, image float32 [H, W, C] (may be null) is written.  s9 / tex null: no screen.  cls int32 [n], tape int32 [K, n], hits / seen uint8 [n].
double env_loss_view(const double* cam21, int H, int W, int s, const double* s9, const float* tex, int th, int tw, int ch, const float* texel, int eh, int ew,
                     const double* R9, const int32_t* faces, const double* verts, int n_tris, double ior_int, double ior_ext, int snell, int reflection,
                     const int32_t* cls, const int32_t* tape, const uint8_t* hits, const uint8_t* seen, const double* fill_invalid, const float* target,
                     const float* weight, double* grad_verts, double* g_ior, int64_t* count, float* image) {
    ImageCam cam;
    memcpy(cam.kinv, cam21, sizeof(double) * 9);
    memcpy(cam.rinv, cam21 + 9, sizeof(double) * 12);
    const bool has_screen = s9 != nullptr;
    ImageScreen sc{d3{0, 0, 0}, d3{1, 0, 0}, d3{0, 1, 0}};
    if (has_screen) sc = ImageScreen{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}};
    const ImageTex tx{has_screen ? tex : nullptr, has_screen ? th : 2, has_screen ? tw : 2, ch};
    const ImageEnv e = env_of(texel, eh, ew, ch, R9);
    const PathCtx c{TraceCtx{nullptr, nullptr, n_tris, nullptr}, faces, verts, ior_int, ior_ext};
    if (snell) return env_view<true>(cam, H, W, s, sc, tx, has_screen, e, c, cls, tape, hits, seen, reflection != 0, fill_invalid, target, weight, grad_verts, g_ior, count, image);
    return env_view<false>(cam, H, W, s, sc, tx, has_screen, e, c, cls, tape, hits, seen, reflection != 0, fill_invalid, target, weight, grad_verts, g_ior, count, image);
}

}  // extern "C"
