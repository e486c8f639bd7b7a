// drt_image_env.h -- an environment map at infinity behind (or instead of) the screen of the refracted image (DESIGN.md section 10.8;
// Scene.render_image with `environment`, drt_render_image_env).  Every other forward quantity is drt_image.h's, unchanged.
//   env      float32 [Eh, Ew, C], Eh, Ew >= 2, lat-long: row 0 looks up (+y of the environment frame), the columns run once around
//   env_R    float64 3 x 3 row-major, world -> environment frame, y up; max |R R^T - I| <= 1e-12
//   e_r      = (R[r][0] d.x + R[r][1] d.y) + R[r][2] d.z
//   theta    = acos(clamp(e_y, -1, 1)),  phi = atan2(e_x, -e_z)
//   u        = ((phi / (2 pi)) + 0.5) Ew - 0.5,  v = (theta / pi) Eh - 0.5          (texel centres at the integers, as on the screen)
//   cell     v clamped to [0, Eh - 1], y0 = min(floor(v), Eh - 2); x0 = floor(u) in -1 .. Ew - 1, columns (x0 + Ew) mod Ew and
//            (x0 + 1) mod Ew (the map closes around the seam); fx = u - x0, fy = v - y0, and image_bilinear's formula
//   colour   of a direct or through sample with exit ray (o, d): T * texture where a screen is given and image_screen_uv puts the ray on it,
//            otherwise T * E(d) -- the environment is weighted like the texture and depends on d alone; an invalid sample keeps its
//            unweighted fill.  With an environment no sample receives `void`.
//   reflect  (opt-in, with the Fresnel term) a sample whose FIRST interaction has sg > 0 and no TIR flag reflects off the outer surface:
//            (ro, wr) = bounce_reflect of that Bounce, R1 = fresnel_R(ci, ior_ext, ior_int), the value whose complement entered T.  One
//            any-hit query of the float32 cast of (ro, wr) under the tracer contract; where it finds nothing and the sample is THROUGH,
//            c[ch] = T B(exit)[ch] + R1 B(ro, wr)[ch], B the background above (screen, else environment).  An occluded reflection, the
//            reflection of an invalid sample and reflections off inner surfaces contribute nothing: stated losses, as 10.2 states its own.
// Plain C++ like drt_image.h: float64, one rounding per operation in the association written (tests/hostsim/image_env.cpp runs these
// bodies on the host against tests/image_env_ref.py).  acos and atan2 are the two calls of the law that are not correctly rounded: u and v
// carry the math library's error (DESIGN.md 10.8 has the bound), everything else is exact against the restatement.
// The adjoint (the loss is drt_image_loss.h's, unchanged) follows torch's conventions: a clamp passes the gradient inside
// its closed bounds; floor, the cell, the wrap column, the occlusion verdict, classes and faces carry none.  An exit ray that goes to the
// environment has the seed g_o = 0 and g_d from image_env_uv_backward; the reflection hands its seeds through bounce_reflect_backward
// (ro, wr), fresnel_R_backward and bounce_ci_backward (R1) into the three vertices of the first face and both IORs.
#pragma once
#include "drt_image_loss.h"

namespace drt {

struct ImageEnv {
    const float* texel;     // float32 [eh, ew, c]
    int eh, ew, c;          // eh, ew >= 2; c in {1, 3}
    double rot[9];          // world -> environment frame, row-major
};

constexpr double kImageEnvPi = 3.141592653589793;         // the double nearest pi; 2 pi below is its exact double
constexpr double kImageEnvRotTol = 1e-12;

// max |R R^T - I| <= 1e-12 (NaN fails)
DRT_HD bool image_env_rot_ok(const double* R) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double g = ((R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2]) - (i == j ? 1.0 : 0.0);
            if (!((g < 0.0 ? -g : g) <= kImageEnvRotTol)) return false;
        }
    return true;
}

// d in the environment frame
DRT_HD d3 image_env_dir(const ImageEnv& e, d3 d) {
    const double* R = e.rot;
    return d3{(R[0] * d.x + R[1] * d.y) + R[2] * d.z, (R[3] * d.x + R[4] * d.y) + R[5] * d.z, (R[6] * d.x + R[7] * d.y) + R[8] * d.z};
}

// (u, v) of a direction, in texel units, before the clamp of v; returns e_y (what the pole test of the tests reads)
DRT_HD double image_env_uv(const ImageEnv& e, d3 d, double& u, double& v) {
    const d3 q = image_env_dir(e, d);
    const double cy = q.y < -1.0 ? -1.0 : (q.y > 1.0 ? 1.0 : q.y);
    const double theta = acos(cy);
    const double phi = atan2(q.x, -q.z);
    u = ((phi / (2.0 * kImageEnvPi)) + 0.5) * (double)e.ew - 0.5;
    v = (theta / kImageEnvPi) * (double)e.eh - 0.5;
    return q.y;
}

// The cell of (u, v): two columns (wrapped), the upper row, the weights.  Every read of the four texels is inside the map for ANY u, v
// (a NaN lands in column -1 / row 0 with NaN weights: a NaN colour, no stray read).
struct ImageEnvCell {
    int xa, xb, y0;
    double fx, fy;
    bool v_inside;          // v was inside its clamp's closed bounds (the gradient passes)
};
DRT_HD ImageEnvCell image_env_cell(const ImageEnv& e, double u, double v) {
    ImageEnvCell c;
    c.v_inside = v >= 0.0 && v <= (double)(e.eh - 1);
    double vc = v;
    if (!(vc >= 0.0)) vc = 0.0;
    if (vc > (double)(e.eh - 1)) vc = (double)(e.eh - 1);
    double y0 = floor(vc);
    if (y0 > (double)(e.eh - 2)) y0 = (double)(e.eh - 2);
    double x0 = floor(u);
    if (!(x0 >= -1.0)) x0 = -1.0;
    if (x0 > (double)(e.ew - 1)) x0 = (double)(e.ew - 1);
    c.fx = u - x0; c.fy = vc - y0;
    c.y0 = (int)y0;
    c.xa = ((int)x0 + e.ew) % e.ew;
    c.xb = ((int)x0 + 1) % e.ew;
    return c;
}

// Bilinear sample of channel ch in a cell, image_bilinear's formula.
DRT_HD double image_env_bilinear(const ImageEnv& e, const ImageEnvCell& c, int ch) {
    const float* up = e.texel + (int64_t)c.y0 * e.ew * e.c + ch;
    const float* down = up + (int64_t)e.ew * e.c;
    const double t00 = (double)up[(int64_t)c.xa * e.c], t01 = (double)up[(int64_t)c.xb * e.c];
    const double t10 = (double)down[(int64_t)c.xa * e.c], t11 = (double)down[(int64_t)c.xb * e.c];
    return ((t00 * (1.0 - c.fx) + t01 * c.fx) * (1.0 - c.fy)) + ((t10 * (1.0 - c.fx) + t11 * c.fx) * c.fy);
}

// ... and its derivatives w.r.t. fx and fy, as image_bilinear_grad has them (d / du = d / dfx; d / dv = d / dfy inside the clamp of v).
DRT_HD double image_env_bilinear_grad(const ImageEnv& e, const ImageEnvCell& c, int ch, double& dE_dfx, double& dE_dfy) {
    const float* up = e.texel + (int64_t)c.y0 * e.ew * e.c + ch;
    const float* down = up + (int64_t)e.ew * e.c;
    const double t00 = (double)up[(int64_t)c.xa * e.c], t01 = (double)up[(int64_t)c.xb * e.c];
    const double t10 = (double)down[(int64_t)c.xa * e.c], t11 = (double)down[(int64_t)c.xb * e.c];
    dE_dfx = ((t01 - t00) * (1.0 - c.fy)) + ((t11 - t10) * c.fy);
    dE_dfy = (t10 * (1.0 - c.fx) + t11 * c.fx) - (t00 * (1.0 - c.fx) + t01 * c.fx);
    return ((t00 * (1.0 - c.fx) + t01 * c.fx) * (1.0 - c.fy)) + ((t10 * (1.0 - c.fx) + t11 * c.fx) * c.fy);
}

// E(d)[ch]
DRT_HD double image_env_lookup(const ImageEnv& e, d3 d, int ch) {
    double u, v;
    image_env_uv(e, d, u, v);
    return image_env_bilinear(e, image_env_cell(e, u, v), ch);
}

// Adjoint of image_env_uv for the incoming (g_u, g_v; g_v already zeroed by the caller where v left its clamp): g_d is SET.
//   u = ((phi / 2pi) + 0.5) Ew - 0.5 ; phi = atan2(a, b), a = e_x, b = -e_z : d phi = (b da - a db) / (a^2 + b^2)
//   v = (theta / pi) Eh - 0.5 ; theta = acos(cy) : d theta = -d cy / sqrt(1 - cy^2), cy = clamp(e_y, -1, 1)
// At a pole (a = b = 0, or |cy| = 1) the quotients are those torch forms: inf or NaN; the tests keep such samples out (pole cut).
// image_env_uv_seed: the seed g_e of the direction q in the ENVIRONMENT frame, which the rotation's own gradient starts from as well
// (drt_image_env_param.h: g_R[r][c] = g_e[r] d[c]); image_env_uv_backward multiplies it by R^T.
DRT_HD d3 image_env_uv_seed(const ImageEnv& e, d3 q, double g_u, double g_v) {
    const double cy = q.y < -1.0 ? -1.0 : (q.y > 1.0 ? 1.0 : q.y);
    const double g_phi = (g_u * (double)e.ew) / (2.0 * kImageEnvPi);
    const double g_theta = (g_v * (double)e.eh) / kImageEnvPi;
    const double a = q.x, b = -q.z;
    const double r2 = a * a + b * b;
    const double g_a = g_phi * (b / r2), g_b = g_phi * (-a / r2);
    const double g_cy = -g_theta / sqrt(1.0 - cy * cy);
    const double g_qy = (q.y >= -1.0 && q.y <= 1.0) ? g_cy : 0.0;
    return d3{g_a, g_qy, -g_b};
}
DRT_HD void image_env_uv_backward(const ImageEnv& e, d3 d, double g_u, double g_v, d3& g_d) {
    const d3 g_q = image_env_uv_seed(e, image_env_dir(e, d), g_u, g_v);
    const double* R = e.rot;
    g_d = d3{(R[0] * g_q.x + R[3] * g_q.y) + R[6] * g_q.z, (R[1] * g_q.x + R[4] * g_q.y) + R[7] * g_q.z, (R[2] * g_q.x + R[5] * g_q.y) + R[8] * g_q.z};
}

enum : int { kImageBgFill = 0, kImageBgScreen = 1, kImageBgEnv = 2 };

// Colour of one sample in front of a screen (has_screen) and an environment: image_sample_colour with the environment in the place of
// `void`.  tx.c is the channel count (without a screen tx holds nothing else).  Returns where the colour came from.  acos / atan2 are
// evaluated for the samples that go to the environment and for no other.  ABSORB (absorbing glass in a room):
// (A_ch * T) times the background, A_ch = exp(-(sigma_ch * L)) -- the environment is attenuated exactly like the texture, in
// image_sample_colour<true>'s association and with its fixed trip count.
template <bool ABSORB = false>
DRT_HD int image_env_sample_colour(const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& env, int cls, d3 o, d3 d, double T,
                                   const double* fill_invalid, double* c, double L = 0.0, const double* sigma = nullptr) {
    if (cls == kImageInvalid) {
        for (int ch = 0; ch < tx.c; ++ch) c[ch] = fill_invalid[ch];
        return kImageBgFill;
    }
    double u, v;
    if (has_screen && image_screen_uv(sc, tx.th, tx.tw, o, d, u, v)) {
        if constexpr (ABSORB) {
            for (int ch = 0; ch < kImageMaxChannels; ++ch)
                if (ch < tx.c) c[ch] = (image_absorb_factor(sigma[ch], L) * T) * image_bilinear(tx, u, v, ch);
        } else {
            for (int ch = 0; ch < tx.c; ++ch) c[ch] = T * image_bilinear(tx, u, v, ch);
        }
        return kImageBgScreen;
    }
    image_env_uv(env, d, u, v);
    const ImageEnvCell cell = image_env_cell(env, u, v);
    if constexpr (ABSORB) {
        for (int ch = 0; ch < kImageMaxChannels; ++ch)
            if (ch < tx.c) c[ch] = (image_absorb_factor(sigma[ch], L) * T) * image_env_bilinear(env, cell, ch);
    } else {
        for (int ch = 0; ch < tx.c; ++ch) c[ch] = T * image_env_bilinear(env, cell, ch);
    }
    return kImageBgEnv;
}

// The background of a ray, unweighted: B[0 .. tx.c).
DRT_HD int image_env_background(const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& env, d3 o, d3 d, double* B) {
    double u, v;
    if (has_screen && image_screen_uv(sc, tx.th, tx.tw, o, d, u, v)) {
        for (int ch = 0; ch < tx.c; ++ch) B[ch] = image_bilinear(tx, u, v, ch);
        return kImageBgScreen;
    }
    image_env_uv(env, d, u, v);
    const ImageEnvCell cell = image_env_cell(env, u, v);
    for (int ch = 0; ch < tx.c; ++ch) B[ch] = image_env_bilinear(env, cell, ch);
    return kImageBgEnv;
}

// The outer-surface reflection of a sample with camera ray (o, d) whose first interaction is the Bounce b: false when it has none
// (leaving the object, or a TIR flag); otherwise the reflected ray -- bounce_reflect, the function the mirrored interactions use -- and R1.
DRT_HD bool image_reflect_ray(const Bounce& b, d3 o, double ior_ext, double ior_int, d3& ro, d3& wr, double& R1) {
    if (!(b.sg > 0.0) || b.tir) return false;
    bounce_reflect(b, o, ro, wr);
    R1 = fresnel_R(b.ci, ior_ext, ior_int);
    return true;
}

// ... with the Bounce recomputed from the first face.
template <bool SNELL>
DRT_HD bool image_reflect_first(const PathCtx& c, int32_t face, d3 o, d3 d, d3& ro, d3& wr, double& R1) {
    if (face < 0 || face >= c.tc.n_tris) return false;
    d3 v0, v1, v2;
    int32_t vid[3];
    Bounce b;
    load_tri64(c, face, v0, v1, v2, vid);
    law_forward<SNELL>(o, d, v0, v1, v2, c.ior_ext, c.ior_int, b);
    return image_reflect_ray(b, o, c.ior_ext, c.ior_int, ro, wr, R1);
}

// c[ch] = c[ch] + R1 * B(ro, wr)[ch] on a through sample whose reflection was seen
DRT_HD void image_env_add_reflection(const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& env, d3 ro, d3 wr, double R1, double* c) {
    double B[kImageMaxChannels];
    image_env_background(sc, tx, has_screen, env, ro, wr, B);
    for (int ch = 0; ch < tx.c; ++ch) c[ch] = c[ch] + R1 * B[ch];
}

// Adjoint of `scale * B(o, d)` under the seeds g_c[0 .. tx.c) (image_env_background; the association of image_sample_backward:
// s_x = sum_ch g_c[ch] dB/dfx, g_u = scale * s_x): g_o, g_d are SET; returns sum_ch g_c[ch] B[ch], the seed of `scale`.
DRT_HD double image_env_background_backward(const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& env, d3 o, d3 d, const double* g_c,
                                            double scale, d3& g_o, d3& g_d) {
    double u, v, s_x = 0.0, s_y = 0.0, g_s = 0.0;
    if (has_screen && image_screen_uv(sc, tx.th, tx.tw, o, d, u, v)) {
        for (int ch = 0; ch < tx.c; ++ch) {
            double bx, by;
            const double B = image_bilinear_grad(tx, u, v, ch, bx, by);
            s_x = ch == 0 ? g_c[ch] * bx : s_x + g_c[ch] * bx;
            s_y = ch == 0 ? g_c[ch] * by : s_y + g_c[ch] * by;
            g_s = ch == 0 ? g_c[ch] * B : g_s + g_c[ch] * B;
        }
        image_screen_uv_backward(sc, o, d, scale * s_x, scale * s_y, g_o, g_d);
        return g_s;
    }
    image_env_uv(env, d, u, v);
    const ImageEnvCell cell = image_env_cell(env, u, v);
    for (int ch = 0; ch < tx.c; ++ch) {
        double bx, by;
        const double B = image_env_bilinear_grad(env, cell, ch, bx, by);
        s_x = ch == 0 ? g_c[ch] * bx : s_x + g_c[ch] * bx;
        s_y = ch == 0 ? g_c[ch] * by : s_y + g_c[ch] * by;
        g_s = ch == 0 ? g_c[ch] * B : g_s + g_c[ch] * B;
    }
    g_o = d3{0.0, 0.0, 0.0};
    image_env_uv_backward(env, d, scale * s_x, cell.v_inside ? scale * s_y : 0.0, g_d);
    return g_s;
}

// image_sample_backward in front of a screen (has_screen) and an environment: every THROUGH sample carries a gradient, through the screen
// where it lands on it (image_sample_backward itself: the same bits) and through the environment lookup otherwise.  LENGTH (absorbing
// glass): on the screen image_sample_backward<.., LENGTH>; to the environment the seeds g_c[ch] A_ch stand in for g_c
// (so g_T = sum g_c A E, and the (u, v) lookup seeds are scaled by A too), and g_L = sum_ch (g_c[ch] (-sigma_ch)) c[ch] with the forward's
// c[ch] = (A_ch T) E_ch goes to every interaction with sg < 0 (image_path_backward<.., LENGTH>).
template <bool SNELL, bool FRESNEL, bool LENGTH = false, typename Add>
DRT_HD bool image_env_sample_backward(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 exit_o, d3 exit_d, double T,
                                      const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& env, const double* g_c, Add add,
                                      double& g_int, double& g_ext, double L = 0.0, const double* sigma = nullptr) {
    double u, v;
    if constexpr (LENGTH) {
        if (has_screen && image_screen_uv(sc, tx.th, tx.tw, exit_o, exit_d, u, v))
            return image_sample_backward<SNELL, FRESNEL, true>(c, o, d, faces, face_stride, n_hits, exit_o, exit_d, T, sc, tx, g_c, add, g_int, g_ext, nullptr, nullptr,
                                                               L, sigma);
        double E[kImageMaxChannels], gA[kImageMaxChannels] = {0.0, 0.0, 0.0}, g_L = 0.0;
        image_env_background(sc, tx, false, env, exit_o, exit_d, E);
        for (int ch = 0; ch < tx.c; ++ch) {
            const double A = image_absorb_factor(sigma[ch], L);
            gA[ch] = g_c[ch] * A;
            const double col = (A * T) * E[ch];             // the forward's c[ch]
            const double gl = (g_c[ch] * (-sigma[ch])) * col;
            g_L = ch == 0 ? gl : g_L + gl;
        }
        d3 g_o, g_d;
        const double g_T = image_env_background_backward(sc, tx, false, env, exit_o, exit_d, gA, T, g_o, g_d);
        image_path_backward<SNELL, FRESNEL, true>(c, o, d, faces, face_stride, n_hits, g_o, g_d, g_T, add, g_int, g_ext, nullptr, nullptr, g_L);
        return true;
    } else {
        if (has_screen && image_screen_uv(sc, tx.th, tx.tw, exit_o, exit_d, u, v))
            return image_sample_backward<SNELL, FRESNEL>(c, o, d, faces, face_stride, n_hits, exit_o, exit_d, T, sc, tx, g_c, add, g_int, g_ext);
        d3 g_o, g_d;
        const double g_T = image_env_background_backward(sc, tx, false, env, exit_o, exit_d, g_c, T, g_o, g_d);
        image_path_backward<SNELL, FRESNEL>(c, o, d, faces, face_stride, n_hits, g_o, g_d, g_T, add, g_int, g_ext);
        return true;
    }
}

// The adjoint of the reflection term R1 * B(ro, wr) of a sample with camera ray (o, d) and first face `face`, under the seeds g_c: one
// triangle, one Bounce.  False (nothing handed to `add`, g_int = g_ext = 0): the sample has no outer-surface reflection.  The camera ray
// is a constant here.
template <bool SNELL, typename Add>
DRT_HD bool image_reflect_backward(const PathCtx& c, int32_t face, d3 o, d3 d, const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& env,
                                   const double* g_c, Add add, double& g_int, double& g_ext) {
    g_int = 0.0; g_ext = 0.0;
    if (face < 0 || face >= c.tc.n_tris) return false;
    d3 v0, v1, v2, ro, wr;
    int32_t vid[3];
    Bounce b;
    double R1;
    load_tri64(c, face, v0, v1, v2, vid);
    law_forward<SNELL>(o, d, v0, v1, v2, c.ior_ext, c.ior_int, b);
    if (!image_reflect_ray(b, o, c.ior_ext, c.ior_int, ro, wr, R1)) return false;
    d3 g_ro, g_wr;
    const double g_R1 = image_env_background_backward(sc, tx, has_screen, env, ro, wr, g_c, R1, g_ro, g_wr);
    const d3 z{0.0, 0.0, 0.0};
    d3 ga = z, gb = z, gc = z, g_o_in, g_d_in;
    bounce_reflect_backward(b, g_ro, g_wr, ga, gb, gc, g_o_in, g_d_in);
    double g_ci = 0.0;
    fresnel_R_backward(b.ci, c.ior_ext, c.ior_int, g_R1, g_ci, g_ext, g_int);          // (entering: eta_i = ext, eta_t = int)
    bounce_ci_backward(b, g_ci, ga, gb, gc, g_d_in);
    add(vid[0], ga); add(vid[1], gb); add(vid[2], gc);
    return true;
}

}  // namespace drt
