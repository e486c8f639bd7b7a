// drt_image_loss.h -- the photometric loss of the refracted image and its adjoint w.r.t. the vertices and the two indices of refraction
// (Scene.image_loss_fused, drt_render_image_loss).  Every forward quantity is drt_image.h's, unchanged:
//   I[p][ch]  = (((c_0 + c_1) + ...) / s^2)        the float64 pixel mean render_image rounds to float32
//   r         = I - (double)target[p][ch]
//   loss     += w_p * ((r_0^2 + r_1^2) + r_2^2)    w_p = 1, or (double)weight[p]
// and the gradient is the derivative of that sum under torch's conventions.  What carries a gradient: only THROUGH samples that land on
// the screen, c[ch] = T * B[ch] with the seed g_c[ch] = 2 w_p r_ch / s^2.  Direct, void and invalid samples are constants; a sample's
// class, the face tape, the TIR flags, the `entering` branch, floor and the x0 clamp of the bilinear cell and the on-screen test carry no
// gradient.  The adjoint of a through sample runs bilinear -> plane -> path, and, with the Fresnel term on, the throughput: every
// refracting interaction k has the factor f_k = 1 - R_k and receives g_f_k = g_T * prod_{j != k} f_j (the product of the OTHER factors, no
// division by f_k); R's adjoint follows fresnel_R line by line and enters the bounce through ci = -(n . d).
// The guards of the two square roots of fresnel_R, as tests/snell_ref.py refract_dir_snell spells its own: where the argument of a sqrt is
// not positive the root is the constant 0 and no gradient passes through it (sqrt's own derivative there would be inf, and inf * 0 at
// normal incidence NaN).  A clamp passes the gradient inside its closed bounds.
// Plain C++ like drt_image.h (tests/hostsim/image_loss.cpp runs these bodies on the host against torch autograd of tests/image_loss_ref.py).
// drt_shade.h's and drt_image.h's functions are used as they are; nothing of them is restated.
#pragma once
#include "drt_image.h"

namespace drt {

// Adjoint of fresnel_R(ci, eta_i, eta_t) for the incoming g_R: accumulates into g_ci, g_eta_i, g_eta_t.
DRT_HD void fresnel_R_backward(double ci, double eta_i, double eta_t, double g_R, double& g_ci, double& g_eta_i, double& g_eta_t) {
    // the forward, statement for statement
    const double x0 = 1.0 - ci * ci;
    const double x = x0 < 0.0 ? 0.0 : (x0 > 1.0 ? 1.0 : x0);
    const double sin_i = sqrt(x);
    const double se = sin_i * eta_i;
    const double sin_t = se / eta_t;
    const double y0 = 1.0 - sin_t * sin_t;
    const double y = y0 < 0.0 ? 0.0 : y0;
    const double cos_t = sqrt(y);
    const double a = eta_t * ci, b = eta_i * cos_t, c = eta_i * ci, e = eta_t * cos_t;
    const double den_l = a + b, den_p = c + e;
    const double r_parl = (a - b) / den_l, r_perp = (c - e) / den_p;
    // R = (r_parl^2 + r_perp^2) / 2
    const double g_sum = g_R / 2.0;
    const double g_rl = (2.0 * r_parl) * g_sum, g_rp = (2.0 * r_perp) * g_sum;
    // r = num / den (torch's quotient rule), num = a - b, den = a + b
    const double g_num_l = g_rl / den_l, g_den_l = -g_rl * (r_parl / den_l);
    const double g_num_p = g_rp / den_p, g_den_p = -g_rp * (r_perp / den_p);
    const double g_a = g_num_l + g_den_l, g_b = g_den_l - g_num_l;
    const double g_c = g_num_p + g_den_p, g_e = g_den_p - g_num_p;
    g_eta_t += g_a * ci;    g_ci += g_a * eta_t;
    g_eta_i += g_c * ci;    g_ci += g_c * eta_i;
    g_eta_i += g_b * cos_t; g_eta_t += g_e * cos_t;
    const double g_cos_t = g_b * eta_i + g_e * eta_t;
    // cos_t = sqrt(max(y0, 0)): nothing through a root that is the constant 0
    const double g_y0 = y > 0.0 ? g_cos_t / (2.0 * cos_t) : 0.0;
    // y0 = 1 - sin_t^2 ; sin_t = (sin_i * eta_i) / eta_t
    const double g_sin_t = (-2.0 * sin_t) * g_y0;
    const double g_se = g_sin_t / eta_t;
    g_eta_t += -g_sin_t * (sin_t / eta_t);
    g_eta_i += g_se * sin_i;
    const double g_sin_i = g_se * eta_i;
    // sin_i = sqrt(clamp(x0, 0, 1)) ; x0 = 1 - ci^2
    const double g_x = x > 0.0 ? g_sin_i / (2.0 * sin_i) : 0.0;
    const double g_x0 = (x0 >= 0.0 && x0 <= 1.0) ? g_x : 0.0;
    g_ci += (-2.0 * ci) * g_x0;
}

// Adjoint of image_transmittance of a REFRACTING bounce (f = 1 - R) for the incoming g_f: g_ci is set; the eta pair goes to the IORs through
// the `entering` branch of the bounce (eta_to_ior's branch: sg = 1: eta_i = ext, eta_t = int), accumulated into g_int / g_ext.
DRT_HD void image_transmittance_backward(const Bounce& b, double ior_ext, double ior_int, double g_f, double& g_ci, double& g_int, double& g_ext) {
    const bool entering = b.sg > 0.0;
    double g_ei = 0.0, g_et = 0.0;
    g_ci = 0.0;
    fresnel_R_backward(b.ci, entering ? ior_ext : ior_int, entering ? ior_int : ior_ext, -g_f, g_ci, g_ei, g_et);
    if (entering) { g_ext += g_ei; g_int += g_et; }
    else { g_int += g_ei; g_ext += g_et; }
}

// What a gradient of Bounce::ci adds to a bounce's adjoint: ci = n . wo = -(n . d), then the normal chain n = sg * n0, n0 = m / |m|,
// m = e1 x e2 statement for statement as bounce_backward has it.  Accumulates into the three vertices and into g_d.
DRT_HD void bounce_ci_backward(const Bounce& b, double g_ci, d3& gv0, d3& gv1, d3& gv2, d3& g_d) {
    const d3 g_n = (-g_ci) * b.d;
    g_d += (-g_ci) * b.n;
    const d3 g_n0 = b.sg * g_n;
    const d3 g_m = (g_n0 - dot(b.n0, g_n0) * b.n0) / b.len;
    const d3 g_e1 = cross(b.e2, g_m);
    const d3 g_e2 = cross(g_m, b.e1);
    gv1 += g_e1;
    gv2 += g_e2;
    gv0 -= g_e1 + g_e2;
}

// Adjoint of t = e2q * inv of bounce_forward for the incoming g_t (absorbing glass: the seed of the interior length), statement for
// statement as bounce_backward has the chain (the way bounce_ci_backward does ci): accumulates into the three vertices and into the
// incoming ray (g_o, g_d).
DRT_HD void bounce_t_backward(const Bounce& b, double g_t, d3& gv0, d3& gv1, d3& gv2, d3& g_o, d3& g_d) {
    // t = (e2 . q) * inv
    d3 g_e2 = (g_t * b.inv) * b.q;
    const d3 g_q = (g_t * b.inv) * b.e2;
    const double g_inv = g_t * b.e2q;
    // q = s x e1
    const d3 g_s = cross(b.e1, g_q);
    d3 g_e1 = cross(g_q, b.s);
    // s = o - v0
    g_o += g_s;
    // inv = 1/det ; det = e1 . p ; p = d x e2
    const double g_det = -g_inv * b.inv * b.inv;
    g_e1 += g_det * b.p;
    const d3 g_p = g_det * b.e1;
    g_d += cross(b.e2, g_p);
    g_e2 += cross(g_p, b.d);
    gv1 += g_e1;
    gv2 += g_e2;
    gv0 -= (g_s + g_e1) + g_e2;
}

// What one pixel adds to d loss / d sigma_ch: -g_c[ch] * lc[ch], lc[ch] = ((L_0 c_0[ch] + L_1 c_1[ch]) + ...) over its through samples on the
// screen, in sample order.
DRT_HD double image_absorb_sigma_term(double g_c, double lc) { return -(g_c * lc); }

// image_bilinear of channel ch and its derivatives w.r.t. fx and fy, the formula differentiated as written; floor and the clamp of the
// cell carry nothing, so d / du = d / dfx and d / dv = d / dfy.
DRT_HD double image_bilinear_grad(const ImageTex& tx, double u, double v, int ch, double& dB_dfx, double& dB_dfy) {
    double x0 = floor(u), y0 = floor(v);
    if (x0 > (double)(tx.tw - 2)) x0 = (double)(tx.tw - 2);
    if (y0 > (double)(tx.th - 2)) y0 = (double)(tx.th - 2);
    const double fx = u - x0, fy = v - y0;
    const float* row = tx.texel + ((int64_t)y0 * tx.tw + (int64_t)x0) * tx.c + ch;     // as image_bilinear: all four reads inside
    const int64_t down = (int64_t)tx.tw * tx.c;
    const double t00 = (double)row[0], t01 = (double)row[tx.c], t10 = (double)row[down], t11 = (double)row[down + tx.c];
    dB_dfx = ((t01 - t00) * (1.0 - fy)) + ((t11 - t10) * fy);
    dB_dfy = (t10 * (1.0 - fx) + t11 * fx) - (t00 * (1.0 - fx) + t01 * fx);
    return ((t00 * (1.0 - fx) + t01 * fx) * (1.0 - fy)) + ((t10 * (1.0 - fx) + t11 * fx) * fy);
}

// Adjoint of image_screen_uv on a ray that sees the screen: (g_u, g_v) -> g_q -> (g_o, g_d; set) through q = o + t d and
// t = ((p0 - o) . n) / (d . n).
DRT_HD void image_screen_uv_backward(const ImageScreen& sc, d3 o, d3 d, double g_u, double g_v, d3& g_o, d3& g_d) {
    const d3 n = cross(sc.eu, sc.ev);
    const double dn = dot(d, n);
    const double t = dot(sc.p0 - o, n) / dn;
    // u = (r . eu) / (eu . eu), v = (r . ev) / (ev . ev), r = q - p0
    const d3 g_q = (g_u / dot(sc.eu, sc.eu)) * sc.eu + (g_v / dot(sc.ev, sc.ev)) * sc.ev;
    // q = o + t d
    g_o = g_q;
    const double g_t = dot(g_q, d);
    g_d = t * g_q;
    // t = a / dn ; a = (p0 - o) . n ; dn = d . n
    const double g_a = g_t / dn, g_dn = -g_t * (t / dn);
    g_o += (-g_a) * n;
    g_d += g_dn * n;
}

// path_recompute_backward_ior_k (drt_paths.h) -- the same recompute from the camera ray and the face tape, the same reverse loop with
// (g_ori, g_dir) as the exit seeds -- that, FRESNEL, also reverses the throughput T = prod f_k with the seed g_T: a refracting interaction
// receives g_T times the product of the other factors (those before it kept from the recompute, those after it gathered by the reverse
// loop), hands it through image_transmittance_backward to the IORs and to ci, and bounce_ci_backward adds ci's share to the vertices
// and to the incoming direction.  A mirrored interaction has no factor.  g_int / g_ext: set.  seed_o / seed_d (both or neither): receive
// what the reverse loop ends with, the adjoint of the camera ray (o, d) -- the Fresnel share of the incoming direction included
// (drt_image_camera.h carries it on to the camera).  LENGTH (absorbing glass): every interaction whose incoming ray
// travelled inside the object (sg < 0) also hands g_L, the seed of the interior length, to its t through bounce_t_backward, into the same
// three vertex gradients and into g_o_in / g_d_in; the interactions before it pass that on, the refracting ones also to the IORs.
template <bool SNELL, bool FRESNEL, bool LENGTH = false, typename Add>
DRT_HD void image_path_backward(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 g_ori, d3 g_dir, double g_T,
                                Add add, double& g_int, double& g_ext, d3* seed_o = nullptr, d3* seed_d = nullptr, double g_L = 0.0) {
    d3 ro[kMaxBounces], rd[kMaxBounces];
    double before[kMaxBounces];                 // prod_{j < k} f_j
    d3 v0, v1, v2;
    int32_t vid[3];
    Bounce b;
    g_int = 0.0; g_ext = 0.0;
    if (n_hits > kMaxBounces) n_hits = kMaxBounces;
    double T = 1.0;
    for (int k = 0; k < n_hits; ++k) {
        ro[k] = o; rd[k] = d;
        if constexpr (FRESNEL) before[k] = T;
        if (k + 1 == n_hits) break;              // (the last interaction is rebuilt by the reverse loop)
        load_tri64(c, faces[k * face_stride], v0, v1, v2, vid);
        law_forward<SNELL>(o, d, v0, v1, v2, c.ior_ext, c.ior_int, b);
        if (b.tir) { d3 no, wr; bounce_reflect(b, o, no, wr); o = no; d = wr; }
        else {
            if constexpr (FRESNEL) T = T * image_transmittance(b, c.ior_ext, c.ior_int);
            o = b.new_o; d = b.wt;
        }
    }
    const d3 z{0.0, 0.0, 0.0};
    d3 g_o = g_ori, g_d = g_dir;
    double after = 1.0;                         // prod_{j > k} f_j
    for (int k = n_hits - 1; k >= 0; --k) {
        load_tri64(c, faces[k * face_stride], v0, v1, v2, vid);
        law_forward<SNELL>(ro[k], rd[k], v0, v1, v2, c.ior_ext, c.ior_int, b);
        d3 ga = z, gb = z, gc = z, g_o_in, g_d_in;
        if (b.tir) {
            bounce_reflect_backward(b, g_o, g_d, ga, gb, gc, g_o_in, g_d_in);
        } else {
            double g_eta;
            law_backward_eta<SNELL>(b, g_o, g_d, ga, gb, gc, g_o_in, g_d_in, g_eta);
            eta_to_ior(b, c.ior_int, c.ior_ext, g_eta, g_int, g_ext);
            if constexpr (FRESNEL) {
                double g_ci;
                image_transmittance_backward(b, c.ior_ext, c.ior_int, g_T * (before[k] * after), g_ci, g_int, g_ext);
                bounce_ci_backward(b, g_ci, ga, gb, gc, g_d_in);
                after = after * image_transmittance(b, c.ior_ext, c.ior_int);
            }
        }
        if constexpr (LENGTH) {
            if (b.sg < 0.0) bounce_t_backward(b, g_L, ga, gb, gc, g_o_in, g_d_in);
        }
        add(vid[0], ga); add(vid[1], gb); add(vid[2], gc);
        g_o = g_o_in; g_d = g_d_in;
    }
    if (seed_o) { *seed_o = g_o; *seed_d = g_d; }
}

// The whole adjoint of one THROUGH sample: camera ray (o, d), face tape, the exit ray and throughput the forward left behind, and the seed
// g_c[0 .. tx.c) of its pixel.  False (nothing handed to `add`, g_int = g_ext = 0): the sample does not land on the screen.
// seed_o / seed_d: image_path_backward's, written only when true is returned.  LENGTH (absorbing glass): A_ch = exp(-(sigma_ch * L)) on
// the seeds of T and of (u, v), and the seed g_L of the interior length L the forward left behind.
template <bool SNELL, bool FRESNEL, bool LENGTH = false, typename Add>
DRT_HD bool image_sample_backward(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 exit_o, d3 exit_d, double T,
                                  const ImageScreen& sc, const ImageTex& tx, const double* g_c, Add add, double& g_int, double& g_ext,
                                  d3* seed_o = nullptr, d3* seed_d = nullptr, double L = 0.0, const double* sigma = nullptr) {
    g_int = 0.0; g_ext = 0.0;
    double u, v;
    if (!image_screen_uv(sc, tx.th, tx.tw, exit_o, exit_d, u, v)) return false;
    double s_x = 0.0, s_y = 0.0, g_T = 0.0, g_L = 0.0;
    for (int ch = 0; ch < tx.c; ++ch) {
        double bx, by;
        const double B = image_bilinear_grad(tx, u, v, ch, bx, by);
        [[maybe_unused]] double A = 1.0;
        double gA = g_c[ch];
        if constexpr (LENGTH) { A = image_absorb_factor(sigma[ch], L); gA = g_c[ch] * A; }
        s_x = ch == 0 ? gA * bx : s_x + gA * bx;
        s_y = ch == 0 ? gA * by : s_y + gA * by;
        g_T = ch == 0 ? gA * B : g_T + gA * B;
        if constexpr (LENGTH) {
            const double col = (A * T) * B;             // the forward's c[ch]
            const double gl = (g_c[ch] * (-sigma[ch])) * col;
            g_L = ch == 0 ? gl : g_L + gl;
        }
    }
    d3 g_o, g_d;
    image_screen_uv_backward(sc, exit_o, exit_d, T * s_x, T * s_y, g_o, g_d);
    image_path_backward<SNELL, FRESNEL, LENGTH>(c, o, d, faces, face_stride, n_hits, g_o, g_d, g_T, add, g_int, g_ext, seed_o, seed_d, g_L);
    return true;
}

// One pixel, from the float64 mean of its s^2 sample colours (summed left to right and divided as k_image_resolve does): the residual
// against the target, the loss term (returned) and the seed g_c[ch] = ((2 w) r_ch) / s^2 of every sample of the pixel.
DRT_HD double image_loss_pixel(const double* mean, int channels, int s2, const float* target, double w, double* g_c) {
    double term = 0.0;
    for (int ch = 0; ch < channels; ++ch) {
        const double r = mean[ch] - (double)target[ch];
        term = ch == 0 ? r * r : term + r * r;
        g_c[ch] = ((2.0 * w) * r) / (double)s2;
    }
    return w * term;
}

}  // namespace drt
