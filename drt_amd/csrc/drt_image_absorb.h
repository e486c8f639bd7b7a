// drt_image_absorb.h -- absorbing glass: Beer-Lambert attenuation in the refracted image and in its photometric loss (DESIGN.md section
// 10.7; Scene.render_image / Scene.image_loss_fused with `absorption`, drt_render_image_absorb, drt_render_image_loss_absorb).
//   sigma[C]  one absorption coefficient per texture channel, per unit of mesh length: float64, finite, >= 0
//   L         the interior length of a sample: ((t_1 + t_2) + ...) in interaction order over the interactions whose incoming ray
//             travelled inside the object (Bounce::sg < 0, refracting or mirrored), t the Bounce::t law_forward<SNELL> leaves -- both laws
//             fill t and sg through bounce_forward's own statements (bounce_forward_snell calls it first).  A direct sample has L = 0
//   A_ch      exp(-(sigma_ch * L))
//   c[ch]     (A_ch * T) * bilinear_ch for a through or direct sample on the screen; the fills are not weighted
// Every other forward quantity is drt_image.h's, unchanged.  With every sigma_ch = 0, A_ch = exp(-0) = 1 and (1 * T) * B has the bits of
// T * B.  The adjoint adds to drt_image_loss.h's one seed: g_L = sum_ch g_c[ch] * (-sigma_ch) * c[ch], handed to the t of every interior
// interaction (bounce_t_backward), from where it reaches the vertices, the incoming ray and, through the existing chain of the earlier
// interactions, the IORs.  d loss / d sigma_ch = -g_c[ch] * sum_j L_j * c_j[ch] over a pixel's through samples on the screen needs forward
// values only.  Class, faces, TIR flags, sg, the texel cell and the screen border carry no gradient, as in 10.3.
// Plain C++ like drt_image.h (tests/hostsim/image_absorb.cpp runs these bodies on the host against tests/image_absorb_ref.py).
// drt_image.h's and drt_image_loss.h's functions are used as they are; nothing of them is restated or edited.
#pragma once
#include "drt_image_loss.h"

namespace drt {

// What an interaction adds to the interior length: L + t when its incoming ray travelled inside the object, L otherwise.
DRT_HD double image_absorb_length(const Bounce& b, double L) { return b.sg < 0.0 ? L + b.t : L; }

// image_interact (drt_image.h) -- the same continuation, the same bits for o, d, T and n_refr -- that also hands the bounce to `length`
// right behind law_forward, before the throughput: the caller adds image_absorb_length to the interior length it keeps (a kernel does so
// in memory at once, so that no length is held in registers across the Fresnel term).
template <bool SNELL, bool FRESNEL, typename Length>
DRT_HD bool image_absorb_interact(const PathCtx& c, int32_t face, bool reflect, d3& o, d3& d, int& n_refr, double& T, Length length) {
    d3 v0, v1, v2;
    int32_t vid[3];
    Bounce b;
    load_tri64(c, face, v0, v1, v2, vid);
    law_forward<SNELL>(o, d, v0, v1, v2, c.ior_ext, c.ior_int, b);
    length(b);
    if (!b.tir) {
        if constexpr (FRESNEL) T = T * image_transmittance(b, c.ior_ext, c.ior_int);
        o = b.new_o; d = b.wt;
        ++n_refr;
        return true;
    }
    if (!reflect) return false;
    d3 no, wr;
    bounce_reflect(b, o, no, wr);
    o = no; d = wr;
    return true;
}

// A_ch = exp(-(sigma_ch * L))
DRT_HD double image_absorb_factor(double sigma, double L) { return exp(-(sigma * L)); }

// image_sample_colour with the attenuation: c[ch] = (A_ch * T) * B_ch on the screen.  True: the sample is direct or through and landed on
// the screen (its colour is a function of T and L); false: c is a fill.
DRT_HD bool image_absorb_sample_colour(const ImageScreen& sc, const ImageTex& tx, int cls, d3 o, d3 d, double T, double L, const double* sigma,
                                       const double* fill_void, const double* fill_invalid, double* c) {
    if (cls == kImageInvalid) {
        for (int ch = 0; ch < tx.c; ++ch) c[ch] = fill_invalid[ch];
        return false;
    }
    double u, v;
    if (!image_screen_uv(sc, tx.th, tx.tw, o, d, u, v)) {
        for (int ch = 0; ch < tx.c; ++ch) c[ch] = fill_void[ch];
        return false;
    }
    for (int ch = 0; ch < kImageMaxChannels; ++ch)          // (a fixed trip count: the three colours stay in registers on the device)
        if (ch < tx.c) c[ch] = (image_absorb_factor(sigma[ch], L) * T) * image_bilinear(tx, u, v, ch);
    return true;
}

// Adjoint of t = e2q * inv of bounce_forward for the incoming g_t, statement for statement as bounce_backward has the chain (the way
// bounce_ci_backward does ci): accumulates into the three vertices and into the incoming ray (g_o, g_d).
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

// image_path_backward (drt_image_loss.h) -- the same recompute, the same reverse loop, the same seeds -- with one addition: every
// interaction whose incoming ray travelled inside the object (sg < 0) hands g_L, the seed of the interior length, to its t through
// bounce_t_backward, into the same three vertex gradients and into g_o_in / g_d_in; the interactions before it pass that on, the
// refracting ones also to the IORs through law_backward_eta.
template <bool SNELL, bool FRESNEL, typename Add>
DRT_HD void image_path_backward_absorb(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 g_ori, d3 g_dir, double g_T,
                                       double g_L, Add add, double& g_int, double& g_ext) {
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
        if (b.sg < 0.0) bounce_t_backward(b, g_L, ga, gb, gc, g_o_in, g_d_in);
        add(vid[0], ga); add(vid[1], gb); add(vid[2], gc);
        g_o = g_o_in; g_d = g_d_in;
    }
}

// The whole adjoint of one THROUGH sample under absorption: image_sample_backward with A_ch on the seeds of T and of (u, v), and the seed
// of the interior length L the forward left behind.  False (nothing handed to `add`, g_int = g_ext = 0): the sample does not land on the
// screen.
template <bool SNELL, bool FRESNEL, typename Add>
DRT_HD bool image_sample_backward_absorb(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 exit_o, d3 exit_d, double T,
                                         double L, const double* sigma, const ImageScreen& sc, const ImageTex& tx, const double* g_c, Add add,
                                         double& g_int, double& g_ext) {
    g_int = 0.0; g_ext = 0.0;
    double u, v;
    if (!image_screen_uv(sc, tx.th, tx.tw, exit_o, exit_d, u, v)) return false;
    double s_x = 0.0, s_y = 0.0, g_T = 0.0, g_L = 0.0;
    for (int ch = 0; ch < tx.c; ++ch) {
        double bx, by;
        const double B = image_bilinear_grad(tx, u, v, ch, bx, by);
        const double A = image_absorb_factor(sigma[ch], L);
        const double gA = g_c[ch] * A;
        s_x = ch == 0 ? gA * bx : s_x + gA * bx;
        s_y = ch == 0 ? gA * by : s_y + gA * by;
        g_T = ch == 0 ? gA * B : g_T + gA * B;
        const double col = (A * T) * B;             // the forward's c[ch]
        const double gl = (g_c[ch] * (-sigma[ch])) * col;
        g_L = ch == 0 ? gl : g_L + gl;
    }
    d3 g_o, g_d;
    image_screen_uv_backward(sc, exit_o, exit_d, T * s_x, T * s_y, g_o, g_d);
    image_path_backward_absorb<SNELL, FRESNEL>(c, o, d, faces, face_stride, n_hits, g_o, g_d, g_T, g_L, add, g_int, g_ext);
    return true;
}

// What one pixel adds to d loss / d sigma_ch: -g_c[ch] * lc[ch], lc[ch] = ((L_0 c_0[ch] + L_1 c_1[ch]) + ...) over its through samples on the
// screen, in sample order.
DRT_HD double image_absorb_sigma_term(double g_c, double lc) { return -(g_c * lc); }

}  // namespace drt
