// drt_image_screen.h -- the adjoint of the photometric loss of the refracted image (drt_image_loss.h) w.r.t. the END of the light path: the
// screen's pose (p0, eu, ev) and the texture (Scene.image_loss_fused with screen_param / texture_param,
// drt_render_image_loss_screen).  Every forward quantity is drt_image.h's and the seed g_c[ch] = 2 w_p r_ch / s^2 is image_loss_pixel's.
// What carries a gradient: every DIRECT and every THROUGH sample that lands on the screen, c[ch] = T * B[ch](u, v) -- T = 1 on a direct
// sample and with the Fresnel term off.  The ray (o, d) of the sample -- the camera ray, or the exit ray of the path -- depends on neither
// the screen nor the texture, so nothing here touches a path: the vertex and IOR gradients are drt_image_loss.h's, unchanged.
//   texture  B = ((t00 (1 - fx) + t01 fx) (1 - fy)) + ((t10 (1 - fx) + t11 fx) fy): texel (y0, x0) receives (g_c[ch] T) ((1 - fx) (1 - fy)),
//            (y0, x0 + 1) ... (fx (1 - fy)), (y0 + 1, x0) ... ((1 - fx) fy), (y0 + 1, x0 + 1) ... (fx fy), w.r.t. (double)texel
//   screen   g_u = T sum_ch g_c dB/dfx, g_v likewise (image_bilinear_grad), then image_screen_uv's statements in reverse: torch's quotient
//            rule, the cross product's adjoints; eu and ev are independent inputs
// The on-screen test, floor, the clamp of the cell, the orthogonality check, a sample's class and the two fills carry no gradient.
// Plain C++ like drt_image_loss.h (tests/hostsim/image_screen.cpp runs these bodies on the host against torch autograd of
// tests/image_screen_ref.py).  drt_image.h's and drt_image_loss.h's functions are used as they are; nothing of them is restated.
#pragma once
#include "drt_image_loss.h"

namespace drt {

// Adjoint of image_screen_uv w.r.t. the screen on a ray that sees it: (g_u, g_v) -> accumulated into g_p0, g_eu, g_ev.
DRT_HD void image_screen_uv_backward_screen(const ImageScreen& sc, d3 o, d3 d, double g_u, double g_v, d3& g_p0, d3& g_eu, d3& g_ev) {
    // the forward, statement for statement
    const d3 n = cross(sc.eu, sc.ev);
    const double dn = dot(d, n);
    const d3 po = sc.p0 - o;
    const double t = dot(po, n) / dn;
    const d3 q = o + t * d;
    const d3 r = q - sc.p0;
    const double uu = dot(sc.eu, sc.eu), vv = dot(sc.ev, sc.ev);
    const double u = dot(r, sc.eu) / uu, v = dot(r, sc.ev) / vv;
    // u = (r . eu) / (eu . eu), v = (r . ev) / (ev . ev)
    const double g_nu = g_u / uu, g_uu = -g_u * (u / uu);
    const double g_nv = g_v / vv, g_vv = -g_v * (v / vv);
    const d3 g_r = g_nu * sc.eu + g_nv * sc.ev;
    g_eu += g_nu * r + (2.0 * g_uu) * sc.eu;
    g_ev += g_nv * r + (2.0 * g_vv) * sc.ev;
    // r = q - p0 ; q = o + t d
    g_p0 -= g_r;
    const double g_t = dot(g_r, d);
    // t = a / dn ; a = (p0 - o) . n ; dn = d . n
    const double g_a = g_t / dn, g_dn = -g_t * (t / dn);
    g_p0 += g_a * n;
    const d3 g_n = g_a * po + g_dn * d;
    // n = eu x ev
    g_eu += cross(sc.ev, g_n);
    g_ev += cross(g_n, sc.eu);
}

// The whole adjoint of one direct or through sample w.r.t. the texture and the screen: its ray (o, d), its throughput T and the seed
// g_c[0 .. tx.c) of its pixel.  tex_add(texel, g) is called four times with the flat texel number y * tw + x of a corner of the cell and
// its tx.c channel contributions; the nine screen partials are accumulated into g_p0, g_eu, g_ev.  False (nothing done): the sample does
// not land on the screen.
template <typename TexAdd>
DRT_HD bool image_sample_backward_screen(const ImageScreen& sc, const ImageTex& tx, d3 o, d3 d, double T, const double* g_c, TexAdd tex_add, d3& g_p0,
                                         d3& g_eu, d3& g_ev) {
    double u, v;
    if (!image_screen_uv(sc, tx.th, tx.tw, o, d, u, v)) return false;
    // the cell, as image_bilinear has it
    double x0 = floor(u), y0 = floor(v);
    if (x0 > (double)(tx.tw - 2)) x0 = (double)(tx.tw - 2);
    if (y0 > (double)(tx.th - 2)) y0 = (double)(tx.th - 2);
    const double fx = u - x0, fy = v - y0;
    const double w00 = (1.0 - fx) * (1.0 - fy), w01 = fx * (1.0 - fy), w10 = (1.0 - fx) * fy, w11 = fx * fy;
    double s_x = 0.0, s_y = 0.0;
    double g00[kImageMaxChannels], g01[kImageMaxChannels], g10[kImageMaxChannels], g11[kImageMaxChannels];
    for (int ch = 0; ch < tx.c; ++ch) {
        double bx, by;
        (void)image_bilinear_grad(tx, u, v, ch, bx, by);
        s_x = ch == 0 ? g_c[ch] * bx : s_x + g_c[ch] * bx;
        s_y = ch == 0 ? g_c[ch] * by : s_y + g_c[ch] * by;
        const double g_B = g_c[ch] * T;
        g00[ch] = g_B * w00; g01[ch] = g_B * w01; g10[ch] = g_B * w10; g11[ch] = g_B * w11;
    }
    const int32_t cell = (int32_t)y0 * tx.tw + (int32_t)x0;
    tex_add(cell, g00);
    tex_add(cell + 1, g01);
    tex_add(cell + tx.tw, g10);
    tex_add(cell + tx.tw + 1, g11);
    image_screen_uv_backward_screen(sc, o, d, T * s_x, T * s_y, g_p0, g_eu, g_ev);
    return true;
}

}  // namespace drt
