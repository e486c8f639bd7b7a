// drt_image_camera.h -- the adjoint of the photometric loss of the refracted image (drt_image_loss.h) w.r.t. the START of the light path: the
// camera, as the kernels read it -- ImageCam{kinv[9], rinv[12]}, 21 numbers (Scene.image_loss_fused with
// camera_param, drt_render_image_loss_camera).  Every forward quantity is drt_image.h's and the seed g_c[ch] = 2 w_p r_ch / s^2 is
// image_loss_pixel's.  What carries a gradient: every DIRECT and every THROUGH sample that lands on the screen, through its camera ray.
//   through  the seeds (g_o, g_d) are what image_path_backward's reverse loop ends with (its seed_o / seed_d): the adjoint of the ray
//            that entered the first interaction, the Fresnel share of the incoming direction (bounce_ci_backward) included
//   direct   the camera ray is the ray that meets the screen, T = 1: the seeds are image_screen_uv_backward's on it, with
//            (s_x, s_y) = sum_ch g_c[ch] (dB/dfx, dB/dfy) of image_bilinear_grad
// and then image_sample_ray's statements in reverse (image_sample_ray_backward) under torch's conventions.  All nine entries of K^-1 and
// all twelve of the top of R^-1 are independent inputs: no bottom row (0, 0, 1) and no orthogonality is assumed.
// A sample's class, the top-box test, the face tape, the TIR flags, the `entering` branch, floor, the clamp of the bilinear cell, the
// on-screen test and the two fills carry no gradient; silhouettes are not differentiated.
// Plain C++ like drt_image_loss.h (tests/hostsim/image_camera.cpp runs these bodies on the host against torch autograd of
// tests/image_camera_ref.py).  drt_image.h's and drt_image_loss.h's functions are used as they are; nothing of them is restated.
#pragma once
#include "drt_image_loss.h"

namespace drt {

constexpr int kImageCamParams = 21;        // kinv[9], then rinv[12]: ImageCam's layout, and camera21's

// Adjoint of image_sample_ray(cam, s, x, y, j, origin, dir) for the incoming (g_o, g_d): ACCUMULATES into g_kinv[9] and g_rinv[12].
DRT_HD void image_sample_ray_backward(const ImageCam& cam, int s, int x, int y, int j, d3 g_o, d3 g_d, double* g_kinv, double* g_rinv) {
    // the forward, statement for statement
    const int a = j % s, b = j / s;
    const double px = ((double)x + ((double)a + 0.5) / (double)s) - 0.5;
    const double py = ((double)y + ((double)b + 0.5) / (double)s) - 0.5;
    const double* K = cam.kinv;
    const double* R = cam.rinv;
    const double p[3] = {(K[0] * px + K[1] * py) + K[2], (K[3] * px + K[4] * py) + K[5], (K[6] * px + K[7] * py) + K[8]};
    const d3 w{(R[0] * p[0] + R[1] * p[1]) + R[2] * p[2], (R[4] * p[0] + R[5] * p[1]) + R[6] * p[2], (R[8] * p[0] + R[9] * p[1]) + R[10] * p[2]};
    const double len = sqrt((w.x * w.x + w.y * w.y) + w.z * w.z);
    const d3 dir = w / len;
    // origin = rinv[:, 3]
    g_rinv[3] += g_o.x; g_rinv[7] += g_o.y; g_rinv[11] += g_o.z;
    // dir = w / len (torch's quotient rule) ; len = sqrt(len2) ; len2 = (w_x^2 + w_y^2) + w_z^2
    const double g_len = -((g_d.x * (dir.x / len) + g_d.y * (dir.y / len)) + g_d.z * (dir.z / len));
    const double g_len2 = g_len / (2.0 * len);
    const d3 g_w = g_d / len + (2.0 * g_len2) * w;
    // w_r = (R[r][0] p_0 + R[r][1] p_1) + R[r][2] p_2
    const double gw[3] = {g_w.x, g_w.y, g_w.z};
    double g_p[3] = {0.0, 0.0, 0.0};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            g_rinv[4 * r + c] += gw[r] * p[c];
            g_p[c] += R[4 * r + c] * gw[r];
        }
    // p_r = (K[r][0] px + K[r][1] py) + K[r][2]
    for (int r = 0; r < 3; ++r) {
        g_kinv[3 * r + 0] += g_p[r] * px;
        g_kinv[3 * r + 1] += g_p[r] * py;
        g_kinv[3 * r + 2] += g_p[r];
    }
}

// The camera-ray seeds of a DIRECT sample of pixel seed g_c[0 .. tx.c): (o, d) is image_sample_ray's ray.  False (g_o, g_d untouched): the
// sample does not land on the screen.
DRT_HD bool image_direct_seeds(const ImageScreen& sc, const ImageTex& tx, d3 o, d3 d, const double* g_c, d3& g_o, d3& g_d) {
    double u, v;
    if (!image_screen_uv(sc, tx.th, tx.tw, o, d, u, v)) return false;
    double s_x = 0.0, s_y = 0.0;
    for (int ch = 0; ch < tx.c; ++ch) {
        double bx, by;
        (void)image_bilinear_grad(tx, u, v, ch, bx, by);
        s_x = ch == 0 ? g_c[ch] * bx : s_x + g_c[ch] * bx;
        s_y = ch == 0 ? g_c[ch] * by : s_y + g_c[ch] * by;
    }
    image_screen_uv_backward(sc, o, d, s_x, s_y, g_o, g_d);
    return true;
}

// Whether a THROUGH sample's seeds exist: image_sample_backward's verdict, from the exit ray alone.
DRT_HD bool image_through_on_screen(const ImageScreen& sc, const ImageTex& tx, d3 exit_o, d3 exit_d) {
    double u, v;
    return image_screen_uv(sc, tx.th, tx.tw, exit_o, exit_d, u, v);
}

}  // namespace drt
