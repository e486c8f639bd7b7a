// drt_image_env_param.h -- the gradients of the photometric loss of the refracted image w.r.t. the environment's texels and rotation
// (Scene.image_loss_fused with env_texels_param / env_rotation_param, drt_render_image_loss_env_param).  The
// forward law and the loss are drt_image_env.h's and drt_image_loss.h's, unchanged; this header states what the environment itself receives.
//   reads    a sample reads the environment along a direction d with a weight w in up to two ways:
//            exit        a DIRECT sample along its camera ray (w = 1), a THROUGH sample along its parked exit ray (w = T; 1 without the
//                        Fresnel term) -- where no screen is given or image_screen_uv does not put that ray on it
//            reflection  a THROUGH sample with the bit kImageReflectSeen, along wr of (ro, wr, R1) = image_reflect_first on the tape's row 0
//                        (w = R1) -- where the screen does not catch (ro, wr)
//            An invalid sample reads nothing.  One sample can contribute twice.
//   texels   the gradient w.r.t. (double)texel: with (cell, fx, fy) = image_env_cell of image_env_uv(d) and the pixel's seeds g_c, texel
//            (y0, xa), (y0, xb), (y0 + 1, xa), (y0 + 1, xb) of channel ch receive (g_c[ch] w) times (1 - fx)(1 - fy), fx (1 - fy),
//            (1 - fx) fy, fx fy; xa, xb are the wrapped columns, so a read across the seam lands in columns Ew - 1 and 0
//   rotation the gradient w.r.t. the nine entries of env.rot as nine independent inputs, row-major: g_u = w sum_ch g_c[ch] dE/dfx, g_v
//            likewise and 0 where v left its clamp (image_env_bilinear_grad), g_e = image_env_uv_seed (the seed of the direction in the
//            environment frame: what image_env_uv_backward multiplies by R^T), g_R[r][c] = g_e[r] d[c]
// No gradient: the test that puts a ray on the screen, the cell, the wrap column, the clamp of v, the orthonormality check, the occlusion
// verdict, the class, and d itself (the vertex and IOR gradients are drt_image_env.h's).  A pole gives the torch forms, inf or NaN.
// Plain C++ like drt_image_env.h: float64, one rounding per operation in the association written (tests/hostsim/image_env_param.cpp runs
// these bodies on the host against tests/image_env_param_ref.py).
#pragma once
#include "drt_image_env.h"

namespace drt {

// One read of the environment along d with weight w under the seeds g_c[0 .. e.c): add_texel(texel number y * Ew + x, gt[0 .. e.c)) four
// times; g_R[0 .. 9) is SET.
template <typename AddTexel>
DRT_HD void image_env_read_backward(const ImageEnv& e, d3 d, double w, const double* g_c, AddTexel add_texel, double* g_R) {
    double u, v;
    image_env_uv(e, d, u, v);
    const ImageEnvCell cell = image_env_cell(e, u, v);
    double gw[kImageMaxChannels] = {0.0, 0.0, 0.0}, gt[kImageMaxChannels] = {0.0, 0.0, 0.0};
    double s_x = 0.0, s_y = 0.0;
    for (int ch = 0; ch < e.c; ++ch) {
        double bx, by;
        image_env_bilinear_grad(e, cell, ch, bx, by);
        s_x = ch == 0 ? g_c[ch] * bx : s_x + g_c[ch] * bx;
        s_y = ch == 0 ? g_c[ch] * by : s_y + g_c[ch] * by;
        gw[ch] = g_c[ch] * w;
    }
    const int32_t up = (int32_t)cell.y0 * e.ew, down = up + e.ew;
    const double w00 = (1.0 - cell.fx) * (1.0 - cell.fy), w01 = cell.fx * (1.0 - cell.fy), w10 = (1.0 - cell.fx) * cell.fy, w11 = cell.fx * cell.fy;
    for (int ch = 0; ch < e.c; ++ch) gt[ch] = gw[ch] * w00;
    add_texel(up + cell.xa, gt);
    for (int ch = 0; ch < e.c; ++ch) gt[ch] = gw[ch] * w01;
    add_texel(up + cell.xb, gt);
    for (int ch = 0; ch < e.c; ++ch) gt[ch] = gw[ch] * w10;
    add_texel(down + cell.xa, gt);
    for (int ch = 0; ch < e.c; ++ch) gt[ch] = gw[ch] * w11;
    add_texel(down + cell.xb, gt);
    const d3 g_e = image_env_uv_seed(e, image_env_dir(e, d), w * s_x, cell.v_inside ? w * s_y : 0.0);
    g_R[0] = g_e.x * d.x; g_R[1] = g_e.x * d.y; g_R[2] = g_e.x * d.z;
    g_R[3] = g_e.y * d.x; g_R[4] = g_e.y * d.y; g_R[5] = g_e.y * d.z;
    g_R[6] = g_e.z * d.x; g_R[7] = g_e.z * d.y; g_R[8] = g_e.z * d.z;
}

// ... of a ray (o, d) in front of a screen (has_screen) and the environment: false, and nothing added, where the screen catches the ray.
template <typename AddTexel>
DRT_HD bool image_env_ray_backward(const ImageScreen& sc, const ImageTex& tx, bool has_screen, const ImageEnv& e, d3 o, d3 d, double w, const double* g_c,
                                   AddTexel add_texel, double* g_R) {
    double u, v;
    if (has_screen && image_screen_uv(sc, tx.th, tx.tw, o, d, u, v)) return false;
    image_env_read_backward(e, d, w, g_c, add_texel, g_R);
    return true;
}

}  // namespace drt
