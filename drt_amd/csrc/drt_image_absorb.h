// drt_image_absorb.h -- absorbing glass: Beer-Lambert attenuation in the refracted image and in its photometric loss (DESIGN.md section
// 10.7; Scene.render_image / Scene.image_loss_fused with `absorption`, drt_render_image_absorb, drt_render_image_loss_absorb).
//   sigma[C]  one absorption coefficient per texture channel, per unit of mesh length: float64, finite, >= 0
//   L         the interior length of a sample: ((t_1 + t_2) + ...) in interaction order over the interactions whose incoming ray
//             travelled inside the object (Bounce::sg < 0, refracting or mirrored), t the Bounce::t law_forward<SNELL> leaves -- both laws
//             fill t and sg through bounce_forward's own statements (bounce_forward_snell calls it first).  A direct sample has L = 0
//   A_ch      exp(-(sigma_ch * L))
//   c[ch]     (A_ch * T) * bilinear_ch for a through or direct sample on the screen; the fills are not weighted
// Every other forward quantity is drt_image.h's.  With every sigma_ch = 0, A_ch = exp(-0) = 1 and (1 * T) * B has the bits of T * B.
// The adjoint adds to drt_image_loss.h's one seed: g_L = sum_ch g_c[ch] * (-sigma_ch) * c[ch], handed to the t of every interior
// interaction (bounce_t_backward), from where it reaches the vertices, the incoming ray and, through the existing chain of the earlier
// interactions, the IORs.  d loss / d sigma_ch = -g_c[ch] * sum_j L_j * c_j[ch] over a pixel's through samples on the screen needs forward
// values only.  Class, faces, TIR flags, sg, the texel cell and the screen border carry no gradient, as in 10.3.
// No body of the law is here.  What absorption adds sits where the law functions that take it in are stated, once for clear and absorbing
// glass: image_absorb_length, image_absorb_factor, image_interact's length hook and image_sample_colour<ABSORB> in drt_image.h;
// bounce_t_backward, image_absorb_sigma_term and the flag LENGTH of image_path_backward / image_sample_backward in drt_image_loss.h.
// Below: the absorbing forms under the names and argument orders the law has (A, T, L, sigma together), each one call of the shared
// function -- what tests/hostsim/image_absorb.cpp runs on the host against tests/image_absorb_ref.py.  The kernels call the shared
// functions directly and do not include this header.
#pragma once
#include "drt_image_loss.h"

namespace drt {

// image_interact with the length hook required: the caller adds image_absorb_length to the interior length it keeps.
template <bool SNELL, bool FRESNEL, typename Length>
DRT_HD bool image_absorb_interact(const PathCtx& c, int32_t face, bool reflect, d3& o, d3& d, int& n_refr, double& T, Length length) {
    return image_interact<SNELL, FRESNEL>(c, face, reflect, o, d, n_refr, T, length);
}

// image_sample_colour<true>: c[ch] = (A_ch * T) * B_ch on the screen.
DRT_HD bool image_absorb_sample_colour(const ImageScreen& sc, const ImageTex& tx, int cls, d3 o, d3 d, double T, double L, const double* sigma,
                                       const double* fill_void, const double* fill_invalid, double* c) {
    return image_sample_colour<true>(sc, tx, cls, o, d, T, fill_void, fill_invalid, c, L, sigma);
}

// image_sample_backward with LENGTH and without seed outputs.
template <bool SNELL, bool FRESNEL, typename Add>
DRT_HD bool image_sample_backward_absorb(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 exit_o, d3 exit_d, double T,
                                         double L, const double* sigma, const ImageScreen& sc, const ImageTex& tx, const double* g_c, Add add,
                                         double& g_int, double& g_ext) {
    return image_sample_backward<SNELL, FRESNEL, true>(c, o, d, faces, face_stride, n_hits, exit_o, exit_d, T, sc, tx, g_c, add, g_int, g_ext, nullptr, nullptr, L,
                                                       sigma);
}

}  // namespace drt
