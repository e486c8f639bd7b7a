// tests/hostsim/image.cpp -- drt_amd/csrc/drt_image.h compiled for the host (g++ -ffp-contract=off): the per-sample bodies of
// k_image_start / k_image_shade / k_image_resolve that need no tracer -- sample rays, the Fresnel term, the screen plane, the bilinear
// fetch and a sample's colour -- run over arrays in plain loops.  Test-only.
#include "../../drt_amd/csrc/drt_image.h"

using namespace drt;

namespace {
ImageCam cam_of(const double* cam21) {
    ImageCam c;
    memcpy(c.kinv, cam21, sizeof(double) * 9);
    memcpy(c.rinv, cam21 + 9, sizeof(double) * 12);
    return c;
}
ImageScreen screen_of(const double* s9) { return ImageScreen{d3{s9[0], s9[1], s9[2]}, d3{s9[3], s9[4], s9[5]}, d3{s9[6], s9[7], s9[8]}}; }
}  // namespace

extern "C" {

// origin / dir float64 [H * W * s * s, 3], pixel-major, sample-minor
void image_rays(const double* cam21, int H, int W, int s, double* origin, double* dir) {
    const ImageCam cam = cam_of(cam21);
    int64_t i = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int j = 0; j < s * s; ++j, ++i) {
                d3 o, d;
                image_sample_ray(cam, s, x, y, j, o, d);
                store_d3(origin, i, o);
                store_d3(dir, i, d);
            }
}

void image_fresnel(const double* ci, const double* eta_i, const double* eta_t, int64_t n, double* R) {
    for (int64_t i = 0; i < n; ++i) R[i] = fresnel_R(ci[i], eta_i[i], eta_t[i]);
}

// the factor of an interaction with the given TIR flag (image_transmittance reads tir, sg and ci of the bounce only)
double image_factor(int tir, double sg, double ci, double ior_ext, double ior_int) {
    Bounce b{};
    b.tir = tir != 0; b.sg = sg; b.ci = ci;
    return image_transmittance(b, ior_ext, ior_int);
}

int image_axes_ok(const double* s9) { return image_screen_ok(screen_of(s9)) ? 1 : 0; }

// per sample: cls int32, exit ray, throughput -> colour float64 [n, C], on uint8 [n], uv float64 [n, 2] (written where on)
void image_colours(const double* s9, const float* texel, int th, int tw, int c, const int32_t* cls, const double* o, const double* d, const double* T,
                   int64_t n, const double* fill_void, const double* fill_invalid, double* colour, uint8_t* on, double* uv) {
    const ImageScreen sc = screen_of(s9);
    const ImageTex tx{texel, th, tw, c};
    for (int64_t i = 0; i < n; ++i) {
        image_sample_colour(sc, tx, cls[i], load_d3(o, i), load_d3(d, i), T[i], fill_void, fill_invalid, colour + i * c);
        double u = 0.0, v = 0.0;
        on[i] = cls[i] != kImageInvalid && image_screen_uv(sc, th, tw, load_d3(o, i), load_d3(d, i), u, v);
        if (on[i]) { uv[2 * i] = u; uv[2 * i + 1] = v; }
    }
}

}  // extern "C"
