// tests/hostsim/decode.cpp -- drt_amd/csrc/drt_decode.h compiled for the host (g++ -ffp-contract=off): the per-pixel bodies of
// k_decode_patterns run over whole stacks in plain loops, byte by byte.  Test-only.
#include "../../drt_amd/csrc/drt_decode.h"

using namespace drt;

extern "C" {

int decode_n_frames(int tex_h, int tex_w) { return decode_frames(tex_h, tex_w); }

// out uint8 [F, tex_h, tex_w]
void decode_patterns(int tex_h, int tex_w, uint8_t* out) {
    const DecodeLaw L = decode_law(tex_h, tex_w, 1, 1);
    const int F = decode_frames(tex_h, tex_w);
    for (int f = 0; f < F; ++f)
        for (int y = 0; y < tex_h; ++y)
            for (int x = 0; x < tex_w; ++x) out[((int64_t)f * tex_h + y) * tex_w + x] = decode_pattern(L, f, x, y);
}

// The arguments of drt_decode_patterns, on host arrays.
void decode_host(const uint8_t* frames, const uint8_t* background, int64_t background_view_stride, int n_views, int height, int width, int tex_h,
                 int tex_w, int min_contrast, int mask_shift, const double* screens, int zero_outside_mask, int16_t* codes, uint8_t* contrast,
                 uint8_t* mask, uint8_t* covered, double* positions) {
    const DecodeLaw L = decode_law(tex_h, tex_w, min_contrast, mask_shift);
    const int64_t plane = (int64_t)height * width, view_bytes = (int64_t)decode_frames(tex_h, tex_w) * plane;
    for (int v = 0; v < n_views; ++v)
        for (int64_t p = 0; p < plane; ++p) {
            const int64_t pix = v * plane + p;
            int x, y, c;
            const bool ok = decode_pixel(L, frames + v * view_bytes + p, plane, x, y, c);
            codes[2 * pix] = (int16_t)x;
            codes[2 * pix + 1] = (int16_t)y;
            contrast[pix] = (uint8_t)c;
            uint8_t m = 255;
            if (background) {
                int xb, yb, cb;
                const bool okb = decode_pixel(L, background + v * background_view_stride + p, plane, xb, yb, cb);
                m = decode_mask(L, ok, x, y, okb, xb, yb);
                if (mask) mask[pix] = m;
                if (covered) covered[pix] = okb ? 1 : 0;
            }
            if (positions) {
                double q[3] = {0.0, 0.0, 0.0};
                if (ok && !(zero_outside_mask && m == 0)) decode_position(screens + 9 * v, x, y, q);
                for (int k = 0; k < 3; ++k) positions[3 * pix + k] = q[k];
            }
        }
}

}  // extern "C"
