// drt_decode.h -- Gray-code pattern photographs -> per-pixel screen codes, silhouette mask and ray targets.
// Plain C++ like the other device math headers, so that tests/hostsim/decode.cpp runs the same bodies on the host against the numpy
// restatement (tests/decode_ref.py) with tolerance 0: everything but the position is integer arithmetic, and the position is one float64
// expression with one rounding per operation in the stated association (the library is built with -ffp-contract=off).
//
// Patterns of a screen of tex_w x tex_h texels (2 <= tex_w, tex_h <= 32768): nbx = ceil(log2 tex_w), nby = ceil(log2 tex_h), each at
// least 1.  Frame 2k (k < nbx) shows at texel column x the bit nbx - 1 - k of g(x) = x ^ (x >> 1), white = 1, constant along y; frame
// 2k + 1 is its complement; frames 2 (nbx + k) and 2 (nbx + k) + 1 are the same for rows with nby.  F = 2 (nbx + nby) <= 60 frames.
#pragma once
#include "drt_common.h"

namespace drt {

constexpr int kDecodeMaxTex = 32768;
constexpr int kDecodeMaxFrames = 60;

struct DecodeLaw {
    int tex_w, tex_h;
    int nbx, nby;           // bits of a column / row code
    int min_contrast;       // 1..255: a pixel decodes only when every bit's |a - b| reaches it
    int mask_shift;         // >= 1: object when the decoded texel moved this far (Chebyshev) from the background's
};

DRT_HD int decode_bits(int n) {                                     // ceil(log2 n), at least 1
    int b = 1;
    while ((1 << b) < n) ++b;
    return b;
}
DRT_HD int decode_frames(int tex_h, int tex_w) { return 2 * (decode_bits(tex_w) + decode_bits(tex_h)); }
DRT_HD DecodeLaw decode_law(int tex_h, int tex_w, int min_contrast, int mask_shift) {
    return DecodeLaw{tex_w, tex_h, decode_bits(tex_w), decode_bits(tex_h), min_contrast, mask_shift};
}

// What frame f shows at texel (x, y): 0 or 255.
DRT_HD uint8_t decode_pattern(const DecodeLaw& L, int f, int x, int y) {
    const int k = f >> 1;
    const unsigned v = (unsigned)(k < L.nbx ? x : y);
    const int bit = k < L.nbx ? L.nbx - 1 - k : L.nby - 1 - (k - L.nbx);
    const unsigned on = (((v ^ (v >> 1)) >> bit) & 1u) ^ (unsigned)(f & 1);
    return on ? 255 : 0;
}

// One bit of one pixel: a = the pattern frame's byte, b = the complement's.  The bits enter `gray` most significant first, the column
// code and then the row code, nbx + nby <= 30 of them; `contrast` starts at 255 and keeps the smallest |a - b|.
DRT_HD void decode_bit(unsigned& gray, int& contrast, int a, int b) {
    gray = (gray << 1) | (unsigned)(a > b);
    const int c = a > b ? a - b : b - a;
    contrast = c < contrast ? c : contrast;
}

DRT_HD unsigned decode_gray_to_binary(unsigned g) {                  // prefix XOR of at most 16 bits
    g ^= g >> 1;
    g ^= g >> 2;
    g ^= g >> 4;
    g ^= g >> 8;
    return g;
}

// The code of a pixel from its accumulated bits: true when it decodes; (-1, -1) otherwise.
DRT_HD bool decode_code(const DecodeLaw& L, unsigned gray, int contrast, int& x, int& y) {
    x = (int)decode_gray_to_binary(gray >> L.nby);
    y = (int)decode_gray_to_binary(gray & ((1u << L.nby) - 1u));
    const bool ok = contrast >= L.min_contrast && x < L.tex_w && y < L.tex_h;
    if (!ok) x = y = -1;
    return ok;
}

// Object (255) iff the background decodes and the object frames do not, or decode to a texel at least mask_shift away.
DRT_HD uint8_t decode_mask(const DecodeLaw& L, bool ok, int x, int y, bool okb, int xb, int yb) {
    if (!okb) return 0;
    if (!ok) return 255;
    const int dx = x > xb ? x - xb : xb - x, dy = y > yb ? y - yb : yb - y;
    return (dx > dy ? dx : dy) >= L.mask_shift ? 255 : 0;
}

// (p0 + x eu) + y ev per component of screen = p0, eu, ev; an x component that is exactly 0 becomes 1e-12 (it would read as invalid).
DRT_HD void decode_position(const double* __restrict__ screen, int x, int y, double out[3]) {
    for (int c = 0; c < 3; ++c) out[c] = (screen[c] + (double)x * screen[3 + c]) + (double)y * screen[6 + c];
    if (out[0] == 0.0) out[0] = 1e-12;
}

// The decoded stack of one pixel, byte by byte: frames points at the pixel's byte in frame 0, consecutive frames lie `plane` bytes apart.
// k_decode_patterns computes the same from wide loads of a run of pixels.
DRT_HD bool decode_pixel(const DecodeLaw& L, const uint8_t* __restrict__ frames, int64_t plane, int& x, int& y, int& contrast) {
    unsigned gray = 0;
    contrast = 255;
    for (int t = 0; t < L.nbx + L.nby; ++t) decode_bit(gray, contrast, frames[(int64_t)(2 * t) * plane], frames[(int64_t)(2 * t + 1) * plane]);
    return decode_code(L, gray, contrast, x, y);
}

}  // namespace drt
