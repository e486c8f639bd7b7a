// drt_image.h -- the forward renderer's law ("the refracted image"): what a pinhole camera sees of a textured
// planar screen through the glass object.  A pixel is the mean of s x s sample rays; a sample is traced through the K-interaction path
// law of drt_paths.h (unchanged), carries a Fresnel throughput, and its exit ray samples the screen's texture bilinearly.
// Plain C++ like the other device math headers, so that tests/hostsim/image.cpp runs the same bodies on the host against the numpy
// restatement (tests/image_ref.py) with tolerance 0: every float64 expression below is one rounding per operation in the stated
// association (the library is built with -ffp-contract=off).  Forward only: nothing here has an adjoint.  Each function is stated once
// for clear and for absorbing glass (drt_image_absorb.h states that law): the clear forms never evaluate an exp.
#pragma once
#include "drt_paths.h"

namespace drt {

struct ImageCam {
    double kinv[9];     // K^-1, row-major
    double rinv[12];    // top 3 x 4 of R^-1 (camera -> world), row-major; its last column is the camera position
};
struct ImageScreen {
    d3 p0;              // world position of texel (0, 0)
    d3 eu, ev;          // world vectors of one texel step along the texture's x and y (orthogonal)
};
struct ImageTex {
    const float* texel; // float32 [th, tw, c]
    int th, tw, c;      // th, tw >= 2; c in {1, 3}
};

constexpr int kImageMaxSuper = 4;          // s in 1 .. 4
constexpr int kImageMaxChannels = 3;
enum : int { kImageDirect = 0, kImageThrough = 1, kImageInvalid = 2 };

// Sample j = b * s + a of pixel (x, y) looks through (x + (a + 0.5) / s - 0.5, y + (b + 0.5) / s - 0.5): at s = 1 the integer pixel
// centre of views.generate_ray.  dir = normalize(R^-1[:3, :3] (K^-1 (px, py, 1))), origin = the camera position.
DRT_HD void image_sample_ray(const ImageCam& cam, int s, int x, int y, int j, d3& origin, d3& dir) {
    const int a = j % s, b = j / s;
    const double px = ((double)x + ((double)a + 0.5) / (double)s) - 0.5;
    const double py = ((double)y + ((double)b + 0.5) / (double)s) - 0.5;
    const double* K = cam.kinv;
    const double* R = cam.rinv;
    const double p0 = (K[0] * px + K[1] * py) + K[2];
    const double p1 = (K[3] * px + K[4] * py) + K[5];
    const double p2 = (K[6] * px + K[7] * py) + K[8];
    const d3 w{(R[0] * p0 + R[1] * p1) + R[2] * p2, (R[4] * p0 + R[5] * p1) + R[6] * p2, (R[8] * p0 + R[9] * p1) + R[10] * p2};
    dir = w / sqrt((w.x * w.x + w.y * w.y) + w.z * w.z);
    origin = d3{R[3], R[7], R[11]};
}

// The reference's FrDielectric (DiffRender.py:51-61), line by line: the unpolarised Fresnel reflectance of Snell's law.  The reference
// computes it and drops it; here 1 - R weights a refracting interaction.  Not called on an interaction whose TIR flag is set.
DRT_HD double fresnel_R(double ci, double eta_i, double eta_t) {
    double x = 1.0 - ci * ci;
    x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);
    const double sin_i = sqrt(x);
    const double sin_t = sin_i * eta_i / eta_t;
    const double y = 1.0 - sin_t * sin_t;
    const double cos_t = sqrt(y < 0.0 ? 0.0 : y);
    const double r_parl = ((eta_t * ci) - (eta_i * cos_t)) / ((eta_t * ci) + (eta_i * cos_t));
    const double r_perp = ((eta_i * ci) - (eta_t * cos_t)) / ((eta_i * ci) + (eta_t * cos_t));
    return (r_parl * r_parl + r_perp * r_perp) / 2.0;
}

// The factor an interaction puts on the throughput: 1 - R with cos(theta_i) from the flipped normal (Bounce::ci) and the eta_i, eta_t
// refract_ray assigned (Bounce::sg: 1 = entering); a mirrored (TIR) interaction leaves the throughput alone and never evaluates R.
DRT_HD double image_transmittance(const Bounce& b, double ior_ext, double ior_int) {
    if (b.tir) return 1.0;
    const bool entering = b.sg > 0.0;
    return 1.0 - fresnel_R(b.ci, entering ? ior_ext : ior_int, entering ? ior_int : ior_ext);
}

// Absorbing glass (drt_image_absorb.h states the law).  What an interaction adds to the interior length: L + t when
// its incoming ray travelled inside the object, L otherwise.
DRT_HD double image_absorb_length(const Bounce& b, double L) { return b.sg < 0.0 ? L + b.t : L; }

// A_ch = exp(-(sigma_ch * L))
DRT_HD double image_absorb_factor(double sigma, double L) { return exp(-(sigma * L)); }

// The length hook of clear glass: nothing.
struct ImageNoLength { DRT_HD void operator()(const Bounce&) const {} };

// path_interact (drt_paths.h) -- the same continuation, the same bits -- that also multiplies the throughput T when FRESNEL is on, and
// hands the bounce to `length` right behind law_forward, before the throughput: an absorbing caller adds image_absorb_length to the
// interior length it keeps (a kernel does so in memory at once, so that no length is held in registers across the Fresnel term).
template <bool SNELL, bool FRESNEL, typename Length = ImageNoLength>
DRT_HD bool image_interact(const PathCtx& c, int32_t face, bool reflect, d3& o, d3& d, int& n_refr, double& T, Length length = Length{}) {
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

// The three classes of a sample.  direct: no interaction at all (its exit ray is the camera ray, T = 1); through: the path completed
// validly (the path's exit ray, T as carried); invalid: everything else.
DRT_HD int image_class(bool hit, bool completed) { return !hit ? kImageDirect : (completed ? kImageThrough : kImageInvalid); }

// Orthogonal, non-zero axes: |dot(eu, ev)| <= 1e-12 |eu| |ev|.
DRT_HD bool image_screen_ok(const ImageScreen& sc) {
    const double lu = sqrt(dot(sc.eu, sc.eu)), lv = sqrt(dot(sc.ev, sc.ev));
    if (!(lu > 0.0 && lv > 0.0) || !(lu < INFINITY && lv < INFINITY)) return false;
    const double c = dot(sc.eu, sc.ev);
    return (c < 0.0 ? -c : c) <= 1e-12 * lu * lv;
}

// Where the exit ray (o, d) meets the screen, in texel units.  False: the sample does not see the screen (parallel, behind, or NaN) or
// lands outside [0, tw - 1] x [0, th - 1] (texel centres at the integers); its colour is `void`.  The screen has two faces.
DRT_HD bool image_screen_uv(const ImageScreen& sc, int th, int tw, d3 o, d3 d, double& u, double& v) {
    const d3 n = cross(sc.eu, sc.ev);
    const double dn = dot(d, n);
    if (!(dn != 0.0)) return false;
    const double t = dot(sc.p0 - o, n) / dn;
    if (!(t > 0.0)) return false;
    const d3 q = o + t * d;
    const d3 r = q - sc.p0;
    u = dot(r, sc.eu) / dot(sc.eu, sc.eu);
    v = dot(r, sc.ev) / dot(sc.ev, sc.ev);
    return u >= 0.0 && u <= (double)(tw - 1) && v >= 0.0 && v <= (double)(th - 1);
}

// Bilinear sample of channel ch at (u, v) inside the texture, the visual hull's formula (drt_hull.h hull_view_sample) in float64.
DRT_HD double image_bilinear(const ImageTex& tx, double u, double v, int ch) {
    double x0 = floor(u), y0 = floor(v);
    if (x0 > (double)(tx.tw - 2)) x0 = (double)(tx.tw - 2);
    if (y0 > (double)(tx.th - 2)) y0 = (double)(tx.th - 2);
    const double fx = u - x0, fy = v - y0;
    const float* row = tx.texel + ((int64_t)y0 * tx.tw + (int64_t)x0) * tx.c + ch;     // 0 <= x0 <= tw - 2, 0 <= y0 <= th - 2: all four reads inside
    const int64_t down = (int64_t)tx.tw * tx.c;
    const double t00 = (double)row[0], t01 = (double)row[tx.c], t10 = (double)row[down], t11 = (double)row[down + tx.c];
    return ((t00 * (1.0 - fx) + t01 * fx) * (1.0 - fy)) + ((t10 * (1.0 - fx) + t11 * fx) * fy);
}

// Colour of one sample, c[0 .. tx.c): `invalid` for an invalid one; for a direct or through one T times the texture where its exit ray
// lands on the screen, `void` elsewhere.  The fill colours are not weighted.  ABSORB: (A_ch * T) times the texture, A_ch from the
// interior length L and sigma[0 .. tx.c).  True: the sample is direct or through and landed on the screen (its colour is a function of
// T and L); false: c is a fill.
template <bool ABSORB = false>
DRT_HD bool image_sample_colour(const ImageScreen& sc, const ImageTex& tx, int cls, d3 o, d3 d, double T, const double* fill_void,
                                const double* fill_invalid, double* c, double L = 0.0, const double* sigma = nullptr) {
    if (cls == kImageInvalid) {
        for (int ch = 0; ch < tx.c; ++ch) c[ch] = fill_invalid[ch];
        return false;
    }
    double u, v;
    if (!image_screen_uv(sc, tx.th, tx.tw, o, d, u, v)) {
        for (int ch = 0; ch < tx.c; ++ch) c[ch] = fill_void[ch];
        return false;
    }
    if constexpr (ABSORB) {
        for (int ch = 0; ch < kImageMaxChannels; ++ch)          // (a fixed trip count: the three colours stay in registers on the device)
            if (ch < tx.c) c[ch] = (image_absorb_factor(sigma[ch], L) * T) * image_bilinear(tx, u, v, ch);
    } else {
        for (int ch = 0; ch < tx.c; ++ch) c[ch] = T * image_bilinear(tx, u, v, ch);
    }
    return true;
}

}  // namespace drt
