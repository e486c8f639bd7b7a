// drt_paths.h -- one camera ray through a refraction path of up to K surface interactions, with optional internal reflection,
// and its adjoint w.r.t. the vertices (and, as functions of their own, the two indices of refraction).
//
// The path law (opt-in: Scene.render_paths; DESIGN.md "Paths of up to K interactions").  A camera ray repeats:
//   trace   closest hit under the tracer contract (float32 cast of the float64 ray); once K interactions are used up the any-hit form
//   miss    the path ends; it is valid iff it has made an even, non-zero number of refractions
//   hit     before the K-th interaction is used up: bounce_forward on the float64 ray and triangle, unchanged
//             not TIR            -> continues as (new_o, wt), one more refraction
//             TIR, tir = drop    -> the path dies
//             TIR, tir = reflect -> continues mirrored (bounce_reflect), no refraction counted
//   hit     with K interactions used up: invalid
// K = 2 with tir = drop is trace_path (drt_path.h): the same rule through the same device functions, the same bits.
// The third element of the law, the refraction formula (template parameter SNELL of everything below): false, the
// default, is the reference's Refract through bounce_forward / bounce_backward -- today's functions; true bends a refracting hit by
// Snell's law (bounce_forward_snell / bounce_backward_snell).  The TIR flag and the mirror continuation are the same under both.
//
//   trace_path_k              forward; records the face of every interaction and their number
//   path_recompute_backward_k recomputes the path from the camera ray and that face tape, reverses it
//   path_loss_backward_k      the ray_loss term of a completed path and its adjoint in one go (the one-pass form)
//   path_recompute_backward_ior_k / path_loss_backward_ior_k   the same two, also w.r.t. the indices of refraction
// Plain C++ (also compiled by tests/hostsim); the gradient sink is a functor as in drt_path.h.
#pragma once
#include "drt_path.h"

namespace drt {

constexpr int kMaxBounces = 8;

// A miss ends the path: valid iff an even, non-zero number of refractions was made.
DRT_HD bool path_exit_valid(int n_refr) { return n_refr > 0 && (n_refr & 1) == 0; }

// The bounce pair of the law.
template <bool SNELL>
DRT_HD void law_forward(d3 o, d3 d, d3 v0, d3 v1, d3 v2, double ior_ext, double ior_int, Bounce& b) {
    if constexpr (SNELL) bounce_forward_snell(o, d, v0, v1, v2, ior_ext, ior_int, b);
    else bounce_forward(o, d, v0, v1, v2, ior_ext, ior_int, b);
}
template <bool SNELL>
DRT_HD void law_backward(const Bounce& b, d3 g_new_o, d3 g_wt, d3& gv0, d3& gv1, d3& gv2, d3& g_o, d3& g_d) {
    if constexpr (SNELL) bounce_backward_snell(b, g_new_o, g_wt, gv0, gv1, gv2, g_o, g_d);
    else bounce_backward(b, g_new_o, g_wt, gv0, gv1, gv2, g_o, g_d);
}

// One interaction of the law on face `face`: the continuing ray in (o, d), the refraction count bumped.  False: the path dies (TIR, drop).
template <bool SNELL = false>
DRT_HD bool path_interact(const PathCtx& c, int32_t face, bool reflect, d3& o, d3& d, int& n_refr) {
    d3 v0, v1, v2;
    int32_t vid[3];
    Bounce b;
    load_tri64(c, face, v0, v1, v2, vid);
    law_forward<SNELL>(o, d, v0, v1, v2, c.ior_ext, c.ior_int, b);
    if (!b.tir) {
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

// Returns true when the path completes; out_o / out_d are then the exit ray.  faces[0 .. n_hits) are the faces of the interactions that
// took place (also on a path that ends invalid: the caller decides what it reports for those), faces[n_hits .. K) are left alone.
template <bool SNELL = false>
DRT_HD bool trace_path_k(const PathCtx& c, Stack& st, d3 o, d3 d, int max_bounces, bool reflect, int32_t* faces, int& n_hits, d3& out_o, d3& out_d) {
    int n_refr = 0;
    n_hits = 0;
    for (int k = 0; k <= max_bounces; ++k) {
        const Hit h = k < max_bounces ? traverse<false>(c.tc.nodes, c.tc.tris, c.tc.n_tris, to_f32(o), to_f32(d), st)
                                      : traverse<true>(c.tc.nodes, c.tc.tris, c.tc.n_tris, to_f32(o), to_f32(d), st);
        if (h.face < 0) {
            if (!path_exit_valid(n_refr)) return false;
            out_o = o; out_d = d;
            return true;
        }
        if (k == max_bounces) return false;
        faces[k] = h.face;
        n_hits = k + 1;
        if (!path_interact<SNELL>(c, h.face, reflect, o, d, n_refr)) return false;
    }
    return false;
}

// Adjoint of a completed path w.r.t. the vertices: recompute the n_hits interactions from the camera ray and the face tape (element k
// at faces[k * face_stride]; the TIR flags are recomputed, the same bits as in the forward: a set flag on a completed path means the ray
// was mirrored), reverse them, hand the vertex gradients to `add(vertex_id, d3)`.  Only the incoming ray of every interaction is kept
// (6 doubles each); its Bounce (about 45 doubles) is rebuilt right before it is reversed.
template <bool SNELL = false, typename Add>
DRT_HD void path_recompute_backward_k(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 g_ori, d3 g_dir, Add add) {
    d3 ro[kMaxBounces], rd[kMaxBounces];
    d3 v0, v1, v2;
    int32_t vid[3];
    Bounce b;
    if (n_hits > kMaxBounces) n_hits = kMaxBounces;
    for (int k = 0; k < n_hits; ++k) {
        ro[k] = o; rd[k] = d;
        if (k + 1 == n_hits) break;              // (the last interaction is rebuilt by the reverse loop)
        load_tri64(c, faces[k * face_stride], v0, v1, v2, vid);
        law_forward<SNELL>(o, d, v0, v1, v2, c.ior_ext, c.ior_int, b);
        if (b.tir) { d3 no, wr; bounce_reflect(b, o, no, wr); o = no; d = wr; }
        else { o = b.new_o; d = b.wt; }
    }
    const d3 z{0.0, 0.0, 0.0};
    d3 g_o = g_ori, g_d = g_dir;
    for (int k = n_hits - 1; k >= 0; --k) {
        load_tri64(c, faces[k * face_stride], v0, v1, v2, vid);
        law_forward<SNELL>(ro[k], rd[k], v0, v1, v2, c.ior_ext, c.ior_int, b);
        d3 ga = z, gb = z, gc = z, g_o_in, g_d_in;
        if (b.tir) bounce_reflect_backward(b, g_o, g_d, ga, gb, gc, g_o_in, g_d_in);
        else law_backward<SNELL>(b, g_o, g_d, ga, gb, gc, g_o_in, g_d_in);
        add(vid[0], ga); add(vid[1], gb); add(vid[2], gc);
        g_o = g_o_in; g_d = g_d_in;
    }
}

// The one-pass form of a completed path: its ray_loss term (ray_loss_term, drt_shade.h) on the exit ray the forward left behind, and the
// adjoint of that term w.r.t. the vertices with a unit seed (no gradient reaches the exit origin: the loss detaches it).  Returns the term.
template <bool SNELL = false, typename Add>
DRT_HD double path_loss_backward_k(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 exit_o, d3 exit_d,
                                   d3 screen_pixel, Add add) {
    d3 g_dir;
    const double term = ray_loss_term(exit_o, exit_d, screen_pixel, g_dir);
    path_recompute_backward_k<SNELL>(c, o, d, faces, face_stride, n_hits, d3{0.0, 0.0, 0.0}, g_dir, add);
    return term;
}

// ---- the same adjoint, also w.r.t. the two indices of refraction --------------------------------------------------------
// law_backward plus the adjoint of eta of a refracting bounce (bounce_backward_eta / bounce_backward_snell_eta).
template <bool SNELL>
DRT_HD void law_backward_eta(const Bounce& b, d3 g_new_o, d3 g_wt, d3& gv0, d3& gv1, d3& gv2, d3& g_o, d3& g_d, double& g_eta) {
    if constexpr (SNELL) bounce_backward_snell_eta(b, g_new_o, g_wt, gv0, gv1, gv2, g_o, g_d, g_eta);
    else bounce_backward_eta(b, g_new_o, g_wt, gv0, gv1, gv2, g_o, g_d, g_eta);
}

// path_recompute_backward_k -- the same recompute from the face tape, the same vertex gradients handed to `add` in the same order -- that
// also returns d / d (ior_int, ior_ext) (g_int, g_ext; set): every refracting interaction adds its g_eta through eta_to_ior.  A mirrored
// interaction adds nothing: bounce_reflect never reads eta, and the TIR flag and the `entering` branch carry no gradient, as in torch.
template <bool SNELL = false, typename Add>
DRT_HD void path_recompute_backward_ior_k(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 g_ori, d3 g_dir,
                                          Add add, double& g_int, double& g_ext) {
    d3 ro[kMaxBounces], rd[kMaxBounces];
    d3 v0, v1, v2;
    int32_t vid[3];
    Bounce b;
    g_int = 0.0; g_ext = 0.0;
    if (n_hits > kMaxBounces) n_hits = kMaxBounces;
    for (int k = 0; k < n_hits; ++k) {
        ro[k] = o; rd[k] = d;
        if (k + 1 == n_hits) break;              // (the last interaction is rebuilt by the reverse loop)
        load_tri64(c, faces[k * face_stride], v0, v1, v2, vid);
        law_forward<SNELL>(o, d, v0, v1, v2, c.ior_ext, c.ior_int, b);
        if (b.tir) { d3 no, wr; bounce_reflect(b, o, no, wr); o = no; d = wr; }
        else { o = b.new_o; d = b.wt; }
    }
    const d3 z{0.0, 0.0, 0.0};
    d3 g_o = g_ori, g_d = g_dir;
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
        }
        add(vid[0], ga); add(vid[1], gb); add(vid[2], gc);
        g_o = g_o_in; g_d = g_d_in;
    }
}

// path_loss_backward_k that also returns the IOR partials of the term (unit seed; set).
template <bool SNELL = false, typename Add>
DRT_HD double path_loss_backward_ior_k(const PathCtx& c, d3 o, d3 d, const int32_t* faces, int64_t face_stride, int n_hits, d3 exit_o, d3 exit_d,
                                       d3 screen_pixel, Add add, double& g_int, double& g_ext) {
    d3 g_dir;
    const double term = ray_loss_term(exit_o, exit_d, screen_pixel, g_dir);
    path_recompute_backward_ior_k<SNELL>(c, o, d, faces, face_stride, n_hits, d3{0.0, 0.0, 0.0}, g_dir, add, g_int, g_ext);
    return term;
}

}  // namespace drt
