// tests/hostsim/paths_ior.cpp -- host harness for the IOR adjoint of the K-interaction path law.  TEST ONLY.
//
// Compiles drt_shade.h / drt_paths.h (the code k_paths_loss_bwd_ior of drt_paths.hip inlines) with g++ and drives
//   bounce_backward_snell_eta / bounce_backward_eta + eta_to_ior   one refracting bounce per row                          (pi_bounce)
//   path_recompute_backward_ior_k                                  one interaction per row, mirrored where its flag is set (pi_interaction)
//   trace_path_k<SNELL>                                            camera rays through the host BVH                        (pi_trace)
//   path_loss_backward_ior_k beside path_loss_backward_k           ray_loss term + adjoints of those paths                 (pi_loss_backward)
//   path_recompute_backward_inputs                                 the two-bounce route of drt_path.h on the same paths    (pi_two_bounce)
// with sequential loops, so tests/test_paths_ior_host.py can hold them against torch autograd of tests/ior_ref.py.
#include <cstring>

#include "hostsim.cpp"

#include "../../drt_amd/csrc/drt_paths.h"

static bool same_bits(d3 a, d3 b) { return memcmp(&a, &b, sizeof(d3)) == 0; }

extern "C" {

// One bounce per row: o, d [n,3], tri [n,3,3], incoming adjoints g_new_o, g_wt [n,3].  snell != 0: bounce_forward_snell +
// bounce_backward_snell_eta, else bounce_forward + bounce_backward_eta -- run on every row, flagged or not.  Out: tir, ct, g_eta, g_int,
// g_ext [n] (eta_to_ior into zeros).  Returns the number of rows whose vertex / ray adjoints differ in any bit from the pair without eta.
int64_t pi_bounce(const double* o, const double* d, const double* tri, int64_t n, double ior_int, double ior_ext, int snell,
                  const double* g_new_o, const double* g_wt, uint8_t* tir, double* ct, double* g_eta, double* g_int, double* g_ext) {
    int64_t differ = 0;
    for (int64_t i = 0; i < n; ++i) {
        Bounce b;
        const d3 v0 = load_d3(tri, 3 * i), v1 = load_d3(tri, 3 * i + 1), v2 = load_d3(tri, 3 * i + 2);
        if (snell) bounce_forward_snell(load_d3(o, i), load_d3(d, i), v0, v1, v2, ior_ext, ior_int, b);
        else bounce_forward(load_d3(o, i), load_d3(d, i), v0, v1, v2, ior_ext, ior_int, b);
        tir[i] = b.tir ? 1 : 0;
        ct[i] = b.ct;
        d3 ga{0, 0, 0}, gb{0, 0, 0}, gc{0, 0, 0}, go, gd, ha{0, 0, 0}, hb{0, 0, 0}, hc{0, 0, 0}, ho, hd;
        double ge = 0.0;
        if (snell) {
            bounce_backward_snell_eta(b, load_d3(g_new_o, i), load_d3(g_wt, i), ga, gb, gc, go, gd, ge);
            bounce_backward_snell(b, load_d3(g_new_o, i), load_d3(g_wt, i), ha, hb, hc, ho, hd);
        } else {
            bounce_backward_eta(b, load_d3(g_new_o, i), load_d3(g_wt, i), ga, gb, gc, go, gd, ge);
            bounce_backward(b, load_d3(g_new_o, i), load_d3(g_wt, i), ha, hb, hc, ho, hd);
        }
        if (!(same_bits(ga, ha) && same_bits(gb, hb) && same_bits(gc, hc) && same_bits(go, ho) && same_bits(gd, hd))) ++differ;
        g_eta[i] = ge;
        g_int[i] = 0.0; g_ext[i] = 0.0;
        eta_to_ior(b, ior_int, ior_ext, ge, g_int[i], g_ext[i]);
    }
    return differ;
}

// One interaction per row through the path function: row i is a "path" of one hit on its own triangle, reversed with the incoming
// adjoints g_o, g_d [n,3].  Out: tir [n], g_int, g_ext [n], g_tri [n,3,3].
void pi_interaction(const double* o, const double* d, const double* tri, int64_t n, double ior_int, double ior_ext, int snell,
                    const double* g_o, const double* g_d, uint8_t* tir, double* g_int, double* g_ext, double* g_tri) {
    const int32_t faces[3] = {0, 1, 2};
    const int32_t tape[1] = {0};
    for (int64_t i = 0; i < n; ++i) {
        const PathCtx c{TraceCtx{nullptr, nullptr, 0, nullptr}, faces, tri + 9 * i, ior_int, ior_ext};
        double* out = g_tri + 9 * i;
        for (int k = 0; k < 9; ++k) out[k] = 0.0;
        auto add = [out](int32_t v, d3 a) { store_d3(out, v, load_d3(out, v) + a); };
        Bounce b;
        bounce_forward(load_d3(o, i), load_d3(d, i), load_d3(tri, 3 * i), load_d3(tri, 3 * i + 1), load_d3(tri, 3 * i + 2), ior_ext, ior_int, b);
        tir[i] = b.tir ? 1 : 0;
        if (snell) path_recompute_backward_ior_k<true>(c, load_d3(o, i), load_d3(d, i), tape, 1, 1, load_d3(g_o, i), load_d3(g_d, i), add, g_int[i], g_ext[i]);
        else path_recompute_backward_ior_k<false>(c, load_d3(o, i), load_d3(d, i), tape, 1, 1, load_d3(g_o, i), load_d3(g_d, i), add, g_int[i], g_ext[i]);
    }
}

// trace_path_k<SNELL> of every ray through the host BVH: the outputs of sn_trace (tests/hostsim/snell_adjoint.cpp), under either formula.
void pi_trace(void* h, const double* verts64, const double* origin, const double* dir, int64_t n, double ior_int, double ior_ext,
              int max_bounces, int reflect, int snell, double* out_ori, double* out_dir, uint8_t* mask, int32_t* tape, uint8_t* hits) {
    HsScene* s = (HsScene*)h;
    const PathCtx c = path_ctx(s, verts64, ior_int, ior_ext);
    HostStack hs;
    for (int64_t i = 0; i < n; ++i) {
        int32_t faces[kMaxBounces];
        int n_hits = 0;
        d3 oo{0, 0, 0}, od{0, 0, 0};
        const bool ok = snell ? trace_path_k<true>(c, hs.st, load_d3(origin, i), load_d3(dir, i), max_bounces, reflect != 0, faces, n_hits, oo, od)
                              : trace_path_k<false>(c, hs.st, load_d3(origin, i), load_d3(dir, i), max_bounces, reflect != 0, faces, n_hits, oo, od);
        for (int k = 0; k < max_bounces; ++k) tape[(int64_t)k * n + i] = k < n_hits ? faces[k] : -1;
        const d3 z{0, 0, 0};
        store_d3(out_ori, i, ok ? oo : z);
        store_d3(out_dir, i, ok ? od : z);
        mask[i] = ok ? 1 : 0;
        hits[i] = ok ? (uint8_t)n_hits : 0;
    }
}

// path_loss_backward_ior_k of every row with mask = 1 and a target: returns the summed loss; per_int / per_ext [n] receive the IOR
// partials of each path (0 on the other rows), grad_verts [V,3] (zeroed by the caller) the vertex gradient.  grad_plain [V,3] (zeroed
// by the caller) receives what path_loss_backward_k gives on the same paths, *loss_plain its loss: the two must agree bit for bit.
double pi_loss_backward(void* h, const double* verts64, const double* origin, const double* dir, int64_t n, double ior_int, double ior_ext,
                        int snell, const uint8_t* mask, const int32_t* tape, const uint8_t* hits, const double* out_ori, const double* out_dir,
                        const double* screen_pixel, const uint8_t* valid, double* per_int, double* per_ext, double* grad_verts,
                        double* grad_plain, double* loss_plain) {
    HsScene* s = (HsScene*)h;
    const PathCtx c = path_ctx(s, verts64, ior_int, ior_ext);
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    auto add_plain = [grad_plain](int32_t v, d3 a) { store_d3(grad_plain, v, load_d3(grad_plain, v) + a); };
    double loss = 0.0, plain = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        per_int[i] = 0.0; per_ext[i] = 0.0;
        if (!mask[i] || !valid[i]) continue;
        const d3 o = load_d3(origin, i), d = load_d3(dir, i), eo = load_d3(out_ori, i), ed = load_d3(out_dir, i), sp = load_d3(screen_pixel, i);
        if (snell) {
            loss += path_loss_backward_ior_k<true>(c, o, d, tape + i, n, (int)hits[i], eo, ed, sp, add, per_int[i], per_ext[i]);
            plain += path_loss_backward_k<true>(c, o, d, tape + i, n, (int)hits[i], eo, ed, sp, add_plain);
        } else {
            loss += path_loss_backward_ior_k<false>(c, o, d, tape + i, n, (int)hits[i], eo, ed, sp, add, per_int[i], per_ext[i]);
            plain += path_loss_backward_k<false>(c, o, d, tape + i, n, (int)hits[i], eo, ed, sp, add_plain);
        }
    }
    *loss_plain = plain;
    return loss;
}

// The two-bounce route of drt_path.h on the paths of a (2, drop) trace under the reference formula: path_recompute_backward_inputs with
// the ray_loss seed of the same exit ray; per_int / per_ext [n] as above.
void pi_two_bounce(void* h, const double* verts64, const double* origin, const double* dir, int64_t n, double ior_int, double ior_ext,
                   const uint8_t* mask, const int32_t* tape, const double* out_ori, const double* out_dir, const double* screen_pixel,
                   const uint8_t* valid, double* per_int, double* per_ext) {
    HsScene* s = (HsScene*)h;
    const PathCtx c = path_ctx(s, verts64, ior_int, ior_ext);
    auto add = [](int32_t, d3) {};
    for (int64_t i = 0; i < n; ++i) {
        per_int[i] = 0.0; per_ext[i] = 0.0;
        if (!mask[i] || !valid[i]) continue;
        d3 g_dir, g_o0, g_d0;
        ray_loss_term(load_d3(out_ori, i), load_d3(out_dir, i), load_d3(screen_pixel, i), g_dir);
        path_recompute_backward_inputs(c, load_d3(origin, i), load_d3(dir, i), tape[i], tape[n + i], d3{0, 0, 0}, g_dir, add, g_o0, g_d0,
                                       per_int[i], per_ext[i]);
    }
}

}  // extern "C"
