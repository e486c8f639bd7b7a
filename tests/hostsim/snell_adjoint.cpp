// tests/hostsim/snell_adjoint.cpp -- host harness for the Snell element of the K-interaction path law.  TEST ONLY.
//
// Compiles drt_shade.h / drt_paths.h (the code the gfx950 kernels of drt_paths.hip inline) with g++ and drives
//   bounce_forward_snell + bounce_backward_snell (or the reference pair)   one refracting bounce per row        (sn_bounce)
//   trace_path_k<true>                                                      camera rays through the host BVH     (sn_trace)
//   path_recompute_backward_k<true>                                         the adjoint of those paths           (sn_backward)
//   path_loss_backward_k<true>                                              ray_loss term + adjoint in one go    (sn_loss_backward)
// with sequential loops, so tests/test_snell_adjoint.py can hold them against torch autograd, finite differences and tests/snell_ref.py.
#include "hostsim.cpp"

#include "../../drt_amd/csrc/drt_paths.h"

extern "C" {

// One bounce per row: o, d [n,3], tri [n,3,3], incoming adjoints g_new_o, g_wt [n,3].  snell != 0: the Snell pair, else the reference's.
// Out: new_o, wt [n,3] (the refract continuation, whatever the TIR flag says), tir [n], ct [n], nrm [n,3] (the flipped normal), eta [n],
// g_tri [n,3,3] (set), g_o, g_d [n,3] -- the backward runs on every row, flagged or not.
void sn_bounce(const double* o, const double* d, const double* tri, int64_t n, double ior_int, double ior_ext, int snell,
               const double* g_new_o, const double* g_wt, double* new_o, double* wt, uint8_t* tir, double* ct, double* nrm, double* eta,
               double* g_tri, double* g_o, double* g_d) {
    for (int64_t i = 0; i < n; ++i) {
        Bounce b;
        const d3 v0 = load_d3(tri, 3 * i), v1 = load_d3(tri, 3 * i + 1), v2 = load_d3(tri, 3 * i + 2);
        if (snell) bounce_forward_snell(load_d3(o, i), load_d3(d, i), v0, v1, v2, ior_ext, ior_int, b);
        else bounce_forward(load_d3(o, i), load_d3(d, i), v0, v1, v2, ior_ext, ior_int, b);
        store_d3(new_o, i, b.new_o);
        store_d3(wt, i, b.wt);
        store_d3(nrm, i, b.n);
        tir[i] = b.tir ? 1 : 0;
        ct[i] = b.ct;
        eta[i] = b.eta;
        d3 ga{0, 0, 0}, gb{0, 0, 0}, gc{0, 0, 0}, go, gd;
        if (snell) bounce_backward_snell(b, load_d3(g_new_o, i), load_d3(g_wt, i), ga, gb, gc, go, gd);
        else bounce_backward(b, load_d3(g_new_o, i), load_d3(g_wt, i), ga, gb, gc, go, gd);
        store_d3(g_tri, 3 * i, ga); store_d3(g_tri, 3 * i + 1, gb); store_d3(g_tri, 3 * i + 2, gc);
        store_d3(g_o, i, go);
        store_d3(g_d, i, gd);
    }
}

// trace_path_k<true> of every ray through the host BVH.  Out: out_ori, out_dir [n,3] (zeros on invalid rows), mask [n], tape [K,n]
// (-1 where there was no such interaction; the interactions of a path that ends invalid stay recorded), hits [n] (0 on invalid rows).
void sn_trace(void* h, const double* verts64, const double* origin, const double* dir, int64_t n, double ior_int, double ior_ext,
              int max_bounces, int reflect, double* out_ori, double* out_dir, uint8_t* mask, int32_t* tape, uint8_t* hits) {
    HsScene* s = (HsScene*)h;
    const PathCtx c = path_ctx(s, verts64, ior_int, ior_ext);
    HostStack hs;
    for (int64_t i = 0; i < n; ++i) {
        int32_t faces[kMaxBounces];
        int n_hits = 0;
        d3 oo{0, 0, 0}, od{0, 0, 0};
        const bool ok = trace_path_k<true>(c, hs.st, load_d3(origin, i), load_d3(dir, i), max_bounces, reflect != 0, faces, n_hits, oo, od);
        for (int k = 0; k < max_bounces; ++k) tape[(int64_t)k * n + i] = k < n_hits ? faces[k] : -1;
        const d3 z{0, 0, 0};
        store_d3(out_ori, i, ok ? oo : z);
        store_d3(out_dir, i, ok ? od : z);
        mask[i] = ok ? 1 : 0;
        hits[i] = ok ? (uint8_t)n_hits : 0;
    }
}

// path_recompute_backward_k<true> of every row with mask = 1, summed into grad_verts [V,3] (zeroed by the caller).
void sn_backward(void* h, const double* verts64, const double* origin, const double* dir, int64_t n, double ior_int, double ior_ext,
                 const uint8_t* mask, const int32_t* tape, const uint8_t* hits, const double* g_ori, const double* g_dir, double* grad_verts) {
    HsScene* s = (HsScene*)h;
    const PathCtx c = path_ctx(s, verts64, ior_int, ior_ext);
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    for (int64_t i = 0; i < n; ++i) {
        if (!mask[i]) continue;
        path_recompute_backward_k<true>(c, load_d3(origin, i), load_d3(dir, i), tape + i, n, (int)hits[i], load_d3(g_ori, i), load_d3(g_dir, i), add);
    }
}

// path_loss_backward_k<true> of every row with mask = 1 and a target (valid = 1) on the exit rays of sn_trace: returns the summed loss,
// the vertex gradient (unit seed) summed into grad_verts [V,3] (zeroed by the caller).
double sn_loss_backward(void* h, const double* verts64, const double* origin, const double* dir, int64_t n, double ior_int, double ior_ext,
                        const uint8_t* mask, const int32_t* tape, const uint8_t* hits, const double* out_ori, const double* out_dir,
                        const double* screen_pixel, const uint8_t* valid, double* grad_verts) {
    HsScene* s = (HsScene*)h;
    const PathCtx c = path_ctx(s, verts64, ior_int, ior_ext);
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    double loss = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        if (!mask[i] || !valid[i]) continue;
        loss += path_loss_backward_k<true>(c, load_d3(origin, i), load_d3(dir, i), tape + i, n, (int)hits[i], load_d3(out_ori, i), load_d3(out_dir, i),
                                           load_d3(screen_pixel, i), add);
    }
    return loss;
}

}  // extern "C"
