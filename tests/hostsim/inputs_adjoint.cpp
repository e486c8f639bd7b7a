// tests/hostsim/inputs_adjoint.cpp -- host harness for the input adjoints of the refraction path.  TEST ONLY.
//
// Compiles drt_shade.h / drt_path.h (the code the gfx950 backward kernels inline) with g++ and drives
// bounce_backward_eta + eta_to_ior (one bounce) and path_recompute_backward_inputs (the two-bounce path) with
// sequential loops, so tests/test_inputs_adjoint.py can hold them against torch autograd on the CPU.
#include <cstdint>

#include "../../drt_amd/csrc/drt_path.h"

using namespace drt;

extern "C" {

// One bounce per row: o, d [n,3], tri [n,3,3], incoming adjoints g_new_o, g_wt [n,3].
// Out: new_o, wt [n,3], sg [n] (+1 entering, -1 leaving), g_tri [n,3,3] (set), g_o, g_d [n,3], g_ior [n,2] (int, ext).
void hi_bounce(const double* o, const double* d, const double* tri, int64_t n, double ior_int, double ior_ext,
               const double* g_new_o, const double* g_wt, double* new_o, double* wt, double* sg, double* g_tri,
               double* g_o, double* g_d, double* g_ior) {
    for (int64_t i = 0; i < n; ++i) {
        Bounce b;
        bounce_forward(load_d3(o, i), load_d3(d, i), load_d3(tri, 3 * i), load_d3(tri, 3 * i + 1), load_d3(tri, 3 * i + 2), ior_ext, ior_int, b);
        store_d3(new_o, i, b.new_o);
        store_d3(wt, i, b.wt);
        sg[i] = b.sg;
        d3 ga{0, 0, 0}, gb{0, 0, 0}, gc{0, 0, 0}, go, gd;
        double g_eta, gi = 0.0, ge = 0.0;
        bounce_backward_eta(b, load_d3(g_new_o, i), load_d3(g_wt, i), ga, gb, gc, go, gd, g_eta);
        eta_to_ior(b, ior_int, ior_ext, g_eta, gi, ge);
        store_d3(g_tri, 3 * i, ga); store_d3(g_tri, 3 * i + 1, gb); store_d3(g_tri, 3 * i + 2, gc);
        store_d3(g_o, i, go);
        store_d3(g_d, i, gd);
        g_ior[2 * i] = gi;
        g_ior[2 * i + 1] = ge;
    }
}

// The two-bounce path of row i through tri1[i] then tri2[i] (no traversal: the faces are given).  Incoming adjoints of the exit ray
// g_ori, g_dir [n,3].  Out: out_o, out_d [n,3]; g_tri [n,6,3] = vertex gradients of tri1 then tri2 from path_recompute_backward_inputs,
// g_tri_plain [n,6,3] the same from path_recompute_backward; g_o, g_d [n,3]; g_ior [n,2].
void hi_path(const double* o, const double* d, const double* tri1, const double* tri2, int64_t n, double ior_int, double ior_ext,
             const double* g_ori, const double* g_dir, double* out_o, double* out_d, double* g_tri, double* g_tri_plain,
             double* g_o, double* g_d, double* g_ior) {
    const int32_t faces[6] = {0, 1, 2, 3, 4, 5};
    for (int64_t i = 0; i < n; ++i) {
        double verts[18];
        for (int k = 0; k < 9; ++k) { verts[k] = tri1[9 * i + k]; verts[9 + k] = tri2[9 * i + k]; }
        PathCtx c{};
        c.faces = faces;
        c.verts = verts;
        c.ior_int = ior_int;
        c.ior_ext = ior_ext;
        Bounce b1, b2;
        bounce_forward(load_d3(o, i), load_d3(d, i), load_d3(verts, 0), load_d3(verts, 1), load_d3(verts, 2), ior_ext, ior_int, b1);
        bounce_forward(b1.new_o, b1.wt, load_d3(verts, 3), load_d3(verts, 4), load_d3(verts, 5), ior_ext, ior_int, b2);
        store_d3(out_o, i, b2.new_o);
        store_d3(out_d, i, b2.wt);
        double* gt = g_tri + 18 * i;
        double* gp = g_tri_plain + 18 * i;
        for (int k = 0; k < 18; ++k) { gt[k] = 0.0; gp[k] = 0.0; }
        auto add = [gt](int32_t v, d3 a) { store_d3(gt, v, load_d3(gt, v) + a); };
        auto add_plain = [gp](int32_t v, d3 a) { store_d3(gp, v, load_d3(gp, v) + a); };
        d3 go, gd;
        double gi, ge;
        path_recompute_backward_inputs(c, load_d3(o, i), load_d3(d, i), 0, 1, load_d3(g_ori, i), load_d3(g_dir, i), add, go, gd, gi, ge);
        path_recompute_backward(c, load_d3(o, i), load_d3(d, i), 0, 1, load_d3(g_ori, i), load_d3(g_dir, i), add_plain);
        store_d3(g_o, i, go);
        store_d3(g_d, i, gd);
        g_ior[2 * i] = gi;
        g_ior[2 * i + 1] = ge;
    }
}

}  // extern "C"
