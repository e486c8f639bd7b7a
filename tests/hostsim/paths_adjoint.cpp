// tests/hostsim/paths_adjoint.cpp -- host harness for refraction paths of up to K interactions with internal reflection.  TEST ONLY.
//
// Compiles drt_shade.h / drt_paths.h (the code the gfx950 kernels of drt_paths.hip inline) with g++ and drives
//   bounce_reflect + bounce_reflect_backward      one interaction per row                         (hp_reflect)
//   path_recompute_backward_k                     a path through GIVEN triangles, no traversal    (hp_path)
//   trace_path_k / path_recompute_backward_k      camera rays through the host BVH of hostsim.cpp (hp_trace, hp_backward)
// with sequential loops, so tests/test_paths_adjoint.py can hold them against torch autograd, finite differences and tests/paths_ref.py.
#include "hostsim.cpp"

#include "../../drt_amd/csrc/drt_paths.h"

extern "C" {

// One interaction per row: o, d [n,3], tri [n,3,3], incoming adjoints g_new_o, g_wr [n,3].
// Out: new_o, wr [n,3] (the reflect continuation, whatever the TIR flag says), tir [n], g_tri [n,3,3] (set), g_o, g_d [n,3].
void hp_reflect(const double* o, const double* d, const double* tri, int64_t n, double ior_int, double ior_ext,
                const double* g_new_o, const double* g_wr, double* new_o, double* wr, uint8_t* tir, double* g_tri, double* g_o, double* g_d) {
    for (int64_t i = 0; i < n; ++i) {
        Bounce b;
        bounce_forward(load_d3(o, i), load_d3(d, i), load_d3(tri, 3 * i), load_d3(tri, 3 * i + 1), load_d3(tri, 3 * i + 2), ior_ext, ior_int, b);
        d3 no, w;
        bounce_reflect(b, load_d3(o, i), no, w);
        store_d3(new_o, i, no);
        store_d3(wr, i, w);
        tir[i] = b.tir ? 1 : 0;
        d3 ga{0, 0, 0}, gb{0, 0, 0}, gc{0, 0, 0}, go, gd;
        bounce_reflect_backward(b, load_d3(g_new_o, i), load_d3(g_wr, i), ga, gb, gc, go, gd);
        store_d3(g_tri, 3 * i, ga); store_d3(g_tri, 3 * i + 1, gb); store_d3(g_tri, 3 * i + 2, gc);
        store_d3(g_o, i, go);
        store_d3(g_d, i, gd);
    }
}

// The path of row i through its own triangles tris[i, 0 .. n_hits[i]) (tris [n,8,3,3]; the faces are given, nothing is traversed; an
// interaction whose TIR flag is set continues mirrored).  Incoming adjoints of the exit ray g_ori, g_dir [n,3].
// Out: out_o, out_d [n,3], flags [n,8] (TIR flag per interaction), n_refr [n], g_tri [n,8,3,3] from path_recompute_backward_k.
void hp_path(const double* o, const double* d, const double* tris, const int32_t* n_hits, int64_t n, double ior_int, double ior_ext,
             const double* g_ori, const double* g_dir, double* out_o, double* out_d, uint8_t* flags, int32_t* n_refr, double* g_tri) {
    int32_t faces[3 * kMaxBounces], tape[kMaxBounces];
    for (int k = 0; k < 3 * kMaxBounces; ++k) faces[k] = k;
    for (int k = 0; k < kMaxBounces; ++k) tape[k] = k;
    for (int64_t i = 0; i < n; ++i) {
        const double* verts = tris + 9 * kMaxBounces * i;
        PathCtx c{};
        c.faces = faces;
        c.verts = verts;
        c.ior_int = ior_int;
        c.ior_ext = ior_ext;
        d3 po = load_d3(o, i), pd = load_d3(d, i);
        int refr = 0;
        for (int k = 0; k < kMaxBounces; ++k) flags[kMaxBounces * i + k] = 0;
        for (int k = 0; k < n_hits[i]; ++k) {
            const int before = refr;
            path_interact(c, k, true, po, pd, refr);
            flags[kMaxBounces * i + k] = refr == before ? 1 : 0;
        }
        store_d3(out_o, i, po);
        store_d3(out_d, i, pd);
        n_refr[i] = refr;
        double* gt = g_tri + 9 * kMaxBounces * i;
        for (int k = 0; k < 9 * kMaxBounces; ++k) gt[k] = 0.0;
        auto add = [gt](int32_t v, d3 a) { store_d3(gt, v, load_d3(gt, v) + a); };
        path_recompute_backward_k(c, load_d3(o, i), load_d3(d, i), tape, 1, n_hits[i], load_d3(g_ori, i), load_d3(g_dir, i), add);
    }
}

// trace_path_k of every camera ray through the host BVH.  Out: out_ori, out_dir [n,3] (zeros on invalid rows), mask [n], tape [K,n]
// (-1 where there was no such interaction; the interactions of a path that ends invalid stay recorded), hits [n] (0 on invalid rows).
void hp_trace(void* h, const double* verts64, const double* origin, const double* dir, int64_t n, double ior_int, double ior_ext,
              int max_bounces, int reflect, double* out_ori, double* out_dir, uint8_t* mask, int32_t* tape, uint8_t* hits) {
    HsScene* s = (HsScene*)h;
    const PathCtx c = path_ctx(s, verts64, ior_int, ior_ext);
    HostStack hs;
    for (int64_t i = 0; i < n; ++i) {
        int32_t faces[kMaxBounces];
        int n_hits = 0;
        d3 oo{0, 0, 0}, od{0, 0, 0};
        const bool ok = trace_path_k(c, hs.st, load_d3(origin, i), load_d3(dir, i), max_bounces, reflect != 0, faces, n_hits, oo, od);
        for (int k = 0; k < max_bounces; ++k) tape[(int64_t)k * n + i] = k < n_hits ? faces[k] : -1;
        const d3 z{0, 0, 0};
        store_d3(out_ori, i, ok ? oo : z);
        store_d3(out_dir, i, ok ? od : z);
        mask[i] = ok ? 1 : 0;
        hits[i] = ok ? (uint8_t)n_hits : 0;
    }
}

// path_recompute_backward_k of every row with mask = 1, summed into grad_verts [V,3] (zeroed by the caller).
void hp_backward(void* h, const double* verts64, const double* origin, const double* dir, int64_t n, double ior_int, double ior_ext,
                 const uint8_t* mask, const int32_t* tape, const uint8_t* hits, const double* g_ori, const double* g_dir, double* grad_verts) {
    HsScene* s = (HsScene*)h;
    const PathCtx c = path_ctx(s, verts64, ior_int, ior_ext);
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    for (int64_t i = 0; i < n; ++i) {
        if (!mask[i]) continue;
        path_recompute_backward_k(c, load_d3(origin, i), load_d3(dir, i), tape + i, n, (int)hits[i], load_d3(g_ori, i), load_d3(g_dir, i), add);
    }
}

}  // extern "C"
