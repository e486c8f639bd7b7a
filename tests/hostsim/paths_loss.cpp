// tests/hostsim/paths_loss.cpp -- host harness for the one-pass form of the K-interaction law (drt_paths.h path_loss_backward_k).  TEST ONLY.
//
// Compiles drt_paths.h (the code k_paths_loss_bwd of drt_paths.hip inlines) with g++ and runs, sequentially over the completed paths of a
// recorded face tape, what the GPU does per list item: the exit ray as the forward leaves it parked (path_interact over the tape), then
// path_loss_backward_k.  tests/test_paths_loss_host.py holds the sums against the golden chain of the reference's own pieces.
#include "hostsim.cpp"

#include "../../drt_amd/csrc/drt_paths.h"

extern "C" {

// faces int32 [F,3], verts64 [V,3], origin / dir / screen_pixel [n,3], valid / mask / hits [n], tape [K,n] (K = tape rows).
// Out: *loss = the summed ray_loss terms, grad_verts [V,3] += their vertex gradient (zeroed by the caller); returns the contributing rays.
int64_t hl_loss_backward(const int32_t* faces, const double* verts64, const double* origin, const double* dir, const double* screen_pixel,
                         const uint8_t* valid, int64_t n, double ior_int, double ior_ext, const uint8_t* mask, const int32_t* tape,
                         const uint8_t* hits, double* loss, double* grad_verts) {
    PathCtx c{};
    c.faces = faces;
    c.verts = verts64;
    c.ior_int = ior_int;
    c.ior_ext = ior_ext;
    auto add = [grad_verts](int32_t v, d3 a) { store_d3(grad_verts, v, load_d3(grad_verts, v) + a); };
    double sum = 0.0;
    int64_t cnt = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!mask[i] || !valid[i]) continue;
        d3 o = load_d3(origin, i), d = load_d3(dir, i);
        int n_refr = 0;
        for (int k = 0; k < (int)hits[i]; ++k) path_interact(c, tape[(int64_t)k * n + i], true, o, d, n_refr);
        sum += path_loss_backward_k(c, load_d3(origin, i), load_d3(dir, i), tape + i, n, (int)hits[i], o, d, load_d3(screen_pixel, i), add);
        ++cnt;
    }
    *loss = sum;
    return cnt;
}

}  // extern "C"
