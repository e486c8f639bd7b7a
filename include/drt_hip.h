/*
 * drt_hip.h -- C ABI of libdrt_hip.so, the MI355X (gfx950) implementation of DRT's
 * differentiable refraction-tracing hot path.
 *
 * Plain pointers and sizes only: every `d_*` argument is a DEVICE pointer on the GPU
 * the scene was created for, `stream` is a hipStream_t passed as void* (NULL = the
 * null stream).  No call synchronises the host; all work is enqueued on `stream`.
 * Every function returns 0 on success or a negative DRT_E_* code; drt_last_error()
 * gives the message for the calling thread.
 *
 * Two nested boundaries of the reference are covered:
 *   B1  the native tracer class `optix_mesh` (reference optix_extend.cpp:6-83), which
 *       the reference builds on NVIDIA OptiX Prime 6.5;
 *   B2  the per-view math of `Scene` in reference DiffRender.py that consumes the face
 *       ids (render_transparent / silhouette / dihedral) and the ray loss of
 *       reference optim.py:91-108, forward and backward.
 */
#ifndef DRT_HIP_H
#define DRT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRT_OK            0
#define DRT_E_INVALID    -1   /* bad argument (null pointer, negative size, no mesh yet) */
#define DRT_E_HIP        -2   /* a HIP runtime call failed */
#define DRT_E_NOMEM      -3

typedef struct drt_scene drt_scene_t;

const char* drt_last_error(void);
int drt_version(void);       /* 2: drt_deterministic / drt_fx_finalize; 3: drt_render_paths_forward / _backward; 4: drt_render_paths_ray_loss_fused;
                            * 5: drt_render_paths_law_* (law_flags: Snell refraction); 6: drt_render_paths_law_ray_loss_ior_fused;
                            * 7: drt_hull_field / drt_hull_mark / drt_hull_emit; 8: drt_render_image; 9: drt_render_image_loss;
                            * 10: drt_route_counts; 11: drt_render_image_loss_screen; 12: drt_render_image_loss_camera;
                            * 13: drt_image_views_create / drt_render_image_loss_views; drt_render_loss_arm / drt_render_loss_taken came
                            * later under the same number (a library that lacks them lacks the symbols) */

/* ---- deterministic accumulation ("race detection / sanitizers"; reference optim.py:155-171 clamps the SUM) --------
 * Every vertex gradient and loss of this library is a sum of contributions scattered with float64 atomics: the same inputs give results
 * that differ from run to run at 1e-16 relative, in the order the hardware served the atomics.  drt_deterministic(1) -- or DRT_DETERMINISTIC=1
 * in the environment, read at the first call that needs to know -- switches the whole PROCESS to order-independent accumulation: every
 * `double* d_grad_verts` / `double* d_loss` / `d_stash` ACCUMULATION TARGET of the entry points below must then point to an array of
 * accumulator cells instead of doubles, DRT_FX_BYTES_PER_VALUE bytes per float64 element (same element numbers), zero-filled by the
 * caller; the kernels add every contribution as a 128-bit fixed-point integer (unit 2^-80, drt_amd/csrc/drt_fixed.h: integer addition
 * is associative, so the sum is the same bit pattern whatever the order; contributions of magnitude >= 3.7e-9 enter exactly, smaller ones
 * are truncated at 8e-25 absolute; |x| >= 7e13, +-inf and NaN set sticky flags and give +-inf / NaN).  drt_fx_finalize converts n cells to
 * float64 with ONE rounding (nearest-even) of the exact sum: d_out[i] = value, or d_out[i] += value with `accumulate`.  Inputs that are
 * READ as gradients (d_grad_out_dir, d_grad_cos, ...) and per-ray outputs stay plain float64.  Same result for eager launches and graph
 * replays, any stream interleaving, any sub-batch split.  The price: two 64-bit integer atomics per component, in the LDS table
 * of the path kernels (half as many slots as the float64 table, drt_amd/csrc/drt_pathsink.h) and again when a slot goes to memory
 * (DESIGN.md section 7 has the measured cost).  drt_deterministic(-1) only queries; returns the previous mode. */
#define DRT_FX_BYTES_PER_VALUE 24
int drt_deterministic(int on);
int drt_fx_finalize(const void* d_cells, int64_t n, double* d_out, int accumulate, void* stream);
/* Sums of sums, still exact: drt_fx_add adds n cells of d_src_cells into d_dst_cells (several calls of one step).  For the step's ONE
 * all-reduce over ranks drt_fx_to_limbs rewrites n cells as int64 [n,4] -- three 43-bit limbs of the 128-bit sum,
 * the top one signed, and the flags as counters -- whose plain per-word SUM over up to 2^20 ranks cannot overflow; drt_fx_from_limbs
 * puts the reduced words back together.  All ranks then convert the SAME integer: N GPUs give the bits one GPU gives. */
int drt_fx_add(void* d_dst_cells, const void* d_src_cells, int64_t n, void* stream);
int drt_fx_to_limbs(const void* d_cells, int64_t n, int64_t* d_limbs, void* stream);
int drt_fx_from_limbs(const int64_t* d_limbs, int64_t n, void* d_cells, void* stream);

/* ---- lifetime: replaces optix_mesh::optix_mesh(cuda_device), optix_extend.cpp:8-12 ---- */
int drt_create(int device, drt_scene_t** out);
void drt_destroy(drt_scene_t* s);

/* ---- B1: acceleration structure -------------------------------------------------------
 * drt_update_mesh  <- optix_mesh::update_mesh(F int32 [F,3], V float32 [V,3]), optix_extend.cpp:14-21
 * drt_update_vert  <- optix_mesh::update_vert(V float32 [V,3]),               optix_extend.cpp:23-27
 * Both copy their inputs (the reference keeps tensor references alive instead) and rebuild
 * the LBVH on `stream`: scene bounds -> 30-bit Morton codes -> radix sort -> Karras
 * hierarchy -> bottom-up box refit -> collapse to a 4-wide tree with <= 4-triangle leaves.
 * drt_update_vert_f64 fuses the reference's `vertices.detach().to(float32)`
 * (DiffRender.py:379) into the rebuild. */
int drt_update_mesh(drt_scene_t* s, const int32_t* d_faces, int64_t n_faces,
                    const float* d_verts, int64_t n_verts, void* stream);
int drt_update_vert(drt_scene_t* s, const float* d_verts, int64_t n_verts, void* stream);
int drt_update_vert_f64(drt_scene_t* s, const double* d_verts, int64_t n_verts, void* stream);

/* drt_intersect <- optix_mesh::intersect(Ray float32 [N,6]) -> T float32 [N], ID int32 [N],
 * optix_extend.cpp:29-57.  Closest hit with t > 0 (equal t: the lowest face id); miss: T = -1, ID = -1.  What a hit is:
 * the float32 Moller-Trumbore test of drt_amd/csrc/drt_tri.h -- the transcription of the reference's own JIT_Dintersect --
 * plus "the hit point lies in the triangle's bounding box grown by 2^-14 of the scene extent", which is what makes the
 * closest hit over ALL triangles computable by a tree for rays that run inside a triangle's plane.
 * Outputs are caller-owned contiguous arrays (the reference returns strided aliases of one buffer).
 * drt_intersect_any writes only a hit flag (uint8) -- what Scene.optix_intersect's callers
 * at DiffRender.py:426 and :224 use. */
int drt_intersect(drt_scene_t* s, const float* d_rays, int64_t n_rays,
                  float* d_T, int32_t* d_ID, void* stream);
int drt_intersect_any(drt_scene_t* s, const float* d_rays, int64_t n_rays,
                      uint8_t* d_hit, void* stream);
/* Same results as drt_intersect by testing every triangle (no BVH); diagnostic used to
 * check the traversal at full workload sizes. */
int drt_intersect_bruteforce(drt_scene_t* s, const float* d_rays, int64_t n_rays,
                             float* d_T, int32_t* d_ID, void* stream);
/* Diagnostic: number of BVH child boxes that fail to enclose their subtree (0 when the
 * build is sound, also counted when the 4-wide tree is too deep for the traversal stack), the binary
 * tree height and (nullable) the depth of the 4-wide tree; host-synchronising. */
int drt_bvh_check(drt_scene_t* s, void* stream, int64_t* n_violations, int32_t* height, int32_t* wide_depth);
/* Diagnostic: copy the Morton-sorted face order (int32 [F]) to d_order. */
int drt_bvh_sorted_faces(drt_scene_t* s, int32_t* d_order, void* stream);
/* How updates treat the tree (also DRT_TREE / DRT_REBUILD_EVERY at drt_create).  mode 0 (default): every update is a full LBVH build --
 * Morton keys, radix sort, Karras hierarchy, refit, 4-wide collapse -- as the reference's OptiX model is rebuilt on every update_vert
 * (optix_extend.cpp:23-27, 61-67).  mode 1: the LBVH's topology is kept for `rebuild_every` updates; the updates in between refit the
 * boxes and re-quantise the wide nodes only (3 launches instead of 7).  mode 2: a binned-SAH topology is built on the HOST at every
 * drt_update_mesh (one device -> host copy of the mesh, milliseconds) and every drt_update_vert* refits it.  Results do not depend on the
 * mode: boxes only decide which triangles are tested (drt_bvh_check validates any of the trees). */
int drt_tree_mode(drt_scene_t* s, int mode, int rebuild_every);
/* Diagnostic: the scene box the last build derived from the vertices -- out7 = lo[3], 1/extent[3], leaf padding (float32; the margin of
 * the hit-point test is half the padding); host-synchronising.  What a replayed capture of an update must reproduce. */
int drt_build_params(drt_scene_t* s, float* out7, void* stream);
/* Diagnostic: one array of the last build, copied device -> device into d_out on `stream` (after the build; not host-synchronising).
 * `bytes` must be exactly the array's size (F faces, I = max(F - 1, 1) inner nodes), else DRT_E_INVALID and nothing is written:
 * KEYS uint32 [F] and ORDER uint32 [F] (sorted Morton keys, face id per slot), NODES 64 B x I (binary nodes), PARENT_INNER int32 [I],
 * PARENT_LEAF int32 [F] (2 * parent + child slot), RANGE_LO / RANGE_HI int32 [I], WIDE 64 B x I (quantised 4-wide nodes; entries of
 * subtrees that fit one leaf are never written, except the root's), TRIS / TRIS_FLAT 48 B x F (records in slot order / in the order the projection pass
 * reads), SLOT_OF_FACE int32 [F], PARAMS 100 B (scene box, padding, Morton plan).  KEYS are those of the last FULL build: stale after a
 * kept-topology update in tree mode 1, undefined in mode 2.  An empty mesh has empty arrays. */
enum {
    DRT_BVH_KEYS = 0, DRT_BVH_ORDER = 1, DRT_BVH_NODES = 2, DRT_BVH_PARENT_INNER = 3, DRT_BVH_PARENT_LEAF = 4, DRT_BVH_RANGE_LO = 5,
    DRT_BVH_RANGE_HI = 6, DRT_BVH_WIDE = 7, DRT_BVH_TRIS = 8, DRT_BVH_TRIS_FLAT = 9, DRT_BVH_SLOT_OF_FACE = 10, DRT_BVH_PARAMS = 11
};
int drt_bvh_export(drt_scene_t* s, int what, void* d_out, int64_t bytes, void* stream);

/* ---- B2: Scene.render_transparent, DiffRender.py:420-432 (trace2 :537-546, Dintersect
 * :492-501, refract_ray :503-535) -------------------------------------------------------
 * In : d_verts float64 [V,3] (the differentiable vertices; the BVH must have been built
 *      from their float32 cast), origin/dir float64 [N,3].
 * Out: out_ori, out_dir float64 [N,3] (zeros where the path is invalid), mask uint8 [N,3]
 *      (the reference's bool [N,3]), face1/face2 int32 [N]: faces hit at bounce 1 / 2,
 *      face2 >= 0 exactly for the rays with mask = 1 (saved for backward), face1 = -1 on
 *      a primary miss.  Optional (both or neither): d_valid_idx int32 [N] receives the indices of
 *      the rays with mask = 1 (unordered), *d_n_valid (int64, device) their number -- handing
 *      them to drt_render_backward spares it a pass over the dense arrays.
 *      tile_w, tile_h: 0, or the width / height in pixels of the image(s) whose rows the rays are (width a multiple
 *      of 64, height a multiple of 4, whole images concatenated): a HINT that lets the pipeline group rays by
 *      16x4-pixel screen tiles and, when every image verifies as a pinhole ray grid (generate_ray, reference
 *      captured_data.py:23-40), decide the primary hits by projecting the triangles instead of traversing the
 *      tree (csrc/drt_raster.h).  Every ray is checked against the fitted grid on the device and takes the
 *      tree otherwise: results do not depend on the hint.
 *      grid_mode, d_grid_cache: DRT_GRID_NONE / NULL, or a caller-owned device buffer of DRT_GRID_CACHE_BYTES per image that
 *      belongs to THIS (origin, dir) pair with THIS tile_w x tile_h.  DRT_GRID_ESTABLISH: the call fits and verifies as
 *      above and records, per image, the model and whether every ray verified.  DRT_GRID_TRUST: the caller guarantees the
 *      ray arrays have not changed since the establishing call; images recorded as all-verified are then not re-fitted,
 *      only the 8x8 lattice of 64 sample rays per image is re-verified against the recorded model (an image that fails is
 *      re-fitted, verified ray by ray like in a call without a cache, and marked untrusted IN THE CACHE for good), and rays of
 *      pixels that no projected triangle touches are not even loaded.  The lattice check catches ray arrays that were replaced
 *      wholesale; a change confined to rays off the lattice is the caller's responsibility.  (The Python layer ties the buffer
 *      to the tensor objects and their version counters.) */
#define DRT_GRID_NONE 0
#define DRT_GRID_ESTABLISH 1
#define DRT_GRID_TRUST 2
#define DRT_GRID_CACHE_BYTES 104
/* OR-ed into grid_mode: d_face1 / d_face2 are only guaranteed for the rays with mask = 1 (what drt_render_backward* read);
 * in DRT_GRID_TRUST mode -- and in any mode when the three dense outputs were offered through drt_outputs_clean -- the -1 entries of
 * all other rays are then not written (8 bytes per ray less to fill). */
#define DRT_GRID_SPARSE_FACES 16
/* OR-ed into DRT_GRID_TRUST: the caller has read the cache back after the establishing call and EVERY image in it is recorded
 * as a pinhole grid in all of its rays (int32 `ok` and `all` at byte offsets 96 and 100 of each DRT_GRID_CACHE_BYTES record
 * both non-zero).  Normally no ray then needs the tree for its primary hit: the launches that serve such rays in front of the
 * first shading stage are not issued and the call waits for the (asynchronous) tree build only in front of the second traversal.
 * A performance hint, not a promise the results depend on: an image can still lose its status inside the call (a triangle reaches
 * its camera plane, its large-triangle list overflows, its rays fail the lattice re-check below); its rays are then traced through
 * the tree by a small fallback launch behind the build (csrc/drt_pipeline.hip, k_gen_late). */
#define DRT_GRID_ALL_VERIFIED 32
int drt_render_forward(drt_scene_t* s, const double* d_verts, const double* d_origin,
                       const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                       double* d_out_ori, double* d_out_dir, uint8_t* d_mask,
                       int32_t* d_face1, int32_t* d_face2,
                       int32_t* d_valid_idx, int64_t* d_n_valid, int tile_w, int tile_h,
                       int grid_mode, void* d_grid_cache, void* stream);
/* Adjoint of drt_render_forward w.r.t. the vertices: d_grad_verts float64 [V,3] += ...
 * (atomic accumulation; zero it first).  Either incoming gradient may be NULL (= zeros). */
int drt_render_backward(drt_scene_t* s, const double* d_verts, const double* d_origin,
                        const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                        const int32_t* d_face1, const int32_t* d_face2,
                        const int32_t* d_valid_idx, const int64_t* d_n_valid,
                        const double* d_grad_out_ori, const double* d_grad_out_dir,
                        double* d_grad_verts, void* stream);
/* drt_render_backward that also returns the gradients w.r.t. the other inputs of the render call (the reference differentiates
 * them all: its path is plain torch autograd).  Each output is optional (NULL = not computed) and added to (+=):
 *   d_grad_origin float64 [N,3]  d / d origin of every ray with a completed path (other rows untouched; one writer per row),
 *   d_grad_dir    float64 [N,3]  d / d ray_dir, likewise,
 *   d_grad_ior    [2]            d / d ior_int, d / d ior_ext -- two float64, or in deterministic mode two fixed-point cells
 *                                (DRT_FX_BYTES_PER_VALUE each) like d_grad_verts.
 * Through the `entering` branch of each bounce eta is ior_ext / ior_int or ior_int / ior_ext; the branch and the total-internal-
 * reflection test carry no gradient.  d_grad_verts gets the same gradient drt_render_backward adds (bit for bit in deterministic mode). */
int drt_render_backward_inputs(drt_scene_t* s, const double* d_verts, const double* d_origin,
                               const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                               const int32_t* d_face1, const int32_t* d_face2,
                               const int32_t* d_valid_idx, const int64_t* d_n_valid,
                               const double* d_grad_out_ori, const double* d_grad_out_dir,
                               double* d_grad_verts, double* d_grad_origin, double* d_grad_dir,
                               double* d_grad_ior, void* stream);

/* ---- refraction paths of up to K surface interactions, with optional internal reflection (opt-in; drt_render_forward is the
 * reference's path and is not altered by this) ---------------------------------------------------------------------------------
 * max_bounces = K, 2 <= K <= 8: at most K surface interactions.  reflect: 0 = a hit with total internal reflection ends the path
 * (as the reference does), 1 = the ray continues mirrored: wr = -wo + (2 dot(wo, n)) n with refract_ray's flipped normal (the
 * reference's Reflect, DiffRender.py:31-33; not renormalised), origin (o + t d) + 1e-5 wr, and counts no refraction.
 * A camera ray repeats { closest hit (the tracer contract of drt_intersect; once K interactions are used up the any-hit form);
 * miss: the path ends, valid iff it has made an even, non-zero number of refractions; hit with K interactions used up: invalid;
 * hit: JIT_Dintersect + refract_ray on the float64 ray, as in drt_render_forward }.  K = 2, reflect = 0 is drt_render_forward's
 * path: the same outputs bit for bit.  Geometry only: no Fresnel weights (the reference drops R too).
 * In : as drt_render_forward.
 * Out: out_ori, out_dir float64 [N,3] (zeros where the path is invalid), mask uint8 [N,3];
 *      d_tape int32 [K,N]: the face of interaction k of ray i at [k * N + i], -1 where the ray had no k-th interaction (the
 *      interactions of a path that ends invalid stay recorded); d_hits uint8 [N]: the number of interactions of a valid path, 0
 *      on invalid rows; d_valid_idx int32 [N] / *d_n_valid (int64, device): the rays with mask = 1, in ray order.
 * All launches go to `stream`, list sizes stay on the device: the call can be captured in a graph once an eager call of at least
 * this many rays has allocated the scene's ray lists.  A K outside 2..8 is DRT_E_INVALID. */
int drt_render_paths_forward(drt_scene_t* s, const double* d_verts, const double* d_origin,
                             const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                             int max_bounces, int reflect,
                             double* d_out_ori, double* d_out_dir, uint8_t* d_mask,
                             int32_t* d_tape, uint8_t* d_hits,
                             int32_t* d_valid_idx, int64_t* d_n_valid, void* stream);
/* Adjoint of drt_render_paths_forward w.r.t. the vertices: d_grad_verts float64 [V,3] += ... (or accumulator cells in deterministic
 * mode, like drt_render_backward).  Every listed path is recomputed from its camera ray and its column of the tape; the total-internal-
 * reflection flags are recomputed too (the same bits).  Either incoming gradient may be NULL (= zeros). */
int drt_render_paths_backward(drt_scene_t* s, const double* d_verts, const double* d_origin,
                              const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                              int max_bounces, int reflect,
                              const int32_t* d_tape, const uint8_t* d_hits,
                              const int32_t* d_valid_idx, const int64_t* d_n_valid,
                              const double* d_grad_out_ori, const double* d_grad_out_dir,
                              double* d_grad_verts, void* stream);

/* The one-pass form of the K-interaction law for a loss loop: ray_loss of this view and its vertex gradient, nothing dense written
 * (what drt_render_ray_loss_fused is to drt_render_forward).  *d_loss += sum over the rays with a target (d_valid) whose path completes
 * of |out_dir - normalize(screen_pixel - out_ori)|^2; d_grad_verts float64 [V,3] += d loss / d vertices with a UNIT seed; *d_n_valid
 * (int64, device; may be NULL) += the number of contributing rays.  In deterministic mode d_loss and d_grad_verts are accumulator cells,
 * as for drt_render_ray_loss_fused.  Several calls (the views of a step) may accumulate into the same targets.  The law and its checks
 * are drt_render_paths_forward's; n_rays = 0, a view that misses the mesh and a view without targets leave the accumulators alone.
 * No caller tensor is written: the float64 ray in flight, the face tape and the hit counts live in the scene's workspace (81 B per ray
 * of the largest call so far, next to the ray lists), a ray without a target is never traced, and origin / dir / valid are read once
 * per camera ray.  All launches go to `stream` and every list size stays on the device: capturable once an eager call of at least this
 * many rays has grown the workspace (a call that would have to grow it inside a capture is DRT_E_INVALID). */
int drt_render_paths_ray_loss_fused(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir,
                                    const double* d_screen_pixel, const uint8_t* d_valid, int64_t n_rays,
                                    double ior_int, double ior_ext, int max_bounces, int reflect,
                                    double* d_loss, double* d_grad_verts, int64_t* d_n_valid, void* stream);

/* The three calls above with the whole law in one argument: `law_flags` (a combination of the bits below; any other bit is
 * DRT_E_INVALID) stands where `reflect` stands, every other argument, output and rule is the namesake's.
 *   DRT_LAW_REFLECT  a hit with total internal reflection mirrors the ray (reflect = 1); unset: it ends the path (reflect = 0).
 *   DRT_LAW_SNELL    a refracting hit is bent by Snell's law, sin(theta_t) = eta sin(theta_i): cosThetaT =
 *                    sqrt(max(1 - eta^2 sin2ThetaI, 0)) in place of the reference's sqrt(1 - sin2ThetaI) (Refract, DiffRender.py:42,
 *                    which gives tan(theta_t) = eta tan(theta_i)); everything else of the bounce -- the hit, the flipped normal, the
 *                    total-internal-reflection flag, w = eta d + k n, its normalisation, the 1e-5 origin offset -- is unchanged.
 *                    The adjoint passes no gradient through cosThetaT where it is 0 (instead of NaN); close to the critical angle it
 *                    grows like 1 / cosThetaT.  Unset: the reference's formula, i.e. the namesake's bits.
 * drt_render_paths_law_backward must be given the law_flags of the forward whose tape it reverses (DRT_LAW_REFLECT does not change
 * what it computes: the flags of a completed path are recomputed).  Without DRT_LAW_SNELL the calls run the namesakes' kernels. */
#define DRT_LAW_REFLECT 1
#define DRT_LAW_SNELL 2
int drt_render_paths_law_forward(drt_scene_t* s, const double* d_verts, const double* d_origin,
                                 const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                                 int max_bounces, int law_flags,
                                 double* d_out_ori, double* d_out_dir, uint8_t* d_mask,
                                 int32_t* d_tape, uint8_t* d_hits,
                                 int32_t* d_valid_idx, int64_t* d_n_valid, void* stream);
int drt_render_paths_law_backward(drt_scene_t* s, const double* d_verts, const double* d_origin,
                                  const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                                  int max_bounces, int law_flags,
                                  const int32_t* d_tape, const uint8_t* d_hits,
                                  const int32_t* d_valid_idx, const int64_t* d_n_valid,
                                  const double* d_grad_out_ori, const double* d_grad_out_dir,
                                  double* d_grad_verts, void* stream);
int drt_render_paths_law_ray_loss_fused(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir,
                                        const double* d_screen_pixel, const uint8_t* d_valid, int64_t n_rays,
                                        double ior_int, double ior_ext, int max_bounces, int law_flags,
                                        double* d_loss, double* d_grad_verts, int64_t* d_n_valid, void* stream);

/* drt_render_paths_law_ray_loss_fused that also differentiates the two indices of refraction: d_grad_ior, two accumulators -- d loss /
 * d ior_int, then d loss / d ior_ext, unit seed -- that are ADDED to: two float64, or, in deterministic mode, two accumulator cells laid
 * out as those of drt_render_backward_ray_loss_inputs.  Every refracting interaction of a completed path contributes through
 * eta = ior_i / ior_t (under either refraction formula); a mirrored one contributes nothing, and the total-internal-reflection flag and
 * the entering / leaving branch carry no gradient.  d_grad_verts may be NULL: no vertex gradient is computed then (the calibration of a
 * fixed mesh: a kernel without the gradient table); otherwise it receives what the namesake writes.  d_grad_ior = NULL, a bad law_flags
 * or a bad max_bounces is DRT_E_INVALID; n_rays = 0 is DRT_OK and touches nothing.  Stream, workspace and capture rules: the namesake's. */
int drt_render_paths_law_ray_loss_ior_fused(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir,
                                            const double* d_screen_pixel, const uint8_t* d_valid, int64_t n_rays,
                                            double ior_int, double ior_ext, int max_bounces, int law_flags,
                                            double* d_loss, double* d_grad_verts, double* d_grad_ior, int64_t* d_n_valid, void* stream);

/* ---- Loss_calculator.ray_loss, optim.py:91-108 ------------------------------------------
 * loss = sum over rays with valid & mask of |out_dir - normalize(screen_pixel - out_ori)|^2.
 * Forward accumulates into *d_loss (float64 scalar, zero it first) and, when
 * d_grad_out_dir is not NULL, writes d loss / d out_dir float64 [N,3] (zeros elsewhere).  Optional
 * (both or neither): d_list int32 [N] receives the indices of the contributing rays and *d_n_list
 * (uint32, device, zero it first) their number. */
int drt_ray_loss(const double* d_out_ori, const double* d_out_dir, const uint8_t* d_mask,
                 const double* d_screen_pixel, const uint8_t* d_valid, int64_t n_rays,
                 double* d_loss, double* d_grad_out_dir,
                 int32_t* d_list, uint32_t* d_n_list, void* stream);
/* The same loss over a list of the rays with mask = 1 (drt_render_forward's d_valid_idx / d_n_valid) instead of a pass over
 * all N rays: *d_loss += ..., and (optional, both or neither) d_rows / *d_n_rows (uint32, zero it first) = the listed rays that
 * also have a target -- what drt_render_backward_ray_loss takes. */
int drt_ray_loss_listed(const double* d_out_ori, const double* d_out_dir, const double* d_screen_pixel,
                        const uint8_t* d_valid, const int32_t* d_paths, const int64_t* d_n_paths, int64_t n_rays,
                        double* d_loss, int32_t* d_rows, uint32_t* d_n_rows, void* stream);
/* Backward helper of the loss: x[list[k], 0..2] *= *d_scale for the *d_n_list rows listed (the rows
 * drt_ray_loss reported as contributing) -- rescales d loss / d out_dir by the incoming scalar
 * gradient without another pass over the dense [N,3] tensor. */
int drt_scale_rows3(double* d_x, const int32_t* d_list, const uint32_t* d_n_list,
                    const double* d_scale, void* stream);

/* Zero `bytes` bytes at d_buf on the library's idle stream (the build stream: free between a forward's join and the next build), after
 * everything already enqueued on `stream`.  A later drt_render_forward on this scene whose d_out_ori, d_out_dir or d_mask IS d_buf (same
 * pointer, the matching size) does not fill that output again -- the fill of the NEXT step's outputs then runs beside the caller's loss /
 * backward / optimiser kernels instead of beside the next forward.  Up to three buffers may be pending; entries are forgotten at the next
 * drt_render_forward.  The reference has no counterpart: its outputs are torch.zeros of every call (DiffRender.py:421-423).
 * drt_prefill_wait: `stream` waits for every zeroing enqueued so far and the pending entries are forgotten -- what a caller does before it
 * releases such a buffer WITHOUT rendering into it (its allocator may hand the memory to work on `stream`); drt_destroy waits by itself. */
int drt_prefill_zero(drt_scene_t* s, void* d_buf, int64_t bytes, void* stream);
int drt_prefill_wait(drt_scene_t* s, void* stream);
/* The outputs of an EARLIER drt_render_forward (same scene or not) offered again as the outputs of the next one of `n_rays` rays: they
 * are zeros in every row but the rows that call listed in d_valid_idx / d_n_valid (a call's dense outputs are zero wherever its mask is
 * -- the reference's torch.zeros + index_put, DiffRender.py:421-431 -- and its list of completed paths is exactly the set rows), so
 * zeroing THOSE rows (51 B per listed row) leaves the three buffers as freshly zeroed ones, and the next drt_render_forward on this scene
 * with exactly these pointers does not fill them again.  The zeroing kernel is enqueued BY that drt_render_forward (same `stream`: behind
 * the fork of its internal pipelines when the call is a trusted-grid one, in front of it otherwise; by the next drt_outputs_clean if no
 * render call comes in between) (the fills are 51 B per RAY: 3.85 GB of the
 * 72 x 1024^2 step, its one HBM-bound stage).  The caller vouches that nothing else wrote the buffers since that earlier call and that
 * nobody else still reads them (drt_amd/diffrender.py: storage use counts and version counters); entries are forgotten at the next
 * drt_render_forward, like drt_prefill_zero's.  Not while a graph is being captured. */
int drt_outputs_clean(drt_scene_t* s, double* d_out_ori, double* d_out_dir, uint8_t* d_mask, int64_t n_rays,
                      const int32_t* d_valid_idx, const int64_t* d_n_valid, void* stream);
/* Withdraws a drt_outputs_clean request that no drt_render_forward has taken yet (the caller could not make the render call after all:
 * an allocation failed in between): the library forgets the five pointers without touching the memory.  No-op without a pending request.
 * A drt_render_forward that returns an error withdraws the request (and every other pointer registered for it) by itself. */
int drt_outputs_cancel(drt_scene_t* s);
/* Temporal hit seeds for the NEXT drt_render_forward / drt_render_ray_loss_fused on this scene of exactly `n_rays` rays (one shot; a call
 * of another size ignores and forgets them).  d_seed_face2: int32 [n_rays], caller-owned, one entry per camera ray: the face id the
 * REFRACTED ray of that pixel hit (traversal #2 of reference DiffRender.py:542) in an earlier call on the same rays, -1 for none -- any
 * other value outside [0, F) is ignored, so a buffer that outlived a topology change is harmless.  The call tests that triangle first and
 * starts the traversal with its distance as the bound, then writes the face it found back into the buffer (entries of rays without a
 * second hit keep their value).  Results are identical bit for bit with any buffer content (drt_amd/csrc/drt_trace_kernel.h TraceSeed):
 * the optimisation loop moves vertices by at most lr x clamp per step (reference optim.py:155-171), so last step's face is nearly always
 * this step's -- what the seed buys is node visits.  The reference has no counterpart (OptiX Prime keeps no state between queries).
 * The buffer must stay valid until the call it is consumed by has finished on its stream.  DRT_HIT_SEED=0 disables.  The ORDER of the
 * entries is the library's business (ray number, or 4 x 4-pixel tiles of the image for whole-image calls: fewer cache lines per wave); a
 * caller only ever initialises the buffer (-1) and hands it back. */
int drt_render_seed(drt_scene_t* s, int32_t* d_seed_face2, int64_t n_rays);
/* ray_loss (reference optim.py:91-108) AND its vertex gradient in one pass over the forward's list of completed paths
 * (drt_render_forward's d_valid_idx / d_n_valid, face ids from the same call): *d_loss += the loss (float64 scalar, zero it first)
 * and d_grad_verts float64 [V,3] += d loss / d vertices with a UNIT seed (the caller scales it by the incoming gradient of the loss:
 * the loss is a scalar, its backward through render_transparent is linear in that seed).  Replaces drt_ray_loss_listed followed,
 * in the backward pass, by drt_render_backward_ray_loss when out_dir is the tensor drt_render_forward produced. */
int drt_ray_loss_listed_grad(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir, int64_t n_rays,
                             double ior_int, double ior_ext, const int32_t* d_face1, const int32_t* d_face2,
                             const double* d_screen_pixel, const uint8_t* d_valid, const int32_t* d_paths, const int64_t* d_n_paths,
                             double* d_loss, double* d_grad_verts, void* stream);
/* The same, started EARLY on the part of the list that is ready early: a drt_render_forward cut into sub-batches keeps the completed paths
 * of its first sub-batch as the head of d_valid_idx (never moved by the join); when d_paths is that list, the head is processed on the
 * internal stream that produced it -- beside the tail of the other pipeline -- and only the rest behind the join on `stream`, which then
 * waits for both.  PRECONDITIONS (the caller's): d_loss and d_grad_verts were zeroed on `stream` BEFORE that drt_render_forward was
 * enqueued, and d_screen_pixel / d_valid were complete by then.  Any other list, or a capture: exactly drt_ray_loss_listed_grad. */
int drt_ray_loss_listed_grad_split(drt_scene_t* s, const double* d_verts, const double* d_origin, const double* d_dir, int64_t n_rays,
                                   double ior_int, double ior_ext, const int32_t* d_face1, const int32_t* d_face2,
                                   const double* d_screen_pixel, const uint8_t* d_valid, const int32_t* d_paths, const int64_t* d_n_paths,
                                   double* d_loss, double* d_grad_verts, void* stream);
/* Arms the NEXT drt_render_forward on this scene of exactly `n_rays` rays with its ray loss (one shot, like drt_render_seed: a call of
 * another size drops the registration, a call that fails clears it).  d_screen_pixel float64 [n_rays,3] and d_valid uint8 [n_rays] are the
 * targets of drt_ray_loss_listed_grad; d_loss and d_grad_verts its two accumulation targets (float64, or cells in deterministic mode).
 * The armed call does drt_ray_loss_listed_grad's work itself: every sub-batch enqueues, on its own internal stream behind its last
 * traversal and in front of the join, the loss + unit-seed vertex gradient of the paths IT completed (a walk over its list of exit rays,
 * the arithmetic of drt_ray_loss_listed_grad; rays with d_valid[i] = 0 are traced and written like any other and add nothing).  When the
 * call returns, `*d_loss` and `d_grad_verts` are ordered on `stream` like its other outputs, and no pass over the list of completed
 * paths is needed any more; that list, the dense outputs and the face ids are written as without the arm.
 * PRECONDITIONS (the caller's, those of drt_ray_loss_listed_grad_split): the accumulators were zeroed on `stream` BEFORE the render call is
 * enqueued, the targets are complete by then, and all four stay valid until the call has finished on its stream.
 * The call DECLINES the arm -- nothing is added to the accumulators, the caller takes drt_ray_loss_listed_grad afterwards -- while a
 * graph is being captured on `stream` and when any of its sub-batches would take the one-kernel path (DRT_MEGA_MAX_LOG2), which keeps no
 * list of exit rays.  Every other route serves it, the establishing and the untrusted (k_cull) calls included: they leave the same list.
 * An armed call cut into sub-batches appends part of its list of completed paths on `stream` itself, so a drt_ray_loss_listed_grad_split on
 * that list runs as the plain form.
 * drt_render_loss_taken: 1 when the LAST drt_render_forward on this scene took an arm, 0 when it had none or declined it. */
int drt_render_loss_arm(drt_scene_t* s, const double* d_screen_pixel, const uint8_t* d_valid, double* d_loss, double* d_grad_verts,
                        int64_t n_rays);
int drt_render_loss_taken(drt_scene_t* s);
/* Adjoint of drt_render_forward followed by drt_ray_loss, for the rays drt_ray_loss listed (d_rows / *d_n_rows):
 * grad_verts [V,3] += *d_scale * d ray_loss / d vertices.  Equivalent to drt_scale_rows3 + drt_render_backward with the
 * dense d loss / d out_dir, without that [N,3] tensor (zero in all but the listed rows) ever being written or read:
 * the loss gradient of a listed ray is recomputed from its path. */
int drt_render_backward_ray_loss(drt_scene_t* s, const double* d_verts, const double* d_origin,
                                 const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                                 const int32_t* d_face1, const int32_t* d_face2,
                                 const int32_t* d_rows, const uint32_t* d_n_rows,
                                 const double* d_screen_pixel, const double* d_scale,
                                 double* d_grad_verts, void* stream);
/* drt_render_backward_ray_loss plus the input gradients of drt_render_backward_inputs (same conventions: each optional, +=).
 * No gradient reaches d_grad_origin from this loss: it detaches out_ori, and with flat faces the exit direction does not depend on
 * the origin (the rows it touches get exact zeros added). */
int drt_render_backward_ray_loss_inputs(drt_scene_t* s, const double* d_verts, const double* d_origin,
                                        const double* d_dir, int64_t n_rays, double ior_int, double ior_ext,
                                        const int32_t* d_face1, const int32_t* d_face2,
                                        const int32_t* d_rows, const uint32_t* d_n_rows,
                                        const double* d_screen_pixel, const double* d_scale,
                                        double* d_grad_verts, double* d_grad_origin, double* d_grad_dir,
                                        double* d_grad_ior, void* stream);

/* One pass: render_transparent + ray_loss + d ray_loss / d vertices, nothing dense written.
 * *d_loss += loss, d_grad_verts [V,3] += gradient (both float64, zero them first);
 * d_n_valid (int64, may be NULL) += number of contributing rays. */
int drt_render_ray_loss_fused(drt_scene_t* s, const double* d_verts, const double* d_origin,
                              const double* d_dir, const double* d_screen_pixel,
                              const uint8_t* d_valid, int64_t n_rays, double ior_int,
                              double ior_ext, double* d_loss, double* d_grad_verts,
                              int64_t* d_n_valid, int tile_w, int tile_h,
                              int grid_mode, void* d_grid_cache, void* stream);

/* ---- smoothness branch: Scene.dihedral_angle (DiffRender.py:440-443, edge_face_norm :149-163)
 * and Loss_calculator.sm_loss (optim.py:82-89) ---------------------------------------------------
 * d_e2f int64 [E,2,3]: the three vertex ids of the two faces of every unique edge (Scene.E2F).
 * forward: cos of the dihedral angle per edge, float64 [E].  backward: grad_verts [V,3] += adjoint
 * for a given d loss / d cos [E].  drt_sm_loss_fused: *d_loss += sum -log(1 + cos) and
 * grad_verts += its gradient in one pass.  (Atomic accumulation: zero the outputs first.) */
int drt_dihedral_forward(const double* d_verts, const int64_t* d_e2f, int64_t n_edges, double* d_cos, void* stream);
int drt_dihedral_backward(const double* d_verts, const int64_t* d_e2f, int64_t n_edges,
                          const double* d_grad_cos, double* d_grad_verts, void* stream);
int drt_sm_loss_fused(const double* d_verts, const int64_t* d_e2f, int64_t n_edges, double* d_loss,
                      double* d_grad_verts, void* stream);

/* ---- silhouette branch ---------------------------------------------------------------------------
 * drt_silhouette_flags <- Scene.silhouette_edge (DiffRender.py:445-457): flags uint8 [E], 1 where the
 * two faces of the edge face opposite ways seen from d_origin3 (float64 [3], device).
 * drt_edge_sample_forward <- Scene.primary_visibility + primary_edge_sample.forward
 * (DiffRender.py:459-479, 189-258) for d_edges int64 [Es,2] (vertex ids): projects both endpoints with
 * d_camera = float64 [50] = R(4x4) | K(3x3) | R^-1(4x4) | K^-1(3x3) row-major on the device, probes one
 * pixel either side of the projected midpoint with any-hit rays; writes index int64 [Es,2] =
 * trunc(midpoint x, y) and f float32 [Es] = hit(+) - hit(-) in {-1, 0, 1}.  The caller keeps edges with
 * |f| > 1e-5 (DiffRender.py:244) and in-view indices (:478): d_keep (uint8 [Es], may be NULL) = exactly that test for a
 * resx x resy image, so that the caller needs one boolean index instead of ten elementwise launches.
 * d_flags (uint8 [Es], may be NULL): d_edges is then the list of ALL unique edges and only the flagged ones (drt_silhouette_flags)
 * are silhouette edges -- the others are skipped (f = 0, keep = 0 are written for them, their index rows are left untouched) -- which
 * spares the caller the device->host round trip of compacting Edges[flags] between the two calls.
 * drt_edge_sample_backward <- primary_edge_sample.backward (DiffRender.py:263-267) chained through the
 * projection (depth row detached when detach_depth != 0, DiffRender.py:470-471):
 * grad_verts [V,3] += sum_e coef[e] * f[e] * d(-N_e . E_pos)/dV, coef float64 [Es] = incoming
 * d loss / d output per edge (0 for dropped edges).
 * drt_edge_sample_backward_rows: the same sum over the kept rows only -- d_rows int64 [n_rows] = edge row of the k-th kept sample
 * (the caller's boolean index), d_g float32 [n_rows] = d loss / d output of that sample, as autograd hands it over. */
int drt_silhouette_flags(const double* d_verts, const int64_t* d_e2f, int64_t n_edges,
                         const double* d_origin3, uint8_t* d_flags, void* stream);
int drt_edge_sample_forward(drt_scene_t* s, const double* d_verts, const int64_t* d_edges, int64_t n_edges,
                            const double* d_camera, const double* d_origin3, int64_t* d_index,
                            float* d_f, uint8_t* d_keep, int resx, int resy, const uint8_t* d_flags, void* stream);
int drt_edge_sample_backward(const double* d_verts, const int64_t* d_edges, int64_t n_edges,
                             const double* d_camera, const float* d_f, const double* d_coef,
                             int detach_depth, double* d_grad_verts, void* stream);
int drt_edge_sample_backward_rows(const double* d_verts, const int64_t* d_edges, int64_t n_edges,
                                  const double* d_camera, const float* d_f, const int64_t* d_rows, int64_t n_rows,
                                  const float* d_g, int detach_depth, double* d_grad_verts, void* stream);

/* drt_vh_term <- the loss expression of ONE view, optim.py:78 `(mask.view(resy, resx)[index[:,1], index[:,0]] - output).abs().sum()`, over
 * the samples a drt_edge_sample_forward call left in place: d_index int64 [E,2] and d_keep uint8 [E] as that call wrote them (rows with
 * keep = 0 are not read), d_soft_mask float64 [resy*resx], `output` = 0.5.  *d_loss += the sum (zero it first); d_dterm float64 [E] =
 * d term / d output per row (-sign(mask - 0.5); 0 for dropped rows) -- times the incoming gradient it is drt_edge_sample_backward's
 * `coef`.  Lets the drop-in pair evaluate the reference's own expression without compacting the samples (no device->host round trip). */
int drt_vh_term(const int64_t* d_index, const uint8_t* d_keep, int64_t n_edges, const double* d_soft_mask, int resx, int resy,
                double* d_loss, double* d_dterm, void* stream);
/* drt_edge_sample_backward with coef[e] = d_dterm[e] * float32(*d_g): drt_vh_term's per-row derivative times the incoming scalar gradient of
 * the view's term (a float64 DEVICE scalar), rounded to float32 as autograd rounds it on its way into the reference's float32 `output`
 * (DiffRender.py:251, 263-267) -- the backward of the lazily evaluated expression in one launch. */
int drt_edge_sample_backward_term(const double* d_verts, const int64_t* d_edges, int64_t n_edges, const double* d_camera, const float* d_f,
                                  const double* d_dterm, const double* d_g, int detach_depth, double* d_grad_verts, void* stream);

/* drt_vh_loss_fused <- Loss_calculator.vh_loss (optim.py:73-78) for n_views views: silhouette_edge +
 * primary_visibility + sum |soft_mask[y, x] - output| and its vertex gradient, entirely on the device
 * (the drop-in methods above return dynamically sized tensors and cost two host syncs per view; here the
 * views are traced together, 16 per launch).  d_edges int64 [E,2] = Scene.Edges, d_e2f int64 [E,2,3] =
 * Scene.E2F (same edge order).  d_cameras / d_origins / d_soft_masks are HOST arrays of n_views DEVICE
 * pointers: camera float64 [50], origin float64 [3], soft mask float64 [resy*resx].
 * *d_loss += loss, d_grad_verts [V,3] += gradient (zero them first). */
int drt_vh_loss_fused(drt_scene_t* s, const double* d_verts, const int64_t* d_edges, const int64_t* d_e2f,
                      int64_t n_edges, int n_views, const double* const* d_cameras,
                      const double* const* d_origins, const double* const* d_soft_masks, int resx, int resy,
                      int detach_depth, double* d_loss, double* d_grad_verts, void* stream);

/* drt_closest_point <- the reference's acceptance metric, "average per-vertex distance (Hausdorff
 * Distance)" against the scanned mesh, which it delegates to meshlabserver (README.md:11; no code in the
 * repository): for each query point the distance to the closest point of the scene's surface, on the same
 * LBVH.  d_points float64 [n,3] -> d_dist float64 [n]; optional (nullable) d_face int32 [n] (a face
 * attaining the minimum) and d_closest float64 [n,3].  float64 arithmetic on the tracer's float32 vertices. */
int drt_closest_point(drt_scene_t* s, const double* d_points, int64_t n, double* d_dist, int32_t* d_face,
                      double* d_closest, void* stream);

/* ---- remeshing between passes ON THE DEVICE: the geometric kernels of drt_amd/remesh_gpu.py (csrc/drt_remesh_gpu.hip) ----------
 * The data-parallel form of drt_remesh_isotropic below (same algorithm and acceptance rules; every candidate operation evaluated at
 * once, the ones whose neighbourhoods do not overlap applied together, in rounds).  d_faces int64 [F,3], d_verts float64 [V,3];
 * d_vf_start int64 [V+1] / d_vf_face int64 [3F]: vertex -> incident faces (CSR, ascending face ids; drt_rm_vertex_faces); d_vn float64
 * [V,3]: area-weighted vertex normals (drt_rm_vertex_normals).  All pointers are DEVICE pointers; everything is enqueued on `stream`.
 *   drt_rm_vertex_faces     the CSR pair of the mesh as it stands (faces whose indices are -1 -- drt_rm_kill_faces -- are in nobody's
 *                           list): count, scan, fill, each run sorted ascending; d_count int32 [V]: workspace.  With d_vn (and d_verts)
 *                           non-null also the vertex normals, summed in list order (what drt_rm_vertex_normals gives).
 *   drt_rm_split_mark       d_flag uint8 [3F]: 1 on the lo -> hi directed-edge slot c = 3 f + k of every edge longer than max_len.
 *   drt_rm_split_plan       d_rank int64 [3F] = inclusive prefix sum of d_flag (the caller's): d_mid_of_slot int64 [3F] = for every slot, on
 *                           both sides of its edge, the new vertex n_verts + rank - 1 of that edge or -1; d_count int64 [F]: faces each face
 *                           becomes (1..4).
 *   drt_rm_split_faces      d_verts float64 [V + n_split, 3] holding the old vertices: writes the midpoints behind them and, with d_offset =
 *                           exclusive prefix sum of the counts, the new faces (1 -> 2, 2 -> 3 by the shorter diagonal, 3 -> 4).
 *   drt_rm_collapse_eval_all  every directed-edge slot c = 3 f + k of d_faces a candidate (below): ok uint8 [3F] = every rule but the surface
 *                           distance; d_query float64 [3F, max_q, 3] / d_n_query int32 [3F]: the points whose distance to the input surface
 *                           is still to be checked (midpoint, centroids of the faces that survive).
 *   drt_rm_collapse_apply   claim (64-bit atomicMin of (claim / apply pair number counting down, length class, hash(edge, seed), edge index)
 *                           on d_lock uint64 [V] -- workspace, preset here when round == 0, the first round of a step; d_length float64
 *                           [3F]: edge lengths at the start of the round) what each candidate with ok = 1 writes, and apply those that
 *                           nobody with a higher priority contests: faces rewritten in place, d_f_alive / d_v_alive cleared for what
 *                           dies, *d_n_done += number applied (cumulative: the caller zeroes it).  `sub_rounds` claim / apply pairs on the
 *                           same evaluation and tables: a collapse that went ahead stamps what it read or wrote in d_dirty uint8 [V]
 *                           (workspace, cleared when round == 0) with round + 1, and later sub-rounds admit only candidates whose
 *                           vertices and rings are clean (their verdict stands).  round in 0 .. 254, consecutive within a step.
 *   drt_rm_flip_eval/apply  the same for edge flips, again one candidate per directed-edge slot (the face across the edge and the "new edge
 *                           exists already" test come from the vertex -> face lists: no edge table); d_quad int64 [3F,6] = a b c d f1 f2 of a
 *                           flip that passes; d_query float64 [3F,3] the midpoint of the new edge; n_items = 3 F; round, d_lock uint64 [V],
 *                           d_dirty uint8 [V] and sub_rounds as above.
 *   drt_rm_smooth_target    tangential relaxation targets float64 [V,3].
 *   drt_rm_face_agreement   cosine between each face normal and the consensus of its corners, float64 [F] (before a move).
 *   drt_rm_move_check       after vertices moved: every face that degenerated or folded (against d_a0) takes its three vertices back from
 *                           d_old; *d_n_bad = their number (the caller repeats, four rounds at most). */
int drt_rm_split_mark(const int64_t* d_faces, int64_t n_faces, const double* d_verts, double max_len, uint8_t* d_flag, void* stream);
int drt_rm_split_plan(const int64_t* d_faces, int64_t n_faces, const int64_t* d_vf_start, const int64_t* d_vf_face, const uint8_t* d_flag,
                      const int64_t* d_rank, int64_t n_verts, int64_t* d_mid_of_slot, int64_t* d_count, void* stream);
int drt_rm_split_faces(const int64_t* d_faces, int64_t n_faces, const int64_t* d_mid_of_slot, double* d_verts, const int64_t* d_offset,
                       int64_t* d_faces_out, void* stream);
int drt_rm_vertex_faces(const int64_t* d_faces, int64_t n_faces, int64_t n_verts, int32_t* d_count, int64_t* d_vf_start, int64_t* d_vf_face,
                        const double* d_verts, double* d_vn, const int32_t* d_live, void* stream);
int drt_rm_vertex_normals(const int64_t* d_faces, const double* d_verts, const int64_t* d_vf_start, const int64_t* d_vf_face, int64_t n_verts,
                          double* d_vn, void* stream);
int drt_rm_collapse_apply(const int64_t* d_cand, int64_t n_cand, const uint8_t* d_ok, const int64_t* d_edges, int64_t* d_faces, double* d_verts,
                          const int64_t* d_vf_start, const int64_t* d_vf_face, int64_t n_verts, double min_len, uint32_t seed, int round, const double* d_length,
                          uint64_t* d_lock, uint8_t* d_f_alive, uint8_t* d_v_alive, uint8_t* d_dirty, int sub_rounds, int32_t* d_n_done, const int32_t* d_live, void* stream);
/* Round 6: the collapse evaluation runs over EVERY directed-edge slot c = 3 f + k of d_faces (no candidate list: no stream compaction, no host round
 * trip per round).  Slots that are not the lo -> hi representative of their edge, not short, or belong to a face an earlier round killed
 * (indices -1, drt_rm_kill_faces) report ok = 0.  Outputs sized [3 n_faces]: d_edge_snap int64 [.,2] (the slot's edge at the start of the
 * round: what drt_rm_collapse_apply takes as d_edges with d_cand = NULL), d_length, d_ok, d_n_query, d_query [., max_q, 3].
 * drt_rm_surface_filter: CheckSurfDist on the device -- item i keeps d_ok[i] only if all of its d_n_query[i] (NULL: one) points
 * d_query[i][k] lie within max_dist of the surface held by scene `s` (the verdict of drt_closest_point's distance, by a search that
 * starts bounded by max_dist and ends at the first triangle inside).
 * drt_rm_kill_faces: faces with d_f_alive[f] == 0 get the indices -1 in place, and d_f_alive[f] = 1 again (all ones for the next round). */
int drt_rm_collapse_eval_all(const int64_t* d_faces, int64_t n_faces, const double* d_verts, const double* d_vn, const int64_t* d_vf_start,
                             const int64_t* d_vf_face, double min_len, double max_len, int max_q, int64_t* d_edge_snap, double* d_length,
                             uint8_t* d_ok, int32_t* d_n_query, double* d_query, int32_t* d_list_item, double* d_list_point, uint32_t* d_list_count,
                             int64_t list_cap, const int32_t* d_live, void* stream);
/* (d_list_item / d_list_point / d_list_count, optional: the query points of the candidates that passed, appended to ONE compact list of at
 * most list_cap entries -- item = slot, point [3] -- whose length stays on the device; a candidate that does not fit is left to the next
 * round.  drt_rm_surface_filter_list is drt_rm_surface_filter over that list.) */
int drt_rm_surface_filter_list(drt_scene_t* s, uint8_t* d_ok, const int32_t* d_list_item, const double* d_list_point, const uint32_t* d_list_count,
                               int64_t list_cap, double max_dist, const int32_t* d_live, void* stream);
int drt_rm_surface_filter(drt_scene_t* s, uint8_t* d_ok, const int32_t* d_n_query, const double* d_query, int64_t n_items, int max_q,
                          double max_dist, const int32_t* d_live, void* stream);
/* The projection step's query: d_closest float64 [n,3] = the closest point of scene `s` to each of d_points float64 [n,3] -- the point
 * drt_closest_point reports, by a search that starts bounded by hint_radius (> 0; the vertices of a remesh sit within a fraction of an
 * edge length of the surface) and falls back to the unbounded one for a point farther out. */
int drt_rm_closest_near(drt_scene_t* s, const double* d_points, int64_t n, double hint_radius, double* d_closest, void* stream);
int drt_rm_kill_faces(int64_t* d_faces, uint8_t* d_f_alive, int64_t n_faces, const int32_t* d_live, void* stream);
/* Round termination on the device.  d_ctl int32 [8], preset {1, 0, 0, 0, 0, ...} at the start of a step: [0] live, [1] operations applied so
 * far (pass d_ctl + 1 as d_n_done of the apply calls), [2] / [3] the previous / the first round's figures, [4] rounds that ran.
 * drt_rm_round_end, enqueued after each round, clears [0] when the round applied nothing or fewer than first / tail_cut; every
 * call above that takes d_live (= d_ctl, or NULL: always live) turns into a no-op from then on -- so the driver enqueues several rounds
 * ahead and reads d_ctl back once per batch instead of once per round. */
int drt_rm_round_end(int32_t* d_ctl, int tail_cut, void* stream);
int drt_rm_flip_eval(const int64_t* d_faces, int64_t n_faces, const double* d_verts, const double* d_vn, const int64_t* d_vf_start,
                     const int64_t* d_vf_face, double max_len, uint8_t* d_ok, int64_t* d_quad, double* d_query, const int32_t* d_live, void* stream);
int drt_rm_flip_apply(int64_t n_items, const uint8_t* d_ok, const int64_t* d_quad, int64_t* d_faces, int64_t n_verts, int round, uint64_t* d_lock,
                      uint8_t* d_dirty, int sub_rounds, int32_t* d_n_done, const int32_t* d_live, void* stream);
int drt_rm_smooth_target(const int64_t* d_faces, const double* d_verts, const int64_t* d_vf_start, const int64_t* d_vf_face, int64_t n_verts,
                         double* d_target, void* stream);
int drt_rm_face_agreement(const int64_t* d_faces, const double* d_verts, const double* d_vn, int64_t n_faces, double* d_a0, void* stream);
int drt_rm_move_check(const int64_t* d_faces, double* d_verts, const double* d_old, const double* d_vn, const double* d_a0, int64_t n_faces,
                      int64_t n_verts, uint8_t* d_revert, int32_t* d_n_bad, void* stream);

/* ---- remeshing between passes (host code; all pointers here are HOST pointers) -------------------------
 * drt_remesh_isotropic <- Meshlabserver.remesh (optim.py:12-52): MeshLab's "Remeshing: Isotropic Explicit
 * Remeshing" with Iterations=iterations (3), TargetLen=target_len, CheckSurfDist / MaxSurfDist=max_surf_dist
 * (1), and the refine / collapse / edge-swap / smooth / reproject steps selected by `flags` (all on in the
 * reference).  Input: a closed manifold, verts float64 [V,3], faces int32 [F,3].  The result is returned
 * in an opaque buffer: query its size, copy it out, free it. */
#define DRT_REMESH_SPLIT 1u
#define DRT_REMESH_COLLAPSE 2u
#define DRT_REMESH_FLIP 4u
#define DRT_REMESH_SMOOTH 8u
#define DRT_REMESH_REPROJECT 16u
#define DRT_REMESH_CHECK_DIST 32u
#define DRT_REMESH_ALL 63u
typedef struct drt_mesh_buf drt_mesh_buf_t;
int drt_remesh_isotropic(const double* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                         double target_len, int iterations, double max_surf_dist, unsigned flags,
                         drt_mesh_buf_t** out);
/* stats4 (nullable): edges split, edges collapsed, edges flipped, iterations run */
int drt_mesh_buf_size(const drt_mesh_buf_t* b, int64_t* n_verts, int64_t* n_faces, int64_t* stats4);
int drt_mesh_buf_copy(const drt_mesh_buf_t* b, double* verts, int32_t* faces);
void drt_mesh_buf_free(drt_mesh_buf_t* b);

/* ---- limit_hook + SGD step (optim.py:155-171, 215) in one pass.  d_grad is sanitised in place when max_abs > 0 (NaN -> 0, clamp to
 * +-max_abs); d_buf is torch.optim.SGD's momentum buffer (first != 0: initialised from the gradient); n = number of float64
 * elements of the parameter. */
int drt_limit_sgd_step(double* d_param, double* d_grad, double* d_buf, int64_t n, double lr, double momentum,
                       int nesterov, int first, double max_abs, void* stream);
/* The same with the weighted sum of the three loss terms in front (all_loss, optim.py:127-129): d_terms float64 [3, n] = d ray / d vertices,
 * d vh / d vertices, d sm / d vertices; d_w3 float64 [3] (device) the weights; grad[i] = (w0 t0[i] + w1 t1[i]) + w2 t2[i] before the limit;
 * optional (both or neither) d_loss_parts float64 [3] -> *d_loss_total = (w0 l0 + w1 l1) + w2 l2. */
int drt_limit_sgd_step3(double* d_param, double* d_grad, double* d_buf, int64_t n, double lr, double momentum, int nesterov, int first,
                        double max_abs, const double* d_terms, const double* d_w3, const double* d_loss_parts, double* d_loss_total, void* stream);
/* The step's tail split around ONE all-reduce over ranks (optim.ShardedIteration).  Float64: drt_weight_terms3 writes a rank's weighted
 * partial gradient d_out [n] = (w0 t0[i] + w1 t1[i]) + w2 t2[i] (the expression of drt_limit_sgd_step3) from d_terms [3, n]; after the sum
 * over ranks drt_limit_sgd_step_total is drt_limit_sgd_step that also writes *d_loss_total = (w0 l0 + w1 l1) + w2 l2 from d_loss_parts [3].
 * Deterministic: d_limbs int64 [3n + 3, 4] = the rank-summed exchange words (drt_fx_to_limbs) of 3n + 3 cells -- the three terms' gradient
 * cells (term k, element i at cell k n + i), then the three loss cells; drt_fx_limbs_limit_sgd_step3 does drt_fx_from_limbs +
 * drt_fx_finalize + drt_limit_sgd_step3 (nesterov, first, max_abs as there) in one pass, same bits, and writes the float64 loss parts
 * d_loss_parts [3] and *d_loss_total. */
int drt_weight_terms3(const double* d_terms, const double* d_w3, int64_t n, double* d_out, void* stream);
int drt_limit_sgd_step_total(double* d_param, double* d_grad, double* d_buf, int64_t n, double lr, double momentum, int nesterov, int first,
                             double max_abs, const double* d_w3, const double* d_loss_parts, double* d_loss_total, void* stream);
int drt_fx_limbs_limit_sgd_step3(const int64_t* d_limbs, int64_t n, double* d_param, double* d_grad, double* d_buf, double lr, double momentum,
                                 int nesterov, int first, double max_abs, const double* d_w3, double* d_loss_parts, double* d_loss_total, void* stream);
/* The library's own HIP streams (which = 0: the build stream, idle once the tree is built; 1 .. DRT_STREAMS: the pipeline streams, of which
 * a call below 2^25 rays uses only the first).  A process gets four hardware queues and further streams are multiplexed onto them: a
 * caller that wants side work to run BESIDE a render call -- not behind the barrier with which the caller's own stream waits for it in
 * the same hardware queue -- enqueues it on one of these (optim.FusedIteration: the silhouette and smoothness terms on pipeline stream 2). */
int drt_internal_stream(drt_scene_t* s, int which, void** out);

/* ---- topology: Scene.init_edge (DiffRender.py:338-355; trimesh group_rows / edges_face on the host in the reference) and
 * the 1 -> 4 midpoint refinement of a level-of-detail step, on the device ---------------------------------------
 * drt_edge_tables: d_faces int64 [F,3], d_verts float64 [V,3] -> d_edges int64 [3F/2,2] (ascending by (min, max) vertex),
 * d_e2f int64 [3F/2,2,3] (vertex ids of the two faces of every edge; first the face with the lower directed-edge row),
 * d_row2edge int32 [3F] (nullable: unique-edge id of directed edge 3f+j = (F[f][j], F[f][(j+1)%3])), *d_mean_len float64
 * (mean length of the 3F directed edges), *d_status int32: 0; bit 0 set when some edge is not shared by exactly two faces (the
 * mesh is not watertight, DiffRender.py:305), bit 1 when a face indexes a vertex outside [0, V) (never dereferenced); the tables
 * are then unspecified.  d_workspace: drt_edge_tables_workspace(F)
 * bytes of device memory.  Everything is enqueued on `stream`; nothing synchronises for an even 3F. */
int64_t drt_edge_tables_workspace(int64_t n_faces);
int drt_edge_tables(const int64_t* d_faces, int64_t n_faces, const double* d_verts, int64_t n_verts,
                    void* d_workspace, int64_t* d_edges, int64_t* d_e2f, int32_t* d_row2edge,
                    double* d_mean_len, int32_t* d_status, void* stream);
/* d_verts_out float64 [V+E,3] = the vertices followed by the midpoint of every unique edge (rounded through float32 when
 * round_f32, like a PLY round trip); d_faces_out int64 [4F,3]: face f -> (v0,m01,m20), (m01,v1,m12), (m20,m12,v2),
 * (m01,m12,m20) at rows 4f..4f+3.  d_edges / d_row2edge: from drt_edge_tables of the same mesh. */
int drt_subdivide_midpoint(const int64_t* d_faces, int64_t n_faces, const double* d_verts, int64_t n_verts,
                           const int64_t* d_edges, int64_t n_edges, const int32_t* d_row2edge, int round_f32,
                           int64_t* d_faces_out, double* d_verts_out, void* stream);

/* ---- the visual hull of a capture's silhouette masks (csrc/drt_hull.h states the law) ----------------------
 * A dense grid of nx x ny x nz corners (each count in [3, 1024]); corner (i, j, k) lies at lo + cell * (i, j, k) and has the linear index
 * (i * ny + j) * nz + k.  All pointers are device pointers; everything is enqueued on `stream`, nothing synchronises; a bad argument
 * gives DRT_E_INVALID with a message that names it.
 * drt_hull_field: d_masks uint8 [n_views, height, width] (nonzero = object), d_proj float64 [n_views, 3, 4] = K R[:3, :] per view ->
 * d_field float32 [nx, ny, nz]: the minimum over the views of the bilinear mask sample at the corner's projection; a view that does not
 * see the corner counts as 0 (keep_outside = 0, "carve") or is skipped (1, "keep"); corners on the six boundary planes are 0.
 * drt_hull_mark: per corner, d_edge_mask uint8 (bit c - 1: the lattice edge to the corner at offset code c = 4 dx + 2 dy + dz crosses
 * `level`, inside <=> field > (float)level), d_n_vert uint8 (its set bits) and d_n_tri uint8 (triangles of the cell that starts there).
 * drt_hull_emit: d_v_inc / d_t_inc int32 = INCLUSIVE prefix sums of d_n_vert / d_n_tri over the linear index, n_verts / n_faces their
 * totals -> d_verts float64 [n_verts, 3], d_faces int32 [n_faces, 3]: marching tetrahedra on the Kuhn subdivision, a closed oriented
 * manifold with outward normals, vertices ordered by (corner, code), triangles by (cell, tetrahedron).  Nothing is written beyond the
 * two totals. */
int drt_hull_field(const uint8_t* d_masks, int n_views, int height, int width, const double* d_proj, double lo_x, double lo_y, double lo_z,
                   double cell, int nx, int ny, int nz, int keep_outside, float* d_field, void* stream);
int drt_hull_mark(const float* d_field, int nx, int ny, int nz, double level, uint8_t* d_edge_mask, uint8_t* d_n_vert, uint8_t* d_n_tri,
                  void* stream);
int drt_hull_emit(const float* d_field, int nx, int ny, int nz, double lo_x, double lo_y, double lo_z, double cell, double level,
                  const uint8_t* d_edge_mask, const int32_t* d_v_inc, const int32_t* d_t_inc, int64_t n_verts, int64_t n_faces,
                  double* d_verts, int32_t* d_faces, void* stream);

/* ---- Gray-code pattern photographs -> screen codes, mask and ray targets (csrc/drt_decode.h states the law) ---
 * Opt-in; drt_version() stays 13: probe for the symbol.  d_frames uint8 [n_views, F, height, width]: F = 2 (nbx + nby) photographs per
 * view of a monitor of tex_w x tex_h texels (each in [2, 32768]; nbx = ceil(log2 tex_w), nby = ceil(log2 tex_h)) that shows bit after
 * bit of the Gray code of the texel column, then of the row, most significant first, every pattern followed by its complement.
 * Per pixel and bit: bit = a > b, c = |a - b|; contrast = min c; the pixel decodes iff contrast >= min_contrast (1..255) and the code
 * lies inside the texture.  d_codes int16 [n_views, height, width, 2] = (x, y), or (-1, -1); d_contrast uint8 [n_views, height, width].
 * d_background (may be NULL): the same patterns photographed without the object, [F, height, width] for all views
 * (background_view_stride = 0) or one stack per view, background_view_stride bytes apart (>= F height width).  With it, d_mask uint8
 * (may be NULL) = 255 where the background decodes and the object frames do not, or decode to a texel max(|dx|, |dy|) >= mask_shift away,
 * else 0; d_covered uint8 (may be NULL) = 1 where the background decodes.  d_positions float64 [n_views, height * width, 3] (may be
 * NULL; needs d_screens float64 [n_views, 9] = p0, eu, ev per view, a DEVICE pointer) = (p0 + x eu) + y ev, an x component that is
 * exactly 0 replaced by 1e-12, and (0, 0, 0) where the pixel does not decode or -- zero_outside_mask = 1 (needs d_background) -- lies
 * outside the mask.  The input pointers may have any alignment and the planes any size; nothing outside the stacks is read.  One
 * kernel on `stream`, no workspace, no atomics: two runs give the same bits.  A bad argument gives DRT_E_INVALID and touches nothing. */
int drt_decode_patterns(const uint8_t* d_frames, const uint8_t* d_background, int64_t background_view_stride, int n_views, int height, int width,
                        int tex_h, int tex_w, int min_contrast, int mask_shift, const double* d_screens, int zero_outside_mask, int16_t* d_codes,
                        uint8_t* d_contrast, uint8_t* d_mask, uint8_t* d_covered, double* d_positions, void* stream);

/* ---- the refracted image of the mesh in front of a textured screen (csrc/drt_image.h states the law) ---------
 * A forward renderer, opt-in, without a gradient: rows [y0, y1) of the float32 image [height, width, channels] a pinhole camera sees.
 * camera21 (HOST, 21 doubles) = K^-1 [3,3] then the top [3,4] of R^-1, row-major; screen9 (HOST) = p0, eu, ev: the world position of
 * texel (0, 0) and the world vectors of one texel step along the texture's x and y; fill_void / fill_invalid (HOST, `channels` doubles).
 * d_verts float64 [V,3], d_texture float32 [tex_h, tex_w, channels], d_image, d_hit / d_through float32 [height, width] (may be NULL):
 * device pointers.  Every expression is float64 in the stated association:
 *   sample  pixel (x, y) has s^2 samples (s = supersample, 1..4); sample j = b s + a looks through (px, py) = (x + (a + 0.5)/s - 0.5,
 *           y + (b + 0.5)/s - 0.5); p_r = (Kinv[r][0] px + Kinv[r][1] py) + Kinv[r][2], w_r = (Rinv[r][0] p_0 + Rinv[r][1] p_1) + Rinv[r][2] p_2,
 *           dir = w / sqrt((w_x^2 + w_y^2) + w_z^2), origin = Rinv[:3, 3]: at s = 1 the ray of the integer pixel centre.
 *   path    the K-interaction law of drt_render_paths_law_forward (max_bounces 2..8, law_flags DRT_LAW_REFLECT | DRT_LAW_SNELL), unchanged,
 *           with a throughput T = 1 that every REFRACTING interaction multiplies by 1 - R when `fresnel` is 1 (0: geometry only): R is the
 *           reference's FrDielectric with cos(theta_i) from the flipped normal and the eta_i, eta_t of that interaction,
 *           sinT = sqrt(clamp(1 - ci ci, 0, 1)) eta_i / eta_t, cosT = sqrt(max(1 - sinT sinT, 0)),
 *           R = (((eta_t ci - eta_i cosT) / (eta_t ci + eta_i cosT))^2 + ((eta_i ci - eta_t cosT) / (eta_i ci + eta_t cosT))^2) / 2;
 *           a mirrored (TIR) interaction leaves T alone.
 *   class   direct: no interaction at all (exit ray = camera ray, T = 1); through: the path completed validly; invalid: everything else.
 *   screen  direct and through samples with exit ray (o, d): n = eu x ev, t = (p0 - o) . n / (d . n); seen iff d . n != 0 and t > 0 (two
 *           faces; NaN fails); u = (o + t d - p0) . eu / (eu . eu), v likewise with ev; on the screen iff 0 <= u <= tex_w - 1 and
 *           0 <= v <= tex_h - 1 (texel centres at the integers): colour = T * the bilinear sample (drt_hull_field's formula, float64);
 *           otherwise fill_void; an invalid sample has fill_invalid.  The fills are not weighted.
 *   pixel   (((c_0 + c_1) + c_2) + ...) / s^2 in sample order, stored as float32; d_hit = the share of samples with at least one
 *           interaction, d_through = the share whose path completed.
 * Only rows [y0, y1) of the three outputs are written; a band gives the bits the whole image gives.  Workspace: 158 bytes per sample of the
 * band, kept by the scene: the ray lists (69) and the rows of the one-pass path call (81: parked float64 ray, hit count and its face tape,
 * which this call leaves alone), shared with those calls and scratch to each, plus one float64 throughput (8); the first call of a size allocates and cannot run inside a
 * stream capture.  Everything is enqueued on `stream`, nothing is read back.  No accumulation target: the call is the same under
 * drt_deterministic, and two runs give the same bits.  A scene without triangles renders every sample as direct.  DRT_E_INVALID (nothing
 * written): supersample outside 1..4, channels not 1 or 3, a texture side below 2, zero / non-finite / non-orthogonal axes
 * (|eu . ev| > 1e-12 |eu| |ev|), a bad max_bounces, law_flags or fresnel, an empty or inverted band or one outside the image, more than
 * 2^31 - 1 samples, a null pointer, a workspace that would have to grow inside a stream capture. */
int drt_render_image(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                     double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                     const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                     float* d_image, float* d_hit, float* d_through, void* stream);

/* ---- the photometric loss of that image, with its vertex and IOR gradients (csrc/drt_image_loss.h states the law) ---
 * drt_render_image's forward on rows [y0, y1) of one view, every forward quantity exactly as stated there, then, per pixel p of the band,
 *   I[p][ch] = the float64 pixel mean (the value drt_render_image rounds to float32),  r = I - (double)d_target[p][ch],
 *   *d_loss += w_p ((r_0^2 + r_1^2) + r_2^2),   w_p = 1, or (double)d_weight[p] with a float32 plane [height, width]
 * and the derivative of that sum w.r.t. the vertices (d_grad_verts [V,3] +=, may be NULL: the kernel then runs without its gradient
 * table), ior_int and ior_ext (d_grad_ior[0] +=, [1] +=; may be NULL), under torch's conventions.  Only THROUGH samples that land on the
 * screen carry a gradient (c = T B, seed 2 w_p r_ch / s^2): bilinear -> screen plane -> path (the adjoint of
 * drt_render_paths_law_ray_loss_ior_fused with the plane's exit seeds) and, with `fresnel`, the throughput -- every refracting
 * interaction receives the seed of T times the product of the OTHER factors, R's adjoint follows FrDielectric line by line (a root whose
 * argument is not positive is the constant 0 and passes nothing) and enters the bounce through ci = -(n . d).  Direct, void and invalid
 * samples are constants; a sample's class, the face tape, the TIR flags, the entering branch, floor and the clamp of the bilinear cell and
 * the on-screen test carry no gradient.  d_target: float32 [height, width, channels].  d_image (may be NULL): float32
 * [height, width, channels], rows [y0, y1) written with the bits of drt_render_image.  *d_count (int64, may be NULL) += the through
 * samples on the screen.  The accumulation targets are float64, or FxCell arrays under drt_deterministic (then exact: bands, runs and a
 * graph replay give the same bits).  Workspace: drt_render_image's plus 8 bytes per pixel and channel; the first call of a size allocates
 * and cannot run inside a stream capture.  Everything is enqueued on `stream`, nothing is read back.  DRT_E_INVALID as drt_render_image. */
int drt_render_image_loss(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                          double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                          const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                          const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                          int64_t* d_count, void* stream);

/* ---- ... and its gradients w.r.t. the screen's pose and the texture (csrc/drt_image_screen.h states the law) --------
 * drt_render_image_loss with two more accumulating targets, both nullable (with both NULL the call IS drt_render_image_loss):
 *   d_grad_screen   nine accumulators += d loss / d (p0, eu, ev) in that order (addressed like d_grad_ior)
 *   d_grad_texture  [tex_h, tex_w, channels] accumulators += d loss / d (double)texel, the array PADDED to a multiple of three values
 * Here the DIRECT samples carry a gradient as well as the through ones: every sample of either class that lands on the screen has the
 * colour c[ch] = T B[ch](u, v) (T = 1 on a direct sample and without `fresnel`) and the seed 2 w_p r_ch / s^2 of its pixel.  Texture: with
 * B = ((t00 (1 - fx) + t01 fx) (1 - fy)) + ((t10 (1 - fx) + t11 fx) fy) the four texels of the cell receive seed T times (1 - fx)(1 - fy),
 * fx (1 - fy), (1 - fx) fy, fx fy.  Screen: g_u = T sum_ch seed dB/dfx, g_v likewise, then the statements of `screen` above in reverse
 * (torch's quotient rule, the cross product's adjoints; eu and ev are independent inputs).  The on-screen test, floor, the clamp of the
 * cell, the orthogonality check, a sample's class and the fills carry no gradient; a sample's ray depends on neither target, so the vertex
 * and IOR gradients are drt_render_image_loss's.  One more kernel over the pixels of the band; it also runs on a scene without triangles
 * (every sample is direct).  No more workspace.  The targets are float64, or FxCell arrays under drt_deterministic.  DRT_E_INVALID as
 * drt_render_image_loss, and for a texture gradient of more than 2^31 - 1 texels. */
int drt_render_image_loss_screen(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                 double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                 const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                 const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                 int64_t* d_count, double* d_grad_screen, double* d_grad_texture, void* stream);

/* ---- ... and its gradient w.r.t. the camera (csrc/drt_image_camera.h states the law) --------------------------------
 * drt_render_image_loss_screen with one more accumulating target, nullable (with NULL the call IS drt_render_image_loss_screen):
 *   d_grad_camera   21 accumulators += d loss / d camera21 in camera21's order, K^-1 [9] then the top 3 x 4 of R^-1 [12] (addressed like
 *                   d_grad_ior)
 * Every direct and every through sample that lands on the screen carries a gradient through its camera ray.  A through sample's seeds are
 * the adjoint (g_o, g_d) of the camera ray that the reverse loop of drt_render_image_loss's path adjoint ends with, the Fresnel share of
 * the incoming direction included; a direct sample's are the screen plane's adjoint on the camera ray itself (T = 1).  Then the
 * statements of `camera21` above in reverse under torch's conventions: origin = R^-1[:, 3], dir = w / sqrt((w_x^2 + w_y^2) + w_z^2),
 * w = R^-1[:3, :3] p, p = K^-1 (px, py, 1); all 21 numbers are independent inputs (no bottom row (0, 0, 1) is assumed).  A sample's
 * class, the face tape, the TIR flags, the entering branch, floor, the clamp of the cell, the on-screen test and the fills carry no
 * gradient; silhouettes are not differentiated.  The other gradients and *d_count are drt_render_image_loss_screen's, bit for bit
 * under drt_deterministic.  The adjoint over the through samples runs whenever d_grad_camera is given (on a scene with triangles) and
 * parks the seeds; one more kernel over the pixels of the band reduces them, and it also runs on a scene without triangles (every sample
 * is direct).  Workspace: drt_render_image_loss's plus 48 bytes per sample of the band; the first call of a size allocates and cannot run
 * inside a stream capture.  DRT_E_INVALID as drt_render_image_loss_screen. */
int drt_render_image_loss_camera(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                 double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                 const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                 const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                 int64_t* d_count, double* d_grad_screen, double* d_grad_texture, double* d_grad_camera, void* stream);

/* ---- absorbing glass: Beer-Lambert attenuation in the image and in its loss (csrc/drt_image_absorb.h states the law)
 * drt_render_image / drt_render_image_loss with one more input, `sigma` (a HOST array of `channels` float64 absorption coefficients per
 * unit of mesh length, each finite and >= 0).  A sample's interior length L is the sum, in interaction order, of the hit distances t of
 * the interactions whose incoming ray travelled inside the object (refracting or mirrored; 0 for a direct sample); a through or direct
 * sample on the screen has the colour (exp(-(sigma_ch L)) T) texture_ch, the fills are not weighted, every other forward quantity is
 * drt_render_image's.  With every sigma_ch = 0 the outputs have the bits of drt_render_image / drt_render_image_loss.
 *   d_length       float32 [height, width], may be NULL: rows [y0, y1) receive the mean of L over the pixel's through samples, 0 where
 *                  there are none
 *   d_grad_sigma   `channels` accumulators += d loss / d sigma_ch (addressed like d_grad_ior), may be NULL; computed by the resolve
 *                  kernel from forward values, so also without any other gradient and on any scene
 * d_grad_verts and d_grad_ior receive the derivative of the whole law, the lengths included.  Workspace: the clear call's plus 8 bytes
 * per sample; the first call of a size allocates and cannot run inside a stream capture.  DRT_E_INVALID (nothing enqueued, no output
 * touched): everything the clear call refuses, then a NULL sigma or an entry that is negative, NaN or infinite (the message names it).
 * drt_version stays 13: probe for the symbols. */
int drt_render_image_absorb(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                            double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                            const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                            float* d_image, float* d_hit, float* d_through, const double* sigma, float* d_length, void* stream);
int drt_render_image_loss_absorb(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                 double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                 const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                 const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                 int64_t* d_count, const double* sigma, double* d_grad_sigma, void* stream);

/* ---- an environment map behind, or instead of, the screen (csrc/drt_image_env.h states the law) ------------------
 * drt_render_image with a lat-long panorama at infinity: d_env float32 [env_h, env_w, channels] (device; env_h, env_w >= 2; row 0 looks
 * along +y of the environment frame), env_rot9 (HOST, nine doubles) the row-major rotation world -> environment frame, y up, with
 * max |R R^T - I| <= 1e-12.  A direct or through sample with exit ray (o, d) takes T * texture where the screen catches it, as in
 * drt_render_image; every other such sample takes T * E(d) instead of fill_void:
 *   e_r = (R[r][0] d.x + R[r][1] d.y) + R[r][2] d.z,  theta = acos(clamp(e_y, -1, 1)),  phi = atan2(e_x, -e_z),
 *   u = ((phi / (2 pi)) + 0.5) env_w - 0.5,  v = (theta / pi) env_h - 0.5, v clamped to [0, env_h - 1], y0 = min(floor(v), env_h - 2),
 *   x0 = floor(u) in -1 .. env_w - 1 with the columns (x0 + env_w) mod env_w and (x0 + 1) mod env_w, and the bilinear formula above.
 * An invalid sample keeps fill_invalid; fill_void is checked and never used.  screen9 and d_texture may BOTH be NULL: no screen, every
 * ray sees the environment (tex_h, tex_w are then ignored; `channels` is the environment's).  d_hit / d_through are drt_render_image's.
 * reflection = 1 (needs fresnel = 1) adds the light that R takes away at the OUTER surface: a sample whose first interaction enters the
 * object (sg > 0, no TIR flag) has the reflected ray (ro, wr) of that interaction (wr = d + 2 ci n, ro = hit point + 1e-5 wr: the mirrored
 * interactions' own formula) and R1 = R of that interaction, the value whose complement entered T.  One any-hit query of the float32 cast
 * of (ro, wr) runs under the tracer contract; where it finds nothing and the sample is THROUGH, colour = T B(exit) + R1 B(ro, wr), B the
 * background of a ray as above (screen, else environment).  Classes, T, the path and the fills are unchanged.  An occluded reflection,
 * the reflection of an invalid sample and reflections off inner surfaces contribute nothing (stated losses).  d_reflect (float32
 * [height, width], may be NULL): rows [y0, y1) receive the share of a pixel's samples whose reflection was added (0 with reflection = 0).
 * Workspace: drt_render_image's; the reflection keeps the face tape of drt_render_image_loss (its row 0 is the first face) and one bit of
 * the state byte, nothing more.  DRT_E_INVALID (nothing enqueued, no output touched): a screen without a texture or the reverse, everything
 * drt_render_image refuses, then a NULL d_env, an environment side below 2, a NULL or non-orthonormal env_rot9, a reflection
 * outside {0, 1}, reflection without fresnel -- the message names the argument.  drt_version stays 13: probe for the symbol. */
int drt_render_image_env(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                         double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                         const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                         float* d_image, float* d_hit, float* d_through, const float* d_env, int env_h, int env_w, const double* env_rot9,
                         int reflection, float* d_reflect, void* stream);

/* ---- ... and its photometric loss --------------------------------------------------------------------------------
 * drt_render_image_loss with drt_render_image_env's background: the loss of drt_render_image_loss on the image of drt_render_image_env
 * (environment, optional screen, optional reflection), and the derivative of the WHOLE law w.r.t. the vertices and the two IORs.  Every
 * THROUGH sample carries a gradient (*d_count += all of them): where its exit ray lands on the screen as in drt_render_image_loss; where
 * it goes to the environment the exit ray's seed is g_o = 0 and g_d through the lookup (atan2, acos, the bilinear gradient in u, v).
 * With reflection = 1 a sample whose reflection was added also hands the seeds of (ro, wr) through the reflection's adjoint and the seed
 * of R1 through FrDielectric's adjoint and ci into the three vertices of its first face and both IORs.  The occlusion verdict, classes,
 * faces, the texel cell, the wrap column and the clamp of v carry no gradient; neither do the environment's texels or rotation.  Both
 * accumulation modes (float64 atomics, FxCell under drt_deterministic).  Workspace: drt_render_image_loss's.  DRT_E_INVALID as
 * drt_render_image_loss and drt_render_image_env. */
int drt_render_image_loss_env(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                              double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                              const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                              const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                              int64_t* d_count, const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection, void* stream);

/* ---- ... and its gradients w.r.t. the environment's texels and rotation (csrc/drt_image_env_param.h states the law) --
 * drt_render_image_loss_env with two more accumulating targets, each nullable (with both NULL the call IS drt_render_image_loss_env):
 *   d_grad_env      [env_h, env_w, channels] accumulators += d loss / d (double)texel, addressed like d_grad_texture: the array is padded
 *                   to a multiple of three values, (env_h * env_w * channels + 2) / 3 * 3 of them
 *   d_grad_env_rot  9 accumulators += d loss / d env_rot9, row-major, the nine entries taken as independent inputs (addressed like
 *                   d_grad_screen)
 * A sample reads the environment along a direction with a weight w: a direct sample that the screen does not catch (or any, without a
 * screen) along its camera ray with w = 1; a through sample whose exit ray the screen does not catch along that ray with w = T (1 with
 * fresnel = 0); and, with reflection = 1, a through sample whose reflection was added and whose reflected ray the screen does not catch,
 * along wr with w = R1.  One sample can read twice; an invalid one reads nothing.  Per read with cell, fx, fy of the lookup and the
 * pixel's seeds g_c: the four texels of the cell (wrapped columns) receive (g_c[ch] w) times the bilinear weights; g_u = w sum_ch
 * g_c[ch] dE/dfx, g_v likewise (0 outside the clamp of v), through atan2 and acos to the seed g_e of the direction in the environment
 * frame, and d_grad_env_rot[3 r + c] += g_e[r] d[c].  The on-screen test, the cell, the wrap column, the clamp of v, the orthonormality
 * check, the occlusion verdict, the class and the direction itself carry no gradient here; the other outputs are
 * drt_render_image_loss_env's, bit for bit under drt_deterministic.  One more kernel over the pixels of the band; it also runs on a
 * scene without triangles (every sample is direct).  No more workspace.  Both accumulation modes.  DRT_E_INVALID as
 * drt_render_image_loss_env, and for d_grad_env with more than 2^31 - 1 texels.  drt_version() stays 13: probe for the symbol. */
int drt_render_image_loss_env_param(drt_scene_t* s, const double* d_verts, const double* camera21, int height, int width, int y0, int y1, int supersample,
                                    double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const double* screen9,
                                    const float* d_texture, int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid,
                                    const float* d_target, const float* d_weight, double* d_loss, double* d_grad_verts, double* d_grad_ior, float* d_image,
                                    int64_t* d_count, const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection, double* d_grad_env,
                                    double* d_grad_env_rot, void* stream);

/* ---- the image term of several views in one call (csrc/drt_image_views.h states the mapping) -----------------------
 * A view table holds the cameras and screens of a capture whose views all have height x width pixels: cameras21 [n_views, 21] and
 * screens9 [n_views, 9], host arrays in drt_render_image's layouts.  drt_image_views_create checks every screen as drt_render_image
 * checks its one (DRT_E_INVALID names the row), uploads the table once (a synchronous copy: not inside a stream capture) and returns a
 * handle.  drt_image_views_destroy frees it; a table still alive when its scene is destroyed is freed with the scene, and its handle
 * must not be used afterwards. */
typedef struct drt_image_views drt_image_views_t;
 /* (drt_image_views_check: the argument checks alone -- host only, no device call) */
int drt_image_views_check(int n_views, const double* cameras21, const double* screens9, int height, int width);
int drt_image_views_create(drt_scene_t* s, int n_views, const double* cameras21, const double* screens9, int height, int width, drt_image_views_t** out);
void drt_image_views_destroy(drt_image_views_t* views);
/* The SUM over the listed views view_ids[0 .. k) (a HOST array; 1 <= k <= 16, each id in [0, n_views), repeats allowed) of what
 * drt_render_image_loss adds for each of them: *d_loss, d_grad_verts, d_grad_ior, *d_count, all accumulated into, the last three
 * nullable -- as ONE forward wavefront and ONE adjoint pass.  The listed views are stacked into a tall image of k * height rows (row r is
 * row r % height of list slot r / height); the call covers its rows [r0, r1), which may straddle a view border, and bands add into the
 * same accumulators.  Path law, supersampling, texture, fills and IORs are shared by the views; d_targets float32 [n_views, height,
 * width, channels] and d_weights float32 [n_views, height, width] (may be NULL) are the capture's stacks, indexed by view id.  The ids
 * reach the kernels by value: nothing is copied per call, and the call can be captured once a call of its size has grown the workspace
 * (drt_render_image_loss's, shared with it).  No image output and no screen, texture or camera gradients: those are
 * drt_render_image_loss_camera's.  Everything is enqueued on `stream`, nothing is read back.  DRT_E_INVALID (nothing enqueued, no output
 * touched): a NULL table or one of another scene, a bad k or id, then everything drt_render_image_loss refuses, with [r0, r1) inside
 * [0, k * height) and at most 2^31 - 1 samples. */
int drt_render_image_loss_views(drt_scene_t* s, const double* d_verts, const drt_image_views_t* views, const int* view_ids, int k, int r0, int r1,
                                int supersample, double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const float* d_texture,
                                int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid, const float* d_targets,
                                const float* d_weights, double* d_loss, double* d_grad_verts, double* d_grad_ior, int64_t* d_count, void* stream);

/* ---- ... in front of one environment ------------------------------------------------------------------------------
 * The SUM over the listed views of what drt_render_image_loss_env adds for each of them -- *d_loss, d_grad_verts, d_grad_ior, *d_count --
 * as ONE forward wavefront, ONE reflection pass and ONE adjoint pass: drt_render_image_loss_views' 26 arguments, then
 * drt_render_image_loss_env's five (d_env, env_h, env_w, env_rot9, reflection) before `stream`.  Shared by the views: the environment
 * (texels and rotation), `reflection`, the path law, supersampling, the texture, fill_invalid and the IORs; per view: camera, screen,
 * target and optional weight plane.  d_texture == NULL: no screen for any view -- the table's screens are then never read (they must
 * still have passed drt_image_views_create), tex_h and tex_w are ignored and `channels` is the environment's.  The reflected ray of a
 * sample is formed with the camera of its row's view and the row within that view.  No environment texel or rotation gradient here:
 * drt_render_image_loss_env_param has those.  Workspace: drt_render_image_loss_views'; growth inside a stream capture is refused with
 * this function's name.  Both accumulation modes.  DRT_E_INVALID (nothing enqueued, no output touched): everything
 * drt_render_image_loss_views refuses about the table and the id list, a NULL d_env (it is looked at first: without a screen it stands
 * in for the texture), everything else that call refuses (but a NULL d_texture), then an environment side below 2, a NULL or non-orthonormal
 * env_rot9, a reflection outside {0, 1}, reflection without fresnel -- the message names the argument.  drt_version() stays 13: probe for
 * the symbol. */
int drt_render_image_loss_views_env(drt_scene_t* s, const double* d_verts, const drt_image_views_t* views, const int* view_ids, int k, int r0, int r1,
                                    int supersample, double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const float* d_texture,
                                    int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid, const float* d_targets,
                                    const float* d_weights, double* d_loss, double* d_grad_verts, double* d_grad_ior, int64_t* d_count, const float* d_env,
                                    int env_h, int env_w, const double* env_rot9, int reflection, void* stream);

/* ---- ... of absorbing glass, in front of the screens, of one environment, or of both --------------------------------
 * The SUM over the listed views of one view's loss under drt_render_image_loss_absorb's law, as ONE forward wavefront, at most ONE
 * reflection pass and ONE adjoint pass: drt_render_image_loss_views' arguments up to d_count, then sigma and d_grad_sigma as in
 * drt_render_image_loss_absorb (sigma: HOST array of `channels` values, finite and >= 0; d_grad_sigma: nullable, `channels` accumulators,
 * wide in deterministic mode like d_grad_ior), then drt_render_image_loss_env's five, then d_images, before `stream`.  A through sample's
 * transmitted colour is (A_ch T) B_ch, A_ch = exp(-(sigma_ch L)); B is the texture where the exit ray lands on its view's screen and
 * otherwise, with an environment, the environment lookup -- attenuated exactly like the texture.  With reflection = 1 the sample also
 * receives R1 B(ro, wr), NOT attenuated: that light never entered the object.  d loss / d sigma_ch = -g_c[ch] sum_j L_j c_j[ch] over the
 * transmitted part of the through samples alone.  d_env == NULL: screens only -- d_texture is required and reflection must be 0.
 * d_env != NULL: drt_render_image_loss_views_env's rules; d_texture == NULL then means no screen for any view.  d_images: nullable; a
 * float32 stack [n_views, height, width, channels] in the capture's layout, of which the rendered pixels of the listed views' rows inside
 * [r0, r1) are written (a view listed twice is written twice with the same values).  With every sigma_ch = 0 the loss, both gradients and
 * the count have the bits of drt_render_image_loss_views / drt_render_image_loss_views_env in deterministic mode; the sigma partial is not
 * zero there.  No environment texel or rotation gradient.  Workspace: drt_render_image_loss_views' and the interior lengths of
 * drt_render_image_loss_absorb; growth inside a stream capture is refused with this function's name.  Both accumulation modes.
 * DRT_E_INVALID (nothing enqueued, no output touched), in this order: what drt_render_image_loss_views refuses (with an environment a NULL
 * d_texture is allowed), a NULL sigma or a coefficient that is negative or not finite, then what drt_render_image_loss_views_env refuses
 * about the environment, or reflection != 0 without one -- the message names the argument.  drt_version() stays 13: probe for the symbol. */
int drt_render_image_loss_views_absorb(drt_scene_t* s, const double* d_verts, const drt_image_views_t* views, const int* view_ids, int k, int r0, int r1,
                                       int supersample, double ior_int, double ior_ext, int max_bounces, int law_flags, int fresnel, const float* d_texture,
                                       int tex_h, int tex_w, int channels, const double* fill_void, const double* fill_invalid, const float* d_targets,
                                       const float* d_weights, double* d_loss, double* d_grad_verts, double* d_grad_ior, int64_t* d_count, const double* sigma,
                                       double* d_grad_sigma, const float* d_env, int env_h, int env_w, const double* env_rot9, int reflection, float* d_images,
                                       void* stream);

/* ---- measurement (bench.py's live per-kernel timing) --------------------------------------------
 * When enabled (on = 1; on = 2 additionally collects the traversal statistics below, which perturbs
 * timing; on = 3 runs the sub-batches of a call one after the other on ONE internal stream instead of two, so that
 * every kernel is timed alone -- the default overlaps the HBM-bound and the latency-bound kernels of two sub-batches,
 * which stretches both) every kernel of the build / forward / backward / fused pipelines is bracketed by a
 * hipEvent pair on the stream it is launched on.  drt_profile_read synchronises that stream and
 * returns, per stage, the summed kernel time in ms, the number of launches and the number of work
 * items (rays in the stage's input queue) since the previous read.  Arrays have DRT_PROFILE_STAGES
 * entries: 0 build, 1 cull, 2 trace1, 3 shade1, 4 trace2, 5 shade2, 6 trace3 (occlusion),
 * 7 finish, 8 collect (backward compaction when no list was saved), 9 backward,
 * 10 fused loss+backward, 11 projected primary visibility (fit + raster kernels), 12 pre-fill of the dense outputs (memsets, DRT_GRID_TRUST),
 * 13 the one-kernel path of small sub-batches (k_path: stages 3-7 in one launch; their rows then only carry item counts).  The event pool grows with the number of launches between two reads; if it could not
 * (allocation failure), drt_profile_read FAILS (DRT_E_INVALID, message with the number of lost timings) instead
 * of returning under-reported stage times. */
#define DRT_PROFILE_STAGES 14
int drt_profile_enable(drt_scene_t* s, int on);
/* Which stages are timed while the profile is on: bit k = stage k of the list above (default: all).  Every timed launch costs
 * two event records on its stream (~1.5 us each inside a step of ~100 launches): a measurement that only needs the traversal
 * kernels' launch times -- bench.py's timed region -- selects those and leaves the rest of the step undisturbed. */
int drt_profile_select(drt_scene_t* s, uint32_t stage_mask);
int drt_profile_read(drt_scene_t* s, double* ms_out, int64_t* launches_out, int64_t* items_out);
/* Traversal diagnostics of the last drt_profile_read interval, 4 values for each of the three
 * k_trace stages: node visits summed over wavefronts ("wave-steps"), over lanes ("lane-steps";
 * lane-steps / (64 * wave-steps) = SIMD lane utilisation), the wave-steps that were leaf (triangle) visits
 * (the others are inner-node visits), longest wavefront. */
int drt_profile_trace_stats(drt_scene_t* s, int64_t* out12);
/* Which route the sub-batches of drt_render_forward / drt_render_ray_loss_fused took: host-side counts since drt_create (no device work,
 * no synchronisation).  out8 = { sub-batches enqueued, of these: with the projected primary visibility (whole images of a multiple-of-64
 * width), as a DRT_GRID_TRUST call of it (k_patch_list + k_cull_listed), with bounce #1 inside the cull of the listed patches
 * (DRT_CULL_DIRECT, sub-batches of at least 2^DRT_CULL_DIRECT_MIN_LOG2 rays), with the refracted float64 rays parked in the rows of the
 * dense outputs (DRT_CULL_PARK), with the dense-output fills issued behind the cull stage (DRT_FILL_OVERLAP), with the wait for the tree
 * moved behind the first shading (DRT_GRID_ALL_VERIFIED), with the one-kernel back half (DRT_MEGA_MAX_LOG2) }.  The K-interaction and
 * image entry points are not counted. */
int drt_route_counts(drt_scene_t* s, int64_t* out8);
/* How the projection pass dealt its work: out2 = { k_raster launches since drt_create that took their ranges of runs from a table made of
 * the previous call's test counts, launches that dealt the runs statically } (two launches per sub-batch with a projection pass; host
 * counters, no synchronisation).  The first call on a set of rays, a call of another shape on the same workspace, a new topology and
 * DRT_RASTER_DEAL=0 deal statically, and so do launches of fewer than DRT_RASTER_DEAL_MIN_RUNS (default 16384) runs of 64 triangles of
 * one image; the results are the same bit for bit.  (DRT_RASTER_DEAL_FIXED, default 64: what a run without tests weighs in the deal,
 * in tests.) */
int drt_raster_deal_counts(drt_scene_t* s, int64_t* out2);

/* Debug builds (hipcc -DDRT_CHECK=1): the persistent traversal kernels assert the invariants of their bound-check-free LDS stack
 * (csrc/drt_traverse.h FastStack) and count violations on the device.  out4 = {stores above a lane's rows, pops of an empty stack,
 * overwritten guard rows, visits that started with an illegal stack} since the library was loaded (host-synchronising); every entry
 * is -1 in a build without the checks. */
int drt_check_violations(int64_t* out4);

#ifdef __cplusplus
}
#endif
#endif /* DRT_HIP_H */
