"""Boundary B2: the ``Scene`` surface of the reference's DiffRender.py, on the HIP path.

``import drt_amd.diffrender as Render`` is a drop-in for the reference's
``import DiffRender as Render`` (optim.py:6) for everything its optimisation loop
touches:

    Scene(mesh_path, cuda_device=0)                   DiffRender.py:298-301
    .update_mesh(path) / .update_verticex(vertices)   DiffRender.py:303-317, 378-384
    .render_transparent(origin, ray_dir)              DiffRender.py:420-432
    .optix_intersect(ray) / .render_mask(...)         DiffRender.py:386-392, 434-438
    .silhouette_edge / .primary_visibility            DiffRender.py:445-479
    .dihedral_angle() / .mean_len / .vertices / .mesh DiffRender.py:440-443, 345
    module globals intIOR, extIOR, resy, resx, device, Float   DiffRender.py:15-21

All per-ray and per-edge work runs in hand-written gfx950 kernels (libdrt_hip.so);
PyTorch only owns the tensors and the autograd plumbing.  Gradients reach
``vertices`` -- hidden in ``self`` by the reference -- through
``torch.autograd.Function``s that take it as an explicit input.
"""
from __future__ import annotations

import collections
import ctypes
import os
import warnings
import weakref

import numpy as np
import torch

from . import _lib, det, mesh_io
from ._util import _f64c, _flag_bytes, _stats, _warn_once, _warned  # noqa: F401
from .optix_mesh import optix_mesh, _stream, _on
from .stepwise import Intersection, StepwiseMixin  # noqa: F401  (Dintersect / refract_ray / trace2 / project_vert)
from .silhouette import (LazyColumn, LazyDiff, LazyGather, LazyIndex, LazyOutput, LazySum, LazyTerm, SampleSet, SilhouetteEdges,  # noqa: F401
                         _Dihedral, _EdgeSample, _SmLossFused, _VhLossFused, _VhTermLazy, enqueue_sm_term, enqueue_vh_term, force, pack_camera)

def cache_report(reset=False):
    """Counters of the transparent caches of this module: grid verdict cache (`grid_trust` calls that relied on a verdict, `grid_establish`
    calls that read and verified every ray, `grid_off` calls without whole-image hints / with GRID_CACHE off, `grid_unattachable` ray tensors
    that take no attributes), output recycling (`recycle_take` calls that rendered into pooled buffers; `recycle_miss_held` the pool had an
    entry of that size but the caller still holds, or wrote, its outputs; `recycle_miss_empty` nothing pooled yet; `recycle_off_capture` inside
    a graph capture; `recycle_off_small` below RECYCLE_MIN_RAYS), hit seeds (`seed_armed`), the loss done by the render call (`loss_armed` calls that took
    it, `loss_arm_declined`, `loss_arm_used` ray_loss calls that issued no native call, `loss_arm_dropped` that could not use it), the one-pass K-interaction term (`paths_fused_calls`; with the IOR gradient `paths_ior_fused_calls`), and the
    switches in force."""
    out = dict(_stats)
    out["switches"] = {"GRID_CACHE": GRID_CACHE, "RECYCLE_OUTPUTS": RECYCLE_OUTPUTS, "storage_use_count_available": hasattr(torch._C, "_storage_Use_Count"),
                       "RECYCLE_MIN_RAYS": RECYCLE_MIN_RAYS, "PREFILL_NEXT": PREFILL_NEXT, "HIT_SEED": HIT_SEED, "GRID_CANARY": GRID_CANARY}
    if reset:
        _stats.clear()
    return out


debug = False
resy = 960
resx = 1280
Float = torch.float64
device = "cuda"
extIOR, intIOR = 1.00029, 1.5      # floats, or 0-dim float64 tensors (CPU or GPU, requires_grad for a learnable IOR: see _ior_host)


def _ior_host(x, what):
    """The float value of an index of refraction.  A tensor (0-dim, e.g. a learnable float64 leaf) is read to the host ONCE per render
    call -- for a GPU tensor a device->host copy that waits for the work queued in front of it; a graph capture cannot do that read."""
    if not isinstance(x, torch.Tensor):
        return float(x)
    if x.numel() != 1:
        raise ValueError(f"{what} must be a float or a 0-dim tensor, got shape {tuple(x.shape)}")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what} is a tensor: its value is read to the host by every render call, which a graph capture cannot do "
                           "(capture with a float IOR; a learnable IOR belongs to the eager loop)")
    return float(x.detach())


def _ior_args(ior_int, ior_ext):
    """(float values, the tensors among them or None -- what autograd may track) of a call's ``ior_int`` / ``ior_ext`` arguments."""
    return (_ior_host(ior_int, "ior_int"), _ior_host(ior_ext, "ior_ext")), tuple(x if isinstance(x, torch.Tensor) else None for x in (ior_int, ior_ext))


def _wants_input_grads(*xs):
    """True when autograd would need d / d x for one of these render inputs (rays, IORs): tensors that require grad, grad mode on."""
    return torch.is_grad_enabled() and any(isinstance(x, torch.Tensor) and x.requires_grad for x in xs)


class Ray:
    """Ray bundle record (reference DiffRender.py:269-283); ray_ind defaults to arange."""

    def __init__(self, origin, direction, ray_ind=None):
        self.origin = origin
        self.direction = direction
        self.ray_ind = torch.arange(len(origin), device=origin.device) if ray_ind is None else ray_ind
        assert len(self.direction) == len(self.ray_ind)

    def select(self, mask):
        return Ray(self.origin[mask], self.direction[mask], self.ray_ind[mask])

    def __len__(self):
        return len(self.ray_ind)


def _tile_hint(n_rays):
    """(image width, image height) for the pipeline when the ray list is whole images of the module's resx x resy (as
    produced by generate_ray, reference captured_data.py:23-40; the module globals are what optim.py:180-181 sets):
    16x4-pixel tile ray grouping and projected primary visibility.  A hint only -- the library checks every ray against
    the grid it fits and falls back to the tree; (0, 0) = no assumption."""
    if resx >= 64 and resx % 64 == 0 and resy % 4 == 0 and n_rays % (resx * resy) == 0:
        return int(resx), int(resy)
    return 0, 0


DENSE_FACE_IDS = False  # True: Scene.last_face1 / last_face2 hold -1 for every ray without a hit (diagnostics, tests); False: only the entries of
                        # the rays with mask = 1 are defined (all the backward needs), which saves filling 8 bytes per ray
GRID_CACHE = True      # remember, per (origin, ray_dir) tensor pair, that its images verified as pinhole grids (see _grid_cache)
_GRID_BYTES = 104      # DRT_GRID_CACHE_BYTES of include/drt_hip.h


# Temporal hit seeds (include/drt_hip.h drt_render_seed): a ray tensor that comes back (TRUST mode of the grid cache below) carries an
# int32 [N] buffer with the face each pixel's refracted ray left the object through in the previous call on it; the traversal of the
# refracted rays starts from that triangle's distance.  Bit-identical results with any buffer content; 4 B per ray next to the 96 B of the
# ray itself.  Created outside graph captures only (a captured fill would reset the seeds at every replay).
# OFF by default (round 5, measured on MI355X, 72 x 1024^2): right seeds take 5 % of the node visits and 6 % of the vector instructions off
# the traversal of the refracted rays (0.394 -> 0.368 ms per launch with the GPU to itself) -- and nothing off the step (1.80 vs 1.82 ms,
# 7.08 vs 7.10 with the object filling the image), while the launch moves 55 % more HBM bytes (a 4-byte gather and scatter per ray into a
# 300 MB array).  A refracted ray starts ON the surface: its visits are the boxes around its origin and along the chord to the exit point,
# which no distance bound removes.  DRT_HIT_SEED=1 / HIT_SEED = True turns them on (tests/test_gpu_seed.py runs with them on).
HIT_SEED = os.environ.get("DRT_HIT_SEED", "0") != "0"
GRID_CANARY = os.environ.get("DRT_GRID_CANARY", "1") != "0"      # (read by the library itself at scene creation; here for cache_report)


def _hit_seed(ray_dir, n):
    if not HIT_SEED:
        return None
    seed = getattr(ray_dir, "_drt_seed2", None)
    if seed is not None and seed.shape[0] == n and seed.device == ray_dir.device:
        return seed
    if torch.cuda.is_current_stream_capturing():
        return None
    seed = torch.full((n,), -1, dtype=torch.int32, device=ray_dir.device)
    try:
        ray_dir._drt_seed2 = seed
    except Exception:
        return None
    return seed


def _arm_seed(handle, grid, n):
    """Registers the seeds of this call's ray tensor (third entry of _grid_cache's result) with the library: consumed by the next render call."""
    seed = grid[2] if len(grid) > 2 else None
    if seed is not None:
        _stats["seed_armed"] += 1
        _lib.check(_lib.lib().drt_render_seed(handle, seed.data_ptr(), n))


def _grid_cache(origin, ray_dir, n, w, h):
    """(grid_mode, cache tensor or None, hit seeds or None) for a render call on these ray tensors.

    The views of a capture are constants of the optimisation: the same tensor objects come back every iteration.  The
    first call on a pair ESTABLISHES, on the device, which of its images are pinhole ray grids in every single ray
    (drt_raster.h); the record -- a small device buffer -- is kept on the ``ray_dir`` tensor object together with the
    identity of ``origin`` and both tensors' in-place version counters, and later calls TRUST it as long as those
    match: the library then does not re-read the rays of pixels nothing projects onto.  Any in-place write to either
    tensor bumps its version and the next call re-establishes.  ``t.data = ...`` and writes through raw pointers (a DLPack / NumPy
    export of the tensor's memory, a kernel of the caller's own) are not seen by the version counter; what catches them is on the device:
    every trusted call re-verifies, per image, the 8 x 8 lattice of rays its model was fitted on AND 64 more rays at pixels that change from
    call to call (k_check_views' canary), and an image that fails is verified ray by ray from then on.  A partial overwrite of a fraction f
    of an image's rays therefore survives a call with probability (1 - f)^64; a caller who writes single rays behind autograd's back must
    set GRID_CACHE = False (or bump the version: ``t.add_(0)``)."""
    if not GRID_CACHE or w <= 0 or h <= 0 or n == 0:
        _stats["grid_off"] += 1
        return 0, None
    rec = getattr(ray_dir, "_drt_grid", None)
    key = (n, w, h, origin._version, ray_dir._version, origin.data_ptr(), ray_dir.data_ptr())
    if rec is not None and rec[0] == key and rec[1]() is origin:
        if rec[3][0] is None and not torch.cuda.is_current_stream_capturing():
            # first call after the establishing one (not while a graph is being captured: the read-back synchronises): read the verdicts back once (one host sync per ray tensor, not per step).
            # All images verified in all rays -> DRT_GRID_ALL_VERIFIED: the launches that serve other rays are not issued.
            flags = rec[2].view(-1, _GRID_BYTES)[:, 96:104].contiguous().view(torch.int32)
            rec[3][0] = bool((flags != 0).all().item())
        _stats["grid_trust"] += 1
        return 2 | (32 if rec[3][0] else 0), rec[2], _hit_seed(ray_dir, n)
    cache = torch.zeros((n // (w * h)) * _GRID_BYTES, dtype=torch.uint8, device=ray_dir.device)
    try:
        ray_dir._drt_grid = (key, weakref.ref(origin), cache, [None])
    except Exception:           # a tensor that takes no attributes: no cache
        _stats["grid_unattachable"] += 1
        _warn_once("grid_unattachable", "the ray_dir tensor takes no attributes: no grid verdict cache for it (every call verifies every ray)")
        return 0, None
    _stats["grid_establish"] += 1
    return 1, cache


class RayBinding:
    """An explicit handle for the rays of a capture (round 6): ``handle = scene.bind_rays(origin, ray_dir[, screen_pixel, valid])``, then
    ``scene.render_transparent(handle)`` every iteration.  The reference hands its loop fresh copies of constant tensors per call
    (captured_data.py:44-59); the drop-in signature therefore has to RECOGNISE constants (tensor identity, version counters, storage use
    counts: `_grid_cache`, `_OutputPool` below).  A caller that can say so instead gets the same fast path by CONTRACT:

      * the bound tensors are constants -- whether their images are pinhole grids is established on the device by the first call and
        trusted afterwards (still re-checked per call on the 8 x 8 lattice + 64 canary rays per image; an in-place write bumps the version
        counter and re-establishes);
      * the handle OWNS one set of dense outputs: the tensors a call returns -- and the autograd graph behind them -- are valid until the NEXT
        ``render_transparent(handle)``; that call zeroes the rows this one set (55 B per completed path instead of a 51 B-per-ray fill)
        and renders into the same memory.  ``backward()`` of a call whose outputs were recycled raises.  No storage use counts, no
        private torch API, works the same inside a graph capture (replay = recycle);
      * targets bound with the rays are known to be complete before any render call: the loss + gradient pass may start on the first
        sub-batch while the second is still tracing (SPLIT_LOSS) without the identity bookkeeping of `_targets_seen_before`."""

    class Shared:
        """The output set(s) and call counter of one handle -- or of several handles that agree to share them (``shared=``: the views of one
        capture, rendered one per iteration: a call on ANY of them recycles the outputs of the previous call on any of them)."""

        def __init__(self):
            self.sets, self.gen = {}, 0

    def __init__(self, scene, origin, ray_dir, screen_pixel=None, valid=None, shared=None):
        self.scene = scene
        self._shared = shared if shared is not None else RayBinding.Shared()
        self.origin, self.ray_dir = _f64c(origin.detach(), "origin"), _f64c(ray_dir.detach(), "ray_dir")
        if self.origin.shape != self.ray_dir.shape or self.origin.dim() != 2 or self.origin.shape[1] != 3:
            raise RuntimeError("bind_rays: origin and ray_dir must both be float64 [N, 3]")
        self.n = self.origin.shape[0]
        self.targets = (screen_pixel, valid) if screen_pixel is not None else None
        self._cache = self._verdict = self._versions = self._seed = self._hint = None

    def _grid(self):
        """(grid_mode, verdict cache, hit seeds) of the next render call on the bound rays."""
        w, h = _tile_hint(self.n)
        versions = (self.origin._version, self.ray_dir._version, w, h)
        if not GRID_CACHE or w <= 0 or self.n == 0:
            return 0, None
        if self._cache is None or versions != self._versions:
            self._cache = torch.zeros((self.n // (w * h)) * _GRID_BYTES, dtype=torch.uint8, device=self.ray_dir.device)
            self._versions, self._verdict = versions, None
            _stats["grid_establish"] += 1
            return 1, self._cache
        if self._verdict is None and not torch.cuda.is_current_stream_capturing():
            flags = self._cache.view(-1, _GRID_BYTES)[:, 96:104].contiguous().view(torch.int32)
            self._verdict = bool((flags != 0).all().item())          # one host sync per handle, ever
        _stats["grid_trust"] += 1
        if HIT_SEED and self._seed is None and not torch.cuda.is_current_stream_capturing():
            self._seed = torch.full((self.n,), -1, dtype=torch.int32, device=self.ray_dir.device)
        return 2 | (32 if self._verdict else 0), self._cache, (self._seed if HIT_SEED else None)

    def _outputs(self):
        """The handle's output set, in the layout of an _OutputPool entry; zero-filled once."""
        dev, sets = self.origin.device, self._shared.sets
        ent = sets.get((self.n, dev))
        if ent is None:
            n = self.n
            bases = (torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 3), dtype=torch.float64, device=dev),
                     torch.zeros((n, 3), dtype=torch.uint8, device=dev))
            ent = sets[(n, dev)] = [n, dev, None, bases, None, torch.empty(n, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)]
        return ent

    @property
    def gen(self):
        """render calls made on this handle (or the handles it shares outputs with): what the autograd graph of an EARLIER call checks in its backward"""
        return self._shared.gen

    def release(self):
        self._shared.sets.clear()
        self._shared.gen += 1


# ray_loss's gradient w.r.t. out_dir is zero in all but a few per cent of the rows.  When the out_dir handed to
# ``ray_loss`` is the very tensor ``render_transparent`` returned, the two autograd nodes exchange that gradient as a ROW
# LIST instead of a dense float64 [N,3] tensor (1.8 GB per 72 x 1024^2 step, written once and read once): ray_loss's
# backward queues (rows, targets, scale) on the link and returns a stride-0 zero tensor; render_transparent's backward
# adds the queued rows (drt_render_backward_ray_loss) to whatever dense gradient other consumers of out_dir produced.
# The values are identical.  What it cannot serve is a caller who asks autograd for d loss / d out_dir ITSELF
# (torch.autograd.grad(loss, out_dir), out_dir.retain_grad()): set SPARSE_LOSS_GRAD = False for that.
SPARSE_LOSS_GRAD = True
# On top of that: when ray_loss is given render_transparent's own, untouched (out_ori, out_dir, mask), its forward pass already computes
# d loss / d vertices with a unit seed next to the loss (ONE pass over the completed paths: drt_ray_loss_listed_grad) and the backward pass
# only scales that stash by the incoming gradient -- instead of a loss pass now and a second pass over the same paths (recompute,
# adjoint, scatter) in render_transparent's backward.  Costs the gradient's work to a caller who needs grad mode on but never calls
# backward(); set EAGER_LOSS_GRAD = False for that.
EAGER_LOSS_GRAD = True
# The dense outputs are zeros in all but a few per cent of the rows, and writing those zeros (51 B per ray) is the one HBM-bound stage of a
# render_transparent call.  With PREFILL_NEXT a call in trusted-grid mode allocates the out_ori and mask of the NEXT call of the same size
# right away and has the library zero them on its idle stream (drt_prefill_zero) -- i.e. while the caller's loss, backward and optimiser
# kernels run, which leave the memory system idle -- instead of beside the next call's traversal.  The tensors a call returns are its own
# fresh allocations either way (nothing is ever handed out twice); the price is one extra out_ori + mask (27 B per ray) held between calls.
PREFILL_NEXT = os.environ.get("DRT_PREFILL_NEXT", "1") != "0"
PREFILL_MIN_RAYS = int(os.environ.get("DRT_PREFILL_MIN_RAYS", 1 << 25))          # below this the two extra allocations and calls cost the host more than the earlier fill saves the GPU (18 views x 1024^2: +3 %, 9 views: +4 %)


# RECYCLE_OUTPUTS goes further: a call's outputs are zeros wherever its mask is, and its list of completed paths names exactly the other
# rows.  The library keeps its own reference to the three buffers of a trusted-grid call (`_OutputPool`); once the caller has let go of
# them -- the storages' use counts are back to the pool's own, the version counters unmoved (an in-place write by the caller would
# show), same stream -- the NEXT call of that size zeroes the listed rows (drt_outputs_clean: 51 B per completed path instead of 51 B
# per ray) and renders into the same memory: no fill of the dense outputs at all (72 x 1024^2: 2.38 -> 1.8 ms per step).  What a call
# returns are fresh tensor objects (detached aliases: same storage, same version counter) that nothing else references; a caller who
# keeps its outputs alive simply gets fresh allocations and the fills, as before.  The price in memory: the usual loop rebinds
# `out = render()` only after the call has returned, so the previous outputs are still held when the pool is asked and the pool ping-pongs
# between TWO entries: two output sets plus their two row lists (2 x 55 B per ray) stay resident per scene (`Scene.release_outputs()`
# drops them).  Inside a graph capture a pooled set becomes the graph's own (replay = recycle: `graph_set` in _RenderTransparent.forward).
# (The use count of a storage is read through torch._C._storage_Use_Count, which torch's own CUDA-graph trees rely on; a torch without it
# simply does not recycle.  As with any caching allocator, a caller who used the outputs on ANOTHER stream must have ordered that work in front
# of the stream of its next render call before dropping them.)
RECYCLE_OUTPUTS = os.environ.get("DRT_RECYCLE_OUTPUTS", "1") != "0" and hasattr(torch._C, "_storage_Use_Count")
if os.environ.get("DRT_RECYCLE_OUTPUTS", "1") != "0" and not RECYCLE_OUTPUTS:
    warnings.warn("drt_amd.diffrender: this torch has no torch._C._storage_Use_Count -- render_transparent cannot tell when its previous outputs "
                  "were released and fills fresh ones every call (about a quarter slower at 72 x 1024^2); see cache_report()", RuntimeWarning)
RECYCLE_MIN_RAYS = int(os.environ.get("DRT_RECYCLE_MIN_RAYS", 1 << 22))


def _use_count(t):
    return torch._C._storage_Use_Count(t.untyped_storage()._cdata)


class _OutputPool:
    """The dense outputs of earlier trusted-grid calls, kept for re-use (see RECYCLE_OUTPUTS).  An entry:
    [n, device, stream, (out_ori, out_dir, mask) base tensors, their use counts with nobody else holding them, valid_idx, n_valid]."""
    MAX = 2

    def __init__(self):
        self.entries = []

    def take(self, n, device, stream):
        """An entry of this size whose buffers nobody else references or has written; removed from the pool."""
        for k, e in enumerate(self.entries):
            if e[0] == n and e[1] == device and (stream is None or e[2] == stream) and all(_use_count(t) == c and t._version == 0 for t, c in zip(e[3], e[4])):
                return self.entries.pop(k)
        return None

    def put(self, n, device, stream, bases, counts, valid_idx, n_valid):
        self.entries.append([n, device, stream, bases, counts, valid_idx, n_valid])
        if len(self.entries) > self.MAX:
            self.entries.pop(0)


# SPLIT_LOSS: the loss + gradient pass over the completed paths of the call's FIRST sub-batch starts on the internal stream that produced
# them, beside the tail of the other pipeline, instead of behind the join (drt_ray_loss_listed_grad_split).  For that its two accumulators
# must have been zeroed before the render call was enqueued (render_transparent creates them: `_GradLink.pre`), and the targets must have
# been complete by then -- known when the very same target tensors (object, storage, version) went through ray_loss before.
SPLIT_LOSS = os.environ.get("DRT_SPLIT_LOSS", "1") != "0"
SPLIT_LOSS_MIN_RAYS = int(os.environ.get("DRT_SPLIT_LOSS_MIN_RAYS", 1 << 25))          # below, a call is not cut into sub-batches (DRT_MIN_SUB_LOG2 = 24 per sub-batch); zeroing the accumulators
                                                                                 # in front of the render call anyway (two launches off the tail, two more in front of the fork) measured +1 % at 9 and 18 views
# ARMED_LOSS: a render call on a RayBinding that carries targets does the loss pass ITSELF (drt_render_loss_arm): every sub-batch adds the
# loss + unit-seed vertex gradient of the paths it completed on its own internal stream, in front of the join, and a ray_loss on the
# call's untouched outputs with the BOUND targets issues no native call at all -- its results are `_GradLink.pre`.  Every other ray_loss
# (other targets, outputs written in place, ...) takes the routes below with fresh accumulators, and an armed result nobody asks for is
# dropped with the link.  Carries no work of its own: what it saves is the chain of dependent dispatches behind the join.
ARMED_LOSS = os.environ.get("DRT_ARMED_LOSS", "1") != "0"
ARMED_LOSS_MIN_RAYS = int(os.environ.get("DRT_ARMED_LOSS_MIN_RAYS", 1 << 24))         # measured with the arm forced on (profiles/armed_loss.txt): 18 views x 1024^2, one sub-batch,
                                                                                     # 0.805 -> 0.784 ms; 9 views 0.664 -> 0.665, nothing either way: off below 2^24 rays
_seen_targets = {}
_render_seq = [0]         # render_transparent calls enqueued so far (any scene): a clock for "was complete before THAT call"


def _targets_seen_before(sp, valid, render_seq):
    """True when these very tensors (same objects, same storage, unchanged version counters) were the targets of a ray_loss that was
    issued BEFORE the render call number ``render_seq`` was enqueued: their content was then complete before that call's fork, which is all
    the internal stream is ordered behind.  (Seen in an earlier ray_loss is not enough: render A, render B, build the targets on the
    stream, ray_loss(A, tgt), ray_loss(B, tgt) -- the second loss would find them registered although they were produced behind B's fork.)
    Registers them either way, with the current clock."""
    ok = True
    for t in (sp, valid):
        rec = _seen_targets.get(id(t))
        if not (rec is not None and rec[0]() is t and rec[1] == t._version and rec[2] == t.data_ptr()):
            ok = False
            if len(_seen_targets) > 4096:
                _seen_targets.clear()
            _seen_targets[id(t)] = (weakref.ref(t), t._version, t.data_ptr(), _render_seq[0])
        elif rec[3] >= render_seq:
            ok = False
    return ok


def _arm_targets(targets, n, device):
    """(screen_pixel, valid bytes) of a RayBinding's targets when the render call can read them as they are (float64 [n, 3] and n flags,
    contiguous, on the rays' device: the very memory ray_loss would pass on), else None -- ray_loss then reports what is wrong with them."""
    sp, valid = targets
    if not (isinstance(sp, torch.Tensor) and isinstance(valid, torch.Tensor)):
        return None
    if not (sp.dtype == torch.float64 and sp.device == device and tuple(sp.shape) == (n, 3) and sp.is_contiguous()):
        return None
    if not (valid.dtype in (torch.bool, torch.uint8) and valid.device == device and valid.numel() == n and valid.is_contiguous()):
        return None
    return sp, valid.view(torch.uint8)


class _GradLink:
    def __init__(self):
        self.armed = False     # the render call took the loss with it (ARMED_LOSS): `pre` holds the loss and the stash of the BOUND targets
        self.pre = None       # (stash zeros_like(vertices), loss zeros(())) created before the render call was enqueued (SPLIT_LOSS)
        self.seq = 0           # _render_seq of the render call this link belongs to
        self.pending = []
        self._token = None
        self.paths = None
        self.mask = None
        self.out_ori = None
        self.render = None      # (scene handle owner, vertices, origin, ray_dir, face1, face2, (ior_int, ior_ext)) of the forward call
        self.targets = None     # (screen_pixel, valid) bound with the rays (RayBinding): complete before any render call on the handle

    def token(self, n, device):
        if self._token is None or self._token.shape[0] != n:
            self._token = torch.zeros((1, 3), dtype=torch.float64, device=device).expand(n, 3)
        return self._token

    def is_token(self, g):
        t = self._token
        return t is not None and g.data_ptr() == t.data_ptr() and g.stride() == t.stride() and g.shape == t.shape


class _RenderTransparent(torch.autograd.Function):
    """render_transparent as a function of the vertices (the reference's implicit input)."""

    @staticmethod
    def forward(ctx, vertices, origin, ray_dir, scene, ior_int, ior_ext, link, grid=(0, None), binding=None):
        ior = (_ior_host(ior_int, "intIOR"), _ior_host(ior_ext, "extIOR"))
        ctx.link = link
        ctx.binding = binding
        v = _f64c(vertices.detach(), "vertices")
        o = _f64c(origin.detach(), "origin")
        d = _f64c(ray_dir.detach(), "ray_dir")
        n = o.shape[0]
        om = scene.optix_mesh            # owns the buffers zeroed ahead of time: its drt_destroy waits for the zeroing before they are released
        capturing = torch.cuda.is_current_stream_capturing()
        # gradients of the rays / IORs requested (drt_render_backward_inputs): the backward needs the list of completed paths, and
        # ray_loss hands over its row list instead of the eager vertex-only stash
        nig = ctx.needs_input_grad
        need_inputs = nig[1] or nig[2] or nig[4] or nig[5]
        ctx.need_inputs = need_inputs
        ctx.ior_like = tuple((x.shape, x.dtype, x.device) if isinstance(x, torch.Tensor) else None for x in (ior_int, ior_ext))
        need_bwd = nig[0] or need_inputs
        recycle = binding is not None or (RECYCLE_OUTPUTS and n >= RECYCLE_MIN_RAYS)  # (any grid mode: a call that verifies every ray -- no cache, or the
                                                                                  #  establishing one -- then at least does not write the dead rows again)
        # Inside a graph capture: REPLAY = RECYCLE.  A set the eager warm-up calls left in the pool is taken out of it for good and becomes the
        # graph's static outputs; the captured call zeroes the rows of the set's row list and then writes ITS list into those very buffers, so
        # every replay undoes exactly what its predecessor set (the set's state at capture time is that of the eager call that filled it
        # last: consistent with its list, which is what the first replay undoes).  No pooled set -- no warm-up call of this size since the
        # last capture -- and the capture brings fresh outputs and their fills, as before.
        graph_set = None
        pre = getattr(om, "_prefilled", None)
        if capturing:
            # a graph replays THESE launches on THESE buffers: the fills must be part of it, and nothing outside the capture may be waited
            # for inside it -- the buffers zeroed ahead of time stay where they are until the next call outside a capture
            pre = None
        else:
            om._prefilled = None
        stream_id = _stream()
        bases = counts = None
        if not recycle and RECYCLE_OUTPUTS:
            _stats["recycle_off_small"] += 1
        ent = None
        if binding is not None:
            # the handle's own set, by contract (RayBinding): the same path a captured call takes with a pooled set -- this call's list goes where
            # its predecessor's was, the set never enters the pool
            graph_set = ent = binding._outputs()
            bases, counts = ent[3], ent[4]
            binding._shared.gen += 1
            ctx.binding_gen = binding.gen
            _stats["recycle_bound"] += 1
        elif recycle:
            pool = getattr(om, "_out_pool", None)
            if pool is None:
                pool = om._out_pool = _OutputPool()
            # (a capture runs on a stream of its own: any pooled set of this size will do -- the capture is ordered behind the warm-up)
            ent = pool.take(n, o.device, None if capturing else getattr(stream_id, "value", stream_id))
            if capturing:
                _stats["recycle_graph_set" if ent is not None else "recycle_off_capture"] += 1
                if ent is None:
                    recycle = False
                else:
                    graph_set = ent                      # (registered in om._graph_sets once the captured call has gone through)
            else:
                _stats["recycle_take" if ent is not None else ("recycle_miss_held" if any(e[0] == n for e in pool.entries) else "recycle_miss_empty")] += 1
            if ent is not None:
                # the outputs of an earlier call that nobody holds any more: the rows that call set are zeroed (drt_outputs_clean, registered
                # below, right in front of the render call and behind every allocation of this one) and the call renders into the same memory
                bases, counts = ent[3], ent[4]
        took = ent if recycle and bases is not None else None
        if bases is not None:
            if pre is not None:
                with _on(o.device):
                    _lib.check(_lib.lib().drt_prefill_wait(om._h, stream_id))
                pre = None
            out_ori, out_dir, mask = bases
        elif pre is not None and pre[0] == n and pre[1] == o.device:
            out_ori, mask = pre[2], pre[3]
            out_dir = torch.empty((n, 3), dtype=torch.float64, device=o.device)
        else:
            if pre is not None:          # another size: let the zeroing finish (on this stream's timeline) before the memory goes back to the allocator
                with _on(o.device):
                    _lib.check(_lib.lib().drt_prefill_wait(om._h, stream_id))
            out_ori = torch.empty((n, 3), dtype=torch.float64, device=o.device)
            mask = torch.empty((n, 3), dtype=torch.uint8, device=o.device)
            out_dir = torch.empty((n, 3), dtype=torch.float64, device=o.device)
        pre = None
        bases_in = bases
        if recycle and bases is None:
            bases = (out_ori, out_dir, mask)
            counts = tuple(_use_count(t) for t in bases)          # with nobody but these three names holding them
        face1 = torch.empty(n, dtype=torch.int32, device=o.device)
        face2 = torch.empty(n, dtype=torch.int32, device=o.device)
        arm = None
        if need_bwd and not need_inputs and EAGER_LOSS_GRAD and link is not None and not capturing:
            if ARMED_LOSS and link.targets is not None and n >= ARMED_LOSS_MIN_RAYS:
                arm = _arm_targets(link.targets, n, o.device)
            if arm is not None or (SPLIT_LOSS and n >= SPLIT_LOSS_MIN_RAYS):
                link.pre = (det.acc(v), det.scalar(o.device))
        _render_seq[0] += 1
        if link is not None:
            link.seq = _render_seq[0]
        want_list = need_bwd or recycle
        if graph_set is not None:
            valid_idx, n_valid = graph_set[5], graph_set[6]           # this call's list goes where its predecessor's was: see above
        else:
            valid_idx = torch.empty(n, dtype=torch.int32, device=o.device) if want_list else None
            n_valid = torch.empty(1, dtype=torch.int64, device=o.device) if want_list else None
        with _on(o.device):
            # The library is handed raw pointers of buffers only this frame keeps alive (`took`: the pooled outputs and their row list):
            # nothing that can raise sits between the registration and the call that consumes it, and a call that fails withdraws them
            # itself (drt_render_forward) -- a request left behind would have the next call zero "rows" of freed memory.
            try:
                if took is not None:
                    _lib.check(_lib.lib().drt_outputs_clean(om._h, bases_in[0].data_ptr(), bases_in[1].data_ptr(), bases_in[2].data_ptr(), n,
                                                            took[5].data_ptr(), took[6].data_ptr(), stream_id))
                _arm_seed(scene.optix_mesh._h, grid, n)
                if arm is not None:       # (registered last: only a failing drt_render_forward sits between this and its consumer, and that clears it)
                    _lib.check(_lib.lib().drt_render_loss_arm(scene.optix_mesh._h, arm[0].data_ptr(), arm[1].data_ptr(), link.pre[1].data_ptr(),
                                                              link.pre[0].data_ptr(), n))
                _lib.check(_lib.lib().drt_render_forward(
                    scene.optix_mesh._h, v.data_ptr(), o.data_ptr(), d.data_ptr(), n, ior[0], ior[1],
                    out_ori.data_ptr(), out_dir.data_ptr(), mask.data_ptr(), face1.data_ptr(), face2.data_ptr(),
                    _lib.ptr(valid_idx), _lib.ptr(n_valid), *_tile_hint(n), grid[0] | (0 if DENSE_FACE_IDS else 16), _lib.ptr(grid[1]), stream_id))
                if arm is not None:
                    link.armed = bool(_lib.lib().drt_render_loss_taken(scene.optix_mesh._h))
                    _stats["loss_armed" if link.armed else "loss_arm_declined"] += 1
                    if not link.armed and not (SPLIT_LOSS and n >= SPLIT_LOSS_MIN_RAYS):
                        link.pre = None
            except BaseException:
                _lib.lib().drt_outputs_cancel(om._h)
                if graph_set is not None and binding is None:      # the capture failed: the set goes back to the pool, the caller falls back to eager calls
                    om._out_pool.entries.append(graph_set)
                if binding is not None:
                    binding.release()                    # (whatever state the failed call left its set in: the next call starts from fresh zeros)
                raise
            if graph_set is not None and binding is None:
                sets = getattr(om, "_graph_sets", None)
                if sets is None:
                    sets = om._graph_sets = []
                sets.append(graph_set)                   # alive as long as the scene (release_outputs(graph_sets=True)): the graph's replays read and write these buffers
            # (with recycling on: only for a caller who evidently KEEPS its outputs -- the pool had nothing to offer for this call and for the one
            # before it; the steady state of a loop that drops them never gets here)
            missed, om._recycle_missed = getattr(om, "_recycle_missed", 0), (0 if took is not None or not recycle else getattr(om, "_recycle_missed", 0) + 1)
            if PREFILL_NEXT and (not recycle or (took is None and missed >= 2)) and (grid[0] & 3) == 2 and n >= PREFILL_MIN_RAYS and not capturing and getattr(om, "_prefilled", None) is None:
                # outputs of the next call of this size: allocated now, zeroed on the library's idle stream behind this forward pass
                h = scene.optix_mesh._h
                nxt_ori = torch.empty((n, 3), dtype=torch.float64, device=o.device)
                nxt_mask = torch.empty((n, 3), dtype=torch.uint8, device=o.device)
                _lib.check(_lib.lib().drt_prefill_zero(h, nxt_ori.data_ptr(), nxt_ori.numel() * 8, stream_id))
                _lib.check(_lib.lib().drt_prefill_zero(h, nxt_mask.data_ptr(), nxt_mask.numel(), stream_id))
                om._prefilled = (n, o.device, nxt_ori, nxt_mask)
        if recycle:
            # the pool keeps the base tensors; the caller gets aliases of its own (same storage, same version counter), so that the
            # storages' use counts say when the caller is done with them  (a graph's set stays out of the pool: `om._graph_sets`)
            if graph_set is None:
                om._out_pool.put(n, o.device, getattr(stream_id, "value", stream_id), bases, counts, valid_idx, n_valid)
            out_ori, out_dir, mask = bases[0].detach(), bases[1].detach(), bases[2].detach()
            bases = None
        if not need_bwd:
            valid_idx = n_valid = None
        ctx.scene = scene
        ctx.ior = ior
        ctx.save_for_backward(v, o, d, face1, face2, valid_idx, n_valid)
        if link is not None:
            link.paths = (valid_idx, n_valid)        # the rays with mask = 1: ray_loss walks this list instead of all N rays
            link.render = (scene, v, o, d, face1, face2, ctx.ior) if need_bwd and not need_inputs else None     # (None: no eager stash)
        # an output the loss does not use must reach backward() as None, not as a materialised [N,3] float64 zero tensor:
        # the reference's ray_loss detaches out_ori (optim.py:100), and filling 1.8 GB of zeros per step cost 0.3 ms
        ctx.set_materialize_grads(False)
        mask_b = mask.view(torch.bool)
        ctx.mark_non_differentiable(mask_b)
        scene.last_face1, scene.last_face2 = face1, face2
        return out_ori, out_dir, mask_b

    @staticmethod
    def backward(ctx, g_ori, g_dir, g_mask):
        v, o, d, face1, face2, valid_idx, n_valid = ctx.saved_tensors
        link = ctx.link
        if ctx.binding is not None and ctx.binding.gen != ctx.binding_gen and (g_ori is not None or (g_dir is not None and not link.is_token(g_dir)) or any(e[0] is not None for e in link.pending)):
            raise RuntimeError("render_transparent(binding): the outputs of this call (and the list of its completed paths) were recycled by a later "
                               "call on the same RayBinding -- run backward() before the next render_transparent(handle), or render without a handle")
        pending, link.pending = link.pending, []
        if g_dir is not None and link.is_token(g_dir):
            g_dir = None                        # ray_loss's placeholder: its gradient is in `pending`
        # (the usual step -- one ray_loss, eager stash, nothing dense -- is ONE small launch: stash * scale)
        grad_v = None if (g_ori is None and g_dir is None and pending and all(e[0] is None for e in pending)) else det.acc(v)
        h = ctx.scene.optix_mesh._h
        # rays / IORs (ctx.need_inputs): zeros for rows without a completed path; no origin gradient when nothing reached out_ori (the
        # reference's ray_loss detaches it, and with flat faces the exit direction does not depend on the origin)
        g_in = (None, None, None)
        if ctx.need_inputs:
            nig, n = ctx.needs_input_grad, o.shape[0]
            g_in = (torch.zeros((n, 3), dtype=torch.float64, device=o.device) if nig[1] and g_ori is not None else None,
                    torch.zeros((n, 3), dtype=torch.float64, device=o.device) if nig[2] else None,
                    det.acc(torch.empty(2, dtype=torch.float64, device=o.device)) if nig[4] or nig[5] else None)
        in_ptrs = tuple(_lib.ptr(t) for t in g_in)
        with _on(o.device):
            if g_ori is not None or g_dir is not None:
                g_ori = None if g_ori is None else _f64c(g_ori, "grad_out_ori")
                g_dir = None if g_dir is None else _f64c(g_dir, "grad_out_dir")
                args = (h, v.data_ptr(), o.data_ptr(), d.data_ptr(), o.shape[0], ctx.ior[0], ctx.ior[1],
                        face1.data_ptr(), face2.data_ptr(), _lib.ptr(valid_idx), _lib.ptr(n_valid),
                        _lib.ptr(g_ori), _lib.ptr(g_dir), grad_v.data_ptr())
                if ctx.need_inputs:
                    _lib.check(_lib.lib().drt_render_backward_inputs(*args, *in_ptrs, _stream()))
                else:
                    _lib.check(_lib.lib().drt_render_backward(*args, _stream()))
            for rows, n_rows, sp, scale in pending:
                if rows is None:                # eager entry: n_rows is the unit-seed vertex gradient ray_loss's forward left
                    continue
                args = (h, v.data_ptr(), o.data_ptr(), d.data_ptr(), o.shape[0], ctx.ior[0], ctx.ior[1], face1.data_ptr(), face2.data_ptr(),
                        rows.data_ptr(), n_rows.data_ptr(), sp.data_ptr(), scale.data_ptr(), grad_v.data_ptr())
                if ctx.need_inputs:
                    _lib.check(_lib.lib().drt_render_backward_ray_loss_inputs(*args, *in_ptrs, _stream()))
                else:
                    _lib.check(_lib.lib().drt_render_backward_ray_loss(*args, _stream()))
        if grad_v is not None:
            grad_v = det.value(grad_v, v)          # (deterministic mode: the exact integer sums, rounded once)
        g_ior = [None, None]
        if g_in[2] is not None:
            both = det.value(g_in[2], torch.empty(2, dtype=torch.float64))       # [d / d ior_int, d / d ior_ext] on the rays' device
            for k in (0, 1):
                if ctx.needs_input_grad[4 + k]:
                    shape, dtype, dev = ctx.ior_like[k]
                    g_ior[k] = both[k].reshape(shape).to(dtype=dtype, device=dev)
        for rows, stash, wide, scale in pending:
            if rows is None:
                if det.SINK is not None and wide is not None:
                    det.SINK.append((wide, scale))        # full_batch_step sums the cells of all calls and ranks exactly, then converts once
                    continue
                grad_v = torch.addcmul(grad_v, stash, scale) if grad_v is not None else stash * scale
        return grad_v, g_in[0], g_in[1], None, g_ior[0], g_ior[1], None, None, None


def _law_flags(tir, refraction):
    """law_flags of the drt_render_paths_law_* entry points (DRT_LAW_REFLECT = 1, DRT_LAW_SNELL = 2)."""
    return int(tir == "reflect") | (2 if refraction == "snell" else 0)


def _paths_entry(name, law_flags):
    """The entry point of a K-interaction call: without the Snell bit the one that takes ``reflect`` -- today's call -- else its
    ``_law`` namesake, which takes the flags in the same place."""
    return getattr(_lib.lib(), name.replace("drt_render_paths_", "drt_render_paths_law_") if law_flags & 2 else name)


class _RenderPaths(torch.autograd.Function):
    """render_paths (paths of up to K interactions, drt_render_paths_forward / drt_render_paths_law_forward) as a function of the
    vertices.  ``law_flags`` (``_law_flags``) goes to the backward with the tape."""

    @staticmethod
    def forward(ctx, vertices, origin, ray_dir, scene, ior, max_bounces, law_flags):
        v = _f64c(vertices.detach(), "vertices")
        o = _f64c(origin.detach(), "origin")
        d = _f64c(ray_dir.detach(), "ray_dir")
        n = o.shape[0]
        dev = o.device
        # (the call writes every row of every output: dead values on the rows without a completed path, -1 through the whole tape first)
        out_ori = torch.empty((n, 3), dtype=torch.float64, device=dev)
        out_dir = torch.empty((n, 3), dtype=torch.float64, device=dev)
        mask = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        tape = torch.empty((max_bounces, n), dtype=torch.int32, device=dev)
        hits = torch.empty(n, dtype=torch.uint8, device=dev)
        valid_idx = torch.empty(n, dtype=torch.int32, device=dev)
        n_valid = torch.zeros(1, dtype=torch.int64, device=dev)
        if n:
            with _on(dev):
                _lib.check(_paths_entry("drt_render_paths_forward", law_flags)(
                    scene.optix_mesh._h, v.data_ptr(), o.data_ptr(), d.data_ptr(), n, ior[0], ior[1], max_bounces, law_flags,
                    out_ori.data_ptr(), out_dir.data_ptr(), mask.data_ptr(), tape.data_ptr(), hits.data_ptr(),
                    valid_idx.data_ptr(), n_valid.data_ptr(), _stream()))
        ctx.scene, ctx.ior, ctx.law = scene, ior, (max_bounces, law_flags)
        ctx.save_for_backward(v, o, d, tape, hits, valid_idx, n_valid)
        ctx.set_materialize_grads(False)
        mask_b = mask.view(torch.bool)
        ctx.mark_non_differentiable(mask_b)
        scene.last_path_hits, scene.last_path_faces = hits, tape
        return out_ori, out_dir, mask_b

    @staticmethod
    def backward(ctx, g_ori, g_dir, g_mask):
        v, o, d, tape, hits, valid_idx, n_valid = ctx.saved_tensors
        if o.shape[0] == 0 or (g_ori is None and g_dir is None):
            return torch.zeros_like(v), None, None, None, None, None, None
        grad_v = det.acc(v)
        g_ori = None if g_ori is None else _f64c(g_ori, "grad_out_ori")
        g_dir = None if g_dir is None else _f64c(g_dir, "grad_out_dir")
        with _on(o.device):
            _lib.check(_paths_entry("drt_render_paths_backward", ctx.law[1])(
                ctx.scene.optix_mesh._h, v.data_ptr(), o.data_ptr(), d.data_ptr(), o.shape[0], ctx.ior[0], ctx.ior[1], *ctx.law,
                tape.data_ptr(), hits.data_ptr(), valid_idx.data_ptr(), n_valid.data_ptr(), _lib.ptr(g_ori), _lib.ptr(g_dir),
                grad_v.data_ptr(), _stream()))
        return det.value(grad_v, v), None, None, None, None, None, None


class _RayLoss(torch.autograd.Function):
    """Loss_calculator.ray_loss (reference optim.py:100-106) in one pass over the rays."""

    @staticmethod
    def forward(ctx, out_ori, out_dir, mask, screen_pixel, valid, link):
        oo = _f64c(out_ori.detach(), "out_ori")
        od = _f64c(out_dir.detach(), "out_dir")
        sp = _f64c(screen_pixel, "screen_pixel")
        n = oo.shape[0]
        m = _flag_bytes(mask, "mask", 3 * n)
        va = _flag_bytes(valid, "valid", n)
        loss = det.scalar(oo.device)
        need = ctx.needs_input_grad[1]
        ctx.link = link if need else None
        g = torch.empty_like(od) if need and link is None else None      # dense d loss / d out_dir only without a link
        ctx.stash = ctx.stash_wide = None
        own = (link is not None and link.paths is not None and link.paths[0] is not None and link.mask is not None
               and link.mask() is mask and mask._version == 0)           # the forward's own mask, untouched: its list of set rows is exact
        eager = (own and need and EAGER_LOSS_GRAD and link.render is not None and link.out_ori is not None and link.out_ori() is out_ori
                 and out_ori._version == 0 and out_dir._version == 0)
        rows = torch.empty(n, dtype=torch.int32, device=oo.device) if need and not eager else None     # (the eager form needs no row list)
        n_rows = torch.zeros(1, dtype=torch.int32, device=oo.device) if need and not eager else None
        with _on(oo.device):
            if eager:
                # loss + unit-seed vertex gradient in one pass over the completed paths (see EAGER_LOSS_GRAD)
                scene, v, o, d, face1, face2, ior = link.render
                pre, link.pre = link.pre, None
                bound = link.targets is not None and link.targets[0] is screen_pixel and link.targets[1] is valid
                early = pre is not None and (bound or _targets_seen_before(screen_pixel, valid, link.seq)) and sp.data_ptr() == screen_pixel.data_ptr() and va.data_ptr() == valid.data_ptr()
                armed, link.armed = link.armed, False
                if armed:      # `pre` already holds the loss and the stash of the bound targets (ARMED_LOSS): this is them, or they are of no use here
                    early = False
                    armed = pre is not None and bound
                    _stats["loss_arm_used" if armed else "loss_arm_dropped"] += 1
                if armed or early:      # accumulators zeroed before the render call: the head of the list can be processed beside the pipelines (SPLIT_LOSS)
                    ctx.stash, loss = pre
                else:
                    ctx.stash = det.acc(v)
                if not armed:
                    fn = _lib.lib().drt_ray_loss_listed_grad_split if early else _lib.lib().drt_ray_loss_listed_grad
                    _lib.check(fn(
                        scene.optix_mesh._h, v.data_ptr(), o.data_ptr(), d.data_ptr(), n, ior[0], ior[1], face1.data_ptr(), face2.data_ptr(),
                        sp.data_ptr(), va.data_ptr(), link.paths[0].data_ptr(), link.paths[1].data_ptr(), loss.data_ptr(), ctx.stash.data_ptr(), _stream()))
                ctx.stash_wide = ctx.stash if ctx.stash.dtype == torch.int64 else None      # (deterministic mode: the cells themselves, for det.SINK)
                ctx.stash = det.value(ctx.stash, v)
            elif own:
                _lib.check(_lib.lib().drt_ray_loss_listed(oo.data_ptr(), od.data_ptr(), sp.data_ptr(), va.data_ptr(), link.paths[0].data_ptr(),
                                                          link.paths[1].data_ptr(), n, loss.data_ptr(), _lib.ptr(rows), _lib.ptr(n_rows), _stream()))
            else:
                _lib.check(_lib.lib().drt_ray_loss(oo.data_ptr(), od.data_ptr(), m.data_ptr(), sp.data_ptr(), va.data_ptr(), n,
                                                   loss.data_ptr(), _lib.ptr(g), _lib.ptr(rows), _lib.ptr(n_rows), _stream()))
        loss = det.value(loss)
        ctx.save_for_backward(g, rows, n_rows, sp if (need and link is not None) else None)
        ctx.applied = None                       # scale already multiplied into the saved rows (see backward)
        ctx.n_rays = n
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        g, rows, n_rows, sp = ctx.saved_tensors
        if ctx.link is not None:                 # row-list hand-off to render_transparent's backward (see _GradLink)
            if ctx.n_rays == 0:
                return None, None, None, None, None, None
            scale = g_loss.detach().to(torch.float64).reshape(1).contiguous()
            if ctx.stash is not None:
                ctx.link.pending.append((None, ctx.stash, ctx.stash_wide, scale))
                return None, ctx.link.token(ctx.n_rays, ctx.stash.device), None, None, None, None
            ctx.link.pending.append((rows, n_rows, sp, scale))
            return None, ctx.link.token(ctx.n_rays, rows.device), None, None, None, None
        if g is None:
            return None, None, None, None, None, None
        if g.numel() == 0:                       # no rays: an empty tensor has no storage to pass down
            return None, g, None, None, None, None
        # scale only the contributing rows (a few % of the rays) instead of streaming the dense tensor again;
        # out_ori is detached in the reference's loss (optim.py:100): no gradient for it
        sc = g_loss.detach().to(torch.float64).reshape(1).contiguous()
        new = sc.clone()
        if ctx.applied is not None:
            # a second backward over the same graph (retain_graph=True): the saved rows already carry the previous
            # incoming gradient, so rescale by the ratio.  Rare path: one host sync to refuse an unrecoverable 0.
            if float(ctx.applied.item()) == 0.0:
                raise RuntimeError("ray_loss: backward was already run with a zero incoming gradient; the saved rows "
                                   "cannot be rescaled -- recompute the loss instead of re-using the graph")
            sc = sc / ctx.applied
        ctx.applied = new
        with _on(g.device):
            _lib.check(_lib.lib().drt_scale_rows3(g.data_ptr(), rows.data_ptr(), n_rows.data_ptr(), sc.data_ptr(), _stream()))
        return None, g, None, None, None, None


def enqueue_ray_term(scene, vertices, origin, ray_dir, target, valid, law, loss_ptr, grad_ptr, count_ptr=None, ior=None, grid=None):
    """Enqueues ONE view's refraction term -- loss and d loss / d vertices (unit seed), nothing dense written -- on the current stream;
    the one place that packs the arguments of drt_render_ray_loss_fused and drt_render_paths_ray_loss_fused.  ``law=None``: the two-bounce
    kernel with the grid verdict of the ray tensors (``grid``: a verdict the caller already has, a RayBinding's), seed arming and tile
    hint; a normalised law tuple (K, tir[, refraction]): the K-interaction kernel under ``_law_flags``.  ``loss_ptr`` / ``grad_ptr`` /
    ``count_ptr`` are raw device addresses the kernels ADD into (float64, or fixed-point cells in deterministic mode; int64 count, may
    be None); ``ior``: (interior, exterior) floats, the module's IORs without it.  The caller is inside ``_on(device)``.  Returns the
    tensors whose memory the enqueued kernels read: the caller keeps them alive until the work is done."""
    o, d, sp = _f64c(origin, "origin"), _f64c(ray_dir, "ray_dir"), _f64c(target, "screen_pixel")
    n = o.shape[0]
    va = _flag_bytes(valid, "valid", n)
    h = scene.optix_mesh._h
    if ior is None:
        ior = _ior_host(intIOR, "intIOR"), _ior_host(extIOR, "extIOR")
    if law is not None:
        flags = _law_flags(law[1], law[2] if len(law) > 2 else "reference")
        _lib.check(_paths_entry("drt_render_paths_ray_loss_fused", flags)(
            h, vertices.data_ptr(), o.data_ptr(), d.data_ptr(), sp.data_ptr(), va.data_ptr(), n, ior[0], ior[1], law[0], flags,
            loss_ptr, grad_ptr, count_ptr, _stream()))
        return [o, d, sp, va]
    if grid is None:
        grid = _grid_cache(origin, ray_dir, n, *_tile_hint(n)) if origin.is_contiguous() and ray_dir.is_contiguous() else (0, None)
    _arm_seed(h, grid, n)
    _lib.check(_lib.lib().drt_render_ray_loss_fused(
        h, vertices.data_ptr(), o.data_ptr(), d.data_ptr(), sp.data_ptr(), va.data_ptr(), n, ior[0], ior[1],
        loss_ptr, grad_ptr, count_ptr, *_tile_hint(n), grid[0], _lib.ptr(grid[1]), _stream()))
    return [o, d, sp, va]


_IMAGE_ENTRIES = {"plain": ("drt_render_image_loss", 0), "screen": ("drt_render_image_loss_screen", 2), "camera": ("drt_render_image_loss_camera", 3)}


def enqueue_image_term(scene, vertices, a, ior, texture, target, weight, loss_ptr, grad_ptr=None, grad_ior_ptr=None, image_ptr=None, count_ptr=None,
                       screen_ptr=None, texture_ptr=None, camera_ptr=None, entry=None):
    """Enqueues ONE view's photometric image term -- loss and its unit-seed gradients, band after band of ``a["bands"]`` into one set of
    accumulators -- on the current stream; the one place that packs the arguments of drt_render_image_loss, drt_render_image_loss_screen
    and drt_render_image_loss_camera.  ``a``: the checked arguments (``render.check_image_loss_args``); ``ior``: (interior, exterior)
    floats; ``texture`` / ``target`` / ``weight``: contiguous float32 device tensors (weight may be None).  ``loss_ptr`` and the other
    ``*_ptr`` are raw device addresses the kernels ADD into (float64, or fixed-point cells in deterministic mode; float32 image, int64
    count); all but the first may be None.  The call goes to the narrowest entry point that has a parameter for every accumulator given
    -- plain, then screen (screen 9, texture), then camera (21) --; ``entry`` ("plain" / "screen" / "camera") names a wider one, whose
    extra parameters are then null.  The caller is inside ``_on(device)``.  Returns what the enqueued kernels read, for the caller to
    keep alive."""
    extra = (screen_ptr, texture_ptr, camera_ptr)
    needed = 3 if camera_ptr is not None else 2 if screen_ptr is not None or texture_ptr is not None else 0
    name, n_extra = _IMAGE_ENTRIES[entry] if entry is not None else next(e for e in _IMAGE_ENTRIES.values() if e[1] >= needed)
    if n_extra < needed:
        raise ValueError(f"entry {entry!r} has no parameter for an accumulator that was given")
    fn, H, W, C = getattr(_lib.lib(), name), a["height"], a["width"], a["channels"]
    for y0, y1 in a["bands"]:
        _lib.check(fn(
            scene.optix_mesh._h, vertices.data_ptr(), a["camera"].ctypes.data, H, W, y0, y1, a["supersample"], ior[0], ior[1], a["max_bounces"],
            a["law_flags"], a["fresnel"], a["screen"].ctypes.data, texture.data_ptr(), texture.shape[0], texture.shape[1], C, a["void"].ctypes.data,
            a["invalid"].ctypes.data, target.data_ptr(), _lib.ptr(weight), loss_ptr, grad_ptr, grad_ior_ptr, image_ptr, count_ptr, *extra[:n_extra], _stream()))
    return [vertices, texture, target, weight]


def enqueue_image_absorb_term(scene, vertices, a, ior, texture, target, weight, loss_ptr, grad_ptr=None, grad_ior_ptr=None, image_ptr=None, count_ptr=None,
                              sigma_ptr=None):
    """``enqueue_image_term`` for absorbing glass: ONE view's photometric image term under ``a["absorption"]`` (C float64
    coefficients on the host, checked by ``render.check_absorption``), band after band into one set of accumulators, on the current
    stream; the one place that packs the arguments of drt_render_image_loss_absorb.  ``sigma_ptr``: C more accumulators, for
    d loss / d sigma, addressed like ``grad_ior_ptr``; like every ``*_ptr`` but the first it may be None.  The caller is inside
    ``_on(device)``.  Returns what the enqueued kernels read, for the caller to keep alive."""
    fn, H, W, C = _lib.lib().drt_render_image_loss_absorb, a["height"], a["width"], a["channels"]
    for y0, y1 in a["bands"]:
        _lib.check(fn(
            scene.optix_mesh._h, vertices.data_ptr(), a["camera"].ctypes.data, H, W, y0, y1, a["supersample"], ior[0], ior[1], a["max_bounces"],
            a["law_flags"], a["fresnel"], a["screen"].ctypes.data, texture.data_ptr(), texture.shape[0], texture.shape[1], C, a["void"].ctypes.data,
            a["invalid"].ctypes.data, target.data_ptr(), _lib.ptr(weight), loss_ptr, grad_ptr, grad_ior_ptr, image_ptr, count_ptr,
            a["absorption"].ctypes.data, sigma_ptr, _stream()))
    return [vertices, texture, target, weight]


def enqueue_image_env_term(scene, vertices, a, ior, texture, env, target, weight, loss_ptr, grad_ptr=None, grad_ior_ptr=None, image_ptr=None, count_ptr=None,
                           env_ptr=None, env_rot_ptr=None, param=False):
    """``enqueue_image_term`` in front of an environment: ONE view's photometric image term under ``a["environment"]`` and
    ``a["reflection"]``, band after band into one set of accumulators, on the current stream; the one place that packs the arguments of
    drt_render_image_loss_env and drt_render_image_loss_env_param.  ``texture``: a contiguous float32 device tensor, or None with
    ``a["screen"]`` None (no screen); ``env``: the environment's texels as a contiguous float32 device tensor.  ``env_ptr`` /
    ``env_rot_ptr``: the accumulators of the environment's texels (padded to a multiple of three values) and of its nine
    rotation entries; given, or with ``param``, the call goes to drt_render_image_loss_env_param, else to drt_render_image_loss_env with
    the arguments of before.  Every ``*_ptr`` but the first may be None.  The caller is inside ``_on(device)``.  Returns what the enqueued
    kernels read, for the caller to keep alive."""
    H, W, C = a["height"], a["width"], a["channels"]
    if param or env_ptr is not None or env_rot_ptr is not None:
        fn, extra = _lib.lib().drt_render_image_loss_env_param, (env_ptr, env_rot_ptr)
    else:
        fn, extra = _lib.lib().drt_render_image_loss_env, ()
    rot = a["environment"].packed()
    for y0, y1 in a["bands"]:
        _lib.check(fn(
            scene.optix_mesh._h, vertices.data_ptr(), a["camera"].ctypes.data, H, W, y0, y1, a["supersample"], ior[0], ior[1], a["max_bounces"],
            a["law_flags"], a["fresnel"], None if texture is None else a["screen"].ctypes.data, _lib.ptr(texture), 0 if texture is None else texture.shape[0],
            0 if texture is None else texture.shape[1], C, a["void"].ctypes.data, a["invalid"].ctypes.data, target.data_ptr(), _lib.ptr(weight), loss_ptr,
            grad_ptr, grad_ior_ptr, image_ptr, count_ptr, env.data_ptr(), env.shape[0], env.shape[1], rot.ctypes.data, int(a["reflection"]), *extra, _stream()))
    return [vertices, texture, env, target, weight]


def enqueue_image_views_term(scene, vertices, binding, view_ids, texture, law, supersample, fresnel, void, invalid, ior, loss_ptr, grad_ptr,
                             grad_ior_ptr=None, count_ptr=None, bands=None, reflection=False, absorption=None, grad_sigma_ptr=None, images_ptr=None):
    """Enqueues the photometric image term of the listed views of ``binding`` (a ``render.ImageViews``) -- the SUM over ``view_ids`` of one
    view's loss and d loss / d vertices (unit seed), as one forward wavefront and one adjoint pass per band -- on the current stream; the
    one place that packs the arguments of drt_render_image_loss_views and drt_render_image_loss_views_env.  The entry point follows the
    binding: one made with an environment goes to drt_render_image_loss_views_env with its resident texels, its
    rotation and ``reflection``; one without packs exactly the arguments of before.  ``law``: a normalised law tuple (K, tir[,
    refraction]); ``texture``: a contiguous float32 device tensor [Th, Tw, C], or None with a binding without screens; ``void`` /
    ``invalid``: float64 numpy arrays of C values; ``ior``: (interior, exterior) floats; ``bands``: rows [r0, r1) of the tall image of
    ``len(view_ids) * H`` rows (``render.plan_bands``), the whole of it without.  ``loss_ptr`` / ``grad_ptr`` / ``grad_ior_ptr`` /
    ``count_ptr`` are raw device addresses the kernels ADD into (float64, or fixed-point cells in deterministic mode; int64 count); all
    but the first may be None.  ``absorption``: C float64 coefficients on the host (``render.check_absorption``), or
    None; with them the call goes to drt_render_image_loss_views_absorb whether or not the binding has an environment, with
    ``grad_sigma_ptr`` (C more accumulators for d loss / d sigma, addressed like ``grad_ior_ptr``) and ``images_ptr`` (a float32 stack
    [n_views, H, W, C] that receives the rendered pixels of the listed views), both nullable; with None the entry point and the packed
    arguments are exactly those of before.  Nothing is checked here but what the library checks.  The caller is inside
    ``_on(device)``.  Returns what the enqueued kernels read, for the caller to keep alive."""
    ids = (ctypes.c_int * len(view_ids))(*view_ids)
    flags = _law_flags(law[1], law[2] if len(law) > 2 else "reference")
    env = getattr(binding, "env", None)
    if absorption is not None:
        fn = _lib.lib().drt_render_image_loss_views_absorb
        more = (absorption.ctypes.data, grad_sigma_ptr) + ((None, 0, 0, None, 0) if env is None else
                                                          (env.data_ptr(), env.shape[0], env.shape[1], binding.env_rot.ctypes.data, int(reflection))) + (images_ptr,)
        tex_args = (None, 0, 0, env.shape[2]) if texture is None else (texture.data_ptr(), texture.shape[0], texture.shape[1], texture.shape[2])
    elif env is None:
        fn, more = _lib.lib().drt_render_image_loss_views, ()
        tex_args = (texture.data_ptr(), texture.shape[0], texture.shape[1], texture.shape[2])
    else:
        fn, more = _lib.lib().drt_render_image_loss_views_env, (env.data_ptr(), env.shape[0], env.shape[1], binding.env_rot.ctypes.data, int(reflection))
        tex_args = (None, 0, 0, env.shape[2]) if texture is None else (texture.data_ptr(), texture.shape[0], texture.shape[1], texture.shape[2])
    for r0, r1 in (bands if bands is not None else [(0, len(view_ids) * binding.height)]):
        _lib.check(fn(
            scene.optix_mesh._h, vertices.data_ptr(), binding._h, ids, len(view_ids), r0, r1, supersample, ior[0], ior[1], law[0], flags, int(fresnel),
            *tex_args, void.ctypes.data, invalid.ctypes.data, binding.targets.data_ptr(),
            _lib.ptr(binding.weights), loss_ptr, grad_ptr, grad_ior_ptr, count_ptr, *more, _stream()))
    return [vertices, texture, binding]


# What a ``Scene`` method states about one loss term for ``_UnitSeedTerm.apply(term, *inputs)``:
#   device   where the loss accumulator lives;
#   accs     {name: (like, users)}: the accumulators the call may want, each for a float64 tensor shaped ``like``; ``users`` None: always
#            allocated, else the positions in ``inputs`` of which one must need a gradient.  An accumulator that is not allocated reaches
#            the library as a null pointer, which selects another kernel instantiation: these rules are each route's own;
#   enqueue  callable(loss, cells) that enqueues the native work into the raw pointers of ``loss`` and ``cells`` = {name: the zeroed
#            accumulators that were allocated}; tensor conversions, ``_on`` and ``_stream`` are its business;
#   feeds    per input, (name, pick): the accumulator that holds its gradient and, where the gradient is not the whole of it, ``pick(scaled
#            values, the input's shape)``;
#   count, image   what the call publishes afterwards: tensors the enqueued work writes, or None.
_Term = collections.namedtuple("_Term", "device accs enqueue feeds count image", defaults=(None, None))
_VERTS = "vertices"                 # the accumulator whose wide cells the deterministic sink takes
_IOR_FEEDS = (("ior", lambda s, shape: s[0]), ("ior", lambda s, shape: s[1]))


def _verts_ior_accs(v, want_verts, ior_users=None):
    """The vertex accumulator (like ``v``) unless ``want_verts`` is off, and the IOR pair on its device."""
    accs = {_VERTS: (v, None)} if want_verts else {}
    accs["ior"] = (torch.empty(2, dtype=torch.float64, device=v.device), ior_users)
    return accs


def _rinv_rows(s, shape):
    """d / d R^-1 of the 21 camera partials [K^-1's nine, R^-1's top three rows]: a [4, 4] R^-1 gets a zero bottom row (the renderer does not read it)."""
    rows = s[9:].reshape(3, 4)
    return torch.cat([rows, rows.new_zeros((1, 4))]) if tuple(shape) == (4, 4) else rows


class _UnitSeedTerm(torch.autograd.Function):
    """Every one-pass loss term of ``Scene`` (ray_loss_fused, paths_ray_loss[_ior]_fused, image_loss[_views]_fused; DESIGN.md 7.4,
    10.3-10.6) as a function of ``inputs`` -- the tensors autograd may track for it, or None: vertices, IORs, screen, texture, R^-1,
    K^-1, whichever the ``term`` (a ``_Term``) has.  The forward allocates the accumulators the term asks for and has it enqueue the
    native work, which computes every gradient with a unit seed; the backward only scales them by the incoming gradient and hands each
    back in its input's own shape, dtype and device.  While ``det.SINK`` is armed the vertex gradient's wide cells go there instead."""

    @staticmethod
    def forward(ctx, term, *inputs):
        nig = ctx.needs_input_grad[1:]
        loss = det.scalar(term.device)
        cells = {name: det.acc(like) for name, (like, users) in term.accs.items() if users is None or any(nig[k] for k in users)}
        term.enqueue(loss, cells)
        wide = cells.get(_VERTS)
        ctx.wide = wide if wide is not None and wide.dtype == torch.int64 else None      # (deterministic mode: the cells themselves, for det.SINK)
        ctx.names, ctx.feeds = tuple(cells), term.feeds
        ctx.like = tuple((x.shape, x.dtype, x.device) if isinstance(x, torch.Tensor) else None for x in inputs)
        ctx.save_for_backward(*(det.value(c, term.accs[name][0]) for name, c in cells.items()))
        return det.value(loss)

    @staticmethod
    def backward(ctx, g_loss):
        stored, scaled, grads = dict(zip(ctx.names, ctx.saved_tensors)), {}, [None]
        for k, feed in enumerate(ctx.feeds):
            grads.append(None)
            if feed is None or feed[0] not in stored or not ctx.needs_input_grad[1 + k]:
                continue
            name, pick = feed
            if name == _VERTS and det.SINK is not None and ctx.wide is not None:
                det.SINK.append((ctx.wide, g_loss))          # full_batch_step sums the cells of all calls and ranks exactly, then converts once
                continue
            if name not in scaled:
                scaled[name] = stored[name] * g_loss
            shape, dtype, dev = ctx.like[k]
            g = scaled[name] if pick is None else pick(scaled[name], shape)
            grads[-1] = g.reshape(shape).to(dtype=dtype, device=dev)
        return tuple(grads)


def _ray_term(scene, origin, ray_dir, screen_pixel, valid, ior, law, grid):
    """The term of ray_loss_fused (``law`` None: the two-bounce kernel with ``grid``) and paths_ray_loss_fused (a normalised law tuple):
    ``enqueue_ray_term`` into a vertex accumulator that is always there; the count of contributing rays only under a law."""
    v = _f64c(scene.vertices.detach(), "vertices")
    count = torch.zeros((), dtype=torch.int64, device=v.device) if law is not None else None

    def enqueue(loss, cells):
        with _on(v.device):
            enqueue_ray_term(scene, v, origin, ray_dir, screen_pixel, valid, law, loss.data_ptr(), cells[_VERTS].data_ptr(), _lib.ptr(count), ior, grid)
    return _Term(v.device, {_VERTS: (v, None)}, enqueue, ((_VERTS, None),), count)


def _paths_ior_term(scene, origin, ray_dir, screen_pixel, valid, ior, max_bounces, law_flags, want_verts):
    """The term of paths_ray_loss_ior_fused (drt_render_paths_law_ray_loss_ior_fused) for the inputs (vertices, ior_int,
    ior_ext): the IOR pair always, the vertex accumulator unless ``want_verts`` is off -- no array is handed over and the library runs
    its kernel without the gradient table."""
    v = _f64c(scene.vertices.detach(), "vertices")
    count = torch.zeros((), dtype=torch.int64, device=v.device)

    def enqueue(loss, cells):
        o, d, sp = _f64c(origin, "origin"), _f64c(ray_dir, "ray_dir"), _f64c(screen_pixel, "screen_pixel")
        va = _flag_bytes(valid, "valid", o.shape[0])
        with _on(v.device):
            _lib.check(_lib.lib().drt_render_paths_law_ray_loss_ior_fused(
                scene.optix_mesh._h, v.data_ptr(), o.data_ptr(), d.data_ptr(), sp.data_ptr(), va.data_ptr(), o.shape[0], ior[0], ior[1], max_bounces,
                law_flags, loss.data_ptr(), _lib.ptr(cells.get(_VERTS)), cells["ior"].data_ptr(), count.data_ptr(), _stream()))
    return _Term(v.device, _verts_ior_accs(v, want_verts), enqueue, ((_VERTS, None),) + _IOR_FEEDS, count)


def _image_term(scene, a, ior, tex, target, weight, entry="plain"):
    """The term of image_loss_fused on the checked arguments ``a`` for the inputs (vertices, ior_int, ior_ext), then (screen_param,
    texture_param) from ``entry`` "screen" on, then (Rinv, Kinv) at "camera"; ``entry`` is also the native entry point the call reaches
    (``enqueue_image_term``).  The vertex accumulator follows ``a["vertices"]``; the IOR pair is always there at "plain" and "screen",
    at "camera" only when an IOR needs a gradient; screen 9, texture (scattered in threes: padded to a multiple of three, sliced back)
    and camera 21 only when such an input needs one."""
    v = _f64c(scene.vertices.detach(), "vertices")
    dev, n_tex = v.device, tex.numel()
    like = lambda n: torch.empty(n, dtype=torch.float64, device=dev)      # noqa: E731
    accs = _verts_ior_accs(v, a["vertices"], (1, 2) if entry == "camera" else None)
    feeds = ((_VERTS, None),) + _IOR_FEEDS
    if entry != "plain":
        accs["screen"], accs["texture"] = (like(9), (3,)), (like((n_tex + 2) // 3 * 3), (4,))
        feeds += (("screen", None), ("texture", lambda s, shape: s[:n_tex]))
    if entry == "camera":
        accs["camera"] = (like(21), (5, 6))
        feeds += (("camera", _rinv_rows), ("camera", lambda s, shape: s[:9]))
    count = torch.zeros((), dtype=torch.int64, device=dev)
    image = torch.empty((a["height"], a["width"], a["channels"]), dtype=torch.float32, device=dev) if a["want_image"] else None

    def enqueue(loss, cells):
        with _on(dev):
            enqueue_image_term(scene, v, a, ior, tex, target, weight, loss.data_ptr(), _lib.ptr(cells.get(_VERTS)), _lib.ptr(cells.get("ior")), _lib.ptr(image),
                               count.data_ptr(), *(_lib.ptr(cells.get(k)) for k in ("screen", "texture", "camera")), entry=entry)
    return _Term(dev, accs, enqueue, feeds, count, image)


def _image_env_term(scene, a, ior, tex, env, target, weight, param=False):
    """The term of image_loss_fused in front of an environment (``enqueue_image_env_term``) for the inputs (vertices,
    ior_int, ior_ext): the vertex accumulator follows ``a["vertices"]``, the IOR pair is always there.  ``param``: the
    inputs go on with (env_texels_param, env_rotation_param), and the call reaches drt_render_image_loss_env_param; the environment's
    texel accumulator (scattered in threes: padded to a multiple of three, sliced back) and the nine of its rotation are there only when
    such an input needs a gradient."""
    v = _f64c(scene.vertices.detach(), "vertices")
    dev, n_env = v.device, env.numel()
    accs, feeds = _verts_ior_accs(v, a["vertices"]), ((_VERTS, None),) + _IOR_FEEDS
    if param:
        like = lambda n: torch.empty(n, dtype=torch.float64, device=dev)      # noqa: E731
        accs["env"], accs["env_rot"] = (like((n_env + 2) // 3 * 3), (3,)), (like(9), (4,))
        feeds += (("env", lambda s, shape: s[:n_env]), ("env_rot", None))
    count = torch.zeros((), dtype=torch.int64, device=dev)
    image = torch.empty((a["height"], a["width"], a["channels"]), dtype=torch.float32, device=dev) if a["want_image"] else None

    def enqueue(loss, cells):
        with _on(dev):
            enqueue_image_env_term(scene, v, a, ior, tex, env, target, weight, loss.data_ptr(), _lib.ptr(cells.get(_VERTS)), _lib.ptr(cells.get("ior")),
                                   _lib.ptr(image), count.data_ptr(), _lib.ptr(cells.get("env")), _lib.ptr(cells.get("env_rot")), param)
    return _Term(dev, accs, enqueue, feeds, count, image)


def _image_absorb_term(scene, a, ior, tex, target, weight):
    """The term of image_loss_fused under an absorption (``enqueue_image_absorb_term``) for the inputs (vertices,
    ior_int, ior_ext, absorption): the vertex accumulator follows ``a["vertices"]``, the IOR pair is always there, the C sigma
    accumulators only when the absorption is a tensor that needs a gradient."""
    v = _f64c(scene.vertices.detach(), "vertices")
    dev = v.device
    accs = _verts_ior_accs(v, a["vertices"])
    accs["sigma"] = (torch.empty(a["channels"], dtype=torch.float64, device=dev), (3,))
    count = torch.zeros((), dtype=torch.int64, device=dev)
    image = torch.empty((a["height"], a["width"], a["channels"]), dtype=torch.float32, device=dev) if a["want_image"] else None

    def enqueue(loss, cells):
        with _on(dev):
            enqueue_image_absorb_term(scene, v, a, ior, tex, target, weight, loss.data_ptr(), _lib.ptr(cells.get(_VERTS)), _lib.ptr(cells.get("ior")),
                                      _lib.ptr(image), count.data_ptr(), _lib.ptr(cells.get("sigma")))
    return _Term(dev, accs, enqueue, ((_VERTS, None),) + _IOR_FEEDS + (("sigma", None),), count, image)


def _image_views_term(scene, binding, a, ior, tex, law):
    """The term of image_loss_views_fused (``enqueue_image_views_term``) for the inputs (vertices, ior_int, ior_ext):
    the vertex accumulator follows ``a["vertices"]``, the IOR pair and the count are always there."""
    v = _f64c(scene.vertices.detach(), "vertices")
    count = torch.zeros((), dtype=torch.int64, device=v.device)

    def enqueue(loss, cells):
        with _on(v.device):
            enqueue_image_views_term(scene, v, binding, a["ids"], tex, law, a["supersample"], a["fresnel"], a["void"], a["invalid"], ior, loss.data_ptr(),
                                     _lib.ptr(cells.get(_VERTS)), cells["ior"].data_ptr(), count.data_ptr(), a["bands"], a.get("reflection", False))
    return _Term(v.device, _verts_ior_accs(v, a["vertices"]), enqueue, ((_VERTS, None),) + _IOR_FEEDS, count)


def _image_views_absorb_term(scene, binding, a, ior, tex, law):
    """The term of image_loss_views_fused under an absorption (``enqueue_image_views_term``) for the inputs (vertices,
    ior_int, ior_ext, absorption): as ``_image_views_term``, with the C sigma accumulators only when the absorption is a tensor that
    needs a gradient, and -- with ``a["want_images"]`` -- ``image``: a stack [n_views, H, W, C] of the capture's
    layout in which the listed views' pixels are written (the others stay zero)."""
    v = _f64c(scene.vertices.detach(), "vertices")
    dev = v.device
    accs = _verts_ior_accs(v, a["vertices"])
    accs["sigma"] = (torch.empty(a["channels"], dtype=torch.float64, device=dev), (3,))
    count = torch.zeros((), dtype=torch.int64, device=dev)
    # (the library writes a listed view's pixels at that view's place in a stack of the capture's layout)
    stack = torch.zeros((binding.n, binding.height, binding.width, a["channels"]), dtype=torch.float32, device=dev) if a["want_images"] else None

    def enqueue(loss, cells):
        with _on(dev):
            enqueue_image_views_term(scene, v, binding, a["ids"], tex, law, a["supersample"], a["fresnel"], a["void"], a["invalid"], ior, loss.data_ptr(),
                                     _lib.ptr(cells.get(_VERTS)), cells["ior"].data_ptr(), count.data_ptr(), a["bands"], a.get("reflection", False),
                                     a["absorption"], _lib.ptr(cells.get("sigma")), _lib.ptr(stack))
    return _Term(dev, accs, enqueue, ((_VERTS, None),) + _IOR_FEEDS + (("sigma", None),), count, stack)


def ray_loss(out_ori, out_dir, mask, screen_pixel, valid):
    """sum over valid & mask rays of |out_dir - normalize(screen_pixel - out_ori.detach())|^2."""
    link = getattr(out_dir, "_drt_link", None) if SPARSE_LOSS_GRAD else None
    if link is not None and not (out_dir.requires_grad and isinstance(out_dir.grad_fn, _RenderTransparent._backward_cls)):
        link = None
    if link is not None:
        # The row-list hand-off RECOMPUTES out_ori / out_dir of the listed rays from the forward's stored path, and lists rays by the
        # forward's own mask: it is only the gradient of THIS call when all three tensors are the forward's own, untouched ones.  A
        # different or modified out_ori / mask (extra rows set, a shifted origin) takes the dense gradient, which reads what was passed.
        own = (link.mask is not None and link.mask() is mask and mask._version == 0
               and link.out_ori is not None and link.out_ori() is out_ori and out_ori._version == 0 and out_dir._version == 0)
        if not own:
            link = None
    return _RayLoss.apply(out_ori, out_dir, mask, screen_pixel, valid, link)


def edge_tables(F, V, want_rows=False, check=True):
    """Edges [E,2], E2F [E,2,3], mean_len (reference DiffRender.py:338-355) on the device of ``F`` / ``V`` -- the reference
    goes through trimesh's host-side ``group_rows`` / ``edges_face``.  One stable radix sort of the 3F directed-edge keys
    in libdrt_hip (``drt_edge_tables``).  Order as pinned in mesh_io.group_rows_pairs: edges ascend by (min vertex, max
    vertex); the first face of a pair is the one with the lower directed-edge row.  Asserts watertightness
    (DiffRender.py:305); that check and ``mean_len`` come back in ONE small device->host copy (a topology change is not
    on the per-iteration path).  ``want_rows``: also the int32 [3F] directed-edge -> unique-edge map.  ``check=False``: no read-back at all
    (``mean_len`` is then None, watertightness is the caller's business: the device remesher's rounds, which keep the mesh closed by
    construction and install the result through ``Scene._set_topology``, which checks)."""
    if not F.is_cuda:
        raise RuntimeError("edge_tables needs GPU tensors (there is no CPU path in the product)")
    Fc = F.to(torch.long).contiguous()
    Vc = _f64c(V.detach(), "V")
    n_f, n_v = Fc.shape[0], Vc.shape[0]
    assert (3 * n_f) % 2 == 0 and n_f > 0, "mesh is not watertight: every edge must be shared by exactly two faces"
    n_e = 3 * n_f // 2
    dev = Fc.device
    Edges = torch.empty((n_e, 2), dtype=torch.long, device=dev)
    E2F = torch.empty((n_e, 2, 3), dtype=torch.long, device=dev)
    rows = torch.empty(3 * n_f, dtype=torch.int32, device=dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)           # [mean_len, status (int32 in the low bytes of word 1)]
    with _on(dev):
        ws = torch.empty(int(_lib.lib().drt_edge_tables_workspace(n_f)), dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().drt_edge_tables(Fc.data_ptr(), n_f, Vc.data_ptr(), n_v, ws.data_ptr(), Edges.data_ptr(), E2F.data_ptr(),
                                              rows.data_ptr(), out.data_ptr(), out[1:].data_ptr(), _stream()))
    if not check:
        return (Edges, E2F, None, rows) if want_rows else (Edges, E2F, None)
    host = out.cpu()
    status = int(host[1:].view(torch.int32)[0])
    if status & 2:
        raise IndexError(f"faces index vertices outside [0, {n_v}) (torch's indexing, which the reference uses here, raises as well)")
    assert status == 0, "mesh is not watertight: every edge must be shared by exactly two faces"
    mean_len = float(host[0])
    return (Edges, E2F, mean_len, rows) if want_rows else (Edges, E2F, mean_len)


class Scene(StepwiseMixin):
    def __init__(self, mesh_path, cuda_device=0):
        self.cuda_device = int(cuda_device)
        self.optix_mesh = optix_mesh(self.cuda_device)
        self._mesh_stale = False
        self._epoch = 0          # bumped by every change of vertices / mesh: what a lazy result (SampleSet) is tied to
        self.update_mesh(mesh_path)

    # ------------------------------------------------------------------ mesh state
    @property
    def _dev(self):
        return torch.device("cuda", self.cuda_device)

    def update_mesh(self, mesh_path):
        mesh = mesh_path if isinstance(mesh_path, mesh_io.TriMesh) else mesh_io.load(mesh_path, process=False)
        self._mesh = mesh
        self._mesh_stale = False
        self._epoch += 1
        self.vertices = torch.tensor(mesh.vertices, dtype=Float, device=self._dev)
        self.faces = torch.tensor(mesh.faces, dtype=torch.long, device=self._dev)
        self.init_edge()                                  # also the watertightness assert of DiffRender.py:305
        opt_v = self.vertices.detach().to(torch.float32)
        opt_F = self.faces.to(torch.int32)
        self.optix_mesh.update_mesh(opt_F, opt_v)

    def init_edge(self):
        self.Edges, self.E2F, self.mean_len, self._row2edge = edge_tables(self.faces, self.vertices.detach(), want_rows=True)

    def subdivide_midpoint(self, float32_positions=True):
        """One 1 -> 4 midpoint refinement of the current mesh entirely on the device (a level-of-detail step that is pure
        subdivision needs no host remesher): new vertices, faces, edge tables and LBVH.  Same vertex / face order as
        drt_amd.mesh_io.subdivide_midpoint."""
        V = _f64c(self.vertices.detach(), "vertices")
        F = self.faces.contiguous()
        n_v, n_f, n_e = V.shape[0], F.shape[0], self.Edges.shape[0]
        V2 = torch.empty((n_v + n_e, 3), dtype=torch.float64, device=V.device)
        F2 = torch.empty((4 * n_f, 3), dtype=torch.long, device=V.device)
        with _on(V.device):
            _lib.check(_lib.lib().drt_subdivide_midpoint(F.data_ptr(), n_f, V.data_ptr(), n_v, self.Edges.contiguous().data_ptr(), n_e,
                                                         self._row2edge.data_ptr(), int(float32_positions), F2.data_ptr(), V2.data_ptr(), _stream()))
        self._set_topology(V2, F2)

    def _set_topology(self, vertices, faces):
        """Install device-resident vertices / faces as the new mesh (host record synced lazily, see `mesh`)."""
        self._epoch += 1
        self.vertices, self.faces = vertices, faces
        self._mesh = mesh_io.TriMesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))
        self._mesh_stale = self._faces_stale = True
        self.init_edge()
        self.optix_mesh.update_mesh(self.faces.to(torch.int32), self.vertices.detach().to(torch.float32))

    @property
    def mesh(self):
        """Host-side mesh record; vertex positions are copied back lazily (the reference pays a
        device->host sync on every iteration for this, DiffRender.py:381)."""
        if getattr(self, "_faces_stale", False):
            self._mesh = mesh_io.TriMesh(self.vertices.detach().cpu().numpy(), self.faces.cpu().numpy())
            self._faces_stale = self._mesh_stale = False
        if self._mesh_stale:
            self._mesh.vertices = self.vertices.detach().cpu().numpy()
            self._mesh_stale = False
        return self._mesh

    @property
    def triangles(self):
        return self.vertices[self.faces]

    def update_verticex(self, vertices: torch.Tensor):
        if vertices.shape != self.vertices.shape:
            raise RuntimeError(f"vertices must have shape {tuple(self.vertices.shape)}")
        self._epoch += 1
        self.vertices = vertices
        self.optix_mesh.update_vert_f64(vertices)
        self._mesh_stale = True

    # ------------------------------------------------------------------ tracer access
    def optix_intersect(self, ray: Ray):
        optix_ray = torch.cat([ray.origin.detach().to(torch.float32), ray.direction.detach().to(torch.float32)], dim=1)
        T, faces_ind = self.optix_mesh.intersect(optix_ray)
        return faces_ind.to(torch.long), T > 0

    def render_mask(self, origin, ray_dir):
        optix_ray = torch.cat([origin.detach().to(torch.float32), ray_dir.detach().to(torch.float32)], dim=1)
        return self.optix_mesh.intersect_any(optix_ray).to(Float)

    def release_outputs(self, graph_sets=False):
        """Drops the dense outputs this scene keeps for re-use (RECYCLE_OUTPUTS: up to two sets of 55 B per ray) and the buffers zeroed
        ahead of time (PREFILL_NEXT); the next render call allocates and fills fresh ones.
        ``graph_sets=True`` also drops the output sets that CAPTURED render calls took for good (a graph's replays read and write those
        buffers: they were allocated before the capture, so the graph's own memory pool does not keep them alive) -- only legal once every
        graph captured on this scene has been destroyed; left alone (the default) they live as long as the scene."""
        om = self.optix_mesh
        with _on(self._dev):
            _lib.check(_lib.lib().drt_outputs_cancel(om._h))
            if getattr(om, "_prefilled", None) is not None:
                _lib.check(_lib.lib().drt_prefill_wait(om._h, _stream()))
        om._prefilled = None
        pool = getattr(om, "_out_pool", None)
        if pool is not None:
            pool.entries.clear()
        if graph_sets:
            om._graph_sets = []

    # ------------------------------------------------------------------ refraction path
    def bind_rays(self, origin, ray_dir, screen_pixel=None, valid=None, shared=None):
        """A handle for constant rays (and, optionally, their constant targets): see RayBinding.  ``render_transparent(handle)``."""
        return RayBinding(self, origin, ray_dir, screen_pixel, valid, shared)

    def render_transparent(self, origin, ray_dir=None):
        link = _GradLink()
        binding = origin if isinstance(origin, RayBinding) else None
        if binding is not None:
            origin, ray_dir = binding.origin, binding.ray_dir
            grid = binding._grid()
            link.targets = binding.targets
        else:
            grid = _grid_cache(origin, ray_dir, origin.shape[0], *_tile_hint(origin.shape[0])) if origin.is_contiguous() and ray_dir.is_contiguous() else (0, None)
        out_ori, out_dir, mask = _RenderTransparent.apply(self.vertices, origin, ray_dir, self, intIOR, extIOR, link, grid, binding)
        out_dir._drt_link = link            # lets ray_loss hand its gradient over as a row list (see _GradLink)
        link.mask = weakref.ref(mask)
        link.out_ori = weakref.ref(out_ori)
        return out_ori, out_dir, mask

    def render_paths(self, origin, ray_dir, max_bounces=4, tir="reflect", refraction="reference"):
        """Refraction paths of up to ``max_bounces`` (2..8) surface interactions: (out_ori, out_dir, mask) as render_transparent.
        ``tir``: what a hit with total internal reflection does -- "drop" ends the path (the reference's rule), "reflect" mirrors the
        ray (the reference's Reflect with refract_ray's flipped normal) and goes on.  A path is valid when it leaves the object after an
        even, non-zero number of refractions within ``max_bounces`` interactions; ``render_paths(o, d, 2, "drop")`` is
        ``render_transparent(o, d)`` bit for bit.  Differentiable w.r.t. ``self.vertices`` only: a gradient requested for ``origin``,
        ``ray_dir`` or a tensor IOR raises NotImplementedError.  Afterwards ``self.last_path_hits`` (uint8 [N]: interactions of each valid
        path, 0 elsewhere) and ``self.last_path_faces`` (int32 [K, N]: face per interaction, -1 past the end) describe the call.  Works
        with ``ray_loss`` through its dense gradient route.
        ``refraction``: how a refracting hit bends the ray -- "reference" (the default: the reference's Refract, which obeys
        tan(theta_t) = eta tan(theta_i); every route of this package) or "snell" (sin(theta_t) = eta sin(theta_i): what real glass
        does; these K-interaction calls only).  ``render_paths(o, d, 2, "drop", "snell")`` is the two-bounce path under
        Snell's law."""
        ior = self._check_paths_call("render_paths", origin, ray_dir, max_bounces, tir, refraction)
        return _RenderPaths.apply(self.vertices, origin, ray_dir, self, ior, int(max_bounces), _law_flags(tir, refraction))

    def render_image(self, camera_M, height, width, screen, texture, *, supersample=1, max_bounces=2, tir="drop", refraction="reference",
                     fresnel=True, void=0.0, invalid=0.0, max_samples=1 << 22, want_planes=False, absorption=None, environment=None, reflection=False):
        """What the pinhole camera ``camera_M`` = (R, K, R^-1, K^-1) sees of a textured planar screen through this mesh: a float32 image
        ``[height, width, C]`` on the device (drt_render_image; csrc/drt_image.h and DESIGN.md 10.2 state the law).  ``screen``: a
        ``drt_amd.render.Screen``; ``texture``: float32 ``[Th, Tw, C]`` (or ``[Th, Tw]``), C in {1, 3}, numpy or a device tensor.
        Every pixel is the mean of ``supersample``^2 (1..4) sample rays made in the kernel (``supersample=1``: ``views.generate_ray``'s
        ray).  A sample follows the path law of ``render_paths`` (``max_bounces``, ``tir``, ``refraction``; ``intIOR`` / ``extIOR`` of
        this module, read as ``render_paths`` reads them); with ``fresnel`` every refracting interaction weights it by 1 - R
        (FrDielectric), a mirrored one does not.  A sample without any interaction looks straight at the screen, one whose path
        completes looks along its exit ray -- the bilinear texture sample, or ``void`` off the screen; every other sample is
        ``invalid`` (each one number or C of them; the fills are not weighted).  The image is rendered in bands of at most
        ``max_samples`` samples (158 B of workspace each, shared with the path calls); the bands give the bits of the whole.  ``want_planes``: also return
        float32 ``[height, width]`` planes ``hit`` (share of samples with an interaction) and ``through`` (share whose path completed).
        Forward only: the image has no autograd graph and no gradient w.r.t. anything.  Two calls give the same bits.
        ``absorption``: None (clear glass: the call is what it was), or Beer-Lambert absorption coefficients per unit of mesh length --
        one number (every channel), C numbers, or a float64 tensor ``[C]``, each finite and >= 0: a through sample is also weighted by
        ``exp(-absorption_ch L)``, ``L`` the length its path travels inside the object (drt_render_image_absorb; csrc/drt_image_absorb.h
        and DESIGN.md 10.7 state the law; 8 B more workspace per sample).  ``want_planes`` then returns a fourth plane, ``length``: the
        mean of ``L`` over the pixel's through samples, 0 where there are none.
        ``environment``: None (the call is what it was), or a ``drt_amd.render.Environment`` -- a lat-long panorama at infinity with a
        rotation world -> environment frame: a direct or through sample that the screen does not catch then takes its weighted
        bilinear sample of the panorama along its exit direction instead of ``void`` (drt_render_image_env; csrc/drt_image_env.h and
        DESIGN.md 10.8 state the law).  ``screen`` and ``texture`` may then both be None: no screen, every ray sees the environment,
        and C is the environment's; with a screen the channel counts must agree.  It does not go with ``absorption``.
        ``want_planes`` then returns a fourth plane, ``reflect``.  ``reflection=True`` (needs an environment and ``fresnel``) adds the
        light the Fresnel term takes away at the outer surface: a sample whose first interaction enters the object reflects there; where
        one any-hit query finds the reflected ray unoccluded and the sample's path completes, its colour is
        ``T B(exit) + R1 B(reflected)`` with ``R1`` the reflectance of that interaction and ``B`` the background of a ray (screen, else
        environment); ``reflect`` is the share of a pixel's samples with such a term (0 everywhere without ``reflection``)."""
        from . import render as _render
        a = _render.check_render_args(camera_M, height, width, screen, texture, supersample, max_bounces, tir, refraction, fresnel, void, invalid,
                                      max_samples, want_planes, absorption, environment, reflection)
        ior = _ior_host(intIOR, "intIOR"), _ior_host(extIOR, "extIOR")
        dev = self._dev
        with _on(dev):
            tex = None if a["texture"] is None else torch.as_tensor(a["texture"], device=dev).to(torch.float32).contiguous()
            v = _f64c(self.vertices.detach(), "vertices")
            H, W, C = a["height"], a["width"], a["channels"]
            image = torch.empty((H, W, C), dtype=torch.float32, device=dev)
            planes = tuple(torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(2)) if a["want_planes"] else (None, None)
            if a["environment"] is not None:
                env = torch.as_tensor(a["environment"].texels, device=dev).to(torch.float32).contiguous()
                rot = a["environment"].packed()
                reflect = torch.empty((H, W), dtype=torch.float32, device=dev) if a["want_planes"] else None
                for y0, y1 in a["bands"]:
                    _lib.check(_lib.lib().drt_render_image_env(
                        self.optix_mesh._h, v.data_ptr(), a["camera"].ctypes.data, H, W, y0, y1, a["supersample"], ior[0], ior[1], a["max_bounces"],
                        a["law_flags"], a["fresnel"], None if tex is None else a["screen"].ctypes.data, _lib.ptr(tex), 0 if tex is None else tex.shape[0],
                        0 if tex is None else tex.shape[1], C, a["void"].ctypes.data, a["invalid"].ctypes.data, image.data_ptr(), _lib.ptr(planes[0]),
                        _lib.ptr(planes[1]), env.data_ptr(), env.shape[0], env.shape[1], rot.ctypes.data, int(a["reflection"]), _lib.ptr(reflect),
                        _stream()))
                return (image,) + planes + (reflect,) if a["want_planes"] else image
            if a["absorption"] is not None:
                length = torch.empty((H, W), dtype=torch.float32, device=dev) if a["want_planes"] else None
                for y0, y1 in a["bands"]:
                    _lib.check(_lib.lib().drt_render_image_absorb(
                        self.optix_mesh._h, v.data_ptr(), a["camera"].ctypes.data, H, W, y0, y1, a["supersample"], ior[0], ior[1], a["max_bounces"],
                        a["law_flags"], a["fresnel"], a["screen"].ctypes.data, tex.data_ptr(), tex.shape[0], tex.shape[1], C, a["void"].ctypes.data,
                        a["invalid"].ctypes.data, image.data_ptr(), _lib.ptr(planes[0]), _lib.ptr(planes[1]), a["absorption"].ctypes.data,
                        _lib.ptr(length), _stream()))
                return (image,) + planes + (length,) if a["want_planes"] else image
            for y0, y1 in a["bands"]:
                _lib.check(_lib.lib().drt_render_image(
                    self.optix_mesh._h, v.data_ptr(), a["camera"].ctypes.data, H, W, y0, y1, a["supersample"], ior[0], ior[1], a["max_bounces"],
                    a["law_flags"], a["fresnel"], a["screen"].ctypes.data, tex.data_ptr(), tex.shape[0], tex.shape[1], C, a["void"].ctypes.data,
                    a["invalid"].ctypes.data, image.data_ptr(), _lib.ptr(planes[0]), _lib.ptr(planes[1]), _stream()))
        return (image,) + planes if a["want_planes"] else image

    def image_loss_fused(self, camera_M, height, width, screen, texture, target, *, weight=None, ior_int=None, ior_ext=None, vertices=True,
                         want_image=False, supersample=1, max_bounces=2, tir="drop", refraction="reference", fresnel=True, void=0.0,
                         invalid=0.0, max_samples=1 << 22, screen_param=None, texture_param=None, camera_param=None, absorption=None, environment=None,
                         reflection=False, env_texels_param=None, env_rotation_param=None):
        """The photometric loss of ``render_image`` against a photograph: sum over pixels and channels of ``w (I - target)^2`` with ``I``
        the float64 pixel mean ``render_image`` rounds to float32 -- as a scalar, with its vertex gradient AND d loss / d (ior_int,
        ior_ext) computed alongside with a unit seed and scaled in the backward pass (drt_render_image_loss; csrc/drt_image_loss.h and
        DESIGN.md 10.3 state the law).  The gradient is the derivative of the whole law, Fresnel weights included, through the samples
        whose path completes and lands on the screen; a sample's class, its faces, the texel cell and the screen's border carry none,
        the screen's pose, the texture and the camera receive one through ``screen_param`` / ``texture_param`` / ``camera_param`` (below).
        ``target``: ``[height, width, C]`` (or ``[height, width]`` with a
        one-channel texture), float32, or uint8 read as value / 255; ``weight``: float32 ``[height, width]`` or None; numpy or device
        tensors.  ``ior_int`` / ``ior_ext``: None (this module's ``intIOR`` / ``extIOR``), floats, or 0-dim tensors (each is read to the
        host once per call, so such a call cannot be captured); the loss is differentiable w.r.t. whichever of them are tensors that
        require grad, and w.r.t. ``self.vertices`` unless ``vertices=False`` (a fixed mesh: no vertex gradient is computed, the kernel
        runs without its gradient table).  The law and band keywords are ``render_image``'s; the bands add into one set of
        accumulators.  ``want_image``: returns ``(loss, image)`` with ``render_image``'s bits.  Afterwards ``self.last_image_count`` is the
        number of through samples that carried a gradient (0-dim int64 tensor on the device).
        ``screen_param``: a float64 tensor ``[3, 3]`` with rows p0, eu, ev on any device that supplies the screen INSTEAD of ``screen``
        (which must then be None); its value is read to the host once per call, like a tensor IOR, and goes through ``Screen``'s checks;
        the loss is differentiable w.r.t. it when it requires grad.  ``texture_param``: a float32 or float64 tensor ``[Th, Tw, C]`` (or
        ``[Th, Tw]``) that supplies the texture instead of ``texture`` (then None); its gradient comes back in its own dtype, device and
        shape.  For these two the DIRECT samples carry a gradient as well (drt_render_image_loss_screen; csrc/drt_image_screen.h and
        DESIGN.md 10.4 state the law); the vertex and IOR gradients are the same with and without them.
        ``camera_param``: the pair ``(Rinv, Kinv)`` of float64 tensors on any device -- ``Rinv`` ``[4, 4]`` or ``[3, 4]`` (camera -> world;
        its top three rows are read), ``Kinv`` ``[3, 3]`` -- that supplies the camera INSTEAD of ``camera_M`` (then None); the values are
        read to the host once per call, and the loss is differentiable w.r.t. whichever of the two requires grad: all 21 numbers the
        renderer reads are independent inputs, and the gradient comes back in the tensors' own shapes (a ``[4, 4]`` ``Rinv`` gets a zero
        bottom row).  Direct and through samples both carry it (drt_render_image_loss_camera; csrc/drt_image_camera.h and DESIGN.md 10.5
        state the law); silhouettes are not differentiated.  It composes with the other keywords, ``vertices`` and tensor IORs, whose
        gradients are the same with and without it.  Without any of the three keywords the call is what it was.
        ``absorption``: ``render_image``'s -- None, one number, C numbers or a float64 tensor ``[C]`` (read to the host once per call,
        like a tensor IOR); the loss is then that of the absorbing image, the vertex and IOR gradients are the derivative of the whole
        law, the interior lengths included, and a tensor that requires grad receives d loss / d absorption, which costs no path
        recompute and is there on any scene and with ``vertices=False`` (drt_render_image_loss_absorb; csrc/drt_image_absorb.h and
        DESIGN.md 10.7 state the law).  It goes with none of ``screen_param`` / ``texture_param`` / ``camera_param``.
        ``environment`` / ``reflection``: ``render_image``'s (``screen`` and ``texture`` may then both be None); the loss is that of the
        image in front of the environment, with the outer-surface reflection when asked for, and the vertex and IOR gradients are the
        derivative of that whole law: the exit direction through the environment lookup, ``R1`` and the reflected ray through the first
        face (drt_render_image_loss_env; csrc/drt_image_env.h and DESIGN.md 10.8 state the law).  Every through sample then carries a
        gradient.  It goes with none of ``absorption`` / ``screen_param`` / ``texture_param`` / ``camera_param``.
        ``env_texels_param`` / ``env_rotation_param`` (both need ``environment``, which stays a ``render.Environment``): a float32 or
        float64 tensor shaped like the environment's texels (``[Eh, Ew, C]``, or ``[Eh, Ew]`` with one channel) that supplies the texels
        in their place, and a float64 tensor ``[3, 3]`` on any device that supplies the rotation in its place -- read to the host once per
        call, like ``screen_param``, and through ``Environment``'s own orthonormality check.  The loss is differentiable w.r.t. each that
        requires grad: every sample that reads the environment carries the gradient -- direct ones, through ones along their exit ray,
        added reflections --, the nine rotation entries are independent inputs, and the gradients come back in the tensors' own dtype,
        device and shape (drt_render_image_loss_env_param; csrc/drt_image_env_param.h and DESIGN.md 10.9 state the law).  The other
        gradients are the same with and without them; without both the call is what it was."""
        from . import render as _render
        a = _render.check_image_loss_args(camera_M, height, width, screen, texture, target, weight, ior_int, ior_ext, vertices, want_image, supersample,
                                          max_bounces, tir, refraction, fresnel, void, invalid, max_samples, screen_param, texture_param, camera_param,
                                          absorption, environment, reflection, env_texels_param, env_rotation_param)
        ior, tracked = _ior_args(intIOR if ior_int is None else ior_int, extIOR if ior_ext is None else ior_ext)
        dev = self._dev
        with _on(dev):
            tex = None if a["texture"] is None else torch.as_tensor(a["texture"], device=dev).to(torch.float32).contiguous()
            tgt = torch.as_tensor(a["target"], device=dev)
            tgt = (tgt.to(torch.float32) / 255.0 if tgt.dtype == torch.uint8 else tgt).reshape(a["height"], a["width"], a["channels"]).contiguous()
            wgt = None if a["weight"] is None else torch.as_tensor(a["weight"], device=dev).contiguous()
        inputs = (self.vertices if a["vertices"] else self.vertices.detach(),) + tracked
        if a["environment"] is not None:
            with _on(dev):
                env = torch.as_tensor(a["environment"].texels, device=dev).to(torch.float32).contiguous()
            param = env_texels_param is not None or env_rotation_param is not None      # (a keyword that is given takes its entry point)
            term = _image_env_term(self, a, ior, tex, env, tgt, wgt, param)
            loss = _UnitSeedTerm.apply(term, *inputs, *((env_texels_param, env_rotation_param) if param else ()))
            self.last_image_count = term.count
            return (loss, term.image) if a["want_image"] else loss
        if a["absorption"] is not None:
            term = _image_absorb_term(self, a, ior, tex, tgt, wgt)
            loss = _UnitSeedTerm.apply(term, *inputs, absorption if isinstance(absorption, torch.Tensor) else None)
            self.last_image_count = term.count
            return (loss, term.image) if a["want_image"] else loss
        if camera_param is not None:         # (a keyword that is given takes its entry point, whether or not its tensor requires grad)
            entry, inputs = "camera", inputs + (screen_param, texture_param, camera_param[0], camera_param[1])
        elif screen_param is not None or texture_param is not None:
            entry, inputs = "screen", inputs + (screen_param, texture_param)
        else:
            entry = "plain"
        term = _image_term(self, a, ior, tex, tgt, wgt, entry)
        loss = _UnitSeedTerm.apply(term, *inputs)
        self.last_image_count = term.count
        return (loss, term.image) if a["want_image"] else loss

    def bind_image_views(self, cameras, height, width, screens, targets, weights=None, *, environment=None):
        """A handle for the views of a capture of photographs (``render.ImageViews``) for ``image_loss_views_fused``: ``cameras`` a list of
        ``camera_M`` tuples, ``screens`` a list of ``render.Screen`` (one per camera), ``targets`` ``[n, height, width(, C)]`` float32, or
        uint8 read as value / 255, ``weights`` float32 ``[n, height, width]`` or None; numpy or device tensors.  The cameras and screens
        go to a device table once; the target and weight stacks stay resident.  ``environment`` (a ``render.Environment`` with the
        targets' channels): the room the capture was taken in, one for all views -- it belongs to the capture, so it
        lives here: its texels stay resident with the stacks, and the calls on this binding render in front of it.  With one,
        ``screens`` may be None: the capture has no screen.  Every argument error is raised before the device is touched
        (``render.check_image_views_args``)."""
        from . import render as _render
        return _render.ImageViews(self, _render.check_image_views_args(cameras, height, width, screens, targets, weights, environment))

    def image_loss_views_fused(self, binding, view_ids, texture, *, ior_int=None, ior_ext=None, vertices=True, supersample=1, max_bounces=2,
                               tir="drop", refraction="reference", fresnel=True, void=0.0, invalid=0.0, max_samples=1 << 22, environment=None,
                               reflection=False, absorption=None, want_images=False):
        """The SUM over ``view_ids`` (1..16 views of ``binding``, repeats allowed) of ``image_loss_fused`` of each view against its target
        (and weight plane) of the binding -- loss, vertex gradient, IOR partials, ``last_image_count`` -- evaluated as ONE forward
        wavefront and ONE adjoint pass instead of one chain of launches per view (drt_render_image_loss_views).  The views
        share ``texture``, the law and band keywords, the fills and the IORs, all as in ``image_loss_fused``; the listed views are stacked
        into an image of ``len(view_ids) * H`` rows, which is evaluated in bands of at most ``max_samples`` samples (a band may straddle
        a view border) into one set of accumulators.  No image output and no screen, texture or camera gradients:
        ``image_loss_fused`` has those.  A binding made with an environment (``bind_image_views(..., environment=)``) renders every view
        in front of it, as ``image_loss_fused(..., environment=)`` does view by view (drt_render_image_loss_views_env);
        ``texture`` is None exactly when that binding has no screens, and ``reflection=True`` (needs such a binding and ``fresnel``) adds
        the outer-surface reflection.  The environment belongs to the capture: ``environment=`` given HERE raises ``ValueError``, and so
        does ``reflection=True`` on a binding without an environment.  The environment's texels and rotation receive no gradient in this
        call; ``image_loss_fused`` keeps those.
        ``absorption``: ``image_loss_fused``'s -- None, one number, C numbers or a float64 tensor ``[C]`` (read to the
        host once per call).  Every view is then rendered with absorbing glass, on a binding with an environment too: the environment
        is attenuated along the interior length exactly like the texture, the reflection is not (that light never entered the object).
        The vertex and IOR gradients are the derivative of the whole law, the interior lengths included; a tensor that requires grad
        receives d loss / d absorption, from the transmitted light alone (drt_render_image_loss_views_absorb).  With None the call is
        what it was.  ``want_images=True`` (needs ``absorption``; 0.0 renders clear glass) returns ``(loss, images)`` with the float32
        images ``[k, H, W, C]`` of the listed views: the way to render a tinted object in a room -- a binding with one view serves for a
        single one, since ``render_image`` refuses that pair."""
        from . import render as _render
        if environment is not None:
            raise ValueError("environment: the multi-view call takes its environment from the binding; give it to bind_image_views(..., environment=)")
        if reflection is not False and not (isinstance(binding, _render.ImageViews) and binding.args.get("environment") is not None):
            raise ValueError("reflection: the multi-view call reflects the binding's environment and this binding has none; "
                             "give one to bind_image_views(..., environment=)")
        a = _render.check_image_views_law(binding, view_ids, texture, ior_int, ior_ext, vertices, supersample, max_bounces, tir, refraction, fresnel,
                                          void, invalid, max_samples, reflection, absorption, want_images)
        if binding.scene is not self:
            raise ValueError("binding was made by another scene's bind_image_views")
        ior, tracked = _ior_args(intIOR if ior_int is None else ior_int, extIOR if ior_ext is None else ior_ext)
        with _on(self._dev):
            tex = None if a["texture"] is None else torch.as_tensor(a["texture"], device=self._dev).to(torch.float32).contiguous()
        inputs = (self.vertices if a["vertices"] else self.vertices.detach(),) + tracked
        if a["absorption"] is not None:
            term = _image_views_absorb_term(self, binding, a, ior, tex, (a["max_bounces"], tir, refraction))
            # (inputs is (vertices, ior_int, ior_ext) -- _ior_args always gives two -- so the absorption sits at position 3, the ``users`` of
            # the term's sigma accumulators)
            assert len(inputs) == 3
            loss = _UnitSeedTerm.apply(term, *inputs, absorption if isinstance(absorption, torch.Tensor) else None)
            self.last_image_count = term.count
            if not a["want_images"]:
                return loss
            with _on(self._dev):
                return loss, term.image[torch.as_tensor(a["ids"], dtype=torch.int64, device=self._dev)]
        term = _image_views_term(self, binding, a, ior, tex, (a["max_bounces"], tir, refraction))
        loss = _UnitSeedTerm.apply(term, *inputs)
        self.last_image_count = term.count
        return loss

    @staticmethod
    def _check_law(max_bounces, tir, refraction):
        """The checks of the law itself, shared by every K-interaction call."""
        if isinstance(max_bounces, bool) or int(max_bounces) != max_bounces or not 2 <= int(max_bounces) <= 8:
            raise ValueError(f"max_bounces must be an integer in 2..8, got {max_bounces!r}")
        if tir not in ("drop", "reflect"):
            raise ValueError(f"tir must be 'drop' or 'reflect', got {tir!r}")
        if not isinstance(refraction, str) or refraction not in ("reference", "snell"):
            raise ValueError(f"refraction must be 'reference' or 'snell', got {refraction!r}")

    @staticmethod
    def _check_paths_call(who, origin, ray_dir, max_bounces, tir, refraction="reference"):
        """The argument checks of the K-interaction calls; returns the (intIOR, extIOR) floats."""
        Scene._check_law(max_bounces, tir, refraction)
        if _wants_input_grads(origin, ray_dir, intIOR, extIOR):
            raise NotImplementedError(f"{who} differentiates the vertices only: origin, ray_dir and the IORs must not require grad "
                                      "(render_transparent has those gradients for the two-bounce path)")
        return _ior_host(intIOR, "intIOR"), _ior_host(extIOR, "extIOR")

    def paths_ray_loss_fused(self, origin, ray_dir, screen_pixel, valid, max_bounces=4, tir="reflect", refraction="reference"):
        """ray_loss of this view under the law of ``render_paths`` -- ``ray_loss(*render_paths(origin, ray_dir, max_bounces, tir,
        refraction), screen_pixel, valid)`` -- in one call that writes no dense output (drt_render_paths_ray_loss_fused): the loss as a scalar, its
        vertex gradient computed alongside with a unit seed and scaled in the backward pass.  Differentiable w.r.t. ``self.vertices``
        only, like ``render_paths``.  ``origin`` may be a RayBinding: its rays are used, nothing else of it (no grid verdicts, seeds or
        recycled outputs exist for this law).  Afterwards ``self.last_path_count`` is the number of contributing rays (0-dim int64 tensor
        on the device; reading it synchronises, producing it does not)."""
        if isinstance(origin, RayBinding):
            origin, ray_dir = origin.origin, origin.ray_dir
        ior = self._check_paths_call("paths_ray_loss_fused", origin, ray_dir, max_bounces, tir, refraction)
        _stats["paths_fused_calls"] += 1
        term = _ray_term(self, origin, ray_dir, screen_pixel, valid, ior, (int(max_bounces), tir, refraction), None)
        loss = _UnitSeedTerm.apply(term, self.vertices)
        self.last_path_count = term.count
        return loss

    def paths_ray_loss_ior_fused(self, origin, ray_dir, screen_pixel, valid, ior_int, ior_ext=None, max_bounces=4, tir="reflect",
                                 refraction="reference", vertices=True):
        """``paths_ray_loss_fused`` that is also differentiable w.r.t. the indices of refraction: the loss as a scalar,
        its vertex gradient AND d loss / d (ior_int, ior_ext) computed alongside with a unit seed and scaled in the backward pass.
        The IORs are ARGUMENTS here: ``ior_int`` / ``ior_ext`` are floats or 0-dim float64 tensors (CPU or GPU; each is read to the
        host once per call, so a call with a tensor IOR cannot be captured), ``ior_ext=None`` is the module's ``extIOR`` read as a
        float; the module globals are not consulted otherwise.  Differentiable w.r.t. ``self.vertices`` when ``vertices=True`` and
        w.r.t. whichever IOR tensors require grad.  ``vertices=False`` is the calibration of a fixed mesh: no vertex gradient is
        computed (the kernel runs without its gradient table) and ``self.vertices`` receives none.  Rays that require grad raise
        NotImplementedError.  ``origin`` may be a RayBinding: its rays are used, nothing else.  The law and its checks are those of
        ``paths_ray_loss_fused``; afterwards ``self.last_path_count`` is the number of contributing rays."""
        if isinstance(origin, RayBinding):
            origin, ray_dir = origin.origin, origin.ray_dir
        Scene._check_law(max_bounces, tir, refraction)
        if _wants_input_grads(origin, ray_dir):
            raise NotImplementedError("paths_ray_loss_ior_fused differentiates the vertices and the IORs: origin and ray_dir must not require "
                                      "grad (render_transparent has those gradients for the two-bounce path)")
        ior, tracked = _ior_args(ior_int, _ior_host(extIOR, "extIOR") if ior_ext is None else ior_ext)
        _stats["paths_ior_fused_calls"] += 1
        term = _paths_ior_term(self, origin, ray_dir, screen_pixel, valid, ior, int(max_bounces), _law_flags(tir, refraction), bool(vertices))
        loss = _UnitSeedTerm.apply(term, self.vertices if vertices else self.vertices.detach(), *tracked)
        self.last_path_count = term.count
        return loss

    def ray_loss_fused(self, origin, ray_dir, screen_pixel, valid):
        """ray_loss of this view without materialising out_ori/out_dir/mask.  The fused kernel differentiates the vertices only: when
        a gradient of the rays or of a tensor IOR is requested, this is render_transparent + ray_loss (`fused_fallback_inputs` in
        cache_report())."""
        if _wants_input_grads(intIOR, extIOR) or (not isinstance(origin, RayBinding) and _wants_input_grads(origin, ray_dir)):
            _stats["fused_fallback_inputs"] += 1
            out_ori, out_dir, mask = self.render_transparent(origin, ray_dir)
            return ray_loss(out_ori, out_dir, mask, screen_pixel, valid)
        ior = _ior_host(intIOR, "intIOR"), _ior_host(extIOR, "extIOR")
        grid = None
        if isinstance(origin, RayBinding):
            origin, ray_dir, grid = origin.origin, origin.ray_dir, origin._grid()
        return _UnitSeedTerm.apply(_ray_term(self, origin, ray_dir, screen_pixel, valid, ior, None, grid), self.vertices)

    # ------------------------------------------------------------------ smoothness branch
    def dihedral_angle(self):
        """cos of the dihedral angle of every unique edge, differentiable w.r.t. vertices (DiffRender.py:440-443)."""
        return _Dihedral.apply(self.vertices, self.E2F)

    def sm_loss_fused(self):
        """sum -log(1 + cos dihedral) (reference optim.py:82-89) with its gradient in one kernel pass."""
        return _SmLossFused.apply(self.vertices, self)

    # ------------------------------------------------------------------ silhouette branch
    def silhouette_edge(self, origin: torch.Tensor):
        assert origin.dim() == 1
        if LAZY_SILHOUETTE and not torch.cuda.is_current_stream_capturing():
            return SilhouetteEdges(self.Edges, None, scene=self, origin=origin)       # (flags and edge set computed when somebody needs them)
        v = _f64c(self.vertices.detach(), "vertices")
        o = _f64c(origin.detach(), "origin")
        n = self.E2F.shape[0]
        flags = torch.empty(n, dtype=torch.uint8, device=v.device)
        with _on(v.device):
            _lib.check(_lib.lib().drt_silhouette_flags(v.data_ptr(), self.E2F.data_ptr(), n, o.data_ptr(), flags.data_ptr(), _stream()))
        if LAZY_SILHOUETTE:
            return SilhouetteEdges(self.Edges, flags)
        return self.Edges[flags.view(torch.bool)]

    def primary_visibility(self, silhouette_edge, camera_M, origin, detach_depth=False):
        """(index int64 [M,2] (x, y), output float32 [M]) of the in-view silhouette samples (DiffRender.py:459-479)."""
        lazy_ok = LAZY_VISIBILITY and not torch.cuda.is_current_stream_capturing()
        if isinstance(silhouette_edge, SilhouetteEdges) and silhouette_edge._t is None and lazy_ok:
            # NOTHING is computed now: the reference's loop feeds the pair straight into `(mask.view(resy, resx)[index[:, 1], index[:, 0]] -
            # output).abs().sum()` (optim.py:78) and adds the views' terms up (optim.py:72-80) -- SampleSet / LazySum evaluate that sum with one
            # fused launch; anything else that looks at the pair gets the sampling kernel, the compaction and the reference's tensors.
            ss = SampleSet(self, self.vertices, silhouette_edge, camera_M, origin, bool(detach_depth), int(resx), int(resy))
            return LazyIndex(ss), LazyOutput(ss)
        if isinstance(silhouette_edge, SilhouetteEdges):      # (unwrapped here: autograd.Function.apply should see plain tensors / tuples)
            silhouette_edge = (silhouette_edge._edges, silhouette_edge._flags) if silhouette_edge._t is None else silhouette_edge.tensor()
        return _EdgeSample.apply(self.vertices, silhouette_edge, camera_M, origin, self, bool(detach_depth), int(resx), int(resy))

    def vh_loss_fused(self, camera_M, origin, soft_mask):
        """sum |soft_mask[y, x] - 0.5| over the visible silhouette samples of one view and its vertex gradient
        (one view of reference optim.py:73-78) without any host round trip."""
        return self.vh_loss_fused_views([(camera_M, origin, soft_mask)])

    def vh_loss_fused_views(self, views):
        """The same summed over ``views`` = [(camera_M, origin[3], soft_mask), ...] (the whole of optim.py:73-78):
        one autograd node, three kernels per view."""
        flat = []
        for camera_M, origin, soft_mask in views:
            flat += [pack_camera(camera_M), origin, soft_mask]
        return _VhLossFused.apply(self.vertices, self, int(resx), int(resy), True, *flat)


LAZY_SILHOUETTE = True
# LAZY_VISIBILITY: primary_visibility returns stand-ins for (index, output) -- see SampleSet.  They behave as the reference's tensors for
# indexing (incl. assignment), len / shape / dtype / any attribute, operators, torch functions, isinstance(x, torch.Tensor) and
# torch.is_tensor(x); what they cannot do is pass a C++-level tensor check that does not go through __torch_function__ (torch.compile /
# torch.jit tracing of the caller's loss, a custom C++ op taking the pair): such callers set LAZY_VISIBILITY = False.
LAZY_VISIBILITY = os.environ.get("DRT_LAZY_VISIBILITY", "1") != "0"
