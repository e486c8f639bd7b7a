"""The optimisation loop the refraction path plugs into -- host-side mirror of the
reference's optim.py, on the HIP-backed ``drt_amd.diffrender``.

    Loss_calculator.ray_loss / vh_loss / sm_loss / all_loss   reference optim.py:59-130
    limit_hook, setup_opt, interp_L / interp_R, optimize       reference optim.py:145-219

Differences from the reference, all outside the per-view math:
  * the capture comes from any object with the reference's ``Data`` interface (``get_view``,
    ``ray_view_generator``, ``silh_view_generator``, ``resx``, ``resy``): drt_amd.captured_data has the
    reference's capture classes and ``SyntheticData``, which stands in for the HDF5 captures (not distributed);
  * the MeshLab remesh between passes (optim.py:12-52, an external program) is done in-process by
    drt_amd.remesh (same algorithm and parameters); ``remesh=`` takes any other callable, or None;
  * multi-GPU: ``full_batch_step`` shards views over ranks and all-reduces the vertex gradient
    once per step (drt_amd.dist); the reference is single-GPU and one view per step.  ``optimize_sharded`` is the whole
    loop on N ranks (ShardedIteration: all three terms, one exchange per iteration; the remesh on rank 0, broadcast).

The loops share their parts: ``check_loop_config`` (every refusal), ``pass_schedule`` / ``resolve_remesh`` / ``run_steps`` (the pass loop)
and ONE iteration class (FusedIteration; ShardedIteration is its form with an exchange), whose terms go through the enqueue functions the
autograd Functions use (diffrender.enqueue_ray_term, silhouette.enqueue_vh_term / enqueue_sm_term).
"""
from __future__ import annotations

import time

import numpy as np
import torch

from . import diffrender as Render
from . import dist as ddist
from . import mesh_io, views
from .captured_data import Data, Data_Pointgray, Data_Redmi, PhotoData, SyntheticData, SyntheticPhotoData, get_data  # noqa: F401  (reference optim.py:7, 132-143)

Float = torch.float64

HyperParams = {          # reference config.py:18-39
    "name": "hand", "IOR": 1.4723, "Pass": 20, "Iters": 200,
    "ray_w": 40, "sm_w": 0.08, "vh_w": 2e-3,
    "momentum": 0.95, "start_lr": 0.1, "lr_decay": 0.5, "start_len": 10, "end_len": 1, "num_view": 72,
}


def path_law(hp):
    """(max_bounces, tir) of ``HyperParams``, or None for the reference's path (both absent, or 2 and "drop"): what selects
    ``Scene.render_paths`` instead of ``render_transparent`` in the drop-in loop.  Bad values raise ValueError here, before a pass starts.
    A third key, ``HyperParams["refraction"]`` (absent, None or "reference": the reference's formula, the results above), adds the
    refraction formula: with "snell" the result is (max_bounces, tir, "snell"), and 2 / "drop" is a law too -- the two-bounce path bent
    by Snell's law.  The tuple is what ``Scene.render_paths`` / ``paths_ray_loss_fused`` take after the rays."""
    k, tir, refraction = hp.get("max_bounces", 2), hp.get("tir", "drop"), hp.get("refraction", "reference")
    k = 2 if k is None else k
    tir = "drop" if tir is None else tir
    refraction = "reference" if refraction is None else refraction
    if isinstance(k, bool) or int(k) != k or not 2 <= int(k) <= 8:
        raise ValueError(f"HyperParams['max_bounces'] must be an integer in 2..8, got {k!r}")
    if tir not in ("drop", "reflect"):
        raise ValueError(f"HyperParams['tir'] must be 'drop' or 'reflect', got {tir!r}")
    if not isinstance(refraction, str) or refraction not in ("reference", "snell"):
        raise ValueError(f"HyperParams['refraction'] must be 'reference' or 'snell', got {refraction!r}")
    if refraction == "snell":
        return (int(k), tir, "snell")
    return None if (int(k) == 2 and tir == "drop") else (int(k), tir)


def law_flags(law):
    """``law_flags`` of the drt_render_paths_law_* entry points for a normalised law."""
    return Render._law_flags(law[1], law[2] if len(law) > 2 else "reference")


def path_law_keyword(law, hp, who):
    """The ``path_law=(max_bounces, tir)`` or ``(max_bounces, tir, refraction)`` keyword of the loops, normalised by the rules of
    ``path_law``: None when absent or (2, "drop") -- today's kernels -- else (int K, tir), or (int K, tir, "snell") under Snell's law
    (a "reference" third element is dropped); bad values raise ValueError.  The keyword selects the ONE-PASS form of the law
    (``Scene.paths_ray_loss_fused`` / drt_render_paths_ray_loss_fused) where the caller runs the one-pass terms; the ``HyperParams``
    keys keep meaning the drop-in route.  Like ``Scene.render_paths`` the law differentiates the vertices only: not with ``ior_lr > 0``.
    Looks at nothing but its arguments."""
    if law is None:
        return None
    try:
        k, tir, *rest = law
        (refraction,) = rest or ("reference",)
    except (TypeError, ValueError):
        raise ValueError(f"path_law must be None or (max_bounces, tir) or (max_bounces, tir, refraction), got {law!r}") from None
    refraction = "reference" if refraction is None else refraction
    if not isinstance(refraction, str) or refraction not in ("reference", "snell"):
        raise ValueError(f"path_law's refraction must be 'reference' or 'snell', got {refraction!r}")
    law = path_law({"max_bounces": k, "tir": tir, "refraction": refraction})
    if law is None:
        return None
    if float(hp.get("ior_lr", 0) or 0) > 0:
        raise NotImplementedError(f"path_law cannot be combined with HyperParams['ior_lr'] > 0 in {who}: the K-interaction law "
                                  "differentiates the vertices only")
    if path_law(hp) is not None:
        raise ValueError("the path law was given twice: HyperParams['max_bounces'] / ['tir'] and the path_law keyword")
    return law


def check_loop_config(hp, law, who, one_pass, loop=False):
    """The one validation of a loop's configuration, before anything touches the scene or the capture; returns the normalised
    ``path_law`` keyword (``path_law_keyword``).  ``who`` names the caller in the messages.  ``one_pass``: the caller runs the one-pass
    terms only, for which the ``HyperParams`` spelling of a law -- the drop-in route -- is refused.  ``loop``: the caller is a whole loop
    (optimize, optimize_sharded), which has ``HyperParams["ior_lr"]`` to honour; the iteration classes never read it.  The
    ``HyperParams`` refusals fire first, bad values of either spelling raise ValueError."""
    ior_lr = float(hp.get("ior_lr", 0) or 0)
    if loop and one_pass and ior_lr > 0:
        raise NotImplementedError(f"HyperParams['ior_lr'] > 0 (a learnable IOR) is not supported by {who}: use the drop-in loop "
                                  "optimize(..., fused=False)")
    if path_law(hp) is not None:
        if one_pass:
            raise NotImplementedError(f"HyperParams['max_bounces'] / ['tir'] other than 2 / 'drop' are not supported by {who}: use the "
                                      "drop-in loop optimize(..., fused=False)")
        if loop and ior_lr > 0:
            raise NotImplementedError("HyperParams['max_bounces'] / ['tir'] cannot be combined with ior_lr > 0: Scene.render_paths "
                                      "differentiates the vertices only")
    return path_law_keyword(law, hp, who)


def loss_weights(hp, resy, mean_len):
    """(w_ray, w_vh, w_sm): the fixed scalings of reference optim.py:127-129."""
    return hp["ray_w"] * 217.5 / resy / resy, hp["vh_w"] * 217.5 / resy, hp["sm_w"] * mean_len / 10


class Loss_calculator:
    """Same role and method names as the reference class (optim.py:59-130); every term is evaluated by
    the HIP kernels behind ``drt_amd.diffrender``.  ``fused=True`` uses the one-pass kernels
    (``Scene.ray_loss_fused`` / ``Scene.vh_loss_fused`` / ``Scene.sm_loss_fused``) -- same values, no dense
    intermediates and no host synchronisation."""

    N_SILHOUETTE_VIEWS = 8          # the reference loops over np.arange(0, 72, 9)

    def __init__(self, scene, data, HyperParams, fused=False, path_law=None):
        self.law = path_law_keyword(path_law, HyperParams, "Loss_calculator")       # (first: bad values raise before anything is touched)
        self.scene, self.data, self.HyperParams, self.fused = scene, data, HyperParams, fused
        self.ray_view = data.ray_view_generator()
        self.silh_view = data.silh_view_generator()

    def _silhouette_term(self, view_id):
        """sum |soft_mask[y, x] - 0.5| over the visible silhouette samples of one view (optim.py:74-78)."""
        _, _, soft_mask, origin, _, camera_M = self.data.get_view(view_id)
        eye = origin[0]
        edges = self.scene.silhouette_edge(eye)
        pix, out = self.scene.primary_visibility(edges, camera_M, eye, detach_depth=True)
        image = soft_mask.view((self.data.resy, self.data.resx))
        return (image[pix[:, 1], pix[:, 0]] - out).abs().sum()

    def vh_loss(self):
        if self.fused:
            views = []
            for _ in range(self.N_SILHOUETTE_VIEWS):
                _, _, soft_mask, origin, _, camera_M = self.data.get_view(next(self.silh_view))
                views.append((camera_M, origin[0], soft_mask))
            return self.scene.vh_loss_fused_views(views)
        # accumulated like the reference does (optim.py:71-78: `vh_loss = 0; vh_loss += term`): with the lazy pair of primary_visibility the
        # terms are not evaluated one by one -- the sum is ONE fused launch over the eight views, enqueued here (Render.force), i.e. on the
        # stream this method is called under
        total = 0
        for _ in range(self.N_SILHOUETTE_VIEWS):
            total += self._silhouette_term(next(self.silh_view))
        return Render.force(total)

    def sm_loss(self):
        if self.fused:
            return self.scene.sm_loss_fused()
        cos_dihedral = self.scene.dihedral_angle()
        return (-torch.log(1 + cos_dihedral)).sum()

    def ray_loss(self):
        view_id = next(self.ray_view)
        target, valid, _, origin, ray_dir, _ = self.data.get_view(view_id)
        bind = getattr(self.data, "get_binding", None)       # a capture whose views are resident constants offers a handle per view (RayBinding)
        if bind is not None:
            origin, ray_dir = bind(self.scene, view_id), None
        law = path_law(self.HyperParams)
        if law is not None and self.fused:       # (the HyperParams keys mean the drop-in route)
            check_loop_config(self.HyperParams, None, "the fused terms", one_pass=True)
        law = law or self.law
        if law is not None:                 # paths of up to K interactions
            if self.fused:                  # (the path_law keyword: the one-pass form with the one-pass terms)
                return self.scene.paths_ray_loss_fused(origin, ray_dir, target, valid, *law)
            if ray_dir is None:
                origin, ray_dir = origin.origin, origin.ray_dir
            exit_o, exit_d, exit_mask = self.scene.render_paths(origin, ray_dir, *law)        # dense outputs, ray_loss's dense gradient
            return Render.ray_loss(exit_o, exit_d, exit_mask, target, valid)
        if self.fused:
            return self.scene.ray_loss_fused(origin, ray_dir, target, valid)
        exit_o, exit_d, exit_mask = self.scene.render_transparent(origin, ray_dir)
        return Render.ray_loss(exit_o, exit_d, exit_mask, target, valid)

    # The three terms of an iteration are independent given the mesh.  The silhouette and smoothness terms are enqueued on a SIDE stream and
    # run beside the refraction term -- at the reference's iteration size (one 960x1280 view, ~50 k primary hits) each term is a chain of
    # small launches that leaves most of the chip idle, so the iteration costs the longest chain instead of their sum.  With the drop-in
    # methods (fused=False) the silhouette term synchronises with the host once per view (its outputs are dynamically sized): on its own
    # stream that wait covers its own launches only, not the refraction term enqueued before it.  Values are unchanged (same kernels, same
    # inputs).
    CONCURRENT_TERMS = True

    def all_loss(self):
        hp = self.HyperParams
        none = torch.zeros((), dtype=Float, device=self.scene.vertices.device)
        if self.CONCURRENT_TERMS and self.scene.vertices.is_cuda and not torch.cuda.is_current_stream_capturing():
            main = torch.cuda.current_stream()
            side = getattr(self, "_side_stream", None)
            if side is None:
                side = self._side_stream = torch.cuda.Stream(device=self.scene.vertices.device)
            side.wait_stream(main)                      # the rebuild (update_verticex) and the vertices are enqueued on `main`
            # (the refraction term first: it is the longest chain, and at this size the HOST's enqueue order is the GPU's start order)
            ray = self.ray_loss() if hp["ray_w"] != 0 else none
            with torch.cuda.stream(side):
                vh = self.vh_loss() if hp["vh_w"] != 0 else none
                sm = self.sm_loss() if hp["sm_w"] != 0 else none
            main.wait_stream(side)
            for t in (vh, sm):
                t.record_stream(main)                   # allocated on the side stream, consumed on `main` from here on
            parts = (ray, vh, sm)
        else:
            parts = (self.ray_loss() if hp["ray_w"] != 0 else none,
                     self.vh_loss() if hp["vh_w"] != 0 else none,
                     self.sm_loss() if hp["sm_w"] != 0 else none)
        w = loss_weights(hp, self.data.resy, self.scene.mean_len)
        if self.fused:
            # one stack + one dot instead of five scalar kernels (and five more in the backward pass): the iteration is a chain of small launches
            key = (w, parts[0].device)
            if getattr(self, "_w_key", None) != key:
                self._w_key, self._w_vec = key, torch.tensor(w, dtype=Float, device=parts[0].device)
            total = torch.dot(torch.stack(parts), self._w_vec)
        else:
            total = w[0] * parts[0] + w[1] * parts[1] + w[2] * parts[2]
        return total, parts


def loss_string(parts):
    ray_loss, vh_loss, sm_loss = parts
    return f"ray={float(ray_loss.detach()):g} vh={float(vh_loss.detach()):g} sm={float(sm_loss.detach()):g}"


def interp_L(start, end, it, Pass):
    assert it <= Pass - 1
    return it * ((end - start) / (Pass - 1)) + start


def interp_R(start, end, it, Pass):
    return 1 / interp_L(1 / start, 1 / end, it, Pass)


def limit_hook(grad, max_abs=1.0):
    """NaN -> 0, clamp to +-1 (reference optim.py:155-162); +-inf clamps like any large value."""
    g = torch.nan_to_num(grad, nan=0.0, posinf=None, neginf=None)
    return g.clamp_(-max_abs, max_abs)


class FusedLimitSGD:
    """limit_hook + torch.optim.SGD(momentum, nesterov) for ONE float64 parameter in one kernel (drt_limit_sgd_step) instead
    of ~8 elementwise launches: ``step()`` sanitises ``parameter.grad`` in place (NaN -> 0, clamp +-max_abs: the
    reference's hook, optim.py:155-162) and applies the update.  Same numbers as the hook + torch.optim.SGD."""

    applies_limit = True

    def __init__(self, parameter, lr, momentum=0.0, nesterov=False, max_abs=1.0):
        self.parameter, self.lr, self.momentum, self.nesterov, self.max_abs = parameter, float(lr), float(momentum), bool(nesterov), float(max_abs)
        self.buf = None
        self.param_groups = [{"params": [parameter], "lr": self.lr, "momentum": self.momentum, "nesterov": self.nesterov}]

    def zero_grad(self, set_to_none=True):
        if set_to_none:
            self.parameter.grad = None
        elif self.parameter.grad is not None:
            self.parameter.grad.zero_()

    def step(self):
        from . import _lib
        from .optix_mesh import _stream, _on
        p, g = self.parameter, self.parameter.grad
        if g is None:
            return
        assert p.is_cuda and p.dtype == torch.float64 and g.dtype == torch.float64 and p.is_contiguous() and g.is_contiguous()
        first = self.buf is None
        if first and self.momentum != 0.0:
            self.buf = torch.empty_like(p)
        with _on(p.device):
            _lib.check(_lib.lib().drt_limit_sgd_step(p.data_ptr(), g.data_ptr(), _lib.ptr(self.buf), p.numel(), self.param_groups[0]["lr"], self.momentum,
                                                      int(self.nesterov), int(first), self.max_abs, _stream()))


def sharded_loss_weights(hp, resy, mean_len, views_per_step=1):
    """The weights of an iteration of ``views_per_step`` refraction views: loss_weights with the refraction weight divided by the step's
    view count (the refraction term is the MEAN over the step's views); ``views_per_step = 1`` gives loss_weights exactly."""
    w_ray, w_vh, w_sm = loss_weights(hp, resy, mean_len)
    return (w_ray / views_per_step if views_per_step != 1 else w_ray), w_vh, w_sm


class FusedIteration:
    """One iteration of the reference's loop (optim.py:198-215: vertices = init + parameter, update_verticex, all_loss, backward,
    limit_hook, SGD) on the one-pass kernels WITHOUT the autograd graph around them.

    With ``Loss_calculator(fused=True)`` every term already returns its loss together with d term / d vertices; autograd only
    multiplies those by the weights and adds them up -- ~15 tiny torch ops, three Function nodes and a backward pass whose HOST cost
    (0.7 ms) exceeds the GPU time of the whole iteration at the reference's size (one 960x1280 refraction view, 8 silhouette views).
    Here ``step()`` has three parts.  It draws the iteration's views (``draw``: same schedule generators as Loss_calculator, or the
    ``schedule=(ray_view, silh_view)`` pair a pass loop carries from stepper to stepper).  It enqueues the terms with the functions the
    autograd Functions use (diffrender.enqueue_ray_term / enqueue_vh_term / enqueue_sm_term) into ONE zeroed accumulator block of
    3n + 3 values -- term k's gradient element i at k n + i, loss k at 3n + k; float64, or fixed-point cells in deterministic mode
    (drt_amd/det.py) -- the silhouette and smoothness terms on a side stream beside the refraction term.  And it runs the tail: the
    weighted sum, limit_hook and SGD(nesterov) in one kernel (drt_limit_sgd_step3; in deterministic mode after the cells' conversion).
    ``path_law=(K, tir)``: the refraction term is the K-interaction law's one-pass kernel.  What the enqueued kernels read stays
    referenced (``_vertices``, ``_keep``) until the next step replaces it."""

    N_SILHOUETTE_VIEWS = 8
    sharded = False          # (ShardedIteration: evaluate the owned views only, ONE exchange over the ranks in the tail)

    def __init__(self, scene, data, HyperParams, lr, concurrent=True, path_law=None, schedule=None):
        self._init(scene, data, HyperParams, lr, 1, concurrent, path_law, schedule)

    def _init(self, scene, data, hp, lr, views_per_step, concurrent, path_law, schedule):
        from . import _lib, det
        self.law = check_loop_config(hp, path_law, type(self).__name__, one_pass=True)
        self._lib = _lib
        self.scene, self.data, self.hp = scene, data, hp
        self.k = int(views_per_step)
        if self.k < 1:
            raise ValueError("views_per_step must be >= 1")
        self.rank, self.world = ddist.rank_world() if self.sharded else (0, 1)
        self.ray_view, self.silh_view = schedule if schedule is not None else (data.ray_view_generator(), data.silh_view_generator())
        self.own_ray = self.own_silh = None
        if self.sharded:
            self.own_ray = set(ddist.owned_views(data.ray_view_ids(), self.rank, self.world))
            self.own_silh = set(ddist.owned_views(data.silh_view_ids(), self.rank, self.world))
        dev = scene.vertices.device
        self.init_vertices = scene.vertices.detach().clone()
        self.parameter = torch.zeros_like(self.init_vertices)
        n = self.n = self.init_vertices.numel()
        shape = tuple(self.init_vertices.shape)
        self.det = det.on()
        words = det._CELL_WORDS if self.det else 1
        acc = self.acc = torch.zeros((3 * n + 3) * words, dtype=torch.int64 if self.det else Float, device=dev)
        self._fills = [acc]                                                    # what a step zeroes
        self._g_ptr = [acc.data_ptr() + 8 * words * k * n for k in range(3)]
        self._l_ptr = [acc.data_ptr() + 8 * words * (3 * n + k) for k in range(3)]
        self.total_grad = torch.empty_like(self.init_vertices)
        if not self.sharded:
            # drt_limit_sgd_step3 reads the block's float64 values: the block itself, or (deterministic) what the cells convert to
            vals = torch.empty(3 * n + 3, dtype=Float, device=dev) if self.det else acc
            self.grads, self.losses = vals[:3 * n].view((3,) + shape), vals[3 * n:]
            self._finalize = [(acc[:3 * n * words], vals[:3 * n]), (acc[3 * n * words:], vals[3 * n:])] if self.det else []
        elif self.det:
            self.limbs = torch.empty((3 * n + 3) * 4, dtype=torch.int64, device=dev)      # the exchange: ONE drt_fx_to_limbs launch
            self.losses = torch.zeros(3, dtype=Float, device=dev)
        else:
            # the exchange is [weighted partial gradient (n), loss parts (3)]: the terms add their losses straight into its tail (the
            # block's own three loss values stay unused)
            self.grads = acc[:3 * n].view((3,) + shape)
            self.xbuf = torch.zeros(n + 3, dtype=Float, device=dev)
            self.losses, self.total_grad = self.xbuf[n:], self.xbuf[:n].view(shape)
            self._l_ptr = [self.xbuf.data_ptr() + 8 * (n + k) for k in range(3)]
            self._fills.append(self.losses)
        self.total = torch.zeros((), dtype=Float, device=dev)
        self.buf = torch.empty_like(self.init_vertices) if hp["momentum"] != 0 else None
        self.first = True
        self.lr, self.momentum = float(lr), float(hp["momentum"])
        self.n_allreduce = 0
        self.collective_events = []
        self.last_owned = (0, 0)
        self._keep = []
        # The side stream of the silhouette / smoothness terms must not share a hardware queue with the caller's stream: a process gets four
        # queues, further streams are multiplexed onto them, and a stream that lands in the caller's queue sits BEHIND the barrier with
        # which the caller's stream waits for the refraction term -- the terms then run one after the other whatever the streams say
        # (rocprofv3: the fresh torch stream shared queue 1 with stream 0).  The library's second pipeline stream is idle during a call of
        # this size and has a queue of its own.
        self.side = None
        if concurrent:
            import ctypes
            h = ctypes.c_void_p()
            rc = _lib.lib().drt_internal_stream(scene.optix_mesh._h, 2, ctypes.byref(h))
            self.side = torch.cuda.ExternalStream(h.value, device=dev) if rc == 0 and h.value else torch.cuda.Stream(device=dev)
        self._w = None

    def draw(self):
        """This iteration's schedule, the same on every rank: (refraction view ids, silhouette view ids)."""
        hp = self.hp
        ray = [next(self.ray_view) for _ in range(self.k)] if hp["ray_w"] != 0 else []
        silh = [next(self.silh_view) for _ in range(self.N_SILHOUETTE_VIEWS)] if hp["vh_w"] != 0 else []
        return ray, silh

    def step(self):
        """Runs the iteration; returns (weighted total, parts [ray, vh, sm]) of the WHOLE iteration (all ranks) as device tensors of
        THIS iteration (views of buffers that the next call overwrites: read them, or clone them, before stepping again)."""
        from . import det
        from .optix_mesh import _stream
        lib, check, ptr = self._lib.lib(), self._lib.check, self._lib.ptr
        scene, hp, data, n = self.scene, self.hp, self.data, self.n
        dev = self.init_vertices.device
        # 1. the iteration's views: everything drawn, or this rank's share of it
        ray_ids, silh_ids = self.draw()
        if self.sharded:
            ray_ids = [v for v in ray_ids if v in self.own_ray]
            silh_ids = [v for v in silh_ids if v in self.own_silh]
        self.last_owned = (len(ray_ids), len(silh_ids))       # (this rank's share of the iteration: refraction views, silhouette views)
        with torch.no_grad(), torch.cuda.device(dev):
            vertices = self.init_vertices + self.parameter
            scene.update_verticex(vertices)
            # 2. the terms, into the zeroed block
            for t in self._fills:
                t.zero_()
            g_ptr, l_ptr = self._g_ptr, self._l_ptr
            main = torch.cuda.current_stream()
            if self.side is not None:
                self.side.wait_stream(main)
            keep = self._enqueue_first_term(vertices, ray_ids)
            with torch.cuda.stream(self.side) if self.side is not None else torch.no_grad():
                # (the smoothness term first: it needs no tree, so it runs while the build finishes; the silhouette probes wait for the tree.
                # On one rank only: the sum over ranks is the term itself, not world times it)
                if hp["sm_w"] != 0 and self.rank == 0:
                    Render.enqueue_sm_term(scene, vertices, l_ptr[2], g_ptr[2])
                if silh_ids:
                    views_ = []
                    for v in silh_ids:
                        _, _, soft_mask, origin, _, camera_M = data.get_view(v)
                        views_.append((camera_M, origin[0], soft_mask))
                    keep += Render.enqueue_vh_term(scene, vertices, views_, data.resx, data.resy, True, l_ptr[1], g_ptr[1])
            if self.side is not None:
                main.wait_stream(self.side)
            # 3. the tail: d total / d vertices (= d total / d parameter) = the weighted sum of the three terms' gradients, limit_hook,
            # SGD(nesterov) -- one kernel, or two around the exchange
            w = self._weights()
            if self._w is None or self._w[0] != w:
                self._w = (w, torch.tensor(w, dtype=Float, device=dev))
            wv = self._w[1]
            step = (self.lr, self.momentum, 1, int(self.first), 1.0)
            if not self.sharded:
                for cells, vals in self._finalize:
                    det.value_into(cells, vals)
                check(lib.drt_limit_sgd_step3(self.parameter.data_ptr(), self.total_grad.data_ptr(), ptr(self.buf), n, *step, self.grads.data_ptr(),
                                              wv.data_ptr(), self.losses.data_ptr(), self.total.data_ptr(), _stream()))
            elif self.det:
                check(lib.drt_fx_to_limbs(self.acc.data_ptr(), 3 * n + 3, self.limbs.data_ptr(), _stream()))
                self._exchange(self.limbs)
                check(lib.drt_fx_limbs_limit_sgd_step3(self.limbs.data_ptr(), n, self.parameter.data_ptr(), self.total_grad.data_ptr(), ptr(self.buf),
                                                       *step, wv.data_ptr(), self.losses.data_ptr(), self.total.data_ptr(), _stream()))
            else:
                check(lib.drt_weight_terms3(self.grads.data_ptr(), wv.data_ptr(), n, self.xbuf.data_ptr(), _stream()))
                self._exchange(self.xbuf)
                check(lib.drt_limit_sgd_step_total(self.parameter.data_ptr(), self.xbuf.data_ptr(), ptr(self.buf), n, *step, wv.data_ptr(),
                                                   self.losses.data_ptr(), self.total.data_ptr(), _stream()))
            self.first = False
            self._vertices, self._keep = vertices, keep      # (alive until the next step: kernels enqueued above read them)
        return self.total, self.losses

    def _enqueue_first_term(self, vertices, ray_ids):
        """Enqueues the term of slot 0 of the accumulator block for the drawn views -- here the refraction term, one call per view -- on
        the current stream; returns what the enqueued kernels read."""
        keep = []
        for v in ray_ids:
            target, valid, _, origin, ray_dir, _ = self.data.get_view(v)
            keep += Render.enqueue_ray_term(self.scene, vertices, origin, ray_dir, target, valid, self.law, self._l_ptr[0], self._g_ptr[0])
        return keep

    def _weights(self):
        """The weights of the block's three terms in this iteration."""
        return sharded_loss_weights(self.hp, self.data.resy, self.scene.mean_len, self.k)

    def _exchange(self, t):
        """The iteration's one collective (a sum over ranks; nothing to do for a single process)."""
        if not ddist.active():
            return
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
        ddist.allreduce_sum_(t)
        ev[1].record()
        self.n_allreduce += 1
        self.collective_events.append(ev)

    def collective_seconds(self):
        """Seconds spent in the collectives since the last call (synchronises the device)."""
        if not self.collective_events:
            return 0.0
        self.collective_events[-1][1].synchronize()
        s = sum(a.elapsed_time(b) for a, b in self.collective_events) / 1e3
        self.collective_events = []
        return s


class ShardedIteration(FusedIteration):
    """The rank-local form of FusedIteration: one iteration of the pass loop on ``world`` ranks with ONE collective.

    Every rank draws the same schedule -- ``views_per_step`` refraction views, then the reference's 8 silhouette views, from the capture's
    generators (same seed on every rank) -- and evaluates only the views it owns (drt_amd.dist.owner: a view's position in the schedule's
    sorted id list, modulo world); the smoothness term is rank 0's.  The rank's contribution is all-reduced once: in float64 mode the
    weighted partial gradient and the three loss parts (n + 3 values; drt_weight_terms3), in deterministic mode the exchange words of
    the whole accumulator block ((3n + 3) x 4 int64; drt_fx_to_limbs).  After it every rank applies the same weighted sum, limit_hook and
    SGD(nesterov) (drt_limit_sgd_step_total / drt_fx_limbs_limit_sgd_step3), so the parameters stay bit-identical across ranks without a
    broadcast.  A rank that owns nothing in an iteration still joins the exchange.  The two-kernel tail runs with one rank too: with one
    rank and ``views_per_step = 1`` this is FusedIteration with another tail (in deterministic mode the same bits).  ``n_allreduce``
    counts the collectives issued; ``collective_events`` holds (start, end) CUDA events around each of them until the caller reads them.
    ``last_owned``: this rank's (refraction, silhouette) view counts of the last step."""

    sharded = True

    def __init__(self, scene, data, HyperParams, lr, views_per_step=1, concurrent=True, path_law=None, schedule=None):
        self._init(scene, data, HyperParams, lr, views_per_step, concurrent, path_law, schedule)


class AbsorptionState:
    """The absorption coefficients of a photometric fit and, when they are fitted, the moments of their optimiser:
    ``sigma`` float64 numpy [C] on the host -- what the next step's call takes --, and ``calibrate.fit_absorption``'s update: Adam
    steps of ``lr`` (in units of sigma) on the C numbers, each followed by the projection onto ``sigma >= 0``.  ``lr == 0``: sigma is
    fixed and ``update`` is never called.  ``optimize_photometric`` makes one and hands it to every pass's stepper, so the fit and its
    moments carry across passes."""

    def __init__(self, absorption, channels, lr=0.0):
        from . import render
        if isinstance(lr, bool) or not isinstance(lr, (int, float, np.integer, np.floating)) or not (float(lr) >= 0.0) or not np.isfinite(float(lr)):
            raise ValueError(f"absorption_lr must be a finite number >= 0, got {lr!r}")
        self.lr = float(lr)
        start = render.check_absorption(0.0 if absorption is None else absorption, channels)
        self.sigma = np.ascontiguousarray(start, dtype=np.float64).copy()
        self.steps = 0
        self._param = self._opt = None
        if self.lr > 0.0:
            self._param = torch.tensor(self.sigma, dtype=torch.float64, requires_grad=True)
            self._opt = torch.optim.Adam([self._param], lr=self.lr)

    @property
    def fitted(self):
        return self.lr > 0.0

    def update(self, grad):
        """One Adam step on ``grad`` (C float64 numbers on the host: d weighted loss / d sigma), then the projection; returns sigma."""
        self._param.grad = torch.as_tensor(np.asarray(grad, dtype=np.float64).reshape(self.sigma.shape)).clone()
        self._opt.step()
        with torch.no_grad():
            self._param.clamp_(min=0.0)
        self.sigma[:] = self._param.detach().numpy()          # (in place: the array the next call's pointer is taken from)
        self.steps += 1
        return self.sigma


class PhotoIteration(FusedIteration):
    """FusedIteration for a capture of plain photographs (captured_data.PhotoData): slot 0 of the accumulator block, where the
    refraction term goes, holds the photometric image term of ``views_per_step`` drawn views, evaluated as ONE forward wavefront and ONE
    adjoint pass (diffrender.enqueue_image_views_term) with the weight ``HyperParams["image_w"] / (views_per_step H W)``
    -- the mean squared residual per pixel.  The silhouette and smoothness terms, the side stream and the tail are FusedIteration's.
    ``path_law`` = (max_bounces, tir[, refraction]), ``fresnel`` and ``supersample`` are the image's law (``Scene.render_image``);
    ``HyperParams["IOR"]`` is the object's index of refraction.  A capture with an ``environment`` is rendered in
    front of it (its binding carries it), without a screen when the capture has none; ``reflection=True`` (needs such a capture and
    ``fresnel``) adds the outer-surface reflection.  ``absorption``: None (clear glass: the call of before),
    ``render.check_absorption``'s forms, or an ``AbsorptionState``; every view is then rendered with absorbing glass
    (drt_render_image_loss_views_absorb), in a room too.  With ``absorption_lr == 0`` sigma is fixed and the step stays free of
    read-backs.  ``absorption_lr > 0`` fits sigma jointly with the mesh (from ``absorption``, or from 0 without one): after each step the
    C accumulated partials are copied to the host -- ONE small device-to-host copy and synchronisation per step, which is why it is
    opt-in --, weighted like the image term, and ``AbsorptionState.update`` makes the Adam step and the projection onto sigma >= 0 that
    the next step's call takes.  ``self.absorption`` is the state (None for clear glass).  One process only."""

    def __init__(self, scene, data, HyperParams, lr, views_per_step=8, path_law=(6, "reflect", "snell"), fresnel=True, supersample=1, concurrent=True,
                 schedule=None, max_samples=1 << 22, reflection=False, absorption=None, absorption_lr=0.0):
        import torch.distributed as tdist
        if tdist.is_available() and tdist.is_initialized():
            raise NotImplementedError("PhotoIteration runs in one process: under an initialised torch.distributed group the photometric term "
                                      "has no exchange (optimize_sharded shards the refraction term of captures with correspondences)")
        from . import render
        hp = dict(HyperParams)
        hp.setdefault("ray_w", 0)
        if "image_w" not in hp:
            raise ValueError("PhotoIteration needs HyperParams['image_w'], the weight of the photometric term")
        k = render._int(views_per_step, "views_per_step")
        if not 1 <= k <= render.MAX_VIEWS_PER_CALL:
            raise ValueError(f"views_per_step must be in 1..{render.MAX_VIEWS_PER_CALL}, got {k}")
        law = path_law_keyword(path_law, hp, "PhotoIteration") or (2, "drop")
        self.image_law = (tuple(law) + ("reference",))[:3]
        if not isinstance(fresnel, (bool, np.bool_)):
            raise ValueError(f"fresnel must be True or False, got {fresnel!r}")
        if not isinstance(reflection, (bool, np.bool_)):
            raise ValueError(f"reflection must be True or False, got {reflection!r}")
        if reflection and getattr(data, "environment", None) is None:
            raise ValueError("reflection=True needs a capture with an environment (PhotoData(..., environment=))")
        if reflection and not fresnel:
            raise ValueError("reflection=True needs fresnel=True: the reflected share is the complement of what the Fresnel term transmits")
        self.fresnel, self.supersample, self.reflection = bool(fresnel), supersample, bool(reflection)
        self.bands_of = lambda n: render.plan_bands(n * data.resy, data.resx, supersample, max_samples)
        self._init(scene, data, hp, lr, k, concurrent, None, schedule)
        self.binding = data.binding(scene)
        dev = scene.vertices.device
        with torch.cuda.device(dev):
            self.texture = None if data.screens is None else torch.as_tensor(render.check_texture(data.texture), device=dev).to(torch.float32).contiguous()
        c = self.binding.channels
        self.fills = (render._fill(getattr(data, "void", 0.0), c, "void"), render._fill(getattr(data, "invalid", 0.0), c, "invalid"))
        self.ior = (Render._ior_host(hp["IOR"], "HyperParams['IOR']"), Render._ior_host(Render.extIOR, "extIOR"))
        self.last_views = []
        if isinstance(absorption, AbsorptionState):
            if absorption.sigma.shape != (c,):
                raise ValueError(f"absorption: the state holds {absorption.sigma.size} coefficients, the capture has {c} channels")
            self.absorption = absorption
        elif absorption is None and not isinstance(absorption_lr, bool) and absorption_lr == 0:
            self.absorption = None
        else:
            self.absorption = AbsorptionState(absorption, c, absorption_lr)
        self._sigma_acc = self._sigma_like = None
        if self.absorption is not None and self.absorption.fitted:
            from . import det
            with torch.cuda.device(dev):
                self._sigma_like = torch.empty(c, dtype=Float, device=dev)
                self._sigma_acc = det.acc(self._sigma_like)
            self._fills.append(self._sigma_acc)

    def draw(self):
        """(image view ids, silhouette view ids) of this iteration, from the capture's two generators."""
        hp = self.hp
        image = [next(self.ray_view) for _ in range(self.k)] if hp["image_w"] != 0 else []
        silh = [next(self.silh_view) for _ in range(self.N_SILHOUETTE_VIEWS)] if hp["vh_w"] != 0 else []
        return image, silh

    def _enqueue_first_term(self, vertices, image_ids):
        self.last_views = list(image_ids)
        if not image_ids:
            return []
        return Render.enqueue_image_views_term(self.scene, vertices, self.binding, image_ids, self.texture, self.image_law, self.supersample, self.fresnel,
                                               *self.fills, self.ior, self._l_ptr[0], self._g_ptr[0], bands=self.bands_of(len(image_ids)),
                                               reflection=self.reflection, absorption=None if self.absorption is None else self.absorption.sigma,
                                               grad_sigma_ptr=None if self._sigma_acc is None else self._sigma_acc.data_ptr())

    def step(self):
        """FusedIteration's step; with ``absorption_lr > 0`` followed by the read-back of the C sigma partials of this step and the
        host-side update of the coefficients (``AbsorptionState.update``)."""
        out = super().step()
        if self._sigma_acc is not None and self.last_views:
            from . import det
            with torch.no_grad(), torch.cuda.device(self._sigma_acc.device):
                partial = det.value(self._sigma_acc, self._sigma_like).cpu().numpy()          # (the step's one synchronisation)
            self.absorption.update(self._weights()[0] * partial)
        return out

    def _weights(self):
        hp, data = self.hp, self.data
        _, w_vh, w_sm = loss_weights(hp, data.resy, self.scene.mean_len)
        return hp["image_w"] / (self.k * data.resy * data.resx), w_vh, w_sm


def optimize_photometric(scene, data, HyperParams, views_per_step=8, remesh="isotropic", output=True, path_law=(6, "reflect", "snell"), fresnel=True,
                         supersample=1, reflection=False, absorption=None, absorption_lr=0.0):
    """The pass / iteration loop of ``optimize_sharded`` on one rank with PhotoIteration steps: fits ``scene``'s mesh to the photographs of
    ``data`` (captured_data.PhotoData) under ``HyperParams`` (``image_w`` in the place of ``ray_w``; the other keys as in ``optimize``).
    ``remesh`` as in ``optimize``; ``reflection``, ``absorption`` and ``absorption_lr`` as in PhotoIteration: ONE ``AbsorptionState`` is made here and
    handed to every pass's stepper, so a fit of the coefficients carries across passes; it is returned in ``stats["absorption"]`` (None for clear glass; its
    ``sigma`` holds the final values).  Returns (scene, history, stats): history = the weighted loss every 100 iterations, stats the passes,
    iterations and ``step_seconds`` (the iterations without the remesh, device-synchronised at the end of each pass)."""
    remesh = resolve_remesh(remesh)
    hp = dict(HyperParams)
    hp.setdefault("ray_w", 0)
    check_loop_config(hp, None, "optimize_photometric", one_pass=True, loop=True)
    Render.intIOR = hp["IOR"]
    Render.resy, Render.resx = data.resy, data.resx
    schedule = (data.ray_view_generator(), data.silh_view_generator())      # one view schedule across passes
    stats = {"views_per_step": int(views_per_step), "passes": 0, "iterations": 0, "step_seconds": 0.0}
    history = []
    state = absorption
    if not isinstance(state, AbsorptionState) and (absorption is not None or absorption_lr != 0):
        from . import render
        state = AbsorptionState(absorption, int(render.check_texture(data.texture).shape[2]) if data.screens is not None else int(data.environment.texels.shape[2]),
                                absorption_lr)
    stats["absorption"] = state
    for i_pass, remesh_len, lr in pass_schedule(hp):
        if output:
            print(f"remesh_len {remesh_len:g} lr {lr:g}")
        if remesh is not None:
            remesh(scene, remesh_len)
        stepper = PhotoIteration(scene, data, hp, lr, views_per_step, path_law=path_law, fresnel=fresnel, supersample=supersample, schedule=schedule,
                                 reflection=reflection, absorption=state)
        torch.cuda.synchronize(scene.vertices.device)
        t0 = time.perf_counter()
        run_steps(stepper, hp["Iters"], history, output)
        torch.cuda.synchronize(scene.vertices.device)
        stats["step_seconds"] += time.perf_counter() - t0
        stats["iterations"] += hp["Iters"]
        stats["passes"] += 1
    return scene, history, stats


def pass_schedule(hp):
    """(i_pass, remesh_len, lr) of every pass (reference optim.py:191-193): both interpolated harmonically from their start to their end
    value over the passes; one pass alone runs at the start values."""
    n = hp["Pass"]
    for i_pass in range(n):
        if n > 1:
            yield i_pass, interp_R(hp["start_len"], hp["end_len"], i_pass, n), interp_R(hp["start_lr"], hp["lr_decay"] * hp["start_lr"], i_pass, n)
        else:
            yield i_pass, hp["start_len"], hp["start_lr"]


def resolve_remesh(remesh):
    """The ``remesh=`` argument of the loops as a callable ``remesh(scene, remesh_len)`` or None: "isotropic" is the device remesher
    (drt_amd.remesh_gpu), "isotropic-host" the sequential host version, its checker (drt_amd.remesh); anything else is returned as is."""
    if remesh == "isotropic":
        from .remesh_gpu import GpuMeshlabserver
        return GpuMeshlabserver().remesh
    if remesh == "isotropic-host":
        from .remesh import Meshlabserver
        return Meshlabserver().remesh
    return remesh


def run_steps(stepper, iters, history, say):
    """``iters`` steps of an iteration object; every 100th is reported (``say``) and its weighted loss appended to ``history``."""
    for it in range(iters):
        total, parts = stepper.step()
        if it % 100 == 0:
            if say:
                print(f"Iteration {it}: {loss_string(tuple(parts))} maxgrad={stepper.total_grad.abs().max():g}")
            history.append(float(total))


def optimize_sharded(scene, data, HyperParams, views_per_step=1, remesh="isotropic", output=True, path_law=None):
    """``optimize(..., fused=True)`` on every rank of the default process group (one process without one): the pass / iteration loop with
    ShardedIteration steps, ONE all-reduce per iteration, and before every pass the remesh on rank 0 with its result broadcast to the
    others (drt_amd.dist.broadcast_mesh_: the remesher need not give the same mesh in two processes).  ``remesh`` as in optimize (run on
    rank 0 only).  Returns (scene, history, stats): history = the weighted loss every 100 iterations; stats counts the collectives
    (``allreduces`` and ``allreduces_per_iteration``, mesh ``broadcasts`` and ``broadcasts_per_pass``) and times the steps
    (``step_seconds``: the iterations without the remesh, device-synchronised at the end of each pass; ``collective_seconds``: CUDA-event
    time between the start and the end of the all-reduces).  ``path_law=(K, tir)``: as in ShardedIteration."""
    rank, world = ddist.rank_world()
    remesh = resolve_remesh(remesh)
    law_kw = check_loop_config(HyperParams, path_law, "optimize_sharded", one_pass=True, loop=True)
    say = output and rank == 0
    Render.intIOR = HyperParams["IOR"]
    Render.resy, Render.resx = data.resy, data.resx
    schedule = (data.ray_view_generator(), data.silh_view_generator())      # one view schedule across passes
    stats = {"world": world, "views_per_step": int(views_per_step), "passes": 0, "iterations": 0, "allreduces": 0, "broadcasts": 0,
             "step_seconds": 0.0, "collective_seconds": 0.0}
    start_time = time.time()
    history = []
    for i_pass, remesh_len, lr in pass_schedule(HyperParams):
        if say:
            print(f"remesh_len {remesh_len:g} lr {lr:g}")
        if remesh is not None:
            if rank == 0:
                remesh(scene, remesh_len)
            stats["broadcasts"] += int(ddist.broadcast_mesh_(scene, src=0))
        stepper = ShardedIteration(scene, data, HyperParams, lr, views_per_step, path_law=law_kw, schedule=schedule)
        torch.cuda.synchronize(scene.vertices.device)
        t0 = time.perf_counter()
        run_steps(stepper, HyperParams["Iters"], history, say)
        torch.cuda.synchronize(scene.vertices.device)
        stats["step_seconds"] += time.perf_counter() - t0
        stats["collective_seconds"] += stepper.collective_seconds()
        stats["allreduces"] += stepper.n_allreduce
        stats["iterations"] += HyperParams["Iters"]
        stats["passes"] += 1
    stats["allreduces_per_iteration"] = stats["allreduces"] / max(1, stats["iterations"])
    stats["broadcasts_per_pass"] = stats["broadcasts"] / max(1, stats["passes"])
    if say:
        print(f"optimize time : {time.time() - start_time}")
    return scene, history, stats


def setup_opt(scene, lr, HyperParams, hook=True, fused=False):
    """``fused=True`` (needs ``hook=False``): a FusedLimitSGD, which applies limit_hook itself inside its one-kernel step."""
    init_vertices = scene.vertices.detach().clone()
    parameter = torch.zeros(init_vertices.shape, dtype=Float, requires_grad=True, device=init_vertices.device)
    if fused:
        assert not hook, "FusedLimitSGD applies the limit itself: build it with hook=False"
        return init_vertices, parameter, FusedLimitSGD(parameter, lr, HyperParams["momentum"], nesterov=True)
    if hook:
        parameter.register_hook(limit_hook)
    # foreach=False: the multi-tensor kernels of the default implementation take ~35 us each for this ONE small tensor
    # (four per step: 0.14 ms of a 1.2 ms iteration); the single-tensor path does the same arithmetic in ~5 us ops
    opt = torch.optim.SGD([parameter], lr=lr, momentum=HyperParams["momentum"], nesterov=True, foreach=False)
    return init_vertices, parameter, opt


def optimize(scene, data, HyperParams, remesh="isotropic", output=True, fused=False, path_law=None):
    """The reference's pass / iteration loop (optim.py:190-215) for an existing scene and data object.
    ``remesh``: "isotropic" (default) re-tessellates to ``remesh_len`` before every pass like the reference's
    ``meshlabserver.remesh`` (optim.py:195), with the device remesher of drt_amd.remesh_gpu ("isotropic-host": the sequential
    host version of drt_amd.remesh); ``None`` keeps the topology; or any callable ``remesh(scene, remesh_len)``.

    ``HyperParams["ior_lr"] > 0`` (absent or 0: the reference's loop): the index of refraction is learned too -- a float64 leaf, starting
    at ``HyperParams["IOR"]``, in its own SGD param group with that learning rate (same momentum / Nesterov, not clamped by limit_hook),
    carried across passes and remeshes.  The drop-in loop only (``fused=False``); returns (scene, history, fitted IOR), and
    ``Render.intIOR`` is the fitted float afterwards.

    ``HyperParams["max_bounces"]`` (absent or 2) and ``HyperParams["tir"]`` (absent or "drop"): with any other value the refraction term
    traces paths of up to that many interactions (``Scene.render_paths`` + ``Render.ray_loss``); the drop-in loop only, and not together
    with ``ior_lr``.

    ``path_law=(max_bounces, tir)`` (keyword; None or (2, "drop"): today's kernels) selects the same law explicitly and works with both
    loops: with ``fused=True`` the refraction term is the one-pass ``Scene.paths_ray_loss_fused``, with ``fused=False`` it takes the
    ``render_paths`` + ``ray_loss`` route of the ``HyperParams`` keys.  Not together with ``ior_lr``."""
    law_kw = check_loop_config(HyperParams, path_law, "the fused loop" if fused else "optimize", one_pass=fused, loop=True)
    remesh = resolve_remesh(remesh)
    ior_lr = float(HyperParams.get("ior_lr", 0) or 0)
    ior = None
    if ior_lr > 0:
        ior = torch.tensor(float(HyperParams["IOR"]), dtype=Float, device=scene.vertices.device, requires_grad=True)
    Render.intIOR = HyperParams["IOR"] if ior is None else ior
    Render.resy, Render.resx = data.resy, data.resx
    loss_calculator = Loss_calculator(scene, data, HyperParams, fused=fused, path_law=law_kw)       # (and the one view schedule across passes)
    start_time = time.time()
    history = []
    for i_pass, remesh_len, lr in pass_schedule(HyperParams):
        if output:
            print(f"remesh_len {remesh_len:g} lr {lr:g}")
        if remesh is not None:
            remesh(scene, remesh_len)
        if fused:      # the one-pass terms without the autograd graph around them (same arithmetic, a third of the host work)
            stepper = FusedIteration(scene, data, HyperParams, lr, path_law=law_kw, schedule=(loss_calculator.ray_view, loss_calculator.silh_view))
            run_steps(stepper, HyperParams["Iters"], history, output)
            continue
        init_vertices, parameter, opt = setup_opt(scene, lr, HyperParams)
        if ior is not None:
            opt.add_param_group({"params": [ior], "lr": ior_lr})
        for it in range(HyperParams["Iters"]):
            opt.zero_grad()
            vertices = init_vertices + parameter
            scene.update_verticex(vertices)
            loss, parts = loss_calculator.all_loss()
            loss.backward()
            if it % 100 == 0 and output:
                print(f"Iteration {it}: {loss_string(parts)} maxgrad={parameter.grad.abs().max():g}")
            history.append(float(loss.detach())) if (it % 100 == 0) else None
            opt.step()
        if ior is not None and output:
            print(f"IOR {float(ior.detach()):.6f}")
    if output:
        print(f"optimize time : {time.time() - start_time}")
    if ior is not None:
        Render.intIOR = float(ior.detach())
        return scene, history, Render.intIOR
    return scene, history


def local_loss_backward(scene, local_views, init_vertices, parameter, ray_w, fused=False):
    """The rank-local part of a full-batch step: rebuild, every local view's ray loss, backward.  Leaves d(ray_w * loss)/d
    parameter in ``parameter.grad`` (None for a rank without views) and returns the unweighted loss."""
    vertices = init_vertices + parameter
    scene.update_verticex(vertices)
    parts = []
    for view in local_views:
        # (target, valid, origin, ray_dir) -- the tensors of Data.get_view -- or (target, valid, handle) with handle = scene.bind_rays(...):
        # the explicit form of "these rays are constants" (diffrender.RayBinding)
        target, valid, origin = view[0], view[1], view[2]
        ray_dir = view[3] if len(view) > 3 else None
        if fused:
            parts.append(scene.ray_loss_fused(origin, ray_dir, target, valid))
        else:
            out_ori, out_dir, mask = scene.render_transparent(origin, ray_dir)
            parts.append(Render.ray_loss(out_ori, out_dir, mask, target, valid))
    if not parts:
        return torch.zeros((), dtype=Float, device=vertices.device)
    loss = parts[0] if len(parts) == 1 else torch.stack(parts).sum()
    if loss.requires_grad:
        # d(ray_w * loss): the weight goes in as the seed of the backward pass (one cached scalar) instead of a multiplication
        # node -- the step is a chain of small launches, and each elementwise kernel of the loss arithmetic is ~5 us of it
        loss.backward(_seed(ray_w, loss))
    return loss


_SEEDS = {}


def _seed(w, like):
    key = (float(w), like.dtype, like.device)
    t = _SEEDS.get(key)
    if t is None:
        if len(_SEEDS) > 64:
            _SEEDS.clear()
        t = _SEEDS[key] = torch.full((), float(w), dtype=like.dtype, device=like.device)
    return t


def full_batch_step(scene, local_views, init_vertices, parameter, opt, ray_w, fused=False):
    """One step over ALL views of this rank (BASELINE.json's '72 views forward+backward per iter'):
    rebuild, per-view ray loss, backward, ONE all-reduce of grad[V,3], limit_hook, SGD step.

    ``parameter`` must NOT carry the gradient hook (``setup_opt(..., hook=False)``): the reference clamps the
    gradient of the whole step (optim.py:155-162), i.e. AFTER the sum over views, so here the clamp follows the
    all-reduce; a hook would clamp every rank's partial sum first.  A rank without views still takes part in the
    all-reduce (with zeros) and applies the same update, so parameters stay identical on every rank."""
    hooks = getattr(parameter, "_backward_hooks", None)
    if hooks:
        raise RuntimeError("full_batch_step: `parameter` has a gradient hook; build it with setup_opt(..., hook=False) "
                           "(limit_hook is applied here, after the all-reduce)")
    opt.zero_grad(set_to_none=True)
    from . import det
    sink = det.begin_sink()                 # deterministic mode: the refraction terms leave their exact accumulators here instead of float64 gradients
    try:
        loss = local_loss_backward(scene, local_views, init_vertices, parameter, ray_w, fused)
    finally:
        entries = det.end_sink()
    if sink is not None:
        # ONE exchange, exact: the 128-bit sums of every call of every rank are added as integers and converted once -- N GPUs, one GPU, any
        # split of the views give the same bits (what autograd did not route through the sink, nothing in this step, is added as before)
        g = det.collect(entries, parameter, ddist.allreduce_sum_, _seed(ray_w, parameter))
        if not (fused or (Render.EAGER_LOSS_GRAD and Render.SPARSE_LOSS_GRAD)):
            # (module switches that route ray_loss's gradient through autograd as float64 instead: the same on every rank, so every rank
            # joins this second collective or none does)
            g = g + ddist.allreduce_sum_(parameter.grad if parameter.grad is not None else torch.zeros_like(parameter))
        elif parameter.grad is not None:
            raise RuntimeError("full_batch_step (deterministic mode): a gradient reached `parameter` outside the exact sink")
    else:
        g = parameter.grad if parameter.grad is not None else torch.zeros_like(parameter)   # a rank with no views
        ddist.allreduce_sum_(g)             # the only exchange of the step
    parameter.grad = g if getattr(opt, "applies_limit", False) else limit_hook(g)     # clamp after the sum over views, as on one GPU
    opt.step()
    return loss
