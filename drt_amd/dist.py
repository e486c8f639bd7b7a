"""View-parallel execution: one process per GPU, views sharded, one all-reduce per step.

The reference is single-GPU (no torch.distributed).  The views
of one optimisation step are independent given the (replicated) mesh, so they shard
with no data-path exchange: view k belongs to rank ``k % world``; every rank holds
the full mesh, rebuilds its own LBVH, accumulates a private float64 ``grad[V,3]``
and ONE all-reduce(sum) of that buffer (0.6 MB at 25 k vertices) precedes the
reference's ``limit_hook`` + SGD step (optim.py:155-171), which every rank then
applies identically, so vertices stay bit-identical without a broadcast
(SURVEY.md section 8e).  Backend ``nccl`` is RCCL over xGMI on ROCm; ``gloo`` is used
by the CPU tests.

The whole reconstruction loop (drt_amd.optim.optimize_sharded) uses ``owner`` instead: a view belongs to the rank of its position
in the schedule's sorted id list, so a schedule over every other view of a capture still spreads over every rank, and
``broadcast_mesh_`` installs rank 0's remeshed mesh on the others before every pass.
"""
from __future__ import annotations

import datetime
import os

import torch
import torch.distributed as dist


# DRT_DIST_FORCE=1: create the process group and issue the collectives even with ONE rank -- the RCCL path of a step
# (communicator, its streams, the all-reduce launch) exercised on a one-GPU box
_FORCE = os.environ.get("DRT_DIST_FORCE", "") not in ("", "0")


def _active():
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or _FORCE)


def env_world():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))


def active():
    """True when collectives go over a process group (more than one rank, or DRT_DIST_FORCE)."""
    return _active()


def rank_world():
    """(rank, world) of the default process group; (0, 1) without one."""
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def init(backend=None, timeout=None):
    """Initialise the default process group from the torchrun environment (no-op for world 1).  ``timeout`` (seconds; default
    DRT_DIST_TIMEOUT or 120): a collective that one rank never joins ends in an error on the others instead of a hang."""
    rank, local_rank, world = env_world()
    if (world > 1 or _FORCE) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        if backend is None:
            backend = os.environ.get("DRT_DIST_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if backend == "nccl":
            torch.cuda.set_device(local_rank)
        if timeout is None:
            timeout = float(os.environ.get("DRT_DIST_TIMEOUT", "120"))
        dist.init_process_group(backend=backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=timeout))
    return rank, local_rank, world


def shard_views(n_views, rank, world):
    """Indices of the views rank ``rank`` owns (round-robin, so a turntable is spread evenly)."""
    return list(range(rank, n_views, world))


def owner(view_id, index_list, world):
    """The rank that owns view ``view_id`` of a schedule: its position in the schedule's SORTED id list, modulo ``world``
    (Data.ray_view_ids / Data.silh_view_ids).  Fixed per view, not per draw, so a rank needs only its own views resident; for a full
    turntable it is ``shard_views``'s ``v % world``, and a schedule over every other view of a capture still spreads over all ranks."""
    ids = sorted(int(v) for v in index_list)
    import bisect
    p = bisect.bisect_left(ids, int(view_id))
    if p == len(ids) or ids[p] != int(view_id):
        raise KeyError(f"view {view_id} is not in the schedule's index list")
    return p % world


def owned_views(index_list, rank, world):
    """The views of a schedule rank ``rank`` owns (``owner(v, index_list, world) == rank``), ascending."""
    ids = sorted(int(v) for v in index_list)
    return ids[rank::world]


def broadcast_mesh_(scene, src=0):
    """Install rank ``src``'s mesh (float64 vertices, int64 faces) on every other rank through ``Scene._set_topology``: the sizes first,
    then the vertex and face words as ONE int64 payload.  No-op for a single process; returns whether a broadcast took place."""
    if not _active():
        return False
    dev = scene.vertices.device
    mine = dist.get_rank() == src
    sizes = torch.tensor([scene.vertices.shape[0], scene.faces.shape[0]] if mine else [0, 0], dtype=torch.int64, device=dev)
    dist.broadcast(sizes, src)
    nv, nf = int(sizes[0]), int(sizes[1])
    if mine:
        payload = torch.cat([scene.vertices.detach().to(torch.float64).contiguous().view(-1).view(torch.int64),
                             scene.faces.to(torch.int64).contiguous().view(-1)])
    else:
        payload = torch.empty(3 * (nv + nf), dtype=torch.int64, device=dev)
    dist.broadcast(payload, src)
    if not mine:
        V = payload[:3 * nv].view(torch.float64).view(nv, 3).clone()
        F = payload[3 * nv:].view(nf, 3).clone()
        scene._set_topology(V, F)
    return True


def allreduce_sum_(t):
    """In-place sum over ranks; identity for a single process."""
    if _active():
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


def allreduce_max_float(x, device):
    t = torch.tensor([x], dtype=torch.float64, device=device)
    if _active():
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def barrier():
    if _active():
        dist.barrier()
