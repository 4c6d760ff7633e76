"""Per-video sharding across the GPUs of one node and the single collective of the path.

Every dataset sample is one (video, object) with its own InferenceCore and no shared state
(reference interactions/eval.py:92-99, generate_fq_dataset.py:60-69); the reference shards evaluation
by ``--min-idx/--max-idx`` (eval_annotation_method.py:34-35).  Here: one process per GPU, a static
longest-processing-time assignment of samples to ranks (work ~ frame count), NO collective inside
propagation, and one end-of-run gather of fixed-width per-sample rows (RCCL over xGMI when the
backend is "nccl"; "gloo" in the CPU tests).  The per-object sessions of a video share one engine and its
frame features by default: the drivers then deal whole videos (``lpt_assign_grouped``, ``chunk_bounds``)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np
import torch
import torch.distributed as dist


def init_from_env():
    """One process per GPU (torch.distributed.run sets RANK / LOCAL_RANK / WORLD_SIZE): binds this process to its device and joins
    the process group - RCCL ("nccl") by default.  STCN_DIST_BACKEND=gloo + STCN_DIST_DEVICE=0 exist for the multi-rank preflight on
    a one-GPU box (all ranks on one device, CPU collectives).  Returns (rank, world); a single process is (0, 1) with no group."""
    import os
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("STCN_DIST_DEVICE", os.environ.get("LOCAL_RANK", 0)))
    if torch.cuda.is_available():
        torch.cuda.set_device(local)
    if world <= 1:
        return 0, 1
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    backend = os.environ.get("STCN_DIST_BACKEND", "nccl")
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
    return dist.get_rank(), world


def lpt_assign(costs: Sequence[float], world: int) -> List[List[int]]:
    """Deterministic LPT (heaviest sample first onto the least-loaded rank, ties -> lowest rank), followed by a refinement that
    moves or swaps samples out of the heaviest rank while that lowers the maximum load.  Plain LPT leaves 5 % imbalance on the 30
    DAVIS-2017-val lengths over 8 ranks (259 frames against a mean of 246); refined: 0.4 % (247)."""
    order = sorted(range(len(costs)), key=lambda i: (-costs[i], i))
    load = [0.0] * world
    out: List[List[int]] = [[] for _ in range(world)]
    for i in order:
        r = min(range(world), key=lambda j: (load[j], j))
        out[r].append(i)
        load[r] += costs[i]
    for _ in range(4 * len(costs)):                       # hill climbing on the maximum load; every step lowers it strictly
        hi = max(range(world), key=lambda j: (load[j], -j))
        best = None                                       # (new pair maximum, i in hi, rank b, j in b or None)
        for i in out[hi]:
            for b in range(world):
                if b == hi:
                    continue
                for j in [None] + out[b]:
                    cj = costs[j] if j is not None else 0.0
                    pair = max(load[hi] - costs[i] + cj, load[b] + costs[i] - cj)
                    if pair < load[hi] - 1e-9 and (best is None or pair < best[0] - 1e-9):
                        best = (pair, i, b, j)
        if best is None:
            break
        _, i, b, j = best
        out[hi].remove(i); out[b].append(i)
        load[hi] -= costs[i]; load[b] += costs[i]
        if j is not None:
            out[b].remove(j); out[hi].append(j)
            load[b] -= costs[j]; load[hi] += costs[j]
    return [sorted(p, key=lambda i: (-costs[i], i)) for p in out]


def _groups_in_order(groups: Sequence) -> List[List[int]]:
    """The members of every group (a hashable key per sample), groups in the order of their first member, members in sample order."""
    members: dict = {}
    for i, g in enumerate(groups):
        members.setdefault(g, []).append(i)
    return list(members.values())


def lpt_assign_grouped(costs: Sequence[float], groups: Sequence, world: int) -> List[List[int]]:
    """``lpt_assign`` over GROUPS of samples: ``groups[i]`` is the key of sample i's group (the drivers: its video), a group is never
    split, and its cost is the sum of its members' (the objects of a video cost its frames each: frames x objects).  The per-object
    sessions of a video run on one engine that keeps the frame features between them (InferenceCore.reset(keep_frame_features=True)), so
    they have to land on one rank.  Deterministic, every sample exactly once; a rank lists its groups in ``lpt_assign``'s order and the
    members of a group in sample order - with one member per group the result IS ``lpt_assign(costs, world)``."""
    if len(groups) != len(costs):
        raise ValueError(f"{len(costs)} costs for {len(groups)} group keys")
    members = _groups_in_order(groups)
    parts = lpt_assign([sum(costs[i] for i in m) for m in members], world)
    return [[i for g in part for i in members[g]] for part in parts]


def chunk_bounds(groups: Sequence, chunks: int, costs: Sequence[float] = None) -> List[int]:
    """Cut a sequence of samples into ``chunks`` contiguous pieces of about equal cost (``costs``; default: one per sample): the
    ``chunks + 1`` bounds, first 0, last ``len(groups)``.  ``groups[i]`` is the group key of sample i, the samples of a group adjacent
    (the drivers: the objects of a video): when there are at least as many groups as chunks every cut falls between two groups and no
    piece is empty; with fewer groups than chunks the pieces hold equal numbers of samples and groups are split."""
    n = len(groups)
    edges = [0] + [i for i in range(1, n) if groups[i] != groups[i - 1]] + [n]      # where a cut splits no group
    if chunks < 1 or len(edges) - 1 < chunks:
        return [n * c // max(chunks, 1) for c in range(max(chunks, 1) + 1)]
    acc = [0.0]
    for i in range(n):
        acc.append(acc[-1] + (costs[i] if costs is not None else 1.0))
    bounds, lo = [0], 0                                   # lo: index into edges of the last cut
    for c in range(1, chunks):
        want = acc[-1] * c / chunks
        # the edge nearest to the ideal cut (ties: the earlier one) that leaves a group for this piece and one for every later piece
        e = min(range(lo + 1, len(edges) - (chunks - c)), key=lambda j: (abs(acc[edges[j]] - want), j))
        bounds.append(edges[e])
        lo = e
    return bounds + [n]


def gather_rows(rows: np.ndarray, width: int, device=None) -> np.ndarray:
    """All ranks contribute a [n_r, width] float32 array (n_r may differ); every rank gets the
    concatenation ordered by the rows' first column (sample id), so the result does not depend on which
    rank processed which sample."""
    rows = np.asarray(rows, np.float32).reshape(-1, width)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return rows[np.argsort(rows[:, 0], kind="stable")]
    world = dist.get_world_size()
    dev = device if device is not None else (torch.device("cuda", torch.cuda.current_device())
                                             if dist.get_backend() == "nccl" else torch.device("cpu"))
    n = torch.tensor([rows.shape[0]], dtype=torch.int64, device=dev)
    counts = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(counts, n)
    nmax = int(max(int(c.item()) for c in counts))
    buf = torch.full((max(nmax, 1), width), float("nan"), dtype=torch.float32, device=dev)
    if rows.shape[0]:
        buf[: rows.shape[0]] = torch.from_numpy(rows).to(dev)
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf)
    out = np.concatenate([p[: int(c.item())].cpu().numpy() for p, c in zip(parts, counts)], 0)
    return out[np.argsort(out[:, 0], kind="stable")]
