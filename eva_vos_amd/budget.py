"""Budgeted dataset annotation: the video ranking of the paper (Eq. 3, ``ranking.rank_curve``) applied WHILE the sessions run.

``eval_driver.run`` takes every video through all its rounds and the ranking is drawn afterwards - it then shows that a budget of
annotator hours, or a quality line, is reached after a fraction of them.  ``run_ranked`` keeps every video's session suspended between its
rounds (``sessions.annotation_rounds``), scores the videos from ONE look-ahead round each, commits the best one, runs that video's next
look-ahead, and stops where the budget or the target says: the rounds the ranking would never have reached are not run.  A look-ahead round
is GPU work, not annotation time: it enters the hours only when the ranking commits it.  Every round that does run is the round
``eval_driver.run`` runs - same engine, same calls, same session generator - so the committed rows are its rows, byte for byte."""
from __future__ import annotations

import contextlib
import functools
import threading
import time
from types import SimpleNamespace

import numpy as np
import torch

from . import ranking
from .eval_driver import ARGUMENTS, POLICY_TABLE, _check_l2_clip, make_annotator, result_rows, write_rows_csv
from .fq_driver import ClipDataset, add_stats, lane_engine_options, run_lanes
from .working_size import ScaledInferenceCore, check_working_size


def free_device_bytes(device) -> "int | None":
    """Free device memory as the driver reports it (``torch.cuda.mem_get_info``); None where there is no device to ask."""
    if torch.cuda.is_available() and str(device).startswith("cuda"):
        return int(torch.cuda.mem_get_info()[0])
    return None


def uses_values(policy: str) -> bool:
    """Which rule ranks a policy's videos, as the reference's ``read_exp`` chooses: the agent's values for ``eva_vos``, the gain otherwise."""
    return policy == "eva_vos"


class _Residency:
    """The residency rule of a ranked run: all N sessions stay alive, nothing is evicted or re-encoded.  The FOOTPRINT of an engine is the
    drop in free device memory across the first engine's creation and its first two rounds; before any later engine is created there must be
    room for one footprint plus a reserve of one more - and one more for every engine that is created but not yet through its two rounds."""

    def __init__(self, device, n_videos: int):
        self.device, self.n, self.lock = device, n_videos, threading.Lock()
        self.footprint, self.created, self.in_flight = None, 0, 0
        self.before = free_device_bytes(device)

    def admit(self):
        """Called (under the lock) before engine ``created`` is asked for; raises where it does not fit."""
        free = free_device_bytes(self.device)
        if self.created and free is not None and self.footprint is not None and free < self.footprint * (2 + self.in_flight):
            raise ValueError(f"ranked run: {self.created} of the {self.n} videos fit the device ({free / 2 ** 30:.2f} GiB free, an engine with its first two "
                             f"rounds took {self.footprint / 2 ** 30:.2f} GiB, one more is kept in reserve); every session stays resident, so use a smaller "
                             "--working-size or a smaller imset")
        self.created += 1
        self.in_flight += 1

    def settled(self):
        """An engine is through its first two rounds; the first one's sets the footprint."""
        with self.lock:
            self.in_flight -= 1
            if self.footprint is None:
                free = free_device_bytes(self.device)
                self.footprint = max(self.before - free, 0) if free is not None else 0


class _Video:
    """One video's suspended session and what the ranking knows of it: the rows of the rounds run so far (float32, as ``eval_driver.run``
    returns them) and the record ``ranking.video_score`` reads, made FROM those rows - the live scores see the values the rows hold."""

    def __init__(self, i, sample, stepped, rows_of, stream=None):
        self.i, self.sample, self.stepped, self.rows_of, self.stream = i, sample, stepped, rows_of, stream
        self.executed, self.more, self.rows, self.rec = 0, True, [], None

    def step(self, spec) -> bool:
        """Run the next round, if there is one, and read the session's rows again - on the HIP stream the session was opened on (``stream``;
        None: the current one), so that all its rounds run on one stream, as they do in ``eval_driver.run``."""
        with torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext():
            ran = self.more and self.stepped.step()
            if ran:
                self.executed += 1
                new = self.rows_of(self.stepped.result(), self.i, self.sample, first_round=len(self.rows))
                self.rows += new
                self.rec = ranking.append_rows(self.rec or dict(video=self.i, mu_metrics=[], annotation_times=[], annotated_frames=[], round_metrics=[]), new, spec)
            self.more = bool(ran) and self.stepped.more()
        return bool(ran)


def ranked_loop(videos, use_values: bool, gamma: float = 0.6, budget_hours=None, target_metric=None, spec=None):
    """The loop of a ranked run over ``videos`` (objects with ``step(spec)``, ``executed``, ``more``, ``rec``), each through its first round and
    one look-ahead round already.  Score every video from its look-ahead, commit the best (``ranking.next_video``), run that video's next
    look-ahead; stop BEFORE the commit that would pass ``budget_hours``, AT the first point >= ``target_metric`` (the first point included),
    or when no video can advance - where ``rank_curve`` stops.  A video can advance while its look-ahead round exists and is not its last.
    Returns (hours, points, order, pointers)."""
    pointers = [0] * len(videos)
    recs = [v.rec for v in videos]
    points = [ranking.curve_point(recs, pointers)]
    times = [np.sum([rec["annotation_times"][0] for rec in recs])]
    order = []
    while target_metric is None or not points[-1] >= target_metric:
        can = [v.executed >= p + 2 and v.more for v, p in zip(videos, pointers)]
        scores = [ranking.video_score(v.rec, p, gamma, use_values, more=ok) for v, p, ok in zip(videos, pointers, can)]
        i = ranking.next_video(scores, can)
        if i is None:
            break
        t = times[-1] + videos[i].rec["annotation_times"][pointers[i] + 1]
        if budget_hours is not None and np.float64(t) / 3600 > budget_hours:
            break
        pointers[i] += 1
        order.append((i, pointers[i]))
        recs = [v.rec for v in videos]
        points.append(ranking.curve_point(recs, pointers))
        times.append(t)
        if target_metric is not None and points[-1] >= target_metric:
            break
        videos[i].step(spec)
    return np.array(times, np.float64) / 3600, np.array(points, np.float64), order, pointers


def open_videos(root: str, imset: str, prop_net, fuse_net, policy: str, rounds: int, metric: str = "j_and_f", qnet=None, seed: int = 0,
                device: str = "cuda", lanes: int = 2, annotator=None, annotation_types=None, agent=None, working_size=None):
    """The SET-UP of a ranked run: every sample of the imset with its own engine and suspended session, through round 0 and one look-ahead
    round, under the residency rule.  Returns a namespace: ``videos`` (in sample order), ``spec``, ``action_names``, ``names`` (sample id ->
    name), ``footprint`` (bytes)."""
    from mivos.inference_core import InferenceCore
    core_class = InferenceCore if check_working_size(working_size) is None else functools.partial(ScaledInferenceCore, working_size=working_size)
    spec = POLICY_TABLE[policy]
    given = dict(qnet=qnet, agent=agent, annotator=annotator, annotation_types=annotation_types)
    for name in spec.needs:
        if given[name] is None:
            raise ValueError(f"{policy} needs {name}=...: {ARGUMENTS[name]}")
    action_names = spec.action_names(annotation_types) if spec.action_names else None
    ds = ClipDataset(root, imset)
    t_max = max(s[2] for s in ds.samples)
    _check_l2_clip(policy, t_max, "the longest clip")
    width = 6 + t_max + len(spec.tail)
    n = len(ds.samples)
    on_gpu = torch.cuda.is_available() and str(device).startswith("cuda")
    residency = _Residency(device, n)
    videos = {}
    rows_of = functools.partial(result_rows, multi_object=False, spec=spec, action_names=action_names, width=width)

    def open_video(i, sample):
        with residency.lock:
            residency.admit()
            proc = core_class(prop_net, fuse_net, sample["rgb"], 1, engine_options=lane_engine_options(1))
        lane = SimpleNamespace(annotator=(make_annotator(annotator) if isinstance(annotator, str) else annotator()) if "annotator" in spec.needs else None)
        job = SimpleNamespace(policy=policy, rounds=rounds, metric=metric, qnet=qnet, agent=agent, annotation_types=annotation_types, seed=seed,
                              multi_object=False, share_frames=False, lane=lane, steps=True)
        own = {}
        video = _Video(i, sample, spec.runner(job, proc, sample, i, own), rows_of, torch.cuda.current_stream() if on_gpu else None)
        video.proc, video.stats = proc, own
        video.step(spec)
        video.step(spec)
        if on_gpu:
            torch.cuda.current_stream().synchronize()
        residency.settled()
        videos[i] = video
        return []

    first, rest = [0], list(range(1, n))
    run_lanes(root, imset, first, 1, open_video, device, None, share_frames=False)        # alone: its footprint is the measure for the others
    if rest:
        run_lanes(root, imset, rest, lanes, open_video, device, None, share_frames=False)
    vids = [videos[i] for i in range(n)]
    return SimpleNamespace(videos=vids, spec=spec, action_names=action_names, names=ds.object_names, footprint=residency.footprint or 0)


def run_ranked(root: str, imset: str, out_csv: str, prop_net, fuse_net, policy: str = "oracle_mask", rounds: int = 60, metric: str = "j_and_f",
               qnet=None, seed: int = 0, device: str = "cuda", lanes: int = 2, stats: dict = None, multi_object: bool = False,
               share_frames: bool = True, annotator=None, annotation_types=None, agent=None, working_size=None, budget_hours=None,
               target_metric=None, gamma: float = 0.6, reference_csv: str = None, ranking_csv: str = None):
    """``eval_driver.run`` with the ranking applied live (single rank, per-object mode).  SET-UP: every sample gets its own engine, scorer
    and session generator (for ``eva_vos`` its own ``QNetSelector``; for the policies with an annotator its own annotator) and runs round 0
    and one look-ahead round - ``lanes`` samples in flight, these 2N rounds being independent.  LOOP (``ranked_loop``): one chain, one round
    at a time.  ``budget_hours``: stop before the commit that would pass it; ``target_metric``: stop at the first point >= it; neither:
    until no video can advance.  ``gamma``: the discount of the value rule (``eva_vos``; the other policies rank by gain).
    OUTPUTS, committed rounds only: ``out_csv`` in ``run``'s schema, ``reference_csv`` in the reference's (``ranking.write_reference_csv``),
    ``ranking_csv`` (``step, video, round, hours, metric``); empty / None: not written.  Returns (rows - the committed rounds' rows in the
    order of ``run``'s CSV - , hours, points, order as (sample id, round)).
    ``stats``: ``committed_rounds``, ``lookahead_rounds`` (rounds executed and never committed: at most one per video), ``interactions`` (their
    sum: every round the engines ran), ``propagated_frames``, ``engines_created``, ``engine_footprint_bytes`` (what the residency rule measured),
    ``setup_s`` and ``chain_s`` / ``chain_rounds`` / ``chain_propagated_frames`` (the steady chain).
    RESIDENCY: all N sessions are alive at once and their memory banks grow with the rounds; nothing is evicted or re-encoded (features
    re-encoded in another batch shape are not bit-identical, and the equality with ``run`` rests on them).  Before engine i is created the
    free device memory is read; below one measured engine footprint plus a reserve of one more, ValueError says how many of the N videos fit.
    REFUSED: more than one rank; ``multi_object``; ``upper_bound_mask`` (its trials would multiply the cost of every look-ahead round).
    ``share_frames`` is off in this mode whatever is given: an engine shared by a video's objects could hold one suspended session only."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise ValueError(f"a ranked run is one chain of rounds on one GPU: world_size {dist.get_world_size()} > 1 is refused (run one process)")
    if multi_object:
        raise ValueError("a ranked run ranks the reference's per-object sessions: --multi-object is refused")
    if policy == "upper_bound_mask":
        raise ValueError("upper_bound_mask is refused in a ranked run: its trials would multiply the cost of every look-ahead round")
    t0 = time.perf_counter()
    opened = open_videos(root, imset, prop_net, fuse_net, policy, rounds, metric, qnet, seed, device, lanes, annotator, annotation_types, agent, working_size)
    vids, spec, action_names, n = opened.videos, opened.spec, opened.action_names, len(opened.videos)
    on_gpu = torch.cuda.is_available() and str(device).startswith("cuda")
    t1 = time.perf_counter()
    setup_rounds, setup_frames = sum(v.executed for v in vids), sum(v.stats.get("propagated_frames", 0) for v in vids)
    hours, points, order, pointers = ranked_loop(vids, uses_values(policy), gamma, budget_hours, target_metric, spec)
    if on_gpu:
        torch.cuda.synchronize()
    t2 = time.perf_counter()
    for v in vids:
        v.stepped.close()
    committed = [np.stack(v.rows)[:p + 1] for v, p in zip(vids, pointers)]
    rows = np.concatenate(committed)
    executed = sum(v.executed for v in vids)
    add_stats(stats, dict(committed_rounds=len(rows), lookahead_rounds=executed - len(rows), interactions=sum(v.stats.get("interactions", 0) for v in vids),
                          propagated_frames=sum(v.stats.get("propagated_frames", 0) for v in vids), engines_created=n,
                          key_frames_encoded=sum(int(getattr(v.proc, "key_frames_encoded", 0)) for v in vids),
                          engine_footprint_bytes=opened.footprint, setup_s=t1 - t0, chain_s=t2 - t1, chain_rounds=executed - setup_rounds,
                          chain_propagated_frames=sum(v.stats.get("propagated_frames", 0) for v in vids) - setup_frames))
    names = opened.names
    recs = ranking.read_rows(rows, spec, names)
    if out_csv:
        write_rows_csv(out_csv, rows, spec, names, action_names)
    if reference_csv:
        ranking.write_reference_csv(reference_csv, recs, action_names, spec.seconds)
    if ranking_csv:
        ranking.write_ranking_csv(ranking_csv, recs, hours, points, order)
    return rows, hours, points, [(vids[i].i, r) for i, r in order]


def rank_rows(rows, policy: str, object_names, annotation_types=None, gamma: float = 0.6, reference_csv: str = None, ranking_csv: str = None):
    """``--rank`` after a full run: the reference-schema CSV and ``ranking.csv`` from the gathered rows of ``eval_driver.run``.  Returns
    ``rank_curve``'s (hours, points, order)."""
    spec = POLICY_TABLE[policy]
    action_names = spec.action_names(annotation_types) if spec.action_names else None
    recs = ranking.read_rows(rows, spec, object_names)
    curve = ranking.rank_curve(recs, gamma, uses_values(policy))
    if reference_csv:
        ranking.write_reference_csv(reference_csv, recs, action_names, spec.seconds)
    if ranking_csv:
        ranking.write_ranking_csv(ranking_csv, recs, *curve)
    return curve
