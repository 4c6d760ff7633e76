"""Annotation-policy evaluation on the HIP engine, sharded over the GPUs of one node (BASELINE config 5, mask policies).

Own counterpart of the reference driver ``eval_annotation_method.py:118-190`` for the policies whose annotations are
ground-truth masks - ``oracle_mask``, ``rand_mask``, ``qnet_mask``, ``upper_bound_mask``, ``l2_mask`` (``interactions/mask.py:10-39,
42-71,74-103,196-227,159-193``) - and the frame selectors of ``interactions/policies.py``; every ``run_*`` below builds a scorer and a
``SessionPolicy`` record for the one session loop of ``eva_vos_amd/sessions.py``, POLICY_TABLE says what ``run`` and the command line know
of each policy (its runner, what it needs, its modes, its extra columns), the dataset and lane side is ``fq_driver``'s.  The click / bbox policies
additionally need SAM (``segment_anything``), which north_star leaves on stock PyTorch-ROCm and which is not installed offline; the
mixed-annotation policies (``run_typed_policy``) and ``eva_vos`` itself (``run_eva_vos``: the QNet picks the frame, the actor-critic agent
the annotation type) therefore run over any predictor with the SAM controller's signature, the ``ComponentPredictor`` stand-in included.

Differences by design:

* J / J&F per frame come from the device (``stcn_metrics_jf_counts``) - masks never visit the host per round;
* QNet frame selection keeps features on the device (``eva_vos_amd.qnet``);
* ``l2_mask`` applies the reference's rule (farthest frame, in L2, from every annotated one) to the ``f16`` features the engine has cached
  for the clip, NOT to the reference's ImageNet / DINO extractors: no second network, one distance matrix per video
  (``InferenceCore.frame_distances``), clips of at most 106 frames;
* two samples are in flight per GPU (host thread + HIP stream each, ``--lanes``): +9..17 % rounds/s;
* the per-object sessions of a video share one engine and the frame features it has computed (``fq_driver.LaneCores``; same rows;
  ``--no-share-frames`` switches it off), so videos, not samples, are dealt to ranks and lanes;
* samples are LPT-sharded over ranks instead of ``--min-idx/--max-idx``; ONE gather of fixed-width rows at the end
  (RCCL over xGMI), rank 0 writes the CSV with the reference's columns ``video, mu_metric, annotation_time, round``;
* ``--multi-object`` (an additional mode; the reference's per-object protocol stays the default): ONE session per video with all its
  objects in one engine - the key encoder runs once per frame, not once per frame and object - scored per round by the k-object
  evaluation on the device (``stcn_metrics_objects_round``); rows stay one per (video, object, round) with the per-object sample ids.
* the dataset-level video ranking of the paper (Eq. 3; ``vis/vis_util.py:40-150``) is ``eva_vos_amd/ranking.py``: ``--rank`` writes the
  reference-schema CSV and the ranking beside the experiment CSV after a full run; ``--budget-hours`` / ``--target-metric`` apply it WHILE
  the sessions run (``eva_vos_amd/budget.py``: every video's session is suspended between its rounds, the rounds the ranking never reaches
  are not run).

Usage:  python -m eva_vos_amd.eval_driver --root data/MOSE --imset data/MOSE/ImageSets/test.txt --policy oracle_mask
        (multi-GPU: python -m torch.distributed.run --nproc-per-node N -m eva_vos_amd.eval_driver ...)
"""
from __future__ import annotations

import argparse
import copy
import csv
import functools
import os
import random
import threading
import time
from collections import namedtuple
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable

import numpy as np
import torch

from . import metrics
from .frame_select import farthest_frame
from .fq_driver import ClipDataset, add_stats, gather_sorted, lane_cores, load_networks, rank_samples, report_and_leave, run_lanes
from .sessions import MASK_SECONDS, NO_OBJECT, SKIP_SECONDS, SessionPolicy, SteppedSession, annotation_rounds, frame_quality, session_result
from .working_size import ScaledInferenceCore, check_working_size

ANNOTATORS = ("component",)                                   # built in; a real SAM controller is passed through run(..., annotator=...)
MAX_OBJECTS = 32                                              # STCN_MAX_OBJECTS
KEY_CACHE_FRAMES = 106                                       # the engine's key cache: a clip of at most this many frames never recycles a slot


def _check_l2_clip(policy: str, T: int, what: str):
    """``l2_mask`` reads every frame's features out of the key cache: a longer clip recycles its slots and is refused before any work."""
    if policy == "l2_mask" and T > KEY_CACHE_FRAMES:
        raise ValueError(f"l2_mask: {what} has {T} frames, the policy needs every frame's features in the key cache, which holds at most {KEY_CACHE_FRAMES}")


def _upper_bound_frame(processor, gt, gt_thw, frames, metric, stats=None):
    """get_frame_upper_bound (interactions/policies.py:90-117): try every remaining frame on a deep copy of the
    processor and keep the one with the best mean metric (last maximum wins, as the reference's ``>=``).  The path of clips longer than
    the key cache: their cache recycles, a trial on the session's own engine would change the shapes of its later launches."""
    best, best_f = -np.inf, -1
    for f in range(gt.shape[0]):
        if f in frames:
            continue
        p = copy.deepcopy(processor)
        p.interact(gt[f][None], f, download=False)
        mu, _, _ = frame_quality(p, gt_thw, frames + [f], metric)
        if mu >= best:
            best, best_f = mu, f
        del p
        if stats is not None:
            stats["trial_interactions"] = stats.get("trial_interactions", 0) + 1
            stats["engine_clones"] = stats.get("engine_clones", 0) + 1
    return best_f


def _upper_bound_frame_in_place(processor, scorer, gt, frames, stats=None):
    """The same selection without a second engine, for clips that fit the key cache: every remaining frame is tried ON the session's engine
    - ``interact``, ``RoundScorer.score_trial``, ``undo`` (undo depth 1) - all candidates enqueued back to back; the host waits once, for
    the table of trial rows.  From the second interaction of such a clip on every key is cached, so a trial that is taken back leaves the
    engine's later results byte-identical (include/stcn_hip.h), and a trial row is what ``frame_quality`` returns for the copy, to the bit:
    with the mean over the frames with an object and the ``>=`` below - the expressions of ``_upper_bound_frame`` - the selection is the
    same by construction."""
    candidates = [f for f in range(gt.shape[0]) if f not in frames]
    for row, f in enumerate(candidates):
        processor.interact(gt[f][None], f, download=False)
        scorer.score_trial(processor, frames, f, row)
        processor.undo(download=False)
    q = scorer.trial_rows(len(candidates))
    empty = scorer.empty_host
    best, best_f = -np.inf, -1
    for row, f in enumerate(candidates):
        mu = float(np.mean(q[row][~empty])) if (~empty).any() else float("nan")
        if mu >= best:
            best, best_f = mu, f
    if stats is not None:
        stats["trial_interactions"] = stats.get("trial_interactions", 0) + len(candidates)
    return best_f


def run_policy(policy: str, processor, sample, rounds: int, metric: str = "j_and_f", qnet=None, rng=None, multi_object: bool = False,
               stats: dict = None, steps: bool = False):
    """One sample through ``rounds`` annotation rounds.  Returns dict(mu_metrics, annotation_times, frames,
    round_metrics, propagated_frames): mu_metrics[r] / annotation_times[r] as the reference returns them; frames = annotated frames in
    order; round_metrics[r] = per-frame quality after round r; propagated_frames = frames the engine really visited (rounds >= 2 only
    walk the spans next to the new annotation).
    ``multi_object``: the sample is a per-video one (``ClipDataset(..., per_video=True)``) and the processor holds all its k objects
    (``InferenceCore(..., num_objects=k)``): the annotation of frame f is the (k+1)-channel one-hot of its label map, background first, through
    the reference's ``scribble=True`` path; a round is scored by the k-object evaluation on the device, the values above are those of the FRAME
    quality (the mean over the objects present in the frame; a frame is valid while any object is present in it), and ``object_metrics[r]``
    [k,T] / ``present`` [k,T] are added.
    ``upper_bound_mask`` tries its candidates on the session's own engine and takes them back (``_upper_bound_frame_in_place``) when the clip
    fits the key cache, on deep copies of the engine (``_upper_bound_frame``) when it does not: decided by the clip length alone.
    ``stats`` (optional dict): ``propagated_frames`` and ``interactions`` of the session's own rounds are added to it, and for the upper
    bound ``trial_interactions`` (candidates tried) and ``engine_clones`` (deep copies made).
    ``l2_mask`` chooses ``farthest_frame(processor.frame_distances(), frames)``; a clip longer than the key cache raises ValueError before the
    processor is touched; ``stats["frame_distance_passes"]`` counts the engine passes the session added (0 when the core came with the matrix).
    ``steps=True``: nothing is run; the suspended session comes back (a ``sessions.SteppedSession``: ``step()`` one round, ``result()`` the
    values above as of the rounds run, ``close()`` at the end) - the engines have no state across sessions and the draws are the session's own,
    so a session stepped between other videos' rounds gives the bytes it gives run straight through."""
    assert policy in POLICIES, policy
    if multi_object and policy not in MULTI_OBJECT_POLICIES:
        raise ValueError(f"multi-object sessions support the policies {' and '.join(MULTI_OBJECT_POLICIES)}, not {policy}")
    T = sample["num_frames"]
    _check_l2_clip(policy, T, f"clip {sample.get('name', '?')}")
    dev = processor.prob.device
    rng = rng or random
    stats = {} if stats is None else stats
    # the evaluation of a round stays on the device (metrics.RoundScorer): one int per round crosses PCIe for the oracle policy, the
    # per-frame quality rows of the whole session are fetched once at the end
    scorer_args = dict(metric="j" if metric == "j" else "j_and_f", max_rounds=max(rounds, 1), no_object=NO_OBJECT)
    if multi_object:
        k = int(sample["num_objects"])
        scorer = metrics.RoundScorer(sample["gt"][0, :, 0].to(dev), num_objects=k, **scorer_args)
        channels = torch.arange(k + 1, device=dev, dtype=torch.uint8)[:, None, None, None]
        mask_of, interact_kw = (lambda f: (scorer.gt[f][None, None] == channels).float()), dict(scribble=True)      # [k+1,1,H,W]
    else:
        gt = sample["gt"][0].to(dev)                               # [T,1,H,W]
        gt_thw = gt[:, 0]
        images = sample["rgb"][0].to(dev) if policy == "qnet_mask" else None
        scorer = metrics.RoundScorer(gt_thw, **scorer_args)
        mask_of, interact_kw = (lambda f: gt[f][None]), {}
    in_place = policy == "upper_bound_mask" and T <= KEY_CACHE_FRAMES

    def choose(worst, types, gen, frames):
        if policy == "oracle_mask":
            return worst
        if policy == "rand_mask":
            return rng.choice(sorted(set(range(T)) - set(frames)))
        if policy == "qnet_mask":
            from .qnet import qnet_frame_selection
            return qnet_frame_selection(qnet, images, gen.float(), frames)
        if policy == "l2_mask":
            return farthest_frame(processor.frame_distances(), frames)
        if in_place:
            return _upper_bound_frame_in_place(processor, scorer, gt, frames, stats)
        return _upper_bound_frame(processor, gt, gt_thw, frames, metric, stats)

    session = SessionPolicy(mask_of, choose, keep_gen=policy == "qnet_mask", interact_kw=interact_kw)
    if policy == "upper_bound_mask":
        stats.setdefault("trial_interactions", 0), stats.setdefault("engine_clones", 0)
    depth = processor.undo_state()["depth"] if in_place else 0
    if in_place:
        processor.set_undo_depth(max(depth, 1))
    passes = processor.frame_distance_passes if policy == "l2_mask" else 0

    def close():
        if in_place:
            processor.set_undo_depth(depth)                        # the core goes back to its lane as it came
        if policy == "l2_mask":
            stats["frame_distance_passes"] = stats.get("frame_distance_passes", 0) + processor.frame_distance_passes - passes

    def result(ses):
        res = dict(session_result(scorer, ses), frames=ses["chosen"])
        if multi_object:
            oq = scorer.object_qualities()
            res.update(object_metrics=[oq[i].copy() for i in range(len(ses["costs"]))], present=scorer.present_host)
        return res

    stepped = SteppedSession(annotation_rounds(processor, scorer, T, rounds, session, stats), result, close)
    return stepped if steps else stepped.run()


def oracle_action(annotator, annotation_types, gt_mask, mivos_mask, im, frame_annots, empty=None):
    """oracle_action (interactions/mulitple_annotations.py:42-85): every annotation type is tried on the frame and the one with the best
    reward = (iou - init_iou) / cost is taken; ``>=`` keeps the LAST best, and a box is skipped where one was given before.  Returns
    (mask, cost, action, logits, clicks, labels, bbox, actions_data)."""
    best = (None, 1e10, None, None, None, None, None)
    best_reward = -1e10
    init_iou = annotator.iou(mivos_mask, gt_mask)
    data = {"init_iou": init_iou}
    for ann_type in annotation_types:
        if ann_type == "bbox" and "bbox" in frame_annots["annotations"]:
            continue
        mask, cost, iou, logits, clicks, labels, bbox = annotator.annotate(ann_type, gt_mask, im, mivos_mask, frame_annots, empty=empty)
        reward = (iou - init_iou) / cost
        data[ann_type] = dict(iou=iou, cost=cost, reward=reward)
        if reward >= best_reward:
            best_reward, best = reward, (mask, cost, ann_type, logits, clicks, labels, bbox)
    data["selected_action"] = best[2]
    return best + (data,)


def _one_object_session(policy: str, processor, sample, rounds: int, metric: str, scorer):
    """What the one-object sessions with other annotations than masks start from: (T, gt [T,1,H,W] and the clip [T,3,H,W] on the engine's
    device, the scorer - a metrics.TypedRoundScorer unless the caller brought one).  A per-video sample is refused."""
    if "object_ids" in sample:                                      # ClipDataset(..., per_video=True)
        raise ValueError(f"{policy} is a one-object policy: multi-object sessions support {' and '.join(MULTI_OBJECT_POLICIES)}")
    dev = processor.prob.device
    gt = sample["gt"][0].to(dev)
    if scorer is None:
        scorer = metrics.TypedRoundScorer(gt[:, 0], "j" if metric == "j" else "j_and_f", max_rounds=max(rounds, 1), no_object=NO_OBJECT)
    return sample["num_frames"], gt, sample["rgb"][0].to(dev), scorer


def run_typed_policy(policy: str, processor, sample, rounds: int, annotator, annotation_types, metric: str = "j_and_f", rng=None,
                     stats: dict = None, scorer=None, choose_action=None, steps: bool = False):
    """One sample through ``rounds`` rounds of a mixed-annotation policy (``rand_type``, ``rand_rand``, ``oracle_oracle``:
    interactions/mulitple_annotations.py:161-220, 223-283, 104-158).  ``annotator``: an ``annotate.PromptAnnotator``; ``annotation_types``:
    'click', 'bbox', 'mask' or '<N>clicks' - exactly one for ``rand_type``, more than one for the others.  The first round is the mask of frame
    0 at 80 s; later rounds annotate the chosen frame with the policy's action - ``rand_type``: its one type, ``rand_rand``: a random one,
    ``oracle_oracle``: ``oracle_action`` - and choose the next frame: the arg-min of the round's quality for ``oracle_oracle``, a random frame
    among those not yet annotated with a mask for the others.  Every draw comes from ``rng`` (the session's own ``random.Random``), so runs are
    not comparable draw for draw with the reference's global NumPy / ``random`` state.  ``choose_action(frame, gen, frame_annots)`` replaces
    the policy's action (the hook an ``eva_vos`` agent needs); ``scorer``: another evaluation with ``TypedRoundScorer``'s interface
    (``metrics.HostTypedScorer``).  Returns the reference's values - ``mu_metrics``, ``annotation_times``, ``annotations_actions``, and
    ``round_metrics`` / ``annotated_frames`` (the reference returns these two for ``oracle_oracle`` only) - plus ``types`` and
    ``propagated_frames``.  ``steps=True``: the suspended session instead (see ``run_policy``)."""
    from .annotate import check_annotation_types
    assert policy in TYPED_POLICIES, policy
    types_ = check_annotation_types(annotation_types)
    if policy == "rand_type" and len(types_) != 1:
        raise ValueError(f"rand_type takes one annotation type, got {types_}")
    if policy != "rand_type" and len(types_) < 2:
        raise ValueError(f"{policy} requires more than one annotation type, got {types_}")
    T, gt, images, scorer = _one_object_session(policy, processor, sample, rounds, metric, scorer)
    rng = rng or random
    empty = scorer.empty_host
    action_data = []

    def policy_action(frame, gen, frame_annots):
        g, mivos = gt[frame, 0], gen[frame][None].to(torch.bool)
        if policy == "oracle_oracle":
            out = oracle_action(annotator, types_, g, mivos, images[frame], frame_annots, empty=bool(empty[frame]))
            action_data.append(dict(out[-1], frame_num=frame))
            return out[:-1]
        action = types_[0] if policy == "rand_type" else rng.choice(types_)
        mask, cost, _, logits, clicks, labels, bbox = annotator.annotate(action, g, images[frame], mivos, frame_annots, empty=bool(empty[frame]))
        return mask, cost, action, logits, clicks, labels, bbox

    def choose_frame(worst, types, gen, frames):
        if policy == "oracle_oracle":
            return worst
        left = np.where(types != 1)[0]
        return int(rng.choice(left.tolist())) if len(left) else None

    session = SessionPolicy(lambda f: gt[f][None], choose_frame, action=choose_action or policy_action, stop_at_T=False)
    stepped = SteppedSession(annotation_rounds(processor, scorer, T, rounds, session, {} if stats is None else stats),
                             lambda ses: dict(session_result(scorer, ses), annotations_actions=ses["actions"], annotated_frames=ses["frames"],
                                              frames=ses["frames"], types=ses["types"], action_data=action_data))
    return stepped if steps else stepped.run()


def run_eva_vos(processor, sample, rounds: int, annotator, qnet, agent, metric: str = "j_and_f", rng=None, stats: dict = None, scorer=None,
                selector=None, steps: bool = False):
    """One sample through ``rounds`` rounds of ``eva_vos`` (interactions/mulitple_annotations.py:307-378): the first round is the mask of frame
    0 at 80 s; every later round the AGENT chooses how the pending frame is annotated (``rl_agent_annotate``, :286-304) and the QNET which
    frame comes next (:356-369).  ``annotator``: an ``annotate.PromptAnnotator`` whose predictor gives an image embedding; ``qnet``: a
    ``QualityNet`` in eval mode; ``agent``: an ``agent.PPOAgent``; ``rng``: the session's ``torch.Generator`` the agent's draws come from (None:
    torch's global one) - runs are reproducible under it and, as for the other typed policies, not comparable draw for draw with the reference.
    ``selector``: the video's ``qnet.QNetSelector`` when the caller keeps one (the sessions of a video's objects), else one is made from
    ``sample['rgb']``; its ``masks_to_input`` (``agent.masks_to_224`` by default) also builds the agent's mask input; ``scorer``: another evaluation with ``TypedRoundScorer``'s interface (``metrics.HostTypedScorer``).
    The annotation types are the reference's hard-coded ``['3clicks', 'mask'][action]``, plus 'no_object' (3 s, value 0, no agent call) on a frame
    without the object.  Returns the reference's values - ``mu_metrics``, ``annotation_times``, ``rl_values`` (the first entry is -2, :316),
    ``annotations_actions``, ``round_metrics``, ``annotated_frames`` - plus ``frames``, ``types`` and ``propagated_frames``.  ``steps=True``: the suspended session instead (see ``run_policy``)."""
    from .agent import AVAIL_ACTIONS, masks_to_224
    from .annotate import ANNOTATION_COSTS
    T, gt, images, scorer = _one_object_session("eva_vos", processor, sample, rounds, metric, scorer)
    if selector is None:
        from .qnet import QNetSelector
        selector = QNetSelector(qnet, images)
    empty = scorer.empty_host
    rl_values = [-2]
    to_input = getattr(selector, "masks_to_input", masks_to_224)     # the selector's route from masks to network input serves the agent too

    def choose_action(frame, gen, frame_annots):
        g = gt[frame, 0]
        if empty[frame]:                                            # frame_annots['metric'] == 20 (:290-291): nothing to ask the agent
            rl_values.append(0)
            return g, ANNOTATION_COSTS["no_object"], "no_object", None, None, None, None
        embedding = annotator.image_embedding(images[frame], g)
        action, value = agent.act(embedding, to_input(gen, [frame]), generator=rng)
        ann_type = AVAIL_ACTIONS[action]
        mask, cost, _, logits, clicks, labels, bbox = annotator.annotate(ann_type, g, images[frame], gen[frame][None].to(torch.bool), frame_annots, empty=False)
        rl_values.append(float(value.squeeze().item()))
        return mask, cost, ann_type, logits, clicks, labels, bbox

    def select(worst, types, gen, frames):
        if len(frames) < T:                                         # round r = len(frames): r < T
            return selector.select(gen, frames)
        # from r >= T on the reference hands the frames NOT yet annotated with a mask to qnet_frame_selection as its "interacted" set
        # (:361-367) - the selection is then the frame farthest from those, which may well be one that has its mask.  Kept as it is.
        left = np.where(types != 1)[0]
        return selector.select(gen, left.tolist()) if len(left) else None

    session = SessionPolicy(lambda f: gt[f][None], select, action=choose_action, stop_at_T=False)
    stepped = SteppedSession(annotation_rounds(processor, scorer, T, rounds, session, {} if stats is None else stats),
                             lambda ses: dict(session_result(scorer, ses), rl_values=rl_values, annotations_actions=ses["actions"],
                                              annotated_frames=ses["frames"], frames=ses["frames"], types=ses["types"]))
    return stepped if steps else stepped.run()


def make_annotator(name: str):
    """The built-in annotators of the command line: 'component' = ``PromptAnnotator`` over the ``ComponentPredictor`` stand-in."""
    from .annotate import ComponentPredictor, PromptAnnotator
    if name != "component":
        raise ValueError(f"unknown annotator {name!r}: built in are {', '.join(ANNOTATORS)}; pass a PromptAnnotator over a SAM controller to run()")
    return PromptAnnotator(ComponentPredictor())


# ------------------------------------------------------------------------------------------------ the policy table
# a row column beyond the common ones: its CSV name, fill(res, r, action_names) - the float a row keeps for round r of a session's result -
# and cell(value, action_names) - what the CSV shows for it
Column = namedtuple("Column", "name fill cell")
ACTIONS = Column("annotation_actions", lambda res, r, names: names.index(res["annotations_actions"][r]), lambda v, names: names[int(v)])
VALUES = Column("rl_values", lambda res, r, names: res["rl_values"][r], lambda v, names: float(v))
# what run() may have to be given, as the error message names it
ARGUMENTS = {"qnet": "a QualityNet in eval mode", "agent": "an agent.PPOAgent", "annotator": "'component' or a factory of PromptAnnotator objects",
             "annotation_types": "'click', 'bbox', 'mask' or '<N>clicks': one type for rand_type, several for the others"}


@dataclass(frozen=True)
class PolicySpec:
    """All that run() and main() know of a policy.  ``runner(job, proc, sample, i, session_stats)``: sample i through its session (``job``: the
    arguments of run(), ``lane``, what the lane thread keeps between its sessions: its annotator, eva_vos's selector, and ``steps``, whether
    the suspended session is wanted instead of its result); ``needs``: the keys of ARGUMENTS the policy cannot run without; ``multi_object``:
    it has a multi-object mode; ``tail``: its extra columns in CSV order, kept at the END of a row, column j at ``row[-1 - j]``;
    ``action_names(annotation_types)``: the names an ACTIONS column indexes; ``seconds``: how the CSV prints ``annotation_time`` - the mask
    policies cost whole seconds, click costs are fractions of one."""
    runner: Callable
    needs: tuple = ()
    multi_object: bool = False
    tail: tuple = ()
    action_names: Callable = None
    seconds: type = int


def _run_mask(job, proc, sample, i, session):
    return run_policy(job.policy, proc, sample, job.rounds, job.metric, job.qnet, random.Random(job.seed * 100003 + i), multi_object=job.multi_object,
                      stats=session, steps=job.steps)


def _run_typed(job, proc, sample, i, session):
    return run_typed_policy(job.policy, proc, sample, job.rounds, job.lane.annotator, job.annotation_types, job.metric,
                            random.Random(job.seed * 100003 + i), stats=session, steps=job.steps)


def _run_agent(job, proc, sample, i, session):
    lane, selector = job.lane, None
    if job.share_frames:                                            # the sessions of a video's objects: one clip, one pass of the QNet's frame branch
        if getattr(lane, "video", None) != sample["video"]:
            from .qnet import QNetSelector
            lane.video, lane.selector = sample["video"], QNetSelector(job.qnet, sample["rgb"][0])
        selector = lane.selector
    return run_eva_vos(proc, sample, job.rounds, lane.annotator, job.qnet, job.agent, job.metric, torch.Generator().manual_seed(job.seed * 100003 + i),
                       stats=session, selector=selector, steps=job.steps)


def _typed_action_names(annotation_types):
    from .annotate import check_annotation_types
    return sorted(set(check_annotation_types(annotation_types or ())) | {"mask"})


# the mixed-annotation policies (interactions/mulitple_annotations.py:104-283): run_typed_policy, with an annotator; one-object sessions
_TYPED = PolicySpec(_run_typed, needs=("annotator", "annotation_types"), tail=(ACTIONS,), action_names=_typed_action_names, seconds=float)
POLICY_TABLE = {
    # QNet takes one binary mask; the upper bound builds on the one-object scorer; the l2 selector needs no mask at all
    "oracle_mask": PolicySpec(_run_mask, multi_object=True),
    "rand_mask": PolicySpec(_run_mask, multi_object=True),
    "qnet_mask": PolicySpec(_run_mask, needs=("qnet",)),
    "upper_bound_mask": PolicySpec(_run_mask),
    "l2_mask": PolicySpec(_run_mask, multi_object=True),
    "rand_type": _TYPED,
    "rand_rand": _TYPED,
    "oracle_oracle": _TYPED,
    # eva_vos (interactions/mulitple_annotations.py:286-378): run_eva_vos, with an annotator, the QNet and the agent; one-object sessions
    "eva_vos": PolicySpec(_run_agent, needs=("qnet", "agent", "annotator"), tail=(VALUES, ACTIONS), seconds=float,
                          action_names=lambda annotation_types: sorted({"3clicks", "mask", "no_object"})),
}
POLICIES, TYPED_POLICIES, AGENT_POLICIES = (tuple(n for n, p in POLICY_TABLE.items() if p.runner is runner) for runner in (_run_mask, _run_typed, _run_agent))
MULTI_OBJECT_POLICIES = tuple(n for n, p in POLICY_TABLE.items() if p.multi_object)


def _session_rows(res: dict, i: int, sample, multi_object: bool):
    """(sample id, round, mu_metric, seconds, annotated frame, per-frame values) of every row a session's result gives: one per round, and in
    multi-object mode one per object and round, with the object's id in the per-object enumeration."""
    if not multi_object:
        for r, (mu, sec, q) in enumerate(zip(res["mu_metrics"], res["annotation_times"], res["round_metrics"])):
            yield i, r, mu, sec, res["frames"][r], q
        return
    for o, sid in enumerate(sample["object_ids"]):
        here = res["present"][o]
        for r, oq in enumerate(res["object_metrics"]):
            f = res["frames"][r]
            yield sid, r, float(np.mean(oq[o][here])) if here.any() else float("nan"), MASK_SECONDS if here[f] else SKIP_SECONDS, f, oq[o]


def result_rows(res: dict, i: int, sample, multi_object: bool, spec: "PolicySpec", action_names, width: int, first_round: int = 0) -> list:
    """The float32 rows of one session's result, as ``run`` returns them: the common columns, the per-frame values, NaN padding up to
    ``width``, the policy's tail columns at the end.  ``first_round``: only the rows of that round and later ones."""
    rows = []
    for sid, r, mu, sec, f, q in _session_rows(res, i, sample, multi_object):
        if r < first_round:
            continue
        row = np.full(width, np.nan, np.float32)
        row[:6] = (sid, r, mu, sec, f, len(q))
        row[6:6 + len(q)] = q
        for j, col in enumerate(spec.tail):
            row[-1 - j] = col.fill(res, r, action_names)
        rows.append(row)
    return rows


def write_rows_csv(out_csv: str, ordered, spec: "PolicySpec", object_names, action_names) -> None:
    """The experiment CSV of ``run``: ``video, mu_metric, annotation_time, round`` and the policy's tail columns, one line per row."""
    os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
    with open(out_csv, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["video", "mu_metric", "annotation_time", "round"] + [col.name for col in spec.tail])
        for row in ordered:
            wr.writerow([object_names[int(row[0])], float(row[2]), spec.seconds(row[3]), int(row[1])]
                        + [col.cell(row[-1 - j], action_names) for j, col in enumerate(spec.tail)])


def run(root: str, imset: str, out_csv: str, prop_net, fuse_net, policy: str = "oracle_mask", rounds: int = 60,
        metric: str = "j_and_f", qnet=None, seed: int = 0, device: str = "cuda", lanes: int = 2, stats: dict = None,
        multi_object: bool = False, share_frames: bool = True, annotator=None, annotation_types=None, agent=None, working_size=None):
    """Process this rank's share of the samples (`lanes` videos in flight); returns the gathered rows on every rank
    (rows: sample id, round, mu_metric, annotation_time, annotated frame, T, then T per-frame values, NaN-padded).
    `stats` (optional dict): this rank's `propagated_frames` (frames the engines visited), `interactions`, `key_frames_encoded` (frames that
    went through the key encoder) and `engines_created` are added to it, for `upper_bound_mask` also `trial_interactions` and `engine_clones`,
    for `l2_mask` also `frame_distance_passes` (one per video when its sessions share an engine).
    `share_frames` (per-object mode; the protocol and the rows stay the reference's): the sessions of a video's objects run one after the
    other on ONE engine that keeps the clip and its frame features between them (fq_driver.LaneCores) - videos, not samples, are dealt to
    ranks and lanes.  False: a fresh engine and a fresh upload per sample, samples dealt one by one.
    A policy of TYPED_POLICIES runs ``run_typed_policy`` with ``annotation_types`` and ``annotator`` - a factory of one ``PromptAnnotator`` per
    lane thread (e.g. ``lambda: PromptAnnotator(sam_controller)``), or the name of a built-in ('component'); per-object mode only.  Its rows
    carry one more column at the end: the index of the round's action in ``sorted(set(annotation_types) | {'mask'})``, which the CSV names
    in an ``annotation_actions`` column beside the reference's (eval_annotation_method.py:138-139,185-186).
    ``eva_vos`` (AGENT_POLICIES) runs ``run_eva_vos`` with ``qnet`` (eval mode), ``agent`` (an ``agent.PPOAgent``) - both shared by the lanes - and
    ``annotator`` as above; each session draws from its own ``torch.Generator`` seeded ``seed * 100003 + sample``, the sessions of a video's
    objects share one ``QNetSelector`` when they share an engine; per-object mode only.  Its rows carry two more columns: the action's index in
    ``sorted({'3clicks', 'mask', 'no_object'})`` and, last, the agent's value (``rl_values``, -2 for the first round); CSV columns
    ``video, mu_metric, annotation_time, round, rl_values, annotation_actions``.
    `multi_object`: one session per VIDEO with all its objects in one engine.  The rows keep their schema and the sample ids of the per-object
    enumeration, one per (video, object, round), so the outputs of the two modes join on (sample id, round): mu_metric = the mean of that
    object's quality over the frames where it is present, annotation_time = 80 s if the object is present in the annotated frame, else
    3 s, the annotated frame is the session's, the per-frame values are that object's.
    `working_size` (an int; None: the clip's own size, as before): the engines propagate on the clip brought down to that shorter side and
    the masks every round is scored on come back at the clip's own size (working_size.ScaledInferenceCore takes InferenceCore's place)."""
    from mivos.inference_core import InferenceCore
    core_class = InferenceCore if check_working_size(working_size) is None else functools.partial(ScaledInferenceCore, working_size=working_size)
    spec = POLICY_TABLE[policy]
    if multi_object and not spec.multi_object:
        raise ValueError(f"multi-object sessions support the policies {' and '.join(MULTI_OBJECT_POLICIES)}, not {policy}")
    given = dict(qnet=qnet, agent=agent, annotator=annotator, annotation_types=annotation_types)
    for name in spec.needs:
        if given[name] is None:
            raise ValueError(f"{policy} needs {name}=...: {ARGUMENTS[name]}")
    action_names = spec.action_names(annotation_types) if spec.action_names else None
    ds = ClipDataset(root, imset, per_video=multi_object)
    for v, k, _ in ds.samples if multi_object else ():
        if k > MAX_OBJECTS:
            raise ValueError(f"video {v} has {k} objects: a multi-object session holds at most {MAX_OBJECTS}")
    t_max = max(s[2] for s in ds.samples)
    _check_l2_clip(policy, t_max, "the longest clip")
    share_frames = share_frames and not multi_object
    rank, mine = rank_samples(ds, share_frames, multi_object)
    cores = lane_cores(core_class, prop_net, fuse_net, lanes, share_frames, multi_object)
    width = 6 + t_max + len(spec.tail)
    job = SimpleNamespace(policy=policy, rounds=rounds, metric=metric, qnet=qnet, agent=agent, annotation_types=annotation_types, seed=seed,
                          multi_object=multi_object, share_frames=share_frames, lane=threading.local(), steps=False)

    def work(i, sample):
        t_c = time.perf_counter()
        proc = cores.core_for(sample)
        t_s = time.perf_counter()
        session = {}
        if "annotator" in spec.needs and not hasattr(job.lane, "annotator"):         # one per lane thread
            job.lane.annotator = make_annotator(annotator) if isinstance(annotator, str) else annotator()
        res = spec.runner(job, proc, sample, i, session)
        cores.done(proc)
        add_stats(stats, dict({n: session[n] for n in ("trial_interactions", "engine_clones", "frame_distance_passes") if n in session},
                              create_s=t_s - t_c, session_s=time.perf_counter() - t_s, propagated_frames=res["propagated_frames"],
                              interactions=len(res["mu_metrics"])))
        return result_rows(res, i, sample, multi_object, spec, action_names, width)

    def lane_done():
        cores.release()
        job.lane.video = job.lane.selector = None

    rows = run_lanes(root, imset, mine, lanes, work, device, stats, per_video=multi_object, share_frames=share_frames, lane_done=lane_done)
    cores.add_to(stats)
    allrows, ordered = gather_sorted(rows, width)
    if rank == 0 and out_csv:
        write_rows_csv(out_csv, ordered, spec, ds.object_names, action_names)
    return allrows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--imset", required=True)
    ap.add_argument("--policy", default="oracle_mask", choices=tuple(POLICY_TABLE))
    ap.add_argument("--annotation-types", nargs="+", default=None, metavar="TYPE", help="the mixed-annotation policies (" + ", ".join(TYPED_POLICIES)
                    + "): 'click', 'bbox', 'mask' or '<N>clicks'; one type for rand_type, several for the others")
    ap.add_argument("--annotator", default="component", choices=ANNOTATORS, help="the segmenter behind clicks and boxes: 'component' is a deterministic "
                    "stand-in that knows the ground truth (NOT a segmenter); a real SAM controller is passed to eval_driver.run(annotator=...)")
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--lanes", type=int, default=2, help="videos in flight per GPU")
    ap.add_argument("--multi-object", action="store_true", help="one session per video with all its objects in one engine (policies: "
                    + ", ".join(MULTI_OBJECT_POLICIES) + "); default: one session per (video, object), the reference's protocol")
    ap.add_argument("--no-share-frames", action="store_true", help="per-object mode: a fresh engine and a fresh upload of the clip for every object "
                    "of a video (default: the sessions of a video's objects share one engine and its frame features; same output)")
    ap.add_argument("--db", default="MOSE")
    ap.add_argument("--prop-weights", default="./model_weights/mivos/stcn.pth")
    ap.add_argument("--fusion-weights", default="./model_weights/mivos/fusion.pth")
    ap.add_argument("--qnet-weights", default="./model_weights/qnet/qnet.pth")
    ap.add_argument("--agent-weights", default="./model_weights/rl_agent/model.pth", help="eva_vos: the actor-critic agent's checkpoint")
    ap.add_argument("--synthetic-weights", action="store_true", help="use the deterministic recipe (no checkpoints)")
    ap.add_argument("--top-k", type=int, default=50, help="rows of the memory bank each query reads, 1..50 (PropagationNetwork(top_k=...): 20 for STCN checkpoints, 50 for MiVOS)")
    ap.add_argument("--km", type=float, default=None, metavar="SIGMA", help="kernelized memory read: standard deviation (1/16-scale positions) of the Gaussian "
                    "around each memory row's best query (prop_model.memory.km of the reference, e.g. 5.6); default: the plain read")
    ap.add_argument("--working-size", type=int, default=None, metavar="N", help="propagate on the clip resized so that its shorter side is N (antialiased bicubic, "
                    "e.g. 480; clips that are no larger keep their size) and score the masks brought back to the clip's own size; default: the clip's own size")
    ap.add_argument("--budget-hours", type=float, default=None, metavar="H", help="rank the videos while they run (budget.run_ranked) and stop before the "
                    "annotation that would pass H annotator hours over the whole imset; one process, per-object sessions, every session resident")
    ap.add_argument("--target-metric", type=float, default=None, metavar="M", help="the same live ranking, stopped at the first curve point >= M (e.g. 0.85)")
    ap.add_argument("--gamma", type=float, default=0.6, help="the ranking's discount of the agent's values (eva_vos; the other policies rank by gain)")
    ap.add_argument("--rank", action="store_true", help="after the full run, write the reference-schema CSV (<policy>_reference.csv) and the ranking "
                    "(<policy>_ranking.csv: step, video, round, hours, metric) from its rows; implied by --budget-hours / --target-metric")
    a = ap.parse_args()
    if a.working_size is not None and a.working_size < 1:
        ap.error(f"--working-size {a.working_size}: the length of the shorter side, at least 1")
    live = a.budget_hours is not None or a.target_metric is not None
    if (live or a.rank) and a.multi_object:
        ap.error("--rank / --budget-hours / --target-metric rank the reference's per-object sessions: --multi-object is refused")
    if live and a.policy == "upper_bound_mask":
        ap.error("--budget-hours / --target-metric refuse upper_bound_mask: its trials would multiply the cost of every look-ahead round")
    spec = POLICY_TABLE[a.policy]
    typed = "annotation_types" in spec.needs
    if a.annotation_types and "agent" in spec.needs:
        ap.error(f"{a.policy} takes no --annotation-types: its agent chooses between '3clicks' and 'mask', as the reference's")
    if typed and a.multi_object:
        ap.error(f"{a.policy} is a one-object policy: --multi-object supports {', '.join(MULTI_OBJECT_POLICIES)}")
    if typed and not a.annotation_types:
        ap.error(f"{a.policy} needs --annotation-types")
    from . import synth
    prop, fuse = load_networks(a)
    qnet = agent = None
    if "qnet" in spec.needs:
        from .qnet import QualityNet
        qnet = QualityNet()
        qnet.load_state_dict(synth.recipe_state_dict(qnet, seed=3) if a.synthetic_weights else torch.load(a.qnet_weights, map_location="cpu"))
        qnet = qnet.cuda().eval()
    if "agent" in spec.needs:
        from .agent import ActorCritic, PPOAgent
        agent = (PPOAgent(state_dict=synth.recipe_state_dict(ActorCritic(), seed=5)) if a.synthetic_weights else PPOAgent(model_path=a.agent_weights))
    out = os.path.join("Experiments", a.db, "_".join([a.policy] + (sorted(a.annotation_types) if typed else [])) + ".csv")
    kw = dict(qnet=qnet, lanes=a.lanes, multi_object=a.multi_object, share_frames=not a.no_share_frames, annotator=a.annotator if "annotator" in spec.needs else None,
              annotation_types=a.annotation_types, agent=agent, working_size=a.working_size)
    ref_csv, rank_csv = out[:-4] + "_reference.csv", out[:-4] + "_ranking.csv"
    if live:
        from . import budget
        rows, hours, points, _ = budget.run_ranked(a.root, a.imset, out, prop, fuse, a.policy, a.rounds, budget_hours=a.budget_hours, target_metric=a.target_metric,
                                                   gamma=a.gamma, reference_csv=ref_csv, ranking_csv=rank_csv, **kw)
        report_and_leave(f"{len(rows)} committed rounds, {hours[-1]:.3f} annotation hours, metric {points[-1]:.4f} -> {out}, {ref_csv}, {rank_csv}")
        return
    rows = run(a.root, a.imset, out, prop, fuse, a.policy, a.rounds, **kw)
    if a.rank:
        import torch.distributed as dist
        if not dist.is_initialized() or dist.get_rank() == 0:
            from . import budget
            budget.rank_rows(rows, a.policy, ClipDataset(a.root, a.imset).object_names, a.annotation_types, a.gamma, ref_csv, rank_csv)
            out = f"{out}, {ref_csv}, {rank_csv}"
    report_and_leave(f"{len(rows)} rounds -> {out}")


if __name__ == "__main__":
    main()
