"""Annotation-policy evaluation on the HIP engine, sharded over the GPUs of one node (BASELINE config 5, mask policies).

Own counterpart of the reference driver ``eval_annotation_method.py:118-190`` for the policies whose annotations are
ground-truth masks - ``oracle_mask``, ``rand_mask``, ``qnet_mask``, ``upper_bound_mask``, ``l2_mask`` (``interactions/mask.py:10-39,
42-71,74-103,196-227,159-193``) - with their helpers ``initialize`` / ``not_avail_frames`` / ``eval_processor_metric``
(``interactions/eval.py:27-117``) and the frame selectors of ``interactions/policies.py``.  The click / bbox policies
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

Usage:  python -m eva_vos_amd.eval_driver --root data/MOSE --imset data/MOSE/ImageSets/test.txt --policy oracle_mask
        (multi-GPU: python -m torch.distributed.run --nproc-per-node N -m eva_vos_amd.eval_driver ...)
"""
from __future__ import annotations

import argparse
import copy
import csv
import os
import random
import time

import numpy as np
import torch

from . import metrics, shard
from .frame_select import farthest_frame
from .fq_driver import NO_OBJECT, ClipDataset, LaneCores, annotation_session, frame_quality, lane_engine_options, run_lanes, typed_annotation_session

POLICIES = ("oracle_mask", "rand_mask", "qnet_mask", "upper_bound_mask", "l2_mask")
# QNet takes one binary mask; the upper bound builds on the one-object scorer; the l2 selector needs no mask at all
MULTI_OBJECT_POLICIES = ("oracle_mask", "rand_mask", "l2_mask")
# the mixed-annotation policies (interactions/mulitple_annotations.py:104-283): run_typed_policy, with an annotator; one-object sessions
TYPED_POLICIES = ("rand_type", "rand_rand", "oracle_oracle")
# eva_vos (interactions/mulitple_annotations.py:286-378): run_eva_vos, with an annotator, the QNet and the agent; one-object sessions
AGENT_POLICIES = ("eva_vos",)
ANNOTATORS = ("component",)                                   # built in; a real SAM controller is passed through run(..., annotator=...)
MAX_OBJECTS = 32                                              # STCN_MAX_OBJECTS
MASK_SECONDS, SKIP_SECONDS = 80, 3            # annotation cost model of interactions/mask.py:33-36


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
               stats: dict = None):
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
    processor is touched; ``stats["frame_distance_passes"]`` counts the engine passes the session added (0 when the core came with the matrix)."""
    assert policy in POLICIES, policy
    if multi_object and policy not in MULTI_OBJECT_POLICIES:
        raise ValueError(f"multi-object sessions support the policies {' and '.join(MULTI_OBJECT_POLICIES)}, not {policy}")
    T = sample["num_frames"]
    _check_l2_clip(policy, T, f"clip {sample.get('name', '?')}")
    dev = processor.prob.device
    rng = rng or random
    # the evaluation of a round stays on the device (metrics.RoundScorer): one int per round crosses PCIe for the oracle policy, the
    # per-frame quality rows of the whole session are fetched once at the end
    scorer_args = dict(max_rounds=max(rounds, 1), no_object=NO_OBJECT)
    if multi_object:
        k = int(sample["num_objects"])
        scorer = metrics.RoundScorer(sample["gt"][0, :, 0].to(dev), "j" if metric == "j" else "j_and_f", num_objects=k, **scorer_args)
        channels = torch.arange(k + 1, device=dev, dtype=torch.uint8)[:, None, None, None]

        def annotate(f):
            processor.interact((scorer.gt[f][None, None] == channels).float(), f, scribble=True, download=False)      # [k+1,1,H,W]
    else:
        gt = sample["gt"][0].to(dev)                               # [T,1,H,W]
        gt_thw = gt[:, 0]
        images = sample["rgb"][0].to(dev) if policy == "qnet_mask" else None
        scorer = metrics.RoundScorer(gt_thw, "j" if metric == "j" else "j_and_f", **scorer_args)

        def annotate(f):
            processor.interact(gt[f][None], f, download=False)

    def choose(worst, gen, frames):
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

    stats = {} if stats is None else stats
    seen = stats.get("propagated_frames", 0)
    in_place = policy == "upper_bound_mask" and T <= KEY_CACHE_FRAMES
    if policy == "upper_bound_mask":
        stats.setdefault("trial_interactions", 0), stats.setdefault("engine_clones", 0)
    depth = processor.undo_state()["depth"] if in_place else 0
    if in_place:
        processor.set_undo_depth(max(depth, 1))
    passes = processor.frame_distance_passes if policy == "l2_mask" else 0
    try:
        frames, gens = annotation_session(processor, scorer, T, rounds, annotate, choose, keep_gen=policy == "qnet_mask", stats=stats)
    finally:
        if in_place:
            processor.set_undo_depth(depth)                        # the core goes back to its lane as it came
    if policy == "l2_mask":
        stats["frame_distance_passes"] = stats.get("frame_distance_passes", 0) + processor.frame_distance_passes - passes
    empty, scored = scorer.empty_host, len(gens)
    times = [MASK_SECONDS] + [SKIP_SECONDS if empty[f] else MASK_SECONDS for f in frames[1:]]
    q = scorer.qualities()
    per_round = [q[i].copy() for i in range(scored)]
    mus = [float(np.mean(row[~empty])) if (~empty).any() else float("nan") for row in per_round]
    res = dict(mu_metrics=mus, annotation_times=times[:-1], frames=frames, round_metrics=per_round, propagated_frames=stats.get("propagated_frames", 0) - seen)
    if multi_object:
        oq = scorer.object_qualities()
        res.update(object_metrics=[oq[i].copy() for i in range(scored)], present=scorer.present_host)
    return res


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


def run_typed_policy(policy: str, processor, sample, rounds: int, annotator, annotation_types, metric: str = "j_and_f", rng=None,
                     stats: dict = None, scorer=None, choose_action=None):
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
    ``propagated_frames``."""
    from .annotate import check_annotation_types
    assert policy in TYPED_POLICIES, policy
    types_ = check_annotation_types(annotation_types)
    if policy == "rand_type" and len(types_) != 1:
        raise ValueError(f"rand_type takes one annotation type, got {types_}")
    if policy != "rand_type" and len(types_) < 2:
        raise ValueError(f"{policy} requires more than one annotation type, got {types_}")
    if "object_ids" in sample:                                      # a per-video sample (ClipDataset(..., per_video=True))
        raise ValueError(f"{policy} is a one-object policy: multi-object sessions support {' and '.join(MULTI_OBJECT_POLICIES)}")
    T = sample["num_frames"]
    dev = processor.prob.device
    rng = rng or random
    gt = sample["gt"][0].to(dev)                                   # [T,1,H,W]
    images = sample["rgb"][0].to(dev)
    if scorer is None:
        scorer = metrics.TypedRoundScorer(gt[:, 0], "j" if metric == "j" else "j_and_f", max_rounds=max(rounds, 1), no_object=NO_OBJECT)
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

    def next_frame(worst, types):
        if policy == "oracle_oracle":
            return worst
        left = np.where(types != 1)[0]
        return int(rng.choice(left.tolist())) if len(left) else None

    stats = {} if stats is None else stats
    seen = stats.get("propagated_frames", 0)
    ses = typed_annotation_session(processor, scorer, T, rounds, gt, choose_action or policy_action, next_frame, stats=stats)
    q = scorer.qualities()
    per_round = [q[i].copy() for i in range(len(ses["costs"]))]
    mus = [float(np.mean(row[~empty])) if (~empty).any() else float("nan") for row in per_round]
    return dict(mu_metrics=mus, annotation_times=ses["costs"], annotations_actions=ses["actions"], round_metrics=per_round,
                annotated_frames=ses["frames"], frames=ses["frames"], types=ses["types"], action_data=action_data,
                propagated_frames=stats.get("propagated_frames", 0) - seen)


def run_eva_vos(processor, sample, rounds: int, annotator, qnet, agent, metric: str = "j_and_f", rng=None, stats: dict = None, scorer=None,
                selector=None):
    """One sample through ``rounds`` rounds of ``eva_vos`` (interactions/mulitple_annotations.py:307-378): the first round is the mask of frame
    0 at 80 s; every later round the AGENT chooses how the pending frame is annotated (``rl_agent_annotate``, :286-304) and the QNET which
    frame comes next (:356-369).  ``annotator``: an ``annotate.PromptAnnotator`` whose predictor gives an image embedding; ``qnet``: a
    ``QualityNet`` in eval mode; ``agent``: an ``agent.PPOAgent``; ``rng``: the session's ``torch.Generator`` the agent's draws come from (None:
    torch's global one) - runs are reproducible under it and, as for the other typed policies, not comparable draw for draw with the reference.
    ``selector``: the video's ``qnet.QNetSelector`` when the caller keeps one (the sessions of a video's objects), else one is made from
    ``sample['rgb']``; its ``masks_to_input`` (``agent.masks_to_224`` by default) also builds the agent's mask input; ``scorer``: another evaluation with ``TypedRoundScorer``'s interface (``metrics.HostTypedScorer``).
    The annotation types are the reference's hard-coded ``['3clicks', 'mask'][action]``, plus 'no_object' (3 s, value 0, no agent call) on a frame
    without the object.  Returns the reference's values - ``mu_metrics``, ``annotation_times``, ``rl_values`` (the first entry is -2, :316),
    ``annotations_actions``, ``round_metrics``, ``annotated_frames`` - plus ``frames``, ``types`` and ``propagated_frames``."""
    from .agent import AVAIL_ACTIONS, masks_to_224
    from .annotate import ANNOTATION_COSTS
    if "object_ids" in sample:                                      # a per-video sample (ClipDataset(..., per_video=True))
        raise ValueError(f"eva_vos is a one-object policy: multi-object sessions support {' and '.join(MULTI_OBJECT_POLICIES)}")
    T = sample["num_frames"]
    dev = processor.prob.device
    gt = sample["gt"][0].to(dev)                                   # [T,1,H,W]
    images = sample["rgb"][0].to(dev)
    if scorer is None:
        scorer = metrics.TypedRoundScorer(gt[:, 0], "j" if metric == "j" else "j_and_f", max_rounds=max(rounds, 1), no_object=NO_OBJECT)
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

    stats = {} if stats is None else stats
    seen = stats.get("propagated_frames", 0)
    ses = typed_annotation_session(processor, scorer, T, rounds, gt, choose_action, None, stats=stats, select=select)
    q = scorer.qualities()
    per_round = [q[i].copy() for i in range(len(ses["costs"]))]
    mus = [float(np.mean(row[~empty])) if (~empty).any() else float("nan") for row in per_round]
    return dict(mu_metrics=mus, annotation_times=ses["costs"], rl_values=rl_values, annotations_actions=ses["actions"], round_metrics=per_round,
                annotated_frames=ses["frames"], frames=ses["frames"], types=ses["types"], propagated_frames=stats.get("propagated_frames", 0) - seen)


def make_annotator(name: str):
    """The built-in annotators of the command line: 'component' = ``PromptAnnotator`` over the ``ComponentPredictor`` stand-in."""
    from .annotate import ComponentPredictor, PromptAnnotator
    if name != "component":
        raise ValueError(f"unknown annotator {name!r}: built in are {', '.join(ANNOTATORS)}; pass a PromptAnnotator over a SAM controller to run()")
    return PromptAnnotator(ComponentPredictor())


def run(root: str, imset: str, out_csv: str, prop_net, fuse_net, policy: str = "oracle_mask", rounds: int = 60,
        metric: str = "j_and_f", qnet=None, seed: int = 0, device: str = "cuda", lanes: int = 2, stats: dict = None,
        multi_object: bool = False, share_frames: bool = True, annotator=None, annotation_types=None, agent=None):
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
    3 s, the annotated frame is the session's, the per-frame values are that object's."""
    import torch.distributed as dist

    from mivos.inference_core import InferenceCore
    rank = dist.get_rank() if dist.is_initialized() else 0
    world = dist.get_world_size() if dist.is_initialized() else 1
    if multi_object and policy not in MULTI_OBJECT_POLICIES:
        raise ValueError(f"multi-object sessions support the policies {' and '.join(MULTI_OBJECT_POLICIES)}, not {policy}")
    typed = policy in TYPED_POLICIES
    agent_policy = policy in AGENT_POLICIES
    if agent_policy:
        for name, given in (("qnet", qnet), ("agent", agent), ("annotator", annotator)):
            if given is None:
                raise ValueError(f"{policy} needs {name}=...: a QualityNet in eval mode, an agent.PPOAgent and an annotator ('component' or a factory "
                                 "of PromptAnnotator objects)")
        action_names = sorted({"3clicks", "mask", "no_object"})
        lane_selectors = __import__("threading").local()
    if typed:
        from .annotate import check_annotation_types
        action_names = sorted(set(check_annotation_types(annotation_types or ())) | {"mask"})
        if annotator is None:
            raise ValueError(f"{policy} needs an annotator: 'component' or a factory of PromptAnnotator objects")
    if typed or agent_policy:
        make = (lambda: make_annotator(annotator)) if isinstance(annotator, str) else annotator
        lane_annotators = __import__("threading").local()
    ds = ClipDataset(root, imset, per_video=multi_object)
    for v, k, _ in ds.samples if multi_object else ():
        if k > MAX_OBJECTS:
            raise ValueError(f"video {v} has {k} objects: a multi-object session holds at most {MAX_OBJECTS}")
    t_max = max(s[2] for s in ds.samples)
    _check_l2_clip(policy, t_max, "the longest clip")
    share_frames = share_frames and not multi_object
    if share_frames:
        mine = sorted(shard.lpt_assign_grouped([s[2] for s in ds.samples], [s[0] for s in ds.samples], world)[rank])      # the objects of a video share an engine
    else:
        mine = sorted(shard.lpt_assign([s[2] * (s[1] if multi_object else 1) for s in ds.samples], world)[rank])      # multi-object: frames x objects
    cores = LaneCores(lambda sample: InferenceCore(prop_net, fuse_net, sample["rgb"], sample["num_objects"] if multi_object else 1,
                                                   engine_options=lane_engine_options(lanes)), share_frames)
    width = 6 + t_max + (1 if typed else 2 if agent_policy else 0)
    stats_lock = __import__("threading").Lock()

    def work(i, sample):
        rows = []
        t_c = time.perf_counter()
        proc = cores.core_for(sample)
        t_s = time.perf_counter()
        session = {}
        if (typed or agent_policy) and not hasattr(lane_annotators, "a"):
            lane_annotators.a = make()
        if agent_policy:
            selector = None
            if share_frames:                                        # the sessions of a video's objects: one clip, one pass of the QNet's frame branch
                if getattr(lane_selectors, "video", None) != sample["video"]:
                    from .qnet import QNetSelector
                    lane_selectors.video, lane_selectors.s = sample["video"], QNetSelector(qnet, sample["rgb"][0])
                selector = lane_selectors.s
            res = run_eva_vos(proc, sample, rounds, lane_annotators.a, qnet, agent, metric, torch.Generator().manual_seed(seed * 100003 + i),
                              stats=session, selector=selector)
        elif typed:
            res = run_typed_policy(policy, proc, sample, rounds, lane_annotators.a, annotation_types, metric, random.Random(seed * 100003 + i), stats=session)
        else:
            res = run_policy(policy, proc, sample, rounds, metric, qnet, random.Random(seed * 100003 + i), multi_object=multi_object, stats=session)
        cores.done(proc)
        if stats is not None:
            with stats_lock:
                stats["create_s"] = stats.get("create_s", 0.0) + t_s - t_c
                stats["session_s"] = stats.get("session_s", 0.0) + time.perf_counter() - t_s
                stats["propagated_frames"] = stats.get("propagated_frames", 0) + res["propagated_frames"]
                stats["interactions"] = stats.get("interactions", 0) + len(res["mu_metrics"])
                for n in ("trial_interactions", "engine_clones", "frame_distance_passes"):
                    if n in session:
                        stats[n] = stats.get(n, 0) + session[n]
        if multi_object:
            for o, sid in enumerate(sample["object_ids"]):
                here = res["present"][o]
                for r, oq in enumerate(res["object_metrics"]):
                    row = np.full(width, np.nan, np.float32)
                    f = res["frames"][r]
                    row[:6] = (sid, r, float(np.mean(oq[o][here])) if here.any() else float("nan"), MASK_SECONDS if here[f] else SKIP_SECONDS, f, oq.shape[1])
                    row[6:6 + oq.shape[1]] = oq[o]
                    rows.append(row)
            return rows
        for r, (mu, sec, q) in enumerate(zip(res["mu_metrics"], res["annotation_times"], res["round_metrics"])):
            row = np.full(width, np.nan, np.float32)
            row[:6] = (i, r, mu, sec, res["frames"][r], len(q))
            row[6:6 + len(q)] = q
            if typed:
                row[-1] = action_names.index(res["annotations_actions"][r])
            if agent_policy:
                row[-2:] = (action_names.index(res["annotations_actions"][r]), res["rl_values"][r])
            rows.append(row)
        return rows

    def lane_done():
        cores.release()
        if agent_policy:
            lane_selectors.video = lane_selectors.s = None

    rows = run_lanes(root, imset, mine, lanes, work, device, stats, per_video=multi_object, share_frames=share_frames, lane_done=lane_done)
    if stats is not None:
        cores.add_to(stats)
    allrows = shard.gather_rows(np.stack(rows) if rows else np.zeros((0, width), np.float32), width)
    if rank == 0 and out_csv:
        os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
        order = np.lexsort((allrows[:, 1], allrows[:, 0]))
        with open(out_csv, "w", newline="") as f:
            wr = csv.writer(f)
            wr.writerow(["video", "mu_metric", "annotation_time", "round"] + (["rl_values"] if agent_policy else [])
                        + (["annotation_actions"] if typed or agent_policy else []))
            for row in allrows[order]:
                if agent_policy:
                    wr.writerow([ds.object_names[int(row[0])], float(row[2]), float(row[3]), int(row[1]), float(row[-1]), action_names[int(row[-2])]])
                    continue
                if typed:                                          # click costs are fractions of a second
                    wr.writerow([ds.object_names[int(row[0])], float(row[2]), float(row[3]), int(row[1]), action_names[int(row[-1])]])
                    continue
                wr.writerow([ds.object_names[int(row[0])], float(row[2]), int(row[3]), int(row[1])])
    return allrows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--imset", required=True)
    ap.add_argument("--policy", default="oracle_mask", choices=POLICIES + TYPED_POLICIES + AGENT_POLICIES)
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
    a = ap.parse_args()
    if a.policy in AGENT_POLICIES and a.annotation_types:
        ap.error(f"{a.policy} takes no --annotation-types: its agent chooses between '3clicks' and 'mask', as the reference's")
    if a.policy in TYPED_POLICIES:
        if a.multi_object:
            ap.error(f"{a.policy} is a one-object policy: --multi-object supports {', '.join(MULTI_OBJECT_POLICIES)}")
        if not a.annotation_types:
            ap.error(f"{a.policy} needs --annotation-types")
    import torch.distributed as dist

    from . import synth
    from .params import FusionNet, PropagationNetwork
    torch.set_grad_enabled(False)
    shard.init_from_env()                                  # one process per GPU; RCCL unless STCN_DIST_BACKEND says otherwise
    prop, fuse, qnet, agent = PropagationNetwork(top_k=a.top_k, km=a.km), FusionNet(), None, None
    if a.policy in ("qnet_mask",) + AGENT_POLICIES:
        from .qnet import QualityNet
        qnet = QualityNet()
    if a.synthetic_weights:
        prop.load_state_dict(synth.recipe_state_dict(prop))
        fuse.load_state_dict(synth.recipe_state_dict(fuse))
        if qnet is not None:
            qnet.load_state_dict(synth.recipe_state_dict(qnet, seed=3))
    else:
        prop.load_state_dict(torch.load(a.prop_weights, map_location="cpu"))
        fuse.load_state_dict(torch.load(a.fusion_weights, map_location="cpu"))
        if qnet is not None:
            qnet.load_state_dict(torch.load(a.qnet_weights, map_location="cpu"))
    if qnet is not None:
        qnet = qnet.cuda().eval()
    if a.policy in AGENT_POLICIES:
        from .agent import ActorCritic, PPOAgent
        agent = (PPOAgent(state_dict=synth.recipe_state_dict(ActorCritic(), seed=5)) if a.synthetic_weights else PPOAgent(model_path=a.agent_weights))
    typed = a.policy in TYPED_POLICIES
    out = os.path.join("Experiments", a.db, "_".join([a.policy] + (sorted(a.annotation_types) if typed else [])) + ".csv")
    rows = run(a.root, a.imset, out, prop.eval(), fuse.eval(), a.policy, a.rounds, qnet=qnet, lanes=a.lanes, multi_object=a.multi_object,
               share_frames=not a.no_share_frames, annotator=a.annotator if typed or agent else None, annotation_types=a.annotation_types, agent=agent)
    if not dist.is_initialized() or dist.get_rank() == 0:
        print(f"{len(rows)} rounds -> {out}")
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
