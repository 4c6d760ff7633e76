"""The annotation session both drivers run: one loop for every policy, and the evaluation and epilogue around it.

Own counterpart of the reference's session loops - the mask policies ``interactions/mask.py:10-39,113-156`` and the mixed-annotation ones
``interactions/mulitple_annotations.py:104-283,307-378`` - and of their helpers ``initialize`` / ``not_avail_frames`` /
``eval_processor_metric`` (``interactions/eval.py:27-117``).  The reference writes the loop out once per policy; here a policy is a
``SessionPolicy`` record - how a frame gets its mask, what else may be done to a frame, how the next frame is chosen, which stop rule
applies - and ``annotation_session`` is the loop (``annotation_rounds``: the same loop, suspended between its rounds).
``fq_driver.oracle_rounds`` and ``eval_driver.run_policy`` / ``run_typed_policy`` / ``run_eva_vos`` build the records; nothing here knows a
policy by name."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np
import torch

from . import metrics

NO_OBJECT = 20.0                        # the reference's token for frames without the object (interactions/eval.py:67)
MASK_SECONDS, SKIP_SECONDS = 80, 3      # annotation cost model of interactions/mask.py:33-36


def frame_quality(processor, gt_thw: torch.Tensor, interacted: List[int], metric: str = "j_and_f"):
    """``eval_processor_metric`` (interactions/eval.py:27-81) for mask annotations: per-frame J or J&F of the engine's
    masks against the ground truth, annotated frames counting with their GT mask (:57-60), NO_OBJECT token for empty GT.
    Returns (mean over frames with an object, generated masks uint8 [T,H,W] on the device, quality[T])."""
    lw, uw, lh, uh = processor.pad
    seg = processor.masks[:, 0, lh:processor.nh - uh, lw:processor.nw - uw] > 0
    gtb = gt_thw > 0.5
    gen = seg.clone()
    if interacted:
        gen[interacted] = gtb[interacted]
    rows = metrics.sequence_scores_gpu(gtb, gen, j_only=metric == "j")      # the boundary measure only when it is asked for
    q = rows[:, 0 if metric == "j" else 2].copy()
    empty = (gtb.flatten(1).sum(1) == 0).cpu().numpy()
    mu = float(np.mean(q[~empty])) if (~empty).any() else float("nan")
    q[empty] = NO_OBJECT
    return mu, gen.to(torch.uint8), q


@dataclass
class SessionPolicy:
    """What ``annotation_session`` needs to know of a policy.
    ``mask_of(f)``: the mask annotation of frame f as ``processor.interact`` takes it - ``gt[f][None]`` for one object, the (k+1)-channel
    one-hot of the label map, with ``interact_kw=dict(scribble=True)``, for k.
    ``choose_frame(worst, types, gen, frames) -> frame or None``: the frame to annotate next, given the scorer's arg-min, the type of every
    frame's current annotation (int64 [T]: 0 none, 1 mask, 2 another), the masks evaluated last (uint8 [T,H,W] on the device) and the
    frames chosen so far; None ends the session.
    ``action(frame, gen, frame_annots) -> (mask, cost, action, logits, clicks, labels, bbox)``: the annotation of the pending frame in every
    round after the first, for a policy that has others than masks (``frame_annots``: pf_annots of ``initialize``, interactions/eval.py:107-115 -
    the actions taken on the frame and the prompts to continue from); None: every round is a mask.
    ``stop_at_T``: which of the reference's two rules ends a session whose rounds outnumber its frames (see ``annotation_session``).
    ``keep_gen``: the policy keeps the evaluated masks of a round beyond the next one (distinct tensors instead of the scorer's scratch).
    ``stop_when_perfect``: the quality rule ends the session at EVERY round, not only from round T on (generate_annotation_dataset.py:109).
    ``check_available``: the ``not_avail_frames`` skip applies (the loop of generate_annotation_dataset.py has none)."""
    mask_of: Callable
    choose_frame: Callable
    action: Optional[Callable] = None
    stop_at_T: bool = True
    keep_gen: bool = False
    interact_kw: dict = field(default_factory=dict)
    stop_when_perfect: bool = False
    check_available: bool = True


class annotation_rounds:
    """``annotation_session``'s loop, suspended between its rounds: ``step()`` runs the next scored round - it walks the round counter past
    the rounds the rules below skip, with the same calls in the same order as the loop written out - and returns False, having run nothing,
    when none is left.  ``ses`` is the running result (what ``annotation_session`` returns, as of the rounds run so far; ``costs[-1]`` is
    the last step's seconds), ``more()`` says whether another ``step()`` would run a round, without running it and without changing the
    session (the stop rules only ever get stricter as the counter grows, so the next counter value decides; it may fetch the quality rows
    once more).  Nothing outside the arguments is touched: sessions stepped in turn give what each gives run straight through."""

    def __init__(self, processor, scorer, T: int, rounds: int, policy: "SessionPolicy", stats: dict = None):
        self.processor, self.scorer, self.T, self.rounds, self.policy, self.stats = processor, scorer, T, rounds, policy, stats
        self.empty = scorer.empty_host
        self.valid = set(np.where(~self.empty)[0].tolist())          # frames that can be annotated at all
        self.types = np.zeros(T, np.int64)
        self.annots = [dict(annotations=[], click_labels=None, click_coords=None, bbox=None, sam_logits=None) for _ in range(T)]
        self.frames, self.done_types, self.costs, self.actions, self.gens = [0], [], [], [], []
        self.gen, self.pending, self.r = None, 0, 0
        self.seen = stats.get("propagated_frames", 0) if stats is not None else 0

    def _skipped(self, r: int) -> bool:
        policy, costs = self.policy, self.costs
        if self.pending is None or not (self.types != 1).any():
            return True
        # the reference's two stop rules for r >= T
        if r >= self.T and policy.stop_at_T:                                                        # interactions/mask.py:16
            return True
        if (r >= self.T or policy.stop_when_perfect) and costs and float(np.min(self.scorer.qualities()[-1])) == 1.0:   # interactions/mulitple_annotations.py:117
            return True
        return bool(policy.check_available and costs and not (self.valid - set(self.frames)))

    def more(self) -> bool:
        return self.r < self.rounds and not self._skipped(self.r + 1)

    def step(self) -> bool:
        while self.r < self.rounds:
            self.r += 1
            if not self._skipped(self.r):
                self._round(self.r)
                return True
        return False

    def _round(self, r: int):
        processor, scorer, policy, stats, types, annots, frames = self.processor, self.scorer, self.policy, self.stats, self.types, self.annots, self.frames
        frame = self.pending
        if r > 1 and policy.action is not None:
            mask, cost, action, logits, clicks, labels, bbox = policy.action(frame, self.gen, annots[frame])
        else:
            mask, cost, action = None, SKIP_SECONDS if r > 1 and self.empty[frame] else MASK_SECONDS, "mask"
        if action == "mask":
            types[frame] = 1
            interaction = policy.mask_of(frame)
        else:
            types[frame] = 2
            interaction = mask.reshape(policy.mask_of(frame).shape).float()
            scorer.set_annotation(frame, mask)
            annots[frame].update(click_labels=labels, click_coords=clicks, bbox=bbox, sam_logits=logits)
        annots[frame]["annotations"].append(action)
        processor.interact(interaction, frame, download=False, **policy.interact_kw)
        if stats is not None:
            stats["propagated_frames"] = stats.get("propagated_frames", 0) + processor.stats()["frames"]
            stats["interactions"] = stats.get("interactions", 0) + 1
        self.done_types.append(int(types[frame]))
        worst, self.gen = scorer.score(processor, frames, keep_gen=policy.keep_gen, **(dict(types=self.done_types) if policy.action is not None else {}))
        self.costs.append(cost)
        self.actions.append(action)
        self.gens.append(self.gen)
        self.pending = policy.choose_frame(worst, types, self.gen, frames)
        if self.pending is not None:
            frames.append(int(self.pending))

    @property
    def ses(self) -> dict:
        n, frames, stats = len(self.costs), self.frames, self.stats
        return dict(frames=frames[:n], types=self.done_types, costs=self.costs, actions=self.actions, gens=self.gens,
                    pending=self.pending if len(frames) > n else None, chosen=frames,
                    propagated_frames=stats.get("propagated_frames", 0) - self.seen if stats is not None else None)


def annotation_session(processor, scorer, T: int, rounds: int, policy: SessionPolicy, stats: dict = None) -> dict:
    """The annotation-session loop of every policy.  Round 1 annotates frame 0 with its mask at 80 s; round r > 1 annotates the frame chosen
    last: with its mask (80 s, or 3 s on a frame without the object) or, where the policy has an ``action``, with what that returns.
    ``store_action_data`` (mulitple_annotations.py:88-101): the action 'mask' makes the frame type 1 and interacts with the ground truth,
    every other action makes it type 2, hands the annotator's mask to ``scorer.set_annotation`` and keeps the prompts for a later annotation
    of the same frame.  The engine propagates (``processor.interact``), ``scorer`` (a metrics.RoundScorer; a metrics.TypedRoundScorer for a
    policy with an ``action``, the only kind that is given ``types=``) evaluates the round on the device, and ``policy.choose_frame`` picks
    the next frame - frames may REPEAT: a type-2 frame stays selectable until it gets its mask.
    A round is skipped when no frame is pending, when every frame has its mask, by the policy's stop rule (below), or - after the first
    scored round - when no frame is left that is neither chosen nor without the object (not_avail_frames, interactions/eval.py:84-89).
    The loop of generate_annotation_dataset.py:108-110 asks for the quality rule at every round and has no not_avail_frames skip:
    ``stop_when_perfect=True``, ``check_available=False`` (one more download of the quality rows per round).
    ``stats`` (optional dict): the frames the engine really visited (``propagated_frames``) and the ``interactions`` are added to it.
    Returns dict(frames, types, costs, actions, gens: per scored round the annotated frame, its type (1 / 2), the seconds, the action and
    the evaluated masks; pending: the frame chosen last, or None; chosen: frames + the pending one; propagated_frames: what this session
    added to ``stats``)."""
    session = annotation_rounds(processor, scorer, T, rounds, policy, stats)
    while session.step():
        pass
    return session.ses


class SteppedSession:
    """What a ``run_*(..., steps=True)`` hands back instead of its result: the suspended session.  ``step()`` runs one scored round (False:
    none was left), ``more()`` says whether another would run, ``costs`` are the seconds of the rounds run so far, ``result()`` is what the
    ``run_*`` would have returned had the session ended after those rounds, ``close()`` gives the engine back as the ``run_*`` found it."""

    def __init__(self, rounds: annotation_rounds, result: Callable, close: Callable = None):
        self.rounds, self._result, self._close = rounds, result, close
        self.step, self.more = rounds.step, rounds.more

    @property
    def costs(self):
        return self.rounds.costs

    def result(self) -> dict:
        return self._result(self.rounds.ses)

    def close(self):
        if self._close is not None:
            self._close, close = None, self._close
            close()

    def run(self) -> dict:
        """Straight through to the end: the ``run_*`` without ``steps``."""
        try:
            while self.step():
                pass
        finally:
            self.close()
        return self.result()


def session_result(scorer, ses: dict) -> dict:
    """What every ``run_*`` returns of a finished session: the per-frame quality of every scored round (fetched from the device once, here),
    its mean over the frames with an object, the seconds of every round and the frames the engine visited."""
    empty = scorer.empty_host
    q = scorer.qualities()
    per_round = [q[i].copy() for i in range(len(ses["costs"]))]
    mus = [float(np.mean(row[~empty])) if (~empty).any() else float("nan") for row in per_round]
    return dict(mu_metrics=mus, annotation_times=ses["costs"], round_metrics=per_round, propagated_frames=ses["propagated_frames"])
