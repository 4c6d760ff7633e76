"""The dataset-level video ranking of the paper (Eq. 3): given what every video's annotation session recorded, which video gets the next
annotation - and the curve "quality against annotation hours over the whole dataset" that order gives.

Own restatement of the reference's ``rank_policy`` (``vis/vis_util.py:40-150``; ``read_exp`` :5-16 chooses the rule by the file name) on
plain per-video records instead of a data frame, of the CSV it reads (``eval_annotation_method.py:122-139,162-190``) and of a reader for
that CSV.  ``budget.run_ranked`` applies ``next_video`` / ``video_score`` - the same functions ``rank_curve`` is made of - while the
sessions still run.  tests/golden/ranking.npz holds the reference's curve on made-up sessions (tools/gen_golden_ranking.py)."""
from __future__ import annotations

import ast
import csv
import os
from typing import List, Optional, Sequence

import numpy as np

NO_NEXT = -1e10                         # the reference's score of a video whose next round is its last (vis_util.py:120-121)
VALUE_SHIFT = 0.04                      # added to the agent's value before it is used (vis_util.py:110)
RANKING_HEADER = ["step", "video", "round", "hours", "metric"]


def video_score(rec: dict, p: int, gamma: float = 0.6, use_values: bool = False, more: bool = True) -> float:
    """The score of a video whose pointer stands at round ``p``, from its rounds ``p`` and ``p + 1`` alone.  Gain rule: what round p + 1 gained
    on the frame it annotated, per second of it.  ``use_values``: the agent's value of round p + 1, shifted by 0.04 and replaced by 0 where the
    SHIFTED value equals -2 (the reference compares after the addition, so the -2 a session's first round carries is not what is caught),
    discounted by ``gamma ** p``, per second.  ``more``: round p + 1 is not the video's last; where it is, the score is NO_NEXT."""
    if not more:
        return NO_NEXT
    cost = rec["annotation_times"][p + 1]
    if use_values:
        value = rec["rl_values"][p + 1] + VALUE_SHIFT
        if value == -2:
            value = 0
        return value * (gamma ** p) / cost
    f = int(rec["annotated_frames"][p + 1])
    return (rec["round_metrics"][p + 1][f] - rec["round_metrics"][p][f]) / cost


def next_video(scores: Sequence[float], can_advance: Sequence[bool]) -> Optional[int]:
    """The video that advances: the best-scored one among those that can, the FIRST of them under an exact tie; None when none can."""
    best = None
    for i, (s, ok) in enumerate(zip(scores, can_advance)):
        if ok and (best is None or s > scores[best]):
            best = i
    return best


def curve_point(sessions: List[dict], pointers: Sequence[int]) -> float:
    """The mean over the videos of ``mu_metrics[pointer]``."""
    return np.mean([rec["mu_metrics"][p] for rec, p in zip(sessions, pointers)])


def rank_curve(sessions: List[dict], gamma: float = 0.6, use_values: bool = False):
    """``rank_policy`` on per-video records.  ``sessions``: one record per video, in first-appearance order, each with ``mu_metrics``,
    ``annotation_times``, ``round_metrics`` (per round the per-frame values), ``annotated_frames`` and, for ``use_values``, ``rl_values`` - what
    ``run_typed_policy`` / ``run_eva_vos`` return (``run_policy`` names the frames ``frames``; ``read_rows`` builds the records from a run's rows).
    Every video has a pointer, 0 at first; the first point is the mean of the videos' ``mu_metrics[0]`` at the sum of their
    ``annotation_times[0]``.  A step: the video with the best ``video_score`` among those whose pointer is not yet ``last_round - 1`` advances
    by one round, the time grows by that round's seconds, the point is the mean of ``mu_metrics[pointer]``.  A video's LAST round is never
    reached, as in the reference (its data for round p exist only where round p + 1 does).  The curve ends when no video can advance.
    Returns (hours float64 [n], points float64 [n], order: the (index into ``sessions``, round) committed at each step, n - 1 of them).
    Two things the reference leaves open are decided here.  TIES: it iterates a Python ``set`` of names, so its order under exactly equal
    scores is undefined; here the video that appears first wins.  SHORT SESSIONS: a video with fewer than two rounds makes the reference
    raise; here it contributes its constant point (and its first round's seconds) and never advances."""
    n = [len(rec["mu_metrics"]) for rec in sessions]
    if not sessions or min(n) < 1:
        raise ValueError("rank_curve: every video needs at least its first round")
    pointers = [0] * len(sessions)
    points = [curve_point(sessions, pointers)]
    times = [np.sum([rec["annotation_times"][0] for rec in sessions])]
    order = []
    while True:
        can = [p + 2 < k for p, k in zip(pointers, n)]
        scores = [video_score(rec, p, gamma, use_values, more=ok) for rec, p, ok in zip(sessions, pointers, can)]
        i = next_video(scores, can)
        if i is None:
            break
        pointers[i] += 1
        order.append((i, pointers[i]))
        points.append(curve_point(sessions, pointers))
        times.append(times[-1] + sessions[i]["annotation_times"][pointers[i]])
    return np.array(times, np.float64) / 3600, np.array(points, np.float64), order


def read_rows(rows, spec=None, names=None) -> List[dict]:
    """The records of ``rank_curve`` from the float rows ``eval_driver.run`` returns (sample id, round, mu_metric, annotation_time, annotated
    frame, T, T per-frame values, NaN padding, then the policy's tail columns, column j at ``row[-1 - j]``), one per sample id, ids and
    rounds ascending - the order in which the dataset lists its videos, whichever lane finished first.  ``spec``: the policy's ``PolicySpec`` (None: no tail) - an ``rl_values`` column becomes ``rl_values``,
    an ``annotation_actions`` column the action's index in ``annotation_actions``.  ``names``: sample id -> name (``ClipDataset.object_names``);
    the record's ``video`` is the name, or the id without them.  Values are the rows' float32 values, widened."""
    rows = np.asarray(rows)
    by_id = {}
    for row in rows:
        by_id.setdefault(int(row[0]), []).append(row)
    sessions = []
    for sid in sorted(by_id):
        rec = dict(video=names[sid] if names is not None else sid, mu_metrics=[], annotation_times=[], annotated_frames=[], round_metrics=[])
        try:
            append_rows(rec, sorted(by_id[sid], key=lambda r: int(r[1])), spec)
        except ValueError:
            raise ValueError(f"sample {sid}: its rows do not hold the rounds 0..{len(by_id[sid]) - 1} once each") from None
        sessions.append(rec)
    return sessions


def append_rows(rec: dict, rows, spec=None) -> dict:
    """Add the next rounds of a video, from their rows, to its record (``read_rows`` for a session that is still running)."""
    tail = [col.name for col in spec.tail] if spec is not None else []
    for r in rows:
        if int(r[1]) != len(rec["mu_metrics"]):
            raise ValueError(f"round {int(r[1])} where round {len(rec['mu_metrics'])} is due")
        rec["mu_metrics"].append(float(r[2]))
        rec["annotation_times"].append(float(r[3]))
        rec["annotated_frames"].append(int(r[4]))
        rec["round_metrics"].append([float(v) for v in r[6:6 + int(r[5])]])
        for j, name in enumerate(tail):
            rec.setdefault(name, []).append(float(r[-1 - j]) if name == "rl_values" else int(r[-1 - j]))
    return rec


def write_reference_csv(path: str, sessions: List[dict], action_names=None, seconds=float) -> None:
    """One CSV in the reference's own schema: ``video, mu_metric, annotation_time, round, round_metrics, annotated_frames`` and, where the
    records have them, ``rl_values`` and ``annotation_actions`` - ``round_metrics`` as a Python list literal, which the reference's ``read_exp``
    / ``rank_policy`` read with ``ast.literal_eval``.  ``read_exp`` chooses its rule by the FILE NAME: 'oracle_oracle' in it gives the gain rule,
    'eva_vos' the value rule.  ``action_names``: the names an integer ``annotation_actions`` entry indexes (None: written as it is);
    ``seconds``: how ``annotation_time`` is printed (``PolicySpec.seconds``).  Floats are written with ``repr``: they read back exactly."""
    has_values = all("rl_values" in rec for rec in sessions)
    has_actions = all("annotation_actions" in rec for rec in sessions)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(["video", "mu_metric", "annotation_time", "round", "round_metrics", "annotated_frames"]
                    + (["rl_values"] if has_values else []) + (["annotation_actions"] if has_actions else []))
        for rec in sessions:
            for r, mu in enumerate(rec["mu_metrics"]):
                line = [rec["video"], repr(float(mu)), repr(seconds(rec["annotation_times"][r])), r,
                        repr([float(v) for v in rec["round_metrics"][r]]), int(rec["annotated_frames"][r])]
                if has_values:
                    line.append(repr(float(rec["rl_values"][r])))
                if has_actions:
                    a = rec["annotation_actions"][r]
                    line.append(action_names[a] if action_names is not None and not isinstance(a, str) else a)
                wr.writerow(line)


def read_reference_csv(path: str, action_names=None) -> List[dict]:
    """The records ``write_reference_csv`` wrote, value for value (``annotation_actions`` as indices into ``action_names`` when given)."""
    sessions, by_name = [], {}
    with open(path, newline="") as f:
        for line in csv.DictReader(f):
            rec = by_name.get(line["video"])
            if rec is None:
                rec = by_name[line["video"]] = dict(video=line["video"], mu_metrics=[], annotation_times=[], round_metrics=[], annotated_frames=[])
                sessions.append(rec)
            if int(line["round"]) != len(rec["mu_metrics"]):
                raise ValueError(f"{path}: video {line['video']}: round {line['round']} where round {len(rec['mu_metrics'])} is due")
            rec["mu_metrics"].append(float(line["mu_metric"]))
            rec["annotation_times"].append(float(line["annotation_time"]))
            rec["round_metrics"].append([float(v) for v in ast.literal_eval(line["round_metrics"])])
            rec["annotated_frames"].append(int(line["annotated_frames"]))
            if "rl_values" in line:
                rec.setdefault("rl_values", []).append(float(line["rl_values"]))
            if "annotation_actions" in line:
                a = line["annotation_actions"]
                rec.setdefault("annotation_actions", []).append(action_names.index(a) if action_names is not None else a)
    return sessions


def write_ranking_csv(path: str, sessions: List[dict], hours, points, order) -> None:
    """``ranking.csv``: ``step, video, round, hours, metric`` - step 0 is the first point (every video's first round; no video, round 0), step
    s >= 1 the (video, round) committed there.  Floats with ``repr``."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow(RANKING_HEADER)
        for s, (h, m) in enumerate(zip(hours, points)):
            i, r = order[s - 1] if s else (None, 0)
            wr.writerow([s, "" if i is None else sessions[i]["video"], r, repr(float(h)), repr(float(m))])


def read_ranking_csv(path: str):
    """(hours, points, [(video name, round) per step >= 1]) of a ``ranking.csv``."""
    with open(path, newline="") as f:
        lines = list(csv.DictReader(f))
    return (np.array([float(ln["hours"]) for ln in lines], np.float64), np.array([float(ln["metric"]) for ln in lines], np.float64),
            [(ln["video"], int(ln["round"])) for ln in lines[1:]])
