"""The video-ranking fixture, from the REAL reference ranking (build container only) -> tests/golden/ranking.npz.

Made-up session records go through ``ranking.write_reference_csv`` into two files and the reference's own ``read_exp`` (``vis/vis_util.py``)
reads them unchanged: a file name with ``oracle_oracle`` in it takes the gain rule, one with ``eva_vos`` the value rule.  The fixture keeps
the records and what the reference returned - data only, a few KB.

The records: 6 videos of 3 to 9 rounds; costs of 80 s (mask), 3 s (a frame without the object) and fractions of a second upward (clicks);
frames with the no-object token 20; an ``rl_values`` entry of exactly -2.04 and one of exactly -2, both where the value rule reads them (the
reference tests ``value + 0.04 == -2``).  Every quality is a multiple of 1/1024 and every video has 4 or 8 frames with the object, so the
means the reference takes are exact in whichever order it adds the videos (it iterates a ``set`` of names).  The reference's order under
exactly equal scores is undefined for the same reason; this tool asserts that the two best scores differ at every step of both curves.

Per video ``v<i>``: ``.mu`` [R], ``.times`` [R], ``.frames`` [R], ``.metrics`` [R,T], ``.values`` [R], ``.actions`` [R] (indices into ``action_names``);
``names``; per rule ``gain`` / ``values``: ``.hours``, ``.points`` as the reference returned them.

Run:  python tools/gen_golden_ranking.py --reference=<checkout of the reference>
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

ACTION_NAMES = ["3clicks", "mask", "no_object"]
TOKEN = 20.0
# name, rounds, frames with the object, frames without
VIDEOS = [("ant__1", 9, 8, 2), ("bee__1", 3, 4, 0), ("bee__2", 6, 4, 1), ("cat__1", 4, 8, 0), ("dog__1", 7, 8, 1), ("eel__1", 5, 4, 3)]
CLICK_SECONDS = [4.5, 5.5, 6.25, 8.5, 11.75]
TOKEN_VIDEO = "eel__1"                                              # the video whose frames without the object get annotated (3 s, gain 0)
PINNED = {("ant__1", 2): -2.04, ("dog__1", 3): -2.0}               # (video, round) -> rl_values entry: read by the value rule at pointer round - 1


def make_sessions(seed: int = 7):
    rs = np.random.RandomState(seed)
    sessions = []
    for name, rounds, n_obj, n_empty in VIDEOS:
        T = n_obj + n_empty
        empty = np.zeros(T, bool)
        empty[rs.choice(np.arange(1, T), n_empty, replace=False)] = True
        q = rs.randint(200, 700, T) / 1024.0
        q[empty] = TOKEN
        rec = dict(video=name, mu_metrics=[], annotation_times=[], round_metrics=[], annotated_frames=[], rl_values=[], annotation_actions=[])
        frame = 0
        for r in range(rounds):
            if r == 0 or (not empty[frame] and rs.rand() < 0.4):
                action, cost = 1, 80.0
            elif empty[frame]:
                action, cost = 2, 3.0
            else:
                action, cost = 0, CLICK_SECONDS[rs.randint(len(CLICK_SECONDS))]
            q = q.copy()
            if not empty[frame]:
                q[frame] = 1.0 if action == 1 else min(1.0, q[frame] + rs.randint(40, 300) / 1024.0)
            near = ~empty & (np.abs(np.arange(T) - frame) == 1)
            q[near] = np.minimum(1.0, q[near] + rs.randint(0, 120, int(near.sum())) / 1024.0)
            rec["mu_metrics"].append(float(np.mean(q[~empty])))
            rec["annotation_times"].append(cost)
            rec["round_metrics"].append([float(v) for v in q])
            rec["annotated_frames"].append(int(frame))
            rec["rl_values"].append(PINNED.get((name, r), -2.0 if r == 0 else 0.0 if action == 2 else float(rs.randint(-300, 1500)) / 997.0))
            rec["annotation_actions"].append(action)
            # the next frame: one that can still gain (frames repeat until they have their mask), so that no two videos stand at a gain of
            # exactly 0 together; frames without the object are annotated in one video only, for the same reason
            left = np.where(~empty & (q < 1.0))[0]
            if name == TOKEN_VIDEO and rs.rand() < 0.4 or not len(left):
                left = np.where(empty)[0] if empty.any() else np.arange(T)
            frame = int(rs.choice(left))
        sessions.append(rec)
    return sessions


def assert_no_ties(sessions, use_values, gamma=0.6):
    """Walk the curve as ``rank_curve`` does and require the two best scores among the videos that can advance to differ at every step."""
    from eva_vos_amd import ranking
    pointers = [0] * len(sessions)
    steps = 0
    while True:
        can = [p + 2 < len(rec["mu_metrics"]) for rec, p in zip(sessions, pointers)]
        scores = [ranking.video_score(rec, p, gamma, use_values, more=ok) for rec, p, ok in zip(sessions, pointers, can)]
        i = ranking.next_video(scores, can)
        if i is None:
            return steps
        live = sorted((s for s, ok in zip(scores, can) if ok), reverse=True)
        assert len(live) < 2 or live[0] != live[1], (steps, live)
        pointers[i] += 1
        steps += 1


def main():
    from eva_vos_amd import ranking
    ref = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--reference=")] or [os.environ.get("EVA_VOS_REFERENCE", "")]
    if not ref[0] or not os.path.isdir(ref[0]):
        sys.exit("give the checkout of the reference: --reference=PATH (or EVA_VOS_REFERENCE)")
    sys.path.insert(0, ref[0])
    from vis.vis_util import read_exp
    assert os.path.abspath(ref[0]) in os.path.abspath(sys.modules["vis.vis_util"].__file__)
    sessions = make_sessions()
    assert sorted(len(s["mu_metrics"]) for s in sessions) == [3, 4, 5, 6, 7, 9]
    costs = {c for s in sessions for c in s["annotation_times"]}
    assert {80.0, 3.0} <= costs and any(c != int(c) for c in costs)
    assert any(TOKEN in row for s in sessions for row in s["round_metrics"])
    used = [v for s in sessions for v in s["rl_values"][1:-1]]          # what the value rule reads: rounds 1 .. last - 1
    assert -2.04 in used and -2.0 in used
    out = {"names": np.array([s["video"] for s in sessions]), "action_names": np.array(ACTION_NAMES)}
    for i, s in enumerate(sessions):
        out[f"v{i}.mu"], out[f"v{i}.times"] = np.array(s["mu_metrics"], np.float64), np.array(s["annotation_times"], np.float64)
        out[f"v{i}.frames"], out[f"v{i}.metrics"] = np.array(s["annotated_frames"], np.int64), np.array(s["round_metrics"], np.float64)
        out[f"v{i}.values"], out[f"v{i}.actions"] = np.array(s["rl_values"], np.float64), np.array(s["annotation_actions"], np.int64)
    with tempfile.TemporaryDirectory(prefix="ranking_") as tmp:
        assert "oracle_oracle" not in tmp and "eva_vos" not in tmp
        for rule, fname, use_values in (("gain", "oracle_oracle_3clicks_mask.csv", False), ("values", "eva_vos.csv", True)):
            steps = assert_no_ties(sessions, use_values)
            path = os.path.join(tmp, fname)
            ranking.write_reference_csv(path, sessions, ACTION_NAMES)
            hours, points = read_exp(path)
            assert len(points) == 1 + steps == 1 + sum(len(s["mu_metrics"]) - 2 for s in sessions), (len(points), steps)
            out[f"{rule}.hours"], out[f"{rule}.points"] = np.asarray(hours, np.float64), np.asarray(points, np.float64)
            print(rule, len(points), "points, hours", hours[0], "..", hours[-1], "metric", points[0], "..", points[-1])
    path = os.path.join(GOLD, "ranking.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
