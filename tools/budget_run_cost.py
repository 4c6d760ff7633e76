"""GPU box: what a ranked run (eval_driver --target-metric; budget.run_ranked) costs and saves against the full run plus --rank.
Synthetic 480p tree, 8 videos x 40 frames, ``oracle_mask`` and ``eva_vos``, 20 rounds, ONE lane.  Per policy: (a) the full run, ranked
afterwards; (b) the ranked run with ``target_metric`` = the value the full curve has at half its total hours.  Wall seconds, engine
interactions, propagated frames, and the rate of the ranked run's steady chain (one round at a time, whichever video is next) beside the rate
of a one-lane session of the full run (rounds / seconds inside the sessions) and the one-lane driver rate as tools/driver_lanes.py takes it
(8 rounds, rows / wall); (c) the same rounds both ways - the ranked run to exhaustion against the same suspended sessions run video by video.
Writes profiles/budget_run.txt.

python tools/budget_run_cost.py [--out=profiles/budget_run.txt] [videos=8] [frames=40] [rounds=20]"""
import gc
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from eva_vos_amd import _lib, budget, eval_driver, fq_driver, synth  # noqa: E402
from eva_vos_amd import agent as A  # noqa: E402
from eva_vos_amd import qnet as Q  # noqa: E402
from eva_vos_amd.params import FusionNet, PropagationNetwork  # noqa: E402

SPREAD = 0.02                                                   # the README's box spread: the steady chain may be this much slower, no more


def main():
    torch.set_grad_enabled(False)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = ([a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--out=")] or [os.path.join(ROOT, "profiles", "budget_run.txt")])[0]
    nv, T, rounds = (int(args[i]) if len(args) > i else d for i, d in enumerate((8, 40, 20)))
    prop, fuse = PropagationNetwork(), FusionNet()
    prop.load_state_dict(synth.recipe_state_dict(prop))
    fuse.load_state_dict(synth.recipe_state_dict(fuse))
    qnet = Q.QualityNet()
    qnet.load_state_dict(synth.recipe_state_dict(qnet, seed=3))
    qnet = qnet.cuda().eval()
    agent = A.PPOAgent(state_dict=synth.recipe_state_dict(A.ActorCritic(), seed=5))
    policies = {"oracle_mask": {}, "eva_vos": dict(annotator="component", qnet=qnet, agent=agent)}
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        torch.cuda.synchronize()
        st = {}
        t0 = time.perf_counter()
        res = fn(st)
        torch.cuda.synchronize()
        return res, st, time.perf_counter() - t0

    say(f"Ranked run against full run + --rank: {nv} videos x {T} frames at 480 x 854, {rounds} rounds, one lane, recipe weights, library source {_lib.src_hash()}, "
        f"{torch.cuda.get_device_name(0)}.  One run each after a warm-up run; a look-ahead round is GPU work, not annotation time.")
    with tempfile.TemporaryDirectory() as tmp:
        db = os.path.join(tmp, "db")
        imset = fq_driver.make_synthetic_tree(db, {f"v{i}": (T, 480, 854, 1) for i in range(nv)})
        names = [f"v{i}__1" for i in range(nv)]
        eval_driver.run(db, imset, "", prop, fuse, "oracle_mask", rounds=2, lanes=1)                        # pool / allocator warm
        rows, st, dt = timed(lambda st: eval_driver.run(db, imset, "", prop, fuse, "oracle_mask", rounds=8, lanes=1, stats=st))
        say(f"one-lane driver rate as tools/driver_lanes.py takes it (eval_driver, oracle_mask, 8 rounds, engine creation included): "
            f"{len(rows)} rounds in {dt:.2f} s = {len(rows) / dt:.1f} rounds/s; inside the sessions {len(rows) / st['session_s']:.1f} rounds/s")
        for policy, kw in policies.items():
            eval_driver.run(db, imset, "", prop, fuse, policy, rounds=2, lanes=1, **kw)
            full, fst, fdt = timed(lambda st: eval_driver.run(db, imset, os.path.join(tmp, "full.csv"), prop, fuse, policy, rounds=rounds, lanes=1, stats=st, **kw))
            t0 = time.perf_counter()
            hours, points, order = budget.rank_rows(full, policy, names, reference_csv=os.path.join(tmp, f"{policy}_reference.csv"),
                                                    ranking_csv=os.path.join(tmp, f"{policy}_ranking.csv"))
            rank_s = time.perf_counter() - t0
            target = float(points[np.searchsorted(hours, hours[-1] / 2, side="right") - 1])
            (rrows, h, p, o), rst, rdt = timed(lambda st: budget.run_ranked(db, imset, os.path.join(tmp, "ranked.csv"), prop, fuse, policy, rounds=rounds, lanes=1,
                                                                           stats=st, target_metric=target, ranking_csv=os.path.join(tmp, "r.csv"), **kw))
            same = np.array_equal(h, hours[:len(h)]) and np.array_equal(p, points[:len(p)]) and o == order[:len(o)]
            session_rate = fst["interactions"] / fst["session_s"]
            chain_rate = rst["chain_rounds"] / rst["chain_s"] if rst["chain_s"] > 0 and rst["chain_rounds"] else float("nan")
            say()
            say(f"{policy} ({'value' if budget.uses_values(policy) else 'gain'} rule)")
            say(f"  (a) full run + --rank : {fdt:7.2f} s wall (+ {rank_s * 1e3:.1f} ms ranking), {fst['interactions']:4d} interactions, {fst['propagated_frames']:6d} propagated frames; "
                f"curve of {len(points)} points, {hours[-1]:.3f} h, metric {points[0]:.4f} -> {points[-1]:.4f}")
            say(f"  (b) --target-metric {target:.4f} (the full curve's value at half its hours): {rdt:7.2f} s wall, {rst['interactions']:4d} interactions "
                f"({rst['committed_rounds']} committed + {rst['lookahead_rounds']} look-ahead), {rst['propagated_frames']:6d} propagated frames; stopped at {h[-1]:.3f} h, "
                f"metric {p[-1]:.4f}; a prefix of (a)'s curve: {same}")
            say(f"      set-up ({2 * nv} rounds, engines and clips included) {rst['setup_s']:.2f} s; steady chain {rst['chain_rounds']} rounds in {rst['chain_s']:.2f} s = "
                f"{chain_rate:.1f} rounds/s, beside {session_rate:.1f} rounds/s inside the one-lane sessions of (a): {100 * (chain_rate / session_rate - 1):+.1f} % "
                f"({'within' if chain_rate >= session_rate * (1 - SPREAD) else 'BELOW'} the -{100 * SPREAD:.0f} % box spread); per propagated frame: chain "
                f"{rst['chain_propagated_frames'] / max(rst['chain_s'], 1e-9):.0f} frames/s, sessions {fst['propagated_frames'] / fst['session_s']:.0f} frames/s (a session's "
                f"first round walks the whole clip, the chain holds none of those)")
            # (c) the SAME rounds both ways: every video's rounds 2 .. last, as the ranked run to exhaustion chains them and video by video
            runs = []
            for _ in range(2):
                (_, _, _, _), cst, _ = timed(lambda st: budget.run_ranked(db, imset, "", prop, fuse, policy, rounds=rounds, lanes=1, stats=st, **kw))
                line = [f"chain {cst['chain_rounds']} rounds in {cst['chain_s']:.2f} s = {cst['chain_rounds'] / cst['chain_s']:.1f} rounds/s"]
                for what, step in (("video by video with the rows kept", lambda v: v.step(opened.spec)), ("video by video, sessions alone", lambda v: v.stepped.step())):
                    opened = budget.open_videos(db, imset, prop, fuse, policy, rounds, lanes=1, **kw)
                    done = sum(v.stats["interactions"] for v in opened.videos)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for v in opened.videos:
                        with torch.cuda.stream(v.stream):
                            while step(v):
                                pass
                    torch.cuda.synchronize()
                    dt, n = time.perf_counter() - t0, sum(v.stats["interactions"] for v in opened.videos) - done
                    for v in opened.videos:
                        v.stepped.close()
                    del opened, v
                    gc.collect()
                    line.append(f"{what} {n} rounds in {dt:.2f} s = {n / dt:.1f} rounds/s (chain {100 * ((cst['chain_rounds'] / cst['chain_s']) / (n / dt) - 1):+.1f} %)")
                runs.append(", ".join(line))
            say("  (c) the same rounds three ways (rounds 2 .. last of every video): the ranked run to exhaustion; the same suspended sessions run video by video "
                "with the per-round rows and records kept but no ranking; and the sessions alone.  " + ";  again: ".join(runs))
            say(f"      engine footprint the residency rule measured (first engine, clip and two rounds): {rst['engine_footprint_bytes'] / 2 ** 30:.2f} GiB; "
                f"{nv} sessions resident, device memory free at the end {torch.cuda.mem_get_info()[0] / 2 ** 30:.1f} GiB")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
