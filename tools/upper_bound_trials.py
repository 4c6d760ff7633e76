"""GPU box: what trying the candidates of ``upper_bound_mask`` on the session's own engine (interact, score_trial, undo) buys against a deep
copy of the engine per candidate.  Synthetic 480x854 tree of 4 videos x 40 frames with one object; eval_driver, upper_bound_mask, j_and_f,
8 rounds, one lane.  Two arms:

  parent   the PARENT COMMIT's library and driver, from a built scratch checkout (--parent DIR): copy.deepcopy + interact + frame_quality
  tree     this tree: undo depth 1 on the session's engine, stcn_metrics_trial, one download of the trial table per round

Every repetition of an arm is a process of its own (the arms are different libraries): it folds the weights, runs one warm-up pass over a
one-video tree, then times eval_driver.run over the four videos - wall time including decode, upload and engine construction - and reads
the device memory in use at the end (the library's buffer pool and PyTorch's allocator keep what they once needed, so this is the peak
footprint of the run).  Three repetitions per arm, interleaved (parent, tree, parent, ...).  The tree arm's last repetition also times the
parts of ONE trial with the device synchronised around each.  A child that fails ends the measurement: nothing more is started.

    git worktree add ../parent HEAD~1 && make -C ../parent/eva_vos_amd/csrc -j8
    python tools/upper_bound_trials.py --parent ../parent > profiles/upper_bound_trials.txt"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDEOS, T, H, W, ROUNDS, REPS = 4, 40, 480, 854, 8, 3
ARMS = ("parent", "tree")
TRIALS = VIDEOS * sum(T - r for r in range(1, ROUNDS + 1))          # every round tries the frames not annotated yet


def _nets(a):
    import torch
    from eva_vos_amd import synth
    from eva_vos_amd.params import FusionNet, PropagationNetwork
    torch.set_grad_enabled(False)
    prop, fuse = PropagationNetwork(), FusionNet()
    prop.load_state_dict(synth.recipe_state_dict(prop))
    fuse.load_state_dict(synth.recipe_state_dict(fuse))
    return prop.eval(), fuse.eval()


def _used_mb():
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2 ** 20


def split_of_one_trial(prop, fuse, root, imset):
    """Device-synchronised ms of the parts of one trial in the middle of a session (frames 0 and 30 annotated, candidate 15: a span of 29
    frames; then frames 0, 10, 20, 30, candidate 15: a span of 9): interact with the journal off (on a deep copy), save + interact with
    depth 1, score_trial, undo - medians of 5."""
    import copy

    import numpy as np
    import torch
    from eva_vos_amd import fq_driver, metrics
    from mivos.inference_core import InferenceCore
    s = fq_driver.ClipDataset(root, imset)[0]
    gt = s["gt"][0].cuda()
    out = []
    for annotated, cand in (([0, 30], 15), ([0, 30, 10, 20], 15)):
        core = InferenceCore(prop, fuse, s["rgb"].cuda(), 1)
        scorer = metrics.RoundScorer(gt[:, 0], "j_and_f", max_rounds=8)
        for i, f in enumerate(annotated):
            core.interact(gt[f][None], f, download=False)
            scorer.score(core, annotated[:i + 1], keep_gen=False)
        plain = copy.deepcopy(core)
        core.set_undo_depth(1)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        rows = []
        for _ in range(6):
            t_plain = timed(lambda: plain.interact(gt[cand][None], cand, download=False))
            plain = copy.deepcopy(core)                              # the untried state again (core is back to it after every undo) ...
            plain.set_undo_depth(0)                                  # ... with the journal off (a copy takes its source's depth)
            t_save_interact = timed(lambda: core.interact(gt[cand][None], cand, download=False))
            nbytes = core.undo_state()["bytes"]
            t_score = timed(lambda: scorer.score_trial(core, annotated, cand, 0))
            t_undo = timed(lambda: core.undo(download=False))
            rows.append((t_plain, t_save_interact, t_score, t_undo))
        med = np.median(np.array(rows[1:]), axis=0)
        lo, hi = max(f for f in annotated if f < cand), min(f for f in annotated if f > cand)
        out.append(dict(span=hi - lo - 1, journal_mb=nbytes / 2 ** 20, interact_ms=med[0], save_interact_ms=med[1], score_ms=med[2], undo_ms=med[3]))
        del core, plain
    return out


def child(a):
    sys.path.insert(0, a.code)
    import numpy as np
    import torch
    from eva_vos_amd import _lib, eval_driver
    assert os.path.dirname(os.path.dirname(os.path.abspath(eval_driver.__file__))) == os.path.abspath(a.code), eval_driver.__file__
    prop, fuse = _nets(a)

    def run(tree):
        root = os.path.join(a.trees, tree)
        imset = os.path.join(root, "ImageSets", "synthetic.txt")
        stats = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = eval_driver.run(root, imset, "", prop, fuse, "upper_bound_mask", rounds=ROUNDS, metric="j_and_f", lanes=1, stats=stats)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, rows, stats

    run("warm")                               # weights folded, buffer pool filled, decode workers up
    wall, rows, stats = run("main")
    res = dict(arm=a.arm, wall=wall, rounds=len(rows), trials=stats.get("trial_interactions", TRIALS), clones=stats.get("engine_clones"),
               used_mb=_used_mb(), rows_sha=hashlib.sha256(np.nan_to_num(np.asarray(rows), nan=-1.0).tobytes()).hexdigest()[:16],
               version=_lib.lib().stcn_version().decode(), device=torch.cuda.get_device_name(0))
    if a.split:
        root = os.path.join(a.trees, "warm")
        res["split"] = split_of_one_trial(prop, fuse, root, os.path.join(root, "ImageSets", "synthetic.txt"))
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit (its eva_vos_amd/libstcn_hip.so in place)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--code")
    ap.add_argument("--trees")
    ap.add_argument("--split", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent or not os.path.exists(os.path.join(a.parent, "eva_vos_amd", "libstcn_hip.so")):
        sys.exit("--parent DIR: a checkout of the parent commit with its library built")
    sys.path.insert(0, HERE)
    from eva_vos_amd import fq_driver
    res = {arm: [] for arm in ARMS}
    with tempfile.TemporaryDirectory() as tmp:
        fq_driver.make_synthetic_tree(os.path.join(tmp, "main"), {f"v{i}": (T, H, W, 1) for i in range(VIDEOS)})
        fq_driver.make_synthetic_tree(os.path.join(tmp, "warm"), {"w0": (T, H, W, 1)})
        for rep in range(REPS):
            for arm in ARMS:
                code = os.path.abspath(a.parent if arm == "parent" else HERE)
                env = {k_: v_ for k_, v_ in os.environ.items() if k_ not in ("PYTHONPATH", "STCN_LIB")}
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--arm", arm, "--code", code, "--trees", tmp]
                if arm == "tree" and rep == REPS - 1:
                    cmd.append("--split")
                out = subprocess.run(cmd, cwd=code, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=420)
                if out.returncode != 0:
                    sys.exit(f"arm {arm}, repetition {rep}: exit status {out.returncode}; nothing more is started\n{out.stderr[-3000:]}")
                res[arm] += [json.loads(line[7:]) for line in out.stdout.splitlines() if line.startswith("RESULT ")]
                print(f"# {arm} repetition {rep}: {res[arm][-1]['wall']:.2f} s", file=sys.stderr, flush=True)
    p0, t0 = res["parent"][0], res["tree"][0]
    print(f"{t0['device']}; {VIDEOS} videos x {T} frames x {H}x{W}, one object each; eval_driver, upper_bound_mask, j_and_f, {ROUNDS} rounds, one lane; "
          f"recipe weights (seed 0)")
    print(f"parent : {p0['version']}")
    print(f"tree   : {t0['version']}")
    print(f"{REPS} interleaved repetitions per arm, one process each (warm-up pass over one video, then the four videos once); wall time of "
          f"eval_driver.run with decode, upload and engine construction; {t0['rounds']} rounds and {TRIALS} trials per run")
    med, spread = {}, {}
    for arm in ARMS:
        rs = res[arm]
        rates = sorted(r["rounds"] / r["wall"] for r in rs)
        med[arm], spread[arm] = rates[len(rates) // 2], rates[-1] - rates[0]
        print(f"{arm:7s}: wall {', '.join(format(r['wall'], '.2f') for r in rs)} s -> rounds/s {', '.join(format(r['rounds'] / r['wall'], '.3f') for r in rs)} "
              f"(median {med[arm]:.3f}, spread {spread[arm]:.3f}); trials/s {', '.join(format(TRIALS / r['wall'], '.1f') for r in rs)}; "
              f"device memory in use at the end {', '.join(format(r['used_mb'], '.0f') for r in rs)} MB; trials counted {rs[0]['trials']}, "
              f"engine clones {rs[0]['clones'] if rs[0]['clones'] is not None else TRIALS} ; rows {rs[0]['rows_sha']}")
    same = len({r["rows_sha"] for arm in ARMS for r in res[arm]}) == 1
    print(f"rows of all runs identical (video, round, mu_metric, annotated frame, per-frame values): {'yes' if same else 'NO'}")
    gain = med["tree"] - med["parent"]
    print(f"tree against parent: {med['tree'] / med['parent']:.3f} x rounds/s ({gain:+.3f}); the parent's own run-to-run spread is {spread['parent']:.3f}: "
          f"the gain {'EXCEEDS' if gain > spread['parent'] else 'DOES NOT EXCEED'} it")
    um = {arm: sorted(r["used_mb"] for r in res[arm])[len(res[arm]) // 2] for arm in ARMS}
    print(f"device memory in use at the end of a run, median: parent {um['parent']:.0f} MB, tree {um['tree']:.0f} MB ({um['tree'] - um['parent']:+.0f} MB)")
    for sp in res["tree"][-1].get("split", []):
        print(f"one trial, span of {sp['span']} frames, device synchronised around each part (median of 5): interact alone {sp['interact_ms']:.2f} ms; "
              f"save + interact {sp['save_interact_ms']:.2f} ms (save = {sp['save_interact_ms'] - sp['interact_ms']:+.2f} ms, journal {sp['journal_mb']:.1f} MB); "
              f"score_trial {sp['score_ms']:.2f} ms; undo {sp['undo_ms']:.2f} ms")


if __name__ == "__main__":
    main()
