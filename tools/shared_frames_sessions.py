"""GPU box: what sharing a video's frame features between the sessions of its objects buys in the per-object protocol.  Synthetic 480x854
trees of 4 videos x 40 frames with 3 and with 5 objects; eval_driver, oracle policy, j_and_f, 8 rounds, one lane and two lanes.  Three arms:

  parent    the PARENT COMMIT's library and drivers, from a built scratch checkout (--parent DIR): the baseline
  noshare   this tree with share_frames=False: the control, expected inside the parent's run-to-run spread
  share     this tree as it runs by default

Every repetition of an arm is a process of its own (the arms are different libraries): it folds the weights, runs one warm-up pass, then times
each (objects, lanes) configuration once - wall time of eval_driver.run including decode, upload and engine construction.  Three repetitions
per arm, interleaved (parent, noshare, share, parent, ...).  A child that fails ends the measurement: nothing more is started.

    git worktree add ../parent HEAD~1 && make -C ../parent/eva_vos_amd/csrc -j8
    python tools/shared_frames_sessions.py --parent ../parent > profiles/shared_frame_features.txt"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIDEOS, T, H, W, ROUNDS, REPS = 4, 40, 480, 854, 8, 3
CONFIGS = [(k, lanes) for k in (3, 5) for lanes in (1, 2)]
ARMS = ("parent", "noshare", "share")


def child(a):
    sys.path.insert(0, a.code)
    import torch
    from eva_vos_amd import _lib, eval_driver, inference_core, synth
    from eva_vos_amd.params import FusionNet, PropagationNetwork
    assert os.path.dirname(os.path.dirname(os.path.abspath(eval_driver.__file__))) == os.path.abspath(a.code), eval_driver.__file__
    torch.set_grad_enabled(False)
    prop, fuse = PropagationNetwork(), FusionNet()
    prop.load_state_dict(synth.recipe_state_dict(prop, 2))
    fuse.load_state_dict(synth.recipe_state_dict(fuse, 2))
    prop, fuse = prop.eval(), fuse.eval()
    encoded = [0]
    if a.arm == "parent":                     # the parent's drivers do not count key-encoder frames: read the engine's counter after every interaction
        plain = inference_core.InferenceCore.interact

        def counted(self, *args, **kw):
            out = plain(self, *args, **kw)
            encoded[0] += self.stats()["key_miss"]
            return out
        inference_core.InferenceCore.interact = counted
    kw = {} if a.arm == "parent" else {"share_frames": a.arm == "share"}

    def run(k, lanes):
        root = os.path.join(a.trees, f"k{k}")
        imset = os.path.join(root, "ImageSets", "synthetic.txt")
        stats, encoded[0] = {}, 0
        t0 = time.perf_counter()
        rows = eval_driver.run(root, imset, "", prop, fuse, "oracle_mask", rounds=ROUNDS, metric="j_and_f", lanes=lanes, stats=stats, **kw)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        return dict(arm=a.arm, k=k, lanes=lanes, wall=wall, object_rounds=len(rows), key_frames_encoded=stats.get("key_frames_encoded", encoded[0]),
                    engines_created=stats.get("engines_created"), version=_lib.lib().stcn_version().decode(), device=torch.cuda.get_device_name(0))

    run(3, 2)                                 # warm-up: weights folded, buffer pool filled, decode workers up
    for k, lanes in CONFIGS:
        print("RESULT " + json.dumps(run(k, lanes)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit (its eva_vos_amd/libstcn_hip.so in place)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--arm", choices=ARMS)
    ap.add_argument("--code")
    ap.add_argument("--trees")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if not a.parent or not os.path.exists(os.path.join(a.parent, "eva_vos_amd", "libstcn_hip.so")):
        sys.exit("--parent DIR: a checkout of the parent commit with its library built")
    sys.path.insert(0, HERE)
    from eva_vos_amd import fq_driver
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k in (3, 5):
            fq_driver.make_synthetic_tree(os.path.join(tmp, f"k{k}"), {f"v{i}": (T, H, W, k) for i in range(VIDEOS)})
        for rep in range(REPS):
            for arm in ARMS:
                code = os.path.abspath(a.parent if arm == "parent" else HERE)
                env = {k_: v_ for k_, v_ in os.environ.items() if k_ not in ("PYTHONPATH", "STCN_LIB")}
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--arm", arm, "--code", code, "--trees", tmp],
                                     cwd=code, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
                if out.returncode != 0:
                    sys.exit(f"arm {arm}, repetition {rep}: exit status {out.returncode}; nothing more is started\n{out.stderr[-3000:]}")
                for line in out.stdout.splitlines():
                    if line.startswith("RESULT "):
                        r = json.loads(line[7:])
                        res.setdefault((r["k"], r["lanes"]), {}).setdefault(arm, []).append(r)
    any_r = next(iter(res.values()))
    print(f"{any_r['share'][0]['device']}; {VIDEOS} videos x {T} frames x {H}x{W}, eval_driver per-object protocol, oracle_mask, j_and_f, {ROUNDS} rounds; "
          f"multi-object recipe (seed 2)")
    print(f"parent : {any_r['parent'][0]['version']}")
    print(f"tree   : {any_r['share'][0]['version']}")
    print(f"{REPS} interleaved repetitions per arm, one process each (warm-up pass, then every configuration once); wall time of eval_driver.run with "
          f"decode, upload and engine construction; rate = object-rounds / wall")
    for (k, lanes), arms in sorted(res.items()):
        print(f"\n== {k} objects per video, {lanes} lane{'s' if lanes > 1 else ''} ==")
        med, spread = {}, {}
        for arm in ARMS:
            rs = arms[arm]
            rates = sorted(r["object_rounds"] / r["wall"] for r in rs)
            med[arm], spread[arm] = rates[len(rates) // 2], rates[-1] - rates[0]
            print(f"{arm:8s}: {rs[0]['object_rounds']} object-rounds, wall {', '.join(format(r['wall'], '.2f') for r in rs)} s -> "
                  f"{', '.join(format(r['object_rounds'] / r['wall'], '.1f') for r in rs)} object-rounds/s (median {med[arm]:.1f}, spread {spread[arm]:.1f}); "
                  f"key_frames_encoded {rs[0]['key_frames_encoded']}, engines_created {rs[0]['engines_created']}")
        gain = med["share"] - med["parent"]
        print(f"share against parent: {med['share'] / med['parent']:.3f} x ({gain:+.1f} object-rounds/s); the parent's own spread is {spread['parent']:.1f}: "
              f"the gain {'EXCEEDS' if gain > spread['parent'] else 'DOES NOT EXCEED'} it")
        lo, hi = med["parent"] - spread["parent"], med["parent"] + spread["parent"]
        print(f"control (noshare against parent): {med['noshare'] / med['parent']:.3f} x, "
              f"{'inside' if lo <= med['noshare'] <= hi else 'OUTSIDE'} the parent's median +- spread ({lo:.1f} .. {hi:.1f})")


if __name__ == "__main__":
    main()
