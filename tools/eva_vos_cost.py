"""GPU box: what does an ``eva_vos`` round cost beside its propagation - and does the mask-resize kernel earn its place?

On a synthetic 480 x 854 tree (4 videos x 40 frames, one lane, 8 rounds - the setting of profiles/click_robot.txt), recipe weights, the
``ComponentPredictor`` stand-in, three repetitions interleaved over what is compared, in one process:

  sessions: rounds/s of ``eva_vos`` beside ``qnet_mask`` and ``oracle_oracle`` ('3clicks', 'mask') on the same tree, clip decoding included;

  the tail of a round by part, ms per call from HIP events (calls back to back: 20, for the resize 2000) and, where the host waits, wall clock:
    agent state + act   : image embedding of the stand-in + masks_to_224 of one frame + PPOAgent.act (wall clock: ends in a download)
    masks_to_224        : the kernel (stcn_masks_resize_nearest) beside the torch route on the same ``gen`` at T = 40 and T = 66 -
                          ``.float()`` + ``interpolate(mode='nearest')`` + the expand made contiguous, which is what the first conv does to it
    mask branch         : qnet.mask_branch over [T,3,224,224]
    rgb branch          : cached (QNetSelector: nothing per round) against recomputed per round (to_224's bicubic resize + qnet.rgb_branch)
    selection           : select_farthest over [T,1024] (wall clock: one index comes back)

KEEP-OR-DROP RULE for the kernel (printed as the verdict, checked on the medians, no margin): it stays only if it is not slower than the torch
route at both T.

NOT measured here: a real SAM behind the annotator, trained QNet / agent weights, real videos, several lanes.

python tools/eva_vos_cost.py [--out profiles/eva_vos_session.txt] [--reps 3] [--no-session]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from eva_vos_amd import _lib, agent as A, annotate, eval_driver, fq_driver, qnet as Q, synth  # noqa: E402
from eva_vos_amd.params import FusionNet, PropagationNetwork  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "eva_vos_session.txt")
H, W, CALLS, ROUNDS = 480, 854, 20, 8
RESIZE_CALLS = 2000           # a resize is some tens of microseconds: enough calls for a window of tens of milliseconds
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return f"{np.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def wall_ms(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / calls


def events_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def torch_route(gen):
    """What a round pays without the kernel: the float copy of the whole clip, the resize, and the expand made real (the first conv's copy)."""
    return A.masks_to_224_torch(gen).contiguous()


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    say(f"eva_vos round tail at {H} x {W}, library source {_lib.src_hash()}, {torch.cuda.get_device_name(0)}; {REPS} repetitions interleaved, "
        f"{CALLS} calls each ({RESIZE_CALLS} for masks_to_224)")
    qnet = Q.QualityNet()
    qnet.load_state_dict(synth.recipe_state_dict(qnet, seed=3))
    qnet = qnet.to(dev).eval()
    agent = A.PPOAgent(state_dict=synth.recipe_state_dict(A.ActorCritic(), seed=5), device=dev)
    ok = True
    parts = {}
    for T in (40, 66):
        gen = (synth.synthetic_mask(T, H, W, 1)[0, :, 0] > 0.5).to(torch.uint8).to(dev)
        assert torch.equal(A.masks_to_224(gen), torch_route(gen))                 # warm-up, and the two routes must agree
        k, t = [], []
        for rep in range(REPS):
            k.append(events_ms(lambda: A.masks_to_224(gen), RESIZE_CALLS))
            t.append(events_ms(lambda: torch_route(gen), RESIZE_CALLS))
        parts[T] = (k, t)
        say(f"masks_to_224, T = {T}: uint8 [{T},{H},{W}] -> fp32 [{T},3,224,224]")
        say(f"   kernel (one launch)                         {spread(k)}")
        say(f"   torch (.float + interpolate + expand copy)  {spread(t)}")
        say(f"   kernel / torch = {np.median(k) / np.median(t):.3f}; per repetition: " + ", ".join(f"{a / b:.3f}" for a, b in zip(k, t)))
        ok = ok and float(np.median(k)) <= float(np.median(t))
    say()
    say("VERDICT (keep-or-drop rule): the kernel is " + ("not slower than the torch route at both T: it STAYS" if ok
                                                         else "SLOWER than the torch route at a T: it is to be TAKEN OUT (masks_to_224 = the torch route)"))
    say()
    T = 40
    clip = synth.synthetic_clip(T, H, W)[0].to(dev)
    gt = (synth.synthetic_mask(T, H, W, 1)[0, :, 0] > 0.5).to(torch.uint8).to(dev)
    gen = gt.roll(3, 2).contiguous()
    ann = annotate.PromptAnnotator(annotate.ComponentPredictor())
    sel = Q.QNetSelector(qnet, clip)
    m3 = A.masks_to_224(gen)
    feats = sel.features(gen)

    def agent_step():
        return agent.act(ann.image_embedding(clip[7], gt[7]), A.masks_to_224(gen, [7]), generator=None)[1].item()

    def rgb_recomputed():
        imgs = F.interpolate(clip, size=(224, 224), mode="bicubic", antialias=True, align_corners=False)
        return qnet.rgb_branch(imgs)

    timed = {"agent state + act (wall clock, embedding of the stand-in on the host included)": (wall_ms, agent_step),
             "   of which PPOAgent.act on ready inputs (wall clock)": (wall_ms, lambda e=ann.image_embedding(clip[7], gt[7]), m=A.masks_to_224(gen, [7]): agent.act(e, m)),
             "mask branch over [40,3,224,224]": (events_ms, lambda: qnet.mask_branch(m3)),
             "rgb branch recomputed (bicubic resize + branch); cached: 0": (events_ms, rgb_recomputed),
             "selection, select_farthest (wall clock)": (wall_ms, lambda: Q.select_farthest(feats, [0, 9, 9, 21]))}
    res = {n: [] for n in timed}
    for fn in timed.values():
        fn[1]()                                                                    # warm-up
    for rep in range(REPS):
        for n, (clock, fn) in timed.items():
            res[n].append(clock(fn, CALLS))
    say(f"the tail of a round by part, T = {T}:")
    for n in timed:
        say(f"   {n:84s} {spread(res[n])}")
    say(f"   {'masks_to_224 of the clip (above)':84s} {spread(parts[40][0])}")
    if "--no-session" not in sys.argv:
        say()
        prop, fuse = PropagationNetwork(), FusionNet()
        prop.load_state_dict(synth.recipe_state_dict(prop))
        fuse.load_state_dict(synth.recipe_state_dict(fuse))
        make = lambda: annotate.PromptAnnotator(annotate.ComponentPredictor())     # noqa: E731
        runs = {"eva_vos": dict(annotator=make, qnet=qnet, agent=agent),
                "qnet_mask": dict(qnet=qnet),
                "oracle_oracle": dict(annotator=make, annotation_types=["3clicks", "mask"])}
        with tempfile.TemporaryDirectory() as tmp:
            imset = fq_driver.make_synthetic_tree(tmp, {f"v{i}": (40, H, W, 1) for i in range(4)})
            rates, rows = {n: [] for n in runs}, {}
            for rep in range(REPS):
                for n, kw in runs.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    rows[n] = eval_driver.run(tmp, imset, "", prop.eval(), fuse.eval(), n, rounds=ROUNDS, seed=1, lanes=1, **kw)
                    rates[n].append(len(rows[n]) / (time.perf_counter() - t))
            say(f"sessions (ComponentPredictor, recipe weights), 4 videos x 40 frames at {H} x {W}, {ROUNDS} rounds each, one lane, clip decoding included:")
            for n in runs:
                say(f"   {n:14s} {np.median(rates[n]):7.2f} rounds/s (min {min(rates[n]):.2f}, max {max(rates[n]):.2f})")
            names = sorted({"3clicks", "mask", "no_object"})
            acts = [names[int(a)] for a in rows["eva_vos"][:, -2]]
            say("   eva_vos actions: " + ", ".join(f"{a} x {acts.count(a)}" for a in names))
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
