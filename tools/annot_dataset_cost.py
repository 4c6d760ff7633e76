"""GPU box: does the export kernel of the annotation-type dataset earn its place - and what do the exports cost a session?

On one MI355X at 480 x 854, three repetitions interleaved over what is compared, in one process:

  frames_to_rgb8 : the kernel (stcn_frames_to_rgb8: three launches for all n frames) beside the torch route over the same clip - ``amin``, ``amax``,
                   subtract, divide, multiply, ``.to(uint8)``, permute made contiguous - at n = 1 (one frame, a view) and n = 9 (the rows of a
                   10-round session: frames out of order, with repeats; both routes upload the index); ms per call from HIP events over
                   calls back to back;

  sessions       : rounds/s of ``annot_driver.run`` beside ``eval_driver.run --policy oracle_oracle --annotation-types 3clicks mask --metric j`` -
                   the same session without the exports (and with the not_avail_frames skip, without the stop at a perfect round) - on the synthetic
                   tree of profiles/click_robot.txt (4 videos x 40 frames, one lane, 10 rounds, ``ComponentPredictor``, recipe weights), clip
                   decoding and, for the dataset driver, the PNG / .npy writers included.  The ratio is reported, not gated.

KEEP-OR-DROP RULE for the kernel (stated before measuring; printed as the verdict, checked on the medians, no margin): it stays only if it is
not slower than the torch route at both n.

NOT measured here: a real SAM behind the annotator (its encoder pass per row), real videos, several lanes, several ranks.

python tools/annot_dataset_cost.py [--out profiles/annot_dataset.txt] [--reps 3] [--no-session]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from eva_vos_amd import _lib, annot_driver, annotate, eval_driver, fq_driver, synth  # noqa: E402
from eva_vos_amd.params import FusionNet, PropagationNetwork  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "annot_dataset.txt")
H, W, T, CALLS, ROUNDS = 480, 854, 40, 1000, 10
FRAMES = {1: [7], 9: [12, 12, 31, 5, 5, 22, 38, 17, 17]}
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return f"{np.median(v):8.4f} ms (min {min(v):.4f}, max {max(v):.4f})"


def events_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def frames_to_rgb8_torch(clip, frames):
    """The torch route over the same clip: amin, amax, subtract, divide, multiply, ``.to(uint8)``, permute made contiguous; a run of frames
    is a view here too, other lists upload their index as the kernel's wrapper does."""
    if frames == list(range(frames[0], frames[0] + len(frames))):
        x = clip[frames[0]:frames[0] + len(frames)]
    else:
        x = clip[torch.tensor(frames, dtype=torch.long).to(clip.device, non_blocking=True)]
    lo, hi = x.amin((1, 2, 3), keepdim=True), x.amax((1, 2, 3), keepdim=True)
    return ((x - lo) / (hi - lo).clamp_min(1e-8) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    say(f"annotation-type dataset at {H} x {W}, library source {_lib.src_hash()}, {torch.cuda.get_device_name(0)}; {REPS} repetitions interleaved, "
        f"{CALLS} calls each")
    clip = synth.synthetic_clip(T, H, W)[0].to(dev)
    ok = True
    for n, frames in FRAMES.items():
        got, ref = annot_driver.frames_to_rgb8(clip, frames), frames_to_rgb8_torch(clip, frames)       # warm-up
        host = torch.from_numpy(annot_driver.frames_to_rgb8_host(clip, frames))
        assert torch.equal(got.cpu(), host)
        differ = int((ref.cpu() != host).sum())                   # torch's division is not the IEEE one everywhere: said, not asserted
        k, t = [], []
        for rep in range(REPS):
            k.append(events_ms(lambda: annot_driver.frames_to_rgb8(clip, frames), CALLS))
            t.append(events_ms(lambda: frames_to_rgb8_torch(clip, frames), CALLS))
        say(f"frames_to_rgb8, n = {n}: fp32 [{T},3,{H},{W}], frames {frames} -> uint8 [{n},{H},{W},3]")
        say(f"   kernel (three launches)                               {spread(k)}")
        say(f"   torch (amin, amax, -, /, *, .to(uint8), permute copy) {spread(t)}   bytes that differ from the host statement: {differ}")
        say(f"   kernel / torch = {np.median(k) / np.median(t):.3f}; per repetition: " + ", ".join(f"{a / b:.3f}" for a, b in zip(k, t)))
        ok = ok and float(np.median(k)) <= float(np.median(t))
    say()
    say("VERDICT (keep-or-drop rule): the kernel is " + ("not slower than the torch route at both n: it STAYS" if ok
                                                         else "SLOWER than the torch route at an n: it is to be TAKEN OUT (the driver exports on the torch route)"))
    if "--no-session" not in sys.argv:
        say()
        prop, fuse = PropagationNetwork(), FusionNet()
        prop.load_state_dict(synth.recipe_state_dict(prop))
        fuse.load_state_dict(synth.recipe_state_dict(fuse))
        prop, fuse = prop.eval(), fuse.eval()
        make = lambda: annotate.PromptAnnotator(annotate.ComponentPredictor())     # noqa: E731
        types_ = ["3clicks", "mask"]
        with tempfile.TemporaryDirectory() as tmp:
            imset = fq_driver.make_synthetic_tree(os.path.join(tmp, "db"), {f"v{i}": (T, H, W, 1) for i in range(4)})
            root = os.path.join(tmp, "db")

            def dataset(stats, rep):
                annot_driver.run(root, imset, os.path.join(tmp, f"annot_{rep}"), prop, fuse, rounds=ROUNDS, annotator=make, annotation_types=types_, lanes=1, stats=stats)

            def oracle(stats, rep):
                eval_driver.run(root, imset, "", prop, fuse, "oracle_oracle", rounds=ROUNDS, metric="j", lanes=1, stats=stats, annotator=make, annotation_types=types_)

            runs = {"annot_driver": dataset, "oracle_oracle": oracle}
            rates, rounds_run = {n: [] for n in runs}, {}
            for rep in range(REPS):
                for name, fn in runs.items():
                    stats = {}
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fn(stats, rep)
                    torch.cuda.synchronize()
                    rates[name].append(stats["interactions"] / (time.perf_counter() - t))
                    rounds_run[name] = stats["interactions"]
            say(f"sessions (ComponentPredictor, recipe weights), 4 videos x {T} frames at {H} x {W}, {ROUNDS} rounds each, one lane, clip decoding included:")
            for name in runs:
                say(f"   {name:14s} {np.median(rates[name]):7.2f} rounds/s (min {min(rates[name]):.2f}, max {max(rates[name]):.2f}), {rounds_run[name]} rounds run")
            say(f"   annot_driver / oracle_oracle = {np.median(rates['annot_driver']) / np.median(rates['oracle_oracle']):.3f} (reported, not gated): "
                "per row one image, one mask and one 4 MB embedding leave the device and are written by host threads")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
