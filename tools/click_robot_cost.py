"""GPU box: what does a simulated click cost - ClickRobot.interact on the device (csrc/robot.hip behind stcn_robot_click) beside the host
restatement the reference's robot amounts to (two mask downloads, scipy.ndimage.label of both error regions, NumPy selection) - and what do
the device robots do to the rounds/s of a mixed-annotation session?

At 480 x 854, three repetitions interleaved over the mask pairs and the routes, in one process:

  (a) an ellipse pair (two frames of synth.synthetic_mask: one large false positive, one large false negative);
  (b) a late-session pair: the prediction differs from the ground truth by a few small components.

  device: ms per call from HIP events (enqueue to completion, CALLS calls back to back), and wall-clock ms per call INCLUDING the 64-byte
          record download (what a caller that needs the click on the host waits for);
  host:   wall-clock ms per call of robots.HostClickRobot.interact on the same device tensors, downloads included.

EXPECTATION (printed as the verdict, checked on the medians, no margin): the device call, record download included, is not slower than the
host route for either pair.

Then a rand_type session ('3clicks', ComponentPredictor stand-in) over a synthetic tree of 4 videos x 40 frames: rounds/s with the device
robots and with the host robots (the evaluation of a round stays on the device in both; one lane).

NOT measured here: a real SAM behind the annotator, real videos, several lanes.

python tools/click_robot_cost.py [--out profiles/click_robot.txt] [--reps 3] [--no-session]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from eva_vos_amd import _lib, annotate, eval_driver, fq_driver, robots, synth  # noqa: E402
from eva_vos_amd.params import FusionNet, PropagationNetwork  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 3
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "click_robot.txt")
H, W, CALLS = 480, 854, 20
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def spread(v):
    return f"{np.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def pairs():
    m = synth.synthetic_mask(6, H, W, 1)[0, :, 0].numpy().astype(np.uint8)
    late = m[2].copy()
    g = np.random.default_rng(3)
    ys, xs = np.nonzero(m[2])
    for i in range(6):                                             # a few small components on and beside the object's edge
        k = int(g.integers(len(ys)))
        y, x = int(ys[k]), int(xs[k])
        late[y:y + 5, x:x + 7] ^= 1
    late[40:44, 60:66] = 1
    return {"(a) ellipse pair": (m[1], m[4]), "(b) late-session pair": (late, m[2])}


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


def main():
    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    say(f"click robot at {H} x {W}, library source {_lib.src_hash()}, {torch.cuda.get_device_name(0)}; {REPS} repetitions interleaved over pairs and routes, "
        f"{CALLS} calls each")
    robot, host = robots.ClickRobot(), robots.HostClickRobot()
    data = {n: (torch.from_numpy(p).to(dev), torch.from_numpy(g).to(dev)) for n, (p, g) in pairs().items()}
    ev, dl, hs = ({n: [] for n in data} for _ in range(3))
    for n, (p, g) in data.items():                                 # warm-up, and the two routes must agree
        a, b = robot.interact(p, g), host.interact(p, g)
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist(), n
    for rep in range(REPS):
        for n, (p, g) in data.items():
            ev[n].append(events_ms(lambda: robot.interact_device(p, g), CALLS))
            dl[n].append(wall_ms(lambda: robot.interact(p, g), CALLS))
            hs[n].append(wall_ms(lambda: host.interact(p, g), CALLS))
    ok = True
    for n, (p, g) in data.items():
        rec = robots.host_click_record(p, g)[0]
        say(f"{n}: {int(rec[robots.FP_COUNT])} false-positive / {int(rec[robots.FN_COUNT])} false-negative components, largest "
            f"{int(rec[robots.FP_SIZE])} / {int(rec[robots.FN_SIZE])} pixels")
        say(f"   device, HIP events (no download)      {spread(ev[n])}")
        say(f"   device, wall clock + record download  {spread(dl[n])}")
        say(f"   host restatement, downloads included  {spread(hs[n])}")
        say(f"   device / host = {np.median(dl[n]) / np.median(hs[n]):.3f}; per repetition: " + ", ".join(f"{a / b:.3f}" for a, b in zip(dl[n], hs[n])))
        ok = ok and float(np.median(dl[n])) <= float(np.median(hs[n]))
    say()
    say("VERDICT: the device call, record download included, is " + ("not slower than the host route for either pair: AS EXPECTED" if ok
                                                                        else "SLOWER than the host route for a pair: NOT as expected"))
    if "--no-session" not in sys.argv:
        say()
        prop, fuse = PropagationNetwork(), FusionNet()
        prop.load_state_dict(synth.recipe_state_dict(prop))
        fuse.load_state_dict(synth.recipe_state_dict(fuse))
        rounds = 6
        with tempfile.TemporaryDirectory() as tmp:
            imset = fq_driver.make_synthetic_tree(tmp, {f"v{i}": (40, H, W, 1) for i in range(4)})
            makers = {"device robots": lambda: annotate.PromptAnnotator(annotate.ComponentPredictor()),
                      "host robots": lambda: annotate.PromptAnnotator.on_host(annotate.ComponentPredictor())}
            rates = {n: [] for n in makers}
            rows = {}
            for rep in range(REPS):
                for n, make in makers.items():
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    rows[n] = eval_driver.run(tmp, imset, "", prop.eval(), fuse.eval(), "rand_type", rounds=rounds, seed=1, lanes=1, annotator=make,
                                              annotation_types=["3clicks"])
                    rates[n].append(len(rows[n]) / (time.perf_counter() - t))
            same = np.array_equal(np.nan_to_num(rows["device robots"]), np.nan_to_num(rows["host robots"]))
            say(f"rand_type sessions ('3clicks', ComponentPredictor), 4 videos x 40 frames at {H} x {W}, {rounds} rounds each, one lane, clip decoding "
                f"included; rows of the two routes identical: {same}")
            for n in makers:
                say(f"   {n:14s} {np.median(rates[n]):7.2f} rounds/s (min {min(rates[n]):.2f}, max {max(rates[n]):.2f})")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
