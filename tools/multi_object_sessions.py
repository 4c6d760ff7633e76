"""GPU box: annotation sessions per (video, object) against ONE session per video with all its objects (eval_driver --multi-object), and the
device time of one k-object scoring call beside k binary calls on the same maps.  Synthetic 480x854 trees of 4 videos x 40 frames with 3 and
with 5 objects; oracle policy, j_and_f, 8 rounds, one lane.  python tools/multi_object_sessions.py > profiles/multi_object_sessions.txt"""
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eva_vos_amd import _lib, eval_driver, fq_driver, metrics, synth  # noqa: E402
from eva_vos_amd.params import FusionNet, PropagationNetwork  # noqa: E402

torch.set_grad_enabled(False)
VIDEOS, T, H, W, ROUNDS, REPS = 4, 40, 480, 854, 8, 3
prop, fuse = PropagationNetwork(), FusionNet()
prop.load_state_dict(synth.recipe_state_dict(prop, 2))
fuse.load_state_dict(synth.recipe_state_dict(fuse, 2))
prop, fuse = prop.eval(), fuse.eval()
print(f"{_lib.lib().stcn_version().decode()}")
print(f"{torch.cuda.get_device_name(0)}; {VIDEOS} videos x {T} frames x {H}x{W}, oracle_mask, j_and_f, {ROUNDS} rounds, one lane; multi-object recipe (seed 2)")
p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731


def sessions(root, imset, multi):
    t0 = time.perf_counter()
    rows = eval_driver.run(root, imset, "", prop, fuse, "oracle_mask", rounds=ROUNDS, metric="j_and_f", lanes=1, multi_object=multi)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, len(rows)


def scoring_calls(root, imset, k):
    """ms of one stcn_metrics_objects_round over the whole clip against k x stcn_metrics_round (one per object, its binary maps made beforehand),
    HIP events around the calls, the two arms interleaved."""
    lab = fq_driver.ClipDataset(root, imset, per_video=True)[0]["gt"][0, :, 0].cuda()          # [T,H,W] labels
    nh, nw = H + (-H) % 16, W + (-W) % 16
    lh, lw = (nh - H) // 2, (nw - W) // 2
    masks = torch.zeros((T, nh, nw), dtype=torch.uint8, device="cuda")
    masks[:, lh:lh + H, lw:lw + W] = torch.roll(lab, (3, -4), (1, 2))                            # "the engine's labels": the objects moved a little
    annotated = torch.zeros(T, dtype=torch.uint8, device="cuda")
    annotated[[0, 20]] = 1
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # k-object arm
    sc = metrics.RoundScorer(lab, "j_and_f", max_rounds=1, no_object=20.0, num_objects=k)
    gen = torch.empty_like(lab)
    # binary arm: one scorer's buffers per object
    one = [metrics.RoundScorer(lab == o, "j_and_f", max_rounds=1, no_object=20.0) for o in range(1, k + 1)]
    masks_o = [(masks == o).to(torch.uint8).contiguous() for o in range(1, k + 1)]
    gens = [torch.empty_like(lab) for _ in range(k)]

    def labels_arm():
        _lib.check(_lib.lib().stcn_metrics_objects_round(stream, p(masks), nh, nw, lh, lw, p(sc.gt), p(annotated), p(sc.present), k, T, H, W, 0, T, 0, 20.0,
                                                         p(gen), p(sc.scratch), p(sc.counts), p(sc.object_quality[0]), p(sc.quality[0]), p(sc.select)))

    def binary_arm():
        for o in range(k):
            s = one[o]
            _lib.check(_lib.lib().stcn_metrics_round(stream, p(masks_o[o]), nh, nw, lh, lw, p(s.gt), p(annotated), p(s.noobj), T, H, W, 0, T, 0, 20.0,
                                                     p(gens[o]), p(s.scratch), p(s.counts), p(s.quality[0]), p(s.select)))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    timed(binary_arm), timed(labels_arm)                                  # warm-up
    same = all(torch.equal(sc.counts[o], one[o].counts) and torch.equal(sc.object_quality[0, o], one[o].quality[0]) for o in range(k))
    ms_b, ms_l = [], []
    for _ in range(REPS):
        ms_b.append(timed(binary_arm))
        ms_l.append(timed(labels_arm))
    return ms_b, ms_l, same


with tempfile.TemporaryDirectory() as tmp:
    for k in (3, 5):
        root = os.path.join(tmp, f"k{k}")
        imset = fq_driver.make_synthetic_tree(root, {f"v{i}": (T, H, W, k) for i in range(VIDEOS)})
        print(f"\n== k = {k} objects per video ==")
        sessions(root, imset, False), sessions(root, imset, True)        # warm-up: weights folded, pools and decode workers up
        res = {}
        for multi in (False, True, False, True):
            res.setdefault(multi, []).append(sessions(root, imset, multi))
        for multi, name in ((False, "per-object mode  "), (True, "multi-object mode")):
            walls = [w for w, _ in res[multi]]
            n = res[multi][0][1]
            print(f"{name}: {n} object-rounds, wall {', '.join(f'{w:.2f}' for w in walls)} s -> {n / min(walls):.1f} object-rounds/s (best of {len(walls)})")
        rate = {m: res[m][0][1] / min(w for w, _ in res[m]) for m in res}
        print(f"expected: the multi-object mode completes more object-rounds per second: {'MET' if rate[True] > rate[False] else 'NOT MET'} "
              f"({rate[True] / rate[False]:.2f} x)")
        ms_b, ms_l, same = scoring_calls(root, imset, k)
        spread = max(ms_b) - min(ms_b)
        print(f"scoring one round of the whole clip ({T} frames, j_and_f), device ms by HIP events, {REPS} interleaved repetitions; counts and per-object "
              f"quality of the two arms identical: {same}")
        print(f"  {k} x stcn_metrics_round       : {', '.join(f'{v:.3f}' for v in ms_b)}  (median {np.median(ms_b):.3f}, spread {spread:.3f})")
        print(f"  1 x stcn_metrics_objects_round : {', '.join(f'{v:.3f}' for v in ms_l)}  (median {np.median(ms_l):.3f})")
        print(f"expected: the k-object call is no slower than the k binary calls, within the spread of the binary arm: "
              f"{'MET' if np.median(ms_l) <= np.median(ms_b) + spread else 'NOT MET'} ({np.median(ms_l) / np.median(ms_b):.2f} x)")
