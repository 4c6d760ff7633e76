"""Mixed-annotation sessions on the GPU: the typed round evaluation (stcn_metrics_round_typed behind metrics.TypedRoundScorer) against a
NumPy restatement of the reference's eval_processor_metric (interactions/eval.py:27-81), and the three typed policies with the device
robots against the same loop with the host robots and host scoring on a second engine.  Every comparison is exact."""
import random

import numpy as np
import pytest
import torch

from eva_vos_amd import annotate, eval_driver, metrics, synth

pytestmark = pytest.mark.gpu
NO = eval_driver.NO_OBJECT


class Proc:                                        # the attributes of an InferenceCore a scorer reads
    pass


def fake_engine(T, H, W, nh, nw, lh, lw, seed):
    rng = np.random.RandomState(seed)
    gt = synth.synthetic_mask(T, H, W, 1, seed=5)[0, :, 0] > 0.5
    gt[3] = False                                                                      # a frame without the object
    pred = (synth.synthetic_mask(T, H, W, 1, seed=6)[0, :, 0] > 0.5) ^ torch.from_numpy(rng.rand(T, H, W) < 0.02)
    annot = (synth.synthetic_mask(T, H, W, 1, seed=5)[0, :, 0] > 0.5) ^ torch.from_numpy(rng.rand(T, H, W) < 0.05)      # imperfect annotator masks
    p = Proc()
    p.nh, p.nw = nh, nw
    p.pad = (lw, nw - W - lw, lh, nh - H - lh)
    masks = torch.from_numpy(rng.randint(0, 256, (T, 1, nh, nw)).astype(np.uint8))      # garbage in the padding
    masks[:, 0, lh:lh + H, lw:lw + W] = pred.to(torch.uint8)
    p.masks = masks.cuda()
    return p, gt, annot, rng


def host_round(p, gt_h, annot_h, cur_types, metric, H, W, lh, lw):
    """eval_processor_metric (interactions/eval.py:27-81) in NumPy: the evaluated masks, their counts, the per-frame quality, the arg-min."""
    gen = p.masks[:, 0, lh:lh + H, lw:lw + W].cpu().numpy() != 0
    for t, ty in enumerate(cur_types):
        if ty == 1:
            gen[t] = gt_h[t]                                                           # :57-60
        elif ty == 2:
            gen[t] = annot_h[t]                                                        # :61-64
    T = len(gt_h)
    jf = np.array([(metrics.jaccard(gt_h[t], gen[t]), metrics.f_measure(gt_h[t], gen[t])) for t in range(T)], np.float64)
    q = jf[:, 0].copy() if metric == "j" else 0.5 * (jf[:, 0] + jf[:, 1])
    q[gt_h.reshape(T, -1).sum(1) == 0] = NO                                            # :66-69
    return gen.astype(np.uint8), metrics.label_counts(gt_h, gen, 1)[0], q, int(np.argmin(q))


# every annotation so far with repeats, and the type of each: frame 4 goes 2 -> 2 (round 4) and 2 -> 1 (round 5), frame 3 has no object
SCRIPT = (([0], [1]), ([0, 4], [1, 2]), ([0, 4, 2], [1, 2, 2]), ([0, 4, 2, 4], [1, 2, 2, 2]), ([0, 4, 2, 4, 4], [1, 2, 2, 2, 1]),
          ([0, 4, 2, 4, 4, 3], [1, 2, 2, 2, 1, 2]))


def windows(frames, T):
    cur, others = frames[-1], set(frames[:-1]) - {frames[-1]}
    return max([f for f in others if f < cur] + [-1]) + 1, min([f for f in others if f > cur] + [T])


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
def test_the_typed_round_equals_the_numpy_restatement_of_the_references_evaluation(metric):
    T, H, W, lh, lw = 6, 37, 53, 5, 5
    p, gt, annot, rng = fake_engine(T, H, W, 48, 64, lh, lw, 7)
    gt_h, annot_h = gt.numpy(), annot.numpy().copy()
    sc = metrics.TypedRoundScorer(gt.cuda(), metric, max_rounds=len(SCRIPT), no_object=NO)
    seen_types = set()
    for r, (frames, types) in enumerate(SCRIPT):
        t0, t1 = windows(frames, T) if r else (0, T)
        if r:                                                                          # what a propagation round may change
            p.masks[t0:t1, 0, lh:lh + H, lw:lw + W] ^= torch.from_numpy(rng.rand(t1 - t0, H, W) < 0.01).to(torch.uint8).cuda()
        if types[-1] == 2:
            if r == 3:                                                                 # 2 -> 2: another annotator mask for the same frame
                annot_h[frames[-1]] ^= rng.rand(H, W) < 0.03
            sc.set_annotation(frames[-1], torch.from_numpy(annot_h[frames[-1]]).cuda())
        sel, gen = sc.score(p, frames, types=types)
        cur = metrics._current_types(T, frames, types)
        seen_types |= set(cur.tolist())
        gen_h, counts, q_ref, sel_ref = host_round(p, gt_h, annot_h, cur, metric, H, W, lh, lw)
        assert np.array_equal(gen.cpu().numpy(), gen_h), r
        got = sc.counts.cpu().numpy()
        print(r, metric, "counts", got.tolist(), "host", counts.tolist())
        assert np.array_equal(got[:, :2], counts[:, :2]) and (np.array_equal(got, counts) if metric != "j" else not got[:, 2:].any()), r
        q = sc.qualities()[r]
        print(r, metric, "quality", q.tolist(), "host", q_ref.tolist(), "selected", sel)
        assert q.dtype == np.float64 and np.array_equal(q.view(np.uint64), q_ref.view(np.uint64)), (r, q, q_ref)
        assert sel == sel_ref, (r, sel, sel_ref)
    assert seen_types == {0, 1, 2}
    q = sc.qualities()
    assert q[3][4] != q[2][4] and q[3][4] < 1.0 and q[4][4] == 1.0 and q[5][3] == NO      # 2 -> 2 changed the frame's value, 2 -> 1 made it 1


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
def test_without_a_type_2_frame_the_typed_round_is_the_round_bit_for_bit(metric):
    T, H, W, lh, lw = 6, 37, 53, 5, 5
    p, gt, annot, rng = fake_engine(T, H, W, 48, 64, lh, lw, 9)
    typed = metrics.TypedRoundScorer(gt.cuda(), metric, max_rounds=4, no_object=NO)
    plain = metrics.RoundScorer(gt.cuda(), metric, max_rounds=4, no_object=NO)
    typed.annot.fill_(1)                                                               # never read
    for r, frames in enumerate(([0], [0, 4], [0, 4, 2])):
        if r:
            t0, t1 = windows(frames, T)
            p.masks[t0:t1, 0, lh:lh + H, lw:lw + W] ^= torch.from_numpy(rng.rand(t1 - t0, H, W) < 0.01).to(torch.uint8).cuda()
        a, b = typed.score(p, frames, types=[1] * len(frames)), plain.score(p, frames)
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(typed.counts, plain.counts)
    assert np.array_equal(typed.qualities().view(np.uint64), plain.qualities().view(np.uint64))
    with pytest.raises(ValueError):
        plain.score(p, [0], types=[1])
    with pytest.raises(ValueError):
        typed.score(p, [0])
    with pytest.raises(RuntimeError):
        typed.score_trial(p, [0, 4, 2], 1, 0)


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
def test_the_incremental_typed_round_equals_a_full_recompute(metric):
    T, H, W, lh, lw = 6, 37, 53, 5, 5
    p, gt, annot, rng = fake_engine(T, H, W, 48, 64, lh, lw, 11)
    annot_h = annot.numpy().copy()
    inc = metrics.TypedRoundScorer(gt.cuda(), metric, max_rounds=len(SCRIPT), no_object=NO)
    full = metrics.TypedRoundScorer(gt.cuda(), metric, max_rounds=len(SCRIPT), no_object=NO)
    for r, (frames, types) in enumerate(SCRIPT):
        if r:
            t0, t1 = windows(frames, T)
            p.masks[t0:t1, 0, lh:lh + H, lw:lw + W] ^= torch.from_numpy(rng.rand(t1 - t0, H, W) < 0.01).to(torch.uint8).cuda()
        if types[-1] == 2:
            annot_h[frames[-1]] ^= rng.rand(H, W) < 0.03
            for sc in (inc, full):
                sc.set_annotation(frames[-1], torch.from_numpy(annot_h[frames[-1]]).cuda())
        a, b = inc.score(p, frames, types=types), full.score(p, frames, types=types, incremental=False)
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(inc.counts, full.counts), r
    assert np.array_equal(inc.qualities().view(np.uint64), full.qualities().view(np.uint64))


# ------------------------------------------------------------------------------------------------ sessions
T, H, W, ROUNDS = 12, 96, 128, 6
SESSIONS = {"rand_type": ["bbox"], "rand_rand": ["3clicks", "mask"], "oracle_oracle": ["3clicks", "mask"]}


def sample():
    gt = synth.synthetic_mask(T, H, W, 1)
    gt[0, T - 1] = 0                                               # one frame without the object: 3 s, and an empty annotator mask
    return {"rgb": synth.synthetic_clip(T, H, W), "gt": gt, "num_frames": T, "name": "syn__1", "video": "syn"}


def simulate_draws(policy, types, seed):
    """The frames and actions the random policies draw, from the session's rng alone (no masks involved): the order of the draws is
    action (rand_rand), then the next frame among those without a mask."""
    rng = random.Random(seed)
    kind = np.zeros(T, int)
    kind[0] = 1
    frames, actions = [0], ["mask"]
    for r in range(2, ROUNDS + 2):
        left = np.where(kind != 1)[0].tolist()
        if not left:
            break
        f = int(rng.choice(left))
        if r > ROUNDS:
            break
        a = types[0] if policy == "rand_type" else rng.choice(types)
        frames.append(f)
        actions.append(a)
        kind[f] = 1 if a == "mask" else 2
    return frames, actions


def choose_seed(policy, types):
    """Chosen on the CPU, before any session runs, from the draws alone: for rand_rand the first seed that annotates some frame twice, the
    first time without a mask; for rand_type with a box the first seed WITHOUT a repeat - a second box on a frame is where the reference's
    own loop asserts (annotator.py:252), and so does the restatement."""
    for seed in range(200):
        frames, actions = simulate_draws(policy, types, seed)
        first, repeat = {}, False
        for i, f in enumerate(frames[:ROUNDS]):
            repeat = repeat or (f in first and actions[first[f]] != "mask")
            first.setdefault(f, i)
        if repeat == (policy == "rand_rand"):
            return seed, frames, actions
    raise AssertionError("no seed found")


@pytest.fixture(scope="module")
def sessions(weights):
    """Every policy once on the device route and once on the host route (host robots, host scoring, a second engine).  A 96 x 128 frame has
    6 x 8 = 48 keys, fewer than the default cut of 50, so the networks are built with top_k = 20 (the cut of STCN checkpoints)."""
    from eva_vos_amd.params import FusionNet, PropagationNetwork
    from mivos.inference_core import InferenceCore
    nets = PropagationNetwork(top_k=20), FusionNet()
    nets[0].load_state_dict(weights[0], strict=True)
    nets[1].load_state_dict(weights[1], strict=True)
    s = sample()
    out = {}
    for policy, types in SESSIONS.items():
        seed, frames, actions = choose_seed(policy, types) if policy != "oracle_oracle" else (0, None, None)
        routes = {}
        for route in ("device", "host"):
            proc = InferenceCore(nets[0], nets[1], s["rgb"].cuda(), 1)
            gt_thw = s["gt"][0, :, 0].cuda()
            if route == "device":
                ann, sc = annotate.PromptAnnotator(annotate.ComponentPredictor()), metrics.TypedRoundScorer(gt_thw, "j_and_f", max_rounds=ROUNDS, no_object=NO)
            else:
                ann, sc = annotate.PromptAnnotator.on_host(annotate.ComponentPredictor()), metrics.HostTypedScorer(gt_thw, "j_and_f", max_rounds=ROUNDS, no_object=NO)
            res = eval_driver.run_typed_policy(policy, proc, s, ROUNDS, ann, types, "j_and_f", random.Random(seed), scorer=sc)
            routes[route] = (res, sc, proc.prob.clone(), ann)
        out[policy] = (routes, frames, actions)
    return s, out


@pytest.mark.parametrize("policy", list(SESSIONS))
def test_the_device_session_equals_the_host_session(sessions, policy):
    s, out = sessions
    routes, frames, actions = out[policy]
    (dev, dsc, dprob, dann), (host, hsc, hprob, hann) = routes["device"], routes["host"]
    assert len(dev["mu_metrics"]) == ROUNDS
    for key in ("annotated_frames", "annotations_actions", "annotation_times", "types"):
        assert dev[key] == host[key], key
    assert np.array_equal(np.stack(dev["round_metrics"]).view(np.uint64), np.stack(host["round_metrics"]).view(np.uint64))
    assert dev["mu_metrics"] == host["mu_metrics"]
    assert torch.equal(dprob, hprob)
    assert np.array_equal(dsc.annot.cpu().numpy(), hsc.annot) and np.array_equal(dsc.counts.cpu().numpy(), hsc.counts)
    assert dann.robot_calls == hann.robot_calls > 0
    assert dev["annotated_frames"][0] == 0 and dev["annotations_actions"][0] == "mask" and dev["annotation_times"][0] == 80
    assert set(dev["annotations_actions"]) <= set(SESSIONS[policy]) | {"mask"}
    if frames is not None:                                         # the random policies draw what the rng alone says
        assert dev["annotated_frames"] == frames[:ROUNDS] and dev["annotations_actions"] == actions[:ROUNDS]
    if policy == "oracle_oracle":
        assert len(dev["action_data"]) == ROUNDS - 1 and all(d["selected_action"] in SESSIONS[policy] for d in dev["action_data"])
        for r in range(1, ROUNDS):                                 # the next frame is the worst of the round before
            assert dev["annotated_frames"][r] == int(np.argmin(dev["round_metrics"][r - 1]))


def test_a_frame_is_annotated_again_and_a_type_2_frame_counts_with_its_annotator_mask(sessions):
    s, out = sessions
    gt = s["gt"][0, :, 0].numpy() > 0.5
    repeats = masks_used = 0
    for policy, (routes, _, _) in out.items():
        res, sc, _, _ = routes["device"]
        fr = res["annotated_frames"]
        repeats += len(fr) - len(set(fr))
        cur = metrics._current_types(T, fr, res["types"])
        gen = sc._gen.cpu().numpy()
        annot = sc.annot.cpu().numpy()
        for t in np.where(cur == 2)[0]:
            assert np.array_equal(gen[t], annot[t])
            masks_used += bool((annot[t] != gt[t]).any())          # evaluated with the annotator's mask, which is not the ground truth
        for t in np.where(cur == 1)[0]:
            assert np.array_equal(gen[t], gt[t])
    assert repeats >= 1 and masks_used >= 1


def test_a_second_box_on_a_frame_is_refused_as_in_the_reference():
    gt = torch.zeros((40, 50), dtype=torch.uint8, device="cuda")
    gt[8:25, 10:34] = 1
    a = annotate.PromptAnnotator(annotate.ComponentPredictor())
    mask, cost, iou, logits, clicks, labels, bbox = a.annotate("bbox", gt)
    assert cost == 7 and bbox.tolist() == [[10.0, 8.0, 33.0, 24.0]]
    with pytest.raises(AssertionError, match="box"):
        a.annotate("bbox", gt, None, mask, dict(sam_logits=logits, click_coords=clicks, click_labels=labels, bbox=bbox))


def test_the_costs_are_the_references():
    assert annotate.ANNOTATION_COSTS == {"no_object": 3, "mask": 80, "click": 1.5, "3clicks": 4.5, "bbox": 7, "click_overhead": 1, "stop": 0}
    assert annotate.annotator_input("3clicks") == ("click", 3) and annotate.annotator_input("bbox") == ("bbox", 1)
    with pytest.raises(AttributeError):
        annotate.annotator_input("scribble")
