"""The ``eva_vos`` policy on the GPU: the mask-resize kernel (stcn_masks_resize_nearest behind agent.masks_to_224) against ``F.interpolate`` and
against the NumPy statement of torch's nearest rule, ``QNetSelector`` against ``qnet_frame_selection``, the policy end to end through
``eval_driver.run``, and the device route of a session against the host route.  The mask comparisons are exact."""
import csv

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eva_vos_amd import agent as A
from eva_vos_amd import annotate, eval_driver, fq_driver, metrics, synth
from eva_vos_amd import qnet as Q

pytestmark = pytest.mark.gpu
NO = eval_driver.NO_OBJECT


# ------------------------------------------------------------------------------------------------ masks_to_224
def _bytes(T, H, W, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (T, H, W)).astype(np.uint8))


def _numpy_nearest(x, oh, ow):
    """min((int)floorf(dst * ((float)in / out)), in - 1) per axis, in fp32."""
    H, W = x.shape[-2:]
    sy = np.minimum(np.floor(np.arange(oh, dtype=np.float32) * (np.float32(H) / np.float32(oh))).astype(np.int64), H - 1)
    sx = np.minimum(np.floor(np.arange(ow, dtype=np.float32) * (np.float32(W) / np.float32(ow))).astype(np.int64), W - 1)
    return x[:, sy][:, :, sx].astype(np.float32)


# (T,H,W), frames, size, channels: 480p; one axis up, one down; tiny; just above 224; a gather out of order; a run of frames (a view, no index);
# another output size with one channel; a plane that is no multiple of four (the scalar stores)
RESIZES = [((3, 480, 854), None, 224, 3), ((2, 100, 150), None, 224, 3), ((1, 7, 5), None, 224, 3), ((2, 225, 223), None, 224, 3),
           ((4, 48, 64), [3, 0], 224, 3), ((4, 48, 64), [1, 2], 224, 3), ((3, 480, 854), None, (16, 24), 1), ((2, 100, 150), [1, 0, 1], (7, 9), 2)]


@pytest.mark.parametrize("shape,frames,size,channels", RESIZES)
def test_masks_to_224_equals_interpolate_and_the_index_rule(shape, frames, size, channels):
    x = _bytes(*shape, seed=sum(shape))
    assert int(x.min()) == 0 and int(x.max()) == 255 or x.numel() < 2000
    xd = x.cuda()
    out = A.masks_to_224(xd, frames, size, channels)
    oh, ow = (size, size) if isinstance(size, int) else size
    taken = xd if frames is None else xd[torch.as_tensor(frames, device="cuda")]
    ref = F.interpolate(taken[:, None].float(), (oh, ow), mode="nearest").expand(-1, channels, -1, -1)
    assert out.shape == ref.shape == (len(taken), channels, oh, ow) and out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out, ref)
    assert torch.equal(out, A.masks_to_224_torch(xd, frames, size, channels))
    rule = _numpy_nearest(taken.cpu().numpy(), oh, ow)
    assert np.array_equal(out.cpu().numpy(), np.broadcast_to(rule[:, None], out.shape))


def test_masks_to_224_refuses_frames_outside_the_clip():
    x = _bytes(2, 8, 8, 1).cuda()
    for frames in ([2], [-1, 0], []):
        with pytest.raises(ValueError, match="frames"):
            A.masks_to_224(x, frames)


# ------------------------------------------------------------------------------------------------ QNetSelector
@pytest.fixture(scope="module")
def qnet():
    net = Q.QualityNet()
    net.load_state_dict(synth.recipe_state_dict(net, seed=3))
    return net.cuda().eval()


def test_the_selector_with_cached_frame_features_selects_what_qnet_frame_selection_selects(qnet):
    T, H, W = 9, 100, 150
    frames = synth.synthetic_clip(T, H, W)[0].cuda()
    sel = Q.QNetSelector(qnet, frames)
    for seed, inter in ((1, [0]), (2, [0, 4]), (3, [2, 3, 8, 3])):
        gen = (_bytes(T, H, W, seed) > 127).to(torch.uint8).cuda()
        with torch.no_grad():
            feats = qnet.extract_features(*Q.to_224(frames, gen.float()))
        got = sel.features(gen)
        scale = float(feats.abs().max())
        print("features: max difference", float((got - feats).abs().max()), "scale", scale)
        assert got.shape == feats.shape == (T, 1024) and float((got - feats).abs().max()) <= 1e-5 * scale
        assert sel.select(gen, inter) == Q.qnet_frame_selection(qnet, frames, gen.float(), inter)


def test_the_selector_refuses_a_qnet_in_training_mode(qnet):
    frames = synth.synthetic_clip(2, 64, 64)[0].cuda()
    net = Q.QualityNet().cuda()
    assert net.training
    with pytest.raises(ValueError, match="eval"):
        Q.QNetSelector(net, frames)
    sel = Q.QNetSelector(net.eval(), frames)
    net.train()
    with pytest.raises(ValueError, match="training"):
        sel.select(torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda"), [0])


# ------------------------------------------------------------------------------------------------ the policy
def recipe_agent():
    return A.PPOAgent(state_dict=synth.recipe_state_dict(A.ActorCritic(), seed=5))


def test_eva_vos_end_to_end_through_the_driver(nets, qnet, tmp_path):
    imset = fq_driver.make_synthetic_tree(str(tmp_path / "db"), {"v0": (6, 112, 128, 2), "v1": (5, 112, 128, 1)})
    agent = recipe_agent()
    names = sorted({"3clicks", "mask", "no_object"})
    out = str(tmp_path / "eva_vos.csv")
    stats = {}
    rows = eval_driver.run(str(tmp_path / "db"), imset, out, nets[0], nets[1], "eva_vos", rounds=4, annotator="component", qnet=qnet, agent=agent, seed=4,
                           stats=stats)
    # the costs asked of this run: 80 (mask), 3 (no object), 3 x 1.5.  The recipe agent's logits lie some 50 apart, it asks for a mask every
    # time; where clicks are really given (the two-route session below) three clicks cost 3 x 1.5 + 1 s of overhead or more, as the reference's
    assert rows.shape[1] == 6 + 6 + 2 and set(rows[:, 0].astype(int)) == {0, 1, 2} and len(rows) == 3 * 4
    for row in rows:
        n = int(row[5])
        q = row[6:6 + n]
        assert np.all(((q >= 0) & (q <= 1)) | (q == NO)) and np.isnan(row[6 + n:-2]).all() and 0 <= row[2] <= 1
        assert names[int(row[-2])] in names and row[3] in (80, 3, 3 * 1.5)
        if row[1] == 0:
            assert names[int(row[-2])] == "mask" and row[3] == 80 and row[-1] == -2 and row[4] == 0
        else:
            assert np.isfinite(row[-1]) and row[-1] != -2
    with open(out) as f:
        lines = list(csv.reader(f))
    print(lines)
    assert lines[0] == ["video", "mu_metric", "annotation_time", "round", "rl_values", "annotation_actions"] and len(lines) == 1 + len(rows)
    assert lines[1][0] == "v0__1" and lines[1][2:] == ["80.0", "0", "-2.0", "mask"]
    assert all(ln[5] in names and float(ln[2]) in (80, 3, 4.5) for ln in lines[1:])
    again = eval_driver.run(str(tmp_path / "db"), imset, "", nets[0], nets[1], "eva_vos", rounds=4, annotator="component", qnet=qnet, agent=agent, seed=4)
    assert np.array_equal(np.nan_to_num(again), np.nan_to_num(rows))
    other = eval_driver.run(str(tmp_path / "db"), imset, "", nets[0], nets[1], "eva_vos", rounds=4, annotator="component", qnet=qnet, agent=agent, seed=5,
                            lanes=1)
    assert other.shape == rows.shape


# the session of the two routes: a frame without the object, fewer keys than the default cut of 50 (so top_k = 20, as in test_gpu_typed_sessions)
T, H, W, ROUNDS = 12, 96, 128, 7


def _sample():
    gt = synth.synthetic_mask(T, H, W, 1)
    gt[0, T - 1] = 0
    return {"rgb": synth.synthetic_clip(T, H, W), "gt": gt, "num_frames": T, "name": "syn__1", "video": "syn"}


def _even_agent():
    """The recipe agent with its policy head zeroed: both actions at probability 1/2, so the actions of a session are the generator's draws
    alone (the recipe's own logits are some 25 apart: one action, always).  Value head and trunk stay the recipe's."""
    agent = recipe_agent()
    with torch.no_grad():
        agent.ac_net.policy.weight.zero_()
        agent.ac_net.policy.bias.zero_()
    return agent


def _draws(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [int(torch.multinomial(torch.tensor([0.5, 0.5], dtype=torch.float64), 1, generator=g).item()) for _ in range(n)]


def _seed_with_both_actions():
    """Chosen on the CPU from the draws alone: the first seed whose first draws ask for clicks twice running and then for a mask."""
    for seed in range(200):
        d = _draws(seed, ROUNDS - 1)
        if d[:2] == [0, 0] and 1 in d[2:]:
            return seed
    raise AssertionError("no seed found")


def test_the_device_route_of_a_session_equals_the_host_route(weights, qnet):
    from eva_vos_amd.params import FusionNet, PropagationNetwork
    from mivos.inference_core import InferenceCore
    nets = PropagationNetwork(top_k=20), FusionNet()
    nets[0].load_state_dict(weights[0], strict=True)
    nets[1].load_state_dict(weights[1], strict=True)
    s, agent, seed = _sample(), _even_agent(), _seed_with_both_actions()
    res = {}
    for route in ("device", "host"):
        proc = InferenceCore(nets[0], nets[1], s["rgb"].cuda(), 1)
        gt_thw = s["gt"][0, :, 0].cuda()
        if route == "device":
            ann, sc, sel = annotate.PromptAnnotator(annotate.ComponentPredictor()), None, None
        else:
            ann = annotate.PromptAnnotator.on_host(annotate.ComponentPredictor())
            sc = metrics.HostTypedScorer(gt_thw, "j_and_f", max_rounds=ROUNDS, no_object=NO)
            sel = Q.QNetSelector(qnet, s["rgb"][0].cuda(), masks_to_input=A.masks_to_224_torch)
        res[route] = eval_driver.run_eva_vos(proc, s, ROUNDS, ann, qnet, agent, "j_and_f", torch.Generator().manual_seed(seed), scorer=sc, selector=sel)
    dev, host = res["device"], res["host"]
    print("frames", dev["annotated_frames"], "actions", dev["annotations_actions"], "costs", dev["annotation_times"], "values", dev["rl_values"])
    for key in ("annotated_frames", "annotations_actions", "annotation_times", "rl_values", "types", "mu_metrics"):
        assert dev[key] == host[key], key
    assert np.array_equal(np.stack(dev["round_metrics"]).view(np.uint64), np.stack(host["round_metrics"]).view(np.uint64))
    assert len(dev["mu_metrics"]) == ROUNDS and dev["rl_values"][0] == -2 and len(dev["rl_values"]) == ROUNDS
    assert dev["annotated_frames"][0] == 0 and dev["annotations_actions"][0] == "mask" and dev["annotation_times"][0] == 80
    # the actions are the generator's draws, in order, wherever the agent was asked (a frame without the object asks nobody)
    asked = [a for a in dev["annotations_actions"][1:] if a != "no_object"]
    assert asked == [A.AVAIL_ACTIONS[d] for d in _draws(seed, len(asked))] and {"3clicks", "mask"} <= set(asked)
    for a, c, v in zip(dev["annotations_actions"][1:], dev["annotation_times"][1:], dev["rl_values"][1:]):
        # three prompts of one or two clicks at 1.5 s each, plus the click overhead of 1 s (annotator/annotator.py:197-244)
        assert (c == {"mask": 80, "no_object": 3}[a]) if a != "3clicks" else 3 * 1.5 + 1 <= c <= 3 * 2 * 1.5 + 1
        assert (v == 0) == (a == "no_object")
