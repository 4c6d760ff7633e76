"""CPU: the pieces of the ``eva_vos`` policy that need no GPU - the actor-critic container against the golden of the reference's module, the
agent's draws, the argument checks of ``stcn_masks_resize_nearest``, the stand-in image embedding, and the session loop against a literal
restatement of the reference's ``eva_vos`` (interactions/mulitple_annotations.py:286-378) on fakes that record every call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from eva_vos_amd import _lib, annotate, eval_driver, fq_driver, sessions, synth
from eva_vos_amd import agent as A
from session_fakes import Agent, Annotator, Proc, Scorer, Selector
from session_fakes import clip as _clip, gen_masks as _gen, quality as _quality

GOLD = os.path.join(os.path.dirname(__file__), "golden", "agent.npz")
NO = fq_driver.NO_OBJECT


def _inputs(n=3, seed=13):          # same stream as tools/gen_golden_agent.py
    g = np.random.Generator(np.random.Philox(key=[seed, 256]))
    emb = torch.from_numpy(g.normal(0, 1, (n, 256, 64, 64)).astype(np.float32))
    msk = torch.from_numpy((g.uniform(0, 1, (n, 1, 224, 224)) > 0.6).astype(np.float32)).expand(-1, 3, -1, -1)
    return emb, msk.contiguous()


# ------------------------------------------------------------------------------------------------ the agent
def test_actor_critic_state_dict_and_outputs_match_the_reference_golden():
    gold = np.load(GOLD)
    net = A.ActorCritic().eval()
    sd = net.state_dict()
    assert list(sd.keys()) == gold["names"].tolist() and len(sd) == 126
    assert [",".join(map(str, v.shape)) for v in sd.values()] == gold["shapes"].tolist()
    assert {k.split(".")[0] for k in sd} == {"mask_branch", "embed_branch", "policy", "value"} and "embed_branch.2.weight" in sd
    net.load_state_dict(synth.recipe_state_dict(net, seed=5), strict=True)
    with torch.no_grad():
        logits, value = net(*_inputs())
    scale = max(np.abs(gold["logits"]).max(), np.abs(gold["value"]).max())
    print("logits", logits.tolist(), "value", value.flatten().tolist(), "scale", scale)
    assert logits.shape == (3, 2) and value.shape == (3, 1)
    assert np.abs(logits.numpy() - gold["logits"]).max() <= 1e-5 * scale          # fp32, same ops: thread-count noise only
    assert np.abs(value.numpy() - gold["value"]).max() <= 1e-5 * scale


def test_actor_critic_refuses_what_is_not_built():
    with pytest.raises(ValueError, match="resnet18"):
        A.ActorCritic(arch="vit_b_16")
    with pytest.raises(ValueError, match="use_cost=False"):
        A.ActorCritic(use_cost=True)


def _agent_with_logits(lo, hi, **kw):
    ag = A.PPOAgent(device="cpu", **kw)
    with torch.no_grad():
        ag.ac_net.policy.weight.zero_()
        ag.ac_net.policy.bias.copy_(torch.tensor([lo, hi]))
    return ag


def test_the_agent_draws_from_the_generator_it_is_given():
    emb, msk = torch.zeros((1, 256, 4, 4)), torch.zeros((1, 3, 224, 224))
    ag = _agent_with_logits(0.0, 0.0)
    assert not ag.ac_net.training
    draws = []
    for _ in range(2):
        g = torch.Generator().manual_seed(7 * 100003 + 2)
        draws.append([ag.act(emb, msk, generator=g)[0] for _ in range(24)])
    assert draws[0] == draws[1] and set(draws[0]) == {0, 1}                        # reproducible, and really drawn
    g = torch.Generator().manual_seed(1)
    assert {_agent_with_logits(50.0, -50.0).act(emb, msk, generator=g)[0] for _ in range(8)} == {0}
    assert {_agent_with_logits(-50.0, 50.0).act(emb, msk, generator=g)[0] for _ in range(8)} == {1}
    action, value = ag.act(emb, msk, generator=g)
    assert isinstance(action, int) and value.shape == (1, 1)
    logits, value = _agent_with_logits(-50.0, 50.0, return_logits=True).act(emb, msk)
    assert logits.tolist() == [[-50.0, 50.0]] and value.shape == (1, 1)


def test_the_agent_loads_weights_strictly():
    sd = synth.recipe_state_dict(A.ActorCritic(), seed=5)
    ag = A.PPOAgent(state_dict=sd, device="cpu")
    assert torch.equal(ag.ac_net.value.weight, sd["value.weight"])
    with pytest.raises(RuntimeError):
        A.PPOAgent(state_dict={k: v for k, v in sd.items() if k != "value.bias"}, device="cpu")


# ------------------------------------------------------------------------------------------------ the policy list, the C ABI
def test_the_agent_policies_are_their_own_tuple():
    assert eval_driver.AGENT_POLICIES == ("eva_vos",)
    assert not set(eval_driver.AGENT_POLICIES) & (set(eval_driver.POLICIES) | set(eval_driver.TYPED_POLICIES))


def _refused(rc, *needles):
    assert rc == -1                                            # STCN_E_INVALID
    msg = _lib.lib().stcn_last_error().decode()
    for n in needles:
        assert n in msg, msg


BUF = (C.c_uint8 * 64)()
PTR = C.cast(BUF, C.c_void_p)           # never dereferenced: every call below is refused on the host


def test_the_resize_entry_is_declared_exported_and_checks_its_arguments_without_a_gpu():
    assert "stcn_masks_resize_nearest" in _lib.PROTOTYPES
    fn = getattr(_lib.lib(), "stcn_masks_resize_nearest")
    who = "stcn_masks_resize_nearest"
    _refused(fn(None, None, 2, 4, 4, None, 2, 224, 224, 3, PTR), who, "null", "src")
    _refused(fn(None, PTR, 2, 4, 4, None, 2, 224, 224, 3, None), who, "null", "out")
    for T, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, -1)):
        _refused(fn(None, PTR, T, H, W, None, 1, 224, 224, 3, PTR), who, "source")
    for oh, ow, ch in ((0, 224, 3), (224, 0, 3), (224, 224, 0), (8192, 8192, 1)):
        _refused(fn(None, PTR, 2, 4, 4, None, 2, oh, ow, ch, PTR), who, "output")
    _refused(fn(None, PTR, 2, 4, 4, PTR, 0, 224, 224, 3, PTR), who, "frames_dev", "n = 0")
    _refused(fn(None, PTR, 2, 4, 4, PTR, -3, 224, 224, 3, PTR), who, "frames_dev", "n = -3")
    _refused(fn(None, PTR, 2, 4, 4, None, 3, 224, 224, 3, PTR), who, "n = 3", "T = 2")
    _refused(fn(None, PTR, 2, 4, 4, None, 0, 224, 224, 3, PTR), who, "n = 0")


def test_masks_to_224_refuses_what_is_not_a_device_byte_clip():
    with pytest.raises(ValueError, match="uint8"):
        A.masks_to_224(torch.zeros((2, 4, 4)))
    with pytest.raises(ValueError, match="uint8"):
        A.masks_to_224(torch.zeros((2, 4, 4), dtype=torch.uint8))              # on the host


# ------------------------------------------------------------------------------------------------ the image embedding
def _image(seed, H=70, W=90):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def test_the_stand_in_embedding_has_sams_shape_and_depends_on_the_image_alone():
    p = annotate.ComponentPredictor()
    with pytest.raises(AssertionError):
        p.get_image_embedding()
    gt = torch.zeros((70, 90), dtype=torch.uint8)
    gt[10:30, 20:50] = 1
    out = []
    for seed in (1, 1, 2):
        p.reset_image()
        p.set_target(gt)
        p.set_image(_image(seed))
        out.append(p.get_image_embedding())
    assert all(e.shape == (1, 256, 64, 64) and e.dtype == torch.float32 and e.device == gt.device for e in out)
    assert torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2])
    assert torch.isfinite(out[0]).all() and float(out[0].abs().max()) > 0
    p.reset_image()
    with pytest.raises(AssertionError):
        p.get_image_embedding()
    # through the annotator: a normalised [3,H,W] frame, as the sessions hand it over
    ann = annotate.PromptAnnotator(p, click_robot=object(), bbox_robot=object(), best_mask=object())
    im = torch.from_numpy((_image(1).astype(np.float32) / 255 - annotate.MEAN) / annotate.STD).permute(2, 0, 1)
    e = ann.image_embedding(im, gt)
    assert e.shape == (1, 256, 64, 64) and float((e - out[0]).abs().max()) < 0.05 * float(out[0].abs().max())      # uint8 rounding of the frame only


def test_the_embedding_is_taken_from_the_controllers_own_predictor_or_refused():
    class Sam:
        def get_image_embedding(self):
            return "embedding"

    class Controller:                                            # sam/sam_controller.py keeps SAM's predictor in .predictor
        def __init__(self):
            self.predictor, self.calls = Sam(), []

        def reset_image(self):
            self.calls.append("reset")

        def set_image(self, im):
            self.calls.append("set")

    class Bare(Controller):
        def __init__(self):
            self.predictor, self.calls = None, []

    ctl = Controller()
    ann = annotate.PromptAnnotator(ctl, click_robot=object(), bbox_robot=object(), best_mask=object())
    assert ann.image_embedding(None, None) == "embedding" and ctl.calls == ["reset", "set"]
    bare = Bare()
    with pytest.raises(ValueError, match="get_image_embedding"):
        annotate.PromptAnnotator(bare, click_robot=object(), bbox_robot=object(), best_mask=object()).image_embedding(None, None)
    assert bare.calls == []


# ------------------------------------------------------------------------------------------------ the loop
def reference_eva_vos(T, rounds, gt, images, annotator, rl_agent, selector, log):
    """``eva_vos`` with ``rl_agent_annotate`` and ``store_action_data`` (interactions/mulitple_annotations.py:286-378, 88-101), restated line by
    line over the fakes: ``eval_processor_metric`` is ``_quality`` of the frame types, ``qnet_frame_selection`` is ``selector.select``."""
    empty = (gt[:, 0].flatten(1).sum(1) == 0).numpy()
    frame_iteraction_type = np.zeros((T,))
    frame_iteraction_type[0] = 1
    metric, frames_list, mu_metrics = None, [0], []
    pf_annots = [dict(annotations=[], click_labels=None, click_coords=None, bbox=None, sam_logits=None, metric=0) for _ in range(T)]
    annotation_times, fully_annotated, rl_values, annotations_actions, round_metrics = [], False, [-2], [], []
    gen_masks = None

    def not_avail_frames(ious, interacted_frames, num_frames):
        zgt = np.where(np.array(ious) == 20)[0].tolist()
        return len(set(range(num_frames)) - set(zgt + interacted_frames)) == 0

    for r in range(1, rounds + 1):
        if (r >= T and np.min(metric) == 1) or fully_annotated:
            continue
        if metric is not None and not_avail_frames(metric, frames_list, T):
            continue
        frame = frames_list[-1]
        if r > 1:
            gt_mask, frame_annots = gt[frame, 0], pf_annots[frame]
            if frame_annots["metric"] == 20:
                sam_mask, cost, ann_action, sam_logits, clicks, labels, bbox, rl_value = gt_mask, 3, "no_object", None, None, None, None, 0
            else:
                emb = annotator.image_embedding(images[frame], gt_mask)
                action, value = rl_agent.act(emb, selector.masks_to_input(gen_masks, [frame]))
                ann_action = ["3clicks", "mask"][action]
                sam_mask, cost, _, sam_logits, clicks, labels, bbox = annotator.annotate(ann_action, gt_mask, images[frame], gen_masks[frame][None].to(torch.bool),
                                                                                        frame_annots)
                rl_value = value.squeeze().item()
            rl_values.append(rl_value)
            if ann_action == "mask":
                frame_iteraction_type[frame] = 1
                mask_for_iteraction = gt[frame][None]
            else:
                mask_for_iteraction = sam_mask.float().reshape(gt[frame].shape)[None]
                frame_iteraction_type[frame] = 2
                log.append(("annotation", frame, sam_mask.flatten().int().tolist()))
                frame_annots.update(click_labels=labels, click_coords=clicks, bbox=bbox, sam_logits=sam_logits)
        else:
            mask_for_iteraction, cost, ann_action = gt[frame][None], 80, "mask"
        pf_annots[frame]["annotations"].append(ann_action)
        log.append(("interact", frame, list(mask_for_iteraction.shape), mask_for_iteraction.flatten().int().tolist()))
        metric = _quality(frame_iteraction_type, empty)
        gen_masks = _gen(T, len(round_metrics) + 1)
        for ii, m in enumerate(metric):
            pf_annots[ii]["metric"] = m
        if r >= T:
            not_annotated_with_mask_frames = np.where(frame_iteraction_type != 1)[0]
            if len(not_annotated_with_mask_frames) == 0:
                fully_annotated, selected_frame = True, -1
            else:
                selected_frame = selector.select(gen_masks, not_annotated_with_mask_frames)
        else:
            selected_frame = selector.select(gen_masks, frames_list)
        frames_list.append(selected_frame)
        mu_metrics.append(float(np.mean(metric[~empty])))
        annotation_times.append(cost)
        annotations_actions.append(ann_action)
        round_metrics.append(metric)
    return mu_metrics, annotation_times, rl_values, annotations_actions, round_metrics, frames_list[:-1]


# T, rounds, frames without the object, the selector's answers, the agent's (action, value) answers
LOOPS = {
    # frame 4 has no object (3 s, value 0, no agent call); frame 1 gets clicks, then its mask; from round 5 = T on the frames without a mask
    # are the selector's set; after round 6 every frame with an object has been chosen: the not_avail_frames skip ends the session
    "no_object_repeat_switch_skip": (5, 10, [4], [4, 1, 1, 2, 2, 3], [(0, 0.25), (1, 0.5), (0, -1.5), (1, 2.0)]),
    # three frames, masks only: before the third mask every frame has been chosen, so the not_avail_frames skip comes first.  It always does
    # for T >= 2: the round that would leave no frame without a mask starts with every frame in the list - the reference's fully_annotated
    # branch (:363-365) is reached only by a one-frame clip (the test below), where the reference itself stops at np.min(None) (:321)
    "masks_only": (3, 6, [], [1, 2], [(1, 0.75)]),
    # fewer rounds than the script: the session ends with a frame pending
    "rounds_run_out": (5, 3, [4], [4, 1, 1], [(0, 0.25)]),
}


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_the_loop_equals_the_literal_restatement_of_the_references_eva_vos(name):
    T, rounds, empty_frames, picks, acts = LOOPS[name]
    gt, rgb = _clip(T, empty_frames)
    ref_log = []
    ref = reference_eva_vos(T, rounds, gt, rgb[0], Annotator(ref_log), Agent(acts, ref_log), Selector(picks, ref_log), ref_log)
    log = []
    selector, agent = Selector(picks, log), Agent(acts, log)
    gen = torch.Generator().manual_seed(3)
    res = eval_driver.run_eva_vos(Proc(log), {"num_frames": T, "gt": gt[None], "rgb": rgb}, rounds, Annotator(log), "qnet", agent, "j_and_f", rng=gen,
                                  scorer=Scorer(gt[:, 0], log), selector=selector)
    print(name, "frames", res["annotated_frames"], "actions", res["annotations_actions"], "costs", res["annotation_times"], "values", res["rl_values"])
    print([e for e in log if e[0] == "select"])
    mu, times, values, actions, round_metrics, frames = ref
    assert res["annotated_frames"] == frames and res["annotations_actions"] == actions and res["annotation_times"] == times
    assert res["rl_values"] == values and res["rl_values"][0] == -2 and res["mu_metrics"] == mu
    assert np.array_equal(np.stack(res["round_metrics"]), np.stack(round_metrics))
    strip = lambda lg: [e[:3] if e[0] == "act" else e for e in lg]             # the restatement's agent takes no generator
    assert strip(log) == strip(ref_log)
    assert all(e[3] is gen for e in log if e[0] == "act")                       # every draw from the session's generator
    assert not selector.script and not agent.script                             # every scripted answer was asked for
    if name == "no_object_repeat_switch_skip":
        assert frames == [0, 4, 1, 1, 2, 2] and actions == ["mask", "no_object", "3clicks", "mask", "3clicks", "mask"]
        assert times == [80, 3, 4.5, 80, 4.5, 80] and values == [-2, 0, 0.25, 0.5, -1.5, 2.0]
        assert [e[2] for e in log if e[0] == "select"] == [[0], [0, 4], [0, 4, 1], [0, 4, 1, 1], [2, 3, 4], [3, 4]]
    if name == "masks_only":
        assert frames == [0, 1] and [e[2] for e in log if e[0] == "select"] == [[0], [0, 1]]


def test_a_session_with_no_frame_left_without_a_mask_is_fully_annotated():
    """r >= T with every frame annotated with its mask: no selection, no pending frame, no further round (:361-365)."""
    gt, rgb = _clip(1, [])
    log = []
    selector, agent = Selector([], log), Agent([], log)
    res = eval_driver.run_eva_vos(Proc(log), {"num_frames": 1, "gt": gt[None], "rgb": rgb}, 4, Annotator(log), "qnet", agent, scorer=Scorer(gt[:, 0], log),
                                  selector=selector)
    assert res["annotated_frames"] == [0] and res["annotations_actions"] == ["mask"] and res["annotation_times"] == [80] and res["rl_values"] == [-2]
    assert [e[0] for e in log] == ["interact"]


def test_eva_vos_refuses_a_multi_object_sample_and_missing_parts():
    gt, rgb = _clip(3, [])
    with pytest.raises(ValueError, match="one-object"):
        eval_driver.run_eva_vos(None, {"num_frames": 3, "gt": gt[None], "rgb": rgb, "object_ids": [0, 1]}, 3, None, None, None)
    for missing in ("qnet", "agent", "annotator"):
        kw = dict(qnet="qnet", agent="agent", annotator="component")
        kw[missing] = None
        with pytest.raises(ValueError, match=missing):
            eval_driver.run("no/such/root", "no/such/imset", None, None, None, "eva_vos", rounds=3, **kw)
    with pytest.raises(ValueError, match="multi-object"):
        eval_driver.run("no/such/root", "no/such/imset", None, None, None, "eva_vos", multi_object=True, qnet="q", agent="a", annotator="component")


def test_the_session_loop_without_select_calls_next_frame_as_before():
    gt, _ = _clip(3, [])
    log, calls = [], []

    def next_frame(worst, types_, gen, frames):
        calls.append((worst, types_.tolist()))
        return None

    ses = sessions.annotation_session(Proc(log), Scorer(gt[:, 0], log), 3, 4, 
                                     sessions.SessionPolicy(lambda f: gt[f][None], next_frame, action=lambda *a: pytest.fail("round 2 never starts"), stop_at_T=False))
    assert calls == [(1, [1, 0, 0])] and ses["frames"] == [0] and ses["pending"] is None
