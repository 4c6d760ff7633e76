"""CPU: the annotation-type dataset driver without a GPU - ``frames_to_rgb8_host`` against what the reference's own helpers stored
(tests/golden/annot_export.npz), the two stop-rule fields of ``SessionPolicy``, ``run_annotation_dataset`` against a literal restatement of
generate_annotation_dataset.py:89-178 on fakes that record every call, the argument checks of ``stcn_frames_to_rgb8`` and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from eva_vos_amd import _lib, annot_driver, sessions
from session_fakes import Annotator, Proc, Scorer
from session_fakes import clip as _clip, gen_masks as _gen, quality as _quality

GOLD = os.path.join(os.path.dirname(__file__), "golden", "annot_export.npz")


# ------------------------------------------------------------------------------------------------ the stored image
def _golden():
    g = np.load(GOLD)
    return {name: (g[f"{name}.frame"], g[f"{name}.rgb8"]) for name in sorted({k.split(".")[0] for k in g.files})}


def test_the_host_restatement_equals_what_the_reference_stored_byte_for_byte():
    cases = _golden()
    assert {"random", "constant", "single_pixel", "all_negative", "min_max_channels"} <= set(cases)
    for name, (frame, rgb8) in cases.items():
        got = annot_driver.frames_to_rgb8_host(frame)
        assert got.dtype == np.uint8 and got.shape == (1,) + rgb8.shape and np.array_equal(got[0], rgb8), name
        assert np.array_equal(annot_driver.frames_to_rgb8_host(torch.from_numpy(frame), [0, 0])[1], rgb8), name
    assert int(cases["constant"][1].max()) == 0 and int(cases["single_pixel"][1].max()) == 255
    with pytest.raises(ValueError, match="frames"):
        annot_driver.frames_to_rgb8_host(cases["random"][0], [1])
    with pytest.raises(ValueError, match="float32"):
        annot_driver.frames_to_rgb8_host(cases["random"][0].astype(np.float64))


def test_frames_to_rgb8_has_no_cpu_fallback():
    with pytest.raises(ValueError, match="on the device"):
        annot_driver.frames_to_rgb8(torch.zeros((2, 3, 4, 4)))
    with pytest.raises(ValueError, match="float32"):
        annot_driver.frames_to_rgb8(torch.zeros((2, 3, 4, 4), dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ the C ABI
def _refused(rc, *needles):
    assert rc == -1                                            # STCN_E_INVALID
    msg = _lib.lib().stcn_last_error().decode()
    for n in needles:
        assert n in msg, msg


BUF = (C.c_uint8 * 64)()
PTR = C.cast(BUF, C.c_void_p)           # never dereferenced: every call below is refused on the host


def test_the_export_entry_is_declared_exported_and_checks_its_arguments_without_a_gpu():
    who = "stcn_frames_to_rgb8"
    assert who in _lib.PROTOTYPES
    fn = getattr(_lib.lib(), who)
    _refused(fn(None, None, 2, 4, 4, None, 2, PTR, PTR), who, "null", "clip_dev")
    _refused(fn(None, PTR, 2, 4, 4, None, 2, None, PTR), who, "null", "scratch_dev")
    _refused(fn(None, PTR, 2, 4, 4, None, 2, PTR, None), who, "null", "out_dev")
    _refused(fn(None, None, 2, 4, 4, None, 0, PTR, PTR), who, "null")                 # also with nothing to do
    _refused(fn(None, PTR, 2, 4, 4, None, -1, PTR, PTR), who, "n = -1")
    _refused(fn(None, PTR, 2, 4, 4, PTR, -3, PTR, PTR), who, "n = -3")
    for T, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, 0), (2, 4, -1), (1, 4097, 4096), (1, 1, 2 ** 24 + 1)):
        _refused(fn(None, PTR, T, H, W, None, 1, PTR, PTR), who, "clip")
    _refused(fn(None, C.c_void_p(PTR.value + 2), 2, 4, 4, None, 1, PTR, PTR), who, "aligned")


# ------------------------------------------------------------------------------------------------ the two stop-rule fields
def _clicks_then_mask(gt, log):
    def action(frame, gen, annots):
        log.append(("action", frame, int(gen[0, 0, 0]), list(annots["annotations"])))
        if "3clicks" in annots["annotations"]:
            return None, 80, "mask", None, None, None, None
        return 1 - gt[frame, 0], 4.5, "3clicks", "logits", "clicks", "labels", None
    return action


def test_a_session_with_both_fields_at_their_defaults_logs_what_it_logged_before():
    """T = 5 (frame 4 without the object), 9 rounds, every frame gets clicks and then its mask, the worst frame is chosen.  The log below is what
    the loop recorded before the two fields existed: the quality rows are fetched from round T on only, and after round 5 every frame with
    an object has been chosen, so the not_avail_frames skip ends the session."""
    T, rounds = 5, 9
    gt, _ = _clip(T, [4])
    log, stats = [], {}
    policy = sessions.SessionPolicy(lambda f: gt[f][None], lambda worst, types, gen, frames: worst, action=_clicks_then_mask(gt, log), stop_at_T=False)
    assert policy.stop_when_perfect is False and policy.check_available is True
    ses = sessions.annotation_session(Proc(log), Scorer(gt[:, 0], log, trace=True), T, rounds, policy, stats)
    assert log == [
        ("interact", 0, [1, 1, 2, 2], [1, 0, 0, 0]),
        ("score", [0], False, True, [1]),
        ("action", 1, 1, []),
        ("annotation", 1, [1, 0, 1, 1]),
        ("interact", 1, [1, 1, 2, 2], [1, 0, 1, 1]),
        ("score", [0, 1], False, True, [1, 2]),
        ("action", 1, 2, ["3clicks"]),
        ("interact", 1, [1, 1, 2, 2], [0, 1, 0, 0]),
        ("score", [0, 1, 1], False, True, [1, 2, 1]),
        ("action", 2, 3, []),
        ("annotation", 2, [0, 1, 1, 1]),
        ("interact", 2, [1, 1, 2, 2], [0, 1, 1, 1]),
        ("score", [0, 1, 1, 2], False, True, [1, 2, 1, 2]),
        ("qualities", 4),
        ("action", 2, 4, ["3clicks"]),
        ("interact", 2, [1, 1, 2, 2], [1, 0, 0, 0]),
        ("score", [0, 1, 1, 2, 2], False, True, [1, 2, 1, 2, 1]),
        ("qualities", 5),
        ("qualities", 5),
        ("qualities", 5),
        ("qualities", 5),
    ]
    assert {k: ses[k] for k in ("frames", "types", "costs", "actions", "pending", "chosen", "propagated_frames")} == {
        "frames": [0, 1, 1, 2, 2], "types": [1, 2, 1, 2, 1], "costs": [80, 4.5, 80, 4.5, 80], "actions": ["mask", "3clicks", "mask", "3clicks", "mask"],
        "pending": 3, "chosen": [0, 1, 1, 2, 2, 3], "propagated_frames": 15}
    assert stats == {"propagated_frames": 15, "interactions": 5}


class PerfectFrom(Scorer):
    """``Scorer`` whose every frame reaches quality 1.0 in round ``first``."""

    def __init__(self, gt_thw, log, first):
        super().__init__(gt_thw, log)
        self.first = first

    def score(self, processor, annotated_frames, keep_gen=True, incremental=True, types=None):
        worst, gen = super().score(processor, annotated_frames, keep_gen, incremental, types)
        if len(self.rows) >= self.first:
            self.rows[-1] = np.where(self.empty_host, 20.0, 1.0)
            worst = int(np.argmin(self.rows[-1]))
        return worst, gen


@pytest.mark.parametrize("stop", [False, True])
def test_stop_when_perfect_ends_a_session_before_round_T(stop):
    T, rounds = 8, 6
    gt, _ = _clip(T, [])
    log = []
    clicks = lambda frame, gen, annots: (1 - gt[frame, 0], 4.5, "3clicks", "logits", "clicks", "labels", None)      # noqa: E731
    policy = sessions.SessionPolicy(lambda f: gt[f][None], lambda worst, types, gen, frames: worst, action=clicks, stop_at_T=False, stop_when_perfect=stop)
    ses = sessions.annotation_session(Proc(log), PerfectFrom(gt[:, 0], log, 3), T, rounds, policy)
    ran = len([e for e in log if e[0] == "interact"])
    print("stop_when_perfect", stop, "rounds run", ran, "frames", ses["frames"])
    assert ran == len(ses["costs"]) == (3 if stop else 6)          # the quality is 1.0 from round 3 on; r < T throughout
    assert ses["frames"][:3] == [0, 1, 1]


@pytest.mark.parametrize("check", [True, False])
def test_check_available_false_keeps_a_session_going_past_its_valid_frames(check):
    T, rounds = 3, 6
    gt, _ = _clip(T, [])
    log, picks = [], [1, 2, 1, 2, 1, 2]
    clicks = lambda frame, gen, annots: (1 - gt[frame, 0], 4.5, "3clicks", "logits", "clicks", "labels", None)      # noqa: E731
    policy = sessions.SessionPolicy(lambda f: gt[f][None], lambda worst, types, gen, frames: picks.pop(0), action=clicks, stop_at_T=False,
                                    check_available=check)
    ses = sessions.annotation_session(Proc(log), Scorer(gt[:, 0], log), T, rounds, policy)
    print("check_available", check, "frames", ses["frames"])
    # after round 2 every frame has been chosen (the pending one counts): the default stops there, the loop without the skip goes on
    # re-annotating the click frames
    assert ses["frames"] == ([0, 1] if check else [0, 1, 2, 1, 2, 1])
    assert ses["actions"] == ["mask"] + ["3clicks"] * (len(ses["frames"]) - 1)


# ------------------------------------------------------------------------------------------------ the session of the dataset
class DatasetAnnotator(Annotator):
    """The fake annotator with what this session needs besides: clicks on a frame that has clicks already improve it by little (so the oracle
    takes the mask the second time), and an embedding that says which call made it."""

    def __init__(self, log):
        super().__init__(log)
        self.embeddings = 0

    def image_embedding(self, im, gt_mask, reuse=False):
        self.log.append(("embedding", list(im.shape), gt_mask.flatten().int().tolist()))
        self.embeddings += 1
        return torch.full((1, 2, 3, 3), float(self.embeddings))

    def annotate(self, annot_type, gt_mask, im=None, mivos_mask=None, frame_annots=None, empty=None):
        out = super().annotate(annot_type, gt_mask, im, mivos_mask, frame_annots, empty)
        if annot_type != "mask" and "3clicks" in frame_annots["annotations"]:
            return out[:2] + (0.26,) + out[3:]
        return out


def reference_annotation_dataset(T, rounds, gt, images, annotator, name, annotation_types, log):
    """generate_annotation_dataset.py:89-178 with ``oracle_action`` (interactions/mulitple_annotations.py:42-85), restated line by line over the
    fakes: ``eval_processor_metric`` is ``_quality`` of the frame types (``metric_no_zgt``: its values on the frames with an object),
    ``compute_iou`` is the annotator's ``iou``, ``predictor.get_image_embedding()`` its ``image_embedding``."""
    empty = (gt[:, 0].flatten(1).sum(1) == 0).numpy()
    db_data = {k: [] for k in ["id", "frame_cost", "video_cost", "selected_annotation", "frame_num", "round", "video_name", "init_iou"]
               + [f"{a}_iou" for a in annotation_types]}
    saved_masks, saved_embeddings = [], []

    def oracle_action(frame_annots, gt_mask, mivos_mask, im):
        best_reward, best = -1e10, (None, 1e10, None, None, None, None, None)
        init_iou = annotator.iou(mivos_mask.unsqueeze(0).to(torch.bool), gt_mask)
        actions_data = {"init_iou": init_iou}
        for ann_type in annotation_types:
            if ann_type == "bbox" and "bbox" in frame_annots["annotations"]:
                continue
            sam_mask, ann_cost, curr_iou, sam_logits, clicks, labels, bbox = annotator.annotate(ann_type, gt_mask, im, mivos_mask.unsqueeze(0).to(torch.bool),
                                                                                                frame_annots)
            r = (curr_iou - init_iou) / ann_cost
            actions_data[ann_type] = {"iou": curr_iou, "cost": ann_cost, "reward": r}
            if r >= best_reward:
                best_reward, best = r, (sam_mask, ann_cost, ann_type, sam_logits, clicks, labels, bbox)
        return best + (actions_data,)

    frames_list = [0]
    metric = metric_no_zgt = gen_masks = None
    frame_iteraction_type = np.zeros((T,))
    frame_iteraction_type[0] = 1
    frames_cost = np.zeros((T,))
    pf_annots = [dict(annotations=[], click_labels=None, click_coords=None, bbox=None, sam_logits=None, metric=0) for _ in range(T)]
    scored = 0
    for r in range(1, rounds + 1):
        if metric_no_zgt is not None and np.min(metric_no_zgt) == 1.0:
            continue
        frame = frames_list[r - 1]
        if r > 1:
            init_iou = metric[frame]
            sam_mask, cost, ann_action, sam_logits, clicks, labels, bbox, action_data = oracle_action(pf_annots[frame], gt[frame, 0], gen_masks[frame], images[frame])
            img_embedding = annotator.image_embedding(images[frame], gt[frame, 0])
            if ann_action == "mask":
                frame_iteraction_type[frame] = 1
                mask_for_iteraction = gt[frame][None]
            else:
                mask_for_iteraction = sam_mask.float().reshape(gt[frame].shape)[None]
                frame_iteraction_type[frame] = 2
                log.append(("annotation", frame, sam_mask.flatten().int().tolist()))
                pf_annots[frame].update(click_labels=labels, click_coords=clicks, bbox=bbox, sam_logits=sam_logits)
        else:
            mask_for_iteraction, cost, ann_action = gt[frame][None], 80, "mask"
        pf_annots[frame]["annotations"].append(ann_action)
        frames_cost[frame] += cost
        log.append(("interact", frame, list(mask_for_iteraction.shape), mask_for_iteraction.flatten().int().tolist()))
        metric = _quality(frame_iteraction_type, empty)
        metric_no_zgt = metric[~empty]
        scored += 1
        gen_masks = _gen(T, scored)
        if r > 1:
            db_data["id"].append(f"{name}_{r}_frame_{frame}")
            db_data["frame_cost"].append(frames_cost[frame])
            db_data["video_cost"].append(np.sum(frames_cost))
            db_data["selected_annotation"].append(ann_action)
            db_data["frame_num"].append(frame)
            db_data["round"].append(r)
            db_data["video_name"].append(name)
            db_data["init_iou"].append(init_iou)
            for action in annotation_types:
                db_data[f"{action}_iou"].append(action_data[action]["iou"])
            saved_masks.append(gen_masks[frame].clone())
            saved_embeddings.append(img_embedding.squeeze(0))
        frames_list.append(int(np.argmin(metric)))
    return db_data, saved_masks, saved_embeddings


# T, rounds, frames without the object
DATASET_LOOPS = {
    # frames 1 and 3 get clicks first and their mask the second time; frame 2 has no object; after round 5 every frame with an object is
    # perfect: rounds 6 .. 8 do not run although T = 4 < 8 and frames repeat (no not_avail_frames skip ended the session at round 4)
    "clicks_then_mask": (4, 8, [2]),
    # the rounds run out with a frame pending
    "rounds_run_out": (6, 4, [5]),
    "one_round": (3, 1, []),
}


@pytest.mark.parametrize("name", sorted(DATASET_LOOPS))
def test_the_dataset_session_equals_the_literal_restatement_of_the_references_loop(name):
    T, rounds, empty_frames = DATASET_LOOPS[name]
    gt, rgb = _clip(T, empty_frames)
    types_ = ["3clicks", "mask"]
    ref_log = []
    db, ref_masks, ref_embeddings = reference_annotation_dataset(T, rounds, gt, rgb[0], DatasetAnnotator(ref_log), "fake__1", types_, ref_log)
    log, stats = [], {}
    res = annot_driver.run_annotation_dataset(Proc(log), {"num_frames": T, "gt": gt[None], "rgb": rgb, "name": "fake__1"}, rounds, DatasetAnnotator(log),
                                              types_, stats=stats, scorer=Scorer(gt[:, 0], log))
    rows = res["rows"]
    print(name, [(r["id"], r["frame_cost"], r["video_cost"], r["selected_annotation"], r["init_iou"], r["3clicks_iou"], r["mask_iou"]) for r in rows])
    assert len(rows) == len(db["id"])
    for key in annot_driver.csv_header(types_):
        assert [row[key] for row in rows] == [float(v) if isinstance(v, (float, np.floating)) else v for v in db[key]], key
    assert all(list(row) == annot_driver.csv_header(types_) for row in rows)
    assert log == ref_log                                        # interactions, annotations, annotator calls: the same, in the same order
    assert [e for e in log if e[0] == "interact"] and stats["interactions"] == len(rows) + 1
    assert res["frames"] == db["frame_num"] and res["masks"].shape == (len(rows), 2, 2)
    assert all(torch.equal(m, r) for m, r in zip(res["masks"], ref_masks))
    if rows:
        assert res["embeddings"].shape == (len(rows), 2, 3, 3) and all(torch.equal(e, r) for e, r in zip(res["embeddings"], ref_embeddings))
    else:
        assert res["embeddings"] is None
    if name == "clicks_then_mask":
        assert [r["id"] for r in rows] == ["fake__1_2_frame_1", "fake__1_3_frame_1", "fake__1_4_frame_3", "fake__1_5_frame_3"]
        assert [r["selected_annotation"] for r in rows] == ["3clicks", "mask", "3clicks", "mask"]
        assert [r["frame_cost"] for r in rows] == [4.5, 84.5, 4.5, 84.5] and [r["video_cost"] for r in rows] == [84.5, 164.5, 169.0, 249.0]
        assert [r["init_iou"] for r in rows] == [0.5] * 4 and [r["3clicks_iou"] for r in rows] == [0.7, 0.26, 0.7, 0.26]
        assert [r["mask_iou"] for r in rows] == [1.0] * 4 and [int(m[0, 0]) for m in res["masks"]] == [2, 3, 4, 5]
        assert res["annotated_frames"] == [0, 1, 1, 3, 3] and float(res["round_metrics"][-1][2]) == 20.0
    if name == "one_round":
        assert rows == [] and res["annotated_frames"] == [0]


def test_the_embedding_after_an_action_costs_no_second_set_image():
    from eva_vos_amd import annotate

    class Controller:
        def __init__(self):
            self.calls = []

        def reset_image(self):
            self.calls.append("reset")

        def set_image(self, im):
            self.calls.append("set")

        def get_image_embedding(self):
            return len(self.calls)

    ctl = Controller()
    ann = annotate.PromptAnnotator(ctl, click_robot=object(), bbox_robot=object(), best_mask=object())
    clip = torch.zeros((2, 3, 4, 4))
    im = clip[1]
    ann.set_image(im, None)                                      # what an annotate() with clicks does to the frame
    assert ann.image_embedding(im, None, reuse=True) == 2 and ctl.calls == ["reset", "set"]
    assert ann.image_embedding(clip[1], None, reuse=True) == 4   # another object, even of the same frame: set again
    assert ann.image_embedding(im, None) == 6                    # and always without reuse
    fresh = annotate.PromptAnnotator(Controller(), click_robot=object(), bbox_robot=object(), best_mask=object())
    assert fresh.image_embedding(im, None, reuse=True) == 2      # nothing set yet: the frame is set


# ------------------------------------------------------------------------------------------------ refusals, the CSV
def test_the_driver_refuses_what_eval_driver_refuses():
    gt, rgb = _clip(3, [])
    with pytest.raises(ValueError, match="one-object"):
        annot_driver.run_annotation_dataset(None, {"num_frames": 3, "gt": gt[None], "rgb": rgb, "object_ids": [0, 1]}, 3, None)
    with pytest.raises(AttributeError, match="does not exist"):
        annot_driver.run_annotation_dataset(None, {"num_frames": 3, "gt": gt[None], "rgb": rgb}, 3, None, ["3clicks", "scribble"])
    with pytest.raises(ValueError, match="annotator"):
        annot_driver.run("no/such/root", "no/such/imset", "no/such/out", None, None, annotator=None)
    with pytest.raises(ValueError, match="unknown annotator"):
        annot_driver.run("no/such/root", "no/such/imset", "no/such/out", None, None, annotator="sam")
    with pytest.raises(AttributeError, match="does not exist"):
        annot_driver.run("no/such/root", "no/such/imset", "no/such/out", None, None, annotation_types=["mask", "polygon"])
    assert not os.path.exists("no/such/out")


def test_the_csv_header_is_the_references_column_order():
    assert annot_driver.csv_header() == ["id", "frame_cost", "video_cost", "selected_annotation", "frame_num", "round", "video_name", "init_iou",
                                         "3clicks_iou", "mask_iou"]
    assert annot_driver.csv_header(["click", "bbox", "mask"])[8:] == ["click_iou", "bbox_iou", "mask_iou"]


def test_fp64_values_survive_the_fp32_rows():
    for x in (0.1, 1 / 3, 20.0, 0.0, 1.0, 0.9237668161434978, float("nan")):
        v = annot_driver._pack64(x)
        assert v.dtype == np.float32 and v.shape == (4,)
        y = annot_driver._unpack64(v)
        assert y == x or (np.isnan(x) and np.isnan(y))
