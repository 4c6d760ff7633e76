"""The simulated annotator of the mixed-annotation sessions: turns "annotate this frame with clicks / a box / a mask" into a mask and a cost,
by prompting a promptable segmenter the way a person would (reference: annotator/annotator.py, util/helpers.py:50-58).

``PromptAnnotator`` restates ``Annotator.get_mask`` and its helpers over ANY predictor with the signature of the reference's SAM controller
(sam/sam_controller.py:24-63): ``set_image(im)``, ``reset_image()``, ``predict(click_coords, click_labels, bbox, mask_input,
multimask_output) -> (masks [n,1,H,W] on the device, scores, logits [n,h,w])``.  The segmenter stays what it is (stock PyTorch where it is
installed); everything around it is ours: the robots and the best-of-three run on the device (eva_vos_amd.robots), and the prompts handed
to the predictor are small host arrays, as SAM takes them.

``ComponentPredictor`` is a deterministic STAND-IN with that signature for tests and offline sessions.  It is NOT a segmenter: it knows the
ground truth of the frame and answers a click with the error component the click lands in."""
from __future__ import annotations

import re

import numpy as np

from . import robots

ANNOTATION_COSTS = {"no_object": 3, "mask": 80, "click": 1.5, "3clicks": 3 * 1.5, "bbox": 7, "click_overhead": 1, "stop": 0}      # util/helpers.py:50-58
SIMILAR_IOU, SIMILAR_TRIES = 0.8, 20            # create_similar_samlogits (annotator.py:62,83)
MEAN, STD = np.array([0.485, 0.456, 0.406], np.float32), np.array([0.229, 0.224, 0.225], np.float32)


def annotator_input(annot_type: str):
    """ann_type_to_annotator_input (interactions/mulitple_annotations.py:20-33): 'click' / 'bbox' / 'mask' / '<N>clicks' -> (kind, prompts)."""
    if annot_type in ("click", "bbox", "mask"):
        return annot_type, 1
    if re.match(r"^\d+clicks$", annot_type):
        return "click", int(annot_type.split("clicks")[0])
    raise AttributeError(f"{annot_type} does not exist!")


def check_annotation_types(types) -> list:
    """eval_annotation_method.py:95-104: 'click', 'bbox', 'mask' or '<N>clicks'."""
    types = list(types)
    for t in types:
        annotator_input(t)
    return types


def _cat(prev, new):
    return new if prev is None else np.concatenate((prev, new), axis=0)


class PromptAnnotator:
    """``Annotator`` (annotator/annotator.py:19-289).  ``prompt_type``: 'a' = no earlier prompts or logits, 'b' = earlier logits + new prompts,
    'c' = earlier prompts + new prompts (the reference's default).  ``click_robot`` / ``bbox_robot`` / ``best_mask``: the device robots by
    default; the host restatements (``robots.HostClickRobot`` ...) give the host route with the same loop."""

    def __init__(self, predictor, prompt_type: str = "c", click_robot=None, bbox_robot=None, best_mask=None):
        assert prompt_type in {"a", "b", "c"}
        self.predictor, self.prompt_type = predictor, prompt_type
        self.click_robot = click_robot or robots.ClickRobot()
        self.bbox_robot = bbox_robot or robots.BboxRobot()
        self._best = best_mask or robots.best_mask
        self.robot_calls = 0                                    # click-robot and best-of-n calls: what tools/click_robot_cost.py counts

    @classmethod
    def on_host(cls, predictor, prompt_type: str = "c"):
        """The same annotator with the host robots: two mask downloads and a SciPy labelling per click, IoUs in torch on the CPU."""
        return cls(predictor, prompt_type, robots.HostClickRobot(), robots.HostBboxRobot(), lambda c, t: robots.host_best_mask(c, t)[:2])

    # ---- the pieces ------------------------------------------------------------------------------------------------------------------
    def best_sam_mask(self, sam_masks, target_mask):
        """annotator.py:38-57 -> (max IoU, index; -1 when no candidate is above 0)."""
        self.robot_calls += 1
        return self._best(sam_masks, target_mask.reshape(target_mask.shape[-2:]))

    def iou(self, mask, target) -> float:
        """compute_iou (interactions/metrics.py:9-19) of one mask: always above 0, so it is what best-of-one reports."""
        return self.best_sam_mask(mask.reshape((1,) + tuple(mask.shape[-2:])), target)[0]

    def _interact(self, pred, gt):
        self.robot_calls += 1
        return self.click_robot.interact(pred, gt)

    def _middle(self, gt):
        self.robot_calls += 1
        return self.click_robot.middle_click(gt)

    def set_image(self, im, gt_mask):
        """annotator.py:30-35: the frame as uint8 [H,W,3] for the predictor; a stand-in that knows the ground truth gets it here."""
        given = im                                              # what image_embedding(reuse=True) recognises the frame by
        if im is not None and hasattr(im, "detach"):
            a = im.detach().cpu().squeeze().numpy().transpose((1, 2, 0)) * STD + MEAN
            im = (a * 255).astype(np.uint8)
        self._image_given = None
        self.predictor.reset_image()
        if hasattr(self.predictor, "set_target"):
            self.predictor.set_target(gt_mask)
        self.predictor.set_image(im)
        self._image_given = given

    def image_embedding(self, im, gt_mask, reuse: bool = False):
        """The segmenter's embedding of the frame, the agent's first input (rl_agent_annotate, interactions/mulitple_annotations.py:293-294):
        ``set_image`` as above, then ``get_image_embedding()`` of the predictor or of ``predictor.predictor`` - where the reference's
        ``SAMController`` keeps SAM's own predictor (sam/sam_controller.py) -> [1,256,64,64].  ``reuse``: where the predictor holds this
        very ``im`` already - the object the last ``set_image`` was given, as after an ``annotate`` with clicks or a box on it - the image
        is not set again (no second pass of the segmenter's encoder: generate_annotation_dataset.py:120 reads the embedding the action left)."""
        for p in (self.predictor, getattr(self.predictor, "predictor", None)):
            if hasattr(p, "get_image_embedding"):
                if not (reuse and im is not None and getattr(self, "_image_given", None) is im):
                    self.set_image(im, gt_mask)
                return p.get_image_embedding()
        raise ValueError(f"eva_vos needs the image embedding its agent reads: {type(self.predictor).__name__} offers no get_image_embedding(), "
                         "neither itself nor through a .predictor attribute (SAMController, ComponentPredictor do)")

    def create_similar_samlogits(self, pred_mask):
        """annotator.py:60-107: a segmenter cannot be prompted with the propagated mask, so make it produce a similar one: a middle click,
        then up to 20 corrective clicks, until the best candidate's IoU with ``pred_mask`` is above 0.8; (None,) * 4 when it never is."""
        import torch
        if torch.count_nonzero(pred_mask).item() == 0:
            return None, None, None, None
        clicks, labels = self._middle(pred_mask)
        masks, _, logits = self.predictor.predict(click_coords=clicks, click_labels=labels)
        max_iou, idx = self.best_sam_mask(masks, pred_mask)
        if max_iou > SIMILAR_IOU:
            return logits[idx][None, :, :], masks[idx], clicks, labels
        best_mask, best_logits = masks[idx], logits[idx]
        for _ in range(SIMILAR_TRIES):
            c, l = self._interact(best_mask, pred_mask)
            clicks, labels = _cat(clicks, c), _cat(labels, l)
            masks, _, logits = self.predictor.predict(mask_input=best_logits[None, :, :], click_coords=clicks, click_labels=labels, multimask_output=True)
            max_iou, idx = self.best_sam_mask(masks, pred_mask)
            best_mask, best_logits = masks[idx], logits[idx]
            if max_iou > SIMILAR_IOU:
                return best_logits[None, :, :], best_mask, clicks, labels
        return None, None, None, None

    def get_prompts(self, mivos_mask, prev_iter_data):
        """annotator.py:148-153,178-193 -> (logits, mask, clicks, labels, bbox) to start from."""
        if prev_iter_data is None or prev_iter_data["sam_logits"] is None:
            sam_logits, sam_mask, clicks, labels = None, None, None, None
            if self.prompt_type in ("b", "c") and mivos_mask is not None:
                sam_logits, sam_mask, clicks, labels = self.create_similar_samlogits(mivos_mask)
            bbox = None
        else:
            sam_mask = mivos_mask
            clicks, labels = prev_iter_data["click_coords"], prev_iter_data["click_labels"]
            sam_logits, bbox = prev_iter_data["sam_logits"], prev_iter_data["bbox"]
        if self.prompt_type == "b":
            clicks, labels, bbox = None, None, None
        return sam_logits, sam_mask, clicks, labels, bbox

    def get_click_mask_n_prompts(self, gt_mask, num_clicks, mivos_mask=None, prev_iter_data=None):
        """annotator.py:197-244."""
        curr_iou, cost = 0, 0
        sam_logits, sam_mask, prev_clicks, prev_labels, bbox = self.get_prompts(mivos_mask, prev_iter_data)
        prompt_clicks = prompt_labels = None
        for _ in range(num_clicks):
            if prev_clicks is None:
                prompt_clicks, prompt_labels = self._middle(gt_mask) if sam_mask is None else self._interact(sam_mask, gt_mask)
                cost += ANNOTATION_COSTS["click"]
            else:
                c, l = self._interact(sam_mask, gt_mask)
                cost += l.shape[0] * ANNOTATION_COSTS["click"]
                prompt_clicks, prompt_labels = _cat(prev_clicks, c), _cat(prev_labels, l)
            masks, _, logits = self.predictor.predict(click_coords=prompt_clicks, click_labels=prompt_labels, mask_input=sam_logits, bbox=bbox,
                                                      multimask_output=True)
            curr_iou, idx = self.best_sam_mask(masks, gt_mask)
            sam_mask, sam_logits = masks[idx], logits[idx][None, :, :]
            prev_clicks, prev_labels = prompt_clicks, prompt_labels
        cost += ANNOTATION_COSTS["click_overhead"]
        return sam_mask, cost, curr_iou, sam_logits, prompt_clicks, prompt_labels, bbox

    def get_bbox_mask_n_prompts(self, gt_mask, prompts, mivos_mask=None, prev_iter_data=None):
        """annotator.py:246-289: a box first, then refinement clicks."""
        curr_iou, cost, new_clicks = 0, 0, False
        sam_logits, sam_mask, prev_clicks, prev_labels, prev_box = self.get_prompts(mivos_mask, prev_iter_data)
        if prev_box is not None:                                # the reference asserts here (annotator.py:252): a frame takes one box
            raise AssertionError("the frame was annotated with a box before: a box is given once per frame (oracle_action skips it)")
        prompt_clicks = prompt_labels = bbox = None
        for ii in range(prompts):
            if ii == 0:
                bbox = self.bbox_robot.interact(gt_mask)
                cost += ANNOTATION_COSTS["bbox"]
                prompt_clicks, prompt_labels = prev_clicks, prev_labels
            else:
                new_clicks = True
                c, l = self._interact(sam_mask, gt_mask)
                cost += l.shape[0] * ANNOTATION_COSTS["click"]
                prompt_clicks, prompt_labels = _cat(prev_clicks if prev_labels is not None else None, c), _cat(prev_labels, l)
            masks, _, logits = self.predictor.predict(click_coords=prompt_clicks, click_labels=prompt_labels, mask_input=sam_logits, bbox=bbox,
                                                      multimask_output=True)
            curr_iou, idx = self.best_sam_mask(masks, gt_mask)
            sam_mask, sam_logits = masks[idx], logits[idx][None, :, :]
            prev_clicks, prev_labels = prompt_clicks, prompt_labels
        if new_clicks:
            cost += ANNOTATION_COSTS["click_overhead"]
        return sam_mask, cost, curr_iou, sam_logits, prompt_clicks, prompt_labels, bbox

    def get_mask(self, annotation_type, gt_mask, im=None, num_prompts=1, mivos_mask=None, prev_iter_data=None, empty=None):
        """annotator.py:110-145 -> (mask, cost in seconds, IoU, logits, clicks, labels, bbox).  An empty object costs 3 s whatever the type;
        'mask' is the ground truth for 80 s.  ``empty``: whether the object is absent, when the caller knows it (saves a device wait)."""
        import torch
        assert annotation_type in {"mask", "click", "bbox"}
        if (torch.count_nonzero(gt_mask).item() == 0) if empty is None else empty:
            return gt_mask, ANNOTATION_COSTS["no_object"], 20, None, None, None, None
        if annotation_type == "mask":
            return gt_mask, ANNOTATION_COSTS["mask"], 1, None, None, None, None
        self.set_image(im, gt_mask)
        g = gt_mask.to(torch.bool)
        fn = self.get_click_mask_n_prompts if annotation_type == "click" else self.get_bbox_mask_n_prompts
        return fn(g, num_prompts, mivos_mask=mivos_mask, prev_iter_data=prev_iter_data)

    def annotate(self, annot_type, gt_mask, im=None, mivos_mask=None, frame_annots=None, empty=None):
        """annotate (interactions/mulitple_annotations.py:36-39)."""
        kind, n = annotator_input(annot_type)
        return self.get_mask(kind, gt_mask, im=im, num_prompts=n, mivos_mask=mivos_mask, prev_iter_data=frame_annots, empty=empty)


class ComponentPredictor:
    """A deterministic stand-in with the SAM controller's ``predict`` signature, for tests and offline sessions.  NOT a segmenter: it is told
    the ground truth of the frame (``set_target``, which ``PromptAnnotator.set_image`` calls) and answers prompts by rule:

    * it starts from ``mask_input > 0`` (its own logits of an earlier call), else from the filled box when one is given, else from nothing;
      a box beside a mask input clips the mask to the box;
    * each click, in order: a positive click adds the 8-connected component of the missing region (object, not in the mask) it lands in, a
      negative click removes the component of the surplus region (mask, not object) it lands in; a click elsewhere changes nothing;
    * it returns three fixed variants of the result - eroded by one pixel, dilated by one, dilated by two (3 x 3 structure) - so that, as
      with a real segmenter, no candidate is the ground truth, with scores (0.9, 0.8, 0.7) and logits of +4 / -4 at full resolution.

    Like SAM's predictor it works on the host and uploads its masks: prompts are small host arrays, logits stay host arrays."""

    EMBED_SEED = 17                                     # Philox key of the fixed 256 x 3 matrix of get_image_embedding

    def __init__(self):
        self.gt = None
        self.image = None
        self.embedded = False
        self.device = None

    def set_target(self, gt_mask):
        self.device = gt_mask.device if hasattr(gt_mask, "device") else None
        self.gt = robots._as_bool(gt_mask)

    def set_image(self, image):
        assert self.gt is not None, "ComponentPredictor: set_target(gt) before set_image"
        self.embedded = True
        self.image = image

    def reset_image(self):
        self.embedded, self.gt, self.image = False, None, None

    def get_image_embedding(self):
        """A deterministic stand-in of the SHAPE of SAM's image embedding, [1,256,64,64] fp32 on the target's device - NOT an embedding of
        anything learned: the 64 x 64 area means of the uint8 image handed to ``set_image``, scaled to 0..1, times a fixed 256 x 3 matrix
        drawn from a Philox stream.  Equal images give equal values, different images different ones; that is all an agent with recipe
        weights needs."""
        import torch
        import torch.nn.functional as F
        assert self.embedded and self.image is not None, "get_image_embedding is called before set_image"
        img = torch.from_numpy(np.ascontiguousarray(self.image, dtype=np.uint8)).permute(2, 0, 1)[None].float() / 255
        means = F.adaptive_avg_pool2d(img, 64)[0]                                      # [3,64,64]
        m = np.random.Generator(np.random.Philox(key=[self.EMBED_SEED, 256])).normal(0, 1, (256, 3)).astype(np.float32)
        emb = torch.einsum("kc,chw->khw", torch.from_numpy(m), means)[None].contiguous()
        return emb.to(self.device) if self.device is not None else emb

    def predict(self, click_coords=None, click_labels=None, bbox=None, mask_input=None, multimask_output=True):
        import torch
        from scipy import ndimage
        assert self.embedded, "prediction is called before set_image"
        gt, ones = self.gt, np.ones((3, 3), bool)
        box = None
        if bbox is not None:
            x1, y1, x2, y2 = (int(v) for v in np.asarray(bbox).reshape(-1)[:4])
            box = np.zeros_like(gt)
            box[y1:y2 + 1, x1:x2 + 1] = True
        if mask_input is not None:
            cur = np.asarray(mask_input)[0] > 0
            if box is not None:
                cur &= box
        else:
            cur = box.copy() if box is not None else np.zeros_like(gt)
        if click_coords is not None:
            for (x, y), label in zip(np.asarray(click_coords).tolist(), np.asarray(click_labels).tolist()):
                region = (~cur & gt) if label == 1 else (cur & ~gt)
                if region[int(y), int(x)]:
                    lab, _ = ndimage.label(region, structure=ones)
                    comp = lab == lab[int(y), int(x)]
                    cur = (cur | comp) if label == 1 else (cur & ~comp)
        variants = np.stack([ndimage.binary_erosion(cur, ones), ndimage.binary_dilation(cur, ones), ndimage.binary_dilation(cur, ones, iterations=2)])
        logits = np.where(variants, np.float32(4), np.float32(-4))
        masks = torch.from_numpy(variants).unsqueeze(1)
        if self.device is not None:
            masks = masks.to(self.device)
        return masks, np.array([0.9, 0.8, 0.7], np.float32), logits
