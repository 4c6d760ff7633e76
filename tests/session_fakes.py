"""Fakes of what an annotation session touches - the engine, the round scorers, the annotator, the agent, the QNet selector - that record
every call, shared by the CPU tests of the session loop and of the drivers (test_eva_vos_api, test_typed_session_loop, test_shared_frames,
test_driver_rows).  A plain module, not a conftest: the tests import what they use."""
import types

import numpy as np
import torch

from eva_vos_amd import metrics

NO = 20.0                                                       # the drivers' NO_OBJECT token


def quality(cur_types, empty):
    """The fake evaluation of the typed sessions: 1 on a frame annotated with its mask, 0.5 elsewhere, the token on a frame without the object."""
    q = np.where(np.asarray(cur_types) == 1, 1.0, 0.5)
    q[empty] = NO
    return q


def gen_masks(T, r):
    return torch.full((T, 2, 2), r, dtype=torch.uint8)


def clip(T, empty_frames):
    """(gt [T,1,2,2], rgb [1,T,3,2,2]): one pixel of object per frame, none on ``empty_frames``."""
    gt = torch.zeros((T, 1, 2, 2))
    for t in range(T):
        gt[t, 0, 0, t % 2] = 1
    for t in empty_frames:
        gt[t] = 0
    return gt, torch.zeros((1, T, 3, 2, 2))


class Proc:
    def __init__(self, log):
        self.log, self.prob, self.calls = log, types.SimpleNamespace(device=torch.device("cpu")), 0

    def interact(self, mask, f, **kw):
        self.calls += 1
        self.log.append(("interact", int(f), list(mask.shape), mask.flatten().int().tolist()))

    def stats(self):
        return {"frames": 3}


class Scorer:
    """``TypedRoundScorer``'s interface over ``quality``.  ``trace``: ``score``'s frames and types and every ``qualities()`` call go to the log."""

    def __init__(self, gt_thw, log, trace=False):
        self.T, self.log, self.rows, self.trace = gt_thw.shape[0], log, [], trace
        self.empty_host = (gt_thw.flatten(1).sum(1) == 0).numpy()

    def set_annotation(self, frame, mask):
        self.log.append(("annotation", int(frame), mask.flatten().int().tolist()))

    def score(self, processor, annotated_frames, keep_gen=True, incremental=True, types=None):
        if self.trace:
            self.log.append(("score", [int(f) for f in annotated_frames], keep_gen, incremental, None if types is None else [int(t) for t in types]))
        cur = metrics._current_types(self.T, annotated_frames, types)
        self.rows.append(quality(cur, self.empty_host))
        return int(np.argmin(self.rows[-1])), gen_masks(self.T, len(self.rows))

    def qualities(self):
        if self.trace:
            self.log.append(("qualities", len(self.rows)))
        return np.stack(self.rows)


class Annotator:
    def __init__(self, log):
        self.log = log

    def image_embedding(self, im, gt_mask):
        self.log.append(("embedding", list(im.shape), gt_mask.flatten().int().tolist()))
        return "embedding"

    def iou(self, mask, gt_mask):
        self.log.append(("iou", mask.flatten().int().tolist()))
        return 0.25

    def annotate(self, annot_type, gt_mask, im=None, mivos_mask=None, frame_annots=None, empty=None):
        self.log.append(("annotate", annot_type, mivos_mask.flatten().int().tolist(), list(frame_annots["annotations"]), frame_annots["click_coords"]))
        if annot_type == "mask":
            return gt_mask, 80, 1, None, None, None, None
        return 1 - gt_mask, 4.5, 0.7, "logits", "clicks", "labels", None         # a mask that is not the ground truth


class Agent:
    def __init__(self, script, log):
        self.script, self.log = list(script), log

    def act(self, x_img, x_mask, generator=None):
        action, value = self.script.pop(0)
        self.log.append(("act", x_img, x_mask, generator))
        return action, torch.tensor([[value]])


class Selector:
    def __init__(self, script, log):
        self.script, self.log = list(script), log

    def masks_to_input(self, gen, frames=None):
        return ("input", int(gen[0, 0, 0]), list(frames))

    def select(self, gen, interacted):
        self.log.append(("select", int(gen[0, 0, 0]), [int(f) for f in interacted]))
        return self.script.pop(0)


# ------------------------------------------------------------------------------------------------ the drivers' fakes
class DriverScorer:
    """metrics.RoundScorer's surface as the session loop uses it: every frame holds the object, the worst frame is the first one not
    annotated yet."""

    def __init__(self, gt_thw, metric="j", max_rounds=64, no_object=20.0, num_objects=None):
        self.T, self.rounds = int(gt_thw.shape[0]), 0
        self.empty_host = np.zeros(self.T, bool)

    def score(self, processor, annotated_frames, keep_gen=True, incremental=True):
        self.rounds += 1
        return min(set(range(self.T)) - set(annotated_frames)), torch.zeros((self.T, 2, 2), dtype=torch.uint8)

    def qualities(self):
        return np.full((self.rounds, self.T), 0.5)


def fake_core_class(log):
    class Core:
        """InferenceCore's surface as the drivers use it.  A frame is key-encoded when an interaction first needs it; the features of a
        clip survive ``reset(keep_frame_features=True)`` only."""

        def __init__(self, prop_net, fuse_net, images, num_objects, mem_profile=0, mem_freq=5, device="cuda", engine_options=None):
            self.t = int(images.shape[1])
            self.images, self.cached, self.key_frames_encoded = images, False, 0
            self.prob = types.SimpleNamespace(device=torch.device("cpu"))
            log.append(("new", self.t, int(num_objects), engine_options))

        def interact(self, mask, idx, scribble=False, download=True):
            if not self.cached:
                self.key_frames_encoded += self.t
                self.cached = True
            log.append(("interact", self.t, int(idx)))

        def reset(self, keep_frame_features=False):
            log.append(("reset", self.t, keep_frame_features))
            self.key_frames_encoded = 0
            self.cached = self.cached and keep_frame_features
            return self.t if self.cached else 0

        def stats(self):
            return {"frames": self.t - 1}
    return Core


class DriverObjectScorer(DriverScorer):
    """The k-object side of it: per-object rows that differ by round, object and frame; the last object is absent from frame 1."""

    def __init__(self, gt_thw, metric="j", max_rounds=64, no_object=20.0, num_objects=None):
        super().__init__(gt_thw)
        self.k, self.gt = num_objects, gt_thw
        self.present_host = np.ones((num_objects, self.T), bool)
        self.present_host[-1, 1] = False

    def object_qualities(self):
        oq = np.array([[[(16 * (i + 1) + 4 * o + t) / 128 for t in range(self.T)] for o in range(self.k)] for i in range(self.rounds)], np.float64)
        return oq.reshape(self.rounds, self.k, self.T)


class DriverTypedScorer(Scorer):
    """metrics.TypedRoundScorer's constructor over ``Scorer``."""

    def __init__(self, gt_thw, metric="j", max_rounds=64, no_object=20.0):
        super().__init__(gt_thw, [])


class CyclingAgent:
    """An agent all sessions of a run share: clicks and masks in turn, a value that counts the calls."""

    def __init__(self):
        self.calls = 0

    def act(self, x_img, x_mask, generator=None):
        self.calls += 1
        return self.calls % 2, torch.tensor([[0.125 * self.calls]])


class DriverSelector:
    """qnet.QNetSelector's surface: given an odd number of frames, the first frame that is not among them (frame 0 when there is none); given
    an even number, the last of them once more - so frames repeat."""

    def __init__(self, qnet, images):
        self.T = int(images.shape[0])

    def masks_to_input(self, gen, frames=None):
        return ("input", list(frames))

    def select(self, gen, interacted):
        given = [int(i) for i in interacted]
        left = [f for f in range(self.T) if f not in given]
        return given[-1] if len(given) % 2 == 0 else left[0] if left else 0
