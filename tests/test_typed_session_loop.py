"""CPU: the session loop behind the mixed-annotation policies (eval_driver.run_typed_policy: rand_type, rand_rand, oracle_oracle) and behind
``eva_vos`` (eval_driver.run_eva_vos) on the fakes of session_fakes.py, which record every call.  The expected logs, return values and
``stats`` below were recorded from the loop these policies had to themselves, before the mask policies and they shared one; the shared loop
reproduces them call for call: what is handed to ``interact`` and to ``set_annotation``, the prompts carried from one annotation of a frame
to the next, ``score``'s frames and types, which rounds read ``qualities()``, the skip rules, and the order of the random draws."""
import random

import numpy as np
import pytest
import torch

from eva_vos_amd import eval_driver
from session_fakes import Agent, Annotator, Proc, Scorer, Selector, clip

# policy, annotation types, T, rounds, frames without the object, seed
TYPED = {
    "rand_type_clicks_repeat": ("rand_type", ["3clicks"], 4, 6, [], 2),           # a frame is annotated twice: its prompts come back
    "rand_type_mask_nothing_left": ("rand_type", ["mask"], 3, 6, [], 0),         # every frame chosen after two rounds: the nothing-left skip
    "rand_rand_click_then_mask": ("rand_rand", ["click", "mask"], 4, 8, [], 2),  # a type-2 frame later gets its mask; rounds > T
    "rand_rand_no_object": ("rand_rand", ["click", "mask"], 5, 7, [2], 3),       # a frame without the object is drawn
    "oracle_oracle_second_box": ("oracle_oracle", ["click", "bbox", "mask"], 4, 6, [3], None),      # frame 1 twice: no second box; r >= T
    "rand_type_rounds_run_out": ("rand_type", ["3clicks"], 5, 3, [4], 6),         # rounds < T: ends with a frame pending
}
# T, rounds, frames without the object, the selector's answers, the agent's (action, value) answers: the sessions of test_eva_vos_api
EVA_VOS = {
    "eva_vos_no_object_repeat_switch_skip": (5, 10, [4], [4, 1, 1, 2, 2, 3], [(0, 0.25), (1, 0.5), (0, -1.5), (1, 2.0)]),
    "eva_vos_masks_only": (3, 6, [], [1, 2], [(1, 0.75)]),
    "eva_vos_rounds_run_out": (5, 3, [4], [4, 1, 1], [(0, 0.25)]),
}


class LoggingRandom:
    """The session's generator, a ``random.Random(seed)``; every ``choice`` goes to the log with what it chose from."""

    def __init__(self, seed, log):
        self.rng, self.log = random.Random(seed), log

    def choice(self, seq):
        got = self.rng.choice(seq)
        self.log.append(("choice", list(seq), got))
        return got


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def _session(name):
    """(call log, return value, stats) of one session on the fakes."""
    log, stats = [], {}
    if name in TYPED:
        policy, ann_types, T, rounds, empty_frames, seed = TYPED[name]
        gt, rgb = clip(T, empty_frames)
        ret = eval_driver.run_typed_policy(policy, Proc(log), {"num_frames": T, "gt": gt[None], "rgb": rgb}, rounds, Annotator(log), ann_types, "j_and_f",
                                           rng=LoggingRandom(seed, log), stats=stats, scorer=Scorer(gt[:, 0], log, trace=True))
    else:
        T, rounds, empty_frames, picks, acts = EVA_VOS[name]
        gt, rgb = clip(T, empty_frames)
        ret = eval_driver.run_eva_vos(Proc(log), {"num_frames": T, "gt": gt[None], "rgb": rgb}, rounds, Annotator(log), "qnet", Agent(acts, log), "j_and_f",
                                      rng=torch.Generator().manual_seed(3), stats=stats, scorer=Scorer(gt[:, 0], log, trace=True), selector=Selector(picks, log))
        log = [e[:3] if e[0] == "act" else e for e in log]          # the generator object itself is no literal
    return _plain(log), _plain(ret), stats


# (call log, return value, stats) per case, recorded once from the typed loop before the loops were merged
EXPECTED = {'eva_vos_masks_only': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['select', 1, [0]],
                         ['embedding', [3, 2, 2], [0, 1, 0, 0]], ['act', 'embedding', ['input', 1, [1]]],
                         ['annotate', 'mask', [1, 1, 1, 1], [], None], ['interact', 1, [1, 1, 2, 2], [0, 1, 0, 0]],
                         ['score', [0, 1], False, True, [1, 1]], ['select', 2, [0, 1]], ['qualities', 2], ['qualities', 2], ['qualities', 2],
                         ['qualities', 2], ['qualities', 2]],
                        {'annotated_frames': [0, 1],
                         'annotation_times': [80, 80],
                         'annotations_actions': ['mask', 'mask'],
                         'frames': [0, 1],
                         'mu_metrics': [0.6666666666666666, 0.8333333333333334],
                         'propagated_frames': 6,
                         'rl_values': [-2, 0.75],
                         'round_metrics': [[1.0, 0.5, 0.5], [1.0, 1.0, 0.5]],
                         'types': [1, 1]},
                        {'interactions': 2, 'propagated_frames': 6}),
 'eva_vos_no_object_repeat_switch_skip': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['select', 1, [0]],
                                           ['annotation', 4, [0, 0, 0, 0]], ['interact', 4, [1, 1, 2, 2], [0, 0, 0, 0]],
                                           ['score', [0, 4], False, True, [1, 2]], ['select', 2, [0, 4]], ['embedding', [3, 2, 2], [0, 1, 0, 0]],
                                           ['act', 'embedding', ['input', 2, [1]]], ['annotate', '3clicks', [1, 1, 1, 1], [], None],
                                           ['annotation', 1, [1, 0, 1, 1]], ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]],
                                           ['score', [0, 4, 1], False, True, [1, 2, 2]], ['select', 3, [0, 4, 1]],
                                           ['embedding', [3, 2, 2], [0, 1, 0, 0]], ['act', 'embedding', ['input', 3, [1]]],
                                           ['annotate', 'mask', [1, 1, 1, 1], ['3clicks'], 'clicks'], ['interact', 1, [1, 1, 2, 2], [0, 1, 0, 0]],
                                           ['score', [0, 4, 1, 1], False, True, [1, 2, 2, 1]], ['select', 4, [0, 4, 1, 1]], ['qualities', 4],
                                           ['embedding', [3, 2, 2], [1, 0, 0, 0]], ['act', 'embedding', ['input', 4, [2]]],
                                           ['annotate', '3clicks', [1, 1, 1, 1], [], None], ['annotation', 2, [0, 1, 1, 1]],
                                           ['interact', 2, [1, 1, 2, 2], [0, 1, 1, 1]], ['score', [0, 4, 1, 1, 2], False, True, [1, 2, 2, 1, 2]],
                                           ['select', 5, [2, 3, 4]], ['qualities', 5], ['embedding', [3, 2, 2], [1, 0, 0, 0]],
                                           ['act', 'embedding', ['input', 5, [2]]], ['annotate', 'mask', [1, 1, 1, 1], ['3clicks'], 'clicks'],
                                           ['interact', 2, [1, 1, 2, 2], [1, 0, 0, 0]],
                                           ['score', [0, 4, 1, 1, 2, 2], False, True, [1, 2, 2, 1, 2, 1]], ['select', 6, [3, 4]], ['qualities', 6],
                                           ['qualities', 6], ['qualities', 6], ['qualities', 6], ['qualities', 6]],
                                          {'annotated_frames': [0, 4, 1, 1, 2, 2],
                                           'annotation_times': [80, 3, 4.5, 80, 4.5, 80],
                                           'annotations_actions': ['mask', 'no_object', '3clicks', 'mask', '3clicks', 'mask'],
                                           'frames': [0, 4, 1, 1, 2, 2],
                                           'mu_metrics': [0.625, 0.625, 0.625, 0.75, 0.75, 0.875],
                                           'propagated_frames': 18,
                                           'rl_values': [-2, 0, 0.25, 0.5, -1.5, 2.0],
                                           'round_metrics': [[1.0, 0.5, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 0.5, 20.0],
                                                             [1.0, 1.0, 0.5, 0.5, 20.0], [1.0, 1.0, 0.5, 0.5, 20.0], [1.0, 1.0, 1.0, 0.5, 20.0]],
                                           'types': [1, 2, 2, 1, 2, 1]},
                                          {'interactions': 6, 'propagated_frames': 18}),
 'eva_vos_rounds_run_out': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['select', 1, [0]],
                             ['annotation', 4, [0, 0, 0, 0]], ['interact', 4, [1, 1, 2, 2], [0, 0, 0, 0]], ['score', [0, 4], False, True, [1, 2]],
                             ['select', 2, [0, 4]], ['embedding', [3, 2, 2], [0, 1, 0, 0]], ['act', 'embedding', ['input', 2, [1]]],
                             ['annotate', '3clicks', [1, 1, 1, 1], [], None], ['annotation', 1, [1, 0, 1, 1]],
                             ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 4, 1], False, True, [1, 2, 2]], ['select', 3, [0, 4, 1]],
                             ['qualities', 3]],
                            {'annotated_frames': [0, 4, 1],
                             'annotation_times': [80, 3, 4.5],
                             'annotations_actions': ['mask', 'no_object', '3clicks'],
                             'frames': [0, 4, 1],
                             'mu_metrics': [0.625, 0.625, 0.625],
                             'propagated_frames': 9,
                             'rl_values': [-2, 0, 0.25],
                             'round_metrics': [[1.0, 0.5, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 0.5, 20.0]],
                             'types': [1, 2, 2]},
                            {'interactions': 3, 'propagated_frames': 9}),
 'oracle_oracle_second_box': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['iou', [1, 1, 1, 1]],
                               ['annotate', 'click', [1, 1, 1, 1], [], None], ['annotate', 'bbox', [1, 1, 1, 1], [], None],
                               ['annotate', 'mask', [1, 1, 1, 1], [], None], ['annotation', 1, [1, 0, 1, 1]],
                               ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1], False, True, [1, 2]], ['iou', [1, 1, 1, 1]],
                               ['annotate', 'click', [1, 1, 1, 1], ['bbox'], 'clicks'], ['annotate', 'mask', [1, 1, 1, 1], ['bbox'], 'clicks'],
                               ['annotation', 1, [1, 0, 1, 1]], ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]],
                               ['score', [0, 1, 1], False, True, [1, 2, 2]], ['qualities', 3], ['iou', [1, 1, 1, 1]],
                               ['annotate', 'click', [1, 1, 1, 1], ['bbox', 'click'], 'clicks'],
                               ['annotate', 'mask', [1, 1, 1, 1], ['bbox', 'click'], 'clicks'], ['annotation', 1, [1, 0, 1, 1]],
                               ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1, 1, 1], False, True, [1, 2, 2, 2]], ['qualities', 4],
                               ['iou', [1, 1, 1, 1]], ['annotate', 'click', [1, 1, 1, 1], ['bbox', 'click', 'click'], 'clicks'],
                               ['annotate', 'mask', [1, 1, 1, 1], ['bbox', 'click', 'click'], 'clicks'], ['annotation', 1, [1, 0, 1, 1]],
                               ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1, 1, 1, 1], False, True, [1, 2, 2, 2, 2]],
                               ['qualities', 5], ['iou', [1, 1, 1, 1]],
                               ['annotate', 'click', [1, 1, 1, 1], ['bbox', 'click', 'click', 'click'], 'clicks'],
                               ['annotate', 'mask', [1, 1, 1, 1], ['bbox', 'click', 'click', 'click'], 'clicks'], ['annotation', 1, [1, 0, 1, 1]],
                               ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1, 1, 1, 1, 1], False, True, [1, 2, 2, 2, 2, 2]],
                               ['qualities', 6]],
                              {'action_data': [{'bbox': {'cost': 4.5, 'iou': 0.7, 'reward': 0.09999999999999999},
                                                'click': {'cost': 4.5, 'iou': 0.7, 'reward': 0.09999999999999999},
                                                'frame_num': 1,
                                                'init_iou': 0.25,
                                                'mask': {'cost': 80, 'iou': 1, 'reward': 0.009375},
                                                'selected_action': 'bbox'},
                                               {'click': {'cost': 4.5, 'iou': 0.7, 'reward': 0.09999999999999999},
                                                'frame_num': 1,
                                                'init_iou': 0.25,
                                                'mask': {'cost': 80, 'iou': 1, 'reward': 0.009375},
                                                'selected_action': 'click'},
                                               {'click': {'cost': 4.5, 'iou': 0.7, 'reward': 0.09999999999999999},
                                                'frame_num': 1,
                                                'init_iou': 0.25,
                                                'mask': {'cost': 80, 'iou': 1, 'reward': 0.009375},
                                                'selected_action': 'click'},
                                               {'click': {'cost': 4.5, 'iou': 0.7, 'reward': 0.09999999999999999},
                                                'frame_num': 1,
                                                'init_iou': 0.25,
                                                'mask': {'cost': 80, 'iou': 1, 'reward': 0.009375},
                                                'selected_action': 'click'},
                                               {'click': {'cost': 4.5, 'iou': 0.7, 'reward': 0.09999999999999999},
                                                'frame_num': 1,
                                                'init_iou': 0.25,
                                                'mask': {'cost': 80, 'iou': 1, 'reward': 0.009375},
                                                'selected_action': 'click'}],
                               'annotated_frames': [0, 1, 1, 1, 1, 1],
                               'annotation_times': [80, 4.5, 4.5, 4.5, 4.5, 4.5],
                               'annotations_actions': ['mask', 'bbox', 'click', 'click', 'click', 'click'],
                               'frames': [0, 1, 1, 1, 1, 1],
                               'mu_metrics': [0.6666666666666666, 0.6666666666666666, 0.6666666666666666, 0.6666666666666666, 0.6666666666666666,
                                              0.6666666666666666],
                               'propagated_frames': 18,
                               'round_metrics': [[1.0, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 20.0],
                                                 [1.0, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 20.0]],
                               'types': [1, 2, 2, 2, 2, 2]},
                              {'interactions': 6, 'propagated_frames': 18}),
 'rand_rand_click_then_mask': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['choice', [1, 2, 3], 1],
                                ['choice', ['click', 'mask'], 'click'], ['annotate', 'click', [1, 1, 1, 1], [], None],
                                ['annotation', 1, [1, 0, 1, 1]], ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1], False, True, [1, 2]],
                                ['choice', [1, 2, 3], 1], ['choice', ['click', 'mask'], 'mask'],
                                ['annotate', 'mask', [1, 1, 1, 1], ['click'], 'clicks'], ['interact', 1, [1, 1, 2, 2], [0, 1, 0, 0]],
                                ['score', [0, 1, 1], False, True, [1, 2, 1]], ['choice', [2, 3], 2], ['qualities', 3],
                                ['choice', ['click', 'mask'], 'mask'], ['annotate', 'mask', [1, 1, 1, 1], [], None],
                                ['interact', 2, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0, 1, 1, 2], False, True, [1, 2, 1, 1]], ['choice', [3], 3],
                                ['qualities', 4], ['qualities', 4], ['qualities', 4], ['qualities', 4], ['qualities', 4]],
                               {'action_data': [],
                                'annotated_frames': [0, 1, 1, 2],
                                'annotation_times': [80, 4.5, 80, 80],
                                'annotations_actions': ['mask', 'click', 'mask', 'mask'],
                                'frames': [0, 1, 1, 2],
                                'mu_metrics': [0.625, 0.625, 0.75, 0.875],
                                'propagated_frames': 12,
                                'round_metrics': [[1.0, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5], [1.0, 1.0, 0.5, 0.5], [1.0, 1.0, 1.0, 0.5]],
                                'types': [1, 2, 1, 1]},
                               {'interactions': 4, 'propagated_frames': 12}),
 'rand_rand_no_object': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['choice', [1, 2, 3, 4], 2],
                          ['choice', ['click', 'mask'], 'click'], ['annotate', 'click', [1, 1, 1, 1], [], None], ['annotation', 2, [1, 1, 1, 1]],
                          ['interact', 2, [1, 1, 2, 2], [1, 1, 1, 1]], ['score', [0, 2], False, True, [1, 2]], ['choice', [1, 2, 3, 4], 3],
                          ['choice', ['click', 'mask'], 'mask'], ['annotate', 'mask', [1, 1, 1, 1], [], None],
                          ['interact', 3, [1, 1, 2, 2], [0, 1, 0, 0]], ['score', [0, 2, 3], False, True, [1, 2, 1]], ['choice', [1, 2, 4], 4],
                          ['choice', ['click', 'mask'], 'click'], ['annotate', 'click', [1, 1, 1, 1], [], None], ['annotation', 4, [0, 1, 1, 1]],
                          ['interact', 4, [1, 1, 2, 2], [0, 1, 1, 1]], ['score', [0, 2, 3, 4], False, True, [1, 2, 1, 2]], ['choice', [1, 2, 4], 4],
                          ['qualities', 4], ['choice', ['click', 'mask'], 'click'], ['annotate', 'click', [1, 1, 1, 1], ['click'], 'clicks'],
                          ['annotation', 4, [0, 1, 1, 1]], ['interact', 4, [1, 1, 2, 2], [0, 1, 1, 1]],
                          ['score', [0, 2, 3, 4, 4], False, True, [1, 2, 1, 2, 2]], ['choice', [1, 2, 4], 2], ['qualities', 5],
                          ['choice', ['click', 'mask'], 'mask'], ['annotate', 'mask', [1, 1, 1, 1], ['click'], 'clicks'],
                          ['interact', 2, [1, 1, 2, 2], [0, 0, 0, 0]], ['score', [0, 2, 3, 4, 4, 2], False, True, [1, 2, 1, 2, 2, 1]],
                          ['choice', [1, 4], 1], ['qualities', 6], ['qualities', 6]],
                         {'action_data': [],
                          'annotated_frames': [0, 2, 3, 4, 4, 2],
                          'annotation_times': [80, 4.5, 80, 4.5, 4.5, 80],
                          'annotations_actions': ['mask', 'click', 'mask', 'click', 'click', 'mask'],
                          'frames': [0, 2, 3, 4, 4, 2],
                          'mu_metrics': [0.625, 0.625, 0.75, 0.75, 0.75, 0.75],
                          'propagated_frames': 18,
                          'round_metrics': [[1.0, 0.5, 20.0, 0.5, 0.5], [1.0, 0.5, 20.0, 0.5, 0.5], [1.0, 0.5, 20.0, 1.0, 0.5],
                                            [1.0, 0.5, 20.0, 1.0, 0.5], [1.0, 0.5, 20.0, 1.0, 0.5], [1.0, 0.5, 20.0, 1.0, 0.5]],
                          'types': [1, 2, 1, 2, 2, 1]},
                         {'interactions': 6, 'propagated_frames': 18}),
 'rand_type_clicks_repeat': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['choice', [1, 2, 3], 1],
                              ['annotate', '3clicks', [1, 1, 1, 1], [], None], ['annotation', 1, [1, 0, 1, 1]],
                              ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1], False, True, [1, 2]], ['choice', [1, 2, 3], 1],
                              ['annotate', '3clicks', [1, 1, 1, 1], ['3clicks'], 'clicks'], ['annotation', 1, [1, 0, 1, 1]],
                              ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1, 1], False, True, [1, 2, 2]], ['choice', [1, 2, 3], 1],
                              ['qualities', 3], ['annotate', '3clicks', [1, 1, 1, 1], ['3clicks', '3clicks'], 'clicks'],
                              ['annotation', 1, [1, 0, 1, 1]], ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]],
                              ['score', [0, 1, 1, 1], False, True, [1, 2, 2, 2]], ['choice', [1, 2, 3], 2], ['qualities', 4],
                              ['annotate', '3clicks', [1, 1, 1, 1], [], None], ['annotation', 2, [0, 1, 1, 1]],
                              ['interact', 2, [1, 1, 2, 2], [0, 1, 1, 1]], ['score', [0, 1, 1, 1, 2], False, True, [1, 2, 2, 2, 2]],
                              ['choice', [1, 2, 3], 1], ['qualities', 5],
                              ['annotate', '3clicks', [1, 1, 1, 1], ['3clicks', '3clicks', '3clicks'], 'clicks'], ['annotation', 1, [1, 0, 1, 1]],
                              ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1, 1, 1, 2, 1], False, True, [1, 2, 2, 2, 2, 2]],
                              ['choice', [1, 2, 3], 3], ['qualities', 6]],
                             {'action_data': [],
                              'annotated_frames': [0, 1, 1, 1, 2, 1],
                              'annotation_times': [80, 4.5, 4.5, 4.5, 4.5, 4.5],
                              'annotations_actions': ['mask', '3clicks', '3clicks', '3clicks', '3clicks', '3clicks'],
                              'frames': [0, 1, 1, 1, 2, 1],
                              'mu_metrics': [0.625, 0.625, 0.625, 0.625, 0.625, 0.625],
                              'propagated_frames': 18,
                              'round_metrics': [[1.0, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5],
                                                [1.0, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5]],
                              'types': [1, 2, 2, 2, 2, 2]},
                             {'interactions': 6, 'propagated_frames': 18}),
 'rand_type_mask_nothing_left': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['choice', [1, 2], 2],
                                  ['annotate', 'mask', [1, 1, 1, 1], [], None], ['interact', 2, [1, 1, 2, 2], [1, 0, 0, 0]],
                                  ['score', [0, 2], False, True, [1, 1]], ['choice', [1], 1], ['qualities', 2], ['qualities', 2], ['qualities', 2],
                                  ['qualities', 2], ['qualities', 2]],
                                 {'action_data': [],
                                  'annotated_frames': [0, 2],
                                  'annotation_times': [80, 80],
                                  'annotations_actions': ['mask', 'mask'],
                                  'frames': [0, 2],
                                  'mu_metrics': [0.6666666666666666, 0.8333333333333334],
                                  'propagated_frames': 6,
                                  'round_metrics': [[1.0, 0.5, 0.5], [1.0, 0.5, 1.0]],
                                  'types': [1, 1]},
                                 {'interactions': 2, 'propagated_frames': 6}),
 'rand_type_rounds_run_out': ([['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0]], ['score', [0], False, True, [1]], ['choice', [1, 2, 3, 4], 1],
                               ['annotate', '3clicks', [1, 1, 1, 1], [], None], ['annotation', 1, [1, 0, 1, 1]],
                               ['interact', 1, [1, 1, 2, 2], [1, 0, 1, 1]], ['score', [0, 1], False, True, [1, 2]], ['choice', [1, 2, 3, 4], 4],
                               ['annotate', '3clicks', [1, 1, 1, 1], [], None], ['annotation', 4, [1, 1, 1, 1]],
                               ['interact', 4, [1, 1, 2, 2], [1, 1, 1, 1]], ['score', [0, 1, 4], False, True, [1, 2, 2]], ['choice', [1, 2, 3, 4], 3],
                               ['qualities', 3]],
                              {'action_data': [],
                               'annotated_frames': [0, 1, 4],
                               'annotation_times': [80, 4.5, 4.5],
                               'annotations_actions': ['mask', '3clicks', '3clicks'],
                               'frames': [0, 1, 4],
                               'mu_metrics': [0.625, 0.625, 0.625],
                               'propagated_frames': 9,
                               'round_metrics': [[1.0, 0.5, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 0.5, 20.0], [1.0, 0.5, 0.5, 0.5, 20.0]],
                               'types': [1, 2, 2]},
                              {'interactions': 3, 'propagated_frames': 9})}


@pytest.mark.parametrize("name", sorted(TYPED) + sorted(EVA_VOS))
def test_the_typed_session_loop_reproduces_the_recorded_calls_and_results(name):
    assert _session(name) == EXPECTED[name]


def _of(name, kind):
    return [e for e in EXPECTED[name][0] if e[0] == kind]


def test_the_recorded_sessions_reach_the_branches_they_are_named_for():
    # a frame annotated twice with clicks: the second annotation starts from the prompts the first one left
    log, ret, _ = EXPECTED["rand_type_clicks_repeat"]
    assert ret["frames"][:3] == [0, 1, 1] and [e[3:] for e in _of("rand_type_clicks_repeat", "annotate")[:2]] == [[[], None], [["3clicks"], "clicks"]]
    # nothing left to annotate: three frames, six rounds, two scored; the four skipped rounds are r >= T and read the quality, as the epilogue does
    log, ret, stats = EXPECTED["rand_type_mask_nothing_left"]
    assert len(ret["frames"]) == 2 and stats["interactions"] == 2 and _of("rand_type_mask_nothing_left", "qualities") == [["qualities", 2]] * (4 + 1)
    assert _of("rand_type_mask_nothing_left", "choice")[-1] == ["choice", [1], 1]                        # the frame left pending is never annotated
    # rand_rand: within every round after the first the action is drawn before the engine runs, the next frame after it
    log, ret, _ = EXPECTED["rand_rand_click_then_mask"]
    kinds = ["i" if e[0] == "interact" else "a" if e[1] == ["click", "mask"] else "f" for e in log if e[0] in ("interact", "choice")]
    assert kinds == ["i"] + ["f", "a", "i"] * (len(ret["frames"]) - 1) + ["f"]
    assert ret["frames"][1:3] == [1, 1] and ret["types"][1:3] == [2, 1]                                   # the clicked frame gets its mask
    assert len(_of("rand_rand_click_then_mask", "annotation")) == 1 and ["qualities", 3] in log        # rounds > T: min == 1 is evaluated from r = T on
    # a frame without the object is drawn, clicked, and later annotated with its (empty) mask
    log, ret, _ = EXPECTED["rand_rand_no_object"]
    assert ret["frames"][1] == ret["frames"][-1] == 2 and ["interact", 2, [1, 1, 2, 2], [0, 0, 0, 0]] in log and all(row[2] == 20.0 for row in ret["round_metrics"])
    # oracle_oracle: frame 1 is chosen again and again; the box that won the first time is not tried a second time
    log, ret, _ = EXPECTED["oracle_oracle_second_box"]
    assert ret["frames"] == [0, 1, 1, 1, 1, 1] and ret["annotations_actions"][:3] == ["mask", "bbox", "click"]
    tried = [[e[1] for e in _of("oracle_oracle_second_box", "annotate") if e[3] == seen] for seen in ([], ["bbox"])]
    assert tried == [["click", "bbox", "mask"], ["click", "mask"]] and "bbox" not in ret["action_data"][1]
    assert [e[1] for e in _of("oracle_oracle_second_box", "qualities")] == [3, 4, 5, 6]                  # rounds 4..6 are r >= T; the epilogue
    # rounds < T: three rounds scored, a fourth frame drawn and left pending; the quality is read once, at the end
    log, ret, stats = EXPECTED["rand_type_rounds_run_out"]
    assert len(ret["frames"]) == 3 == stats["interactions"] and len(_of("rand_type_rounds_run_out", "choice")) == 3
    assert 4 in ret["frames"] and _of("rand_type_rounds_run_out", "qualities") == [["qualities", 3]]
    # eva_vos: the sessions of test_eva_vos_api, here with the scorer's side of them
    log, ret, _ = EXPECTED["eva_vos_no_object_repeat_switch_skip"]
    assert ret["annotations_actions"] == ["mask", "no_object", "3clicks", "mask", "3clicks", "mask"]
    assert _of("eva_vos_no_object_repeat_switch_skip", "score")[-1][4] == [1, 2, 2, 1, 2, 1]
    assert [e[2] for e in _of("eva_vos_no_object_repeat_switch_skip", "select")][-2:] == [[2, 3, 4], [3, 4]]      # r >= T: the frames without a mask
    assert len(EXPECTED["eva_vos_rounds_run_out"][1]["frames"]) == 3 and EXPECTED["eva_vos_masks_only"][1]["frames"] == [0, 1]
