"""CPU: the annotation-session loop of the drivers (fq_driver.oracle_rounds, eval_driver.run_policy in its per-object and its multi-object
mode) on a fake processor and a fake scorer that record every call.  The expected call sequences and return values below were recorded
from the three separate loops the drivers had before they shared one; the shared loop has to reproduce them call for call: the
``r >= T`` skip, the nothing-left-to-annotate skip, what is handed to ``interact`` and to ``score``, the ``stats`` bookkeeping and the
order in which the random generator is consumed."""
import random
import types

import numpy as np
import pytest
import torch

from eva_vos_amd import eval_driver, fq_driver, metrics

T, ROUNDS, K = 4, 6, 2
NO = fq_driver.NO_OBJECT


def _labels(last_frame_empty):
    lab = torch.zeros((T, 2, 2), dtype=torch.uint8)
    for t in range(T):
        lab[t, 0, 0], lab[t, 1, t % 2] = 1, 2          # object 1 top-left; object 2 in the bottom row, moving
    if last_frame_empty:
        lab[T - 1] = 0
    return lab


class _Gen(str):
    """The fake scorer's gen token with the ``float()`` the QNet policy calls on the evaluated masks."""
    def float(self):
        return self + ".float"


class Proc:
    def __init__(self, log):
        self.log, self.prob, self.calls = log, types.SimpleNamespace(device=torch.device("cpu")), 0

    def interact(self, mask, f, **kw):
        self.calls += 1
        self.log.append(("interact", f, list(mask.shape), mask.flatten().int().tolist(), sorted(kw.items())))

    def stats(self):
        return {"frames": 10 * self.calls + 1}


def _scorer_class(log, worsts):
    class Scorer:
        def __init__(self, gt_thw, metric="j", max_rounds=64, no_object=20.0, num_objects=None):
            log.append(("scorer", list(gt_thw.shape), metric, max_rounds, no_object, num_objects))
            self.k, self.rounds, self.no_object = num_objects, 0, no_object
            self.gt = gt_thw if num_objects is not None else (gt_thw > 0.5).to(torch.uint8)
            if num_objects is None:
                self.empty_host = (self.gt.flatten(1).sum(1) == 0).numpy()
            else:
                self.present_host = np.stack([(self.gt == o).flatten(1).any(1).numpy() for o in range(1, num_objects + 1)])
                self.empty_host = ~self.present_host.any(0)

        def score(self, processor, annotated_frames, keep_gen=True, incremental=True):
            log.append(("score", [int(f) for f in annotated_frames], keep_gen, incremental))
            self.rounds += 1
            return worsts[self.rounds - 1], _Gen(f"gen{self.rounds}")

        def qualities(self):
            q = np.array([[(8 * (i + 1) + t) / 64 for t in range(T)] for i in range(self.rounds)], np.float64).reshape(self.rounds, T)
            q[:, self.empty_host] = self.no_object
            return q

        def object_qualities(self):
            oq = np.array([[[(16 * (i + 1) + 4 * o + t) / 128 for t in range(T)] for o in range(self.k)] for i in range(self.rounds)], np.float64)
            oq = oq.reshape(self.rounds, self.k, T)
            oq[:, ~self.present_host] = self.no_object
            return oq
    return Scorer


def _plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def _session(monkeypatch, which, last_frame_empty, worsts, seed=None):
    """(call log, return value, stats) of one session of ``which`` on the fakes."""
    log = []
    monkeypatch.setattr(metrics, "RoundScorer", _scorer_class(log, worsts))
    lab = _labels(last_frame_empty)
    proc = Proc(log)
    rng = random.Random(seed) if seed is not None else None
    stats = {}
    if which == "fq":
        sample = {"num_frames": T, "gt": (lab == 1).float()[None, :, None]}
        ret = fq_driver.oracle_rounds(proc, sample, ROUNDS, stats)
    elif which.startswith("multi_"):
        sample = {"num_frames": T, "num_objects": K, "gt": lab[None, :, None]}
        ret = eval_driver.run_policy(which[6:], proc, sample, ROUNDS, "j_and_f", rng=rng, multi_object=True)
    else:
        sample = {"num_frames": T, "gt": (lab == 1).float()[None, :, None], "rgb": torch.zeros((1, T, 3, 2, 2))}
        if which == "qnet_mask":
            from eva_vos_amd import qnet as qnet_module

            def select(qnet, images, gen, frames):
                log.append(("qnet", qnet, list(images.shape), gen, list(frames)))
                return max(set(range(T)) - set(frames))
            monkeypatch.setattr(qnet_module, "qnet_frame_selection", select)
        ret = eval_driver.run_policy(which, proc, sample, ROUNDS, "j", qnet="net", rng=rng)
    return _plain(log), _plain(ret), stats


CASES = {}


def _case(name, *args, **kw):
    CASES[name] = (args, kw)


_case("fq_exhausted", "fq", True, [1, 2, 0])
_case("fq_past_T", "fq", False, [2, 1, 3])
_case("oracle_exhausted", "oracle_mask", True, [1, 2, 0])
_case("oracle_past_T", "oracle_mask", False, [3, 1, 2])
_case("rand_seed5", "rand_mask", True, [1, 1, 1], seed=5)          # draws the frame without the object: 3 s
_case("rand_seed11", "rand_mask", False, [1, 1, 1], seed=11)
_case("qnet", "qnet_mask", False, [1, 1, 1])
_case("multi_oracle_exhausted", "multi_oracle_mask", True, [2, 1, 0])
_case("multi_oracle_past_T", "multi_oracle_mask", False, [1, 3, 2])
_case("multi_rand_seed5", "multi_rand_mask", True, [0, 0, 0], seed=5)

# (call log, return value, stats) per case, recorded once from the separate loops
EXPECTED = {'fq_exhausted': ([['scorer', [4, 2, 2], 'j', 6, 20.0, None], ['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]],
                   ['score', [0], True, True], ['interact', 1, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 1], True, True]],
                  [[[1, [0.125, 0.140625, 0.15625, 20.0]], [2, [0.25, 0.265625, 0.28125, 20.0]]], ['gen1', 'gen2']],
                  {'interactions': 2, 'propagated_frames': 32}),
 'fq_past_T': ([['scorer', [4, 2, 2], 'j', 6, 20.0, None], ['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]],
                ['score', [0], True, True], ['interact', 2, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 2], True, True],
                ['interact', 1, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 2, 1], True, True]],
               [[[2, [0.125, 0.140625, 0.15625, 0.171875]], [1, [0.25, 0.265625, 0.28125, 0.296875]], [3, [0.375, 0.390625, 0.40625, 0.421875]]],
                ['gen1', 'gen2', 'gen3']],
               {'interactions': 3, 'propagated_frames': 63}),
 'multi_oracle_exhausted': ([['scorer', [4, 2, 2], 'j_and_f', 6, 20.0, 2],
                             ['interact', 0, [3, 1, 2, 2], [0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0], [['download', False], ['scribble', True]]],
                             ['score', [0], False, True],
                             ['interact', 2, [3, 1, 2, 2], [0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0], [['download', False], ['scribble', True]]],
                             ['score', [0, 2], False, True]],
                            {'annotation_times': [80, 80],
                             'frames': [0, 2, 1],
                             'mu_metrics': [0.140625, 0.265625],
                             'object_metrics': [[[0.125, 0.1328125, 0.140625, 20.0], [0.15625, 0.1640625, 0.171875, 20.0]],
                                                [[0.25, 0.2578125, 0.265625, 20.0], [0.28125, 0.2890625, 0.296875, 20.0]]],
                             'present': [[True, True, True, False], [True, True, True, False]],
                             'propagated_frames': 32,
                             'round_metrics': [[0.125, 0.140625, 0.15625, 20.0], [0.25, 0.265625, 0.28125, 20.0]]},
                            {}),
 'multi_oracle_past_T': ([['scorer', [4, 2, 2], 'j_and_f', 6, 20.0, 2],
                          ['interact', 0, [3, 1, 2, 2], [0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0], [['download', False], ['scribble', True]]],
                          ['score', [0], False, True],
                          ['interact', 1, [3, 1, 2, 2], [0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1], [['download', False], ['scribble', True]]],
                          ['score', [0, 1], False, True],
                          ['interact', 3, [3, 1, 2, 2], [0, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1], [['download', False], ['scribble', True]]],
                          ['score', [0, 1, 3], False, True]],
                         {'annotation_times': [80, 80, 80],
                          'frames': [0, 1, 3, 2],
                          'mu_metrics': [0.1484375, 0.2734375, 0.3984375],
                          'object_metrics': [[[0.125, 0.1328125, 0.140625, 0.1484375], [0.15625, 0.1640625, 0.171875, 0.1796875]],
                                             [[0.25, 0.2578125, 0.265625, 0.2734375], [0.28125, 0.2890625, 0.296875, 0.3046875]],
                                             [[0.375, 0.3828125, 0.390625, 0.3984375], [0.40625, 0.4140625, 0.421875, 0.4296875]]],
                          'present': [[True, True, True, True], [True, True, True, True]],
                          'propagated_frames': 63,
                          'round_metrics': [[0.125, 0.140625, 0.15625, 0.171875], [0.25, 0.265625, 0.28125, 0.296875],
                                            [0.375, 0.390625, 0.40625, 0.421875]]},
                         {}),
 'multi_rand_seed5': ([['scorer', [4, 2, 2], 'j_and_f', 6, 20.0, 2],
                       ['interact', 0, [3, 1, 2, 2], [0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0], [['download', False], ['scribble', True]]],
                       ['score', [0], False, True],
                       ['interact', 3, [3, 1, 2, 2], [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0], [['download', False], ['scribble', True]]],
                       ['score', [0, 3], False, True],
                       ['interact', 2, [3, 1, 2, 2], [0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0], [['download', False], ['scribble', True]]],
                       ['score', [0, 3, 2], False, True]],
                      {'annotation_times': [80, 3, 80],
                       'frames': [0, 3, 2, 1],
                       'mu_metrics': [0.140625, 0.265625, 0.390625],
                       'object_metrics': [[[0.125, 0.1328125, 0.140625, 20.0], [0.15625, 0.1640625, 0.171875, 20.0]],
                                          [[0.25, 0.2578125, 0.265625, 20.0], [0.28125, 0.2890625, 0.296875, 20.0]],
                                          [[0.375, 0.3828125, 0.390625, 20.0], [0.40625, 0.4140625, 0.421875, 20.0]]],
                       'present': [[True, True, True, False], [True, True, True, False]],
                       'propagated_frames': 63,
                       'round_metrics': [[0.125, 0.140625, 0.15625, 20.0], [0.25, 0.265625, 0.28125, 20.0], [0.375, 0.390625, 0.40625, 20.0]]},
                      {}),
 'oracle_exhausted': ([['scorer', [4, 2, 2], 'j', 6, 20.0, None], ['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]],
                       ['score', [0], False, True], ['interact', 1, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]],
                       ['score', [0, 1], False, True]],
                      {'annotation_times': [80, 80],
                       'frames': [0, 1, 2],
                       'mu_metrics': [0.140625, 0.265625],
                       'propagated_frames': 32,
                       'round_metrics': [[0.125, 0.140625, 0.15625, 20.0], [0.25, 0.265625, 0.28125, 20.0]]},
                      {}),
 'oracle_past_T': ([['scorer', [4, 2, 2], 'j', 6, 20.0, None], ['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]],
                    ['score', [0], False, True], ['interact', 3, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 3], False, True],
                    ['interact', 1, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 3, 1], False, True]],
                   {'annotation_times': [80, 80, 80],
                    'frames': [0, 3, 1, 2],
                    'mu_metrics': [0.1484375, 0.2734375, 0.3984375],
                    'propagated_frames': 63,
                    'round_metrics': [[0.125, 0.140625, 0.15625, 0.171875], [0.25, 0.265625, 0.28125, 0.296875],
                                      [0.375, 0.390625, 0.40625, 0.421875]]},
                   {}),
 'qnet': ([['scorer', [4, 2, 2], 'j', 6, 20.0, None], ['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0], True, True],
           ['qnet', 'net', [4, 3, 2, 2], 'gen1.float', [0]], ['interact', 3, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]],
           ['score', [0, 3], True, True], ['qnet', 'net', [4, 3, 2, 2], 'gen2.float', [0, 3]],
           ['interact', 2, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 3, 2], True, True],
           ['qnet', 'net', [4, 3, 2, 2], 'gen3.float', [0, 3, 2]]],
          {'annotation_times': [80, 80, 80],
           'frames': [0, 3, 2, 1],
           'mu_metrics': [0.1484375, 0.2734375, 0.3984375],
           'propagated_frames': 63,
           'round_metrics': [[0.125, 0.140625, 0.15625, 0.171875], [0.25, 0.265625, 0.28125, 0.296875], [0.375, 0.390625, 0.40625, 0.421875]]},
          {}),
 'rand_seed11': ([['scorer', [4, 2, 2], 'j', 6, 20.0, None], ['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]],
                  ['score', [0], False, True], ['interact', 2, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 2], False, True],
                  ['interact', 3, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 2, 3], False, True]],
                 {'annotation_times': [80, 80, 80],
                  'frames': [0, 2, 3, 1],
                  'mu_metrics': [0.1484375, 0.2734375, 0.3984375],
                  'propagated_frames': 63,
                  'round_metrics': [[0.125, 0.140625, 0.15625, 0.171875], [0.25, 0.265625, 0.28125, 0.296875], [0.375, 0.390625, 0.40625, 0.421875]]},
                 {}),
 'rand_seed5': ([['scorer', [4, 2, 2], 'j', 6, 20.0, None], ['interact', 0, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]],
                 ['score', [0], False, True], ['interact', 3, [1, 1, 2, 2], [0, 0, 0, 0], [['download', False]]], ['score', [0, 3], False, True],
                 ['interact', 2, [1, 1, 2, 2], [1, 0, 0, 0], [['download', False]]], ['score', [0, 3, 2], False, True]],
                {'annotation_times': [80, 3, 80],
                 'frames': [0, 3, 2, 1],
                 'mu_metrics': [0.140625, 0.265625, 0.390625],
                 'propagated_frames': 63,
                 'round_metrics': [[0.125, 0.140625, 0.15625, 20.0], [0.25, 0.265625, 0.28125, 20.0], [0.375, 0.390625, 0.40625, 20.0]]},
                {})}


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_session_loop_reproduces_the_recorded_calls_and_results(monkeypatch, name):
    args, kw = CASES[name]
    got = _session(monkeypatch, *args, **kw)
    assert got == EXPECTED[name]


def test_the_random_policy_draws_what_the_generator_gives_in_the_recorded_order(monkeypatch):
    """rand_mask consumes exactly one ``choice`` over the sorted frames not yet annotated per scored round, and nothing else."""
    for name, seed in (("rand_seed5", 5), ("rand_seed11", 11), ("multi_rand_seed5", 5)):
        args, kw = CASES[name]
        _, ret, _ = _session(monkeypatch, *args, **kw)
        rng, frames = random.Random(seed), [0]
        while len(frames) < len(ret["frames"]):
            frames.append(rng.choice(sorted(set(range(T)) - set(frames))))
        assert ret["frames"] == frames == EXPECTED[name][1]["frames"], name
