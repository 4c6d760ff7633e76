"""CPU: undo of an interaction and the trial round of the scorer - what of them can be checked without a GPU.  The four new symbols are
declared and exported, every argument check they make runs before any device call, and the driver's upper-bound round tries its
candidates on the session's own core (interact, score_trial, undo, back to back) - on fakes that log every call.  GPU twin:
tests/test_gpu_undo.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from eva_vos_amd import _lib, eval_driver, metrics

INVALID = -1                     # STCN_E_INVALID
NEW = ("stcn_engine_set_undo", "stcn_engine_undo", "stcn_engine_get_undo", "stcn_metrics_trial")


def _refused(rc, *words):
    assert rc == INVALID, rc
    msg = _lib.lib().stcn_last_error().decode()
    assert msg and all(w in msg for w in words), msg


def test_the_new_symbols_are_declared_and_exported():
    lib = _lib.lib()
    for name in NEW:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert _lib.PROTOTYPES["stcn_engine_set_undo"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib.PROTOTYPES["stcn_engine_undo"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)])
    assert _lib.PROTOTYPES["stcn_engine_get_undo"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)])
    assert len(_lib.PROTOTYPES["stcn_metrics_trial"][1]) == 22


def test_the_engine_calls_refuse_a_null_engine_and_write_nothing():
    lib = _lib.lib()
    _refused(lib.stcn_engine_set_undo(None, 1), "stcn_engine_set_undo", "null engine")
    _refused(lib.stcn_engine_set_undo(None, -3), "stcn_engine_set_undo")
    idx, still = C.c_int32(41), C.c_int32(42)
    _refused(lib.stcn_engine_undo(None, C.byref(idx), C.byref(still)), "stcn_engine_undo", "null engine")
    assert (idx.value, still.value) == (41, 42)
    d, n, b = C.c_int32(5), C.c_int32(6), C.c_int64(7)
    _refused(lib.stcn_engine_get_undo(None, C.byref(d), C.byref(n), C.byref(b)), "stcn_engine_get_undo", "null engine")
    assert (d.value, n.value, b.value) == (5, 6, 7)


def _trial(**kw):
    """stcn_metrics_trial on host buffers that are never dereferenced: every case below is refused before a device call."""
    T, H, W, nh, nw = 4, 50, 60, 64, 64
    bufs = {n: (C.c_uint8 * 16)() for n in ("masks", "gt", "annotated", "noobj", "counts", "span_gen", "scratch", "span_counts", "quality")}
    a = {n: C.cast(b, C.c_void_p) for n, b in bufs.items()}
    a.update(nh=nh, nw=nw, lh=7, lw=2, candidate=1, T=T, H=H, W=W, t0=0, t1=3, j_only=0)
    a.update(kw)
    return _lib.lib().stcn_metrics_trial(None, a["masks"], a["nh"], a["nw"], a["lh"], a["lw"], a["gt"], a["annotated"], a["noobj"], a["candidate"], a["T"],
                                         a["H"], a["W"], a["t0"], a["t1"], a["j_only"], 20.0, a["counts"], a["span_gen"], a["scratch"],
                                         a["span_counts"], a["quality"])


@pytest.mark.parametrize("name", ["masks", "gt", "annotated", "noobj", "counts", "span_gen", "scratch", "span_counts", "quality"])
def test_the_trial_refuses_null_pointers(name):
    _refused(_trial(**{name: None}), "stcn_metrics_trial", "null")


def test_the_trial_reads_no_boundary_scratch_for_j_but_checks_everything_else_first():
    # j_only takes no boundary map: a null scratch is not what gets this call refused - its span is
    _refused(_trial(scratch=None, j_only=1, t0=3, t1=2), "stcn_metrics_trial", "[3, 2)")


@pytest.mark.parametrize("t0,t1", [(3, 2), (-1, 2), (0, 5), (4, 3)])
def test_the_trial_refuses_a_span_that_is_no_range_of_the_clip(t0, t1):
    _refused(_trial(t0=t0, t1=t1), "stcn_metrics_trial", f"[{t0}, {t1})")


@pytest.mark.parametrize("candidate", [-1, 4, 1000])
def test_the_trial_refuses_a_candidate_outside_the_clip(candidate):
    _refused(_trial(candidate=candidate), "stcn_metrics_trial", "candidate", str(candidate))


def test_the_trial_refuses_bad_shapes_and_crops():
    _refused(_trial(H=1), "stcn_metrics_trial", "bad shape")
    _refused(_trial(T=0), "stcn_metrics_trial", "bad shape")
    _refused(_trial(nh=40), "stcn_metrics_trial", "crop")


# ------------------------------------------------------------------------------------------------ the driver's round, on fakes
class _Core:
    """InferenceCore's surface as run_policy uses it for the upper bound; logs every call."""

    def __init__(self, T, log):
        self.t, self.log, self.depth, self.journal = T, log, 0, []
        self.prob = types.SimpleNamespace(device=torch.device("cpu"))

    def interact(self, mask, idx, scribble=False, download=True):
        assert not download
        self.log.append(("interact", int(idx)))
        if self.depth:
            self.journal = (self.journal + [int(idx)])[-self.depth:]

    def undo(self, download=True):
        assert not download and self.journal, "undo without an entry"
        self.log.append(("undo", self.journal.pop()))

    def set_undo_depth(self, n):
        self.log.append(("depth", n))
        self.depth = n

    def undo_state(self):
        return dict(depth=self.depth, entries=len(self.journal), bytes=0)

    def stats(self):
        return {"frames": self.t - 1}

    def __deepcopy__(self, memo):
        raise AssertionError("a clip that fits the key cache is tried in place: no deep copy")


class _Scorer:
    """RoundScorer's surface: frame f's trial row is worth f % 3 everywhere, so the best candidates tie and the LAST of them must win."""

    def __init__(self, gt_thw, metric="j", max_rounds=64, no_object=20.0, num_objects=None):
        self.T, self.rounds, self.trials = int(gt_thw.shape[0]), 0, {}
        self.empty_host = np.zeros(self.T, bool)
        self.empty_host[1] = True

    def score(self, processor, annotated_frames, keep_gen=True, incremental=True):
        processor.log.append(("score", tuple(annotated_frames)))
        self.rounds += 1
        return 0, torch.zeros((self.T, 2, 2), dtype=torch.uint8)

    def score_trial(self, processor, annotated_frames, candidate, row):
        processor.log.append(("trial", tuple(annotated_frames), int(candidate), int(row)))
        self.trials[int(row)] = np.full(self.T, float(candidate % 3))

    def trial_rows(self, n):
        processor_rows = np.stack([self.trials[r] for r in range(n)])
        self.trials = {}
        return processor_rows

    def qualities(self):
        return np.full((self.rounds, self.T), 0.5)


def test_an_upper_bound_round_tries_every_candidate_in_place_and_takes_it_back(monkeypatch):
    monkeypatch.setattr(metrics, "RoundScorer", _Scorer)
    T, log, stats = 7, [], {}
    sample = dict(num_frames=T, gt=torch.zeros((1, T, 1, 4, 4)), rgb=torch.zeros((1, T, 3, 4, 4)))
    core = _Core(T, log)
    res = eval_driver.run_policy("upper_bound_mask", core, sample, rounds=2, metric="j", stats=stats)
    # values f % 3 over frames 1..6 are 1 2 0 1 2 0: the maximum 2 is at 2 and 5, the last one wins (the reference's >=); then among
    # 1 2 3 4 6 -> 1 2 0 1 0: frame 2
    assert res["frames"] == [0, 5, 2]
    assert log[0] == ("depth", 1) and log[-1] == ("depth", 0), "the core returns with the depth it came with"
    body = log[1:-1]
    want = [("interact", 0), ("score", (0,))]
    for row, f in enumerate(range(1, T)):
        want += [("interact", f), ("trial", (0,), f, row), ("undo", f)]
    want += [("interact", 5), ("score", (0, 5))]
    for row, f in enumerate([1, 2, 3, 4, 6]):
        want += [("interact", f), ("trial", (0, 5), f, row), ("undo", f)]
    assert body == want
    assert stats["trial_interactions"] == 6 + 5 and stats["engine_clones"] == 0 and stats["interactions"] == 2
    assert res["propagated_frames"] == 2 * (T - 1), "trials do not count as the session's propagation"


def test_a_clip_longer_than_the_key_cache_keeps_the_deep_copy_path(monkeypatch):
    """The choice is made from the clip length alone: T = 107 never touches the journal and clones per candidate."""
    monkeypatch.setattr(metrics, "RoundScorer", _Scorer)
    monkeypatch.setattr(eval_driver, "frame_quality", lambda p, gt, frames, metric: (float(frames[-1] % 3), None, None))
    T, log, stats = eval_driver.KEY_CACHE_FRAMES + 1, [], {}

    class Cloning(_Core):
        def __deepcopy__(self, memo):
            self.log.append(("clone",))
            return Cloning(self.t, [])

    sample = dict(num_frames=T, gt=torch.zeros((1, T, 1, 4, 4)), rgb=torch.zeros((1, T, 3, 4, 4)))
    res = eval_driver.run_policy("upper_bound_mask", Cloning(T, log), sample, rounds=1, metric="j", stats=stats)
    assert not [e for e in log if e[0] in ("depth", "undo", "trial")]
    assert len([e for e in log if e[0] == "clone"]) == T - 1 == stats["engine_clones"] == stats["trial_interactions"]
    assert res["frames"] == [0, 104]                                # the last frame with f % 3 == 2


def test_the_upper_bound_stays_a_one_object_policy():
    assert "upper_bound_mask" not in eval_driver.MULTI_OBJECT_POLICIES
