"""CPU: the per-object sessions of a video share its frame features - what of that can be checked without a GPU.  The ABI of
``stcn_engine_reset_ex`` (argument validation runs before any device call), the grouped shard assignment and the lane chunking that keep
the objects of a video together, and the drivers' engine reuse on a fake ``InferenceCore`` that logs every call."""
import ctypes as C
import random

import numpy as np
import pytest

from eva_vos_amd import _lib, eval_driver, fq_driver, metrics, shard
from session_fakes import DriverScorer as _FakeScorer, fake_core_class as _fake_core_class


# ------------------------------------------------------------------------------------------------ ABI
def test_reset_ex_is_declared_exported_and_validates_before_any_device_call():
    assert _lib.PROTOTYPES["stcn_engine_reset_ex"] == (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)])
    lib = _lib.lib()
    assert hasattr(lib, "stcn_engine_reset_ex") and _lib.RESET_KEEP_FRAMES == 1
    assert lib.stcn_engine_reset_ex(None, 1, None) == -1                      # STCN_E_INVALID
    assert b"null engine" in lib.stcn_last_error()
    kept = C.c_int32(77)
    assert lib.stcn_engine_reset_ex(None, 0x12, C.byref(kept)) == -1          # an unknown flag bit on a null engine
    assert lib.stcn_last_error() and kept.value == 77                           # refused with a message, nothing written
    assert lib.stcn_engine_reset(None) == -1                                   # the plain form is unchanged
    n = C.c_int64(5)
    assert lib.stcn_get_key_frames(None, C.byref(n)) == -1 and n.value == 5    # the session's key-encoder frames: no engine, nothing written


# ------------------------------------------------------------------------------------------------ sharding
def _random_groups(rng, n_groups):
    """(costs, group keys): videos of 2..60 frames with 1..5 objects each, the objects of a video adjacent and of equal cost."""
    costs, groups = [], []
    for g in range(n_groups):
        t = rng.randint(2, 60)
        for _ in range(rng.randint(1, 5)):
            costs.append(t)
            groups.append(f"v{g}")
    return costs, groups


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_grouped_assignment_never_splits_a_group_and_places_every_sample_once(seed, world):
    costs, groups = _random_groups(random.Random(seed), 3 + 4 * seed)
    parts = shard.lpt_assign_grouped(costs, groups, world)
    assert len(parts) == world and sorted(i for p in parts for i in p) == list(range(len(costs)))
    owner = {}
    for r, p in enumerate(parts):
        for i in p:
            assert owner.setdefault(groups[i], r) == r, f"group {groups[i]} is on ranks {owner[groups[i]]} and {r}"
    assert parts == shard.lpt_assign_grouped(costs, groups, world), "deterministic"
    # the cost of a group is frames x objects: the loads are those of lpt_assign over the groups' sums
    sums = {}
    for c, g in zip(costs, groups):
        sums[g] = sums.get(g, 0) + c
    want = sorted(sum(list(sums.values())[j] for j in p) for p in shard.lpt_assign(list(sums.values()), world))
    assert sorted(sum(costs[i] for i in p) for p in parts) == want


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_grouped_assignment_of_singleton_groups_is_lpt_assign(world):
    rng = random.Random(world)
    costs = [rng.randint(1, 90) for _ in range(37)]
    assert shard.lpt_assign_grouped(costs, list(range(len(costs))), world) == shard.lpt_assign(costs, world)
    assert shard.lpt_assign_grouped(costs, [f"video{i}" for i in range(len(costs))], world) == shard.lpt_assign(costs, world)
    with pytest.raises(ValueError):
        shard.lpt_assign_grouped(costs, [0], world)


@pytest.mark.parametrize("seed", range(8))
def test_lane_chunks_keep_videos_whole_when_there_are_enough_videos(seed):
    rng = random.Random(100 + seed)
    n_groups = rng.randint(1, 9)
    costs, groups = _random_groups(rng, n_groups)
    n = len(groups)
    for lanes in range(1, 7):
        for cost_arg in (None, costs):
            b = shard.chunk_bounds(groups, lanes, cost_arg)
            assert len(b) == lanes + 1 and b[0] == 0 and b[-1] == n and b == sorted(b)
            if n_groups >= lanes:
                for cut in b[1:-1]:
                    assert groups[cut] != groups[cut - 1], (lanes, b, groups)      # every cut falls between two videos
                assert all(b[l + 1] > b[l] for l in range(lanes)), "no lane without a video"
            else:
                assert b == [n * l // lanes for l in range(lanes + 1)]             # too few videos: equal sample counts, as before
    # balance: four equal videos over two lanes are cut in the middle, whatever their object counts
    assert shard.chunk_bounds(list("aaabccccdd"), 2, [5] * 10) == [0, 4, 10]
    assert shard.chunk_bounds(list("aabbccdd"), 4) == [0, 2, 4, 6, 8]


def test_run_lanes_hands_a_video_to_one_lane(tmp_path):
    imset = fq_driver.make_synthetic_tree(str(tmp_path / "db"), {"a": (3, 48, 64, 3), "b": (4, 48, 64, 1), "c": (2, 48, 64, 2)})
    import threading
    for lanes in (1, 2, 3):
        lane_of = {}

        def work(i, sample):
            lane_of.setdefault(sample["video"], set()).add(threading.get_ident())
            return [np.array([i], np.float32)]

        rows = fq_driver.run_lanes(str(tmp_path / "db"), imset, range(6), lanes, work, device="cpu")
        assert sorted(int(r[0]) for r in rows) == list(range(6))
        assert all(len(v) == 1 for v in lane_of.values()), lane_of


# ------------------------------------------------------------------------------------------------ drivers on fakes
@pytest.fixture
def fake_tree(tmp_path, monkeypatch):
    import mivos.inference_core
    log = []
    monkeypatch.setattr(mivos.inference_core, "InferenceCore", _fake_core_class(log))
    monkeypatch.setattr(metrics, "RoundScorer", _FakeScorer)
    root = str(tmp_path / "db")
    imset = fq_driver.make_synthetic_tree(root, {"a": (3, 48, 64, 3), "b": (4, 48, 64, 2)})
    return root, imset, log


def _drive(which, root, imset, out, **kw):
    if which == "eval":
        return eval_driver.run(root, imset, "", None, None, "oracle_mask", rounds=2, device="cpu", **kw)
    return fq_driver.run(root, imset, out, None, None, rounds=2, save_masks=False, device="cpu", **kw)


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("which", ["eval", "fq"])
def test_a_lane_keeps_its_core_for_the_objects_of_a_video(fake_tree, tmp_path, which, lanes):
    root, imset, log = fake_tree
    stats = {}
    rows = _drive(which, root, imset, str(tmp_path / "out"), lanes=lanes, stats=stats)
    news, resets = [e for e in log if e[0] == "new"], [e for e in log if e[0] == "reset"]
    assert sorted(news) == [("new", 3, 1, fq_driver.lane_engine_options(lanes)), ("new", 4, 1, fq_driver.lane_engine_options(lanes))]
    assert sorted(resets) == [("reset", 3, True)] * 2 + [("reset", 4, True)], log
    assert stats["engines_created"] == 2 and stats["key_frames_encoded"] == 3 + 4
    assert stats["interactions"] == 5 * 2 and len([e for e in log if e[0] == "interact"]) == 10
    # every session of a video follows the previous one on the same core: new or reset, then its interactions from frame 0
    for t in (3, 4):
        mine = [e for e in log if e[1] == t]
        assert [e[0] for e in mine] == (["new", "interact", "interact"] + ["reset", "interact", "interact"] * (5 - t))
        assert [e[2] for e in mine if e[0] == "interact"][::2] == [0] * (6 - t)
    log_shared, rows_shared = list(log), np.array(rows)

    log.clear()
    stats = {}
    rows = _drive(which, root, imset, str(tmp_path / "out2"), lanes=lanes, stats=stats, share_frames=False)
    assert len([e for e in log if e[0] == "new"]) == 5 and not [e for e in log if e[0] == "reset"]
    assert stats["engines_created"] == 5 and stats["key_frames_encoded"] == 3 * 3 + 2 * 4
    assert np.array_equal(np.array(rows), rows_shared, equal_nan=True)
    assert sorted(e for e in log if e[0] == "interact") == sorted(e for e in log_shared if e[0] == "interact")


def test_the_multi_object_mode_builds_one_core_per_video_and_never_re_targets(fake_tree, monkeypatch):
    """--multi-object is untouched: its samples are videos, each on a fresh core with all its objects."""
    root, imset, log = fake_tree

    class Scorer(_FakeScorer):
        def __init__(self, gt_thw, metric="j", max_rounds=64, no_object=20.0, num_objects=None):
            super().__init__(gt_thw)
            self.k, self.gt = num_objects, gt_thw
            self.present_host = np.ones((num_objects, self.T), bool)

        def object_qualities(self):
            return np.full((self.rounds, self.k, self.T), 0.5)

    monkeypatch.setattr(metrics, "RoundScorer", Scorer)
    stats = {}
    eval_driver.run(root, imset, "", None, None, "oracle_mask", rounds=2, device="cpu", lanes=1, stats=stats, multi_object=True)
    assert [e[:3] for e in log if e[0] == "new"] == [("new", 3, 3), ("new", 4, 2)] and not [e for e in log if e[0] == "reset"]
    assert stats["engines_created"] == 2
