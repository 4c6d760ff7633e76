"""GPU: the per-object sessions of a video share its frame features.  ``InferenceCore.reset(keep_frame_features=True)`` re-targets a
core to another object of the same clip without dropping what the key encoder left in the cache; the drivers use it for the consecutive
objects of a video.  Stated here: bit-identity with a fresh core where the sessions start with the same frame (the drivers' case), the
plain reset for clips longer than the cache, closeness up to the rounding of differently shaped launches where the next session starts
with another frame, and byte-identical driver outputs with and without the sharing.  CPU twin: tests/test_shared_frames.py."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import iou
from eva_vos_amd import eval_driver, fq_driver, synth

pytestmark = pytest.mark.gpu


def _core(nets, img, k, mem_freq, engine_options=None):
    from mivos.inference_core import InferenceCore
    return InferenceCore(nets[0], nets[1], img, k, mem_freq=mem_freq, engine_options=engine_options)


def _session(core, script):
    """Run [(mask, frame, scribble), ...]; returns the masks handed back and the engine's counters per interaction."""
    outs, stats = [], []
    for mask, idx, scribble in script:
        outs.append(core.interact(mask, idx, scribble=scribble).copy())
        stats.append(core.stats())
    return outs, stats


def _assert_same_state(a, b, outs_a, outs_b):
    assert torch.equal(a.prob, b.prob) and torch.equal(a.masks, b.masks)
    assert len(outs_a) == len(outs_b) and all(np.array_equal(x, y) for x, y in zip(outs_a, outs_b))


@pytest.mark.parametrize("engine_options", [None, {"lookahead": 0}], ids=["default", "lookahead0"])
def test_a_re_targeted_core_equals_a_fresh_one_bit_for_bit(nets, engine_options):
    """The drivers' case: every session starts at frame 0, so the kept slots are in the order, and were encoded in the batches, of a
    fresh engine's - object 2 on the core that served object 1 gives the fresh core's bits, and encodes no key."""
    T, H, W = 12, 128, 160
    img, msk = synth.synthetic_clip(T, H, W).cuda(), synth.synthetic_mask(T, H, W, 2).cuda()
    first = [(msk[0:1, 0], 0, False), (msk[0:1, 5], 5, False)]
    second = [(msk[1:2, 0], 0, False), (msk[1:2, 7], 7, False)]
    core = _core(nets, img, 1, 5, engine_options)
    _, st1 = _session(core, first)
    assert sum(s["key_miss"] for s in st1) == T == core.key_frames_encoded
    assert core.reset(keep_frame_features=True) == T
    assert core.interacted == set() and core.key_frames_encoded == 0
    assert float(core.prob[1:].abs().max()) == 0.0 and int(core.masks.max()) == 0, "prob / masks are re-initialised"
    early = copy.deepcopy(core)                                  # a clone of the re-targeted core before it has interacted
    outs, st = _session(core, second)
    fresh = _core(nets, img, 1, 5, engine_options)
    outs_f, st_f = _session(fresh, second)
    _assert_same_state(core, fresh, outs, outs_f)
    assert [s["key_miss"] for s in st] == [0, 0] and core.key_frames_encoded == 0
    assert sum(s["key_miss"] for s in st_f) == T, "the fresh core pays for the clip again"
    assert [s["value_enc"] for s in st] == [s["value_enc"] for s in st_f]
    assert [s["frames"] for s in st] == [s["frames"] for s in st_f]
    outs_e, st_e = _session(early, second)
    _assert_same_state(early, fresh, outs_e, outs_f)
    assert [s["key_miss"] for s in st_e] == [0, 0]
    third = [(msk[1:2, 3], 3, False)]                            # ... and clones taken after the session go on alike
    c1, c2 = copy.deepcopy(core), copy.deepcopy(fresh)
    o1, s1 = _session(c1, third)
    o2, s2 = _session(c2, third)
    _assert_same_state(c1, c2, o1, o2)
    assert s1 == s2
    # the plain form still forgets the features
    assert core.reset() == 0
    again = _core(nets, img, 1, 5, engine_options)
    o1, s1 = _session(core, second[:1])
    o2, s2 = _session(again, second[:1])
    _assert_same_state(core, again, o1, o2)
    assert s1 == s2 and s1[0]["key_miss"] > 0


def test_a_clip_longer_than_the_cache_keeps_nothing(nets):
    """T = 110 > 106 slots: the recycling cache has no stable content, reset(keep_frame_features=True) is the plain reset."""
    T, H, W = 110, 128, 160
    img, msk = synth.synthetic_clip(T, H, W).cuda(), synth.synthetic_mask(T, H, W, 2).cuda()
    core = _core(nets, img, 1, 5)
    _session(core, [(msk[0:1, 0], 0, False), (msk[0:1, 60], 60, False)])
    assert core.reset(keep_frame_features=True) == 0
    second = [(msk[1:2, 0], 0, False), (msk[1:2, 50], 50, False)]
    outs, st = _session(core, second)
    fresh = _core(nets, img, 1, 5)
    outs_f, st_f = _session(fresh, second)
    _assert_same_state(core, fresh, outs, outs_f)
    assert st == st_f and st[0]["key_miss"] >= T


def test_another_first_frame_after_the_re_target_differs_by_rounding_only(nets_multi):
    """The next session starts at frame 7, not 0: a fresh engine would fill its slots from frame 7 on and encode in other batches, so
    decode groups that run batched there run frame by frame here and the reverse.  Only the rounding of differently shaped launches
    may differ - the mechanism, the configuration and the bounds of
    test_gpu_sequence.py::test_multi_object_decode_groups_equal_the_frame_by_frame_path."""
    T, H, W, k = 12, 240, 432, 3
    img, msk = synth.synthetic_clip(T, H, W, seed=3).cuda(), synth.synthetic_mask(T, H, W, k, seed=4)

    def onehot(f):
        return torch.cat([1 - msk[:, f].sum(0, keepdim=True).clamp(0, 1), msk[:, f]], 0).cuda()

    core = _core(nets_multi, img, k, 5)
    _session(core, [(onehot(0), 0, True), (onehot(7), 7, True)])
    assert core.reset(keep_frame_features=True) == T
    second = [(onehot(7), 7, True), (onehot(2), 2, True)]
    outs, st = _session(core, second)
    fresh = _core(nets_multi, img, k, 5)
    outs_f, st_f = _session(fresh, second)
    assert [s["key_miss"] for s in st] == [0, 0] and sum(s["key_miss"] for s in st_f) == T
    worst = min(iou(a == o, b == o) for a, b in zip(outs, outs_f) for o in range(1, k + 1))
    d = (core.prob - fresh.prob).abs()
    q = float(torch.quantile(d.flatten()[::3].float(), 0.999))
    print(f"re-target to another first frame: worst per-object mask IoU {worst:.6f}, p99.9 |dprob| {q:.2e}, max {float(d.max()):.2e}")
    assert worst >= 1 - 1e-3
    assert q < 1e-3, float(d.max())


# ------------------------------------------------------------------------------------------------ drivers
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("shared_frames_db"))
    return root, fq_driver.make_synthetic_tree(root, {"va": (8, 128, 160, 3), "vb": (10, 128, 160, 2)})


def _files(top):
    out = {}
    for d, _, names in os.walk(top):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, top)] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("policy", ["oracle_mask", "rand_mask"])
def test_eval_driver_output_is_byte_identical_with_and_without_sharing(nets, tree, tmp_path, policy, lanes):
    root, imset = tree
    res = {}
    for share in (True, False):
        stats, out = {}, str(tmp_path / f"share{int(share)}" / f"{policy}.csv")
        rows = eval_driver.run(root, imset, out, nets[0], nets[1], policy, rounds=3, seed=4, lanes=lanes, stats=stats, share_frames=share)
        res[share] = (rows, open(out, "rb").read(), stats)
    assert np.array_equal(res[True][0], res[False][0], equal_nan=True) and len(res[True][0]) == 5 * 3
    assert res[True][1] == res[False][1]
    assert res[True][2]["key_frames_encoded"] == 8 + 10 and res[False][2]["key_frames_encoded"] == 3 * 8 + 2 * 10
    assert res[True][2]["engines_created"] == 2 and res[False][2]["engines_created"] == 5
    assert res[True][2]["interactions"] == res[False][2]["interactions"] == 15


@pytest.mark.parametrize("lanes", [1, 2])
def test_fq_driver_output_is_byte_identical_with_and_without_sharing(nets, tree, tmp_path, lanes):
    root, imset = tree
    res = {}
    for share in (True, False):
        stats, out = {}, str(tmp_path / f"fq{int(share)}")
        rows = fq_driver.run(root, imset, out, nets[0], nets[1], rounds=3, save_masks=True, lanes=lanes, stats=stats, share_frames=share)
        res[share] = (rows, _files(out), stats)
    assert np.array_equal(res[True][0], res[False][0], equal_nan=True) and len(res[True][0]) > 0
    a, b = res[True][1], res[False][1]
    assert sorted(a) == sorted(b) and "res_synthetic.csv" in a and sum(n.endswith(".png") for n in a) >= 18 + len(res[True][0]) * 8
    assert all(a[n] == b[n] for n in a), [n for n in a if a[n] != b[n]][:5]
    assert res[True][2]["key_frames_encoded"] == 8 + 10 and res[False][2]["key_frames_encoded"] == 3 * 8 + 2 * 10
    assert res[True][2]["engines_created"] == 2 and res[False][2]["engines_created"] == 5


def test_the_next_object_of_a_video_gets_the_same_device_clip(tree):
    """No second upload: prefetched() hands the consecutive objects of a video ONE device tensor; share_frames=False uploads per sample."""
    root, imset = tree
    ds = fq_driver.ClipDataset(root, imset)
    got = [(s["video"], s["rgb"].data_ptr(), s["rgb"]) for _, s in fq_driver.prefetched(ds, range(len(ds)), "cuda")]
    assert [v for v, _, _ in got] == ["va"] * 3 + ["vb"] * 2
    assert len({p for _, p, _ in got[:3]}) == 1 and len({p for _, p, _ in got[3:]}) == 1 and got[0][1] != got[3][1]
    for i, (_, _, rgb) in enumerate(got):
        assert torch.equal(rgb[0].cpu(), ds[i]["rgb"][0])
    alone = [s["rgb"] for _, s in fq_driver.prefetched(ds, range(3), "cuda", share_frames=False)]
    assert len({t.data_ptr() for t in alone}) == 3 and all(torch.equal(t, got[0][2]) for t in alone)
