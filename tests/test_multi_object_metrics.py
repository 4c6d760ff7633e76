"""CPU: the k-object (label map) metric entry points - ABI table, argument checks before any device call -, the host restatement of a
k-object round (eva_vos_amd.metrics.label_round_quality) against the per-object binary measures, the per-video view of ClipDataset and
the policies the multi-object driver mode refuses."""
import ctypes as C

import numpy as np
import pytest

from eva_vos_amd import _lib, eval_driver, fq_driver, metrics

NEW = ("stcn_metrics_objects_scratch", "stcn_metrics_objects_jf_counts", "stcn_metrics_objects_j_counts", "stcn_metrics_objects_round")
P = C.c_void_p(64)                    # a non-null pointer that is never dereferenced: every case below must fail before a device call


def test_new_symbols_are_declared_and_exported():
    lib = _lib.lib()
    for n in NEW:
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n


def _refused(rc, *words):
    msg = _lib.lib().stcn_last_error().decode()
    assert rc == -1 and all(w in msg for w in words), (rc, msg)


def _round(lib, k=3, t0=0, t1=4, j_only=0, **null):
    a = dict(masks=P, gt=P, annotated=P, present=P, gen=P, scratch=P, counts=P, oq=P, q=P, select=P)
    a.update({n: None for n in null})
    return lib.stcn_metrics_objects_round(None, a["masks"], 48, 64, 4, 2, a["gt"], a["annotated"], a["present"], k, 4, 40, 60, t0, t1, j_only, 20.0,
                                          a["gen"], a["scratch"], a["counts"], a["oq"], a["q"], a["select"])


def test_bad_arguments_are_refused_with_a_message_before_any_device_call():
    lib = _lib.lib()
    n = C.c_int64(-7)
    for k in (0, 33, -1):
        _refused(lib.stcn_metrics_objects_scratch(k, 4, 40, 60, C.byref(n)), "stcn_metrics_objects_scratch", "1..32")
        _refused(lib.stcn_metrics_objects_jf_counts(None, P, P, k, 4, 40, 60, P, P), "stcn_metrics_objects_jf_counts", "1..32")
        _refused(lib.stcn_metrics_objects_j_counts(None, P, P, k, 4, 40, 60, P), "stcn_metrics_objects_j_counts", "1..32")
        _refused(_round(lib, k=k), "stcn_metrics_objects_round", "1..32")
    assert n.value == -7
    _refused(lib.stcn_metrics_objects_scratch(3, 4, 40, 60, None), "null")
    for hole in range(4):
        a = [P] * 4
        a[hole] = None
        _refused(lib.stcn_metrics_objects_jf_counts(None, a[0], a[1], 3, 4, 40, 60, a[2], a[3]), "stcn_metrics_objects_jf_counts", "null")
    for hole in range(3):
        a = [P] * 3
        a[hole] = None
        _refused(lib.stcn_metrics_objects_j_counts(None, a[0], a[1], 3, 4, 40, 60, a[2]), "stcn_metrics_objects_j_counts", "null")
    for name in ("masks", "gt", "annotated", "present", "gen", "scratch", "counts", "oq", "q", "select"):
        _refused(_round(lib, **{name: True}), "stcn_metrics_objects_round", "null")
    for t0, t1 in ((3, 2), (2, 2), (-1, 2), (0, 5)):
        _refused(_round(lib, t0=t0, t1=t1), "stcn_metrics_objects_round", f"[{t0}, {t1})")
    _refused(lib.stcn_metrics_objects_jf_counts(None, P, P, 3, 0, 40, 60, P, P), "bad shape")
    _refused(lib.stcn_metrics_objects_round(None, P, 40, 64, 4, 2, P, P, P, 3, 4, 40, 60, 0, 4, 0, 20.0, P, P, P, P, P, P), "crop")


def test_the_binary_entry_points_say_what_is_wrong_too():
    lib = _lib.lib()

    def rnd(t0=0, t1=4, nh=48, H=40, **null):
        a = dict(masks=P, gt=P, annotated=P, noobj=P, gen=P, scratch=P, counts=P, q=P, select=P)
        a.update({n: None for n in null})
        return lib.stcn_metrics_round(None, a["masks"], nh, 64, 4, 2, a["gt"], a["annotated"], a["noobj"], 4, H, 60, t0, t1, 0, 20.0, a["gen"],
                                      a["scratch"], a["counts"], a["q"], a["select"])
    _refused(lib.stcn_metrics_jf_counts(None, P, P, 4, 1, 60, P, P), "stcn_metrics_jf_counts", "bad shape", "H, W >= 2", "H=1")
    _refused(lib.stcn_metrics_j_counts(None, P, P, 4, 40, 0, P), "stcn_metrics_j_counts", "bad shape", "H, W >= 1", "W=0")
    _refused(lib.stcn_metrics_jf_counts(None, P, P, 0, 40, 60, P, P), "stcn_metrics_jf_counts", "bad shape", "T=0")
    for hole in range(4):
        a = [P] * 4
        a[hole] = None
        _refused(lib.stcn_metrics_jf_counts(None, a[0], a[1], 4, 40, 60, a[2], a[3]), "stcn_metrics_jf_counts", "null")
        if hole < 3:
            _refused(lib.stcn_metrics_j_counts(None, a[0], a[1], 4, 40, 60, a[2]), "stcn_metrics_j_counts", "null")
    for name in ("masks", "gt", "annotated", "noobj", "gen", "scratch", "counts", "q", "select"):
        _refused(rnd(**{name: True}), "stcn_metrics_round", "null")
    _refused(rnd(H=1), "stcn_metrics_round", "bad shape")
    _refused(rnd(nh=40), "stcn_metrics_round", "crop")
    for t0, t1 in ((3, 2), (2, 2), (-1, 2), (0, 5)):
        _refused(rnd(t0=t0, t1=t1), "stcn_metrics_round", f"[{t0}, {t1})")


def test_scratch_size_is_stated_by_the_library():
    lib = _lib.lib()
    n = C.c_int64()
    for k, per_pixel in ((1, 2), (8, 2), (9, 8), (32, 8)):            # a pair of object sets per pixel: bytes up to 8 objects, words above
        assert lib.stcn_metrics_objects_scratch(k, 3, 37, 53, C.byref(n)) == 0 and n.value == 3 * 37 * 53 * per_pixel


def _maps():
    """Three 24 x 30 frames, k = 3.  Frame 0: all three objects in both maps, 1 and 2 share a border, all three meet at a point.  Frame 1:
    object 2 absent from the ground truth (but predicted), object 3 absent from the prediction only.  Frame 2: no object at all in the
    ground truth (a stray prediction), plus a label above k that counts as background."""
    gt, gen = np.zeros((3, 24, 30), np.uint8), np.zeros((3, 24, 30), np.uint8)
    gt[0, 4:12, 3:12], gt[0, 4:12, 12:22], gt[0, 12:20, 6:18] = 1, 2, 3
    gen[0, 5:12, 3:13], gen[0, 4:13, 13:22], gen[0, 13:20, 6:17] = 1, 2, 3
    gt[1, 2:10, 2:10], gt[1, 14:24, 20:30] = 1, 3
    gen[1, 2:10, 3:10], gen[1, 12:16, 4:9] = 1, 2
    gt[2, 3:6, 3:6] = 4
    gen[2, 10:13, 10:14] = 2
    return gt, gen


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
def test_host_restatement_equals_the_per_object_measures_mean_and_argmin(metric):
    gt, gen = _maps()
    k, NO = 3, 20.0
    q, Q, sel = metrics.label_round_quality(gt, gen, k, metric, NO)
    assert q.shape == (3, 3) and q.dtype == Q.dtype == np.float64
    present = np.array([[(gt[t] == o).any() for t in range(3)] for o in (1, 2, 3)])
    assert present.tolist() == [[True, True, False], [True, False, False], [True, True, False]]
    for o in range(k):
        for t in range(3):
            g, p = gt[t] == o + 1, gen[t] == o + 1
            j, f = metrics.jaccard(g, p), metrics.f_measure(g, p)
            want = NO if not present[o, t] else j if metric == "j" else 0.5 * (j + f)
            assert q[o, t] == want, (o, t, q[o, t], want)
    assert q[2, 1] == 0.0                                               # object 3 is there but nothing of it was predicted
    assert Q[0] == (q[0, 0] + q[1, 0] + q[2, 0]) / 3 and Q[1] == (q[0, 1] + q[2, 1]) / 2 and Q[2] == NO
    assert sel == int(np.argmin(Q)) == 1
    # the counts are those of the binary measures, and given counts are used as they are
    c = metrics.label_counts(gt, gen, k)
    assert c.shape == (3, 3, 6) and c[0, 0, 0] == ((gt[0] == 1) & (gen[0] == 1)).sum() and c[1, 1, 1] == (gen[1] == 2).sum()
    assert c[:, 2].sum() == (gen[2] == 2).sum() + metrics.boundary_map(gen[2] == 2).sum()      # frame 2: only the stray prediction counts
    q2, Q2, sel2 = metrics.label_round_quality(gt, gen, k, metric, NO, counts=c)
    assert np.array_equal(q, q2) and np.array_equal(Q, Q2) and sel == sel2


def test_first_minimum_wins_a_tie():
    gt = np.zeros((3, 8, 8), np.uint8)
    gt[:, 2:5, 2:5] = 1
    q, Q, sel = metrics.label_round_quality(gt, gt, 1, "j_and_f")
    assert Q.tolist() == [1.0, 1.0, 1.0] and sel == 0


def test_per_video_view_of_the_clip_dataset(tmp_path):
    imset = fq_driver.make_synthetic_tree(str(tmp_path / "db"), {"a": (3, 48, 64, 1), "b": (4, 48, 64, 2), "c": (3, 48, 64, 3)})
    per_object = fq_driver.ClipDataset(str(tmp_path / "db"), imset)
    assert per_object.samples == [("a", 1, 3), ("b", 1, 4), ("b", 2, 4), ("c", 1, 3), ("c", 2, 3), ("c", 3, 3)]
    assert [per_object.name(i) for i in range(6)] == ["a__1", "b__1", "b__2", "c__1", "c__2", "c__3"] == per_object.object_names
    s = per_object[2]
    assert tuple(s["gt"].shape) == (1, 4, 1, 48, 64) and s["gt"].dtype.is_floating_point and "num_objects" not in s and s["name"] == "b__2"
    per_video = fq_driver.ClipDataset(str(tmp_path / "db"), imset, per_video=True)
    assert per_video.samples == [("a", 1, 3), ("b", 2, 4), ("c", 3, 3)] and len(per_video) == 3
    assert per_video.object_names == per_object.object_names
    for i, (k, ids) in enumerate(((1, [0]), (2, [1, 2]), (3, [3, 4, 5]))):
        v = per_video[i]
        assert v["num_objects"] == k and v["object_ids"] == ids and v["name"] == v["video"] == per_video.name(i) == "abc"[i]
        lab = v["gt"]
        assert lab.dtype.is_floating_point is False and tuple(lab.shape) == (1, v["num_frames"], 1, 48, 64) and int(lab.max()) == k
        for o, sid in enumerate(ids):                                   # the label map holds what the per-object samples hold
            assert np.array_equal((lab == o + 1).numpy(), per_object[sid]["gt"].numpy() > 0.5)
        assert v["rgb"].shape == per_object[ids[0]]["rgb"].shape


@pytest.mark.parametrize("policy", ["qnet_mask", "upper_bound_mask"])
def test_multi_object_mode_refuses_the_one_mask_policies(policy):
    with pytest.raises(ValueError, match="oracle_mask and rand_mask"):
        eval_driver.run_policy(policy, None, {"num_frames": 4, "num_objects": 2}, 3, multi_object=True)


def test_a_video_with_more_than_32_objects_is_refused_by_the_multi_object_mode(tmp_path):
    imset = fq_driver.make_synthetic_tree(str(tmp_path / "db"), {"crowd": (2, 96, 64, 33)})
    assert fq_driver.ClipDataset(str(tmp_path / "db"), imset, per_video=True).samples == [("crowd", 33, 2)]
    with pytest.raises(ValueError, match="crowd has 33 objects.*at most 32"):
        eval_driver.run(str(tmp_path / "db"), imset, "", None, None, "oracle_mask", rounds=2, multi_object=True)
