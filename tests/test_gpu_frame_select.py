"""GPU: squared L2 distances between cached frame features (csrc/frame_select.hip: an fp64 Gram matrix on v_mfma_f64_16x16x4_f64) against
fp64 on the host, the engine accessors built on them, and the l2_mask policy of eva_vos_amd.eval_driver.

The bound of every comparison: |D - D_ref| <= 1e-9 * (G_ii + G_jj), G_ii = |x_i|^2.  The products of fp32 values are exact in fp64, so the
kernel's only error is fp64 summation of K <= 1.7 M terms, worst case K * 2^-53 = 1.8e-10 of G_ii + G_jj - the bound is that with a factor
of five, not a figure taken from the kernel."""
import copy
import functools

import numpy as np
import pytest
import torch

from eva_vos_amd import _lib, eval_driver, fq_driver, synth
from eva_vos_amd.frame_select import farthest_frame, pairwise_sq_distances

pytestmark = pytest.mark.gpu
REL = 1e-9


def _yardstick(xd: torch.Tensor):
    """((xd[:, None] - xd[None]) ** 2).sum(-1) in float64 on the host, a few rows at a time, and the squared norms."""
    T, K = xd.shape
    rows = max(1, (1 << 25) // (T * K))
    ref = torch.cat([((xd[i:i + rows, None] - xd[None]) ** 2).sum(-1) for i in range(0, T, rows)])
    return ref.numpy(), (xd * xd).sum(-1).numpy()


def _assert_within_bound(D, xd, what):
    ref, g = _yardstick(xd)
    lim = REL * (g[:, None] + g[None])
    err = np.abs(D - ref)
    print(what, "worst |D - ref| / bound", float((err / np.maximum(lim, 1e-300)).max()), "max D", float(ref.max()))
    assert D.shape == ref.shape and D.dtype == np.float64
    assert (err <= lim).all(), (what, float((err / np.maximum(lim, 1e-300)).max()))
    assert np.array_equal(D, D.T) and not D.diagonal().any()
    return ref, lim


def test_lane_map_is_exact_on_an_asymmetric_integer_fixture():
    """x[t][k] = t + 1 at k = 4 t + (t % 4), else 0: every frame owns one k, in a k-group that changes with the frame, so the Gram matrix is
    diag((t + 1)^2) and D[i][j] = (i + 1)^2 + (j + 1)^2 off the diagonal - exact integers.  The f32 C/D row formula on the f64 MFMA, a
    row / column swap of the diagonal tiles' store, or A and B disagreeing about the k of a lane group put a square in the wrong place."""
    T, K = 33, 132
    x = torch.zeros((T, K))
    for t in range(T):
        x[t, 4 * t + t % 4] = t + 1
    sq = torch.arange(1, T + 1, dtype=torch.float64) ** 2
    want = sq[:, None] + sq[None]
    want.fill_diagonal_(0)
    got = pairwise_sq_distances(x.cuda()).cpu()
    assert torch.equal(got, want), (got - want).abs().max()


@functools.lru_cache(maxsize=None)
def _normal(T, K):
    g = torch.Generator().manual_seed(1000 * T + K)
    return torch.randn((T, K), generator=g)


@pytest.mark.parametrize("K", [4, 252, 4100, 81920])
@pytest.mark.parametrize("T", [1, 2, 16, 17, 33, 106])
def test_generic_entry_against_fp64(T, K):
    x = _normal(T, K)
    dense = x.cuda()
    gapped = torch.full((T, K + 12), float("nan"), device="cuda")      # rows K + 12 apart, NaN in between: a read past K poisons a distance
    gapped[:, :K] = dense
    view = gapped[:, :K]
    assert T == 1 or not view.is_contiguous()
    d1 = pairwise_sq_distances(dense)
    d2 = pairwise_sq_distances(dense)
    d3 = pairwise_sq_distances(view)
    assert d1.dtype == torch.float64 and d1.is_cuda and tuple(d1.shape) == (T, T)
    assert torch.equal(d1, d2), "two runs differ"
    assert torch.equal(d1, d3), "the row stride changed the result (NaN: a read past K)"      # so one comparison serves both strides
    _assert_within_bound(d1.cpu().numpy(), x.double(), f"T={T} K={K}")


def test_near_duplicate_frames_do_not_cancel():
    """40 frames that differ from one base vector of magnitude ~10 by 1e-3: the distances are ~1e-8 of the squared norms they are the
    difference of.  On the host, torch's fp32 `x @ x.T` misses the bound on this fixture 311-fold, its fp64 one sits at 1.2e-6 of it."""
    T, K = 40, 4100
    g = torch.Generator().manual_seed(7)
    x = 10 * torch.randn((1, K), generator=g) + 1e-3 * torch.randn((T, K), generator=g)
    ref, lim = _assert_within_bound(pairwise_sq_distances(x.cuda()).cpu().numpy(), x.double(), "near-duplicates")
    off = ~np.eye(T, dtype=bool)
    assert ref[off].max() < 20 * lim[off].min(), "the fixture no longer cancels"


# ------------------------------------------------------------------------------------------------ engine
def _labels(T, H, W, k):
    m = synth.synthetic_mask(T, H, W, k)[:, :, 0]
    lab = torch.zeros((T, H, W), dtype=torch.uint8)
    for o in range(k):
        lab[m[o] > 0.5] = o + 1
    return lab


def _annotate_frame0(core, T, H, W, k):
    if k == 1:
        core.interact(synth.synthetic_mask(T, H, W, 1)[:, 0], 0, download=False)
    else:
        lab = _labels(T, H, W, k)
        core.interact(torch.stack([lab[0] == c for c in range(k + 1)]).float()[:, None], 0, scribble=True, download=False)


def _features(core):
    return torch.stack([core.frame_features(t) for t in range(core.t)])


@pytest.mark.parametrize("H,W,k", [(128, 160, 1), (100, 150, 3)])
def test_engine_distances_against_fp64_of_the_downloaded_features(nets, nets_multi, H, W, k):
    from mivos.inference_core import InferenceCore
    T = 9
    net = nets if k == 1 else nets_multi
    img = synth.synthetic_clip(T, H, W).cuda()
    core = InferenceCore(net[0], net[1], img, k)
    with pytest.raises(RuntimeError, match="holds no cached features"):
        core.frame_distances()
    with pytest.raises(RuntimeError, match="holds no cached features"):
        core.frame_features(0)
    _annotate_frame0(core, T, H, W, k)
    clone = copy.deepcopy(core)                                    # no matrix yet: the clone computes its own from the copied slots
    fd = core.frame_distances()
    feats = _features(core)
    assert tuple(feats.shape) == (T, core.kh, core.kw, 1024) and core.frame_features(T - 1).shape == (core.kh, core.kw, 1024)
    assert fd.shape == (T, T) and core.frame_distance_passes == 1
    ref, _ = _assert_within_bound(fd, feats.reshape(T, -1).cpu().double(), f"engine {H}x{W} k={k}")
    assert ref[~np.eye(T, dtype=bool)].min() > 0
    assert core.frame_distances() is fd and core.frame_distance_passes == 1
    assert np.array_equal(clone.frame_distances(), fd) and clone.frame_distances() is not fd
    both = copy.deepcopy(core).frame_distances()                   # a matrix that exists is copied
    assert np.array_equal(both, fd) and both is not fd
    with pytest.raises(RuntimeError, match=r"frame 9 outside \[0,9\)"):
        core.frame_features(T)
    # the next object's session keeps the features and the matrix; a plain reset drops both
    assert core.reset(keep_frame_features=True) == T and core.frame_distances() is fd
    assert torch.equal(_features(core), feats)
    assert core.reset() == 0
    with pytest.raises(RuntimeError, match="holds no cached features"):
        core.frame_distances()
    _annotate_frame0(core, T, H, W, k)
    again = core.frame_distances()
    assert again is not fd and core.frame_distance_passes == 2
    _assert_within_bound(again, _features(core).reshape(T, -1).cpu().double(), "after a plain reset")


def test_engine_refuses_a_long_clip_and_a_failed_state(nets):
    from mivos.inference_core import InferenceCore
    long_clip = InferenceCore(nets[0], nets[1], torch.zeros((1, 110, 3, 112, 128)).cuda(), 1)       # 7 x 8 positions: the smallest frame the top-50 read takes
    with pytest.raises(RuntimeError, match="110 frames, the key cache holds 106"):
        long_clip.frame_distances()
    with pytest.raises(RuntimeError, match="110 frames, the key cache holds 106"):
        long_clip.frame_features(0)
    del long_clip
    T, H, W = 9, 128, 160
    core = InferenceCore(nets[0], nets[1], synth.synthetic_clip(T, H, W).cuda(), 1)
    _lib.check(_lib.lib().stcn_test_fail_at(25))
    try:
        with pytest.raises(RuntimeError, match="injected fault"):
            _annotate_frame0(core, T, H, W, 1)
    finally:
        _lib.check(_lib.lib().stcn_test_fail_at(0))
    with pytest.raises(RuntimeError, match="failed state"):
        core.frame_distances()
    with pytest.raises(RuntimeError, match="failed state"):
        core.frame_features(0)
    assert core.reset(keep_frame_features=True) == 0               # a failed engine keeps no features
    with pytest.raises(RuntimeError, match="holds no cached features"):
        core.frame_distances()


# ------------------------------------------------------------------------------------------------ policy
def _expected_frames(core, rounds):
    """farthest_frame round by round on the fp64 yardstick of the features the engine holds; every round's choice must stand clear of the
    runner-up by more than twice the bound, or the comparison would be decided by rounding."""
    x = _features(core).reshape(core.t, -1).cpu().double()
    ref, g = _yardstick(x)
    lim = float(REL * 2 * g.max())
    frames = [0]
    for r in range(rounds):
        lo = np.sort(ref[:, sorted(set(frames))].min(axis=1))
        print("round", r, "largest / second minimum distance", lo[-1], lo[-2], "bound", lim)
        assert lo[-1] - lo[-2] > 2 * lim, (r, lo[-1], lo[-2], lim)
        frames.append(farthest_frame(ref, frames))
    return frames


def test_l2_mask_sessions_choose_what_the_yardstick_chooses(nets, nets_multi):
    from mivos.inference_core import InferenceCore
    T, H, W, rounds = 10, 128, 160, 4
    img = synth.synthetic_clip(T, H, W, seed=5)
    gt = synth.synthetic_mask(T, H, W, 1)
    sample = {"rgb": img, "gt": gt, "num_frames": T, "name": "syn__1", "video": "syn"}
    core = InferenceCore(nets[0], nets[1], img.cuda(), 1)
    stats = {}
    got = eval_driver.run_policy("l2_mask", core, sample, rounds, stats=stats)
    want = _expected_frames(core, rounds)
    assert got["frames"] == want and len(set(want)) == rounds + 1 and len(got["mu_metrics"]) == rounds
    assert stats["frame_distance_passes"] == 1 and stats["interactions"] == rounds
    # the next object's session on the same core: the matrix is there already
    core.reset(keep_frame_features=True)
    assert eval_driver.run_policy("l2_mask", core, sample, rounds, stats=stats)["frames"] == want and stats["frame_distance_passes"] == 1
    # all objects in one engine
    k = 2
    lab = _labels(T, H, W, k)
    multi = {"rgb": img, "gt": lab[None, :, None], "num_frames": T, "num_objects": k, "name": "syn", "video": "syn", "object_ids": [0, 1]}
    core = InferenceCore(nets_multi[0], nets_multi[1], img.cuda(), k)
    got = eval_driver.run_policy("l2_mask", core, multi, rounds, multi_object=True)
    assert got["frames"] == _expected_frames(core, rounds) and len(got["object_metrics"]) == rounds


def test_driver_runs_l2_mask_with_one_distance_pass_per_video(nets_multi, tmp_path):
    root = str(tmp_path / "db")
    imset = fq_driver.make_synthetic_tree(root, {"v3": (6, 112, 128, 3), "v1": (5, 112, 128, 1)})

    def run(**kw):
        stats = {}
        rows = eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], "l2_mask", rounds=3, seed=4, stats=stats, **kw)
        return np.nan_to_num(rows[np.lexsort((rows[:, 1], rows[:, 0]))]), stats

    shared, st = run()
    assert shared.shape == (4 * 3, 6 + 6) and st["frame_distance_passes"] == 2 and st["engines_created"] == 2
    for a in (1, 2):                                               # the objects of v3 see the same features: the same frames
        assert np.array_equal(shared[shared[:, 0] == 0][:, 4], shared[shared[:, 0] == a][:, 4])
    fresh, st = run(share_frames=False)
    assert st["frame_distance_passes"] == 4 and st["engines_created"] == 4 and np.array_equal(fresh, shared)
    again, _ = run()
    assert np.array_equal(again, shared)
    multi, st = run(multi_object=True)
    assert multi.shape == shared.shape and st["frame_distance_passes"] == 2 and np.array_equal(multi[:, 4], shared[:, 4])
