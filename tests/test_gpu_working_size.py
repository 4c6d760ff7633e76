"""GPU: the working-resolution switch - the two kernels of csrc/rescale.hip through the C ABI against the float64 restatements of
working_size_cases.py (pinned to torch's float64 operators by test_working_size_api.py), ``ScaledInferenceCore`` against its own
definition (pass-through, composition, incremental re-derivation, undo, reset, deepcopy, scoring) and the two drivers with
``working_size=`` against plain loops over the wrapper scored on the host."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import working_size_cases as WC
from eva_vos_amd import _lib, eval_driver, fq_driver, metrics, synth, working_size
from eva_vos_amd.working_size import ScaledInferenceCore
from gpu_util import ptr, stream

pytestmark = pytest.mark.gpu
SENTINEL = 0xCC


def _up(prob, hw, HW, t0, t1, out, pad=None):
    """The ABI call on a device tensor [k1,T,1,nh,nw]; ``out``: a device uint8 tensor or a raw address."""
    k1, T, _, nh, nw = prob.shape
    lw, uw, lh, uh = pad or WC.pad_of(hw)
    where = out if isinstance(out, int) else out.data_ptr()
    _lib.check(_lib.lib().stcn_prob_upsample_argmax(stream(), ptr(prob), k1, T, nh, nw, lh, lw, hw[0], hw[1], HW[0], HW[1], t0, t1, where),
               "stcn_prob_upsample_argmax")
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the up kernel
@pytest.mark.parametrize("case", range(len(WC.UP_CASES)))
def test_up_kernel_equals_the_restatement_outside_near_ties(case):
    """Two frames of different probabilities in a NaN-padded plane: a read outside the window would show as a wrong label, a wrong frame
    or plane offset as the other frame's mask."""
    k, hw, HW = WC.UP_CASES[case]
    wins = [WC.probs(case, k, *hw), WC.probs(case + 100, k, *hw)]
    prob = WC.padded(wins, hw).cuda()
    out = torch.full((2, 1) + HW, SENTINEL, dtype=torch.uint8, device="cuda")
    _up(prob, hw, HW, 0, 2, out)
    got = out.cpu().numpy()
    for t, win in enumerate(wins):
        differ, excluded = WC.check_masks(got[t, 0], win.numpy(), HW, what=f"case {case} frame {t}")
        print(f"up case {case} (k={k}, {hw} -> {HW}) frame {t}: {differ} pixels differ, {excluded} excluded as near-ties")


def test_up_kernel_takes_the_lowest_index_at_an_exact_tie():
    hw, HW = (48, 57), (101, 120)
    win = torch.empty(3, *hw)
    win[0] = win[1] = WC.probs(7, 1, *hw)[0] * 0.5 + 0.3           # two identical channels ...
    win[2] = 0.1                                                     # ... above a third
    out = torch.full((1, 1) + HW, SENTINEL, dtype=torch.uint8, device="cuda")
    _up(WC.padded([win], hw).cuda(), hw, HW, 0, 1, out)
    assert int(out.max()) == 0
    win2 = torch.stack([win[2], win[0], win[1]])                     # the tie between channels 1 and 2 above channel 0
    _up(WC.padded([win2], hw).cuda(), hw, HW, 0, 1, out)
    assert int(out.min()) == 1 and int(out.max()) == 1


def test_up_kernel_leaves_the_frames_outside_its_range_alone():
    k, hw, HW = WC.UP_CASES[0]
    T = 5
    wins = [WC.probs(20 + t, k, *hw) for t in range(T)]
    prob = WC.padded(wins, hw).cuda()
    full = torch.full((T, 1) + HW, SENTINEL, dtype=torch.uint8, device="cuda")
    _up(prob, hw, HW, 0, T, full)
    assert int((full == SENTINEL).sum()) == 0
    for t0, t1 in ((0, 1), (1, 4), (4, 5), (2, 2), (0, 0), (5, 5)):
        out = torch.full((T + 1, 1) + HW, SENTINEL, dtype=torch.uint8, device="cuda")     # one frame more: nothing is written behind T either
        _up(prob, hw, HW, t0, t1, out)
        assert torch.equal(out[t0:t1], full[t0:t1]), (t0, t1)
        assert bool((out[:t0] == SENTINEL).all()) and bool((out[t1:] == SENTINEL).all()), (t0, t1)


def test_up_kernel_writes_the_same_masks_to_an_unaligned_output():
    k, hw, HW = WC.UP_CASES[1]                                       # W = 231: rows start at every byte offset
    T = 3
    prob = WC.padded([WC.probs(30 + t, k, *hw) for t in range(T)], hw).cuda()
    n = T * HW[0] * HW[1]
    aligned = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    shifted = torch.full((n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    _up(prob, hw, HW, 0, T, aligned)
    _up(prob, hw, HW, 0, T, shifted.data_ptr() + 1)
    assert aligned.data_ptr() % 4 == 0
    assert torch.equal(shifted[1:n + 1], aligned[:n])
    assert int(shifted[0]) == SENTINEL and bool((shifted[n + 1:] == SENTINEL).all()) and bool((aligned[n:] == SENTINEL).all())


def test_up_kernel_at_an_output_above_4_gib():
    """T = 257 frames of 4096 x 4096 from 48 x 48 windows: frame 255 ends at byte 2^32 of the output, frame 256 starts there.  Every frame
    has one of seven windows (frames 0, 255, 256: three different ones); sampled rows of those frames against the restatement."""
    free = torch.cuda.mem_get_info()[0]
    if free < 6 * 2 ** 30:
        pytest.skip(f"the extent case needs 6 GB of free device memory, {free / 2 ** 30:.1f} GB are free")
    T, hw, HW = 257, (48, 48), (4096, 4096)
    wins = [WC.probs(40 + s, 1, *hw) for s in range(7)]
    prob = WC.padded([wins[t % 7] for t in range(T)], hw).cuda()
    out = torch.full((T, 1) + HW, SENTINEL, dtype=torch.uint8, device="cuda")
    assert out.numel() > 2 ** 32
    _up(prob, hw, HW, 0, T, out)
    rows = np.array([0, 1, 2, 3, 1023, 2047, 2048, 3000, 4093, 4094, 4095])
    for t in (0, 255, 256):
        win = wins[t % 7].numpy()
        got = out[t, 0][torch.from_numpy(rows).cuda()].cpu().numpy()
        differ, excluded = WC.check_masks(got, win, HW, rows=rows, what=f"frame {t}")
        print(f"up extent frame {t}: {differ} pixels differ, {excluded} excluded on {len(rows)} rows")
    assert int((out[1:255:37] == SENTINEL).sum()) == 0              # labels are 0 or 1: a frame left out would still hold the sentinel
    assert torch.equal(out[7], out[0]) and torch.equal(out[255 - 7], out[255]) and not torch.equal(out[255], out[256])


# ------------------------------------------------------------------------------------------------ the down kernel
def _down(x, hw):
    planes, H, W = x.shape
    out = torch.full((planes,) + tuple(hw), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().stcn_frames_downsample_aa(stream(), ptr(x), planes, H, W, hw[0], hw[1], ptr(out)), "stcn_frames_downsample_aa")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("HW,hw,planes", WC.DOWN_CASES)
def test_down_kernel_is_within_4x_torchs_own_fp32_distance_from_float64(HW, hw, planes):
    """The bound is 4 x what torch's CPU fp32 operator differs from float64 on this very input (1.4e-5 at the first size, 1.0e-4 at 1080p,
    measured on the CPU): room for another summation order of the same products; a wrong tap or weight misses by about 1e-2."""
    x = torch.randn(planes, *HW, generator=torch.Generator().manual_seed(HW[0] + hw[1] + planes))
    ref = WC.downsample_aa_ref(x.numpy(), hw)
    t32 = F.interpolate(x[None], size=hw, mode="bicubic", antialias=True, align_corners=False)[0].numpy()
    yard = float(np.abs(t32.astype(np.float64) - ref).max())
    got = _down(x.cuda(), hw).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"down {HW} -> {hw}, {planes} planes: kernel {err:.3e}, torch fp32 {yard:.3e}, ratio {err / yard:.3f}")
    assert np.isfinite(got).all() and err <= 4 * yard, (err, yard)


@pytest.mark.parametrize("HW,hw", [((203, 231), (96, 109)), ((100, 131), (96, 125)), ((800, 1000), (96, 120))])
def test_down_kernel_keeps_a_constant_image_constant(HW, hw):
    """Where the support is clipped at a border the weights are renormalised: a constant stays the constant to 1 ulp, borders included."""
    for c in (1.0, -2.1179039478302, 0.3):
        c32 = np.float32(c)
        got = _down(torch.full((2,) + HW, float(c32), device="cuda"), hw).cpu().numpy()
        ulp = np.spacing(np.abs(c32))
        assert np.abs(got - c32).max() <= ulp, (c, float(np.abs(got - c32).max()), float(ulp))


def test_downsample_frames_chunks_and_host_input_change_no_bit():
    x = synth.synthetic_clip(5, 270, 310)                            # [1,5,3,270,310] on the host
    whole = working_size.downsample_frames(x.cuda(), 128, chunk=8)
    assert whole.shape == (1, 5, 3, 128, 146) and whole.dtype == torch.float32 and whole.is_cuda
    for chunk in (1, 2, 5):
        assert torch.equal(working_size.downsample_frames(x, 128, chunk=chunk), whole), chunk
    ref = WC.downsample_aa_ref(x[0].numpy(), (128, 146))
    assert np.abs(whole[0].cpu().numpy() - ref).max() <= 1e-5
    same = working_size.downsample_frames(x, 270)
    assert same.is_cuda and torch.equal(same.cpu(), x)               # min(H, W) <= size: the clip itself


# ------------------------------------------------------------------------------------------------ the wrapper
def _clip(T, H, W, k=1, seed=0):
    return synth.synthetic_clip(T, H, W, seed=seed), synth.synthetic_mask(T, H, W, k, seed=seed)        # [1,T,3,H,W], [k,T,1,H,W]


def _onehot(msk, t):
    """[k,T,1,H,W] object masks -> the (k+1)-channel one-hot annotation of frame t, background first: [k+1,1,H,W]."""
    lab = torch.zeros(msk.shape[-2:], dtype=torch.long)
    for o in range(msk.shape[0]):
        lab[msk[o, t, 0] > 0.5] = o + 1
    return torch.stack([(lab == c).float() for c in range(msk.shape[0] + 1)])[:, None]


def _rederived(core):
    """Every frame's own-size mask from the inner core's probabilities, into a fresh tensor."""
    out = torch.full_like(core.masks, SENTINEL)
    working_size.upsample_argmax(core.inner.prob, core.inner.pad, core.working_hw, (core.h, core.w), 0, core.t, out)
    return out


def test_pass_through_is_the_plain_core(nets):
    from mivos.inference_core import InferenceCore
    img, msk = _clip(6, 128, 160)
    plain = InferenceCore(nets[0], nets[1], img, 1, mem_freq=2)
    core = ScaledInferenceCore(nets[0], nets[1], img, 1, mem_freq=2, working_size=128)
    assert not core.scaled and core.masks is core.inner.masks and (core.h, core.w, core.nh, core.nw, core.pad) == (128, 160, 128, 160, (0, 0, 0, 0))
    for idx in (0, 4):
        a, b = plain.interact(msk[:, idx], idx), core.interact(msk[:, idx], idx)
        assert a.dtype == b.dtype == np.uint8 and np.array_equal(a, b) and np.array_equal(plain.np_masks, core.np_masks)
        assert torch.equal(plain.masks, core.masks) and core.interacted == plain.interacted
    # a clip that needs padding: the own-size view holds the inner core's bytes, unpadded
    img, msk = _clip(5, 120, 150, seed=3)
    plain = InferenceCore(nets[0], nets[1], img, 1)
    core = ScaledInferenceCore(nets[0], nets[1], img, 1, working_size=None)
    a, b = plain.interact(msk[:, 0], 0), core.interact(msk[:, 0], 0)
    assert np.array_equal(a, b) and core.masks.shape == (5, 1, 120, 150) and np.array_equal(core.masks[:, 0].cpu().numpy(), a)


@pytest.mark.parametrize("k,scribble", [(1, False), (3, True)])
def test_scaled_core_is_the_composition_of_its_three_rules(nets_multi, k, scribble):
    """270 x 310 at 128: a 128 x 146 window, padded to 128 x 160 with 7 / 7."""
    T, H, W = 6, 270, 310
    img, msk = _clip(T, H, W, k, seed=11)
    core = ScaledInferenceCore(nets_multi[0], nets_multi[1], img, k, working_size=128)
    assert core.scaled and core.working_hw == (128, 146) and (core.inner.nh, core.inner.nw, core.inner.pad) == (128, 160, (7, 7, 0, 0))
    assert (core.t, core.k, core.h, core.w, core.nh, core.nw, core.pad) == (T, k, H, W, H, W, (0, 0, 0, 0))
    assert core.prob is core.inner.prob and core.masks.shape == (T, 1, H, W) and core.masks.dtype == torch.uint8 and core.masks.is_cuda
    assert core.top_k == core.inner.top_k and core.km == core.inner.km and core.device == core.inner.device
    assert torch.equal(core.inner._images_unpadded, working_size.downsample_frames(img, 128))
    out = None
    for idx in (0, 4):
        out = core.interact(_onehot(msk, idx) if scribble else msk[:, idx], idx, scribble=scribble)
    assert out.shape == (T, H, W) and out.dtype == np.uint8 and np.array_equal(out, core.masks[:, 0].cpu().numpy()) and out is core.np_masks
    assert core.interacted == {0, 4} and out.max() <= k and out.max() >= 1
    prob = core.inner.prob.cpu().numpy()
    if not scribble:
        # a one-object core keeps the annotation of an interacted frame in BOTH channels (the reference's broadcast): exact ties everywhere,
        # the lowest index wins, the frame's mask is empty - as the plain core's is; the drivers score such frames by their ground truth
        assert all(np.array_equal(prob[0, idx], prob[1, idx]) and not out[idx].any() for idx in (0, 4))
    for t in range(T):
        win = prob[:, t, 0, :, 7:7 + 146]
        differ, excluded = WC.check_masks(out[t], win, (H, W), what=f"k={k} frame {t}")
        print(f"composition k={k} frame {t}: {differ} pixels differ, {excluded} excluded as near-ties")
    with pytest.raises(RuntimeError, match=f"1,{H},{W}"):
        core.interact(msk[:, 1, :, :128, :146], 1)                   # an annotation at the working size is refused


def test_own_size_masks_follow_interactions_undo_and_reset_incrementally(nets):
    T, H, W = 8, 270, 310
    img, msk = _clip(T, H, W, seed=12)
    core = ScaledInferenceCore(nets[0], nets[1], img, 1, working_size=128)
    core.set_undo_depth(1)
    assert core.undo_state()["depth"] == 1
    core.masks.fill_(SENTINEL)                                       # whatever a step fails to re-derive keeps the sentinel or a stale mask
    before = None
    for step, idx in (("interact", 0), ("interact", 5), ("interact", 2), ("undo", None), ("interact", 3)):
        if step == "interact":
            before = core.masks.clone()
            assert core.interact(msk[:, idx], idx, download=False) is None
        else:
            got = core.undo()
            assert torch.equal(core.masks, before), "undo: the own-size masks are what they were before the undone call"
            assert np.array_equal(got, before[:, 0].cpu().numpy()) and core.interacted == {0, 5}
        assert torch.equal(core.masks, _rederived(core)), (step, idx)
    with pytest.raises(RuntimeError):
        core.undo()
        core.undo()                                                  # depth 1: at most one step back
    assert torch.equal(core.masks, _rederived(core))
    kept = core.reset(keep_frame_features=True)
    assert kept == T and core.interacted == set() and not core.np_masks.any()
    core.masks.fill_(SENTINEL)
    core.interact(msk[:, 1], 1, download=False)
    assert torch.equal(core.masks, _rederived(core)) and int((core.masks == SENTINEL).sum()) == 0


def test_a_deep_copy_continues_like_its_source(nets):
    T, H, W = 6, 270, 310
    img, msk = _clip(T, H, W, seed=13)
    core = ScaledInferenceCore(nets[0], nets[1], img, 1, working_size=128)
    core.interact(msk[:, 0], 0)
    twin = copy.deepcopy(core)
    assert twin.inner is not core.inner and twin.masks is not core.masks and torch.equal(twin.masks, core.masks)
    assert np.array_equal(twin.np_masks, core.np_masks) and twin.interacted == core.interacted == {0}
    a, b = core.interact(msk[:, 3], 3), twin.interact(msk[:, 3], 3)
    assert np.array_equal(a, b) and torch.equal(twin.masks, core.masks)
    twin.interact(msk[:, 5], 5)
    assert core.interacted == {0, 3} and np.array_equal(core.masks[:, 0].cpu().numpy(), a)      # the source is not touched


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
def test_round_scorer_reads_a_scaled_core_like_any_core(nets, metric):
    T, H, W = 6, 270, 310
    img, msk = _clip(T, H, W, seed=14)
    msk[0, T - 1] = 0                                                # one frame without the object
    gt = msk[0, :, 0].cuda()
    core = ScaledInferenceCore(nets[0], nets[1], img, 1, working_size=128)
    scorer = metrics.RoundScorer(gt, metric, max_rounds=4, no_object=eval_driver.NO_OBJECT)
    frames = []
    for idx in (0, 4, 2):
        frames.append(idx)
        own = core.interact(msk[:, idx], idx)
        sel, gen = scorer.score(core, frames)
        pred = own > 0
        pred[frames] = msk[0, frames, 0].numpy() > 0.5
        want = metrics.sequence_scores(msk[0, :, 0].numpy() > 0.5, pred)[:, 1 if metric == "j" else 3].astype(np.float64)
        want[T - 1] = eval_driver.NO_OBJECT
        q = scorer.qualities()[len(frames) - 1]
        assert np.array_equal(gen.cpu().numpy() > 0, pred)
        assert np.abs(q - want).max() <= 1e-6 and sel == int(np.argmin(want)), (idx, q, want)     # sequence_scores rounds its rows to fp32


# ------------------------------------------------------------------------------------------------ the drivers
TREE = {"v0": (6, 270, 310, 2), "v1": (6, 270, 310, 1)}
ROUNDS, SIZE = 3, 128


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("working_size_db"))
    return root, fq_driver.make_synthetic_tree(root, TREE)


def _sorted(rows):
    return np.nan_to_num(rows[np.lexsort((rows[:, 1], rows[:, 0]))])


def _core(nets, rgb, k):
    return ScaledInferenceCore(nets[0], nets[1], rgb.cuda(), k, working_size=SIZE)


def test_eval_driver_rows_equal_a_plain_loop_over_the_scaled_core(nets_multi, tree):
    root, imset = tree
    got = _sorted(eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], "oracle_mask", rounds=ROUNDS, working_size=SIZE))
    ds = fq_driver.ClipDataset(root, imset)
    want = []
    for i in range(len(ds)):
        s = ds[i]
        gt = s["gt"][0].cuda()
        proc = _core(nets_multi, s["rgb"], 1)
        assert proc.scaled and proc.working_hw == (128, 146)
        frames = [0]
        for r in range(ROUNDS):
            proc.interact(gt[frames[r]][None], frames[r], download=False)
            mu, _, q = eval_driver.frame_quality(proc, gt[:, 0], sorted(set(frames)), "j_and_f")
            row = np.full(12, np.nan, np.float32)
            row[:6] = (i, r, mu, 80, frames[r], len(q))
            row[6:6 + len(q)] = q
            want.append(row)
            frames.append(int(np.argmin(q)))
    assert got.shape == (3 * ROUNDS, 12) and np.array_equal(got, np.nan_to_num(np.stack(want)))
    native = _sorted(eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], "oracle_mask", rounds=ROUNDS))
    assert not np.array_equal(native[:, 6:], got[:, 6:]), "the switch changes what is propagated"
    # without the switch the rows are those of a wrapper that passes everything through: the native path is untouched
    through = _sorted(eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], "oracle_mask", rounds=ROUNDS, working_size=4096))
    assert np.array_equal(native, through)


def test_eval_driver_multi_object_rows_equal_a_plain_loop_over_the_scaled_core(nets_multi, tree):
    root, imset = tree
    got = _sorted(eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], "oracle_mask", rounds=ROUNDS, multi_object=True, working_size=SIZE))
    ds = fq_driver.ClipDataset(root, imset, per_video=True)
    want = []
    for i in range(len(ds)):
        s = ds[i]
        k, T = s["num_objects"], s["num_frames"]
        gt = s["gt"][0, :, 0]                                        # uint8 label map [T,H,W]
        proc = _core(nets_multi, s["rgb"], k)
        channels = torch.arange(k + 1, dtype=torch.uint8)[:, None, None, None]
        frames = [0]
        for r in range(ROUNDS):
            f = frames[r]
            proc.interact((gt[f][None, None] == channels).float(), f, scribble=True)
            gen = proc.np_masks.copy()
            gen[frames] = gt[frames].numpy()
            q, Q, sel = metrics.label_round_quality(gt.numpy(), gen, k, "j_and_f", eval_driver.NO_OBJECT)
            present = np.stack([(gt.numpy() == o).reshape(T, -1).any(1) for o in range(1, k + 1)])
            for o, sid in enumerate(s["object_ids"]):
                row = np.full(12, np.nan, np.float32)
                row[:6] = (sid, r, float(np.mean(q[o][present[o]])), 80 if present[o][f] else 3, f, T)
                row[6:6 + T] = q[o]
                want.append(row)
            frames.append(sel)
    assert got.shape == (3 * ROUNDS, 12) and np.array_equal(got, _sorted(np.stack(want)))


def test_fq_driver_rows_equal_a_plain_loop_over_the_scaled_core(nets_multi, tree, tmp_path):
    root, imset = tree
    got = fq_driver.run(root, imset, str(tmp_path / "fq"), nets_multi[0], nets_multi[1], rounds=ROUNDS, save_masks=False, working_size=SIZE)
    got = _sorted(got)
    ds = fq_driver.ClipDataset(root, imset)
    want = []
    for i in range(len(ds)):
        s = ds[i]
        gt = s["gt"][0].cuda()
        proc = _core(nets_multi, s["rgb"], 1)
        frames, sid = [0], 1
        for r in range(ROUNDS):
            proc.interact(gt[frames[r]][None], frames[r], download=False)
            _, _, q = fq_driver.frame_quality(proc, gt[:, 0], sorted(set(frames)), "j")
            worst = int(np.argmin(q))
            frames.append(worst)
            if float(q[worst]) == fq_driver.NO_OBJECT:
                continue
            row = np.full(10, np.nan, np.float32)
            row[:4] = (i, sid, worst, len(q))
            row[4:4 + len(q)] = q
            want.append(row)
            sid += 1
    assert np.array_equal(got, _sorted(np.stack(want)))


@pytest.fixture(scope="module")
def qnet():
    from eva_vos_amd.qnet import QualityNet
    net = QualityNet()
    net.load_state_dict(synth.recipe_state_dict(net, seed=3))
    return net.cuda().eval()


@pytest.fixture(scope="module")
def first_round(nets, tree):
    """mu_metric of round 0 - frame 0 annotated with its mask - per sample, from the oracle_mask policy at the working size."""
    r = eval_driver.run(tree[0], tree[1], "", nets[0], nets[1], "oracle_mask", rounds=1, working_size=SIZE)
    return _sorted(r)[:, 2]


SWITCHED = ([(p, {}) for p in eval_driver.POLICIES] + [(p, dict(multi_object=True)) for p in eval_driver.MULTI_OBJECT_POLICIES]
            + [("oracle_oracle", dict(annotator="component", annotation_types=["3clicks", "mask"]))])


@pytest.mark.parametrize("policy,kw", SWITCHED, ids=[p + ("-multi" if kw.get("multi_object") else "") for p, kw in SWITCHED])
def test_policies_run_through_the_driver_with_the_switch(nets, tree, qnet, first_round, policy, kw):
    """The session loop, the scorers and the robots read a core by duck typing: every mask policy (per-object), the multi-object ones and a
    mixed-annotation policy over the stand-in annotator give well-formed rows at a working size, and the first round of a one-object
    session - frame 0 with its mask - is the same whatever the policy."""
    root, imset = tree
    r = eval_driver.run(root, imset, "", nets[0], nets[1], policy, rounds=2, qnet=qnet, seed=4, working_size=SIZE, **kw)
    tail = 1 if policy == "oracle_oracle" else 0
    assert r.shape[1] == 12 + tail and set(r[:, 0].astype(int)) == {0, 1, 2} and len(r) >= 3, r.shape
    for row in r:
        q = row[6:6 + int(row[5])]
        assert np.all(((q >= 0) & (q <= 1)) | (q == eval_driver.NO_OBJECT)) and 0 <= row[2] <= 1, row
        if policy in eval_driver.POLICIES and not kw.get("multi_object"):
            assert q[int(row[4])] == 1.0, row                        # a frame annotated with its mask counts with its ground truth
    if not kw.get("multi_object"):
        assert np.array_equal(_sorted(r[r[:, 1] == 0])[:, 2], first_round)


def test_upper_bound_trials_by_undo_equal_deep_copies_on_a_scaled_core(nets):
    T, H, W, rounds = 6, 270, 310, 3
    img, msk = _clip(T, H, W, seed=15)
    s = {"rgb": img, "gt": msk, "num_frames": T, "name": "syn__1", "video": "syn"}
    stats = {}
    proc = ScaledInferenceCore(nets[0], nets[1], img, 1, working_size=SIZE)
    got = eval_driver.run_policy("upper_bound_mask", proc, s, rounds, "j_and_f", stats=stats)
    assert stats["engine_clones"] == 0 and stats["trial_interactions"] == sum(T - 1 - r for r in range(rounds))
    assert proc.undo_state() == dict(depth=0, entries=0, bytes=0)
    # the selection as it was formulated before undo: a deep copy of the processor per candidate, frame_quality on the host
    proc = ScaledInferenceCore(nets[0], nets[1], img, 1, working_size=SIZE)
    gt = msk[0].cuda()
    frames, mus, rows = [0], [], []
    for _ in range(rounds):
        proc.interact(gt[frames[-1]][None], frames[-1], download=False)
        mu, _, q = fq_driver.frame_quality(proc, gt[:, 0], frames, "j_and_f")
        mus.append(mu)
        rows.append(q)
        best, best_f = -np.inf, -1
        for f in (f for f in range(T) if f not in frames):
            p = copy.deepcopy(proc)
            p.interact(gt[f][None], f, download=False)
            m = fq_driver.frame_quality(p, gt[:, 0], frames + [f], "j_and_f")[0]
            if m >= best:
                best, best_f = m, f
        frames.append(best_f)
    assert got["frames"] == frames and got["mu_metrics"] == mus
    assert all(np.array_equal(a, b) for a, b in zip(got["round_metrics"], rows))
