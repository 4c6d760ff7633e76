"""GPU: an interaction taken back in place (``InferenceCore.undo``, stcn_engine_undo), the scorer's trial rounds
(``RoundScorer.score_trial``, stcn_metrics_trial) and the upper-bound round of the eval driver that is built on both.  Stated here: after
``undo()`` the core's ``prob`` and ``masks`` are BYTE-equal to what they were before the undone call, and - where the undone call encoded
no key - so is everything the core computes afterwards, against a twin that never ran it; the journal's rules; a trial row equals
``frame_quality`` of the tried state as float64 bit patterns and leaves the scorer as it was; the driver's selection, means and rows are
those of the deep-copy formulation.  CPU twin: tests/test_undo_api.py."""
import copy

import numpy as np
import pytest
import torch

from conftest import iou
from eva_vos_amd import _lib, eval_driver, fq_driver, metrics, synth

pytestmark = pytest.mark.gpu


def _core(nets, img, k=1, mem_freq=5, depth=0):
    from mivos.inference_core import InferenceCore
    core = InferenceCore(nets[0], nets[1], img, k, mem_freq=mem_freq)
    if depth:
        core.set_undo_depth(depth)
    return core


def _snap(core):
    return core.prob.clone(), core.masks.clone(), set(core.interacted)


def _same(core, snap):
    return torch.equal(core.prob, snap[0]) and torch.equal(core.masks, snap[1]) and core.interacted == snap[2]


def _cropped(core, masks):
    lw, uw, lh, uh = core.pad
    return masks[:, 0, lh:core.nh - uh, lw:core.nw - uw].cpu().numpy()


@pytest.fixture(scope="module")
def clip14():
    T, H, W = 14, 128, 160
    return synth.synthetic_clip(T, H, W, seed=31).cuda(), synth.synthetic_mask(T, H, W, 1, seed=32).cuda()


def test_undo_restores_exactly_and_later_rounds_equal_an_untrialled_twin(nets, clip14):
    """mem_freq = 2: both spans of the trial insert temporary memory.  The twin runs with the journal off."""
    img, msk = clip14
    core, twin = _core(nets, img, 1, 2, depth=1), _core(nets, img, 1, 2)
    for c in (core, twin):
        c.interact(msk[:, 0], 0)
        c.interact(msk[:, 9], 9)
    snap = _snap(core)
    assert _same(twin, snap), "an engine with the journal on computes what one without it computes"
    core.interact(msk[:, 4], 4, download=False)
    st = core.stats()
    assert st["key_miss"] == 0 and st["frames"] == 7 and st["bank_fwd"] > 3 and st["bank_bwd"] > 3, st
    assert not torch.equal(core.prob[:, 1:9], snap[0][:, 1:9]), "the trial must have changed its span"
    assert core.undo_state() == dict(depth=1, entries=1, bytes=core.undo_state()["bytes"]) and core.undo_state()["bytes"] >= 8 * 128 * 160 * 9
    out = core.undo()
    assert _same(core, snap) and np.array_equal(out, _cropped(core, snap[1])) and core.undo_state()["entries"] == 0
    a, b = core.interact(msk[:, 5], 5), twin.interact(msk[:, 5], 5)
    assert np.array_equal(a, b) and torch.equal(core.prob, twin.prob) and torch.equal(core.masks, twin.masks)
    assert core.stats() == twin.stats()


def test_undo_at_the_edges_of_the_span_logic(nets):
    """One-sided sweeps (frame 0, frame T - 1), a trial whose two neighbours are annotated (both sweeps empty) and a re-annotation of an
    annotated frame: the interacted set keeps it and the certain slot is popped - the next round's bank sizes are the twin's."""
    T, H, W = 12, 128, 160
    img, msk = synth.synthetic_clip(T, H, W, seed=33).cuda(), synth.synthetic_mask(T, H, W, 1, seed=34).cuda()
    core, twin = _core(nets, img, 1, 3, depth=1), _core(nets, img, 1, 3)
    for c in (core, twin):
        for f in (3, 5, 8):
            c.interact(msk[:, f], f, download=False)
    snap = _snap(core)
    for f, frames, m in ((0, 2, 0), (T - 1, 2, T - 1), (4, 0, 4), (5, 3, 6)):      # (trial frame, frames its sweeps visit, frame whose mask it draws)
        core.interact(msk[:, m], f, download=False)
        assert core.stats()["frames"] == frames and core.interacted == {3, 5, 8, f}
        assert not torch.equal(core.prob, snap[0]), f
        assert core.undo(download=False) is None
        assert _same(core, snap), f"trial at frame {f}"
    a, b = core.interact(msk[:, 6], 6), twin.interact(msk[:, 6], 6)
    assert np.array_equal(a, b) and torch.equal(core.prob, twin.prob) and core.stats() == twin.stats()


def test_undo_restores_every_row_of_a_padded_multi_object_core(nets_multi):
    """k = 3 through the scribble path at 100 x 150 (padded by 6, 6 and 5, 5): four prob rows, T * npix floats apart."""
    T, H, W, k = 10, 100, 150, 3
    img, msk = synth.synthetic_clip(T, H, W, seed=35).cuda(), synth.synthetic_mask(T, H, W, k, seed=36).cuda()

    def onehot(f):
        return torch.cat([1 - msk[:, f].sum(0, keepdim=True).clamp(0, 1), msk[:, f]], 0)

    core = _core(nets_multi, img, k, 5, depth=1)
    assert core.pad == (5, 5, 6, 6)
    core.interact(onehot(0), 0, scribble=True, download=False)
    core.interact(onehot(7), 7, scribble=True, download=False)
    snap = _snap(core)
    core.interact(onehot(3), 3, scribble=True, download=False)
    for row in range(k + 1):
        assert not torch.equal(core.prob[row, 1:7], snap[0][row, 1:7]), f"row {row}: the trial must have changed its span"
        assert torch.equal(core.prob[row, 7:], snap[0][row, 7:]) and torch.equal(core.prob[row, :1], snap[0][row, :1]), "frames outside the span"
    assert core.undo_state()["bytes"] >= 6 * core.nh * core.nw * (4 * (k + 1) + 1)
    core.undo(download=False)
    for row in range(k + 1):
        assert torch.equal(core.prob[row], snap[0][row]), row
    assert _same(core, snap)


def test_an_undo_issued_at_once_is_ordered_behind_late_side_streams(nets, clip14):
    """Every offloaded FusionNet group, the second sweep's stream and the key-encoder stream start 400 us late (the existing hook); the
    undo is enqueued right behind the trial with no host wait in between.  Still exact."""
    img, msk = clip14
    core = _core(nets, img, 1, 2, depth=1)
    core.interact(msk[:, 0], 0, download=False)
    core.interact(msk[:, 9], 9, download=False)
    snap = _snap(core)
    _lib.check(_lib.lib().stcn_test_side_delay_us(400))
    try:
        core.interact(msk[:, 4], 4, download=False)
        fused = core.stats()["fused"]
        core.undo(download=False)
        torch.cuda.synchronize()
    finally:
        _lib.check(_lib.lib().stcn_test_side_delay_us(0))
    assert fused > 0 and _same(core, snap)


def test_journal_rules(nets, clip14):
    img, msk = clip14
    core = _core(nets, img, 1, 5)
    assert core.undo_state() == dict(depth=0, entries=0, bytes=0)
    core.interact(msk[:, 0], 0, download=False)
    assert core.undo_state() == dict(depth=0, entries=0, bytes=0), "depth 0: nothing is kept"
    with pytest.raises(RuntimeError, match="nothing to undo"):
        core.undo()
    with pytest.raises(RuntimeError, match="negative"):
        core.set_undo_depth(-1)
    # depth 3: three interactions, three undos, the base state; a fourth is refused and changes nothing
    core.set_undo_depth(3)
    snaps = [_snap(core)]
    for f in (5, 9, 2):
        core.interact(msk[:, f], f, download=False)
        snaps.append(_snap(core))
    assert core.undo_state()["entries"] == 3
    for want in (snaps[2], snaps[1], snaps[0]):
        core.undo(download=False)
        assert _same(core, want)
    with pytest.raises(RuntimeError, match="nothing to undo"):
        core.undo()
    assert _same(core, snaps[0]) and core.undo_state()["entries"] == 0
    # the oldest entries go first: at overflow, and when the depth is lowered
    for f in (5, 9, 2, 12):
        core.interact(msk[:, f], f, download=False)
    assert core.undo_state()["entries"] == 3
    core.set_undo_depth(2)
    assert core.undo_state()["depth"] == 2 and core.undo_state()["entries"] == 2
    core.undo(download=False)                                        # takes 12 back
    before_12 = _snap(core)
    assert before_12[2] == {0, 5, 9, 2}
    core.undo(download=False)                                        # takes 2 back
    assert core.interacted == {0, 5, 9} and _same(core, (snaps[2][0], snaps[2][1], {0, 5, 9}))
    with pytest.raises(RuntimeError, match="nothing to undo"):
        core.undo()
    # a deep copy starts with an empty journal and its source's depth; the source's undo still restores exactly
    core.interact(msk[:, 7], 7, download=False)
    clone = copy.deepcopy(core)
    assert clone.undo_state() == dict(depth=2, entries=0, bytes=0) and core.undo_state()["entries"] == 1
    with pytest.raises(RuntimeError, match="nothing to undo"):
        clone.undo()
    core.undo(download=False)
    assert _same(core, (snaps[2][0], snaps[2][1], {0, 5, 9}))
    clone.interact(msk[:, 3], 3, download=False)
    assert clone.undo_state()["entries"] == 1
    # reset() empties the journal and keeps the depth
    core.interact(msk[:, 7], 7, download=False)
    core.reset()
    assert core.undo_state() == dict(depth=2, entries=0, bytes=0)
    with pytest.raises(RuntimeError, match="nothing to undo"):
        core.undo()


def test_failures_and_the_journal(nets):
    """Through the host-side injection hook: a call refused in its up-front reservation adds no entry - the next undo takes the PREVIOUS
    interaction back; a failure inside an interaction leaves the engine failed, its journal empty, and undo refused until reset()."""
    T, H, W = 9, 128, 160
    img, msk = synth.synthetic_clip(T, H, W, seed=13).cuda(), synth.synthetic_mask(T, H, W, 1, seed=14).cuda()
    core = _core(nets, img, 1, 3, depth=2)
    core.interact(msk[:, 2], 2, download=False)
    snap = _snap(core)
    core.interact(msk[:, 6], 6, download=False)
    assert core.undo_state()["entries"] == 2
    _lib.check(_lib.lib().stcn_test_fail_at(-1))
    with pytest.raises(RuntimeError, match="bank_reserve"):
        core.interact(msk[:, 4], 4, download=False)
    assert core.undo_state()["entries"] == 2 and core.interacted == {2, 6}
    core.undo(download=False)
    assert _same(core, snap), "the undo after a refused call takes the previous interaction back"
    _lib.check(_lib.lib().stcn_test_fail_at(25))
    try:
        with pytest.raises(RuntimeError, match="injected fault"):
            core.interact(msk[:, 6], 6, download=False)
    finally:
        _lib.check(_lib.lib().stcn_test_fail_at(0))
    assert core.undo_state()["entries"] == 0 and core.interacted == {2}
    with pytest.raises(RuntimeError, match="failed state"):
        core.undo()
    core.reset()
    fresh = _core(nets, img, 1, 3)
    a, b = core.interact(msk[:, 2], 2), fresh.interact(msk[:, 2], 2)
    assert np.array_equal(a, b) and torch.equal(core.prob, fresh.prob) and core.undo_state()["entries"] == 1


def test_undo_of_the_very_first_interaction(nets, clip14):
    img, msk = clip14
    core, fresh = _core(nets, img, 1, 5, depth=1), _core(nets, img, 1, 5)
    init = _snap(fresh)
    core.interact(msk[:, 0], 0, download=False)
    out = core.undo()
    assert _same(core, init) and not out.any()
    a, b = core.interact(msk[:, 0], 0), fresh.interact(msk[:, 0], 0)
    assert np.array_equal(a, b) and torch.equal(core.prob, fresh.prob) and torch.equal(core.masks, fresh.masks)
    assert core.stats()["key_miss"] == 0 and fresh.stats()["key_miss"] == 14


def test_a_clip_longer_than_the_key_cache(nets):
    """T = 110 > 106 slots.  Restoration is exact whatever the cache does; the trial leaves other frames in the recycling cache than the
    twin holds, so the next interaction encodes and decodes in other batches: it agrees within the bounds of the decode-batch comparison in
    tests/test_gpu_shared_frames.py (masks IoU >= 1 - 1e-3, p99.9 |dprob| <= 1e-3).
    Measured on an MI355X: mask IoU 1.000000, p99.9 |dprob| 0.00e+00, max 0.00e+00 - at this size the differently filled cache happened
    to lead to the same launches; the bound is what the mechanism allows, not what this clip shows."""
    T, H, W = 110, 128, 160
    img, msk = synth.synthetic_clip(T, H, W, seed=37).cuda(), synth.synthetic_mask(T, H, W, 1, seed=38).cuda()
    core, twin = _core(nets, img, 1, 5, depth=1), _core(nets, img, 1, 5)
    for c in (core, twin):
        c.interact(msk[:, 0], 0, download=False)
        c.interact(msk[:, 60], 60, download=False)
    snap = _snap(core)
    core.interact(msk[:, 30], 30, download=False)
    assert core.stats()["key_miss"] > 0, "the trial of a long clip re-encodes keys: the case the bound is for"
    core.undo(download=False)
    assert _same(core, snap)
    a, b = core.interact(msk[:, 90], 90), twin.interact(msk[:, 90], 90)
    worst = iou(a, b)
    d = (core.prob - twin.prob).abs()
    q = float(torch.quantile(d.flatten()[::3].float(), 0.999))
    print(f"T = 110, interaction after an undone trial against the untrialled twin: mask IoU {worst:.6f}, p99.9 |dprob| {q:.2e}, max {float(d.max()):.2e}")
    assert worst >= 1 - 1e-3
    assert q <= 1e-3, float(d.max())


# ------------------------------------------------------------------------------------------------ scorer
@pytest.mark.parametrize("metric,H,W", [("j", 120, 200), ("j_and_f", 120, 200), ("j_and_f", 101, 77)])
def test_trial_rows_equal_frame_quality_and_leave_the_scorer_alone(metric, H, W):
    """A trial = what a tried interaction does to the engine's masks (the frames between the annotated neighbours of the candidate change)
    + score_trial; then the masks are put back, as undo does.  Candidates: in front of the first annotated frame (a span from frame 0),
    behind the last (a span to frame T - 1), between two, next to one (a span of one frame), a frame with empty ground truth.  A twin
    scorer that runs no trial must see the same rounds."""

    class Proc:
        pass
    T = 11
    rng = np.random.RandomState(H + W)
    gt = synth.synthetic_mask(T, H, W, 1, seed=5)[0, :, 0]
    gt[3] = 0
    gt[9] = 0
    p = Proc()
    lh, lw = (-H) % 16 // 2, (-W) % 16 // 2
    p.nh, p.nw = H + (-H) % 16, W + (-W) % 16
    p.pad = (lw, p.nw - W - lw, lh, p.nh - H - lh)
    pred = ((synth.synthetic_mask(T, H, W, 1, seed=6)[0, :, 0] > 0.5) ^ torch.from_numpy(rng.rand(T, H, W) < 0.02)).to(torch.uint8)
    masks = torch.zeros((T, 1, p.nh, p.nw), dtype=torch.uint8)
    masks[:, 0, lh:lh + H, lw:lw + W] = pred
    p.masks = masks.cuda()
    gt_dev = gt.cuda()
    sc, plain = (metrics.RoundScorer(gt_dev, metric, max_rounds=4, no_object=eval_driver.NO_OBJECT) for _ in range(2))
    with pytest.raises(RuntimeError, match="scored last"):
        sc.score_trial(p, [4], 5, 0)                                  # no round scored yet
    for r, annotated in enumerate(([4], [4, 7], [4, 7, 6])):
        if r:
            cur, others = annotated[-1], set(annotated[:-1])
            lo, hi = max([f for f in others if f < cur] + [-1]), min([f for f in others if f > cur] + [T])
            p.masks[lo + 1:hi, 0, lh:lh + H, lw:lw + W] ^= torch.from_numpy(rng.rand(hi - lo - 1, H, W) < 0.01).to(torch.uint8).cuda()
        sel, gen = sc.score(p, annotated)
        sel2, gen2 = plain.score(p, annotated)
        assert sel == sel2 and torch.equal(gen, gen2) and torch.equal(sc.counts, plain.counts)
        state = (sc.counts.clone(), sc.annotated.clone(), gen.clone(), sc.rounds)
        want = {}
        cands = [c for c in (0, 10, 5, 8, 3, 9, 1) if c not in annotated]
        for row, c in enumerate(cands):
            lo, hi = max([f for f in annotated if f < c] + [-1]), min([f for f in annotated if f > c] + [T])
            keep = p.masks[lo + 1:hi].clone()
            p.masks[lo + 1:hi, 0, lh:lh + H, lw:lw + W] ^= torch.from_numpy(rng.rand(hi - lo - 1, H, W) < 0.03).to(torch.uint8).cuda()
            sc.score_trial(p, annotated, c, row)
            want[row] = eval_driver.frame_quality(p, gt_dev, sorted(annotated + [c]), metric)[2]
            p.masks[lo + 1:hi] = keep
        got = sc.trial_rows(len(cands))
        assert got.dtype == np.float64 and got.shape == (len(cands), T)
        for row, c in enumerate(cands):
            assert np.array_equal(got[row], want[row]) and np.array_equal(got[row].view(np.uint64), want[row].view(np.uint64)), (r, c, np.abs(got[row] - want[row]).max())
            assert got[row][c] == (eval_driver.NO_OBJECT if c in (3, 9) else 1.0)
        assert torch.equal(sc.counts, state[0]) and torch.equal(sc.annotated, state[1]) and torch.equal(gen, state[2]) and sc.rounds == state[3]
    assert np.array_equal(sc.qualities().view(np.uint64), plain.qualities().view(np.uint64))
    with pytest.raises(RuntimeError, match="scored last"):
        sc.score_trial(p, [4, 7], 5, 0)                               # not the frames of the last round
    multi = metrics.RoundScorer(gt_dev.to(torch.uint8), metric, max_rounds=1, num_objects=2)
    with pytest.raises(RuntimeError, match="one-object"):
        multi.score_trial(p, [4], 5, 0)


# ------------------------------------------------------------------------------------------------ driver
def _deep_copy_upper_bound(proc, sample, rounds, metric):
    """The upper-bound session as it was formulated before undo: a deep copy of the processor per candidate, frame_quality on the host."""
    gt = sample["gt"][0].cuda()
    gt_thw, T = gt[:, 0], sample["num_frames"]
    frames, mus, rows = [0], [], []
    for _ in range(rounds):
        proc.interact(gt[frames[-1]][None], frames[-1], download=False)
        mu, _, q = fq_driver.frame_quality(proc, gt_thw, frames, metric)
        mus.append(mu)
        rows.append(q)
        best, best_f = -np.inf, -1
        for f in (f for f in range(T) if f not in frames):
            p = copy.deepcopy(proc)
            p.interact(gt[f][None], f, download=False)
            m = fq_driver.frame_quality(p, gt_thw, frames + [f], metric)[0]
            if m >= best:
                best, best_f = m, f
        frames.append(best_f)
    return frames, mus, rows


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
def test_the_upper_bound_in_place_selects_what_the_deep_copies_select(nets, metric):
    T, H, W, rounds = 10, 128, 160, 4
    gt = synth.synthetic_mask(T, H, W, 1, seed=40)
    gt[0, T - 1] = 0                                                 # one frame without the object
    s = {"rgb": synth.synthetic_clip(T, H, W, seed=39), "gt": gt, "num_frames": T, "name": "syn__1", "video": "syn"}
    stats = {}
    proc = _core(nets, s["rgb"].cuda(), 1, 5)
    got = eval_driver.run_policy("upper_bound_mask", proc, s, rounds, metric, stats=stats)
    frames, mus, rows = _deep_copy_upper_bound(_core(nets, s["rgb"].cuda(), 1, 5), s, rounds, metric)
    assert got["frames"] == frames
    assert got["mu_metrics"] == mus
    assert len(got["round_metrics"]) == rounds and all(np.array_equal(a, b) for a, b in zip(got["round_metrics"], rows))
    assert stats["engine_clones"] == 0 and stats["trial_interactions"] == sum(T - 1 - r for r in range(rounds)) and stats["interactions"] == rounds
    assert proc.undo_state() == dict(depth=0, entries=0, bytes=0), "the core leaves the session as it came"
