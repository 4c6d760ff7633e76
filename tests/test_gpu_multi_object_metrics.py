"""GPU: the k-object (label map) evaluation of an annotation round - counts per object against the binary entry point, the round scorer
against the host restatement (bit for bit), a session and the driver's multi-object mode."""
import numpy as np
import pytest
import torch

import gpu_util as G
from eva_vos_amd import eval_driver, fq_driver, metrics, synth

pytestmark = pytest.mark.gpu
NO = eval_driver.NO_OBJECT


# ------------------------------------------------------------------------------------------------ counts
def _label_maps(T, H, W, k, seed):
    """gt, pred uint8 [T,H,W] with k >= 3 labels.  Objects 1 and 2 are rectangles side by side (a common vertical border), object 3 lies
    under both down to the last row and across to the last column, so the three meet at a point; objects 4..k are small squares in the strip
    above.  pred = gt moved by (1, 2) pixels with 1 % of its pixels relabelled at random (object sets of up to four labels per pixel).  In the
    LAST frame one object is taken out of gt only, one out of pred only and one out of both."""
    rng = np.random.RandomState(seed)
    h0 = H // 4
    h1 = h0 + max(21, H // 3)
    cm = W // 2
    gt = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        s = t % 3                                                    # the layout moves a little from frame to frame
        gt[t, h0:h1, 4 + s:cm + s] = 1
        gt[t, h0:h1, cm + s:W - 6 + s] = 2
        gt[t, h1:, cm + s - W // 4:] = 3
        n = k - 3
        if n:
            pitch = min(12, W // n)
            size = min(pitch - 2, h0 - 2)
            assert size >= 3
            for e in range(n):
                gt[t, 1:1 + size, e * pitch + 1:e * pitch + 1 + size] = 4 + e
    pred = np.roll(gt, (1, 2), (1, 2))
    noise = rng.rand(T, H, W) < 0.01
    pred[noise] = rng.randint(0, k + 1, int(noise.sum()))
    a, b, c = (4, 3, 5) if k >= 5 else (1, 2, 3)                     # out of gt, out of pred, out of both
    assert k >= 5 or T > 1
    gt[-1][(gt[-1] == a) | (gt[-1] == c)] = 0
    pred[-1][(pred[-1] == b) | (pred[-1] == c)] = 0
    return gt, pred, (a, b, c)


def _assert_the_maps_hold_the_hard_cases(gt, pred, k, missing):
    f = gt[0]                                                        # (with one frame the objects taken out below are none of 1, 2, 3 in gt)
    assert int(((f[:, :-1] == 1) & (f[:, 1:] == 2)).sum()) >= 20                                     # two objects share a border
    win = np.stack([f[:-1, :-1], f[:-1, 1:], f[1:, :-1], f[1:, 1:]])                                 # own, east, south, south-east
    distinct = sum(((win == o).any(0)).astype(int) for o in range(1, k + 1))
    assert int(distinct.max()) >= 3                                                                  # three objects meet at a point
    assert f[-1, -1] == 3 and (f[-1] == 3).sum() > 4 and (f[:, -1] == 3).sum() > 4                   # last row and last column
    a, b, c = missing
    g, p = gt[-1], pred[-1]
    assert not (g == a).any() and (p == a).any() and (g == b).any() and not (p == b).any() and not (g == c).any() and not (p == c).any()
    if len(gt) > 1:
        assert (gt == k).any() and (pred == k).any() and int(gt.max()) == k                          # the top label (bit / slot) is in use
    # object sets of three and more labels at one pixel occur in pred
    sets = np.stack([pred[0][:-1, :-1], pred[0][:-1, 1:], pred[0][1:, :-1], pred[0][1:, 1:]])
    assert int(sum(((sets == o).any(0)).astype(int) for o in range(1, k + 1)).max()) >= 3


def _radius(H, W):
    return int(np.ceil(0.008 * np.hypot(H, W)))


def _binary_counts(gt, pred, k, j_only):
    """[k,T,6] from the EXISTING binary entry points on (gt == o, pred == o), one call per object."""
    T, H, W = gt.shape
    out = []
    for o in range(1, k + 1):
        g, p = (gt == o).to(torch.uint8).contiguous(), (pred == o).to(torch.uint8).contiguous()
        c = torch.full((T, 6), -1, dtype=torch.int32, device="cuda")
        if j_only:
            G.call("stcn_metrics_j_counts", G.stream(), g, p, T, H, W, c)
        else:
            G.call("stcn_metrics_jf_counts", G.stream(), g, p, T, H, W, c, torch.empty(T * H * W, dtype=torch.uint8, device="cuda"))
        out.append(c)
    return torch.stack(out)


# 37 x 53: radius 1, frames of 1961 pixels - no multiple of 64, most waves lie across a frame boundary; k = 9 is the first k whose object
# sets are 32-bit words (k <= 8: bytes).  200 x 300: radius 3.  480 x 854: radius 8.
CASES = [(3, 37, 53, 3, 1), (3, 37, 53, 9, 1), (2, 200, 300, 3, 3), (2, 200, 300, 32, 3), (1, 480, 854, 5, 8)]


@pytest.mark.parametrize("j_only", [False, True], ids=["jf", "j"])
@pytest.mark.parametrize("T,H,W,k,radius", CASES)
def test_counts_per_object_equal_the_binary_entry_point(T, H, W, k, radius, j_only):
    assert _radius(H, W) == radius
    gt_h, pred_h, missing = _label_maps(T, H, W, k, seed=T * H + k)
    _assert_the_maps_hold_the_hard_cases(gt_h, pred_h, k, missing)
    gt, pred = torch.from_numpy(gt_h).cuda(), torch.from_numpy(pred_h).cuda()
    nc = k * T * 6 * 4
    cbuf = G.guarded(nc, torch.uint8)
    counts = cbuf[:nc].view(torch.int32).view(k, T, 6)
    if j_only:
        G.call("stcn_metrics_objects_j_counts", G.stream(), gt, pred, k, T, H, W, counts)
    else:
        ns = metrics._objects_scratch(k, T, H, W, "cuda").numel()
        sbuf = G.guarded(ns, torch.uint8)
        G.call("stcn_metrics_objects_jf_counts", G.stream(), gt, pred, k, T, H, W, counts, sbuf)
        assert G.guard_intact(sbuf, ns)
    assert G.guard_intact(cbuf, nc)
    want = _binary_counts(gt, pred, k, j_only)
    assert torch.equal(counts, want), (counts - want).abs().amax((1, 2)).tolist()
    if not j_only:
        assert int(want[..., 4].sum()) > 0 and int((want[..., 2] - want[..., 4]).sum()) > 0      # matched and unmatched boundary pixels
        if H < 100:                                                  # the host restatement counts the same (small case only: SciPy dilations)
            assert np.array_equal(want.cpu().numpy(), metrics.label_counts(gt_h, pred_h, k))


def test_labels_above_k_count_as_background():
    gt_h, pred_h, _ = _label_maps(3, 37, 53, 9, seed=3)
    gt, pred = torch.from_numpy(gt_h).cuda(), torch.from_numpy(pred_h).cuda()
    k = 4                                                            # labels 5..9 are objects that "appear later"
    counts = torch.empty((k, 3, 6), dtype=torch.int32, device="cuda")
    G.call("stcn_metrics_objects_jf_counts", G.stream(), gt, pred, k, 3, 37, 53, counts, metrics._objects_scratch(k, 3, 37, 53, "cuda"))
    assert torch.equal(counts, _binary_counts(gt, pred, k, False))
    rows = metrics.sequence_scores_objects_gpu(gt, pred, k)
    for o in range(k):
        one = metrics.sequence_scores_gpu(gt == o + 1, pred == o + 1)
        assert np.array_equal(rows[o].view(np.uint64), one.view(np.uint64))
    assert np.array_equal(metrics.sequence_scores_objects_gpu(gt, pred, k, j_only=True)[..., 0], rows[..., 0])


# ------------------------------------------------------------------------------------------------ rounds
class _Proc:                                       # the attributes of an InferenceCore the scorer reads
    def __init__(self, labels_thw):
        T, H, W = labels_thw.shape
        lh, lw = (-H) % 16 // 2, (-W) % 16 // 2
        self.nh, self.nw = H + (-H) % 16, W + (-W) % 16
        self.pad = (lw, self.nw - W - lw, lh, self.nh - H - lh)
        masks = torch.full((T, 1, self.nh, self.nw), 1, dtype=torch.uint8)          # garbage in the padding must not matter
        masks[:, 0, lh:lh + H, lw:lw + W] = labels_thw
        self.masks = masks.cuda()
        self.box = (slice(None), 0, slice(lh, lh + H), slice(lw, lw + W))

    def labels(self):
        return self.masks[self.box]


def _session_script(T):
    """Annotated frames per round, the new one last: round 2 annotates frame 5 BETWEEN two annotated ones (t0 = 1, t1 = 9 < T)."""
    return ([0], [0, 9], [0, 9, 5], [0, 9, 5, T - 1])


def test_k1_equals_the_binary_round_entry_point():
    """num_objects = 1 on a 0/1 map: counts, per-frame quality (bits) and selection of stcn_metrics_round."""
    T, H, W = 11, 101, 77
    rng = np.random.RandomState(7)
    gt = synth.synthetic_mask(T, H, W, 1, seed=5)[0, :, 0].to(torch.uint8)
    gt[3] = 0
    pred = synth.synthetic_mask(T, H, W, 1, seed=6)[0, :, 0].to(torch.uint8)
    pred[5] = 0
    pred ^= torch.from_numpy((rng.rand(T, H, W) < 0.02).astype(np.uint8))
    p = _Proc(pred)
    for metric in ("j", "j_and_f"):
        one = metrics.RoundScorer(gt.cuda(), metric, max_rounds=4, no_object=NO)
        lab = metrics.RoundScorer(gt.cuda(), metric, max_rounds=4, no_object=NO, num_objects=1)
        for annotated in _session_script(T):
            s1, g1 = one.score(p, annotated)
            s2, g2 = lab.score(p, annotated)
            assert s1 == s2 and torch.equal(g1, g2) and torch.equal(one.counts, lab.counts[0])
        q1, q2 = one.qualities(), lab.qualities()
        assert np.array_equal(q1.view(np.uint64), q2.view(np.uint64)) and np.array_equal(q2, lab.object_qualities()[:, 0])
        assert (q2[:, 3] == NO).all()


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
def test_round_scorer_of_three_objects_equals_the_host_restatement_bit_for_bit(metric):
    T, H, W, k = 12, 128, 160, 3
    rng = np.random.RandomState(11)

    def label_map(seed):
        m = synth.synthetic_mask(T, H, W, k, seed=seed)[:, :, 0]
        lab = torch.zeros((T, H, W), dtype=torch.uint8)
        for o in range(k):
            lab[m[o] > 0.5] = o + 1
        return lab

    gt = label_map(2)
    gt[4][gt[4] == 2] = 0                                              # object 2 leaves frame 4
    gt[7] = 0                                                          # a frame without any object
    pred = torch.roll(label_map(2), (2, -3), (1, 2))
    pred[6][pred[6] == 3] = 0                                          # object 3 is there but not predicted
    noise = torch.from_numpy(rng.rand(T, H, W) < 0.02)
    pred[noise] = torch.from_numpy(rng.randint(0, k + 1, int(noise.sum())).astype(np.uint8))
    gt_h = gt.numpy()
    scorers = {inc: metrics.RoundScorer(gt.cuda(), metric, max_rounds=4, no_object=NO, num_objects=k) for inc in (True, False)}
    assert scorers[True].present_host.tolist() == [[t != 7 for t in range(T)], [t not in (4, 7) for t in range(T)], [t != 7 for t in range(T)]]
    assert scorers[True].empty_host.tolist() == [t == 7 for t in range(T)]
    p = _Proc(pred)
    for r, annotated in enumerate(_session_script(T)):
        if r:                                                          # what a propagation round may change: the frames between the neighbours
            cur, others = annotated[-1], set(annotated[:-1])
            lo, hi = max([f for f in others if f < cur] + [-1]), min([f for f in others if f > cur] + [T])
            if r == 2:
                assert (lo + 1, hi) == (1, 9)                          # t0 > 0 and t1 < T
            flip = torch.from_numpy(rng.rand(hi - lo - 1, H, W) < 0.01).cuda()
            lab = p.labels()[lo + 1:hi]
            p.masks[:, 0, p.box[2], p.box[3]][lo + 1:hi] = torch.where(flip, (lab + 1) % (k + 1), lab)
        gen_h = p.labels().cpu().numpy().copy()
        gen_h[annotated] = gt_h[annotated]
        q_ref, Q_ref, sel_ref = metrics.label_round_quality(gt_h, gen_h, k, metric, NO)
        for inc, sc in scorers.items():
            sel, gen = sc.score(p, annotated, incremental=inc)
            assert np.array_equal(gen.cpu().numpy(), gen_h), (r, inc)
            Q, q = sc.qualities()[r], sc.object_qualities()[r]
            print(f"round {r} incremental={inc}: max |dQ| {np.abs(Q - Q_ref).max():.1e}, max |dq| {np.abs(q - q_ref).max():.1e}, select {sel} / {sel_ref}")
            assert Q.dtype == q.dtype == np.float64
            assert np.array_equal(q.view(np.uint64), q_ref.view(np.uint64)), (r, inc)
            assert np.array_equal(Q.view(np.uint64), Q_ref.view(np.uint64)), (r, inc)
            assert sel == sel_ref, (r, inc)
            for f in annotated:                                        # annotated frames score 1.0 for every present object
                assert all(q[o, f] == (1.0 if sc.present_host[o, f] else NO) for o in range(k)) and Q[f] == 1.0
            assert (q[:, 7] == NO).all() and Q[7] == NO and q[1, 4] == NO and Q[4] == (q[0, 4] + q[2, 4]) / 2
    assert scorers[True].qualities().shape == (4, T) and scorers[True].object_qualities().shape == (4, k, T)


# ------------------------------------------------------------------------------------------------ session
def test_oracle_session_of_three_objects_equals_a_host_loop(nets_multi):
    """run_policy(oracle_mask, multi_object) against a second engine from the same weights driven by a literal host loop: download the
    labels, score them with the host restatement, take the arg-min.  The engine is bit-reproducible, so this isolates the new code."""
    from mivos.inference_core import InferenceCore
    T, H, W, k, rounds = 8, 128, 160, 3, 5
    img = synth.synthetic_clip(T, H, W)
    m = synth.synthetic_mask(T, H, W, k)[:, :, 0]
    lab = torch.zeros((T, H, W), dtype=torch.uint8)
    for o in range(k):
        lab[m[o] > 0.5] = o + 1
    lab[T - 1][lab[T - 1] == 2] = 0                                    # object 2 is gone in the last frame
    sample = {"rgb": img, "gt": lab[None, :, None], "num_frames": T, "num_objects": k, "name": "syn", "video": "syn", "object_ids": [0, 1, 2]}
    got = eval_driver.run_policy("oracle_mask", InferenceCore(nets_multi[0], nets_multi[1], img.cuda(), k), sample, rounds, "j_and_f", multi_object=True)
    core = InferenceCore(nets_multi[0], nets_multi[1], img.cuda(), k)
    gt_h = lab.numpy()
    frames, Qs, qs = [0], [], []
    for r in range(rounds):
        f = frames[r]
        onehot = torch.stack([lab[f] == c for c in range(k + 1)]).float()[:, None]
        gen = core.interact(onehot, f, scribble=True).copy()
        gen[frames] = gt_h[frames]
        q, Q, sel = metrics.label_round_quality(gt_h, gen, k, "j_and_f", NO)
        frames.append(sel)
        Qs.append(Q)
        qs.append(q)
    assert got["frames"] == frames, (got["frames"], frames)
    assert len(got["round_metrics"]) == rounds == len(got["object_metrics"])
    for r in range(rounds):
        assert np.array_equal(got["round_metrics"][r].view(np.uint64), Qs[r].view(np.uint64)), r
        assert np.array_equal(got["object_metrics"][r].view(np.uint64), qs[r].view(np.uint64)), r
    assert got["annotation_times"] == [eval_driver.MASK_SECONDS] * rounds and got["present"][1, T - 1] == 0
    assert len(set(frames[:-1])) == rounds                             # five different frames were annotated


# ------------------------------------------------------------------------------------------------ driver
def test_driver_in_multi_object_mode_and_the_per_object_mode_beside_it(nets_multi, tmp_path):
    from mivos.inference_core import InferenceCore
    root = str(tmp_path / "db")
    imset = fq_driver.make_synthetic_tree(root, {"v1": (5, 112, 128, 1), "v2": (6, 112, 128, 2), "v3": (5, 112, 128, 3)})
    rows = {}
    for policy in eval_driver.MULTI_OBJECT_POLICIES:
        out = str(tmp_path / f"{policy}.csv")
        r = rows[policy] = eval_driver.run(root, imset, out, nets_multi[0], nets_multi[1], policy, rounds=3, seed=4, multi_object=True)
        assert r.shape == (6 * 3, 6 + 6)
        order = np.lexsort((r[:, 1], r[:, 0]))
        r = rows[policy] = r[order]
        assert r[:, 0].astype(int).tolist() == [s for s in range(6) for _ in range(3)] and r[:, 1].astype(int).tolist() == [0, 1, 2] * 6
        assert np.isfinite(r[:, 2]).all() and (r[:, 2] >= 0).all() and (r[:, 2] <= 1).all()
        assert (r[r[:, 1] == 0][:, 4] == 0).all()                      # round 0 annotates frame 0
        for row in r:
            n = int(row[5])
            q = row[6:6 + n]
            assert np.all(((q >= 0) & (q <= 1)) | (q == NO)) and np.isnan(row[6 + n:]).all() and row[3] in (3, 80)
            assert q[int(row[4])] in (1.0, NO) and (row[3] == 80) == (q[int(row[4])] == 1.0)
        for a, b in ((1, 2), (3, 4), (4, 5)):                          # the objects of one video share the session's frames
            assert np.array_equal(r[r[:, 0] == a][:, 4], r[r[:, 0] == b][:, 4])
        again = eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], policy, rounds=3, seed=4, multi_object=True)
        assert np.array_equal(np.nan_to_num(again[np.lexsort((again[:, 1], again[:, 0]))]), np.nan_to_num(r))     # two runs; rand_mask: its seed
        lines = open(out).read().split()
        assert lines[0] == "video,mu_metric,annotation_time,round" and len(lines) == 19 and lines[1].startswith("v1__1,") and lines[-1].startswith("v3__3,")
    assert np.array_equal(rows["rand_mask"][rows["rand_mask"][:, 1] == 0][:, 2:6], rows["oracle_mask"][rows["oracle_mask"][:, 1] == 0][:, 2:6])
    other = eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], "rand_mask", rounds=3, seed=5, multi_object=True)
    assert other.shape == (18, 12)
    with pytest.raises(ValueError, match="oracle_mask and rand_mask"):
        eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], "qnet_mask", rounds=3, multi_object=True)
    # the per-object mode on the same tree: what the parent commit's loop gives - one engine per (video, object), scored on the host path
    # that predates the device scorer (eval_driver.frame_quality + numpy.argmin), written out here
    per_object = eval_driver.run(root, imset, "", nets_multi[0], nets_multi[1], "oracle_mask", rounds=3, seed=4)
    per_object = per_object[np.lexsort((per_object[:, 1], per_object[:, 0]))]
    ds = fq_driver.ClipDataset(root, imset)
    want = []
    for i in range(len(ds)):
        s = ds[i]
        gt = s["gt"][0].cuda()
        proc = InferenceCore(nets_multi[0], nets_multi[1], s["rgb"].cuda(), 1)
        frames = [0]
        for r in range(3):
            proc.interact(gt[frames[r]][None], frames[r], download=False)
            mu, _, q = eval_driver.frame_quality(proc, gt[:, 0], sorted(set(frames)), "j_and_f")
            empty = q == NO
            row = np.full(12, np.nan, np.float32)
            row[:6] = (i, r, mu, 80, frames[r], len(q))
            row[6:6 + len(q)] = q
            want.append(row)
            frames.append(int(np.argmin(q)))
            assert not empty[frames[-1]]
    assert np.array_equal(np.nan_to_num(per_object), np.nan_to_num(np.stack(want)))
