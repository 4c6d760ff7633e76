"""The J / F metric kernels (csrc/metrics.hip) on the cases of tests/metric_cases.py: frames shorter than, as long as and just longer
than the 1024 pixels a wave walks (waves across many frame boundaries: the per-pixel global atomics of every counting kernel), frames of
one row or column, radii whose 0.008 x diagonal is an integer with marks on and just outside the circle, radii above an extent of the
frame, disks clipped by a corner, the largest accepted radius, 2^24 pixels, a clip of more than 2^31 pixels, the round scorers on 300
tiny frames with tied minima, and the scratch the calls ask for.  Every comparison is exact: the six integers per frame and object,
quality as float64 bit patterns, the selection.  The yardstick is the feature-transform count of tests/metric_cases.py, which
tests/test_metric_cases.py holds to the host metrics and each case to what it is named for."""
import numpy as np
import pytest
import torch

import metric_cases as mc
from eva_vos_amd import _lib, metrics

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
_ptr, _stream = metrics._ptr, metrics._stream


def to_dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the cases are read-only arrays


def device_counts(gt, pred, k=None, j_only=False, scratch=None):
    """The counts of device masks / label maps uint8 [T,H,W] through the C entry points: int32 [T,6] or [k,T,6] as a NumPy array.  The
    counters start as -1: every one has to be written."""
    T, H, W = gt.shape
    name = f"stcn_metrics_{'' if k is None else 'objects_'}{'j' if j_only else 'jf'}_counts"
    counts = torch.full((T, 6) if k is None else (k, T, 6), -1, dtype=torch.int32, device=DEV)
    if not j_only and scratch is None:
        scratch = metrics._boundary_scratch(k, T, H, W, DEV)
    with torch.cuda.device(DEV):
        _lib.check(getattr(_lib.lib(), name)(_stream(), _ptr(gt), _ptr(pred), *(() if k is None else (k,)), T, H, W, _ptr(counts),
                                             *(() if j_only else (_ptr(scratch),))), name)
    return counts.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_clip(name):
    """A named clip in the four forms: binary J&F, binary J, label maps of 3 objects (byte sets) and of 9 (32-bit sets), those in both too."""
    for k in mc.FORMS:
        gt, pred = mc.clip(name, k)
        want = mc.want(name, k)
        g, p = to_dev(gt), to_dev(pred)
        got = device_counts(g, p, k)
        assert np.array_equal(got, want), (name, k, np.argwhere(got != want)[:8].tolist())
        got_j = device_counts(g, p, k, j_only=True)
        assert np.array_equal(got_j[..., :2], want[..., :2]) and not got_j[..., 2:].any(), (name, k)
        # the public calls: rows (J, F, J&F) as float64, from these integers
        if k is None:
            assert same_bits(metrics.sequence_scores_gpu(g, p), metrics._scores_from_counts(want)), name
        else:
            assert same_bits(metrics.sequence_scores_objects_gpu(g, p, k), np.stack([metrics._scores_from_counts(c) for c in want])), (name, k)


@pytest.mark.parametrize("T,H,W", mc.WALK_SHAPES)
def test_frames_shorter_than_as_long_as_and_just_longer_than_a_waves_walk(T, H, W):
    check_clip(("noise", T, H, W))


@pytest.mark.parametrize("T,H,W", mc.LINE_SHAPES)
def test_the_region_measure_of_frames_of_one_row_one_column_one_pixel(T, H, W):
    gt, pred = mc.clip(("noise", T, H, W))
    want = mc.counts(gt, pred)
    assert not want[:, 2:].any()
    got = device_counts(to_dev(gt), to_dev(pred), j_only=True)
    assert np.array_equal(got, want)
    rows = metrics.sequence_scores_gpu(to_dev(gt), to_dev(pred), j_only=True)
    assert same_bits(rows[:, 0], metrics._scores_from_counts(want)[:, 0]) and np.isnan(rows[:, 1:]).all()


@pytest.mark.parametrize("H,W", mc.CIRCLE_SHAPES)
def test_integer_radius_products_and_marks_on_and_one_outside_the_circle(H, W):
    """Equal counts on frame 1 - marks whose far boundary pixels lie at d^2 = r^2 and r^2 + 1 - say that the library's radius is the host's:
    one more would match the pixels at r^2 + 1, one less would lose those at r^2."""
    check_clip(("circle", H, W))


@pytest.mark.parametrize("T,H,W", mc.THIN_SHAPES)
def test_a_radius_above_an_extent_of_the_frame(T, H, W):
    check_clip(("noise", T, H, W))


def test_disks_clipped_by_each_of_the_four_corners():
    check_clip(("corners",))


@pytest.mark.parametrize("name,k", [("cap_row", None), ("cap_row", 3), ("cap_column", None), ("cap_column", 3)])
def test_the_largest_accepted_radius(name, k):
    """2 x 5 792 374 at r = 46339, the limit, with pairs at dx = r, dy = 0 (matched) and dx = r, dy = 1 (d^2 = r^2 + 1, unmatched).  The
    scan costs O(r) per row of the disk that lies inside the frame: two rows here, so an unmatched pixel is cheap.  In a column-thin frame
    every row does, an unmatched boundary pixel costs about r^2 loop trips in one lane - 4e9 at the limit - so the column-thin case stays
    at 125000 x 2 (r = 1001), and both keep their unmatched pixels to four."""
    g, p, want = mc.sparse(name, k)
    got = device_counts(to_dev(g[None]), to_dev(p[None]), k)
    assert np.array_equal(got[..., 0, :], want), (got.tolist(), want.tolist())


@pytest.mark.parametrize("k", [None, 32])
def test_2_pow_24_pixels_objects_in_the_four_corners_and_the_centre(k):
    g, p, want = mc.sparse("big_frame", k)
    gd, pd = to_dev(g[None]), to_dev(p[None])
    got = device_counts(gd, pd, k)
    assert np.array_equal(got[..., 0, :], want), (got.tolist(), want.tolist())
    got_j = device_counts(gd, pd, k, j_only=True)
    assert np.array_equal(got_j[..., 0, :2], want[..., :2]) and not got_j[..., 2:].any()


def test_a_clip_of_more_than_2_pow_31_pixels():
    """2050 x 1024 x 1024, zeroed on the device, content pasted into frames 0, 2047, 2048 and 2049 only: frame 2048 starts at byte 2^31.
    Binary masks, label maps of 3 objects, and one incremental round whose recounted frames are 2048 and 2049.  About 9 GB of device memory."""
    T, H, W = mc.LONG
    gt = torch.zeros((T, H, W), dtype=torch.uint8, device=DEV)
    pred = torch.zeros((T, H, W), dtype=torch.uint8, device=DEV)
    try:
        for k in (None, 3):
            for t, (y, x, g, p) in mc.long_patches(k).items():
                gt[t, y:y + 96, x:x + 96], pred[t, y:y + 96, x:x + 96] = to_dev(g), to_dev(p)
            scratch = metrics._boundary_scratch(k, T, H, W, DEV)
            assert scratch.numel() == T * H * W * (1 if k is None else 2) > 1 << 31
            want = mc.long_counts(k)
            got = device_counts(gt, pred, k, scratch=scratch)
            assert np.array_equal(got, want), (k, np.argwhere(got != want)[:8].tolist())
            if k is None:
                # the round after frame 2049 was annotated: frames [2048, 2050) are composed and counted again, the others keep their counts
                counts = to_dev(got)
                counts[2048:] = -5
                flags = np.zeros(T, np.uint8)
                flags[2049] = 1
                noobj = np.ones(T, np.uint8)
                noobj[list(mc.LONG_FRAMES)] = 0
                gen = torch.empty((T, H, W), dtype=torch.uint8, device=DEV)
                gen[2047:] = 9
                quality = torch.full((T,), -1.0, dtype=torch.float64, device=DEV)
                select = torch.full((1,), -1, dtype=torch.int32, device=DEV)
                fl, no = to_dev(flags), to_dev(noobj)
                with torch.cuda.device(DEV):
                    _lib.check(_lib.lib().stcn_metrics_round(_stream(), _ptr(pred), H, W, 0, 0, _ptr(gt), _ptr(fl), _ptr(no), T, H, W, 2048, T, 0, mc.NO,
                                                             _ptr(gen), _ptr(scratch), _ptr(counts), _ptr(quality), _ptr(select)), "stcn_metrics_round")
                want_r = mc.long_counts(None, gen_is_gt=(2049,))
                assert np.array_equal(counts.cpu().numpy(), want_r)
                assert torch.equal(gen[2048], pred[2048]) and torch.equal(gen[2049], gt[2049]) and bool((gen[2047] == 9).all())
                q = metrics._scores_from_counts(want_r)[:, 2].copy()
                q[noobj != 0] = mc.NO
                assert same_bits(quality.cpu().numpy(), q) and q[2049] == 1.0
                assert int(select.item()) == int(np.argmin(q)) and int(np.argmin(q)) in mc.LONG_FRAMES
                del gen, counts
            del scratch
    finally:
        del gt, pred
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ scorers: 300 tiny frames, tied minima
class Proc:                                        # the attributes of an InferenceCore a scorer reads
    pass


def processor(plane):
    s = mc.SESSION
    p = Proc()
    p.nh, p.nw = s["nh"], s["nw"]
    p.pad = (s["lw"], s["nw"] - s["W"] - s["lw"], s["lh"], s["nh"] - s["H"] - s["lh"])
    p.masks = to_dev(plane)
    return p


def check_round(sc, r, sel, gen, host, metric, k):
    gen_h, c, q, Q, sel_h = host
    assert np.array_equal(gen.cpu().numpy(), gen_h), r
    got = sc.counts.cpu().numpy()
    assert np.array_equal(got[..., :2], c[..., :2]) and (np.array_equal(got, c) if metric != "j" else not got[..., 2:].any()), r
    row = sc.qualities()[r]
    assert same_bits(row, Q), (r, np.flatnonzero(row != Q)[:8].tolist())
    if k is not None:
        assert same_bits(sc.object_qualities()[r], q), r
    assert sel == sel_h == int(np.argmin(row)), (r, sel, sel_h)


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
@pytest.mark.parametrize("kind", ["plain", "typed", "objects"])
def test_the_scorers_on_300_frames_of_3_x_5_with_tied_minima(kind, metric):
    """T = 300 > 256: a thread of the quality kernel takes frames t and t + 256, and the minimum is tied first between frames 5 and 260 -
    thread 5's first trip against thread 4's second, and against its own second trip (frame 261) - then between 260 and 270, both second
    trips.  The selection is numpy.argmin of the
    host row; the rows are equal bit for bit.  The second round is incremental: frames [0, 100) are composed and counted again.  Between
    the rounds the one-object scorer runs trials, which leave it as it was."""
    s = mc.SESSION
    T, k = s["T"], (3 if kind == "objects" else None)
    gt, planes, annot = mc.session(k)
    if kind == "typed":
        sc = metrics.TypedRoundScorer(to_dev(gt), metric, max_rounds=2, no_object=mc.NO)
    else:
        sc = metrics.RoundScorer(to_dev(gt), metric, max_rounds=2, no_object=mc.NO, num_objects=k)
    types = (lambda n: dict(types=[1, 2][:n])) if kind == "typed" else (lambda n: {})
    flags = np.zeros(T, np.uint8)
    flags[s["first"]] = 1
    p = processor(planes[0])
    sel, gen = sc.score(p, [s["first"]], **types(1))
    check_round(sc, 0, sel, gen, mc.host_round(gt, planes[0], flags, metric, k, annot), metric, k)
    assert sel == s["ties"][0][0] == 5
    if kind == "plain":
        rng = np.random.RandomState(7)
        cands, rows = (5, 260, 299, 2, 99, 101), []
        for row, c in enumerate(cands):                       # spans [0, 100) and [101, 300); frame 2 has no object
            lo, hi = (0, s["first"]) if c < s["first"] else (s["first"] + 1, T)
            tried = planes[0].copy()
            tried[lo:hi, 0, s["lh"]:s["lh"] + s["H"], s["lw"]:s["lw"] + s["W"]] ^= (rng.rand(hi - lo, s["H"], s["W"]) < 0.2).astype(np.uint8)
            f2 = flags.copy()
            f2[c] = 1
            rows.append(mc.host_round(gt, tried, f2, metric)[3])
            p.masks = to_dev(tried)
            sc.score_trial(p, [s["first"]], c, row)
        got = sc.trial_rows(len(cands))
        for row, c in enumerate(cands):
            assert same_bits(got[row], rows[row]), (c, np.flatnonzero(got[row] != rows[row])[:8].tolist())
            assert got[row][c] == (mc.NO if c == 2 else 1.0)
    if kind == "typed":
        sc.set_annotation(5, to_dev(annot[5]))
    flags[5] = 2 if kind == "typed" else 1
    p.masks = to_dev(planes[1])
    sel, gen = sc.score(p, [s["first"], 5], **types(2))
    check_round(sc, 1, sel, gen, mc.host_round(gt, planes[1], flags, metric, k, annot), metric, k)
    assert sel == s["ties"][1][0] == 260


# ------------------------------------------------------------------------------------------------ the scratch is what the kernels write
SENTINEL = 0xA5                  # no boundary byte (values 0 .. 3) and no byte of an object set of k <= 9 objects takes this value
TAIL = 1 << 16


@pytest.mark.parametrize("k", mc.FORMS)
@pytest.mark.parametrize("T,H,W", [(41, 2, 3), (3, 37, 53)])
def test_the_kernels_write_all_of_the_scratch_they_ask_for_and_nothing_behind_it(T, H, W, k):
    gt, pred = mc.clip(("noise", T, H, W), k)
    if k is None:
        need = T * H * W
    else:
        need = metrics._objects_scratch(k, T, H, W, DEV).numel()
        assert need == T * H * W * (2 if k <= 8 else 8)
    big = torch.full((need + TAIL,), SENTINEL, dtype=torch.uint8, device=DEV)
    got = device_counts(to_dev(gt), to_dev(pred), k, scratch=big)
    assert bool((big[need:] == SENTINEL).all())
    assert not bool((big[:need] == SENTINEL).any())              # every byte of the scratch was written
    assert np.array_equal(got, mc.want(("noise", T, H, W), k))
