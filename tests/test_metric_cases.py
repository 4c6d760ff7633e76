"""CPU: the yardstick and the cases of tests/metric_cases.py, and the radius limit of the metric entry points.  The yardstick (nearest
boundary pixel by the feature transform) equals the host metrics (dilation by a disk) wherever both can be computed; every named case is
what it is named for; a shape whose disk radius exceeds METRICS_MAX_RADIUS is refused by every entry point that builds boundary maps,
before any device call - the calls below pass host buffers that are never dereferenced, and every call that is NOT refused for its radius
is made so that a later argument check refuses it.  GPU twin: tests/test_gpu_metric_extents.py."""
import ctypes as C

import numpy as np
import pytest

import metric_cases as mc
from eva_vos_amd import _lib, metrics

INVALID = -1                     # STCN_E_INVALID
SMALL = ((2, 2), (2, 3), (5, 7), (3, 341), (32, 32), (25, 41), (37, 53), (75, 100), (300, 400), (375, 500), (2, 1000), (1000, 2))


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("H,W", SMALL)
def test_the_yardstick_equals_the_dilation_path_on_binary_masks(H, W):
    rng = np.random.RandomState(H * W)
    gt = np.stack([rng.rand(H, W) < d for d in (0.5, 0.02, 0.002, 0.5, 0.0)]).astype(np.uint8)
    pred = np.stack([rng.rand(H, W) < d for d in (0.5, 0.02, 0.002, 0.002, 0.02)]).astype(np.uint8)
    c = mc.counts(gt, pred)
    assert np.array_equal(c, metrics.label_counts(gt, pred, 1)[0])
    rows = metrics._scores_from_counts(c)
    for t in range(len(gt)):
        assert rows[t, 0] == metrics.jaccard(gt[t], pred[t]) and rows[t, 1] == metrics.f_measure(gt[t], pred[t]), t


@pytest.mark.parametrize("H,W", [(2, 3), (5, 7), (25, 41), (75, 100), (2, 1000)])
def test_the_yardstick_equals_the_dilation_path_on_label_maps(H, W):
    gt, pred = mc.noise_clip(4, H, W, k=3, seed=1)
    assert gt.max() == 4 or H * W < 30, "a label above k takes part"
    assert np.array_equal(mc.label_counts(gt, pred, 3), metrics.label_counts(gt, pred, 3))


def test_windows_give_the_counts_of_the_whole_frame():
    for k in (None, 3):                                                   # 125000 x 2: small enough for the transform of the whole frame
        g, p, c = mc.sparse("cap_column", k)
        whole = mc.frame_counts(g != 0, p != 0) if k is None else np.stack([mc.frame_counts(g == o, p == o) for o in range(1, k + 1)])
        assert np.array_equal(whole, c) and c.any()


# ------------------------------------------------------------------------------------------------ the cases are what they are named for
def _nearest(g, p):
    """(d^2 of every gt boundary pixel to the nearest pred boundary pixel, the same for the pred boundary pixels)"""
    gb, fb = metrics.boundary_map(g != 0), metrics.boundary_map(p != 0)
    return mc.nearest_sq(gb, fb), mc.nearest_sq(fb, gb)


def test_frames_shorter_than_equal_to_and_longer_than_the_walk():
    sizes = [H * W for _, H, W in mc.WALK_SHAPES]
    assert sizes == [4, 6, 35, 1023, 1024, 1025, 1024] and mc.WALK == 1024
    assert mc.WALK // 4 == 256 and 300 * 4 > mc.WALK                     # 2 x 2: 256 frames in a wave, and a second wave
    for T, H, W in mc.WALK_SHAPES:
        for k in mc.FORMS:
            gt, pred = mc.clip(("noise", T, H, W), k)
            assert not gt[1].any() and not pred[1].any() and gt[2].all() and pred[2].all()
            dens = [float((gt[t] != 0).mean()) for t in range(0, T, 2) if t != 2]
            assert gt[0].any() and (H * W < 1000 or all(0.4 < d < 0.6 for d in dens))
    assert all(min(H, W) == 1 for _, H, W in mc.LINE_SHAPES)


def test_the_radius_products_are_integers_and_the_marks_lie_on_and_one_outside_the_circle():
    for (H, W), r in zip(mc.CIRCLE_SHAPES, (1, 4, 5)):
        assert 0.008 * np.linalg.norm((H, W)) == float(r) and mc.radius(H, W) == r
        gt, pred = mc.clip(("circle", H, W))
        for d2 in _nearest(gt[1], pred[1]):
            assert r * r in d2 and r * r + 1 in d2 and d2.max() == r * r + 1
        c = mc.want(("circle", H, W))[1]
        assert 0 < c[4] < c[2] and 0 < c[5] < c[3]
        for k in (3, 9):                                                  # with another object's mark beside every predicted one
            w = mc.want(("circle", H, W), k)[:, 1]
            assert (w[:, 4] < w[:, 2]).any() and (w[:, 5] < w[:, 3]).any()
    offs = [(dy, dx) for (gy, gx), (py, px) in mc.circle_pairs(375, 500) for dy, dx in [(abs(py - gy), abs(px - gx))]]
    assert {(3, 4), (5, 0), (1, 5)} <= set(offs)


def test_thin_frames_are_thinner_than_their_radius_and_corner_disks_are_clipped():
    assert [mc.radius(H, W) for _, H, W in mc.THIN_SHAPES] == [9, 9, 161]
    assert all(mc.radius(H, W) >= min(H, W) for _, H, W in mc.THIN_SHAPES)
    gt, pred = mc.clip(("corners",))
    H, W = gt.shape[1:]
    assert (H, W) == (60, 90) and mc.radius(H, W) == 1
    for t in range(2):
        assert all((gt[t] | pred[t])[y, x] for y in (0, H - 1) for x in (0, W - 1))
        a, b = _nearest(gt[t], pred[t])
        assert {1, 2} <= set(a.tolist()) | set(b.tolist())


@pytest.mark.parametrize("name", ["cap_row", "cap_column"])
def test_the_pairs_at_the_largest_radius_lie_on_and_one_outside_the_circle(name):
    g, p, c = mc.sparse(name)
    H, W = g.shape
    r = mc.radius(H, W)
    if name == "cap_row":
        assert H == 2 and W == mc.cap_width() and r == mc.MAX_RADIUS and mc.radius(2, W + 1) == r + 1 and mc.radius(W + 1, 2) == r + 1
    else:
        assert (H, W) == (125000, 2) and r == 1001
    assert c[2] + c[3] <= 100 and (c[2] - c[4]) + (c[3] - c[5]) == 4, "few boundary pixels, four of them unmatched"
    assert c[2] > c[4] and c[3] > c[5]
    edge = g | p
    assert edge[:, :2].any() and edge[:, -1].any() if name == "cap_row" else edge[:2].any() and edge[-1].any()
    y0, y1, x0, x1 = (mc.cap_row if name == "cap_row" else mc.cap_column)()[2][1]
    for d2 in _nearest(g[y0:y1, x0:x1], p[y0:y1, x0:x1]):
        assert r * r in d2 and d2.max() <= r * r + 1
    both = np.concatenate(_nearest(g[y0:y1, x0:x1], p[y0:y1, x0:x1]))
    assert r * r + 1 in both
    ck = mc.sparse(name, 3)[2]
    assert np.array_equal(ck.sum(0)[2:], c[2:]), "one object per pair: the objects' boundary counts add up to the binary ones"


def test_the_2_pow_24_pixel_frame_has_objects_in_its_corners_and_its_centre():
    for k in (None, 32):
        g, p, c = mc.sparse("big_frame", k)
        assert g.shape == (mc.BIG, mc.BIG) and g.size == 1 << 24 and mc.radius(*g.shape) == 47
        S, m = 40, mc.BIG // 2
        for ys, xs in ((slice(0, S), slice(0, S)), (slice(0, S), slice(-S, None)), (slice(-S, None), slice(0, S)), (slice(-S, None), slice(-S, None)),
                       (slice(m, m + S), slice(m, m + S))):
            assert g[ys, xs].any() and p[ys, xs].any()
        assert np.count_nonzero(g) < 2000
        if k is None:
            assert c[3] - c[5] >= 1 and c[2] - c[4] >= 1                  # the pair at (47, 1): d^2 = 47^2 + 1
        else:
            assert g.max() == 33 and (c[:, 1] > 0).all()


def test_the_long_clip_passes_2_pow_31_pixels_and_has_content_in_four_frames_only():
    T, H, W = mc.LONG
    assert T * H * W > 1 << 31 and 2048 * H * W == 1 << 31
    assert sorted(mc.LONG_FRAMES) == [0, 2047, 2048, 2049]
    for k in (None, 3):
        pt = mc.long_patches(k)
        y, x, g, p = pt[2048]
        assert (y, x) == (0, 0) and g[0, 0] and p[0, 0]                   # the pixel at byte 2^31
        y, x, g, p = pt[2049]
        assert (y + 96, x + 96) == (H, W) and g[-1, -1] and p[-1, -1]     # the last pixel of the clip
        y, x, g, p = pt[2047]
        assert (y + 96, x + 96) == (H, W) and g[-1, -1]                   # the pixel in front of byte 2^31
        c = mc.long_counts(k)
        rest = np.ones(T, bool)
        rest[list(mc.LONG_FRAMES)] = False
        assert not c[..., rest, :].any() and (c[..., ~rest, :][..., :4] > 0).all()
    full = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    y, x, g, p = mc.long_patches()[2049]
    full[0][y:, x:], full[1][y:, x:] = g, p
    assert np.array_equal(mc.frame_counts(full[0] != 0, full[1] != 0), mc.long_counts()[2049]), "the window is the frame"


@pytest.mark.parametrize("metric", ["j", "j_and_f"])
@pytest.mark.parametrize("k", [None, 3])
def test_the_sessions_tie_where_they_say(k, metric):
    s = mc.SESSION
    gt, planes, annot = mc.session(k)
    assert gt.shape == (300, 3, 5) and planes[0].shape == (300, 1, 16, 16) and not gt[:4].any() and gt[4:].reshape(296, -1).any(1).all()
    flags = np.zeros(s["T"], np.uint8)
    flags[s["first"]] = 1
    for rnd, (a, b) in enumerate(s["ties"]):
        for second in ((1, 2) if rnd and k is None else (1,)):            # a typed session annotates frame 5 with clicks (type 2)
            if rnd:
                flags[5] = second
            gen, c, q, Q, sel = mc.host_round(gt, planes[rnd], flags, metric, k, annot)
            low = np.flatnonzero(Q == Q.min())
            assert low.tolist() == [f for f in (5, 260, 261, 270) if f >= a] and b in low and sel == a and (Q[:4] == mc.NO).all() and Q[s["first"]] == 1.0
            assert a % 256 > b % 256 or a // 256 == b // 256 == 1, "the first minimum belongs to a LATER thread of the quality kernel, or both to second trips"
            if rnd:
                assert (Q[5] == 1.0) == (second == 1) and Q[5] > Q.min()
    assert not np.array_equal(planes[0][:100], planes[1][:100]) and np.array_equal(planes[0][100:, 0, 6:9, 5:10], planes[1][100:, 0, 6:9, 5:10])


# ------------------------------------------------------------------------------------------------ the radius limit
W_OK = mc.cap_width()            # 2 x W_OK: radius 46339, the last accepted thin frame
W_BAD = W_OK + 1                 # radius 46340: (r + 1)^2 leaves int

_bufs = {}


def _p(name):
    _bufs.setdefault(name, (C.c_uint8 * 16)())
    return C.cast(_bufs[name], C.c_void_p)


def _call(entry, H, W, j_only=0, last=True, nh=1 << 24):
    """One metric call on host buffers.  ``last=False``: the last pointer of a counts call is null; ``nh``: 16 makes the crop of a round
    call leave its tensor - the check that follows the shape's."""
    lib, k, T = _lib.lib(), 3, 2
    last_p = lambda n: _p(n) if last else None                            # noqa: E731
    if entry == "stcn_metrics_jf_counts":
        return lib.stcn_metrics_jf_counts(None, _p("gt"), _p("pred"), T, H, W, _p("counts"), last_p("scratch"))
    if entry == "stcn_metrics_j_counts":
        return lib.stcn_metrics_j_counts(None, _p("gt"), _p("pred"), T, H, W, last_p("counts"))
    if entry == "stcn_metrics_objects_jf_counts":
        return lib.stcn_metrics_objects_jf_counts(None, _p("gt"), _p("pred"), k, T, H, W, _p("counts"), last_p("scratch"))
    if entry == "stcn_metrics_objects_j_counts":
        return lib.stcn_metrics_objects_j_counts(None, _p("gt"), _p("pred"), k, T, H, W, last_p("counts"))
    head = (None, _p("masks"), nh, nh, 0, 0, _p("gt"), _p("flags"))
    tail = (T, H, W, 0, T, j_only, 20.0, _p("gen"), _p("scratch"), _p("counts"))
    if entry == "stcn_metrics_round":
        return lib.stcn_metrics_round(*head, _p("noobj"), *tail, _p("quality"), _p("select"))
    if entry == "stcn_metrics_round_typed":
        return lib.stcn_metrics_round_typed(*head, _p("annot"), _p("noobj"), *tail, _p("quality"), _p("select"))
    if entry == "stcn_metrics_objects_round":
        return lib.stcn_metrics_objects_round(*head, _p("present"), k, *tail, _p("oq"), _p("quality"), _p("select"))
    assert entry == "stcn_metrics_trial"
    return lib.stcn_metrics_trial(*head, _p("noobj"), 1, T, H, W, 0, T, j_only, 20.0, _p("counts"), _p("gen"), _p("scratch"), _p("span"), _p("quality"))


def _refused(rc, *words):
    assert rc == INVALID, rc
    msg = _lib.lib().stcn_last_error().decode()
    assert msg and all(str(w) in msg for w in words), msg
    return msg


COUNTS = ("stcn_metrics_jf_counts", "stcn_metrics_objects_jf_counts")
J_COUNTS = ("stcn_metrics_j_counts", "stcn_metrics_objects_j_counts")
ROUNDS = ("stcn_metrics_round", "stcn_metrics_round_typed", "stcn_metrics_objects_round", "stcn_metrics_trial")


def test_the_limit_is_the_largest_radius_whose_scan_stays_in_int():
    r = mc.MAX_RADIUS
    assert (r + 1) ** 2 <= 2 ** 31 - 1 < (r + 2) ** 2 and r == 46339
    assert mc.radius(2, W_OK) == r and mc.radius(2, W_BAD) == r + 1 and mc.radius(2, 5792500) == r + 2
    assert 2 * W_BAD < 1 << 24, "fewer pixels than the engine's largest frame"


@pytest.mark.parametrize("H,W", [(2, W_BAD), (W_BAD, 2), (2, 5792500), (40000000, 40000000)])
@pytest.mark.parametrize("entry", COUNTS + ROUNDS)
def test_a_radius_above_the_limit_is_refused_by_every_call_that_builds_boundary_maps(entry, H, W):
    _refused(_call(entry, H, W), entry, f"H={H}", f"W={W}", mc.radius(H, W), "46339", "METRICS_MAX_RADIUS")


@pytest.mark.parametrize("H,W", [(2, W_BAD), (W_BAD, 2)])
def test_the_scratch_size_of_such_a_shape_is_refused_and_nothing_is_written(H, W):
    n = C.c_int64(-7)
    _refused(_lib.lib().stcn_metrics_objects_scratch(3, 2, H, W, C.byref(n)), "stcn_metrics_objects_scratch", f"H={H}", f"W={W}", 46340, "46339")
    assert n.value == -7


@pytest.mark.parametrize("H,W", [(2, W_OK), (W_OK, 2)])
def test_the_last_accepted_thin_frame_is_not_refused_for_its_radius(H, W):
    n = C.c_int64(-7)
    assert _lib.lib().stcn_metrics_objects_scratch(3, 2, H, W, C.byref(n)) == 0 and n.value == 2 * 2 * H * W
    assert _lib.lib().stcn_metrics_objects_scratch(9, 2, H, W, C.byref(n)) == 0 and n.value == 8 * 2 * H * W
    for entry in COUNTS:                                                  # the checks behind the radius are reached
        assert "radius" not in _refused(_call(entry, H, W, last=False), entry, "null pointer")
    for entry in ROUNDS:
        assert "radius" not in _refused(_call(entry, H, W, nh=16), entry, "crop")


@pytest.mark.parametrize("H,W", [(2, W_BAD), (W_BAD, 2), (40000000, 40000000)])
def test_the_j_only_calls_have_no_disk_and_take_every_shape(H, W):
    for entry in J_COUNTS:
        assert "radius" not in _refused(_call(entry, H, W, last=False), entry, "null pointer")
    for entry in ROUNDS:
        assert "radius" not in _refused(_call(entry, H, W, j_only=1, nh=16), entry, "crop")
