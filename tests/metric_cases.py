"""Cases for the J / F metric kernels (csrc/metrics.hip) at the extents of their domain, and the yardstick they are held to.  Host only
(NumPy / SciPy): tests/test_metric_cases.py checks that the yardstick equals the host metrics and that every case is what it is named
for, tests/test_gpu_metric_extents.py runs the cases on the device.

The yardstick of the six counts of a frame - intersection, union, gt boundary px, pred boundary px, matched gt boundary px, matched pred
boundary px - takes the boundary maps from ``metrics.boundary_map`` (which tests/golden/metrics.npz holds to the reference) and matches
them NOT by dilation but by the nearest-boundary feature transform: a boundary pixel is matched iff the nearest pixel of the other map
lies at an integer squared distance d^2 <= r^2.  That is independent of the kernel's disk walk and of the host's ``binary_dilation``, and
it works at radii whose (2 r + 1)^2 structuring element cannot be built.

A wave of the counting kernels owns 64 x PPT = 1024 consecutive pixels of the clip (``WALK``)."""
import functools

import numpy as np
from scipy import ndimage

from eva_vos_amd import metrics

WALK = 1024                     # metrics.hip: 64 lanes x PPT pixels
MAX_RADIUS = 46339              # kernels.h METRICS_MAX_RADIUS: the largest r with (r + 1)^2 <= INT_MAX
NO = 20.0                       # the NO_OBJECT token of the drivers
assert (MAX_RADIUS + 1) ** 2 <= 2 ** 31 - 1 < (MAX_RADIUS + 2) ** 2


def radius(H, W) -> int:
    """The disk radius of the boundary measure as the host metrics compute it (metrics.f_measure, metrics.label_counts)."""
    return int(np.ceil(0.008 * np.linalg.norm((H, W))))


# ------------------------------------------------------------------------------------------------ the yardstick
def nearest_sq(b, other) -> np.ndarray:
    """int64, one per pixel of the boolean map ``b`` in raster order: the squared distance to the nearest pixel of ``other`` (not empty)."""
    idx = ndimage.distance_transform_edt(~other, return_distances=False, return_indices=True)
    yy, xx = np.nonzero(b)
    dy, dx = idx[0][yy, xx].astype(np.int64) - yy, idx[1][yy, xx].astype(np.int64) - xx
    return dy * dy + dx * dx


def matched(b, other, r) -> int:
    if not b.any() or not other.any():
        return 0
    return int((nearest_sq(b, other) <= int(r) * int(r)).sum())


def frame_counts(g, p, r=None) -> np.ndarray:
    """int64 [6] of one frame of boolean masks; ``r``: the radius, the frame's own when None (a window of a larger frame passes it)."""
    g, p = np.asarray(g, bool), np.asarray(p, bool)
    r = radius(*g.shape) if r is None else r
    if min(g.shape) < 2:                                      # the J-only forms take frames of one row or column: no boundary there
        return np.array([(g & p).sum(), (g | p).sum(), 0, 0, 0, 0], np.int64)
    gb, fb = metrics.boundary_map(g), metrics.boundary_map(p)
    return np.array([(g & p).sum(), (g | p).sum(), gb.sum(), fb.sum(), matched(gb, fb, r), matched(fb, gb, r)], np.int64)


def counts(gt, pred) -> np.ndarray:
    """uint8 [T,H,W] masks (non-zero = object) -> int64 [T,6]."""
    return np.stack([frame_counts(g != 0, p != 0) for g, p in zip(gt, pred)])


def label_counts(gt, pred, k) -> np.ndarray:
    """Label maps [T,H,W] -> int64 [k,T,6]: per object o the counts of ``gt == o`` and ``pred == o`` (a label above k is background)."""
    return np.stack([np.stack([frame_counts(g == o, p == o) for g, p in zip(gt, pred)]) for o in range(1, k + 1)])


def window_counts(g, p, boxes, k=None) -> np.ndarray:
    """The counts of ONE large, mostly empty frame from windows (y0, y1, x0, x1): int64 [6], or [k,6] for label maps.  Checked here:
    the windows are disjoint, nothing is set outside them, and inside a window everything set keeps more than r + 1 pixels from every
    edge of the window that is not an edge of the frame - so no boundary pixel and no match involves two windows or a cut."""
    H, W = g.shape
    r = radius(H, W)
    total = np.zeros((6,) if k is None else (k, 6), np.int64)
    inside = 0
    for n, (y0, y1, x0, x1) in enumerate(boxes):
        for m, (v0, v1, u0, u1) in enumerate(boxes[:n]):
            assert y1 <= v0 or v1 <= y0 or x1 <= u0 or u1 <= x0, (n, m)
        gw, pw = g[y0:y1, x0:x1], p[y0:y1, x0:x1]
        on = (gw != 0) | (pw != 0)
        inside += int(on.sum())
        yy, xx = np.nonzero(on)
        if yy.size:
            m = r + 2
            assert (y0 == 0 or yy.min() >= m) and (y1 == H or yy.max() < y1 - y0 - m), (n, "rows")
            assert (x0 == 0 or xx.min() >= m) and (x1 == W or xx.max() < x1 - x0 - m), (n, "columns")
        if k is None:
            total += frame_counts(gw != 0, pw != 0, r)
        else:
            total += np.stack([frame_counts(gw == o, pw == o, r) for o in range(1, k + 1)])
    assert inside == int(np.count_nonzero((g != 0) | (p != 0))), "content outside the windows"
    return total


# ------------------------------------------------------------------------------------------------ builders
def _noise_pair(rng, shape, density, k=None):
    """(gt, pred) uint8: seeded noise of one density, the prediction agreeing with the ground truth on about 70 % of the pixels and drawn
    afresh on the others.  Label maps draw labels 1 .. k + 1: the last one is an object that appears later (background)."""
    def draw():
        on = rng.rand(*shape) < density
        return (on if k is None else on * rng.randint(1, k + 2, shape)).astype(np.uint8)
    gt, fresh = draw(), draw()
    return gt, np.where(rng.rand(*shape) < 0.7, gt, fresh).astype(np.uint8)


def noise_clip(T, H, W, k=None, seed=0):
    """(gt, pred) uint8 [T,H,W]: frames alternate between densities 0.5 and 0.02 (a single frame has one in each half); with T >= 3
    frame 1 is empty in both maps and frame 2 all set (label maps: all object 2) in both, with T >= 5 frame 3 has an empty ground truth
    and frame 4 an empty prediction."""
    rng = np.random.RandomState(1000 * T + 10 * H + W + 7 * seed + (0 if k is None else k))
    gt, pred = np.zeros((T, H, W), np.uint8), np.zeros((T, H, W), np.uint8)
    for t in range(T):
        gt[t], pred[t] = _noise_pair(rng, (H, W), 0.5 if t % 2 == 0 else 0.02, k)
    if T == 1:                                                # one frame: the sparse density in its right half
        gt[0, :, W // 2:], pred[0, :, W // 2:] = _noise_pair(rng, (H, W - W // 2), 0.02, k)
    if T >= 3:
        gt[1] = pred[1] = 0
        gt[2] = pred[2] = 1 if k is None else 2
    if T >= 5:
        gt[3] = 0
        pred[4] = 0
    return gt, pred


def _value(n, k):
    return 1 if k is None else 1 + n % k


def marks(H, W, pairs, k=None, foreign=False):
    """One frame (gt, pred) of isolated one-pixel marks: pairs of ((gy, gx), (py, px)) - a ground-truth pixel and the predicted pixel that
    belongs to it; pair n carries object 1 + n % k in a label map.  A lone pixel has a 2 x 2 block of boundary pixels (up and to the left
    of it; less at the frame's edges).  ``foreign`` (label maps): one more predicted pixel of ANOTHER object right beside every predicted
    one - a boundary inside the disk that must not count for the pair's object."""
    gt, pred = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    for n, ((gy, gx), (py, px)) in enumerate(pairs):
        assert gt[gy, gx] == 0 and pred[py, px] == 0
        gt[gy, gx] = pred[py, px] = _value(n, k)
        if foreign and k is not None and px + 1 < W:
            pred[py, px + 1] = _value(n + 1, k)
    return gt, pred


# offsets (dy, dx) of the predicted mark from its ground-truth mark, per radius: the far corner of the ground-truth mark's boundary block
# has its nearest counterpart at exactly this offset, so d^2 = dy^2 + dx^2 - on the circle (= r^2) or one outside it (= r^2 + 1)
CIRCLE_OFFSETS = {1: ((1, 0), (0, 1), (1, 1)), 4: ((4, 0), (0, 4), (4, 1), (1, 4)), 5: ((3, 4), (4, 3), (5, 0), (0, 5), (1, 5), (5, 1))}


def circle_pairs(H, W):
    r = radius(H, W)
    step = 3 * r + 8
    pairs = []
    for n, (dy, dx) in enumerate(CIRCLE_OFFSETS[r] * 2):      # every offset twice: once pred after gt, once gt after pred
        y, x = step * (1 + n // 4), step * (1 + n % 4)
        a, b = (y, x), (y + dy, x + dx)
        pairs.append((a, b) if n < len(CIRCLE_OFFSETS[r]) else (b, a))
    return pairs


def circle_clip(H, W, k=None):
    """(gt, pred) [2,H,W] for a shape whose 0.008 x diagonal is an integer: frame 0 noise (density 0.5 in the top quarter, 0.02 below),
    frame 1 the marks on and just outside the circle."""
    rng = np.random.RandomState(H + W + (0 if k is None else k))
    gt, pred = np.zeros((2, H, W), np.uint8), np.zeros((2, H, W), np.uint8)
    gt[0], pred[0] = _noise_pair(rng, (H, W), 0.02, k)
    gt[0, :H // 4], pred[0, :H // 4] = _noise_pair(rng, (H // 4, W), 0.5, k)
    gt[1], pred[1] = marks(H, W, circle_pairs(H, W), k, foreign=True)
    return gt, pred


def corners_clip(k=None):
    """(gt, pred) [2,60,90], r = 1: frame 0 has a mark in each of the four corner pixels and its counterpart one step inwards (diagonal for
    two corners: d^2 = 2, outside the disk), frame 1 the same with the maps exchanged - every disk is clipped by a corner."""
    H, W = 60, 90
    pairs = [((0, 0), (1, 0)), ((0, W - 1), (1, W - 2)), ((H - 1, 0), (H - 1, 1)), ((H - 1, W - 1), (H - 2, W - 2))]
    g, p = marks(H, W, pairs, k)
    return np.stack([g, p]), np.stack([p, g])


def cap_width() -> int:
    """The widest W of a 2 x W frame whose radius is MAX_RADIUS."""
    W = int(MAX_RADIUS / 0.008)
    while radius(2, W + 1) <= MAX_RADIUS:
        W += 1
    while radius(2, W) > MAX_RADIUS:
        W -= 1
    return W


def cap_row(k=None):
    """One frame 2 x cap_width() at the largest accepted radius r, and its windows.  A pair = a mark in row 0 (boundary pixels in row 0
    only) and one in row 1, r columns further (a 2 x 2 boundary block): the outer pixel of the block in row 0 has its nearest counterpart
    at dx = r, dy = 0 (matched, on the circle), the one in row 1 at dx = r, dy = 1 (d^2 = r^2 + 1: the ONE unmatched pixel of the pair,
    which scans its whole disk).  Pairs at the left edge, at a third, at two thirds (maps exchanged) and at the right edge."""
    r, W = MAX_RADIUS, cap_width()
    xs = (1, W // 3, 2 * W // 3, W - 1 - r)
    pairs = [((0, x), (1, x + r)) for x in xs]
    pairs[2] = (pairs[2][1], pairs[2][0])
    pairs[1] = ((0, xs[1] + r), (1, xs[1]))                   # the block to the LEFT of its counterpart
    pairs[3] = ((0, W - 1), (1, W - 1 - r))                   # the same, the counterpart in the frame's last column
    g, p = marks(2, W, pairs, k)
    boxes = [(0, 2, max(0, x - r - 8), min(W, x + 2 * r + 8)) for x in xs]
    return g, p, boxes


def cap_column(k=None):
    """One frame 125000 x 2, the only column-thin frame at a large radius: here every row of the disk lies inside the frame and costs the
    scan O(r), so an unmatched boundary pixel costs about r^2 loop trips (at MAX_RADIUS: 4e9 in one lane).  The pairs of cap_row, turned."""
    H, W = 125000, 2
    r = radius(H, W)
    ys = (1, H // 3, 2 * H // 3, H - 1 - r)
    pairs = [((y, 0), (y + r, 1)) for y in ys]
    pairs[2] = (pairs[2][1], pairs[2][0])
    pairs[1] = ((ys[1] + r, 0), (ys[1], 1))
    pairs[3] = ((H - 1, 0), (H - 1 - r, 1))
    g, p = marks(H, W, pairs, k)
    boxes = [(max(0, y - r - 8), min(H, y + 2 * r + 8), 0, 2) for y in ys]
    return g, p, boxes


BIG = 4096


def big_frame(k=None):
    """One frame of 2^24 pixels (r = 47) and its windows: a 40 x 40 patch of noise in each corner and in the centre, and beside the centre
    patch two lone pairs at (0, 47) - on the circle - and (47, 1), one outside it."""
    H = W = BIG
    r = radius(H, W)
    rng = np.random.RandomState(24 + (0 if k is None else k))
    gt, pred = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    S, c = 40, H // 2
    for y, x in ((0, 0), (0, W - S), (H - S, 0), (H - S, W - S), (c, c)):
        gt[y:y + S, x:x + S], pred[y:y + S, x:x + S] = _noise_pair(rng, (S, S), 0.1, k)
    lone = [((c + 10, c + 200), (c + 10, c + 200 + r)), ((c + 10, c + 500), (c + 10 + r, c + 501))]
    for n, ((gy, gx), (py, px)) in enumerate(lone):
        gt[gy, gx] = pred[py, px] = _value(n, k)
    m = S + r + 4
    boxes = [(0, m, 0, m), (0, m, W - m, W), (H - m, H, 0, m), (H - m, H, W - m, W), (c - m, c + m, c - m, c + m),
             (c - m, c + 2 * m, c + 200 - m, c + 200 + 2 * m), (c - m, c + 2 * m, c + 500 - m, c + 500 + 2 * m)]
    return gt, pred, boxes


# A clip of more than 2^31 pixels: frame 2048 starts exactly at byte 2^31.  Only these frames have content, a patch each:
LONG = (2050, 1024, 1024)
LONG_FRAMES = {0: (0, 0), 2047: (1024 - 96, 1024 - 96), 2048: (0, 0), 2049: (1024 - 96, 1024 - 96)}       # frame: (y, x) of its 96 x 96 patch


def long_patches(k=None):
    """{frame: (y, x, gt patch, pred patch)}: noise of density 0.5 in the left half of a patch, 0.02 in the right half."""
    rng = np.random.RandomState(31 + (0 if k is None else k))
    out = {}
    for t, (y, x) in LONG_FRAMES.items():
        g, p = _noise_pair(rng, (96, 96), 0.02, k)
        g[:, :48], p[:, :48] = _noise_pair(rng, (96, 48), 0.5, k)
        g[0, 0] = p[0, 0] = g[-1, -1] = p[-1, -1] = 1        # the first and the last pixel of the patch: of the frame, for a corner patch
        out[t] = (y, x, g, p)
    return out


def long_counts(k=None, gen_is_gt=()):
    """int64 [T,6] or [k,T,6] of the long clip: zero but in LONG_FRAMES.  ``gen_is_gt``: frames evaluated with their ground truth."""
    T, H, W = LONG
    r = radius(H, W)
    c = np.zeros((T, 6) if k is None else (k, T, 6), np.int64)
    for t, (y, x, g, p) in long_patches(k).items():
        if t in gen_is_gt:
            p = g
        pad = r + 4                                          # the patch in a window with that margin where the frame goes on
        gw, pw = (np.pad(a, ((0 if y == 0 else pad, pad if y == 0 else 0), (0 if x == 0 else pad, pad if x == 0 else 0))) for a in (g, p))
        if k is None:
            c[t] = frame_counts(gw != 0, pw != 0, r)
        else:
            c[:, t] = np.stack([frame_counts(gw == o, pw == o, r) for o in range(1, k + 1)])
    return c


# ------------------------------------------------------------------------------------------------ scorer sessions
SESSION = dict(T=300, H=3, W=5, nh=16, nw=16, lh=6, lw=5, first=100, ties=((5, 260), (260, 270)))


def session(k=None, seed=0):
    """A two-round session on 3 x 5 frames cropped at (6, 5) out of 16 x 16 planes, T = 300 (the quality kernel's threads take two frames
    each, frames 256 .. 299 in their second trip).  Returns (gt [T,H,W], planes: the engine's [T,1,nh,nw] mask tensor before each of the two
    rounds, annot [T,H,W]: the annotator's imperfect masks of a typed session).
    Frames 0 .. 3 have no object.  Frames 5, 260, 261 and 270 carry the same poor pair of masks, every other frame a prediction that
    misses at most two pixels: round 1 (frame 100 annotated) ties first at 5 and 260, round 2 (100, then 5; the even frames of [0, 100) now
    predicted exactly) at 260 and 270.  261 = 5 + 256 is the second frame of the thread that has frame 5: a tie inside a thread, which has
    to keep its first.  The padding of the planes is garbage."""
    s = SESSION
    T, H, W = s["T"], s["H"], s["W"]
    rng = np.random.RandomState(300 + seed + (0 if k is None else k))
    hi = 2 if k is None else k + 2                           # labels 1 .. k + 1 for a label map
    gt = np.zeros((T, H, W), np.uint8)
    pred = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        g = rng.randint(1, hi, (H, W)).astype(np.uint8) * (rng.rand(H, W) < 0.7)
        g[1, 1:4] = 1 + np.arange(3) % (1 if k is None else k)        # every object is in every frame
        p = g.copy()
        for _ in range(rng.randint(0, 3)):
            p[rng.randint(H), rng.randint(W)] = 0
        p[1, 1:4] = g[1, 1:4]
        gt[t], pred[t] = g, p
    gt[:4] = 0
    poor_g = np.zeros((H, W), np.uint8)
    poor_p = np.zeros((H, W), np.uint8)
    poor_g[0:2, 0:3] = 1 + np.arange(3) % (1 if k is None else k)
    poor_p[1:3, 2:5] = 1 + np.arange(3) % (1 if k is None else k)
    for t in (5, 260, 261, 270):
        gt[t], pred[t] = poor_g, poor_p
    planes = []
    for rnd in range(2):
        if rnd:                                               # what the second round's propagation changes: the even frames of [0, first)
            pred = pred.copy()
            pred[0:s["first"]:2] = gt[0:s["first"]:2]
            pred[0:4, 1, 1] = 1                               # (and something in the frames without an object)
        full = rng.randint(0, 256, (T, 1, s["nh"], s["nw"])).astype(np.uint8)
        full[:, 0, s["lh"]:s["lh"] + H, s["lw"]:s["lw"] + W] = pred
        planes.append(full)
    annot = gt.copy()
    annot[:, 2, 4] = np.where(annot[:, 2, 4] == 0, 1, 0)     # an annotator that gets one pixel wrong
    return gt, planes, annot


def host_round(gt, plane, flags, metric, k=None, annot=None):
    """One round restated on the host: ``flags`` uint8 [T] - 0 = the engine's mask, 1 = ground truth, 2 = the annotator's mask.  Returns
    (gen, counts, per-object quality or None, quality [T], selection): the counts are the yardstick's, the quality the existing
    restatements' (metrics._scores_from_counts; metrics.label_round_quality for label maps), the selection numpy.argmin."""
    s = SESSION
    T, H, W = gt.shape
    seg = plane[:, 0, s["lh"]:s["lh"] + H, s["lw"]:s["lw"] + W]
    seg = (seg != 0).astype(np.uint8) if k is None else np.where(seg > k, 0, seg).astype(np.uint8)
    gtk = gt if k is None else np.where(gt > k, 0, gt).astype(np.uint8)
    f = np.asarray(flags)[:, None, None]
    gen = np.where(f == 2, (annot != 0).astype(np.uint8) if annot is not None else gtk, np.where(f != 0, gtk, seg)).astype(np.uint8)
    if k is not None:
        c = label_counts(gtk, gen, k)
        q, Q, sel = metrics.label_round_quality(gtk, gen, k, metric, NO, counts=c)
        return gen, c, q, Q, sel
    c = counts(gtk, gen)
    Q = metrics._scores_from_counts(c)[:, 0 if metric == "j" else 2].copy()
    Q[gtk.reshape(T, -1).sum(1) == 0] = NO
    return gen, c, None, Q, int(np.argmin(Q))


# ------------------------------------------------------------------------------------------------ the table
WALK_SHAPES = ((300, 2, 2), (41, 2, 3), (7, 5, 7), (3, 3, 341), (3, 32, 32), (3, 25, 41), (5, 2, 512))
LINE_SHAPES = ((5, 1, 70), (5, 70, 1), (3, 1, 1))                                        # J-only, binary
CIRCLE_SHAPES = ((75, 100), (300, 400), (375, 500))                                      # r = 1, 4, 5: 0.008 x diagonal is an integer
THIN_SHAPES = ((2, 2, 1000), (2, 1000, 2), (1, 2, 20000))                                # r = 9, 9, 161: at least one extent below r
FORMS = (None, 3, 9)                                                                     # binary, byte sets, 32-bit sets


@functools.lru_cache(maxsize=None)
def clip(name, k=None):
    """(gt, pred) uint8 [T,H,W] of a named clip, built once; read-only."""
    kind, *shape = name
    if kind == "noise":
        out = noise_clip(*shape, k=k)
    elif kind == "circle":
        out = circle_clip(*shape, k=k)
    elif kind == "corners":
        out = corners_clip(k)
    else:
        raise KeyError(name)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(name, k=None):
    """The yardstick's counts of a named clip, computed once per process: [T,6], or [k,T,6] for label maps."""
    gt, pred = clip(name, k)
    c = counts(gt, pred) if k is None else label_counts(gt, pred, k)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def sparse(name, k=None):
    """(gt, pred, counts) of a one-frame case given with windows: cap_row, cap_column, big_frame."""
    g, p, boxes = {"cap_row": cap_row, "cap_column": cap_column, "big_frame": big_frame}[name](k)
    c = window_counts(g, p, boxes, k)
    for a in (g, p, c):
        a.setflags(write=False)
    return g, p, c
