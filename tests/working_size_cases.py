"""Shared by test_working_size_api.py (CPU) and test_gpu_working_size.py: the cases of the working-resolution kernels and float64 NumPy
restatements of the two definitions - antialiased bicubic resampling (tap tables and the resample) and bilinear interpolation plus first-max
arg-max.  The CPU file pins the restatements to torch's CPU operators in float64; the GPU file holds the kernels to the restatements."""
import numpy as np
import torch
import torch.nn.functional as F

# (k, (h, w) window of the probabilities, (H, W) own size); the window sits in its 16-padded plane as InferenceCore pads it
UP_CASES = [
    (1, (96, 109), (203, 231)),
    (3, (96, 109), (203, 231)),
    (1, (109, 96), (231, 203)),          # portrait
    (5, (120, 213), (270, 480)),
    (32, (48, 57), (101, 120)),
    (1, (96, 125), (100, 131)),          # a scale barely above 1
    (2, (96, 120), (800, 1000)),         # a scale of 8.3
]
# ((H, W) -> (h, w), planes): N(0,1) data; 800 x 1000 -> 96 x 120 has 35 taps per axis
DOWN_CASES = [
    ((203, 231), (96, 109), 3),
    ((231, 203), (109, 96), 3),
    ((100, 131), (96, 125), 3),
    ((800, 1000), (96, 120), 3),
    ((1080, 1920), (480, 853), 6),       # two frames
    ((203, 231), (96, 109), 1),
    ((203, 231), (96, 109), 9),
]
EXCLUDED_SHARE = 2e-4                    # pixels of a case whose float64 top-2 gap is below eps: a condition on the case, not a measurement


def pad16(n):
    d = (-n) % 16
    return d // 2, d - d // 2


def pad_of(hw):
    """(lw, uw, lh, uh) as InferenceCore.pad."""
    (lh, uh), (lw, uw) = pad16(hw[0]), pad16(hw[1])
    return lw, uw, lh, uh


def probs(seed, k, h, w):
    """fp32 [k+1,h,w]: seeded low-resolution normal logits x 4, bicubic to h x w, softmax over the channels, clamped as the engine's are."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(1, k + 1, h // 8 + 2, w // 8 + 2, generator=g) * 4
    lg = F.interpolate(lo, size=(h, w), mode="bicubic", align_corners=False)[0]
    return torch.softmax(lg, 0).clamp(1e-7, 1 - 1e-7)


def padded(windows, hw):
    """windows: list of T tensors [k+1,h,w] -> fp32 [k+1,T,1,nh,nw] with the windows at (lh, lw) and NaN in every padded row and column."""
    lw, uw, lh, uh = pad_of(hw)
    k1 = windows[0].shape[0]
    out = torch.full((k1, len(windows), 1, hw[0] + lh + uh, hw[1] + lw + uw), float("nan"), dtype=torch.float32)
    for t, win in enumerate(windows):
        out[:, t, 0, lh:lh + hw[0], lw:lw + hw[1]] = win
    return out


# ------------------------------------------------------------------------------------------------ antialiased bicubic, float64
def cubic(x, a=-0.5):
    x = np.abs(x)
    return np.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1, np.where(x < 2, (((x - 5) * x + 8) * x - 4) * a, 0.0))


def aa_taps(n_in, n_out):
    """(first [out] int64, count [out] int64, weight [out,taps] float64) of one axis: the support is 2 * scale source pixels to either side
    of the output's centre (2 when enlarging), the weights are those of Keys' cubic at A = -0.5 on distances divided by the scale, normalised
    over the taps inside the image; taps = 2 * ceil(support) + 1."""
    scale = n_in / n_out
    support, inv = (2.0 * scale, 1.0 / scale) if scale >= 1 else (2.0, 1.0)
    taps = int(np.ceil(support)) * 2 + 1
    center = scale * (np.arange(n_out) + 0.5)
    first = np.maximum((center - support + 0.5).astype(np.int64), 0)              # truncation, as a C cast
    count = np.clip(np.minimum((center + support + 0.5).astype(np.int64), n_in) - first, 1, taps)
    j = np.arange(taps)
    wt = np.where(j[None] < count[:, None], cubic((j[None] + first[:, None] - center[:, None] + 0.5) * inv), 0.0)
    return first, count, wt / wt.sum(1, keepdims=True)


def resample_axis(x, n_out, axis):
    first, count, wt = aa_taps(x.shape[axis], n_out)
    x = np.moveaxis(x, axis, -1)
    out = np.zeros(x.shape[:-1] + (n_out,), np.float64)
    for j in range(wt.shape[1]):
        out += x[..., np.minimum(first + j, x.shape[-1] - 1)] * wt[:, j]           # weights behind `count` are zero
    return np.moveaxis(out, -1, axis)


def downsample_aa_ref(x, hw):
    """x [...,H,W] -> float64 [...,h,w]: horizontal, then vertical."""
    return resample_axis(resample_axis(np.asarray(x, np.float64), hw[1], -1), hw[0], -2)


# ------------------------------------------------------------------------------------------------ bilinear + first-max arg-max, float64
def bilinear_matrix(n_in, n_out):
    """float64 [out,in]: src = (dst + 0.5) * in / out - 0.5, clamped below at 0, i1 = min(i0 + 1, in - 1)."""
    src = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    lam = src - i0
    m = np.zeros((n_out, n_in), np.float64)
    np.add.at(m, (np.arange(n_out), i0), 1.0 - lam)
    np.add.at(m, (np.arange(n_out), i1), lam)
    return m


def upsample_ref(win, HW, rows=None):
    """win [k+1,h,w] -> float64 [k+1,H,W] (``rows``: only these output rows)."""
    win = np.asarray(win, np.float64)
    my, mx = bilinear_matrix(win.shape[1], HW[0]), bilinear_matrix(win.shape[2], HW[1])
    if rows is not None:
        my = my[rows]
    return np.einsum("yh,chw,xw->cyx", my, win, mx, optimize=True)


def argmax_ref(up):
    """(uint8 mask, float64 top-2 gap) of float64 [k+1,H,W]; np.argmax keeps the first maximum."""
    top = np.sort(up, 0)
    return up.argmax(0).astype(np.uint8), top[-1] - top[-2]


def fp32_eps(win, HW):
    """4 x the largest |torch CPU fp32 interpolation - float64| on this very input: 2 for the two competing values times 2 for another legal
    fp32 evaluation order."""
    win = torch.as_tensor(win, dtype=torch.float32)
    a32 = F.interpolate(win[None], size=tuple(HW), mode="bilinear", align_corners=False)
    a64 = F.interpolate(win[None].double(), size=tuple(HW), mode="bilinear", align_corners=False)
    return 4.0 * float((a32.double() - a64).abs().max())


def check_masks(got, win, HW, eps=None, rows=None, what=""):
    """``got`` uint8 [H,W] (or the ``rows`` of it) against the restatement on ``win``: equal except where the float64 top-2 gap is below eps,
    and such pixels are at most EXCLUDED_SHARE of the case.  Returns (differing pixels, excluded pixels).
    A channel whose plane repeats a lower channel's bit for bit (a one-object core stores the annotation of an interacted frame in both of its
    channels, as the reference's broadcast does) is an EXACT tie with it at every pixel in any evaluation order: the tie rule says it never
    wins, so it is left out of the gap - and out of the labels ``got`` may hold."""
    eps = fp32_eps(win, HW) if eps is None else eps
    win = np.asarray(win)
    first = np.array([c for c in range(len(win)) if not any(np.array_equal(win[c], win[d]) for d in range(c))])
    up = upsample_ref(win[first], HW, rows)
    if len(first) > 1:
        ref, gap = argmax_ref(up)
        ref = first[ref].astype(np.uint8)
    else:
        ref, gap = np.full(up.shape[1:], first[0], np.uint8), np.full(up.shape[1:], np.inf)
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.uint8, (what, got.shape, ref.shape)
    close = gap < eps
    assert close.mean() <= EXCLUDED_SHARE, (what, "excluded share", float(close.mean()), eps)
    bad = (got != ref) & ~close
    assert not bad.any(), (what, int(bad.sum()), "pixels differ where the float64 gap is at least", eps, np.argwhere(bad)[:4].tolist())
    return int((got != ref).sum()), int(close.sum())
