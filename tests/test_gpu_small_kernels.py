"""GPU: every kernel of elementwise.hip that had no test of its own, one launch each through stcn_test_kernel, against the same operation in
torch on the CPU - exact (torch.equal with the fp32 operation) where the kernel only moves or compares data, else against fp64 with a bound
worked out from the arithmetic.  Every output lies in front of a NaN guard that must survive."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import EPS, aggregate_bound, dev, guard_intact, guarded, kernel, tap_max, torch_aggregate_wbg, up4_prob
from oracle import stcn_oracle as O

pytestmark = pytest.mark.gpu

KG = [(3, 2), (2, 3), (1, 4)]       # batches B = k * G laid out [object][frame]


def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * m for s, m in zip(seed, (1, 131, 10007, 1000003, 7, 77))) + 1)


# ------------------------------------------------------------------------------------------------ maxpool
MAXPOOL = [(H, W, C, B) for (H, W) in [(2, 2), (4, 6), (18, 34), (30, 54)] for C in (4, 64) for B in (1, 3)]


def test_maxpool_sizes_cover_the_walks_of_xcd_contiguous_block():
    """One block, fewer blocks than the 8 XCDs, and block counts that are no multiple of 8 (the r8 != 0 branch)."""
    blocks = sorted({-(-(B * (H // 2) * (W // 2) * (C // 4)) // 256) for H, W, C, B in MAXPOOL})
    assert 1 in blocks and any(1 < b < 8 for b in blocks) and any(b > 8 and b % 8 for b in blocks), blocks


@pytest.mark.parametrize("H,W,C,B", MAXPOOL)
def test_maxpool_equals_max_pool2d_on_negative_inputs(H, W, C, B):
    """All inputs negative: a zero where MaxPool2d pads with -inf would win every border window."""
    x = -torch.rand(B, C, H, W, generator=gen(H, W, C, B)) - 0.01
    ref = F.max_pool2d(x, 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    n = ref.numel()
    y = guarded(n)
    kernel("maxpool3x3s2", [dev(x.permute(0, 2, 3, 1)), y], [B, H, W, C])
    assert guard_intact(y, n)
    assert torch.equal(y[:n].cpu().reshape(ref.shape), ref)


# ------------------------------------------------------------------------------------------------ upsample2x_add
UPS = [(h, w, C, form) for (h, w) in [(1, 1), (1, 5), (3, 2), (7, 9)] for C in (4, 256, 512) for form in ("dense", "broadcast", "frames")]


@pytest.mark.parametrize("h,w,C,form", UPS)
def test_upsample2x_add_matches_interpolate_plus_skip(h, w, C, form):
    """|error| <= 16 * 2^-24 * (|skip| + max |x| of the four taps) per element: four products and four adds in fp32 on weights (0.25, 0.75
    and their products) that are exact.  Skip per batch element, broadcast, or per frame of an [object][frame] batch (slots dense + 96 apart;
    the buffer holds B slots, those beyond G junk, so that a wrong modulo reads wrong data and not outside it)."""
    k, G = KG[(h + w + C // 4 + len(form)) % 3]
    B = k * G
    g = gen(h, w, C, len(form))
    x = torch.randn(B, C, h, w, generator=g)
    dense = 4 * h * w * C
    if form == "dense":
        skip = torch.randn(B, C, 2 * h, 2 * w, generator=g)
        sbuf, sbs, bmod, sk = dev(skip.permute(0, 2, 3, 1)), dense, 0, skip
    elif form == "broadcast":
        skip = torch.randn(1, C, 2 * h, 2 * w, generator=g)
        sbuf, sbs, bmod, sk = dev(skip.permute(0, 2, 3, 1)), 0, 0, skip.expand(B, -1, -1, -1)
    else:
        skip = torch.randn(G, C, 2 * h, 2 * w, generator=g)
        sbs, bmod = dense + 96, G
        buf = torch.full((B, sbs), 1.0e30)
        buf[:G, :dense] = skip.permute(0, 2, 3, 1).reshape(G, dense)
        sbuf, sk = buf.reshape(-1).cuda(), skip[[b % G for b in range(B)]]
    ref = F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False) + sk.double()
    bound = 16 * EPS * (sk.abs().double() + tap_max(x.double(), 0.5))
    n = B * dense
    u = guarded(n)
    kernel("upsample2x_add", [dev(x.permute(0, 2, 3, 1)), sbuf, u], [B, h, w, C, sbs, bmod])
    assert guard_intact(u, n)
    got = u[:n].cpu().reshape(B, 2 * h, 2 * w, C).permute(0, 3, 1, 2).double()
    assert torch.isfinite(got).all()
    excess = ((got - ref).abs() - bound).max().item()
    print(f"B={B} G={G} {form}: max |error| {float((got - ref).abs().max()):.2e}, max (error - bound) {excess:.2e}")
    assert excess <= 0, excess


# ------------------------------------------------------------------------------------------------ decoder tail
# wide: the frames' agg blocks further apart than (k + 1) rows - only at G > 1: a one-frame launch never reads agg_gs.  The launch itself has no
# default for it (0 at G > 1 would lay the frames over each other); the engine's default, (k + 1) * agg_stride, is what the cases that are not wide pass
UP4 = [(k, G, hw, wide) for k in (1, 3, 8, 9, 32) for G in (1, 3) for hw in [(1, 1), (4, 4), (5, 7)] for wide in (False, True) if G > 1 or not wide]


def up4_case(k, G, h4, w4):
    """Seeded logits [k, G, h4, w4] uniform in [-8, 8], the fp64 result [G, k + 1, H, W] and the same formula in torch fp32 on the CPU."""
    logit = torch.rand(k, G, h4, w4, generator=gen(k, G, h4, w4)) * 16 - 8
    ref = torch.stack([torch_aggregate_wbg(up4_prob(logit[:, g].double()), keep_bg=True) for g in range(G)])
    f32 = torch.stack([torch_aggregate_wbg(up4_prob(logit[:, g]), keep_bg=True) for g in range(G)])
    return logit, ref, f32


@functools.lru_cache(maxsize=None)
def fp32_figure(k):
    """The largest error of the formula in torch fp32 on the CPU against fp64 over the cases of k objects: no kernel output enters it."""
    return max(float((f32.double() - ref).abs().max()) for kc, G, (h4, w4), wide in UP4 if kc == k and not wide for _, ref, f32 in [up4_case(k, G, h4, w4)])


@pytest.mark.parametrize("k,G,hw,wide", UP4)
def test_up4_sigmoid_aggregate_matches_the_fp64_formula(k, G, hw, wide):
    """Both instances (8 objects in registers, STCN_MAX_OBJECTS) and the boundary between them; G frames in one launch with the logits laid
    out [object][frame] (obj_stride = G * hw4, logit_gs = hw4); rows of agg further apart than npix, frames further apart than (k + 1) rows
    (wide).  Logits uniform in [-8, 8]: every probability is at least 3e-4 from 0 and 1, no pixel is excluded.

    Bound: the project's 1e-6 (test_aggregate_wbg_matches_the_torch_formula) holds for k = 1 only.  With several objects it is too tight for
    ANY fp32 evaluation on these logits: the formula forms 1 - p from an fp32 sigmoid, and at p = 1 - 3e-4 the 6e-8 rounding of p is 2e-4 of
    1 - p, hence of the odds, which the softmax over the rows spreads to the others.  The same formula in torch fp32 on the CPU against fp64
    (fp32_figure: the worst of the cases of one k) gives 1.9e-7 at k = 1, 2.6e-5 at k = 3, 3.2e-5 at k = 8, 3.8e-5 at k = 9 and 6.3e-5 at
    k = 32, so the bound of a case is max(1e-6, 4 x the figure of its k) - taken from the reference's own fp32 error, never from the kernel's
    output.  Both figures are printed."""
    h4, w4 = hw
    hw4, npix = h4 * w4, 16 * h4 * w4
    logit, ref, f32 = up4_case(k, G, h4, w4)
    stride = npix + 24
    gs = (k + 1) * stride + (40 if wide else 0)
    n = G * gs
    agg = guarded(n)
    kernel("up4_sigmoid_aggregate", [dev(logit), agg], [k, h4, w4, stride, G * hw4 if G > 1 else 0, G, hw4 if G > 1 else 0, gs if G > 1 else 0])
    assert guard_intact(agg, n)
    body = agg[:n].cpu().reshape(G, gs)
    rows = body[:, :(k + 1) * stride].reshape(G, k + 1, stride)
    assert torch.isnan(rows[:, :, npix:]).all() and torch.isnan(body[:, (k + 1) * stride:]).all(), "a gap between rows or frames was written"
    got = rows[:, :, :npix].reshape(G, k + 1, 4 * h4, 4 * w4).double()
    assert torch.isfinite(got).all()
    err, err32, bound = float((got - ref).abs().max()), float((f32.double() - ref).abs().max()), aggregate_bound(fp32_figure(k))
    print(f"k={k} G={G} {h4}x{w4}: kernel {err:.2e}, torch fp32 on the CPU {err32:.2e} (worst of k = {k}: {fp32_figure(k):.2e}), bound {bound:.2e}")
    assert err < bound, (err, bound)


@pytest.mark.parametrize("hw", [(1, 1), (4, 4), (5, 7)])
@pytest.mark.parametrize("k", [1, 3, 8, 9, 32])
def test_up4_sigmoid_matches_the_fp64_formula(k, hw):
    h4, w4 = hw
    npix = 16 * h4 * w4
    logit = torch.rand(k, h4, w4, generator=gen(k, h4, w4, 5)) * 16 - 8
    ref, f32 = up4_prob(logit.double()), up4_prob(logit)
    prob = guarded(k * npix)
    kernel("up4_sigmoid", [dev(logit), prob], [k, h4, w4])
    assert guard_intact(prob, k * npix)
    got = prob[:k * npix].cpu().reshape(k, 4 * h4, 4 * w4).double()
    err, err32 = float((got - ref).abs().max()), float((f32.double() - ref).abs().max())
    print(f"k={k} {h4}x{w4}: kernel {err:.2e}, torch fp32 on the CPU {err32:.2e}")
    assert err < 1e-6, err


@pytest.mark.parametrize("k", [1, 5, 9])
def test_sigmoid_aggregate_matches_the_fp64_formula(k):
    """The fusion tail on 1000 pixels, rows of agg 1024 apart.  Bound as in test_up4_sigmoid_aggregate_matches_the_fp64_formula, for the same
    reason: max(1e-6, 4 x the error of the formula in torch fp32 on the CPU against fp64 on these logits) - 1.2e-7, 7.4e-5 and 7.7e-5 for
    k = 1, 5 and 9; both figures are printed."""
    npix, stride = 1000, 1024
    logit = torch.rand(k, npix, generator=gen(k, 9)) * 16 - 8
    ref = torch_aggregate_wbg(torch.sigmoid(logit.double()), keep_bg=True)
    f32 = torch_aggregate_wbg(torch.sigmoid(logit), keep_bg=True)
    n = (k + 1) * stride
    agg = guarded(n)
    kernel("sigmoid_aggregate", [dev(logit), agg], [k, npix, stride])
    assert guard_intact(agg, n)
    rows = agg[:n].cpu().reshape(k + 1, stride)
    assert torch.isnan(rows[:, npix:]).all(), "a gap between two rows was written"
    err, err32 = float((rows[:, :npix].double() - ref).abs().max()), float((f32.double() - ref).abs().max())
    print(f"k={k}: kernel {err:.2e}, torch fp32 on the CPU {err32:.2e}, bound {aggregate_bound(err32):.2e}")
    assert err < aggregate_bound(err32), (err, err32)


# ------------------------------------------------------------------------------------------------ argmax
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("kk", [2, 6, 33])
def test_argmax_takes_the_first_maximum(kk, T):
    """Values from four levels in the first half of every frame, so most of its pixels have exact ties, and from 4096 levels in the second,
    so every row wins somewhere; the first 40 pixels of every frame have all rows equal.  The fewest ties are at kk = 2: two rows agree on one
    of four levels with probability 1/4, on half the pixels, plus the 40 equal ones - about 0.16 of all pixels; 0.1 is the floor the check of
    the construction holds every kk to."""
    npix = 777
    prob = torch.randint(0, 4096, (kk, T, npix), generator=gen(kk, T)).float() / 4096
    prob[:, :, :npix // 2] = (prob[:, :, :npix // 2] * 4).floor() / 4
    prob[:, :, :40] = 0.5
    masks = guarded(T * npix, torch.uint8)
    kernel("argmax", [dev(prob), masks], [kk, T, npix])
    assert guard_intact(masks, T * npix)
    ref = np.argmax(prob.numpy(), axis=0)
    tied = (prob == prob.amax(0, keepdim=True)).sum(0) > 1
    assert (ref[:, :40] == 0).all() and float(tied.float().mean()) > 0.1 and len(np.unique(ref)) >= min(kk, 20)
    assert np.array_equal(masks[:T * npix].cpu().numpy().reshape(T, npix), ref.astype(np.uint8))


# ------------------------------------------------------------------------------------------------ rowsumsq
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 15, 17, 1620])
def test_rowsumsq_batched_with_strides(n, B):
    """64 squares and 63 adds per row, all terms positive: relative error <= 64 * 2^-24.  Batch elements n * 64 + 128 and n + 7 floats apart;
    the rows beyond n of every output slot stay NaN."""
    C = 64
    x = torch.randn(B, n, C, generator=gen(n, B))
    x_bs, out_bs = n * C + 128, n + 7
    xb = torch.full((B, x_bs), 1.0e30)
    xb[:, :n * C] = x.reshape(B, -1)
    out = guarded(B * out_bs)
    kernel("rowsumsq", [xb.reshape(-1).cuda(), out], [n, C, B, x_bs, out_bs])
    assert guard_intact(out, B * out_bs)
    body = out[:B * out_bs].cpu().reshape(B, out_bs)
    assert torch.isnan(body[:, n:]).all(), "rows beyond n were written"
    ref = (x.double() ** 2).sum(2)
    rel = ((body[:, :n].double() - ref).abs() / ref).max().item()
    assert rel <= 64 * EPS, rel


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("H,W,nh,nw,lh,lw", [(100, 150, 112, 160, 6, 5), (101, 151, 112, 160, 5, 4), (96, 160, 96, 160, 0, 0)])
def test_pack_image_pads_and_interleaves_exactly(H, W, nh, nw, lh, lw):
    img = torch.rand(3, H, W, generator=gen(H, W))
    ref = torch.zeros(nh, nw, 4)
    ref[lh:lh + H, lw:lw + W, :3] = img.permute(1, 2, 0)
    out = guarded(nh * nw * 4)
    kernel("pack_image", [dev(img), out], [H, W, nh, nw, lw, lh])
    assert guard_intact(out, nh * nw * 4)
    got = out[:nh * nw * 4].cpu().reshape(nh, nw, 4)
    assert torch.equal(got, ref) and (got[..., 3] == 0).all()


@pytest.mark.parametrize("k", [1, 3, 32])
def test_pack_value_input_sums_the_other_masks_in_ascending_order(k):
    npix, mstride = 1000, 1040
    g = gen(k, 3)
    img4, masks = torch.rand(npix, 4, generator=g), torch.rand(k, npix, generator=g)
    mb = torch.full((k, mstride), 1.0e30)
    mb[:, :npix] = masks
    ref = torch.zeros(k, npix, 8)
    for i in range(k):
        others = torch.zeros(npix)
        for j in range(k):
            if j != i:
                others = others + masks[j]
        ref[i, :, :3], ref[i, :, 3], ref[i, :, 4] = img4[:, :3], masks[i], others
    out = guarded(k * npix * 8)
    kernel("pack_value_input", [dev(img4), mb.reshape(-1).cuda(), out], [mstride, k, npix])
    assert guard_intact(out, k * npix * 8)
    got = out[:k * npix * 8].cpu().reshape(k, npix, 8)
    assert torch.equal(got, ref) and (got[..., 5:] == 0).all()
    if k == 1:
        assert (got[..., 4] == 0).all()


def test_pack_fusion_input_is_exact():
    npix, nc, nr = 1000, 0.375, 0.8125
    g = gen(12)
    img4, prev, curr, attn = torch.rand(npix, 4, generator=g), torch.rand(npix, generator=g), torch.rand(npix, generator=g), torch.rand(2, npix, generator=g)
    ref = torch.zeros(npix, 12)
    ref[:, :3], ref[:, 3], ref[:, 4], ref[:, 5], ref[:, 6], ref[:, 7], ref[:, 8] = img4[:, :3], prev, curr, attn[0], attn[1], nc, nr
    out = guarded(npix * 12)
    kernel("pack_fusion_input", [dev(img4), dev(prev), dev(curr), dev(attn), out], [npix], [nc, nr])
    assert guard_intact(out, npix * 12)
    assert torch.equal(out[:npix * 12].cpu().reshape(npix, 12), ref)


@pytest.mark.parametrize("H,W,nh,nw,lh,lw", [(20, 30, 32, 32, 6, 1), (32, 32, 32, 32, 0, 0)], ids=["padded", "unpadded"])
@pytest.mark.parametrize("mc", [1, 3])
def test_interact_mask_is_exact(mc, H, W, nh, nw, lh, lw):
    """mc = 1: the mask is broadcast over the kk = 3 rows.  The rows of prob are T * npix apart (frame idx of [kk][T][npix]): the other frames
    must stay as they were."""
    kk, T, idx, npix = 3, 3, 1, nh * nw
    g = gen(mc, H, lh)
    mask, prob = torch.rand(mc, H, W, generator=g), torch.rand(kk, T, npix, generator=g)
    pad = torch.zeros(mc, nh, nw)
    pad[:, lh:lh + H, lw:lw + W] = mask
    m = pad.reshape(mc, npix).expand(kk, npix)
    d = m - prob[:, idx]
    ref_pos, ref_neg = d.clamp(0, 1), (-d).clamp(0, 1)
    ref_prob = prob.clone()
    ref_prob[:, idx] = m
    pd = dev(prob)
    padded, pos, neg = guarded(mc * npix), guarded(kk * npix), guarded(kk * npix)
    kernel("interact_mask", [dev(mask), pd.reshape(-1)[idx * npix:], padded, pos, neg], [mc, H, W, nh, nw, lw, lh, T * npix, kk])
    assert guard_intact(padded, mc * npix) and guard_intact(pos, kk * npix) and guard_intact(neg, kk * npix)
    assert torch.equal(padded[:mc * npix].cpu().reshape(mc, nh, nw), pad)
    assert torch.equal(pos[:kk * npix].cpu().reshape(kk, npix), ref_pos) and torch.equal(neg[:kk * npix].cpu().reshape(kk, npix), ref_neg)
    assert torch.equal(pd.cpu(), ref_prob)


# ------------------------------------------------------------------------------------------------ CBAM
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (6, 7), (30, 54)])
def test_cbam_matches_the_oracle_in_fp64(h, w, B):
    """x + CBAM(x) with random weights: fewer pixels than the 16 pooling slices, frames smaller than the 7x7 window, and 64 channels that are
    negative everywhere (a max pool that starts from 0 would show)."""
    g = gen(h, w, B)
    x = torch.randn(B, 512, h, w, generator=g)
    x[:, :64] = -x[:, :64].abs() - 0.1
    w1, b1 = torch.randn(32, 512, generator=g) / 512 ** 0.5, torch.randn(32, generator=g) * 0.1
    w2, b2 = torch.randn(512, 32, generator=g) / 32 ** 0.5, torch.randn(512, generator=g) * 0.1
    wsp, bsp = torch.randn(1, 2, 7, 7, generator=g) * 0.2, torch.randn(1, generator=g) * 0.1
    fw = {"a.ChannelGate.mlp.1": (w1.double(), b1.double()), "a.ChannelGate.mlp.3": (w2.double(), b2.double()),
          "a.SpatialGate.spatial.conv": (wsp.double(), bsp.double())}
    ref = x.double() + O._cbam(x.double(), fw, "a")
    n = B * h * w * 512
    out = guarded(n)
    kernel("cbam", [dev(x.permute(0, 2, 3, 1)), out, dev(w1), dev(b1), dev(w2), dev(b2), dev(wsp)], [B, h, w], [float(bsp)])
    assert guard_intact(out, n)
    got = out[:n].cpu().reshape(B, h, w, 512).permute(0, 3, 1, 2).double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"B={B} {h}x{w}: max-norm relative error {err:.2e}")
    assert err < 2e-5, err


# ------------------------------------------------------------------------------------------------ copies
def test_copy_rows_with_strides_is_exact():
    rows, n, ss, ds = 5, 77, 100, 90
    src = torch.rand(rows, ss, generator=gen(1))
    dst = guarded(rows * ds)
    kernel("copy_rows", [dev(src), dst], [ss, ds, rows, n])
    assert guard_intact(dst, rows * ds)
    body = dst[:rows * ds].cpu().reshape(rows, ds)
    assert torch.equal(body[:, :n], src[:, :n]) and torch.isnan(body[:, n:]).all()


@pytest.mark.parametrize("na", [0, 4, 1020, 103680])
@pytest.mark.parametrize("nb", [1, 63])
def test_copy2_is_exact(na, nb):
    g = gen(na, nb)
    a, b = torch.rand(max(na, 4), generator=g), torch.rand(nb, generator=g)
    da, db = guarded(na), guarded(nb)
    kernel("copy2", [dev(a), da, dev(b), db], [na, nb])
    assert guard_intact(da, na) and guard_intact(db, nb)
    assert torch.equal(da[:na].cpu(), a[:na]) and torch.equal(db[:nb].cpu(), b)


@pytest.mark.parametrize("n", [1, 1000, 4096 * 256 + 300])
def test_fill_is_exact(n):
    """The last size is more than the 4096 blocks of the launch cover in one pass: the grid-stride loop runs twice."""
    p = guarded(n)
    kernel("fill", [p], [n], [3.25])
    assert guard_intact(p, n) and bool((p[:n] == 3.25).all())
