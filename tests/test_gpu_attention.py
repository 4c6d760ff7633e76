"""GPU: the fusion attention read (area_pool16 -> colmax pass -> attention pass<4, 4|8|12|20> -> finalize -> bilinear x16, memread.hip) at
every launch plan, against oracle.stcn_oracle.attention_read evaluated in fp64, with its two intermediate results in view
(stcn_test_attention_ex).

Shapes: the keys of test_attention_plan.SHAPES, one per regime of attention_plan(hw) - that test pins each shape to its regime.  kk = 2 mask
rows on every shape; kk = 1, 5, 9, 11, 33 (every instance of the pass kernel and the slicing into 20 channels: 20 + 2, 20 + 20 + 20 + 6) on
5x7 (ragged query waves), 30x54 (480p) and 33x63 (three steps per chunk).

Inputs, seeded per case: masks as an interaction leaves them (gpu_util.blob_masks: exact zeros, a few blobs, a faint background on every
second row, one row of pos and one of neg all zero when kk >= 2); keys randn * scale with scale 1, and 0.2 and 3 at 30x54.  At scale 3 a
column of S spreads over more than 100 and one or two rows carry all the weight (the case with the largest error: S itself is large).  At
scale 0.2 the softmax is nearly flat and every row carries weight.  Every operand and every output sits in front of a guard of NaNs, so the rows behind mk / qk
are NaN; the kk = 2 case of every shape passes its own |mk|^2 whose 64 pad floats are NaN (readable, never used).

Bounds.  pooled: 256 * EPS * the block mean (255 adds of non-negative terms and one multiply); zero cells and padded channels are exact.
amap and the final output: gpu_util.aggregate_bound(figure) = max(1e-6, 4 * figure), figure = the error of the same formula in torch fp32
on the CPU against fp64 for this very case (no kernel output enters it); 4 for the kernel's other summation order (per-lane blocks, two
shuffles, up to 16 chunk partials) and expf against torch's exp.

Every multi-step case is shown able to fail, on the host in fp64: dropping the last 64-row step from the softmax and swapping pos with neg
each move the reference by more than 10 bounds, masking one row of the ragged last step by more than one.

Four more cases, kk = 2 at 5x13, 23x45, 30x54 and 45x80, take "matched" keys (host_case): random keys of any scale leave the two best rows of
a column a few units apart, so a column maximum taken over the wrong rows changes nothing that fp32 can show - a build whose pass 2 never
saw the last chunk's maxima passed every random-key case, scale 3 included, and fails these four with NaN.

Measured on an MI355X, max |kernel - fp64| (amap; the output is within 10 % of it unless given) / fp32 figure / bound:
  hw 1, 3, 15, 35, 64, 65 (kk 2)     5.4e-9, 8.6e-8, 1.5e-7, 3.9e-8, 2.6e-7, 1.3e-7 / 3.9e-9 .. 2.2e-7 / 1.0e-6
  hw 1024 (NC 16, spc 1)             1.1e-7 / 2.6e-7 / 1.0e-6
  hw 1035 (spc 2, NCeff 9)           1.6e-7 / 4.3e-7 / 1.7e-6
  hw 1620 (NCeff 13 < NC), kk 2      1.3e-7 / 3.4e-7 / 1.4e-6;  kk 1, 5, 9, 11, 33: 1.3e-7 .. 3.1e-7 / 2.7e-7 .. 5.4e-7 / 1.1e-6 .. 2.1e-6
  hw 2079 (spc 3, NCeff 11), kk 2    1.4e-7 / 1.9e-7 / 1.0e-6;  kk 1, 5, 9, 11, 33: 1.0e-7 .. 2.7e-7 / 1.8e-7 .. 4.8e-7 / 1.0e-6 .. 1.9e-6
  hw 35, kk 1, 5, 9, 11, 33          1.2e-7 .. 3.7e-7 / 5.9e-8 .. 3.5e-7 / 1.0e-6 .. 1.4e-6
  hw 3600 (NC 9, spc 7)              9.8e-8 / 9.2e-8 / 1.0e-6
  hw 8160 (NC 4, spc 32)             8.7e-8 / 3.3e-7 / 1.3e-6 (output: 8.8e-8 / 7.0e-7 / 2.8e-6)
  hw 1620, scale 0.2                 1.9e-8 / 1.3e-7 / 1.0e-6
  hw 1620, scale 3                   3.3e-6 / 2.7e-6 / 1.1e-5 (output: 3.1e-6 / 2.5e-6 / 1.0e-5)
  matched keys, hw 65 .. 3600        5.2e-8 .. 9.4e-8 / 1.7e-7 .. 4.9e-7 / 1.0e-6 .. 1.9e-6 (output: 9.2e-8 .. 1.3e-7)
  pooled: at most 0.02 of its bound everywhere; a constant mask row (kk 33): 1.2e-7 (hw 35), 1.8e-7 (hw 1620) from its constant, bound 1e-6
The figures move with the host (thread count of the fp32 matrix product); the kernel errors do not: every run is bit-identical."""
import pytest
import torch

from gpu_util import EPS, aggregate_bound, attention_stages, blob_masks, call, guard_intact, guarded, stream
from oracle import stcn_oracle as O
from test_attention_plan import SHAPES, restated

pytestmark = pytest.mark.gpu

CASES = [(h, w, 2, 1.0, "randn") for h, w in SHAPES]
CASES += [(h, w, kk, 1.0, "randn") for h, w in ((5, 7), (30, 54), (33, 63)) for kk in (1, 5, 9, 11, 33)]
CASES += [(30, 54, 2, 0.2, "randn"), (30, 54, 2, 3.0, "randn")]
# every query next to one memory row of its own (a frame against its neighbour): see host_case
CASES += [(h, w, 2, 5.0, "matched") for h, w in ((5, 13), (23, 45), (30, 54), (45, 80))]


def nchp_of(nch):
    """attention_nchp: the channel count the pooled rows are padded to"""
    return 4 if nch <= 4 else 8 if nch <= 8 else 12 if nch <= 12 else 20 * -(-nch // 20)


def on_device(t, guard=64):
    """a copy of t in front of a guard of NaNs: (buffer, view of the copy)"""
    buf = guarded(t.numel(), guard=guard)
    buf[:t.numel()] = t.reshape(-1).to("cuda", torch.float32)
    return buf, buf[:t.numel()].view(t.shape)


class Run:
    """one call of stcn_test_attention_ex with every output in front of its own guard"""

    def __init__(self, mk, qk, pos, neg, kk, h, w, msq=None, pooled_in=None):
        hw, self.nchp = h * w, nchp_of(2 * kk)
        self.sizes = dict(pooled=hw * self.nchp, amap=2 * kk * hw, out=2 * kk * 256 * hw)
        self.buf = {n: guarded(s) for n, s in self.sizes.items()}
        call("stcn_test_attention_ex", stream(), mk, qk, pos, neg, kk, 16 * h, 16 * w, msq, pooled_in, self.buf["pooled"], self.buf["amap"], self.buf["out"])
        self.pooled = self.buf["pooled"][:self.sizes["pooled"]].view(hw, self.nchp)
        self.amap = self.buf["amap"][:self.sizes["amap"]].view(2 * kk, hw)
        self.out = self.buf["out"][:self.sizes["out"]].view(kk, 2, 16 * h, 16 * w)

    def written_and_within_bounds(self):
        return all(bool(torch.isfinite(b[:self.sizes[n]]).all()) and guard_intact(b, self.sizes[n]) for n, b in self.buf.items())

    def same_bits(self, other):
        return all(torch.equal(self.buf[n][:s].view(torch.int32), other.buf[n][:s].view(torch.int32)) for n, s in self.sizes.items())


def host_case(h, w, kk, scale, keys):
    """inputs, fp64 references, fp32 figures and bounds of one case; asserts that the case can fail.  No GPU."""
    hw, H, W = h * w, 16 * h, 16 * w
    g = torch.Generator().manual_seed(1000 * hw + 10 * kk + int(10 * scale) % 10 + (keys == "matched"))
    mk, qk = torch.randn(hw, 64, generator=g) * scale, torch.randn(hw, 64, generator=g) * scale
    if keys == "matched":
        # Random keys leave the two best rows of a column a few units apart, however wide the column spreads: with a column maximum taken
        # over the wrong rows the exponentials grow, and their ratio stays right.  Here query q is memory row perm[q] up to 0.05 * randn:
        # that row stands more than 89 > log(FLT_MAX) above every other row, so a chunk whose maxima do not reach pass 2 overflows expf
        # for the queries matched into it - asserted for every chunk of the plan.
        qk = mk[torch.randperm(hw, generator=g)] + 0.05 * torch.randn(hw, 64, generator=g)
        S = O.affinity_logits(mk.double(), qk.double())
        spc, nchunks = restated(hw)[3:]
        chunk = torch.arange(hw) // (64 * spc)
        for c in range(nchunks):
            lead = S[chunk == c].max(0).values - S[chunk != c].max(0).values
            assert lead.max().item() > 89, (c, lead.max().item())
        del S
    zp, zn = (0, kk - 1) if kk >= 2 else (None, None)
    pos, neg = blob_masks(kk, H, W, g, 1, zp), blob_masks(kk, H, W, g, 0, zn)

    # ---- references: fp64, and the same formulas in fp32 for the figures
    ref_out = O.attention_read(mk.double(), qk.double(), pos.double(), neg.double())
    ref_pooled, ref_amap, Wm = attention_stages(mk.double(), qk.double(), pos.double(), neg.double())
    fig_amap = (attention_stages(mk, qk, pos, neg)[1].double() - ref_amap).abs().max().item()
    fig_out = (O.attention_read(mk, qk, pos, neg).double() - ref_out).abs().max().item()
    bound_amap, bound_out = aggregate_bound(fig_amap), aggregate_bound(fig_out)

    # ---- construction: the case can fail (host only).  The read without the rows R of the memory, from the softmax over all rows:
    # (amap - pooled[:, R] @ Wm[R]) / (1 - sum of Wm[R])
    steps = -(-hw // 64)
    if steps > 1:
        without = lambda R: (ref_amap - ref_pooled[:, R] @ Wm[R]) / (1 - Wm[R].sum(0, keepdim=True)).clamp(min=1e-300)     # noqa: E731
        n0 = (steps - 1) * 64
        d_step = (without(slice(n0, hw)) - ref_amap).abs().max().item()
        assert d_step > 10 * bound_amap, (d_step, bound_amap)
        d_row = float("nan")
        if hw % 64:
            row = n0 + int(ref_pooled[:, n0:].abs().sum(0).argmax())             # the row of the ragged step with the most mask
            d_row = (without(slice(row, row + 1)) - ref_amap).abs().max().item()
            assert d_row > bound_amap, (d_row, bound_amap)
        d_swap = (ref_amap.view(kk, 2, hw).flip(1).reshape(2 * kk, hw) - ref_amap).abs().max().item()
        assert d_swap > 10 * bound_amap, (d_swap, bound_amap)
        print(f"h16 x w16 = {h} x {w} kk={kk} scale={scale} {keys} can fail: last step dropped {d_step:.2e}, one row of it masked {d_row:.2e}, pos <-> neg {d_swap:.2e}")
    del Wm
    return dict(mk=mk, qk=qk, pos=pos, neg=neg, zp=zp, zn=zn, ref_out=ref_out, ref_pooled=ref_pooled, ref_amap=ref_amap, fig_amap=fig_amap, fig_out=fig_out,
                bound_amap=bound_amap, bound_out=bound_out)


@pytest.mark.parametrize("h,w,kk,scale,keys", CASES)
def test_attention_read_and_its_stages_match_fp64(h, w, kk, scale, keys):
    c = host_case(h, w, kk, scale, keys)
    hw = h * w
    mk, qk, pos, neg, zp, zn = (c[n] for n in ("mk", "qk", "pos", "neg", "zp", "zn"))
    ref_out, ref_pooled, ref_amap, fig_amap, fig_out, bound_amap, bound_out = (c[n] for n in ("ref_out", "ref_pooled", "ref_amap", "fig_amap", "fig_out", "bound_amap", "bound_out"))

    # ---- the kernels
    (bmk, dmk), (bqk, dqk), (bpos, dpos), (bneg, dneg) = on_device(mk), on_device(qk), on_device(pos), on_device(neg)
    msq = None
    if kk == 2 and scale == 1.0:            # one case per shape: |mk|^2 from the caller, NaN in its 64 pad floats
        msq = guarded(hw)
        msq[:hw] = (dmk * dmk).sum(1)
    first = Run(dmk, dqk, dpos, dneg, kk, h, w, msq)
    assert first.written_and_within_bounds()
    assert all(guard_intact(b, t.numel()) for b, t in ((bmk, mk), (bqk, qk), (bpos, pos), (bneg, neg)))

    pooled = first.pooled.cpu().double()
    assert bool((pooled[:, 2 * kk:] == 0).all())
    err_pooled = (pooled[:, :2 * kk].t() - ref_pooled).abs()
    ratio = (err_pooled / (256 * EPS * ref_pooled).clamp(min=1e-300)).max().item()
    amap, out = first.amap.cpu().double(), first.out.cpu().double()
    err_amap, err_out = (amap - ref_amap).abs().max().item(), (out - ref_out).abs().max().item()
    zeros = (ref_pooled == 0).double().mean().item()
    print(f"h16 x w16 = {h} x {w} (hw {hw}) kk={kk} scale={scale} {keys}: pooled error / bound {ratio:.2f} ({100 * zeros:.0f} % of the cells exact zeros); "
          f"amap kernel error {err_amap:.2e}, fp32 figure {fig_amap:.2e}, bound {bound_amap:.2e}; "
          f"output kernel error {err_out:.2e}, fp32 figure {fig_out:.2e}, bound {bound_out:.2e}")
    assert bool((err_pooled <= 256 * EPS * ref_pooled).all()), ratio
    assert err_amap <= bound_amap, (err_amap, fig_amap, bound_amap)
    assert err_out <= bound_out, (err_out, fig_out, bound_out)
    # all-zero mask rows come out as exact zeros at every stage: nothing leaks between channels, slices, or pos and neg
    if kk >= 2:
        for c in (2 * zp, 2 * zn + 1):
            assert bool((pooled[:, c] == 0).all()) and bool((amap[c] == 0).all()) and bool((out[c // 2, c % 2] == 0).all()), c

    # ---- the path of every later frame of an interaction: pooled reused, no masks; and the fixed summation order
    reuse = Run(dmk, dqk, None, None, kk, h, w, msq, pooled_in=first.pooled)
    assert reuse.written_and_within_bounds() and reuse.same_bits(first)
    again = Run(dmk, dqk, dpos, dneg, kk, h, w, msq)
    assert again.written_and_within_bounds() and again.same_bits(first)


@pytest.mark.parametrize("h,w", [(5, 7), (30, 54)])
def test_a_constant_mask_row_comes_out_as_its_constant(h, w):
    """kk = 33 (four slices of the pass kernel), pos[r] = (r + 1) / 64 and neg[r] = (r + 1) / 64 + 1 / 128 everywhere: a softmax sums to
    one, so output channel (r, 0 | 1) is that constant whatever the keys are - a channel that lands in another slot shows by 1 / 128."""
    kk, hw, H, W = 33, h * w, 16 * h, 16 * w
    g = torch.Generator().manual_seed(hw)
    (bmk, dmk), (bqk, dqk) = on_device(torch.randn(hw, 64, generator=g)), on_device(torch.randn(hw, 64, generator=g))
    const = torch.stack([(torch.arange(kk) + 1) / 64, (torch.arange(kk) + 1) / 64 + 1 / 128], 1).float()        # [kk][2], exact in fp32
    (bpos, dpos), (bneg, dneg) = on_device(const[:, 0].view(kk, 1, 1, 1).expand(kk, 1, H, W)), on_device(const[:, 1].view(kk, 1, 1, 1).expand(kk, 1, H, W))
    run = Run(dmk, dqk, dpos, dneg, kk, h, w)
    assert run.written_and_within_bounds()
    assert torch.equal(run.pooled[:, :2 * kk].cpu(), const.reshape(1, 2 * kk).expand(hw, 2 * kk))              # 256 equal dyadic values sum exactly
    err = (run.out.cpu().double() - const.double().view(kk, 2, 1, 1)).abs().amax((2, 3))
    print(f"h16 x w16 = {h} x {w} kk=33: largest distance of a channel from its constant {err.max().item():.2e}")
    assert err.max().item() <= 1e-6, err
