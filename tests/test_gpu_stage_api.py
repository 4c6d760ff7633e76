"""GPU: the reference's stage interface on the HIP kernels - PropagationNetwork.encode_key / encode_value / segment_with_query /
get_attention, FusionNet.forward, aggregate_wbg - in the reference's NCHW shapes: the layout conversion alone (exact), every stage against
the oracle and the reference goldens (fixtures and tolerances of test_gpu_stages.py), and a frame-by-frame loop on the six public calls
against the sequence goldens."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_err, sample_of
from eva_vos_amd import _lib, synth
from eva_vos_amd.params import PropagationNetwork
from gpu_util import aggregate_bound, blob_masks, torch_aggregate_wbg
from oracle import stcn_oracle as O
from test_oracle_golden import check_sequence_against_golden, run_sequence

pytestmark = pytest.mark.gpu
STAGE = {"stA": (128, 160, 1), "stB": (100, 150, 3), "stC": (96, 208, 2)}
KEY_NAMES = ["k16", "f16_thin", "f16", "f8", "f4"]


# ------------------------------------------------------------------------------------------------ 1. the layout conversion
def transpose(src, dst, B, R, Cc, ld, planes_bs, to_rows):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().stcn_test_transpose(s, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), B, R, Cc, ld, planes_bs, to_rows), "stcn_test_transpose")


@pytest.mark.parametrize("B", [1, 3])
def test_transposes_are_exact(B):
    """Both directions for row counts around the 64-row tile (1, 63, 64, 65, 70 = the keys of stB, 1120) x channel counts 4 .. 1024.  The
    output sits in front of a guard of NaNs that must stay NaNs: nothing is written past a ragged edge."""
    g = torch.Generator(device="cuda").manual_seed(3)
    for R in (1, 63, 64, 65, 70, 1120):
        for Cc in (4, 64, 256, 1024):
            x = torch.randn(B, Cc, R, device="cuda", generator=g)
            want = x.transpose(-1, -2).contiguous()
            for src, ref, to_rows in ((x, want, 1), (want, x, 0)):
                buf = torch.full((B * R * Cc + 64,), float("nan"), device="cuda")
                transpose(src, buf, B, R, Cc, R, Cc * R, to_rows)
                assert torch.equal(buf[:B * R * Cc].view(ref.shape), ref), (B, R, Cc, to_rows)
                assert bool(torch.isnan(buf[B * R * Cc:]).all()), (B, R, Cc, to_rows)


@pytest.mark.parametrize("t0", [0, 1])
def test_transposes_read_and_write_a_t_slice_in_place(t0):
    """keys[:, :, :m_front] of a preallocated [1,64,5,7,10] bank (inference_core.py:150-170): channel planes 350 floats apart, 140 of them
    read - no plane after the first starts on a 16-byte boundary; the slice [1:3] does not start on one either."""
    g = torch.Generator(device="cuda").manual_seed(4)
    bank = torch.randn(1, 64, 5, 7, 10, device="cuda", generator=g)
    sl = bank[:, :, t0:t0 + 2]
    want = sl.reshape(1, 64, 140).transpose(-1, -2).contiguous()
    rows = torch.empty(1, 140, 64, device="cuda")
    transpose(sl, rows, 1, 140, 64, 350, 0, 1)
    assert torch.equal(rows, want)
    back = torch.full_like(bank, -7.0)
    transpose(rows, back[:, :, t0:t0 + 2], 1, 140, 64, 350, 0, 0)
    assert torch.equal(back[:, :, t0:t0 + 2], sl)
    keep = torch.ones(5, dtype=torch.bool, device="cuda")
    keep[t0:t0 + 2] = False
    assert bool((back[:, :, keep] == -7.0).all())


# ------------------------------------------------------------------------------------------------ 2. stage parity
_ORACLE = {}


def oracle_stages(tag, weights):
    """The oracle's stages of a fixture, computed once per session and left unchanged: key features of frames 0 and 2, the value of frame
    0, the read of frame 2 from that one-frame memory and its decoded probabilities."""
    if tag not in _ORACLE:
        H, W, k = STAGE[tag]
        fw = O.fold_bn(weights[0])
        imgs, _ = O.pad16(synth.synthetic_clip(3, H, W))
        m0, _ = O.pad16(synth.synthetic_mask(3, H, W, k)[:, 0])
        kf0, kf2 = O.encode_key(fw, imgs[:, 0]), O.encode_key(fw, imgs[:, 2])
        v0 = O.encode_value(fw, imgs[:, 0], kf0[2], m0)
        h, w = kf0[0].shape[-2:]
        rows = lambda x: x.flatten(2).transpose(1, 2).contiguous()      # noqa: E731
        _, _, ro = O.memory_read(rows(kf0[0])[0], rows(v0), rows(kf2[0])[0])
        prob, _ = O.decode(fw, ro.transpose(1, 2).reshape(k, 512, h, w), kf2[1], kf2[3], kf2[4])
        _ORACLE[tag] = dict(imgs=imgs, m0=m0, kf0=kf0, kf2=kf2, v0=v0, prob=prob, k=k)
    return _ORACLE[tag]


@pytest.mark.parametrize("tag", list(STAGE))
def test_encode_key_and_encode_value_match_the_oracle_and_the_goldens(tag, nets, weights):
    o, g = oracle_stages(tag, weights), load_golden(tag)
    k, nh, nw = o["k"], *o["imgs"].shape[-2:]
    kf = nets[0].encode_key(o["imgs"][:, 0].cuda())
    assert [tuple(t.shape) for t in kf] == [tuple(t.shape) for t in o["kf0"]] and not any(t.requires_grad for t in kf)
    for n, a, b in zip(KEY_NAMES, kf, o["kf0"]):
        e1, e2 = rel_err(a.cpu().numpy(), b.numpy()), rel_err(sample_of(a, 1 if n == "k16" else 37), g[f"{tag}.key0.{n}.sample"])
        print(f"{tag} encode_key {n}: rel err vs oracle {e1:.2e}, vs golden {e2:.2e}")
        assert e1 < 2e-5 and e2 < 2e-5, n
    v = nets[0].encode_value(o["imgs"][:, 0].cuda(), kf[2], o["m0"].cuda())
    assert tuple(v.shape) == (k, 512, 1, nh // 16, nw // 16)
    e1, e2 = rel_err(v[:, :, 0].cpu().numpy(), o["v0"].numpy()), rel_err(sample_of(v[:, :, 0], 11), g[f"{tag}.value0.sample"])
    print(f"{tag} encode_value: rel err vs oracle {e1:.2e}, vs golden {e2:.2e}")
    assert e1 < 3e-5 and e2 < 3e-5


@pytest.mark.parametrize("tag", list(STAGE))
def test_fusion_net_is_callable_and_matches_the_oracle_and_the_golden(tag, nets, weights):
    """The inputs of test_gpu_stages.py::test_fusion_net; `time` once as the CPU tensor of inference_core.py:201 and once on the device."""
    H, W, _ = STAGE[tag]
    g = load_golden(tag)
    imgs, _ = O.pad16(synth.synthetic_clip(2, H, W))
    rng = np.random.Generator(np.random.Philox(key=[7, 7]))
    nh, nw = imgs.shape[-2:]
    prev = torch.from_numpy(rng.uniform(0, 1, (1, 1, nh, nw)).astype(np.float32))
    curr = torch.from_numpy(rng.uniform(0, 1, (1, 1, nh, nw)).astype(np.float32))
    attn = torch.from_numpy(rng.uniform(0, 0.2, (1, 2, nh, nw)).astype(np.float32))
    ref = O.fusion_net(O.fold_bn(weights[1]), imgs[:, 1], prev, curr, attn, 0.25, 0.75)
    time = torch.FloatTensor([0.25, 0.75]).unsqueeze(0)
    out = nets[1](imgs[:, 1].cuda(), prev.cuda(), curr.cuda(), attn.cuda(), time)
    assert tuple(out.shape) == (1, 1, nh, nw) and not out.requires_grad
    d1, d2 = float((out.cpu() - ref).abs().max()), float(np.abs(sample_of(out, 13) - g[f"{tag}.fusion_logit.sample"]).max())
    print(f"{tag} FusionNet: max |d| vs oracle {d1:.2e}, vs golden {d2:.2e}")
    assert d1 < 2e-4 and d2 < 2e-4
    assert torch.equal(nets[1](imgs[:, 1].cuda(), prev.cuda(), curr.cuda(), attn.cuda(), time.cuda()), out)


@pytest.mark.parametrize("tag", list(STAGE))
def test_get_attention_matches_the_oracle(tag, nets, weights):
    """Oracle and tolerance of test_gpu_kernels.py::test_attention_read_matches_oracle (1e-5), on the fixture's own keys: frame 0 as the
    memory, frame 2 as the query, k + 1 mask planes."""
    o = oracle_stages(tag, weights)
    m0 = o["m0"]
    pos = torch.cat([torch.full_like(m0[:1], 0.1), (m0 - 0.3).clamp(0, 1)], 0)
    neg = torch.cat([torch.full_like(m0[:1], 0.2), (0.3 - m0).clamp(0, 1)], 0)
    rows = lambda x: x.flatten(2).transpose(1, 2)[0]      # noqa: E731
    ref = O.attention_read(rows(o["kf0"][0]), rows(o["kf2"][0]), pos, neg)
    out = nets[0].get_attention(o["kf0"][0].unsqueeze(2).cuda(), pos.cuda(), neg.cuda(), o["kf2"][0].cuda())
    assert tuple(out.shape) == tuple(ref.shape)
    d = float((out.cpu() - ref).abs().max())
    print(f"{tag} get_attention: max |d| vs oracle {d:.2e}")
    assert d < 1e-5


@pytest.mark.parametrize("nh,nw", [(16, 16), (16, 48)])
def test_get_attention_on_the_smallest_frames(nh, nw, nets):
    """One and three 1/16-scale positions (a softmax over one row; one source row for the x16 upsample), b = 2 mask planes, random keys:
    against the oracle in fp64, within gpu_util.aggregate_bound of the error of the oracle in fp32 (reference and bound of
    test_gpu_attention.py)."""
    h, w = nh // 16, nw // 16
    g = torch.Generator().manual_seed(nh * nw)
    mk, qk = torch.randn(1, 64, h, w, generator=g), torch.randn(1, 64, h, w, generator=g)
    pos, neg = blob_masks(2, nh, nw, g, 1), blob_masks(2, nh, nw, g, 0)
    rows = lambda x: x.flatten(2).transpose(1, 2)[0]      # noqa: E731
    ref = O.attention_read(rows(mk).double(), rows(qk).double(), pos.double(), neg.double())
    figure = float((O.attention_read(rows(mk), rows(qk), pos, neg).double() - ref).abs().max())
    out = nets[0].get_attention(mk.unsqueeze(2).cuda(), pos.cuda(), neg.cuda(), qk.cuda())
    assert tuple(out.shape) == (2, 2, nh, nw) and bool(torch.isfinite(out).all())
    d = float((out.cpu().double() - ref).abs().max())
    print(f"get_attention {nh} x {nw}: max |d| vs fp64 {d:.2e}, fp32 figure {figure:.2e}, bound {aggregate_bound(figure):.2e}")
    assert d <= aggregate_bound(figure)


@pytest.mark.parametrize("k", [1, 3, 32])
@pytest.mark.parametrize("keep_bg", [False, True])
def test_aggregate_wbg_matches_the_torch_formula(k, keep_bg):
    """1e-6 on every pixel whose inputs are all at least 1e-6 away from 0 and 1.  The formula is evaluated in fp64 on the same fp32 inputs:
    evaluated in fp32 it carries 6e-7 of its own at k = 32 (its logits reach 16, where one ulp of the logarithm is 2e-6 in the odds) - more
    than half the bound.  The fp32 figure is printed."""
    from mivos.model.aggregate import aggregate_wbg
    g = torch.Generator(device="cuda").manual_seed(10 + k)
    p = torch.rand(k, 1, 97, 131, device="cuda", generator=g)
    p[:, 0, 0, :8] = torch.tensor([0.0, 1.0, 1e-7, 1 - 1e-7, 5e-7, 1 - 5e-7, 0.0, 1.0], device="cuda")      # excluded pixels still have to come out finite
    out = aggregate_wbg(p, keep_bg=keep_bg)
    assert tuple(out.shape) == (k + 1 if keep_bg else k, 1, 97, 131) and bool(torch.isfinite(out).all())
    ok = ((p > 1e-6) & (p < 1 - 1e-6)).all(0, keepdim=True).expand_as(out)
    assert float(ok.float().mean()) > 0.99
    d64 = float((out.double() - torch_aggregate_wbg(p.double(), keep_bg))[ok].abs().max())
    d32 = float((out - torch_aggregate_wbg(p, keep_bg))[ok].abs().max())
    print(f"aggregate_wbg k={k} keep_bg={keep_bg}: max |d| vs the formula in fp64 {d64:.2e}, in fp32 {d32:.2e}")
    assert d64 < 1e-6


def test_aggregate_wbg_hard_is_one_hot_where_the_formula_is():
    """hard=True (logits x 1000): wherever the two largest logits of the torch formula lie at least 0.1 apart the softmax is one-hot to
    fp32 (exp(-100) = 0) - same winner, ones and zeros."""
    from mivos.model.aggregate import aggregate_wbg
    p = torch.rand(3, 1, 64, 80, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    out, ref = aggregate_wbg(p, keep_bg=True, hard=True), torch_aggregate_wbg(p.double(), True, True)
    soft = torch.log(torch_aggregate_wbg(p.double(), True))
    top2 = soft.topk(2, dim=0).values
    clear = ((top2[0] - top2[1]) >= 0.1).expand_as(out)
    assert float(clear.float().mean()) > 0.5
    assert float((out.double() - ref)[clear].abs().max()) < 1e-6
    assert torch.equal(aggregate_wbg(p, keep_bg=False, hard=True), out[1:])


# ------------------------------------------------------------------------------------------------ 3. segment_with_query
_CONTAINERS = {}


def _container(weights, **hyper):
    """A PropagationNetwork(**hyper) with the recipe weights, one per hyper-parameter set and session (each is its own folded model)."""
    key = tuple(sorted(hyper.items()))
    if key not in _CONTAINERS:
        p = PropagationNetwork(**hyper)
        p.load_state_dict(weights[0], strict=True)
        _CONTAINERS[key] = p.eval()
    return _CONTAINERS[key]


def segment_inputs(o):
    kf0, kf2 = o["kf0"], o["kf2"]
    return dict(mk16=kf0[0].unsqueeze(2).cuda(), mv16=o["v0"].unsqueeze(2).cuda(), qf8=kf2[3].cuda(), qf4=kf2[4].cuda(), qk16=kf2[0].cuda(), qv16=kf2[1].cuda())


@pytest.mark.parametrize("tag", list(STAGE))
def test_segment_with_query_matches_the_oracle(tag, nets, weights):
    """Memory = the oracle's key and value of frame 0, query = its features of frame 2 (the isolation of test_stage_graphs); the statement
    of that test's decode check on the probabilities: p99.9 < 1e-3 (saturated multi-object pixels are ill-conditioned), max < 1e-3 at k = 1."""
    o = oracle_stages(tag, weights)
    k, a = o["k"], segment_inputs(oracle_stages(tag, weights))
    net = nets[0]
    prob = net.segment_with_query(**a)
    assert tuple(prob.shape) == tuple(o["prob"].shape) and not prob.requires_grad
    d = (prob.cpu() - o["prob"]).abs().numpy()
    print(f"{tag} segment_with_query: |dprob| p99.9 {np.quantile(d, 0.999):.2e} max {d.max():.2e}")
    assert np.quantile(d, 0.999) < 1e-3
    if k == 1:
        assert d.max() < 1e-3
    # the bank as T-slices of larger preallocated tensors (inference_core.py:150-170): read in place, the same bits
    h, w = a["qk16"].shape[-2:]
    keys, values = torch.full((1, 64, 5, h, w), float("nan"), device="cuda"), torch.full((k, 512, 5, h, w), float("nan"), device="cuda")
    keys[:, :, :1], values[:, :, :1] = a["mk16"], a["mv16"]
    sl = dict(a, mk16=keys[:, :, :1], mv16=values[:, :, :1])
    assert not sl["mk16"].is_contiguous() and sl["mk16"].data_ptr() == keys.data_ptr()
    assert torch.equal(net.segment_with_query(**sl), prob)
    # the model's hyper-parameters apply: another top_k and the kernelized read give other probabilities
    for hyper in (dict(top_k=20), dict(km=5.6)):
        other = _container(weights, **hyper).segment_with_query(**a)
        assert bool(torch.isfinite(other).all()) and not torch.equal(other, prob), hyper
    assert torch.equal(net.segment_with_query(**a), prob)           # ... and the default container still reads with its own


def test_segment_with_query_refuses_a_memory_smaller_than_top_k(nets):
    z = lambda *s: torch.zeros(*s, device="cuda")      # noqa: E731
    with pytest.raises((ValueError, RuntimeError), match="top_k"):
        nets[0].segment_with_query(z(1, 64, 3, 2, 2), z(1, 512, 3, 2, 2), z(1, 512, 4, 4), z(1, 256, 8, 8), z(1, 64, 2, 2), z(1, 512, 2, 2))


# ------------------------------------------------------------------------------------------------ 4. a loop on the public methods
class StageLoopCore:
    """mivos/inference_core.py:34-99 and :126-259 of the reference restated on the six public calls (encode_key, encode_value,
    segment_with_query, get_attention, FusionNet.__call__, aggregate_wbg), frame by frame, with the surface run_sequence drives."""

    def __init__(self, prop_net, fuse_net, images, num_objects, mem_freq=5):
        from mivos.model.aggregate import aggregate_wbg
        self.aggregate_wbg = aggregate_wbg
        self.prop_net, self.fuse_net, self.mem_freq, self.k = prop_net, fuse_net, mem_freq, num_objects
        self.t = images.shape[1]
        images, self.pad = O.pad16(images.float())
        self.images = images.cuda()
        self.nh, self.nw = images.shape[-2:]
        self.prob = torch.zeros((self.k + 1, self.t, 1, self.nh, self.nw), device="cuda")
        self.prob[0] = 1e-7
        self.masks = torch.zeros((self.t, 1, self.nh, self.nw), dtype=torch.uint8, device="cuda")
        self.interacted, self.key_buf = set(), {}
        self.certain_mem_k = self.certain_mem_v = None

    def key_feat(self, idx):
        if idx not in self.key_buf:
            self.key_buf[idx] = self.prop_net.encode_key(self.images[:, idx])
        return self.key_buf[idx]

    def do_pass(self, key_k, key_v, idx, forward=True):
        m_front = num_certain = self.certain_mem_k.shape[2]
        if forward:
            closest_ti = min([ti for ti in self.interacted if ti > idx] + [self.t])
            total_m = (closest_ti - idx - 1) // self.mem_freq + 1 + num_certain
            this_range, end = range(idx + 1, closest_ti), closest_ti - 1
        else:
            closest_ti = max([ti for ti in self.interacted if ti < idx] + [-1])
            total_m = (idx - closest_ti - 1) // self.mem_freq + 1 + num_certain
            this_range, end = range(idx - 1, closest_ti, -1), closest_ti + 1
        _, CK, _, H, W = key_k.shape
        K, CV = key_v.shape[:2]
        keys = torch.empty((1, CK, total_m, H, W), device="cuda")
        values = torch.empty((K, CV, total_m, H, W), device="cuda")
        keys[:, :, :num_certain], values[:, :, :num_certain] = self.certain_mem_k, self.certain_mem_v
        last_ti = idx
        for ti in this_range:
            k16, qv16, qf16, qf8, qf4 = self.key_feat(ti)
            out_mask = self.prop_net.segment_with_query(keys[:, :, :m_front], values[:, :, :m_front], qf8, qf4, k16, qv16)
            out_mask = self.aggregate_wbg(out_mask, keep_bg=True)
            if ti != end and abs(ti - last_ti) >= self.mem_freq:
                keys[:, :, m_front:m_front + 1] = k16.unsqueeze(2)
                values[:, :, m_front:m_front + 1] = self.prop_net.encode_value(self.images[:, ti], qf16, out_mask[1:])
                m_front += 1
                last_ti = ti
            if closest_ti != self.t and closest_ti != -1:
                self.prob[:, ti] = self.fuse_one_frame(closest_ti, idx, ti, self.prob[:, ti], out_mask, key_k, k16)
            else:
                self.prob[:, ti] = out_mask

    def fuse_one_frame(self, tc, tr, ti, prev_mask, curr_mask, mk16, qk16):
        prob = torch.zeros((self.k, 1, self.nh, self.nw), device="cuda")
        dist = torch.FloatTensor([abs(tc - ti) / abs(tc - tr), abs(tr - ti) / abs(tc - tr)]).unsqueeze(0)
        attn_map = self.prop_net.get_attention(mk16, self.pos_mask_diff, self.neg_mask_diff, qk16)
        for k in range(1, self.k + 1):
            prob[k - 1] = torch.sigmoid(self.fuse_net(self.images[:, ti], prev_mask[k:k + 1], curr_mask[k:k + 1], attn_map[k:k + 1], dist))[0]
        return self.aggregate_wbg(prob, keep_bg=True)

    def interact(self, mask, idx, scribble=False):
        self.interacted.add(idx)
        mask = F.pad(mask.float().cuda(), self.pad)
        mask_diff = mask - self.prob[:, idx]
        self.pos_mask_diff, self.neg_mask_diff = mask_diff.clamp(0, 1), (-mask_diff).clamp(0, 1)
        self.prob[:, idx] = mask
        key_k, _, qf16, _, _ = self.key_feat(idx)
        key_k = key_k.unsqueeze(2)
        key_v = self.prop_net.encode_value(self.images[:, idx], qf16, mask[1:] if scribble else mask)
        if self.certain_mem_k is None:
            self.certain_mem_k, self.certain_mem_v = key_k, key_v
        else:
            self.certain_mem_k, self.certain_mem_v = torch.cat([self.certain_mem_k, key_k], 2), torch.cat([self.certain_mem_v, key_v], 2)
        self.do_pass(key_k, key_v, idx, True)
        self.do_pass(key_k, key_v, idx, False)
        self.masks[:] = torch.argmax(self.prob, dim=0)
        lw, uw, lh, uh = self.pad
        self.np_masks = self.masks[:, 0, lh:self.nh - uh, lw:self.nw - uw].cpu().numpy().astype(np.uint8)
        return self.np_masks


@pytest.mark.parametrize("tag", ["seqA", "seqC"])
def test_a_loop_on_the_public_methods_reproduces_the_reference(tag, nets):
    """seqA: k = 1, fusion, a re-annotated frame; seqC: k = 3, the scribble path.  Masks under the suite's clip_bound / frame_bound against
    the reference's own goldens, probabilities to prob_atol = 3e-3.  (Not bit-identical with InferenceCore by construction: the loop
    decodes frame by frame, the engine in groups.)"""
    g = load_golden(tag)
    outs = run_sequence(lambda img, k, mf: StageLoopCore(nets[0], nets[1], img, k, mem_freq=mf), tag, g)
    check_sequence_against_golden(outs, tag, g, prob_atol=3e-3, who="stage loop")


# ------------------------------------------------------------------------------------------------ 5. streams
def test_two_streams_never_share_scratch(nets):
    """The same encode_key under two current streams, back to back with no synchronisation in between: each stream has its own stage
    context, so both results are the single-stream result, bit for bit."""
    img = O.pad16(synth.synthetic_clip(1, 128, 160))[0][:, 0].cuda()
    want = nets[0].encode_key(img)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = []
    for s in (s1, s2, s1, s2):
        with torch.cuda.stream(s):
            got.append(nets[0].encode_key(img))
    torch.cuda.synchronize()
    for o in got:
        assert all(torch.equal(a, b) for a, b in zip(o, want))


def test_results_do_not_depend_on_the_objects_a_context_has_room_for(nets):
    """The conv planners pick a kernel family by what fits the Winograd workspace, and a context made for more objects has a larger one
    (at 128x160 key_proj takes F(4x4) only in a workspace for >= 4 objects): every call plans with the capacity of its OWN object count.
    encode_key before and after a 3-object encode_value at the same frame size (which replaces the 1-object context by a 4-object one),
    and a 1-object encode_value in both contexts, bit for bit."""
    img = O.pad16(synth.synthetic_clip(1, 128, 160))[0][:, 0].cuda()
    m3 = O.pad16(synth.synthetic_mask(1, 128, 160, 3)[:, 0])[0].cuda()
    with torch.cuda.stream(torch.cuda.Stream()):           # a stream no other test has a context on: the first context here is a 1-object one
        kf = nets[0].encode_key(img)
        v1 = nets[0].encode_value(img, kf[2], m3[:1])
        v3 = nets[0].encode_value(img, kf[2], m3)
        assert all(torch.equal(a, b) for a, b in zip(nets[0].encode_key(img), kf))
        assert torch.equal(nets[0].encode_value(img, kf[2], m3[:1]), v1)
        assert torch.equal(nets[0].encode_value(img, kf[2], m3), v3)
    torch.cuda.synchronize()
