"""GPU: ``top_k`` in 1..49 - the memory read alone (stcn_test_memory_read_k) against the CPU oracle with its cut patched, and the engine
on whole interact() sequences against fixtures of the REAL reference's ``PropagationNetwork(top_k=20)`` (tools/gen_golden_topk.py) and
against the oracle; the default (``top_k=50``) must stay bit-identical.  Tolerances are the suite's: 2e-5 on weights and read-out,
1e-4 as the near-tie window, the reference's own spread (tests/golden/selfnoise_topk.npz) on sequences."""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

import test_oracle_golden as TG
from conftest import load_golden
from eva_vos_amd import _lib, synth
from gpu_util import call, dev, ptr, stream
from oracle import stcn_oracle as O
from test_gpu_kernels import _dense, _memread, _plan
from test_gpu_sequence import CLEAN_FP32, make_core, masks_close
from test_topk_api import TOPK_TAGS, topk_noise

pytestmark = pytest.mark.gpu


def _memread_k(mk, mv, qk, top_k):
    N, Q, k = mk.shape[0], qk.shape[0], mv.shape[0]
    idx = torch.full((Q, top_k), -1, dtype=torch.int32, device="cuda")
    w = torch.zeros(Q, top_k, device="cuda")
    ro = torch.empty(k, Q, 512, device="cuda")
    call("stcn_test_memory_read_k", stream(), dev(mk), dev(mv), dev(qk), N, Q, k, top_k, idx, w, ro)
    return idx.cpu().long(), w.cpu(), ro.cpu()


def _check_own(mk, mv, qk, gi, gw, gro, queries):
    """Queries that selected other rows than the oracle: a valid top-k of the fp64 scores to the near-tie window, the softmax of ITS
    rows and the read-out of ITS rows (as test_memory_read_at_config3_bank_sizes_matches_oracle)."""
    N = mk.shape[0]
    for q in queries:
        sq = O.affinity_logits(mk.double(), qk[q:q + 1].double())[:, 0]
        sel = torch.zeros(N, dtype=torch.bool)
        sel[gi[q]] = True
        if (~sel).any():
            assert sq[sel].min() >= sq[~sel].max() - 1e-4, q
        assert (torch.softmax(sq[gi[q]], 0).float() - gw[q]).abs().max() < 2e-5, q
        own = torch.einsum("j,kjc->kc", gw[q], mv[:, gi[q]])
        assert (gro[:, q] - own).abs().max() / own.abs().max() < 2e-5, q


# ------------------------------------------------------------------------------------------ the read alone
BANKS = [("K", 16, 1, 1.0), ("36", 36, 1, 1.0), (160, 80, 1, 1.0), (1620, 333, 2, 1.0), (5000, 200, 3, 0.5), (32400, 97, 1, 1.0)]


def test_a_listed_bank_runs_a_multi_chunk_sampled_plan():
    pl = _plan(32400, 97)
    assert pl["nc2"] >= 2 and pl["ss"] >= 2 and pl["nc1"] >= 2, pl


def random_bank(N, Q, k, scale=1.0):
    """mk [N,64], mv [k,N,512], qk [Q,64] drawn as test_gpu_kernels.test_memory_read_matches_oracle draws them"""
    g = torch.Generator().manual_seed(N + Q)
    mk = torch.randn(N, 64, generator=g) * scale
    qk = torch.randn(Q, 64, generator=g) * scale
    mv = torch.randn(k, N, 512, generator=g)
    return mk, mv, qk


def check_read_k_against_oracle(mk, mv, qk, top_k):
    """The statements of test_memory_read_k_matches_oracle for one bank (O.TOP_K is already top_k): returns the numbers of near-tie queries
    and of queries that selected other rows than the oracle.  Shared with tests/switch_arm_cases.py."""
    N, Q, k = mk.shape[0], qk.shape[0], mv.shape[0]
    oi, ow, oro, gap = O.memory_read(mk, mv, qk, return_gap=True)
    assert oi.shape == (Q, top_k)
    gi, gw, gro = _memread_k(mk, mv, qk, top_k)
    assert (gi >= 0).all() and (gi < N).all()
    assert (torch.sort(gi, 1).values.diff(dim=1) > 0).all(), "duplicate rows selected"
    assert torch.allclose(gw.sum(1), torch.ones(Q), atol=1e-5)
    near = gap < 1e-4
    same = (torch.sort(gi, 1).values == torch.sort(oi, 1).values).all(1)
    pl = _plan(N, Q)
    print(f"top_k={top_k} N={N} Q={Q} k={k}: plan {pl}; {int(near.sum())} near-tie queries, {int((~same).sum())} selected differently")
    assert near.float().mean() <= 0.04, float(near.float().mean())
    assert same[~near].all(), "a clear-cut query selected other rows than the oracle"
    dw = (_dense(gi, gw, N) - _dense(oi, ow, N)).abs().max(1).values
    assert dw[same].max() < 2e-5, float(dw[same].max())
    err = (gro - oro).abs().amax((0, 2)) / oro.abs().max()
    assert err[same].max() < 2e-5, float(err[same].max())
    _check_own(mk, mv, qk, gi, gw, gro, torch.nonzero(~same).flatten().tolist())
    return int(near.sum()), int((~same).sum())


@pytest.mark.parametrize("bank", BANKS, ids=lambda b: f"N{b[0]}-Q{b[1]}-k{b[2]}")
@pytest.mark.parametrize("top_k", [1, 2, 20, 49])
def test_memory_read_k_matches_oracle(top_k, bank, monkeypatch):
    """Inputs drawn as test_gpu_kernels.test_memory_read_matches_oracle draws them.  Clear-cut queries (gap between the top_k-th and the
    next score >= 1e-4): the oracle's selection, weights and read-out.  Near-tie queries (at most 4 % of a case, asserted): any valid
    top-k of the fp64 scores with its own weights and read-out."""
    N, Q, k, scale = bank
    N = top_k if N == "K" else (max(36, top_k) if N == "36" else N)
    monkeypatch.setattr(O, "TOP_K", top_k)
    check_read_k_against_oracle(*random_bank(N, Q, k, scale), top_k)


def rising_scores_bank():
    """The bank of test_memory_read_rising_scores_forces_many_selects: scores rise with the row index.  Under the two-pass read the
    threshold of pass 1 lands about 50 rows from the end of the bank and all candidates sit in one short chunk: its longest list is 32,
    25 or 8 entries at top_k = 50, 20 or 1 (tests/test_memread_lists.py prints them), below the 64 a list holds, so no list overflows
    and none is cut back inside pass 2."""
    N, Q = 4000, 48
    u = torch.randn(64, generator=torch.Generator().manual_seed(3))
    u = u / u.norm() * 3.0
    a = torch.linspace(0.0, 0.9, N)[:, None]
    mk = a * u[None, :] + 1e-3 * torch.randn(N, 64, generator=torch.Generator().manual_seed(4))
    qk = u[None, :].repeat(Q, 1) + 0.05 * torch.randn(Q, 64, generator=torch.Generator().manual_seed(5))
    mv = torch.randn(1, N, 512, generator=torch.Generator().manual_seed(6))
    return mk, mv, qk


def check_rising_scores_read(top_k):
    """(O.TOP_K is already top_k) weights and read-out of the rising-scores bank within 5e-5 of the oracle's; returns the two figures"""
    mk, mv, qk = rising_scores_bank()
    N = mk.shape[0]
    oi, ow, oro = O.memory_read(mk, mv, qk)
    gi, gw, gro = _memread_k(mk, mv, qk, top_k)
    dw, err = float((_dense(gi, gw, N) - _dense(oi, ow, N)).abs().max()), float((gro - oro).abs().max() / oro.abs().max())
    assert dw < 5e-5
    assert err < 5e-5
    return dw, err


@pytest.mark.parametrize("top_k", [1, 20])
def test_rising_scores_cut_full_lists_back_to_top_k(top_k, monkeypatch):
    """The rising-scores bank at top_k < 50: the longest pass-2 list is 25 (top_k = 20) or 8 (top_k = 1) entries, so only the select at
    the chunk's write-out (a list longer than top_k) runs here; the name dates from the one-pass read.  Lists that overflow their 64
    entries and are cut back inside pass 2: tests/test_gpu_memread_lists.py."""
    monkeypatch.setattr(O, "TOP_K", top_k)
    check_rising_scores_read(top_k)


def test_exact_ties_at_top_k_20(monkeypatch):
    """Every row 4 times (identical values behind tied rows): any tie-break is valid, 20 DISTINCT rows and the read-out must hold."""
    monkeypatch.setattr(O, "TOP_K", 20)
    N, Q = 640, 32
    g = torch.Generator().manual_seed(9)
    mk = torch.randn(N // 4, 64, generator=g).repeat(4, 1)
    mv = torch.randn(1, N // 4, 512, generator=g).repeat(1, 4, 1)
    qk = torch.randn(Q, 64, generator=g)
    _, _, oro = O.memory_read(mk, mv, qk)
    gi, gw, gro = _memread_k(mk, mv, qk, 20)
    assert all(len(set(r.tolist())) == 20 for r in gi)
    assert torch.allclose(gw.sum(1), torch.ones(Q), atol=1e-5)
    assert (gro - oro).abs().max() / oro.abs().max() < 2e-5


@pytest.mark.parametrize("top_k", [20, 49])
def test_near_tie_triplets_at_top_k(top_k, monkeypatch):
    """The triplet bank of test_near_tie_queries_are_the_only_ones_that_differ: clear-cut queries identical to the oracle, near-tie
    queries a valid top-k (to 1e-4) with their own weights and read-out.  (Exactness to 1e-9 is not asserted here: whether every
    near-tie candidate survives the per-chunk cut depends on the chunk plan at this top_k.)"""
    monkeypatch.setattr(O, "TOP_K", top_k)
    g = torch.Generator().manual_seed(21)
    single = torch.randn(300, 64, generator=g)
    base = torch.randn(300, 64, generator=g)
    trip = torch.cat([base * (1 + 1e-7 * torch.randn(300, 1, generator=g)) for _ in range(3)], 0)
    mk = torch.cat([single, trip], 0)[torch.randperm(1200, generator=g)]
    qk = torch.randn(256, 64, generator=g)
    mv = torch.randn(2, 1200, 512, generator=g)
    oi, ow, oro, gap = O.memory_read(mk, mv, qk, return_gap=True)
    gi, gw, gro = _memread_k(mk, mv, qk, top_k)
    S = O.affinity_logits(mk.double(), qk.double()).t()
    near = gap < 1e-4
    print(f"top_k={top_k}: share of near-tie queries {float(near.float().mean()):.2f}")
    assert 0.15 < near.float().mean() < 0.85, "the construction must yield both kinds of queries"
    N = mk.shape[0]
    assert (torch.sort(gi, 1).values.diff(dim=1) > 0).all(), "duplicate rows selected"
    dd = (_dense(gi, gw, N) - _dense(oi, ow, N)).abs().max(1).values
    assert dd[~near].max() < 2e-5, float(dd[~near].max())
    err = (gro - oro).abs().amax((0, 2)) / oro.abs().max()
    assert err[~near].max() < 2e-5, float(err[~near].max())
    sel = torch.zeros(qk.shape[0], N, dtype=torch.bool)
    sel.scatter_(1, gi, True)
    lo = torch.where(sel, S, torch.full_like(S, float("inf"))).min(1).values
    hi = torch.where(~sel, S, torch.full_like(S, -float("inf"))).max(1).values
    assert (lo >= hi - 1e-4).all(), float((hi - lo).max())
    ws = torch.softmax(torch.gather(S, 1, gi), 1).float()
    assert (ws - gw).abs().max() < 2e-5
    own = torch.einsum("qj,kqjc->kqc", gw, mv[:, gi])
    assert (gro - own).abs().max() / own.abs().max() < 2e-5


@pytest.mark.parametrize("N,Q,k", [(1620, 333, 2), (32400, 97, 1)])
def test_top_k_50_is_the_default_read_bit_for_bit(N, Q, k):
    g = torch.Generator().manual_seed(N + Q)
    mk, qk, mv = torch.randn(N, 64, generator=g), torch.randn(Q, 64, generator=g), torch.randn(k, N, 512, generator=g)
    a, b = _memread(mk, mv, qk), _memread_k(mk, mv, qk, 50)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_bank_smaller_than_top_k_is_refused():
    mk, qk, mv, ro = dev(torch.randn(19, 64)), dev(torch.randn(4, 64)), dev(torch.randn(1, 19, 512)), torch.empty(1, 4, 512, device="cuda")
    rc = _lib.lib().stcn_test_memory_read_k(stream(), ptr(mk), ptr(mv), ptr(qk), 19, 4, 1, 20, None, None, ptr(ro))
    assert rc == -1 and "top_k" in _lib.lib().stcn_last_error().decode()                    # STCN_E_INVALID
    ms = C.c_float()
    rc = _lib.lib().stcn_bench_memory_read_k(stream(), ptr(mk), ptr(mv), ptr(qk), 19, 4, 1, 20, 1, ptr(ro), C.byref(ms), None)
    assert rc == -1
    assert _lib.lib().stcn_test_memory_read_k(stream(), ptr(mk), ptr(mv), ptr(qk), 19, 4, 1, 51, None, None, ptr(ro)) == -1


# ------------------------------------------------------------------------------------------ the engine
def _container(weights, top_k):
    from eva_vos_amd.params import PropagationNetwork
    p = PropagationNetwork(top_k=top_k)
    p.load_state_dict(weights[0], strict=True)
    return p.eval()


@pytest.fixture(scope="module")
def nets20(weights, nets):
    return _container(weights, 20), nets[1]


_SOLO = {}


def solo(tag, nets_k):
    """One engine, the fixture's script from a fresh core: [(masks, prob)] per round.  Computed once per (fixture, top_k) and shared."""
    key = (tag, nets_k[0].top_k)
    if key not in _SOLO:
        _SOLO[key] = TG.run_sequence(make_core(nets_k), tag, load_golden(tag))
    return _SOLO[key]


def _same(a, b):
    return all(np.array_equal(ma, mb) and torch.equal(pa, pb) for (ma, pa), (mb, pb) in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("tag", TOPK_TAGS)
def test_sequences_at_top_k_20_match_reference_and_oracle(tag, nets20, weights, monkeypatch):
    """The HIP engine with a top_k=20 model against the REFERENCE's masks and probabilities (checks and bounds of
    test_gpu_sequence.test_sequences_match_reference_goldens, yardsticks from selfnoise_topk.npz), and against the oracle at the same cut:
    masks within clip_bound / frame_bound of the reference's own spread, for k = 1 probabilities within 2e-4 on the frames before the
    first near-tie.  seqT20s is a 96x112 frame: 42 keys, fewer than the default cut."""
    g = load_golden(tag)
    top_k, k = int(g[f"{tag}.top_k"]), int(g[f"{tag}.shape"][3])
    noise = topk_noise(monkeypatch)
    monkeypatch.setattr(O, "TOP_K", top_k)
    outs = solo(tag, nets20)
    orcs = []

    def oracle(img, k_, mf):
        orcs.append(O.OracleCore(weights[0], weights[1], img, k_, mem_freq=mf))
        return orcs[0]

    oouts = TG.run_sequence(oracle, tag, g)
    ties = TG.tie_summary(orcs[0])
    TG.check_sequence_against_golden(outs, tag, g, prob_atol=3e-3, ties=ties, who="HIP")
    for r, ((a, pa), (b, pb)) in enumerate(zip(outs, oouts)):
        masks_close(a, b, k, f"{tag} r{r}", yard=noise[tag][r])
        if k == 1:
            clean = sorted(ties[r]["clean"])
            d = (pa - pb).abs()
            worst = float(d[:, clean].max()) if clean else 0.0
            print(f"HIP vs oracle {tag} r{r}: {len(clean)} clean frames, max |dprob| {worst:.1e} (all frames {float(d.max()):.1e})")
            assert worst < CLEAN_FP32, (tag, r, worst)


def test_small_frame_needs_a_smaller_top_k(nets, nets20):
    img = synth.synthetic_clip(2, 96, 112)                   # 6 x 7 = 42 keys
    with pytest.raises(RuntimeError, match=r"42 must be >= top_k = 50"):
        make_core(nets)(img, 1, 5)
    core = make_core(nets20)(img, 1, 5)
    assert core.top_k == 20
    assert core.interact(synth.synthetic_mask(2, 96, 112, 1)[:, 0], 0).shape == (2, 96, 112)


def test_top_k_changes_the_result(nets, nets20):
    """The reference's own masks at top_k = 20 and 50 differ in thousands of pixels on this clip: an engine that ignored the value
    would pass every other comparison of the default."""
    a, b = solo("seqT20", nets20), solo("seqT20", nets)
    diff = [int((ma != mb).sum()) for (ma, _), (mb, _) in zip(a, b)]
    print("mask pixels differing between top_k=20 and top_k=50 per round:", diff)
    assert max(diff) > 100, diff


def test_models_of_two_top_k_do_not_share_a_cache_entry(weights, nets, nets20):
    """Two containers with the same weights, top_k 20 and 50, used alternately on one device: each reproduces its solo run bit for bit.
    And ONE container whose top_k is changed between two cores gets another model."""
    from mivos.inference_core import InferenceCore
    g = load_golden("seqT20")
    T, H, W, k, mf = [int(v) for v in g["seqT20.shape"]]
    img, msk = synth.synthetic_clip(T, H, W), synth.synthetic_mask(T, H, W, k)
    cores = {20: InferenceCore(nets20[0], nets20[1], img, k, mem_freq=mf), 50: InferenceCore(nets[0], nets[1], img, k, mem_freq=mf)}
    assert cores[20].top_k == 20 and cores[50].top_k == 50 and cores[20]._model is not cores[50]._model
    outs = {20: [], 50: []}
    for mf_, idx in g["seqT20.script"]:
        for tk in (20, 50):
            m = cores[tk].interact(msk[:, int(mf_)].clone(), int(idx))
            outs[tk].append((m.copy(), cores[tk].prob.detach().float().cpu().clone()))
    assert _same(outs[20], solo("seqT20", nets20)) and _same(outs[50], solo("seqT20", nets))
    one = _container(weights, 20)
    first = InferenceCore(one, nets[1], img, k, mem_freq=mf)
    one.top_k = 50
    second = InferenceCore(one, nets[1], img, k, mem_freq=mf)
    assert (first.top_k, second.top_k) == (20, 50) and first._model is not second._model
    m = second.interact(msk[:, 0].clone(), 0)
    assert np.array_equal(m, solo("seqT20", nets)[0][0]) and torch.equal(second.prob.cpu(), solo("seqT20", nets)[0][1])


def test_clone_and_reset_keep_the_models_top_k(nets20):
    g = load_golden("seqT20")
    T, H, W, k, mf = [int(v) for v in g["seqT20.shape"]]
    img, msk = synth.synthetic_clip(T, H, W), synth.synthetic_mask(T, H, W, k)
    script = [(int(a), int(b)) for a, b in g["seqT20.script"]]
    ref = solo("seqT20", nets20)
    core = make_core(nets20)(img, k, mf)
    first = core.interact(msk[:, script[0][0]].clone(), script[0][1])
    assert np.array_equal(first, ref[0][0])
    twin = copy.deepcopy(core)
    assert twin.top_k == 20
    for r, (mf_, idx) in enumerate(script[1:], 1):
        m = twin.interact(msk[:, mf_].clone(), idx)
        assert np.array_equal(m, ref[r][0]) and torch.equal(twin.prob.cpu(), ref[r][1]), r
    core.reset()
    assert core.top_k == 20
    for r, (mf_, idx) in enumerate(script):
        m = core.interact(msk[:, mf_].clone(), idx)
        assert np.array_equal(m, ref[r][0]) and torch.equal(core.prob.cpu(), ref[r][1]), r


def test_reference_style_module_hands_over_memory_top_k(nets):
    """A live reference PropagationNetwork has no .top_k: its memory reader holds it (prop_net.py:149)."""

    class RefStyle:
        def __init__(self, net):
            self._net, self.memory = net, types.SimpleNamespace(top_k=20)

        def state_dict(self, *a, **kw):
            return self._net.state_dict(*a, **kw)

    mod = RefStyle(nets[0])
    assert not hasattr(mod, "top_k")
    core = make_core((mod, nets[1]))(synth.synthetic_clip(2, 96, 112), 1, 5)     # 42 keys: only a model below the default cut takes it
    assert core.top_k == 20
