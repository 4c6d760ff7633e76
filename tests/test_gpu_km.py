"""GPU: the kernelized memory read (``km``) - the read alone (stcn_test_memory_read_km: row centres, biased selection, weights, read-out)
against the fp64 restatement of tests/km_oracle.py, and the engine on whole interact() sequences against fixtures of the REAL reference with
``net.memory.km`` set (tools/gen_golden_km.py) and against the km oracle.  Tolerances are the suite's: 2e-5 on weights and read-out, 1e-4
as the near-tie window, the reference's own spread (tests/golden/selfnoise_km.npz) on sequences."""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

import km_oracle
import test_oracle_golden as TG
from conftest import load_golden
from eva_vos_amd import _lib, synth
from gpu_util import call, dev, stream
from oracle import stcn_oracle as O
from test_gpu_kernels import _dense, _plan
from test_gpu_sequence import CLEAN_FP32, make_core, masks_close
from test_gpu_topk import _memread_k
from test_km_api import KM_TAGS, km_noise, km_oracle_for

pytestmark = pytest.mark.gpu


def _memread_km(mk, mv, qk, top_k, h16, w16, km):
    N, Q, k = mk.shape[0], qk.shape[0], mv.shape[0]
    cen = torch.full((Q // (h16 * w16), N), -1, dtype=torch.int32, device="cuda")
    idx = torch.full((Q, top_k), -1, dtype=torch.int32, device="cuda")
    w = torch.zeros(Q, top_k, device="cuda")
    ro = torch.empty(k, Q, 512, device="cuda")
    call("stcn_test_memory_read_km", stream(), dev(mk), dev(mv), dev(qk), N, Q, k, top_k, h16, w16, float(km), cen, idx, w, ro)
    return cen.cpu().long(), idx.cpu().long(), w.cpu(), ro.cpu()


# ------------------------------------------------------------------------------------------ the read alone
# (h16, w16, N, Q, top_k, objects): a single frame; a two-frame group whose 64-query blocks straddle the frame boundary at query 80; a
# multi-chunk, sampled plan at the 480p frame
BANKS = {"frame": (8, 10, 240, 80, 50, 2), "group": (8, 10, 240, 160, 20, 1), "480p": (30, 54, 32400, 1620, 50, 1)}
CASES = [("frame", 5.6), ("group", 5.6), ("480p", 5.6), ("480p", 1.5)]
_DATA = {}


def bank(name):
    """Inputs of a bank (drawn as test_gpu_kernels.test_memory_read_matches_oracle draws them), its fp64 affinity and the plain read of the
    engine: computed once, shared by the tests below, never written to."""
    if name not in _DATA:
        h16, w16, N, Q, top_k, k = BANKS[name]
        g = torch.Generator().manual_seed(N + Q)
        mk, qk, mv = torch.randn(N, 64, generator=g), torch.randn(Q, 64, generator=g), torch.randn(k, N, 512, generator=g)
        S = O.affinity_logits(mk.double(), qk.double())
        _DATA[name] = dict(mk=mk, qk=qk, mv=mv, S=S, plain=_memread_k(mk, mv, qk, top_k))
    return _DATA[name]


def _check_own(B, mv, gi, gw, gro, queries):
    """The argument of test_gpu_topk._check_own on the biased scores B [N, Q] (fp64): a valid top-k to the near-tie window, the softmax of
    ITS rows and the read-out of ITS rows."""
    N = B.shape[0]
    for q in queries:
        sq = B[:, q]
        sel = torch.zeros(N, dtype=torch.bool)
        sel[gi[q]] = True
        if (~sel).any():
            assert sq[sel].min() >= sq[~sel].max() - 1e-4, q
        assert (torch.softmax(sq[gi[q]], 0).float() - gw[q]).abs().max() < 2e-5, q
        own = torch.einsum("j,kjc->kc", gw[q], mv[:, gi[q]])
        assert (gro[:, q] - own).abs().max() / own.abs().max() < 2e-5, q


def test_the_480p_bank_runs_a_multi_chunk_sampled_plan():
    pl = _plan(32400, 1620)
    assert pl["nc2"] >= 2 and pl["ss"] >= 2 and pl["nc1"] >= 2, pl


@pytest.mark.parametrize("name,km", CASES, ids=[f"{n}-km{s}" for n, s in CASES])
def test_memory_read_km_matches_fp64_oracle(name, km):
    """Centres: every one a valid argmax of its row within its frame (fp64 score within 1e-4 of the row's maximum), exactly the fp64 argmax
    where the best two queries differ by more than 1e-4.  The read: expected in fp64 FROM THE ENGINE'S OWN CENTRES, so the two checks are
    independent and no row or query is left out.  Clear-cut queries (top_k-th and next biased score more than 1e-4 apart): the oracle's
    rows - compared where the fp64 weight is >= 1e-12, below that the reference's product form is zero and ranks arbitrarily -, weights and
    read-out to 2e-5.  Every other query: a valid top-k of the biased scores with its own weights and read-out."""
    h16, w16, N, Q, top_k, k = BANKS[name]
    hw16 = h16 * w16
    d = bank(name)
    mk, qk, mv, S = d["mk"], d["qk"], d["mv"], d["S"]
    cen, gi, gw, gro = _memread_km(mk, mv, qk, top_k, h16, w16, km)
    assert cen.shape == (Q // hw16, N) and (cen >= 0).all() and (cen < hw16).all()
    flips = 0
    for f in range(Q // hw16):
        Sf = S[:, f * hw16:(f + 1) * hw16]
        top2 = torch.topk(Sf, 2, dim=1).values
        got = Sf.gather(1, cen[f][:, None])[:, 0]
        assert (top2[:, 0] - got).max() <= 1e-4, (f, float((top2[:, 0] - got).max()))
        clear = top2[:, 0] - top2[:, 1] > 1e-4
        assert (cen[f] == Sf.argmax(1))[clear].all(), f
        flips += int((cen[f] != Sf.argmax(1)).sum())
    B, _ = km_oracle.biased_logits(mk.double(), qk.double(), h16, w16, km, centres=cen)
    oi, ow, oro, gap = km_oracle.read_from_logits(B, mv.double(), top_k, return_gap=True)
    assert (gi >= 0).all() and (gi < N).all()
    assert (torch.sort(gi, 1).values.diff(dim=1) > 0).all(), "duplicate rows selected"
    assert torch.allclose(gw.sum(1), torch.ones(Q), atol=1e-5)
    clear = gap > 1e-4
    heavy = _dense(oi, ow.float(), N) >= 1e-12
    sel = torch.zeros(Q, N, dtype=torch.bool)
    sel.scatter_(1, gi, True)
    same = ~(heavy & ~sel).any(1)            # every row the oracle gives weight to was selected (all top_k of them heavy: the identical set)
    print(f"{name} km={km}: plan {_plan(N, Q)}; {flips} centres off the fp64 argmax (all within 1e-4); {int((~clear).sum())} near-tie queries, "
          f"{int((~same).sum())} selected differently; rows of weight < 1e-12 among the oracle's: {int((~heavy).sum() - Q * (N - top_k))}")
    assert same[clear].all(), "a clear-cut query selected other rows than the oracle"
    dw = (_dense(gi, gw, N) - _dense(oi, ow.float(), N)).abs().max(1).values
    assert dw[same].max() < 2e-5, float(dw[same].max())
    err = (gro - oro.float()).abs().amax((0, 2)) / oro.abs().max()
    assert err[same].max() < 2e-5, float(err[same].max())
    _check_own(B, mv, gi, gw, gro, torch.nonzero(~same).flatten().tolist())


@pytest.mark.parametrize("name", list(BANKS))
def test_a_wide_kernel_is_the_plain_read(name):
    """km = 1e4: the bias is at most (h16^2 + w16^2) / 2e8 - 6.5e-7 on the 8x10 frame, below the rounding of a score, and 1.9e-5 on the
    30x54 frame, inside the near-tie window.  The plain read's row sets for every query whose plain top_k-th and next scores lie more than
    1e-4 apart, read-out within 2e-5 on them."""
    h16, w16, N, Q, top_k, k = BANKS[name]
    d = bank(name)
    pi, pw, pro = d["plain"]
    _, gi, gw, gro = _memread_km(d["mk"], d["mv"], d["qk"], top_k, h16, w16, 1e4)
    vals = torch.topk(d["S"], top_k + 1, dim=0).values
    clear = vals[top_k - 1] - vals[top_k] > 1e-4
    same = (torch.sort(gi, 1).values == torch.sort(pi, 1).values).all(1)
    print(f"{name}: {int((~clear).sum())} near-tie queries, {int((~same).sum())} row sets differ from the plain read")
    assert same[clear].all()
    err = (gro - pro).abs().amax((0, 2)) / pro.abs().max()
    assert err[clear].max() < 2e-5, float(err[clear].max())


@pytest.mark.parametrize("name", list(BANKS))
def test_a_narrow_kernel_changes_most_queries(name):
    h16, w16, N, Q, top_k, k = BANKS[name]
    d = bank(name)
    _, gi, _, _ = _memread_km(d["mk"], d["mv"], d["qk"], top_k, h16, w16, 1.5)
    differ = (torch.sort(gi, 1).values != torch.sort(d["plain"][0], 1).values).any(1)
    print(f"{name}: {int(differ.sum())} of {Q} queries select other rows at km = 1.5 than the plain read")
    assert differ.float().mean() > 0.5


def test_bad_km_arguments_are_refused():
    from gpu_util import ptr
    mk, qk, mv, ro = dev(torch.randn(240, 64)), dev(torch.randn(80, 64)), dev(torch.randn(1, 240, 512)), torch.empty(1, 80, 512, device="cuda")
    fn = _lib.lib().stcn_test_memory_read_km
    for h16, w16, km in [(8, 9, 5.6), (8, 10, 0.0), (8, 10, float("nan")), (8, 10, float("inf")), (0, 0, 5.6)]:
        assert fn(stream(), ptr(mk), ptr(mv), ptr(qk), 240, 80, 1, 20, h16, w16, km, None, None, None, ptr(ro)) == -1, (h16, w16, km)
    ms = C.c_float()
    assert _lib.lib().stcn_bench_memory_read_km(stream(), ptr(mk), ptr(mv), ptr(qk), 240, 80, 1, 20, 8, 9, 5.6, 1, ptr(ro), C.byref(ms), None) == -1
    assert _lib.lib().stcn_bench_memory_read_km(stream(), ptr(mk), ptr(mv), ptr(qk), 240, 80, 1, 20, 8, 10, 5.6, 1, ptr(ro), C.byref(ms), None) == 0
    assert ms.value > 0


# ------------------------------------------------------------------------------------------ the engine
def _container(weights, top_k, km):
    from eva_vos_amd.params import PropagationNetwork
    p = PropagationNetwork(top_k=top_k, km=km)
    p.load_state_dict(weights[0], strict=True)
    return p.eval()


_NETS, _SOLO = {}, {}


def nets_km(weights, nets, top_k, km):
    if (top_k, km) not in _NETS:
        _NETS[(top_k, km)] = (_container(weights, top_k, km), nets[1])
    return _NETS[(top_k, km)]


def solo(tag, nets_k):
    """One engine, the fixture's script from a fresh core: [(masks, prob)] per round.  Computed once per (fixture, top_k, km) and shared."""
    key = (tag, nets_k[0].top_k, nets_k[0].km)
    if key not in _SOLO:
        _SOLO[key] = TG.run_sequence(make_core(nets_k), tag, load_golden(tag))
    return _SOLO[key]


def _same(a, b):
    return all(np.array_equal(ma, mb) and torch.equal(pa, pb) for (ma, pa), (mb, pb) in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("tag", KM_TAGS)
def test_sequences_with_km_match_reference_and_oracle(tag, weights, nets, monkeypatch):
    """The HIP engine with a km model against the REFERENCE's masks and probabilities with ``memory.km`` set, and against the km oracle:
    the check function, bounds and 1.5 x self-noise policy of test_gpu_topk.test_sequences_at_top_k_20_match_reference_and_oracle, yardsticks
    from selfnoise_km.npz.  What one run measured is kept in profiles/km_parity.txt."""
    g = load_golden(tag)
    km, top_k = km_oracle_for(monkeypatch, g, tag)
    k = int(g[f"{tag}.shape"][3])
    noise = km_noise(monkeypatch)
    outs = solo(tag, nets_km(weights, nets, top_k, km))
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


def test_km_changes_the_result(weights, nets):
    """An engine that ignored km would pass every comparison of the default."""
    a, b = solo("seqKM", nets_km(weights, nets, 50, 5.6)), solo("seqKM", nets)
    diff = [int((ma != mb).sum()) for (ma, _), (mb, _) in zip(a, b)]
    dp = [float((pa - pb).abs().max()) for (_, pa), (_, pb) in zip(a, b)]
    print("seqKM, km = 5.6 against the plain read per round: mask pixels differing", diff, "max |dprob|", dp)
    assert max(diff) > 0 and max(dp) > 1e-2, (diff, dp)


def test_models_of_two_km_do_not_share_a_cache_entry(weights, nets):
    """Containers with the same weights and km 5.6 / 1.5 / None used alternately on one device: each reproduces its solo run bit for bit.
    And ONE container whose km is changed between two cores gets another model."""
    from mivos.inference_core import InferenceCore
    g = load_golden("seqKM")
    T, H, W, k, mf = [int(v) for v in g["seqKM.shape"]]
    img, msk = synth.synthetic_clip(T, H, W), synth.synthetic_mask(T, H, W, k)
    sets = {5.6: nets_km(weights, nets, 50, 5.6), 1.5: nets_km(weights, nets, 50, 1.5), None: nets}
    cores = {km: InferenceCore(n[0], n[1], img, k, mem_freq=mf) for km, n in sets.items()}
    assert cores[5.6].km == pytest.approx(5.6, rel=1e-6) and cores[1.5].km == 1.5 and cores[None].km is None
    assert len({id(c._model) for c in cores.values()}) == 3
    outs = {km: [] for km in sets}
    for mf_, idx in g["seqKM.script"]:
        for km in sets:
            m = cores[km].interact(msk[:, int(mf_)].clone(), int(idx))
            outs[km].append((m.copy(), cores[km].prob.detach().float().cpu().clone()))
    for km, n in sets.items():
        assert _same(outs[km], solo("seqKM", n)), km
    one = _container(weights, 50, 5.6)
    first = InferenceCore(one, nets[1], img, k, mem_freq=mf)
    one.km = None
    second = InferenceCore(one, nets[1], img, k, mem_freq=mf)
    assert first.km == pytest.approx(5.6, rel=1e-6) and second.km is None and first._model is not second._model
    m = second.interact(msk[:, 0].clone(), 0)
    assert np.array_equal(m, solo("seqKM", nets)[0][0]) and torch.equal(second.prob.cpu(), solo("seqKM", nets)[0][1])


def test_clone_and_reset_keep_the_models_km(weights, nets):
    n = nets_km(weights, nets, 50, 5.6)
    g = load_golden("seqKM")
    T, H, W, k, mf = [int(v) for v in g["seqKM.shape"]]
    img, msk = synth.synthetic_clip(T, H, W), synth.synthetic_mask(T, H, W, k)
    script = [(int(a), int(b)) for a, b in g["seqKM.script"]]
    ref = solo("seqKM", n)
    core = make_core(n)(img, k, mf)
    first = core.interact(msk[:, script[0][0]].clone(), script[0][1])
    assert np.array_equal(first, ref[0][0])
    twin = copy.deepcopy(core)
    assert twin.km == pytest.approx(5.6, rel=1e-6)
    for r, (mf_, idx) in enumerate(script[1:], 1):
        m = twin.interact(msk[:, mf_].clone(), idx)
        assert np.array_equal(m, ref[r][0]) and torch.equal(twin.prob.cpu(), ref[r][1]), r
    core.reset()
    assert core.km == pytest.approx(5.6, rel=1e-6)
    for r, (mf_, idx) in enumerate(script):
        m = core.interact(msk[:, mf_].clone(), idx)
        assert np.array_equal(m, ref[r][0]) and torch.equal(core.prob.cpu(), ref[r][1]), r


def test_reference_style_module_hands_over_memory_km(weights, nets):
    """A live reference PropagationNetwork has no .km: the caller sets it on the memory reader (``prop_model.memory.km = 5.6``)."""

    class RefStyle:
        def __init__(self, net):
            self._net, self.memory = net, types.SimpleNamespace(top_k=50, km=5.6)

        def state_dict(self, *a, **kw):
            return self._net.state_dict(*a, **kw)

    mod = RefStyle(nets[0])
    assert not hasattr(mod, "km")
    g = load_golden("seqKM")
    T, H, W, k, mf = [int(v) for v in g["seqKM.shape"]]
    core = make_core((mod, nets[1]))(synth.synthetic_clip(T, H, W), k, mf)
    assert core.km == pytest.approx(5.6, rel=1e-6) and core.top_k == 50
    v = C.c_float()
    _lib.check(_lib.lib().stcn_model_get_km(core._model.handle, C.byref(v)), "stcn_model_get_km")
    assert v.value == np.float32(5.6)
    m = core.interact(synth.synthetic_mask(T, H, W, k)[:, 0], 0)
    assert np.array_equal(m, solo("seqKM", nets_km(weights, nets, 50, 5.6))[0][0])
