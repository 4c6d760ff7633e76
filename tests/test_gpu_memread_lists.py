"""GPU: the top-k memory read (stcn_test_memory_read_km, memread.hip) on banks whose pass-2 candidate lists overflow their CAP2 = 64
entries in LDS - the cut-back to the best top_k inside affinity_tile_kernel<true>, the raised threshold and the replay of the appends that
found the list full.  No other hook test reaches that path (test_memread_lists.py prints the list lengths of their banks: 50 at most).

The banks and cases are those of tests/memread_lists.py; test_memread_lists.py shows on the host, without a GPU, that each of them fills
a list (129 .. 611 candidates for one (query, chunk)), is clear-cut, and can fail.  Here every case runs through the hook with every operand
and every output in front of a guard of NaNs, against oracle.stcn_oracle.memory_read (the kernelized read: tests/km_oracle.py from the
engine's own centres) on fp64 operands.  Bounds are the suite's: 2e-5 on weights and read-out (test_memory_read_matches_oracle), 1e-4 =
RESCORE_W as the near-tie window.  Every case is read twice: the same SET of rows per query (list positions come from LDS atomics, so
neither the order nor the last bit of a weight is promised; with distinct values behind tied keys the set is not either).

Measured on an MI355X, max |weight - fp64| / max |read-out - fp64| relative to max |read-out| (bound 2e-5 each); no query of any case
selected other rows than the oracle, a second read never another set:
  hidden-rising, top_k 50 / 20 / 1            7.5e-9 / 3.4e-7,  1.9e-8 / 2.7e-7,  0 / 0
  many-rising / -falling / -shuffled          7.5e-9 / 3.3e-7,  7.5e-9 / 4.1e-7,  7.5e-9 / 4.2e-7
  many-ss8                                    7.5e-9 / 3.4e-7
  column-rising                               9.3e-9 / 3.9e-7
  mixed                                       3.4e-8 / 3.9e-7
  split (with idx and w)                      7.5e-9 / 3.4e-7;  without them against with them: 0
  tied (a) top_k 50 / 20                      0 / 4.9e-7,  0 / 2.4e-7
  tied (b) top_k 50 / 20                      0 / 1.7e-7,  0 / 1.2e-7 (against the read-out of its own rows)
  kernelized, km 1e4 / 3                      9.3e-9 / 4.4e-7,  7.5e-9 / 2.6e-7 (one near-tie query at km 3, the oracle's rows too)
The whole file takes about 2 s.  With the cut-back and the replay taken out of a build (a full list loses its appends) eleven of the
seventeen tests fail with "a clear-cut query selected other rows than the oracle"; many-falling (the best rows come first), the tied
cases (any rows of the tie are right) and the split-against-merged comparison cannot see that fault."""
import pytest
import torch

import km_oracle
import memread_lists as L
from gpu_util import call, guard_intact, guarded, stream
from oracle import stcn_oracle as O
from test_gpu_attention import on_device
from test_gpu_kernels import _dense, _plan
from test_gpu_km import _check_own as check_own_biased
from test_gpu_topk import _check_own

pytestmark = pytest.mark.gpu

_DEV = {}


def operands(name):
    """the bank on the device, every operand in front of its guard: {mk, mv, qk: (buffer, view)}; one bank at a time"""
    if name not in _DEV:
        _DEV.clear()
        b = L.bank(name)
        _DEV[name] = {n: on_device(b[n]) for n in ("mk", "mv", "qk")}
    return _DEV[name]


class Read:
    """one call of stcn_test_memory_read_km, every output in front of its own guard; outputs=False: the engine's form (no idx, no w)"""

    def __init__(self, name, top_k, sigma=None, outputs=True):
        b, d = L.bank(name), operands(name)
        N, Q, k = b["mk"].shape[0], b["qk"].shape[0], b["mv"].shape[0]
        self.sizes = dict(idx=Q * top_k, w=Q * top_k, ro=k * Q * 512, cen=N)
        self.buf = {n: guarded(s) for n, s in self.sizes.items()}              # idx, cen: int32 behind the same bits (a NaN is no row)
        out = {n: self.buf[n][:s] for n, s in self.sizes.items()}
        h16, w16 = L.KM_FRAME if sigma else (0, 0)
        call("stcn_test_memory_read_km", stream(), d["mk"][1], d["mv"][1], d["qk"][1], N, Q, k, top_k, h16, w16, float(sigma or 0.0),
             out["cen"] if sigma else None, out["idx"] if outputs else None, out["w"] if outputs else None, out["ro"])
        self.intact = all(guard_intact(self.buf[n], s) for n, s in self.sizes.items())
        self.intact &= all(guard_intact(buf, view.numel()) for buf, view in d.values())
        self.idx = out["idx"].view(torch.int32).view(Q, top_k).cpu().long()
        self.w, self.ro = out["w"].view(Q, top_k).cpu(), out["ro"].view(k, Q, 512).cpu()
        self.cen = out["cen"].view(torch.int32).view(1, N).cpu().long()
        self.sets = torch.sort(self.idx, 1).values

    def check_form(self, N):
        """rows of the bank, distinct per query; weights that sum to 1; every element written and finite; no guard touched"""
        Q = self.idx.shape[0]
        assert self.intact, "a guard behind an operand or an output was written"
        assert (self.idx >= 0).all() and (self.idx < N).all()
        assert (self.sets.diff(dim=1) > 0).all(), "duplicate rows selected"
        assert torch.isfinite(self.w).all() and torch.isfinite(self.ro).all()
        assert torch.allclose(self.w.sum(1), torch.ones(Q), atol=1e-5)


def check_against(r, oracle, N, own, label):
    """The statements of test_memory_read_k_matches_oracle for the read r against oracle = (idx, w, read-out, gap) in fp64: clear-cut
    queries the oracle's rows; where the rows are the oracle's, its weights and read-out to 2e-5; every other query through own(queries)."""
    oi, ow, oro, gap = oracle
    near = gap < 1e-4
    same = (r.sets == torch.sort(oi, 1).values).all(1)
    dw = (_dense(r.idx, r.w, N) - _dense(oi, ow.float(), N)).abs().max(1).values
    err = (r.ro - oro.float()).abs().amax((0, 2)) / float(oro.abs().max())
    print(f"{label}: plan {_plan(N, r.idx.shape[0])}; {int(near.sum())} near-tie queries, {int((~same).sum())} selected differently; "
          f"max weight error {float(dw[same].max()):.2e}, max read-out error {float(err[same].max()):.2e}")
    assert near.float().mean() <= 0.04, float(near.float().mean())
    assert same[~near].all(), "a clear-cut query selected other rows than the oracle"
    assert dw[same].max() < 2e-5, float(dw[same].max())
    assert err[same].max() < 2e-5, float(err[same].max())
    own(torch.nonzero(~same).flatten().tolist())


PLAIN = [(c, i) for c, i in zip(L.CASES, L.CASE_IDS) if c[2] is None and not L.order_of(c[0]).startswith("tied")]


@pytest.mark.parametrize("name,top_k,sigma", [c for c, _ in PLAIN], ids=[i for _, i in PLAIN])
def test_overflowing_lists_match_oracle(name, top_k, sigma, monkeypatch):
    b = L.bank(name)
    mk, mv, qk = b["mk"], b["mv"], b["qk"]
    N = mk.shape[0]
    monkeypatch.setattr(O, "TOP_K", top_k)
    oracle = O.memory_read(mk.double(), mv.double(), qk.double(), return_gap=True)
    r = Read(name, top_k)
    r.check_form(N)
    check_against(r, oracle, N, lambda qs: _check_own(mk, mv, qk, r.idx, r.w, r.ro, qs), f"{name} top_k={top_k}")
    again = Read(name, top_k)
    again.check_form(N)
    assert torch.equal(again.sets, r.sets), "a second read selected other rows"


@pytest.mark.parametrize("top_k", [50, 20])
@pytest.mark.parametrize("form", ["a", "b"])
def test_more_than_a_list_of_equal_scores(form, top_k, monkeypatch):
    """128 identical keys hidden from pass 1, every query pointed at them: the cut falls inside the tie.  (a) one value row behind all of
    them: the oracle's read-out whichever rows are kept.  (b) distinct value rows: any top_k of the tied rows, weights 1 / top_k, the
    read-out of the rows selected."""
    name = f"tied-{form}"
    b = L.bank(name)
    mk, mv, qk = b["mk"], b["mv"], b["qk"]
    N, Q = mk.shape[0], qk.shape[0]
    r = Read(name, top_k)
    r.check_form(N)
    cluster = torch.zeros(N, dtype=torch.bool)
    cluster[b["rows"]] = True
    assert cluster[r.idx].all(), "a row outside the tied cluster was selected"
    assert (r.w - 1.0 / top_k).abs().max() < 2e-5, float((r.w - 1.0 / top_k).abs().max())
    if form == "a":
        monkeypatch.setattr(O, "TOP_K", top_k)
        _, _, oro = O.memory_read(mk.double(), mv.double(), qk.double())
        err = float((r.ro - oro.float()).abs().max() / oro.abs().max())
        assert torch.equal(Read(name, top_k).sets, r.sets), "a second read selected other rows"
    else:
        own = torch.einsum("qj,kqjc->kqc", r.w.double(), mv.double()[:, r.idx])
        err = float((r.ro - own.float()).abs().max() / own.abs().max())
    print(f"{name} top_k={top_k}: max weight error {float((r.w - 1.0 / top_k).abs().max()):.2e}, max read-out error {err:.2e}")
    assert err < 2e-5, err


KM = [(c, i) for c, i in zip(L.CASES, L.CASE_IDS) if c[2]]


@pytest.mark.parametrize("name,top_k,sigma", [c for c, _ in KM], ids=[i for _, i in KM])
def test_overflowing_lists_of_the_kernelized_read(name, top_k, sigma):
    """The bank of the first case under one 8 x 10 frame of queries.  km = 1e4 (the bias below the rounding of a score) is the plain read;
    km = 3 takes the cluster from the queries far from its centre - 49 of 80 select other rows, 45 still overflow.  Expected in fp64 from
    the engine's own centres (each within 1e-4 of its row's best query), as test_memory_read_km_matches_fp64_oracle."""
    b = L.bank(name)
    mk, mv, qk = b["mk"], b["mv"], b["qk"]
    N, Q = mk.shape[0], qk.shape[0]
    r = Read(name, top_k, sigma)
    r.check_form(N)
    assert (r.cen >= 0).all() and (r.cen < Q).all()
    S = O.affinity_logits(mk.double(), qk.double())
    assert float((S.max(1).values - S.gather(1, r.cen[0][:, None])[:, 0]).max()) <= 1e-4
    B, _ = km_oracle.biased_logits(mk.double(), qk.double(), *L.KM_FRAME, sigma, centres=r.cen)
    oracle = km_oracle.read_from_logits(B, mv.double(), top_k, return_gap=True)
    check_against(r, oracle, N, lambda qs: check_own_biased(B, mv, r.idx, r.w, r.ro, qs), f"{name} top_k={top_k} km={sigma:g}")
    assert torch.equal(Read(name, top_k, sigma).sets, r.sets), "a second read selected other rows"
    plain = Read(name, top_k)
    differ = (plain.sets != r.sets).any(1)
    print(f"{name} km={sigma:g}: {int(differ.sum())} of {Q} queries select other rows than the plain read")
    vals = torch.topk(S, top_k + 1, dim=0).values
    clear = vals[top_k - 1] - vals[top_k] > 1e-4
    assert (not differ[clear].any()) if sigma == 1e4 else differ.float().mean() > 0.5


def test_split_read_of_overflowing_lists_is_the_merged_one():
    """k = 2 and neither idx nor w (the read the engine runs: the selection stays in scratch, gather_readout_kernel reads it) against the
    read with them, which test_overflowing_lists_match_oracle[split-top50] holds against the oracle"""
    whole, split = Read("split", 50), Read("split", 50, outputs=False)
    assert whole.intact and split.intact
    assert torch.isfinite(split.ro).all() and torch.isnan(split.w).all()          # every read-out element written, no idx / w touched
    err = float((split.ro - whole.ro).abs().max() / whole.ro.abs().max())
    print(f"split against merged read-out of overflowing lists: max relative difference {err:.2e}")
    assert err < 2e-5, err
