"""CPU: the cases of test_gpu_memread_lists.py do what they are listed for - judged on the host in fp64 by tests/memread_lists.py, which
restates the plan, pass 1's grouping and the threshold rule of memread.hip and never sees a kernel's output.

  * restated_plan is the library's memread_plan (stcn_memread_plan) on every case and on the sweep of test_memread_plan.py;
  * every case fills a pass-2 candidate list beyond CAP2 = 64 entries (beyond 4 * CAP2 the "many" ones): the cut-back inside the kernel,
    the raised threshold and the replay of the kept-back appends run;
  * every case but the tied ones is clear-cut: at least 96 % of its queries have 1e-4 or more between the top_k-th and the next score;
  * every rising case can fail: a list that loses the appends that found it full hands the merge a wrong top_k for every overflowing
    query, and the same walk without that fault hands it the right one;
  * the shuffled cases need the raised threshold: without it more than 64 further appends pass the filter after the first cut-back.
The last test prints the same figures for every fixed bank of the older memory-read tests: none of their lists reaches 64 entries."""
import pytest
import torch

import memread_lists as L
from test_memread_plan import NS, QS, plan

cases = pytest.mark.parametrize("name,top_k,sigma", L.CASES, ids=L.CASE_IDS)


def overflowing(name, top_k, sigma):
    """(S, tau, list sizes [Q, nc2], the queries whose list of the cluster's chunk is longer than CAP2)"""
    S = L.case_scores(name, sigma)
    ls, tau = L.list_sizes_of_scores(S, top_k)
    return S, tau, ls, torch.nonzero(ls[:, L.bank(name)["chunk"]] > L.CAP2).flatten().tolist()


def chunk_rows(b):
    r0 = b["chunk"] * b["plan"]["spc2"] * L.HROWS
    return r0, min(b["mk"].shape[0], r0 + b["plan"]["spc2"] * L.HROWS)


def test_restated_plan_is_the_librarys():
    shapes = {spec[2:4] for spec in L.BANK_SPECS.values()} | {(N, Q) for N in NS for Q in QS}
    for N, Q in sorted(shapes):
        assert L.restated_plan(N, Q) == plan(N, Q), (N, Q)


@cases
def test_case_fills_a_list_beyond_its_capacity(name, top_k, sigma):
    b = L.bank(name)
    S, tau, ls, over = overflowing(name, top_k, sigma)
    Q = S.shape[1]
    longest = int(ls.max())
    print(f"{name} top_k={top_k} km={sigma}: plan {b['plan']}; {len(b['rows'])} cluster rows in chunk {b['chunk']}; candidates per query mean "
          f"{float(ls.sum(1).float().mean()):.0f} max {int(ls.sum(1).max())}; longest list {longest}; {len(over)} of {Q} queries overflow")
    assert longest > b["bound"], (longest, b["bound"])
    assert int(ls.argmax()) % ls.shape[1] == b["chunk"]
    if name == "mixed":
        # overflowing and short lists side by side in every 16-query wave, the ragged last one (query 96 alone) overflowing
        short = sorted(set(range(Q)) - set(over))
        assert int(ls[short].max()) < L.CAP2 // 2, int(ls[short].max())
        for q0 in range(0, Q, 16):
            n = sum(q0 <= q < q0 + 16 for q in over)
            assert (6 <= n <= 10) if q0 + 16 <= Q else n >= 1, (q0, n)
    elif sigma is None:
        assert len(over) == Q
    else:
        assert len(over) >= Q // 2, len(over)
    if name.startswith("many-rising"):
        p = b["plan"]
        assert b["chunk"] == p["nc2"] - 1 and b["rows"][-1] == S.shape[0] - 1 and S.shape[0] % L.HROWS == 16      # the ragged last step


@cases
def test_case_is_clear_cut(name, top_k, sigma):
    S = L.case_scores(name, sigma)
    v = torch.topk(S, top_k + 1, dim=0).values
    gap = v[top_k - 1] - v[top_k]
    clear = float((gap >= 1e-4).float().mean())
    print(f"{name} top_k={top_k} km={sigma}: {clear:.3f} of the queries clear-cut, smallest gap {float(gap.min()):.1e}")
    if L.bank(name)["tied"]:
        assert float(gap.max()) == 0.0          # every query: the cut falls inside the tied scores
    else:
        assert clear >= 0.96, clear


def test_the_narrow_kernel_changes_the_selection():
    """km = 3 takes the cluster from the queries far from its centre: they select background rows"""
    sel = [torch.topk(L.case_scores("km-frame", s), 50, dim=0).indices.sort(0).values for s in (None, 1e4, 3.0)]
    differ = [int((s != sel[0]).any(0).sum()) for s in sel[1:]]
    print(f"km-frame: queries that select other rows than the plain read at km = 1e4: {differ[0]}, at km = 3: {differ[1]} of 80")
    assert differ[0] == 0 and differ[1] >= 40


def merged(S, tau, q, b, top_k, **fault):
    """rows query q selects when the list of the cluster's chunk is kept by walk_chunk(**fault): every other candidate reaches the merge"""
    r0, r1 = chunk_rows(b)
    s = S[:, q]
    kept, cuts, late = L.walk_chunk(s[r0:r1].tolist(), r0, float(tau[q]), top_k, **fault)
    cand = torch.nonzero(s > tau[q]).flatten()
    cand = torch.cat([cand[(cand < r0) | (cand >= r1)], torch.as_tensor(kept, dtype=torch.long)])
    return sorted(cand[torch.topk(s[cand], top_k).indices].tolist()), cuts, late


@pytest.mark.parametrize("name,top_k,sigma", [c for c in L.CASES if L.order_of(c[0]) == "rising"],
                         ids=[i for c, i in zip(L.CASES, L.CASE_IDS) if L.order_of(c[0]) == "rising"])
def test_rising_case_can_fail(name, top_k, sigma):
    b = L.bank(name)
    S, tau, ls, over = overflowing(name, top_k, sigma)
    wrong = cuts = 0
    for q in over:
        true = sorted(torch.topk(S[:, q], top_k).indices.tolist())
        good, c, _ = merged(S, tau, q, b, top_k)
        assert good == true, q                                      # the walk as the kernel states it
        bad, _, _ = merged(S, tau, q, b, top_k, lose_full=True)
        wrong, cuts = wrong + (bad != true), cuts + c
    print(f"{name} top_k={top_k} km={sigma}: {len(over)} overflowing queries, {cuts / len(over):.1f} cut-backs each; "
          f"appends to a full list lost: {wrong} wrong selections")
    assert over and wrong == len(over)


@pytest.mark.parametrize("name", ["many-shuffled", "many-ss8"])
def test_shuffled_case_needs_the_raised_threshold(name):
    b = L.bank(name)
    S, tau, ls, over = overflowing(name, 50, None)
    figures = []
    for q in over[::4]:
        true = sorted(torch.topk(S[:, q], 50).indices.tolist())
        good, cuts, late = merged(S, tau, q, b, 50)
        flat, cuts0, late0 = merged(S, tau, q, b, 50, raise_tau=False)
        assert good == true and flat == true, q                     # more work, the same rows
        assert late0 > L.CAP2 and late0 > 2 * late and cuts0 > cuts, (q, late0, late, cuts0, cuts)
        figures.append((late, cuts, late0, cuts0))
    f = torch.tensor(figures, dtype=torch.float64).mean(0).tolist()
    print(f"{name}: appends after the first cut-back / cut-backs per query: {f[0]:.0f} / {f[1]:.1f}; threshold never raised: {f[2]:.0f} / {f[3]:.1f}")


def test_lists_of_the_older_fixed_banks_stay_short():
    """Statements of fact about the banks of test_gpu_kernels.py and test_gpu_topk.py, for the log: the cut-back inside the kernel does
    not run on any of them (the write-out select does where a list exceeds top_k < 50)."""
    for label, mk, qk, top_k in L.older_banks():
        p = L.restated_plan(mk.shape[0], qk.shape[0])
        ls = L.list_sizes(mk, qk, top_k)
        per_q = ls.sum(1).float()
        print(f"{label}: ss {p['ss']}, spc2 {p['spc2']}; candidates per query mean {float(per_q.mean()):.0f} max {int(per_q.max())}; "
              f"longest (query, chunk) list {int(ls.max())}")
