"""Host-only helpers of test_memread_lists.py / test_gpu_memread_lists.py: how long the pass-2 candidate lists of the top-k memory read
(eva_vos_amd/csrc/memread.hip) get on a given bank, restated in fp64 from the rules the kernels state, and banks that make them overflow.
No GPU, no kernel output, no call into the library: test_memread_lists.py pins restated_plan to the library's planner.

The rules restated (memread.hip):
  * the plan: 64-row steps; pass 1 visits every ss-th step (ss = 1 / 2 / 4 / 8 from 0 / 96 / 192 / 768 steps); either pass splits its
    steps into as many chunks as one round of co-resident workgroups holds (1024 / 768 workgroups over ceil(Q / 64) query blocks), at most
    8 / 32, of spc1 / spc2 steps each;
  * pass 1 keeps, per query and pass-1 chunk, 64 running maxima: group = row % 64 (in another order), over the sampled steps of the chunk,
    rows beyond the bank -inf;
  * threshold_kernel: tau = the top_k-th largest finite group maximum, one fp32 key down, minus 1.5 * RESCORE_W (-inf with fewer than
    top_k finite maxima);
  * pass 2 walks every step and appends every score > tau to the list of its (query, pass-2 chunk), CAP2 = 64 entries in LDS.  An append
    that finds the list full is kept back; the list is cut to its best top_k, the query's threshold rises to the top_k-th, the kept-back
    appends above it are replayed (and may fill the list again).  At the end of the chunk a list longer than top_k is cut the same way.

The banks (build_bank): a quiet seeded background - keys 0.1 * randn, so |mk|^2 / 2 costs a background row 0.3 - in which a cluster of rows
a_i * u, |u| = 3, stands out for every query pointed at u (qk = u + 0.05 * randn): their scores (9 a - 4.5 a^2) / 4 are spread evenly over
[0.4, 1.0], adjacent ones 1e-3 .. 5e-3 apart, the best background row of such a query near 0.2.  The keys carry no noise of their own: the
1e-3 noise of the older rising-scores bank leaves some queries a gap of 5e-6 at the cut on these banks.  Queries that are not pointed at u
are 4 * randn with their component along u set to -0.1 u: the cluster scores below -0.08 for them, their top_k are background rows
spread like those of a randn bank (a 0.1 * randn background under a small query would pack them: a fifth of the queries near-tied)."""
import math

import numpy as np
import torch

CAP2, TOPK, RESCORE_W, HROWS = 64, 50, 1e-4, 64
PLAN_KEYS = ("steps", "ss", "ns", "nc1", "spc1", "nc2", "spc2")


def restated_plan(N, Q):
    steps, qblocks = -(-N // HROWS), -(-Q // 64)
    ss = 8 if steps >= 768 else 4 if steps >= 192 else 2 if steps >= 96 else 1
    ns = -(-steps // ss)

    def chunks(st, resident, hi):
        nc = min(max(resident // qblocks, 1), hi, st)
        spc = -(-st // nc)
        return -(-st // spc), spc

    (nc1, spc1), (nc2, spc2) = chunks(ns, 1024, 8), chunks(steps, 768, 32)
    return dict(steps=steps, ss=ss, ns=ns, nc1=nc1, spc1=spc1, nc2=nc2, spc2=spc2)


def scores(mk, qk):
    """S [N, Q] in fp64 = (mk.qk - |mk|^2 / 2) / 4: the reference's affinity without its per-query constant, as the kernels score"""
    mk, qk = mk.double(), qk.double()
    return (mk @ qk.t() - 0.5 * (mk * mk).sum(1, keepdim=True)) / 4.0


def thresholds(S, top_k, plan):
    """tau [Q] of scores S [N, Q] (any per-query constant in S shifts tau alike)"""
    N, Q = S.shape
    pad = torch.full((plan["steps"] * HROWS - N, Q), -math.inf, dtype=S.dtype)
    sampled = torch.cat([S, pad]).view(plan["steps"], HROWS, Q)[::plan["ss"]]
    assert sampled.shape[0] == plan["ns"]
    G = torch.cat([sampled[c * plan["spc1"]:(c + 1) * plan["spc1"]].amax(0) for c in range(plan["nc1"])])      # [nc1 * 64, Q]
    if G.shape[0] < top_k:
        return torch.full((Q,), -math.inf, dtype=S.dtype)
    kth = torch.topk(G, top_k, dim=0).values[top_k - 1]
    down = np.nextafter(kth.numpy().astype(np.float32), np.float32(-np.inf)) - np.float32(1.5 * RESCORE_W)
    return torch.where(torch.isfinite(kth), torch.from_numpy(down.astype(np.float64)), torch.full_like(kth, -math.inf))


def list_sizes_of_scores(S, top_k, plan=None):
    """raw number of scores above tau per (query, pass-2 chunk) [Q, nc2], and tau [Q]"""
    N, Q = S.shape
    plan = plan or restated_plan(N, Q)
    tau = thresholds(S, top_k, plan)
    per_step = torch.zeros(plan["nc2"] * plan["spc2"], Q, dtype=torch.long)
    above = (S > tau[None, :])
    pad = torch.zeros(plan["steps"] * HROWS - N, Q, dtype=torch.bool)
    per_step[:plan["steps"]] = torch.cat([above, pad]).view(plan["steps"], HROWS, Q).sum(1)
    return per_step.view(plan["nc2"], plan["spc2"], Q).sum(1).t().contiguous(), tau


def list_sizes(mk, qk, top_k, block=256):
    """[Q, nc2] raw pass-2 candidates of every (query, chunk), queries in blocks (the fp64 scores of a block: N x block)"""
    plan = restated_plan(mk.shape[0], qk.shape[0])
    return torch.cat([list_sizes_of_scores(scores(mk, qk[q:q + block]), top_k, plan)[0] for q in range(0, qk.shape[0], block)])


def walk_chunk(s, row0, tau, top_k, raise_tau=True, lose_full=False):
    """One (query, pass-2 chunk) list as affinity_tile_kernel<true> keeps it: s = fp64 scores of the chunk's rows (first row row0, a
    multiple of 64).  Returns (rows the chunk hands to the merge, number of cut-backs before the write-out, appends that passed the filter
    after the first cut-back).  raise_tau=False: the cut-back leaves the threshold alone.  lose_full=True: an append that finds the list
    full is lost (no cut-back, no replay)."""
    lst, t, cuts, late = [], tau, 0, 0
    cut = lambda l: sorted(l, key=lambda e: -e[0])[:top_k]          # noqa: E731
    for st in range(0, len(s), HROWS):
        drop = []
        for r in range(st, min(st + HROWS, len(s))):
            if s[r] > t:
                late += cuts > 0
                (lst if len(lst) < CAP2 else drop).append((s[r], row0 + r))
        while drop and not lose_full:
            lst, cuts = cut(lst), cuts + 1
            if raise_tau:
                t = max(t, lst[-1][0])
            again = []
            for e in drop:
                if e[0] > t:
                    late += 1
                    (lst if len(lst) < CAP2 else again).append(e)
            drop = again
    return sorted(r for _, r in cut(lst)), cuts, late


# ------------------------------------------------------------------------------------------ banks
def hidden_rows(N, Q, chunk, limit=None):
    """every row of the unsampled steps (step % ss != 0) of pass-2 chunk `chunk` (negative: from the end), the first `limit` of them"""
    p = restated_plan(N, Q)
    c = chunk % p["nc2"]
    steps = [s for s in range(c * p["spc2"], min(p["steps"], (c + 1) * p["spc2"])) if s % p["ss"]]
    rows = [r for s in steps for r in range(s * HROWS, min(N, (s + 1) * HROWS))]
    return rows[:limit], c


def column_rows(N, Q, chunk):
    """ss = 1: rows with row % 64 < 40 of the steps of pass-2 chunk `chunk` that lie inside the pass-1 chunk of its first step"""
    p = restated_plan(N, Q)
    assert p["ss"] == 1
    first = chunk * p["spc2"]
    steps = [s for s in range(first, min(p["steps"], first + p["spc2"])) if s // p["spc1"] == first // p["spc1"]]
    return [s * HROWS + r for s in steps for r in range(40) if s * HROWS + r < N], chunk


def build_bank(N, Q, k, rows, order, pointed, seed, tied=None):
    """mk [N, 64], mv [k, N, 512], qk [Q, 64] (fp32): the background of the module docstring, the cluster on `rows` (a sorted list) in
    `order` = rising / falling / shuffled scores along the rows, the queries `pointed` (indices) at u.
    tied: every cluster key 0.5 u; "a": one value row behind all of them, "b": the distinct value rows of the draw."""
    g = torch.Generator().manual_seed(seed)
    mk, qk, mv = 0.1 * torch.randn(N, 64, generator=g), 4.0 * torch.randn(Q, 64, generator=g), torch.randn(k, N, 512, generator=g)
    u = torch.randn(64, generator=g).double()
    u = u / u.norm() * 3.0
    n = len(rows)
    a = 1.0 - torch.sqrt(1.0 - 8.0 * torch.linspace(0.4, 1.0, n, dtype=torch.float64) / 9.0)     # (9 a - 4.5 a^2) / 4 = 0.4 .. 1.0
    if order == "falling":
        a = a.flip(0)
    elif order == "shuffled":
        a = a[torch.randperm(n, generator=g)]
    else:
        assert order == "rising", order
    if tied:
        a = torch.full_like(a, 0.5)
    rows = torch.as_tensor(rows)
    mk[rows] = (a[:, None] * u[None, :]).float()
    if tied == "a":
        mv[:, rows] = mv[:, rows[:1]]
    qd = qk.double()
    qk = (qd - (qd @ u)[:, None] * u[None, :] / 9.0 - 0.1 * u[None, :]).float()
    pointed = torch.as_tensor(pointed)
    qk[pointed] = (u[None, :] + 0.05 * torch.randn(len(pointed), 64, generator=g).double()).float()
    return mk, mv, qk


#        name: (kind, order, N, Q, k, chunk, cluster rows at most, pointed queries, list bound the case is listed for)
EVERY = lambda Q: list(range(Q))                                     # noqa: E731
BANK_SPECS = {
    "hidden-rising": ("hidden", "rising", 8100, 97, 1, 13, None, EVERY, CAP2),
    "many-rising": ("hidden", "rising", 32400, 97, 1, -1, None, EVERY, 4 * CAP2),
    "many-falling": ("hidden", "falling", 32400, 97, 1, -1, None, EVERY, 4 * CAP2),
    "many-shuffled": ("hidden", "shuffled", 32400, 97, 1, -1, None, EVERY, 4 * CAP2),
    "many-ss8": ("hidden", "shuffled", 49100, 97, 1, 17, 600, EVERY, 4 * CAP2),
    "column-rising": ("column", "rising", 5000, 200, 2, 11, None, EVERY, CAP2),
    "mixed": ("hidden", "rising", 8100, 97, 1, 13, None, lambda Q: list(range(0, Q, 2)), CAP2),
    "tied-a": ("hidden", "tied-a", 8100, 97, 1, 13, None, EVERY, CAP2),
    "tied-b": ("hidden", "tied-b", 8100, 97, 1, 13, None, EVERY, CAP2),
    "km-frame": ("hidden", "rising", 8100, 80, 1, 13, None, EVERY, CAP2),
    "split": ("hidden", "rising", 8100, 97, 2, 13, None, EVERY, CAP2),
}
_BANKS = {}


def order_of(name):
    return BANK_SPECS[name][1]


def bank(name):
    """dict(mk, mv, qk, rows, chunk, pointed, bound, plan) of a bank of BANK_SPECS: built once, shared, never written to"""
    if name not in _BANKS:
        kind, order, N, Q, k, chunk, limit, pointed, bound = BANK_SPECS[name]
        rows, chunk = column_rows(N, Q, chunk) if kind == "column" else hidden_rows(N, Q, chunk, limit)
        tied = order[5:] if order.startswith("tied") else None
        mk, mv, qk = build_bank(N, Q, k, rows, "rising" if tied else order, pointed(Q), seed=1000 + N + Q, tied=tied)
        _BANKS[name] = dict(mk=mk, mv=mv, qk=qk, rows=rows, chunk=chunk, pointed=pointed(Q), bound=bound, plan=restated_plan(N, Q),
                            order=order, tied=tied)
    return _BANKS[name]


#        (bank, top_k, sigma of the kernelized read over one 8 x 10 frame of queries or None): the cases of both test files
KM_FRAME = (8, 10)
CASES = [("hidden-rising", 50, None), ("hidden-rising", 20, None), ("hidden-rising", 1, None), ("many-rising", 50, None),
         ("many-falling", 50, None), ("many-shuffled", 50, None), ("many-ss8", 50, None), ("column-rising", 50, None), ("mixed", 50, None),
         ("tied-a", 50, None), ("tied-a", 20, None), ("tied-b", 50, None), ("tied-b", 20, None), ("km-frame", 50, 1e4), ("km-frame", 50, 3.0),
         ("split", 50, None)]
CASE_IDS = [f"{n}-top{t}" + (f"-km{s:g}" if s else "") for n, t, s in CASES]
_SCORES = {}


def case_scores(name, sigma=None):
    """fp64 scores [N, Q] a case is judged by on the host: scores() of its bank, under the kernelized read the biased scores of
    tests/km_oracle.py from the fp64 centres.  Kept for the three banks every test of a file comes back to, recomputed for the large ones."""
    if (name, sigma) in _SCORES:
        return _SCORES[name, sigma]
    b = bank(name)
    if sigma:
        import km_oracle
        S = km_oracle.biased_logits(b["mk"].double(), b["qk"].double(), *KM_FRAME, sigma)[0]
    else:
        S = scores(b["mk"], b["qk"])
    if S.shape[0] <= 8100:
        _SCORES[name, sigma] = S
    return S


# ------------------------------------------------------------------------------------------ the fixed banks of the older tests
def older_banks():
    """(label, mk, qk, top_k) of every fixed bank of test_gpu_kernels.py / test_gpu_topk.py, drawn as those tests draw them"""
    def rand(N, Q, scale, seed):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(N, 64, generator=g) * scale, torch.randn(Q, 64, generator=g) * scale

    for N, Q, scale in ((160, 80, 1.0), (1620, 333, 1.0), (5000, 200, 0.5), (50, 16, 1.0), (32400, 97, 1.0)):
        yield (f"random {N} x {Q}", *rand(N, Q, scale, N + Q), 50)
    yield ("random 84240 x 1620 (config 3, T = 52)", *rand(84240, 1620, 0.8, 84240 + 1620 + 1), 50)
    u = torch.randn(64, generator=torch.Generator().manual_seed(3))
    u = u / u.norm() * 3.0
    mk = torch.linspace(0.0, 0.9, 4000)[:, None] * u[None, :] + 1e-3 * torch.randn(4000, 64, generator=torch.Generator().manual_seed(4))
    qk = u[None, :].repeat(48, 1) + 0.05 * torch.randn(48, 64, generator=torch.Generator().manual_seed(5))
    for top_k in (50, 20, 1):
        yield (f"rising scores 4000 x 48, top_k {top_k}", mk, qk, top_k)
    g = torch.Generator().manual_seed(9)
    mk = torch.randn(160, 64, generator=g).repeat(4, 1)
    torch.randn(1, 160, 512, generator=g)
    yield ("every row x 4 (exact ties) 640 x 32", mk, torch.randn(32, 64, generator=g), 50)
    g = torch.Generator().manual_seed(21)
    single, base = torch.randn(300, 64, generator=g), torch.randn(300, 64, generator=g)
    trip = torch.cat([base * (1 + 1e-7 * torch.randn(300, 1, generator=g)) for _ in range(3)], 0)
    mk = torch.cat([single, trip], 0)[torch.randperm(1200, generator=g)]
    yield ("near-tie triplets 1200 x 256", mk, torch.randn(256, 64, generator=g), 50)
