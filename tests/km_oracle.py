"""The kernelized memory read (reference ``EvalMemoryReader(top_k, km)``, model/propagation/prop_net.py:33-51,74-106) restated in the log
domain, for tests and for tools/gen_golden_km.py.  Nothing under ``oracle/`` knows ``km``; a test switches this read in for
``oracle.stcn_oracle.memory_read`` while it runs.

The reference takes, for every memory row n, the query it matches best (``affinity.max(2)[1]``, :94), centres a Gaussian of standard
deviation ``km`` on that query's position and cuts ``exp(S - max) * g`` to its ``top_k`` best before normalising (:49-57).  With
    B[n, q] = S[n, q] - ((y_q - cy_n)^2 + (x_q - cx_n)^2) / (2 km^2)
that product is ``exp(B - max)``: monotone in B, so the selection is the top-k of B and the weights are the softmax of B over the selected
rows.  Where the reference's product underflows to zero (B more than ~87 below the column maximum) it ranks zeros arbitrarily and gives
them weight zero; here such rows keep their order and a weight below 1e-37 - the same read-out.

The queries may be several whole frames (a decode group of the engine): frame f owns the queries [f * h16 * w16, (f + 1) * h16 * w16) and
is read as the reference reads one frame - its own centres, its own Gaussian."""
import torch

from oracle import stcn_oracle as O


def biased_logits(mk, qk, h16, w16, km, centres=None):
    """B [N, Q] and the centres [frames, N] it was built from (``centres`` given: those instead of the argmax)."""
    hw16 = h16 * w16
    S = O.affinity_logits(mk, qk)
    assert S.shape[1] % hw16 == 0, (S.shape, h16, w16)
    if centres is None:
        centres = torch.stack([S[:, f:f + hw16].argmax(1) for f in range(0, S.shape[1], hw16)])
    pos = torch.arange(hw16)
    y, x = (pos // w16)[None, :], (pos % w16)[None, :]
    for f in range(S.shape[1] // hw16):
        c = centres[f].long()
        d2 = (y - (c // w16)[:, None]) ** 2 + (x - (c % w16)[:, None]) ** 2
        S[:, f * hw16:(f + 1) * hw16] -= d2.to(S.dtype) / (2.0 * km * km)
    return S, centres


def read_from_logits(B, mv, top_k, return_gap=False):
    """Cut, softmax and read-out of ``oracle.stcn_oracle.memory_read`` on given scores B [N, Q]."""
    kk = min(top_k + 1, B.shape[0]) if return_gap else top_k
    vals, idx = torch.topk(B, kk, dim=0)
    gap = (vals[top_k - 1] - vals[top_k]) if kk > top_k else torch.full((B.shape[1],), float("inf"))
    vals, idx = vals[:top_k], idx[:top_k]
    e = torch.exp(vals - vals[0:1])
    w = (e / e.sum(0, keepdim=True)).t().contiguous()
    idx = idx.t().contiguous()
    out = torch.einsum("qj,kqjc->kqc", w, mv[:, idx])
    return (idx, w, out, gap) if return_gap else (idx, w, out)


def memory_read(h16, w16, km):
    """A drop-in for ``oracle.stcn_oracle.memory_read`` (same arguments, same returns, the cut is ``O.TOP_K`` when it is called) that reads
    frames of h16 x w16 queries with the Gaussian of standard deviation ``km``."""

    def read(mk, mv, qk, return_gap=False, centres=None):
        return read_from_logits(biased_logits(mk, qk, h16, w16, km, centres)[0], mv, O.TOP_K, return_gap)

    return read
