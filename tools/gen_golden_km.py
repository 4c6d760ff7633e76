"""Sequence fixtures of the KERNELIZED memory read, captured from the REAL reference (build container only) -> tests/golden/seqKM*.npz and
their reference-vs-itself rows -> tests/golden/selfnoise_km.npz.

The reference's ``PropagationNetwork.__init__`` hands ``km=None`` to its ``EvalMemoryReader`` (model/propagation/prop_net.py:149), but the
reader is a plain attribute: ``net.memory.km = 5.6`` switches the Gaussian of prop_net.py:92-99 on with unchanged weights.  Everything else
is ``oracle/gen_golden.py``'s, as in tools/gen_golden_topk.py: ``seq_case`` (reference and oracle side by side, fixture arrays, report)
and ``self_noise`` (the reference at 1 / 2 / 4 / 8 intra-op threads).  Two things are swapped while a case runs:
  * ``make_gaussian`` (prop_net.py:36-37) calls ``.cuda()`` on its grids; the capture runs on the CPU, so ``torch.Tensor.cuda`` is the
    identity for that time;
  * ``seq_case`` runs the oracle beside the reference for its report; the oracle's ``memory_read`` is the km-aware restatement of
    tests/km_oracle.py (log domain, closed over the frame's key grid and km) for that time.  Nothing under ``oracle/`` changes.
Each fixture records its ``<tag>.km`` and ``<tag>.top_k``.

Run:  python tools/gen_golden_km.py [--only=seqKMn]
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402  (the reference import shims come with it)
from oracle import stcn_oracle as O  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import km_oracle  # noqa: E402
from gen_golden_topk import load_reference_topk  # noqa: E402

KM_CASES = {
    # the seqA script (fusion, and a re-annotated frame) at the sigma the reference's callers use
    "seqKM": dict(km=5.6, top_k=50, H=128, W=160, k=1, T=12, mem_freq=5, script=[(0, 0), (8, 8), (7, 8)]),
    # three objects through the scribble path (the seqC script) at the STCN cut
    "seqKMk3": dict(km=5.6, top_k=20, H=128, W=160, k=3, T=8, mem_freq=2, script=[(0, 0), (5, 5)]),
    # a narrow kernel: the bias, not the affinity, decides the selection
    "seqKMn": dict(km=1.5, top_k=50, H=128, W=160, k=1, T=12, mem_freq=5, script=[(0, 0), (8, 8), (7, 8)]),
}


@contextlib.contextmanager
def km_capture(h16, w16, km, top_k):
    """While a case runs: ``.cuda()`` is the identity, the oracle cuts at ``top_k`` and reads through the km restatement."""
    saved = torch.Tensor.cuda, O.memory_read, O.TOP_K
    torch.Tensor.cuda = lambda self, *a, **kw: self
    O.memory_read, O.TOP_K = km_oracle.memory_read(h16, w16, km), top_k
    try:
        yield
    finally:
        torch.Tensor.cuda, O.memory_read, O.TOP_K = saved


def main():
    only = [a.split("=")[1] for a in sys.argv if a.startswith("--only=")]
    noise_path = os.path.join(G.GOLD, "selfnoise_km.npz")
    noise = dict(np.load(noise_path)) if only and os.path.exists(noise_path) else {}
    for tag, c in KM_CASES.items():
        if only and tag not in only:
            continue
        net, fus, psd, fsd = load_reference_topk(c["top_k"])
        net.memory.km = c["km"]
        with km_capture((c["H"] + 15) // 16, (c["W"] + 15) // 16, c["km"], c["top_k"]):
            out = {}
            rep = G.seq_case(tag, net=net, fus=fus, psd=psd, fsd=fsd, out=out, **c)
            out[f"{tag}.top_k"] = np.array(c["top_k"])
            out[f"{tag}.km"] = np.array(c["km"])
            np.savez_compressed(os.path.join(G.GOLD, f"{tag}.npz"), **out)
            print(tag, rep, flush=True)
            noise[tag] = G.self_noise(tag, net=net, fus=fus, **c)
            print("selfnoise", tag, noise[tag].tolist(), flush=True)
    np.savez_compressed(noise_path, **noise)


if __name__ == "__main__":
    main()
