"""Sequence fixtures at another ``top_k`` than 50, captured from the REAL reference (build container only) -> tests/golden/seqT20*.npz and
their reference-vs-itself rows -> tests/golden/selfnoise_topk.npz.

Everything is ``oracle/gen_golden.py``'s: its import shims for the reference, its ``seq_case`` (reference and oracle side by side, fixture
arrays, oracle-vs-reference report) and its ``self_noise`` (the reference at 1 / 2 / 4 / 8 intra-op threads).  This file only builds the
reference's ``PropagationNetwork(top_k=K)`` (model/propagation/prop_net.py:141) on the seed-0 weight recipe and sets the oracle's cut,
the module global ``oracle.stcn_oracle.TOP_K``, to the same K while a case runs.  Each fixture records its ``<tag>.top_k``.

No ``top_k=1`` sequence: one flipped row moves a probability by 0.46 there, and the reference differs from itself by 20 px on an
8-frame clip - nothing a sequence test could be held to.  tests/test_gpu_topk.py covers ``top_k=1`` on the read alone.

Run:  python tools/gen_golden_topk.py [--only=seqT20s]
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402  (the reference import shims come with it)
from oracle import stcn_oracle as O  # noqa: E402

TOPK_CASES = {
    # the seqA script (fusion, and a re-annotated frame) at the cut STCN checkpoints are evaluated with
    "seqT20": dict(top_k=20, H=128, W=160, k=1, T=12, mem_freq=5, script=[(0, 0), (8, 8), (7, 8)]),
    # a frame of 6 x 7 = 42 keys: fewer than 50, so it exists only below the default cut (the reference itself raises there at top_k=50)
    "seqT20s": dict(top_k=20, H=96, W=112, k=1, T=8, mem_freq=2, script=[(0, 0), (5, 5)]),
    # three objects through the scribble path (the seqC script): one merge per query, one gather wave per (query, object)
    "seqT20k3": dict(top_k=20, H=128, W=160, k=3, T=8, mem_freq=2, script=[(0, 0), (5, 5)]),
}


def load_reference_topk(top_k, seed=0):
    """The reference's networks under the weight recipe, its memory readers built for ``top_k``."""
    with contextlib.redirect_stdout(io.StringIO()):
        net, fus = G.RefNet(top_k=top_k).eval(), G.RefFus().eval()
    psd = G.synth.recipe_state_dict(G.PropagationNetwork(), seed)
    fsd = G.synth.recipe_state_dict(G.FusionNet(), seed)
    net.load_state_dict(psd, strict=True)
    fus.load_state_dict(fsd, strict=True)
    assert net.memory.top_k == top_k
    return net, fus, psd, fsd


def main():
    only = [a.split("=")[1] for a in sys.argv if a.startswith("--only=")]
    noise_path = os.path.join(G.GOLD, "selfnoise_topk.npz")
    noise = dict(np.load(noise_path)) if only and os.path.exists(noise_path) else {}
    default_cut = O.TOP_K
    for tag, c in TOPK_CASES.items():
        if only and tag not in only:
            continue
        net, fus, psd, fsd = load_reference_topk(c["top_k"])
        O.TOP_K = c["top_k"]
        try:
            out = {}
            rep = G.seq_case(tag, net=net, fus=fus, psd=psd, fsd=fsd, out=out, **c)
            out[f"{tag}.top_k"] = np.array(c["top_k"])
            np.savez_compressed(os.path.join(G.GOLD, f"{tag}.npz"), **out)
            print(tag, rep, flush=True)
            noise[tag] = G.self_noise(tag, net=net, fus=fus, **c)
            print("selfnoise", tag, noise[tag].tolist(), flush=True)
        finally:
            O.TOP_K = default_cut
    np.savez_compressed(noise_path, **noise)


if __name__ == "__main__":
    main()
