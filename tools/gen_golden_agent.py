"""Capture a golden vector of the REAL reference actor-critic agent (build container only) -> tests/golden/agent.npz.

Imports the reference's ``models/rl_agent.py`` over the stub ``torchvision`` of ``oracle/_stub`` (own ResNet-18 with torchvision's attribute
names; the branch wiring, the embedding branch, the merge and the two heads are the reference's own code).  Weights come from
``eva_vos_amd.synth.recipe_state_dict(own module, seed=5)`` and are loaded strictly into both modules; the inputs - 3 embeddings
[3,256,64,64] drawn normal, 3 thresholded masks [3,3,224,224] - are regenerated from a Philox stream (``inputs()``; the test imports it).
Stored: ``logits`` [3,2], ``value`` [3,1], and the reference's ``state_dict`` ``names`` and ``shapes``; inputs and weights never.

Run:  python tools/gen_golden_agent.py --reference=<checkout of the reference>
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT_SEED = 5


def inputs(n=3, seed=13):
    g = np.random.Generator(np.random.Philox(key=[seed, 256]))
    emb = torch.from_numpy(g.normal(0, 1, (n, 256, 64, 64)).astype(np.float32))
    msk = torch.from_numpy((g.uniform(0, 1, (n, 1, 224, 224)) > 0.6).astype(np.float32)).expand(-1, 3, -1, -1)
    return emb, msk.contiguous()


def main():
    ref_root = [a.split("=", 1)[1] for a in sys.argv if a.startswith("--reference=")] or [os.environ.get("EVA_VOS_REFERENCE", "")]
    if not ref_root[0] or not os.path.isdir(ref_root[0]):
        sys.exit("give the checkout of the reference: --reference=PATH (or EVA_VOS_REFERENCE)")
    sys.path[:0] = [os.path.join(ROOT, "oracle", "_stub"), ref_root[0], ROOT]
    torch.set_grad_enabled(False)
    from models.rl_agent import ActorCritic as RefActorCritic      # the reference

    from eva_vos_amd import synth
    from eva_vos_amd.agent import ActorCritic
    mine = ActorCritic(out_dim=2).eval()
    sd = synth.recipe_state_dict(mine, seed=WEIGHT_SEED)
    ref = RefActorCritic(out_dim=2, arch="resnet18", dropout=0).eval()
    ref.load_state_dict(sd, strict=True)              # names and shapes equal the reference's
    mine.load_state_dict(sd, strict=True)
    emb, msk = inputs()
    logits, value = ref(emb, msk)
    own_logits, own_value = mine(emb, msk)
    print(len(ref.state_dict()), "tensors,", sum(v.numel() for v in ref.parameters()) / 1e6, "M parameters")
    print("logits", logits.tolist(), "value", value.flatten().tolist())
    print("max |ref - own| =", float(max((logits - own_logits).abs().max(), (value - own_value).abs().max())),
          "scale", float(max(logits.abs().max(), value.abs().max())))
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "agent.npz"), logits=logits.numpy(), value=value.numpy(),
                        names=np.array(list(ref.state_dict().keys())),
                        shapes=np.array([",".join(map(str, v.shape)) for v in ref.state_dict().values()]))


if __name__ == "__main__":
    main()
