"""The annotation-type agent of ``eva_vos`` on stock PyTorch-ROCm, and the device route of its - and the QNet's - mask input.

* ``ActorCritic``: own container of the reference's actor-critic network (``models/rl_agent.py:6-56``) in the configuration ``eva_vos`` runs:
  ``arch='resnet18'``, no cost branch.  A ResNet-18 branch over the 3x-repeated 224 x 224 mask (``qnet._Branch``), a pooled linear branch over
  the annotator's image embedding [B,256,64,64], concatenated -> 1024 features -> ``policy`` (out_dim logits) and ``value`` (1).  The
  ``state_dict`` names and shapes equal the reference's (126 tensors), so ``model.pth`` loads strictly.
* ``PPOAgent``: ``ppo/ppo_agent.py`` - eval mode, no grad, the action sampled from ``Categorical(logits)``.  The reference draws from torch's
  global generator; here the draw takes the session's own ``torch.Generator``, so a session is reproducible under its seed whatever runs
  beside it (and is not comparable draw for draw with the reference).
* ``masks_to_224``: the masks a round evaluated (uint8 [T,H,W] on the device) as network input [n,channels,224,224] fp32 in ONE launch
  (``stcn_masks_resize_nearest``, csrc/resize.hip) in place of ``.float()`` of the whole clip + ``interpolate`` + an ``expand`` that the first
  conv materialises.  ``masks_to_224_torch`` is that torch route, kept for comparison (tests, tools/eva_vos_cost.py).
"""
from __future__ import annotations

import ctypes as C
import threading

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .qnet import _Branch

ARCHS = ("resnet18",)
AVAIL_ACTIONS = ("3clicks", "mask")           # rl_agent_annotate's hard-coded avail_actions (interactions/mulitple_annotations.py:298)


class ActorCritic(nn.Module):
    def __init__(self, out_dim: int = 2, arch: str = "resnet18", dropout: float = 0.0, use_cost: bool = False):
        super().__init__()
        if arch not in ARCHS:
            raise ValueError(f"ActorCritic: arch {arch!r} is not built; supported: {', '.join(ARCHS)}")
        if use_cost:
            raise ValueError("ActorCritic: use_cost=True (the cost branch) is not built; supported: use_cost=False, what eva_vos runs")
        self.mask_branch = _Branch()
        self.embed_branch = nn.Sequential(nn.AdaptiveAvgPool2d(output_size=1), nn.Flatten(), nn.Linear(256, 512))
        self.dropout = nn.Dropout(dropout)
        self.policy = nn.Linear(1024, out_dim)
        self.value = nn.Linear(1024, 1)

    def forward(self, x_img, x_mask):
        """x_img: image embedding [B,256,h,w]; x_mask [B,3,224,224] -> (logits [B,out_dim], value [B,1])."""
        x = self.dropout(torch.cat((self.embed_branch(x_img), self.mask_branch(x_mask).flatten(1)), dim=1))
        return self.policy(x), self.value(x)


_DETERMINISTIC_CONVS = threading.Lock()


class PPOAgent:
    """``model_path``: a checkpoint of the reference (``model.pth``), loaded strictly; ``state_dict``: the weights themselves (recipe weights);
    neither: the module's own initialisation.
    The forward pass runs with the convolution library's deterministic solvers (``torch.backends.cudnn.deterministic`` for the call, then
    put back): at batch 1 its default choice for the 14 x 14 and 7 x 7 stages accumulates in an order that changes from call to call - the
    value moved in its last 3 bits between identical calls on an MI355X - and a session's ``rl_values`` have to be the same bits on every
    run under one seed."""

    def __init__(self, action_space: int = 2, arch: str = "resnet18", model_path: str = None, state_dict: dict = None, return_logits: bool = False,
                 device: str = "cuda"):
        if model_path is not None and state_dict is not None:
            raise ValueError("PPOAgent: model_path or state_dict, not both")
        self.device, self.action_space, self.return_logits = torch.device(device), action_space, return_logits
        self.ac_net = ActorCritic(out_dim=action_space, arch=arch, dropout=0.0)
        self.ac_net.eval()
        if model_path is not None:
            state_dict = torch.load(model_path, map_location="cpu")
        if state_dict is not None:
            self.ac_net.load_state_dict(state_dict, strict=True)
        self.ac_net.to(self.device)

    @torch.no_grad()
    def act(self, x_img, x_mask, generator: torch.Generator = None):
        """-> (action, value [B,1]); with ``return_logits``: (logits [B,action_space], value).  ``generator``: a CPU ``torch.Generator`` the
        draw is taken from (None: torch's global one, as the reference)."""
        with _DETERMINISTIC_CONVS:                                # a process-wide switch: one agent call at a time flips it and puts it back
            was = torch.backends.cudnn.deterministic
            torch.backends.cudnn.deterministic = True
            try:
                logits, value = self.ac_net(x_img.to(self.device), x_mask.to(self.device))
            finally:
                torch.backends.cudnn.deterministic = was
        if self.return_logits:
            return logits, value
        # Categorical(logits).sample() is multinomial over the normalised probabilities; drawn on the host from the session's generator
        probs = torch.softmax(logits.reshape(-1, logits.shape[-1])[0].double(), dim=0).cpu()
        return int(torch.multinomial(probs, 1, generator=generator).item()), value


def masks_to_224_torch(gen: torch.Tensor, frames=None, size=224, channels: int = 3) -> torch.Tensor:
    """The torch route of ``masks_to_224``: ``.float()``, ``interpolate(mode='nearest')``, ``expand`` (a view: the consumer materialises it)."""
    oh, ow = (size, size) if isinstance(size, int) else size
    x = gen if frames is None else gen[torch.as_tensor(list(frames), device=gen.device, dtype=torch.long)]
    return F.interpolate(x[:, None].float(), size=(oh, ow), mode="nearest").expand(-1, channels, -1, -1)


def masks_to_224(gen: torch.Tensor, frames=None, size=224, channels: int = 3) -> torch.Tensor:
    """gen: uint8 [T,H,W] on the device (the evaluated masks of a round; any byte values) -> fp32 [n,channels,size,size], nearest-resized by
    torch's rule, the byte's value as a float, every channel the same plane.  ``frames``: the frames to take, in order (None: all T);
    ``size``: an int or (h, w).  One launch on the current stream; torch allocates the output."""
    if gen.dtype != torch.uint8 or gen.dim() != 3 or not gen.is_cuda:
        raise ValueError(f"masks_to_224 takes uint8 [T,H,W] on the device, got {gen.dtype} {tuple(gen.shape)} on {gen.device}")
    gen = gen.contiguous()
    T, H, W = (int(v) for v in gen.shape)
    oh, ow = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    idx = None
    if frames is not None:
        frames = [int(f) for f in frames]
        if not frames or min(frames) < 0 or max(frames) >= T:
            raise ValueError(f"masks_to_224: frames {frames} of a clip of {T}")
        if frames == list(range(frames[0], frames[0] + len(frames))):      # a run of frames (the agent's one frame): a view, no index upload
            gen, T = gen[frames[0]:frames[0] + len(frames)], len(frames)
        else:
            idx = torch.tensor(frames, dtype=torch.int32).to(gen.device, non_blocking=True)
    n = T if idx is None else len(frames)
    out = torch.empty((n, channels, oh, ow), dtype=torch.float32, device=gen.device)
    with torch.cuda.device(gen.device):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().stcn_masks_resize_nearest(stream, C.c_void_p(gen.data_ptr()), T, H, W, C.c_void_p(idx.data_ptr()) if idx is not None else None,
                                                        n, oh, ow, int(channels), C.c_void_p(out.data_ptr())), "stcn_masks_resize_nearest")
    return out
