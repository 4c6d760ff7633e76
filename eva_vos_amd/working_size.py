"""A clip at a working resolution: the engine propagates on frames brought down to ``working_size``, masks come back at the clip's own size.

Every STCN / XMem evaluation script has a ``--res 480`` switch; the engine itself runs at the size of the frames it is handed.  Three rules
("Working resolution"):

* **working shape** - ``working_shape(H, W, size)``: torchvision's ``Resize(int)``: the shorter side becomes ``size``, the longer
  ``size * long // short``; a clip whose shorter side is at most ``size`` (and ``size=None``) keeps its shape - frames are never enlarged;
* **frames down** - antialiased bicubic, ``align_corners=False``, A = -0.5, on the normalised fp32 frames (``downsample_frames``,
  ``stcn_frames_downsample_aa``: the map ``F.interpolate(mode="bicubic", antialias=True)`` defines, summed in fp64); annotation masks go
  down with torch's ``nearest`` rule per channel, so a one-hot stays one-hot;
* **masks up** - per frame the unpadded window of the engine's probabilities, bilinear (``align_corners=False``) to the clip's size for every
  channel, arg-max with the lowest index winning a tie, one byte per pixel (``upsample_argmax``, ``stcn_prob_upsample_argmax``): the
  (k+1) * T * H * W interpolated floats a torch route would materialise never exist.

``ScaledInferenceCore`` wraps an ``InferenceCore`` on the working clip and looks like a core at the clip's own size to the session loop, the
round scorers and the robots.  There is no CPU fallback: the kernels are the product."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import torch

from . import _lib


def check_working_size(size):
    """``size`` as the working-resolution switch takes it: ``None`` (the clip's own size) or an int >= 1; anything else raises ValueError."""
    if size is None:
        return None
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or size < 1:
        raise ValueError(f"working_size={size!r}: None (the clip's own size) or an int >= 1, the length of the shorter side")
    return int(size)


def working_shape(H: int, W: int, size):
    """The shape a clip of H x W is propagated at: (H, W) when ``size`` is None or the shorter side is at most ``size``, else the shorter side
    becomes ``size`` and the longer ``size * long // short`` (1080 x 1920 at 480: 480 x 853, which the core pads to 480 x 864)."""
    size = check_working_size(size)
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"working_shape: a clip of {H} x {W}")
    if size is None or min(H, W) <= size:
        return H, W
    return (size, size * W // H) if H <= W else (size * H // W, size)


def _device_of(t: torch.Tensor, device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("eva_vos_amd.working_size needs a HIP device (there is no CPU fallback)")
    if device is None:
        return t.device if t.is_cuda else torch.device(f"cuda:{torch.cuda.current_device()}")
    d = torch.device(device if device != "cuda" else f"cuda:{torch.cuda.current_device()}")
    if d.type != "cuda":
        raise RuntimeError(f"device {device!r}: the resampling kernels only run on a GPU")
    return d


def _ptr(t: torch.Tensor):
    return C.c_void_p(t.data_ptr())


def downsample_frames(images: torch.Tensor, size, chunk: int = 8, device=None) -> torch.Tensor:
    """images: ``[1,T,3,H,W]`` on the host or on the device (any real dtype; converted to fp32) -> fp32 ``[1,T,3,h,w]`` on the device,
    (h, w) = ``working_shape(H, W, size)``: antialiased bicubic, ``align_corners=False`` (``stcn_frames_downsample_aa``).  ``chunk`` frames are
    uploaded, converted and resampled at a time, so the fp32 clip at its own size is never resident as a whole.  A clip that keeps its shape comes
    back as fp32 on the device and no kernel runs.  Enqueues on the current stream (the first call for a pair of sizes uploads its tap tables)."""
    if images.dim() != 5 or images.shape[0] != 1:
        raise ValueError(f"downsample_frames takes [1,T,C,H,W], got {tuple(images.shape)}")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"downsample_frames: chunk={chunk!r}, at least 1 frame at a time")
    _, T, Cn, H, W = (int(v) for v in images.shape)
    h, w = working_shape(H, W, size)
    dev = _device_of(images, device)
    with torch.cuda.device(dev):
        if (h, w) == (H, W):
            return images.detach().to(dev, torch.float32).contiguous()
        out = torch.empty((1, T, Cn, h, w), dtype=torch.float32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        fn = _lib.lib().stcn_frames_downsample_aa
        for a in range(0, T, chunk):
            part = images[0, a:a + chunk].detach().to(dev, torch.float32).contiguous()
            _lib.check(fn(stream, _ptr(part), int(part.shape[0]) * Cn, H, W, h, w, _ptr(out[0, a:a + chunk])), "stcn_frames_downsample_aa")
    return out


def upsample_argmax(prob: torch.Tensor, pad, hw, HW, t0: int, t1: int, out: torch.Tensor) -> torch.Tensor:
    """prob: fp32 ``[k+1,T,1,nh,nw]`` on the device (a core's padded probabilities), ``pad`` = (lw, uw, lh, uh) as ``InferenceCore.pad``,
    ``hw`` = the unpadded window, ``HW`` = the size of ``out``: uint8 ``[T,1,H,W]`` or ``[T,H,W]``, contiguous, on the same device.  Frames
    ``[t0,t1)`` of ``out`` become the arg-max over channels of the window interpolated bilinearly to H x W (``stcn_prob_upsample_argmax``);
    the other frames are not touched.  Enqueues one launch on the current stream; returns ``out``."""
    (h, w), (H, W) = (int(v) for v in hw), (int(v) for v in HW)
    lw, uw, lh, uh = (int(v) for v in pad)
    if not (prob.is_cuda and prob.dtype == torch.float32 and prob.dim() == 5 and prob.shape[2] == 1 and prob.is_contiguous()):
        raise ValueError(f"upsample_argmax takes contiguous float32 [k+1,T,1,nh,nw] on the device, got {prob.dtype} {tuple(prob.shape)} on {prob.device}")
    k1, T, _, nh, nw = (int(v) for v in prob.shape)
    if (lh + h + uh, lw + w + uw) != (nh, nw):
        raise ValueError(f"upsample_argmax: pad {tuple(pad)} around {h} x {w} is not the padded plane {nh} x {nw}")
    if not (out.is_cuda and out.device == prob.device and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == T * H * W
            and tuple(out.shape[-2:]) == (H, W)):
        raise ValueError(f"upsample_argmax: out must be contiguous uint8 [{T},1,{H},{W}] on {prob.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    with torch.cuda.device(prob.device):
        _lib.check(_lib.lib().stcn_prob_upsample_argmax(C.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(prob), k1, T, nh, nw, lh, lw, h, w,
                                                        H, W, int(t0), int(t1), _ptr(out)), "stcn_prob_upsample_argmax")
    return out


class ScaledInferenceCore:
    """An ``InferenceCore`` on the clip brought down to ``working_size`` (``.inner``) that looks like a core at the clip's OWN size to
    everything that reads one: ``t, k, h, w``, ``nh = h``, ``nw = w``, ``pad = (0, 0, 0, 0)``, ``masks`` uint8 ``[T,1,H,W]`` on the device,
    ``np_masks``, ``interacted``, ``device``, ``top_k``, ``km``; ``interact`` takes the annotation at ``[C,1,H,W]``.

    ``prob`` STAYS THE INNER CORE'S TENSOR, at the working resolution and padded (``inner.pad``): probabilities at the clip's own size are
    exactly what this class avoids - (k+1) * T * H * W floats, 5 GB for 100 frames of 1080p with five objects.  Callers use it for its
    device; whoever wants probabilities resamples the window they need.  Likewise ``kh, kw``, ``images``, ``get_image_buffered``,
    ``frame_features`` and every other attribute not named here are the inner core's, i.e. those of the working clip.

    The own-size masks are re-derived only where an interaction can have rewritten the probabilities: the open span between the neighbouring
    interacted frames (the span ``RoundScorer.score`` evaluates); ``undo`` re-derives the span of the interaction it takes back; after
    ``reset`` the first ``interact`` re-derives every frame.  An annotated frame's own-size mask is therefore the ROUND TRIP of its annotation
    (down with ``nearest``, up with bilinear + arg-max), not the annotation itself.

    When ``working_shape`` keeps the clip's shape the wrapper is a pass-through: neither resampling kernel runs and ``masks`` holds the inner
    core's bytes, unpadded (the inner tensor itself where the clip needs no padding)."""

    def __init__(self, prop_net, fuse_net, images, num_objects, mem_profile=0, mem_freq=5, device="cuda", engine_options=None, working_size=480):
        from .inference_core import InferenceCore
        self.working_size = check_working_size(working_size)
        if images.dim() != 5 or images.shape[0] != 1:
            raise ValueError(f"images must be [1,T,3,H,W], got {tuple(images.shape)}")
        self.h, self.w = (int(v) for v in images.shape[-2:])
        self.working_hw = working_shape(self.h, self.w, self.working_size)
        self.scaled = self.working_hw != (self.h, self.w)
        if self.scaled:
            images = downsample_frames(images, self.working_size, device=_device_of(images, device))
        self.inner = InferenceCore(prop_net, fuse_net, images, num_objects, mem_profile, mem_freq, device, engine_options)
        self.t, self.k = self.inner.t, self.inner.k
        self.nh, self.nw, self.pad = self.h, self.w, (0, 0, 0, 0)
        if self.scaled or self.inner.pad != (0, 0, 0, 0):
            with torch.cuda.device(self.device):
                self.masks = torch.zeros((self.t, 1, self.h, self.w), dtype=torch.uint8, device=self.device)
        else:
            self.masks = self.inner.masks
        self.np_masks = np.zeros((self.t, self.h, self.w), dtype=np.uint8)
        self._spans = []                                           # [t0, t1) of the interactions that can still be taken back, oldest first
        self._undo_depth = 0

    def __getattr__(self, name):                                    # whatever is not kept at the clip's own size is the inner core's
        if name == "inner":
            raise AttributeError(name)
        return getattr(self.inner, name)

    prob = property(lambda self: self.inner.prob)
    device = property(lambda self: self.inner.device)
    interacted = property(lambda self: self.inner.interacted)

    # ------------------------------------------------------------------------------------------
    def rederive(self, t0: int = 0, t1: int = None) -> None:
        """Own-size masks of the frames [t0, t1) from the inner core's state (enqueue only)."""
        t1 = self.t if t1 is None else t1
        if self.scaled:
            upsample_argmax(self.inner.prob, self.inner.pad, self.working_hw, (self.h, self.w), t0, t1, self.masks)
        elif self.masks is not self.inner.masks:
            lw, uw, lh, uh = self.inner.pad
            self.masks[t0:t1].copy_(self.inner.masks[t0:t1, :, lh:self.inner.nh - uh, lw:self.inner.nw - uw])

    def _download(self):
        if not self.scaled:
            self.np_masks = self.inner._download_masks()
        else:
            with torch.cuda.device(self.device):
                self.np_masks = self.masks[:, 0].cpu().numpy()      # D2H sync on the current stream, which is ordered behind the engine's
        return self.np_masks

    def interact(self, mask, idx, scribble=False, download=True):
        """``InferenceCore.interact`` with the annotation at the clip's own size: ``mask`` ``[C,1,H,W]`` goes down to the working shape with
        torch's ``nearest`` rule per channel, the inner core propagates (``download=False``), and the own-size masks of the span the
        interaction can have rewritten are re-derived.  Returns np.uint8 ``[T,H,W]``, or None with ``download=False``."""
        idx = int(idx)
        with torch.cuda.device(self.device):
            mask = mask.detach().to(self.device, torch.float32)
            if mask.dim() != 4 or mask.shape[1] != 1 or tuple(mask.shape[-2:]) != (self.h, self.w):
                raise RuntimeError(f"mask must be [C,1,{self.h},{self.w}], got {tuple(mask.shape)}")
            if self.scaled:
                mask = torch.nn.functional.interpolate(mask, size=self.working_hw, mode="nearest")
            others = set(self.inner.interacted) - {idx}
            span = (max([f for f in others if f < idx] + [-1]) + 1, min([f for f in others if f > idx] + [self.t]))
            self.inner.interact(mask, idx, scribble=scribble, download=False)
            self._spans.append(span)
            del self._spans[:-max(self._undo_depth, 1)]
            self.rederive(*span)
            return self._download() if download else None

    def set_undo_depth(self, n: int) -> None:
        self.inner.set_undo_depth(n)
        self._undo_depth = int(n)
        del self._spans[:-max(self._undo_depth, 1)]

    def undo(self, download=True):
        """``InferenceCore.undo``; the own-size masks of the span the undone interaction had rewritten are re-derived from what came back."""
        self.inner.undo(download=False)                             # raises when there is nothing to take back: nothing changes here then
        span = self._spans.pop() if self._spans else (0, self.t)
        self.rederive(*span)
        return self._download() if download else None

    def undo_state(self) -> dict:
        return self.inner.undo_state()

    def reset(self, keep_frame_features=False) -> int:
        """``InferenceCore.reset``.  The own-size masks are left as they are, like the probabilities behind them: the next session's first
        ``interact`` has no interacted neighbour and re-derives every frame."""
        kept = self.inner.reset(keep_frame_features=keep_frame_features)
        self._spans.clear()
        self.np_masks = np.zeros((self.t, self.h, self.w), dtype=np.uint8)
        return kept

    def frame_distances(self) -> np.ndarray:
        return self.inner.frame_distances()

    @property
    def frame_distance_passes(self) -> int:
        return self.inner.frame_distance_passes

    @property
    def top_k(self) -> int:
        return self.inner.top_k

    @property
    def km(self):
        return self.inner.km

    def __deepcopy__(self, memo):
        new = object.__new__(type(self))
        for k, v in self.__dict__.items():
            if k not in ("inner", "masks", "np_masks", "_spans"):
                new.__dict__[k] = v
        new.inner = copy.deepcopy(self.inner, memo)                 # synchronises the current stream: the clone below reads finished masks
        with torch.cuda.device(self.device):
            new.masks = new.inner.masks if self.masks is self.inner.masks else self.masks.clone()
        new.np_masks, new._spans = self.np_masks.copy(), list(self._spans)
        return new
