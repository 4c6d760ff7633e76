"""Frame selection by feature distance: the reference's ``l2_mask`` rule (``interactions/policies.py:21-36,69-88``) on distances the HIP
library computes (``csrc/frame_select.hip``: an fp64 Gram matrix on the matrix cores).

``pairwise_sq_distances`` is the generic entry over any ``[T, K]`` fp32 device tensor; ``InferenceCore.frame_distances()`` runs the same
kernels over the engine's cached ``f16`` maps.  ``farthest_frame`` is pure host code."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_FRAMES = 106            # STCN_FRAME_GRAM_MAX_T: the frames of the engine's key cache


def gram_plan(T: int, K: int) -> tuple:
    """(scratch bytes, slices of K) of the distance kernels for T vectors of K values - the host-side launch plan, no GPU needed."""
    b, s = C.c_int64(), C.c_int32()
    _lib.check(_lib.lib().stcn_frame_gram_scratch(int(T), int(K), C.byref(b), C.byref(s)), "stcn_frame_gram_scratch")
    return int(b.value), int(s.value)


def pairwise_sq_distances(x: torch.Tensor) -> torch.Tensor:
    """Squared L2 distances between the rows of ``x``: fp32 CUDA ``[T, K]``, 1 <= T <= 106, K a multiple of 4 -> float64 ``[T, T]`` on the
    device, symmetric and with a zero diagonal to the bit, enqueued on the current stream.  Rows may be strided (``x[:, :K]`` of a wider
    tensor is read in place when its rows start on 16-byte boundaries; what lies between the rows is never read); any other layout is
    copied once."""
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda:
        raise TypeError(f"pairwise_sq_distances takes an fp32 CUDA tensor [T, K], got {x.dtype} {tuple(x.shape)} on {x.device}")
    T, K = x.shape
    in_place = x.stride(1) == 1 and x.data_ptr() % 16 == 0 and (T == 1 or (x.stride(0) >= K and x.stride(0) % 4 == 0))
    if not in_place:
        x = x.contiguous()
    stride = x.stride(0) if T > 1 else K
    with torch.cuda.device(x.device):
        nbytes, _ = gram_plan(T, K)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        dist = torch.empty((T, T), dtype=torch.float64, device=x.device)
        _lib.check(_lib.lib().stcn_frame_sq_distances(torch.cuda.current_stream().cuda_stream, x.data_ptr(), T, K, stride, scratch.data_ptr(),
                                                      dist.data_ptr()), "stcn_frame_sq_distances")
    return dist


def farthest_frame(dist, annotated) -> int:
    """The frame to annotate next, ``get_frame_l2`` restated on a distance matrix: per frame the minimum distance to the annotated frames
    (``get_min_l2_dist``), then the FIRST frame at which that minimum is largest - the reference's loop keeps a candidate only on a strict
    ``>``.  Annotated frames take part with their distance 0 to themselves, as there, so all frames annotated gives frame 0.  ``dist``:
    host float64 ``[T, T]`` (squared distances select the same frame as the reference's norms: the square root is monotone)."""
    d = np.asarray(dist, dtype=np.float64)
    return int(np.argmax(d[:, sorted(set(int(f) for f in annotated))].min(axis=1)))
