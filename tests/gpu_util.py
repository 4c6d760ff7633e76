"""Helpers for the -m gpu tests: device tensors in the engine's NHWC layout, C-ABI calls."""
import ctypes as C

import torch
import torch.nn.functional as F

from eva_vos_amd import _lib
from eva_vos_amd.inference_core import _model_for


def dev(t):
    if t.dtype in (torch.int32, torch.uint8):
        return t.detach().to("cuda").contiguous()
    return t.detach().to("cuda", torch.float32).contiguous()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def nhwc(x):           # [B,C,H,W] -> [B,H,W,C] contiguous on device
    return dev(x.permute(0, 2, 3, 1))


def rows_to_nchw(x, h, w):   # [B,h*w,C] (device) -> [B,C,h,w] cpu
    return x.reshape(x.shape[0], h, w, -1).permute(0, 3, 1, 2).contiguous().cpu()


def model_handle(nets):
    return _model_for(nets[0], nets[1], torch.cuda.current_device()).handle


def call(name, *args):
    """Call a C-ABI entry point.  Tensor arguments are passed as tensors (kept alive for the whole call
    and converted to device pointers here); None -> NULL."""
    keep = [dev(a) if isinstance(a, torch.Tensor) and (a.device.type != "cuda" or not a.is_contiguous()) else a
            for a in args]
    conv = [C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in keep]
    _lib.check(getattr(_lib.lib(), name)(*conv), name)
    torch.cuda.synchronize()
    del keep


def kernel(name, ptrs, iv, fv=()):
    """stcn_test_kernel: one launch of a small kernel by name (argument order: include/stcn_hip.h); ptrs are device tensors."""
    pa = (C.c_void_p * max(1, len(ptrs)))(*[t.data_ptr() for t in ptrs])
    ia = (C.c_int64 * max(1, len(iv)))(*[int(v) for v in iv])
    fa = (C.c_double * max(1, len(fv)))(*[float(v) for v in fv])
    _lib.check(_lib.lib().stcn_test_kernel(name.encode(), stream(), pa, len(ptrs), ia, len(iv), fa, len(fv)), name)
    torch.cuda.synchronize()


def guarded(n, dtype=torch.float32, guard=64):
    """A NaN-filled (uint8: 0xFF) device buffer of n elements in front of `guard` more that a kernel must leave alone."""
    if dtype == torch.uint8:
        return torch.full((n + guard,), 255, dtype=torch.uint8, device="cuda")
    return torch.full((n + guard,), float("nan"), dtype=dtype, device="cuda")


def guard_intact(buf, n):
    tail = buf[n:]
    return bool((tail == 255).all()) if buf.dtype == torch.uint8 else bool(torch.isnan(tail).all())


def torch_aggregate_wbg(prob, keep_bg=False, hard=False):
    """model/aggregate.py:22-37, in the precision of `prob`."""
    new_prob = torch.cat([torch.prod(1 - prob, dim=0, keepdim=True), prob], 0).clamp(1e-7, 1 - 1e-7)
    logits = torch.log((new_prob / (1 - new_prob)))
    if hard:
        logits = logits * 1000
    return F.softmax(logits, dim=0) if keep_bg else F.softmax(logits, dim=0)[1:]


# ---- shared by test_gpu_small_kernels.py and test_gpu_large_extents.py
EPS = 2.0 ** -24


def taps(n_out, n_in, scale):
    """Source indices of F.interpolate(mode="bilinear", align_corners=False) per output index."""
    s = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * scale - 0.5).clamp(min=0)
    i0 = s.floor().long().clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1)


def tap_max(a, scale):
    """max |a| over the four bilinear taps of every output pixel; a [..., h, w]."""
    h, w = a.shape[-2:]
    (y0, y1), (x0, x1) = taps(round(h / scale), h, scale), taps(round(w / scale), w, scale)
    a = a.abs()
    return torch.stack([a[..., ys, :][..., xs] for ys in (y0, y1) for xs in (x0, x1)]).amax(0)


def up4_prob(logit):
    """logit [..., h4, w4] (3 leading dimensions at most) -> sigmoid(bilinear x4), in the precision of `logit`."""
    lead = logit.shape[:-2]
    p = torch.sigmoid(F.interpolate(logit.reshape(1, -1, *logit.shape[-2:]), scale_factor=4, mode="bilinear", align_corners=False))
    return p.reshape(*lead, *p.shape[-2:])


def aggregate_bound(figure):
    return max(1e-6, 4 * figure)


# ---- shared by test_gpu_attention.py and test_gpu_stage_api.py
def blob_masks(kk, H, W, g, noisy, zero_row=None):
    """[kk,1,H,W] mask differences as an interaction leaves them: exact zeros except one to three elliptical blobs of uniform values per row;
    rows r with r % 2 == noisy carry 0.02 * rand everywhere in addition; row `zero_row` stays all zero."""
    out = torch.zeros(kk, 1, H, W)
    u = lambda: torch.rand(1, generator=g).item()           # noqa: E731
    for r in range(kk):
        if r == zero_row:
            continue
        for _ in range(1 + int(3 * u())):
            cy, cx, ry, rx = u() * H, u() * W, 4 + u() * H / 6, 4 + u() * W / 6
            y0, y1, x0, x1 = max(0, int(cy - ry)), min(H, int(cy + ry) + 2), max(0, int(cx - rx)), min(W, int(cx + rx) + 2)
            yy, xx = torch.meshgrid(torch.arange(y0, y1), torch.arange(x0, x1), indexing="ij")
            m = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).float() * torch.rand(y1 - y0, x1 - x0, generator=g)
            out[r, 0, y0:y1, x0:x1] = torch.maximum(out[r, 0, y0:y1, x0:x1], m)
        if r % 2 == noisy:
            out[r, 0] += 0.02 * torch.rand(H, W, generator=g)
    return out


def attention_stages(mk, qk, pos, neg):
    """The stages of oracle.stcn_oracle.attention_read in the precision of the operands: pooled [2 kk][hw] (channel 2 r = pos[r], 2 r + 1 =
    neg[r]; F.interpolate(mode='area') to 1/16 = 16x16 block means), amap [2 kk][hw] = pooled @ Wm, and Wm [hw][hw] = the softmax over
    the memory rows."""
    from oracle import stcn_oracle as O
    kk, hw = pos.shape[0], mk.shape[0]
    pooled = torch.stack([F.avg_pool2d(pos, 16).reshape(kk, hw), F.avg_pool2d(neg, 16).reshape(kk, hw)], 1).reshape(2 * kk, hw)
    Wm = torch.softmax(O.affinity_logits(mk, qk), dim=0)
    return pooled, pooled @ Wm, Wm
