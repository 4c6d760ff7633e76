"""The reference's stage-level interface on the HIP kernels (ctypes side).

``PropagationNetwork.encode_key / encode_value / segment_with_query / get_attention`` (reference ``model/propagation/prop_net.py:153-211``),
``FusionNet.forward`` (``model/fusion_net.py:32-50``) and ``aggregate_wbg`` (``model/aggregate.py:22-37``) for callers that run their own
propagation loop instead of ``InferenceCore``.  Tensors come and go in the reference's shapes (NCHW, batch 1); this module validates them,
allocates the outputs and calls the ``stcn_stage_*`` entry points of include/stcn_hip.h - no torch op computes any part of a stage.

Limits: fp32 CUDA tensors, batch 1, no autograd (inputs are detached, outputs carry no grad), frames already padded to multiples of 16
(``InferenceCore`` pads in the reference), 1..32 objects, ``top_k`` / ``km`` as ``InferenceCore`` takes them from the container.

Stage contexts (workspace + scratch of one frame size) are cached per (model, nh, nw, current stream): two streams never share scratch, and
a call is ordered on the current stream like any torch op.  Each call looks the folded model up through the same fingerprint cache as
``InferenceCore`` (new weights, another ``top_k`` or ``km`` on the container -> another model)."""
from __future__ import annotations

import ctypes as C
import threading
import weakref

import torch

from . import _lib
from .inference_core import _fingerprint, _km_of, _model_for, _top_k_of

MAX_OBJECTS = 32            # STCN_MAX_OBJECTS of include/stcn_hip.h
_CONTEXTS_PER_MODEL = 8     # LRU of stage contexts per model (frame sizes x streams)
_LOCK = threading.Lock()
_FUSION_MODELS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()      # fuse_net -> {(device, fingerprint): _FusionModel}


def _need_gpu(what: str) -> None:
    if not torch.cuda.is_available():
        raise RuntimeError(f"eva_vos_amd {what} needs a HIP device (there is no CPU fallback); "
                           "the CPU oracle lives in oracle/ and is test infrastructure only")


def _arg(name: str, t, shape, device=None):
    """``t`` as a stage call takes it: a detached fp32 CUDA tensor of ``shape`` (None entries are free)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: a torch.Tensor is required, got {type(t).__name__}")
    if t.dtype != torch.float32 or t.device.type != "cuda":
        raise ValueError(f"{name}: an fp32 CUDA tensor is required (got {t.dtype} on {t.device}); there is no CPU fallback")
    if device is not None and t.device != device:
        raise ValueError(f"{name}: on {t.device}, the other arguments are on {device}")
    if t.dim() != len(shape) or any(s is not None and int(d) != s for d, s in zip(t.shape, shape)):
        want = "[" + ",".join("*" if s is None else str(s) for s in shape) + "]"
        raise ValueError(f"{name}: shape {want} is required (batch 1, the reference's layout), got {list(t.shape)}")
    return t.detach()


def _dense(t):
    return t if t.is_contiguous() else t.contiguous()


def _frame_dims(name, t):
    nh, nw = int(t.shape[-2]), int(t.shape[-1])
    if nh < 16 or nw < 16 or nh % 16 or nw % 16:
        raise ValueError(f"{name}: {nh}x{nw} - frames arrive padded to multiples of 16 (tensor_util.pad_divide_by, as InferenceCore does)")
    return nh, nw


class _FusionModel:
    """A ``stcn_model`` of a FusionNet alone (stcn_fusion_model_create)."""

    def __init__(self, fuse_net, device_index: int):
        lib = _lib.lib()
        sd = {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in fuse_net.state_dict().items() if v.is_floating_point()}
        arr = (_lib.WeightDesc * len(sd))()
        for i, (name, t) in enumerate(sd.items()):
            arr[i].name, arr[i].data, arr[i].ndim = name.encode(), t.data_ptr(), t.dim()
            for d in range(t.dim()):
                arr[i].shape[d] = t.shape[d]
        h = C.c_void_p()
        _lib.check(lib.stcn_fusion_model_create(device_index, arr, len(sd), C.byref(h)), "stcn_fusion_model_create")
        self.handle = h
        self._finalizer = weakref.finalize(self, lib.stcn_model_destroy, h)


def _fusion_model_for(fuse_net, device_index: int) -> _FusionModel:
    key = (device_index, _fingerprint(fuse_net))
    with _LOCK:
        per_net = _FUSION_MODELS.setdefault(fuse_net, {})
        hit = per_net.get(key)
        if hit is None:
            per_net.clear()                  # other weights in the same module: the old snapshot dies with its contexts
            hit = per_net[key] = _FusionModel(fuse_net, device_index)
        return hit


def _context(model, nh: int, nw: int, k: int, device) -> C.c_void_p:
    """The stage context of (model, frame size, current stream), created for at least k objects.  Contexts live in the model object; their
    finalizers are registered on it AFTER the model's own, so they run first (weak-reference callbacks run newest first)."""
    stream = torch.cuda.current_stream(device).cuda_stream
    key = (nh, nw, device.index, stream)
    with _LOCK:
        ctxs = model.__dict__.setdefault("_stage_contexts", {})
        hit = ctxs.pop(key, None)
        if hit is not None and hit[1] < k:
            hit[2]()                         # too few objects: destroy (waits for its stream), make a larger one
            hit = None
        if hit is None:
            for old in list(ctxs)[:max(0, len(ctxs) - (_CONTEXTS_PER_MODEL - 1))]:
                ctxs.pop(old)[2]()
            max_k = min(MAX_OBJECTS, 1 << (k - 1).bit_length())
            h = C.c_void_p()
            _lib.check(_lib.lib().stcn_stage_create(model.handle, nh, nw, max_k, C.c_void_p(stream), C.byref(h)), "stcn_stage_create")
            hit = (h, max_k, weakref.finalize(model, _lib.lib().stcn_stage_destroy, h))
        ctxs[key] = hit                      # most recently used last
        return hit[0]


def _destroy_contexts(model) -> int:
    """Destroys every cached stage context of ``model`` (each waits for its stream); returns how many there were.  The next stage call
    makes a new one."""
    with _LOCK:
        ctxs = model.__dict__.get("_stage_contexts", {})
        n = len(ctxs)
        while ctxs:
            ctxs.popitem()[1][2]()
    return n


def _prop_model(prop_net, device):
    return _model_for(prop_net, None, device.index, _top_k_of(prop_net), _km_of(prop_net))


def _p(t):
    return C.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------------------------- PropagationNetwork
def encode_key(prop_net, frame):
    """prop_net.py:172-177.  frame [1,3,nh,nw] -> (k16 [1,64,h,w], f16_thin [1,512,h,w], f16 [1,1024,h,w], f8 [1,512,2h,2w], f4 [1,256,4h,4w])."""
    _need_gpu("PropagationNetwork.encode_key")
    frame = _dense(_arg("frame", frame, (1, 3, None, None)))
    nh, nw = _frame_dims("frame", frame)
    dev = frame.device
    with torch.cuda.device(dev):
        model = _prop_model(prop_net, dev)
        ctx = _context(model, nh, nw, 1, dev)
        h, w = nh // 16, nw // 16
        out = [torch.empty((1, c, h * s, w * s), dtype=torch.float32, device=dev) for c, s in ((64, 1), (512, 1), (1024, 1), (512, 2), (256, 4))]
        _lib.check(_lib.lib().stcn_stage_encode_key(ctx, _p(frame), *[_p(o) for o in out]), "stcn_stage_encode_key")
    return tuple(out)


def encode_value(prop_net, frame, kf16, masks):
    """prop_net.py:153-170.  frame [1,3,nh,nw], kf16 [1,1024,h,w], masks [k,1,nh,nw] -> [k,512,1,h,w]."""
    _need_gpu("PropagationNetwork.encode_value")
    masks = _dense(_arg("masks", masks, (None, 1, None, None)))
    nh, nw = _frame_dims("masks", masks)
    k, dev = int(masks.shape[0]), masks.device
    if not 1 <= k <= MAX_OBJECTS:
        raise ValueError(f"masks: {k} objects, 1..{MAX_OBJECTS} are supported")
    frame = _dense(_arg("frame", frame, (1, 3, nh, nw), dev))
    kf16 = _dense(_arg("kf16", kf16, (1, 1024, nh // 16, nw // 16), dev))
    with torch.cuda.device(dev):
        model = _prop_model(prop_net, dev)
        ctx = _context(model, nh, nw, k, dev)
        out = torch.empty((k, 512, 1, nh // 16, nw // 16), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().stcn_stage_encode_value(ctx, _p(frame), _p(kf16), _p(masks), k, _p(out)), "stcn_stage_encode_value")
    return out


def _bank_in_place(t):
    """A [B,C,T,h,w] bank tensor whose channel planes are dense [T,h,w] blocks (the T-slice ``keys[:, :, :m_front]`` of a preallocated bank,
    inference_core.py:150-170): read in place with its plane stride.  Anything else is made contiguous first."""
    B, Cc, T, h, w = t.shape
    st = t.stride()
    dense_plane = st[4] == 1 and st[3] == w and (st[2] == h * w or T == 1)
    if not (dense_plane and st[1] >= T * h * w and (B == 1 or st[0] >= 0)):
        t = t.contiguous()
        st = t.stride()
    return t, int(st[1]), int(st[0]) if B > 1 else 0


def segment_with_query(prop_net, mk16, mv16, qf8, qf4, qk16, qv16):
    """prop_net.py:179-192.  mk16 [1,64,T,h,w], mv16 [k,512,T,h,w] (T-slices of larger banks are read in place), qf8 [1,512,2h,2w],
    qf4 [1,256,4h,4w], qk16 [1,64,h,w], qv16 [1,512,h,w] -> per-object probabilities [k,1,nh,nw] (not aggregated)."""
    _need_gpu("PropagationNetwork.segment_with_query")
    qk16 = _dense(_arg("qk16", qk16, (1, 64, None, None)))
    h, w = int(qk16.shape[2]), int(qk16.shape[3])
    dev = qk16.device
    mk16 = _arg("mk16", mk16, (1, 64, None, h, w), dev)
    T = int(mk16.shape[2])
    mv16 = _arg("mv16", mv16, (None, 512, T, h, w), dev)
    k = int(mv16.shape[0])
    if T < 1 or not 1 <= k <= MAX_OBJECTS:
        raise ValueError(f"memory of T={T} frames and k={k} objects: T >= 1 and 1..{MAX_OBJECTS} objects are supported")
    qf8 = _dense(_arg("qf8", qf8, (1, 512, 2 * h, 2 * w), dev))
    qf4 = _dense(_arg("qf4", qf4, (1, 256, 4 * h, 4 * w), dev))
    qv16 = _dense(_arg("qv16", qv16, (1, 512, h, w), dev))
    top_k = _top_k_of(prop_net)
    if T * h * w < top_k:
        raise ValueError(f"the memory has T*h*w = {T * h * w} rows, fewer than top_k = {top_k} (the reference's torch.topk raises as well)")
    mk16, mk_ps, _ = _bank_in_place(mk16)
    mv16, mv_ps, mv_os = _bank_in_place(mv16)
    with torch.cuda.device(dev):
        model = _prop_model(prop_net, dev)
        ctx = _context(model, 16 * h, 16 * w, k, dev)
        prob = torch.empty((k, 1, 16 * h, 16 * w), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().stcn_stage_segment(ctx, _p(mk16), mk_ps, _p(mv16), mv_ps, mv_os, T, k, _p(qf8), _p(qf4), _p(qk16), _p(qv16), _p(prob)),
                   "stcn_stage_segment")
    return prob


def get_attention(prop_net, mk16, pos_mask, neg_mask, qk16):
    """prop_net.py:198-211.  mk16 [1,64,1,h,w], pos_mask / neg_mask [b,1,nh,nw], qk16 [1,64,h,w] -> [b,2,nh,nw]."""
    _need_gpu("PropagationNetwork.get_attention")
    pos_mask = _dense(_arg("pos_mask", pos_mask, (None, 1, None, None)))
    nh, nw = _frame_dims("pos_mask", pos_mask)
    b, dev = int(pos_mask.shape[0]), pos_mask.device
    if not 1 <= b <= MAX_OBJECTS + 1:
        raise ValueError(f"pos_mask: {b} planes, 1..{MAX_OBJECTS + 1} (objects + background) are supported")
    neg_mask = _dense(_arg("neg_mask", neg_mask, (b, 1, nh, nw), dev))
    mk16 = _dense(_arg("mk16", mk16, (1, 64, 1, nh // 16, nw // 16), dev))
    qk16 = _dense(_arg("qk16", qk16, (1, 64, nh // 16, nw // 16), dev))
    with torch.cuda.device(dev):
        model = _prop_model(prop_net, dev)
        ctx = _context(model, nh, nw, max(1, b - 1), dev)
        attn = torch.empty((b, 2, nh, nw), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().stcn_stage_attention(ctx, _p(mk16), _p(pos_mask), _p(neg_mask), _p(qk16), b, _p(attn)), "stcn_stage_attention")
    return attn


# --------------------------------------------------------------------------------------------- FusionNet, aggregate_wbg
def fusion_forward(fuse_net, im, seg1, seg2, attn, time):
    """fusion_net.py:32-50.  im [1,3,nh,nw], seg1 / seg2 [1,1,nh,nw], attn [1,2,nh,nw], time [1,2] -> logit [1,1,nh,nw].
    ``time`` on the device costs one 8-byte blocking copy (its two values are kernel arguments); a CPU tensor costs nothing."""
    _need_gpu("FusionNet.forward")
    im = _dense(_arg("im", im, (1, 3, None, None)))
    nh, nw = _frame_dims("im", im)
    dev = im.device
    seg1 = _dense(_arg("seg1", seg1, (1, 1, nh, nw), dev))
    seg2 = _dense(_arg("seg2", seg2, (1, 1, nh, nw), dev))
    attn = _dense(_arg("attn", attn, (1, 2, nh, nw), dev))
    if not isinstance(time, torch.Tensor) or tuple(time.shape) != (1, 2) or not time.is_floating_point():
        raise ValueError("time: a floating-point tensor [1,2] = (nc, nr) is required (inference_core.py:199-201)")
    nc, nr = (float(v) for v in time.detach().reshape(2).tolist())
    with torch.cuda.device(dev):
        model = _fusion_model_for(fuse_net, dev.index)
        ctx = _context(model, nh, nw, 1, dev)
        logit = torch.empty((1, 1, nh, nw), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().stcn_stage_fusion(ctx, _p(im), _p(seg1), _p(seg2), _p(attn), nc, nr, _p(logit)), "stcn_stage_fusion")
    return logit


def aggregate_wbg(prob, keep_bg=False, hard=False):
    """model/aggregate.py:22-37.  prob [k,1,h,w] -> [k+1,1,h,w] (``keep_bg``) or [k,1,h,w]; ``hard``: logits x 1000."""
    _need_gpu("aggregate_wbg")
    prob = _dense(_arg("prob", prob, (None, 1, None, None)))
    k, _, h, w = (int(v) for v in prob.shape)
    if not 1 <= k <= MAX_OBJECTS or h * w < 1:
        raise ValueError(f"prob: {k} objects of {h}x{w}, 1..{MAX_OBJECTS} non-empty planes are supported")
    with torch.cuda.device(prob.device):
        out = torch.empty((k + 1 if keep_bg else k, 1, h, w), dtype=torch.float32, device=prob.device)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().stcn_aggregate_wbg(stream, _p(prob), k, h * w, 1 if keep_bg else 0, 1 if hard else 0, _p(out)), "stcn_aggregate_wbg")
    return out
