"""The simulated user of the mixed-annotation sessions: where a person would click to correct a mask, the box they would draw, and which
of a segmenter's candidates is closest to a target (reference: robots/click_robot.py, robots/bbox_robot.py, annotator/annotator.py:38-57).

Two statements of the same arithmetic:

* the DEVICE robots (``ClickRobot``, ``BboxRobot``, ``best_mask``) run HIP kernels (csrc/robot.hip behind ``stcn_robot_*``): no mask leaves
  the device, a call enqueues only, and the ``*_device`` forms return the record tensor without a sync;
* the HOST restatement (``host_click_record``, ``HostClickRobot``, ``host_bbox``, ``host_best_mask``) does what the reference does - labels
  the error regions with ``scipy.ndimage.label`` (structure of ones = 8-connectivity) after downloading both masks.  It is the yardstick of the
  tests and the baseline of tools/click_robot_cost.py.

Masks are "non-zero = object" everywhere.  ``three_pos_clicks`` / ``three_refinement_clicks`` of the reference have no caller there and are
not restated."""
from __future__ import annotations

import ctypes as C

import numpy as np

# the click record (include/stcn_hip.h: STCN_ROBOT_*)
N_CLICKS, X0, Y0, LABEL0, X1, Y1, LABEL1, CLASS, FP_SIZE, FN_SIZE, FP_COUNT, FN_COUNT, MOVED = range(13)
RECORD_INTS = 16
INTERACT, MIDDLE = 0, 1
BBOX_INTS = 5
MAX_CANDIDATES = 8
BEST_INTS = 2 + 2 * MAX_CANDIDATES
MAX_PIXELS = 1 << 24


# ------------------------------------------------------------------------------------------------ host restatement
def _frame_shape(shape):
    """(H, W) of one mask given in any accepted shape, or None.  A 2-D mask is taken as it is - a [1,W] or [H,1] frame is a frame; a mask
    with more dimensions loses its dimensions of extent one, and where that leaves fewer than two (the reference's [1,1,H,W] of a one-row
    frame) the last two dimensions are the frame."""
    shape = tuple(int(v) for v in shape)
    if len(shape) == 2:
        return shape
    kept = tuple(v for v in shape if v != 1)
    if len(kept) == 2:
        return kept
    if len(shape) > 2 and len(kept) < 2 and all(v == 1 for v in shape[:-2]):
        return shape[-2:]
    return None


def _as_bool(mask) -> np.ndarray:
    if hasattr(mask, "detach"):
        mask = mask.detach().cpu().numpy()          # the download the reference's robot starts with (click_robot.py:15-16)
    m = np.asarray(mask)
    hw = _frame_shape(m.shape)
    assert hw is not None, "one [H,W] mask"
    return m.reshape(hw) != 0


def _nearest_object_pixel(gt: np.ndarray, x: int, y: int):
    """click_robot.py:51-55 / :88-93: (x, y) itself when it is on the object, else the object pixel with the smallest squared distance - the
    first one in raster order (np.argmin of the fp64 sqrt of these integers, which is strictly monotone on them)."""
    if gt[y, x]:
        return x, y, 0
    ys, xs = np.nonzero(gt)
    k = int(np.argmin((xs - x).astype(np.int64) ** 2 + (ys - y).astype(np.int64) ** 2))
    return int(xs[k]), int(ys[k]), 1


def _largest_component(region: np.ndarray):
    """(components, size, label map == the largest): on equal sizes the component whose first pixel comes first in raster order - np.argmax
    of the bincount takes the smallest label and scipy.ndimage.label numbers components by their first pixels (click_robot.py:23-31)."""
    from scipy import ndimage
    lab, n = ndimage.label(region, structure=np.ones((3, 3), int))
    if n == 0:
        return 0, 0, None
    sizes = np.bincount(lab.ravel())[1:]
    return n, int(sizes.max()), lab == int(np.argmax(sizes)) + 1


def _centroid(component: np.ndarray):
    ys, xs = np.where(component)
    return int(np.mean(xs)), int(np.mean(ys))      # sums below 2^53: the mean is the correctly rounded quotient


def host_click_record(pred, gt, mode: int = INTERACT, iou=None):
    """``ClickRobot.interact`` (mode INTERACT) / ``ClickRobot.middle_click`` (mode MIDDLE, ``pred`` unused) on the host.
    Returns (record int32 [RECORD_INTS] as ``stcn_robot_click`` writes it, component uint8 [H,W])."""
    g = _as_bool(gt)
    rec = np.zeros(RECORD_INTS, np.int32)
    comp = np.zeros(g.shape, np.uint8)
    n_fp = n_fn = s_fp = s_fn = 0
    if mode == INTERACT:
        p = _as_bool(pred)
        assert p.shape == g.shape
        n_fp, s_fp, c_fp = _largest_component(p & ~g)
        n_fn, s_fn, c_fn = _largest_component(~p & g)
        rec[[FP_SIZE, FN_SIZE, FP_COUNT, FN_COUNT]] = s_fp, s_fn, n_fp, n_fn
    if n_fp == 0 and n_fn == 0:                     # click_robot.py:64-65 and :78-99
        ys, xs = np.nonzero(g)
        if ys.size == 0:
            return rec, comp                        # nothing to click on (the reference raises on the median of nothing)
        x, y, moved = _nearest_object_pixel(g, int(np.median(xs)), int(np.median(ys)))
        rec[[N_CLICKS, X0, Y0, LABEL0, MOVED]] = 1, x, y, 1, moved
        return rec, comp
    fn_click = None
    if n_fn:
        fn_click = _nearest_object_pixel(g, *_centroid(c_fn))
    if s_fp >= s_fn:                                # np.argmax(components_len): the false positive is first in the list
        x, y = _centroid(c_fp)
        rec[[N_CLICKS, X0, Y0, LABEL0, CLASS]] = 1, x, y, 0, 1
        comp[c_fp] = 1
        if iou is not None and iou < 0.1 and fn_click is not None:        # :71-74
            rec[[N_CLICKS, X1, Y1, LABEL1, MOVED]] = 2, fn_click[0], fn_click[1], 1, fn_click[2]
    else:
        rec[[N_CLICKS, X0, Y0, LABEL0, CLASS, MOVED]] = 1, fn_click[0], fn_click[1], 1, 2, fn_click[2]
        comp[c_fn] = 1
    return rec, comp


def clicks_from_record(rec):
    """record -> the reference's return value: (np.array [[x, y], ...], np.array labels)."""
    rec = np.asarray(rec)
    n = int(rec[N_CLICKS])
    if n == 0:
        raise ValueError("the click robot has nothing to click on: the object mask is empty")
    clicks = [[int(rec[X0]), int(rec[Y0])], [int(rec[X1]), int(rec[Y1])]][:n]
    labels = [int(rec[LABEL0]), int(rec[LABEL1])][:n]
    return np.array(clicks), np.array(labels)


class HostClickRobot:
    """The reference's robot restated on the host (two mask downloads and a SciPy labelling per call)."""

    def interact(self, pred_mask, gt_mask, iou=None):
        return clicks_from_record(host_click_record(pred_mask, gt_mask, INTERACT, iou)[0])

    def middle_click(self, gt_mask):
        return clicks_from_record(host_click_record(None, gt_mask, MIDDLE)[0])


def host_bbox(mask):
    """record int32 [BBOX_INTS] = (1, x1, y1, x2, y2) of the non-zero pixels, or zeros for an empty mask (torchvision masks_to_boxes)."""
    ys, xs = np.nonzero(_as_bool(mask))
    if ys.size == 0:
        return np.zeros(BBOX_INTS, np.int32)
    return np.array([1, xs.min(), ys.min(), xs.max(), ys.max()], np.int32)


def box_from_record(rec):
    rec = np.asarray(rec)
    if not rec[0]:
        raise ValueError("the box robot has no box to draw: the mask is empty")
    return rec[1:5].astype(np.float32)[None]        # masks_to_boxes: float [1, 4] = x1, y1, x2, y2


class HostBboxRobot:
    def interact(self, gt_mask):
        return box_from_record(host_bbox(gt_mask))


def host_best_mask(candidates, target):
    """``Annotator.best_sam_mask`` with ``compute_iou`` (interactions/metrics.py:9-19) in torch on the CPU: (fp32 IoU as a float, index,
    integer counts [M,2])."""
    import torch
    cands = [torch.as_tensor(np.asarray(_as_bool(c)))[None] for c in candidates]
    tgt = torch.as_tensor(np.asarray(_as_bool(target)))[None]
    best, idx, counts = 0, -1, []
    for ii, c in enumerate(cands):
        inter, union = (c & tgt).float().sum((1, 2)), (c | tgt).float().sum((1, 2))
        iou = ((inter + 1e-6) / (union + 1e-6)).mean().item()
        counts.append((int((c & tgt).sum()), int((c | tgt).sum())))
        if iou > best:
            best, idx = iou, ii
    return float(best), idx, np.asarray(counts, np.int64)


# ------------------------------------------------------------------------------------------------ device robots
def _mask_u8(mask):
    """A torch mask on the device, [H,W] as it is or any shape that squeezes to [H,W] -> uint8 [H,W] contiguous, non-zero = object (no sync)."""
    import torch
    hw = _frame_shape(mask.shape)
    if hw is None or not mask.is_cuda:
        raise ValueError(f"a device robot takes one [H,W] mask on the GPU, got shape {tuple(mask.shape)} on {mask.device}")
    m = mask.reshape(hw)
    if m.numel() == 0 or m.numel() > MAX_PIXELS:
        raise ValueError(f"a frame of {m.shape[0]} x {m.shape[1]} pixels: the robots take 1 .. 2^24")
    if m.dtype != torch.uint8:
        m = m > 0.5 if m.is_floating_point() else m != 0
        m = m.to(torch.uint8)
    return m.contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def scratch_bytes(H: int, W: int) -> int:
    """``stcn_robot_scratch``: the bytes of scratch a click call needs for an H x W frame (works without a GPU)."""
    from . import _lib
    n = C.c_int64()
    _lib.check(_lib.lib().stcn_robot_scratch(int(H), int(W), C.byref(n)), "stcn_robot_scratch")
    return int(n.value)


class ClickRobot:
    """``robots.click_robot.ClickRobot`` on the device.  ``interact`` / ``middle_click`` return what the reference returns (one 64-byte
    record crosses PCIe); ``interact_device`` / ``middle_click_device`` return the int32 record tensor and do not wait.  The scratch is
    kept per frame size and reused: calls are ordered by the stream they are enqueued on (use one robot per stream)."""

    def __init__(self):
        self._scratch = {}

    def _scratch_for(self, H, W, device):
        import torch
        key = (H, W, device)
        if key not in self._scratch:
            self._scratch[key] = torch.empty((scratch_bytes(H, W) + 7) // 8, dtype=torch.int64, device=device)
        return self._scratch[key]

    def _click(self, pred, gt, mode, iou, component):
        import torch

        from . import _lib
        g = _mask_u8(gt)
        p = None
        if mode == INTERACT:
            p = _mask_u8(pred)
            if p.shape != g.shape or p.device != g.device:
                raise ValueError("pred and gt differ in shape or device")
        H, W = (int(v) for v in g.shape)
        if component is not None and (component.dtype != torch.uint8 or tuple(component.shape) != (H, W) or not component.is_contiguous()
                                      or component.device != g.device):
            raise ValueError("component: a contiguous uint8 [H,W] tensor beside the masks")
        with torch.cuda.device(g.device):
            rec = torch.empty((RECORD_INTS,), dtype=torch.int32, device=g.device)
            _lib.check(_lib.lib().stcn_robot_click(_stream(), _ptr(p), _ptr(g), H, W, mode, 0 if iou is None else 1, 0.0 if iou is None else float(iou),
                                                   _ptr(self._scratch_for(H, W, g.device)), _ptr(rec), _ptr(component)), "stcn_robot_click")
        return rec

    def interact_device(self, pred_mask, gt_mask, iou=None, component=None):
        """The record of ``interact`` as a device tensor, enqueued only.  ``iou``: a host number (or None).  ``component``: optional uint8
        [H,W] device tensor that receives the pixels of the clicked component."""
        return self._click(pred_mask, gt_mask, INTERACT, iou, component)

    def middle_click_device(self, gt_mask):
        return self._click(None, gt_mask, MIDDLE, None, None)

    def interact(self, pred_mask, gt_mask, iou=None):
        return clicks_from_record(self.interact_device(pred_mask, gt_mask, iou).cpu().numpy())

    def middle_click(self, gt_mask):
        return clicks_from_record(self.middle_click_device(gt_mask).cpu().numpy())


class BboxRobot:
    """``robots.bbox_robot.BboxRobot`` on the device: the box of ONE mask, float32 [1,4] = x1, y1, x2, y2 as ``masks_to_boxes`` gives it."""

    def interact_device(self, gt_mask):
        """int32 [BBOX_INTS] on the device: (1, x1, y1, x2, y2), or zeros when the mask is empty ("no box"); enqueued only."""
        import torch

        from . import _lib
        g = _mask_u8(gt_mask)
        with torch.cuda.device(g.device):
            rec = torch.empty((BBOX_INTS,), dtype=torch.int32, device=g.device)
            _lib.check(_lib.lib().stcn_robot_bbox(_stream(), _ptr(g), int(g.shape[0]), int(g.shape[1]), _ptr(rec)), "stcn_robot_bbox")
        return rec

    def interact(self, gt_mask):
        return box_from_record(self.interact_device(gt_mask).cpu().numpy())


def best_mask_device(candidates, target):
    """``stcn_robot_best_mask``: candidates [M,H,W] (M <= 8) against target [H,W], both on the device -> int32 [BEST_INTS] on the device =
    (selection, bits of its fp32 IoU, M pairs (intersection, union)); enqueued only."""
    import torch

    from . import _lib
    t = _mask_u8(target)
    c = candidates
    if c.dim() == 4:
        c = c.squeeze(1)
    if c.dim() != 3 or tuple(c.shape[1:]) != tuple(t.shape) or not 1 <= c.shape[0] <= MAX_CANDIDATES or c.device != t.device:
        raise ValueError(f"candidates [M,H,W] with 1 <= M <= {MAX_CANDIDATES} beside the target, got {tuple(candidates.shape)}")
    if c.dtype != torch.uint8:
        c = (c > 0.5 if c.is_floating_point() else c != 0).to(torch.uint8)
    c = c.contiguous()
    with torch.cuda.device(t.device):
        out = torch.empty((BEST_INTS,), dtype=torch.int32, device=t.device)
        _lib.check(_lib.lib().stcn_robot_best_mask(_stream(), _ptr(c), _ptr(t), int(c.shape[0]), int(t.shape[0]), int(t.shape[1]), _ptr(out)),
                   "stcn_robot_best_mask")
    return out


def best_mask(candidates, target):
    """``Annotator.best_sam_mask``: (max IoU as a float, index); eight bytes cross PCIe."""
    head = best_mask_device(candidates, target)[:2].cpu().numpy()
    return float(head[1:2].view(np.float32)[0]), int(head[0])
